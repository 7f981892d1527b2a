"""CPU: export and import of the online separator's per-stream state (sepkernels/online.py: export_state, import_state, OnlineState;
csrc/online.hip: sep_online_state_row_bytes / _export / _import; the row format is version 1 of include/sepkernels.h).

(a) the kernel SOURCE on the host (tools/hostsim.py): the kernel cases of tests/test_online_state_gpu.py -- byte equality with the restated row
    format, import under another slot list into buffers of another size, sentinels of unnamed slots, round trip, argument errors.
(b) the fp64 emulator (StateEmu below adds the three calls, written from the header's contract, to the emulator of
    tests/test_dense_tcn_cpu.py): rollback, migration against the reference at 1e-9, the trip through torch.save, the refusals.
(c) rollback on the host simulation of the kernel sources, recorded: the bitwise checks on what the device runs.
(d) the library itself, which loads without a GPU: row sizes and the argument checks that precede every launch."""
import pytest
import torch

import sepkernels
import test_online_gpu as OG
import test_online_state_gpu as TG
from test_dense_tcn_cpu import DenseEmu, _Named
from test_online_cpu import needs_clang, sim_library, on_host          # noqa: F401  (fixtures)


class StateEmu(DenseEmu):
    """DenseEmu plus the three state calls from their contract in include/sepkernels.h: row j of blob is [int64 frames | sums | zeros to a
    multiple of 16 | rings | carry | tail | zeros to a multiple of 16] of stream slots[j], copied as bytes.  The emulator keeps carry, rings
    and tail in the dtype of the model it serves (fp64 in these tests), so an element of those sections takes `itemsize` bytes here where the
    library's takes 4; with fp32 buffers the rows are the library's (test_the_emulator_packs_the_documented_rows)."""
    itemsize = 8

    def online_state_row_bytes(self, carry_len, sums_len, rings_len, tail_len):
        return TG.row_layout(carry_len, sums_len, rings_len, tail_len, self.itemsize)[4]

    def _sections(self, frames, carry, carry_len, sums, sums_len, rings, rings_len, tail, tail_len):
        r, c, t, e, rb = TG.row_layout(carry_len, sums_len, rings_len, tail_len, self.itemsize)
        return rb, [(frames, 1, 0), (sums, sums_len, 8), (rings, rings_len, r), (carry, carry_len, c), (tail, tail_len, t)]

    def online_state_export(self, slots, num_streams, frames, carry, carry_len, sums, sums_len, rings, rings_len, tail, tail_len, blob, row_pitch):
        rb, sections = self._sections(frames, carry, carry_len, sums, sums_len, rings, rings_len, tail, tail_len)
        assert row_pitch >= rb and row_pitch % 16 == 0
        rows = blob.reshape(-1)[:num_streams * row_pitch].view(num_streams, row_pitch)
        rows[:, :rb] = 0
        for j, s in enumerate(slots[:num_streams].tolist()):
            for buf, n, at in sections:
                if n:
                    b = buf.reshape(-1)[s * n:(s + 1) * n].view(torch.uint8)
                    rows[j, at:at + b.numel()] = b

    def online_state_import(self, slots, num_streams, frames, carry, carry_len, sums, sums_len, rings, rings_len, tail, tail_len, blob, row_pitch):
        rb, sections = self._sections(frames, carry, carry_len, sums, sums_len, rings, rings_len, tail, tail_len)
        assert row_pitch >= rb and row_pitch % 16 == 0
        rows = blob.reshape(-1)[:num_streams * row_pitch].view(num_streams, row_pitch)
        for j, s in enumerate(slots[:num_streams].tolist()):
            for buf, n, at in sections:
                if n:
                    b = buf.reshape(-1)[s * n:(s + 1) * n].view(torch.uint8)
                    b.copy_(rows[j, at:at + b.numel()])


@pytest.fixture()
def emu():
    old = sepkernels._set_backend_for_tests(StateEmu())
    try:
        yield
    finally:
        sepkernels._set_backend_for_tests(old)


def _case(name):
    return TG.fixture_case(name, "cpu", torch.float64)


# ------------------------------------------------------------------------------------------------------ (a) the kernel sources on the host
@needs_clang
@pytest.mark.parametrize("args", TG.STATE_SHAPES, ids=[str(i) for i in range(len(TG.STATE_SHAPES))])
def test_state_kernel_source_on_the_host(on_host, args):
    TG.case_state(*args)


@needs_clang
def test_state_argument_errors_on_the_host(on_host):
    TG.case_argument_errors()


@needs_clang
def test_the_byte_check_is_not_vacuous(on_host):
    """the same case fails when the device side packs something else (here: the rows of other slots)"""
    class Skewed:
        def __getattr__(self, name):
            return getattr(on_host, name)

        def online_state_export(self, slots, *rest):
            return on_host.online_state_export(slots.flip(0).contiguous(), *rest)
    OG.HIP = Skewed()
    with pytest.raises(AssertionError):
        TG.case_state(*TG.STATE_SHAPES[0])


# ------------------------------------------------------------------------------------------------------ (b) the fp64 emulator
def test_the_emulator_packs_the_documented_rows():
    """StateEmu with 4-byte elements on fp32 buffers against the restatement the device is held to, and back"""
    K = StateEmu()
    K.itemsize = 4
    for Bs, slots, *lens in TG.STATE_SHAPES:
        src = TG.random_state(Bs, *lens)
        rb = K.online_state_row_bytes(*lens)
        blob = torch.full((len(slots), rb + 16), 0xA5, dtype=torch.uint8)
        st = torch.tensor(slots, dtype=torch.int32)
        K.online_state_export(st, len(slots), *TG._args(src, lens), blob, rb + 16)
        assert torch.equal(blob[:, :rb], TG.pack_rows(src, slots)) and (blob[:, rb:] == 0xA5).all()
        dst = TG.sentinel_state(Bs, *lens)
        K.online_state_import(st, len(slots), *TG._args(dst, lens), blob, rb + 16)
        for a, b in zip(dst, src):
            TG.same_bits(a[slots], b[slots], "emulator import")


@pytest.mark.parametrize("name", TG.NAMES)
def test_rollback_to_an_earlier_export_repeats_the_same_bits_in_fp64(emu, name):
    model, cfg, x, _ = _case(name)
    TG.check_rollback(model, cfg, x, recorded=False)


@pytest.mark.parametrize("name", TG.NAMES)
def test_migrated_stream_matches_the_reference_in_fp64(emu, name):
    """17 hops in slot 3 of 5, the rest in slot 1 of 2 of another separator: the reference's output (causal16_dense: the model's offline
    forward) on the zero-prefixed input to 1e-9 of its maximum, the bar of the other online fp64 tests"""
    model, cfg, x, ref = _case(name)
    TG.check_migration(model, cfg, x, ref, 1e-9)


@pytest.mark.parametrize("name", ["causal16_p5", "causal16_dense"])
def test_state_survives_the_host_and_torch_save(emu, name):
    model, cfg, x, _ = _case(name)
    TG.check_host_round_trip(model, cfg, x)


def test_imports_that_do_not_fit_are_refused(emu):
    TG.check_refusals({n: _case(n)[0] for n in TG.NAMES})


def test_a_state_of_another_dtype_is_refused(emu):
    model, cfg, x, _ = _case("causal16")
    sep = model.online_separator(num_streams=2)
    state = sep.export_state()
    assert state.dtype == "float64"
    with pytest.raises(ValueError, match="dtype"):
        sep.import_state(TG.OnlineState(state.blob, dict(state.header, dtype="float32")))


# ------------------------------------------------------------------------------------------------------ (c) rollback on the kernel sources
@needs_clang
@pytest.mark.parametrize("name", ["causal16_p5", "causal16_dense"])
def test_rollback_on_the_kernel_sources_recorded(on_host, name):
    old = sepkernels._set_backend_for_tests(_Named(on_host))
    try:
        model, cfg, x, _ = TG.fixture_case(name, "cpu", torch.float32)
        TG.check_rollback(model, cfg, x, recorded=True)
    finally:
        sepkernels._set_backend_for_tests(old)


@needs_clang
def test_migration_on_the_kernel_sources_moves_the_bits(on_host):
    """what slot 3 of one separator holds is, after export and import, bit for bit what slot 1 of another holds -- and nothing else there"""
    old = sepkernels._set_backend_for_tests(_Named(on_host))
    try:
        model, cfg, x, _ = TG.fixture_case("causal16_dense", "cpu", torch.float32)
        S = cfg["stride"]
        a, b = model.online_separator(num_streams=5, chunk_size=4 * S), model.online_separator(num_streams=2, chunk_size=4 * S)
        a(x[:1, :, :4 * S].contiguous(), streams=[3])
        a(x[:1, :, 4 * S:5 * S].contiguous(), streams=[3])
        b.import_state(a.export_state([3]), [1])
        for name in TG.STATE:
            assert torch.equal(getattr(b, name)[1], getattr(a, name)[3]) and not getattr(b, name)[0].any(), name
        ya, yb = a(x[:1, :, 5 * S:9 * S].contiguous(), streams=[3]), b(x[:1, :, 5 * S:9 * S].contiguous(), streams=[1])
        assert torch.equal(ya, yb) and torch.equal(a.flush([3]), b.flush([1]))
    finally:
        sepkernels._set_backend_for_tests(old)


# ------------------------------------------------------------------------------------------------------ (d) the library without a GPU
def test_row_sizes_of_the_library_are_the_documented_ones():
    lib = sepkernels.load()
    for _, _, *lens in TG.STATE_SHAPES + [(0, 0, 0, 0, 0, 0), (0, 0, 8, 100, 1568768, 16)]:
        got = lib.sep_online_state_row_bytes(*lens)
        assert got == TG.row_layout(*lens)[4] and got % 16 == 0, lens
    assert lib.sep_online_state_row_bytes(-1, 2, 16, 0) == 0
    assert lib.sep_seq_lookup(b"sep_online_state_row_bytes") == -1 and lib.sep_seq_lookup(b"sep_online_state_export") >= 0
    assert sepkernels.HipBackend().online_state_row_bytes(8, 6, 96, 16) == TG.row_layout(8, 6, 96, 16)[4]


def test_argument_checks_of_the_library_precede_the_launch():
    """no launch happens here: each call fails its own checks before any HIP call (the pointers are never followed)"""
    lib = sepkernels.load()
    rb = TG.row_layout(8, 6, 96, 16)[4]
    p = 1 << 12                                                                       # a 16-byte aligned address nobody reads
    for fn, name in ((lib.sep_online_state_export, b"sep_online_state_export"), (lib.sep_online_state_import, b"sep_online_state_import")):
        for blob, pitch, nstreams, words in ((None, rb, 2, b"bad arguments"), (p, rb - 16, 2, b"row_pitch"), (p, rb + 8, 2, b"multiple of 16"),
                                             (p + 8, rb, 2, b"aligned"), (p, rb, 0, b"bad arguments"), (p, rb, 70000, b"bad arguments")):
            assert fn(p, nstreams, p, p, 8, p, 6, p, 96, p, 16, blob, pitch, None) < 0
            msg = lib.sep_last_error()
            assert name in msg and words in msg, msg
        assert fn(p, 2, p, None, 8, p, 6, p, 96, p, 16, p, rb, None) < 0 and b"state buffer missing" in lib.sep_last_error()
