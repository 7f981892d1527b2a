"""GPU: export and import of the online separator's per-stream state -- sep.export_state / sep.import_state, OnlineState, the entry points
sep_online_state_row_bytes / _export / _import (sepkernels/online.py, csrc/online.hip, row format version 1 in include/sepkernels.h).

The kernel cases (`case_*`, listed in CASES) fill the five state buffers with random BIT PATTERNS (NaNs with payloads and denormals in the fp32
sections, frame counters above 2^32, fp64 sums) and compare bytes: the exported blob with a torch restatement of the documented row format
(pack_rows), an import into buffers of another size under another slot list with the source slots, every entry of every slot that is not named
with its sentinel, and a second export with the first.  tests/test_online_state_cpu.py runs the same functions on the host simulation of the
kernel sources (they go through test_online_gpu's HIP, to_device and device_sync, which it swaps) and the separator checks below on the fp64
emulator; tools/hostsim/state_main.cpp runs the same shapes in a stand-alone program under the host sanitizers.  The separator checks
(check_rollback, check_migration, check_host_round_trip, check_refusals) take the separator's device and dtype from the model they are given,
so the same code runs here on the device and there on the emulator and the host simulation."""
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sepkernels
import test_online_gpu as OG
from sepkernels.online import OnlineState
from test_online_gpu import _round_up, close, rnd

pytestmark = pytest.mark.gpu

ROOT = OG.ROOT
STATE = ("frames", "carry", "sums", "rings", "tail")
SENTINEL_BYTE = 0xA5


# ------------------------------------------------------------------------------------------------------ the row format, restated
def row_layout(carry_len, sums_len, rings_len, tail_len, itemsize=4):
    """-> byte offsets (rings, carry, tail, end) and row_bytes of row format 1: int64 frames | sums_len doubles | zeros to a multiple of 16 |
    rings | carry | tail | zeros to a multiple of 16.  itemsize: bytes of an element of the three last sections (4: the library's fp32)"""
    r = _round_up(8 + 8 * sums_len, 16)
    c = r + itemsize * rings_len
    t = c + itemsize * carry_len
    e = t + itemsize * tail_len
    return r, c, t, e, _round_up(e, 16)


def _bytes(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.uint8)


def pack_rows(state, slots, itemsize=4):
    """state: host tensors frames (Bs,), carry (Bs, cl), sums (Bs, sl), rings (Bs, rl), tail (Bs, tl) -> (len(slots), row_bytes) uint8"""
    frames, carry, sums, rings, tail = state
    r, c, t, e, rb = row_layout(carry.shape[1], sums.shape[1], rings.shape[1], tail.shape[1], itemsize)
    rows = torch.zeros(len(slots), rb, dtype=torch.uint8)
    for j, s in enumerate(slots):
        rows[j, 0:8] = _bytes(frames[s:s + 1])
        rows[j, 8:8 + 8 * sums.shape[1]] = _bytes(sums[s])
        rows[j, r:c] = _bytes(rings[s])
        rows[j, c:t] = _bytes(carry[s])
        rows[j, t:e] = _bytes(tail[s])
    return rows


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(got, want, what):
    assert torch.equal(_bits(got), _bits(want)), what


# ------------------------------------------------------------------------------------------------------ kernel cases
G = torch.Generator().manual_seed(4242)
PATTERNS = [0x7FC00001, 0xFFA5A5A5 - (1 << 32), 0x7F800001, 0x00000001, 0x807FFFFF - (1 << 32), 0x7F800000, 0x80000000 - (1 << 32), 0x7FFFFFFF]


def random_words(*shape):
    """fp32 tensor of random bit patterns; where there is room the first words are quiet and signalling NaNs with payloads, denormals of both
    signs, an infinity and a negative zero"""
    w = torch.randint(-2 ** 31, 2 ** 31, shape, generator=G, dtype=torch.int64).to(torch.int32)
    flat = w.view(-1)
    k = min(len(PATTERNS), flat.numel())
    flat[:k] = torch.tensor(PATTERNS[:k], dtype=torch.int64).to(torch.int32)
    if flat.numel() > 2 * k:
        flat[-k:] = torch.tensor(PATTERNS[:k], dtype=torch.int64).to(torch.int32)
    return w.view(torch.float32)


def random_state(Bs, carry_len, sums_len, rings_len, tail_len):
    frames = (1 << 33) + torch.randint(0, 1 << 40, (Bs,), generator=G, dtype=torch.int64)
    sums = torch.randn(Bs, sums_len, generator=G, dtype=torch.float64) * 1e3
    return [frames, random_words(Bs, carry_len), sums, random_words(Bs, rings_len), random_words(Bs, tail_len)]


def sentinel_state(Bs, carry_len, sums_len, rings_len, tail_len):
    """the scheme of tests/test_online_streams_gpu.py: finite sentinels in the state"""
    return [torch.arange(1000, 1000 + Bs, dtype=torch.int64), rnd(Bs, carry_len) + 3.0,
            torch.randn(Bs, sums_len, generator=G, dtype=torch.float64) + 77.0, rnd(Bs, rings_len) + 3.0, rnd(Bs, tail_len) + 3.0]


def _slots(sel):
    return OG.to_device(torch.tensor(sel, dtype=torch.int32))


def _args(dev, lens):
    """the state arguments of both entry points: a section of length zero goes in as a null pointer"""
    carry_len, sums_len, rings_len, tail_len = lens
    frames, carry, sums, rings, tail = dev
    return (frames, carry if carry_len else None, carry_len, sums if sums_len else None, sums_len, rings if rings_len else None, rings_len,
            tail if tail_len else None, tail_len)


def case_state(Bs, slots, carry_len, sums_len, rings_len, tail_len):
    lens = (carry_len, sums_len, rings_len, tail_len)
    A = len(slots)
    rb = row_layout(*lens)[4]
    assert OG.HIP.online_state_row_bytes(*lens) == rb and rb % 16 == 0
    src = random_state(Bs, *lens)
    src_d = [OG.to_device(t) for t in src]
    want = pack_rows(src, slots)
    # (a) export, once into rows that sit exactly side by side and once with a pitch beyond row_bytes: the bytes beyond keep their sentinel
    blob = None
    for pitch in (rb, rb + 32):
        b = OG.to_device(torch.full((A, pitch), SENTINEL_BYTE, dtype=torch.uint8))
        OG.HIP.online_state_export(_slots(slots), A, *_args(src_d, lens), b, pitch)
        OG.device_sync()
        bc = b.cpu()
        assert torch.equal(bc[:, :rb], want), "export: the blob is not the documented row format"
        assert torch.equal(bc[:, rb:], torch.full((A, pitch - rb), SENTINEL_BYTE, dtype=torch.uint8)), "export: bytes beyond row_bytes were written"
        blob = b if pitch == rb else blob
    for t, t0, what in zip(src_d, src, STATE):
        same_bits(t, t0, "export changed " + what)
    # (b) import into buffers of another size under another slot list, (c) every other entry keeps its sentinel
    Bs2 = Bs + 2
    slots2 = [s + 1 for s in reversed(slots)]
    dst = sentinel_state(Bs2, *lens)
    dst_d = [OG.to_device(t) for t in dst]
    nxt = [OG.to_device(torch.full((Bs2, max(carry_len, 1)), float("nan"))), OG.to_device(torch.full((Bs2, max(tail_len, 1)), float("nan")))]
    OG.HIP.online_state_import(_slots(slots2), A, *_args(dst_d, lens), blob, rb)
    OG.device_sync()
    rest = [s for s in range(Bs2) if s not in slots2]
    for t, t0, s0, what in zip(dst_d, dst, src, STATE):
        tc = t.cpu()
        same_bits(tc[slots2], s0[slots], "import: {} of a named slot is not the source slot's".format(what))
        same_bits(tc[rest], t0[rest], "import: {} of a slot that is not named changed".format(what))
    for t, n in zip(nxt, (max(carry_len, 1), max(tail_len, 1))):
        same_bits(t, torch.full((Bs2, n), float("nan")), "import: a second buffer changed")
    # (d) round trip
    again = OG.to_device(torch.full((A, rb), SENTINEL_BYTE, dtype=torch.uint8))
    OG.HIP.online_state_export(_slots(slots2), A, *_args(dst_d, lens), again, rb)
    OG.device_sync()
    assert torch.equal(again.cpu(), blob.cpu()), "export -> import -> export: the blobs differ"


def case_argument_errors():
    """(e) a null blob, a pitch below row_bytes and a pitch that is no multiple of 16 are errors with a message; nothing is launched, so neither
    the blob nor the state changes"""
    Bs, slots, lens = 3, [2, 0], (8, 6, 32, 16)
    rb = row_layout(*lens)[4]
    src = random_state(Bs, *lens)
    for importing in (False, True):
        call = OG.HIP.online_state_import if importing else OG.HIP.online_state_export
        for pitch, null, words in ((rb, True, "bad arguments"), (rb - 16, False, "row_pitch"), (rb + 8, False, "multiple of 16")):
            dev = [OG.to_device(t) for t in src]
            blob = OG.to_device(torch.full((len(slots), rb + 16), SENTINEL_BYTE, dtype=torch.uint8))
            with pytest.raises(sepkernels.SepKernelsError, match=words):
                call(_slots(slots), len(slots), *_args(dev, lens), None if null else blob, pitch)
            OG.device_sync()
            assert torch.equal(blob.cpu(), torch.full((len(slots), rb + 16), SENTINEL_BYTE, dtype=torch.uint8))
            for t, t0, what in zip(dev, src, STATE):
                same_bits(t, t0, what + " changed by a refused call")


# (Bs, slots, carry_len, sums_len, rings_len, tail_len): a scrambled subset; a slot index above 255, carry_len no multiple of 4, no rings; L == S
# (no carry and no tail: null pointers); a row spread over several workgroups; the smallest odd lengths
STATE_SHAPES = [(5, [4, 0, 2], 8, 6, 96, 16), (257, [256, 0], 10, 2, 0, 20), (2, [1], 0, 14, 16, 0), (3, [0, 1, 2], 8, 98, 49152, 24), (1, [0], 3, 2, 16, 3)]
CASES = [("case_state", STATE_SHAPES), ("case_argument_errors", [()])]


@pytest.mark.parametrize("args", STATE_SHAPES, ids=[str(i) for i in range(len(STATE_SHAPES))])
def test_state_kernels_against_the_row_format(args):
    case_state(*args)


def test_state_argument_errors_come_back_with_a_message():
    case_argument_errors()


# ------------------------------------------------------------------------------------------------------ the separator on the fixtures
NAMES = ("causal16", "causal16_p5", "causal16_dense")


def fixture_case(name, device, dtype=torch.float32):
    """-> (model on device in dtype, its config, x (R, 1, T) without pre-roll, ref (R, n_src, T + L - S) or None).  ref is the unmodified
    reference's fp64 output on the pre-rolled input where the online fixture holds it (causal16, causal16_p5); for causal16_dense it is None
    and the bar is the model's own offline forward on the zero-prefixed input (as in tests/test_dense_tcn_gpu.py)"""
    if name == "causal16_dense":
        import test_dense_tcn_gpu as DG
        from dense_tcn_configs import CONFIGS
        model, cfg = DG.fixture_model(name), CONFIGS[name]
        x = 0.1 * torch.randn(3, 1, 40 * cfg["stride"], generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        return model.to(device=device, dtype=dtype), cfg, x.to(device=device, dtype=dtype), None
    from oracle.make_golden import CONFIGS
    from models.conv_tasnet import ConvTasNet
    g = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_{}.npz".format(name)))
    model, cfg = ConvTasNet(**CONFIGS[name]), CONFIGS[name]
    model.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")})
    o = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_causal_online.npz"))
    x = torch.from_numpy(o[name + "/input"])[..., cfg["kernel_size"] - cfg["stride"]:]
    return model.to(device=device, dtype=dtype), cfg, x.to(device=device, dtype=dtype).contiguous(), torch.from_numpy(o[name + "/output_f64"])


def _snapshot(sep, names=STATE + ("carry_next", "tail_next")):
    return {a: getattr(sep, a).clone() for a in names}


def _feed(sep, x, pos, slots, hops, ragged=False):
    """one call for `slots`, slot s reading hops[j] hops of row s % R of x from its own position; ragged: at the width of chunk_size"""
    S, R = sep.S, x.shape[0]
    W = sep.chunk_size if ragged else max(hops) * S
    chunk = torch.zeros(len(slots), 1, W, device=x.device, dtype=x.dtype)
    for j, (s, h) in enumerate(zip(slots, hops)):
        chunk[j, 0, :h * S] = x[s % R, 0, pos[s] * S:(pos[s] + h) * S]
        pos[s] += h
    if ragged:
        return sep(chunk, streams=slots, lengths=[h * S for h in hops])
    return sep(chunk) if slots == list(range(sep.num_streams)) else sep(chunk, streams=slots)


def check_rollback(model, cfg, x, recorded):
    """5 slots.  Three ticks in which every slot receives audio (an all-streams call, a subset call, a ragged call); export of slots [3, 1];
    three more ticks for those two (a uniform subset call off chunk_size, a ragged call, a call at chunk_size), outputs and a second export
    kept; import of the first export; the same three ticks again: outputs and final export are bitwise what they were.  The import leaves
    every other slot (and both second buffers) bitwise alone, and with `recorded` the recordings survive it: sep.replays grows afterwards."""
    S = cfg["stride"]
    assert x.shape[-1] >= 20 * S
    sep = model.online_separator(num_streams=5, chunk_size=4 * S)
    assert sep.record == recorded
    pos = [0] * 5
    _feed(sep, x, pos, [0, 1, 2, 3, 4], [4] * 5)
    _feed(sep, x, pos, [3, 1, 0], [2, 2, 2])
    _feed(sep, x, pos, [1, 3, 4], [1, 3, 2], ragged=True)
    before_export = _snapshot(sep)
    first = sep.export_state([3, 1])
    for a, t in before_export.items():
        assert torch.equal(getattr(sep, a), t), "export_state changed " + a
    assert len(first) == 2 and first.frames.tolist() == [pos[3], pos[1]] == [9, 7]

    def three():
        p = list(pos)
        return [_feed(sep, x, p, [1, 3], [3, 3]), _feed(sep, x, p, [3, 1], [4, 2], ragged=True), _feed(sep, x, p, [3, 1], [4, 4])]

    outs = three()
    second = sep.export_state([3, 1])
    assert second.frames.tolist() == [20, 16] and not torch.equal(second.blob, first.blob)
    snap = _snapshot(sep)
    seqs = (sep._seq, dict(sep._sub_seqs))
    sep.import_state(first, [3, 1])
    rest = [0, 2, 4]
    for a in STATE:
        assert torch.equal(getattr(sep, a)[rest], snap[a][rest]), "import_state changed {} of a slot it does not name".format(a)
    for a in ("carry_next", "tail_next"):
        assert torch.equal(getattr(sep, a), snap[a]), "import_state touched " + a
    assert sep._seq is seqs[0] and dict(sep._sub_seqs) == seqs[1], "import_state dropped a recording"
    assert torch.equal(sep.export_state([3, 1]).blob, first.blob)
    replays = sum(sep.replays.values())
    again = three()
    for a, b in zip(outs, again):
        assert torch.equal(a, b), "after the rollback a tick gives other bits"
    assert torch.equal(sep.export_state([3, 1]).blob, second.blob), "after the rollback the state differs"
    for a in STATE:
        assert torch.equal(getattr(sep, a)[rest], snap[a][rest])
    if recorded:
        assert sep._seq is seqs[0] and sum(sep.replays.values()) > replays, "the recordings did not survive the import"


def check_migration(model, cfg, x, ref, tol):
    """row 0 of x: 17 hops into slot 3 of a 5-slot separator (in pieces of 4, 4, 4, 4, 1 hops), exported, imported into slot 1 of a 2-slot
    separator of the same model, the rest streamed there and flushed: the concatenation is the offline result within tol of its maximum"""
    L, S = cfg["kernel_size"], cfg["stride"]
    total = x.shape[-1] // S
    assert total > 17 + 4
    a = model.online_separator(num_streams=5, chunk_size=4 * S)
    pieces, t = [], 0
    for h in (4, 4, 4, 4, 1):
        pieces.append(a(x[:1, :, t * S:(t + h) * S].contiguous(), streams=[3])[0])
        t += h
    state = a.export_state([3])
    assert len(state) == 1 and state.frames.tolist() == [17] and state.frames.dtype == torch.int64
    b = model.online_separator(num_streams=2, chunk_size=4 * S)
    b.import_state(state, [1])
    assert b.frames.tolist() == [0, 17] and not b.carry[0].any() and not b.rings[0].any()
    while t < total:
        h = min(4, total - t)
        pieces.append(b(x[:1, :, t * S:(t + h) * S].contiguous(), streams=[1])[0])
        t += h
    pieces.append(b.flush([1])[0])
    est = torch.cat(pieces, -1)
    if ref is None:
        with torch.no_grad():
            ref = model(F.pad(x[:1], (L - S, 0)))
    want = ref[0].detach().cpu()
    assert est.shape == want.shape
    close(est, want, tol, "migrated stream")


def check_host_round_trip(model, cfg, x):
    """state.cpu().state_dict() through torch.save / torch.load on a BytesIO, from_state_dict, .to(device), import into a fresh separator: the
    re-export is byte-equal; state.select([1]) (and state[1]) imported into one slot likewise"""
    S = cfg["stride"]
    sep = model.online_separator(num_streams=3, chunk_size=4 * S)
    pos = [0] * 3
    _feed(sep, x, pos, [0, 1, 2], [4] * 3)
    _feed(sep, x, pos, [2, 0], [3, 1], ragged=True)
    state = sep.export_state()
    assert len(state) == 3 and state.version == 1 and (state.L, state.S, state.n_sources) == (sep.L, sep.S, sep.n_src)
    assert (state.n_norms, state.ring_len, state.separable) == (sep.n_norms, sep.ring_len, not sep.dense) and state.config == model.get_config()
    assert state.dtype == str(sep.dtype).replace("torch.", "") and state.frames.tolist() == [5, 4, 7]
    assert state.blob.device == sep.device and state.blob.dtype == torch.uint8 and state.blob.shape[1] % 16 == 0
    d = state.cpu().state_dict()
    assert all(torch.is_tensor(v) or isinstance(v, (int, float, bool, str, dict, type(None))) for v in d.values())
    buf = io.BytesIO()
    torch.save(d, buf)
    buf.seek(0)
    back = OnlineState.from_state_dict(torch.load(buf))
    assert back.blob.device.type == "cpu" and back.header == state.header
    other = model.online_separator(num_streams=3, chunk_size=4 * S)
    other.import_state(back.to(sep.device))
    assert torch.equal(other.export_state().blob, state.blob)
    for a in STATE:
        assert torch.equal(getattr(other, a), getattr(sep, a)), a
    third = model.online_separator(num_streams=3)
    third.import_state(back, [2, 1, 0])                                      # a state on another device is moved first; any order of slots
    assert torch.equal(third.export_state([2, 1, 0]).blob, state.blob)
    one = model.online_separator(num_streams=1)
    one.import_state(state.select([1]))
    assert torch.equal(one.export_state().blob, state.blob[1:2]) and torch.equal(state[1].blob, state.blob[1:2])
    assert torch.equal(state[1:].blob, state.blob[1:]) and len(state.select([2, 0])) == 2 and state.select([2, 0]).frames.tolist() == [7, 5]


def check_refusals(models):
    """models: name -> model for the three fixtures.  Every refused import is a ValueError that leaves the separator's state bitwise alone"""
    seps = {n: m.online_separator(num_streams=3) for n, m in models.items()}
    for n, sep in seps.items():
        f = dict(device=sep.device, dtype=sep.dtype)
        sep(0.1 * torch.randn(3, 1, 3 * sep.S, generator=torch.Generator().manual_seed(5)).to(**f))
    states = {n: sep.export_state([2, 0]) for n, sep in seps.items()}
    good = states["causal16"]
    d = good.state_dict()
    cut = OnlineState(good.blob[:, :-16].contiguous(), good.header)
    refused = [("causal16_p5", good, [2, 0]),                                              # another model structure (P = 5: other histories)
               ("causal16", states["causal16_dense"], [2, 0]),                             # separable=False into a separable separator
               ("causal16", good, [0, 1, 2]), ("causal16", good, None),                    # row count against the selection / against num_streams
               ("causal16", good, [1, 1]), ("causal16", good, [0, 3]),                     # duplicate, out of range
               ("causal16", cut, [2, 0]),                                                  # a truncated blob
               ("causal16", OnlineState(good.blob.view(torch.int8), good.header), [2, 0]),           # another dtype of the blob
               ("causal16", OnlineState.from_state_dict(dict(d, format_version=2)), [2, 0]),     # a future format
               ("causal16", d, [2, 0])]                                                    # not a state at all
    for target, state, streams in refused:
        sep = seps[target]
        snap = _snapshot(sep)
        with pytest.raises(ValueError):
            sep.import_state(state, streams)
        for a, t in snap.items():
            assert torch.equal(getattr(sep, a), t), "a refused import changed " + a
    seps["causal16"].import_state(OnlineState.from_state_dict(d), [1, 2])                        # ... and the same state is taken where it fits
    assert seps["causal16"].frames.tolist() == [3, 3, 3]


def _on_device(name):
    return fixture_case(name, "cuda")


@pytest.mark.parametrize("name", NAMES)
def test_rollback_to_an_earlier_export_repeats_the_same_bits_on_the_device(name):
    model, cfg, x, _ = _on_device(name)
    check_rollback(model, cfg, x, recorded=True)


@pytest.mark.parametrize("arith", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_migrated_stream_matches_the_reference_on_the_device(name, arith):
    """1e-3 of the maximum in every arithmetic of the products, the bar of
    test_online_ragged_gpu.py::test_fixture_on_ragged_clocks_matches_the_reference_on_the_device"""
    prev = sepkernels.set_gemm_arith(arith)
    try:
        model, cfg, x, ref = _on_device(name)
        check_migration(model, cfg, x, ref, 1e-3)
    finally:
        sepkernels.set_gemm_arith(prev)


@pytest.mark.parametrize("name", ["causal16_p5", "causal16_dense"])
def test_state_survives_the_host_and_torch_save_on_the_device(name):
    model, cfg, x, _ = _on_device(name)
    check_host_round_trip(model, cfg, x)


def test_imports_that_do_not_fit_are_refused_on_the_device():
    check_refusals({n: _on_device(n)[0] for n in NAMES})
