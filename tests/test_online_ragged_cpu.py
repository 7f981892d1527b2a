"""CPU: ragged online calls -- sep(chunk, streams=..., lengths=...), sep([x0, x1, ...], streams=...), the sep_online_*_rag entry points
(ConvTasNet.online_separator -> sepkernels/online.py -> csrc/online.hip).

(a) fp64 parity on ragged clocks: the separator's host orchestration on an fp64 emulation of the five _rag entry points (RagEmu, on top of SelEmu
    of tests/test_online_streams_cpu.py), driven through test_online_ragged_gpu.run_ragged_schedule -- five jobs in 5 slots, each bringing its
    own number of hops to every call -- against the unmodified reference's output per stream (tests/golden/convtasnet_causal_online.npz) to
    1e-9 of its maximum, with no call touching a slot it does not name.
(b) the refusals, each leaving the state as it was; the list form against the tensor form; lengths all equal to W against the uniform subset call.
(c) the kernel SOURCE on the host (tools/hostsim.py): the kernel cases of tests/test_online_ragged_gpu.py, the equal-lengths bitwise check, and
    a tiny model streamed with ragged calls, recorded against eager, with more distinct (A, ldt) than recordings are kept."""
import pytest
import torch
import torch.nn.functional as F

import sepkernels
import test_online_cpu as OC
import test_online_ragged_gpu as RG
import test_online_streams_gpu as SG
from test_online_cpu import needs_clang, sim_library, on_host          # noqa: F401  (fixtures)
from test_online_streams_cpu import SelEmu


class RagEmu(SelEmu):
    """SelEmu plus the five entry points that take a length per stream, built from the plain ones: per column block, its columns and its
    stream's state row are gathered, the one-stream plain entry point runs on them, and the results are scattered back -- columns beyond the
    last block come back as zero, rows and samples the lists do not name are never read."""

    @staticmethod
    def _blocks(num_streams, slots, offs):
        o = offs[:num_streams + 1].tolist()
        return [(j, int(slots[j]), o[j], o[j + 1] - o[j]) for j in range(num_streams)]

    def online_encoder_fwd_rag(self, chunk, E, carry, carry_next, w, num_streams, N, L, S, n_cap, ldt, relu, slots, offs):
        w.zero_()
        for j, s, o, n in self._blocks(num_streams, slots, offs):
            c = carry[s:s + 1].clone() if carry is not None else None
            cn = torch.empty_like(c) if c is not None else None
            wj = torch.zeros(N, n, dtype=w.dtype)
            self.online_encoder_fwd(chunk[j:j + 1, :n * S], E, c, cn, wj, 1, N, L, S, n, n, relu)
            w[:, o:o + n] = wj
            if cn is not None:
                carry_next[s] = cn[0]

    def online_cln_fwd_rag(self, x, alpha, gamma, beta, y, sums, sums_stride, frames, num_streams, C, n_cap, ldt, eps, slots, offs):
        y.zero_()
        for j, s, o, n in self._blocks(num_streams, slots, offs):
            at = s * sums_stride
            own = sums[at:at + 2].clone()
            yj = torch.zeros(C, n, dtype=y.dtype)
            self.online_cln_fwd(x[:, o:o + n].contiguous(), alpha, gamma, beta, yj, own, 2, frames[s:s + 1], 1, C, n, n, eps)
            y[:, o:o + n] = yj
            sums[at:at + 2] = own

    def online_depthwise_fwd_rag(self, x, w, bias, ring, ring_stride, y, num_streams, C, n_cap, ldt, P, dilation, slots, offs):
        CD = C * (P - 1) * dilation
        y.zero_()
        for j, s, o, n in self._blocks(num_streams, slots, offs):
            own = ring[s * ring_stride:s * ring_stride + CD].clone()
            yj = torch.zeros(C, n, dtype=y.dtype)
            self.online_depthwise_fwd(x[:, o:o + n].contiguous(), w, bias, own, CD, yj, 1, C, n, n, P, dilation)
            y[:, o:o + n] = yj
            ring[s * ring_stride:s * ring_stride + CD] = own

    def online_decoder_fwd_rag(self, w, mask, D, tail, tail_next, out, num_streams, n_src, N, L, S, n_cap, ldt, slots, offs):
        out.zero_()
        for j, s, o, n in self._blocks(num_streams, slots, offs):
            t = tail[s:s + 1].clone() if tail is not None else None
            tn = torch.empty_like(t) if t is not None else None
            oj = torch.zeros(1, n_src, n * S, dtype=out.dtype)
            self.online_decoder_fwd(w[:, o:o + n].contiguous(), mask[:, o:o + n].contiguous(), D, t, tn, oj, 1, n_src, N, L, S, n, n)
            out[j, :, :n * S] = oj[0]
            if tn is not None:
                tail_next[s] = tn[0]

    def online_advance_rag(self, frames, carry, carry_next, carry_len, tail, tail_next, tail_len, num_streams, n_cap, slots, offs):
        for j, s, o, n in self._blocks(num_streams, slots, offs):
            frames[s] += n
            if carry_len:
                carry[s] = carry_next[s]
            if tail_len:
                tail[s] = tail_next[s]


@pytest.fixture()
def emu():
    old = sepkernels._set_backend_for_tests(RagEmu())
    try:
        yield
    finally:
        sepkernels._set_backend_for_tests(old)


def _state(sep):
    return [getattr(sep, a).clone() for a in SG.STATE]


# ------------------------------------------------------------------------------------------------------ (a) fp64 parity and isolation
@pytest.mark.parametrize("name", ["causal16", "causal16_p5"])
def test_fixture_on_ragged_clocks_matches_the_reference_in_fp64(emu, name):
    """five jobs in 5 slots, every one bringing its own number of hops to every call (run_ragged_schedule): every job's pieces and its own flush
    are its fixture row to 1e-9 of its maximum, and no call touches a slot it does not name"""
    model, cfg = OC._model(name)
    L, S = cfg["kernel_size"], cfg["stride"]
    xin, ref = OC._fixture(name)
    x = xin[..., L - S:]
    sep = model.online_separator(num_streams=5, chunk_size=4 * S)
    sep.carry_next.fill_(float("nan"))                                    # what no call may read before it wrote it
    sep.tail_next.fill_(float("nan"))
    done, _, shapes = RG.run_ragged_schedule(sep, x, isolation=True)
    assert sorted(row for row, _ in done) == sorted(k % x.shape[0] for k in range(5))
    assert len(shapes) > 5 and {a for a, _ in shapes} >= {1, 2, 3, 4}
    for row, est in done:
        assert est.shape == ref[row].shape
        assert OC._rel(est, ref[row]) <= 1e-9, (row, OC._rel(est, ref[row]))
    for a in SG.STATE:
        assert not getattr(sep, a).any()                                  # every job was flushed


# ------------------------------------------------------------------------------------------------------ (b) refusals, the two forms
def test_lengths_that_cannot_be_served_are_refused(emu):
    model, cfg = OC._model("causal16_p5")
    S = cfg["stride"]
    sep = model.online_separator(num_streams=4)
    z = lambda rows, hops=3: torch.zeros(rows, 1, hops * S, dtype=torch.float64)      # noqa: E731
    sep(z(2), streams=[1, 3], lengths=[S, 2 * S])                          # the state is not all zeros when the refusals are tried
    before = _state(sep)
    with pytest.raises(ValueError, match="3 lengths for 2 rows"):
        sep(z(2), streams=[0, 1], lengths=[S, S, S])
    with pytest.raises(ValueError, match="1 lengths for 4 rows"):
        sep(z(4), lengths=[S])
    for bad in (0, -S, S + 1, 4 * S):
        with pytest.raises(ValueError, match="positive multiple of the stride"):
            sep(z(2), streams=[0, 1], lengths=[S, bad])
    with pytest.raises(ValueError, match="positive multiple of the stride"):
        sep(z(2), streams=[0, 1], lengths=torch.tensor([S, 0]))
    with pytest.raises(ValueError, match="integer tensor"):
        sep(z(2), streams=[0, 1], lengths=torch.tensor([float(S), float(S)]))
    with pytest.raises(ValueError, match="integer tensor"):
        sep(z(2), streams=[0, 1], lengths=torch.tensor([True, True]))
    with pytest.raises(ValueError, match="integers"):
        sep(z(2), streams=[0, 1], lengths=[S, S + 0.5])
    # the existing refusals of the selection, with lengths and with a list
    with pytest.raises(ValueError, match="duplicate"):
        sep(z(2), streams=[1, 1], lengths=[S, S])
    with pytest.raises(ValueError, match="out of range"):
        sep(z(2), streams=[0, 4], lengths=[S, S])
    with pytest.raises(ValueError, match="empty"):
        sep(z(0), streams=[], lengths=[])
    with pytest.raises(ValueError, match="2 selected streams"):
        sep(z(3), streams=[0, 1], lengths=[S, S])
    with pytest.raises(ValueError, match="duplicate"):
        sep([z(1)[0], z(1)[0]], streams=[2, 2])
    with pytest.raises(ValueError, match="1 pieces for 2 selected"):
        sep([z(1)[0]], streams=[0, 1])
    with pytest.raises(ValueError, match="positive multiple of the stride"):
        sep([torch.zeros(1, S + 1, dtype=torch.float64)], streams=[0])
    with pytest.raises(ValueError, match="a piece is"):
        sep([torch.zeros(2, S, dtype=torch.float64)], streams=[0])
    with pytest.raises(ValueError, match="carries its own lengths"):
        sep([z(1)[0]], streams=[0], lengths=[S])
    for a, b in zip(_state(sep), before):
        assert torch.equal(a, b)                                           # a refused call leaves no trace
    assert sep.chunk_size == 3 * S


def test_the_list_form_is_the_tensor_form(emu):
    model, cfg = OC._model("causal16_p5")
    S = cfg["stride"]
    g = torch.Generator().manual_seed(8)
    idx, hops = [3, 0, 2], [5, 1, 3]
    pieces = [0.1 * torch.randn(1, h * S, generator=g, dtype=torch.float64) for h in hops]
    chunk = torch.full((3, 1, 5 * S), float("nan"), dtype=torch.float64)
    for j, p in enumerate(pieces):
        chunk[j, :, :p.shape[-1]] = p
    a, b = model.online_separator(num_streams=4), model.online_separator(num_streams=4)
    ya = a(chunk, streams=idx, lengths=torch.tensor([h * S for h in hops], dtype=torch.int32))
    yb = b([pieces[0], pieces[1][0], pieces[2]], streams=torch.tensor(idx))    # a (k S,) piece among (1, k S) ones
    assert ya.shape == (3, a.n_src, 5 * S) and isinstance(yb, list)
    for j, h in enumerate(hops):
        assert yb[j].shape == (a.n_src, h * S) and torch.equal(yb[j], ya[j, :, :h * S]) and not ya[j, :, h * S:].any()
    assert torch.equal(a.frames, torch.tensor([1, 0, 3, 5])) and all(torch.equal(p, q) for p, q in zip(_state(a), _state(b)))
    # streams=None: the all-streams ragged call, in both forms
    full = [0.1 * torch.randn(1, h * S, generator=g, dtype=torch.float64) for h in (2, 1, 1, 4)]
    yl = b(full)
    ct = torch.zeros(4, 1, 4 * S, dtype=torch.float64)
    for j, p in enumerate(full):
        ct[j, :, :p.shape[-1]] = p
    yt = a(ct, lengths=[2 * S, S, S, 4 * S])
    assert all(torch.equal(yl[j], yt[j, :, :full[j].shape[-1]]) for j in range(4))
    assert torch.equal(a.frames, torch.tensor([3, 1, 4, 9])) and torch.equal(a.flush(), b.flush())


def test_lengths_all_equal_to_the_width_agree_with_the_uniform_subset_call(emu):
    model, cfg = OC._model("causal16")
    S = cfg["stride"]
    g = torch.Generator().manual_seed(9)
    a, b = model.online_separator(num_streams=4), model.online_separator(num_streams=4)
    for idx, h in (([2, 0, 3], 4), ([1], 2), ([3, 2], 7)):
        x = 0.1 * torch.randn(len(idx), 1, h * S, generator=g, dtype=torch.float64)
        ya, yb = a(x, streams=idx, lengths=[h * S] * len(idx)), b(x, streams=idx)
        assert OC._rel(ya, yb) <= 1e-12
    for p, q in zip(_state(a), _state(b)):
        assert torch.equal(p, q) if p.dtype == torch.int64 else (p - q).abs().max() <= 1e-12 * (1 + q.abs().max())


# ------------------------------------------------------------------------------------------------------ (c) on the host simulation
@needs_clang
@pytest.mark.parametrize("name,params", RG.CASES, ids=[c[0][5:] for c in RG.CASES])
def test_online_rag_kernel_source_on_the_host(on_host, name, params):
    for p in params:
        getattr(RG, name)(*p)


@needs_clang
def test_equal_lengths_through_rag_are_bitwise_the_sel_call_on_the_host(on_host):
    RG.check_equal_lengths_are_the_sel_call()


# (selection, hops per selected stream) of 16 calls at the recorded width of 3 hops: three sizes A = 1, 2, 3 (ldt is 128 for every one), equal
# sizes with different members, orders and lengths -- a replay that kept the first call's slot list or lengths would fail
CALLS = [([0, 1], [3, 1]), ([2, 3], [1, 2]), ([4], [2]), ([1, 0, 3], [2, 3, 1]), ([2, 4, 0], [1, 1, 3]), ([3], [3]), ([0, 1], [1, 3]), ([4, 3], [2, 2]),
         ([1, 2], [3, 3]), ([0], [1]), ([3, 4, 1], [3, 2, 1]), ([4, 1, 0], [1, 2, 2]), ([2], [3]), ([0, 3], [2, 1]), ([4, 2], [1, 3]), ([1, 3, 4], [2, 2, 2])]


@needs_clang
def test_recorded_ragged_steps_equal_eager_launches_bitwise(on_host):
    """the tiny model of tests/test_online_cpu.py in 5 slots, the 16 ragged calls of CALLS at the recorded width with three distinct (A, ldt)
    against two kept recordings (so recordings are evicted and made again); then every slot is flushed.  Recorded == eager to the last bit,
    every slot's output is the offline staged forward on what it received, and a ragged recording has as many launches as a subset one"""
    model = OC._tiny()
    cap, S, L = 3, 4, 8
    x = 0.1 * torch.randn(5, 1, 16 * cap * S, generator=torch.Generator().manual_seed(6))
    old = sepkernels._set_backend_for_tests(OC._Named(on_host))
    try:
        runs = []
        for record in (True, False):
            sep = model.online_separator(num_streams=5, chunk_size=cap * S, record=record, max_recordings=2)
            assert sep.record == record
            done, outs, keys = [0] * 5, [[] for _ in range(5)], set()
            for idx, hops in CALLS:
                chunk = torch.full((len(idx), 1, cap * S), float("nan"))
                for r, (s, h) in enumerate(zip(idx, hops)):
                    chunk[r, :, :h * S] = x[s, :, done[s] * S:(done[s] + h) * S]
                y = sep(chunk, streams=idx, lengths=[h * S for h in hops])
                keys.add((len(idx), 128))
                for r, (s, h) in enumerate(zip(idx, hops)):
                    assert not y[r, :, h * S:].any()
                    outs[s].append(y[r, :, :h * S])
                    done[s] += h
                assert len(sep._sub_seqs) <= 2
            assert len(keys) == 3
            tails = sep.flush(list(range(5)))
            runs.append([torch.cat(outs[s] + [tails[s]], -1) for s in range(5)])
            if record:
                assert len(sep._sub_seqs) == 2 and set(sep._sub_seqs) <= keys and len(sep._ws) == 1 and sum(sep.replays.values()) >= 1
                ragged = {len(q) for q in sep._sub_seqs.values()}
                sep(torch.zeros(2, 1, cap * S), streams=[0, 1])             # a subset step of the same model, recorded
                assert ragged == {len(sep._sub_seqs[2])} and len(sep._sub_seqs[2]) > 10
                assert len(sep._ws) == 1                                # ragged and uniform subset calls of one width share a workspace
        with torch.no_grad():
            refs = [model(F.pad(x[s:s + 1, :, :done[s] * S], (L - S, 0)))[0] for s in range(5)]
    finally:
        sepkernels._set_backend_for_tests(old)
    for s in range(5):
        assert torch.equal(runs[0][s], runs[1][s]), "slot {}: recorded differs from eager".format(s)
        assert OC._rel(runs[0][s], refs[s]) <= 1e-5, (s, OC._rel(runs[0][s], refs[s]))
