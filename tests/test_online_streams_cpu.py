"""CPU: online separation with streams on their own clocks -- sep(chunk, streams=...), flush(streams), the sep_online_*_sel entry points
(ConvTasNet.online_separator -> sepkernels/online.py -> csrc/online.hip).

(a) fp64 parity under independent clocks: the separator's host orchestration on an fp64 emulation of the five _sel entry points (SelEmu, on top
    of the emulator of tests/test_online_cpu.py), driven through test_online_streams_gpu.run_schedule -- streams that start, pause, end and
    restart on their own in 5 slots -- against the unmodified reference's output per stream (tests/golden/convtasnet_causal_online.npz) to
    1e-9 of its maximum, the bar of the all-streams fp64 test.
(b) isolation: after every subset call of (a) the unselected slots' slices of all five state tensors are what they were; after flush([s]) only
    slot s is zero.
(c) the refusals.
(d), (e) the kernel SOURCE on the host (tools/hostsim.py): the kernel cases of tests/test_online_streams_gpu.py, and a tiny model streamed with
    subset calls, recorded against eager, with more distinct selection sizes than recordings are kept.
(f) streams=None and streams=list(range(num_streams)) agree.
(g) on the kernel sources: all-streams, subset and ragged calls interleaved at one width share one workspace, recorded against eager."""
import pytest
import torch
import torch.nn.functional as F

import sepkernels
import test_online_cpu as OC
import test_online_gpu as OG
import test_online_streams_gpu as SG
from test_online_cpu import needs_clang, sim_library, on_host          # noqa: F401  (fixtures)


class SelEmu(OC.OnlineEmu):
    """OnlineEmu plus the five entry points that take a slot list: the selected rows of the state are gathered, the plain entry point runs on
    them as if they were all the streams there are, and the rows are scattered back -- rows the list does not name are never touched."""

    def online_encoder_fwd_sel(self, chunk, E, carry, carry_next, w, num_streams, N, L, S, n, ldt, relu, slots):
        idx = slots[:num_streams].long()
        c = carry[idx] if carry is not None else None
        cn = torch.empty_like(c) if c is not None else None
        self.online_encoder_fwd(chunk, E, c, cn, w, num_streams, N, L, S, n, ldt, relu)
        if cn is not None:
            carry_next[idx] = cn

    def online_cln_fwd_sel(self, x, alpha, gamma, beta, y, sums, sums_stride, frames, num_streams, C, n, ldt, eps, slots):
        idx = slots[:num_streams].long()
        at = idx * sums_stride
        own = torch.stack([sums[at], sums[at + 1]], 1).reshape(-1)
        self.online_cln_fwd(x, alpha, gamma, beta, y, own, 2, frames[idx], num_streams, C, n, ldt, eps)
        sums[at], sums[at + 1] = own[0::2], own[1::2]

    def online_depthwise_fwd_sel(self, x, w, bias, ring, ring_stride, y, num_streams, C, n, ldt, P, dilation, slots):
        idx, CD = slots[:num_streams].tolist(), C * (P - 1) * dilation
        own = torch.stack([ring[s * ring_stride:s * ring_stride + CD] for s in idx]).reshape(-1)
        self.online_depthwise_fwd(x, w, bias, own, CD, y, num_streams, C, n, ldt, P, dilation)
        for j, s in enumerate(idx):
            ring[s * ring_stride:s * ring_stride + CD] = own[j * CD:(j + 1) * CD]

    def online_decoder_fwd_sel(self, w, mask, D, tail, tail_next, out, num_streams, n_src, N, L, S, n, ldt, slots):
        idx = slots[:num_streams].long()
        t = tail[idx] if tail is not None else None
        tn = torch.empty_like(t) if t is not None else None
        self.online_decoder_fwd(w, mask, D, t, tn, out, num_streams, n_src, N, L, S, n, ldt)
        if tn is not None:
            tail_next[idx] = tn

    def online_advance_sel(self, frames, carry, carry_next, carry_len, tail, tail_next, tail_len, num_streams, n, slots):
        idx = slots[:num_streams].long()
        frames[idx] += n
        if carry_len:
            carry[idx] = carry_next[idx]
        if tail_len:
            tail[idx] = tail_next[idx]


@pytest.fixture()
def emu():
    old = sepkernels._set_backend_for_tests(SelEmu())
    try:
        yield
    finally:
        sepkernels._set_backend_for_tests(old)


# ------------------------------------------------------------------------------------------------------ (a), (b) fp64 parity and isolation
@pytest.mark.parametrize("name,ticks", [("causal16", 486), ("causal16_p5", 330)])
def test_fixture_on_independent_clocks_matches_the_reference_in_fp64(emu, name, ticks):
    """5 slots, the fixture's streams in slots [4, 0, 2], the schedule of run_schedule (calls with every A from 1 to the number of streams; the
    slot of job 0 is reused, once that job has ended, by a job that streams the last row again): every job's pieces and its own flush are its fixture row to
    1e-9 of its maximum, and no call touches a slot it does not name"""
    model, cfg = OC._model(name)
    L, S = cfg["kernel_size"], cfg["stride"]
    xin, ref = OC._fixture(name)
    x = xin[..., L - S:]
    R = x.shape[0]
    sep = model.online_separator(num_streams=5, chunk_size=3 * S)
    # poison what no call may read: the second buffers of every slot (a selected slot's rows are written before sep_online_advance_sel reads them)
    sep.carry_next.fill_(float("nan"))
    sep.tail_next.fill_(float("nan"))
    done, t, sizes = SG.run_schedule(sep, x, [4, 0, 2][:R], isolation=True)
    assert t == ticks and sizes == set(range(1, R + 1))
    assert sorted(row for row, _ in done) == list(range(R)) + [R - 1]
    for row, est in done:
        assert est.shape == ref[row].shape
        assert OC._rel(est, ref[row]) <= 1e-9, (row, OC._rel(est, ref[row]))
    for a in SG.STATE:
        assert not getattr(sep, a).any()                                  # every job was flushed, the slots nobody used never held anything


# ------------------------------------------------------------------------------------------------------ (c) refusals
def test_selections_that_cannot_be_served_are_refused(emu):
    model, cfg = OC._model("causal16_p5")
    S = cfg["stride"]
    sep = model.online_separator(num_streams=4)
    z = lambda rows: torch.zeros(rows, 1, 2 * S, dtype=torch.float64)      # noqa: E731
    before = [getattr(sep, a).clone() for a in SG.STATE]
    with pytest.raises(ValueError, match="duplicate"):
        sep(z(3), streams=[1, 2, 1])
    with pytest.raises(ValueError, match="out of range"):
        sep(z(2), streams=[0, 4])
    with pytest.raises(ValueError, match="out of range"):
        sep(z(1), streams=torch.tensor([-1]))
    with pytest.raises(ValueError, match="empty"):
        sep(z(0), streams=[])
    with pytest.raises(ValueError, match="empty"):
        sep(z(0), streams=torch.zeros(4, dtype=torch.bool))
    with pytest.raises(ValueError, match="mask has 3 entries"):
        sep(z(2), streams=torch.tensor([True, True, False]))
    with pytest.raises(ValueError, match="2 selected streams"):
        sep(z(3), streams=[0, 1])
    with pytest.raises(ValueError, match="2 selected streams"):
        sep(z(4), streams=torch.tensor([True, False, False, True]))
    for bad, what in (([2, 2], "duplicate"), ([7], "out of range"), ([], "empty"), (torch.zeros(5, dtype=torch.bool), "mask has 5 entries")):
        with pytest.raises(ValueError, match=what):
            sep.flush(bad)
    with pytest.raises(ValueError, match="max_recordings"):
        model.online_separator(max_recordings=0)
    for a, b in zip(SG.STATE, before):
        assert torch.equal(getattr(sep, a), b)                             # a refused call leaves no trace


def test_a_bool_mask_selects_in_ascending_order_and_a_tensor_in_its_own(emu):
    model, cfg = OC._model("causal16_p5")
    S = cfg["stride"]
    x = 0.1 * torch.randn(3, 1, 4 * S, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    a, b, c = (model.online_separator(num_streams=4) for _ in range(3))
    ya = a(x, streams=[0, 2, 3])
    yb = b(x, streams=torch.tensor([True, False, True, True]))
    yc = c(x.flip(0).contiguous(), streams=torch.tensor([3, 2, 0]))
    assert torch.equal(ya, yb) and OC._rel(yc.flip(0), ya) <= 1e-12
    assert torch.equal(a.frames, torch.tensor([4, 0, 4, 4])) and torch.equal(c.frames, a.frames)
    assert torch.equal(a.flush([3, 0]), b.flush(torch.tensor([3, 0])))
    assert torch.equal(a.frames, torch.tensor([0, 0, 4, 0]))


# ------------------------------------------------------------------------------------------------------ (f) the two routes to all streams
def test_all_streams_by_name_agree_with_the_plain_call(emu):
    model, cfg = OC._model("causal16")
    L, S = cfg["kernel_size"], cfg["stride"]
    xin, ref = OC._fixture("causal16")
    x = xin[..., L - S:]
    Bs = x.shape[0]
    plain, named = model.online_separator(num_streams=Bs), model.online_separator(num_streams=Bs)
    a, b, t, i = [], [], 0, 0
    while t < x.shape[-1]:
        k = min([3, 1, 12, 2, 5][i % 5] * S, x.shape[-1] - t)
        a.append(plain(x[..., t:t + k].contiguous()))
        b.append(named(x[..., t:t + k].contiguous(), streams=list(range(Bs))))
        t, i = t + k, i + 1
    a, b = torch.cat(a + [plain.flush()], -1), torch.cat(b + [named.flush(list(range(Bs)))], -1)
    assert OC._rel(b, a) <= 1e-9 and OC._rel(b, ref) <= 1e-9


# ------------------------------------------------------------------------------------------------------ (d), (e) on the host simulation
@needs_clang
@pytest.mark.parametrize("name,params", SG.CASES, ids=[c[0][5:] for c in SG.CASES])
def test_online_sel_kernel_source_on_the_host(on_host, name, params):
    for p in params:
        getattr(SG, name)(*p)


@needs_clang
def test_plain_entry_points_are_the_sel_ones_with_the_identity_list(on_host):
    """both forms launch the same kernels: a chunk through sep_online_*_fwd and through the _sel forms with slots = 0 .. Bs-1 is bitwise equal"""
    Bs, C, n, P, d = 3, 16, 5, 3, 2
    ldt = 128
    x, w, b = OG.rnd(C, ldt), OG.rnd(C, P), OG.rnd(C)
    x[:, Bs * n:] = 0
    ring = OG.rnd(Bs, C * (P - 1) * d)
    ident = torch.arange(Bs, dtype=torch.int32)
    r1, r2, y1, y2 = ring.clone(), ring.clone(), torch.zeros(C, ldt), torch.zeros(C, ldt)
    on_host.online_depthwise_fwd(x, w, b, r1.view(-1), r1.shape[1], y1, Bs, C, n, ldt, P, d)
    on_host.online_depthwise_fwd_sel(x, w, b, r2.view(-1), r2.shape[1], y2, Bs, C, n, ldt, P, d, ident)
    assert torch.equal(y1, y2) and torch.equal(r1, r2)
    sums = torch.randn(Bs, 2, dtype=torch.float64)
    frames = torch.tensor([3, 0, 9])
    g, be = OG.rnd(C), OG.rnd(C)
    s1, s2 = sums.clone(), sums.clone()
    on_host.online_cln_fwd(x, None, g, be, y1, s1.view(-1), 2, frames, Bs, C, n, ldt, 1e-8)
    on_host.online_cln_fwd_sel(x, None, g, be, y2, s2.view(-1), 2, frames, Bs, C, n, ldt, 1e-8, ident)
    assert torch.equal(y1, y2) and torch.equal(s1, s2)


SELECTIONS = [[0, 1], [2, 3], [4], [1, 0, 3], [2, 4, 0], [3], [0, 1, 2, 4], [4, 3, 2, 1], [1, 2], [0], [3, 4], [4, 1, 0], [2], [0, 3, 1, 2], [4, 2],
              [1, 3, 4]]


@needs_clang
def test_recorded_subset_steps_equal_eager_launches_bitwise(on_host):
    """the tiny model of tests/test_online_cpu.py in 5 slots, 16 subset calls at the recorded chunk size whose equal-size selections differ in
    membership and order (a replay that kept the first call's slot list would fail), with four distinct sizes against two kept recordings (so
    recordings are evicted and made again); then every slot is flushed.  Recorded == eager to the last bit, and every slot's output is the
    offline staged forward on what it received"""
    model = OC._tiny()
    hop, S, L = 2, 4, 8
    x = 0.1 * torch.randn(5, 1, len(SELECTIONS) * hop * S, generator=torch.Generator().manual_seed(6))
    old = sepkernels._set_backend_for_tests(OC._Named(on_host))
    try:
        runs = []
        for record in (True, False):
            sep = model.online_separator(num_streams=5, chunk_size=hop * S, record=record, max_recordings=2)
            assert sep.record == record
            done, outs = [0] * 5, [[] for _ in range(5)]
            for idx in SELECTIONS:
                chunk = torch.stack([x[s, :, done[s] * hop * S:(done[s] + 1) * hop * S] for s in idx]).contiguous()
                y = sep(chunk, streams=idx)
                for r, s in enumerate(idx):
                    outs[s].append(y[r])
                    done[s] += 1
                assert len(sep._sub_seqs) <= 2
            if record:
                assert len(sep._sub_seqs) == 2 and len(sep._ws) == 1 and all(len(q) > 10 for q in sep._sub_seqs.values())
                assert sep.launches_per_chunk() is None                     # no all-streams step was recorded
            tails = sep.flush(list(range(5)))
            runs.append([torch.cat(outs[s] + [tails[s]], -1) for s in range(5)])
        with torch.no_grad():
            refs = [model(F.pad(x[s:s + 1, :, :done[s] * hop * S], (L - S, 0)))[0] for s in range(5)]
    finally:
        sepkernels._set_backend_for_tests(old)
    for s in range(5):
        assert torch.equal(runs[0][s], runs[1][s]), "slot {}: recorded differs from eager".format(s)
        assert OC._rel(runs[0][s], refs[s]) <= 1e-5, (s, OC._rel(runs[0][s], refs[s]))


@needs_clang
@pytest.mark.parametrize("unit", [1, 9])
def test_all_streams_recording_replays_after_subset_and_ragged_passes_on_its_workspace(on_host, unit):
    """the three call forms of the tiny model interleaved on one workspace (test_online_streams_gpu.check_mixed_forms_share_a_workspace) on the
    kernel sources, to 1e-5 of every slot's maximum, the bar of the test above"""
    old = sepkernels._set_backend_for_tests(OC._Named(on_host))
    try:
        SG.check_mixed_forms_share_a_workspace(OC._tiny(), 8, 4, 1e-5, unit)
    finally:
        sepkernels._set_backend_for_tests(old)
