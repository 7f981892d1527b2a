"""GPU: online separation with streams on their own clocks -- sep(chunk, streams=...), flush(streams), the sep_online_*_sel entry points
(sepkernels/online.py, csrc/online.hip).

The kernel cases (`case_*`, listed in CASES) feed chunk after chunk through a SELECTION of the slots of the state buffers and compare with the
fp64 restatements of tests/test_online_gpu.py (bars as there: 2e-5 for outputs, 0 for carry and ring, 1e-6 for the fp64 sums).  Before the
first chunk the unselected slots hold sentinels -- finite values in the state, NaN in carry_next / tail_next -- and afterwards every unselected
entry is bitwise its sentinel.  tests/test_online_streams_cpu.py runs the same functions on the host simulation of the kernel sources (they go
through test_online_gpu's HIP, to_device and device_sync, which it swaps).  The model tests drive the reference's fixture through a schedule in
which every stream starts, pauses, ends and restarts on its own (run_schedule), a paper-size model with a different half of 64 slots in
every call, and all-streams, subset and ragged calls interleaved on the one workspace of their width (check_mixed_forms_share_a_workspace, also
run by the CPU module on the kernel sources)."""
import os

import numpy as np
import pytest
import torch

import sepkernels
import test_online_gpu as OG
from test_online_gpu import _round_up, close, cols, ref_cln, ref_decoder, ref_depthwise, ref_encoder, rnd, uncols

pytestmark = pytest.mark.gpu

ROOT = OG.ROOT
NAN = float("nan")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(got, want, what):
    assert torch.equal(_bits(got), _bits(want)), what + ": an entry of an unselected slot changed"


def _others(Bs, sel):
    return [s for s in range(Bs) if s not in sel]


def _slots(sel):
    return OG.to_device(torch.tensor(sel, dtype=torch.int32))


def _sentinel(shape, sel, selected=0.0):
    """finite sentinels everywhere, `selected` in the rows of the selection"""
    t = rnd(*shape) + 3.0
    t[sel] = selected
    return t


# ------------------------------------------------------------------------------------------------------ kernel cases
def case_encoder_sel(Bs, sel, N, L, S, plan, relu):
    A, keep, total = len(sel), L - S, sum(plan)
    x = rnd(A, total * S)
    E = rnd(N, L, scale=0.3)
    ref = ref_encoder(torch.cat([torch.zeros(A, keep), x], 1), E, S, relu)
    carry0 = _sentinel((Bs, keep), sel)
    frames0 = torch.arange(1000, 1000 + Bs, dtype=torch.int64)
    frames0[sel] = 0
    carry, carry_next, frames = OG.to_device(carry0), OG.to_device(torch.full((Bs, keep), NAN)), OG.to_device(frames0)
    Ed, slots = OG.to_device(E), _slots(sel)
    f0 = 0
    for n in plan:
        ldt = _round_up(A * n, 128)
        w = OG.to_device(torch.full((N, ldt), NAN))
        chunk = OG.to_device(x[:, f0 * S:(f0 + n) * S].contiguous())
        OG.HIP.online_encoder_fwd_sel(chunk, Ed, carry, carry_next, w, A, N, L, S, n, ldt, relu, slots)
        OG.HIP.online_advance_sel(frames, carry, carry_next, keep, None, None, 0, A, n, slots)
        OG.device_sync()
        wc = w.cpu()
        assert torch.equal(wc[:, A * n:], torch.zeros(N, ldt - A * n)), "encoder: pad columns not zero"
        close(uncols(wc, A, n), ref[..., f0:f0 + n], 2e-5, "encoder w, chunk at frame {}".format(f0))
        f0 += n
    rest = _others(Bs, sel)
    if keep:
        close(carry.cpu()[sel], torch.cat([torch.zeros(A, keep), x], 1)[:, -keep:], 0, "encoder carry")
        same_bits(carry.cpu()[rest], carry0[rest], "carry")
        same_bits(carry_next.cpu()[rest], torch.full((len(rest), keep), NAN), "carry_next")
    fc = frames.cpu()
    assert torch.equal(fc[sel], torch.full((A,), total, dtype=torch.int64)) and torch.equal(fc[rest], frames0[rest])


def case_cln_sel(Bs, sel, C, plan, act):
    A, total = len(sel), sum(plan)
    x = rnd(A, C, total, scale=1.5) + 0.3
    gamma, beta = rnd(C) * 0.2 + 1.0, rnd(C) * 0.1
    alpha = torch.tensor([0.2]) if act else None
    u = torch.where(x > 0, x, 0.2 * x) if act else x
    ref = ref_cln(u.double(), gamma, beta, 1e-8)
    nn = 3                                                       # the norm under test sits at slot 1 of 3 of a stream's sums
    sums0 = torch.randn(Bs, 2 * nn, generator=OG.G, dtype=torch.float64) + 77.0
    sums0[sel] = 0.0
    for s in sel:
        sums0[s, 4:] = 123.0
    frames0 = torch.arange(1000, 1000 + Bs, dtype=torch.int64)
    frames0[sel] = 0
    sums_d, frames = OG.to_device(sums0), OG.to_device(frames0)
    g_d, b_d, a_d = OG.to_device(gamma), OG.to_device(beta), (OG.to_device(alpha) if act else None)
    slots = _slots(sel)
    f0 = 0
    for n in plan:
        ldt = _round_up(A * n, 128)
        xd = OG.to_device(cols(x[..., f0:f0 + n], A, n, ldt))
        y = OG.to_device(torch.full((C, ldt), NAN))
        OG.HIP.online_cln_fwd_sel(xd, a_d, g_d, b_d, y, sums_d.view(-1)[2:], 2 * nn, frames, A, C, n, ldt, 1e-8, slots)
        OG.HIP.online_advance_sel(frames, None, None, 0, None, None, 0, A, n, slots)
        OG.device_sync()
        yc = y.cpu()
        assert torch.equal(yc[:, A * n:], torch.zeros(C, ldt - A * n)), "cln: pad columns not zero"
        close(uncols(yc, A, n), ref[..., f0:f0 + n], 2e-5, "cln y, chunk at frame {}".format(f0))
        f0 += n
    s, rest = sums_d.cpu(), _others(Bs, sel)
    close(s[sel, 2], u.double().sum((1, 2)), 1e-6, "cln running sum")
    close(s[sel, 3], (u.double() ** 2).sum((1, 2)), 1e-6, "cln running sum of squares")
    assert torch.equal(s[sel][:, :2], torch.zeros(A, 2, dtype=torch.float64)) and torch.equal(s[sel][:, 4:], torch.full((A, 2), 123.0, dtype=torch.float64))
    same_bits(s[rest], sums0[rest], "sums")
    fc = frames.cpu()
    assert torch.equal(fc[sel], torch.full((A,), total, dtype=torch.int64)) and torch.equal(fc[rest], frames0[rest])


def case_depthwise_sel(Bs, sel, C, plan, P, d):
    A, total, D = len(sel), sum(plan), (P - 1) * d
    x = rnd(A, C, total)
    w, b = rnd(C, P, scale=0.5), rnd(C, scale=0.1)
    ref = ref_depthwise(x, w, b, d)
    off, stride = 5, C * D + 9
    rings0 = _sentinel((Bs, stride), sel)
    rings = OG.to_device(rings0)
    wd, bd, slots = OG.to_device(w), OG.to_device(b), _slots(sel)
    f0 = 0
    for n in plan:
        ldt = _round_up(A * n, 128)
        xd = OG.to_device(cols(x[..., f0:f0 + n], A, n, ldt))
        y = OG.to_device(torch.full((C, ldt), NAN))
        OG.HIP.online_depthwise_fwd_sel(xd, wd, bd, rings.view(-1)[off:], stride, y, A, C, n, ldt, P, d, slots)
        OG.device_sync()
        yc = y.cpu()
        assert torch.equal(yc[:, A * n:], torch.zeros(C, ldt - A * n)), "depthwise: pad columns not zero"
        close(uncols(yc, A, n), ref[..., f0:f0 + n], 2e-5, "depthwise y, chunk at frame {}".format(f0))
        f0 += n
    r, rest = rings.cpu(), _others(Bs, sel)
    hist = torch.nn.functional.pad(x, (D, 0))[..., -D:]
    close(r[sel][:, off:off + C * D].reshape(A, C, D), hist, 0, "depthwise ring")
    assert torch.equal(r[sel][:, :off], torch.zeros(A, off)) and torch.equal(r[sel][:, off + C * D:], torch.zeros(A, stride - off - C * D))
    same_bits(r[rest], rings0[rest], "ring")


def case_decoder_sel(Bs, sel, n_src, N, L, S, plan):
    A, keep, total = len(sel), L - S, sum(plan)
    w, m = rnd(A, N, total), torch.rand(A, n_src, N, total, generator=OG.G).float()
    D = rnd(N, L, scale=0.3)
    ref = ref_decoder(w.unsqueeze(1) * m, D, S)
    tail0 = _sentinel((Bs, n_src, keep), sel)
    tail, tail_next = OG.to_device(tail0), OG.to_device(torch.full((Bs, n_src, keep), NAN))
    frames = OG.to_device(torch.zeros(Bs, dtype=torch.int64))
    Dd, slots = OG.to_device(D), _slots(sel)
    f0, got = 0, []
    for n in plan:
        ldt = _round_up(A * n, 128)
        wd = OG.to_device(cols(w[..., f0:f0 + n], A, n, ldt))
        md = OG.to_device(torch.cat([cols(m[:, s, :, f0:f0 + n], A, n, ldt) for s in range(n_src)], 0))
        out = OG.to_device(torch.full((A, n_src, n * S), NAN))
        OG.HIP.online_decoder_fwd_sel(wd, md, Dd, tail, tail_next, out, A, n_src, N, L, S, n, ldt, slots)
        OG.HIP.online_advance_sel(frames, None, None, 0, tail, tail_next, n_src * keep, A, n, slots)
        OG.device_sync()
        got.append(out.cpu())
        f0 += n
    got.append(tail.cpu()[sel])
    close(torch.cat(got, -1), ref, 2e-5, "decoder output")
    rest = _others(Bs, sel)
    if keep:
        same_bits(tail.cpu()[rest], tail0[rest], "tail")
        same_bits(tail_next.cpu()[rest], torch.full((len(rest), n_src, keep), NAN), "tail_next")


def case_advance_sel(Bs, sel, keep, n_src, n):
    """the counters move by n and both copies are made for the selected slots; nothing else changes, the second buffers not at all"""
    A, tl = len(sel), n_src * keep
    frames0 = torch.arange(1000, 1000 + Bs, dtype=torch.int64)
    host = [frames0, rnd(Bs, keep) + 3, rnd(Bs, keep) - 3, rnd(Bs, tl) + 3, rnd(Bs, tl) - 3]
    frames, carry, carry_next, tail, tail_next = [OG.to_device(t) for t in host]
    OG.HIP.online_advance_sel(frames, carry if keep else None, carry_next if keep else None, keep, tail if tl else None, tail_next if tl else None, tl,
                              A, n, _slots(sel))
    OG.device_sync()
    rest = _others(Bs, sel)
    fc = frames.cpu()
    assert torch.equal(fc[sel], frames0[sel] + n) and torch.equal(fc[rest], frames0[rest])
    for cur, nxt, cur0, nxt0, what in ((carry, carry_next, host[1], host[2], "carry"), (tail, tail_next, host[3], host[4], "tail")):
        same_bits(cur.cpu()[sel], nxt0[sel], what + " of the selected slots")
        same_bits(cur.cpu()[rest], cur0[rest], what)
        same_bits(nxt.cpu(), nxt0, what + "_next")


CASES = [
    # 5 slots, an unordered selection with gaps; one selected slot with one-hop chunks, then across the cLN's 32-frame tile; a slot index beyond
    # any 256-wide indexing with A far below the slot count; a history longer than the chunk; L == S (no carry, no tail)
    ("case_encoder_sel", [(5, [4, 0, 2], 32, 20, 10, [7, 1, 12], 1), (5, [3], 16, 16, 4, [1, 1, 1, 2, 1], 0), (257, [256, 0], 16, 16, 8, [1, 2], 1),
                          (2, [1], 16, 16, 16, [3, 1], 0)]),
    ("case_cln_sel", [(5, [4, 0, 2], 48, [7, 1, 33], False), (5, [3], 16, [1] * 5 + [40, 3], True), (257, [256, 0], 16, [1, 2], True)]),
    ("case_depthwise_sel", [(5, [4, 0, 2], 32, [5, 1, 9, 30], 5, 4), (5, [3], 16, [1] * 6 + [40], 3, 2), (257, [256, 0], 16, [1, 2], 3, 2),
                            (3, [2, 1], 16, [1] * 6, 3, 128)]),
    ("case_decoder_sel", [(5, [4, 0, 2], 3, 32, 20, 10, [7, 1, 12]), (5, [3], 2, 16, 16, 4, [1, 1, 1, 3]), (257, [256, 0], 2, 16, 16, 8, [1, 2]),
                          (2, [1], 2, 16, 8, 8, [2, 1])]),
    ("case_advance_sel", [(5, [4, 0, 2], 8, 2, 3), (257, [256, 0], 10, 3, 1), (2, [1], 0, 3, 5)]),
]


@pytest.mark.parametrize("name,params", CASES, ids=[c[0][5:] for c in CASES])
def test_online_sel_kernels_against_the_restatement(name, params):
    for p in params:
        globals()[name](*p)


# ------------------------------------------------------------------------------------------------------ streams on their own clocks
HOPS = [3, 1, 7, 2]
STATE = ("frames", "carry", "sums", "rings", "tail")


def run_schedule(sep, x, slots, isolation=False):
    """x (R, 1, T): fixture row k is job k in slot slots[k].  Tick t offers HOPS[t % 4] hops.  Job k starts at tick 3 k, sits out every tick with
    (t + k) % (k + 2) == 0 and every tick that offers more hops than it has left; the index list of a call is ascending on even ticks and
    descending on odd ones.  A job that reaches its end is ended with flush([slot]) while the others go on; when job 0 ends, its slot is taken
    by a new job (k = R) that streams the last row again from the start.
    -> ([(row, output (n_src, T + L - S))] per job, ticks, the set of call sizes A).  isolation: after every call the unselected slots' slices
    of the five state tensors must be what they were, and after flush([s]) only slot s is zero."""
    S, R, total = sep.S, x.shape[0], x.shape[-1] // sep.S
    jobs = [dict(k=k, row=k, slot=slots[k], start=3 * k, done=0, out=[]) for k in range(R)]
    finished, sizes, t = [], set(), 0

    def snapshot():
        return [getattr(sep, a).clone() for a in STATE]

    def untouched(before, touched, what):
        rest = [s for s in range(sep.num_streams) if s not in touched]
        for a, b in zip(STATE, before):
            assert torch.equal(getattr(sep, a)[rest], b[rest]), "{}: {} of an unselected slot changed".format(what, a)

    while jobs:
        h = HOPS[t % len(HOPS)]
        live = [j for j in jobs if t >= j["start"] and (t + j["k"]) % (j["k"] + 2) != 0 and h <= total - j["done"]]
        live.sort(key=lambda j: j["slot"], reverse=bool(t % 2))
        if live:
            idx = [j["slot"] for j in live]
            chunk = torch.stack([x[j["row"], :, j["done"] * S:(j["done"] + h) * S] for j in live]).contiguous()
            before = snapshot() if isolation else None
            y = sep(chunk, streams=idx)
            assert y.shape == (len(live), sep.n_src, h * S)
            sizes.add(len(live))
            if isolation:
                untouched(before, idx, "sep(chunk, streams={})".format(idx))
            for r, j in enumerate(live):
                j["out"].append(y[r])
                j["done"] += h
        for j in [j for j in jobs if j["done"] == total]:
            before = snapshot() if isolation else None
            j["out"].append(sep.flush([j["slot"]])[0])
            if isolation:
                untouched(before, [j["slot"]], "flush([{}])".format(j["slot"]))
                for a in STATE:
                    assert not getattr(sep, a)[j["slot"]].any(), "flush([{}]): {} of the slot is not zero".format(j["slot"], a)
            jobs.remove(j)
            finished.append((j["row"], torch.cat(j["out"], -1)))
            if j["k"] == 0:
                jobs.append(dict(k=R, row=R - 1, slot=j["slot"], start=max(3 * R, t + 1), done=0, out=[]))
        t += 1
        assert t < 5000, "the schedule does not terminate"
    return finished, t, sizes


@pytest.mark.parametrize("arith", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("name", ["causal16", "causal16_p5"])
def test_fixture_on_independent_clocks_matches_the_reference_on_the_device(name, arith):
    """the schedule of run_schedule in 5 slots, streams in slots [4, 0, 2]: every job within 1e-3 of its fixture row (the bar of the all-streams
    test), recorded per A, and bitwise what the eager launches (record=False) give on the same schedule"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_causal_online.npz"))
    prev = sepkernels.set_gemm_arith(arith)
    try:
        model, cfg = OG._fixture_model(name)
        x = torch.from_numpy(g[name + "/input"])[..., cfg["kernel_size"] - cfg["stride"]:].cuda()
        ref = torch.from_numpy(g[name + "/output_f64"])
        slots = [4, 0, 2][:x.shape[0]]
        runs = []
        for record in (True, False):
            sep = model.online_separator(num_streams=5, chunk_size=3 * cfg["stride"], record=record)
            done, _, sizes = run_schedule(sep, x, slots)
            assert len(done) == x.shape[0] + 1 and sizes == set(range(1, x.shape[0] + 1))
            runs.append(done)
        for (row, est), (row_e, est_e) in zip(*runs):
            close(est, ref[row], 1e-3, "{} {} job of row {}".format(name, arith, row))
            assert row == row_e and torch.equal(est, est_e), "recorded subset steps differ from eager launches"
    finally:
        sepkernels.set_gemm_arith(prev)


# ------------------------------------------------------------------------------------------------------ the three call forms on one workspace
# (slots, hops per slot) at the recorded width of 3 hops: slots None is the all-streams call, hops None a uniform call, an integer an all-streams
# call at that other width.  The all-streams recording is replayed after subset and ragged passes have run over the storage it points into; the
# subset and ragged calls change size, members and order; their recordings of A = 3 and of two rows with ldt 128 are replayed once each, then A = 2
# and three ragged rows come in and push both out of the two that are kept.
MIXED = [(None, None), ([3, 0, 4], None), (None, None), ([1, 4], [2, 3]), (None, None), ([4, 1, 0], None), ([0, 3], [3, 1]), ([2, 1], None),
         (None, None), ([4, 0, 2], [1, 3, 2]), (None, 2), ([1, 2], None), (None, None)]


def check_mixed_forms_share_a_workspace(model, L, S, tol, unit=1):
    """5 slots, chunk_size 3 hops, max_recordings 2, the calls of MIXED (the eleventh runs eagerly), then every slot flushed.  A recording separator
    and an eager one agree to the last bit for every slot; every slot's output is the offline forward on what it received within tol of its
    maximum; the recorded width has one workspace; the all-streams recording is one object from its first call on, and at most two of the
    others are kept at any time.  With unit = 1 every pass has ldt 128 and the passes differ in which columns they use; `unit` multiplies every
    hop count, and at 9 the all-streams pass has ldt 256 and the subset and ragged passes 128 inside the same storage"""
    flat = model.flat_parameters()
    x = 0.1 * torch.randn(5, 1, 30 * unit * S, generator=torch.Generator().manual_seed(23)).to(device=flat.device, dtype=flat.dtype)
    runs = []
    for record in (True, False):
        sep = model.online_separator(num_streams=5, chunk_size=3 * unit * S, record=record, max_recordings=2)
        assert sep.record == record
        pos, outs, first = [0] * 5, [[] for _ in range(5)], None
        for slots, hops in MIXED:
            idx = list(range(5)) if slots is None else slots
            ragged = isinstance(hops, list)
            n = unit * (hops if isinstance(hops, int) else 3)
            counts = [unit * h for h in hops] if ragged else [n] * len(idx)
            chunk = torch.zeros(len(idx), 1, n * S, device=x.device, dtype=x.dtype)
            for j, (s, h) in enumerate(zip(idx, counts)):
                chunk[j, 0, :h * S] = x[s, 0, pos[s] * S:(pos[s] + h) * S]
            y = sep(chunk, streams=slots, lengths=[h * S for h in counts] if ragged else None)
            assert y.shape == (len(idx), sep.n_src, n * S)
            for j, (s, h) in enumerate(zip(idx, counts)):
                assert not y[j, :, h * S:].any()
                outs[s].append(y[j, :, :h * S])
                pos[s] += h
            first = sep._seq if first is None else first
            assert sep._seq is first and len(sep._sub_seqs) <= 2 and 3 * unit in sep._ws and set(sep._ws) <= {3 * unit, 2 * unit}
        if record:
            assert first is not None and sep.launches_per_chunk() == len(first) and list(sep._sub_seqs) == [(3, 128), 2] and sum(sep.replays.values()) == 1
        else:
            assert first is None and not sep._sub_seqs
        tails = sep.flush()
        runs.append([torch.cat(outs[s] + [tails[s]], -1) for s in range(5)])
    for s in range(5):
        assert torch.equal(runs[0][s], runs[1][s]), "slot {}: recorded differs from eager".format(s)
        with torch.no_grad():
            ref = model(torch.nn.functional.pad(x[s:s + 1, :, :pos[s] * S], (L - S, 0)))[0]
        close(runs[0][s], ref.cpu(), tol, "slot {} after {} hops".format(s, pos[s]))


@pytest.mark.parametrize("unit", [1, 9])
def test_all_streams_recording_replays_after_subset_and_ragged_passes_on_its_workspace(unit):
    """causal16_p5 in the default arithmetic, to the 1e-3 bar of test_fixture_on_independent_clocks_matches_the_reference_on_the_device"""
    model, cfg = OG._fixture_model("causal16_p5")
    check_mixed_forms_share_a_workspace(model, cfg["kernel_size"], cfg["stride"], 1e-3, unit)


def test_paper_size_model_with_a_different_half_of_64_slots_in_every_call():
    """N512 L16 S8 H512 B128 Sc128 P3 X8 R3 in 64 slots, 20 chunks of 80 samples, each for a fresh half of the slots in a fresh order: every
    slot's pieces and its flush within 1e-4 of the offline staged forward on what that slot received (the bar of the all-streams paper-size test:
    same product kernels and weight bound, only the column a frame sits in differs)"""
    from models.conv_tasnet import ConvTasNet
    torch.manual_seed(0)
    model = ConvTasNet(**OG.PAPER).cuda()
    Bs, L, S, calls, size = 64, 16, 8, 20, 80
    g = torch.Generator().manual_seed(11)
    x = 0.1 * torch.randn(Bs, 1, calls * size, generator=g).cuda()
    sep = model.online_separator(num_streams=Bs, chunk_size=size)
    done, outs = [0] * Bs, [[] for _ in range(Bs)]
    for _ in range(calls):
        idx = torch.randperm(Bs, generator=g)[:Bs // 2].tolist()
        chunk = torch.stack([x[s, :, done[s] * size:(done[s] + 1) * size] for s in idx]).contiguous()
        y = sep(chunk, streams=idx)
        for r, s in enumerate(idx):
            outs[s].append(y[r])
            done[s] += 1
    tails = sep.flush(list(range(Bs)))
    assert not sep.frames.any() and not sep.tail.any()
    for count in sorted(set(done) - {0}):
        group = [s for s in range(Bs) if done[s] == count]
        with torch.no_grad():
            ref = model(torch.nn.functional.pad(x[group][..., :count * size], (L - S, 0)))
        est = torch.stack([torch.cat(outs[s] + [tails[s]], -1) for s in group])
        close(est, ref.cpu(), 1e-4, "slots that received {} chunks".format(count))
