"""GPU: ragged online calls -- sep(chunk, streams=..., lengths=...), sep([x0, x1, ...], streams=...), the sep_online_*_rag entry points
(sepkernels/online.py, csrc/online.hip).

The kernel cases (`case_*`, listed in CASES) feed call after call through a SELECTION of the slots, every selected stream bringing its own number
of frames to every call (a `plan` is a list of calls, a call a list of per-block lengths), and compare with the fp64 restatements of
tests/test_online_gpu.py (bars as there: 2e-5 for outputs, 0 for carry and ring, 1e-6 for the fp64 sums).  Column block j of a call is
[offs[j], offs[j + 1]) and ldt = round_up(offs[A], 128).  Before the first call the unselected slots hold finite sentinels and carry_next /
tail_next hold NaN; afterwards every unselected entry is bitwise its sentinel.  Outputs are pre-filled with NaN and their pad columns
[offs[A], ldt) must come back as zero; the pad columns of the INPUT matrices hold NaN (no state kernel may read them); chunk rows hold NaN
beyond their length; out beyond n_j S must be exactly zero.  The row pitch n_cap of chunk / out is the widest block on even calls and one hop
more on odd ones.  tests/test_online_ragged_cpu.py runs the same functions on the host simulation of the kernel sources (they go through
test_online_gpu's HIP, to_device and device_sync, which it swaps).  The model tests drive the reference's fixture through a schedule in which
every job brings its own number of hops to every call (run_ragged_schedule), and a paper-size model with a different half of 64 slots and
different lengths in every call."""
import os

import numpy as np
import pytest
import torch

import sepkernels
import test_online_gpu as OG
from test_online_gpu import _round_up, close, ref_cln, ref_decoder, ref_depthwise, ref_encoder, rnd
from test_online_streams_gpu import NAN, STATE, _others, _sentinel, _slots, same_bits

pytestmark = pytest.mark.gpu

ROOT = OG.ROOT


def _layout(call, k):
    """-> (A, offs list, total columns, ldt, n_cap) of call number k of a plan"""
    offs = [0]
    for n in call:
        offs.append(offs[-1] + n)
    return len(call), offs, offs[-1], _round_up(offs[-1], 128), max(call) + k % 2


def _offs(offs):
    return OG.to_device(torch.tensor(offs, dtype=torch.int32))


def rcols(parts, ldt):
    """[(C, n_j)] -> compact (C, ldt) columns, NaN beyond the last block"""
    m = torch.cat(parts, 1)
    return torch.cat([m, torch.full((m.shape[0], ldt - m.shape[1]), NAN, dtype=m.dtype)], 1)


# ------------------------------------------------------------------------------------------------------ kernel cases
def case_encoder_rag(Bs, sel, N, L, S, plan, relu):
    A, keep = len(sel), L - S
    totals = [sum(call[j] for call in plan) for j in range(A)]
    x = [rnd(1, t * S) for t in totals]
    E = rnd(N, L, scale=0.3)
    ref = [ref_encoder(torch.cat([torch.zeros(1, keep), xj], 1), E, S, relu)[0] for xj in x]          # (N, total_j) each
    carry0 = _sentinel((Bs, keep), sel)
    frames0 = torch.arange(1000, 1000 + Bs, dtype=torch.int64)
    frames0[sel] = 0
    carry, carry_next, frames = OG.to_device(carry0), OG.to_device(torch.full((Bs, keep), NAN)), OG.to_device(frames0)
    Ed, slots = OG.to_device(E), _slots(sel)
    done = [0] * A
    for k, call in enumerate(plan):
        _, offs, cols, ldt, cap = _layout(call, k)
        w = OG.to_device(torch.full((N, ldt), NAN))
        ch = torch.full((A, cap * S), NAN)
        for j, n in enumerate(call):
            ch[j, :n * S] = x[j][0, done[j] * S:(done[j] + n) * S]
        od = _offs(offs)
        OG.HIP.online_encoder_fwd_rag(OG.to_device(ch), Ed, carry, carry_next, w, A, N, L, S, cap, ldt, relu, slots, od)
        OG.HIP.online_advance_rag(frames, carry, carry_next, keep, None, None, 0, A, cap, slots, od)
        OG.device_sync()
        wc = w.cpu()
        assert torch.equal(wc[:, cols:], torch.zeros(N, ldt - cols)), "encoder: pad columns not zero"
        for j, n in enumerate(call):
            close(wc[:, offs[j]:offs[j + 1]], ref[j][:, done[j]:done[j] + n], 2e-5, "encoder w, call {} block {}".format(k, j))
            done[j] += n
    rest = _others(Bs, sel)
    if keep:
        want = torch.stack([torch.cat([torch.zeros(keep), xj[0]])[-keep:] for xj in x])
        close(carry.cpu()[sel], want, 0, "encoder carry")
        same_bits(carry.cpu()[rest], carry0[rest], "carry")
        same_bits(carry_next.cpu()[rest], torch.full((len(rest), keep), NAN), "carry_next")
    fc = frames.cpu()
    assert torch.equal(fc[sel], torch.tensor(totals, dtype=torch.int64)) and torch.equal(fc[rest], frames0[rest])


def case_cln_rag(Bs, sel, C, plan, act):
    A = len(sel)
    totals = [sum(call[j] for call in plan) for j in range(A)]
    x = [rnd(C, t, scale=1.5) + 0.3 for t in totals]
    gamma, beta = rnd(C) * 0.2 + 1.0, rnd(C) * 0.1
    alpha = torch.tensor([0.2]) if act else None
    u = [torch.where(xj > 0, xj, 0.2 * xj) if act else xj for xj in x]
    ref = [ref_cln(uj.double().unsqueeze(0), gamma, beta, 1e-8)[0] for uj in u]
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
    done = [0] * A
    for k, call in enumerate(plan):
        _, offs, cols, ldt, cap = _layout(call, k)
        xd = OG.to_device(rcols([x[j][:, done[j]:done[j] + n] for j, n in enumerate(call)], ldt))
        y = OG.to_device(torch.full((C, ldt), NAN))
        od = _offs(offs)
        OG.HIP.online_cln_fwd_rag(xd, a_d, g_d, b_d, y, sums_d.view(-1)[2:], 2 * nn, frames, A, C, cap, ldt, 1e-8, slots, od)
        OG.HIP.online_advance_rag(frames, None, None, 0, None, None, 0, A, cap, slots, od)
        OG.device_sync()
        yc = y.cpu()
        assert torch.equal(yc[:, cols:], torch.zeros(C, ldt - cols)), "cln: pad columns not zero"
        for j, n in enumerate(call):
            close(yc[:, offs[j]:offs[j + 1]], ref[j][:, done[j]:done[j] + n], 2e-5, "cln y, call {} block {}".format(k, j))
            done[j] += n
    s, rest = sums_d.cpu(), _others(Bs, sel)
    close(s[sel, 2], torch.stack([uj.double().sum() for uj in u]), 1e-6, "cln running sum")
    close(s[sel, 3], torch.stack([(uj.double() ** 2).sum() for uj in u]), 1e-6, "cln running sum of squares")
    assert torch.equal(s[sel][:, :2], torch.zeros(A, 2, dtype=torch.float64)) and torch.equal(s[sel][:, 4:], torch.full((A, 2), 123.0, dtype=torch.float64))
    same_bits(s[rest], sums0[rest], "sums")
    fc = frames.cpu()
    assert torch.equal(fc[sel], torch.tensor(totals, dtype=torch.int64)) and torch.equal(fc[rest], frames0[rest])


def case_depthwise_rag(Bs, sel, C, plan, P, d):
    A, D = len(sel), (P - 1) * d
    totals = [sum(call[j] for call in plan) for j in range(A)]
    x = [rnd(C, t) for t in totals]
    w, b = rnd(C, P, scale=0.5), rnd(C, scale=0.1)
    ref = [ref_depthwise(xj.unsqueeze(0), w, b, d)[0] for xj in x]
    off, stride = 5, C * D + 9                                   # the ring of the layer sits inside a wider per-stream buffer
    rings0 = _sentinel((Bs, stride), sel)
    rings = OG.to_device(rings0)
    wd, bd, slots = OG.to_device(w), OG.to_device(b), _slots(sel)
    done = [0] * A
    for k, call in enumerate(plan):
        _, offs, cols, ldt, cap = _layout(call, k)
        xd = OG.to_device(rcols([x[j][:, done[j]:done[j] + n] for j, n in enumerate(call)], ldt))
        y = OG.to_device(torch.full((C, ldt), NAN))
        OG.HIP.online_depthwise_fwd_rag(xd, wd, bd, rings.view(-1)[off:], stride, y, A, C, cap, ldt, P, d, slots, _offs(offs))
        OG.device_sync()
        yc = y.cpu()
        assert torch.equal(yc[:, cols:], torch.zeros(C, ldt - cols)), "depthwise: pad columns not zero"
        for j, n in enumerate(call):
            close(yc[:, offs[j]:offs[j + 1]], ref[j][:, done[j]:done[j] + n], 2e-5, "depthwise y, call {} block {}".format(k, j))
            done[j] += n
    r, rest = rings.cpu(), _others(Bs, sel)
    hist = torch.stack([torch.nn.functional.pad(xj, (D, 0))[:, -D:] for xj in x])
    close(r[sel][:, off:off + C * D].reshape(A, C, D), hist, 0, "depthwise ring")
    assert torch.equal(r[sel][:, :off], torch.zeros(A, off)) and torch.equal(r[sel][:, off + C * D:], torch.zeros(A, stride - off - C * D))
    same_bits(r[rest], rings0[rest], "ring")


def case_decoder_rag(Bs, sel, n_src, N, L, S, plan):
    A, keep = len(sel), L - S
    totals = [sum(call[j] for call in plan) for j in range(A)]
    w = [rnd(N, t) for t in totals]
    m = [torch.rand(n_src, N, t, generator=OG.G).float() for t in totals]
    D = rnd(N, L, scale=0.3)
    ref = [ref_decoder((wj.unsqueeze(0) * mj).unsqueeze(0), D, S)[0] for wj, mj in zip(w, m)]      # (n_src, S (total_j - 1) + L) each
    tail0 = _sentinel((Bs, n_src, keep), sel)
    tail, tail_next = OG.to_device(tail0), OG.to_device(torch.full((Bs, n_src, keep), NAN))
    frames = OG.to_device(torch.zeros(Bs, dtype=torch.int64))
    Dd, slots = OG.to_device(D), _slots(sel)
    done, got = [0] * A, [[] for _ in range(A)]
    for k, call in enumerate(plan):
        _, offs, cols, ldt, cap = _layout(call, k)
        wd = OG.to_device(rcols([w[j][:, done[j]:done[j] + n] for j, n in enumerate(call)], ldt))
        md = OG.to_device(torch.cat([rcols([m[j][s, :, done[j]:done[j] + n] for j, n in enumerate(call)], ldt) for s in range(n_src)], 0))
        out = OG.to_device(torch.full((A, n_src, cap * S), NAN))
        od = _offs(offs)
        OG.HIP.online_decoder_fwd_rag(wd, md, Dd, tail, tail_next, out, A, n_src, N, L, S, cap, ldt, slots, od)
        OG.HIP.online_advance_rag(frames, None, None, 0, tail, tail_next, n_src * keep, A, cap, slots, od)
        OG.device_sync()
        oc = out.cpu()
        for j, n in enumerate(call):
            assert torch.equal(oc[j, :, n * S:], torch.zeros(n_src, (cap - n) * S)), "decoder: out beyond n_j S is not zero (call {} block {})".format(k, j)
            got[j].append(oc[j, :, :n * S])
            done[j] += n
    tc = tail.cpu()
    for j, s in enumerate(sel):
        close(torch.cat(got[j] + [tc[s]], -1), ref[j], 2e-5, "decoder output of block {}".format(j))
    rest = _others(Bs, sel)
    if keep:
        same_bits(tc[rest], tail0[rest], "tail")
        same_bits(tail_next.cpu()[rest], torch.full((len(rest), n_src, keep), NAN), "tail_next")
    assert torch.equal(frames.cpu()[sel], torch.tensor(totals, dtype=torch.int64))


def case_advance_rag(Bs, sel, keep, n_src, call):
    """the counters move by n_j and both copies are made for the named slots; nothing else changes, the second buffers not at all"""
    A, tl = len(sel), n_src * keep
    _, offs, _, _, cap = _layout(call, 1)
    frames0 = torch.arange(1000, 1000 + Bs, dtype=torch.int64)
    host = [frames0, rnd(Bs, keep) + 3, rnd(Bs, keep) - 3, rnd(Bs, tl) + 3, rnd(Bs, tl) - 3]
    frames, carry, carry_next, tail, tail_next = [OG.to_device(t) for t in host]
    OG.HIP.online_advance_rag(frames, carry if keep else None, carry_next if keep else None, keep, tail if tl else None, tail_next if tl else None, tl,
                              A, cap, _slots(sel), _offs(offs))
    OG.device_sync()
    rest = _others(Bs, sel)
    fc = frames.cpu()
    assert torch.equal(fc[sel], frames0[sel] + torch.tensor(call, dtype=torch.int64)) and torch.equal(fc[rest], frames0[rest])
    for cur, nxt, cur0, nxt0, what in ((carry, carry_next, host[1], host[2], "carry"), (tail, tail_next, host[3], host[4], "tail")):
        same_bits(cur.cpu()[sel], nxt0[sel], what + " of the selected slots")
        same_bits(cur.cpu()[rest], cur0[rest], what)
        same_bits(nxt.cpu(), nxt0, what + "_next")


CASES = [
    # an unordered selection with gaps and three lengths per call; a block wider than a workgroup next to a one-frame block with a slot index
    # beyond 255; L == S (no carry, no tail); totals of exactly 128 and of 129 columns (no pad column, 127 of them)
    ("case_encoder_rag", [(5, [4, 0, 2], 32, 20, 10, [[7, 1, 12], [1, 1, 1], [2, 40, 3]], 1), (257, [256, 0], 16, 16, 8, [[1, 300], [300, 1]], 1),
                          (2, [1], 16, 16, 16, [[3], [1]], 0), (3, [2, 0, 1], 16, 16, 8, [[100, 27, 1]], 0), (3, [2, 0, 1], 16, 16, 8, [[100, 28, 1]], 0)]),
    # across the 32-frame tile of the cLN, with and without PReLU
    ("case_cln_rag", [(5, [4, 0, 2], 48, [[7, 1, 33], [31, 32, 1], [1, 1, 64]], False), (5, [4, 0, 2], 48, [[7, 1, 33], [31, 32, 1], [1, 1, 64]], True),
                      (257, [256, 0], 16, [[1, 2], [40, 1]], True)]),
    # a history of 256 frames that is longer than one block and shorter than the other in the same launch
    ("case_depthwise_rag", [(3, [2, 1], 16, [[1, 300], [2, 1], [1, 1]], 3, 128), (5, [4, 0, 2], 32, [[5, 1, 9], [30, 2, 1]], 5, 4)]),
    ("case_decoder_rag", [(5, [4, 0, 2], 3, 32, 20, 10, [[7, 1, 12], [1, 2, 1]]), (257, [256, 0], 2, 16, 16, 8, [[1, 40], [40, 1]]),
                          (2, [1], 2, 16, 8, 8, [[2], [1]])]),
    ("case_advance_rag", [(5, [4, 0, 2], 8, 2, [3, 1, 7]), (257, [256, 0], 10, 3, [1, 40]), (2, [1], 0, 3, [5])]),
]


@pytest.mark.parametrize("name,params", CASES, ids=[c[0][5:] for c in CASES])
def test_online_rag_kernels_against_the_restatement(name, params):
    for p in params:
        globals()[name](*p)


def check_equal_lengths_are_the_sel_call():
    """all n_j = n: a call through the _rag entry points and the same call through _sel are bitwise equal in outputs and state (depthwise, cLN)"""
    Bs, sel, C, n, P, d = 5, [4, 0, 2], 16, 5, 3, 2
    A, ldt = len(sel), 128
    offs = _offs([j * n for j in range(A + 1)])
    x, w, b = rnd(C, ldt), rnd(C, P), rnd(C)
    x[:, A * n:] = 0
    slots = _slots(sel)
    xd, wd, bd = OG.to_device(x), OG.to_device(w), OG.to_device(b)
    ring = rnd(Bs, C * (P - 1) * d)
    r1, r2 = OG.to_device(ring), OG.to_device(ring)
    y1, y2 = OG.to_device(torch.full((C, ldt), NAN)), OG.to_device(torch.full((C, ldt), NAN))
    OG.HIP.online_depthwise_fwd_sel(xd, wd, bd, r1.view(-1), ring.shape[1], y1, A, C, n, ldt, P, d, slots)
    OG.HIP.online_depthwise_fwd_rag(xd, wd, bd, r2.view(-1), ring.shape[1], y2, A, C, n, ldt, P, d, slots, offs)
    OG.device_sync()
    assert torch.equal(y1.cpu(), y2.cpu()) and torch.equal(r1.cpu(), r2.cpu()), "depthwise: equal lengths differ from the _sel call"
    sums = torch.randn(Bs, 2, generator=OG.G, dtype=torch.float64)
    frames = OG.to_device(torch.tensor([3, 0, 9, 1, 700]))
    g, be, al = OG.to_device(rnd(C)), OG.to_device(rnd(C)), OG.to_device(torch.tensor([0.2]))
    for alpha in (None, al):
        s1, s2 = OG.to_device(sums), OG.to_device(sums)
        y1, y2 = OG.to_device(torch.full((C, ldt), NAN)), OG.to_device(torch.full((C, ldt), NAN))
        OG.HIP.online_cln_fwd_sel(xd, alpha, g, be, y1, s1.view(-1), 2, frames, A, C, n, ldt, 1e-8, slots)
        OG.HIP.online_cln_fwd_rag(xd, alpha, g, be, y2, s2.view(-1), 2, frames, A, C, n, ldt, 1e-8, slots, offs)
        OG.device_sync()
        assert torch.equal(y1.cpu(), y2.cpu()) and torch.equal(s1.cpu(), s2.cpu()), "cln: equal lengths differ from the _sel call"


def test_equal_lengths_through_rag_are_bitwise_the_sel_call():
    check_equal_lengths_are_the_sel_call()


# ------------------------------------------------------------------------------------------------------ the fixture on ragged clocks
HOPS = [3, 1, 4, 2]
JOB_SLOTS = [4, 0, 2, 3, 1]


def run_ragged_schedule(sep, x, isolation=False):
    """x (R, 1, T): five jobs, job k streams fixture row k % R in slot JOB_SLOTS[k].  At tick t job k offers min(HOPS[(t + 2 k) % 4], hops left)
    hops and sits out the ticks with (t + k) % (k + 2) == 0; the jobs of a tick go into ONE call of width 4 S (the recorded width) whose index
    order is ascending on even ticks and descending on odd ones, each row NaN beyond its length.  A job that reaches its end is flushed on its
    own while the others go on.  -> ([(row, output (n_src, T + L - S))] in the order the jobs ended, ticks, the set of (A, total hops) of the
    calls).  isolation: after every call (and flush) the unselected slots' slices of the five state tensors must be what they were."""
    S, R, total = sep.S, x.shape[0], x.shape[-1] // sep.S
    W = 4 * S
    jobs = [dict(k=k, row=k % R, slot=JOB_SLOTS[k], done=0, out=[]) for k in range(5)]
    finished, shapes, t = [], set(), 0

    def snapshot():
        return [getattr(sep, a).clone() for a in STATE]

    def untouched(before, touched, what):
        rest = [s for s in range(sep.num_streams) if s not in touched]
        for a, b in zip(STATE, before):
            assert torch.equal(getattr(sep, a)[rest], b[rest]), "{}: {} of an unselected slot changed".format(what, a)

    while jobs:
        live = [j for j in jobs if (t + j["k"]) % (j["k"] + 2) != 0]
        live.sort(key=lambda j: j["slot"], reverse=bool(t % 2))
        if live:
            idx = [j["slot"] for j in live]
            hops = [min(HOPS[(t + 2 * j["k"]) % 4], total - j["done"]) for j in live]
            chunk = torch.full((len(live), 1, W), NAN, dtype=x.dtype, device=x.device)
            for r, (j, h) in enumerate(zip(live, hops)):
                chunk[r, :, :h * S] = x[j["row"], :, j["done"] * S:(j["done"] + h) * S]
            before = snapshot() if isolation else None
            y = sep(chunk, streams=idx, lengths=[h * S for h in hops])
            assert y.shape == (len(live), sep.n_src, W)
            shapes.add((len(live), sum(hops)))
            if isolation:
                untouched(before, idx, "sep(chunk, streams={}, lengths=...)".format(idx))
            for r, (j, h) in enumerate(zip(live, hops)):
                assert not y[r, :, h * S:].any(), "a row of the result is not zero beyond its length"
                j["out"].append(y[r, :, :h * S])
                j["done"] += h
        for j in [j for j in jobs if j["done"] == total]:
            before = snapshot() if isolation else None
            j["out"].append(sep.flush([j["slot"]])[0])
            if isolation:
                untouched(before, [j["slot"]], "flush([{}])".format(j["slot"]))
            jobs.remove(j)
            finished.append((j["row"], torch.cat(j["out"], -1)))
        t += 1
        assert t < 5000, "the schedule does not terminate"
    return finished, t, shapes


@pytest.mark.parametrize("arith", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("name", ["causal16", "causal16_p5"])
def test_fixture_on_ragged_clocks_matches_the_reference_on_the_device(name, arith):
    """run_ragged_schedule in 5 slots: every job within 1e-3 of its fixture row (the bar of the all-streams test), recorded per (A, ldt) with at
    least one recording replayed, and bitwise what the eager launches (record=False) give on the same schedule"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_causal_online.npz"))
    prev = sepkernels.set_gemm_arith(arith)
    try:
        model, cfg = OG._fixture_model(name)
        x = torch.from_numpy(g[name + "/input"])[..., cfg["kernel_size"] - cfg["stride"]:].cuda()
        ref = torch.from_numpy(g[name + "/output_f64"])
        runs = []
        for record in (True, False):
            sep = model.online_separator(num_streams=5, chunk_size=4 * cfg["stride"], record=record)
            done, _, shapes = run_ragged_schedule(sep, x)
            assert len(done) == 5 and len(shapes) > 5
            if record:
                assert sum(sep.replays.values()) >= 1 and all(isinstance(k, tuple) and k[1] % 128 == 0 for k in sep.replays)
            else:
                assert not sep.replays and not sep._sub_seqs
            runs.append(done)
        for (row, est), (row_e, est_e) in zip(*runs):
            close(est, ref[row], 1e-3, "{} {} job of row {}".format(name, arith, row))
            assert row == row_e and torch.equal(est, est_e), "recorded ragged steps differ from eager launches"
    finally:
        sepkernels.set_gemm_arith(prev)


def test_paper_size_model_with_a_different_half_of_64_slots_and_different_lengths_in_every_call():
    """N512 L16 S8 H512 B128 Sc128 P3 X8 R3 in 64 slots, chunk_size 80, 20 calls, each for a fresh half of the slots in a fresh order, every
    stream bringing 1 .. 10 hops: every slot's pieces and its flush within 1e-4 of the offline staged forward on exactly what that slot received
    (the bar of the all-streams paper-size test: same product kernels and weight bound, only the column a frame sits in differs)"""
    from models.conv_tasnet import ConvTasNet
    torch.manual_seed(0)
    model = ConvTasNet(**OG.PAPER).cuda()
    Bs, L, S, calls, cap = 64, 16, 8, 20, 10
    g = torch.Generator().manual_seed(12)
    x = 0.1 * torch.randn(Bs, 1, calls * cap * S, generator=g).cuda()
    sep = model.online_separator(num_streams=Bs, chunk_size=cap * S)
    done, outs = [0] * Bs, [[] for _ in range(Bs)]
    for _ in range(calls):
        idx = torch.randperm(Bs, generator=g)[:Bs // 2].tolist()
        hops = torch.randint(1, cap + 1, (len(idx),), generator=g).tolist()
        chunk = torch.full((len(idx), 1, cap * S), NAN, device="cuda")
        for r, (s, h) in enumerate(zip(idx, hops)):
            chunk[r, :, :h * S] = x[s, :, done[s] * S:(done[s] + h) * S]
        y = sep(chunk, streams=idx, lengths=torch.tensor(hops) * S)
        for r, (s, h) in enumerate(zip(idx, hops)):
            outs[s].append(y[r, :, :h * S])
            done[s] += h
    assert torch.equal(sep.frames.cpu(), torch.tensor(done))
    tails = sep.flush(list(range(Bs)))
    assert not sep.frames.any() and not sep.tail.any()
    for count in sorted(set(done) - {0}):
        group = [s for s in range(Bs) if done[s] == count]
        with torch.no_grad():
            ref = model(torch.nn.functional.pad(x[group][..., :count * S], (L - S, 0)))
        est = torch.stack([torch.cat(outs[s] + [tails[s]], -1) for s in group])
        close(est, ref.cpu(), 1e-4, "slots that received {} hops".format(count))
