"""GPU: the causal Conv-TasNet WITHOUT separable convolutions (ConvTasNet(causal=True, separable=False): two full P-tap dilated convolutions per
TCN layer, reference src/models/tdcn.py:100-147) on this library's kernels -- the dilated unfold over the taps and its adjoint
(csrc/causal.hip: sep_unfold_dilated, sep_fold_dilated), the online form (csrc/online.hip: sep_online_unfold_fwd, _sel, _rag), the staged
forward / backward, the recorded training step and the online separator.

The kernel cases (`case_*`, listed in CASES) check the entry points against torch written from their contracts in include/sepkernels.h;
tests/test_dense_tcn_cpu.py runs the same functions on the host simulation of the kernel sources (it swaps HIP, to_device, device_sync and
device_name), and reuses check_recorded_equals_live and run_online_schedule.  The model tests run the unmodified reference's fixtures
tests/golden/convtasnet_causal16_dense*.npz (tools/make_dense_tcn_golden.py; configurations in tests/dense_tcn_configs.py)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sepkernels
from dense_tcn_configs import CONFIGS, NAMES

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
G = torch.Generator().manual_seed(1207)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def to_device(t):
    return t.cuda()


def device_sync():
    torch.cuda.synchronize()


def device_name():
    return "cuda"


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, generator=G) * scale).float()


def _round_up(a, b):
    return (a + b - 1) // b * b


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------------ the contracts, restated
def ref_unfold(x, T, P, dil, pad):
    """x (B, C, ldt) -> cols (B, C P, ldt): cols[b][c P + p][t] = x[b][c][t + p dil - pad] where t < T and 0 <= t + p dil - pad < T, zero
    elsewhere (include/sepkernels.h).  Copies in the dtype of x; what x holds in [T, ldt) is never looked at."""
    B, C, ldt = x.shape
    cols = torch.zeros(B, C, P, ldt, dtype=x.dtype)
    for p in range(P):
        sh = p * dil - pad
        lo, hi = max(0, -sh), min(T, T - sh)
        if hi > lo:
            cols[:, :, p, lo:hi] = x[:, :, lo + sh:hi + sh]
    return cols.reshape(B, C * P, ldt)


def ref_fold(dcols, T, P, dil, pad):
    """dcols (B, C P, ldt) -> (dx, sum of |terms|), both (B, C, ldt) in fp64: dx[b][c][u] = sum_p dcols[b][c P + p][u - p dil + pad] over the
    p whose column lies in [0, T), for u < T; zero beyond"""
    B, CP, ldt = dcols.shape
    d = dcols.double().reshape(B, CP // P, P, ldt)
    dx, mag = torch.zeros(B, CP // P, ldt, dtype=torch.float64), torch.zeros(B, CP // P, ldt, dtype=torch.float64)
    for p in range(P):
        sh = p * dil - pad                              # column i = u - sh
        lo, hi = max(0, sh), min(T, T + sh)
        if hi > lo:
            dx[:, :, lo:hi] += d[:, :, p, lo - sh:hi - sh]
            mag[:, :, lo:hi] += d[:, :, p, lo - sh:hi - sh].abs()
    return dx, mag


# ------------------------------------------------------------------------------------------------------ offline kernel cases
def case_unfold_fold(B, C, T, ldt, P, dil, pad):
    """sep_unfold_dilated is torch.equal to the restatement (it only copies); sep_fold_dilated is within P 2^-24 sum_p |term| per element (P - 1
    fp32 additions in ascending p); every element of both outputs is written, the pad columns as zero, with NaN in the pad columns of both
    inputs; and the two are adjoint: <dcols, unfold(x)> == <fold(dcols), x> in fp64 accumulation to 1e-6 relative."""
    xc = rnd(B, C, ldt)
    xc[..., T:] = NAN
    dc = rnd(B, C * P, ldt)
    dc[..., T:] = NAN
    x, dcols = to_device(xc), to_device(dc)
    f32 = dict(device=device_name(), dtype=torch.float32)
    cols, dx = torch.full((B, C * P, ldt), NAN, **f32), torch.full((B, C, ldt), NAN, **f32)
    HIP.unfold_dilated(x, cols, B, C, T, ldt, P, dil, pad)
    HIP.fold_dilated(dcols, dx, B, C, T, ldt, P, dil, pad)
    device_sync()
    cols, dx = cols.cpu(), dx.cpu()
    want = ref_unfold(xc, T, P, dil, pad)
    assert torch.isfinite(cols).all(), "unfold: unwritten or NaN output"
    assert torch.equal(cols, want), "unfold differs from the restatement at {} elements".format(int((cols != want).sum()))
    ref, mag = ref_fold(dc, T, P, dil, pad)
    assert torch.isfinite(dx).all(), "fold: unwritten or NaN output"
    assert (dx[..., T:] == 0).all(), "fold: columns beyond T"
    excess = ((dx.double() - ref).abs() - P * 2.0 ** -24 * mag).max().item()
    assert excess <= 0, "fold: {:.3e} above P 2^-24 sum |term|".format(excess)
    lhs = (dc.double()[..., :T] * cols.double()[..., :T]).sum().item()
    rhs = (dx.double()[..., :T] * xc.double()[..., :T]).sum().item()
    print("unfold/fold", (B, C, T, ldt, P, dil, pad), "fold err / bound", ((dx.double() - ref).abs() / (P * 2.0 ** -24 * mag + 1e-300)).max().item(),
          "adjoint", lhs, rhs)
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs)), (lhs, rhs)


# ------------------------------------------------------------------------------------------------------ online kernel cases
def _stream_cols(parts, ldt, fill):
    """[(C, n_j)] -> compact (C, ldt) columns, `fill` beyond the last block"""
    m = torch.cat(parts, 1)
    return torch.cat([m, torch.full((m.shape[0], ldt - m.shape[1]), fill, dtype=m.dtype)], 1)


def _online_unfold(form, xd, rings, off, stride, y, A, C, n, ldt, P, d, slots, offs):
    if form == "plain":
        HIP.online_unfold_fwd(xd, rings.view(-1)[off:], stride, y, A, C, n, ldt, P, d)
    elif form == "sel":
        HIP.online_unfold_fwd_sel(xd, rings.view(-1)[off:], stride, y, A, C, n, ldt, P, d, slots)
    else:
        HIP.online_unfold_fwd_rag(xd, rings.view(-1)[off:], stride, y, A, C, n, ldt, P, d, slots, offs)


def case_online_unfold(form, Bs, sel, C, plan, P, d):
    """Consecutive calls against ONE offline unfold of every stream's concatenated frames (causal: pad = (P - 1) d).  plan: a list of calls, a
    call a list of frames per selected stream (form "plain" / "sel": all equal; "rag": any).  The layer's ring sits inside a wider per-stream
    buffer (offset, stride) as OnlineSeparator keeps it; unselected slots hold sentinels that must come back bit for bit; the input's dead
    columns hold NaN, the output is pre-filled with NaN and its dead columns must come back as zero; copies only, so everything is exact."""
    A, D = len(sel), (P - 1) * d
    assert form != "plain" or sel == list(range(Bs))
    totals = [sum(call[j] for call in plan) for j in range(A)]
    x = [rnd(C, t) for t in totals]
    ref = [ref_unfold(xj.unsqueeze(0), xj.shape[1], P, d, D)[0] for xj in x]          # (C P, total_j) each
    off, stride = 5, C * D + 9
    rings0 = rnd(Bs, stride) + 3.0
    rings0[sel] = 0.0
    rings = to_device(rings0)
    slots = to_device(torch.tensor(sel, dtype=torch.int32))
    done = [0] * A
    for k, call in enumerate(plan):
        offs = [0]
        for n in call:
            offs.append(offs[-1] + n)
        used, ldt = offs[-1], _round_up(offs[-1], 128)
        cap = max(call) + (k % 2 if form == "rag" else 0)
        xd = to_device(_stream_cols([x[j][:, done[j]:done[j] + n] for j, n in enumerate(call)], ldt, NAN))
        y = to_device(torch.full((C * P, ldt), NAN))
        _online_unfold(form, xd, rings, off, stride, y, A, C, cap, ldt, P, d, slots, to_device(torch.tensor(offs, dtype=torch.int32)))
        device_sync()
        yc = y.cpu()
        assert torch.equal(yc[:, used:], torch.zeros(C * P, ldt - used)), "online unfold: dead columns not zero"
        for j, n in enumerate(call):
            assert torch.equal(yc[:, offs[j]:offs[j + 1]], ref[j][:, done[j]:done[j] + n]), "online unfold: call {} block {}".format(k, j)
            done[j] += n
    r = rings.cpu()
    rest = [s for s in range(Bs) if s not in sel]
    hist = torch.stack([F.pad(xj, (D, 0))[:, xj.shape[1]:] for xj in x]) if D else torch.zeros(A, C, 0)
    assert torch.equal(r[sel][:, off:off + C * D].reshape(A, C, D), hist), "online unfold: ring"
    assert torch.equal(r[sel][:, :off], torch.zeros(A, off)) and torch.equal(r[sel][:, off + C * D:], torch.zeros(A, stride - off - C * D))
    assert torch.equal(_bits(r[rest]), _bits(rings0[rest])), "online unfold: an entry of an unselected slot changed"


def case_online_unfold_rag_is_sel(Bs, sel, C, n, calls, P, d):
    """a _rag call in which every stream brings n frames is bitwise the _sel call: the unfolded rows and the rings"""
    A, D = len(sel), (P - 1) * d
    stride = C * D + 3
    ldt = _round_up(A * n, 128)
    slots = to_device(torch.tensor(sel, dtype=torch.int32))
    offs = to_device(torch.arange(0, (A + 1) * n, n, dtype=torch.int32))
    ring0 = rnd(Bs, stride)
    ra, rb = to_device(ring0), to_device(ring0)
    for _ in range(calls):
        xc = rnd(C, ldt)
        xc[:, A * n:] = NAN
        xd = to_device(xc)
        ya, yb = to_device(torch.full((C * P, ldt), NAN)), to_device(torch.full((C * P, ldt), NAN))
        HIP.online_unfold_fwd_sel(xd, ra.view(-1), stride, ya, A, C, n, ldt, P, d, slots)
        HIP.online_unfold_fwd_rag(xd, rb.view(-1), stride, yb, A, C, n, ldt, P, d, slots, offs)
        device_sync()
        assert torch.isfinite(ya.cpu()).all() and torch.equal(_bits(ya), _bits(yb))
    assert torch.equal(_bits(ra), _bits(rb)) and not torch.equal(_bits(ra), _bits(ring0))


# (function, argument tuples): what the host simulation runs too
UNFOLD_SHAPES = [(2, 16, 203, 256, 3, 1, 2),
                 (1, 32, 130, 256, 3, 64, 128),        # a history nearly as long as the signal
                 (2, 16, 37, 128, 5, 16, 64),          # (P - 1) d > T
                 (1, 48, 1030, 1152, 3, 4, 8),
                 (1, 16, 100, 128, 2, 8, 4)]           # pad in the middle: taps reaching past T
CASES = [
    ("case_unfold_fold", UNFOLD_SHAPES),
    ("case_online_unfold", [("plain", 3, [0, 1, 2], 16, [[5] * 3, [5] * 3], 3, 4),              # n below (P - 1) d = 8 ...
                            ("plain", 2, [0, 1], 16, [[11] * 2, [11] * 2, [3] * 2], 3, 4),       # ... and above it, then below
                            ("plain", 2, [0, 1], 32, [[70] * 2, [70] * 2], 5, 16),               # more than one workgroup pass over P n, two column tiles
                            ("sel", 5, [3, 0], 16, [[6] * 2, [6] * 2], 3, 8),
                            ("sel", 4, [2], 16, [[130], [130]], 2, 1),
                            ("rag", 5, [4, 1, 2], 16, [[1, 7, 3], [1, 7, 3], [6, 1, 20]], 3, 2),   # n_j below and above (P - 1) d = 4 in one launch
                            ("rag", 3, [2, 0, 1], 16, [[1, 7, 3], [40, 2, 90]], 5, 8)]),
    ("case_online_unfold_rag_is_sel", [(5, [3, 0, 4], 16, 6, 2, 3, 4), (2, [1, 0], 32, 70, 2, 5, 1)]),
]


@pytest.mark.parametrize("B,C,T,ldt,P,dil,pad", UNFOLD_SHAPES)
def test_unfold_and_fold_against_the_restatement(B, C, T, ldt, P, dil, pad):
    case_unfold_fold(B, C, T, ldt, P, dil, pad)


@pytest.mark.parametrize("name,params", CASES[1:], ids=[c[0] for c in CASES[1:]])
def test_online_unfold_against_the_offline_unfold(name, params):
    for p in params:
        globals()[name](*p)


# ------------------------------------------------------------------------------------------------------ the models on the fixtures
def load_fixture(name):
    """-> dict of the fixture's arrays; a fixture too large for one committed file keeps its grad/* keys in convtasnet_<name>_grads.npz"""
    base = os.path.join(ROOT, "tests", "golden", "convtasnet_{}".format(name))
    g = dict(np.load(base + ".npz"))
    if os.path.exists(base + "_grads.npz"):
        g.update(np.load(base + "_grads.npz"))
    return g


def fixture_model(name, g=None):
    from models.conv_tasnet import ConvTasNet
    g = load_fixture(name) if g is None else g
    model = ConvTasNet(**CONFIGS[name])
    model.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in g.items() if k.startswith("param/")})
    return model


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("name", NAMES)
def test_staged_dense_path_on_the_reference_fixtures(name):
    """forward + PIT1d(NegSISDR) + backward through the model's autograd path on the device against the unmodified reference: the model is
    staged (not fused, no reason); output and loss within 1e-3 of their own scale, the permutation equal, EVERY gradient tensor within 1e-3 of
    its own scale (the bar of test_gpu_model.py for the staged family, the slopes included here); one sep_unfold_dilated and one
    sep_fold_dilated per layer, no depthwise call."""
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    g = load_fixture(name)
    model = fixture_model(name, g)
    assert model.staged and not model.fused and model.staged_reason is None
    model.cuda()
    cfg = CONFIGS[name]
    if cfg["sep_bottleneck_channels"] % 128 == 0:           # the pairs adjacent in the flat buffer: the joint [Wo; Ws] product
        layer = model.separator.tdcn.net[0].net[0]
        assert layer.output_conv1d.weight.data_ptr() + 4 * layer.output_conv1d.weight.numel() == layer.skip_conv1d.weight.data_ptr()
        assert layer.output_conv1d.bias.data_ptr() + 4 * layer.output_conv1d.bias.numel() == layer.skip_conv1d.bias.data_ptr()
    calls = []
    K = sepkernels.backend()
    saved = {}
    for fn in ("unfold_dilated", "fold_dilated", "depthwise_fwd", "depthwise_cln_fwd", "pw_gemm"):
        saved[fn] = getattr(K, fn)
        setattr(K, fn, (lambda o, n: (lambda *a, **k: (calls.append((n, k.get("m_split", 0))), o(*a, **k))[1]))(saved[fn], fn))
    try:
        mixture, sources = torch.from_numpy(g["mixture"]).cuda(), torch.from_numpy(g["sources"]).cuda()
        est, latent = model.extract_latent(mixture)
        ref = torch.from_numpy(g["output_f64"])
        assert est.shape == ref.shape
        print(name, "output rel", _rel(est, ref))
        assert _rel(est, ref) <= 1e-3
        assert abs(latent.double().sum().item() - float(g["latent_f64_sum"])) <= 1e-3 * float(g["latent_f64_abs_sum"])
        loss, pattern = PIT1d(NegSISDR(), n_sources=cfg["n_sources"])(est, sources)
        print(name, "loss", loss.item(), float(g["loss_f64"]))
        assert abs(loss.item() - float(g["loss_f64"])) <= 1e-3 * abs(float(g["loss_f64"]))
        assert np.array_equal(pattern.cpu().numpy(), g["pattern"])
        loss.backward()
        torch.cuda.synchronize()
    finally:
        for fn, o in saved.items():
            delattr(K, fn)
    nl = cfg["sep_num_blocks"] * cfg["sep_num_layers"]
    names = [c[0] for c in calls]
    assert names.count("unfold_dilated") == nl and names.count("fold_dilated") == nl
    assert names.count("depthwise_fwd") == 0 and names.count("depthwise_cln_fwd") == 0
    joint = sum(1 for n, ms in calls if n == "pw_gemm" and ms)
    assert joint == (nl - 1 if cfg["sep_bottleneck_channels"] % 128 == 0 else 0)
    worst = ("", 0.0)
    for k, q in model.named_parameters():
        r = torch.from_numpy(g["grad/" + k]).double()
        rel = (q.grad.double().cpu() - r).abs().max().item() / (r.abs().max().item() + 1e-30)
        worst = max(worst, (k, rel), key=lambda kv: kv[1])
        assert np.isfinite(rel) and rel <= 1e-3, "{}: {:.3e}".format(k, rel)
    print(name, "worst gradient", worst)


def check_recorded_equals_live(name, wrap=None, T=1203, B=2):
    """FusedTrainStep on the fixture's model, three batches, a learning-rate change before the last: (a) one record() and two replays (ONE
    sep_run_sequence call each) against (b) the driver run live every step (a fresh record() per step on one step object).  Losses and
    parameters are equal to the last bit: same entry points, same arguments, same order -- the claim tests/test_causal_recorded_cpu.py makes
    for the separable family.  wrap: what to install as the backend (the host simulation of the CPU tier), None on the device."""
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    from sepkernels.train import FusedTrainStep
    n_src = CONFIGS[name]["n_sources"]
    gen = torch.Generator().manual_seed(5)
    batches = [0.1 * torch.randn(B, n_src, T, generator=gen) for _ in range(3)]
    old = sepkernels._set_backend_for_tests(wrap) if wrap is not None else None
    runs = {}
    try:
        for mode in ("replay", "live"):
            model = fixture_model(name)
            if wrap is None:
                model.cuda()
            step = FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=n_src), lr=1e-3, max_norm=5.0)
            assert model.staged and step.recordable() is None
            losses = []
            for i, src in enumerate(batches):
                src = to_device(src)
                mix = src.sum(1, keepdim=True).contiguous()
                if i == 2:
                    step.lr = 5e-4
                if mode == "live" or i == 0:
                    losses.append(float(step.record(mix, src)))
                    if mode == "replay":
                        names = step._seq.names()
                        assert names[0] == "sep_absmax" and names[-1] == "sep_adam_step_dev"
                        for want in ("sep_unfold_dilated", "sep_fold_dilated", "sep_cln_fwd", "sep_cln_bwd", "sep_pw_gemm", "sep_pw_wgrad", "sep_pit_finish"):
                            assert want in names, want
                        nl = CONFIGS[name]["sep_num_blocks"] * CONFIGS[name]["sep_num_layers"]
                        assert names.count("sep_unfold_dilated") == nl and names.count("sep_fold_dilated") == nl
                        assert not any(n.startswith("sep_depthwise") for n in names)
                else:
                    before = step._seq
                    losses.append(float(step(mix, src)))
                    assert step._seq is before and before is not None
            device_sync()
            assert step.step_count == 3 and int(step._step_dev.item()) == 3
            runs[mode] = (losses, model.flat_parameters().detach().cpu().clone())
    finally:
        if wrap is not None:
            sepkernels._set_backend_for_tests(old)
    (la, pa), (lb, pb) = runs["replay"], runs["live"]
    print(name, "replay", la, "live", lb)
    assert all(np.isfinite(v) for v in la) and la[0] != la[-1]
    assert la == lb and torch.equal(pa, pb)


@pytest.mark.parametrize("name", NAMES)
def test_recorded_dense_step_equals_the_live_driver_bitwise(name):
    check_recorded_equals_live(name)


# ------------------------------------------------------------------------------------------------------ online separation
def run_online_schedule(sep, x, hops=4):
    """x (3, 1, T), T a multiple of the stride: streams 0 and 2 take part in every call while they have audio, stream 1 only in every other
    call; a call offers `hops` hops to each participant (less at a stream's end), except call 2, where the streams bring [hops, 2, 3] hops.
    A call in which all three bring the same number is the plain all-streams call, one in which the participants bring the same number a
    subset call (streams=), any other a ragged call (streams= and lengths=).  A stream that reaches its end is flushed on its own.
    -> ([(n_src, T + L - S)] per stream, the kinds of call made in order)"""
    S, T = sep.S, x.shape[-1]
    total = T // S
    pos, pieces, kinds = [0, 0, 0], [[], [], []], []
    tick = 0
    while any(p < total for p in pos):
        who = [s for s in range(3) if pos[s] < total and (s != 1 or tick % 2 == 0 or (pos[0] >= total and pos[2] >= total))]
        want = {s: min(hops, total - pos[s]) for s in who}
        if tick == 2:
            want = {s: min(h, total - pos[s]) for s, h in zip(who, (hops, 2, 3))}
        tick += 1
        if not who:
            continue
        counts = [want[s] for s in who]
        W = max(counts)
        chunk = torch.zeros(len(who), 1, W * S, device=x.device, dtype=x.dtype)
        for j, s in enumerate(who):
            chunk[j, 0, :counts[j] * S] = x[s, 0, pos[s] * S:(pos[s] + counts[j]) * S]
        if len(set(counts)) > 1:
            y = sep(chunk, streams=who, lengths=[c * S for c in counts])
            kinds.append("ragged")
        elif len(who) == 3:
            y = sep(chunk)
            kinds.append("uniform")
        else:
            y = sep(chunk, streams=who)
            kinds.append("subset")
        for j, s in enumerate(who):
            pieces[s].append(y[j, :, :counts[j] * S].clone())
            assert not y[j, :, counts[j] * S:].any()
            pos[s] += counts[j]
            if pos[s] == total:
                pieces[s].append(sep.flush([s])[0])
    return [torch.cat(p, -1) for p in pieces], kinds


def test_dense_model_streams_like_its_offline_forward():
    """causal16_dense, 3 streams of 40 hops in chunks of 4 hops, stream 1 in every other call through streams=, one ragged call, flush per
    stream: every stream equals model(F.pad(x_s, (L - S, 0))) within 1e-3 of its own scale, and the run with recorded chunk steps equals the
    run that launches every chunk eagerly bit for bit"""
    name = "causal16_dense"
    model = fixture_model(name).cuda()
    L, S = CONFIGS[name]["kernel_size"], CONFIGS[name]["stride"]
    x = (0.1 * torch.randn(3, 1, 40 * S, generator=torch.Generator().manual_seed(3))).cuda()
    with torch.no_grad():
        ref = model(F.pad(x, (L - S, 0)))
    outs = {}
    for record in (True, False):
        sep = model.online_separator(num_streams=3, chunk_size=4 * S, record=record)
        assert sep.record == record and sep.dense and sep.n_norms == 1 + len(sep.layers)
        est, kinds = run_online_schedule(sep, x)
        assert {"uniform", "subset", "ragged"} <= set(kinds), kinds
        if record:
            assert sep._seq is not None and len(sep._sub_seqs) >= 1
            assert "sep_online_unfold_fwd" in sep._seq.names() and "sep_online_depthwise_fwd" not in sep._seq.names()
        for s in range(3):
            assert est[s].shape == ref[s].shape
            print("stream", s, "rel", _rel(est[s], ref[s]))
            assert _rel(est[s], ref[s]) <= 1e-3
        for a in ("frames", "carry", "sums", "rings", "tail"):
            assert not getattr(sep, a).any()
        outs[record] = est
    for a, b in zip(outs[True], outs[False]):
        assert torch.equal(a, b)
