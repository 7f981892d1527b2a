"""GPU: the causal layer's first norm folded into its depthwise kernels (csrc/causal.hip: sep_cln_stats, sep_depthwise_cln_fwd,
sep_depthwise_cln_bwd_weight) and the recorded causal training step (sepkernels/causal.py, sepkernels.train.FusedTrainStep).

The kernel cases (`case_*`, listed in CASES) check the three entry points against torch fp64 written from their contract in
include/sepkernels.h; tests/test_causal_recorded_cpu.py runs the same functions on the host simulation of the kernel sources (it swaps
HIP, to_device, device_sync and device_name).  The model tests run the reference's causal fixtures through the folded staged path and a
paper-size causal model through ten recorded steps against ten eager ones."""
import os

import numpy as np
import pytest
import torch

import sepkernels
from oracle.make_golden import CONFIGS, STAGED

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
G = torch.Generator().manual_seed(77)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def to_device(t):
    return t.cuda()


def device_sync():
    torch.cuda.synchronize()


def device_name():
    return "cuda"


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, generator=G) * scale).float()


def _ws(B, C, T, ldt):
    return torch.empty((HIP.cln_ws_bytes(B, C, T, ldt) + 7) // 8, device=device_name(), dtype=torch.float64)


def _input(B, C, T, ldt):
    x = torch.zeros(B, C, ldt)
    x[..., :T] = rnd(B, C, T) * torch.linspace(0.3, 2.5, T) + 0.1          # non-stationary, non-zero mean
    return x


# ------------------------------------------------------------------------------------------------------ sep_cln_stats
def case_cln_stats(B, C, T, a):
    """mean / rstd of sep_cln_stats are those of sep_cln_fwd bit for bit (chain form for C <= 512, three launches above), with and without
    the PReLU in front; nothing else is written."""
    ldt = (T + 127) // 128 * 128
    x = to_device(_input(B, C, T, ldt))
    alpha = to_device(torch.tensor([a])) if a is not None else None
    gamma, beta = to_device(rnd(C) + 1), to_device(rnd(C))
    f32 = dict(device=device_name(), dtype=torch.float32)
    y = torch.empty(B, C, ldt, **f32)
    m0, r0 = torch.zeros(B, ldt, **f32), torch.zeros(B, ldt, **f32)
    m1, r1 = torch.zeros(B, ldt, **f32), torch.zeros(B, ldt, **f32)
    HIP.cln_fwd(x, gamma, beta, y, m0, r0, _ws(B, C, T, ldt), B, C, T, ldt, 1e-12, alpha=alpha)
    HIP.cln_stats(x, m1, r1, _ws(B, C, T, ldt), B, C, T, ldt, 1e-12, alpha=alpha)
    device_sync()
    assert torch.isfinite(m1[:, :T]).all() and torch.isfinite(r1[:, :T]).all() and (r1[:, :T] > 0).all()
    assert torch.equal(m0[:, :T].cpu(), m1[:, :T].cpu()) and torch.equal(r0[:, :T].cpu(), r1[:, :T].cpu())


def case_sum_f64(n):
    """sep_sum_f64 against torch's fp64 sum of the same floats: equal after the rounding to fp32 (cancelling terms)"""
    x = rnd(n) * 100.0
    out = torch.full((1,), float("nan"), device=device_name(), dtype=torch.float32)
    HIP.sum_f64(to_device(x), n, out)
    device_sync()
    want = x.sum(dtype=torch.float64)
    # one rounding to fp32 of the result, and the fp64 summation's own bound n 2^-53 sum |x| (any order)
    assert abs(out.item() - want.item()) <= 2.0 ** -24 * abs(want.item()) + n * 2.0 ** -53 * x.abs().sum(dtype=torch.float64).item()


# ------------------------------------------------------------------------------------------------------ the folded depthwise kernels
def ref_v1(x, alpha, gamma, beta, mean, rstd, T):
    """v1 = gamma (PReLU(x) - mean_t) rstd_t + beta on frames < T, zero beyond (include/sepkernels.h), fp64"""
    x = x.double()
    u = torch.where(x > 0, x, alpha.double().reshape(()) * x) if alpha is not None else x
    v = (u - mean.double().unsqueeze(1)) * rstd.double().unsqueeze(1) * gamma.double().view(1, -1, 1) + beta.double().view(1, -1, 1)
    v[..., T:] = 0
    return v


def case_depthwise_cln(B, C, T, ldt, Kw, dil, causal, a, tol=2e-4):
    """sep_depthwise_cln_fwd / sep_depthwise_cln_bwd_weight against y = bias + sum_k w_k v1[t + k dil - pad] with v1 zero outside [0, T)
    (the reference pads after the norm) and the sums of dy * v1(tap k), dy over the frames, in fp64; the statistics are sep_cln_stats' own.
    Tolerance: 2e-4 of the result's scale, the bar of test_gpu_kernels.py::test_depthwise_tcn_geometry."""
    pad = (Kw - 1) * dil if causal else (Kw - 1) * dil // 2
    xc = _input(B, C, T, ldt)
    alpha_c = torch.tensor([a]) if a is not None else None
    gamma_c, beta_c, w_c, bias_c = rnd(C) + 1, rnd(C), rnd(C, 1, Kw), rnd(C)
    dy_c = torch.zeros(B, C, ldt)
    dy_c[..., :T] = rnd(B, C, T)
    x, gamma, beta, w, bias, dy = (to_device(t) for t in (xc, gamma_c, beta_c, w_c, bias_c, dy_c))
    alpha = to_device(alpha_c) if a is not None else None
    f32 = dict(device=device_name(), dtype=torch.float32)
    mean, rstd = torch.zeros(B, ldt, **f32), torch.zeros(B, ldt, **f32)
    HIP.cln_stats(x, mean, rstd, _ws(B, C, T, ldt), B, C, T, ldt, 1e-12, alpha=alpha)
    y = torch.full((B, C, ldt), float("nan"), **f32)
    HIP.depthwise_cln_fwd(x, alpha, gamma, beta, mean, rstd, w, bias, y, B, C, T, ldt, Kw, pad, dil)
    y0 = torch.full((B, C, ldt), float("nan"), **f32)
    HIP.depthwise_cln_fwd(x, alpha, gamma, beta, mean, rstd, w, None, y0, B, C, T, ldt, Kw, pad, dil)
    part = torch.full((B, C, Kw + 1), float("nan"), **f32)
    HIP.depthwise_cln_bwd_weight(dy, x, alpha, gamma, beta, mean, rstd, part, B, C, T, ldt, Kw, pad, dil)
    device_sync()
    v1 = ref_v1(xc, alpha_c, gamma_c, beta_c, mean.cpu(), rstd.cpu(), T)
    vp = torch.nn.functional.pad(v1, (pad, (Kw - 1) * dil - pad))
    ref0 = torch.nn.functional.conv1d(vp, w_c.double(), None, dilation=dil, groups=C)
    ref0[..., T:] = 0
    ref = ref0 + bias_c.double().view(1, C, 1)
    ref[..., T:] = 0
    for got, want, what in ((y, ref, "y"), (y0, ref0, "y without bias")):
        got = got.cpu().double()
        assert torch.isfinite(got).all(), what + ": unwritten output"
        assert (got[..., T:] == 0).all(), what + ": frames beyond T"
        assert (got - want).abs().max().item() <= tol * want.abs().max().item(), (what, (got - want).abs().max().item(), want.abs().max().item())
    g64 = dy_c.double()
    refp = torch.stack([(g64[..., :T] * vp[..., k * dil:k * dil + T]).sum(2) for k in range(Kw)] + [g64[..., :T].sum(2)], 2)
    got = part.cpu().double()
    assert torch.isfinite(got).all()
    assert (got - refp).abs().max().item() <= tol * refp.abs().max().item(), ((got - refp).abs().max().item(), refp.abs().max().item())


# (function, argument tuples): the shapes the host simulation runs too -- Kw in {3, 5}, dil in {1, 2, 64, 128}, both paddings, T not a
# multiple of 4, T smaller than the halo, with and without the slope, C in {16, 512, 528}
CASES = [
    ("case_sum_f64", [(1,), (255,), (8192,), (70001,)]),
    ("case_cln_stats", [(2, 16, 203, None), (1, 512, 150, 0.25), (2, 528, 131, -0.3), (2, 96, 1030, 0.0)]),
    ("case_depthwise_cln", [(2, 16, 203, 256, 3, 1, True, 0.25), (2, 16, 203, 256, 3, 2, True, None), (1, 16, 301, 384, 3, 64, True, 0.25),
                            (1, 16, 301, 384, 3, 128, True, -0.3), (1, 16, 301, 384, 3, 128, False, 0.25), (2, 16, 203, 256, 5, 2, True, 0.25),
                            (2, 16, 203, 256, 5, 1, False, None), (1, 16, 301, 384, 5, 64, False, 0.25), (1, 16, 301, 384, 5, 128, True, None),
                            (1, 16, 101, 128, 3, 64, True, 0.25), (1, 16, 50, 128, 5, 128, False, 0.25),          # T smaller than the halo
                            (1, 512, 131, 256, 3, 2, True, 0.25), (1, 528, 131, 256, 3, 4, True, 0.1), (1, 528, 67, 128, 5, 1, False, None)]),
]


@pytest.mark.parametrize("n", [1, 255, 8192, 70001])
def test_sum_f64(n):
    case_sum_f64(n)


@pytest.mark.parametrize("B,C,T,a", CASES[1][1] + [(16, 512, 3999, 0.25), (2, 640, 5003, 0.25)])
def test_cln_stats_equals_cln_fwd_bitwise(B, C, T, a):
    case_cln_stats(B, C, T, a)


@pytest.mark.parametrize("B,C,T,ldt,Kw,dil,causal,a", CASES[2][1] + [(16, 512, 3999, 4096, 3, 1, True, 0.25), (16, 512, 3999, 4096, 3, 128, True, 0.25),
                                                                      (1, 16, 16500, 16512, 3, 4, True, 0.25), (1, 16, 16500, 16512, 5, 3, False, None)])
def test_depthwise_cln_fwd_and_weight_gradient(B, C, T, ldt, Kw, dil, causal, a):
    """the shapes of the host tier plus the paper-size layer (B = 16, C = 512, ldt = 4096, dil 1 and 128) and rows longer than the LDS row"""
    case_depthwise_cln(B, C, T, ldt, Kw, dil, causal, a)


def test_cln_stats_then_apply_matches_cln_fwd_at_the_bar_of_the_norm():
    """the folded forward against the two-kernel form at the bar of test_gpu_kernels.py::test_prelu_cln_fwd_bwd (2e-5 of the scale): v1 read
    back from a depthwise kernel with ONE tap of weight 1 is the norm's output"""
    B, C, T = 2, 96, 3999
    ldt = (T + 127) // 128 * 128
    x, gamma, beta, alpha = _input(B, C, T, ldt).cuda(), (rnd(C) + 1).cuda(), rnd(C).cuda(), torch.tensor([-0.3]).cuda()
    y, mean, rstd = torch.empty(B, C, ldt).cuda(), torch.empty(B, ldt).cuda(), torch.empty(B, ldt).cuda()
    HIP.cln_fwd(x, gamma, beta, y, mean, rstd, _ws(B, C, T, ldt), B, C, T, ldt, 1e-12, alpha=alpha)
    z = torch.full((B, C, ldt), float("nan")).cuda()
    HIP.depthwise_cln_fwd(x, alpha, gamma, beta, mean, rstd, torch.ones(C, 1, 1).cuda(), None, z, B, C, T, ldt, 1, 0, 1)
    torch.cuda.synchronize()
    assert (z - y).abs().max().item() <= 2e-5 * y.abs().max().item()


# ------------------------------------------------------------------------------------------------------ the folded staged path on the fixtures
@pytest.mark.parametrize("arith", ["f16x3", "f32"])
@pytest.mark.parametrize("fold", ["1", "0"])
@pytest.mark.parametrize("name", STAGED)
def test_folded_staged_path_on_the_reference_fixtures(golden_dir, name, arith, fold, monkeypatch):
    """causal16* forward, loss, permutation and every gradient against the unmodified reference's fixture, with the folded kernels (the
    default) and under SEPK_CAUSAL_FOLD=0, at the bars of test_gpu_model.py::_golden_case for the staged names; the folded run must issue
    sep_depthwise_cln_fwd once per layer and no sep_depthwise_fwd."""
    import test_gpu_model as GM
    monkeypatch.setenv("SEPK_CAUSAL_FOLD", fold)
    calls = []
    backend = sepkernels.backend()
    for fn in ("depthwise_cln_fwd", "depthwise_fwd", "cln_stats", "depthwise_cln_bwd_weight"):
        orig = getattr(backend, fn)
        monkeypatch.setattr(backend, fn, (lambda o, n: (lambda *a, **k: (calls.append(n), o(*a, **k))[1]))(orig, fn), raising=False)
    prev = sepkernels.set_gemm_arith(arith)
    try:
        GM._golden_case(golden_dir, name)
    finally:
        sepkernels.set_gemm_arith(prev)
    nl = CONFIGS[name]["sep_num_blocks"] * CONFIGS[name]["sep_num_layers"]
    if fold == "1":
        assert calls.count("depthwise_cln_fwd") == nl and calls.count("cln_stats") == nl and calls.count("depthwise_cln_bwd_weight") == nl
        assert calls.count("depthwise_fwd") == 0
    else:
        assert calls.count("depthwise_fwd") == nl and calls.count("depthwise_cln_fwd") == 0


@pytest.mark.parametrize("name", STAGED)
def test_driver_on_the_reference_fixtures(golden_dir, name):
    """sepkernels.causal.forward / backward (the explicit driver the recorded step is made of) on the device against the same fixtures and
    bars: output, loss, permutation, every gradient"""
    from models.conv_tasnet import ConvTasNet
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    from sepkernels import causal
    g = np.load(os.path.join(golden_dir, "convtasnet_{}.npz".format(name)))
    model = ConvTasNet(**CONFIGS[name])
    model.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")})
    model.cuda()
    mixture, sources = torch.from_numpy(g["mixture"]).cuda(), torch.from_numpy(g["sources"]).cuda()
    P = {k: v.detach() for k, v in model.named_parameters()}
    with torch.no_grad():
        est, _, sv = causal.forward(model.get_config(), P, mixture.contiguous(), False, True)
    ref = torch.from_numpy(g["output_f64"])
    assert (est.view(ref.shape).double().cpu() - ref).abs().max().item() <= 1e-3 * ref.abs().max().item()
    leaf = est.detach().view(ref.shape).requires_grad_(True)
    loss, pattern = PIT1d(NegSISDR(), n_sources=CONFIGS[name]["n_sources"])(leaf, sources)
    assert abs(loss.item() - float(g["loss_f64"])) <= 1e-3 * abs(float(g["loss_f64"]))
    assert np.array_equal(pattern.cpu().numpy(), g["pattern"])
    loss.backward()
    G_ = {k: torch.full_like(v, float("nan")) for k, v in P.items()}
    with torch.no_grad():
        causal.backward(model.get_config(), P, sv, leaf.grad.view(est.shape).contiguous(), G_)
    torch.cuda.synchronize()
    num = den = 0.0
    for k, v in G_.items():
        r = torch.from_numpy(g["grad/" + k]).double()
        e = (v.double().cpu() - r).abs().max().item()
        assert np.isfinite(e), k
        num, den = max(num, e), max(den, r.abs().max().item())
        assert e <= 1e-3 * r.abs().max().item() or v.numel() == 1, "{}: {:.3e}".format(k, e / r.abs().max().item())
    assert num <= 1e-3 * den


# ------------------------------------------------------------------------------------------------------ recorded == eager at paper size
def test_recorded_causal_step_at_paper_size_trains_like_the_eager_step(monkeypatch):
    """PAPER with causal=True, 16 utterances of 4 s, ten DIFFERENT batches: recording + nine replays against ten eager steps, every loss at
    the bar of test_gpu_model.py::test_recorded_step_at_paper_best_sixteen_utterances_trains_like_the_eager_step.  Every replayed step is
    exactly ONE sep_run_sequence call and no other call on the library handle; a torch kernel that ran while recording would be missing
    from the replays and show as a wrong loss on the later batches.

    The eager staged step and the driver issue the same kernels with the same arguments (the tail through net.tail_forward / tail_backward in
    both, gradient sums by one rounding of x + y in both): on one batch every gradient is bit-identical, and over these ten steps the losses
    are equal for six steps and within 1e-6 relative afterwards (device-side Adam scalars; profiles/r10_causal_recorded.json)."""
    import test_gpu_model as GM
    from models.conv_tasnet import ConvTasNet
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    from sepkernels.train import FusedTrainStep
    cfg = dict(GM.PAPER, causal=True)
    g = torch.Generator().manual_seed(111)
    batches = [(0.1 * torch.randn(16, 2, 32000, generator=g)).cuda() for _ in range(10)]
    runs = []
    for recorded in (False, True):
        torch.manual_seed(111)
        model = ConvTasNet(**cfg).cuda()
        assert model.staged and not model.fused
        step = FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=2), lr=1e-3, max_norm=5.0, auto_record=recorded)
        assert step.recordable() is None
        losses, counts = [], []
        for i, src in enumerate(batches):
            mix = src.sum(1, keepdim=True).contiguous()
            if recorded and i > 0:
                lib = sepkernels.load()
                seen = []

                class Counting:
                    def __getattr__(self, name):
                        fn = getattr(lib, name)
                        if name in ("sep_last_error",):
                            return fn
                        return lambda *a: (seen.append(name), fn(*a))[1]
                monkeypatch.setattr(sepkernels, "_lib", Counting())
                losses.append(step(mix, src).item())
                monkeypatch.setattr(sepkernels, "_lib", lib)
                counts.append(seen)
            else:
                losses.append(step(mix, src).item())
        torch.cuda.synchronize()
        assert (step._seq is not None) == recorded and step.step_count == 10
        if recorded:
            assert all(c == ["sep_run_sequence"] for c in counts), [c[:4] for c in counts if c != ["sep_run_sequence"]][:2]
            names = step._seq.names()
            assert names[0] == "sep_absmax" and names[-1] == "sep_adam_step_dev" and "sep_depthwise_cln_fwd" in names and "sep_cln_bwd" in names
        runs.append(losses)
        del model, step
        torch.cuda.empty_cache()
    l0, l1 = runs
    print("eager   ", l0)
    print("recorded", l1)
    assert l0[-1] < l0[0]                                            # (the steps did train)
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 1e-5 * max(1.0, abs(a)), (l0, l1)
