"""GPU: mixture invariant training (criterion/mixit.py; csrc/mixit.hip: sep_mixit_gram, sep_mixit_search, sep_mixit_bwd).

The oracle is a brute-force MixIT in fp64 torch, written from the paper (Wisdom et al. 2020) and from the formulas stated in criterion/sdr.py
-- the reference's src/criterion/mixit.py is a stub, there is nothing to compare with: every assignment of itertools.product(range(N),
repeat=M), the remix by a 0/1 matrix, the measure of every (remix, mixture) pair from the waveforms (projection and energy ratio for SI-SDR;
no Gram matrix), torch.max / torch.min, autograd for the gradient.

(1) sep_mixit_gram against an fp64 product on the host; symmetric, repeatable and batch-independent bit for bit.
(2) sep_mixit_search on Gram matrices formed in fp64 on the host: code, value and per-mixture values, ties, the largest search, N = 1.
(3) sep_mixit_bwd against autograd of the oracle.
(4) MixIT(Neg...) end to end on the device, and the composed route forced by a clipped criterion whose clip never binds.
(5) estimates at 30 dB, where |x - y|^2 = tt - 2a + yy cancels: the error of the new route next to the error of criterion.sdr.sisdr on the
    materialised best remix (the kernels this tree had before), both against the oracle.
(6) one training step through FusedTrainStep.
The case functions take their device through the hooks below, so tests/test_mixit_cpu.py runs them on an emulator of the three calls and on
the host simulation of the kernel sources."""
import functools
import itertools
import math

import pytest
import torch

import sepkernels

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
to_device = lambda t: t.cuda()                      # noqa: E731
device_sync = lambda: torch.cuda.synchronize()      # noqa: E731

SLAB = sepkernels.MIXIT_SLAB
EPS, SNR_MAX = 1e-12, 30.0
TAU = 10.0 ** (-SNR_MAX / 10.0)
KINDS = ("sisdr", "sdr", "snr")                       # kind 0, 1, 2 of the kernels
# (B, M, N, T); the generator seed of a shape is its index
SHAPES = [(3, 4, 2, 4001), (2, 8, 2, 1537), (2, 3, 3, 257), (4, 2, 2, 64), (2, 1, 2, 100), (2, 5, 1, 300)]
SHAPE_IDS = ["x".join(map(str, s)) for s in SHAPES]
GRAM_T = [1, 255, 257, SLAB - 1, SLAB, SLAB + 1, 2 * SLAB + 17]
GRAM_MN = [(1, 1), (3, 2), (8, 2), (16, 8)]           # R = 2, 5, 10, 24: the last is the declared limit


def nan(*shape, dtype=torch.float32):
    return to_device(torch.full(shape, float("nan"), dtype=dtype))


# ---------------------------------------------------------------------------------------------------------------- inputs and the oracle
@functools.lru_cache(maxsize=None)
def make_case(index, noise=0.3, gain=0.8):
    """-> est (B, M, T), tgt (B, N, T) as fp64 tensors holding fp32-representable values, and the planted assignment (B, M)"""
    B, M, N, T = SHAPES[index]
    g = torch.Generator().manual_seed(index)
    src = torch.randn(B, M, T, generator=g, dtype=torch.float64)
    assign = torch.randint(N, (B, M), generator=g)
    tgt = torch.zeros(B, N, T, dtype=torch.float64)
    for b in range(B):
        for m in range(M):
            tgt[b, assign[b, m]] += src[b, m]
    est = gain * src + noise * torch.randn(B, M, T, generator=g, dtype=torch.float64)
    return est.float().double(), tgt.float().double(), assign


def measure(kind, y, x, eps=EPS, tau=TAU):
    """the measure of (remix y, mixture x) over the last axis in dB, as criterion/sdr.py states the formulas"""
    if kind == "sisdr":
        tt = x.square().sum(-1, keepdim=True) + eps
        proj = (y * x).sum(-1, keepdim=True) / tt * x
        return 10 * torch.log10((proj.square().sum(-1) + eps) / ((proj - y).square().sum(-1) + eps))
    tt = x.square().sum(-1)
    return 10 * torch.log10((tt + eps) / ((x - y).square().sum(-1) + (tau * tt if kind == "snr" else 0.0) + eps))


def remix_matrix(M, N, codes=None):
    """(K, N, M) 0/1 fp64: [k][n][m] = 1 where assignment k of itertools.product order hands estimate m to mixture n"""
    table = torch.tensor(list(itertools.product(range(N), repeat=M)), dtype=torch.int64)
    if codes is not None:
        table = table[codes]
    return torch.nn.functional.one_hot(table, N).transpose(1, 2).double()


def all_values(kind, est, tgt):
    """(B, N^M, N): the measure of every mixture under every assignment"""
    M, N = est.shape[1], tgt.shape[1]
    remix = torch.einsum("knm,bmt->bknt", remix_matrix(M, N), est)
    return measure(kind, remix, tgt.unsqueeze(1))


@functools.lru_cache(maxsize=None)
def case_values(index, kind, noise=0.3, gain=0.8):
    est, tgt, _ = make_case(index, noise, gain)
    return all_values(kind, est, tgt)


def extremum(values, maximize, use_mean):
    """values (B, K, N) -> best (B,), code (B,), per_mix (B, N), gap (B,): the lead of the extremum over the runner-up (inf for K = 1)"""
    score = values.mean(-1) if use_mean else values.sum(-1)
    best, code = score.max(1) if maximize else score.min(1)
    ranked = score.sort(1, descending=bool(maximize))[0]
    gap = (ranked[:, 0] - ranked[:, 1]).abs() if score.shape[1] > 1 else torch.full_like(best, float("inf"))
    return best, code, values[torch.arange(values.shape[0]), code], gap


def oracle_gradient(kind, est, tgt, code, gw, eps=EPS):
    """d / d est of sum_b gw_b sum_n measure_n under the assignment `code`, by autograd"""
    M, N = est.shape[1], tgt.shape[1]
    leaf = est.clone().requires_grad_(True)
    remix = torch.einsum("bnm,bmt->bnt", remix_matrix(M, N, code), leaf)
    (measure(kind, remix, tgt, eps=eps).sum(-1) * gw).sum().backward()
    return leaf.grad


def check_planted(index, kind):
    """the planted assignment is the oracle's best for this measure, by at least 1 dB: an equality test on the assignment hides nothing"""
    B, M, N, T = SHAPES[index]
    best, code, _, gap = extremum(case_values(index, kind), True, True)
    planted = (make_case(index)[2] * torch.tensor([N ** (M - 1 - m) for m in range(M)])).sum(1)
    assert torch.equal(code, planted), (SHAPES[index], kind, code, planted)
    assert gap.min().item() >= 1.0, (SHAPES[index], kind, gap)


def host_gram(est, tgt):
    rows = torch.cat([est, tgt], 1)
    return rows @ rows.transpose(1, 2)


# ---------------------------------------------------------------------------------------------------------------- (1) sep_mixit_gram
def _call_gram(est, tgt):
    B, M, T = est.shape
    N = tgt.shape[1]
    nbytes = HIP.mixit_scratch_bytes(B, M, N, T)
    assert nbytes == 8 * B * ((T + SLAB - 1) // SLAB) * (M + N) ** 2
    scratch = nan(nbytes // 8, dtype=torch.float64)
    gram = nan(B, M + N, M + N, dtype=torch.float64)
    HIP.mixit_gram(to_device(est.float().contiguous()), to_device(tgt.float().contiguous()), gram, scratch, B, M, N, T)
    device_sync()
    return gram.cpu()


def case_gram(M, N, T, batch_check=False):
    g = torch.Generator().manual_seed(100 * (M + N) + T % 97)
    B = 3 if batch_check else 1
    est = torch.randn(B, M, T, generator=g).double()
    tgt = torch.randn(B, N, T, generator=g).double()
    got = _call_gram(est, tgt)
    want = host_gram(est, tgt)
    diag = torch.diagonal(want, dim1=1, dim2=2)
    err = ((got - want).abs() / torch.sqrt(diag.unsqueeze(2) * diag.unsqueeze(1))).max().item()
    print("gram M={} N={} T={}: max error relative to sqrt(G_ii G_jj) {:.3e}".format(M, N, T, err))
    assert torch.isfinite(got).all() and err <= 1e-6, (M, N, T, err)
    assert torch.equal(got, got.transpose(1, 2)), "the Gram matrix must be symmetric bit for bit"
    assert torch.equal(got, _call_gram(est, tgt)), "two runs must give the same bits"
    if batch_check:
        assert torch.equal(got[1:2], _call_gram(est[1:2], tgt[1:2])), "an item must give the same bits in any batch"


@pytest.mark.parametrize("T", GRAM_T)
@pytest.mark.parametrize("MN", GRAM_MN, ids=["R2", "R5", "R10", "R24"])
def test_gram_kernel(MN, T):
    case_gram(MN[0], MN[1], T, batch_check=(T == SLAB + 1))


# ---------------------------------------------------------------------------------------------------------------- (2) sep_mixit_search
def _call_search(gram, M, N, kind, maximize, use_mean):
    B = gram.shape[0]
    best_val, best_idx, per_mix = nan(B), to_device(torch.full((B,), -7, dtype=torch.int64)), nan(B, N)
    HIP.mixit_search(to_device(gram.contiguous()), B, M, N, KINDS.index(kind), maximize, use_mean, EPS, TAU, best_val, best_idx, per_mix)
    device_sync()
    return best_val.cpu().double(), best_idx.cpu(), per_mix.cpu().double()


def case_search(index, kind, maximize, use_mean):
    B, M, N, T = SHAPES[index]
    check_planted(index, kind)
    est, tgt, _ = make_case(index)
    best, code, per_mix, gap = extremum(case_values(index, kind), maximize, use_mean)
    # the lead of the extremum over the runner-up, four decades above the value tolerance: the planted best by >= 1 dB (checked above); the
    # minimum -- the worst assignment, which nothing plants -- must still be told apart far above the fp64 noise of either side
    assert gap.min().item() >= (1.0 if maximize else 1e-3), (SHAPES[index], kind, maximize, use_mean, gap)
    got_val, got_idx, got_mix = _call_search(host_gram(est, tgt), M, N, kind, maximize, use_mean)
    print("search {} {} max={} mean={}: value error {:.3e} dB, per-mixture {:.3e} dB".format(
        SHAPES[index], kind, maximize, use_mean, (got_val - best).abs().max().item(), (got_mix - per_mix).abs().max().item()))
    assert torch.equal(got_idx, code), (got_idx, code)
    assert (got_val - best).abs().max().item() <= 1e-5 and (got_mix - per_mix).abs().max().item() <= 1e-5


@pytest.mark.parametrize("use_mean", [1, 0], ids=["mean", "sum"])
@pytest.mark.parametrize("maximize", [1, 0], ids=["max", "min"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_search_kernel(index, kind, maximize, use_mean):
    case_search(index, kind, maximize, use_mean)


def case_search_tie(kind):
    """estimates 0 and 1 are the same signal e, mixture 0 holds one copy of it and mixture 1 the other plus a third source (both with some
    noise, so that no difference cancels to nothing): the codes (0, 1, 1) = 3 and (1, 0, 1) = 5 score alike to the bit and beat every
    other: the lower wins.  Row and column 1 of the Gram matrix are copies of row and column 0, as sep_mixit_gram gives them for equal rows."""
    g = torch.Generator().manual_seed(77)
    e, s = torch.randn(2, 1, 500, generator=g).float().double(), torch.randn(2, 1, 500, generator=g).float().double()
    noise = 0.3 * torch.randn(2, 2, 500, generator=g, dtype=torch.float64)
    est, tgt = torch.cat([e, e, s], 1), (torch.cat([e, e + s], 1) + noise).float().double()
    gram = host_gram(est, tgt)
    gram[:, 1, :] = gram[:, 0, :]
    gram[:, :, 1] = gram[:, :, 0]
    values = all_values(kind, est, tgt)
    for maximize, use_mean in ((1, 1), (1, 0)):
        score = values.mean(-1) if use_mean else values.sum(-1)
        assert torch.equal(score[:, 3], score[:, 5]) and (score.max(1)[1] == 3).all(), "the oracle itself must see the tie, and break it downwards"
        got_val, got_idx, _ = _call_search(gram, 3, 2, kind, maximize, use_mean)
        assert got_idx.tolist() == [3, 3], got_idx
        assert (got_val - score[:, 3]).abs().max().item() <= 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_search_kernel_breaks_ties_towards_the_lower_code(kind):
    case_search_tie(kind)


def case_search_largest(kind):
    """N^M = 2^16 = 65536 assignments: the declared limit (every thread of the workgroup scores 256 codes)"""
    M, N, T = 16, 2, 24
    g = torch.Generator().manual_seed(16)
    src = torch.randn(1, M, T, generator=g, dtype=torch.float64)
    assign = torch.randint(N, (1, M), generator=g)
    tgt = torch.zeros(1, N, T, dtype=torch.float64)
    for m in range(M):
        tgt[0, assign[0, m]] += src[0, m]
    est, tgt = (0.8 * src + 0.3 * torch.randn(1, M, T, generator=g, dtype=torch.float64)).float().double(), tgt.float().double()
    best, code, per_mix, gap = extremum(all_values(kind, est, tgt), True, True)
    assert gap.min().item() >= 1e-3, gap
    got_val, got_idx, got_mix = _call_search(host_gram(est, tgt), M, N, kind, 1, 1)
    assert torch.equal(got_idx, code), (got_idx, code)
    assert (got_val - best).abs().max().item() <= 1e-5 and (got_mix - per_mix).abs().max().item() <= 1e-5


@pytest.mark.parametrize("kind", KINDS)
def test_search_kernel_at_65536_assignments(kind):
    case_search_largest(kind)


# ---------------------------------------------------------------------------------------------------------------- (3) sep_mixit_bwd
def _check_bwd(kind, est, tgt, code, eps=EPS):
    B, M, T = est.shape
    N = tgt.shape[1]
    gw = torch.linspace(-1.0, 1.5, B, dtype=torch.float64).float().double()
    want = oracle_gradient(kind, est, tgt, code, gw, eps)
    d_est = nan(B, M, T)
    HIP.mixit_bwd(to_device(est.float().contiguous()), to_device(tgt.float().contiguous()), to_device(host_gram(est, tgt).contiguous()),
                  to_device(code.contiguous()), to_device(gw.float()), d_est, B, M, N, T, KINDS.index(kind), eps, TAU)
    device_sync()
    got = d_est.cpu().double()
    err = (got - want).abs().max().item() / want.abs().max().item()
    print("bwd {} B={} M={} N={} T={}: error relative to the largest entry {:.3e}".format(kind, B, M, N, T, err))
    assert torch.isfinite(got).all() and err <= 1e-5, (kind, est.shape, err)


def case_bwd(index, kind):
    est, tgt, _ = make_case(index)
    _check_bwd(kind, est, tgt, extremum(case_values(index, kind), True, True)[1])


def case_bwd_lengths(kind, T):
    """T = 1 and one sample past the 1024-sample tile of a workgroup; the code is given, not searched: (1, 1, 0) leaves no mixture empty,
    (2, 2, 2) hands everything to the last one of three.  A one-sample remix is always a multiple of its mixture: SI-SDR is then decided by eps
    alone (the residual is eps) and its gradient is a difference of terms 1 / eps apart, which no arithmetic resolves at eps = 1e-12; the
    kernel takes eps as an argument, and at T = 1 the case passes eps = 1, which keeps every term of the gradient of order one."""
    g = torch.Generator().manual_seed(T)
    est, tgt = torch.randn(2, 3, T, generator=g).double(), torch.randn(2, 3, T, generator=g).double()
    _check_bwd(kind, est, tgt, torch.tensor([1 * 9 + 1 * 3 + 0, 2 * 9 + 2 * 3 + 2]), eps=1.0 if T == 1 else EPS)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_bwd_kernel(index, kind):
    case_bwd(index, kind)


@pytest.mark.parametrize("T", [1, 1025])
@pytest.mark.parametrize("kind", KINDS)
def test_bwd_kernel_at_the_tile_edges(kind, T):
    case_bwd_lengths(kind, T)


# ---------------------------------------------------------------------------------------------------------------- (4) the criterion
def criteria():
    from criterion.sdr import NegSDR, NegSISDR, NegThresholdedSNR
    return {"sisdr": NegSISDR, "sdr": NegSDR, "snr": NegThresholdedSNR}


def case_criterion(index, kind):
    from criterion.mixit import MixIT
    B, M, N, T = SHAPES[index]
    check_planted(index, kind)
    est, tgt, assign = make_case(index)
    best, code, _, _ = extremum(case_values(index, kind), True, True)
    crit = MixIT(criteria()[kind]())
    leaf = to_device(est.float()).requires_grad_(True)
    target = to_device(tgt.float())
    loss, got_assign = crit(leaf, target)
    loss.backward()
    per_item, again = crit(leaf.detach(), target, batch_mean=False)
    device_sync()
    want_grad = oracle_gradient(kind, est, tgt, code, torch.full((B,), -1.0 / (B * N), dtype=torch.float64))
    err_loss = abs(loss.item() + best.mean().item())
    err_grad = (leaf.grad.cpu().double() - want_grad).abs().max().item() / want_grad.abs().max().item()
    print("MixIT {} {}: loss error {:.3e} dB, gradient error {:.3e}".format(SHAPES[index], kind, err_loss, err_grad))
    assert got_assign.dtype == torch.int64 and got_assign.device == leaf.device
    assert torch.equal(got_assign.cpu(), assign) and torch.equal(again.cpu(), assign)
    assert loss.dim() == 0 and err_loss <= 1e-4
    assert per_item.shape == (B,) and (per_item.cpu().double() + best).abs().max().item() <= 1e-4
    assert err_grad <= 1e-5


def case_composed(index):
    """a clipped criterion takes the composed route; with a clip that never binds it must find the same assignment and the same loss"""
    from criterion.mixit import MixIT
    from criterion.sdr import ClippedNegSISDR
    B, M, N, T = SHAPES[index]
    est, tgt, assign = make_case(index)
    best = extremum(case_values(index, "sisdr"), True, True)[0]
    leaf = to_device(est.float()).requires_grad_(True)
    loss, got_assign = MixIT(ClippedNegSISDR(min=-1000.0))(leaf, to_device(tgt.float()), batch_mean=False)
    loss.sum().backward()
    device_sync()
    assert torch.equal(got_assign.cpu(), assign)
    assert loss.shape == (B,) and (loss.detach().cpu().double() + best).abs().max().item() <= 1e-4
    assert torch.isfinite(leaf.grad).all() and leaf.grad.abs().max().item() > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_criterion_on_the_device_against_the_oracle(index, kind):
    case_criterion(index, kind)


@pytest.mark.parametrize("index", range(len(SHAPES)), ids=SHAPE_IDS)
def test_composed_route_agrees(index):
    case_composed(index)


# ---------------------------------------------------------------------------------------------------------------- (5) high SNR
def test_high_snr_error_next_to_the_materialised_remix():
    """est = src + 0.03 randn (about 30 dB) on the (3, 4, 2, 4001) input.  The value error of MixIT(NegSISDR()) against the fp64 oracle may be
    at most twice the error of criterion.sdr.sisdr on the materialised best remix (sep_sisdr_dots: short fp32 runs folded into fp64) plus
    1e-5 dB.  Measured on an MI355X: new route 8.9e-07 dB, sisdr on the materialised remix 2.3e-05 dB."""
    from criterion.mixit import MixIT
    from criterion.sdr import NegSISDR, sisdr
    B, M, N, T = SHAPES[0]
    est, tgt, assign = make_case(0, 0.03, 1.0)
    best, code, per_mix, gap = extremum(case_values(0, "sisdr", 0.03, 1.0), True, True)
    assert gap.min().item() >= 1.0 and best.min().item() >= 25.0, (gap, best)
    e32, t32 = to_device(est.float()), to_device(tgt.float())
    loss, got_assign = MixIT(NegSISDR())(e32, t32, batch_mean=False)
    remix = torch.einsum("bnm,bmt->bnt", to_device(remix_matrix(M, N, code).float()), e32)
    parent = sisdr(remix, t32)
    device_sync()
    err_new = (loss.cpu().double() + best).abs().max().item()
    err_parent = (parent.cpu().double().mean(1) - best).abs().max().item()
    print("high SNR ({:.1f} dB): new route {:.3e} dB, sisdr on the materialised remix {:.3e} dB".format(best.mean().item(), err_new, err_parent))
    assert torch.equal(got_assign.cpu(), assign)
    assert err_new <= 2.0 * err_parent + 1e-5, (err_new, err_parent)


# ---------------------------------------------------------------------------------------------------------------- (6) one training step
def test_one_training_step():
    from criterion.mixit import MixIT
    from criterion.sdr import NegThresholdedSNR
    from models.conv_tasnet import ConvTasNet
    from sepkernels.train import FusedTrainStep
    torch.manual_seed(5)
    model = ConvTasNet(n_basis=16, kernel_size=4, stride=2, enc_basis="trainable", dec_basis="trainable", enc_nonlinear=None, sep_hidden_channels=16,
                       sep_bottleneck_channels=16, sep_skip_channels=16, sep_kernel_size=3, sep_num_blocks=1, sep_num_layers=2, causal=False,
                       n_sources=4).cuda()
    assert model.fused
    mixtures = 0.1 * torch.randn(2, 2, 512, device="cuda")
    mixture = mixtures.sum(1, keepdim=True)
    step = FusedTrainStep(model, MixIT(NegThresholdedSNR()), lr=1e-3, max_norm=5.0)
    assert step.recordable() is not None            # MixIT steps eagerly: recording it is out of scope
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    first = step(mixture, mixtures).item()
    second = step(mixture, mixtures).item()
    assert math.isfinite(first) and math.isfinite(second) and second < first, (first, second)
    for k, p in model.named_parameters():
        assert not torch.equal(p.detach(), before[k]), "{} did not move".format(k)
