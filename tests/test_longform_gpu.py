"""GPU: window-by-window separation of long recordings (sepkernels/longform.py; csrc/stitch.hip: sep_stitch_cost, sep_stitch_chain, sep_stitch_ola).

The reference has nothing of the kind.  The oracle is written here from the definitions of include/sepkernels.h in numpy fp64, the matching by
brute force over itertools.permutations (n <= 4; beyond that the composed route of the module, itself held to this oracle by
tests/test_longform_cpu.py, is the yardstick).

(1) sep_stitch_cost against the fp64 sums within 1e-12 relative (a sum of O <= 1060 non-negative fp64 terms, each with at most two roundings, is
    off by at most (O + 2) 2^-53 = 1.2e-13 in any order); identical rows cost exactly 0; written, not accumulated; a second run has the same bits.
(2) sep_stitch_chain against a Python loop, exactly; entries outside [0, n) never index out of range.
(3) sep_stitch_ola against the fp64 oracle: inside a cross-fade within 1e-6 max|est| (three fp32 roundings on values bounded by max|est|, times
    a margin of about four), elsewhere a copy bit for bit; every element written.
(4) stitch() on the kernels against the composed route on the same values in fp64, on inputs with a guaranteed gap between the best and every
    other matching.   (5) separate_long on the device with a tiny Conv-TasNet.
The issue's window geometries (2, 1), (128, 65), (130, 65), (1100, 571) give overlaps of 1, 63, 65 and 529 samples around the wave width; none of
them has win and hop both multiples of 4, so (128, 64) and (2200, 1140) are added for the 16-byte paths (the second: a second step of the
workgroup's walk over the overlap, 1060 > 4 x 256).
The case functions take their device through the hooks below, so tests/test_longform_cpu.py runs them on the host simulation of the kernel
sources."""
import functools
import itertools

import numpy as np
import pytest
import torch

import sepkernels
from sepkernels import longform

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
to_device = lambda t: t.cuda()                      # noqa: E731
device_sync = lambda: torch.cuda.synchronize()      # noqa: E731

GEOMS = [(2, 1), (128, 65), (130, 65), (1100, 571)]             # (win, hop) of the issue
VEC_GEOMS = [(128, 64), (2200, 1140)]                            # win, hop multiples of 4: the 16-byte loads
ALL_GEOMS = GEOMS + VEC_GEOMS
GEOM_IDS = ["{}-{}".format(*g) for g in ALL_GEOMS]
COST_N = [1, 2, 3, 9, 64]


def nan(*shape, dtype=torch.float32):
    return to_device(torch.full(shape, float("nan"), dtype=dtype))


# ---------------------------------------------------------------------------------------------------------------- the oracle (numpy fp64)
def oracle_cost(est, hop):
    """est (B, W, n, win) fp64 -> (B, W - 1, n, n): the squared distance of every pair of rows of neighbouring windows on their overlap"""
    B, W, n, win = est.shape
    out = np.empty((B, max(W - 1, 0), n, n))
    for b in range(B):
        for w in range(W - 1):
            d = est[b, w][:, None, hop:] - est[b, w + 1][None, :, :win - hop]
            out[b, w] = (d * d).sum(-1)
    return out


def oracle_match(cost):
    """(n, n) -> (perm, best, second): the cheapest of the n! matchings by brute force, its value and the value of the runner-up (inf for n = 1)"""
    n = cost.shape[0]
    scored = sorted((sum(cost[i, p[i]] for i in range(n)), p) for p in itertools.permutations(range(n)))
    return list(scored[0][1]), scored[0][0], (scored[1][0] if len(scored) > 1 else float("inf"))


def oracle_chain(perm_local, n):
    """(B, W - 1, n) integers -> (B, W, n): perm_abs[0] = identity, perm_abs[w + 1][s] = perm_local[w][perm_abs[w][s]], an entry outside [0, n) read as 0"""
    B, Wm1 = perm_local.shape[:2]
    out = np.zeros((B, Wm1 + 1, n), dtype=np.int64)
    for b in range(B):
        out[b, 0] = np.arange(n)
        for w in range(Wm1):
            for s in range(n):
                v = int(perm_local[b, w, out[b, w, s]])
                out[b, w + 1, s] = v if 0 <= v < n else 0
    return out


def oracle_ola(est, perm_abs, hop, T):
    """est (B, W, n, win) fp64, perm_abs (B, W, n) -> out (B, n, T) fp64 and fade (T,) bool: which samples lie in a cross-fade"""
    B, W, n, win = est.shape
    O = win - hop
    out, fade = np.empty((B, n, T)), np.zeros(T, dtype=bool)
    for t in range(T):
        w = min(t // hop, W - 1)
        k = t - w * hop
        fade[t] = w >= 1 and k < O
        for b in range(B):
            c = est[b, w, perm_abs[b, w], k]
            if fade[t]:
                a = est[b, w - 1, perm_abs[b, w - 1], hop + k]
                out[b, :, t] = a + (k + 0.5) / O * (c - a)
            else:
                out[b, :, t] = c
    return out, fade


@functools.lru_cache(maxsize=None)
def gapped(B, W, n, win, hop, seed=0):
    """-> estimates (B, W, n, win) fp64 holding fp32-representable values, scramble (B, W, n): n long randn tracks cut into windows, the rows of
    every window scrambled (row r of window w is track scramble[b][w][r]), 0.01 randn added.  The matching that continues every track costs
    about 2 O 1e-4 at a boundary, every other one at least about 4 O."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * n + win)
    tracks = torch.randn(B, n, (W - 1) * hop + win, generator=g, dtype=torch.float64)
    scramble = torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(W)]) for _ in range(B)])
    est = torch.empty(B, W, n, win, dtype=torch.float64)
    for b in range(B):
        for w in range(W):
            est[b, w] = tracks[b, scramble[b, w], w * hop:w * hop + win]
    est += 0.01 * torch.randn(B, W, n, win, generator=g, dtype=torch.float64)
    return est.float().double(), scramble


def undoes_the_scramble(perm_abs, scramble):
    """row perm_abs[b][w][s] of window w is the track that row s of window 0 is"""
    return torch.equal(scramble.gather(2, perm_abs.cpu()), scramble[:, :1].expand_as(scramble))


# ---------------------------------------------------------------------------------------------------------------- (1) sep_stitch_cost
def case_cost(B, W, n, win, hop, offset=0):
    """offset: floats by which est is moved off its 16-byte alignment"""
    O = win - hop
    g = torch.Generator().manual_seed(B + 10 * W + 100 * n + win)
    est = torch.randn(B, W, n, win, generator=g)
    est[B - 1, 1, 0, :O] = est[B - 1, 0, n - 1, hop:]                       # two identical rows: a cost of exactly 0
    flat = to_device(torch.cat([torch.zeros(offset), est.reshape(-1)]))
    d_est = flat[offset:].view(B, W, n, win)
    got = nan(B, W - 1, n, n, dtype=torch.float64)
    HIP.stitch_cost(d_est, got, B, W, n, win, hop)
    again = nan(B, W - 1, n, n, dtype=torch.float64)
    HIP.stitch_cost(d_est, again, B, W, n, win, hop)
    device_sync()
    got, again = got.cpu(), again.cpu()
    want = torch.from_numpy(oracle_cost(est.double().numpy(), hop))
    assert torch.isfinite(got).all(), "an entry was not written"
    assert torch.equal(got, again), "two runs differ"
    assert got[B - 1, 0, n - 1, 0].item() == 0.0
    err = ((got - want).abs() / want.clamp_min(1e-300)).max().item()
    assert err <= 1e-12, (B, W, n, win, hop, err)


@pytest.mark.parametrize("win,hop", ALL_GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("n", COST_N)
def test_stitch_cost(n, win, hop):
    for B in (1, 2):
        for W in (2, 5):
            case_cost(B, W, n, win, hop)


def test_stitch_cost_off_the_16_byte_alignment():
    for n in (3, 9):
        case_cost(2, 3, n, 128, 64, offset=1)


def case_refusals():
    """refused with a message before any launch: the outputs keep their NaN"""
    est = to_device(torch.randn(1, 3, 2, 8))
    cost, out = nan(1, 2, 2, 2, dtype=torch.float64), nan(1, 2, 16)
    perm = to_device(torch.zeros(1, 3, 2, dtype=torch.int64))
    for W, n, win, hop in ((3, 2, 8, 3), (3, 2, 8, 8), (3, 0, 8, 4), (3, 65, 8, 4), (0, 2, 8, 4), (3, 2, 1, 1)):
        with pytest.raises(sepkernels.SepKernelsError, match="sep_stitch_cost: bad arguments"):
            HIP.stitch_cost(est, cost, 1, W, n, win, hop)
        with pytest.raises(sepkernels.SepKernelsError, match="sep_stitch_ola: bad arguments"):
            HIP.stitch_ola(est, perm, out, 1, W, n, win, hop, 16)
    with pytest.raises(sepkernels.SepKernelsError, match="sep_stitch_ola: bad arguments"):
        HIP.stitch_ola(est, perm, out, 1, 3, 2, 8, 4, 17)                     # three windows of 8 at hop 4 cover 16 samples
    with pytest.raises(sepkernels.SepKernelsError, match="sep_stitch_ola: bad arguments"):
        HIP.stitch_ola(est, perm, out, 1, 3, 2, 8, 4, 0)
    for B, W, n in ((0, 3, 2), (1, 0, 2), (1, 3, 65), (1, 3, 0)):
        with pytest.raises(sepkernels.SepKernelsError, match="sep_stitch_chain: bad arguments"):
            HIP.stitch_chain(perm[:, :2], perm, B, W, n)
    with pytest.raises(sepkernels.SepKernelsError, match="null pointer"):
        HIP.stitch_cost(est, None, 1, 3, 2, 8, 4)
    HIP.stitch_cost(est, None, 1, 1, 2, 8, 4)                                 # one window: no boundary, nothing is launched
    device_sync()
    assert torch.isnan(cost.cpu()).all() and torch.isnan(out.cpu()).all()


def test_stitch_refusals():
    case_refusals()


# ---------------------------------------------------------------------------------------------------------------- (2) sep_stitch_chain
def case_chain(B, W, n):
    g = torch.Generator().manual_seed(B + 10 * W + 1000 * n)
    local = torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(W - 1)]) for _ in range(B)]) if W > 1 else torch.zeros(B, 0, n, dtype=torch.int64)
    variants = [local]
    if W > 1:
        bad = local.clone()
        bad[B - 1, 0, 0], bad[0, W - 2, n - 1] = -1, n                         # one entry below, one beyond the range
        variants.append(bad)
    for pl in variants:
        got = to_device(torch.full((B, W, n), -7, dtype=torch.int64))
        HIP.stitch_chain(to_device(pl) if W > 1 else None, got, B, W, n)
        device_sync()
        got = got.cpu()
        assert got.min() >= 0 and got.max() < n
        assert torch.equal(got, torch.from_numpy(oracle_chain(pl.numpy(), n))), (B, W, n)


@pytest.mark.parametrize("W", [1, 2, 300])
@pytest.mark.parametrize("n", [1, 2, 64])
def test_stitch_chain(n, W):
    for B in (1, 3):
        case_chain(B, W, n)


# ---------------------------------------------------------------------------------------------------------------- (3) sep_stitch_ola
def case_ola(B, W, n, win, hop, offset=0):
    g = torch.Generator().manual_seed(B + 10 * W + 100 * n + win)
    est = torch.randn(B, W, n, win, generator=g)
    perm_abs = torch.stack([torch.stack([torch.randperm(n, generator=g) for _ in range(W)]) for _ in range(B)])
    flat = to_device(torch.cat([torch.zeros(offset), est.reshape(-1)]))
    d_est, d_perm = flat[offset:].view(B, W, n, win), to_device(perm_abs)
    tol = 1e-6 * est.abs().max().item()
    for T in sorted({win, win + 1, (W - 1) * hop + 1, (W - 1) * hop + win}):
        want, fade = oracle_ola(est.double().numpy(), perm_abs.numpy(), hop, T)
        got = nan(B, n, T)
        HIP.stitch_ola(d_est, d_perm, got, B, W, n, win, hop, T)
        device_sync()
        got = got.cpu()
        assert torch.isfinite(got).all(), "an element was not written"
        want, fade = torch.from_numpy(want), torch.from_numpy(fade)
        assert torch.equal(got[..., ~fade].double(), want[..., ~fade]), (B, W, n, win, hop, T, "outside a cross-fade: not a copy")
        if fade.any():
            err = (got[..., fade].double() - want[..., fade]).abs().max().item()
            assert err <= tol, (B, W, n, win, hop, T, err, tol)


@pytest.mark.parametrize("win,hop", ALL_GEOMS, ids=GEOM_IDS)
def test_stitch_ola(win, hop):
    for W in (2, 5):
        case_ola(2, W, 3, win, hop)
    case_ola(1, 3, 64, win, hop)


def test_stitch_ola_off_the_16_byte_alignment():
    case_ola(2, 3, 3, 128, 64, offset=1)


def test_stitch_ola_reads_a_bad_entry_as_row_zero():
    est = torch.randn(1, 2, 3, 8)
    perm = torch.tensor([[[0, 1, 2], [-1, 3, 1]]])
    out = nan(1, 3, 12)
    HIP.stitch_ola(to_device(est), to_device(perm), out, 1, 2, 3, 8, 4, 12)
    device_sync()
    assert torch.equal(out.cpu()[0, :2, 8:], est[0, 1, [0, 0], 4:]) and torch.equal(out.cpu()[0, 2, 8:], est[0, 1, 1, 4:])


# ---------------------------------------------------------------------------------------------------------------- (4) stitch on the kernels
def case_stitch(B, W, n, win, hop, T):
    est, scramble = gapped(B, W, n, win, hop)
    want_out, want_perm, want_cost = longform._stitch_composed(est, hop, T)
    out, perm_abs, boundary = longform.stitch(to_device(est.float()), hop, T)
    device_sync()
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, n, T) and tuple(boundary.shape) == (B, W - 1)
    assert torch.equal(perm_abs.cpu(), want_perm) and undoes_the_scramble(perm_abs, scramble)
    assert (out.cpu().double() - want_out).abs().max().item() <= 1e-6 * est.abs().max().item()
    assert ((boundary.cpu() - want_cost).abs() / want_cost).max().item() <= 1e-12


@pytest.mark.parametrize("n", [2, 5, 20])
def test_stitch_kernel_route_against_the_composed_route(n):
    case_stitch(2, 7, n, 1100, 571, 6 * 571 + 1100 - 37)


def test_stitch_of_one_window_is_a_copy():
    est = torch.randn(2, 1, 3, 64)
    out, perm_abs, boundary = longform.stitch(to_device(est), 40, 50)
    assert torch.equal(out.cpu(), est[:, 0, :, :50]) and tuple(boundary.shape) == (2, 0) and torch.equal(perm_abs.cpu(), torch.arange(3).repeat(2, 1, 1))


# ---------------------------------------------------------------------------------------------------------------- (5) separate_long
def test_separate_long_on_the_device():
    from models.conv_tasnet import ConvTasNet
    from oracle.make_golden import CONFIGS
    torch.manual_seed(5)
    model = ConvTasNet(**CONFIGS["tiny"]).cuda().eval()
    window, hop, T = 800, 400, 2300
    x = 0.1 * torch.randn(1, 1, T).cuda()
    got = model.separate_long(x, window)
    W = 5                                                                   # 4 x 400 + 800 = 2400 >= 2300 > 3 x 400 + 800
    padded = torch.nn.functional.pad(x, (0, (W - 1) * hop + window - T))
    wins = torch.stack([padded[0, :, w * hop:w * hop + window] for w in range(W)])        # sep_segment: window w is samples [w hop, w hop + window)
    with torch.no_grad():
        est = model(wins)
        want, perm_abs, _ = longform.stitch(est.view(1, W, 2, window), hop, T)
        assert tuple(got.shape) == (1, 2, T) and torch.equal(got, want)
        assert torch.equal(model.separate_long(x[0, 0], window, hop=hop), want[0])
        short = x[..., :window].contiguous()
        assert torch.equal(model.separate_long(short, window), model(short))
