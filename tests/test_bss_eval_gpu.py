"""GPU: BSS-eval v3 ("sources") -- SDR, SIR, SAR -- on the device (utils/bss.py; csrc/bss.hip: sep_bss_xcorr, sep_bss_energies).

(a) the two kernels, case by case, against fp64 numpy restatements of their contract in include/sepkernels.h at 1e-12 relative (the kernels
    are fp64, only the order of summation differs): the lagged correlations against sums over explicitly zero-padded signals, the energies
    against the product with the explicit matrix of delayed references.  The case functions take their device through the hooks below, so
    tests/test_bss_eval_cpu.py runs the same functions on the host simulation of the kernel sources.
(b) the metric end to end against an oracle that is NOT the normal equations: the (T + flen - 1, n flen) matrix of delayed references is
    built explicitly, every projection is numpy.linalg.lstsq on it, the three ratios are formed from the projected signals.  1e-9 dB, the
    project's fp64 bar (both routes in exact arithmetic give the same projection; in fp64 the normal equations lose cond(G) ~ 4e3 of the
    1e-16, far inside the bar), and the permutation.
(c) two runs give the same bits; the batch form with a length per row gives what the single calls give.
Agreement with the mir_eval PACKAGE is not tested (it is on none of the project's machines): these tests pin the published definition."""
import functools
import itertools

import numpy as np
import pytest
import torch

import sepkernels

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
to_device = lambda t: t.cuda()                      # noqa: E731
device_sync = lambda: torch.cuda.synchronize()      # noqa: E731

# (B, n, m, T, flen, lengths): the issue's four -- the third has every lag beyond the signal, the fourth a T one past the 2048-sample slab --
# plus n != m (the index order of out) and more lags than one workgroup's 256
XCORR_CASES = [(2, 2, 2, 700, 32, None), (2, 2, 2, 700, 32, [700, 131]), (1, 1, 1, 20, 32, None), (1, 2, 2, 2049, 16, None),
               (1, 2, 3, 300, 8, None), (1, 1, 1, 600, 200, None)]
# ... the issue's two, an output length (T + flen - 1 = 1025) one past the 1024-sample slab, and a filter longer than one 256-tap tile
ENERGY_CASES = [(2, 2, 2, 700, 32, None), (2, 2, 2, 700, 32, [700, 131]), (1, 2, 2, 1010, 16, None), (1, 1, 2, 300, 300, None)]
# (n, T, flen) of the end-to-end cases
SHAPES = [(3, 257, 16), (2, 700, 32), (4, 513, 8), (2, 4000, 512)]


def _audio(rng, *shape):
    """fp32-representable white noise through x[t] += 0.9 x[t-1], as fp64"""
    x = rng.standard_normal(shape)
    for t in range(1, shape[-1]):
        x[..., t] += 0.9 * x[..., t - 1]
    return x.astype(np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- (a) the kernels
def xcorr_reference(a, c, lengths, lag_lo, nlag):
    """out[b][i][k][l] = sum_t a[b][i][t] c[b][k][t + lag_lo + l] with c zero outside [0, T_b): plain sums over a zero-padded copy"""
    B, n, T = a.shape
    m = c.shape[1]
    pad = abs(lag_lo) + nlag + T
    out = np.zeros((B, n, m, nlag))
    for b in range(B):
        Tb = T if lengths is None else lengths[b]
        cp = np.zeros((m, Tb + 2 * pad))
        cp[:, pad:pad + Tb] = c[b, :, :Tb]
        for i in range(n):
            for k in range(m):
                for l in range(nlag):
                    out[b, i, k, l] = np.sum(a[b, i, :Tb] * cp[k, pad + lag_lo + l:pad + lag_lo + l + Tb])
    return out


def _call_xcorr(a, c, lengths, lag_lo, nlag, flen):
    B, n, T = a.shape
    m = c.shape[1]
    dev = lambda x: to_device(torch.from_numpy(x).float().contiguous())          # noqa: E731
    ln = None if lengths is None else to_device(torch.tensor(lengths, dtype=torch.int32))
    nbytes = HIP.bss_scratch_bytes(B, max(n, m), max(n, m), T, flen)
    assert nbytes >= 8 * B * n * m * ((T + 2047) // 2048) * nlag
    scratch = to_device(torch.full((nbytes // 8,), float("nan"), dtype=torch.float64))
    out = to_device(torch.full((B, n, m, nlag), float("nan"), dtype=torch.float64))
    HIP.bss_xcorr(dev(a), dev(c), ln, out, scratch, B, n, m, T, lag_lo, nlag)
    device_sync()
    return out.cpu().numpy()


def case_xcorr(B, n, m, T, flen, lengths):
    rng = np.random.default_rng(1000 + T + flen)
    a, c = _audio(rng, B, n, T), _audio(rng, B, m, T)
    if lengths is not None:                          # what lies beyond a row's length must not matter: poison it
        for b, Tb in enumerate(lengths):
            a[b, :, Tb:] = np.nan
            c[b, :, Tb:] = np.nan
    for lag_lo, nlag in ((-(flen - 1), 2 * flen - 1), (0, flen)):
        got = _call_xcorr(a, c, lengths, lag_lo, nlag, flen)
        want = xcorr_reference(a, c, lengths, lag_lo, nlag)
        for b in range(B):
            Tb = T if lengths is None else lengths[b]
            # 1e-12 relative to the Cauchy-Schwarz bound of every lag of the pair (a lag's own value can be any small number by cancellation)
            scale = np.sqrt((a[b, :, :Tb] ** 2).sum(-1))[:, None, None] * np.sqrt((c[b, :, :Tb] ** 2).sum(-1))[None, :, None]
            err = np.abs(got[b] - want[b]) / scale
            assert np.isfinite(got[b]).all() and err.max() <= 1e-12, (B, n, m, T, flen, lag_lo, b, err.max())
            lags = lag_lo + np.arange(nlag)
            empty = np.abs(lags) >= Tb
            assert (got[b][:, :, empty] == 0.0).all(), "a lag without overlap must be exactly 0"
    return got


def energies_reference(ref, est, fa, fo, lengths):
    """the contract of sep_bss_energies through the explicit (T_b + flen - 1, flen) matrix of delayed copies of every reference"""
    B, n, T = ref.shape
    m, flen = est.shape[1], fa.shape[-1]
    out = np.zeros((B, m, n, 5))
    for b in range(B):
        Tb = T if lengths is None else lengths[b]
        Tx = Tb + flen - 1
        delayed = np.zeros((n, Tx, flen))
        for k in range(n):
            for tau in range(flen):
                delayed[k, tau:tau + Tb, tau] = ref[b, k, :Tb]
        for j in range(m):
            e = np.zeros(Tx)
            e[:Tb] = est[b, j, :Tb]
            p_all = sum(delayed[k] @ fa[b, j, k] for k in range(n))
            for i in range(n):
                s = delayed[i] @ fo[b, j, i]
                interf, artif = p_all - s, e - p_all
                out[b, j, i] = [np.sum(v ** 2) for v in (s, interf, artif, interf + artif, s + interf)]
    return out


def case_energies(B, n, m, T, flen, lengths):
    rng = np.random.default_rng(2000 + T + flen)
    ref, est = _audio(rng, B, n, T), _audio(rng, B, m, T)
    fa, fo = rng.standard_normal((B, m, n, flen)) / np.sqrt(flen), rng.standard_normal((B, m, n, flen)) / np.sqrt(flen)
    if lengths is not None:
        for b, Tb in enumerate(lengths):
            ref[b, :, Tb:] = np.nan
            est[b, :, Tb:] = np.nan
    f32 = lambda x: to_device(torch.from_numpy(x).float().contiguous())          # noqa: E731
    f64 = lambda x: to_device(torch.from_numpy(x).contiguous())                  # noqa: E731
    ln = None if lengths is None else to_device(torch.tensor(lengths, dtype=torch.int32))
    nbytes = HIP.bss_scratch_bytes(B, n, m, T, flen)
    assert nbytes >= 40 * B * n * m * ((T + flen - 1 + 1023) // 1024)
    scratch = to_device(torch.full((nbytes // 8,), float("nan"), dtype=torch.float64))
    out = to_device(torch.full((B, m, n, 5), float("nan"), dtype=torch.float64))
    HIP.bss_energies(f32(ref), f32(est), f64(fa), f64(fo), ln, out, scratch, B, n, m, T, flen)
    device_sync()
    got, want = out.cpu().numpy(), energies_reference(ref, est, fa, fo, lengths)
    err = np.abs(got - want) / want
    assert np.isfinite(got).all() and err.max() <= 1e-12, (B, n, m, T, flen, err.max())


@pytest.mark.parametrize("case", XCORR_CASES, ids=[str(i) for i in range(len(XCORR_CASES))])
def test_xcorr_kernel_matches_the_direct_sums(case):
    case_xcorr(*case)


@pytest.mark.parametrize("case", ENERGY_CASES, ids=[str(i) for i in range(len(ENERGY_CASES))])
def test_energies_kernel_matches_the_delayed_matrix_product(case):
    case_energies(*case)


# ---------------------------------------------------------------------------------------------------------------- (b) end to end
@functools.lru_cache(maxsize=None)
def make_case(n, T, flen):
    """-> reference, estimates (n, T) fp32 tensors.  References: white noise through x[t] += 0.9 x[t-1].  Estimates: A refs + 0.1 noise with
    A = I + 0.2 randn -- at the production filter length 5-tap mixtures (identity plus 0.2 randn per tap) plus 0.05 noise -- and handed over
    in ANOTHER order than the references, so the permutation to be found is not the identity."""
    rng = np.random.default_rng(77 + n + T + flen)
    ref = _audio(rng, n, T)
    if flen == 512:
        taps = 0.2 * rng.standard_normal((n, n, 5))
        taps[np.arange(n), np.arange(n), 0] += 1.0
        est = np.stack([sum(np.convolve(ref[i], taps[j, i])[:T] for i in range(n)) for j in range(n)]) + 0.05 * rng.standard_normal((n, T))
    else:
        est = (np.eye(n) + 0.2 * rng.standard_normal((n, n))) @ ref + 0.1 * rng.standard_normal((n, T))
    order = np.roll(np.arange(n), 1)
    return torch.from_numpy(ref.astype(np.float32)), torch.from_numpy(est[order].astype(np.float32))


def _ratio_db(num, den):
    return np.inf if den == 0 else 10 * np.log10(num / den)


def oracle_pairs(ref, est, flen):
    """(n, T) fp64 arrays -> sdr, sir, sar [estimate j][reference i] straight from the definition: explicit delayed-reference matrix, lstsq
    projections, energy ratios of the projected signals"""
    n, T = ref.shape
    Tx = T + flen - 1
    M = np.zeros((Tx, n * flen))
    for i in range(n):
        for tau in range(flen):
            M[tau:tau + T, i * flen + tau] = ref[i]
    E = np.zeros((Tx, n))
    E[:T] = est.T
    p_all = M @ np.linalg.lstsq(M, E, rcond=None)[0]
    sdr, sir, sar = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        Mi = M[:, i * flen:(i + 1) * flen]
        s = Mi @ np.linalg.lstsq(Mi, E, rcond=None)[0]
        for j in range(n):
            interf, artif = p_all[:, j] - s[:, j], E[:, j] - p_all[:, j]
            sdr[j, i] = _ratio_db(np.sum(s[:, j] ** 2), np.sum((interf + artif) ** 2))
            sir[j, i] = _ratio_db(np.sum(s[:, j] ** 2), np.sum(interf ** 2))
            sar[j, i] = _ratio_db(np.sum((s[:, j] + interf) ** 2), np.sum(artif ** 2))
    return sdr, sir, sar


@functools.lru_cache(maxsize=None)
def oracle(n, T, flen, compute_permutation=True):
    """-> sdr, sir, sar, perm (n,) of make_case(n, T, flen), and the margin in mean SIR between the best and the second-best permutation"""
    ref, est = make_case(n, T, flen)
    sdr, sir, sar = oracle_pairs(ref.double().numpy(), est.double().numpy(), flen)
    true = np.arange(n)
    if not compute_permutation:
        return sdr[true, true], sir[true, true], sar[true, true], true, None
    perms = list(itertools.permutations(range(n)))
    means = np.array([sir[list(p), true].mean() for p in perms])
    best = int(np.argmax(means))
    perm = np.array(perms[best])
    return sdr[perm, true], sir[perm, true], sar[perm, true], perm, means[best] - np.sort(means)[-2]


def check_against_oracle(got, n, T, flen, compute_permutation=True, tol=1e-9):
    sdr, sir, sar, perm = got
    want = oracle(n, T, flen, compute_permutation)
    assert sdr.dtype == sir.dtype == sar.dtype == torch.float64 and perm.dtype == torch.int64 and not sdr.is_cuda and not perm.is_cuda
    assert perm.tolist() == want[3].tolist(), (perm.tolist(), want[3].tolist())
    worst = max(np.abs(g.numpy() - w).max() for g, w in zip((sdr, sir, sar), want[:3]))
    print("bss_eval (n={}, T={}, flen={}): max |dB - oracle| = {:.3e}, permutation {} (margin {} dB)".format(
        n, T, flen, worst, perm.tolist(), None if want[4] is None else round(float(want[4]), 2)))
    assert all(np.isfinite(w).all() for w in want[:3]) and worst <= tol, worst
    return worst


@pytest.fixture()
def native(monkeypatch):
    monkeypatch.setenv("SEPK_BSS_EVAL", "native")
    import utils.bss as bss
    return bss


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_metric_on_the_device_matches_the_definition(native, shape):
    n, T, flen = shape
    ref, est = make_case(n, T, flen)
    if flen == 512:
        got = native.bss_eval_sources(ref, est)                      # the drop-in entry point at mir_eval's fixed filter length, CPU tensors in
    else:
        got = [v[0] for v in native.bss_eval_sources_batch(ref[None].cuda(), est[None].cuda(), filter_length=flen)]
    print("dense solves ran on the", native.solve_route())
    assert native.solve_route() in ("device", "host")
    check_against_oracle(got, n, T, flen)


def test_two_runs_give_the_same_bits(native):
    ref, est = make_case(2, 700, 32)
    a = native.bss_eval_sources_batch(ref[None].cuda(), est[None].cuda(), filter_length=32)
    b = native.bss_eval_sources_batch(ref[None].cuda(), est[None].cuda(), filter_length=32)
    ea = native.bss_energies_batch(ref[None].cuda(), est[None].cuda(), filter_length=32)
    eb = native.bss_energies_batch(ref[None].cuda(), est[None].cuda(), filter_length=32)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and torch.equal(ea, eb)


def check_batch_equals_single_calls(bss, dev):
    """rows of 700 and 257 samples in one (2, 2, 700) batch against the two single calls: the same bits"""
    r0, e0 = make_case(2, 700, 32)
    r1, e1 = (x[:2, :257].contiguous() for x in make_case(3, 257, 16))
    ref, est = torch.full((2, 2, 700), float("nan")), torch.full((2, 2, 700), float("nan"))
    ref[0], est[0], ref[1, :, :257], est[1, :, :257] = r0, e0, r1, e1
    batch = bss.bss_eval_sources_batch(ref.to(dev), est.to(dev), lengths=[700, 257], filter_length=32)
    for b, (r, e) in enumerate(((r0, e0), (r1, e1))):
        single = bss.bss_eval_sources_batch(r[None].to(dev), e[None].to(dev), filter_length=32)
        for x, y in zip(batch, single):
            assert torch.isfinite(y.double()).all() and torch.equal(x[b], y[0]), (b, x[b], y[0])


def test_batch_with_lengths_equals_the_single_calls(native):
    check_batch_equals_single_calls(native, "cuda")


def test_compute_permutation_off_scores_in_the_given_order(native):
    ref, est = make_case(3, 257, 16)
    got = [v[0] for v in native.bss_eval_sources_batch(ref[None].cuda(), est[None].cuda(), filter_length=16, compute_permutation=False)]
    check_against_oracle(got, 3, 257, 16, compute_permutation=False)
