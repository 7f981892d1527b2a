"""GPU: BSS-eval v4 ("images") -- museval's framewise SDR, ISR, SIR, SAR -- on the device (utils/bss.py; csrc/bss.hip: sep_bss_image_energies).

(a) the kernel's nine sums per (source, frame) against an fp64 numpy restatement of its contract in include/sepkernels.h with GIVEN filters
    (numpy.convolve per frame segment) at 1e-12 relative: the kernel is fp64, only the order of summation differs.  The case functions take
    their device through the hooks below, so tests/test_bss_images_cpu.py runs the same functions on an emulator and on the host simulation of
    the kernel source.
(b) the metric end to end against an oracle that is NOT the normal equations: the explicit (T + F - 1, n C F) matrix of delayed reference
    channels, every filter by numpy.linalg.lstsq, the FIR passes by numpy.convolve per frame segment, the ratios from the signals.  1e-9 dB,
    the project's fp64 bar: the delayed-reference matrices of these inputs have condition numbers 1.8 to 6.3, so the normal equations lose
    cond^2 < 40 of the 1e-16; a normal-equations route in numpy and this oracle differ by at most 6e-14 dB on them.
(c) batch with lengths = the single calls bitwise; two runs give the same bits; a row's bits do not depend on the pitch or its neighbours; the
    silent-frame rule; the call recorded in a Sequence replays to the same bits.
Agreement with the museval PACKAGE is not tested (it is on none of the project's machines): these tests pin the definition."""
import functools

import numpy as np
import pytest
import torch

import sepkernels

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
to_device = lambda t: t.cuda()                      # noqa: E731
device_sync = lambda: torch.cuda.synchronize()      # noqa: E731

# (n, C, T, F, W, H): basic stereo; mono with overlapping frames and a dropped trailing partial frame; four stereo sources; a frame shorter than
# the filter; the production filter length (two 256-tap tiles, two 1024-sample slabs per frame)
SHAPES = [(2, 2, 300, 8, 100, 100), (3, 1, 257, 16, 64, 48), (4, 2, 1100, 32, 256, 256), (2, 2, 600, 64, 40, 40), (2, 2, 4000, 512, 1500, 1500)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


def num_frames(T, W, H):
    return max(0, (T - W + H) // H) if T >= W else 0


@functools.lru_cache(maxsize=None)
def make_case(n, C, T, F):
    """-> references, estimates (n, C, T) fp32 tensors.  References: seeded Gaussian noise rounded to fp32.  Estimates: a random mixing of the
    references (identity plus 0.3 randn over all n C channels), plus 0.1 noise, plus a leak of the source's other channel (the next source's
    channel when mono) delayed by 3 samples."""
    rng = np.random.default_rng(411 + 7 * n + 3 * C + T + F)
    ref = rng.standard_normal((n * C, T)).astype(np.float32).astype(np.float64)
    est = (np.eye(n * C) + 0.3 * rng.standard_normal((n * C, n * C))) @ ref + 0.1 * rng.standard_normal((n * C, T))
    other = np.arange(n * C).reshape(n, C)[:, ::-1].reshape(-1) if C > 1 else np.roll(np.arange(n), -1)
    est[:, 3:] += 0.25 * ref[other, :-3]
    return torch.from_numpy(ref.astype(np.float32)).reshape(n, C, T), torch.from_numpy(est.astype(np.float32)).reshape(n, C, T)


def _db(num, den):
    return np.inf if den == 0 else 10 * np.log10(num / den)


def frame_sums(r_w, e_w, fa, fo, j):
    """the nine sums of source j on one frame segment r_w, e_w (n, C, W) with filters fa (C, n C, F) = h_all[j], fo (C, C, F) = h_one[j]"""
    n, C, W = r_w.shape
    F = fa.shape[-1]
    rc = r_w.reshape(n * C, W)
    v = np.zeros(9)
    for c in range(C):
        s, e = np.zeros(W + F - 1), np.zeros(W + F - 1)
        s[:W], e[:W] = r_w[j, c], e_w[j, c]
        p_all = sum(np.convolve(fa[c, kc], rc[kc]) for kc in range(n * C))
        p_j = sum(np.convolve(fo[c, c2], r_w[j, c2]) for c2 in range(C))
        for q, x in enumerate((s, e - s, p_j - s, p_j, p_all - p_j, p_all, e - p_all)):
            v[q] += np.sum(x ** 2)
    v[7], v[8] = np.count_nonzero(r_w[j].sum(0)), np.count_nonzero(e_w[j].sum(0))
    return v


def sums_reference(ref, est, fa, fo, lengths, W, H, nwin):
    """ref, est (B, n, C, T) fp64, fa (B, n, C, n C, F), fo (B, n, C, C, F) -> (B, n, nwin, 9), zeros at and beyond a row's frame count"""
    B, n, C, T = ref.shape
    out = np.zeros((B, n, nwin, 9))
    for b in range(B):
        Tb = T if lengths is None else lengths[b]
        for w in range(min(nwin, num_frames(Tb, W, H))):
            for j in range(n):
                out[b, j, w] = frame_sums(ref[b, :, :, w * H:w * H + W], est[b, :, :, w * H:w * H + W], fa[b, j], fo[b, j], j)
    return out


def call_image_energies(ref, est, fa, fo, lengths, W, H, nwin):
    """numpy in, numpy out through HIP.bss_image_energies on NaN-filled out and scratch of exactly the size the library asks for"""
    B, n, C, T = ref.shape
    F = fa.shape[-1]
    f32 = lambda x: to_device(torch.from_numpy(x).float().contiguous())          # noqa: E731
    f64 = lambda x: to_device(torch.from_numpy(x).contiguous())                  # noqa: E731
    ln = None if lengths is None else to_device(torch.tensor(lengths, dtype=torch.int32))
    nbytes = HIP.bss_image_scratch_bytes(B, n, C, F, W, nwin)
    assert nbytes >= 72 * B * n * nwin * ((W + F - 1 + 1023) // 1024)
    scratch = to_device(torch.full((max(1, nbytes // 8),), float("nan"), dtype=torch.float64))
    out = to_device(torch.full((B, n, nwin, 9), float("nan"), dtype=torch.float64))
    HIP.bss_image_energies(f32(ref), f32(est), f64(fa), f64(fo), ln, out, scratch, B, n, C, T, F, W, H, nwin)
    device_sync()
    return out.cpu().numpy()


def case_sums(n, C, T, F, W, H, batch=True):
    """two rows, the second shorter (NaN beyond its length: reading it shows), random filters, one frame more than any row has"""
    rng = np.random.default_rng(3000 + T + F + W)
    B = 2 if batch else 1
    ref = rng.standard_normal((B, n, C, T)).astype(np.float32).astype(np.float64)
    est = rng.standard_normal((B, n, C, T)).astype(np.float32).astype(np.float64)
    fa = rng.standard_normal((B, n, C, n * C, F)) / np.sqrt(F * n * C)
    fo = rng.standard_normal((B, n, C, C, F)) / np.sqrt(F * C)
    lengths = [T, T - H - 1][:B] if batch else None
    if lengths is not None:
        ref[1, :, :, lengths[1]:] = np.nan
        est[1, :, :, lengths[1]:] = np.nan
        ref[0, 0, :, H:H + 3] = 0.0                                    # the counts are not all W
        est[0, n - 1, :, 5] = 0.0
    nwin = num_frames(T, W, H) + 1
    got = call_image_energies(ref, est, fa, fo, lengths, W, H, nwin)
    want = sums_reference(ref, est, fa, fo, lengths, W, H, nwin)
    assert np.isfinite(got).all()
    assert (got[..., 7:] == want[..., 7:]).all(), "the silence counts are exact"
    live = want[..., :7] > 0
    assert (got[..., :7][~live] == 0.0).all(), "frames beyond a row's count are written as zeros"
    err = np.abs(got[..., :7][live] - want[..., :7][live]) / want[..., :7][live]
    print("image sums {}: max relative error {:.3e} over {} sums".format((n, C, T, F, W, H), err.max(), err.size))
    assert err.max() <= 1e-12, err.max()
    return got


def oracle_arrays(ref, est, F, W, H):
    """ref, est (n, C, T) fp64 arrays -> (4, n, nwin): SDR, ISR, SIR, SAR per source and frame, straight from the definition"""
    n, C, T = ref.shape
    nc, Tx = n * C, T + F - 1
    M = np.zeros((Tx, nc * F))
    for kc in range(nc):
        for tau in range(F):
            M[tau:tau + T, kc * F + tau] = ref.reshape(nc, T)[kc]
    E = np.zeros((Tx, nc))
    E[:T] = est.reshape(nc, T).T
    h_all = np.linalg.lstsq(M, E, rcond=None)[0].T.reshape(n, C, nc, F)                       # [j][c][(k, c2)][tau]
    h_one = np.zeros((n, C, C, F))
    for j in range(n):
        cols = slice(j * C * F, (j + 1) * C * F)
        h_one[j] = np.linalg.lstsq(M[:, cols], E[:, j * C:(j + 1) * C], rcond=None)[0].T.reshape(C, C, F)
    nwin = num_frames(T, W, H)
    out = np.full((4, n, nwin), np.nan)
    for w in range(nwin):
        r_w, e_w = ref[:, :, w * H:w * H + W], est[:, :, w * H:w * H + W]
        if any(not r_w[i].sum(0).any() for i in range(n)) or any(not e_w[i].sum(0).any() for i in range(n)):
            continue                                                   # some source silent: NaN for every source
        for j in range(n):
            v = frame_sums(r_w, e_w, h_all[j], h_one[j], j)
            out[:, j, w] = [_db(v[0], v[1]), _db(v[0], v[2]), _db(v[3], v[4]), _db(v[5], v[6])]
    return out


@functools.lru_cache(maxsize=None)
def oracle(n, C, T, F, W, H):
    ref, est = make_case(n, C, T, F)
    return oracle_arrays(ref.double().numpy(), est.double().numpy(), F, W, H)


def check_close(got, want, tol=1e-9, what=""):
    """got: sdr, isr, sir, sar tensors (n, nwin); want (4, n, nwin): NaN where and only where the oracle has NaN, the rest within tol dB"""
    worst = 0.0
    for g, w in zip(got, want):
        assert g.dtype == torch.float64 and not g.is_cuda and tuple(g.shape) == w.shape, (g.dtype, g.shape, w.shape)
        g = g.numpy()
        assert (np.isnan(g) == np.isnan(w)).all(), (what, g, w)
        ok = ~np.isnan(w)
        assert (np.isinf(g[ok]) == np.isinf(w[ok])).all(), (what, g, w)
        fin = ok & np.isfinite(w)
        if fin.any():
            worst = max(worst, np.abs(g[fin] - w[fin]).max())
    print("bss_eval_images {}: max |dB - oracle| = {:.3e}".format(what, worst))
    assert worst <= tol, worst
    return worst


def check_metric(bss, dev, shape):
    n, C, T, F, W, H = shape
    ref, est = make_case(n, C, T, F)
    want = oracle(*shape)
    assert np.isfinite(want).all() and want.shape[2] == num_frames(T, W, H) >= 2
    if C == 1:                                                          # the (n, T) form of mono signals
        got = bss.bss_eval_images(ref[:, 0].to(dev), est[:, 0].to(dev), W, H, filter_length=F)
    elif F == 512:                                                      # the default filter length
        got = bss.bss_eval_images(ref.to(dev), est.to(dev), W, H)
    else:
        got = bss.bss_eval_images_batch(ref[None].to(dev), est[None].to(dev), None, W, H, F)
        assert got[4].tolist() == [want.shape[2]]
        got = [v[0] for v in got[:4]]
    return check_close(got, want, what=str(shape))


def check_batch_equals_single_calls(bss, dev):
    """rows of 300 and 200 samples in one (2, 2, 2, 300) batch against the two single calls: the same bits, NaN beyond the shorter row's frames"""
    F, W, H = 8, 64, 48
    r0, e0 = make_case(2, 2, 300, 8)
    r1, e1 = make_case(2, 2, 200, 8)
    ref, est = torch.full((2, 2, 2, 300), float("nan")), torch.full((2, 2, 2, 300), float("nan"))
    ref[0], est[0], ref[1, :, :, :200], est[1, :, :, :200] = r0, e0, r1, e1
    batch = bss.bss_eval_images_batch(ref.to(dev), est.to(dev), [300, 200], W, H, F)
    assert batch[4].tolist() == [num_frames(300, W, H), num_frames(200, W, H)] == [5, 3]
    for b, (r, e) in enumerate(((r0, e0), (r1, e1))):
        single = bss.bss_eval_images_batch(r[None].to(dev), e[None].to(dev), None, W, H, F)
        k = int(single[4][0])
        for x, y in zip(batch[:4], single[:4]):
            assert torch.isfinite(y).all() and torch.equal(x[b, :, :k], y[0]) and torch.isnan(x[b, :, k:]).all(), (b, x[b], y[0])


def check_silent_frames(bss, dev):
    """each of the three ways a frame is silent blanks that frame for EVERY source and leaves its neighbours as the oracle has them"""
    n, C, T, F, W, H = SHAPES[0]
    for kind in ("reference", "estimate", "L = -R"):
        ref, est = (x.clone() for x in make_case(n, C, T, F))
        if kind == "reference":
            ref[1, :, W:2 * W] = 0
        elif kind == "estimate":
            est[0, :, W:2 * W] = 0
        else:
            ref[0, 1, W:2 * W] = -ref[0, 0, W:2 * W]
        want = oracle_arrays(ref.double().numpy(), est.double().numpy(), F, W, H)
        assert np.isnan(want[:, :, 1]).all() and np.isfinite(want[:, :, [0, 2]]).all()
        got = bss.bss_eval_images(ref.to(dev), est.to(dev), W, H, filter_length=F)
        check_close(got, want, what="silent " + kind)


# ---------------------------------------------------------------------------------------------------------------- the tests on the device
@pytest.fixture()
def native(monkeypatch):
    monkeypatch.setenv("SEPK_BSS_EVAL", "native")
    import utils.bss as bss
    return bss


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_nine_sums_match_the_restatement(shape):
    case_sums(*shape)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_metric_on_the_device_matches_the_definition(native, shape):
    check_metric(native, "cuda", shape)
    print("dense solves ran on the", native.solve_route())
    assert native.solve_route() in ("device", "host")


def test_batch_with_lengths_equals_the_single_calls(native):
    check_batch_equals_single_calls(native, "cuda")


def test_two_runs_give_the_same_bits(native):
    n, C, T, F, W, H = SHAPES[2]
    ref, est = (x[None].cuda() for x in make_case(n, C, T, F))
    a, b = (native.bss_image_energies_batch(ref, est, None, W, H, F)[0] for _ in range(2))
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert np.array_equal(case_sums(*SHAPES[3]), case_sums(*SHAPES[3]))


def test_a_rows_bits_do_not_depend_on_pitch_or_neighbours():
    n, C, T, F, W, H = SHAPES[0]
    rng = np.random.default_rng(5)
    ref = rng.standard_normal((1, n, C, T)).astype(np.float32).astype(np.float64)
    est = rng.standard_normal((1, n, C, T)).astype(np.float32).astype(np.float64)
    fa, fo = rng.standard_normal((1, n, C, n * C, F)), rng.standard_normal((1, n, C, C, F))
    nwin = num_frames(T, W, H)
    alone = call_image_energies(ref, est, fa, fo, None, W, H, nwin)
    wide = lambda x: np.concatenate([np.concatenate([rng.standard_normal(x.shape), x, rng.standard_normal(x.shape)]),       # noqa: E731
                                     np.full((3, n, C, 1234), np.nan)], -1)
    rep = lambda f: np.concatenate([rng.standard_normal(f.shape), f, rng.standard_normal(f.shape)])                         # noqa: E731
    among = call_image_energies(wide(ref), wide(est), rep(fa), rep(fo), [T + 1234, T, 50], W, H, nwin + 12)
    assert np.array_equal(among[1, :, :nwin], alone[0]) and (among[1, :, nwin:] == 0).all() and (among[2] == 0).all()


def test_silent_frames(native):
    check_silent_frames(native, "cuda")


def test_the_call_records_in_a_sequence_and_replays_to_the_same_bits():
    n, C, T, F, W, H = SHAPES[0]
    g = torch.Generator().manual_seed(9)
    ref, est = torch.randn(1, n, C, T, generator=g).cuda(), torch.randn(1, n, C, T, generator=g).cuda()
    fa = torch.randn(1, n, C, n * C, F, generator=g, dtype=torch.float64).cuda()
    fo = torch.randn(1, n, C, C, F, generator=g, dtype=torch.float64).cuda()
    nwin = num_frames(T, W, H)
    scratch = torch.empty(HIP.bss_image_scratch_bytes(1, n, C, F, W, nwin) // 8, dtype=torch.float64, device="cuda")
    eager = torch.full((1, n, nwin, 9), float("nan"), dtype=torch.float64, device="cuda")
    HIP.bss_image_energies(ref, est, fa, fo, None, eager, scratch, 1, n, C, T, F, W, H, nwin)
    out = torch.full_like(eager, float("nan"))
    seq = sepkernels.Sequence()
    with sepkernels.recording(seq):
        HIP.bss_image_energies(ref, est, fa, fo, None, out, scratch, 1, n, C, T, F, W, H, nwin)
    assert len(seq) == 1
    out.fill_(float("nan"))
    seq.run()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.equal(out, eager)
