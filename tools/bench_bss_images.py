"""BSS-eval v4 ("images") benchmark (utils/bss.py; csrc/bss.hip: sep_bss_xcorr, sep_bss_image_energies): museval's framewise SDR / ISR / SIR /
SAR of one MUSDB18-like track -- n = 4 stereo sources, filter length 512, window = hop = 44100 -- at T = 30 s and 240 s.  One JSON line per T:

    native_ms_median             utils.bss.bss_eval_images_batch on device tensors, HIP events around the whole call (checks, the two correlation
                                 calls, the solves, the image kernel, the copy of the result to the host); median of --reps after --warmup
    xcorr_rr_ms, xcorr_re_ms     sep_bss_xcorr alone: references x references at 1023 lags, references x estimates at 512 lags (n C = 8 rows each)
    solve_ms, solve_route        the dense solves alone (one (n C F)^2 = 4096^2 system and n (C F)^2 = 1024^2 systems) and where torch ran them
    image_kernel_ms              sep_bss_image_energies alone (its launch and its slab reduction)
    scratch_bytes                what the calls share: max(sep_bss_scratch_bytes(1, 8, 8, T, 512), sep_bss_image_scratch_bytes(...)); xcorr_scratch_bytes
                                 and image_scratch_bytes are the two terms
    host_ms                      the same metric as a host composition written HERE, not the code under test: correlations by FFT,
                                 numpy.linalg.solve, the FIR passes of every frame by FFT, fp64 numpy on the host's threads (host_threads).  Checked
                                 against the lstsq oracle of tests/test_bss_images_gpu.py at 1e-9 dB before it is timed.  Median of --host-reps.
    max_db_native_vs_host        largest difference of any frame's SDR / ISR / SIR / SAR between the two on the timed input

    python tools/bench_bss_images.py [--seconds 30,240] [--reps 5] [--warmup 1] [--host-reps 1] [--out profiles/r18_bss_images.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dnn-based_source_separation_amd", "src"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from bench_bss_eval import _event_times      # noqa: E402

N, C, FLEN, RATE = 4, 2, 512, 44100


def host_bss_images(ref, est, F, W, H):
    """(n, C, T) fp64 arrays -> (4, n, nwin) SDR, ISR, SIR, SAR: normal equations from FFT correlations, numpy.linalg.solve, FIR passes by FFT"""
    n, c, T = ref.shape
    nc = n * c
    nfft = 1 << int(np.ceil(np.log2(T + 2 * F)))                     # circular lags |lag| < F stay free of wrap-around
    R, E = np.fft.rfft(ref.reshape(nc, T), nfft), np.fft.rfft(est.reshape(nc, T), nfft)
    lag = (np.arange(F)[:, None] - np.arange(F)[None, :]) % nfft
    G, D = np.zeros((nc * F, nc * F)), np.zeros((nc * F, nc))
    for i in range(nc):
        for k in range(nc):
            G[i * F:(i + 1) * F, k * F:(k + 1) * F] = np.fft.irfft(np.conj(R[i]) * R[k], nfft)[lag]      # cc[p - q], cc[l] = sum_t r_i[t] r_k[t + l]
        D[i * F:(i + 1) * F] = np.fft.irfft(np.conj(R[i])[None] * E, nfft)[:, :F].T
    del R, E
    h_all = np.linalg.solve(G, D).reshape(nc, F, nc).transpose(2, 0, 1)                                  # [(j, c)][(k, c2)][tau]
    h_one = np.zeros((n, c, c, F))
    for j in range(n):
        blk = slice(j * c * F, (j + 1) * c * F)
        h_one[j] = np.linalg.solve(G[blk, blk], D[blk, j * c:(j + 1) * c]).reshape(c, F, c).transpose(2, 0, 1)
    del G, D
    Wx = W + F - 1
    nf = 1 << int(np.ceil(np.log2(Wx)))
    HA, HO = np.fft.rfft(h_all, nf), np.fft.rfft(h_one, nf)
    nwin = max(0, (T - W + H) // H) if T >= W else 0
    out = np.full((4, n, nwin), np.nan)
    db = lambda num, den: np.where(den == 0, np.inf, 10 * np.log10(num / np.where(den == 0, 1.0, den)))      # noqa: E731
    for w in range(nwin):
        r_w, e_w = ref[:, :, w * H:w * H + W], est[:, :, w * H:w * H + W]
        if not (r_w.sum(1) != 0).any(-1).all() or not (e_w.sum(1) != 0).any(-1).all():
            continue
        Rw = np.fft.rfft(r_w, nf)                                                                        # (n, c, nf / 2 + 1)
        p_all = np.fft.irfft(np.einsum("jkf,kf->jf", HA, Rw.reshape(nc, -1)), nf)[:, :Wx].reshape(n, c, Wx)
        p_j = np.fft.irfft(np.einsum("jcdf,jdf->jcf", HO, Rw), nf)[..., :Wx]
        s, e = np.zeros((n, c, Wx)), np.zeros((n, c, Wx))
        s[..., :W], e[..., :W] = r_w, e_w
        en = lambda x: np.sum(x ** 2, axis=(1, 2))                                                       # noqa: E731
        out[:, :, w] = [db(en(s), en(e - s)), db(en(s), en(p_j - s)), db(en(p_j), en(p_all - p_j)), db(en(p_all), en(e - p_all))]
    return out


def check_host_composition():
    """the host composition against the lstsq oracle of the tests at every shape of theirs: 1e-9 dB"""
    import test_bss_images_gpu as TG
    worst = 0.0
    for n, c, T, F, W, H in TG.SHAPES:
        ref, est = TG.make_case(n, c, T, F)
        got, want = host_bss_images(ref.double().numpy(), est.double().numpy(), F, W, H), TG.oracle(n, c, T, F, W, H)
        worst = max(worst, float(np.abs(got - want).max()))
    assert worst <= 1e-9, worst
    return worst


def make_track(T, seed=0):
    """(N, C, T) fp32 references of Gaussian noise and estimates: a random mixing of all channels plus noise plus a delayed leak of the other channel"""
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((N * C, T), dtype=np.float32)
    est = (np.eye(N * C) + 0.3 * rng.standard_normal((N * C, N * C))).astype(np.float32) @ ref + 0.1 * rng.standard_normal((N * C, T), dtype=np.float32)
    other = np.arange(N * C).reshape(N, C)[:, ::-1].reshape(-1)
    est[:, 3:] += 0.25 * ref[other, :-3]
    return ref.reshape(N, C, T), est.reshape(N, C, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", default="30,240")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bss_images.py measures on the GPU: none is visible")
    import sepkernels
    import utils.bss as bss
    K = sepkernels.backend()
    check = check_host_composition()
    print(json.dumps({"host_composition_max_db_vs_oracle": check}), flush=True)
    results = {"device": torch.cuda.get_device_name(0), "n_sources": N, "channels": C, "filter_length": FLEN, "window": RATE, "hop": RATE, "reps": args.reps,
               "warmup": args.warmup, "host_threads": os.environ.get("OMP_NUM_THREADS"), "host_composition_max_db_vs_oracle": check, "rows": []}
    nc = N * C
    for seconds in map(int, args.seconds.split(",")):
        T = seconds * RATE
        ref_np, est_np = make_track(T)
        ref, est = torch.from_numpy(ref_np)[None].cuda(), torch.from_numpy(est_np)[None].cuda()
        native = bss.bss_eval_images_batch(ref, est, None, RATE, RATE, FLEN)
        nwin = int(native[4][0])
        whole = _event_times(torch, lambda: bss.bss_eval_images_batch(ref, est, None, RATE, RATE, FLEN), args.reps, args.warmup)
        xc_bytes, im_bytes = K.bss_scratch_bytes(1, nc, nc, T, FLEN), K.bss_image_scratch_bytes(1, N, C, FLEN, RATE, nwin)
        scratch = torch.empty(max(xc_bytes, im_bytes) // 8, device="cuda", dtype=torch.float64)
        r2, e2 = ref.reshape(1, nc, T), est.reshape(1, nc, T)
        xrr = torch.empty(1, nc, nc, 2 * FLEN - 1, device="cuda", dtype=torch.float64)
        xre = torch.empty(1, nc, nc, FLEN, device="cuda", dtype=torch.float64)
        t_rr = _event_times(torch, lambda: K.bss_xcorr(r2, r2, None, xrr, scratch, 1, nc, nc, T, -(FLEN - 1), 2 * FLEN - 1), args.reps, args.warmup)
        t_re = _event_times(torch, lambda: K.bss_xcorr(r2, e2, None, xre, scratch, 1, nc, nc, T, 0, FLEN), args.reps, args.warmup)
        filt_all, filt_one = bss._image_filters(xrr, xre, N, C, FLEN)
        t_solve = _event_times(torch, lambda: bss._image_filters(xrr, xre, N, C, FLEN), args.reps, args.warmup)
        out = torch.empty(1, N, nwin, 9, device="cuda", dtype=torch.float64)
        t_img = _event_times(torch, lambda: K.bss_image_energies(ref, est, filt_all, filt_one, None, out, scratch, 1, N, C, T, FLEN, RATE, RATE, nwin),
                             args.reps, args.warmup)
        del scratch, xrr, xre
        host, got = [], None
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            got = host_bss_images(ref_np.astype(np.float64), est_np.astype(np.float64), FLEN, RATE, RATE)
            host.append(1e3 * (time.perf_counter() - t0))
        diff = max(float(np.abs(native[q][0].numpy() - got[q]).max()) for q in range(4))
        row = {"seconds": seconds, "T": T, "frames": nwin, "native_ms_median": round(whole[0], 3), "xcorr_rr_ms": round(t_rr[0], 3), "xcorr_re_ms": round(t_re[0], 3),
               "solve_ms": round(t_solve[0], 3), "solve_route": bss.solve_route(), "image_kernel_ms": round(t_img[0], 3), "scratch_bytes": max(xc_bytes, im_bytes),
               "xcorr_scratch_bytes": xc_bytes, "image_scratch_bytes": im_bytes, "host_ms": round(sorted(host)[len(host) // 2], 3), "host_reps": args.host_reps,
               "max_db_native_vs_host": diff}
        print(json.dumps(row), flush=True)
        results["rows"].append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
