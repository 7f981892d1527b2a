"""BSS-eval benchmark (utils/bss.py; csrc/bss.hip: sep_bss_xcorr, sep_bss_energies): SDR / SIR / SAR of n = 2 sources at the production
filter length 512, T = 32000 and 80000 samples (4 s and 10 s at 8 kHz), B = 1 and B = 16 utterances per call.  One JSON line per (T, B):

    native_ms_median / _p99      utils.bss.bss_eval_sources_batch on device tensors, HIP events around the whole call (checks, kernels, solves,
                                 the copy of the result to the host), synchronised per call; median of --reps (50) after --warmup (5)
    kernels_ms_median            the two sep_bss_xcorr calls and sep_bss_energies alone (four launches of ours plus their two reductions)
    solve_ms_median, solve_route the dense solves alone (per row one (n flen)^2 system and n flen^2 systems) and where torch ran them
    host_ms_median               the same metric as the usual host composition -- correlations and FIR passes by FFT, numpy.linalg.solve, fp64
                                 numpy / scipy on the host's threads (host_threads) -- for the B utterances one after the other; what the
                                 mir_eval route would cost.  Written here, not the code under test, and checked against the lstsq oracle of
                                 tests/test_bss_eval_gpu.py at 1e-9 dB before it is timed.  Median of --host-reps (5) after one warm-up.
    max_db_native_vs_host        largest difference of any SDR / SIR / SAR between the two on the timed input (row 0)

    python tools/bench_bss_eval.py [--lengths 32000,80000] [--batches 1,16] [--reps 50] [--warmup 5] [--host-reps 5] [--out FILE]
"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dnn-based_source_separation_amd", "src"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FLEN = 512


def host_bss_eval(ref, est, flen=FLEN):
    """(n, T) fp64 arrays -> sdr, sir, sar, perm: the normal equations with every correlation and every FIR pass through the FFT"""
    import scipy.linalg
    n, T = ref.shape
    Tx = T + flen - 1
    nfft = 1 << int(np.ceil(np.log2(Tx + flen)))                   # circular lags |lag| < flen stay free of wrap-around
    R, E = np.fft.rfft(ref, nfft), np.fft.rfft(est, nfft)
    G = np.zeros((n * flen, n * flen))
    D = np.zeros((n * flen, n))
    for i in range(n):
        for k in range(n):
            cc = np.fft.irfft(np.conj(R[i]) * R[k], nfft)            # cc[lag] = sum_t r_i[t] r_k[t + lag]
            G[i * flen:(i + 1) * flen, k * flen:(k + 1) * flen] = scipy.linalg.toeplitz(cc[:flen], np.concatenate(([cc[0]], cc[:-flen:-1])))
        D[i * flen:(i + 1) * flen] = np.fft.irfft(np.conj(R[i])[None] * E, nfft)[:, :flen].T
    try:
        C = np.linalg.solve(G, D)
    except np.linalg.LinAlgError:
        C = np.linalg.lstsq(G, D, rcond=None)[0]
    e = np.zeros((n, Tx))
    e[:, :T] = est
    p_all = sum(np.fft.irfft(np.fft.rfft(C[k * flen:(k + 1) * flen].T, nfft) * R[k][None], nfft)[:, :Tx] for k in range(n))      # (estimate j, Tx)
    db = lambda num, den: np.inf if den == 0 else 10 * np.log10(num / den)      # noqa: E731
    sdr, sir, sar = np.zeros((n, n)), np.zeros((n, n)), np.zeros((n, n))
    for i in range(n):
        blk = slice(i * flen, (i + 1) * flen)
        try:
            Ci = np.linalg.solve(G[blk, blk], D[blk])
        except np.linalg.LinAlgError:
            Ci = np.linalg.lstsq(G[blk, blk], D[blk], rcond=None)[0]
        s = np.fft.irfft(np.fft.rfft(Ci.T, nfft) * R[i][None], nfft)[:, :Tx]
        for j in range(n):
            interf, artif = p_all[j] - s[j], e[j] - p_all[j]
            sdr[j, i] = db(np.sum(s[j] ** 2), np.sum((interf + artif) ** 2))
            sir[j, i] = db(np.sum(s[j] ** 2), np.sum(interf ** 2))
            sar[j, i] = db(np.sum((s[j] + interf) ** 2), np.sum(artif ** 2))
    true = np.arange(n)
    perms = list(itertools.permutations(range(n)))
    perm = np.array(perms[int(np.argmax([sir[list(p), true].mean() for p in perms]))])
    return sdr[perm, true], sir[perm, true], sar[perm, true], perm


def check_host_composition():
    """the host composition against the lstsq oracle of the tests, at the tests' production-length case: 1e-9 dB and the permutation"""
    import test_bss_eval_gpu as TG
    n, T, flen = TG.SHAPES[-1]
    ref, est = TG.make_case(n, T, flen)
    got = host_bss_eval(ref.double().numpy(), est.double().numpy(), flen)
    want = TG.oracle(n, T, flen)
    worst = max(np.abs(g - w).max() for g, w in zip(got[:3], want[:3]))
    assert got[3].tolist() == want[3].tolist() and worst <= 1e-9, (worst, got[3], want[3])
    return float(worst)


def make_batch(B, T, seed=0):
    """speech-like test signals: references are white noise through x[t] += 0.9 x[t-1], estimates 5-tap mixtures of them plus noise"""
    rng = np.random.default_rng(seed)
    ref = rng.standard_normal((B, 2, T))
    for t in range(1, T):
        ref[..., t] += 0.9 * ref[..., t - 1]
    taps = 0.2 * rng.standard_normal((B, 2, 2, 5))
    taps[:, [0, 1], [0, 1], 0] += 1.0
    est = np.stack([np.stack([sum(np.convolve(ref[b, i], taps[b, j, i])[:T] for i in range(2)) for j in range(2)]) for b in range(B)])
    est += 0.05 * rng.standard_normal(est.shape)
    return ref.astype(np.float32), est.astype(np.float32)


def _event_times(torch, fn, reps, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
        b.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[min(len(ms) - 1, int(round(0.99 * (len(ms) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="32000,80000")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bss_eval.py measures on the GPU: none is visible")
    import sepkernels
    import utils.bss as bss
    K = sepkernels.backend()
    check = check_host_composition()
    print(json.dumps({"host_composition_max_db_vs_oracle": check}), flush=True)
    results = {"device": torch.cuda.get_device_name(0), "filter_length": FLEN, "n_sources": 2, "reps": args.reps, "warmup": args.warmup,
               "host_threads": os.environ.get("OMP_NUM_THREADS"), "host_composition_max_db_vs_oracle": check, "rows": []}
    for T in map(int, args.lengths.split(",")):
        for B in map(int, args.batches.split(",")):
            ref_np, est_np = make_batch(B, T)
            ref, est = torch.from_numpy(ref_np).cuda(), torch.from_numpy(est_np).cuda()
            native = bss.bss_eval_sources_batch(ref, est)
            host0 = host_bss_eval(ref_np[0].astype(np.float64), est_np[0].astype(np.float64))
            diff = max(np.abs(native[q][0].numpy() - host0[q]).max() for q in range(3))
            assert native[3][0].tolist() == host0[3].tolist()
            whole = _event_times(torch, lambda: bss.bss_eval_sources_batch(ref, est), args.reps, args.warmup)
            scratch = torch.empty(K.bss_scratch_bytes(B, 2, 2, T, FLEN) // 8, device="cuda", dtype=torch.float64)
            xrr, xre = bss._correlations(K, ref, est, None, FLEN, scratch)
            filt_all, filt_one = bss._filters(xrr, xre, FLEN)

            def kernels():
                bss._correlations(K, ref, est, None, FLEN, scratch)
                bss._energies(K, ref, est, filt_all, filt_one, None, FLEN, scratch)
            kern = _event_times(torch, kernels, args.reps, args.warmup)
            solve = _event_times(torch, lambda: bss._filters(xrr, xre, FLEN), args.reps, args.warmup)
            host = []
            for r in range(args.host_reps + 1):
                t0 = time.perf_counter()
                for b in range(B):
                    host_bss_eval(ref_np[b].astype(np.float64), est_np[b].astype(np.float64))
                host.append(1e3 * (time.perf_counter() - t0))
            host = sorted(host[1:])
            row = {"T": T, "B": B, "native_ms_median": round(whole[0], 3), "native_ms_p99": round(whole[1], 3), "kernels_ms_median": round(kern[0], 3),
                   "solve_ms_median": round(solve[0], 3), "solve_route": bss.solve_route(), "host_ms_median": round(host[len(host) // 2], 3),
                   "host_reps": args.host_reps, "max_db_native_vs_host": float(diff)}
            print(json.dumps(row), flush=True)
            results["rows"].append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(results, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
