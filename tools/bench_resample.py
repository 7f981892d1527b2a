"""Resampling benchmark (sepkernels/resample.py; csrc/resample.hip: sep_resample_fwd, sep_resample_stream_fwd) on one MI355X: the kernel route
and the composed route (the same definition as F.pad + F.conv1d(stride = o) + reshape + crop on stock torch ops) side by side on the same GPU in
the same process, alternating, on the same inputs.

    offline   (16, 1, 64000) 16 k -> 8 k and 8 k -> 16 k; (8, 2, 441000) 44.1 k -> 8 k
    stream    64 streams x 160-sample chunks 16 k -> 8 k through StreamResampler (one call = one chunk of every stream), the composed route being
              cat([history, chunk]) + conv1d + the history update written below

One JSON row per shape: kernel_ms_median / _p99 and composed_ms_median / _p99 (HIP events around each call, synchronised per call, --reps after
--warmup), algorithmic_bytes = 4 R (T + T_out), the kernel's fraction of 8 TB/s on those bytes, the instance that ran (sep_last_kernel) and the
largest difference between the two routes relative to max |y|.  A 160-sample chunk is a measurement of launch overhead, not of bandwidth; its
fraction is reported for completeness.

    python tools/bench_resample.py [--reps 50] [--warmup 5] [--out profiles/r17_resample.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dnn-based_source_separation_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

PEAK_BYTES_PER_S = 8e12
OFFLINE = [((16, 1, 64000), 16000, 8000), ((16, 1, 64000), 8000, 16000), ((8, 2, 441000), 44100, 8000)]


def _alternate(torch, fns, reps, warm):
    """the median and p99 in ms of every function of `fns`, timed in turn so that the routes share whatever else the machine is doing"""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    out = []
    for ms in times:
        ms.sort()
        out.append((round(ms[len(ms) // 2], 4), round(ms[min(len(ms) - 1, int(round(0.99 * (len(ms) - 1))))], 4)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_resample.json"))
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the GPU: none is visible")
    import sepkernels
    from sepkernels import resample as RS
    rows = []
    g = torch.Generator(device="cuda").manual_seed(0)
    for shape, orig, new in OFFLINE:
        flt = RS.get_filter(orig, new)
        x = torch.randn(*shape, generator=g, device="cuda")
        R, T = x.numel() // shape[-1], shape[-1]
        T_out = -(-flt.u * T // flt.o)

        def composed():
            return flt.conv(F.pad(x.view(R, T), (flt.width, flt.width + flt.o)), T_out)
        yk = RS.resample(x, orig, new)
        name = sepkernels.last_kernel()
        yc = composed()
        diff = ((yk.view(R, T_out) - yc).abs().max() / yk.abs().max()).item()
        (km, kp), (cm, cp) = _alternate(torch, [lambda: RS.resample(x, orig, new), composed], args.reps, args.warmup)
        nbytes = 4 * R * (T + T_out)
        rows.append(dict(case="offline", shape=list(shape), orig_freq=orig, new_freq=new, o=flt.o, u=flt.u, K=flt.K, Kc=flt.Kc, instance=name,
                         kernel_ms_median=km, kernel_ms_p99=kp, composed_ms_median=cm, composed_ms_p99=cp, algorithmic_bytes=nbytes,
                         kernel_fraction_of_8TBps=round(nbytes / (km * 1e-3) / PEAK_BYTES_PER_S, 4), composed_over_kernel=round(cm / km, 3),
                         routes_max_rel_diff=diff))
        print(json.dumps(rows[-1]), flush=True)
    Bs, n, orig, new = 64, 160, 16000, 8000
    flt = RS.get_filter(orig, new)
    rs = RS.StreamResampler(Bs, orig, new, device="cuda")
    chunk = torch.randn(Bs, n, generator=g, device="cuda")
    hist = torch.zeros(Bs, flt.H, device="cuda")

    def composed_stream():
        cat = torch.cat([hist, chunk], 1)
        y = flt.conv(cat, n // flt.o * flt.u)
        hist.copy_(cat[:, n:])
        return y
    yk = rs(chunk)
    name = sepkernels.last_kernel()
    diff = ((yk - composed_stream()).abs().max() / yk.abs().max()).item()
    (km, kp), (cm, cp) = _alternate(torch, [lambda: rs(chunk), composed_stream], args.reps, args.warmup)
    nbytes = 4 * Bs * (n + n // flt.o * flt.u)
    rows.append(dict(case="stream", streams=Bs, chunk=n, orig_freq=orig, new_freq=new, o=flt.o, u=flt.u, K=flt.K, Kc=flt.Kc, instance=name,
                     kernel_ms_median=km, kernel_ms_p99=kp, composed_ms_median=cm, composed_ms_p99=cp, algorithmic_bytes=nbytes,
                     kernel_fraction_of_8TBps=round(nbytes / (km * 1e-3) / PEAK_BYTES_PER_S, 6), composed_over_kernel=round(cm / km, 3),
                     routes_max_rel_diff=diff, state_bytes=rs.state_bytes, delay_samples=rs.delay))
    print(json.dumps(rows[-1]), flush=True)
    doc = dict(tool="tools/bench_resample.py", device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, timing="HIP events per call, median and p99",
               rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
