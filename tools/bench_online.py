"""Online separation benchmark (sepkernels/online.py): the paper-size CAUSAL Conv-TasNet (N512 L16 S8 H512 B128 Sc128 P3 X8 R3, sigmoid, 2 sources,
seeded default weights) separating `streams` concurrent 8 kHz streams chunk by chunk.  One JSON line per (streams, chunk) configuration:

    chunk_ms_median / chunk_ms_p99            per-chunk time of the RECORDED step (one sep_run_sequence call per chunk), HIP events on the
                                              launch stream around the whole call (input copy, replay, output copy), synchronised per chunk
    eager_ms_median / eager_ms_p99            the same with every launch issued from Python
    rtf / eager_rtf                           median chunk time / chunk duration (real time: < 1)
    launches_per_chunk, state_bytes, frames_per_s (encoder frames of all streams per second of the recorded step)

With --active A1,A2,... every (streams, chunk) configuration is followed by one line per A <= streams with "active": A -- subset calls
sep(chunk, streams=idx) for A of the `streams` slots, a FRESH selection (A distinct slots in random order, drawn before the clock starts) at every
call, the upload of the slot list inside the timed span; same fields, state_bytes still that of all slots, frames_per_s of the A streams.

    python tools/bench_online.py [--streams 1,16,64,256,1024] [--chunks 80,160,800] [--active 64,256] [--reps 200] [--eager-reps 200] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dnn-based_source_separation_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

PAPER = dict(n_basis=512, kernel_size=16, stride=8, enc_basis="trainable", dec_basis="trainable", enc_nonlinear=None, sep_hidden_channels=512,
             sep_bottleneck_channels=128, sep_skip_channels=128, sep_kernel_size=3, sep_num_blocks=3, sep_num_layers=8, dilated=True,
             separable=True, causal=True, sep_nonlinear="prelu", sep_norm=True, mask_nonlinear="sigmoid", n_sources=2)
RATE = 8000


def _times(torch, sep, x, reps, warm, active=None):
    """active: None, or the number of slots of a subset call; every call then names a fresh selection"""
    g = torch.Generator().manual_seed(1)
    picks = [torch.randperm(sep.num_streams, generator=g)[:active].tolist() if active else None for _ in range(warm + reps)]
    for k in range(warm):
        sep(x, picks[k]) if active else sep(x)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k, (a, b) in enumerate(ev):
        a.record()
        sep(x, picks[warm + k]) if active else sep(x)
        b.record()
        b.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[min(len(ms) - 1, int(round(0.99 * (len(ms) - 1))))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,64,256,1024")
    ap.add_argument("--chunks", default="80,160,800")
    ap.add_argument("--active", default="", help="also time subset calls with this many of the slots, e.g. 64,256")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--eager-reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    import sepkernels
    from models.conv_tasnet import ConvTasNet
    if not torch.cuda.is_available():
        raise SystemExit("bench_online.py measures on the GPU; none is visible")
    torch.manual_seed(0)
    model = ConvTasNet(**PAPER).cuda()
    assert model.staged and not model.fused
    lines = []
    for B in [int(v) for v in args.streams.split(",")]:
        for chunk in [int(v) for v in args.chunks.split(",")]:
            x = 0.1 * torch.randn(B, 1, chunk, device="cuda")
            rec = model.online_separator(num_streams=B, chunk_size=chunk)
            med, p99 = _times(torch, rec, x, args.reps, 5)
            eager = model.online_separator(num_streams=B, chunk_size=chunk, record=False)
            emed, ep99 = _times(torch, eager, x, args.eager_reps, 3)
            dur_ms = 1000.0 * chunk / RATE
            row = dict(model="convtasnet_causal_paper", streams=B, chunk_samples=chunk, chunk_ms_audio=dur_ms, arith=sepkernels.gemm_arith_name(),
                       chunk_ms_median=round(med, 4), chunk_ms_p99=round(p99, 4), eager_ms_median=round(emed, 4), eager_ms_p99=round(ep99, 4),
                       rtf=round(med / dur_ms, 4), eager_rtf=round(emed / dur_ms, 4), launches_per_chunk=rec.launches_per_chunk(),
                       state_bytes=rec.state_bytes, frames_per_s=round(B * (chunk // PAPER["stride"]) / (med / 1000.0), 1),
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(row), flush=True)
            lines.append(row)
            for A in [int(v) for v in args.active.split(",") if v]:
                if A > B:
                    continue
                xa = x[:A].contiguous()
                med, p99 = _times(torch, rec, xa, args.reps, 5, active=A)
                emed, ep99 = _times(torch, eager, xa, args.eager_reps, 3, active=A)
                sub = dict(row, active=A, chunk_ms_median=round(med, 4), chunk_ms_p99=round(p99, 4), eager_ms_median=round(emed, 4),
                           eager_ms_p99=round(ep99, 4), rtf=round(med / dur_ms, 4), eager_rtf=round(emed / dur_ms, 4),
                           frames_per_s=round(A * (chunk // PAPER["stride"]) / (med / 1000.0), 1))
                print(json.dumps(sub), flush=True)
                lines.append(sub)
            del rec, eager, x
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
