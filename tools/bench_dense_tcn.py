"""Timing of the causal Conv-TasNet WITHOUT separable convolutions (ConvTasNet(causal=True, separable=False): two full P-tap dilated convolutions
per TCN layer) at paper size: N512 L16 S8 H512 B128 Sc128 P3 X8 R3, sigmoid mask, 2 sources, seeded default weights.  One JSON line per measurement:

    --what step      the training step (forward + PIT(SI-SDR) + backward + clip + Adam, sepkernels.train.FusedTrainStep) on `--batch` utterances of
                     `--seconds` s at 8 kHz: "eager" (every launch from Python) and, where the model is staged, "recorded" (one sep_run_sequence
                     call per step).  On a tree whose staged family refuses separable=False the eager step is the module-by-module composition on
                     torch convolutions -- `route` says which ran -- so the same file times the parent of the change that put the family on
                     kernels: export that commit into a directory of its own, build it there, copy THIS file over its tools/ and run it there.
    --what kernels   sep_unfold_dilated and sep_fold_dilated alone at the step's shape, per dilation 1 .. 128 (HIP events around `--reps` launches),
                     with the bytes they move: the unfold reads H x frames once and writes it P times, the fold the reverse.
    --what online    `--streams` streams x `--chunk` samples per call through model.online_separator(): recorded and eager chunk time.

Medians over `--reps` timed repetitions after `--warmup`; HIP events on the launch stream, synchronised per repetition.

    python tools/bench_dense_tcn.py --what step,kernels,online [--batch 4] [--seconds 4] [--reps 20] [--warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dnn-based_source_separation_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

PAPER_DENSE = dict(n_basis=512, kernel_size=16, stride=8, enc_basis="trainable", dec_basis="trainable", enc_nonlinear=None, sep_hidden_channels=512,
                   sep_bottleneck_channels=128, sep_skip_channels=128, sep_kernel_size=3, sep_num_blocks=3, sep_num_layers=8, dilated=True,
                   separable=False, causal=True, sep_nonlinear="prelu", sep_norm=True, mask_nonlinear="sigmoid", n_sources=2)
RATE = 8000


def _median_ms(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0], ms[-1]


def bench_step(torch, args, emit):
    from models.conv_tasnet import ConvTasNet
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    from sepkernels.train import FusedTrainStep
    g = torch.Generator().manual_seed(7)
    batches = [(0.1 * torch.randn(args.batch, 2, int(args.seconds * RATE), generator=g)).cuda() for _ in range(4)]
    for recorded in (False, True):
        torch.manual_seed(111)
        model = ConvTasNet(**PAPER_DENSE).cuda()
        staged = bool(getattr(model, "staged", False))
        if recorded and not staged:
            continue
        step = FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=2), lr=1e-3, max_norm=5.0, auto_record=recorded)
        k = [0]

        def one():
            src = batches[k[0] % len(batches)]
            k[0] += 1
            step(src.sum(1, keepdim=True).contiguous(), src)
        med, lo, hi = _median_ms(torch, one, args.reps, args.warmup)
        assert (step._seq is not None) == recorded
        emit(dict(what="step", mode="recorded" if recorded else "eager", route="staged" if staged else "composed", batch=args.batch,
                  seconds=args.seconds, step_ms_median=round(med, 3), step_ms_min=round(lo, 3), step_ms_max=round(hi, 3),
                  launches=len(step._seq) if recorded else None))
        del model, step
        torch.cuda.empty_cache()


def bench_kernels(torch, args, emit):
    import sepkernels
    from sepkernels import net as _net
    K = sepkernels.backend()
    cfg = PAPER_DENSE
    geo = _net.Geometry(int(args.seconds * RATE), cfg["kernel_size"], cfg["stride"])
    B, C, P, T, ldt = args.batch, cfg["sep_hidden_channels"], cfg["sep_kernel_size"], geo.F, geo.ldt
    x = torch.randn(B, C, ldt, device="cuda")
    cols = torch.empty(B, C * P, ldt, device="cuda")
    dx = torch.empty_like(x)
    nbytes = (1 + P) * B * C * ldt * 4
    for d in [2 ** k for k in range(cfg["sep_num_layers"])]:
        pad = (P - 1) * d
        for name, fn in (("sep_unfold_dilated", lambda: K.unfold_dilated(x, cols, B, C, T, ldt, P, d, pad)),
                         ("sep_fold_dilated", lambda: K.fold_dilated(cols, dx, B, C, T, ldt, P, d, pad))):
            med, lo, hi = _median_ms(torch, fn, args.reps, args.warmup)
            emit(dict(what="kernel", name=name, B=B, C=C, T=T, ldt=ldt, P=P, dil=d, us_median=round(1e3 * med, 2), us_min=round(1e3 * lo, 2),
                      bytes=nbytes, GBps=round(nbytes / (med * 1e-3) / 1e9, 1)))


def bench_online(torch, args, emit):
    from models.conv_tasnet import ConvTasNet
    torch.manual_seed(0)
    model = ConvTasNet(**PAPER_DENSE).cuda()
    x = 0.1 * torch.randn(args.streams, 1, args.chunk, device="cuda")
    for record in (True, False):
        sep = model.online_separator(num_streams=args.streams, chunk_size=args.chunk, record=record)
        med, lo, hi = _median_ms(torch, lambda: sep(x), args.reps * 5, args.warmup * 2)
        emit(dict(what="online", mode="recorded" if record else "eager", streams=args.streams, chunk=args.chunk, chunk_ms_median=round(med, 3),
                  chunk_ms_min=round(lo, 3), rtf=round(med / (1e3 * args.chunk / RATE), 4), launches_per_chunk=sep.launches_per_chunk(),
                  state_bytes=sep.state_bytes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="step,kernels,online")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=80)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    import torch
    lines = []

    def emit(d):
        d = dict(d, tag=args.tag)
        lines.append(d)
        print(json.dumps(d), flush=True)
    for what in args.what.split(","):
        {"step": bench_step, "kernels": bench_kernels, "online": bench_online}[what](torch, args, emit)
    if args.out:
        with open(args.out, "a") as f:
            for d in lines:
                f.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
