"""MixIT benchmark (criterion/mixit.py; csrc/mixit.hip: sep_mixit_gram, sep_mixit_search, sep_mixit_bwd): forward + backward of
MixIT(NegThresholdedSNR()) on (B, M, T) estimates of (B, N, T) mixtures, T = 32000 (4 s at 8 kHz), on the kernel route and on the composed
route (remixes for a block of assignments at a time, the criterion itself on them; forced by a subclass of the criterion, which the route
selection does not take for the exact class) in the same session.  One JSON line per shape:

    kernel_ms_median / _p99      HIP events around loss + backward, synchronised per call; median of --reps (50) after --warmup (5)
    composed_ms_median / _p99    the same on the composed route
    kernels_only_ms_median       the three entry points alone on preallocated buffers (Gram + its reduction, search, gradient)
    algorithmic_bytes            what the algorithm has to move: the R = M + N rows read twice (Gram pass, gradient pass) and M rows written
    kernel_route_gbytes_per_s    algorithmic_bytes over kernels_only_ms_median (a whole-call rate, not a share of peak of one kernel)
    loss_difference_db           |kernel route - composed route| on the timed input; the assignments must agree

Each shape runs in a process of its own under `timeout`; the first failing shape ends the run.

    python tools/bench_mixit.py [--shapes 4x4x2x32000,16x4x2x32000,16x8x2x32000,4x6x3x32000] [--reps 50] [--warmup 5] [--out profiles/r13_mixit.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dnn-based_source_separation_amd", "src")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = "4x4x2x32000,16x4x2x32000,16x8x2x32000,4x6x3x32000"


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


def make_batch(torch, B, M, N, T, seed=0):
    """mixtures of M planted sources, estimates at about 8 dB: the kind of input a half-trained model produces"""
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(B, M, T, generator=g)
    assign = torch.randint(N, (B, M), generator=g)
    tgt = torch.zeros(B, N, T)
    tgt.scatter_add_(1, assign.unsqueeze(2).expand(B, M, T), src)
    return (0.8 * src + 0.3 * torch.randn(B, M, T, generator=g)).cuda(), tgt.cuda(), assign


def run_shape(B, M, N, T, reps, warm):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixit.py measures on the GPU: none is visible")
    import sepkernels
    from criterion.mixit import MixIT
    from criterion.sdr import NegThresholdedSNR

    class Composed(NegThresholdedSNR):        # the same criterion; not the exact class, so criterion.mixit takes the composed route
        pass
    K = sepkernels.backend()
    est, tgt, assign = make_batch(torch, B, M, N, T)
    leaf = est.clone().requires_grad_(True)

    def step(crit):
        leaf.grad = None
        loss, got = crit(leaf, tgt)
        loss.backward()
        return loss, got
    fast, slow = MixIT(NegThresholdedSNR()), MixIT(Composed())
    l1, a1 = step(fast)
    g1 = leaf.grad.clone()
    l2, a2 = step(slow)
    g2 = leaf.grad.clone()
    assert torch.equal(a1, a2) and torch.equal(a1.cpu(), assign), "the two routes must agree on the assignment (and find the planted one)"
    grad_diff = ((g1 - g2).abs().max() / g2.abs().max()).item()
    kernel = _event_times(torch, lambda: step(fast), reps, warm)
    composed = _event_times(torch, lambda: step(slow), max(5, reps // 5), max(2, warm // 2))
    R = M + N
    gram = torch.empty(B, R, R, device="cuda", dtype=torch.float64)
    scratch = torch.empty(K.mixit_scratch_bytes(B, M, N, T) // 8, device="cuda", dtype=torch.float64)
    best, code, per = torch.empty(B, device="cuda"), torch.empty(B, device="cuda", dtype=torch.int64), torch.empty(B, N, device="cuda")
    gw, d_est = torch.full((B,), -1.0 / (B * N), device="cuda"), torch.empty_like(est)
    tau = NegThresholdedSNR().tau

    def kernels():
        K.mixit_gram(est, tgt, gram, scratch, B, M, N, T)
        K.mixit_search(gram, B, M, N, 2, 1, 1, 1e-12, tau, best, code, per)
        K.mixit_bwd(est, tgt, gram, code, gw, d_est, B, M, N, T, 2, 1e-12, tau)
    only = _event_times(torch, kernels, reps, warm)
    nbytes = 4 * B * T * (2 * R + M)
    return {"B": B, "M": M, "N": N, "T": T, "assignments": N ** M, "kernel_ms_median": round(kernel[0], 4), "kernel_ms_p99": round(kernel[1], 4),
            "composed_ms_median": round(composed[0], 4), "composed_ms_p99": round(composed[1], 4), "kernels_only_ms_median": round(only[0], 4),
            "algorithmic_bytes": nbytes, "kernel_route_gbytes_per_s": round(nbytes / (only[0] * 1e-3) / 1e9, 1),
            "composed_over_kernel": round(composed[0] / kernel[0], 2), "loss_difference_db": abs(l1.item() - l2.item()),
            "gradient_difference_rel": grad_diff, "device": torch.cuda.get_device_name(0), "reps": reps, "warmup": warm}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds one shape may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run this shape in this process and print its row")
    args = ap.parse_args()
    if args.one:
        print(json.dumps(run_shape(*map(int, args.one.split("x")), args.reps, args.warmup)), flush=True)
        return 0
    rows = []
    for shape in args.shapes.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", shape, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-4000:])
            print("shape {} ended with status {}: stopping".format(shape, r.returncode))
            return 1
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({"criterion": "MixIT(NegThresholdedSNR(30))", "rows": rows}, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
