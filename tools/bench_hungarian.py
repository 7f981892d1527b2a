"""Optimal-permutation training benchmark (criterion/hungarian.py; csrc/assign.hip: sep_pair_gram, sep_assign, sep_pair_assign, sep_pair_bwd) on one
MI355X.  Forward + backward of a permutation-invariant negative SI-SDR on (B, n, T) = (4, n, 32000) (4 s at 8 kHz), n in {2, 5, 10, 20}, three ways
in the same session -- one JSON row per n:

    kernel_ms_median / _p99      HungarianLoss(NegSISDR()): sep_pair_gram, sep_pair_assign, sep_pair_bwd
    pit_ms_median / _p99         PIT1d(NegSISDR(), n) where its table of n! permutations is feasible (n <= 8), else null
    composed_ms_median / _p99    criterion.sdr.sisdr_pairs (sep_sisdr_dots, sep_sisdr_from_dots, sep_sisdr_bwd), sep_assign on the matrix between them
    pair_gram_ms / sisdr_dots_ms the two waveform passes alone on preallocated buffers (sep_sisdr_dots accumulates with atomics: its outputs are
                                 zeroed inside the timed region, as every caller must), and algorithmic_bytes = the 2 n rows read once over each time
    loss_difference_db           |kernel route - composed route| on the timed input; the patterns must agree (and be the planted one)

then `assign` rows: sep_assign alone at B = 64, n in {5, 20, 64} on Gaussian matrices, and `high_sdr`: estimates at 30 dB on (2, 5, 4001), the
error of HungarianLoss(NegSISDR()) and of criterion.sdr.sisdr on the same matched pairs against an fp64 evaluation from the waveforms.
HIP events around each call, synchronised per call; the median of --reps (50) after --warmup (5).  Each row runs in a process of its own under
`timeout`; the first failing row ends the run.

    python tools/bench_hungarian.py [--sources 2,5,10,20] [--reps 50] [--warmup 5] [--out profiles/r14_hungarian.json]
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

B, T = 4, 32000


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
    return round(ms[len(ms) // 2], 4), round(ms[min(len(ms) - 1, int(round(0.99 * (len(ms) - 1))))], 4)


def make_batch(torch, B, n, T, noise=0.3, gain=0.8, seed=0):
    """targets, estimates = a planted permutation of them at about 8 dB: the kind of input a half-trained model produces"""
    g = torch.Generator().manual_seed(seed)
    tgt = torch.randn(B, n, T, generator=g)
    planted = torch.stack([torch.randperm(n, generator=g) for _ in range(B)])
    est = gain * tgt[torch.arange(B).unsqueeze(1), planted] + noise * torch.randn(B, n, T, generator=g)
    return est, tgt, planted


def _need_gpu(torch):
    if not torch.cuda.is_available():
        raise SystemExit("bench_hungarian.py measures on the GPU: none is visible")


def run_sources(n, reps, warm):
    import torch
    _need_gpu(torch)
    import sepkernels
    from criterion.hungarian import HungarianLoss
    from criterion.pit import PIT1d
    from criterion.sdr import NegSISDR, sisdr_pairs
    K = sepkernels.backend()
    est, tgt, planted = make_batch(torch, B, n, T)
    est, tgt = est.cuda(), tgt.cuda()
    leaf = est.clone().requires_grad_(True)
    rows = torch.arange(B, device="cuda").unsqueeze(1)
    perm, total, duals = torch.empty(B, n, device="cuda", dtype=torch.int64), torch.empty(B, device="cuda", dtype=torch.float64), torch.empty(B, 2 * n, device="cuda", dtype=torch.float64)

    def composed():
        leaf.grad = None
        val = sisdr_pairs(leaf, tgt)
        K.assign(val.detach().double().contiguous(), B, n, 1, perm, total, duals)
        loss = -val[rows, torch.arange(n, device="cuda").unsqueeze(0), perm].mean()
        loss.backward()
        return loss, perm

    def through(crit):
        def step():
            leaf.grad = None
            loss, pattern = crit(leaf, tgt)
            loss.backward()
            return loss, pattern
        return step
    fast = through(HungarianLoss(NegSISDR()))
    l1, p1 = fast()
    g1 = leaf.grad.clone()
    l2, p2 = composed()
    g2 = leaf.grad.clone()
    assert torch.equal(p1.cpu(), planted) and torch.equal(p2.cpu(), planted), "both routes must find the planted pattern"
    row = {"B": B, "n": n, "T": T, "loss_difference_db": abs(l1.item() - l2.item()), "gradient_difference_rel": ((g1 - g2).abs().max() / g2.abs().max()).item()}
    row["kernel_ms_median"], row["kernel_ms_p99"] = _event_times(torch, fast, reps, warm)
    row["composed_ms_median"], row["composed_ms_p99"] = _event_times(torch, composed, reps, warm)
    row["pit_ms_median"] = row["pit_ms_p99"] = None
    if n <= 8:
        slow = through(PIT1d(NegSISDR(), n))
        l3, p3 = slow()
        assert torch.equal(p3.cpu(), planted)
        row["pit_ms_median"], row["pit_ms_p99"] = _event_times(torch, slow, max(5, reps // 5) if n > 6 else reps, warm)
    dots, tt, xx = torch.empty(B, n, n, device="cuda", dtype=torch.float64), torch.empty(B, n, device="cuda", dtype=torch.float64), torch.empty(B, n, device="cuda", dtype=torch.float64)
    scratch = torch.empty(K.pair_gram_scratch_bytes(B, n, T) // 8, device="cuda", dtype=torch.float64)

    def old_pass():
        dots.zero_()
        tt.zero_()
        xx.zero_()
        K.sisdr_dots(est, tgt, dots, tt, xx, B, n, T, True)
    nbytes = 4 * B * 2 * n * T
    row["pair_gram_ms"] = _event_times(torch, lambda: K.pair_gram(est, tgt, dots, tt, xx, scratch, B, n, T), reps, warm)[0]
    row["sisdr_dots_ms"] = _event_times(torch, old_pass, reps, warm)[0]
    row.update(algorithmic_bytes=nbytes, pair_gram_gbytes_per_s=round(nbytes / (row["pair_gram_ms"] * 1e-3) / 1e9, 1),
               sisdr_dots_gbytes_per_s=round(nbytes / (row["sisdr_dots_ms"] * 1e-3) / 1e9, 1), device=torch.cuda.get_device_name(0), reps=reps, warmup=warm)
    return row


def run_assign(n, reps, warm):
    import torch
    _need_gpu(torch)
    import sepkernels
    K = sepkernels.backend()
    nb = 64
    cost = torch.randn(nb, n, n, generator=torch.Generator().manual_seed(n), dtype=torch.float64).cuda()
    perm, total, duals = torch.empty(nb, n, device="cuda", dtype=torch.int64), torch.empty(nb, device="cuda", dtype=torch.float64), torch.empty(nb, 2 * n, device="cuda", dtype=torch.float64)
    med, p99 = _event_times(torch, lambda: K.assign(cost, nb, n, 0, perm, total, duals), reps, warm)
    assert all(sorted(r) == list(range(n)) for r in perm.cpu().tolist())
    return {"assign": True, "B": nb, "n": n, "assign_ms_median": med, "assign_ms_p99": p99}


def run_high_sdr():
    import torch
    _need_gpu(torch)
    from criterion.hungarian import HungarianLoss
    from criterion.sdr import NegSISDR, sisdr
    est, tgt, planted = make_batch(torch, 2, 5, 4001, noise=0.03, gain=1.0, seed=70)
    e64, t64 = est.double(), tgt.double()[torch.arange(2).unsqueeze(1), planted]
    tt = t64.square().sum(-1, keepdim=True) + 1e-12
    proj = (e64 * t64).sum(-1, keepdim=True) / tt * t64
    want = (10 * torch.log10((proj.square().sum(-1) + 1e-12) / ((proj - e64).square().sum(-1) + 1e-12))).mean(1)
    loss, pattern = HungarianLoss(NegSISDR())(est.cuda(), tgt.cuda(), batch_mean=False)
    matched = sisdr(est.cuda(), tgt.cuda()[torch.arange(2, device="cuda").unsqueeze(1), planted.cuda()])
    assert torch.equal(pattern.cpu(), planted)
    return {"high_sdr": True, "B": 2, "n": 5, "T": 4001, "sisdr_db": want.mean().item(), "hungarian_error_db": (loss.cpu().double() + want).abs().max().item(),
            "sisdr_on_matched_pairs_error_db": (matched.cpu().double().mean(1) - want).abs().max().item()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", default="2,5,10,20")
    ap.add_argument("--assign", default="5,20,64")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=180, help="seconds one row may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run this row in this process and print it")
    args = ap.parse_args()
    if args.one:
        what, _, n = args.one.partition(":")
        row = run_high_sdr() if what == "high_sdr" else (run_assign if what == "assign" else run_sources)(int(n), args.reps, args.warmup)
        print(json.dumps(row), flush=True)
        return 0
    jobs = ["sources:" + n for n in args.sources.split(",") if n] + ["assign:" + n for n in args.assign.split(",") if n] + ["high_sdr:"]
    rows = []
    for job in jobs:
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--one", job, "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-4000:])
            print("row {} ended with status {}: stopping".format(job, r.returncode))
            return 1
        row = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump({"criterion": "HungarianLoss(NegSISDR())", "rows": [r for r in rows if "assign" not in r and "high_sdr" not in r],
                   "assign": [r for r in rows if "assign" in r], "high_sdr": [r for r in rows if "high_sdr" in r]}, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
