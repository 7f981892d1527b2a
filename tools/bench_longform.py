"""Long-recording benchmark (sepkernels/longform.py; csrc/stitch.hip: sep_stitch_cost, sep_stitch_chain, sep_stitch_ola) on one MI355X: a
10-minute recording at 8 kHz in windows of 4 s at a hop of 2 s (win = 32000, hop = 16000, W = 299 windows, 298 boundaries).

(a) `stitch` rows, n in {2, 5, 10}: the stage after the model alone, on synthetic windows (n long tracks cut into windows, rows scrambled per
    window, 1 % noise) -- one JSON row per n:
        kernels_ms_median / _p99     longform.stitch: sep_stitch_cost, sep_assign, sep_stitch_chain, sep_stitch_ola, no synchronisation in between
        cost_ms / assign_ms / chain_ms / ola_ms    the four launches alone on preallocated buffers
        torch_ms_median / _p99       the same stage on stock torch ops on the device, written below without the module: the pair costs as
                                     |a|^2 + |c|^2 - 2 a.c with one fp64 bmm per call (the direct differences would need a (W - 1) n^2 O
                                     temporary), the chain as W - 1 gathers, the cross-fade as a gather of the rows and slice arithmetic.  Stock
                                     torch has no assignment solver: the baseline calls sep_assign as well, so the comparison is of the other three
        torch_cost_ms / torch_chain_ms / torch_ola_ms    its three parts alone
        algorithmic_bytes            cost: the 2 n overlap rows of every boundary read once; ola: n T samples read (twice in a cross-fade) and written
    Both routes must return the planted order and agree on the output within 1e-6 max|est|.
(b) `end_to_end`: the paper-best Conv-TasNet with random weights in eval() on that recording, batch_windows = 16: separate_long as a whole, the
    stitching stage alone on the model's own window outputs, and its share of the total.
HIP events around each call, synchronised per call; the median of --reps after --warmup.  Each row runs in a process of its own under `timeout`;
the first failing row ends the run.

    python tools/bench_longform.py [--sources 2,5,10] [--reps 30] [--warmup 3] [--out profiles/r15_longform.json]
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

SR, WIN, HOP, T = 8000, 32000, 16000, 600 * 8000
W = (T - WIN) // HOP + 1          # 299: (W - 1) HOP + WIN = T exactly
PAPER = dict(n_basis=512, kernel_size=16, stride=8, enc_basis="trainable", dec_basis="trainable", enc_nonlinear=None, sep_hidden_channels=512,
             sep_bottleneck_channels=128, sep_skip_channels=128, sep_kernel_size=3, sep_num_blocks=3, sep_num_layers=8, dilated=True, separable=True,
             causal=False, sep_nonlinear="prelu", sep_norm=True, mask_nonlinear="sigmoid", n_sources=2)


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


def _need_gpu(torch):
    if not torch.cuda.is_available():
        raise SystemExit("bench_longform.py measures on the GPU: none is visible")


def make_windows(torch, n, seed=0):
    """-> est (1, W, n, WIN) fp32 on the device, scramble (W, n): row r of window w is track scramble[w][r] plus 1 % noise"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    tracks = torch.randn(n, T, generator=g, device="cuda")
    scramble = torch.stack([torch.randperm(n, generator=g, device="cuda") for _ in range(W)])
    est = tracks.unfold(1, WIN, HOP).transpose(0, 1).gather(1, scramble.view(W, n, 1).expand(-1, -1, WIN))
    return (est + 0.01 * torch.randn(W, n, WIN, generator=g, device="cuda")).unsqueeze(0).contiguous(), scramble


# ---- the stage on stock torch ops (sep_assign between them: torch has no solver) ------------------------------------------------------
def torch_cost(torch, est):
    a, c = est[0, :-1, :, HOP:].double(), est[0, 1:, :, :WIN - HOP].double()
    return (a.square().sum(-1).unsqueeze(2) + c.square().sum(-1).unsqueeze(1) - 2.0 * torch.bmm(a, c.transpose(1, 2))).contiguous()


def torch_chain(torch, perm_local):
    rows = [torch.arange(perm_local.shape[1], device=perm_local.device)]
    for w in range(perm_local.shape[0]):
        rows.append(perm_local[w].gather(0, rows[-1]))
    return torch.stack(rows)


def torch_ola(torch, est, perm_abs):
    n, O = est.shape[2], WIN - HOP
    al = est[0].gather(1, perm_abs.view(W, n, 1).expand(-1, -1, WIN))              # every window in the order of the first
    out = torch.empty(n, T, device=est.device, dtype=est.dtype)
    body = out[:, :W * HOP].view(n, W, HOP)
    g = ((torch.arange(O, device=est.device, dtype=est.dtype) + 0.5) / O).view(1, 1, O)
    tail, head = al[:-1, :, HOP:], al[1:, :, :O]
    body[:, 0] = al[0, :, :HOP]
    body[:, 1:, :O] = (tail + g * (head - tail)).transpose(0, 1)
    if HOP > O:
        body[:, 1:, O:] = al[1:, :, O:HOP].transpose(0, 1)
    out[:, W * HOP:] = al[W - 1, :, HOP:]
    return out.unsqueeze(0)


def run_stitch(n, reps, warm):
    import torch
    _need_gpu(torch)
    import sepkernels
    from sepkernels import longform
    K = sepkernels.backend()
    est, scramble = make_windows(torch, n)
    dev = est.device
    cost = torch.empty(1, W - 1, n, n, device=dev, dtype=torch.float64)
    perm_local = torch.empty(1, W - 1, n, device=dev, dtype=torch.int64)
    total, duals = torch.empty(1, W - 1, device=dev, dtype=torch.float64), torch.empty(W - 1, 2 * n, device=dev, dtype=torch.float64)
    perm_abs, out = torch.empty(1, W, n, device=dev, dtype=torch.int64), torch.empty(1, n, T, device=dev, dtype=torch.float32)

    def assign(c):
        K.assign(c, W - 1, n, 0, perm_local, total, duals)
        return perm_local[0]

    def stock():
        return torch_ola(torch, est, torch_chain(torch, assign(torch_cost(torch, est))))

    got, got_perm, _ = longform.stitch(est, HOP, T)
    want = stock()
    planted = scramble.gather(1, got_perm[0])
    assert torch.equal(planted, scramble[:1].expand_as(scramble)), "the kernel route must undo the scramble"
    assert torch.equal(torch_chain(torch, perm_local[0]), got_perm[0]), "both routes must find the same order"
    diff = (got - want).abs().max().item()
    assert diff <= 1e-6 * est.abs().max().item(), diff
    row = {"stitch": True, "n": n, "W": W, "win": WIN, "hop": HOP, "T": T, "output_difference": diff}
    row["kernels_ms_median"], row["kernels_ms_p99"] = _event_times(torch, lambda: longform.stitch(est, HOP, T), reps, warm)
    row["torch_ms_median"], row["torch_ms_p99"] = _event_times(torch, stock, reps, warm)
    row["cost_ms"] = _event_times(torch, lambda: K.stitch_cost(est, cost, 1, W, n, WIN, HOP), reps, warm)[0]
    row["assign_ms"] = _event_times(torch, lambda: assign(cost), reps, warm)[0]
    row["chain_ms"] = _event_times(torch, lambda: K.stitch_chain(perm_local, perm_abs, 1, W, n), reps, warm)[0]
    row["ola_ms"] = _event_times(torch, lambda: K.stitch_ola(est, perm_abs, out, 1, W, n, WIN, HOP, T), reps, warm)[0]
    row["torch_cost_ms"] = _event_times(torch, lambda: torch_cost(torch, est), reps, warm)[0]
    row["torch_chain_ms"] = _event_times(torch, lambda: torch_chain(torch, perm_local[0]), reps, warm)[0]
    row["torch_ola_ms"] = _event_times(torch, lambda: torch_ola(torch, est, perm_abs[0]), reps, warm)[0]
    cost_bytes, ola_bytes = 4 * (W - 1) * 2 * n * (WIN - HOP), 4 * n * (2 * T + (W - 1) * (WIN - HOP))
    row.update(cost_algorithmic_bytes=cost_bytes, ola_algorithmic_bytes=ola_bytes, cost_gbytes_per_s=round(cost_bytes / (row["cost_ms"] * 1e-3) / 1e9, 1),
               ola_gbytes_per_s=round(ola_bytes / (row["ola_ms"] * 1e-3) / 1e9, 1), device=torch.cuda.get_device_name(0), reps=reps, warmup=warm)
    return row


def run_end_to_end(reps, warm):
    import torch
    _need_gpu(torch)
    from models.conv_tasnet import ConvTasNet
    from sepkernels import longform
    torch.manual_seed(0)
    model = ConvTasNet(**PAPER).cuda().eval()
    x = 0.1 * torch.randn(1, 1, T, device="cuda")
    kept = []
    hook = model.register_forward_hook(lambda m, inp, out: kept.append(out))
    want = model.separate_long(x, WIN, hop=HOP, batch_windows=16)
    hook.remove()
    est = torch.cat(kept).view(1, W, 2, WIN)
    assert torch.equal(longform.stitch(est, HOP, T)[0], want)
    row = {"end_to_end": True, "model": "paper-best Conv-TasNet, random weights, eval()", "n": 2, "W": W, "win": WIN, "hop": HOP, "T": T, "batch_windows": 16,
           "forwards": len(kept)}
    row["total_ms_median"], row["total_ms_p99"] = _event_times(torch, lambda: model.separate_long(x, WIN, hop=HOP, batch_windows=16), reps, warm)
    row["stitch_ms_median"], row["stitch_ms_p99"] = _event_times(torch, lambda: longform.stitch(est, HOP, T), reps, warm)
    row["model_and_windows_ms"] = round(row["total_ms_median"] - row["stitch_ms_median"], 4)
    row["stitch_share"] = round(row["stitch_ms_median"] / row["total_ms_median"], 5)
    row["times_real_time"] = round(T / SR / (row["total_ms_median"] * 1e-3), 1)
    row.update(device=torch.cuda.get_device_name(0), reps=reps, warmup=warm)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", default="2,5,10")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds one row may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="(internal) run this row in this process and print it")
    args = ap.parse_args()
    if args.one:
        what, _, n = args.one.partition(":")
        row = run_end_to_end(max(3, args.reps // 6), 1) if what == "end_to_end" else run_stitch(int(n), args.reps, args.warmup)
        print(json.dumps(row), flush=True)
        return 0
    jobs = ["stitch:" + n for n in args.sources.split(",") if n] + ["end_to_end:"]
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
        json.dump({"recording": "10 min at 8 kHz, windows of 4 s at a hop of 2 s", "stitch": [r for r in rows if "stitch" in r],
                   "end_to_end": [r for r in rows if "end_to_end" in r]}, open(args.out, "w"), indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
