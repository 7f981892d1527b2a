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

With --ragged nothing of the above runs.  chunk_size is 120 samples (15 hops), and for (A, slots) in (64, 1024), (256, 1024), (16, 256) every
call ("tick") names a fresh selection of A slots and draws each one's length uniformly from 5 .. 15 hops (all drawn before the clock starts).
One JSON line per (A, slots) and route, "route" being
    ragged    ONE call sep(x, streams=idx, lengths=...) per tick; the upload of slots, offs and chunk is inside the timed span
    grouped   the same audio as one uniform subset call per distinct length (11 calls per tick, the 15-hop one recorded, the others eager):
              the only route a tree without ragged calls offers, so this route also runs on such a tree (--routes grouped)
with chunk_ms_median / chunk_ms_p99 of the tick (recorded), eager_ms_median (ragged route: every launch from Python) and rtf = median / 15 ms
(a tick carries at most 15 ms of audio per stream; 10 ms on average).
Only calls at chunk_size are recorded, so 10 of the 11 calls of a grouped tick are eager launches: a property of the interface, and part of what
the grouped route costs.  To time the grouped route on a commit that has no --ragged (the parent of the change that added it), export that
commit into a directory of its own, build it there, copy THIS file over its tools/bench_online.py (the tool finds the package relative to itself)
and run it there with --ragged --routes grouped.

With --state nothing of the above runs either.  For the same (A, slots) pairs it times sep.export_state(idx) and sep.import_state(state, idx) of
A of the slots at paper size, a fresh selection of A slots at every call (drawn before the clock starts), HIP events around the whole call
(the upload of the slot list, the allocation of the blob and the one launch), synchronised per call.  One JSON line per pair: row_bytes,
export_ms_median / _p99, import_ms_median / _p99, bytes_moved_per_call (A row_bytes read plus A row_bytes written) and the GB/s that makes.

    python tools/bench_online.py [--streams 1,16,64,256,1024] [--chunks 80,160,800] [--active 64,256] [--reps 200] [--eager-reps 200] [--out FILE]
    python tools/bench_online.py --ragged [--routes ragged,grouped] [--reps 200] [--out FILE]
    python tools/bench_online.py --state [--reps 200] [--out FILE]
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


RAGGED = ((64, 1024), (256, 1024), (16, 256))
RAGGED_CHUNK, RAGGED_HOPS = 120, (5, 15)


def _tick_times(torch, tick, reps, warm):
    """tick(k): everything call number k issues -> (median, p99) ms over `reps` timed ticks after `warm` untimed ones, synchronised per tick"""
    for k in range(warm):
        tick(k)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for k, (a, b) in enumerate(ev):
        a.record()
        tick(warm + k)
        b.record()
        b.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2], ms[min(len(ms) - 1, int(round(0.99 * (len(ms) - 1))))]


def _ragged(torch, sepkernels, model, args):
    S, lo, hi = PAPER["stride"], RAGGED_HOPS[0], RAGGED_HOPS[1]
    routes = [r for r in args.routes.split(",") if r]
    warm, lines = 30, []
    dur_ms = 1000.0 * RAGGED_CHUNK / RATE
    for A, Bs in RAGGED:
        g = torch.Generator().manual_seed(1)
        picks = [torch.randperm(Bs, generator=g)[:A].tolist() for _ in range(warm + args.reps)]
        hops = [torch.randint(lo, hi + 1, (A,), generator=g).tolist() for _ in range(warm + args.reps)]
        x = 0.1 * torch.randn(A, 1, RAGGED_CHUNK, device="cuda")
        base = dict(model="convtasnet_causal_paper", slots=Bs, active=A, chunk_size=RAGGED_CHUNK, hops=list(RAGGED_HOPS), chunk_ms_audio=dur_ms,
                    arith=sepkernels.gemm_arith_name(), reps=args.reps, device=torch.cuda.get_device_name(0))
        if "ragged" in routes:
            rec = model.online_separator(num_streams=Bs, chunk_size=RAGGED_CHUNK)
            med, p99 = _tick_times(torch, lambda k: rec(x, picks[k], [h * S for h in hops[k]]), args.reps, warm)
            keys = sorted(rec._sub_seqs)
            launches = len(next(iter(rec._sub_seqs.values())))
            replayed = sum(rec.replays.values())
            del rec
            eager = model.online_separator(num_streams=Bs, chunk_size=RAGGED_CHUNK, record=False)
            emed, _ = _tick_times(torch, lambda k: eager(x, picks[k], [h * S for h in hops[k]]), min(args.reps, args.eager_reps), 3)
            del eager
            row = dict(base, route="ragged", calls_per_tick=1, chunk_ms_median=round(med, 4), chunk_ms_p99=round(p99, 4), eager_ms_median=round(emed, 4),
                       rtf=round(med / dur_ms, 4), recordings=[list(k) for k in keys], replays=replayed, launches_per_chunk=launches,
                       frames_per_s=round(A * (lo + hi) / 2.0 / (med / 1000.0), 1))
            print(json.dumps(row), flush=True)
            lines.append(row)
        if "grouped" in routes:
            rec = model.online_separator(num_streams=Bs, chunk_size=RAGGED_CHUNK)
            xh = {h: x[:, :, :h * S].contiguous() for h in range(lo, hi + 1)}
            groups = [[(h, [s for s, v in zip(picks[k], hops[k]) if v == h]) for h in range(lo, hi + 1)] for k in range(warm + args.reps)]

            def tick(k):
                for h, idx in groups[k]:
                    if idx:
                        rec(xh[h][:len(idx)], idx)
            med, p99 = _tick_times(torch, tick, args.reps, warm)
            calls = sorted(sum(1 for _, idx in gk if idx) for gk in groups[warm:])
            row = dict(base, route="grouped", calls_per_tick=calls[len(calls) // 2], chunk_ms_median=round(med, 4), chunk_ms_p99=round(p99, 4),
                       rtf=round(med / dur_ms, 4), frames_per_s=round(A * (lo + hi) / 2.0 / (med / 1000.0), 1))
            print(json.dumps(row), flush=True)
            lines.append(row)
            del rec
        torch.cuda.empty_cache()
    return lines


def _state(torch, sepkernels, model, args):
    warm, lines = 10, []
    for A, Bs in RAGGED:
        sep = model.online_separator(num_streams=Bs, chunk_size=RAGGED_CHUNK)
        g = torch.Generator().manual_seed(1)
        picks = [torch.randperm(Bs, generator=g)[:A].tolist() for _ in range(warm + args.reps)]
        for t in (sep.carry, sep.rings, sep.tail):                     # a state that is not all zeros (the copies do not care)
            t.normal_()
        sep.sums.normal_()
        sep.frames.fill_(12345)
        held = []
        emed, ep99 = _tick_times(torch, lambda k: held.__setitem__(slice(None), [sep.export_state(picks[k])]), args.reps, warm)
        state = held[0]
        imed, ip99 = _tick_times(torch, lambda k: sep.import_state(state, picks[k]), args.reps, warm)
        moved = 2 * A * state.blob.shape[1]
        row = dict(model="convtasnet_causal_paper", slots=Bs, active=A, row_bytes=state.blob.shape[1], bytes_moved_per_call=moved,
                   export_ms_median=round(emed, 4), export_ms_p99=round(ep99, 4), import_ms_median=round(imed, 4), import_ms_p99=round(ip99, 4),
                   export_gb_per_s=round(moved / (emed * 1e6), 1), import_gb_per_s=round(moved / (imed * 1e6), 1), reps=args.reps,
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(row), flush=True)
        lines.append(row)
        del sep, state, held
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", default="1,16,64,256,1024")
    ap.add_argument("--chunks", default="80,160,800")
    ap.add_argument("--active", default="", help="also time subset calls with this many of the slots, e.g. 64,256")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--eager-reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--ragged", action="store_true", help="time ragged calls (a length per stream) and the grouped route instead")
    ap.add_argument("--routes", default="ragged,grouped", help="with --ragged: which routes to time")
    ap.add_argument("--state", action="store_true", help="time export_state / import_state of A of the slots instead")
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
    if args.state:
        lines = _state(torch, sepkernels, model, args)
        args.streams = ""
    elif args.ragged:
        lines = _ragged(torch, sepkernels, model, args)
        args.streams = ""
    for B in [int(v) for v in args.streams.split(",") if v]:
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
