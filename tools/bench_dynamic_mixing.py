"""Dynamic-mixing benchmark (sepkernels/mixing.py; csrc/mixing.hip: sep_mix_draw, sep_mix_render) on one MI355X: what it costs to feed the training
step from a device-resident corpus, beside what the fixed-mixture loader costs on the same box.

    1. mixer      one mixer() call (draw + render) at (16, 2, 32000) and (4, 2, 32000) from a synthetic int16 corpus of 2 000 utterances of 3 - 10 s
                  (20 speakers): HIP events around each call, synchronised per call
    2. loader     the same batch shapes served by TrainDataLoader + DevicePrefetcher (16 workers) from 16-bit wav files written to a temporary folder
                  (mix/, s1/, s2/ of 6 - 10 s): per batch a HIP event before asking for it and one at its arrival on the compute stream, synchronised per
                  batch, the host's clock beside it; the first batches (worker start-up) left out.  Nothing consumes the batches here, and every worker
                  decodes whole batches ahead, so they arrive in bursts: the MEAN is the loader's throughput, the median mostly the drain of its queue
    3. step       ms per step of the recorded paper-best training step (bench.py's model and batch, FusedTrainStep with auto_record) over --steps steps,
                  fed by the mixer and fed by the loader: HIP events at the end of consecutive steps
Medians (and p99) of the HIP-event times; the kernels move about 8 MB per paper-size batch and are bound by launch and fill, so no fraction of a roof
is reported.

    python tools/bench_dynamic_mixing.py [--reps 50] [--warmup 5] [--steps 50] [--workers 16] [--out profiles/r20_dynamic_mixing.json]

With --speeds 95,100,105 the tool measures speed perturbation instead (sep_mix_draw_speed, sep_mix_render_speed) and writes
profiles/r21_dynamic_mixing_speed.json:
    1. mixer      one mixer() call at the two shapes with speeds and without, the two alternating in one loop
    2. composed   the same perturbation from what the library had before: per drawn row resample() of the whole utterance on the device, then crop,
                  gain and sum in torch, on the speed mixer's own plans (the outputs agree with the kernel's to the resampler's rounding)
    3. step       the recorded paper-best step fed by either mixer
Bytes are counted for the render only (int16 span reads and fp32 writes); no fraction of a roof is reported.
"""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "dnn-based_source_separation_amd", "src"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

SR, T = 8000, 32000
SHAPES = [(16, 2, T), (4, 2, T)]


def _stats(ms):
    ms = sorted(ms)
    return round(ms[len(ms) // 2], 4), round(ms[min(len(ms) - 1, int(round(0.99 * (len(ms) - 1))))], 4)


def _intervals(torch, produce, count, skip):
    """ms between the ends of consecutive iterations of `produce` (an iterator whose items are consumed on the current stream)"""
    events = []
    for k, _ in enumerate(produce):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        events.append(e)
        if k + 1 >= count + skip + 1:
            break
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in zip(events[skip:-1], events[skip + 1:])]


def _arrivals(torch, batches, count, skip):
    """per batch of the iterator `batches`: ms from asking for it to its arrival on the current stream, as HIP events (synchronised per batch) and on
    the host's clock -> (event ms, wall ms)"""
    import time
    it, ev, wall = iter(batches), [], []
    for k in range(count + skip):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        try:
            next(it)
        except StopIteration:
            break
        b.record()
        b.synchronize()
        t1 = time.perf_counter()
        if k >= skip:
            ev.append(a.elapsed_time(b))
            wall.append(1e3 * (t1 - t0))
    del it
    return ev, wall


def synthetic_corpus(torch, device, utterances=2000, speakers=20, seed=0):
    from sepkernels.mixing import DeviceCorpus
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(3 * SR, 10 * SR + 1, (utterances,), generator=g).tolist()
    waves = [torch.randint(-8000, 8000, (n,), generator=g, dtype=torch.int16) for n in lengths]
    return DeviceCorpus.from_waveforms(waves, [k % speakers for k in range(utterances)], device=device)


def write_wav_folder(torch, root, mixtures=320, seed=1):
    from recipes.audio_io import write_wav
    g = torch.Generator().manual_seed(seed)
    ids = []
    for sub in ("mix", "s1", "s2"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for k in range(mixtures):
        n = int(torch.randint(6 * SR, 10 * SR + 1, (1,), generator=g))
        s = torch.randint(-8000, 8000, (2, n), generator=g).float() / 32768.0
        ID = "{:03d}a{:04d}_0_{:03d}b{:04d}_0".format(k % 20, k, (k + 7) % 20, k)
        write_wav(os.path.join(root, "s1", ID + ".wav"), s[0], SR, 16)
        write_wav(os.path.join(root, "s2", ID + ".wav"), s[1], SR, 16)
        write_wav(os.path.join(root, "mix", ID + ".wav"), s.sum(0), SR, 16)
        ids.append(ID)
    lst = os.path.join(root, "list.txt")
    with open(lst, "w") as f:
        f.write("\n".join(ids) + "\n")
    return lst


def _timed(torch, fn, reps):
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return ms


def composed_from_resample(torch, mixer):
    """the batch of the speed mixer's last plan formed with resample() per row: whole-utterance resampling, then crop, gain and sum in torch"""
    from sepkernels.resample import resample
    c, T = mixer.corpus, mixer.samples
    plan, gain, speed = mixer.plan[0].tolist(), mixer.plan[1], mixer.speed.tolist()
    rows = []
    for b, item in enumerate(plan):
        for i, (u, start, lead, _) in enumerate(item):
            x = c.utterance(u).to(torch.float32)
            P = mixer.speeds[speed[b][i]]
            v = x if P == 100 else resample(x, P, 100)
            row = torch.zeros(T, device=x.device)
            count = min(T - lead, v.numel() - start)
            row[lead:lead + count] = gain[b, i] * (v[start:start + count] * 2.0 ** -15)
            rows.append(row)
    sources = torch.stack(rows).view(len(plan), len(plan[0]), T)
    return sources.sum(1, keepdim=True), sources


def speed_main(args, speeds):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dynamic_mixing.py measures on the GPU: none is visible")
    import sepkernels
    from bench_legs import PAPER
    from criterion.pit import PIT1d
    from criterion.sdr import NegSISDR
    from models.conv_tasnet import ConvTasNet
    from sepkernels.mixing import DynamicMixer
    from sepkernels.train import FusedTrainStep
    dev = torch.device("cuda", 0)
    rows = []
    corpus = synthetic_corpus(torch, dev)
    for B, n, t in SHAPES:
        plain = DynamicMixer(corpus, n_sources=n, samples=t, batch_size=B, seed=111)
        fast = DynamicMixer(corpus, n_sources=n, samples=t, batch_size=B, seed=111, speeds=speeds)
        for _ in range(args.warmup):
            plain(), fast()
        torch.cuda.synchronize()
        ms = {"plain": [], "speed": []}
        for _ in range(args.reps):                      # the two alternate: one box, one minute
            ms["plain"] += _timed(torch, plain, 1)
            ms["speed"] += _timed(torch, fast, 1)
            kernel = sepkernels.last_kernel()
        perturbed = sum(1 for P in speeds if P != 100) / len(speeds)
        for name in ("plain", "speed"):
            med, p99 = _stats(ms[name])
            rows.append(dict(case="mixer", speeds=list(speeds) if name == "speed" else None, shape=[B, n, t], instance=kernel if name == "speed" else "mix_render_vec<int16,8>",
                             ms_median=med, ms_p99=p99, ms_mean=round(sum(ms[name]) / len(ms[name]), 4), bytes_written=4 * B * (n + 1) * t, bytes_read_about=2 * B * n * t,
                             fp64_multiply_adds_about=int(13 * B * n * t * perturbed) if name == "speed" else 0,
                             seconds_of_audio_per_second=round(B * t / SR / (med * 1e-3), 1)))
            print(json.dumps(rows[-1]), flush=True)
        # 2. the same perturbation composed from resample(): on the speed mixer's plans, compared with its output first
        mixture, sources = fast()
        ref_mix, ref_src = composed_from_resample(torch, fast)
        err = float((sources - ref_src).abs().max())
        for _ in range(2):
            fast.draw()
            composed_from_resample(torch, fast)
        torch.cuda.synchronize()
        reps = max(5, args.reps // 5)

        def both():
            fast.draw()
            composed_from_resample(torch, fast)
        ms_c = _timed(torch, both, reps)
        med, p99 = _stats(ms_c)
        rows.append(dict(case="composed from resample()", speeds=list(speeds), shape=[B, n, t], reps=reps, ms_median=med, ms_p99=p99, ms_mean=round(sum(ms_c) / len(ms_c), 4),
                         launches_about="one resample per perturbed row, then crop, gain, stack and sum in torch", max_abs_difference_from_the_kernel=err))
        print(json.dumps(rows[-1]), flush=True)

    # 3. the recorded paper-best step fed by either mixer, alternating blocks
    B = 16
    for name, sp in (("plain", None), ("speed", speeds), ("plain", None), ("speed", speeds)):
        torch.manual_seed(111)
        model = ConvTasNet(**PAPER).to(dev)
        step = FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=2), lr=1e-3, max_norm=5.0, auto_record=True)
        mixer = DynamicMixer(corpus, n_sources=2, samples=T, batch_size=B, seed=111, speeds=sp)

        def steps():
            for _ in range(args.steps + args.warmup + 2):
                mixture, sources = mixer()
                yield step(mixture, sources)
        ms_s = _intervals(torch, steps(), args.steps, args.warmup)
        med, p99 = _stats(ms_s)
        rows.append(dict(case="step", fed_by=name + " mixer", speeds=None if sp is None else list(sp), shape=[B, 2, T], recorded=step._seq is not None, steps_timed=len(ms_s),
                         ms_per_step_median=med, ms_per_step_p99=p99, ms_per_step_mean=round(sum(ms_s) / len(ms_s), 4)))
        print(json.dumps(rows[-1]), flush=True)
        del model, step
    doc = dict(tool="tools/bench_dynamic_mixing.py --speeds " + ",".join(str(P) for P in speeds), device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup,
               steps=args.steps, timing="HIP events, median and p99; plain and speed mixer alternate in one loop",
               corpus=dict(utterances=corpus.num_utterances, speakers=corpus.num_speakers, kind="int16"), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--speeds", default=None, help="integer percentages such as 95,100,105: measure speed perturbation (profiles/r21_dynamic_mixing_speed.json)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "r21_dynamic_mixing_speed.json" if args.speeds else "r20_dynamic_mixing.json")
    if args.speeds:
        return speed_main(args, tuple(int(P) for P in args.speeds.split(",")))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dynamic_mixing.py measures on the GPU: none is visible")
    import sepkernels
    from bench_legs import PAPER
    from criterion.pit import PIT1d
    from criterion.sdr import NegSISDR
    from models.conv_tasnet import ConvTasNet
    from recipes.wsj0mix import DevicePrefetcher, TrainDataLoader, WaveTrainDataset
    from sepkernels.mixing import DynamicMixer
    from sepkernels.train import FusedTrainStep
    dev = torch.device("cuda", 0)
    rows = []
    corpus = synthetic_corpus(torch, dev)
    corpus_mb = round(corpus.samples.numel() * corpus.samples.element_size() / 1e6, 1)

    # 1. one mixer() call
    for B, n, t in SHAPES:
        mixer = DynamicMixer(corpus, n_sources=n, samples=t, batch_size=B, seed=111)
        for _ in range(args.warmup):
            mixer()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            mixer()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        med, p99 = _stats(ms)
        rows.append(dict(case="mixer", shape=[B, n, t], instance=sepkernels.last_kernel(), ms_median=med, ms_p99=p99, ms_mean=round(sum(ms) / len(ms), 4),
                         bytes_written=4 * B * (n + 1) * t,
                         bytes_read=2 * B * n * t, seconds_of_audio_per_second=round(B * t / SR / (med * 1e-3), 1)))
        print(json.dumps(rows[-1]), flush=True)

    with tempfile.TemporaryDirectory() as root:
        lst = write_wav_folder(torch, root)
        train_set = WaveTrainDataset(root, lst, samples=T, overlap=T // 2, n_sources=2)

        def loader(B):
            return DevicePrefetcher(TrainDataLoader(train_set, batch_size=B, shuffle=True, drop_last=True, num_workers=args.workers), dev)

        # 2. the same shapes from wav files
        for B, n, t in SHAPES:
            count = min(args.reps, len(train_set) // B - args.warmup - 2)
            ms, wall = _arrivals(torch, loader(B), count, args.warmup)
            med, p99 = _stats(ms)
            mean = sum(ms) / len(ms)             # the workers deliver in bursts (each decodes whole batches ahead): the mean is the throughput
            rows.append(dict(case="loader", shape=[B, n, t], workers=args.workers, items=len(train_set), batches_timed=len(ms), ms_median=med, ms_p99=p99,
                             ms_mean=round(mean, 4), wall_ms_median=_stats(wall)[0], wall_ms_mean=round(sum(wall) / len(wall), 4),
                             seconds_of_audio_per_second=round(B * t / SR / (mean * 1e-3), 1)))
            print(json.dumps(rows[-1]), flush=True)

        # 3. the recorded paper-best step fed each way
        B = 16
        for feed in ("mixer", "loader"):
            torch.manual_seed(111)
            model = ConvTasNet(**PAPER).to(dev)
            step = FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=2), lr=1e-3, max_norm=5.0, auto_record=True)
            if feed == "mixer":
                mixer = DynamicMixer(corpus, n_sources=2, samples=T, batch_size=B, seed=111)
                batches = (mixer() for _ in range(args.steps + args.warmup + 2))
            else:
                batches = iter(loader(B))

            def steps():
                for mixture, sources in batches:
                    yield step(mixture, sources)
            count = min(args.steps, len(train_set) // B - args.warmup - 2) if feed == "loader" else args.steps
            ms = _intervals(torch, steps(), count, args.warmup)
            med, p99 = _stats(ms)
            rows.append(dict(case="step", fed_by=feed, shape=[B, 2, T], recorded=step._seq is not None, steps_timed=len(ms), ms_per_step_median=med, ms_per_step_p99=p99,
                             ms_per_step_mean=round(sum(ms) / len(ms), 4)))
            print(json.dumps(rows[-1]), flush=True)
            del batches

    doc = dict(tool="tools/bench_dynamic_mixing.py", device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, steps=args.steps,
               timing="HIP events, median and p99", corpus=dict(utterances=corpus.num_utterances, speakers=corpus.num_speakers, kind="int16", megabytes=corpus_mb), rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
