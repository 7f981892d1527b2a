"""
Score a trained music Conv-TasNet on the MUSDB18 test tracks with museval's figure, BSS-eval v4 ("images"): framewise SDR, ISR, SIR and SAR,
the median over a track's one-second frames and then over the tracks (utils.bss.eval_track; definition in DESIGN.md 4.14).  Where the
reference's music tester ends (egs/musdb18/conv-tasnet/src/adhoc_driver.py:352-380, museval.eval_mus_track).

    python -m recipes.evaluate_musdb18 --model_path M.pth --musdb18_root R [--out_dir D] [--window_s 4 --hop_s 2] [--batch_windows 16] [--use_cuda 0|1]

Reads `<R>/test/<track>/{mixture,bass,drums,other,vocals}.wav` (decoded stems, every directory under `<R>/test`, or the names of `<R>/test.txt` if
that file exists), separates every track window by window, writes `<D>/<track>/<target>.wav` and `<D>/<track>.json` (the frame lists and medians
of every target, `accompaniment` included), prints the per-target medians of each track and, at the end, the medians over the tracks.

Separation: a model of one input channel goes through sepkernels.longform.separate_long with the track's channels as its batch.  separate_long
takes one channel and re-orders every window's outputs by matching neighbours; a model of several input channels (the music recipe: stereo, its
sources in a FIXED order) is run on the same windows and its outputs are cross-faded with the same weights in the order the model gives them.

`evaluate_tracks` is the function form: it takes tensors, so nothing has to be on disk.
"""
import argparse
import json
import os

import torch
import torch.nn.functional as F

from models.conv_tasnet import ConvTasNet
from sepkernels.longform import separate_long
from utils.bss import FILTER_LENGTH, IMAGE_METRICS, eval_track, nanmedian

from .audio_io import read_wav, write_wav
from .musdb18 import SAMPLE_RATE_MUSDB18, SOURCES
from .wsj0mix import _read_ids


def _separate_fixed_order(model, mixture, window, hop, batch_windows):
    """mixture (C, T), C = model.in_channels > 1 -> (n_sources, C, T): windows [w hop, w hop + window) (zeros beyond T), `batch_windows` per
    forward, cross-faded over the overlaps with the weights of sepkernels.longform.stitch, every source in the row the model gives it"""
    C, T = mixture.shape
    if not (window <= 2 * hop and hop < window):
        raise ValueError("hop must lie in [window / 2, window): window {}, hop {}".format(window, hop))
    with torch.no_grad():
        if T <= window:
            return model(mixture[None, None])[0]
        W = -(-(T - window) // hop) + 1
        wins = F.pad(mixture, (0, (W - 1) * hop + window - T)).unfold(1, window, hop).permute(1, 0, 2)         # (W, C, window)
        est = torch.cat([model(wins[k:k + batch_windows, None].contiguous()) for k in range(0, W, batch_windows)])   # (W, n, C, window)
        O = window - hop
        out = torch.zeros(est.shape[1], C, (W - 1) * hop + window, device=est.device, dtype=est.dtype)
        g = (torch.arange(O, device=est.device, dtype=est.dtype) + 0.5) / O
        for w in range(W):
            piece = est[w].clone()
            if w > 0:
                piece[..., :O] *= g
            if w < W - 1:
                piece[..., hop:] *= 1 - g
            out[..., w * hop:w * hop + window] += piece
        return out[..., :T]


def separate_track(model, mixture, window, hop=None, batch_windows=16):
    """mixture (C, T) -> estimates (n_sources, C, T); the caller chooses model.eval() and the device"""
    window = int(window)
    hop = window // 2 if hop is None else int(hop)
    if mixture.dim() != 2:
        raise ValueError("separate_track takes a (channels, T) mixture, given {}".format(tuple(mixture.shape)))
    if getattr(model, "in_channels", 1) == 1:
        return separate_long(model, mixture[:, None, :], window, hop=hop, batch_windows=batch_windows).permute(1, 0, 2)
    if mixture.shape[0] != model.in_channels:
        raise ValueError("the track has {} channels, the model was built with in_channels={}".format(mixture.shape[0], model.in_channels))
    return _separate_fixed_order(model, mixture, window, hop, batch_windows)


def _line(name, scores):
    return "{}: ".format(name) + "; ".join("{} ".format(t) + " ".join("{} {:.3f}".format(m, s[m]) for m in IMAGE_METRICS) for t, s in scores.items())


def evaluate_tracks(model, tracks, rate, targets=SOURCES, window=None, hop=None, batch_windows=16, out_dir=None, bits_per_sample=16, filter_length=FILTER_LENGTH):
    """tracks: iterable of (name, mixture (C, T), references {target: (C, T)}) on the device the model is on; the model's output row k is
    targets[k].  -> {"tracks": {name: {target: {"frames": {...}, "SDR": ..., "ISR": ..., "SIR": ..., "SAR": ...}}},
    "median": {target: {"SDR": median over tracks, ...}}} with `accompaniment` among the targets when `vocals` is (utils.bss.eval_track).
    window, hop: samples of the separation windows (default 4 s at stride 2 s).  With out_dir the estimates go to <out_dir>/<name>/<target>.wav
    and a track's scores to <out_dir>/<name>.json."""
    targets = list(targets)
    window = 4 * rate if window is None else int(window)
    model.eval()
    results = {}
    for name, mixture, references in tracks:
        estimates = separate_track(model, mixture, window, hop, batch_windows)
        if estimates.shape[0] != len(targets):
            raise ValueError("the model gives {} sources, {} targets are named".format(estimates.shape[0], len(targets)))
        estimates = {t: estimates[k] for k, t in enumerate(targets)}
        scores = eval_track({t: references[t] for t in targets}, estimates, rate, filter_length=filter_length)
        results[name] = scores
        print(_line(name, scores))
        if out_dir is not None:
            os.makedirs(os.path.join(out_dir, name), exist_ok=True)
            for t, e in estimates.items():
                write_wav(os.path.join(out_dir, name, t + ".wav"), e.detach().cpu().clamp(-1, 1), rate, bits_per_sample)
            with open(os.path.join(out_dir, name + ".json"), "w") as f:
                json.dump({"track": name, "rate": rate, "targets": scores}, f)
    names = list(next(iter(results.values()))) if results else []
    median = {t: {m: nanmedian([results[k][t][m] for k in results]) for m in IMAGE_METRICS} for t in names}
    if results:
        print(_line("median over {} tracks".format(len(results)), median))
    return {"tracks": results, "median": median}


def musdb18_test_tracks(root, device="cpu", targets=SOURCES):
    """the tracks of <root>/test, one at a time: (name, mixture, {target: stem}) as (channels, T) tensors on `device`"""
    test = os.path.join(os.path.abspath(root), "test")
    listed = os.path.join(os.path.abspath(root), "test.txt")
    names = _read_ids(listed) if os.path.exists(listed) else sorted(d for d in os.listdir(test) if os.path.isdir(os.path.join(test, d)))
    for name in names:
        mixture, rate = read_wav(os.path.join(test, name, "mixture.wav"))
        if rate != SAMPLE_RATE_MUSDB18:
            raise AssertionError("{}: sample rate {}".format(name, rate))
        yield name, mixture.to(device), {t: read_wav(os.path.join(test, name, t + ".wav"))[0].to(device) for t in targets}


def build_parser():
    p = argparse.ArgumentParser(description="museval's framewise SDR, ISR, SIR, SAR of a music Conv-TasNet on the MUSDB18 test tracks")
    p.add_argument("--model_path", required=True, help="checkpoint package (best.pth / last.pth of the training recipes)")
    p.add_argument("--musdb18_root", required=True, help="directory with test/<track>/{mixture,bass,drums,other,vocals}.wav")
    p.add_argument("--out_dir", default="./musdb18_eval", help="estimates as <track>/<target>.wav and scores as <track>.json go here")
    p.add_argument("--window_s", type=float, default=4.0, help="separation window in seconds: the segment length the model was trained on")
    p.add_argument("--hop_s", type=float, default=None, help="window stride in seconds, window_s / 2 <= hop_s < window_s (default: half the window)")
    p.add_argument("--batch_windows", type=int, default=16, help="windows per forward of the model")
    p.add_argument("--use_cuda", type=int, default=1)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    model = ConvTasNet.build_model(args.model_path, load_state_dict=True)
    device = "cuda" if args.use_cuda else "cpu"
    model = model.to(device)
    rate = SAMPLE_RATE_MUSDB18
    window = int(round(args.window_s * rate))
    hop = None if args.hop_s is None else int(round(args.hop_s * rate))
    return evaluate_tracks(model, musdb18_test_tracks(args.musdb18_root, device), rate, SOURCES, window, hop, args.batch_windows, args.out_dir)


if __name__ == "__main__":
    main()
