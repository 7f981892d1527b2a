"""
Separate one wav file of any length with a trained Conv-TasNet:

    python -m recipes.separate --model_path M.pth --input mix.wav --out_dir D [--window_s 4.0] [--hop_s 2.0] [--batch_windows 16] [--use_cuda 0|1]

The model is built from the checkpoint package (the reference's driver.save_model format: the configuration beside `state_dict`), the mono
wav is read with recipes.audio_io, separated window by window (sepkernels.longform.separate_long: windows of `window_s` seconds at stride
`hop_s`, default half the window, stitched into continuous tracks; a file no longer than one window is one forward) and written as
<name>_<k>.wav, k = 1 .. n_sources, at the input's sample rate and scale.
"""
import argparse
import os

import torch

from models.conv_tasnet import ConvTasNet
from sepkernels.longform import separate_long

from .audio_io import read_wav, wav_info, write_wav


def build_parser():
    p = argparse.ArgumentParser(description="Separate a wav file of any length, window by window")
    p.add_argument("--model_path", required=True, help="checkpoint package (best.pth / last.pth of the training recipes)")
    p.add_argument("--input", required=True, help="mono PCM wav")
    p.add_argument("--out_dir", required=True)
    p.add_argument("--window_s", type=float, default=4.0, help="window length in seconds: the segment length the model was trained on")
    p.add_argument("--hop_s", type=float, default=None, help="window stride in seconds, window_s / 2 <= hop_s < window_s (default: half the window)")
    p.add_argument("--batch_windows", type=int, default=16, help="windows per forward of the model")
    p.add_argument("--use_cuda", type=int, default=1)
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    model = ConvTasNet.build_model(args.model_path, load_state_dict=True)
    mixture, sample_rate = read_wav(args.input)
    if mixture.shape[0] != 1:
        raise ValueError("{} has {} channels, the separator takes a mono recording".format(args.input, mixture.shape[0]))
    window = int(round(args.window_s * sample_rate))
    hop = window // 2 if args.hop_s is None else int(round(args.hop_s * sample_rate))
    if args.use_cuda:
        model, mixture = model.cuda(), mixture.cuda()
    model.eval()
    estimates = separate_long(model, mixture, window, hop=hop, batch_windows=args.batch_windows).cpu()
    os.makedirs(args.out_dir, exist_ok=True)
    name = os.path.splitext(os.path.basename(args.input))[0]
    bits = 32 if wav_info(args.input)[3] == 4 else 16
    paths = []
    for k, est in enumerate(estimates):
        paths.append(os.path.join(args.out_dir, "{}_{}.wav".format(name, k + 1)))
        write_wav(paths[-1], est, sample_rate, bits)
    print("{}: {} samples at {} Hz -> {}".format(args.input, mixture.shape[-1], sample_rate, ", ".join(paths)))
    return paths


if __name__ == "__main__":
    main()
