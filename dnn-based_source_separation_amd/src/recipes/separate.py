"""
Separate one wav file of any length with a trained Conv-TasNet:

    python -m recipes.separate --model_path M.pth --input mix.wav --out_dir D [--window_s 4.0] [--hop_s 2.0] [--batch_windows 16] [--use_cuda 0|1]
                               [--model_rate HZ]

The model is built from the checkpoint package (the reference's driver.save_model format: the configuration beside `state_dict`), the mono
wav is read with recipes.audio_io, separated window by window (sepkernels.longform.separate_long: windows of `window_s` seconds at stride
`hop_s`, default half the window, stitched into continuous tracks; a file no longer than one window is one forward) and written as
<name>_<k>.wav, k = 1 .. n_sources, at the input's sample rate and scale.  Without --model_rate the samples go to the model at the wav's own
rate.  With it, a wav of another rate is resampled to the model's (sepkernels.resample), the windows are taken at that rate, and the estimates
are resampled back and cropped or zero-padded to the input's length.
"""
import argparse
import os

import torch
import torch.nn.functional as F

from models.conv_tasnet import ConvTasNet
from sepkernels.longform import separate_long
from sepkernels.resample import resample

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
    p.add_argument("--model_rate", type=int, default=None, help="sample rate in Hz the model was trained at: a wav of another rate is resampled to it and "
                   "the estimates back (default: the wav is handed to the model at its own rate)")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    model = ConvTasNet.build_model(args.model_path, load_state_dict=True)
    mixture, sample_rate = read_wav(args.input)
    if mixture.shape[0] != 1:
        raise ValueError("{} has {} channels, the separator takes a mono recording".format(args.input, mixture.shape[0]))
    convert = args.model_rate is not None and args.model_rate != sample_rate
    rate = args.model_rate if convert else sample_rate
    window = int(round(args.window_s * rate))
    hop = window // 2 if args.hop_s is None else int(round(args.hop_s * rate))
    if args.use_cuda:
        model, mixture = model.cuda(), mixture.cuda()
    model.eval()
    if convert:
        length = mixture.shape[-1]
        estimates = separate_long(model, resample(mixture, sample_rate, rate), window, hop=hop, batch_windows=args.batch_windows)
        estimates = resample(estimates.contiguous(), rate, sample_rate)
        estimates = F.pad(estimates, (0, max(0, length - estimates.shape[-1])))[..., :length].cpu()
    else:
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
