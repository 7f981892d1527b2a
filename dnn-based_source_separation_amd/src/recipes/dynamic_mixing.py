"""
Corpora for dynamic mixing (sepkernels/mixing.py) from wav files.

* corpus_from_mix_list  a wsj0-mix folder is enough, no raw wsj0 tree: utterance k of mixture `ID` is `wav_root/s<k>/<ID>.wav`, its name is field
                        2 (k - 1) of ID.split("_") (`011a0101_1.5_02bo0302_-1.5`: names 011a0101 and 02bo0302 between their SNRs), its speaker the
                        first three characters of the name.  An utterance that appears in several mixtures is kept once, in its longest copy (the
                        'min' versions of wsj0-mix cut every source to the shorter partner).  The files hold the sources as scaled for THEIR mixture;
                        with normalize=True (default) every utterance is brought to ref_rms by its plain RMS, so those scales do not matter.
* corpus_from_files     the generic builder: one single-channel wav per utterance and a speaker label for each.

Both return a sepkernels.mixing.DeviceCorpus with `names` / `paths` of its utterances in corpus order.  16-bit files are stored as int16 (the round
trip through read_wav is exact).  torch.save(corpus.state_dict(), path) caches the decoded corpus; DeviceCorpus.from_state_dict brings it back.
"""
import os

from sepkernels.mixing import DEFAULT_REF_RMS, DeviceCorpus

from .audio_io import read_wav, wav_info
from .wsj0mix import _read_ids


def corpus_from_files(paths, speakers, dtype="auto", ref_rms=DEFAULT_REF_RMS, normalize=True, device=None, names=None):
    paths = list(paths)
    if len(paths) != len(speakers):
        raise ValueError("{} speaker labels for {} files".format(len(speakers), len(paths)))
    waves = []
    for p in paths:
        x, _ = read_wav(p)
        if x.shape[0] != 1:
            raise ValueError("{} has {} channels: a corpus holds single-channel utterances".format(p, x.shape[0]))
        waves.append(x[0])
    corpus = DeviceCorpus.from_waveforms(waves, speakers, dtype=dtype, ref_rms=ref_rms, normalize=normalize, device=device)
    corpus.paths = [paths[k] for k in corpus.order]
    corpus.names = [(names[k] if names is not None else os.path.splitext(os.path.basename(paths[k]))[0]) for k in corpus.order]
    return corpus


def utterances_of_mix_list(wav_root, list_path, n_sources):
    """-> [(name, speaker, path)] of the distinct utterances behind a mixture list, each in its longest copy, in order of first appearance"""
    best = {}
    for ID in _read_ids(list_path):
        fields = ID.split("_")
        if len(fields) < 2 * n_sources - 1:
            raise ValueError("the mixture ID '{}' does not name {} utterances (name_snr_name_snr...)".format(ID, n_sources))
        for k in range(n_sources):
            name = fields[2 * k]
            if len(name) < 3:
                raise ValueError("the utterance name '{}' of mixture '{}' is shorter than its speaker's three characters".format(name, ID))
            path = os.path.join(os.path.abspath(wav_root), "s{}".format(k + 1), ID + ".wav")
            frames = wav_info(path)[0]
            if name not in best or frames > best[name][0]:
                best[name] = (frames, path)
    return [(name, name[:3], path) for name, (_, path) in best.items()]


def corpus_from_mix_list(wav_root, list_path, n_sources, dtype="auto", ref_rms=DEFAULT_REF_RMS, normalize=True, device=None):
    found = utterances_of_mix_list(wav_root, list_path, n_sources)
    if not found:
        raise ValueError("{} lists no mixture".format(list_path))
    return corpus_from_files([p for _, _, p in found], [s for _, s, _ in found], dtype=dtype, ref_rms=ref_rms, normalize=normalize, device=device,
                             names=[n for n, _, _ in found])


__all__ = ["corpus_from_mix_list", "corpus_from_files", "utterances_of_mix_list"]
