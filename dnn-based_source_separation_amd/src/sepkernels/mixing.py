"""
Dynamic mixing on the device: a training set resident in device memory (DeviceCorpus) and a mixer that draws and renders a fresh batch of
mixtures per step from it (DynamicMixer) -- new speakers, utterances, crops and gains every step, no mixture seen twice, no per-step data work
on the host.  The reference mixes on the fly only for music (egs/musdb18/*/local/train.py with utils/augmentation.py) and in its tutorials
(egs/tutorials/common/src/dataset.py:44); its wsj0-mix recipes serve the fixed mixtures on disk.

The corpus.  All utterances in ONE flat tensor `samples` (int16 or float32; one corpus has one kind) with GUARD = 16 zero elements in front of
the first utterance and behind the last (the render kernel loads whole aligned 16-byte words); `offsets` (U + 1,) int64, utterance u is
samples[offsets[u] : offsets[u + 1]]; `spk_first` (S + 1,) int32, utterances sorted by speaker; `level` (U,) float32 = ref_rms / rms_u with
rms_u the plain RMS of the whole utterance (fp64, samples scaled to [-1, 1)), 0 for a silent one, 1 everywhere with normalize=False.  This is
NOT the ITU-T P.56 active speech level that wsj0-mix's Matlab scripts normalise to: pauses count here, so an utterance with long pauses comes out
louder than there.

The draw (include/sepkernels.h states it in full; tests/test_dynamic_mixing_gpu.py restates it in Python integers), in wrapping uint64:
    mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
    word(seed, item, k) = mix64(mix64(seed + 0x9E3779B97F4A7C15 * (item + 1)) + k),   below(w, m) = ((w >> 32) * m) >> 32
    item = step * (B * world) + rank * B + b
so the global batch of a step is the same set of mixtures however it is cut into ranks.  Gains come from a table of `gain_steps` entries between
gain_db[0] and gain_db[1], built here in fp64: nothing transcendental runs on the device and the plan is reproducible bit for bit.

Speed perturbation (speeds=(95, 100, 105); include/sepkernels.h states it in full).  Every source also draws one of J integer percentages P
(50 .. 200, at most 16, distinct), j = below(word(.., 4 n + 3 + i), J), and is resampled from rate P to rate 100 before it is cropped: tempo and
pitch move together, P > 100 is shorter and higher (sox `speed`), P = 100 is the plain copy.  The filter is sepkernels.resample.get_filter(P, 100)
in its compact form; with g = gcd(P, 100), o = P / g, u = 100 / g the perturbed utterance has len' = ceil(u len / o) samples,
    v[i u + p] = (float)(sum over k < Kc, ascending, in fp64, of (double)table[k][p] * (double)x[i o + first[p] + k - width])
with x the RAW sample (the int16 integer or the fp32 value), zero outside its own utterance, and a row is gain * (v[start + t - lead] * scale) under
the predicate of the plain render with len' in place of len; the position is drawn from len'.  Every product is exact in fp64, so the kernels, numpy
and the host simulation give the same bits.  The level is NOT renormalised after the perturbation (gain = level[u] * gain_table[g] as before: the
RMS of a perturbed utterance differs from the original's by the filter's pass band, about 1e-3), and the noise row is never perturbed.

Routes.  A corpus on the GPU runs csrc/mixing.hip (sep_mix_draw, sep_mix_render; with speeds sep_mix_draw_speed, sep_mix_render_speed).  A corpus on
the CPU -- and any backend without the two methods -- runs the same definitions composed in numpy (uint64 for the draw, an fp64 loop over the taps
for a perturbed row) and torch; both give the same plan and the same bits.

Not offered: perturbing the noise row, non-integer percentages, renormalising the level after the perturbation, peak normalisation of the mixture,
mixtures of mixtures, a multi-channel corpus.
"""
import math

import numpy as np
import torch

import sepkernels

GUARD = sepkernels.MIX_GUARD
MAX_SOURCES = sepkernels.MIX_MAX_SOURCES
MAX_SPEEDS, SPEED_MIN, SPEED_MAX = sepkernels.MIX_MAX_SPEEDS, sepkernels.MIX_SPEED_MIN, sepkernels.MIX_SPEED_MAX
DEFAULT_REF_RMS = 10.0 ** (-25.0 / 20.0)          # -25 dB re full scale, the figure wsj0-mix's scripts normalise the (active) level to
_GOLD, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
_MASK = (1 << 64) - 1


def _mix64(z):
    """z: numpy uint64 array (wrapping arithmetic)"""
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def _below(w, m):
    """w uint64 array, m uint64 array or scalar in [1, 2^31) -> ((w >> 32) * m) >> 32"""
    return ((w >> np.uint64(32)) * np.asarray(m, dtype=np.uint64)) >> np.uint64(32)


def gain_table(lo_db, hi_db, steps):
    """(steps,) float32: (float)10^((lo + (hi - lo) j / (steps - 1)) / 20), formed in fp64"""
    steps = int(steps)
    if steps < 1 or steps >= 1 << 31:
        raise ValueError("gain_steps must be in [1, 2^31), given {}".format(steps))
    if steps == 1:
        if float(lo_db) != float(hi_db):
            raise ValueError("gain_steps = 1 needs gain_db = (x, x), given ({}, {})".format(lo_db, hi_db))
        db = np.array([float(lo_db)], dtype=np.float64)
    else:
        db = float(lo_db) + (float(hi_db) - float(lo_db)) * np.arange(steps, dtype=np.float64) / (steps - 1)
    return torch.from_numpy((10.0 ** (db / 20.0)).astype(np.float32))


class DeviceCorpus:
    """a training set in device memory: samples, offsets, spk_first, level (the module's docstring); build one with from_waveforms,
    recipes.dynamic_mixing.corpus_from_mix_list / corpus_from_files, or from_state_dict"""

    def __init__(self, samples, offsets, spk_first, level, ref_rms=DEFAULT_REF_RMS, device=None):
        """host tensors, checked here BEFORE anything is uploaded; ValueError for an index that is not a corpus"""
        if samples.dim() != 1 or samples.dtype not in (torch.int16, torch.float32):
            raise ValueError("the samples of a corpus are one flat int16 or float32 tensor, given {} of {}".format(samples.dtype, tuple(samples.shape)))
        offsets = offsets.detach().to("cpu", torch.int64).reshape(-1)
        spk_first = spk_first.detach().to("cpu", torch.int64).reshape(-1)
        U, S = offsets.numel() - 1, spk_first.numel() - 1
        if U < 1 or S < 1:
            raise ValueError("a corpus holds at least one utterance of one speaker")
        lengths = offsets[1:] - offsets[:-1]
        if int(lengths.min()) < 1:
            raise ValueError("utterance {} has a length of {}: every utterance holds at least one sample".format(int(lengths.argmin()), int(lengths.min())))
        if int(lengths.max()) >= 1 << 31:
            raise ValueError("utterance {} holds {} samples: a length stays below 2^31".format(int(lengths.argmax()), int(lengths.max())))
        if int(offsets[0]) < GUARD or samples.numel() - int(offsets[-1]) < GUARD:
            raise ValueError("the storage carries at least {} zero elements in front of the first utterance and behind the last".format(GUARD))
        counts = spk_first[1:] - spk_first[:-1]
        if int(spk_first[0]) != 0 or int(spk_first[-1]) != U or int(counts.min()) < 1:
            bad = int(counts.argmin()) if int(counts.min()) < 1 else -1
            raise ValueError("spk_first must run from 0 to U = {} and give every speaker at least one utterance (speaker {} is empty)".format(U, bad) if bad >= 0 else
                             "spk_first must run from 0 to U = {}, given {} .. {}".format(U, int(spk_first[0]), int(spk_first[-1])))
        if level.numel() != U:
            raise ValueError("level has {} entries for {} utterances".format(level.numel(), U))
        head, tail = samples[:int(offsets[0])], samples[int(offsets[-1]):]
        if bool(head.any()) or bool(tail.any()):
            raise ValueError("the guard elements of the storage must be zero")
        self.num_utterances, self.num_speakers, self.ref_rms = U, S, float(ref_rms)
        self.offsets_host = offsets.numpy().copy()                    # the composed route and the checks read the index on the host
        self.spk_first_host = spk_first.numpy().copy()
        dev = torch.device(device) if device is not None else samples.device
        self.samples = samples.detach().to(dev).contiguous()
        self.offsets = offsets.to(dev)
        self.spk_first = spk_first.to(torch.int32).to(dev)
        self.level = level.detach().to(torch.float32).reshape(-1).to(dev).contiguous()

    # ---- builders ----------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_waveforms(cls, waveforms, speakers=None, dtype="auto", ref_rms=DEFAULT_REF_RMS, normalize=True, device=None):
        """waveforms: list of 1-D float tensors in [-1, 1) (or of 1-D int16 tensors, taken as PCM); speakers: a label per waveform (None: one
        speaker owns them all -- a noise corpus).  dtype "auto" stores int16 when every x * 2^15 is an integer in range -- what read_wav returns
        for 16-bit files, so the round trip is exact -- and float32 otherwise; "int16" / "float32" insist."""
        if len(waveforms) < 1:
            raise ValueError("a corpus holds at least one utterance")
        if speakers is None:
            speakers = [0] * len(waveforms)
        if len(speakers) != len(waveforms):
            raise ValueError("{} speaker labels for {} waveforms".format(len(speakers), len(waveforms)))
        kinds = {w.dtype == torch.int16 for w in waveforms}
        if len(kinds) > 1:
            raise ValueError("mixed sample kinds: int16 and floating-point waveforms in one corpus")
        for k, w in enumerate(waveforms):
            if w.dim() != 1:
                raise ValueError("waveform {} has shape {}: a corpus holds 1-D (single-channel) utterances".format(k, tuple(w.shape)))
            if w.numel() < 1:
                raise ValueError("waveform {} has a length of 0".format(k))
            if w.numel() >= 1 << 31:
                raise ValueError("waveform {} holds 2^31 samples or more".format(k))
            if w.dtype != torch.int16 and not w.is_floating_point():
                raise ValueError("waveform {} is {}: int16 or floating point".format(k, w.dtype))
        pcm_in = kinds == {True}
        if dtype not in ("auto", "int16", "float32", torch.int16, torch.float32):
            raise ValueError("dtype must be 'auto', 'int16' or 'float32', given {}".format(dtype))
        want = {"int16": torch.int16, "float32": torch.float32}.get(dtype, dtype)

        def is_pcm(w):
            s = w.detach().double().cpu() * 32768.0
            return bool((s == s.round()).all()) and bool((s >= -32768.0).all()) and bool((s <= 32767.0).all())
        if pcm_in:
            if want == torch.float32:
                raise ValueError("mixed sample kinds: int16 waveforms for a float32 corpus")
            store = torch.int16
        elif want == "auto":
            store = torch.int16 if all(is_pcm(w) for w in waveforms) else torch.float32
        else:
            store = want
            if store == torch.int16 and not all(is_pcm(w) for w in waveforms):
                raise ValueError("mixed sample kinds: a waveform is not 16-bit PCM (x * 2^15 an integer in range), the corpus was asked to be int16")
        labels = sorted(set(speakers), key=lambda s: (str(type(s)), s))
        order = sorted(range(len(waveforms)), key=lambda k: (labels.index(speakers[k]), k))          # by speaker, stable within one
        total = sum(waveforms[k].numel() for k in order)
        samples = torch.zeros(total + 2 * GUARD, dtype=store)
        offsets, level, spk_first, pos, prev = [GUARD], [], [], GUARD, object()
        for j, k in enumerate(order):
            w = waveforms[k].detach().cpu()
            if speakers[k] != prev:
                spk_first.append(j)
                prev = speakers[k]
            if store == torch.int16:
                row = w if pcm_in else (w.double() * 32768.0).to(torch.int16)
                unit = row.double() / 32768.0
            else:
                row = w.to(torch.float32)
                unit = row.double()
            samples[pos:pos + row.numel()] = row
            rms = float(unit.pow(2).mean().sqrt())
            level.append(1.0 if not normalize else (float(ref_rms) / rms if rms > 0.0 else 0.0))
            pos += row.numel()
            offsets.append(pos)
        spk_first.append(len(order))
        corpus = cls(samples, torch.tensor(offsets, dtype=torch.int64), torch.tensor(spk_first, dtype=torch.int64), torch.tensor(level, dtype=torch.float64).float(),
                     ref_rms=ref_rms, device=device)
        corpus.speakers = labels
        corpus.order = order                  # utterance j of the corpus is waveforms[order[j]]
        return corpus

    # ---- plain tensors: torch.save(corpus.state_dict()) caches a decoded corpus --------------------------------------------------------------
    def state_dict(self):
        return {"samples": self.samples.detach().cpu(), "offsets": self.offsets.detach().cpu(), "spk_first": self.spk_first.detach().cpu(),
                "level": self.level.detach().cpu(), "ref_rms": torch.tensor(self.ref_rms, dtype=torch.float64)}

    @classmethod
    def from_state_dict(cls, state, device=None):
        return cls(state["samples"], state["offsets"], state["spk_first"], state["level"], ref_rms=float(state["ref_rms"]), device=device)

    def to(self, device):
        moved = DeviceCorpus.from_state_dict(self.state_dict(), device=device)
        for name in ("speakers", "order", "names", "paths"):           # what the builders know about the utterances travels along
            if hasattr(self, name):
                setattr(moved, name, getattr(self, name))
        return moved

    @property
    def device(self):
        return self.samples.device

    @property
    def dtype(self):
        return self.samples.dtype

    def lengths(self):
        return torch.from_numpy(self.offsets_host[1:] - self.offsets_host[:-1])

    def utterance(self, u):
        """the stored samples of utterance u (a view)"""
        return self.samples[int(self.offsets_host[u]):int(self.offsets_host[u + 1])]

    def speaker_of(self, u):
        return int(np.searchsorted(self.spk_first_host, u, side="right")) - 1


# ---- the composed route: the definitions of include/sepkernels.h in numpy uint64 and torch --------------------------------------------------------
def _place(key, k_pos, k_gain, u, lengths, T, G, ln=None):
    """-> start, lead, gain index (int64 arrays) of rows whose utterances are u (ln: the rows' own lengths where they are not the utterances')"""
    ln = lengths[u].astype(np.int64) if ln is None else ln
    w = _mix64(key + np.uint64(k_pos))
    long_ = ln >= T
    start = np.where(long_, _below(w, np.where(long_, ln - T + 1, 1)), 0).astype(np.int64)
    lead = np.where(long_, 0, _below(w, np.where(long_, 1, T - ln + 1))).astype(np.int64)
    g = _below(_mix64(key + np.uint64(k_gain)), G).astype(np.int64)
    return start, lead, g


def check_speeds(speeds):
    """-> the speeds as a tuple of ints; ValueError for anything sep_mix_draw_speed does not take"""
    try:
        given = list(speeds)
    except TypeError:
        raise ValueError("speeds is a list of integer percentages, given {!r}".format(speeds))
    if len(given) < 1:
        raise ValueError("speeds is empty: at least one percentage (None switches speed perturbation off)")
    if len(given) > MAX_SPEEDS:
        raise ValueError("{} speeds, at most {}".format(len(given), MAX_SPEEDS))
    out = []
    for P in given:
        if isinstance(P, bool) or not isinstance(P, (int, float, np.integer, np.floating)) or not math.isfinite(P) or int(P) != P:
            raise ValueError("a speed is an integer percentage, given {!r}".format(P))
        if not SPEED_MIN <= int(P) <= SPEED_MAX:
            raise ValueError("a speed lies in [{}, {}] percent, given {}".format(SPEED_MIN, SPEED_MAX, int(P)))
        out.append(int(P))
    if len(set(out)) != len(out):
        raise ValueError("duplicate speeds in {}".format(out))
    return tuple(out)


class SpeedFilters:
    """the filters of a list of speeds as sep_mix_render_speed takes them: desc (J, 8) int32 {o, u, width, Kc, table offset, first offset, P, 0},
    table fp32 and first int32 of every speed one behind the other (host tensors; an identity speed has no filter)"""

    def __init__(self, speeds):
        from sepkernels.resample import get_filter
        self.speeds = check_speeds(speeds)
        desc, tables, firsts, self.filters = [], [], [], []
        toff = foff = 0
        for P in self.speeds:
            if P == 100:
                desc.append([1, 1, 0, 1, 0, 0, 100, 0])
                self.filters.append(None)
                continue
            f = get_filter(P, 100)
            if f.Kc > sepkernels.MIX_SPEED_MAX_TAPS or f.u > 100 or f.o > SPEED_MAX:
                raise ValueError("the filter of speed {} has {} taps of {} phases: beyond what the kernels take".format(P, f.Kc, f.u))
            desc.append([f.o, f.u, f.width, f.Kc, toff, foff, P, 0])
            tables.append(f.table.reshape(-1))
            firsts.append(f.first.reshape(-1))
            toff, foff = toff + f.Kc * f.u, foff + f.u
            self.filters.append(f)
        self.desc = torch.tensor(desc, dtype=torch.int32)
        self.table = torch.cat(tables).contiguous() if tables else torch.zeros(1, dtype=torch.float32)
        self.first = torch.cat(firsts).to(torch.int32).contiguous() if firsts else torch.zeros(1, dtype=torch.int32)

    def length(self, j, length):
        """len' of an utterance of `length` samples at speed j"""
        o, u = int(self.desc[j, 0]), int(self.desc[j, 1])
        return min(max((u * int(length) + o - 1) // o, 1), (1 << 31) - 1)


def draw_composed(corpus, noise, table, noise_table, seed, step, item_stride, item_first, B, n, T, speeds=None):
    """-> plan (B, R, 4) int64 and gain (B, R) float32, on the CPU: what sep_mix_draw writes for step `step`; with speeds (a list of percentages or a
    SpeedFilters) also speed (B, R) int32: what sep_mix_draw_speed writes"""
    if speeds is not None and not isinstance(speeds, SpeedFilters):
        speeds = SpeedFilters(speeds)
    first = (int(step) * int(item_stride) + int(item_first)) & _MASK
    item = np.array([(first + b) & _MASK for b in range(B)], dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = _mix64(np.uint64(int(seed) & _MASK) + _GOLD * (item + np.uint64(1)))
        S, spk, lengths = corpus.num_speakers, corpus.spk_first_host, corpus.offsets_host[1:] - corpus.offsets_host[:-1]
        R = n + (1 if noise is not None else 0)
        plan = np.zeros((B, R, 4), dtype=np.int64)
        speed = np.full((B, R), -1, dtype=np.int32)
        taken = np.zeros((B, 0), dtype=np.int64)                    # ascending per item
        for i in range(n):
            r = _below(_mix64(key + np.uint64(i)), S - i).astype(np.int64)
            for c in range(i):
                r = r + (r >= taken[:, c])
            taken = np.sort(np.concatenate([taken, r[:, None]], axis=1), axis=1)
            u = spk[r] + _below(_mix64(key + np.uint64(n + i)), spk[r + 1] - spk[r]).astype(np.int64)
            ln = None
            if speeds is not None:
                j = _below(_mix64(key + np.uint64(4 * n + 3 + i)), len(speeds.speeds)).astype(np.int64)
                speed[:, i] = j
                o, up = speeds.desc[:, 0].numpy().astype(np.int64)[j], speeds.desc[:, 1].numpy().astype(np.int64)[j]
                ln = np.clip((up * lengths[u].astype(np.int64) + o - 1) // o, 1, (1 << 31) - 1)          # len' of every row
            start, lead, g = _place(key, 2 * n + i, 3 * n + i, u, lengths, T, table.numel(), ln)
            plan[:, i] = np.stack([u, start, lead, g], axis=1)
        if noise is not None:
            nl = noise.offsets_host[1:] - noise.offsets_host[:-1]
            u = _below(_mix64(key + np.uint64(4 * n)), noise.num_utterances).astype(np.int64)
            start, lead, g = _place(key, 4 * n + 1, 4 * n + 2, u, nl, T, noise_table.numel())
            plan[:, n] = np.stack([u, start, lead, g], axis=1)
    plan = torch.from_numpy(plan)
    gain = corpus.level.detach().cpu()[plan[:, :n, 0]] * table.cpu()[plan[:, :n, 3]]
    if noise is not None:
        gain = torch.cat([gain, noise.level.detach().cpu()[plan[:, n:, 0]] * noise_table.cpu()[plan[:, n:, 3]]], dim=1)
    if speeds is not None:
        return plan, gain.contiguous(), torch.from_numpy(speed)
    return plan, gain.contiguous()


def _render_row(corpus, row, g, T):
    """one row of a plan on the corpus's device: the formula of sep_mix_render with its clamps and its predicate"""
    U = corpus.num_utterances
    u = min(max(int(row[0]), 0), U - 1)
    o0, ln = int(corpus.offsets_host[u]), int(corpus.offsets_host[u + 1] - corpus.offsets_host[u])
    start = max(min(int(row[1]), ln - 1), 0)
    lead = min(max(int(row[2]), -(1 << 40)), 1 << 40)               # beyond +-2^40 no sample passes the predicate either way
    t = torch.arange(T, dtype=torch.int64, device=corpus.device)
    inside = (t >= lead) & (t - lead < ln - start)
    idx = torch.where(inside, o0 + start + t - lead, torch.full_like(t, o0))
    scale = 2.0 ** -15 if corpus.dtype == torch.int16 else 1.0
    val = g * (corpus.samples[idx].to(torch.float32) * scale)
    return torch.where(inside, val, torch.zeros_like(val))


def _render_row_speed(corpus, row, g, T, flt):
    """one perturbed row: the formula of sep_mix_render_speed with its clamps and its predicate, the taps summed in fp64 in numpy"""
    U = corpus.num_utterances
    uu = min(max(int(row[0]), 0), U - 1)
    o0, ln = int(corpus.offsets_host[uu]), int(corpus.offsets_host[uu + 1] - corpus.offsets_host[uu])
    o, u, width, Kc = flt.o, flt.u, flt.width, flt.Kc
    lenp = min(max((u * ln + o - 1) // o, 1), (1 << 31) - 1)
    start = max(min(int(row[1]), lenp - 1), 0)
    lead = min(max(int(row[2]), -(1 << 40)), 1 << 40)
    t = np.arange(T, dtype=np.int64)
    inside = (t >= lead) & (t - lead < lenp - start)
    m = np.where(inside, start + t - lead, 0)
    i, p = m // u, m % u
    x = corpus.samples[o0:o0 + ln].detach().cpu().numpy().astype(np.float64)
    table, first = flt.table.numpy(), flt.first.numpy().astype(np.int64)
    acc = np.zeros(T, dtype=np.float64)
    for k in range(Kc):
        idx = i * o + first[p] + k - width
        ok = (idx >= 0) & (idx < ln)
        acc = acc + table[k, p].astype(np.float64) * np.where(ok, x[np.clip(idx, 0, ln - 1)], 0.0)
    v = torch.from_numpy(acc.astype(np.float32)).to(corpus.device)
    scale = 2.0 ** -15 if corpus.dtype == torch.int16 else 1.0
    val = g * (v * scale)
    return torch.where(torch.from_numpy(inside).to(corpus.device), val, torch.zeros_like(val))


def render_composed(corpus, noise, plan, gain, n, T, speeds=None, speed=None):
    """-> sources (B, n, T), mixture (B, 1, T)[, noise (B, 1, T)] float32 on the corpus's device: what sep_mix_render writes for this plan; with speeds
    (a list of percentages or a SpeedFilters) and speed (B, R): what sep_mix_render_speed writes"""
    B, R = plan.shape[0], plan.shape[1]
    if (speeds is None) != (speed is None):
        raise ValueError("speeds and the speed indices of a plan come together or not at all")
    if speeds is not None:
        if not isinstance(speeds, SpeedFilters):
            speeds = SpeedFilters(speeds)
        if tuple(speed.shape) != (B, R):
            raise ValueError("the speed indices of a plan of {} rows per item are ({}, {}), given {}".format(R, B, R, tuple(speed.shape)))
        picks, J = speed.detach().cpu().tolist(), len(speeds.speeds)

        def one(b, i, g):
            j = min(max(picks[b][i], -1), J - 1)
            flt = speeds.filters[j] if j >= 0 else None
            return _render_row(corpus, rows[b][i], g, T) if flt is None else _render_row_speed(corpus, rows[b][i], g, T, flt)
    else:
        def one(b, i, g):
            return _render_row(corpus, rows[b][i], g, T)
    if R != n + (1 if noise is not None else 0):
        raise ValueError("the plan has {} rows per item, {} sources{} need {}".format(R, n, " and a noise row" if noise is not None else "", n + (noise is not None)))
    rows, gains = plan.detach().cpu().tolist(), gain.detach().to(corpus.device, torch.float32)
    sources = torch.stack([torch.stack([one(b, i, gains[b, i]) for i in range(n)]) for b in range(B)])
    mixture = sources[:, 0]
    for i in range(1, n):
        mixture = mixture + sources[:, i]
    if noise is None:
        return sources, mixture.unsqueeze(1).contiguous()
    extra = torch.stack([_render_row(noise, rows[b][n], gains[b, n], T) for b in range(B)]).unsqueeze(1)
    return sources, (mixture.unsqueeze(1) + extra).contiguous(), extra


# ---- the public interface -------------------------------------------------------------------------------------------------------------------------
class DynamicMixer:
    """mixer = DynamicMixer(corpus, n_sources=2, samples=32000, batch_size=16, seed=111)
    mixture, sources = mixer()            # (B, 1, T), (B, n, T) float32 on the corpus's device; with noise=...: (mixture, sources, noise)
    mixer.plan                            # the last draw: ((B, R, 4) int64 {utterance, start, lead, gain index}, (B, R) gains), for logging and render()
    mixer.step, mixer.seek(step), mixer.state_dict(), mixer.load_state_dict(...)      # {seed, step}: a resumed run continues the stream
    DynamicMixer(..., speeds=(95, 100, 105))      # speed perturbation of every source (the module's docstring): draw() -> (plan, gain, speed),
    mixer.speed                                   # (B, R) int32, the index into speeds per row (-1: the noise row); render(plan, gain, speed)"""

    def __init__(self, corpus, n_sources=2, samples=32000, batch_size=16, seed=111, gain_db=(-2.5, 2.5), gain_steps=256, noise=None,
                 noise_gain_db=(-6.0, 3.0), rank=None, world=None, composed=False, speeds=None):
        """rank / world default to torch.distributed's when it is initialised (else 0 of 1); composed=True keeps a mixer off the kernels (the composed
        route on whatever device the corpus is on: the same plan and the same bits)"""
        n, T, B = int(n_sources), int(samples), int(batch_size)
        if n < 1 or n > MAX_SOURCES:
            raise ValueError("n_sources must be in [1, {}], given {}".format(MAX_SOURCES, n))
        if n > corpus.num_speakers:
            raise ValueError("{} sources of distinct speakers from a corpus of {} speakers".format(n, corpus.num_speakers))
        if T < 1 or T >= 1 << 31:
            raise ValueError("samples must be in [1, 2^31), given {}".format(T))
        if B < 1 or B > 65535:
            raise ValueError("batch_size must be in [1, 65535], given {}".format(B))
        filters = SpeedFilters(speeds) if speeds is not None else None          # (its ValueErrors come before anything is uploaded)
        if noise is not None:
            if noise.dtype != corpus.dtype:
                raise ValueError("the noise corpus holds {}, the corpus {}: one sample kind".format(noise.dtype, corpus.dtype))
            if noise.device != corpus.device:
                raise ValueError("the noise corpus is on {}, the corpus on {}".format(noise.device, corpus.device))
        if rank is None or world is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank = (dist.get_rank() if on else 0) if rank is None else rank
            world = (dist.get_world_size() if on else 1) if world is None else world
        if int(world) < 1 or not 0 <= int(rank) < int(world):
            raise ValueError("rank {} of world {}".format(rank, world))
        self.corpus, self.noise, self.n_sources, self.samples, self.batch_size = corpus, noise, n, T, B
        self.seed, self.rank, self.world = int(seed) & _MASK, int(rank), int(world)
        dev = corpus.device
        self.gain_table = gain_table(gain_db[0], gain_db[1], gain_steps).to(dev)
        self.noise_gain_table = gain_table(noise_gain_db[0], noise_gain_db[1], gain_steps).to(dev) if noise is not None else None
        self.composed = bool(composed)
        self._step = 0
        self._counter = torch.zeros(1, dtype=torch.int64, device=dev)      # the step as the draw kernel reads and advances it
        self.plan = None
        self.speeds, self.speed, self._filters = (filters.speeds if filters else None), None, filters
        if filters is not None:
            self._desc, self._ftable, self._ffirst = filters.desc.to(dev), filters.table.to(dev), filters.first.to(dev)

    @property
    def rows(self):
        return self.n_sources + (1 if self.noise is not None else 0)

    def _on_kernels(self):
        K = sepkernels.backend()
        if self.composed:
            return False
        names = ("mix_draw", "mix_render") if self.speeds is None else ("mix_draw_speed", "mix_render_speed")
        return self.corpus.samples.is_cuda or (K.name != "hip" and all(hasattr(K, name) for name in names))

    @property
    def step(self):
        """the step the next call draws"""
        return self._step

    def seek(self, step):
        self._step = int(step)
        self._counter.fill_(self._step)

    def state_dict(self):
        state = {"seed": self.seed, "step": self._step}
        if self.speeds is not None:
            state["speeds"] = list(self.speeds)
        return state

    def load_state_dict(self, state):
        theirs = state.get("speeds")
        if (None if theirs is None else tuple(int(P) for P in theirs)) != self.speeds:
            raise ValueError("the state was written with speeds {}, this mixer has {}: the stream would differ".format(theirs, self.speeds))
        self.seed = int(state["seed"]) & _MASK
        self.seek(int(state["step"]))

    def draw(self):
        """-> (plan, gain) of this step on the corpus's device -- with speeds (plan, gain, speed); advances the step"""
        c, nz, B, n, T = self.corpus, self.noise, self.batch_size, self.n_sources, self.samples
        stride, first = B * self.world, self.rank * B
        speed = None
        if self._on_kernels():
            plan = torch.empty(B, self.rows, 4, dtype=torch.int64, device=c.device)
            gain = torch.empty(B, self.rows, dtype=torch.float32, device=c.device)
            if self.speeds is not None:
                speed = torch.empty(B, self.rows, dtype=torch.int32, device=c.device)
                sepkernels.backend().mix_draw_speed(c.offsets, c.spk_first, c.num_utterances, c.num_speakers, None if nz is None else nz.offsets,
                                                    0 if nz is None else nz.num_utterances, c.level, self.gain_table, self.gain_table.numel(),
                                                    None if nz is None else nz.level, self.noise_gain_table, 0 if nz is None else self.noise_gain_table.numel(),
                                                    self._counter, self.seed, stride, first, B, n, T, self._desc, len(self.speeds), plan, gain, speed)
            else:
                sepkernels.backend().mix_draw(c.offsets, c.spk_first, c.num_utterances, c.num_speakers, None if nz is None else nz.offsets,
                                              0 if nz is None else nz.num_utterances, c.level, self.gain_table, self.gain_table.numel(),
                                              None if nz is None else nz.level, self.noise_gain_table, 0 if nz is None else self.noise_gain_table.numel(),
                                              self._counter, self.seed, stride, first, B, n, T, plan, gain)
        else:
            out = draw_composed(c, nz, self.gain_table, self.noise_gain_table, self.seed, self._step, stride, first, B, n, T, speeds=self._filters)
            plan, gain = out[0].to(c.device), out[1].to(c.device)
            speed = out[2].to(c.device) if self.speeds is not None else None
            self._counter += 1
        self._step += 1
        self.plan, self.speed = (plan, gain), speed
        return (plan, gain) if self.speeds is None else (plan, gain, speed)

    def render(self, plan, gain, speed=None):
        """-> (mixture, sources[, noise]) of a plan (this mixer's or a logged one); a mixer with speeds takes the plan's speed indices too"""
        c, nz, n, T = self.corpus, self.noise, self.n_sources, self.samples
        B = plan.shape[0]
        if tuple(plan.shape) != (B, self.rows, 4) or tuple(gain.shape) != (B, self.rows) or B < 1:
            raise ValueError("a plan is (B, {}, 4) int64 with gains (B, {}), given {} and {}".format(self.rows, self.rows, tuple(plan.shape), tuple(gain.shape)))
        if (speed is None) != (self.speeds is None) or (speed is not None and tuple(speed.shape) != (B, self.rows)):
            raise ValueError("a mixer with speeds renders (plan, gain, speed) with speed ({}, {}) int32, one without renders (plan, gain); given speed {}".format(
                B, self.rows, None if speed is None else tuple(speed.shape)))
        if self._on_kernels():
            sources = torch.empty(B, n, T, dtype=torch.float32, device=c.device)
            mixture = torch.empty(B, 1, T, dtype=torch.float32, device=c.device)
            extra = torch.empty(B, 1, T, dtype=torch.float32, device=c.device) if nz is not None else None
            if self.speeds is not None:
                sepkernels.backend().mix_render_speed(c.samples, c.offsets, c.num_utterances, None if nz is None else nz.samples, None if nz is None else nz.offsets,
                                                      0 if nz is None else nz.num_utterances, plan.to(torch.int64).contiguous(), gain.to(torch.float32).contiguous(),
                                                      speed.to(c.device, torch.int32).contiguous(), self._desc, len(self.speeds), self._ftable, self._ffirst, B, n, T,
                                                      sources, mixture, extra)
                return (mixture, sources) if nz is None else (mixture, sources, extra)
            sepkernels.backend().mix_render(c.samples, c.offsets, c.num_utterances, None if nz is None else nz.samples, None if nz is None else nz.offsets,
                                            0 if nz is None else nz.num_utterances, plan.to(torch.int64).contiguous(), gain.to(torch.float32).contiguous(), B, n, T,
                                            sources, mixture, extra)
            return (mixture, sources) if nz is None else (mixture, sources, extra)
        out = render_composed(c, nz, plan, gain, n, T, speeds=self._filters, speed=speed)
        return (out[1], out[0]) if nz is None else (out[1], out[0], out[2])

    def __call__(self):
        with torch.no_grad():
            return self.render(*self.draw())


__all__ = ["DeviceCorpus", "DynamicMixer", "SpeedFilters", "check_speeds", "gain_table", "draw_composed", "render_composed", "GUARD", "MAX_SOURCES", "MAX_SPEEDS",
           "SPEED_MIN", "SPEED_MAX", "DEFAULT_REF_RMS"]
