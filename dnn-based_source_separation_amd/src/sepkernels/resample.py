"""
Sample-rate conversion on the device: whole signals (resample, Resample) and online streams (StreamResampler).

The recipes hand a model samples at the rate it was trained at; live audio and most recordings come at another one.  The reference calls
torchaudio.transforms.Resample for this (egs/musdb18/common/src/dataset.py:623); that package is not on our machines, so the definition of
torchaudio.functional.resample is restated here (and in include/sepkernels.h).  With g = gcd(orig_freq, new_freq), o = orig_freq / g,
u = new_freq / g, lpw = lowpass_filter_width, all in fp64:
    base  = min(o, u) rolloff,   width = ceil(lpw o / base),   K = 2 width + o
    t[p][k] = clamp(((k - width) / o - p / u) base, -lpw, lpw)
    h[p][k] = sinc(pi t) w(t) base / o,    w = cos(pi t / (2 lpw))^2 (sinc_interp_hann) or i0(beta sqrt(1 - (t / lpw)^2)) / i0(beta) (sinc_interp_kaiser)
    y[i u + p] = sum_k h[p][k] x[i o + k - width],   x = 0 outside [0, T),   T_out = ceil(u T / o)
Most of the K taps of a phase are zero: the window ends where |t| reaches lpw.  The kernels (csrc/resample.hip) take the COMPACT table: per
phase the run between the first and the last tap of at least 2^-60 of the phase's largest, Kc taps from first[p] on for the longest run
(67 of 509 at 44.1 k -> 8 k).  The rule reads the fp64 values, so it holds for any method, width and rolloff.

Routes.  Contiguous fp32 device tensors that do not require grad run the kernels; CPU tensors, other dtypes, views with strides, tensors that
require grad and a filter the kernels refuse (include/sepkernels.h lists what) run the same definition composed in torch --
F.pad + F.conv1d(stride = o) + reshape + crop -- which is differentiable.

Streams.  StreamResampler mirrors the online separator's contract.  D = ceil(width / o) o.  A stream starts with D zero samples of pre-roll;
a chunk of m o samples returns m u; flush() returns the last D / o * u and resets; for x of n o samples
    cat([rs(c) for c in chunks] + [rs.flush()]) == resample(pad(x, (D, 0)))
bit for bit on the kernel route, however x is cut.  The delay is D input samples, the state the last H = width + D samples per stream.
Not offered: a length per stream in one call (ragged), export / import of the state, recording a resampler into a sepkernels.Sequence.
"""
import functools
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

import sepkernels

DROP = 2.0 ** -60                  # taps below this fraction of their phase's largest, at either end of the phase, are left out
_KAISER_BETA = 14.769656459379492
# what csrc/resample.hip takes (include/sepkernels.h): the staged span, the phases, the table's LDS, the history, outputs per tile
_SPAN, _PHASES, _TAB_FRAMES, _TAB, _HISTORY, _OUT = 8192, 1024, 2048, 6144, 2048, 2048


class Filter:
    """the polyphase filter of one conversion: o, u, width, K; h (u, K) fp64; first (u,) and Kc of the compact form; D and H of a stream"""

    def __init__(self, orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta):
        if int(orig_freq) != orig_freq or int(new_freq) != new_freq or orig_freq <= 0 or new_freq <= 0:
            raise ValueError("resample takes positive integer frequencies, given {} and {}".format(orig_freq, new_freq))
        if resampling_method == "sinc_interpolation":          # the name before torchaudio 0.13
            resampling_method = "sinc_interp_hann"
        if resampling_method not in ("sinc_interp_hann", "sinc_interp_kaiser"):
            raise ValueError("resampling_method must be sinc_interp_hann or sinc_interp_kaiser, given {}".format(resampling_method))
        if lowpass_filter_width <= 0:
            raise ValueError("lowpass_filter_width must be positive")
        g = math.gcd(int(orig_freq), int(new_freq))
        self.o, self.u = o, u = int(orig_freq) // g, int(new_freq) // g
        lpw = lowpass_filter_width
        base = min(o, u) * rolloff
        self.width = width = int(math.ceil(lpw * o / base))
        self.K = K = 2 * width + o
        k = torch.arange(-width, width + o, dtype=torch.float64).view(1, K) / o
        p = torch.arange(0, -u, -1, dtype=torch.float64).view(u, 1) / u
        t = ((k + p) * base).clamp_(-lpw, lpw)
        if resampling_method == "sinc_interp_hann":
            window = torch.cos(t * math.pi / lpw / 2) ** 2
        else:
            b = torch.tensor(_KAISER_BETA if beta is None else float(beta), dtype=torch.float64)
            window = torch.i0(b * torch.sqrt(1 - (t / lpw) ** 2)) / torch.i0(b)
        t = t * math.pi
        self.h = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / torch.where(t == 0, torch.ones_like(t), t)) * window * (base / o)
        keep = self.h.abs() >= DROP * self.h.abs().amax(1, keepdim=True)
        lo = keep.to(torch.int64).argmax(1)
        hi = K - 1 - keep.flip(1).to(torch.int64).argmax(1)
        self.Kc = Kc = int((hi - lo + 1).max())
        self.first = torch.minimum(lo, torch.full_like(lo, K - Kc)).to(torch.int32)       # a short run is padded with the phase's own next taps
        cols = self.first.to(torch.int64).view(u, 1) + torch.arange(Kc).view(1, Kc)
        self.table = self.h.gather(1, cols).t().contiguous().float()                     # (Kc, u): tap-major
        self.D = -(-width // o) * o
        self.H = width + self.D
        self._dev = {}

    def on(self, device):
        """(table, first) on `device`, uploaded once"""
        got = self._dev.get(device)
        if got is None:
            got = self._dev[device] = (self.table.to(device), self.first.to(device))
        return got

    def tile_frames(self):
        """frames per workgroup as csrc/resample.hip chooses them"""
        return min((_SPAN - self.K) // self.o + 1, _OUT if self.u <= 3 and self.Kc * self.u <= _TAB_FRAMES else max(1, _OUT // self.u))

    def kernels_take_it(self):
        return self.K <= _SPAN and self.u <= _PHASES and self.Kc * self.u <= _TAB

    def kernels_take_a_stream(self, m):
        ft = self.tile_frames() if self.kernels_take_it() else 0
        return ft > 0 and self.H <= _HISTORY and (m <= ft or ft * self.o >= self.H)

    def conv(self, x, crop):
        """(R, T') -> (R, crop): the K taps of every phase at stride o on x as it is (the caller has padded it)"""
        R = x.shape[0]
        y = F.conv1d(x.unsqueeze(1), self.h.to(device=x.device, dtype=x.dtype).unsqueeze(1), stride=self.o)
        return y.transpose(1, 2).reshape(R, -1)[:, :crop]


@functools.lru_cache(maxsize=64)
def _filter(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta):
    return Filter(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)


def get_filter(orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """the cached Filter of a conversion (one table per set of arguments, one upload per device)"""
    return _filter(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)


def _on_kernels(t):
    """contiguous fp32 without a tape where the backend's kernels can take it: the device beside the HIP library, any tensor beside another backend"""
    return (t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad and t.numel() > 0
            and (t.is_cuda or sepkernels.backend().name != "hip"))


def _apply(flt, waveform):
    if not waveform.is_floating_point():
        raise ValueError("resample takes a floating-point waveform, given {}".format(waveform.dtype))
    if waveform.dim() < 1:
        raise ValueError("resample takes a waveform of (..., time)")
    if flt.o == flt.u:
        return waveform
    lead, T = waveform.shape[:-1], waveform.shape[-1]
    T_out = -(-flt.u * T // flt.o)
    if waveform.numel() == 0:
        return waveform.new_zeros(lead + (T_out,))
    if flt.kernels_take_it() and _on_kernels(waveform):
        R = waveform.numel() // T
        table, first = flt.on(waveform.device)
        y = torch.empty(lead + (T_out,), device=waveform.device, dtype=torch.float32)
        sepkernels.backend().resample_fwd(waveform, T, table, first, y, T_out, R, T, T_out, flt.o, flt.u, flt.width, flt.Kc)
        return y
    x = F.pad(waveform.reshape(-1, T), (flt.width, flt.width + flt.o))
    return flt.conv(x, T_out).reshape(lead + (T_out,))


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None):
    """torchaudio.functional.resample: waveform (..., T) at orig_freq -> (..., ceil(new_freq T / orig_freq)) at new_freq; the input itself if the
    two are equal"""
    return _apply(get_filter(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta), waveform)


class Resample(nn.Module):
    """torchaudio.transforms.Resample: no parameters, no state_dict entries; the table is built once and uploaded once per device"""

    def __init__(self, orig_freq=16000, new_freq=16000, resampling_method="sinc_interp_hann", lowpass_filter_width=6, rolloff=0.99, beta=None, *, dtype=None):
        super().__init__()
        self.orig_freq, self.new_freq, self.resampling_method = orig_freq, new_freq, resampling_method
        self.lowpass_filter_width, self.rolloff, self.beta = lowpass_filter_width, rolloff, beta
        self._filter = get_filter(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)

    def forward(self, waveform):
        return _apply(self._filter, waveform)

    def extra_repr(self):
        return "orig_freq={}, new_freq={}, resampling_method={}".format(self.orig_freq, self.new_freq, self.resampling_method)


class StreamResampler:
    """num_streams independent streams (each of `channels` rows) through one conversion, chunk by chunk.

        rs = StreamResampler(64, 16000, 8000, device="cuda")
        y = rs(chunk)                    # chunk (64, m o) -> (64, m u); with channels = C: (64, C, m o) -> (64, C, m u)
        y = rs(chunk, streams=[3, 1])    # row j belongs to stream streams[j]; the others are neither read nor advanced
        tail = rs.flush()                # the last D / o * u samples of every stream (of streams=...), which then start anew
    """

    def __init__(self, num_streams, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method="sinc_interp_hann", beta=None,
                 device=None, dtype=torch.float32, channels=1):
        if int(num_streams) < 1 or int(channels) < 1:
            raise ValueError("a StreamResampler has at least one stream and one channel")
        self.num_streams, self.channels = int(num_streams), int(channels)
        self.filter = flt = get_filter(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta)
        self.identity = flt.o == flt.u
        self.o, self.u = flt.o, flt.u
        self.D, self.H = (0, 0) if self.identity else (flt.D, flt.H)
        self.history = torch.zeros(self.num_streams, self.channels, self.H, device=device, dtype=dtype)

    @property
    def delay(self):
        """input samples between a sample's arrival and the output it is the centre of"""
        return self.D

    @property
    def state_bytes(self):
        return self.history.numel() * self.history.element_size()

    def _select(self, streams):
        """-> the selected stream indices in call order, checked as OnlineSeparator._select checks them"""
        Bs = self.num_streams
        if torch.is_tensor(streams) and streams.dtype == torch.bool:
            if streams.numel() != Bs:
                raise ValueError("the stream mask has {} entries, the resampler has {} streams".format(streams.numel(), Bs))
            idx = torch.nonzero(streams.reshape(-1)).reshape(-1).tolist()
        else:
            idx = [int(i) for i in (streams.reshape(-1).tolist() if torch.is_tensor(streams) else streams)]
        if not idx:
            raise ValueError("the selection of streams is empty")
        if any(i < 0 or i >= Bs for i in idx):
            raise ValueError("stream index out of range 0 .. {}".format(Bs - 1))
        if len(set(idx)) != len(idx):
            raise ValueError("duplicate stream indices in the selection: every selected stream takes one row of the chunk")
        return idx

    def _rows(self, idx):
        """the history rows (stream, channel) of a selection, as the kernel's slot list"""
        C = self.channels
        return torch.tensor([s * C + c for s in idx for c in range(C)], dtype=torch.int32, device=self.history.device)

    def __call__(self, chunk, streams=None):
        idx = None if streams is None else self._select(streams)
        A, C = self.num_streams if idx is None else len(idx), self.channels
        want = (A, chunk.shape[-1]) if C == 1 and chunk.dim() == 2 else (A, C, chunk.shape[-1])
        if tuple(chunk.shape) != want or chunk.shape[-1] < 1:
            raise ValueError("the chunk must be ({}, {}samples) for {} streams, given {}".format(A, "{}, ".format(C) if C > 1 else "", A, tuple(chunk.shape)))
        n = chunk.shape[-1]
        if n % self.o:
            raise ValueError("a chunk of a {} -> {} stream holds a multiple of {} samples, given {}".format(self.o, self.u, self.o, n))
        if chunk.device != self.history.device or chunk.dtype != self.history.dtype:
            raise ValueError("the chunk must be {} on {}, given {} on {}".format(self.history.dtype, self.history.device, chunk.dtype, chunk.device))
        if self.identity:
            return chunk.clone()
        m, flt = n // self.o, self.filter
        with torch.no_grad():
            hist = self.history.view(self.num_streams * C, self.H)
            if flt.kernels_take_a_stream(m) and _on_kernels(chunk):
                table, first = flt.on(chunk.device)
                y = torch.empty(A * C, m * self.u, device=chunk.device, dtype=torch.float32)
                sepkernels.backend().resample_stream_fwd(chunk, table, first, hist, y, None if idx is None else self._rows(idx), A * C,
                                                         self.num_streams * C, m, self.o, self.u, flt.width, flt.Kc)
            else:
                rows = slice(None) if idx is None else self._rows(idx).long()
                cat = torch.cat([hist[rows], chunk.reshape(A * C, n)], 1)
                y = flt.conv(cat, m * self.u)
                hist[rows] = cat[:, n:]
        return y.view(chunk.shape[:-1] + (m * self.u,))

    def flush(self, streams=None):
        """-> (A, [channels,] D / o * u): what the D samples of delay still hold; the flushed streams start anew"""
        A = self.num_streams if streams is None else len(self._select(streams))
        shape = (A, self.D) if self.channels == 1 else (A, self.channels, self.D)
        zeros = torch.zeros(shape, device=self.history.device, dtype=self.history.dtype)
        out = zeros if self.identity else self(zeros, streams)
        self.reset(streams)
        return out

    def reset(self, streams=None):
        if streams is None:
            self.history.zero_()
        else:
            self.history[torch.tensor(self._select(streams), dtype=torch.int64, device=self.history.device)] = 0


__all__ = ["resample", "Resample", "StreamResampler", "get_filter", "Filter"]
