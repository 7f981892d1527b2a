"""GPU: sample-rate conversion (sepkernels/resample.py; csrc/resample.hip: sep_resample_fwd, sep_resample_stream_fwd).

The reference calls torchaudio for this, which is on none of our machines.  The oracle is the definition of include/sepkernels.h written here in
numpy fp64 with the FULL table of K taps (the kernels take the compact one).  The bound per output is derived, not measured:
    |y - ref| <= (Kc + 3) 2^-24 sum_k |h[p][k]| |x[...]|  +  2^-60 max_k |h[p][k]| sum_window |x|
the fp32 rounding of Kc coefficients, products and sums in any order, plus the taps the compaction drops.  The composed fp32 route is held to
the same bound with K in place of Kc.

(1) offline: ten rate pairs x lengths around the filter's half width, the frame and the tile x R in {1, 3}, every row with a magnitude of its own in
    2^-6 .. 2^6, exactly-sized pitched buffers pre-filled with NaN between guard bands; shapes (T,), (C, T), (B, C, T) and a strided view through the
    module.   (2) impulses return the table's columns.   (3) every named instance is reached; a second run gives the same bits.
(4) streams: streamed + flush against the oracle of the pre-rolled signal, bit-identical to resample(pad(x, (D, 0))) and across chunk plans.
(5) calls on a subset of the slots.   (6) 16 k in -> StreamResampler -> online separator -> StreamResampler -> 16 k out against the same chain offline.
The case functions take their device through the hooks below, so tests/test_resample_cpu.py runs them on the host simulation of the kernel source."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sepkernels
from sepkernels import resample as RS

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
to_device = lambda t: t.cuda()                      # noqa: E731
device_sync = lambda: torch.cuda.synchronize()      # noqa: E731

PAIRS = [(8000, 16000), (16000, 8000), (32000, 16000), (48000, 8000), (3, 2), (2, 3), (48000, 44100), (44100, 8000), (44100, 16000)]
PAIR_IDS = ["{}-{}".format(*p) for p in PAIRS]
STREAM_PAIRS = [(16000, 8000), (8000, 16000), (48000, 44100), (44100, 8000)]
# (o, u, width, K, longest run of taps that are not negligible) as the issue lists them
KNOWN = {(8000, 16000): (1, 2, 7, 15, 13), (16000, 8000): (2, 1, 13, 28, 25), (48000, 8000): (6, 1, 37, 80, 73), (48000, 44100): (160, 147, 7, 174, 14),
         (44100, 8000): (441, 80, 34, 509, 67), (44100, 16000): (441, 160, 17, 475, 34)}
INSTANCE = {(8000, 16000): "frames<2>", (16000, 8000): "frames<1>", (32000, 16000): "frames<1>", (48000, 8000): "frames<1>", (3, 2): "frames<2>", (2, 3): "frames<3>",
            (48000, 44100): "phases", (44100, 8000): "phases", (44100, 16000): "phases"}


# ---------------------------------------------------------------------------------------------------------------- the oracle (numpy fp64)
class Oracle:
    """the definition, sinc_interp_hann: h (u, K) fp64 and, by the rule of the compact table, the longest run Kc"""

    def __init__(self, orig, new, lpw=6, rolloff=0.99):
        g = math.gcd(orig, new)
        self.o, self.u = o, u = orig // g, new // g
        base = min(o, u) * rolloff
        self.width = width = int(math.ceil(lpw * o / base))
        self.K = K = 2 * width + o
        t = ((np.arange(K)[None, :] - width) / o - np.arange(u)[:, None] / u) * base
        t = np.clip(t, -lpw, lpw)
        safe = np.where(t == 0, 1.0, t)
        self.h = np.where(t == 0, 1.0, np.sin(np.pi * safe) / (np.pi * safe)) * np.cos(np.pi * t / (2 * lpw)) ** 2 * base / o
        keep = np.abs(self.h) >= 2.0 ** -60 * np.abs(self.h).max(1, keepdims=True)
        self.lo = keep.argmax(1)
        self.hi = K - 1 - keep[:, ::-1].argmax(1)
        self.Kc = int((self.hi - self.lo + 1).max())
        self.D = -(-width // o) * o
        self.H = width + self.D

    def __call__(self, x):
        """x (R, T) fp64 -> y (R, T_out), sum_k |h| |x| behind every output, max_k |h[p]| times the sum of |x| over the output's window"""
        R, T = x.shape
        o, u, K = self.o, self.u, self.K
        T_out = -(-u * T // o)
        nf = -(-T_out // u)
        xp = np.zeros((R, (nf - 1) * o + K))
        stop = min(T, xp.shape[1] - self.width)
        xp[:, self.width:self.width + stop] = x[:, :stop]
        win = np.lib.stride_tricks.sliding_window_view(xp, K, axis=1)[:, ::o][:, :nf]           # (R, nf, K)
        y = np.einsum("rfk,pk->rfp", win, self.h).reshape(R, nf * u)[:, :T_out]
        mag = np.einsum("rfk,pk->rfp", np.abs(win), np.abs(self.h)).reshape(R, nf * u)[:, :T_out]
        drop = (np.abs(win).sum(2)[:, :, None] * np.abs(self.h).max(1)[None, None, :]).reshape(R, nf * u)[:, :T_out]
        return y, mag, drop

    def bound(self, taps, mag, drop):
        return (taps + 3) * 2.0 ** -24 * mag + 2.0 ** -60 * drop


def oracle_of(orig, new, cache={}):
    if (orig, new) not in cache:
        cache[(orig, new)] = Oracle(orig, new)
    return cache[(orig, new)]


def signal(R, T, seed):
    """(R, T) fp32 on the CPU: noise, row r scaled by 2^-6 .. 2^6"""
    x = torch.randn(R, T, generator=torch.Generator().manual_seed(seed))
    scale = torch.tensor([2.0 ** (-6 + (12 * r // max(R - 1, 1))) for r in range(R)]) if R > 1 else torch.tensor([0.75])
    return x * scale.view(R, 1)


def within(y, x, orc, taps, what):
    """y (R, T_out) of x (R, T), both CPU tensors: all finite and inside the derived bound"""
    ref, mag, drop = orc(x.double().numpy())
    got = y.double().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what + ": an output was not written"
    excess = np.abs(got - ref) - orc.bound(taps, mag, drop)
    assert excess.max() <= 0, "{}: |y - ref| exceeds the bound by {:.3e} at {}".format(what, excess.max(), np.unravel_index(excess.argmax(), excess.shape))


def lengths_of(orc):
    """the issue's lengths, plus one that needs a second tile of the kernel plus one sample"""
    flt_tile = min((8192 - orc.K) // orc.o + 1, 2048 if orc.u <= 3 else max(1, 2048 // orc.u))
    if orc.o == 441:
        return [1, 440, 441, 1000, 4411, flt_tile * orc.o + 1]
    w, o = orc.width, orc.o
    return sorted({T for T in (1, w - 1, w, w + 1, 3 * o - 1, 3 * o, 3 * o + 1, flt_tile * o + 1) if T >= 1})


# ---------------------------------------------------------------------------------------------------------------- (1) offline
def case_offline(orig, new, R, T, seed=0):
    """sep_resample_fwd on pitched buffers of exact size between guard bands"""
    orc, flt = oracle_of(orig, new), RS.get_filter(orig, new)
    assert (flt.o, flt.u, flt.width, flt.K, flt.Kc) == (orc.o, orc.u, orc.width, orc.K, orc.Kc)
    T_out = -(-orc.u * T // orc.o)
    G, xp, yp = 64, T + 3, T_out + 5
    x = signal(R, T, seed + T)
    xbuf = torch.full((R, xp), float("nan"))
    xbuf[:, :T] = x
    xd = to_device(xbuf)
    ybuf = to_device(torch.full((2 * G + R * yp,), float("nan")))
    table, first = (to_device(t) for t in (flt.table, flt.first))
    HIP.resample_fwd(xd, xp, table, first, ybuf[G:G + R * yp], yp, R, T, T_out, orc.o, orc.u, orc.width, orc.Kc)
    device_sync()
    assert sepkernels.last_kernel() == "resample_" + INSTANCE[(orig, new)]
    out = ybuf.cpu()
    assert torch.isnan(out[:G]).all() and torch.isnan(out[G + R * yp:]).all(), "a guard band was written"
    rows = out[G:G + R * yp].view(R, yp)
    assert torch.isnan(rows[:, T_out:]).all(), "elements between T_out and the pitch were written"
    assert torch.equal(xd.cpu()[:, :T], x) and torch.isnan(xd.cpu()[:, T:]).all(), "the input was changed"
    within(rows[:, :T_out], x, orc, orc.Kc, "{} -> {} R {} T {}".format(orig, new, R, T))
    again = to_device(torch.full((2 * G + R * yp,), float("nan")))
    HIP.resample_fwd(xd, xp, table, first, again[G:G + R * yp], yp, R, T, T_out, orc.o, orc.u, orc.width, orc.Kc)
    device_sync()
    assert torch.equal(again.cpu()[G:G + R * yp].view(R, yp)[:, :T_out], rows[:, :T_out]), "a second run gave other bits"


@pytest.mark.parametrize("orig,new", PAIRS, ids=PAIR_IDS)
def test_offline_kernel_against_the_oracle(orig, new):
    orc = oracle_of(orig, new)
    if (orig, new) in KNOWN:
        assert (orc.o, orc.u, orc.width, orc.K, orc.Kc) == KNOWN[(orig, new)]
    for T in lengths_of(orc):
        for R in (1, 3):
            case_offline(orig, new, R, T)


def case_shapes(orig, new):
    """the module: any leading dimensions; a strided view and fp64 take the composed route, held to the bound with K taps"""
    orc = oracle_of(orig, new)
    T = 3 * orc.o + orc.width + 1
    for shape in ((T,), (3, T), (2, 3, T)):
        x = signal(int(np.prod(shape[:-1])), T, 5).view(shape)
        y = RS.resample(to_device(x), orig, new)
        device_sync()
        assert y.dtype == torch.float32 and tuple(y.shape) == shape[:-1] + (-(-orc.u * T // orc.o),)
        within(y.cpu().reshape(-1, y.shape[-1]), x.reshape(-1, T), orc, orc.Kc, "{} -> {} shape {}".format(orig, new, shape))
        assert torch.equal(RS.Resample(orig, new)(to_device(x)), y)
    same = to_device(signal(2, 37, 7))
    assert RS.resample(same, 8000, 8000) is same


def case_strided_view(orig, new):
    """a view with a pitch is not the kernels': the composed route on the device's own convolution, held to the bound with K taps"""
    orc = oracle_of(orig, new)
    T = 3 * orc.o + orc.width + 1
    wide = to_device(signal(3, T + 7, 6))
    view = wide[:, 2:2 + T]
    assert not view.is_contiguous()
    y = RS.resample(view, orig, new)
    within(y.cpu(), view.cpu(), orc, orc.K, "{} -> {} strided view".format(orig, new))


@pytest.mark.parametrize("orig,new", [(16000, 8000), (2, 3), (44100, 16000)], ids=["16000-8000", "2-3", "44100-16000"])
def test_module_takes_any_leading_dimensions(orig, new):
    case_shapes(orig, new)


def test_a_strided_view_takes_the_composed_route():
    case_strided_view(16000, 8000)


# ---------------------------------------------------------------------------------------------------------------- (2) impulses
def case_impulse(orig, new):
    """x = delta(t - t0) returns the columns of the table: a tap or a first[p] off by one shows here at full scale"""
    orc = oracle_of(orig, new)
    T = 3 * orc.o + 2 * orc.width + 2
    T_out = -(-orc.u * T // orc.o)
    for t0 in (0, orc.width, T - 1):
        x = torch.zeros(1, T)
        x[0, t0] = 1.0
        y = RS.resample(to_device(x), orig, new).cpu()
        device_sync()
        t = np.arange(T_out)
        k = t0 - (t // orc.u) * orc.o + orc.width
        want = np.where((k >= 0) & (k < orc.K), orc.h[t % orc.u, np.clip(k, 0, orc.K - 1)], 0.0)
        err = np.abs(y[0].double().numpy() - want)
        assert (err <= 2.0 ** -24 * np.abs(want) + 2.0 ** -60 * np.abs(orc.h).max(1)[t % orc.u]).all(), (orig, new, t0, err.max())
        assert np.abs(want).max() > 0.01 * orc.h.max()


@pytest.mark.parametrize("orig,new", PAIRS, ids=PAIR_IDS)
def test_impulses_return_the_columns_of_the_table(orig, new):
    case_impulse(orig, new)


# ---------------------------------------------------------------------------------------------------------------- (3) instances
def case_instances():
    seen = set()
    for (orig, new), name in INSTANCE.items():
        orc = oracle_of(orig, new)
        x = to_device(signal(2, 2 * orc.o + 3, 9))
        a = RS.resample(x, orig, new)
        assert sepkernels.last_kernel() == "resample_" + name
        b = RS.resample(x, orig, new)
        device_sync()
        assert torch.equal(a, b)
        rs = RS.StreamResampler(2, orig, new, device=x.device)
        rs(x[:, :2 * orc.o].contiguous())
        assert sepkernels.last_kernel() == "resample_stream_" + name
        seen.add(name)
    assert seen == {"frames<1>", "frames<2>", "frames<3>", "phases"}


def test_every_named_instance_is_reached():
    case_instances()


# ---------------------------------------------------------------------------------------------------------------- (4) streams
def stream_through(rs, x, plan, streams=None):
    """x (A, n o) through rs in chunks of plan[i] o samples, then flush"""
    outs, pos = [], 0
    for m in plan:
        outs.append(rs(x[..., pos:pos + m * rs.o].contiguous(), streams))
        pos += m * rs.o
    assert pos == x.shape[-1]
    outs.append(rs.flush(streams))
    return torch.cat(outs, -1)


def case_stream(orig, new, num_streams, plan):
    orc = oracle_of(orig, new)
    n = sum(plan)
    x = signal(num_streams, n * orc.o, 11 + n)
    xd = to_device(x)
    rs = RS.StreamResampler(num_streams, orig, new, device=xd.device)
    assert rs.delay == orc.D and rs.state_bytes == 4 * num_streams * orc.H and (rs.D, rs.H) == (orc.D, orc.H)
    got = stream_through(rs, xd, plan)
    device_sync()
    assert tuple(got.shape) == (num_streams, (n + orc.D // orc.o) * orc.u)
    assert not rs.history.any(), "flush() left a history behind"
    padded = F.pad(x, (orc.D, 0))
    within(got.cpu(), padded, orc, orc.Kc, "{} -> {} streamed in {}".format(orig, new, plan))
    whole = RS.resample(to_device(padded), orig, new)
    assert torch.equal(got, whole), "{} -> {} streamed in {}: not resample(pad(x, (D, 0))) bit for bit".format(orig, new, plan)
    other = list(reversed(plan)) if len(plan) > 1 else [1] * n
    assert torch.equal(stream_through(rs, xd, other), got), "two chunk plans gave other bits"
    if len(plan) > 1:
        assert torch.equal(stream_through(rs, xd, [n]), got), "one chunk gave other bits"


def plans_of(orig, new):
    return [[1], [1, 3, 7, 29]] + ([[1, 2, 1]] if (orig, new) == (44100, 8000) else [])


@pytest.mark.parametrize("num_streams", [1, 3])
@pytest.mark.parametrize("orig,new", STREAM_PAIRS, ids=["{}-{}".format(*p) for p in STREAM_PAIRS])
def test_streams_against_the_oracle_and_the_offline_call(orig, new, num_streams):
    for plan in plans_of(orig, new):
        case_stream(orig, new, num_streams, plan)


def case_stream_of_many_tiles():
    """a chunk longer than a tile of the kernel: only the workgroup of the first tile touches the history"""
    case_stream(8000, 16000, 2, [2100, 1])
    case_stream(48000, 44100, 1, [30, 2])


def test_a_chunk_of_several_tiles():
    case_stream_of_many_tiles()


# ---------------------------------------------------------------------------------------------------------------- (5) subset calls
def case_subsets(orig, new):
    orc = oracle_of(orig, new)
    Bs, o = 5, orc.o
    dev = to_device(torch.zeros(1)).device
    rs = RS.StreamResampler(Bs, orig, new, device=dev)
    mask = torch.tensor([True, False, True, True, False])
    calls = [([3, 1], 3), ([4], 1), (mask, 2), ([3, 1], 1), ([4], 5), (mask, 1)]
    fed = {s: [] for s in range(Bs)}
    out = {s: [] for s in range(Bs)}
    g = torch.Generator().manual_seed(21)
    for sel, m in calls:
        idx = torch.nonzero(mask).view(-1).tolist() if torch.is_tensor(sel) else sel
        chunk = torch.randn(len(idx), m * o, generator=g) * torch.tensor([2.0 ** (s - 2) for s in idx]).view(-1, 1)
        before = rs.history.clone()
        y = rs(to_device(chunk), streams=to_device(sel) if torch.is_tensor(sel) else sel)
        device_sync()
        assert tuple(y.shape) == (len(idx), m * orc.u)
        rest = [s for s in range(Bs) if s not in idx]
        assert torch.equal(rs.history[rest], before[rest]), "the history of a slot that was not named changed"
        for j, s in enumerate(idx):
            fed[s].append(chunk[j])
            out[s].append(y[j])
    for s in range(Bs):
        before = rs.history.clone()
        tail = rs.flush([s])
        rest = [q for q in range(Bs) if q != s]
        assert torch.equal(rs.history[rest], before[rest]) and not rs.history[s].any()
        got = torch.cat(out[s] + [tail[0]])
        want = RS.resample(to_device(F.pad(torch.cat(fed[s]), (orc.D, 0))), orig, new)
        assert torch.equal(got, want), "slot {}: its pieces and its flush are not its own offline result".format(s)
    rs(to_device(torch.randn(Bs, 4 * o, generator=g)))
    before = rs.history.clone()
    rs.reset([1])
    assert not rs.history[1].any() and torch.equal(rs.history[[0, 2, 3, 4]], before[[0, 2, 3, 4]]) and before[1].any()
    chunk = to_device(torch.zeros(2, 2 * o))
    for bad, words in (([1, 1], "duplicate"), ([0, 5], "out of range"), ([-1, 0], "out of range"), ([], "empty"), (torch.zeros(5, dtype=torch.bool), "empty"),
                       (torch.ones(4, dtype=torch.bool), "mask has 4 entries"), ([0, 1, 2], "chunk must be")):
        with pytest.raises(ValueError, match=words):
            rs(chunk, streams=bad)
    with pytest.raises(ValueError, match="chunk must be"):
        rs(chunk)
    if o > 1:
        with pytest.raises(ValueError, match="multiple of {}".format(o)):
            rs(to_device(torch.zeros(2, 2 * o + 1)), streams=[0, 1])
    with pytest.raises(ValueError, match="duplicate"):
        rs.flush([2, 2])
    with pytest.raises(ValueError, match="out of range"):
        rs.reset([7])


@pytest.mark.parametrize("orig,new", [(16000, 8000), (48000, 44100)], ids=["16000-8000", "48000-44100"])
def test_calls_on_a_subset_of_the_slots(orig, new):
    case_subsets(orig, new)


# ---------------------------------------------------------------------------------------------------------------- (6) with the online separator
def test_resamplers_around_the_online_separator():
    """2 streams of 16 kHz audio -> StreamResampler(16000, 8000) -> the causal16 fixture model's online separator -> StreamResampler(8000, 16000) over
    the n_src rows of every stream, a dozen calls of 2 k S samples without a flush: the first samples of the same chain run offline on the device,
    resample(pad(model(pad(resample(pad(x, D1)), L - S)), D3)), within 1e-3 of its maximum (what the online tests ask of device against offline)"""
    from test_online_gpu import _fixture_model
    model, cfg = _fixture_model("causal16")
    model.eval()
    L, S, n_src, Bs, k, calls = cfg["kernel_size"], cfg["stride"], cfg["n_sources"], 2, 5, 12
    x = 0.1 * torch.randn(Bs, calls * 2 * k * S, generator=torch.Generator().manual_seed(4)).cuda()
    down = RS.StreamResampler(Bs, 16000, 8000, device=x.device)
    sep = model.online_separator(num_streams=Bs, chunk_size=k * S)
    up = RS.StreamResampler(Bs, 8000, 16000, device=x.device, channels=n_src)
    outs = []
    for c in range(calls):
        low = down(x[:, c * 2 * k * S:(c + 1) * 2 * k * S].contiguous())
        est = sep(low.view(Bs, 1, k * S))
        outs.append(up(est.contiguous()))
    got = torch.cat(outs, -1)
    assert tuple(got.shape) == (Bs, n_src, x.shape[-1])
    with torch.no_grad():
        low = RS.resample(F.pad(x, (down.D, 0)), 16000, 8000)[..., :calls * k * S]       # what the stream has handed on: whole hops for the model
        est = model(F.pad(low.unsqueeze(1), (L - S, 0)))
        want = RS.resample(F.pad(est, (up.D, 0)).contiguous(), 8000, 16000)[..., :got.shape[-1]]
    err = (got - want).abs().max().item()
    assert err <= 1e-3 * want.abs().max().item(), (err, want.abs().max().item())
