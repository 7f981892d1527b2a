"""GPU: dynamic mixing from a device-resident corpus (sepkernels/mixing.py: DeviceCorpus, DynamicMixer; csrc/mixing.hip: sep_mix_draw, sep_mix_render).

The oracle of the draw is the rule of include/sepkernels.h restated here in Python integers (mix64, word, below, draw_item): plans and gains are
compared with torch.equal.  The oracle of the render is the formula restated in torch (render_ref) applied to the DEVICE's plan, bit for bit.
    mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
    word(seed, item, k) = mix64(mix64(seed + 0x9E3779B97F4A7C15 * (item + 1)) + k),  below(w, m) = ((w >> 32) * m) >> 32,  all in wrapping uint64
    item = step * item_stride + item_first + b
Fixture corpus: 3 speakers, 7 utterances of 1, 5, 8, 31, 64, 100, 257 samples (spk_first 0, 2, 3, 7) in both sample kinds, the fp32 copy with a
magnitude per utterance in 2^-6 .. 2^6.  Output and plan buffers are sized exactly, pre-filled with NaN (plans: a sentinel) and held between guard
bands; the inputs and the bands are checked after every call.

(1) draw: (B, n) x T x steps 0 .. 15 x rank 0 of 1 and 1 of 2, with and without a noise index; the known answers.   (2) render: both kinds, T 16 and 64
(vector instance), 30 (scalar), an output view offset by one float (scalar), start 0 .. 7 on the last utterance; instances by name; finite; a second run.
(3) the counter: steps k and k + 1, seek; a recorded Sequence of one draw and one render replayed three times.   (4) partition invariance.
(5) the loader's wavs: every source row is the read_wav crop its plan names.   (6) three training steps fed by the kernels and by the composed route.
The case functions take their device through the hooks below, so tests/test_dynamic_mixing_cpu.py runs them on the host simulation of the kernel source."""
import os

import pytest
import torch

import sepkernels
from sepkernels import mixing as MX

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
to_device = lambda t: t.cuda()                      # noqa: E731
device_sync = lambda: torch.cuda.synchronize()      # noqa: E731
corpus_device = lambda: "cuda"                      # noqa: E731

LENGTHS, SPK_FIRST, SPEAKERS = [1, 5, 8, 31, 64, 100, 257], [0, 2, 3, 7], [0, 0, 1, 2, 2, 2, 2]
NOISE_LENGTHS = [3, 40, 129]
KINDS = ["int16", "float32"]
BAND = 64                                           # guard band in elements (a multiple of four floats: the view between the bands stays 16-byte aligned)
MASK = (1 << 64) - 1
SENTINEL = -(1 << 62) - 12345


# ---------------------------------------------------------------------------------------------------------------- the rule in Python integers
def mix64(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def word(seed, item, k):
    return mix64((mix64((seed + 0x9E3779B97F4A7C15 * (item + 1)) & MASK) + k) & MASK)


def below(w, m):
    assert 1 <= m < 1 << 31
    return ((w >> 32) * m) >> 32


def place(length, T, w):
    """-> (start, lead)"""
    return (below(w, length - T + 1), 0) if length >= T else (0, below(w, T - length + 1))


def draw_item(seed, item, n, T, G, spk_first=SPK_FIRST, lengths=LENGTHS, noise_lengths=None, G_noise=None):
    """-> rows (speaker, utterance, start, lead, gain index); the noise row (speaker -1) last"""
    S, rows, chosen = len(spk_first) - 1, [], []
    for i in range(n):
        r = below(word(seed, item, i), S - i)
        for c in chosen:                         # ascending
            if r >= c:
                r += 1
        chosen = sorted(chosen + [r])
        u = spk_first[r] + below(word(seed, item, n + i), spk_first[r + 1] - spk_first[r])
        start, lead = place(lengths[u], T, word(seed, item, 2 * n + i))
        rows.append((r, u, start, lead, below(word(seed, item, 3 * n + i), G)))
    if noise_lengths is not None:
        u = below(word(seed, item, 4 * n), len(noise_lengths))
        start, lead = place(noise_lengths[u], T, word(seed, item, 4 * n + 1))
        rows.append((-1, u, start, lead, below(word(seed, item, 4 * n + 2), G_noise)))
    return rows


def table_ref(lo, hi, G):
    return torch.tensor([10.0 ** ((lo + (hi - lo) * j / (G - 1) if G > 1 else lo) / 20.0) for j in range(G)], dtype=torch.float64).float()


def plan_ref(corpus, noise, table, noise_table, seed, step, stride, first, B, n, T):
    """-> plan (B, R, 4) int64, gain (B, R) float32 by the rule, on the CPU"""
    plan, gain = [], []
    for b in range(B):
        rows = draw_item(seed, (step * stride + first + b) & MASK, n, T, table.numel(), corpus.spk_first_host.tolist(), corpus.lengths().tolist(),
                         None if noise is None else noise.lengths().tolist(), None if noise is None else noise_table.numel())
        plan.append([list(r[1:]) for r in rows])
        gain.append(torch.stack([(corpus.level.cpu()[r[1]] * table[r[4]]) if r[0] >= 0 else (noise.level.cpu()[r[1]] * noise_table[r[4]]) for r in rows]))
    return torch.tensor(plan, dtype=torch.int64), torch.stack(gain)


def render_ref(corpus, noise, plan, gain, n, T):
    """the formula of sep_mix_render with its clamps and its predicate, in torch on the CPU -> sources (B, n, T), mixture (B, 1, T), noise (B, 1, T) or None"""
    def row(c, p, g):
        samples, off = c.samples.cpu(), c.offsets_host
        u = min(max(int(p[0]), 0), c.num_utterances - 1)
        length = int(off[u + 1] - off[u])
        start = max(min(int(p[1]), length - 1), 0)
        lead, out = int(p[2]), torch.zeros(T, dtype=torch.float32)
        lo, hi = max(lead, 0), min(T, lead + length - start)                      # lead <= t and t - lead < len - start
        if hi > lo:
            seg = samples[int(off[u]) + start + lo - lead:int(off[u]) + start + hi - lead]
            out[lo:hi] = g * (seg.to(torch.float32) * (2.0 ** -15 if samples.dtype == torch.int16 else 1.0))
        return out
    B, R = plan.shape[0], plan.shape[1]
    assert R == n + (noise is not None)
    plan, gain = plan.cpu(), gain.cpu()
    src = torch.stack([torch.stack([row(corpus, plan[b, i], gain[b, i]) for i in range(n)]) for b in range(B)])
    mix = src[:, 0]
    for i in range(1, n):
        mix = mix + src[:, i]
    if noise is None:
        return src, mix.unsqueeze(1), None
    nz = torch.stack([row(noise, plan[b, n], gain[b, n]) for b in range(B)]).unsqueeze(1)
    return src, mix.unsqueeze(1) + nz, nz


# ---------------------------------------------------------------------------------------------------------------- the fixture corpus
def make_corpus(kind, lengths=LENGTHS, speakers=SPEAKERS, seed=0, cache={}):
    """the fixture corpus on the CPU (computed once per kind and left unchanged)"""
    key = (kind, tuple(lengths), seed)
    if key not in cache:
        g = torch.Generator().manual_seed(seed + len(lengths))
        if kind == "int16":
            waves = [torch.randint(-32768, 32768, (length,), generator=g).float() / 32768.0 for length in lengths]
        else:
            waves = [torch.randn(length, generator=g) * 2.0 ** (2 * u - 6) for u, length in enumerate(lengths)]
        cache[key] = MX.DeviceCorpus.from_waveforms(waves, speakers, dtype=kind)
        assert cache[key].dtype == getattr(torch, kind)
    return cache[key]


def make_noise(kind):
    return make_corpus(kind, NOISE_LENGTHS, None, seed=5)


class OnDevice:
    """the tensors of a corpus as the entry points take them, on the device of the hooks, with the copies that must come back unchanged"""

    def __init__(self, corpus):
        self.corpus = corpus
        self.host = [corpus.samples.cpu().clone(), corpus.offsets.cpu().clone(), corpus.spk_first.cpu().clone(), corpus.level.cpu().clone()]
        self.samples, self.offsets, self.spk_first, self.level = (to_device(t) for t in self.host)
        self.U, self.S = corpus.num_utterances, corpus.num_speakers

    def unchanged(self):
        return all(torch.equal(a.cpu(), b) for a, b in zip((self.samples, self.offsets, self.spk_first, self.level), self.host))


def banded(numel, dtype, shift=0):
    """-> (whole buffer on the device, the view of `numel` elements between two bands, `shift` elements further in)"""
    fill = float("nan") if dtype.is_floating_point else SENTINEL
    buf = to_device(torch.full((2 * BAND + numel + shift,), fill, dtype=dtype))
    return buf, buf[BAND + shift:BAND + shift + numel]


def bands_intact(buf, numel, shift=0):
    host = buf.cpu()
    edge = torch.cat([host[:BAND + shift], host[BAND + shift + numel:]])
    return bool(torch.isnan(edge).all()) if host.dtype.is_floating_point else bool((edge == SENTINEL).all())


def device_draw(dev, noise_dev, table, noise_table, counter, seed, stride, first, B, n, T):
    """one sep_mix_draw into fresh banded buffers -> plan (B, R, 4), gain (B, R) on the CPU"""
    R = n + (noise_dev is not None)
    pbuf, plan = banded(B * R * 4, torch.int64)
    gbuf, gain = banded(B * R, torch.float32)
    HIP.mix_draw(dev.offsets, dev.spk_first, dev.U, dev.S, None if noise_dev is None else noise_dev.offsets, 0 if noise_dev is None else noise_dev.U, dev.level, table,
                 table.numel(), None if noise_dev is None else noise_dev.level, noise_table, 0 if noise_dev is None else noise_table.numel(), counter, seed, stride, first,
                 B, n, T, plan, gain)
    device_sync()
    assert bands_intact(pbuf, B * R * 4) and bands_intact(gbuf, B * R), "a guard band of the plan was written"
    assert dev.unchanged() and (noise_dev is None or noise_dev.unchanged()), "the draw changed the corpus"
    return plan.cpu().view(B, R, 4).clone(), gain.cpu().view(B, R).clone()


# ---------------------------------------------------------------------------------------------------------------- (1) the draw
DRAW_BN = [(1, 1), (5, 2), (3, 3)]
DRAW_T = [16, 64, 300]          # 300 is longer than every utterance: every row has a lead


def case_draw(B, n, T, with_noise, seed=1234):
    corpus, noise = make_corpus("int16"), make_noise("int16") if with_noise else None
    dev, ndev = OnDevice(corpus), OnDevice(noise) if with_noise else None
    table_h, ntable_h = MX.gain_table(-2.5, 2.5, 256), MX.gain_table(-6.0, 3.0, 256)
    assert torch.equal(table_h, table_ref(-2.5, 2.5, 256)) and torch.equal(ntable_h, table_ref(-6.0, 3.0, 256))
    table, ntable = to_device(table_h), to_device(ntable_h) if with_noise else None
    for rank, world in ((0, 1), (1, 2)):
        counter = to_device(torch.zeros(1, dtype=torch.int64))
        for step in range(16):
            plan, gain = device_draw(dev, ndev, table, ntable, counter, seed, B * world, rank * B, B, n, T)
            want_plan, want_gain = plan_ref(corpus, noise, table_h, ntable_h, seed, step, B * world, rank * B, B, n, T)
            assert torch.equal(plan, want_plan), (B, n, T, rank, step, plan.tolist(), want_plan.tolist())
            assert torch.equal(gain, want_gain), (B, n, T, rank, step)
            assert int(counter.cpu()) == step + 1, "the kernel leaves counter + 1"
            if T == 300:
                assert bool((plan[:, :, 1] == 0).all()) and bool((plan[:, :n, 2] <= 300 - corpus.lengths()[plan[:, :n, 0]]).all())


@pytest.mark.parametrize("with_noise", [False, True], ids=["speech", "noise"])
@pytest.mark.parametrize("T", DRAW_T)
@pytest.mark.parametrize("B,n", DRAW_BN)
def test_draw_is_the_rule(B, n, T, with_noise):
    case_draw(B, n, T, with_noise)


KNOWN_WORDS = [((1234, 0, 0), 0x2851ddd6c202938b), ((1234, 0, 1), 0xf344a9a461c929aa), ((1234, 1, 0), 0xc4c7e6b923620b24), ((1234, 1, 1), 0x22531db8ef59e66f),
               ((0, 0, 0), 0x48218226ff3cd4bf), ((1 << 63, (1 << 40) + 3, 31), 0x568966ec49cd65d1)]
KNOWN_ITEM_0 = [(0, 0, 0, 53, 11), (2, 6, 66, 0, 177)]                          # n = 2, T = 64, G = 256, seed 1234
KNOWN_ITEM_7 = [(2, 4, 0, 0, 28), (0, 0, 0, 49, 49), (1, 2, 0, 25, 35)]         # n = 3


def case_known_answers():
    for args, want in KNOWN_WORDS:
        assert word(*args) == want, (args, hex(word(*args)))
    assert draw_item(1234, 0, 2, 64, 256) == KNOWN_ITEM_0 and draw_item(1234, 7, 3, 64, 256) == KNOWN_ITEM_7
    corpus = make_corpus("int16")
    dev, table = OnDevice(corpus), to_device(MX.gain_table(-2.5, 2.5, 256))
    zero = lambda: to_device(torch.zeros(1, dtype=torch.int64))          # noqa: E731
    plan, _ = device_draw(dev, None, table, None, zero(), 1234, 1, 0, 1, 2, 64)
    assert plan[0].tolist() == [list(r[1:]) for r in KNOWN_ITEM_0]
    plan, _ = device_draw(dev, None, table, None, zero(), 1234, 1, 7, 1, 3, 64)
    assert plan[0].tolist() == [list(r[1:]) for r in KNOWN_ITEM_7]
    # seed 2^63 and an item beyond 2^40 through the ABI: the seed is read as unsigned, the item arithmetic wraps in 64 bits
    plan, _ = device_draw(dev, None, table, None, to_device(torch.tensor([1 << 40], dtype=torch.int64)), 1 << 63, 1, 3, 1, 2, 64)
    assert plan[0].tolist() == [list(r[1:]) for r in draw_item(1 << 63, (1 << 40) + 3, 2, 64, 256)]
    # items 0 .. 319 at n = 2 in ONE call (more items than the workgroup has threads)
    plan, _ = device_draw(dev, None, table, None, zero(), 1234, 320, 0, 320, 2, 64)
    assert plan.tolist() == [[list(r[1:]) for r in draw_item(1234, item, 2, 64, 256)] for item in range(320)]
    speakers = [[corpus.speaker_of(int(u)) for u in item] for item in plan[:, :, 0]]
    assert all(a != b for a, b in speakers), "an item repeats a speaker"
    counts = torch.bincount(plan[:, :, 0].reshape(-1), minlength=7)
    assert int(counts.min()) >= 46 and int(counts.max()) <= 204 and int(counts.sum()) == 640, counts.tolist()
    starts = plan[:, :, 1][plan[:, :, 0] == 6]
    assert int(starts.min()) == 5 and int(starts.max()) == 193 == 257 - 64, (int(starts.min()), int(starts.max()))


def test_known_answers():
    case_known_answers()


# ---------------------------------------------------------------------------------------------------------------- (2) the render
INSTANCE = {("int16", True): "mix_render_vec<int16,8>", ("int16", False): "mix_render_scalar<int16>",
            ("float32", True): "mix_render_vec<float,4>", ("float32", False): "mix_render_scalar<float>"}


def device_render(dev, ndev, plan, gain, B, n, T, shift, kind, finite=True):
    """one sep_mix_render of a CPU plan into banded, exactly-sized outputs; checked for bands, inputs, the instance, finiteness (unless the caller's gains
    are not finite themselves) and a second run -> sources (B, n, T), mixture (B, 1, T), noise (B, 1, T) or None on the CPU"""
    plan_d, gain_d = to_device(plan.contiguous()), to_device(gain.contiguous())
    runs = []
    for _ in range(2):
        sbuf, src = banded(B * n * T, torch.float32, shift)
        mbuf, mix = banded(B * T, torch.float32, shift)
        zbuf, nz = banded(B * T, torch.float32, shift) if ndev is not None else (None, None)
        HIP.mix_render(dev.samples, dev.offsets, dev.U, None if ndev is None else ndev.samples, None if ndev is None else ndev.offsets, 0 if ndev is None else ndev.U,
                       plan_d, gain_d, B, n, T, src, mix, nz)
        device_sync()
        vector = T % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in (src, mix, nz))
        assert vector == (T % 4 == 0 and shift % 4 == 0), "the test's buffers are not aligned as it believes"
        assert sepkernels.last_kernel() == INSTANCE[(kind, vector)], (sepkernels.last_kernel(), kind, T, shift)
        assert bands_intact(sbuf, B * n * T, shift) and bands_intact(mbuf, B * T, shift) and (zbuf is None or bands_intact(zbuf, B * T, shift)), "a guard band was written"
        assert dev.unchanged() and (ndev is None or ndev.unchanged()) and torch.equal(plan_d.cpu(), plan) and \
            torch.equal(gain_d.cpu().view(torch.int32), gain.contiguous().view(torch.int32)), "an input was changed"
        out = (src.cpu().view(B, n, T).clone(), mix.cpu().view(B, 1, T).clone(), None if nz is None else nz.cpu().view(B, 1, T).clone())
        assert not finite or all(o is None or bool(torch.isfinite(o).all()) for o in out), "an output element was left unwritten"
        runs.append(out)
    assert all(a is None or torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs)), "a second run gave other bits"
    return runs[0]


def assert_same_bits(got, want, what):
    for name, a, b in zip(("sources", "mixture", "noise"), got, want):
        assert (a is None) == (b is None)
        if a is not None:
            assert torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32)), "{}: {} differ from the formula at {}".format(
                what, name, torch.nonzero(a.view(torch.int32) != b.contiguous().view(torch.int32))[:4].tolist())


def case_render(kind, T, shift, with_noise):
    """the DEVICE's plan of step 3 (B = 5; n = 2, or n = 3 plus a noise row) rendered and compared with the formula on that plan"""
    corpus, noise = make_corpus(kind), make_noise(kind) if with_noise else None
    dev, ndev = OnDevice(corpus), OnDevice(noise) if with_noise else None
    B, n = 5, 3 if with_noise else 2
    table, ntable = to_device(MX.gain_table(-2.5, 2.5, 256)), to_device(MX.gain_table(-6.0, 3.0, 7)) if with_noise else None
    plan, gain = device_draw(dev, ndev, table, ntable, to_device(torch.tensor([3], dtype=torch.int64)), 99, B, 0, B, n, T)
    got = device_render(dev, ndev, plan, gain, B, n, T, shift, kind)
    assert_same_bits(got, render_ref(corpus, noise, plan, gain, n, T), "{} T {} shift {}".format(kind, T, shift))
    assert bool(got[0].abs().sum(-1).gt(0).all()), "a source row is silent"


@pytest.mark.parametrize("with_noise", [False, True], ids=["speech", "noise"])
@pytest.mark.parametrize("T,shift", [(16, 0), (64, 0), (30, 0), (64, 1)], ids=["T16", "T64", "T30-scalar", "T64-offset-scalar"])
@pytest.mark.parametrize("kind", KINDS)
def test_render_is_the_formula_on_the_device_plan(kind, T, shift, with_noise):
    case_render(kind, T, shift, with_noise)


def case_render_every_misalignment(kind):
    """a hand-written plan: start = 0 .. 7 from the end of the last utterance (the last read ends on the last sample of the storage's utterances), a short
    tail behind a lead, and start = 0 .. 7 from its first sample; vector and scalar instance"""
    corpus = make_corpus(kind)
    dev = OnDevice(corpus)
    rows, gains = [], []
    for s in range(8):
        rows.append([[6, 257 - 64 - s, 0, 0], [6, 257 - 16 + s - 7, 9 - s, 0]])
        gains.append([1.0, -0.5])
    plan, gain = torch.tensor(rows, dtype=torch.int64), torch.tensor(gains)
    assert int(corpus.offsets_host[7]) == corpus.samples.numel() - MX.GUARD and int((plan[:, 0, 1] + 64).max()) == 257
    for T in (64, 62):
        got = device_render(dev, None, plan, gain, 8, 2, T, 0, kind)
        assert_same_bits(got, render_ref(corpus, None, plan, gain, 2, T), "{} end of the storage, T {}".format(kind, T))
    assert torch.equal(device_render(dev, None, plan, gain, 8, 2, 64, 0, kind)[0][0, 0], corpus.utterance(6).cpu()[193:].float() * (2.0 ** -15 if kind == "int16" else 1.0))
    plan[:, 0, 1] = torch.arange(8)
    got = device_render(dev, None, plan, gain, 8, 2, 64, 0, kind)
    assert_same_bits(got, render_ref(corpus, None, plan, gain, 2, 64), "{} start 0 .. 7".format(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_render_every_misalignment_up_to_the_last_sample(kind):
    case_render_every_misalignment(kind)


# ---------------------------------------------------------------------------------------------------------------- (3) the counter
def device_corpus(kind, which=make_corpus):
    return which(kind).to(corpus_device())


def case_counter(kind):
    corpus = device_corpus(kind)
    mixer = MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=4, seed=7)
    host = MX.DynamicMixer(make_corpus(kind), n_sources=2, samples=64, batch_size=4, seed=7)          # the composed route
    assert mixer.step == 0
    first, second = mixer(), mixer()
    plan1 = mixer.plan[0].cpu().clone()
    assert mixer.step == 2 and int(mixer._counter.cpu()) == 2
    table = MX.gain_table(-2.5, 2.5, 256)
    for k, got in enumerate((first, second)):
        want_plan, want_gain = plan_ref(make_corpus(kind), None, table, None, 7, k, 4, 0, 4, 2, 64)
        src, mix, _ = render_ref(make_corpus(kind), None, want_plan, want_gain, 2, 64)
        assert torch.equal(got[0].cpu(), mix) and torch.equal(got[1].cpu(), src), "step {}".format(k)
        h = host()
        assert torch.equal(h[0], mix) and torch.equal(h[1], src) and torch.equal(host.plan[0], want_plan) and torch.equal(host.plan[1], want_gain)
    assert torch.equal(plan1, plan_ref(make_corpus(kind), None, table, None, 7, 1, 4, 0, 4, 2, 64)[0])
    assert not torch.equal(first[0], second[0])
    mixer.seek(0)
    again = mixer()
    assert mixer.step == 1 and torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), "seek(0) rewinds the stream"
    state = mixer.state_dict()
    assert state == {"seed": 7, "step": 1}
    resumed = MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=4, seed=0)
    resumed.load_state_dict(state)
    out = resumed()
    assert torch.equal(out[0], second[0]) and torch.equal(out[1], second[1]), "a resumed mixer continues the stream"
    assert torch.equal(mixer.render(*resumed.plan)[1], second[1]), "render(plan, gain) of a logged plan"


@pytest.mark.parametrize("kind", KINDS)
def test_counter_steps_seek_and_state(kind):
    case_counter(kind)


def case_sequence(kind):
    """ONE recorded draw + render replayed three times equals three eager calls bit for bit: the step is device memory, a replay draws the NEXT batch"""
    corpus, noise = make_corpus(kind), make_noise(kind)
    dev, ndev = OnDevice(corpus), OnDevice(noise)
    B, n, T, R = 3, 2, 64, 3
    table, ntable = to_device(MX.gain_table(-2.5, 2.5, 256)), to_device(MX.gain_table(-6.0, 3.0, 256))

    def call(counter, plan, gain, src, mix, nz):
        HIP.mix_draw(dev.offsets, dev.spk_first, dev.U, dev.S, ndev.offsets, ndev.U, dev.level, table, 256, ndev.level, ntable, 256, counter, 1 << 63, B, 0, B, n, T, plan, gain)
        HIP.mix_render(dev.samples, dev.offsets, dev.U, ndev.samples, ndev.offsets, ndev.U, plan, gain, B, n, T, src, mix, nz)

    def buffers():
        return [to_device(torch.zeros(1, dtype=torch.int64)), to_device(torch.full((B, R, 4), SENTINEL, dtype=torch.int64)), to_device(torch.full((B, R), float("nan")))] + \
               [to_device(torch.full(shape, float("nan"))) for shape in ((B, n, T), (B, 1, T), (B, 1, T))]
    eager_bufs, eager = buffers(), []
    for _ in range(3):
        call(*eager_bufs)
        device_sync()
        eager.append([t.cpu().clone() for t in eager_bufs])
    bufs, seq = buffers(), sepkernels.Sequence()
    with sepkernels.recording(seq):
        call(*bufs)
    assert seq.names() == ["sep_mix_draw", "sep_mix_render"]
    bufs[0].fill_(0)                                                         # the recording ran step 0: rewind
    for k in range(3):
        seq.run()
        device_sync()
        assert all(torch.equal(a.cpu(), b) for a, b in zip(bufs, eager[k])), "replay {} differs from eager call {}".format(k, k)
    assert int(bufs[0].cpu()) == 3 and not torch.equal(eager[0][3], eager[1][3])
    want_plan, want_gain = plan_ref(corpus, noise, table.cpu(), ntable.cpu(), 1 << 63, 2, B, 0, B, n, T)
    assert torch.equal(eager[2][1], want_plan) and torch.equal(eager[2][2], want_gain)


@pytest.mark.parametrize("kind", KINDS)
def test_recorded_sequence_replays_into_the_next_batches(kind):
    case_sequence(kind)


# ---------------------------------------------------------------------------------------------------------------- (4) partition invariance
def case_partition(kind):
    corpus, noise = device_corpus(kind), device_corpus(kind, make_noise)
    whole = MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=6, seed=5, noise=noise, rank=0, world=1)
    halves = [MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=3, seed=5, noise=noise, rank=r, world=2) for r in (0, 1)]
    for step in range(3):
        w = whole()
        parts = [h() for h in halves]
        for k in range(3):                               # mixture, sources, noise
            assert torch.equal(w[k], torch.cat([p[k] for p in parts])), "step {}: the halves are not the whole".format(step)
        assert torch.equal(whole.plan[0], torch.cat([h.plan[0] for h in halves])) and torch.equal(whole.plan[1], torch.cat([h.plan[1] for h in halves]))
    assert tuple(w[0].shape) == (6, 1, 64) and tuple(w[1].shape) == (6, 2, 64) and tuple(w[2].shape) == (6, 1, 64) and w[0].device == corpus.device


@pytest.mark.parametrize("kind", KINDS)
def test_partition_invariance(kind):
    case_partition(kind)


# ---------------------------------------------------------------------------------------------------------------- (5) the loader's files
MIX_IDS = ["011a0101_1.5_02bo0302_-1.5", "011a0102_0.3_22ga0101_-0.3", "02bo0302_2.1_22ga0102_-2.1", "22ga0101_0.7_011a0101_-0.7"]


def write_mix_folder(root, lengths=(700, 900, 650, 1200)):
    """a wsj0-mix style folder of 16-bit wavs; 011a0101, 02bo0302 and 22ga0101 appear twice, in copies of different lengths -> {name: longest (1, T) tensor}"""
    from recipes.audio_io import read_wav, write_wav
    g = torch.Generator().manual_seed(11)
    for sub in ("mix", "s1", "s2"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    full = {}
    for ID, T in zip(MIX_IDS, lengths):
        names = ID.split("_")[0::2]
        for k, name in enumerate(names):
            if name not in full:
                full[name] = 0.3 * torch.randn(1, 1500, generator=g)
            write_wav(os.path.join(root, "s{}".format(k + 1), ID + ".wav"), full[name][:, :T], 8000, 16)
        write_wav(os.path.join(root, "mix", ID + ".wav"), sum(full[n][:, :T] for n in names).clamp(-1, 1), 8000, 16)
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("\n".join(MIX_IDS) + "\n")
    return read_wav


def case_loader_equivalence(root):
    from recipes.dynamic_mixing import corpus_from_mix_list
    read_wav = write_mix_folder(root)
    corpus = corpus_from_mix_list(root, os.path.join(root, "list.txt"), 2, normalize=False, device=corpus_device())
    assert corpus.dtype == torch.int16 and corpus.num_speakers == 3 and corpus.num_utterances == 5 and bool((corpus.level == 1).all())
    T, B = 800, 6
    mixer = MX.DynamicMixer(corpus, n_sources=2, samples=T, batch_size=B, seed=3, gain_db=(0.0, 0.0), gain_steps=1)
    seen_long = seen_short = False
    for _ in range(3):
        mixture, sources = mixer()
        plan, gain = mixer.plan[0].cpu(), mixer.plan[1].cpu()
        assert bool((gain == 1).all())
        for b in range(B):
            for i in range(2):
                u, start, lead, _ = plan[b, i].tolist()
                wav = read_wav(corpus.paths[u])[0][0]
                want = torch.zeros(T)
                count = min(T - lead, wav.numel() - start)
                want[lead:lead + count] = wav[start:start + count]
                assert torch.equal(sources[b, i].cpu(), want), (b, i, plan[b, i].tolist())
                seen_long, seen_short = seen_long or wav.numel() >= T, seen_short or wav.numel() < T
            assert torch.equal(mixture[b, 0], sources[b, 0] + sources[b, 1])
            assert corpus.names[plan[b, 0, 0]][:3] != corpus.names[plan[b, 1, 0]][:3]
    assert seen_long and seen_short


def test_sources_are_the_crops_of_the_wav_files(tmp_path):
    case_loader_equivalence(str(tmp_path))


# ---------------------------------------------------------------------------------------------------------------- (6) training
def case_training(kind):
    """three steps of a tiny fused Conv-TasNet under FusedTrainStep on mixer() batches, and on the batches of the composed route of an identically seeded
    mixer moved to the device: the losses are equal bit for bit"""
    from oracle.make_golden import CONFIGS
    from criterion.pit import PIT1d
    from criterion.sdr import NegSISDR
    from models.conv_tasnet import ConvTasNet
    from sepkernels.train import FusedTrainStep
    dev = corpus_device()
    runs = []
    for composed in (False, True):
        corpus = make_corpus(kind) if composed else device_corpus(kind)
        mixer = MX.DynamicMixer(corpus, n_sources=2, samples=803, batch_size=2, seed=21, composed=composed)
        torch.manual_seed(1)
        model = ConvTasNet(**CONFIGS["tiny"]).to(dev)
        step = FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=2), lr=1e-3, max_norm=5.0)
        losses = []
        for _ in range(3):
            mixture, sources = mixer()
            assert mixture.device.type == ("cpu" if composed else torch.device(dev).type)
            losses.append(float(step(mixture.to(dev), sources.to(dev))))
        runs.append(losses)
    assert runs[0] == runs[1] and len(set(runs[0])) == 3 and all(x == x for x in runs[0]), runs


def test_three_training_steps_fed_by_the_mixer():
    case_training("int16")
