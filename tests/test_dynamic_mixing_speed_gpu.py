"""GPU: speed perturbation in dynamic mixing (sepkernels/mixing.py: DynamicMixer(speeds=...); csrc/mixing.hip: sep_mix_draw_speed, sep_mix_render_speed).

The oracle of the draw is the rule of include/sepkernels.h restated in Python integers (draw_item_speed: the speed index of source i is
below(word(.., 4 n + 3 + i), J), the position is drawn from len' = ceil(u len / o)); plans, gains and speed indices are compared with torch.equal.  The
oracle of the render is the formula restated in Python floats (fp64) on the DEVICE's plan, bit for bit:
    v[i u + p] = (float)(sum over k < Kc, ascending, from +0.0, in fp64, of (double)table[k][p] * (double)x[i o + first[p] + k - width]),  x raw, 0 outside its utterance
    src[t] = gain * (v[start + t - lead] * scale)  where lead <= t and t - lead < len' - start,  +0.0f elsewhere
with table / first / Kc / width of sepkernels.resample.get_filter(P, 100).  Fixture corpus, guard bands and hooks are those of
tests/test_dynamic_mixing_gpu.py, so tests/test_dynamic_mixing_speed_cpu.py runs the case functions on the host simulation of the kernel source.

(1) draw: (B, n) x T x steps 0 .. 15 x rank 0 of 1 and 1 of 2, with and without noise, speeds (95, 100, 105) and (50, 97, 200); speeds = (100,) is
sep_mix_draw; the known answers.   (2) render: both kinds, T 16 and 64 (16-byte stores), 30 and an offset view (scalar stores); instances by name; bands,
inputs and filter buffers unchanged; a second run.   (3) hand-written plans: every phase of P = 97, 50, 200 on the 257-sample utterance with both
zero-extended edges, the one-sample utterance at every speed, start 0 .. 7, a row across a workgroup's tile boundary.   (4) copy rows are
sep_mix_render's.   (5) agreement with resample() within 2^-22 max|x| max_p sum_k |h[p][k]|.   (6) direction: a 1 kHz tone comes out at 10 P Hz.
(7) the mixer: seek, state, partition invariance, a recorded Sequence, a training step."""
import math

import numpy as np
import pytest
import torch

import sepkernels
import test_dynamic_mixing_gpu as TG
from sepkernels import mixing as MX
from sepkernels.resample import get_filter, resample
from test_dynamic_mixing_gpu import OnDevice, banded, bands_intact, below, make_corpus, make_noise, word

pytestmark = pytest.mark.gpu

KINDS = TG.KINDS
SPEED_SETS = [(95, 100, 105), (50, 97, 200)]
MASK = TG.MASK
SPEED_SENTINEL = -(1 << 30) - 12345


# ---------------------------------------------------------------------------------------------------------------- the definition, restated
class Speed:
    """o, u and the compact filter of one percentage (None for P = 100)"""

    def __init__(self, P):
        g = math.gcd(P, 100)
        self.P, self.o, self.u = P, P // g, 100 // g
        self.flt = None if P == 100 else get_filter(P, 100)
        if self.flt is not None:
            assert (self.flt.o, self.flt.u) == (self.o, self.u) and self.flt.Kc <= 25 and self.flt.table.shape == (self.flt.Kc, self.u)

    def length(self, length):
        return min(max(-(-self.u * length // self.o), 1), (1 << 31) - 1)


class Filters:
    """the descriptors and filter buffers of a list of speeds as include/sepkernels.h lays them out, on the device of the hooks, with the host copies"""

    def __init__(self, speeds):
        self.speeds = [Speed(P) for P in speeds]
        desc, tables, firsts = [], [torch.zeros(0)], [torch.zeros(0, dtype=torch.int32)]
        toff = foff = 0
        for s in self.speeds:
            if s.flt is None:
                desc.append([1, 1, 0, 1, 0, 0, 100, 0])
                continue
            desc.append([s.o, s.u, s.flt.width, s.flt.Kc, toff, foff, s.P, 0])
            tables.append(s.flt.table.reshape(-1))
            firsts.append(s.flt.first.reshape(-1).to(torch.int32))
            toff, foff = toff + s.flt.Kc * s.u, foff + s.u
        if toff == 0:
            tables.append(torch.zeros(1))
            firsts.append(torch.zeros(1, dtype=torch.int32))
        self.host = [torch.tensor(desc, dtype=torch.int32), torch.cat(tables).float().contiguous(), torch.cat(firsts).contiguous()]
        self.desc, self.table, self.first = (TG.to_device(t) for t in self.host)
        self.J = len(speeds)

    def unchanged(self):
        return all(torch.equal(a.cpu(), b) for a, b in zip((self.desc, self.table, self.first), self.host))


def draw_item_speed(seed, item, n, T, G, speeds, spk_first=TG.SPK_FIRST, lengths=TG.LENGTHS, noise_lengths=None, G_noise=None):
    """-> rows (speaker, utterance, start, lead, gain index, speed index); the noise row (speaker -1, speed index -1) last"""
    S, rows, chosen = len(spk_first) - 1, [], []
    for i in range(n):
        r = below(word(seed, item, i), S - i)
        for c in chosen:
            if r >= c:
                r += 1
        chosen = sorted(chosen + [r])
        u = spk_first[r] + below(word(seed, item, n + i), spk_first[r + 1] - spk_first[r])
        j = below(word(seed, item, 4 * n + 3 + i), len(speeds))
        start, lead = TG.place(speeds[j].length(lengths[u]), T, word(seed, item, 2 * n + i))
        rows.append((r, u, start, lead, below(word(seed, item, 3 * n + i), G), j))
    if noise_lengths is not None:
        u = below(word(seed, item, 4 * n), len(noise_lengths))
        start, lead = TG.place(noise_lengths[u], T, word(seed, item, 4 * n + 1))
        rows.append((-1, u, start, lead, below(word(seed, item, 4 * n + 2), G_noise), -1))
    return rows


def plan_ref_speed(corpus, noise, table, noise_table, seed, step, stride, first, B, n, T, speeds):
    """-> plan (B, R, 4) int64, gain (B, R) float32, speed (B, R) int32 by the rule, on the CPU"""
    plan, gain, speed = [], [], []
    for b in range(B):
        rows = draw_item_speed(seed, (step * stride + first + b) & MASK, n, T, table.numel(), speeds, corpus.spk_first_host.tolist(), corpus.lengths().tolist(),
                               None if noise is None else noise.lengths().tolist(), None if noise is None else noise_table.numel())
        plan.append([list(r[1:5]) for r in rows])
        speed.append([r[5] for r in rows])
        gain.append(torch.stack([(corpus.level.cpu()[r[1]] * table[r[4]]) if r[0] >= 0 else (noise.level.cpu()[r[1]] * noise_table[r[4]]) for r in rows]))
    return torch.tensor(plan, dtype=torch.int64), torch.stack(gain), torch.tensor(speed, dtype=torch.int32)


def perturbed(x, s):
    """the perturbed utterance v (list of np.float32, len' entries) of the raw samples x (list of Python numbers) at speed s: the fp64 sum, tap by tap"""
    f = s.flt
    table, first = f.table.tolist(), f.first.tolist()
    out = []
    for m in range(s.length(len(x))):
        i, p = divmod(m, s.u)
        acc = 0.0
        for k in range(f.Kc):
            e = i * s.o + first[p] + k - f.width
            acc = acc + table[k][p] * (float(x[e]) if 0 <= e < len(x) else 0.0)          # Python floats are fp64; the product is exact
        out.append(np.float32(acc))
    return out


def render_ref_speed(corpus, noise, plan, gain, speed, speeds, n, T, cache=None):
    """the formula of sep_mix_render_speed with its clamps and its predicate -> sources (B, n, T), mixture (B, 1, T), noise (B, 1, T) or None on the CPU"""
    cache = {} if cache is None else cache
    J = len(speeds)

    def row(c, p, g, j):
        j = min(max(int(j), -1), J - 1)
        if j < 0 or speeds[j].flt is None:
            return None
        samples, off = c.samples.cpu(), c.offsets_host
        u = min(max(int(p[0]), 0), c.num_utterances - 1)
        key = (id(c), u, j)
        if key not in cache:
            cache[key] = perturbed(samples[int(off[u]):int(off[u + 1])].tolist(), speeds[j])
        v = cache[key]
        start, lead = max(min(int(p[1]), len(v) - 1), 0), int(p[2])
        scale, g32 = np.float32(2.0 ** -15 if samples.dtype == torch.int16 else 1.0), np.float32(float(g))
        out = np.zeros(T, dtype=np.float32)
        for t in range(max(lead, 0), min(T, lead + len(v) - start)):
            out[t] = g32 * (v[start + t - lead] * scale)
        return torch.from_numpy(out)
    B, R = plan.shape[0], plan.shape[1]
    assert R == n + (noise is not None) and tuple(speed.shape) == (B, R)
    plan, gain = plan.cpu(), gain.cpu()
    copies = TG.render_ref(corpus, noise, plan, gain, n, T)
    src = copies[0].clone()
    for b in range(B):
        for i in range(n):
            r = row(corpus, plan[b, i], gain[b, i], speed[b, i])
            if r is not None:
                src[b, i] = r
    mix = src[:, 0]
    for i in range(1, n):
        mix = mix + src[:, i]
    if noise is None:
        return src, mix.unsqueeze(1), None
    return src, mix.unsqueeze(1) + copies[2], copies[2]                                        # the noise row is never perturbed


# ---------------------------------------------------------------------------------------------------------------- the entry points on banded buffers
def device_draw_speed(dev, noise_dev, table, noise_table, counter, seed, stride, first, B, n, T, filt):
    """one sep_mix_draw_speed into fresh banded buffers -> plan (B, R, 4), gain (B, R), speed (B, R) on the CPU"""
    R = n + (noise_dev is not None)
    pbuf, plan = banded(B * R * 4, torch.int64)
    gbuf, gain = banded(B * R, torch.float32)
    sbuf = TG.to_device(torch.full((2 * TG.BAND + B * R,), SPEED_SENTINEL, dtype=torch.int32))          # (TG.banded's sentinel does not fit an int32)
    speed = sbuf[TG.BAND:TG.BAND + B * R]
    TG.HIP.mix_draw_speed(dev.offsets, dev.spk_first, dev.U, dev.S, None if noise_dev is None else noise_dev.offsets, 0 if noise_dev is None else noise_dev.U, dev.level,
                          table, table.numel(), None if noise_dev is None else noise_dev.level, noise_table, 0 if noise_dev is None else noise_table.numel(), counter, seed,
                          stride, first, B, n, T, filt.desc, filt.J, plan, gain, speed)
    TG.device_sync()
    edge = torch.cat([sbuf.cpu()[:TG.BAND], sbuf.cpu()[TG.BAND + B * R:]])
    assert bands_intact(pbuf, B * R * 4) and bands_intact(gbuf, B * R) and bool((edge == SPEED_SENTINEL).all()), "a guard band of the plan was written"
    assert dev.unchanged() and (noise_dev is None or noise_dev.unchanged()) and filt.unchanged(), "the draw changed an input"
    return plan.cpu().view(B, R, 4).clone(), gain.cpu().view(B, R).clone(), speed.cpu().view(B, R).clone()


INSTANCE = {("int16", True): "mix_render_speed<int16>", ("int16", False): "mix_render_speed_scalar<int16>",
            ("float32", True): "mix_render_speed<float>", ("float32", False): "mix_render_speed_scalar<float>"}


def device_render_speed(dev, ndev, plan, gain, speed, filt, B, n, T, shift, kind):
    """one sep_mix_render_speed of a CPU plan into banded, exactly-sized outputs; checked for bands, inputs, the instance, finiteness and a second run
    -> sources (B, n, T), mixture (B, 1, T), noise (B, 1, T) or None on the CPU"""
    plan_d, gain_d, speed_d = TG.to_device(plan.contiguous()), TG.to_device(gain.contiguous()), TG.to_device(speed.contiguous())
    runs = []
    for _ in range(2):
        sbuf, src = banded(B * n * T, torch.float32, shift)
        mbuf, mix = banded(B * T, torch.float32, shift)
        zbuf, nz = banded(B * T, torch.float32, shift) if ndev is not None else (None, None)
        TG.HIP.mix_render_speed(dev.samples, dev.offsets, dev.U, None if ndev is None else ndev.samples, None if ndev is None else ndev.offsets,
                                0 if ndev is None else ndev.U, plan_d, gain_d, speed_d, filt.desc, filt.J, filt.table, filt.first, B, n, T, src, mix, nz)
        TG.device_sync()
        vector = T % 4 == 0 and all(t is None or t.data_ptr() % 16 == 0 for t in (src, mix, nz))
        assert vector == (T % 4 == 0 and shift % 4 == 0), "the test's buffers are not aligned as it believes"
        assert sepkernels.last_kernel() == INSTANCE[(kind, vector)], (sepkernels.last_kernel(), kind, T, shift)
        assert bands_intact(sbuf, B * n * T, shift) and bands_intact(mbuf, B * T, shift) and (zbuf is None or bands_intact(zbuf, B * T, shift)), "a guard band was written"
        assert dev.unchanged() and (ndev is None or ndev.unchanged()) and filt.unchanged() and torch.equal(plan_d.cpu(), plan) and torch.equal(speed_d.cpu(), speed) and \
            torch.equal(gain_d.cpu().view(torch.int32), gain.contiguous().view(torch.int32)), "an input was changed"
        out = (src.cpu().view(B, n, T).clone(), mix.cpu().view(B, 1, T).clone(), None if nz is None else nz.cpu().view(B, 1, T).clone())
        assert all(o is None or bool(torch.isfinite(o).all()) for o in out), "an output element was left unwritten"
        runs.append(out)
    assert all(a is None or torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs)), "a second run gave other bits"
    return runs[0]


# ---------------------------------------------------------------------------------------------------------------- (1) the draw
def case_draw_speed(B, n, T, with_noise, speeds, seed=1234):
    corpus, noise = make_corpus("int16"), make_noise("int16") if with_noise else None
    dev, ndev, filt = OnDevice(corpus), OnDevice(noise) if with_noise else None, Filters(speeds)
    table_h, ntable_h = MX.gain_table(-2.5, 2.5, 256), MX.gain_table(-6.0, 3.0, 256)
    table, ntable = TG.to_device(table_h), TG.to_device(ntable_h) if with_noise else None
    seen = set()
    for rank, world in ((0, 1), (1, 2)):
        counter = TG.to_device(torch.zeros(1, dtype=torch.int64))
        for step in range(16):
            plan, gain, speed = device_draw_speed(dev, ndev, table, ntable, counter, seed, B * world, rank * B, B, n, T, filt)
            want = plan_ref_speed(corpus, noise, table_h, ntable_h, seed, step, B * world, rank * B, B, n, T, filt.speeds)
            assert torch.equal(plan, want[0]), (B, n, T, rank, step, plan.tolist(), want[0].tolist())
            assert torch.equal(gain, want[1]) and torch.equal(speed, want[2]), (B, n, T, rank, step, speed.tolist(), want[2].tolist())
            assert int(counter.cpu()) == step + 1, "the kernel leaves counter + 1"
            assert not with_noise or bool((speed[:, n] == -1).all())
            seen |= set(speed[:, :n].reshape(-1).tolist())
    assert B * n < 4 or seen == set(range(len(speeds))), seen


@pytest.mark.parametrize("speeds", SPEED_SETS, ids=["95-100-105", "50-97-200"])
@pytest.mark.parametrize("with_noise", [False, True], ids=["speech", "noise"])
@pytest.mark.parametrize("T", TG.DRAW_T)
@pytest.mark.parametrize("B,n", TG.DRAW_BN)
def test_draw_is_the_rule(B, n, T, with_noise, speeds):
    case_draw_speed(B, n, T, with_noise, speeds)


def case_identity_draw():
    """speeds = (100,): the plan and the gains are sep_mix_draw's, every speed index is 0"""
    corpus, noise = make_corpus("int16"), make_noise("int16")
    dev, ndev, filt = OnDevice(corpus), OnDevice(noise), Filters((100,))
    table, ntable = TG.to_device(MX.gain_table(-2.5, 2.5, 256)), TG.to_device(MX.gain_table(-6.0, 3.0, 256))
    for T in (16, 64, 300):
        for with_noise in (False, True):
            nd, nt = (ndev, ntable) if with_noise else (None, None)
            a, b = TG.to_device(torch.tensor([5], dtype=torch.int64)), TG.to_device(torch.tensor([5], dtype=torch.int64))
            plan, gain, speed = device_draw_speed(dev, nd, table, nt, a, 77, 5, 0, 5, 2, T, filt)
            want_plan, want_gain = TG.device_draw(dev, nd, table, nt, b, 77, 5, 0, 5, 2, T)
            assert torch.equal(plan, want_plan) and torch.equal(gain, want_gain) and bool((speed[:, :2] == 0).all()) and int(a.cpu()) == int(b.cpu()) == 6


def test_one_identity_speed_is_the_plain_draw():
    case_identity_draw()


KNOWN_WORDS = [((1234, 0, 11), 0x718ad7f33aef0177, 1), ((1234, 0, 12), 0x0de521a7eba82090, 0), ((1234, 1, 11), 0x5f314ef19e801a70, 1),
               ((0, 0, 7), 0x915f11bbbfb2963d, 1), ((1 << 63, (1 << 40) + 3, 42), 0xd90fbd8340eb6aa8, 2)]


def case_known_answers():
    for args, want, j in KNOWN_WORDS:
        assert word(*args) == want and below(want, 3) == j, (args, hex(word(*args)))
    for args, want in TG.KNOWN_WORDS:
        assert word(*args) == want
    # n = 2: the speed draws of item 0 are words 11 and 12, of item 1 word 11 first -- through the device
    corpus = make_corpus("int16")
    dev, table, filt = OnDevice(corpus), TG.to_device(MX.gain_table(-2.5, 2.5, 256)), Filters((95, 100, 105))
    _, _, speed = device_draw_speed(dev, None, table, None, TG.to_device(torch.zeros(1, dtype=torch.int64)), 1234, 2, 0, 2, 2, 64, filt)
    assert speed[0].tolist() == [1, 0] and speed[1, 0].item() == 1
    # seed 2^63 and an item beyond 2^40: n = 3, source 0 draws word 4 n + 3 = 15; the rule as restated, and 320 items in ONE call
    plan, _, speed = device_draw_speed(dev, None, table, None, TG.to_device(torch.tensor([1 << 40], dtype=torch.int64)), 1 << 63, 1, 3, 1, 3, 64, filt)
    rows = draw_item_speed(1 << 63, (1 << 40) + 3, 3, 64, 256, filt.speeds)
    assert plan[0].tolist() == [list(r[1:5]) for r in rows] and speed[0].tolist() == [r[5] for r in rows]
    plan, _, speed = device_draw_speed(dev, None, table, None, TG.to_device(torch.zeros(1, dtype=torch.int64)), 1234, 320, 0, 320, 2, 64, filt)
    rows = [draw_item_speed(1234, item, 2, 64, 256, filt.speeds) for item in range(320)]
    assert plan.tolist() == [[list(r[1:5]) for r in it] for it in rows] and speed.tolist() == [[r[5] for r in it] for it in rows]
    counts = torch.bincount(speed.reshape(-1).long(), minlength=3)
    assert int(counts.min()) >= 160 and int(counts.sum()) == 640, counts.tolist()
    for j, length in enumerate((271, 257, 245)):                                        # the 257-sample utterance: a start up to len' - T
        starts = plan[:, :, 1][(plan[:, :, 0] == 6) & (speed == j)]
        assert starts.numel() > 0 and int(starts.max()) <= length - 64, (j, starts.tolist())


def test_known_answers():
    case_known_answers()


# ---------------------------------------------------------------------------------------------------------------- (2) the render
def case_render_speed(kind, T, shift, with_noise, speeds):
    """the DEVICE's plan of step 3 (B = 5; n = 2, or n = 3 plus a noise row) rendered and compared with the formula on that plan"""
    corpus, noise = make_corpus(kind), make_noise(kind) if with_noise else None
    dev, ndev, filt = OnDevice(corpus), OnDevice(noise) if with_noise else None, Filters(speeds)
    B, n = 5, 3 if with_noise else 2
    table, ntable = TG.to_device(MX.gain_table(-2.5, 2.5, 256)), TG.to_device(MX.gain_table(-6.0, 3.0, 7)) if with_noise else None
    plan, gain, speed = device_draw_speed(dev, ndev, table, ntable, TG.to_device(torch.tensor([3], dtype=torch.int64)), 99, B, 0, B, n, T, filt)
    got = device_render_speed(dev, ndev, plan, gain, speed, filt, B, n, T, shift, kind)
    TG.assert_same_bits(got, render_ref_speed(corpus, noise, plan, gain, speed, filt.speeds, n, T), "{} T {} shift {} speeds {}".format(kind, T, shift, speeds))
    assert bool(got[0].abs().sum(-1).gt(0).all()), "a source row is silent"
    assert len(set(speed[:, :n].reshape(-1).tolist())) >= 2, "the plan holds one speed only"


@pytest.mark.parametrize("speeds", SPEED_SETS, ids=["95-100-105", "50-97-200"])
@pytest.mark.parametrize("with_noise", [False, True], ids=["speech", "noise"])
@pytest.mark.parametrize("T,shift", [(16, 0), (64, 0), (30, 0), (64, 1)], ids=["T16", "T64", "T30-scalar", "T64-offset-scalar"])
@pytest.mark.parametrize("kind", KINDS)
def test_render_is_the_formula_on_the_device_plan(kind, T, shift, with_noise, speeds):
    case_render_speed(kind, T, shift, with_noise, speeds)


# ---------------------------------------------------------------------------------------------------------------- (3) hand-written plans
ALL_SPEEDS = (95, 100, 105, 50, 97, 200)


def case_every_phase(kind):
    """the 257-sample utterance from its first perturbed sample to its last and beyond, at P = 97 (u = 100: len' = 265), 50 (u = 2: 514) and 200 (u = 1: 129):
    every phase, both zero-extended edges; T = 516 (16-byte stores) and 515 (scalar)"""
    corpus = make_corpus(kind)
    dev, filt = OnDevice(corpus), Filters((97, 50, 200))
    assert [s.length(257) for s in filt.speeds] == [265, 514, 129]
    plan = torch.tensor([[[6, 0, 0, 0], [6, 0, 0, 0], [6, 0, 0, 0]], [[6, 0, 1, 0], [6, 0, 2, 0], [6, 0, 380, 0]]], dtype=torch.int64)
    gain, speed = torch.tensor([[1.0, -0.5, 2.0], [0.75, 1.0, -1.0]]), torch.tensor([[0, 1, 2], [0, 1, 2]], dtype=torch.int32)
    cache = {}
    for T in (516, 515):
        got = device_render_speed(dev, None, plan, gain, speed, filt, 2, 3, T, 0, kind)
        TG.assert_same_bits(got, render_ref_speed(corpus, None, plan, gain, speed, filt.speeds, 3, T, cache), "{} every phase, T {}".format(kind, T))
        assert bool((got[0][0, 0, 265:] == 0).all()) and bool((got[0][0, 2, 129:] == 0).all()) and float(got[0][0, 1, 513].abs()) > 0


def case_one_sample_utterance(kind):
    """the one-sample utterance at every speed (len' = 1, or 2 at P = 50), behind a lead and at t = 0"""
    corpus = make_corpus(kind)
    dev, filt = OnDevice(corpus), Filters(ALL_SPEEDS)
    assert [s.length(1) for s in filt.speeds] == [2, 1, 1, 2, 2, 1]
    plan = torch.tensor([[[0, 0, 0, 0]] * 6, [[0, 0, 13, 0]] * 6, [[0, 1, 15, 0]] * 6], dtype=torch.int64)
    gain, speed = torch.full((3, 6), 1.5), torch.arange(6, dtype=torch.int32).repeat(3, 1)
    for T in (16, 15):
        got = device_render_speed(dev, None, plan, gain, speed, filt, 3, 6, T, 0, kind)
        TG.assert_same_bits(got, render_ref_speed(corpus, None, plan, gain, speed, filt.speeds, 6, T), "{} one sample, T {}".format(kind, T))
        assert bool(got[0][:2].abs().sum(-1).gt(0).all()) and bool((got[0][:, :, 2:13] == 0).all())


def case_every_start(kind):
    """start 0 .. 7 on the last utterance of the storage, from its first perturbed sample and up to its last, at P = 95 and 105"""
    corpus = make_corpus(kind)
    dev, filt = OnDevice(corpus), Filters((95, 105))
    lens = [s.length(257) for s in filt.speeds]
    assert lens == [271, 245] and int(corpus.offsets_host[7]) == corpus.samples.numel() - MX.GUARD
    rows = [[[6, s, 0, 0], [6, lens[1] - 64 - s, 0, 0], [6, lens[0] - 16 + s - 7, 9 - s, 0]] for s in range(8)]
    plan, gain, speed = torch.tensor(rows, dtype=torch.int64), torch.tensor([[1.0, -0.5, 0.25]] * 8), torch.tensor([[0, 1, 0]] * 8, dtype=torch.int32)
    cache = {}
    for T in (64, 62):
        got = device_render_speed(dev, None, plan, gain, speed, filt, 8, 3, T, 0, kind)
        TG.assert_same_bits(got, render_ref_speed(corpus, None, plan, gain, speed, filt.speeds, 3, T, cache), "{} start 0 .. 7, T {}".format(kind, T))


def case_across_tiles(kind):
    """rows that straddle the boundary between two workgroups' tiles (2048 samples for int16, 1024 for fp32), and one that ends on it"""
    corpus = make_corpus(kind)
    dev, filt = OnDevice(corpus), Filters((50, 97, 105))
    plan = torch.tensor([[[6, 0, 1900, 0], [6, 0, 900, 0], [6, 3, 2048 - 242, 0], [5, 0, 2040, 0]]], dtype=torch.int64)
    gain, speed = torch.tensor([[1.0, 0.5, -1.0, 2.0]]), torch.tensor([[0, 1, 2, 0]], dtype=torch.int32)
    assert filt.speeds[2].length(257) == 245
    for T in (2560, 2559):
        got = device_render_speed(dev, None, plan, gain, speed, filt, 1, 4, T, 0, kind)
        TG.assert_same_bits(got, render_ref_speed(corpus, None, plan, gain, speed, filt.speeds, 4, T), "{} across tiles, T {}".format(kind, T))
        assert float(got[0][0, 0, 2047].abs()) > 0 and float(got[0][0, 0, 2048].abs()) > 0 and float(got[0][0, 2, 2047].abs()) > 0 and bool((got[0][0, 2, 2048:] == 0).all())


@pytest.mark.parametrize("kind", KINDS)
def test_every_phase_and_both_edges(kind):
    case_every_phase(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_one_sample_utterance_at_every_speed(kind):
    case_one_sample_utterance(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_every_start_up_to_the_last_sample(kind):
    case_every_start(kind)


@pytest.mark.parametrize("kind", KINDS)
def test_rows_across_the_tile_boundary(kind):
    case_across_tiles(kind)


# ---------------------------------------------------------------------------------------------------------------- (4) copy rows
def case_copy_rows(kind):
    """P = 100 rows and the noise row are sep_mix_render's output for the same plan, bit for bit -- beside perturbed rows in the same items"""
    corpus, noise = make_corpus(kind), make_noise(kind)
    dev, ndev, filt = OnDevice(corpus), OnDevice(noise), Filters((95, 100, 105))
    table, ntable = TG.to_device(MX.gain_table(-2.5, 2.5, 256)), TG.to_device(MX.gain_table(-6.0, 3.0, 7))
    for T, shift in ((64, 0), (30, 0), (64, 1)):
        plan, gain = TG.device_draw(dev, ndev, table, ntable, TG.to_device(torch.tensor([2], dtype=torch.int64)), 5, 6, 0, 6, 3, T)
        plain = TG.device_render(dev, ndev, plan, gain, 6, 3, T, shift, kind)
        speed = torch.tensor([[1, 1, 1, -1]] * 6, dtype=torch.int32)
        TG.assert_same_bits(device_render_speed(dev, ndev, plan, gain, speed, filt, 6, 3, T, shift, kind), plain, "{} copy rows T {}".format(kind, T))
        speed[:, 1] = torch.tensor([0, 2, 0, 2, 0, 2], dtype=torch.int32)                     # the middle source perturbed: the others and the noise row stay
        got = device_render_speed(dev, ndev, plan, gain, speed, filt, 6, 3, T, shift, kind)
        assert torch.equal(got[0][:, 0], plain[0][:, 0]) and torch.equal(got[0][:, 2], plain[0][:, 2]) and torch.equal(got[2], plain[2])
        assert not torch.equal(got[0][:, 1], plain[0][:, 1]) and torch.equal(got[1], ((got[0][:, 0] + got[0][:, 1]) + got[0][:, 2]).unsqueeze(1) + got[2])


@pytest.mark.parametrize("kind", KINDS)
def test_copy_rows_are_the_plain_render(kind):
    case_copy_rows(kind)


# ---------------------------------------------------------------------------------------------------------------- (5) the project's resampler
def case_resampler_agreement(kind):
    """every utterance at every speed, gain 1, start 0: within 2^-22 max|x| max_p sum_k |h[p][k]| of resample(utterance.double(), P, 100) -- fp32 taps, one
    output rounding and the dropped taps, with a factor of two of margin (the bound is about 3e-7 for |x| <= 1)"""
    corpus = make_corpus(kind)
    speeds = tuple(P for P in ALL_SPEEDS if P != 100)
    dev, filt = OnDevice(corpus), Filters(speeds)
    U, J, T = corpus.num_utterances, len(speeds), 516
    plan = torch.tensor([[[u, 0, 0, 0]] * J for u in range(U)], dtype=torch.int64)
    gain, speed = torch.ones(U, J), torch.arange(J, dtype=torch.int32).repeat(U, 1)
    got = device_render_speed(dev, None, plan, gain, speed, filt, U, J, T, 0, kind)[0].double()
    scale = 2.0 ** -15 if kind == "int16" else 1.0
    for u in range(U):
        x = corpus.utterance(u).cpu().double()
        for j, s in enumerate(filt.speeds):
            want = resample(x, s.P, 100) * scale
            assert want.numel() == s.length(x.numel())
            bound = 2.0 ** -22 * float(x.abs().max()) * scale * float(s.flt.h.abs().sum(1).max())
            err = float((got[u, j, :want.numel()] - want).abs().max())
            assert err <= bound, (kind, u, s.P, err, bound)
            assert bool((got[u, j, want.numel():] == 0).all())


@pytest.mark.parametrize("kind", KINDS)
def test_perturbed_rows_agree_with_the_resampler(kind):
    case_resampler_agreement(kind)


# ---------------------------------------------------------------------------------------------------------------- (6) direction
def tone_corpus(cache={}):
    if "c" not in cache:
        t = torch.arange(4000, dtype=torch.float64)
        tone = lambda ph: torch.round(20000.0 * torch.sin(2 * math.pi * 1000.0 * t / 8000.0 + ph)).to(torch.int16)          # noqa: E731
        cache["c"] = MX.DeviceCorpus.from_waveforms([tone(0.0), tone(1.0)], [0, 1], normalize=False)
    return cache["c"]


def case_direction():
    """1 kHz int16 tones, amplitude 20000, 4000 samples at 8 kHz: the peak of a 2048-point Hann DFT of a rendered source lies within one bin of 10 P Hz"""
    corpus = tone_corpus()
    speeds = (95, 105, 50, 200, 100)
    dev, filt = OnDevice(corpus), Filters(speeds)
    T = 2048
    plan = torch.tensor([[[0, 0, 0, 0]] * 5], dtype=torch.int64)
    speed = torch.arange(5, dtype=torch.int32).view(1, 5)
    src = device_render_speed(dev, None, plan, torch.ones(1, 5), speed, filt, 1, 5, T, 0, "int16")[0][0].double()
    for j, P in enumerate(speeds):
        n = min(T, filt.speeds[j].length(4000))                      # P = 200 has 2000 samples: the DFT of what there is, zero-padded
        spec = torch.fft.rfft(src[j] * torch.cat([torch.hann_window(n, periodic=True, dtype=torch.float64), torch.zeros(T - n, dtype=torch.float64)])).abs()
        peak = int(spec.argmax())
        assert abs(peak - 1000.0 * P / 100.0 * 2048 / 8000.0) <= 1.0, (P, peak)
        rms = float(src[j][:n].pow(2).mean().sqrt()) / (20000.0 / 32768.0 / math.sqrt(2.0))
        assert abs(rms - 1.0) < 0.02, (P, rms)                       # the level is not renormalised, and need not be


def test_a_tone_moves_with_the_speed():
    case_direction()


# ---------------------------------------------------------------------------------------------------------------- (7) the mixer
def case_mixer(kind):
    """seek, the state-dict round trip with speeds, partition invariance, and the device route against the rule and the formula"""
    speeds = (95, 100, 105)
    corpus, noise = TG.device_corpus(kind), TG.device_corpus(kind, make_noise)
    mixer = MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=4, seed=7, speeds=speeds)
    assert mixer.speeds == speeds and mixer.step == 0 and mixer.speed is None
    first, second = mixer(), mixer()
    assert mixer.step == 2 and int(mixer._counter.cpu()) == 2 and tuple(mixer.speed.shape) == (4, 2) and mixer.speed.dtype == torch.int32
    table, ref_speeds = MX.gain_table(-2.5, 2.5, 256), [Speed(P) for P in speeds]
    for k, got in enumerate((first, second)):
        want = plan_ref_speed(make_corpus(kind), None, table, None, 7, k, 4, 0, 4, 2, 64, ref_speeds)
        src, mix, _ = render_ref_speed(make_corpus(kind), None, *want, ref_speeds, 2, 64)
        assert torch.equal(got[0].cpu(), mix) and torch.equal(got[1].cpu(), src), "step {}".format(k)
    assert torch.equal(mixer.plan[0].cpu(), want[0]) and torch.equal(mixer.plan[1].cpu(), want[1]) and torch.equal(mixer.speed.cpu(), want[2])
    plain = MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=4, seed=7)
    assert not torch.equal(plain()[1], first[1]), "the speed mixer renders the plain mixer's batch"
    mixer.seek(0)
    again = mixer()
    assert mixer.step == 1 and torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]), "seek(0) rewinds the stream"
    state = mixer.state_dict()
    assert state == {"seed": 7, "step": 1, "speeds": [95, 100, 105]}
    resumed = MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=4, seed=0, speeds=speeds)
    resumed.load_state_dict(state)
    out = resumed()
    assert torch.equal(out[0], second[0]) and torch.equal(out[1], second[1]), "a resumed mixer continues the stream"
    assert torch.equal(mixer.render(*resumed.plan, resumed.speed)[1], second[1]), "render(plan, gain, speed) of a logged plan"
    for other in (MX.DynamicMixer(corpus, samples=64, batch_size=4, speeds=(95, 105)), plain):
        with pytest.raises(ValueError, match="stream would differ"):
            other.load_state_dict(state)
    with pytest.raises(ValueError, match="stream would differ"):
        mixer.load_state_dict({"seed": 7, "step": 1})
    with pytest.raises(ValueError, match="speed"):
        mixer.render(*resumed.plan)
    # two ranks of B are one of 2 B, with a noise row
    whole = MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=6, seed=5, noise=noise, rank=0, world=1, speeds=speeds)
    halves = [MX.DynamicMixer(corpus, n_sources=2, samples=64, batch_size=3, seed=5, noise=noise, rank=r, world=2, speeds=speeds) for r in (0, 1)]
    for step in range(3):
        w = whole()
        parts = [h() for h in halves]
        for k in range(3):
            assert torch.equal(w[k], torch.cat([p[k] for p in parts])), "step {}: the halves are not the whole".format(step)
        assert torch.equal(whole.plan[0], torch.cat([h.plan[0] for h in halves])) and torch.equal(whole.speed, torch.cat([h.speed for h in halves]))
    assert bool((whole.speed[:, 2] == -1).all()) and tuple(w[2].shape) == (6, 1, 64)


@pytest.mark.parametrize("kind", KINDS)
def test_mixer_seek_state_and_partition(kind):
    case_mixer(kind)


def case_sequence(kind):
    """ONE recorded draw + render replayed three times equals three eager calls bit for bit"""
    corpus, noise = make_corpus(kind), make_noise(kind)
    dev, ndev, filt = OnDevice(corpus), OnDevice(noise), Filters((95, 100, 105))
    B, n, T, R = 3, 2, 64, 3
    table, ntable = TG.to_device(MX.gain_table(-2.5, 2.5, 256)), TG.to_device(MX.gain_table(-6.0, 3.0, 256))

    def call(counter, plan, gain, speed, src, mix, nz):
        TG.HIP.mix_draw_speed(dev.offsets, dev.spk_first, dev.U, dev.S, ndev.offsets, ndev.U, dev.level, table, 256, ndev.level, ntable, 256, counter, 1 << 63, B, 0, B, n, T,
                              filt.desc, filt.J, plan, gain, speed)
        TG.HIP.mix_render_speed(dev.samples, dev.offsets, dev.U, ndev.samples, ndev.offsets, ndev.U, plan, gain, speed, filt.desc, filt.J, filt.table, filt.first, B, n, T,
                                src, mix, nz)

    def buffers():
        return [TG.to_device(torch.zeros(1, dtype=torch.int64)), TG.to_device(torch.full((B, R, 4), TG.SENTINEL, dtype=torch.int64)), TG.to_device(torch.full((B, R), float("nan"))),
                TG.to_device(torch.full((B, R), -7, dtype=torch.int32))] + [TG.to_device(torch.full(shape, float("nan"))) for shape in ((B, n, T), (B, 1, T), (B, 1, T))]
    eager_bufs, eager = buffers(), []
    for _ in range(3):
        call(*eager_bufs)
        TG.device_sync()
        eager.append([t.cpu().clone() for t in eager_bufs])
    bufs, seq = buffers(), sepkernels.Sequence()
    with sepkernels.recording(seq):
        call(*bufs)
    assert seq.names() == ["sep_mix_draw_speed", "sep_mix_render_speed"]
    bufs[0].fill_(0)
    for k in range(3):
        seq.run()
        TG.device_sync()
        assert all(torch.equal(a.cpu(), b) for a, b in zip(bufs, eager[k])), "replay {} differs from eager call {}".format(k, k)
    assert int(bufs[0].cpu()) == 3 and not torch.equal(eager[0][4], eager[1][4])
    want = plan_ref_speed(corpus, noise, table.cpu(), ntable.cpu(), 1 << 63, 2, B, 0, B, n, T, filt.speeds)
    assert torch.equal(eager[2][1], want[0]) and torch.equal(eager[2][2], want[1]) and torch.equal(eager[2][3], want[2])
    src, mix, nz = render_ref_speed(corpus, noise, *want, filt.speeds, n, T)
    assert torch.equal(eager[2][4], src) and torch.equal(eager[2][5], mix) and torch.equal(eager[2][6], nz)


@pytest.mark.parametrize("kind", KINDS)
def test_recorded_sequence_replays_into_the_next_batches(kind):
    case_sequence(kind)


def case_training(kind):
    """one step of a tiny fused Conv-TasNet on a batch of the speed mixer, and on the batch of the composed route of an identically seeded mixer: equal losses"""
    from oracle.make_golden import CONFIGS
    from criterion.pit import PIT1d
    from criterion.sdr import NegSISDR
    from models.conv_tasnet import ConvTasNet
    from sepkernels.train import FusedTrainStep
    dev = TG.corpus_device()
    runs = []
    for composed in (False, True):
        corpus = make_corpus(kind) if composed else TG.device_corpus(kind)
        mixer = MX.DynamicMixer(corpus, n_sources=2, samples=803, batch_size=2, seed=21, composed=composed, speeds=(95, 100, 105))
        torch.manual_seed(1)
        model = ConvTasNet(**CONFIGS["tiny"]).to(dev)
        step = FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=2), lr=1e-3, max_norm=5.0)
        mixture, sources = mixer()
        assert mixture.device.type == ("cpu" if composed else torch.device(dev).type) and tuple(sources.shape) == (2, 2, 803)
        runs.append((float(step(mixture.to(dev), sources.to(dev))), mixer.speed.cpu().tolist()))
    assert runs[0] == runs[1] and math.isfinite(runs[0][0]), runs


def test_a_training_step_fed_by_the_speed_mixer():
    case_training("int16")
