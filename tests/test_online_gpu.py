"""GPU: online (chunk-by-chunk) separation of a causal Conv-TasNet (sepkernels/online.py, csrc/online.hip).

The kernel cases (`case_*`, listed in CASES) check every sep_online_* entry point against a torch fp64 restatement of the reference formulas --
filterbank.py:205-251 (encoder / decoder), modules/norm.py:58-101 (cLN), tdcn.py:125-132 (causal dilated taps) -- fed chunk after chunk, so
the state they carry (encoder carry, fp64 cLN sums, depthwise histories, overlap-add tail) is checked too.  tests/test_online_cpu.py runs the
same functions on the host simulation of the kernel sources (it swaps HIP, to_device and device_sync).  The model tests stream the reference's
fixture and a paper-size causal model through the online path on the device."""
import os

import numpy as np
import pytest
import torch

import sepkernels

pytestmark = pytest.mark.gpu

HIP = sepkernels.HipBackend()
G = torch.Generator().manual_seed(2024)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def to_device(t):
    return t.cuda()


def device_sync():
    torch.cuda.synchronize()


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, generator=G) * scale).float()


def close(got, ref, tol, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert torch.isfinite(got).all(), what + ": non-finite values"
    err, den = (got - ref).abs().max().item(), ref.abs().max().item() + 1e-30
    assert err <= tol * den, "{}: max err {:.3e} vs scale {:.3e}".format(what, err, den)


def _round_up(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------------------------------------------ fp64 restatements of the reference
def ref_encoder(x, E, S, relu):
    """x (Bs, T) whole signal (pre-roll included), E (N, L) -> (Bs, N, F) with F = (T - L) / S + 1 (filterbank.py:205-235)"""
    L = E.shape[1]
    fr = x.double().unfold(1, L, S)                                   # (Bs, F, L)
    y = torch.einsum("bfl,nl->bnf", fr, E.double())
    return y.clamp_min(0) if relu else y


def ref_cln(u, gamma, beta, eps):
    """u (Bs, C, F) -> cumulative layer norm over channels and frames <= t (norm.py:58-101), fp64"""
    C = u.shape[1]
    n = torch.arange(1, u.shape[2] + 1, dtype=torch.float64) * C
    m = u.sum(1).cumsum(1) / n
    var = ((u * u).sum(1).cumsum(1) / n - m * m).clamp_min(0)
    return (u - m.unsqueeze(1)) / (var.sqrt().unsqueeze(1) + eps) * gamma.double().view(1, -1, 1) + beta.double().view(1, -1, 1)


def ref_depthwise(x, w, b, d):
    """x (Bs, C, F), w (C, P), b (C,) -> causal dilated depthwise convolution, (P - 1) d zeros on the left (tdcn.py:125-132)"""
    C, P = w.shape
    xp = torch.nn.functional.pad(x.double(), ((P - 1) * d, 0))
    return torch.nn.functional.conv1d(xp, w.double().view(C, 1, P), b.double(), dilation=d, groups=C)


def ref_decoder(lat, D, S):
    """lat (Bs, n_src, N, F), D (N, L) -> overlap-add of D^T lat, (Bs, n_src, S (F - 1) + L) (filterbank.py:236-251)"""
    Bs, ns, N, F = lat.shape
    L = D.shape[1]
    fr = torch.einsum("bsnf,nl->bslf", lat.double(), D.double())
    y = torch.nn.functional.fold(fr.reshape(Bs * ns, L, F), (1, S * (F - 1) + L), (1, L), stride=(1, S))
    return y.reshape(Bs, ns, -1)


def cols(t, Bs, n, ldt):
    """(Bs, C, n) -> stream-major (C, ldt) columns, zeros beyond Bs n"""
    C = t.shape[1]
    out = torch.zeros(C, ldt, dtype=t.dtype)
    out[:, :Bs * n] = t.permute(1, 0, 2).reshape(C, Bs * n)
    return out


def uncols(m, Bs, n):
    """(C, ldt) stream-major columns -> (Bs, C, n)"""
    C = m.shape[0]
    return m[:, :Bs * n].reshape(C, Bs, n).permute(1, 0, 2)


# ------------------------------------------------------------------------------------------------------ kernel cases
def case_encoder(Bs, N, L, S, plan, relu):
    """chunks of `plan` frames one after another: w of every chunk and the carry against the encoder over the whole pre-rolled signal"""
    keep = L - S
    total = sum(plan)
    x = rnd(Bs, total * S)
    E = rnd(N, L, scale=0.3)
    ref = ref_encoder(torch.cat([torch.zeros(Bs, keep), x], 1), E, S, relu)        # (Bs, N, total)
    Ed = to_device(E)
    carry, carry_next = to_device(torch.zeros(Bs, keep)), to_device(torch.full((Bs, keep), float("nan")))
    frames = to_device(torch.zeros(Bs, dtype=torch.int64))
    f0 = 0
    for n in plan:
        ldt = _round_up(Bs * n, 128)
        w = to_device(torch.full((N, ldt), float("nan")))
        chunk = to_device(x[:, f0 * S:(f0 + n) * S].contiguous())
        HIP.online_encoder_fwd(chunk, Ed, carry, carry_next, w, Bs, N, L, S, n, ldt, relu)
        HIP.online_advance(frames, carry, carry_next, keep, None, None, 0, Bs, n)
        device_sync()
        wc = w.cpu()
        assert torch.equal(wc[:, Bs * n:], torch.zeros(N, ldt - Bs * n)), "encoder: pad columns not zero"
        close(uncols(wc, Bs, n), ref[..., f0:f0 + n], 2e-5, "encoder w, chunk at frame {}".format(f0))
        f0 += n
    if keep:
        close(carry.cpu(), torch.cat([torch.zeros(Bs, keep), x], 1)[:, -keep:], 0, "encoder carry")
    assert torch.equal(frames.cpu(), torch.full((Bs,), total, dtype=torch.int64))


def case_cln(Bs, C, plan, act):
    """[PReLU ->] cLN over chunks of `plan` frames against the cumulative norm over the whole sequence: the fp64 running sums (one norm's slot
    inside a buffer of three) and the frame counters carry it from chunk to chunk"""
    total = sum(plan)
    x = rnd(Bs, C, total, scale=1.5) + 0.3
    gamma, beta = rnd(C) * 0.2 + 1.0, rnd(C) * 0.1
    alpha = torch.tensor([0.2]) if act else None
    u = torch.where(x > 0, x, 0.2 * x) if act else x
    ref = ref_cln(u.double(), gamma, beta, 1e-8)
    nn = 3                                                       # the norm under test sits at slot 1 of 3: the stride is honoured
    sums = torch.zeros(Bs, 2 * nn, dtype=torch.float64)
    sums[:, 4:] = 123.0
    sums_d, frames = to_device(sums), to_device(torch.zeros(Bs, dtype=torch.int64))
    g_d, b_d, a_d = to_device(gamma), to_device(beta), (to_device(alpha) if act else None)
    f0 = 0
    for n in plan:
        ldt = _round_up(Bs * n, 128)
        xd = to_device(cols(x[..., f0:f0 + n], Bs, n, ldt))
        y = to_device(torch.full((C, ldt), float("nan")))
        HIP.online_cln_fwd(xd, a_d, g_d, b_d, y, sums_d.view(-1)[2:], 2 * nn, frames, Bs, C, n, ldt, 1e-8)
        HIP.online_advance(frames, None, None, 0, None, None, 0, Bs, n)
        device_sync()
        yc = y.cpu()
        assert torch.equal(yc[:, Bs * n:], torch.zeros(C, ldt - Bs * n)), "cln: pad columns not zero"
        close(uncols(yc, Bs, n), ref[..., f0:f0 + n], 2e-5, "cln y, chunk at frame {}".format(f0))
        f0 += n
    s = sums_d.cpu()
    close(s[:, 2], u.double().sum((1, 2)), 1e-6, "cln running sum")
    close(s[:, 3], (u.double() ** 2).sum((1, 2)), 1e-6, "cln running sum of squares")
    assert torch.equal(s[:, :2], torch.zeros(Bs, 2)) and torch.equal(s[:, 4:], torch.full((Bs, 2), 123.0, dtype=torch.float64))


def case_depthwise(Bs, C, plan, P, d):
    """causal dilated taps over chunks of `plan` frames against the convolution of the whole sequence; the ring of every layer sits inside one
    per-stream buffer (offset, stride) like OnlineSeparator keeps it"""
    total = sum(plan)
    D = (P - 1) * d
    x = rnd(Bs, C, total)
    w, b = rnd(C, P, scale=0.5), rnd(C, scale=0.1)
    ref = ref_depthwise(x, w, b, d)
    off, stride = 5, C * D + 9
    rings = to_device(torch.zeros(Bs, stride))
    wd, bd = to_device(w), to_device(b)
    f0 = 0
    for n in plan:
        ldt = _round_up(Bs * n, 128)
        xd = to_device(cols(x[..., f0:f0 + n], Bs, n, ldt))
        y = to_device(torch.full((C, ldt), float("nan")))
        HIP.online_depthwise_fwd(xd, wd, bd, rings.view(-1)[off:], stride, y, Bs, C, n, ldt, P, d)
        device_sync()
        yc = y.cpu()
        assert torch.equal(yc[:, Bs * n:], torch.zeros(C, ldt - Bs * n)), "depthwise: pad columns not zero"
        close(uncols(yc, Bs, n), ref[..., f0:f0 + n], 2e-5, "depthwise y, chunk at frame {}".format(f0))
        f0 += n
    r = rings.cpu()
    hist = torch.nn.functional.pad(x, (D, 0))[..., -D:]                                 # the last D frames, zeros before the first
    close(r[:, off:off + C * D].reshape(Bs, C, D), hist, 0, "depthwise ring")
    assert torch.equal(r[:, :off], torch.zeros(Bs, off)) and torch.equal(r[:, off + C * D:], torch.zeros(Bs, stride - off - C * D))


def case_decoder(Bs, n_src, N, L, S, plan):
    """mask * w, synthesis and overlap-add over chunks of `plan` frames against the transposed convolution of the whole sequence: n S final
    samples per chunk, the tail carries the rest"""
    keep = L - S
    total = sum(plan)
    w, m = rnd(Bs, N, total), torch.rand(Bs, n_src, N, total, generator=G).float()
    D = rnd(N, L, scale=0.3)
    ref = ref_decoder(w.unsqueeze(1) * m, D, S)                                         # (Bs, n_src, S (total - 1) + L)
    Dd = to_device(D)
    tail, tail_next = to_device(torch.zeros(Bs, n_src, keep)), to_device(torch.full((Bs, n_src, keep), float("nan")))
    frames = to_device(torch.zeros(Bs, dtype=torch.int64))
    f0, got = 0, []
    for n in plan:
        ldt = _round_up(Bs * n, 128)
        wd = to_device(cols(w[..., f0:f0 + n], Bs, n, ldt))
        md = to_device(torch.cat([cols(m[:, s, :, f0:f0 + n], Bs, n, ldt) for s in range(n_src)], 0))
        out = to_device(torch.full((Bs, n_src, n * S), float("nan")))
        HIP.online_decoder_fwd(wd, md, Dd, tail, tail_next, out, Bs, n_src, N, L, S, n, ldt)
        HIP.online_advance(frames, None, None, 0, tail, tail_next, n_src * keep, Bs, n)
        device_sync()
        got.append(out.cpu())
        f0 += n
    got.append(tail.cpu())
    close(torch.cat(got, -1), ref, 2e-5, "decoder output")


def case_reset(Bs, keep, n_src):
    """sep_online_reset zeroes the selected streams' slices of every state buffer and nothing else"""
    frames = to_device(torch.arange(1, Bs + 1, dtype=torch.int64))
    carry, sums, rings, tail = (to_device(rnd(Bs, keep) + 5), to_device(torch.randn(Bs, 6, generator=G, dtype=torch.float64) + 5),
                                to_device(rnd(Bs, 1000) + 5), to_device(rnd(Bs, n_src * keep) + 5))
    before = [t.cpu().clone() for t in (frames, carry, sums, rings, tail)]
    sel = torch.zeros(Bs, dtype=torch.uint8)
    sel[::2] = 1
    HIP.online_reset(to_device(sel), Bs, frames, carry, keep, sums, 6, rings, 1000, tail, n_src * keep)
    device_sync()
    for t, b in zip((frames, carry, sums, rings, tail), before):
        tc = t.cpu()
        assert torch.equal(tc[sel == 1], torch.zeros_like(b[sel == 1]))
        assert torch.equal(tc[sel == 0], b[sel == 0])


CASES = [
    ("case_encoder", [(1, 16, 16, 4, [1, 1, 1, 2, 1], 0), (3, 32, 20, 10, [7, 1, 12], 1), (257, 16, 16, 8, [1, 2], 1), (2, 16, 16, 16, [3, 1], 0)]),
    ("case_cln", [(1, 16, [1] * 5 + [40, 3], True), (3, 48, [7, 1, 33], False), (257, 16, [1, 2], True), (2, 32, [257, 70], True)]),
    ("case_depthwise", [(1, 16, [1] * 6 + [300], 3, 128), (3, 32, [5, 1, 9, 30], 5, 4), (257, 16, [3, 1], 3, 2), (2, 16, [1, 2, 1], 2, 1)]),
    ("case_decoder", [(1, 2, 16, 16, 4, [1, 1, 1, 3]), (3, 3, 32, 20, 10, [7, 1, 12]), (257, 2, 16, 16, 8, [1, 2]), (2, 2, 16, 8, 8, [2, 1])]),
    ("case_reset", [(5, 8, 2), (1, 0, 3)]),
]


@pytest.mark.parametrize("name,params", CASES, ids=[c[0][5:] for c in CASES])
def test_online_kernels_against_the_restatement(name, params):
    for p in params:
        globals()[name](*p)


# ------------------------------------------------------------------------------------------------------ whole model on the device
def _fixture_model(name, device="cuda"):
    from oracle.make_golden import CONFIGS
    from models.conv_tasnet import ConvTasNet
    g = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_{}.npz".format(name)))
    model = ConvTasNet(**CONFIGS[name])
    model.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")})
    return model.to(device), CONFIGS[name]


def stream_through(sep, x, plan):
    """x (Bs, 1, T) through sep in chunks of plan[i % len(plan)] hops, then flush -> (Bs, n_src, T + L - S)"""
    S, T = sep.S, x.shape[-1]
    outs, t, i = [], 0, 0
    while t < T:
        k = min(plan[i % len(plan)] * S, T - t)
        outs.append(sep(x[..., t:t + k].contiguous()))
        t, i = t + k, i + 1
    outs.append(sep.flush())
    return torch.cat(outs, -1)


@pytest.mark.parametrize("arith", ["f16x3", "bf16x6", "f32"])
@pytest.mark.parametrize("name", ["causal16", "causal16_p5"])
def test_fixture_streamed_on_the_device_matches_the_reference(name, arith):
    """the unmodified reference's output on the pre-rolled input (tests/golden/convtasnet_causal_online.npz), streamed 7 hops at a time (recorded
    replay) and one hop at a time: within 1e-3 of its maximum in every arithmetic of the products"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_causal_online.npz"))
    prev = sepkernels.set_gemm_arith(arith)
    try:
        model, cfg = _fixture_model(name)
        x = torch.from_numpy(g[name + "/input"])[..., cfg["kernel_size"] - cfg["stride"]:].cuda()
        ref = torch.from_numpy(g[name + "/output_f64"])
        for plan in ([7], [1]):
            sep = model.online_separator(num_streams=x.shape[0], chunk_size=plan[0] * cfg["stride"])
            est = stream_through(sep, x, plan)
            close(est, ref, 1e-3, "{} {} plan {}".format(name, arith, plan))
    finally:
        sepkernels.set_gemm_arith(prev)


PAPER = dict(n_basis=512, kernel_size=16, stride=8, enc_basis="trainable", dec_basis="trainable", enc_nonlinear=None, sep_hidden_channels=512,
             sep_bottleneck_channels=128, sep_skip_channels=128, sep_kernel_size=3, sep_num_blocks=3, sep_num_layers=8, dilated=True,
             separable=True, causal=True, sep_nonlinear="prelu", sep_norm=True, mask_nonlinear="sigmoid", n_sources=2)


def test_paper_size_causal_model_streams_like_the_offline_staged_forward():
    """N512 L16 S8 H512 B128 Sc128 P3 X8 R3, 64 streams x 2 s at 8 kHz in 80-sample (10 ms) chunks, recorded: within 1e-4 of the offline staged
    forward on the same pre-rolled inputs (same product kernels and weight bound on the same columns; cLN summation order and where the sigmoid
    is applied differ)"""
    from models.conv_tasnet import ConvTasNet
    torch.manual_seed(0)
    model = ConvTasNet(**PAPER).cuda()
    assert model.staged and not model.fused
    Bs, T, L, S = 64, 16000, 16, 8
    x = 0.1 * torch.randn(Bs, 1, T, generator=torch.Generator().manual_seed(3)).cuda()
    with torch.no_grad():
        ref = model(torch.nn.functional.pad(x, (L - S, 0)))
    sep = model.online_separator(num_streams=Bs, chunk_size=80)
    est = stream_through(sep, x, [10])
    assert sep.launches_per_chunk() is not None and est.shape == ref.shape
    close(est, ref.cpu(), 1e-4, "paper-size online vs offline staged")


def test_recorded_replay_equals_eager_launches_bitwise_on_the_device():
    model, cfg = _fixture_model("causal16_p5")
    x = 0.1 * torch.randn(4, 1, 50 * 3 * cfg["stride"], generator=torch.Generator().manual_seed(9)).cuda()
    a = stream_through(model.online_separator(num_streams=4, chunk_size=3 * cfg["stride"]), x, [3])
    b = stream_through(model.online_separator(num_streams=4, chunk_size=3 * cfg["stride"], record=False), x, [3])
    assert torch.equal(a, b)
