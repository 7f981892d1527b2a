"""CPU: online (chunk-by-chunk) separation of a causal Conv-TasNet (ConvTasNet.online_separator -> sepkernels/online.py -> csrc/online.hip).

(a) fp64 parity: the separator's host orchestration on an fp64 CPU emulation of the new entry points (OnlineEmu below, a subclass of
    tests/emulator.EmuBackend), streamed through several chunk plans and flushed, against the unmodified reference's output on the pre-rolled
    input (tests/golden/convtasnet_causal_online.npz, written by tools/make_online_golden.py; parameters from convtasnet_<name>.npz).
(b) the kernel SOURCE on the host (tools/hostsim.py): the kernel cases of tests/test_online_gpu.py, and a tiny causal model streamed on the host
    simulation against the offline staged path on the same backend.
(c) behaviour: recorded replay == eager launches bit for bit, per-stream reset, long runs of one-hop chunks, the refusals."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sepkernels
from emulator import EmuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                          # noqa: E402
import test_online_gpu as OG            # noqa: E402


class OnlineEmu(EmuBackend):
    """EmuBackend plus the online entry points (include/sepkernels.h, 'online separation'), the weight bound and the memset, in torch
    arithmetic of the buffers' own dtype.  It issues nothing through the library handle, so the separator steps eagerly on it (no recording)."""

    def absmax(self, x, out, n):
        out.reshape(-1)[0] = x.reshape(-1)[:n].abs().max()

    def memset(self, t, value=0):
        t.fill_(value)

    def online_encoder_fwd(self, chunk, E, carry, carry_next, w, num_streams, N, L, S, n, ldt, relu):
        keep = L - S
        ext = torch.cat([carry, chunk], 1) if keep else chunk
        y = torch.einsum("bfl,nl->nbf", ext.unfold(1, L, S), E.reshape(N, L)).reshape(N, num_streams * n)
        w.zero_()
        w[:, :num_streams * n] = y.clamp_min(0) if relu else y
        if keep:
            carry_next.copy_(ext[:, n * S:])

    def online_cln_fwd(self, x, alpha, gamma, beta, y, sums, sums_stride, frames, num_streams, C, n, ldt, eps):
        Bs = num_streams
        u = x[:, :Bs * n].reshape(C, Bs, n)
        if alpha is not None:
            u = torch.where(u > 0, u, alpha.reshape(()) * u)
        u64 = u.double()
        idx = torch.arange(Bs) * sums_stride
        a = u64.sum(0).cumsum(1) + sums[idx].unsqueeze(1)
        q = (u64 * u64).sum(0).cumsum(1) + sums[idx + 1].unsqueeze(1)
        cnt = C * (frames.double().unsqueeze(1) + torch.arange(1, n + 1, dtype=torch.float64))
        m = a / cnt
        r = 1.0 / ((q / cnt - m * m).clamp_min(0).sqrt() + eps)
        m, r = m.to(x.dtype), r.to(x.dtype)
        y.zero_()
        y[:, :Bs * n] = ((u - m) * r * gamma.view(C, 1, 1) + beta.view(C, 1, 1)).reshape(C, Bs * n)
        sums[idx] = a[:, -1]
        sums[idx + 1] = q[:, -1]

    def online_depthwise_fwd(self, x, w, bias, ring, ring_stride, y, num_streams, C, n, ldt, P, dilation):
        Bs, D = num_streams, (P - 1) * dilation
        hist = ring.as_strided((Bs, C, D), (ring_stride, D, 1))
        ext = torch.cat([hist, x[:, :Bs * n].reshape(C, Bs, n).permute(1, 0, 2)], 2)
        out = F.conv1d(ext, w.reshape(C, 1, P), bias, dilation=dilation, groups=C)
        y.zero_()
        y[:, :Bs * n] = out.permute(1, 0, 2).reshape(C, Bs * n)
        hist.copy_(ext[..., n:].clone())

    def online_decoder_fwd(self, w, mask, D, tail, tail_next, out, num_streams, n_src, N, L, S, n, ldt):
        Bs, keep = num_streams, L - S
        lat = (w[:, :Bs * n].reshape(1, N, Bs, n) * mask[:, :Bs * n].reshape(n_src, N, Bs, n)).permute(2, 0, 1, 3)
        fr = torch.einsum("bsnf,nl->bslf", lat, D.reshape(N, L))
        yv = F.fold(fr.reshape(Bs * n_src, L, n), (1, S * (n - 1) + L), (1, L), stride=(1, S)).reshape(Bs, n_src, -1)
        if keep:
            yv[..., :keep] += tail
            tail_next.copy_(yv[..., n * S:])
        out.copy_(yv[..., :n * S])

    def online_advance(self, frames, carry, carry_next, carry_len, tail, tail_next, tail_len, num_streams, n):
        frames += n
        if carry_len:
            carry.copy_(carry_next)
        if tail_len:
            tail.copy_(tail_next)

    def online_reset(self, mask, num_streams, frames, carry, carry_len, sums, sums_len, rings, rings_len, tail, tail_len):
        sel = mask.bool()
        frames[sel] = 0
        for t in (carry, sums, rings, tail):
            if t is not None:
                t.view(num_streams, -1)[sel] = 0


@pytest.fixture()
def emu():
    old = sepkernels._set_backend_for_tests(OnlineEmu())
    try:
        yield
    finally:
        sepkernels._set_backend_for_tests(old)


def _model(name, dtype=torch.float64):
    from oracle.make_golden import CONFIGS
    from models.conv_tasnet import ConvTasNet
    g = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_{}.npz".format(name)))
    model = ConvTasNet(**CONFIGS[name])
    model.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")})
    return model.to(dtype), CONFIGS[name]


def _fixture(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_causal_online.npz"))
    return torch.from_numpy(g[name + "/input"]).double(), torch.from_numpy(g[name + "/output_f64"])


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


# ------------------------------------------------------------------------------------------------------ (a) fp64 parity with the reference
@pytest.mark.parametrize("name", ["causal16", "causal16_p5"])
def test_streamed_fixture_matches_the_reference_in_fp64(emu, name):
    """one hop at a time, 7 hops at a time, and a mixed plan (3, 1, 12, 2, 5 hops: the eager route with workspaces per size), each followed by
    flush(): the concatenation is the reference's output on the pre-rolled input to 1e-9 of its maximum"""
    model, cfg = _model(name)
    L, S = cfg["kernel_size"], cfg["stride"]
    xin, ref = _fixture(name)
    x = xin[..., L - S:]
    for plan in ([1], [7], [3, 1, 12, 2, 5]):
        sep = model.online_separator(num_streams=x.shape[0], chunk_size=plan[0] * S)
        assert sep.delay == L - S and sep.state_bytes > 0 and not sep.record
        est = OG.stream_through(sep, x, plan)
        assert est.shape == ref.shape
        assert _rel(est, ref) <= 1e-9, (plan, _rel(est, ref))


def test_three_hundred_one_hop_chunks_keep_the_bar(emu):
    """300 chunks of one hop: the int64 frame counters and the fp64 cLN sums hold up; against the offline staged forward (the path that meets
    the reference at 1e-9, tests/test_composed_cpu.py) on the same pre-rolled 300-hop input"""
    model, cfg = _model("causal16_p5")
    L, S = cfg["kernel_size"], cfg["stride"]
    xin, _ = _fixture("causal16_p5")
    x = torch.cat([xin[..., L - S:], xin[..., L - S:]], -1)[..., :300 * S]
    with torch.no_grad():
        ref = model(F.pad(x, (L - S, 0)))
    sep = model.online_separator(num_streams=x.shape[0])
    est = OG.stream_through(sep, x, [1])
    assert _rel(est, ref) <= 1e-9


def test_resetting_one_stream_leaves_the_others_untouched(emu):
    """stream 0 is reset half way and fed a new signal: it comes out as that signal's own offline result; streams 1.. are bitwise what a run
    without the reset gives"""
    model, cfg = _model("causal16")
    L, S = cfg["kernel_size"], cfg["stride"]
    g = torch.Generator().manual_seed(5)
    Bs, hops = 3, 40
    x = 0.1 * torch.randn(Bs, 1, hops * S, generator=g, dtype=torch.float64)
    fresh = 0.1 * torch.randn(1, 1, 20 * S, generator=g, dtype=torch.float64)
    plain = OG.stream_through(model.online_separator(num_streams=Bs), x, [4])
    sep = model.online_separator(num_streams=Bs)
    first = [sep(x[..., t:t + 4 * S]) for t in range(0, 20 * S, 4 * S)]
    sep.reset([0])
    y = x.clone()
    y[0, :, 20 * S:] = fresh
    second = [sep(y[..., t:t + 4 * S]) for t in range(20 * S, hops * S, 4 * S)] + [sep.flush()]
    est = torch.cat(first + second, -1)
    assert torch.equal(est[1:], plain[1:])
    with torch.no_grad():
        own = model(F.pad(fresh, (L - S, 0)))
    assert _rel(est[:1, :, 20 * S:], own) <= 1e-9
    # the same through a bool mask
    sep.reset(torch.tensor([False, True, False]))
    assert int(sep.frames[1]) == 0 and int(sep.frames[0]) == 0


def test_refusals():
    from oracle.make_golden import CONFIGS
    from models.conv_tasnet import ConvTasNet
    with pytest.raises(ValueError, match="causal"):
        ConvTasNet(**CONFIGS["tiny"]).online_separator()
    outside = ConvTasNet(**CONFIGS["causal"])                  # causal, widths not multiples of 16: not staged
    with pytest.raises(NotImplementedError) as e:
        outside.online_separator()
    assert outside.staged_reason and outside.staged_reason in str(e.value)
    stereo = ConvTasNet(**dict(CONFIGS["causal16_p5"], in_channels=2))
    with pytest.raises(NotImplementedError, match="in_channels"):
        stereo.online_separator()
    model = ConvTasNet(**CONFIGS["causal16_p5"])              # on the CPU, under the HIP backend
    with pytest.raises(RuntimeError):
        model.online_separator()


def test_chunk_lengths_that_are_not_hops_are_refused(emu):
    model, cfg = _model("causal16_p5")
    sep = model.online_separator(num_streams=2)
    with pytest.raises(ValueError):
        sep(torch.zeros(2, 1, cfg["stride"] + 1, dtype=torch.float64))
    with pytest.raises(ValueError):
        sep(torch.zeros(3, 1, cfg["stride"], dtype=torch.float64))
    with pytest.raises(ValueError):
        model.online_separator(chunk_size=cfg["stride"] * 2 + 3)


# ------------------------------------------------------------------------------------------------------ (b), (c) on the host simulation
needs_clang = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++ (ext_vector_type)")


@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim.build(str(tmp_path_factory.mktemp("hostsim_online")))


@pytest.fixture()
def on_host(sim_library):
    saved = (OG.HIP, OG.to_device, OG.device_sync)
    with hostsim.HostSimBackend(sim_library) as K:
        OG.HIP, OG.to_device, OG.device_sync = K, (lambda t: t.clone()), (lambda: None)
        try:
            yield K
        finally:
            OG.HIP, OG.to_device, OG.device_sync = saved


@needs_clang
@pytest.mark.parametrize("name,params", OG.CASES, ids=[c[0][5:] for c in OG.CASES])
def test_online_kernel_source_on_the_host(on_host, name, params):
    for p in params:
        getattr(OG, name)(*p)


TINY = dict(n_basis=16, kernel_size=8, stride=4, enc_basis="trainable", dec_basis="trainable", enc_nonlinear="relu", sep_hidden_channels=32,
            sep_bottleneck_channels=16, sep_skip_channels=16, sep_kernel_size=3, sep_num_blocks=1, sep_num_layers=2, dilated=True, separable=True,
            causal=True, sep_nonlinear="prelu", sep_norm=True, mask_nonlinear="sigmoid", n_sources=2)


class _Named:
    """the host-simulation binding under a name the model does not take for the GPU build (CPU tensors are then accepted)"""
    name = "hostsim"

    def __init__(self, K):
        self._K = K

    def __getattr__(self, attr):
        return getattr(self._K, attr)


def _tiny():
    from models.conv_tasnet import ConvTasNet
    torch.manual_seed(7)
    model = ConvTasNet(**TINY)
    assert model.staged
    return model


@needs_clang
def test_tiny_model_streams_on_the_kernel_sources_like_the_offline_staged_path(on_host):
    model = _tiny()
    x = 0.1 * torch.randn(3, 1, 24 * 4, generator=torch.Generator().manual_seed(1))
    old = sepkernels._set_backend_for_tests(_Named(on_host))
    try:
        with torch.no_grad():
            ref = model(F.pad(x, (4, 0)))
        sep = model.online_separator(num_streams=3, chunk_size=3 * 4)
        assert sep.record
        est = OG.stream_through(sep, x, [3, 3, 1, 5])
    finally:
        sepkernels._set_backend_for_tests(old)
    assert _rel(est, ref) <= 1e-5, _rel(est, ref)


@needs_clang
def test_recorded_replay_equals_eager_launches_bitwise(on_host):
    """50 chunks: the first is recorded, the other 49 are one sep_run_sequence call each, and they equal a separator that launches every chunk
    eagerly to the last bit.  (On the host simulation: recording wraps a library handle, so on the pure-Python emulator the separator steps
    eagerly and there is nothing to compare.)"""
    model = _tiny()
    x = 0.1 * torch.randn(2, 1, 50 * 2 * 4, generator=torch.Generator().manual_seed(2))
    old = sepkernels._set_backend_for_tests(_Named(on_host))
    try:
        rec = model.online_separator(num_streams=2, chunk_size=8)
        a = OG.stream_through(rec, x, [2])
        assert rec.launches_per_chunk() == len(rec._seq) > 10
        b = OG.stream_through(model.online_separator(num_streams=2, chunk_size=8, record=False), x, [2])
    finally:
        sepkernels._set_backend_for_tests(old)
    assert torch.equal(a, b)
