"""CPU: the causal Conv-TasNet WITHOUT separable convolutions (ConvTasNet(causal=True, separable=False), reference src/models/tdcn.py:100-147)
on the kernel path: sep_unfold_dilated / sep_fold_dilated, sep_online_unfold_fwd (+ _sel, _rag), the staged forward / backward, the explicit
driver of the recorded step, the online separator.

(1) fp64 emulator (DenseEmu below adds the five new calls, written from their contracts in include/sepkernels.h, to the emulator of
    tests/test_online_ragged_cpu.py): the model's autograd path and causal.forward / causal.backward against the unmodified reference's
    fixtures tests/golden/convtasnet_causal16_dense*.npz, with the calls per layer counted; the online separator against the offline forward
    on uniform, subset and ragged clocks.
(2) the kernel SOURCE on the host (tools/hostsim.py): the kernel cases of tests/test_dense_tcn_gpu.py; recorded == live; the online
    schedule recorded == eager.
(3) the live reference (skipped where its tree is absent): this tree's composition and the emulator path against the imported reference
    model in fp64, and the fixtures against it.
(4) the refusals that stay."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sepkernels
from dense_tcn_configs import CONFIGS, NAMES
from test_online_ragged_cpu import RagEmu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                          # noqa: E402
import test_dense_tcn_gpu as DG         # noqa: E402

needs_clang = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++ (ext_vector_type)")
REF_SRC = "/root/reference/src"


class DenseEmu(RagEmu):
    """the emulator of the online tests plus the dilated unfold, its adjoint and the online unfold in its three forms, in torch arithmetic of
    the buffers' own dtype, written from their contracts (include/sepkernels.h)"""

    def unfold_dilated(self, x, cols, B, C, T, ldt, P, dil, pad):
        xv, cv = x.reshape(B, C, ldt), cols.reshape(B, C, P, ldt)
        cv.zero_()
        for p in range(P):
            for t in range(T):
                i = t + p * dil - pad
                if 0 <= i < T:
                    cv[:, :, p, t] = xv[:, :, i]

    def fold_dilated(self, dcols, dx, B, C, T, ldt, P, dil, pad):
        dv, xv = dcols.reshape(B, C, P, ldt), dx.reshape(B, C, ldt)
        xv.zero_()
        for p in range(P):                               # ascending p
            for u in range(T):
                i = u - p * dil + pad
                if 0 <= i < T:
                    xv[:, :, u] += dv[:, :, p, i]

    def online_unfold_fwd(self, x, ring, ring_stride, cols, num_streams, C, n, ldt, P, dilation):
        Bs, D = num_streams, (P - 1) * dilation
        hist = ring.as_strided((Bs, C, D), (ring_stride, D, 1))
        ext = torch.cat([hist, x[:, :Bs * n].reshape(C, Bs, n).permute(1, 0, 2)], 2)              # (Bs, C, D + n)
        out = torch.stack([ext[..., p * dilation:p * dilation + n] for p in range(P)], 2)            # (Bs, C, P, n): ext[f + p d]
        cols.zero_()
        cols[:, :Bs * n] = out.permute(1, 2, 0, 3).reshape(C * P, Bs * n)
        hist.copy_(ext[..., n:].clone())

    def online_unfold_fwd_sel(self, x, ring, ring_stride, cols, num_streams, C, n, ldt, P, dilation, slots):
        idx, CD = slots[:num_streams].tolist(), C * (P - 1) * dilation
        own = torch.stack([ring[s * ring_stride:s * ring_stride + CD] for s in idx]).reshape(-1)
        self.online_unfold_fwd(x, own, CD, cols, num_streams, C, n, ldt, P, dilation)
        for j, s in enumerate(idx):
            ring[s * ring_stride:s * ring_stride + CD] = own[j * CD:(j + 1) * CD]

    def online_unfold_fwd_rag(self, x, ring, ring_stride, cols, num_streams, C, n_cap, ldt, P, dilation, slots, offs):
        CD = C * (P - 1) * dilation
        cols.zero_()
        for j, s, o, n in self._blocks(num_streams, slots, offs):
            own = ring[s * ring_stride:s * ring_stride + CD].clone()
            cj = torch.zeros(C * P, n, dtype=cols.dtype)
            self.online_unfold_fwd(x[:, o:o + n].contiguous(), own, CD, cj, 1, C, n, n, P, dilation)
            cols[:, o:o + n] = cj
            ring[s * ring_stride:s * ring_stride + CD] = own


COUNTED = ("cln_fwd", "cln_bwd", "unfold_dilated", "fold_dilated", "pw_gemm", "depthwise_fwd", "depthwise_bwd_input", "depthwise_bwd_weight")


@pytest.fixture()
def emu():
    """-> the list of (call name, m_split) the emulator served"""
    K = DenseEmu()
    calls = []
    for fn in COUNTED:
        setattr(K, fn, (lambda o, n: (lambda *a, **k: (calls.append((n, k.get("m_split", 0))), o(*a, **k))[1]))(getattr(K, fn), fn))
    old = sepkernels._set_backend_for_tests(K)
    try:
        yield calls
    finally:
        sepkernels._set_backend_for_tests(old)


def _check_calls(calls, cfg, backward):
    """per layer: one cln_fwd (plus the separator's), one unfold_dilated, no depthwise call; the joint product where the bottleneck allows it"""
    nl = cfg["sep_num_blocks"] * cfg["sep_num_layers"]
    names = [c[0] for c in calls]
    assert names.count("cln_fwd") == nl + 1 and names.count("unfold_dilated") == nl
    assert not any(n.startswith("depthwise") for n in names)
    joint = sum(1 for n, ms in calls if n == "pw_gemm" and ms)
    assert joint == (nl - 1 if cfg["sep_bottleneck_channels"] % 128 == 0 else 0)
    if backward:
        assert names.count("fold_dilated") == nl and names.count("cln_bwd") == nl + 1


def _check_grads(G, g):
    for k, v in G.items():
        gr = torch.from_numpy(g["grad/" + k]).double()
        assert (v - gr).abs().max() <= 2e-6 * max(gr.abs().max().item(), 1e-6), k


# ------------------------------------------------------------------------------------------------------ (1) fp64 emulator
@pytest.mark.parametrize("name", NAMES)
def test_staged_dense_path_matches_the_reference_in_fp64(emu, name):
    """the model's autograd path (ConvTasNet._run_staged through sepkernels.functional) on the fp64 emulator: output and loss within 1e-9
    relative, the permutation equal, every gradient within 2e-6 of its own scale (the fixture keeps the fp64 gradients as fp32) -- the bars of
    tests/test_composed_cpu.py::test_staged_causal_path_matches_the_reference"""
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    g = DG.load_fixture(name)
    model = DG.fixture_model(name, g).double()
    assert model.staged and not model.fused and model.staged_reason is None
    mixture, sources = torch.from_numpy(g["mixture"]).double(), torch.from_numpy(g["sources"]).double()
    est, latent = model.extract_latent(mixture)
    ref = torch.from_numpy(g["output_f64"])
    assert est.shape == ref.shape and (est - ref).abs().max() <= 1e-9 * ref.abs().max()
    assert abs(latent.sum().item() - float(g["latent_f64_sum"])) <= 1e-8 * float(g["latent_f64_abs_sum"])
    loss, pattern = PIT1d(NegSISDR(), n_sources=CONFIGS[name]["n_sources"])(est, sources)
    assert abs(loss.item() - float(g["loss_f64"])) <= 1e-9 * abs(float(g["loss_f64"]))
    assert np.array_equal(pattern.numpy(), g["pattern"])
    loss.backward()
    _check_calls(emu, CONFIGS[name], True)
    _check_grads({k: p.grad for k, p in model.named_parameters()}, g)
    assert sorted(model.state_dict()) == sorted(k[6:] for k in g if k.startswith("param/"))          # keys and shapes as the reference's
    assert all(tuple(v.shape) == g["param/" + k].shape for k, v in model.state_dict().items())


@pytest.mark.parametrize("name", NAMES)
def test_dense_driver_matches_the_reference_in_fp64(emu, name):
    """sepkernels.causal.forward / backward (what the recorded step is made of) on the fp64 emulator, at the same bars; gradients land in
    views of one NaN-filled buffer"""
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    from sepkernels import causal
    g = DG.load_fixture(name)
    model = DG.fixture_model(name, g).double()
    cfg = model.get_config()
    mixture, sources = torch.from_numpy(g["mixture"]).double(), torch.from_numpy(g["sources"]).double()
    P = {k: v.detach() for k, v in model.named_parameters()}
    with torch.no_grad():
        est, latent, sv = causal.forward(cfg, P, mixture.contiguous(), True, True)
    _check_calls(emu, CONFIGS[name], False)
    ref = torch.from_numpy(g["output_f64"])
    assert (est.view(ref.shape) - ref).abs().max() <= 1e-9 * ref.abs().max()
    assert abs(latent[..., :sv.geo.F].sum().item() - float(g["latent_f64_sum"])) <= 1e-8 * float(g["latent_f64_abs_sum"])
    leaf = est.detach().view(ref.shape).clone().requires_grad_(True)
    loss, pattern = PIT1d(NegSISDR(), n_sources=cfg["n_sources"])(leaf, sources)
    assert abs(loss.item() - float(g["loss_f64"])) <= 1e-9 * abs(float(g["loss_f64"]))
    assert np.array_equal(pattern.numpy(), g["pattern"])
    loss.backward()
    flat = torch.full((sum(v.numel() for v in P.values()),), float("nan"), dtype=torch.float64)
    G, off = {}, 0
    for k, v in P.items():
        G[k] = flat[off:off + v.numel()].view(v.shape)
        off += v.numel()
    ready = []
    with torch.no_grad():
        causal.backward(cfg, P, sv, leaf.grad.view(est.shape).contiguous(), G, ready.append)
    assert ready == list(range(cfg["sep_num_blocks"] - 1, 0, -1))
    _check_calls(emu, CONFIGS[name], True)
    assert torch.isfinite(flat).all()
    _check_grads(G, g)


@pytest.mark.parametrize("name", NAMES)
def test_dense_model_streams_like_its_offline_forward_in_fp64(emu, name):
    """the online separator on the emulator against the offline forward on the pre-rolled input, to 1e-9 of its maximum: every stream in every
    call (chunks of 1, 7 and mixed hops), and the schedule of test_dense_tcn_gpu.run_online_schedule (plain, subset and ragged calls, a
    flush per stream)"""
    import test_online_gpu as OG
    model = DG.fixture_model(name).double()
    L, S = CONFIGS[name]["kernel_size"], CONFIGS[name]["stride"]
    x = 0.1 * torch.randn(3, 1, 40 * S, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    with torch.no_grad():
        ref = model(F.pad(x, (L - S, 0)))
    for plan in ([1], [7], [3, 1, 12, 2, 5]):
        sep = model.online_separator(num_streams=3, chunk_size=plan[0] * S)
        assert sep.dense and not sep.record and sep.n_norms == 1 + len(sep.layers)
        est = OG.stream_through(sep, x, plan)
        assert est.shape == ref.shape and ((est - ref).abs().max() / ref.abs().max()).item() <= 1e-9, plan
    sep = model.online_separator(num_streams=3, chunk_size=4 * S)
    est, kinds = DG.run_online_schedule(sep, x)
    assert {"uniform", "subset", "ragged"} <= set(kinds), kinds
    for s in range(3):
        assert est[s].shape == ref[s].shape and ((est[s] - ref[s]).abs().max() / ref[s].abs().max()).item() <= 1e-9, s
    for a in ("frames", "carry", "sums", "rings", "tail"):
        assert not getattr(sep, a).any()


# ------------------------------------------------------------------------------------------------------ (2) the kernel sources on the host
@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim.build(str(tmp_path_factory.mktemp("hostsim_dense")))


@pytest.fixture()
def on_host(sim_library):
    saved = (DG.HIP, DG.to_device, DG.device_sync, DG.device_name)
    with hostsim.HostSimBackend(sim_library) as K:
        DG.HIP, DG.to_device, DG.device_sync, DG.device_name = K, (lambda t: t.clone()), (lambda: None), (lambda: "cpu")
        try:
            yield K
        finally:
            DG.HIP, DG.to_device, DG.device_sync, DG.device_name = saved


@needs_clang
@pytest.mark.parametrize("name,args", [(n, a) for n, params in DG.CASES for a in params])
def test_dense_kernel_sources_on_the_host(on_host, name, args):
    getattr(DG, name)(*args)


@needs_clang
def test_the_unfold_check_is_not_vacuous(on_host):
    """the same case fails when the device side computes something else (here: one frame less of padding)"""
    class Skewed:
        def __getattr__(self, name):
            return getattr(on_host, name)

        def unfold_dilated(self, x, cols, B, C, T, ldt, P, dil, pad):
            return on_host.unfold_dilated(x, cols, B, C, T, ldt, P, dil, pad - 1)
    DG.HIP = Skewed()
    with pytest.raises(AssertionError):
        DG.case_unfold_fold(2, 16, 203, 256, 3, 1, 2)


class _Named:
    name = "hostsim"

    def __init__(self, K):
        self._K = K

    def __getattr__(self, attr):
        return getattr(self._K, attr)


@needs_clang
@pytest.mark.parametrize("name,T,B", [("causal16_dense", 403, 2), ("causal16_dense_joint", 323, 1)])
def test_recorded_dense_step_equals_the_live_driver_on_the_host(on_host, name, T, B):
    DG.check_recorded_equals_live(name, wrap=_Named(on_host), T=T, B=B)


@needs_clang
def test_recorded_dense_chunks_equal_eager_launches_on_the_host(on_host):
    """the online schedule (plain, subset and ragged calls) on the kernel sources: recorded chunk steps against eager launches, bit for bit,
    and both within 1e-4 of the offline staged forward on the same backend"""
    name = "causal16_dense"
    old = sepkernels._set_backend_for_tests(_Named(on_host))
    try:
        model = DG.fixture_model(name)
        L, S = CONFIGS[name]["kernel_size"], CONFIGS[name]["stride"]
        x = 0.1 * torch.randn(3, 1, 24 * S, generator=torch.Generator().manual_seed(3))
        with torch.no_grad():
            ref = model(F.pad(x, (L - S, 0)))
        outs = {}
        for record in (True, False):
            sep = model.online_separator(num_streams=3, chunk_size=4 * S, record=record)
            assert sep.record == record
            outs[record], kinds = DG.run_online_schedule(sep, x)
            assert {"uniform", "subset", "ragged"} <= set(kinds)
            if record:
                assert "sep_online_unfold_fwd" in sep._seq.names() and any("sep_online_unfold_fwd_rag" in q.names() for q in sep._sub_seqs.values())
        for s in range(3):
            assert torch.equal(outs[True][s], outs[False][s])
            assert ((outs[True][s] - ref[s]).abs().max() / ref[s].abs().max()).item() <= 1e-4
    finally:
        sepkernels._set_backend_for_tests(old)


# ------------------------------------------------------------------------------------------------------ (3) the live reference
_REFERENCE_CHILD = r"""
import sys, types
import numpy as np
import torch
sys.modules.setdefault("torchaudio", types.ModuleType("torchaudio"))
sys.path.insert(0, {ref!r})
sys.path.insert(0, {tests!r})
from models.conv_tasnet import ConvTasNet
from dense_tcn_configs import CONFIGS
assert ConvTasNet.__module__ == "models.conv_tasnet" and sys.modules["models.conv_tasnet"].__file__.startswith({ref!r})
for name in CONFIGS:
    g = np.load({golden!r} + "/convtasnet_" + name + ".npz")
    model = ConvTasNet(**CONFIGS[name])
    model.load_state_dict({{k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")}})
    with torch.no_grad():
        out = model.double()(torch.from_numpy(g["mixture"]).double())
    np.save({out!r} + "/" + name + ".npy", out.numpy())
"""


@pytest.mark.skipif(not os.path.isdir(REF_SRC), reason="reference tree not present")
@pytest.mark.parametrize("name", NAMES)
def test_composition_and_emulator_path_equal_the_live_reference(tmp_path_factory, emu, name):
    """both configurations in fp64: the UNMODIFIED reference's model, imported in a process of its own, against (a) the fixture it is said to
    have written, (b) this tree's module-by-module composition and (c) the kernel path on the emulator, each within 1e-9 of its maximum"""
    out = tmp_path_factory.getbasetemp() / "dense_live_reference"
    if not (out / (name + ".npy")).exists():
        out.mkdir(exist_ok=True)
        code = _REFERENCE_CHILD.format(ref=REF_SRC, tests=os.path.join(ROOT, "tests"), golden=os.path.join(ROOT, "tests", "golden"), out=str(out))
        env = {k: v for k, v in os.environ.items() if k != "PYTHONPATH"}
        subprocess.run([sys.executable, "-c", code], check=True, env=env, cwd=str(out), timeout=600)
    live = torch.from_numpy(np.load(str(out / (name + ".npy"))))
    g = DG.load_fixture(name)
    scale = live.abs().max()
    assert (torch.from_numpy(g["output_f64"]) - live).abs().max() <= 1e-12 * scale                 # the fixture is the reference's own output
    model = DG.fixture_model(name, g).double()
    mixture = torch.from_numpy(g["mixture"]).double()
    with torch.no_grad():
        composed, _ = model._run_composed(mixture.contiguous(), False)
        staged = model(mixture)
    assert any(n == "unfold_dilated" for n, _ in emu)
    assert (composed.view(live.shape) - live).abs().max() <= 1e-9 * scale
    assert (staged - live).abs().max() <= 1e-9 * scale


# ------------------------------------------------------------------------------------------------------ (4) the refusals that stay
def test_configurations_outside_the_family_keep_their_refusals(emu):
    from models.conv_tasnet import ConvTasNet
    base = CONFIGS["causal16_dense"]
    for change, words in ((dict(causal=False), ("causal=False outside the fused family", "separable=True and dilated=True are required")),
                          (dict(dilated=False), ("separable=True and dilated=True are required",)),
                          (dict(sep_hidden_channels=40), ("sep_hidden_channels must be a multiple of 16",))):
        model = ConvTasNet(**dict(base, **change))
        assert not model.staged and not model.fused
        for w in words:
            assert w in model.staged_reason, (change, model.staged_reason)
        with pytest.raises(ValueError if change.get("causal") is False else NotImplementedError):
            model.online_separator()
        if "dilated" in change:
            continue
        with torch.no_grad():                                                       # ... and still run, as the composition
            y = model(0.1 * torch.randn(1, 1, 160, generator=torch.Generator().manual_seed(1)))
        assert y.shape == (1, 2, 160) and not any(n == "unfold_dilated" for n, _ in emu)
    model = ConvTasNet(**dict(base, dilated=False, separable=True))                 # (the separable family's refusal of dilated=False, unchanged)
    assert not model.staged and "separable=True and dilated=True are required" in model.staged_reason
    model = ConvTasNet(**dict(base, in_channels=2))                                 # multi-channel online streams: refused by the separator
    assert model.staged
    with pytest.raises(NotImplementedError, match="mono"):
        model.online_separator()
