"""CPU: the recorded causal Conv-TasNet training step (sepkernels/causal.py, sepkernels.train.FusedTrainStep for `staged` models) and the
folded first norm of the causal layers (csrc/causal.hip).

(1) the explicit driver causal.forward / causal.backward on the fp64 emulator of the C ABI against the unmodified reference's fixtures
    (tests/golden/convtasnet_causal16*.npz), with and without the folded calls (FoldEmu below adds them to tests/emulator.EmuBackend);
(2) the kernel SOURCE on the host (tools/hostsim.py): the kernel cases of tests/test_causal_recorded_gpu.py;
(3) on the host simulation: one recording + two replays == the driver run live each step, bit for bit; both train like three eager
    autograd steps; PIT and SinkPIT;
(4) refusals and invalidation of a recording."""
import os
import sys

import numpy as np
import pytest
import torch

import sepkernels
from emulator import EmuBackend, _prelu
from oracle.make_golden import CONFIGS, STAGED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                          # noqa: E402
import test_causal_recorded_gpu as CG   # noqa: E402

needs_clang = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++ (ext_vector_type)")


class FoldEmu(EmuBackend):
    """EmuBackend plus the three folded calls (include/sepkernels.h, 'first norm folded into its depthwise convolution') in torch arithmetic
    of the buffers' own dtype, written from their contract"""

    def cln_stats(self, x, mean, rstd, ws, B, C, T, ldt, eps, alpha=None):
        EmuBackend.cln_fwd(self, x, torch.ones(C, dtype=x.dtype), torch.zeros(C, dtype=x.dtype), torch.empty(B, C, ldt, dtype=x.dtype), mean, rstd, ws, B, C, T,
                           ldt, eps, alpha=alpha)

    @staticmethod
    def _v1(x, alpha, gamma, beta, mean, rstd, B, C, T, ldt):
        u = _prelu(x, alpha) if alpha is not None else x
        v = torch.zeros(B, C, ldt, dtype=x.dtype)
        v[:, :, :T] = ((u.reshape(B, C, ldt) - mean.reshape(B, 1, ldt)) * rstd.reshape(B, 1, ldt) * gamma.view(1, C, 1) + beta.view(1, C, 1))[:, :, :T]
        return v

    def depthwise_cln_fwd(self, x, alpha, gamma, beta, mean, rstd, w, bias, y, B, C, T, ldt, Kw, pad, dil):
        v1 = self._v1(x, alpha, gamma, beta, mean, rstd, B, C, T, ldt)
        out = self._depthwise(v1, w, bias, C, ldt, ldt, Kw, 1, pad, dil).clone()
        out[:, :, T:] = 0
        y.reshape(B, C, ldt).copy_(out)

    def depthwise_cln_bwd_weight(self, dy, x, alpha, gamma, beta, mean, rstd, partial, B, C, T, ldt, Kw, pad, dil):
        v1 = self._v1(x, alpha, gamma, beta, mean, rstd, B, C, T, ldt)
        g = dy.reshape(B, C, ldt).clone()
        g[:, :, T:] = 0
        EmuBackend.depthwise_bwd_weight(self, g, v1, partial, B, C, ldt, ldt, Kw, 1, pad, dil)


def _load(golden_dir, name):
    from models.conv_tasnet import ConvTasNet
    g = np.load(os.path.join(golden_dir, "convtasnet_{}.npz".format(name)))
    model = ConvTasNet(**CONFIGS[name])
    model.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")})
    return g, model


# ---------------------------------------------------------------------------------------------- (1) the driver against the reference
@pytest.mark.parametrize("folded", [True, False])
@pytest.mark.parametrize("name", STAGED)
def test_driver_matches_the_reference(golden_dir, name, folded):
    """causal.forward + PIT(NegSI-SDR) + causal.backward in fp64: output and loss within 1e-9 relative, the permutation equal, every
    gradient within 2e-6 of its own scale -- the bars of tests/test_composed_cpu.py::test_staged_causal_path_matches_the_reference."""
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    from sepkernels import causal
    calls = []
    K = FoldEmu() if folded else EmuBackend()
    for fn in ("cln_fwd", "depthwise_fwd", "pw_gemm") + (("cln_stats", "depthwise_cln_fwd", "depthwise_cln_bwd_weight") if folded else ()):
        setattr(K, fn, (lambda o, n: (lambda *a, **k: (calls.append(n), o(*a, **k))[1]))(getattr(K, fn), fn))
    old = sepkernels._set_backend_for_tests(K)
    try:
        g, model = _load(golden_dir, name)
        model = model.double()
        assert model.staged and not model.fused
        mixture, sources = torch.from_numpy(g["mixture"]).double(), torch.from_numpy(g["sources"]).double()
        P = {k: v.detach() for k, v in model.named_parameters()}
        cfg = model.get_config()
        with torch.no_grad():
            est, latent, sv = causal.forward(cfg, P, mixture.contiguous(), True, True)
        nl = cfg["sep_num_blocks"] * cfg["sep_num_layers"]
        if folded:
            assert calls.count("cln_stats") == nl and calls.count("depthwise_cln_fwd") == nl and calls.count("depthwise_fwd") == 0
            assert calls.count("cln_fwd") == nl + 1                # only the second norms (and the separator's first) are written out
        else:
            assert calls.count("cln_fwd") == 2 * nl + 1 and calls.count("depthwise_fwd") == nl
        ref = torch.from_numpy(g["output_f64"])
        assert (est.view(ref.shape) - ref).abs().max() <= 1e-9 * ref.abs().max()
        F_ = sv.geo.F
        assert abs(latent[..., :F_].sum().item() - float(g["latent_f64_sum"])) <= 1e-8 * float(g["latent_f64_abs_sum"])
        leaf = est.detach().view(ref.shape).clone().requires_grad_(True)
        loss, pattern = PIT1d(NegSISDR(), n_sources=cfg["n_sources"])(leaf, sources)
        assert abs(loss.item() - float(g["loss_f64"])) <= 1e-9 * abs(float(g["loss_f64"]))
        assert np.array_equal(pattern.numpy(), g["pattern"])
        loss.backward()
        flat = torch.full((sum(v.numel() for v in P.values()),), float("nan"), dtype=torch.float64)      # gradients land in views of one buffer
        G, off = {}, 0
        for k, v in P.items():
            G[k] = flat[off:off + v.numel()].view(v.shape)
            off += v.numel()
        ready = []
        with torch.no_grad():
            causal.backward(cfg, P, sv, leaf.grad.view(est.shape).contiguous(), G, ready.append)
        assert ready == list(range(cfg["sep_num_blocks"] - 1, 0, -1))
        if folded:
            assert calls.count("depthwise_cln_bwd_weight") == nl
        assert torch.isfinite(flat).all()
        for k in P:
            gr = torch.from_numpy(g["grad/" + k]).double()
            assert (G[k] - gr).abs().max() <= 2e-6 * max(gr.abs().max().item(), 1e-6), k
    finally:
        sepkernels._set_backend_for_tests(old)


# ---------------------------------------------------------------------------------------------- (2) the kernel sources on the host
@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim.build(str(tmp_path_factory.mktemp("hostsim_causal")))


@pytest.fixture()
def on_host(sim_library):
    saved = (CG.HIP, CG.to_device, CG.device_sync, CG.device_name)
    with hostsim.HostSimBackend(sim_library) as K:
        CG.HIP, CG.to_device, CG.device_sync, CG.device_name = K, (lambda t: t.clone()), (lambda: None), (lambda: "cpu")
        try:
            yield K
        finally:
            CG.HIP, CG.to_device, CG.device_sync, CG.device_name = saved


@needs_clang
@pytest.mark.parametrize("name,args", [(n, a) for n, params in CG.CASES for a in params])
def test_kernel_sources_on_the_host(on_host, name, args):
    getattr(CG, name)(*args)


@needs_clang
def test_the_folded_check_is_not_vacuous(on_host):
    """the same case fails when the device side computes something else (here: a gain 1 % off)"""
    class Skewed:
        def __getattr__(self, name):
            return getattr(on_host, name)

        def depthwise_cln_fwd(self, x, alpha, gamma, *rest):
            return on_host.depthwise_cln_fwd(x, alpha, gamma * 1.01, *rest)
    CG.HIP = Skewed()
    with pytest.raises(AssertionError):
        CG.case_depthwise_cln(2, 16, 203, 256, 3, 2, True, 0.25)


# ---------------------------------------------------------------------------------------------- (3) replay == live driver ~ eager steps
class _Named:
    name = "hostsim"

    def __init__(self, K):
        self._K = K

    def __getattr__(self, attr):
        return getattr(self._K, attr)


def _criterion(kind, n):
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d, SinkPIT
    return PIT1d(NegSISDR(), n_sources=n) if kind == "pit" else SinkPIT(NegSISDR(), n_sources=n, coldness=1.0, iteration=7)


@needs_clang
@pytest.mark.parametrize("kind", ["pit", "sinkpit"])
def test_recorded_causal_step_replays_and_trains_like_the_eager_step(golden_dir, on_host, kind):
    """A causal16 model, three batches, a learning-rate change before the last.  (a) one record() and two replays (ONE sep_run_sequence call
    each); (b) the driver run live every step (a fresh record() per step on one step object: moments and step count carry over); (c) three
    eager autograd steps.  (a) == (b) to the last bit, losses and parameters: same entry points, same arguments, same order.  (a) against
    (c): every loss within 1e-5 relative (DESIGN.md section 4.5's bar for recorded against eager) -- the two issue the same kernels in the
    same arithmetic, but the step's scalars (Adam's bias corrections, the PIT mean) are formed on the device in one and on the host in the
    other; parameters are not compared with (c) (after Adam's normalisation an ulp in a near-zero gradient is worth 2 lr)."""
    from sepkernels.train import FusedTrainStep
    n_src = CONFIGS["causal16"]["n_sources"]
    gen = torch.Generator().manual_seed(5)
    batches = [0.1 * torch.randn(2, n_src, 1203, generator=gen) for _ in range(3)]
    old = sepkernels._set_backend_for_tests(_Named(on_host))
    runs = {}
    try:
        for mode in ("replay", "live", "eager"):
            _, model = _load(golden_dir, "causal16")
            step = FusedTrainStep(model, _criterion(kind, n_src), lr=1e-3, max_norm=5.0)
            assert step.recordable() is None
            losses = []
            for i, src in enumerate(batches):
                mix = src.sum(1, keepdim=True).contiguous()
                if i == 2:
                    step.lr = 5e-4
                if mode == "live" or (mode == "replay" and i == 0):
                    losses.append(float(step.record(mix, src)))
                    if mode == "replay":
                        names = step._seq.names()
                        assert names[0] == "sep_absmax" and names[-1] == "sep_adam_step_dev"
                        for want in ("sep_cln_fwd", "sep_cln_bwd", "sep_cln_stats", "sep_depthwise_cln_fwd", "sep_depthwise_cln_bwd_weight", "sep_pit_finish",
                                     "sep_pw_gemm", "sep_pw_wgrad", "sep_memset"):
                            assert want in names, want
                        assert "sep_depthwise_fwd" not in names and "sep_depthwise_bwd_weight" not in names
                        assert ("sep_sinkhorn_bwd" in names) == (kind == "sinkpit") and ("sep_pit_search" in names) == (kind == "pit")
                else:
                    before = step._seq
                    losses.append(float(step(mix, src)))
                    assert step._seq is before and (before is not None) == (mode == "replay")
            assert step.step_count == 3 and (mode == "eager" or int(step._step_dev.item()) == 3)
            runs[mode] = (losses, model.flat_parameters().detach().clone(), step.last_pattern if mode != "eager" else None)
    finally:
        sepkernels._set_backend_for_tests(old)
    (la, pa, pattern), (lb, pb, _), (lc, _, _) = runs["replay"], runs["live"], runs["eager"]
    print(kind, "replay", la, "live", lb, "eager", lc)
    assert la == lb and torch.equal(pa, pb)
    assert la[0] != la[-1]
    for a, c in zip(la, lc):
        assert abs(a - c) <= 1e-5 * abs(c), (la, lc)
    assert pattern.shape == (2, n_src) and sorted(pattern[0].tolist()) == list(range(n_src))


# ---------------------------------------------------------------------------------------------- (4) refusals and invalidation
def test_refusals_name_the_path_and_keep_their_messages(golden_dir):
    from models.conv_tasnet import ConvTasNet
    from criterion.sdr import NegSISDR, ClippedNegSISDR
    from criterion.pit import PIT1d
    from sepkernels.train import FusedTrainStep
    old = sepkernels._set_backend_for_tests(EmuBackend())
    try:
        odd = ConvTasNet(**dict(CONFIGS["causal16"], sep_hidden_channels=40))          # causal, widths off the kernels' multiples of 16
        assert not odd.fused and not odd.staged
        why = FusedTrainStep(odd, PIT1d(NegSISDR(), n_sources=3)).recordable()
        assert why is not None and "composed" in why
        with pytest.raises(RuntimeError, match="composed"):
            FusedTrainStep(odd, PIT1d(NegSISDR(), n_sources=3)).record(torch.zeros(1, 1, 800), torch.zeros(1, 3, 800))
        _, model = _load(golden_dir, "causal16")
        assert FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=3)).recordable() is None
        assert "over SI-SDR" in FusedTrainStep(model, PIT1d(ClippedNegSISDR(min=-30), n_sources=3)).recordable()
        next(model.parameters()).requires_grad_(False)
        assert "frozen parameters" in FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=3)).recordable()
    finally:
        sepkernels._set_backend_for_tests(old)


def test_a_staged_model_with_a_gradient_exchange_steps_eagerly(golden_dir, tmp_path):
    """ranks > 1 (here: a one-rank gloo group with exercise_collectives, which takes the same exchange path): recordable() names the reason"""
    import torch.distributed as dist
    from criterion.sdr import NegSISDR
    from criterion.pit import PIT1d
    from sepkernels.train import FusedTrainStep
    old = sepkernels._set_backend_for_tests(EmuBackend())
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "pg"), rank=0, world_size=1)
    try:
        _, model = _load(golden_dir, "causal16")
        step = FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=3), distributed=True, exercise_collectives=True)
        assert step.comm and "single rank" in step.recordable()
        with pytest.raises(RuntimeError, match="single rank"):
            step.record(torch.zeros(1, 1, 800), torch.zeros(1, 3, 800))
        assert FusedTrainStep(model, PIT1d(NegSISDR(), n_sources=3), distributed=False).recordable() is None
    finally:
        dist.destroy_process_group()
        sepkernels._set_backend_for_tests(old)


@needs_clang
def test_a_recording_is_dropped_or_bypassed_when_it_no_longer_fits(golden_dir, on_host):
    """model.to() / .float() re-homes the parameters: the next call steps eagerly and the list is gone.  A batch of another shape steps
    eagerly, keeps the recording and keeps the device-side step count in line with step_count."""
    from sepkernels.train import FusedTrainStep
    gen = torch.Generator().manual_seed(9)
    src = 0.1 * torch.randn(1, 3, 803, generator=gen)
    other = 0.1 * torch.randn(1, 3, 1003, generator=gen)
    old = sepkernels._set_backend_for_tests(_Named(on_host))
    try:
        _, model = _load(golden_dir, "causal16")
        step = FusedTrainStep(model, _criterion("pit", 3), lr=1e-3, max_norm=5.0)
        step.record(src.sum(1, keepdim=True).contiguous(), src)
        seq = step._seq
        assert seq is not None
        step(other.sum(1, keepdim=True).contiguous(), other)                      # another shape: eager, the recording stays
        assert step._seq is seq and step.step_count == 2 and int(step._step_dev.item()) == 2
        step(src.sum(1, keepdim=True).contiguous(), src)                          # the recorded shape again: a replay
        assert step._seq is seq and step.step_count == 3 and int(step._step_dev.item()) == 3
        model.float()                                                             # nn.Module._apply: a new flat buffer
        step(src.sum(1, keepdim=True).contiguous(), src)
        assert step._seq is None and step.step_count == 4
    finally:
        sepkernels._set_backend_for_tests(old)
