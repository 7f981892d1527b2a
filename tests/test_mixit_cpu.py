"""CPU: mixture invariant training -- criterion/mixit.py, csrc/mixit.hip: sep_mixit_gram / sep_mixit_search / sep_mixit_bwd, recipes.wsj0mix.MixtureOfMixtures,
`--criterion mixit` of recipes.train_conv_tasnet.

(a) the criterion-level cases of tests/test_mixit_gpu.py (its brute-force fp64 oracle) on an emulator of the three calls (MixitEmu below, written
    from their contract in include/sepkernels.h), and one training step.
(b) the kernel SOURCES on the host (tools/hostsim.py): the kernel cases of tests/test_mixit_gpu.py.
(c) the stand-alone program of tools/hostsim_mixit.py built with -fsanitize=address,undefined and run as a program.
(d) refusals, and which inputs take which route (counted on the emulator); the library's own argument checks, which need no GPU.
(e) MixtureOfMixtures on the wav tree of tests/test_recipe_cpu.py; the recipe's options.
Without the feature `import criterion.mixit` fails: every test here fails."""
import itertools
import math
import os
import subprocess
import sys

import pytest
import torch

import sepkernels
import test_mixit_gpu as TG
from criterion.mixit import MixIT, mixit
from criterion.sdr import ClippedNegSISDR, NegSDR, NegSISDR, NegThresholdedSNR, SISDR, ThresholdedSNR, thresholded_snr
from emulator import EmuBackend
from test_recipe_cpu import SR, wav_tree          # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                         # noqa: E402
import hostsim_mixit                   # noqa: E402

needs_clang = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++")


class MixitEmu(EmuBackend):
    """EmuBackend plus the MixIT calls from their contract in include/sepkernels.h, in fp64 torch on CPU tensors: the Gram matrix as one
    product, the three inner products of every assignment as contractions of it with the 0/1 assignment matrices, the gradient from the two
    coefficients the header names.  Counts its calls."""

    def __init__(self):
        super().__init__()
        self.calls = {"gram": 0, "search": 0, "bwd": 0}

    def mixit_scratch_bytes(self, B, M, N, T):
        return 8

    def mixit_gram(self, est, tgt, gram, scratch, B, M, N, T):
        self.calls["gram"] += 1
        rows = torch.cat([est.reshape(B, M, T), tgt.reshape(B, N, T)], 1).double()
        gram.copy_(rows @ rows.transpose(1, 2))

    @staticmethod
    def _mixit_terms(kind, a, tt, yy, eps, tau):
        """-> value, cT, cE of include/sepkernels.h for inner products of any common shape"""
        Kc = 10.0 / math.log(10.0)
        if kind == 0:
            c = tt + eps
            alpha = a / c
            S = alpha * alpha * tt + eps
            Nn = (alpha * alpha * tt - 2 * alpha * a + yy).clamp_min(0) + eps
            return 10 * torch.log10(S / Nn), Kc * (2 * alpha * tt / (c * S) - ((2 * alpha * tt - 2 * a) / c - 2 * alpha) / Nn), Kc * (-2.0 / Nn)
        den = (tt - 2 * a + yy).clamp_min(0) + (tau * tt if kind == 2 else 0.0) + eps
        return 10 * torch.log10((tt + eps) / den), 2 * Kc / den, -2 * Kc / den

    def mixit_search(self, gram, B, M, N, kind, maximize, use_mean, eps, tau, best_val, best_idx, per_mix):
        self.calls["search"] += 1
        assert N ** M <= sepkernels.MIXIT_MAX_CODES and M <= sepkernels.MIXIT_MAX_EST and N <= sepkernels.MIXIT_MAX_MIX
        A = TG.remix_matrix(M, N)                                                     # (K, N, M)
        a = torch.einsum("knm,bnm->bkn", A, gram[:, M:, :M])
        yy = torch.einsum("knm,bmq,knq->bkn", A, gram[:, :M, :M], A)
        tt = torch.diagonal(gram, dim1=1, dim2=2)[:, M:].unsqueeze(1)
        values = self._mixit_terms(kind, a, tt, yy, eps, tau)[0]
        score = values.mean(-1) if use_mean else values.sum(-1)
        val, idx = score.max(1) if maximize else score.min(1)
        best_val.copy_(val)
        best_idx.copy_(idx)
        per_mix.copy_(values[torch.arange(B), idx])

    def mixit_bwd(self, est, tgt, gram, best_idx, gw, d_est, B, M, N, T, kind, eps, tau):
        self.calls["bwd"] += 1
        A = TG.remix_matrix(M, N, best_idx)                                           # (B, N, M)
        a = torch.einsum("bnm,bnm->bn", A, gram[:, M:, :M])
        yy = torch.einsum("bnm,bmq,bnq->bn", A, gram[:, :M, :M], A)
        _, cT, cE = self._mixit_terms(kind, a, torch.diagonal(gram, dim1=1, dim2=2)[:, M:], yy, eps, tau)
        remix = torch.einsum("bnm,bmt->bnt", A, est.double())
        per_mixture = gw.double().view(B, 1, 1) * (cT.unsqueeze(2) * tgt.double() + cE.unsqueeze(2) * remix)
        d_est.copy_(torch.einsum("bnm,bnt->bmt", A, per_mixture))


@pytest.fixture()
def emu():
    K = MixitEmu()
    saved = (TG.HIP, TG.to_device, TG.device_sync)
    old = sepkernels._set_backend_for_tests(K)
    TG.HIP, TG.to_device, TG.device_sync = K, (lambda t: t.clone()), (lambda: None)
    try:
        yield K
    finally:
        TG.HIP, TG.to_device, TG.device_sync = saved
        sepkernels._set_backend_for_tests(old)


# ------------------------------------------------------------------------------------------------------ (a) the criterion on the emulator
@pytest.mark.parametrize("kind", TG.KINDS)
@pytest.mark.parametrize("index", range(len(TG.SHAPES)), ids=TG.SHAPE_IDS)
def test_criterion_against_the_oracle(emu, index, kind):
    TG.case_criterion(index, kind)
    assert emu.calls == {"gram": 2, "search": 2, "bwd": 1}                # the two forward calls of the case and its one backward


@pytest.mark.parametrize("index", range(len(TG.SHAPES)), ids=TG.SHAPE_IDS)
def test_composed_route_agrees(emu, index):
    TG.case_composed(index)
    assert emu.calls == {"gram": 0, "search": 0, "bwd": 0}


def test_positive_measures_maximise(emu):
    """SISDR / SDR / ThresholdedSNR (maximize = True) pick the same assignment as their negatives and return the value with the other sign"""
    est, tgt, assign = TG.make_case(2)
    for pos, neg in ((SISDR, NegSISDR), (ThresholdedSNR, NegThresholdedSNR)):
        for reduction in ("mean", "sum"):
            up, a1 = mixit(pos(reduction=reduction), est.float(), tgt.float(), batch_mean=False)
            down, a2 = MixIT(neg(reduction=reduction))(est.float(), tgt.float(), batch_mean=False)
            assert torch.equal(a1, assign) and torch.equal(a2, assign) and torch.equal(up, -down)
    best = TG.extremum(TG.case_values(2, "snr"), True, False)[0]
    assert (mixit(ThresholdedSNR(reduction="sum"), est.float(), tgt.float(), batch_mean=False)[0].double() - best).abs().max() <= 1e-4


def test_thresholded_snr_on_its_own(emu):
    """the new criterion class through the row-distance machinery: value and gradient against the formula in fp64, and its saturation"""
    g = torch.Generator().manual_seed(3)
    t = torch.randn(3, 2, 500, generator=g)
    x = (t + 0.1 * torch.randn(3, 2, 500, generator=g)).requires_grad_(True)
    loss = NegThresholdedSNR(snr_max=20.0)(x, t)
    loss.backward()
    x64 = x.detach().double().requires_grad_(True)
    want = -TG.measure("snr", x64, t.double(), tau=10.0 ** -2.0).mean(1).mean(0)
    want.backward()
    assert abs(loss.item() - want.item()) <= 1e-5 and (x.grad.double() - x64.grad).abs().max() <= 1e-5 * x64.grad.abs().max()
    assert ThresholdedSNR().maximize and not NegThresholdedSNR().maximize and ThresholdedSNR(snr_max=20.0).tau == pytest.approx(0.01)
    exact = thresholded_snr(t, t, snr_max=30.0)
    assert (exact - 30.0).abs().max() <= 1e-4                                   # a perfect estimate scores snr_max, not infinity
    with pytest.raises(NotImplementedError):
        NegThresholdedSNR()(x.detach(), t.clone().requires_grad_(True))


def test_one_training_step_on_the_emulator(emu):
    from models.conv_tasnet import ConvTasNet
    from sepkernels.train import FusedTrainStep
    torch.manual_seed(5)
    model = ConvTasNet(n_basis=16, kernel_size=4, stride=2, enc_basis="trainable", dec_basis="trainable", enc_nonlinear=None, sep_hidden_channels=16,
                       sep_bottleneck_channels=16, sep_skip_channels=16, sep_kernel_size=3, sep_num_blocks=1, sep_num_layers=2, causal=False, n_sources=4)
    assert model.fused
    mixtures = 0.1 * torch.randn(2, 2, 512)
    step = FusedTrainStep(model, MixIT(NegThresholdedSNR()), lr=1e-3, max_norm=5.0)
    assert "other criteria run eagerly" in step.recordable()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    first, second = step(mixtures.sum(1, keepdim=True), mixtures).item(), step(mixtures.sum(1, keepdim=True), mixtures).item()
    assert math.isfinite(first) and second < first, (first, second)
    assert all(not torch.equal(p.detach(), before[k]) for k, p in model.named_parameters())
    assert emu.calls == {"gram": 2, "search": 2, "bwd": 2}


# ------------------------------------------------------------------------------------------------------ (b) the kernel sources on the host
@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim_mixit.build_library(str(tmp_path_factory.mktemp("hostsim_mixit")))


@pytest.fixture()
def on_host(sim_library):
    saved = (TG.HIP, TG.to_device, TG.device_sync)
    with hostsim.HostSimBackend(sim_library) as K:
        TG.HIP, TG.to_device, TG.device_sync = K, (lambda t: t.clone()), (lambda: None)
        try:
            yield K
        finally:
            TG.HIP, TG.to_device, TG.device_sync = saved


@needs_clang
@pytest.mark.parametrize("T", TG.GRAM_T)
@pytest.mark.parametrize("MN", TG.GRAM_MN, ids=["R2", "R5", "R10", "R24"])
def test_gram_kernel_source_on_the_host(on_host, MN, T):
    TG.case_gram(MN[0], MN[1], T, batch_check=(T == TG.SLAB + 1))


@needs_clang
@pytest.mark.parametrize("kind", TG.KINDS)
@pytest.mark.parametrize("index", range(len(TG.SHAPES)), ids=TG.SHAPE_IDS)
def test_search_kernel_source_on_the_host(on_host, index, kind):
    for maximize, use_mean in itertools.product((1, 0), (1, 0)):
        TG.case_search(index, kind, maximize, use_mean)


@needs_clang
@pytest.mark.parametrize("kind", TG.KINDS)
def test_search_kernel_source_ties_and_the_largest_search(on_host, kind):
    TG.case_search_tie(kind)
    TG.case_search_largest(kind)


@needs_clang
@pytest.mark.parametrize("kind", TG.KINDS)
@pytest.mark.parametrize("index", range(len(TG.SHAPES)), ids=TG.SHAPE_IDS)
def test_bwd_kernel_source_on_the_host(on_host, index, kind):
    TG.case_bwd(index, kind)


@needs_clang
@pytest.mark.parametrize("kind", TG.KINDS)
def test_bwd_kernel_source_at_the_tile_edges(on_host, kind):
    TG.case_bwd_lengths(kind, 1)
    TG.case_bwd_lengths(kind, 1025)


@needs_clang
def test_the_kernel_comparison_is_not_vacuous(on_host):
    """the same cases fail when the device side computes something else: estimates and mixtures swapped in the Gram matrix, the other
    extremum, the gradient of another measure"""
    class Skewed:
        def __getattr__(self, name):
            return getattr(on_host, name)

        def mixit_gram(self, est, tgt, gram, scratch, B, M, N, T):
            return on_host.mixit_gram(est.flip(1).contiguous(), tgt, gram, scratch, B, M, N, T)

        def mixit_search(self, gram, B, M, N, kind, maximize, *rest):
            return on_host.mixit_search(gram, B, M, N, kind, 1 - maximize, *rest)

        def mixit_bwd(self, est, tgt, gram, best_idx, gw, d_est, B, M, N, T, kind, eps, tau):
            return on_host.mixit_bwd(est, tgt, gram, best_idx, gw, d_est, B, M, N, T, 2 - kind, eps, tau)
    TG.HIP = Skewed()
    with pytest.raises(AssertionError):
        TG.case_gram(3, 2, 257)
    with pytest.raises(AssertionError):
        TG.case_search(3, "sisdr", 1, 1)
    with pytest.raises(AssertionError):
        TG.case_bwd(3, "sisdr")


@needs_clang
def test_criterion_through_the_kernel_sources(on_host):
    """criterion/mixit.py end to end with the host simulation of the kernels behind the binding"""
    class Named:
        name = "hostsim"

        def __getattr__(self, attr):
            return getattr(on_host, attr)
    old = sepkernels._set_backend_for_tests(Named())
    try:
        for kind in TG.KINDS:
            TG.case_criterion(2, kind)
    finally:
        sepkernels._set_backend_for_tests(old)


# ------------------------------------------------------------------------------------------------------ (c) the sanitized program
@needs_clang
def test_stand_alone_program_under_the_address_and_undefined_sanitizers():
    """tools/hostsim/mixit_main.cpp + the kernel sources, built with -fsanitize=address,undefined into a program of its own and run: the three
    kernels at R = 2, 10, 24 and T = 1, 2 SLAB + 17 against plain double loops on exactly-sized buffers, zero sanitizer reports"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostsim_mixit.py"), "--asan"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "7 cases, 0 mismatches" in r.stdout and "sanitizer reports: 0" in r.stdout, r.stdout[-3000:]


# ------------------------------------------------------------------------------------------------------ (d) refusals and routes
def test_refusals(emu):
    est, tgt = torch.randn(2, 3, 64), torch.randn(2, 2, 64)
    with pytest.raises(NotImplementedError):
        mixit(NegSISDR(), est, tgt.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):                              # ... on the composed route too
        mixit(ClippedNegSISDR(min=-30.0), est, tgt.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        mixit(NegSISDR(), est, tgt[:1])                                   # batch sizes differ
    with pytest.raises(ValueError):
        mixit(NegSISDR(), est, tgt[:, :, :63])                            # lengths differ
    with pytest.raises(ValueError):
        mixit(NegSISDR(), est, tgt[:, 0])                                 # not (B, N, T)
    with pytest.raises(ValueError):
        mixit(NegSISDR(reduction=None), est, tgt)                         # no value per item to search on
    assert emu.calls == {"gram": 0, "search": 0, "bwd": 0}


def test_what_takes_the_composed_route(emu):
    """counted on the emulator: a clipped criterion, N^M beyond 65536, a 4-D input, a criterion of another family, fp64 -- no kernel call"""
    from criterion.distance import MeanSquaredError
    g = torch.Generator().manual_seed(0)
    est, tgt = torch.randn(2, 3, 64, generator=g), torch.randn(2, 2, 64, generator=g)
    want = mixit(NegSISDR(), est, tgt, batch_mean=False)
    assert emu.calls == {"gram": 1, "search": 1, "bwd": 0}
    got = mixit(ClippedNegSISDR(min=-1000.0), est, tgt, batch_mean=False)
    assert torch.equal(got[1], want[1]) and (got[0] - want[0]).abs().max() <= 1e-4
    got = mixit(NegSISDR(), est.double(), tgt.double(), batch_mean=False)
    assert torch.equal(got[1], want[1]) and (got[0] - want[0]).abs().max() <= 1e-4
    loss, assign = mixit(NegSISDR(), est.view(2, 3, 2, 32), tgt.view(2, 2, 2, 32))                    # (B, M, channels, T)
    assert loss.dim() == 0 and assign.shape == (2, 3)
    loss, assign = mixit(MeanSquaredError(dim=2, reduction="mean"), est, tgt, batch_mean=False)
    brute = torch.stack([((torch.einsum("nm,bmt->bnt", TG.remix_matrix(3, 2)[k].float(), est) - tgt) ** 2).mean(2).mean(1) for k in range(8)], 1)
    assert torch.equal(assign, torch.tensor(list(itertools.product(range(2), repeat=3)))[brute.argmin(1)])
    small = torch.randn(1, 17, 4, generator=g)                            # 2^17 assignments: beyond the kernels, searched block by block
    loss, assign = mixit(NegSISDR(), small, torch.randn(1, 2, 4, generator=g))
    assert assign.shape == (1, 17) and math.isfinite(loss.item())
    assert emu.calls == {"gram": 1, "search": 1, "bwd": 0}


def test_composed_route_searches_in_blocks(emu, monkeypatch):
    """the running extremum over blocks of assignments equals the search over all of them at once, ties included: identical estimates make
    codes 3 and 5 score alike and 3 must be kept although 5 lies in a later block"""
    import criterion.mixit as CM
    g = torch.Generator().manual_seed(77)
    e, s = torch.randn(2, 1, 200, generator=g), torch.randn(2, 1, 200, generator=g)
    est, tgt = torch.cat([e, e, s], 1), torch.cat([e, e + s], 1) + 0.3 * torch.randn(2, 2, 200, generator=g)
    crit = ClippedNegSISDR(min=-1000.0)
    whole = mixit(crit, est, tgt, batch_mean=False)
    monkeypatch.setattr(CM, "_BLOCK_ELEMS", 2 * tgt.numel())             # two assignments at a time: 3 and 5 fall into different blocks
    blocks = mixit(crit, est, tgt, batch_mean=False)
    assert whole[1].tolist() == [[0, 1, 1], [0, 1, 1]] and torch.equal(blocks[1], whole[1]) and torch.equal(blocks[0], whole[0])


def test_cpu_tensors_beside_the_hip_library_take_the_composed_route():
    """the product's own backend object: CPU tensors never reach a kernel (`--use_cuda 0` evaluation), the criteria evaluate with ATen"""
    assert sepkernels.backend().name == "hip"
    for index, kind in ((2, "sisdr"), (3, "sdr"), (2, "snr")):
        est, tgt, assign = TG.make_case(index)
        best = TG.extremum(TG.case_values(index, kind), True, True)[0]
        leaf = est.float().requires_grad_(True)
        loss, got = MixIT(TG.criteria()[kind]())(leaf, tgt.float(), batch_mean=False)
        loss.sum().backward()
        assert torch.equal(got, assign) and (loss.detach().double() + best).abs().max() <= 1e-4 and torch.isfinite(leaf.grad).all()


def test_library_argument_checks_precede_the_launch():
    """no launch happens here: each call fails its own checks before any HIP call (the pointers are never followed)"""
    lib = sepkernels.load()
    p, big = 1 << 12, 1 << 30
    for B, M, N, T in [(1, 2, 2, 100), (16, 8, 2, 32000), (3, 16, 8, 2 * TG.SLAB + 17)]:
        want = 8 * B * -(-T // TG.SLAB) * (M + N) ** 2
        assert lib.sep_mixit_scratch_bytes(B, M, N, T) == want == sepkernels.HipBackend().mixit_scratch_bytes(B, M, N, T)
    assert lib.sep_mixit_scratch_bytes(1, 17, 2, 100) == 0 and lib.sep_mixit_scratch_bytes(1, 2, 9, 100) == 0 and lib.sep_mixit_scratch_bytes(1, 2, 2, 0) == 0
    assert '#define SEP_MIXIT_SLAB {}'.format(sepkernels.MIXIT_SLAB) in open(os.path.join(ROOT, "include", "sepkernels.h")).read()
    for args, words in (((None, p, p, p, big, 1, 2, 2, 100), b"null pointer"), ((p, p, p, p, big, 1, 17, 2, 100), b"bad arguments"),
                        ((p, p, p, p, big, 70000, 2, 2, 100), b"bad arguments"), ((p, p, p, p, 8 * 16 - 1, 1, 2, 2, 100), b"scratch holds")):
        assert lib.sep_mixit_gram(*args, None) < 0
        assert b"sep_mixit_gram" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    for args, words in (((None, 1, 2, 2, 0, 1, 1, 1e-12, 1e-3, p, p, p), b"null pointer"), ((p, 1, 2, 2, 3, 1, 1, 1e-12, 1e-3, p, p, p), b"bad arguments"),
                        ((p, 1, 17, 2, 0, 1, 1, 1e-12, 1e-3, p, p, p), b"bad arguments"), ((p, 1, 6, 8, 0, 1, 1, 1e-12, 1e-3, p, p, p), b"exceeds 65536")):
        assert lib.sep_mixit_search(*args, None) < 0
        assert b"sep_mixit_search" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    for args, words in (((p, p, p, p, None, p, 1, 2, 2, 100, 0, 1e-12, 1e-3), b"null pointer"), ((p, p, p, p, p, p, 1, 2, 2, 0, 0, 1e-12, 1e-3), b"bad arguments"),
                        ((p, p, p, p, p, p, 1, 2, 2, 100, 5, 1e-12, 1e-3), b"bad arguments")):
        assert lib.sep_mixit_bwd(*args, None) < 0
        assert b"sep_mixit_bwd" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    assert lib.sep_seq_lookup(b"sep_mixit_scratch_bytes") == -1 and min(lib.sep_seq_lookup(n) for n in (b"sep_mixit_gram", b"sep_mixit_search", b"sep_mixit_bwd")) >= 0
    with pytest.raises(sepkernels.SepKernelsError):                       # CPU tensors never reach a kernel
        sepkernels.HipBackend().mixit_gram(torch.zeros(1, 1, 8), torch.zeros(1, 1, 8), torch.zeros(1, 2, 2, dtype=torch.float64),
                                           torch.zeros(4, dtype=torch.float64), 1, 1, 1, 8)


# ------------------------------------------------------------------------------------------------------ (e) the dataset and the recipe
def test_mixture_of_mixtures(wav_tree, monkeypatch):              # noqa: F811
    import recipes.wsj0mix as WM
    root, lst = wav_tree
    opened = []
    real = WM.read_wav
    monkeypatch.setattr(WM, "read_wav", lambda path, *a, **k: (opened.append(os.path.basename(os.path.dirname(path))), real(path, *a, **k))[1])
    plain = WM.WaveEvalDataset(root, lst, n_sources=2)
    mom = WM.MixtureOfMixtures(plain, n_mixtures=2, seed=4)
    assert len(mom) == len(plain) == 3
    lengths = [e - s for _, s, e in plain.items]
    for i in range(3):
        mixture, mixtures, ID = mom[i]
        (j,) = mom.partners(i)
        assert j != i and ID == plain.items[i][0]
        T = min(lengths[i], lengths[j])
        assert mixture.shape == (1, T) and mixtures.shape == (2, T)
        assert torch.equal(mixture, mixtures.sum(0, keepdim=True))
        assert torch.equal(mixtures[0], real(plain._path("mix", plain.items[i][0]), 0, T)[0][0])
        assert torch.equal(mixtures[1], real(plain._path("mix", plain.items[j][0]), 0, T)[0][0])
    assert opened and set(opened) == {"mix"}, "the isolated sources must never be opened"
    # the pairing is a function of (seed, epoch, item): fixed while the epoch stands (validation), new with the epoch, back with the seed
    pairs = lambda ds: [tuple(ds.partners(i)) for i in range(len(ds))]          # noqa: E731
    train = WM.MixtureOfMixtures(WM.WaveTrainDataset(root, lst, samples=100, overlap=0, n_sources=2), n_mixtures=3, seed=4)
    assert len(train) == 10 + 7 + 4 and all(len(set(p) | {i}) == 3 for i, p in enumerate(pairs(train)))
    first = pairs(train)
    assert pairs(train) == first
    train.set_epoch(1)
    second = pairs(train)
    assert second != first
    again = WM.MixtureOfMixtures(train.dataset, n_mixtures=3, seed=4)
    assert pairs(again) == first and pairs(WM.MixtureOfMixtures(train.dataset, n_mixtures=3, seed=5)) != first
    mixture, mixtures = train[20]
    assert mixture.shape == (1, 100) and mixtures.shape == (3, 100) and torch.equal(mixture, mixtures.sum(0, keepdim=True))
    assert set(opened) == {"mix"}
    # through the loaders the trainer uses
    for mixture, mixtures, ids in WM.EvalDataLoader(mom, batch_size=1, shuffle=False):
        assert mixture.dim() == 3 and mixtures.shape[:2] == (1, 2) and len(ids) == 1
    mixture, mixtures = next(iter(WM.TrainDataLoader(train, batch_size=4, shuffle=True, drop_last=True)))
    assert mixture.shape == (4, 1, 100) and mixtures.shape == (4, 3, 100)
    with pytest.raises(ValueError):
        WM.MixtureOfMixtures(plain, n_mixtures=4)


def test_recipe_options():
    from criterion.pit import PIT1d
    from recipes.train_conv_tasnet import build_criterion, build_parser
    base = ["--train_wav_root", "a", "--valid_wav_root", "b", "--train_list_path", "c", "--valid_list_path", "d"]
    args = build_parser().parse_args(base)
    assert args.criterion == "sisdr" and isinstance(build_criterion(args), PIT1d) and type(build_criterion(args).criterion) is NegSISDR
    args = build_parser().parse_args(base + ["--criterion", "mixit", "--n_sources", "4"])
    crit = build_criterion(args)
    assert args.n_mixtures == 2 and args.mixit_measure == "snr"
    assert isinstance(crit, MixIT) and type(crit.criterion) is NegThresholdedSNR and crit.criterion.snr_max == 30.0
    args = build_parser().parse_args(base + ["--criterion", "mixit", "--mixit_measure", "sisdr", "--n_mixtures", "3"])
    assert args.n_mixtures == 3 and type(build_criterion(args).criterion) is NegSISDR
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--criterion", "pit"])
