"""CPU: optimal-permutation (Hungarian) training -- criterion/hungarian.py, csrc/assign.hip: sep_pair_gram / sep_assign / sep_pair_assign / sep_pair_bwd,
`--criterion hungarian` of recipes.train_conv_tasnet.

(a) the cases of tests/test_hungarian_gpu.py (its textbook fp64 oracle) on an emulator of the four calls (HungarianEmu below, written from their
    contract in include/sepkernels.h), call counts, routes, and one training step.
(b) the kernel SOURCES on the host (tools/hostsim.py): the kernel cases of tests/test_hungarian_gpu.py, and non-finite costs, which run nowhere else.
(c) the stand-alone program of tools/hostsim_hungarian.py built with -fsanitize=address,undefined and run as a program.
(d) refusals; the library's own argument checks, which need no GPU; the recipe's options.
Without the feature `import criterion.hungarian` fails: every test here fails."""
import math
import os
import subprocess
import sys

import pytest
import torch

import sepkernels
import test_hungarian_gpu as TG
from criterion.hungarian import HungarianLoss, hungarian
from criterion.sdr import ClippedNegSISDR, NegSISDR, NegThresholdedSNR
from emulator import EmuBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                         # noqa: E402
import hostsim_hungarian               # noqa: E402

needs_clang = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++")


class HungarianEmu(EmuBackend):
    """EmuBackend plus the four calls from their contract in include/sepkernels.h, in fp64 torch on CPU tensors: the inner products as one
    product, the measures and the two coefficients as the header names them, the assignment by the textbook solver of the test file (any
    optimal assignment satisfies the contract).  Counts its calls."""

    def __init__(self):
        super().__init__()
        self.calls = {"gram": 0, "assign": 0, "pair_assign": 0, "bwd": 0}

    def pair_gram_scratch_bytes(self, B, n, T):
        return 8 * B * -(-T // sepkernels.PAIR_SLAB) * (n * n + 2 * n) if 1 <= n <= 64 and 1 <= B <= 65535 and T >= 1 else 0

    def pair_gram(self, est, tgt, dots, tt, xx, scratch, B, n, T):
        self.calls["gram"] += 1
        if not (1 <= n <= sepkernels.ASSIGN_MAX_N and 1 <= B <= 65535 and T >= 1):
            raise sepkernels.SepKernelsError("sep_pair_gram: bad arguments")
        if 8 * scratch.numel() < self.pair_gram_scratch_bytes(B, n, T):
            raise sepkernels.SepKernelsError("sep_pair_gram: scratch holds {} bytes".format(8 * scratch.numel()))
        e, t = est.reshape(B, n, T).double(), tgt.reshape(B, n, T).double()
        dots.copy_(e @ t.transpose(1, 2))
        tt.copy_(t.square().sum(-1))
        xx.copy_(e.square().sum(-1))

    @staticmethod
    def _solve(C, perm, duals):
        for b in range(C.shape[0]):
            p, u, v = TG.solve(C[b])
            perm[b] = torch.tensor(p)
            if duals is not None:
                duals[b] = torch.tensor(u + v, dtype=torch.float64)

    def assign(self, cost, B, n, maximize, perm, total, duals):
        self.calls["assign"] += 1
        assert 1 <= n <= sepkernels.ASSIGN_MAX_N
        self._solve(-cost if maximize else cost, perm, duals)
        total.copy_(torch.gather(cost, 2, perm.unsqueeze(2)).squeeze(2).sum(1))

    @staticmethod
    def _pair_terms(kind, a, tt, xx, eps, tau):
        """-> value, cT, cE of include/sepkernels.h for inner products of any common shape"""
        Kc = 10.0 / math.log(10.0)
        if kind == 0:
            c = tt + eps
            alpha = a / c
            S = alpha * alpha * tt + eps
            Nn = (alpha * alpha * tt - 2 * alpha * a + xx).clamp_min(0) + eps
            return 10 * torch.log10(S / Nn), Kc * (2 * alpha * tt / (c * S) - ((2 * alpha * tt - 2 * a) / c - 2 * alpha) / Nn), Kc * (-2.0 / Nn)
        den = (tt - 2 * a + xx).clamp_min(0) + (tau * tt if kind == 2 else 0.0) + eps
        return 10 * torch.log10((tt + eps) / den), 2 * Kc / den, -2 * Kc / den

    def pair_assign(self, dots, tt, xx, B, n, kind, maximize, use_mean, eps, tau, best_val, perm, per_src, duals=None):
        self.calls["pair_assign"] += 1
        assert 1 <= n <= sepkernels.ASSIGN_MAX_N
        M = self._pair_terms(kind, dots, tt.unsqueeze(1), xx.unsqueeze(2), eps, tau)[0]
        self._solve(-M if maximize else M, perm, duals)
        chosen = torch.gather(M, 2, perm.unsqueeze(2)).squeeze(2)
        per_src.copy_(chosen)
        best_val.copy_(chosen.mean(1) if use_mean else chosen.sum(1))

    def pair_bwd(self, est, tgt, dots, tt, xx, perm, gw, d_est, B, n, T, kind, eps, tau):
        self.calls["bwd"] += 1
        rows = torch.arange(B).unsqueeze(1)
        _, cT, cE = self._pair_terms(kind, torch.gather(dots, 2, perm.unsqueeze(2)).squeeze(2), tt[rows, perm], xx, eps, tau)
        d_est.copy_(gw.double().view(B, 1, 1) * (cT.unsqueeze(2) * tgt.double()[rows, perm] + cE.unsqueeze(2) * est.double()))


@pytest.fixture()
def emu():
    K = HungarianEmu()
    saved = (TG.HIP, TG.to_device, TG.device_sync)
    old = sepkernels._set_backend_for_tests(K)
    TG.HIP, TG.to_device, TG.device_sync = K, (lambda t: t.clone()), (lambda: None)
    try:
        yield K
    finally:
        TG.HIP, TG.to_device, TG.device_sync = saved
        sepkernels._set_backend_for_tests(old)


# ------------------------------------------------------------------------------------------------------ (a) the criterion on the emulator
def test_the_oracle_itself():
    """the textbook solver against brute force (n <= 7) and scipy (if there) on every kind of matrix the tests use, both senses"""
    for n in (1, 2, 3, 5, 7):
        g = torch.Generator().manual_seed(1000 + n)
        for C in list(torch.randn(3, n, n, generator=g, dtype=torch.float64)) + list(TG.structured_matrices(n)[0].values()):
            TG.oracle_min(C)
            TG.oracle_min(-C)
    for index in range(2):
        for kind in TG.KINDS:
            TG.case_optimum(index, kind, True)
            TG.case_optimum(index, kind, False)
    perm, u, v = TG.solve([[4.0, 1.0, 3.0], [2.0, 0.0, 5.0], [3.0, 2.0, 2.0]])        # by hand: 1 + 2 + 2
    assert perm == [1, 0, 2] and abs(sum(u) + sum(v) - 5.0) <= 1e-12


@pytest.mark.parametrize("sign", [-1, 1], ids=["neg", "pos"])
@pytest.mark.parametrize("kind", TG.KINDS)
@pytest.mark.parametrize("index", range(len(TG.SHAPES)), ids=TG.SHAPE_IDS)
def test_criterion_against_the_oracle(emu, index, kind, sign):
    TG.case_criterion(index, kind, sign)
    assert emu.calls == {"gram": 2, "assign": 0, "pair_assign": 2, "bwd": 1}           # the two forward calls of the case and its one backward


@pytest.mark.parametrize("kind", TG.KINDS)
def test_sum_reduction_and_default_constructor(emu, kind):
    TG.case_criterion_sum(2, kind)
    TG.case_default_constructor()
    assert emu.calls == {"gram": 3, "assign": 0, "pair_assign": 3, "bwd": 0}


@pytest.mark.parametrize("n", [2, 3, 4, 6])
def test_criterion_agrees_with_pit(emu, n):
    TG.case_against_pit(n)


@pytest.mark.parametrize("index", range(len(TG.SHAPES)), ids=TG.SHAPE_IDS)
def test_composed_route_agrees(emu, index):
    TG.case_composed(index)
    assert emu.calls == {"gram": 1, "assign": 1, "pair_assign": 1, "bwd": 0}            # the clipped criterion: sep_assign alone; then the kernel route of the case


@pytest.mark.parametrize("case", ["gram", "assign", "structured", "pair_assign", "bwd"])
def test_kernel_cases_hold_on_the_emulator(emu, case):
    """the case functions against an independent statement of the contract: a case that the contract cannot pass would fail here first"""
    if case == "gram":
        TG.case_gram(9, 257, B=3)
        TG.case_gram_refusals()
    elif case == "assign":
        for n in (1, 5, 16):
            TG.case_assign(n, 0)
            TG.case_assign(n, 1)
    elif case == "structured":
        TG.case_assign_structured(7)
    elif case == "pair_assign":
        for kind in TG.KINDS:
            TG.case_pair_assign(1, kind, 1, 1)
            TG.case_pair_assign(1, kind, 0, 0)
    else:
        for kind in TG.KINDS:
            TG.case_pair_bwd(1, kind)


def test_batches_beyond_the_grid_limit_go_through_in_slices(emu, monkeypatch):
    import criterion.hungarian as CH
    est, tgt, planted = TG.make_case(1)
    est, tgt, planted = est.repeat(3, 1, 1)[:5], tgt.repeat(3, 1, 1)[:5], planted.repeat(3, 1)[:5]
    whole_leaf = est.float().requires_grad_(True)
    whole = hungarian(NegSISDR(), whole_leaf, tgt.float(), batch_mean=False)
    whole[0].sum().backward()
    calls = dict(emu.calls)
    monkeypatch.setattr(CH, "_MAX_ROWS", 2)
    leaf = est.float().requires_grad_(True)
    sliced = hungarian(NegSISDR(), leaf, tgt.float(), batch_mean=False)
    sliced[0].sum().backward()
    assert torch.equal(sliced[0], whole[0]) and torch.equal(sliced[1], planted) and torch.equal(leaf.grad, whole_leaf.grad)
    assert {k: emu.calls[k] - calls[k] for k in calls} == {"gram": 3, "assign": 0, "pair_assign": 3, "bwd": 3}


def test_one_training_step_on_the_emulator(emu, tmp_path):
    TG.case_training_step(tmp_path, "cpu")
    assert emu.calls == {"gram": 1, "assign": 0, "pair_assign": 1, "bwd": 1}


# ------------------------------------------------------------------------------------------------------ (b) the kernel sources on the host
@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim_hungarian.build_library(str(tmp_path_factory.mktemp("hostsim_hungarian")))


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
@pytest.mark.parametrize("n,T", TG.GRAM_CASES, ids=["n{}-T{}".format(n, T) for n, T in TG.GRAM_CASES])
def test_pair_gram_kernel_source_on_the_host(on_host, n, T):
    """one host thread per lane: the batch of three (an item alone against the same item in a batch) runs where a workgroup owns the whole matrix
    and at one length of the blocked form; the device runs it at three lengths for every n"""
    TG.case_gram(n, T, B=3 if T == 257 or (n <= 8 and T in (1, TG.SLAB + 1)) else 1)


@needs_clang
def test_pair_gram_refusals_on_the_host(on_host):
    TG.case_gram_refusals()


@needs_clang
@pytest.mark.parametrize("n", TG.ASSIGN_N)
def test_assign_kernel_source_on_the_host(on_host, n):
    TG.case_assign(n, 0)
    TG.case_assign(n, 1)


@needs_clang
@pytest.mark.parametrize("n", [1, 2, 7, 16, 64])
def test_assign_kernel_source_on_structured_matrices(on_host, n):
    TG.case_assign_structured(n)


_NONFINITE_CHILD = """
import sys
sys.path[:0] = {paths!r}
import hostsim
import test_hungarian_gpu as TG
with hostsim.HostSimBackend({so!r}) as K:
    TG.HIP, TG.to_device, TG.device_sync = K, (lambda t: t.clone()), (lambda: None)
    for n in (1, 2, 9, 33, 64):
        TG.case_assign_nonfinite(n)
print("non-finite costs: every call came back with a permutation")
"""


@needs_clang
def test_nonfinite_costs_end_with_a_permutation(sim_library):
    """a matrix with NaNs, one of all NaN, one with +-Inf, both senses, on the host simulation ONLY and in a process of its own under a time
    limit: the solver's loops have trip counts fixed by n, so the call comes back whatever the comparisons say"""
    paths = [p for p in sys.path if p]
    r = subprocess.run([sys.executable, "-c", _NONFINITE_CHILD.format(paths=paths, so=sim_library)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "every call came back" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@needs_clang
@pytest.mark.parametrize("kind", TG.KINDS)
@pytest.mark.parametrize("index", range(len(TG.SHAPES)), ids=TG.SHAPE_IDS)
def test_pair_assign_and_bwd_kernel_sources_on_the_host(on_host, index, kind):
    for maximize in (1, 0):
        for use_mean in (1, 0):
            TG.case_pair_assign(index, kind, maximize, use_mean)
    TG.case_pair_bwd(index, kind)


@needs_clang
def test_the_kernel_comparison_is_not_vacuous(on_host):
    """the same cases fail when the device side computes something else: estimates reordered in the inner products, a matching that is not the
    best, the other sense, the gradient of another measure"""
    class Skewed:
        def __getattr__(self, name):
            return getattr(on_host, name)

        def pair_gram(self, est, tgt, *rest):
            return on_host.pair_gram(est.flip(1).contiguous(), tgt, *rest)

        def assign(self, cost, B, n, maximize, perm, total, duals):
            on_host.assign(cost, B, n, maximize, perm, total, duals)
            perm.copy_(perm.roll(1, 1))

        def pair_assign(self, dots, tt, xx, B, n, kind, maximize, *rest):
            return on_host.pair_assign(dots, tt, xx, B, n, kind, 1 - maximize, *rest)

        def pair_bwd(self, est, tgt, dots, tt, xx, perm, gw, d_est, B, n, T, kind, eps, tau):
            return on_host.pair_bwd(est, tgt, dots, tt, xx, perm, gw, d_est, B, n, T, 2 - kind, eps, tau)
    TG.HIP = Skewed()
    with pytest.raises(AssertionError):
        TG.case_gram(9, 257)
    with pytest.raises(AssertionError):
        TG.case_assign(5, 0)
    with pytest.raises(AssertionError):
        TG.case_pair_assign(1, "sisdr", 1, 1)
    with pytest.raises(AssertionError):
        TG.case_pair_bwd(1, "sisdr")


@needs_clang
def test_criterion_through_the_kernel_sources(on_host):
    """criterion/hungarian.py end to end with the host simulation of the kernels behind the binding: the kernel route, the composed route
    (sep_assign), and the 30 dB case next to sep_sisdr_dots"""
    class Named:
        name = "hostsim"

        def __getattr__(self, attr):
            return getattr(on_host, attr)
    old = sepkernels._set_backend_for_tests(Named())
    try:
        for kind in TG.KINDS:
            TG.case_criterion(1, kind)
        TG.case_criterion(2, "snr", 1)
        TG.case_composed(1)
        TG.test_high_sdr_error_next_to_the_existing_kernels()
    finally:
        sepkernels._set_backend_for_tests(old)


# ------------------------------------------------------------------------------------------------------ (c) the sanitized program
@needs_clang
def test_stand_alone_program_under_the_address_and_undefined_sanitizers():
    """tools/hostsim/hungarian_main.cpp + the kernel sources, built with -fsanitize=address,undefined into a program of its own and run: the four
    kernels at n = 1, 9, 64 and T = 1, 2 SLAB + 17 against plain double loops on exactly-sized buffers, NaN and Inf matrices, zero reports"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostsim_hungarian.py"), "--asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "22 cases, 0 mismatches" in r.stdout and "sanitizer reports: 0" in r.stdout, r.stdout[-3000:]


# ------------------------------------------------------------------------------------------------------ (d) refusals and routes
def test_refusals(emu):
    est, tgt = torch.randn(2, 3, 64), torch.randn(2, 3, 64)
    with pytest.raises(NotImplementedError):
        hungarian(NegSISDR(), est, tgt.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):                              # ... on the composed route too
        hungarian(ClippedNegSISDR(min=-30.0), est, tgt.clone().requires_grad_(True))
    with pytest.raises(ValueError):
        hungarian(NegSISDR(), est, tgt[:1])                               # batch sizes differ
    with pytest.raises(ValueError):
        hungarian(NegSISDR(), est, tgt[:, :, :63])                        # lengths differ
    with pytest.raises(ValueError):
        hungarian(NegSISDR(), est, tgt[:, :2])                            # numbers of sources differ
    with pytest.raises(ValueError):
        hungarian(NegSISDR(), est, tgt[:, 0])                             # not (B, n, T)
    with pytest.raises(ValueError):
        hungarian(NegSISDR(reduction=None), est, tgt)                     # no value per item to search on
    assert emu.calls == {"gram": 0, "assign": 0, "pair_assign": 0, "bwd": 0}


def test_what_takes_the_composed_route(emu):
    """counted on the emulator: a clipped criterion, a criterion of another family, a 4-D input, fp64, n = 65 -- no call of the waveform kernels"""
    from criterion.distance import MeanSquaredError
    g = torch.Generator().manual_seed(0)
    tgt = torch.randn(2, 4, 64, generator=g)
    planted = torch.stack([torch.randperm(4, generator=g) for _ in range(2)])
    est = 0.8 * tgt[torch.arange(2).unsqueeze(1), planted] + 0.3 * torch.randn(2, 4, 64, generator=g)
    want = hungarian(NegSISDR(), est, tgt, batch_mean=False)
    assert emu.calls == {"gram": 1, "assign": 0, "pair_assign": 1, "bwd": 0} and torch.equal(want[1], planted)
    got = hungarian(ClippedNegSISDR(min=-1000.0), est, tgt, batch_mean=False)
    assert torch.equal(got[1], planted) and (got[0] - want[0]).abs().max() <= 1e-5
    got = hungarian(NegSISDR(), est.double(), tgt.double(), batch_mean=False)
    assert torch.equal(got[1], planted) and (got[0] - want[0]).abs().max() <= 1e-5
    loss, pattern = hungarian(NegSISDR(), est.view(2, 4, 2, 32), tgt.view(2, 4, 2, 32))                  # (B, n, channels, T)
    assert loss.dim() == 0 and torch.equal(pattern, planted)
    leaf = est.clone().requires_grad_(True)
    loss, pattern = hungarian(MeanSquaredError(dim=2, reduction="mean"), leaf, tgt, batch_mean=False)
    loss.sum().backward()
    pairs = (est.unsqueeze(2) - tgt.unsqueeze(1)).double().square().mean(3)
    assert torch.equal(pattern, planted) and all(abs(TG.oracle_min(pairs[b])[0] / 4 - loss[b].item()) <= 1e-6 for b in range(2)) and leaf.grad.abs().max() > 0
    assert emu.calls == {"gram": 1, "assign": 4, "pair_assign": 1, "bwd": 0}
    big_t = torch.randn(1, 65, 16, generator=g)                              # n = 65: beyond the wavefront, the module's own solver
    big_p = torch.randperm(65, generator=g).unsqueeze(0)
    loss, pattern = hungarian(NegSISDR(), 0.8 * big_t[:, big_p[0]] + 0.1 * torch.randn(1, 65, 16, generator=g), big_t)
    assert torch.equal(pattern, big_p) and math.isfinite(loss.item())
    assert emu.calls == {"gram": 1, "assign": 4, "pair_assign": 1, "bwd": 0}


def test_composed_route_forms_the_pair_matrix_in_blocks(emu, monkeypatch):
    import criterion.hungarian as CH
    est, tgt, planted = TG.make_case(1)
    crit = ClippedNegSISDR(min=-1000.0)
    whole = hungarian(crit, est.float(), tgt.float(), batch_mean=False)
    monkeypatch.setattr(CH, "_BLOCK_ELEMS", 3 * 257)                       # three single-source rows at a time
    blocks = hungarian(crit, est.float(), tgt.float(), batch_mean=False)
    assert torch.equal(blocks[1], planted) and torch.equal(blocks[1], whole[1]) and torch.equal(blocks[0], whole[0])


def test_the_host_solver_of_the_module():
    """criterion.hungarian._solve_host (CPU tensors beside the HIP library, n > 64): optimal by value on random and structured matrices, a
    permutation on non-finite ones"""
    from criterion.hungarian import _solve_host
    for n in (1, 2, 5, 7, 16, 65):
        mats = torch.cat([torch.randn(2, n, n, generator=torch.Generator().manual_seed(n), dtype=torch.float64), torch.stack(list(TG.structured_matrices(n)[0].values()))])
        perm = _solve_host(mats.numpy())
        for b in range(mats.shape[0]):
            best, _ = TG.oracle_min(mats[b])
            assert sorted(perm[b].tolist()) == list(range(n)) and abs(TG.value_of(mats[b], perm[b].tolist()) - best) <= 1e-9 * n * max(1.0, mats[b].abs().max().item())
        for row in _solve_host(TG.nonfinite_matrices(n).numpy()):
            assert sorted(row.tolist()) == list(range(n))


def test_cpu_tensors_beside_the_hip_library_take_the_composed_route():
    """the product's own backend object: CPU tensors never reach a kernel (`--use_cuda 0` evaluation): the criteria evaluate with ATen, the
    assignment is the module's own solver"""
    assert sepkernels.backend().name == "hip"
    for index, kind in ((1, "sisdr"), (0, "sdr"), (2, "snr")):
        B, n, T = TG.SHAPES[index]
        est, tgt, planted = TG.make_case(index)
        best = TG.case_optimum(index, kind, True)[1]
        leaf = est.float().requires_grad_(True)
        loss, got = HungarianLoss(TG.criteria()[kind, -1]())(leaf, tgt.float(), batch_mean=False)
        loss.sum().backward()
        assert torch.equal(got, planted) and (loss.detach().double() + best / n).abs().max() <= 1e-4 and torch.isfinite(leaf.grad).all()


def test_library_argument_checks_precede_the_launch():
    """no launch happens here: each call fails its own checks before any HIP call (the pointers are never followed)"""
    lib = sepkernels.load()
    p, big = 1 << 12, 1 << 30
    for B, n, T in [(1, 2, 100), (4, 20, 32000), (3, 64, 2 * TG.SLAB + 17)]:
        want = 8 * B * -(-T // TG.SLAB) * (n * n + 2 * n)
        assert lib.sep_pair_gram_scratch_bytes(B, n, T) == want == sepkernels.HipBackend().pair_gram_scratch_bytes(B, n, T)
    assert lib.sep_pair_gram_scratch_bytes(1, 65, 100) == 0 and lib.sep_pair_gram_scratch_bytes(1, 0, 100) == 0 and lib.sep_pair_gram_scratch_bytes(1, 2, 0) == 0
    header = open(os.path.join(ROOT, "include", "sepkernels.h")).read()
    assert "#define SEP_PAIR_SLAB {}".format(sepkernels.PAIR_SLAB) in header and "#define SEP_ASSIGN_MAX_N {}".format(sepkernels.ASSIGN_MAX_N) in header
    assert "#define SEP_ABI_VERSION 23" in header
    for args, words in (((None, p, p, p, p, p, big, 1, 2, 100), b"null pointer"), ((p, p, p, p, p, p, big, 1, 65, 100), b"bad arguments"),
                        ((p, p, p, p, p, p, big, 1, 0, 100), b"bad arguments"), ((p, p, p, p, p, p, big, 70000, 2, 100), b"bad arguments"),
                        ((p, p, p, p, p, p, 8 * 8 - 1, 1, 2, 100), b"scratch holds")):
        assert lib.sep_pair_gram(*args, None) < 0
        assert b"sep_pair_gram" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    for args, words in (((None, 1, 2, 0, p, p, p), b"null pointer"), ((p, 1, 2, 0, p, p, None), b"null pointer"), ((p, 1, 65, 0, p, p, p), b"bad arguments"),
                        ((p, 1, 0, 0, p, p, p), b"bad arguments"), ((p, 0, 2, 0, p, p, p), b"bad arguments")):
        assert lib.sep_assign(*args, None) < 0
        assert b"sep_assign" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    for args, words in (((None, p, p, 1, 2, 0, 1, 1, 1e-12, 1e-3, p, p, p, None), b"null pointer"), ((p, p, p, 1, 2, 3, 1, 1, 1e-12, 1e-3, p, p, p, None), b"bad arguments"),
                        ((p, p, p, 1, 65, 0, 1, 1, 1e-12, 1e-3, p, p, p, None), b"bad arguments")):
        assert lib.sep_pair_assign(*args, None) < 0
        assert b"sep_pair_assign" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    for args, words in (((p, p, p, p, p, p, None, p, 1, 2, 100, 0, 1e-12, 1e-3), b"null pointer"), ((p, p, p, p, p, p, p, p, 1, 2, 0, 0, 1e-12, 1e-3), b"bad arguments"),
                        ((p, p, p, p, p, p, p, p, 1, 2, 100, 5, 1e-12, 1e-3), b"bad arguments"), ((p, p, p, p, p, p, p, p, 1, 65, 100, 0, 1e-12, 1e-3), b"bad arguments")):
        assert lib.sep_pair_bwd(*args, None) < 0
        assert b"sep_pair_bwd" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    assert lib.sep_seq_lookup(b"sep_pair_gram_scratch_bytes") == -1
    assert min(lib.sep_seq_lookup(n) for n in (b"sep_pair_gram", b"sep_assign", b"sep_pair_assign", b"sep_pair_bwd")) >= 0
    with pytest.raises(sepkernels.SepKernelsError):                       # CPU tensors never reach a kernel
        sepkernels.HipBackend().assign(torch.zeros(1, 2, 2, dtype=torch.float64), 1, 2, 0, torch.zeros(1, 2, dtype=torch.int64), torch.zeros(1, dtype=torch.float64),
                                       torch.zeros(1, 4, dtype=torch.float64))


def test_recipe_options():
    from criterion.pit import PIT1d
    from recipes.train_conv_tasnet import build_criterion, build_parser
    base = ["--train_wav_root", "a", "--valid_wav_root", "b", "--train_list_path", "c", "--valid_list_path", "d"]
    args = build_parser().parse_args(base)
    assert args.criterion == "sisdr" and isinstance(build_criterion(args), PIT1d)
    args = build_parser().parse_args(base + ["--criterion", "hungarian", "--n_sources", "20"])
    crit = build_criterion(args)
    assert args.hungarian_measure == "sisdr" and isinstance(crit, HungarianLoss) and type(crit.criterion) is NegSISDR
    args = build_parser().parse_args(base + ["--criterion", "hungarian", "--hungarian_measure", "snr"])
    crit = build_criterion(args)
    assert isinstance(crit, HungarianLoss) and type(crit.criterion) is NegThresholdedSNR and crit.criterion.snr_max == 30.0
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--criterion", "hungarian", "--hungarian_measure", "mse"])
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--criterion", "munkres"])
