"""CPU: window-by-window separation of long recordings -- sepkernels/longform.py (stitch, separate_long), csrc/stitch.hip: sep_stitch_cost /
sep_stitch_chain / sep_stitch_ola, ConvTasNet.separate_long, recipes.trainer.Tester's long_form_window, `python -m recipes.separate`.

(1) the composed route of stitch() against the numpy fp64 oracle of tests/test_longform_gpu.py (matching by brute force) on inputs with a
    guaranteed gap between the best matching of every boundary and the runner-up.
(2) separate_long around a fake model that scrambles its outputs from call to call.
(3) refusals and routes (call counts on an emulator of the three calls).   (4) the header and the binding; the library's own argument checks.
(5) the kernel SOURCES on the host (tools/hostsim_stitch.py): the kernel cases of tests/test_longform_gpu.py, and the stand-alone program built
    with -fsanitize=address,undefined and run as a program.
(6) the command line and the tester.
Without the feature `import sepkernels.longform` fails: every test here fails."""
import argparse
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import sepkernels
import test_longform_gpu as TG
from emulator import EmuBackend
from sepkernels import longform
from sepkernels.longform import separate_long, stitch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dnn-based_source_separation_amd", "src")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                         # noqa: E402
import hostsim_stitch                  # noqa: E402

needs_clang = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++")

SHAPES = [(2, 1, 5), (128, 65, 400), (130, 65, 391), (1100, 571, 3000)]          # (win, hop, T)
SHAPE_IDS = ["{}-{}-{}".format(*s) for s in SHAPES]


def windows_for(win, hop, T):
    return max(1, -(-(T - win) // hop) + 1)


# ------------------------------------------------------------------------------------------------------ (1) the composed route against the oracle
@pytest.mark.parametrize("win,hop,T", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_composed_route_against_the_oracle(n, win, hop, T):
    B, W = 2, windows_for(win, hop, T)
    est, scramble = TG.gapped(B, W, n, win, hop)
    cost = TG.oracle_cost(est.numpy(), hop)
    local = np.empty((B, W - 1, n), dtype=np.int64)
    for b in range(B):
        for w in range(W - 1):                                              # EVERY boundary has its gap
            local[b, w], best, second = TG.oracle_match(cost[b, w])
            assert second - best >= 1e-6 * best, (b, w, best, second)
    want_perm = TG.oracle_chain(local, n)
    want_out, _ = TG.oracle_ola(est.numpy(), want_perm, hop, T)
    out, perm_abs, boundary = stitch(est, hop, T)
    assert out.dtype == torch.float64 and tuple(out.shape) == (B, n, T) and tuple(boundary.shape) == (B, W - 1)
    assert torch.equal(perm_abs, torch.from_numpy(want_perm))
    assert (out - torch.from_numpy(want_out)).abs().max().item() <= 1e-12
    assert TG.undoes_the_scramble(perm_abs, scramble)
    matched = np.take_along_axis(cost, local[..., None], 3).sum((2, 3))
    assert np.abs(boundary.numpy() - matched).max() <= 1e-12 * matched.max()


def test_the_oracle_is_not_vacuous():
    """a window order that is not undone, a cross-fade on the wrong side, are caught by the comparison above"""
    est, scramble = TG.gapped(1, 4, 3, 130, 65)
    out, perm_abs, _ = stitch(est, 65, 300)
    assert not TG.undoes_the_scramble(perm_abs.roll(1, 2), scramble)
    wrong, _ = TG.oracle_ola(est.numpy(), perm_abs.roll(1, 2).numpy(), 65, 300)
    assert (out - torch.from_numpy(wrong)).abs().max().item() > 0.1


# ------------------------------------------------------------------------------------------------------ (2) a scrambling fake model
class Scrambler(nn.Module):
    """(b, 1, t) -> (b, n, t): source s is gain_s x, the rows rotated by a counter that advances per call"""

    def __init__(self, gains):
        super().__init__()
        self.gains, self.calls = torch.tensor(gains), 0

    def forward(self, x):
        self.calls += 1
        return (self.gains.to(x.dtype).view(1, -1, 1) * x).roll(self.calls, 1)


@pytest.mark.parametrize("batch_windows", [1, 3, 16])
def test_separate_long_undoes_a_scrambling_model(batch_windows):
    gains = [1.0, -0.5, 0.25]
    g = torch.Generator().manual_seed(batch_windows)
    window, hop, T = 128, 65, 700
    for shape in ((T,), (1, T), (2, 1, T)):
        x = torch.randn(*shape, generator=g)
        model = Scrambler(gains)
        out = separate_long(model, x, window, hop=hop, batch_windows=batch_windows)
        W = windows_for(window, hop, T)
        B = shape[0] if len(shape) == 3 else 1
        assert model.calls == -(-B * W // batch_windows)
        assert tuple(out.shape) == ((2, 3, T) if len(shape) == 3 else (3, T))
        out, xs = out.reshape(B, 3, T), x.reshape(B, 1, T)
        for b in range(B):
            ratio = (out[b] * xs[b]).sum(-1) / xs[b].square().sum()          # the gain of every track: one fixed permutation of the gains
            order = [min(range(3), key=lambda s: abs(gains[s] - r)) for r in ratio.tolist()]
            assert sorted(order) == [0, 1, 2]
            want = torch.tensor(gains)[order].view(3, 1) * xs[b]
            assert (out[b] - want).abs().max().item() <= 1e-6 * xs[b].abs().max().item()


def test_separate_long_of_a_short_recording_is_one_call():
    x = torch.randn(2, 1, 100, generator=torch.Generator().manual_seed(0))
    for T in (100, 37):
        model, single = Scrambler([1.0, 0.5]), Scrambler([1.0, 0.5])
        assert torch.equal(separate_long(model, x[..., :T], 100), single(x[..., :T])) and model.calls == 1
        assert torch.equal(separate_long(Scrambler([1.0, 0.5]), x[0, 0, :T], 100), Scrambler([1.0, 0.5])(x[:1, :, :T])[0])
    model = Scrambler([1.0, 0.5])
    assert separate_long(model, x[..., :99], 64).shape == (2, 2, 99) and model.calls == 1          # default hop 32: 3 windows x 2 in one batch


def test_separate_long_leaves_the_mode_alone_and_runs_without_a_tape():
    seen = []

    class Probe(Scrambler):
        def forward(self, x):
            seen.append((self.training, torch.is_grad_enabled()))
            return super().forward(x)
    model = Probe([1.0, 0.5])
    model.train()
    separate_long(model, torch.randn(300), 128)
    model.eval()
    separate_long(model, torch.randn(100), 128)
    assert seen[0] == (True, False) and seen[-1] == (False, False) and not model.training


# ------------------------------------------------------------------------------------------------------ (3) refusals and routes
def test_refusals():
    est = torch.randn(1, 3, 2, 8, dtype=torch.float64)
    for hop in (3, 8, 9, 0):                                                 # hop < win / 2, hop >= win
        with pytest.raises(ValueError, match="hop must lie"):
            stitch(est, hop, 12)
    with pytest.raises(ValueError, match="cover 16 samples"):
        stitch(est, 4, 17)
    with pytest.raises(ValueError, match="cover 16 samples"):
        stitch(est, 4, 0)
    with pytest.raises(ValueError, match="n_windows, n_sources, window"):
        stitch(est[0], 4, 12)
    with pytest.raises(ValueError, match="floating-point"):
        stitch(est.long(), 4, 12)
    assert stitch(est, 4, 16)[0].shape == (1, 2, 16) and stitch(est, 7, 22)[0].shape == (1, 2, 22)
    model = Scrambler([1.0, 0.5])
    for hop in (31, 64, 100):
        with pytest.raises(ValueError, match="hop must lie"):
            separate_long(model, torch.randn(300), 64, hop=hop)
    with pytest.raises(ValueError, match="mixture"):
        separate_long(model, torch.randn(2, 300), 64)
    with pytest.raises(ValueError, match="mixture"):
        separate_long(model, torch.randn(1, 2, 2, 300), 64)
    with pytest.raises(ValueError, match="batch_windows"):
        separate_long(model, torch.randn(300), 64, batch_windows=0)
    assert model.calls == 0


class StitchEmu(EmuBackend):
    """EmuBackend plus the three calls (and sep_assign) from their contract in include/sepkernels.h, through the numpy oracle of the test file.
    Counts its calls."""

    def __init__(self):
        super().__init__()
        self.calls = {"cost": 0, "assign": 0, "chain": 0, "ola": 0}

    def stitch_cost(self, est, cost, B, W, n, win, hop):
        self.calls["cost"] += 1
        assert est.dtype == torch.float32 and 1 <= n <= 64 and win <= 2 * hop < 2 * win
        cost.copy_(torch.from_numpy(TG.oracle_cost(est.double().numpy(), hop)))

    def assign(self, cost, B, n, maximize, perm, total, duals):
        self.calls["assign"] += 1
        assert not maximize and 1 <= n <= 64
        from criterion.hungarian import _solve_host
        perm.view(B, n).copy_(torch.from_numpy(_solve_host(cost.reshape(B, n, n).numpy())))
        total.view(B).copy_(cost.reshape(B, n, n).gather(2, perm.view(B, n, 1)).sum((1, 2)))

    def stitch_chain(self, perm_local, perm_abs, B, W, n):
        self.calls["chain"] += 1
        perm_abs.copy_(torch.from_numpy(TG.oracle_chain(perm_local.numpy() if perm_local is not None else np.zeros((B, 0, n), dtype=np.int64), n)))

    def stitch_ola(self, est, perm_abs, out, B, W, n, win, hop, T):
        self.calls["ola"] += 1
        out.copy_(torch.from_numpy(TG.oracle_ola(est.double().numpy(), perm_abs.numpy(), hop, T)[0]))


@pytest.fixture()
def emu():
    K = StitchEmu()
    old = sepkernels._set_backend_for_tests(K)
    try:
        yield K
    finally:
        sepkernels._set_backend_for_tests(old)


def test_what_takes_which_route(emu):
    """counted on the emulator: contiguous fp32 with n <= 64 is the four launches, once each; fp64 and a strided view are composed in torch around
    sep_assign alone (criterion.hungarian._assign); n = 65 reaches no call at all"""
    est, scramble = TG.gapped(2, 4, 3, 130, 65)
    want = longform._stitch_composed(est, 65, 300)
    assert emu.calls == {"cost": 0, "assign": 1, "chain": 0, "ola": 0}
    got = stitch(est.float(), 65, 300)
    assert emu.calls == {"cost": 1, "assign": 2, "chain": 1, "ola": 1}
    assert torch.equal(got[1], want[1]) and (got[0].double() - want[0]).abs().max() <= 1e-6 * est.abs().max() and got[0].dtype == torch.float32
    assert (got[2] - want[2]).abs().max() <= 1e-12 * want[2].max()
    out, perm_abs, boundary = stitch(est.float()[:, :1].contiguous(), 65, 100)           # one window: no boundary, no cost and no matching
    assert emu.calls == {"cost": 1, "assign": 2, "chain": 2, "ola": 2} and tuple(boundary.shape) == (2, 0)
    assert torch.equal(stitch(est, 65, 300)[1], want[1])                                                      # fp64
    strided = torch.empty(2, 4, 3, 131)[..., :130].copy_(est)
    assert not strided.is_contiguous() and torch.equal(stitch(strided, 65, 300)[1], want[1])                  # a view with a pitch
    assert emu.calls == {"cost": 1, "assign": 4, "chain": 2, "ola": 2}
    big, big_scramble = TG.gapped(1, 3, 65, 16, 9)                                                            # n = 65: beyond the wavefront
    out, perm_abs, _ = stitch(big.float(), 9, 30)
    assert TG.undoes_the_scramble(perm_abs, big_scramble) and out.dtype == torch.float32
    assert emu.calls == {"cost": 1, "assign": 4, "chain": 2, "ola": 2}


def test_cpu_tensors_beside_the_hip_library_take_the_composed_route():
    """the product's own backend object: CPU tensors never reach a kernel"""
    assert sepkernels.backend().name == "hip"
    est, scramble = TG.gapped(2, 4, 3, 130, 65)
    out, perm_abs, _ = stitch(est.float(), 65, 300)
    assert out.dtype == torch.float32 and TG.undoes_the_scramble(perm_abs, scramble)
    with pytest.raises(sepkernels.SepKernelsError):
        sepkernels.HipBackend().stitch_chain(torch.zeros(1, 1, 2, dtype=torch.int64), torch.zeros(1, 2, 2, dtype=torch.int64), 1, 2, 2)


def test_composed_route_forms_the_costs_in_blocks(monkeypatch):
    est, _ = TG.gapped(2, 6, 3, 130, 65)
    whole = stitch(est, 65, 400)
    monkeypatch.setattr(longform, "_BLOCK_ELEMS", 2 * 2 * 9 * 65)            # two boundaries at a time
    blocks = stitch(est, 65, 400)
    assert all(torch.equal(a, b) for a, b in zip(whole, blocks))


# ------------------------------------------------------------------------------------------------------ (4) the header, the binding, the library's checks
def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "sepkernels.h")).read()
    assert "#define SEP_ABI_VERSION 23" in header
    lib = sepkernels.load()
    for name in ("sep_stitch_cost", "sep_stitch_chain", "sep_stitch_ola"):
        assert "int {}(".format(name) in header and name in sepkernels.SIGNATURES and hasattr(lib, name)
        assert lib.sep_seq_lookup(name.encode()) >= 0
        assert hasattr(sepkernels.HipBackend, name[4:])
    import utils.longform
    from models.conv_tasnet import ConvTasNet
    assert utils.longform.stitch is stitch and utils.longform.separate_long is separate_long and callable(ConvTasNet.separate_long)


def test_library_argument_checks_precede_the_launch():
    """no launch happens here: each call fails its own checks before any HIP call (the pointers are never followed)"""
    lib = sepkernels.load()
    p = 1 << 12
    for args, words in (((None, p, 1, 2, 2, 8, 4), b"null pointer"), ((p, None, 1, 2, 2, 8, 4), b"null pointer"), ((p, p, 1, 2, 2, 8, 3), b"bad arguments"),
                        ((p, p, 1, 2, 2, 8, 8), b"bad arguments"), ((p, p, 1, 2, 65, 8, 4), b"bad arguments"), ((p, p, 1, 2, 0, 8, 4), b"bad arguments"),
                        ((p, p, 0, 2, 2, 8, 4), b"bad arguments"), ((p, p, 1, 0, 2, 8, 4), b"bad arguments"), ((p, p, 1, 2, 2, 1, 1), b"bad arguments"),
                        ((p, p, 1 << 20, 1 << 20, 2, 8, 4), b"bad arguments")):
        assert lib.sep_stitch_cost(*args, None) < 0
        assert b"sep_stitch_cost" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    assert lib.sep_stitch_cost(p, None, 1, 1, 2, 8, 4, None) == 0              # one window: no boundary, nothing is launched
    for args, words in (((p, None, 1, 2, 2), b"null pointer"), ((None, p, 1, 2, 2), b"null pointer"), ((p, p, 1, 2, 65), b"bad arguments"),
                        ((p, p, 1, 2, 0), b"bad arguments"), ((p, p, 0, 2, 2), b"bad arguments"), ((p, p, 1, 0, 2), b"bad arguments")):
        assert lib.sep_stitch_chain(*args, None) < 0
        assert b"sep_stitch_chain" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    for args, words in (((None, p, p, 1, 2, 2, 8, 4, 12), b"null pointer"), ((p, None, p, 1, 2, 2, 8, 4, 12), b"null pointer"), ((p, p, None, 1, 2, 2, 8, 4, 12), b"null pointer"),
                        ((p, p, p, 1, 2, 2, 8, 4, 13), b"bad arguments"), ((p, p, p, 1, 2, 2, 8, 4, 0), b"bad arguments"), ((p, p, p, 1, 2, 2, 8, 3, 8), b"bad arguments"),
                        ((p, p, p, 1, 2, 2, 8, 8, 8), b"bad arguments"), ((p, p, p, 1, 2, 65, 8, 4, 8), b"bad arguments"), ((p, p, p, 70000, 2, 2, 8, 4, 8), b"bad arguments")):
        assert lib.sep_stitch_ola(*args, None) < 0
        assert b"sep_stitch_ola" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()


# ------------------------------------------------------------------------------------------------------ (5) the kernel sources on the host
@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim_stitch.build_library(str(tmp_path_factory.mktemp("hostsim_stitch")))


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
@pytest.mark.parametrize("win,hop", TG.ALL_GEOMS, ids=TG.GEOM_IDS)
@pytest.mark.parametrize("n", TG.COST_N)
def test_stitch_cost_kernel_source_on_the_host(on_host, n, win, hop):
    """one host thread per lane, a workgroup per (boundary, 8 x 8 tile): n = 64 is 64 workgroups per boundary and runs at one batch of two
    boundaries here; the device runs every (B, W) of the case at every n"""
    if n == 64:
        TG.case_cost(2, 2, n, win, hop)
    else:
        TG.test_stitch_cost(n, win, hop)


@needs_clang
def test_stitch_cost_alignment_and_refusals_on_the_host(on_host):
    TG.test_stitch_cost_off_the_16_byte_alignment()
    TG.case_refusals()


@needs_clang
@pytest.mark.parametrize("W", [1, 2, 300])
@pytest.mark.parametrize("n", [1, 2, 64])
def test_stitch_chain_kernel_source_on_the_host(on_host, n, W):
    TG.test_stitch_chain(n, W)


@needs_clang
@pytest.mark.parametrize("win,hop", TG.ALL_GEOMS, ids=TG.GEOM_IDS)
def test_stitch_ola_kernel_source_on_the_host(on_host, win, hop):
    TG.test_stitch_ola(win, hop)


@needs_clang
def test_stitch_ola_alignment_and_bad_entries_on_the_host(on_host):
    TG.test_stitch_ola_off_the_16_byte_alignment()
    TG.test_stitch_ola_reads_a_bad_entry_as_row_zero()


@needs_clang
def test_the_kernel_comparison_is_not_vacuous(on_host):
    """the same cases fail when the device side computes something else: the other end of the window, a chain composed the other way round,
    tracks taken from the wrong rows"""
    class Skewed:
        def __getattr__(self, name):
            return getattr(on_host, name)

        def stitch_cost(self, est, *rest):
            return on_host.stitch_cost(est.flip(3).contiguous(), *rest)

        def stitch_chain(self, perm_local, perm_abs, B, W, n):
            on_host.stitch_chain(perm_local, perm_abs, B, W, n)
            perm_abs.copy_(perm_abs.argsort(2))

        def stitch_ola(self, est, perm_abs, out, B, W, n, win, hop, T):
            on_host.stitch_ola(est, perm_abs.flip(2).contiguous(), out, B, W, n, win, hop, T)
    TG.HIP = Skewed()
    with pytest.raises(AssertionError):
        TG.case_cost(1, 2, 3, 130, 65)
    with pytest.raises(AssertionError):
        TG.case_chain(1, 5, 4)
    with pytest.raises(AssertionError):
        TG.case_ola(1, 3, 3, 130, 65)


@needs_clang
def test_stitch_through_the_kernel_sources(on_host):
    """sepkernels/longform.py end to end with the host simulation of the kernels behind the binding (sep_assign among them), against the
    composed route"""
    class Named:
        name = "hostsim"

        def __getattr__(self, attr):
            return getattr(on_host, attr)
    old = sepkernels._set_backend_for_tests(Named())
    try:
        TG.case_stitch(2, 4, 2, 1100, 571, 3 * 571 + 1100 - 37)
        TG.case_stitch(1, 7, 5, 128, 64, 6 * 64 + 128)
        TG.case_stitch(1, 3, 20, 130, 65, 2 * 65 + 129)
    finally:
        sepkernels._set_backend_for_tests(old)


@needs_clang
def test_stand_alone_program_under_the_address_and_undefined_sanitizers():
    """tools/hostsim/stitch_main.cpp + the kernel sources, built with -fsanitize=address,undefined into a program of its own and run: the three
    kernels over the window geometries of the tests on exactly-sized buffers against plain double loops, the four launches in a row, zero reports"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostsim_stitch.py"), "--asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "70 cases, 0 mismatches" in r.stdout and "sanitizer reports: 0" in r.stdout, r.stdout[-3000:]


# ------------------------------------------------------------------------------------------------------ (6) the command line and the tester
SR = 8000
TINY = dict(n_basis=16, kernel_size=4, stride=2, enc_basis="trainable", dec_basis="trainable", enc_nonlinear=None, causal=False, sep_hidden_channels=32,
            sep_bottleneck_channels=16, sep_skip_channels=16, sep_kernel_size=3, sep_num_blocks=1, sep_num_layers=2, n_sources=2)


def test_the_separate_command_writes_one_wav_per_source(tmp_path):
    from models.conv_tasnet import ConvTasNet
    from recipes import audio_io
    torch.manual_seed(3)
    model = ConvTasNet(**TINY)
    package = model.get_config()
    package["state_dict"] = model.state_dict()
    torch.save(package, str(tmp_path / "model.pth"))
    window = 400                                                             # 0.05 s at 8 kHz
    x = 0.2 * torch.randn(1, 1000, generator=torch.Generator().manual_seed(4))      # 2.5 windows
    audio_io.write_wav(str(tmp_path / "meeting.wav"), x, SR)
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([SRC, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", "recipes.separate", "--model_path", str(tmp_path / "model.pth"), "--input", str(tmp_path / "meeting.wav"),
                        "--out_dir", str(tmp_path / "out"), "--window_s", "0.05", "--use_cuda", "0"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    read, _ = audio_io.read_wav(str(tmp_path / "meeting.wav"))
    model.eval()
    want = separate_long(model, read, window)
    for k in range(2):
        got, sr = audio_io.read_wav(str(tmp_path / "out" / "meeting_{}.wav".format(k + 1)))
        assert sr == SR and tuple(got.shape) == (1, 1000)
        assert (got[0] - want[k].clamp(-1, 1)).abs().max().item() <= 1.0 / 32768
    assert not os.path.exists(str(tmp_path / "out" / "meeting_3.wav"))


def test_tester_with_and_without_the_long_form_window(tmp_path, capsys):
    from criterion.pit import PIT1d
    from criterion.sdr import NegSISDR
    from models.conv_tasnet import ConvTasNet
    from recipes import audio_io
    from recipes.trainer import Tester
    from recipes.wsj0mix import TestDataLoader, WaveTestDataset
    g = torch.Generator().manual_seed(7)
    root = tmp_path / "wav"
    for sub in ("mix", "s1", "s2"):
        (root / sub).mkdir(parents=True)
    lengths = {"long": 1000, "short": 300}
    for ID, T in lengths.items():
        s = 0.2 * torch.randn(2, T, generator=g)
        audio_io.write_wav(str(root / "s1" / (ID + ".wav")), s[0], SR)
        audio_io.write_wav(str(root / "s2" / (ID + ".wav")), s[1], SR)
        audio_io.write_wav(str(root / "mix" / (ID + ".wav")), s.sum(0), SR)
    (tmp_path / "list.txt").write_text("\n".join(lengths) + "\n")
    torch.manual_seed(2)
    model = ConvTasNet(**TINY)
    criterion = PIT1d(NegSISDR(), n_sources=2)

    def run(**extra):
        loader = TestDataLoader(WaveTestDataset(str(root), str(tmp_path / "list.txt"), n_sources=2), batch_size=1)
        res = Tester(model, loader, criterion, argparse.Namespace(sample_rate=SR, n_sources=2, out_dir=None, model_path=None, **extra)).run()
        return res, capsys.readouterr().out

    plain, plain_rows = run()
    unset, unset_rows = run(long_form_window=None, long_form_hop=None)
    assert unset == plain and unset_rows == plain_rows                       # unset: exactly what it returns today
    res, rows = run(long_form_window=400, long_form_hop=200)
    assert set(res) == set(plain) and all(math.isfinite(v) for v in res.values())
    assert rows.splitlines()[2] == plain_rows.splitlines()[2] and rows.splitlines()[1] != plain_rows.splitlines()[1]       # `short` is one forward, `long` is not

    seen = []
    hook = model.register_forward_hook(lambda m, inp, out: seen.append(inp[0].shape[-1]))
    run(long_form_window=400)
    hook.remove()
    assert seen.count(400) >= 1 and 1000 not in seen and 300 in seen
