"""CPU: sample-rate conversion -- sepkernels/resample.py (resample, Resample, StreamResampler), csrc/resample.hip: sep_resample_fwd /
sep_resample_stream_fwd, the torchaudio stand-in of recipes/audio_io.py, `python -m recipes.separate --model_rate`.

(1) the composed route against the numpy fp64 oracle of tests/test_resample_gpu.py: fp64 within 1e-12 of sum |h| |x|, fp32 within the derived bound
    with K taps; the filter against the issue's table; Kaiser; the old method name; gradients; streams on the composed route.
(2) the module object, the shim.   (3) the header and the binding; the library's own argument checks.
(4) the kernel SOURCE on the host (tools/hostsim_resample.py): the kernel cases of tests/test_resample_gpu.py, and the stand-alone program built
    with -fsanitize=address,undefined and run as a program.
(5) the command line with and without --model_rate.
Without the feature `import sepkernels.resample` fails: every test here fails."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sepkernels
import test_resample_gpu as TG
from sepkernels import resample as RS
from sepkernels.resample import Resample, StreamResampler, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "dnn-based_source_separation_amd", "src")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                         # noqa: E402
import hostsim_resample                # noqa: E402

needs_clang = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++")
ALL_PAIRS = TG.PAIRS
STREAM_IDS = ["{}-{}".format(*p) for p in TG.STREAM_PAIRS]


# ------------------------------------------------------------------------------------------------------ (1) the composed route against the oracle
@pytest.mark.parametrize("orig,new", ALL_PAIRS, ids=TG.PAIR_IDS)
def test_filter_is_the_definition_and_the_compact_table_its_core(orig, new):
    orc, flt = TG.oracle_of(orig, new), RS.get_filter(orig, new)
    assert (flt.o, flt.u, flt.width, flt.K, flt.Kc, flt.D, flt.H) == (orc.o, orc.u, orc.width, orc.K, orc.Kc, orc.D, orc.H)
    if (orig, new) in TG.KNOWN:
        assert (flt.o, flt.u, flt.width, flt.K, flt.Kc) == TG.KNOWN[(orig, new)]
    assert np.abs(flt.h.numpy() - orc.h).max() <= 1e-15
    gain = flt.h.sum(1)
    assert 1.00003 <= gain.min().item() and gain.max().item() <= 1.001                   # the DC gain of every phase (1.00004 .. 1.0009)
    first = flt.first.long()
    assert tuple(flt.table.shape) == (flt.Kc, flt.u) and first.min() >= 0 and (first + flt.Kc).max() <= flt.K
    cols = first.view(-1, 1) + torch.arange(flt.Kc).view(1, -1)
    assert torch.equal(flt.table, flt.h.gather(1, cols).t().float())
    left = flt.h.clone().scatter_(1, cols, 0.0).abs().amax(1)                              # what the compact table leaves out
    assert (left <= 2.0 ** -60 * flt.h.abs().amax(1)).all()
    assert (first <= torch.from_numpy(orc.lo)).all() and (first + flt.Kc - 1 >= torch.from_numpy(orc.hi)).all()


@pytest.mark.parametrize("orig,new", ALL_PAIRS, ids=TG.PAIR_IDS)
def test_composed_route_against_the_oracle(orig, new):
    orc = TG.oracle_of(orig, new)
    for T in TG.lengths_of(orc)[:-1]:
        for R in (1, 3):
            x = TG.signal(R, T, T)
            ref, mag, drop = orc(x.double().numpy())
            y = resample(x.double(), orig, new)
            assert y.dtype == torch.float64 and tuple(y.shape) == ref.shape
            assert (np.abs(y.numpy() - ref) <= 1e-12 * mag + 1e-300).all(), (orig, new, R, T)
            TG.within(resample(x, orig, new), x, orc, orc.K, "composed fp32 {} -> {} R {} T {}".format(orig, new, R, T))


def test_a_sine_comes_back_as_the_filter_allows():
    """1 kHz from 16 k to 8 k: within 1.4e-4 of the analytic sine away from the edges -- a property of the filter, not an error"""
    t = torch.arange(16000, dtype=torch.float64)
    y = resample(torch.sin(2 * np.pi * 1000 * t / 16000), 16000, 8000)
    want = torch.sin(2 * np.pi * 1000 * torch.arange(8000, dtype=torch.float64) / 8000)
    err = (y - want)[100:-100].abs().max().item()
    assert 1e-6 < err <= 1.4e-4 * 1.05, err


def test_kaiser_window_old_method_name_and_arguments():
    x = torch.randn(2, 300, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    assert torch.equal(resample(x, 16000, 8000, resampling_method="sinc_interpolation"), resample(x, 16000, 8000))
    flt = RS.get_filter(16000, 8000, resampling_method="sinc_interp_kaiser")
    o, lpw, base, beta = 2, 6, 0.99, 14.769656459379492
    t = np.clip((np.arange(flt.K) - flt.width) / o * base, -lpw, lpw)
    safe = np.where(t == 0, 1.0, t)
    want = np.where(t == 0, 1.0, np.sin(np.pi * safe) / (np.pi * safe)) * np.i0(beta * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(beta) * base / o
    assert np.abs(flt.h[0].numpy() - want).max() <= 1e-12 and flt.Kc <= flt.K
    y = resample(x, 16000, 8000, resampling_method="sinc_interp_kaiser", beta=9.0)
    assert tuple(y.shape) == (2, 150) and not torch.equal(y, resample(x, 16000, 8000))
    wide = RS.get_filter(16000, 8000, lowpass_filter_width=16, rolloff=0.9)
    assert wide.width == int(np.ceil(16 * 2 / 0.9)) and wide.Kc > RS.get_filter(16000, 8000).Kc
    for bad in (dict(orig_freq=0, new_freq=8000), dict(orig_freq=16000.5, new_freq=8000), dict(orig_freq=2, new_freq=1, resampling_method="linear"),
                dict(orig_freq=2, new_freq=1, lowpass_filter_width=0)):
        with pytest.raises(ValueError):
            resample(x, **bad)
    with pytest.raises(ValueError, match="floating-point"):
        resample(torch.zeros(4, dtype=torch.int16), 2, 1)
    assert resample(x, 8000, 8000) is x and resample(x[:, :0], 2, 1).shape == (2, 0)


def test_gradients_flow_through_the_composed_route():
    x = torch.randn(2, 40, dtype=torch.float64, requires_grad=True, generator=torch.Generator().manual_seed(1))
    assert torch.autograd.gradcheck(lambda v: resample(v, 3, 2), (x,))
    y = Resample(8000, 16000)(x.detach().float().requires_grad_())
    assert y.requires_grad and y.shape == (2, 80)


@pytest.mark.parametrize("orig,new", TG.STREAM_PAIRS, ids=STREAM_IDS)
def test_streams_on_the_composed_route_equal_the_padded_signal(orig, new):
    """fp64 on the CPU: chunks of m = 1 where H > o among them; equality to resample(pad(x, (D, 0))) within the rounding of one more summation order"""
    orc = TG.oracle_of(orig, new)
    for plan in TG.plans_of(orig, new):
        x = TG.signal(3, sum(plan) * orc.o, 3).double()
        rs = StreamResampler(3, orig, new, dtype=torch.float64)
        got = TG.stream_through(rs, x, plan)
        want = resample(F.pad(x, (orc.D, 0)), orig, new)
        _, mag, _ = orc(F.pad(x, (orc.D, 0)).numpy())
        assert got.shape == want.shape and (np.abs((got - want).numpy()) <= 1e-12 * mag + 1e-300).all()
        assert rs.delay == orc.D and rs.state_bytes == 8 * 3 * orc.H and not rs.history.any()
    same = StreamResampler(2, 8000, 8000)
    chunk = torch.randn(2, 5)
    assert torch.equal(same(chunk), chunk) and same.delay == 0 and same.state_bytes == 0 and same.flush().shape == (2, 0)


def test_cpu_tensors_beside_the_hip_library_take_the_composed_route():
    """the product's own backend object: CPU tensors never reach a kernel, and the binding refuses them loudly"""
    assert sepkernels.backend().name == "hip"
    x = TG.signal(3, 200, 2)
    TG.within(resample(x, 48000, 44100), x, TG.oracle_of(48000, 44100), TG.oracle_of(48000, 44100).K, "CPU fp32")
    rs = StreamResampler(3, 48000, 44100)
    assert torch.equal(rs(x[:, :160]), resample(F.pad(x[:, :160], (160, 0)), 48000, 44100)[:, :147])
    flt = RS.get_filter(16000, 8000)
    with pytest.raises(sepkernels.SepKernelsError):
        sepkernels.HipBackend().resample_fwd(torch.zeros(1, 8), 8, flt.table, flt.first, torch.zeros(1, 4), 4, 1, 8, 4, 2, 1, 13, 25)


# ------------------------------------------------------------------------------------------------------ (2) the module object, the shim
def test_resample_module_has_no_parameters_and_no_state():
    m = Resample(16000, 8000)
    assert list(m.parameters()) == [] and list(m.buffers()) == [] and m.state_dict() == {}
    assert m._filter is Resample(16000, 8000)._filter and m._filter.on(torch.device("cpu")) is m._filter.on(torch.device("cpu"))      # one table, one upload
    assert "orig_freq=16000" in repr(m)
    x = torch.randn(2, 1, 100)
    assert torch.equal(m(x), resample(x, 16000, 8000)) and Resample(8000, 8000)(x) is x
    assert Resample(44100, 8000, "sinc_interp_kaiser", 6, 0.99, None)(x).shape == (2, 1, 19)
    import utils.resample
    assert utils.resample.resample is resample and utils.resample.Resample is Resample and utils.resample.StreamResampler is StreamResampler


def test_torchaudio_shim_offers_resample():
    code = ("import sys; sys.path[:0] = [{!r}, {!r}]\n"
            "try:\n    import torchaudio\n    print('REAL')\nexcept ImportError:\n"
            "    from recipes.audio_io import install_torchaudio_shim\n    assert install_torchaudio_shim()\n"
            "    import torch, torchaudio, torchaudio.transforms, torchaudio.functional\n    from sepkernels.resample import Resample, resample\n"
            "    assert torchaudio.transforms.Resample is Resample and torchaudio.functional.resample is resample\n"
            "    from torchaudio.transforms import Resample as R2\n"
            "    y = R2(44100, 8000)(torch.zeros(2, 441))\n    assert y.shape == (2, 80) and callable(torchaudio.load) and callable(torchaudio.info)\n"
            "    print('SHIM')\n").format(SRC, ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() in ("SHIM", "REAL"), r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------------ (3) the header, the binding, the library's checks
def test_header_and_binding():
    header = open(os.path.join(ROOT, "include", "sepkernels.h")).read()
    assert "#define SEP_ABI_VERSION 23" in header and "#define SEP_RESAMPLE_MAX_HISTORY 2048" in header
    lib = sepkernels.load()
    for name in ("sep_resample_fwd", "sep_resample_stream_fwd"):
        assert "int {}(".format(name) in header and name in sepkernels.SIGNATURES and hasattr(lib, name)
        assert lib.sep_seq_lookup(name.encode()) >= 0
        assert hasattr(sepkernels.HipBackend, name[4:])


def test_library_argument_checks_precede_the_launch():
    """no launch happens here: each call fails its own checks before any HIP call (the pointers are never followed)"""
    lib = sepkernels.load()
    p = 1 << 12
    ok = (p, 8, p, p, p, 4, 1, 8, 4, 2, 1, 13, 25)

    def fwd(**change):
        names = ("x", "x_pitch", "table", "first", "y", "y_pitch", "R", "T", "T_out", "o", "u", "width", "Kc")
        return [change.get(n, v) for n, v in zip(names, ok)]
    for args, words in ((fwd(x=None), b"null pointer"), (fwd(table=None), b"null pointer"), (fwd(first=None), b"null pointer"), (fwd(y=None), b"null pointer"),
                        (fwd(T_out=5, y_pitch=5), b"T_out = ceil"), (fwd(x_pitch=7), b"bad arguments"), (fwd(y_pitch=3), b"bad arguments"), (fwd(R=0), b"bad arguments"),
                        (fwd(T=0, T_out=0), b"bad arguments"), (fwd(Kc=29), b"Kc exceeds"), (fwd(Kc=0), b"refused"), (fwd(o=0), b"refused"), (fwd(u=0), b"refused"),
                        (fwd(width=4096), b"staged span"), (fwd(u=1025, T_out=4100, y_pitch=4100, Kc=5), b"more phases"),
                        (fwd(u=1000, T_out=4000, y_pitch=4000, Kc=7), b"exceeds the kernels' LDS"), (fwd(R=1 << 30, T=1 << 30, x_pitch=1 << 30, T_out=1 << 29, y_pitch=1 << 29), b"tiles")):
        assert lib.sep_resample_fwd(*args, None) < 0
        assert b"sep_resample_fwd" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    good = (p, p, p, p, p, None, 1, 1, 2, 2, 1, 13, 25)

    def stream(**change):
        names = ("chunk", "table", "first", "history", "y", "slots", "A", "num_streams", "m", "o", "u", "width", "Kc")
        return [change.get(n, v) for n, v in zip(names, good)]
    for args, words in ((stream(chunk=None), b"null pointer"), (stream(history=None), b"null pointer"), (stream(y=None), b"null pointer"),
                        (stream(num_streams=2), b"bad arguments"), (stream(A=2), b"bad arguments"), (stream(m=0), b"bad arguments"), (stream(A=0), b"bad arguments"),
                        (stream(Kc=29), b"Kc exceeds"), (stream(o=2000, width=1500), b"history of 3500"), (stream(o=1, u=1000, width=7, Kc=6, m=5), b"shorter than the history")):
        assert lib.sep_resample_stream_fwd(*args, None) < 0
        assert b"sep_resample_stream_fwd" in lib.sep_last_error() and words in lib.sep_last_error(), lib.sep_last_error()
    for flt in (RS.get_filter(*pair) for pair in ALL_PAIRS):          # what the module believes the kernels take is what they take
        assert flt.kernels_take_it() and flt.kernels_take_a_stream(1) and flt.kernels_take_a_stream(10 ** 6)
    big = RS.get_filter(1, 400)                                            # tiles of 5 frames, a history of 14 samples
    assert big.kernels_take_it() and big.kernels_take_a_stream(5) and not big.kernels_take_a_stream(6)
    assert not RS.get_filter(1023, 1024).kernels_take_it() and not RS.get_filter(1025, 1).kernels_take_it()
    x = torch.randn(1, 3000, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    assert resample(x, 1025, 1).shape == (1, 3)                            # ... and what they refuse is composed


# ------------------------------------------------------------------------------------------------------ (4) the kernel source on the host
@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim_resample.build_library(str(tmp_path_factory.mktemp("hostsim_resample")))


@pytest.fixture()
def on_host(sim_library):
    """the hooks of tests/test_resample_gpu.py and the package's backend on the host simulation of csrc/resample.hip"""
    saved = (TG.HIP, TG.to_device, TG.device_sync)
    with hostsim.HostSimBackend(sim_library) as K:
        class Named:
            name = "hostsim"

            def __getattr__(self, attr):
                return getattr(K, attr)
        TG.HIP, TG.to_device, TG.device_sync = K, (lambda t: t.clone()), (lambda: None)
        old = sepkernels._set_backend_for_tests(Named())
        try:
            yield K
        finally:
            sepkernels._set_backend_for_tests(old)
            TG.HIP, TG.to_device, TG.device_sync = saved


@needs_clang
@pytest.mark.parametrize("orig,new", ALL_PAIRS, ids=TG.PAIR_IDS)
def test_offline_kernel_source_on_the_host(on_host, orig, new):
    TG.test_offline_kernel_against_the_oracle(orig, new)


@needs_clang
def test_module_shapes_impulses_and_instances_on_the_host(on_host):
    for pair in ((16000, 8000), (2, 3), (44100, 16000)):
        TG.case_shapes(*pair)
        TG.case_strided_view(*pair)
    for pair in ALL_PAIRS:
        TG.case_impulse(*pair)
    TG.case_instances()


@needs_clang
@pytest.mark.parametrize("num_streams", [1, 3])
@pytest.mark.parametrize("orig,new", TG.STREAM_PAIRS, ids=STREAM_IDS)
def test_stream_kernel_source_on_the_host(on_host, orig, new, num_streams):
    TG.test_streams_against_the_oracle_and_the_offline_call(orig, new, num_streams)


@needs_clang
def test_subsets_and_long_chunks_on_the_host(on_host):
    TG.case_subsets(16000, 8000)
    TG.case_subsets(48000, 44100)
    TG.case_stream_of_many_tiles()


@needs_clang
def test_the_kernel_comparison_is_not_vacuous(on_host):
    """the same cases fail when the device side computes something else: a table shifted by one tap, a history that is not carried"""
    class Skewed:
        def __getattr__(self, name):
            return getattr(on_host, name)

        def resample_fwd(self, x, x_pitch, table, first, *rest):
            return on_host.resample_fwd(x, x_pitch, table, (first + 1).contiguous(), *rest)

        def resample_stream_fwd(self, chunk, table, first, history, *rest):
            on_host.resample_stream_fwd(chunk, table, first, history, *rest)
            history.zero_()
    TG.HIP = Skewed()
    with pytest.raises(AssertionError):
        TG.case_offline(16000, 8000, 1, 40)
    Skewed.name = "hostsim"
    sepkernels._set_backend_for_tests(Skewed())
    with pytest.raises(AssertionError):
        TG.case_impulse(44100, 8000)
    with pytest.raises(AssertionError):
        TG.case_stream(16000, 8000, 1, [1, 3, 7, 29])


@needs_clang
def test_stand_alone_program_under_the_address_and_undefined_sanitizers():
    """tools/hostsim/resample_main.cpp + the kernel source, built with -fsanitize=address,undefined into a program of its own and run: both kernels
    over the rate pairs and lengths of the tests on exactly-sized buffers against plain double loops, zero reports"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "hostsim_resample.py"), "--asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "88 cases, 0 mismatches" in r.stdout and "sanitizer reports: 0" in r.stdout, r.stdout[-3000:]


# ------------------------------------------------------------------------------------------------------ (5) the command line
TINY = dict(n_basis=16, kernel_size=4, stride=2, enc_basis="trainable", dec_basis="trainable", enc_nonlinear=None, causal=False, sep_hidden_channels=32,
            sep_bottleneck_channels=16, sep_skip_channels=16, sep_kernel_size=3, sep_num_blocks=1, sep_num_layers=2, n_sources=2)


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    from models.conv_tasnet import ConvTasNet
    torch.manual_seed(3)
    model = ConvTasNet(**TINY)
    package = model.get_config()
    package["state_dict"] = model.state_dict()
    path = str(tmp_path_factory.mktemp("ckpt") / "model.pth")
    torch.save(package, path)
    return model.eval(), path


def _separate(tmp_path, path, wav, out, *extra):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([SRC, ROOT, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-m", "recipes.separate", "--model_path", path, "--input", str(tmp_path / wav), "--out_dir", str(tmp_path / out),
                        "--window_s", "0.05", "--use_cuda", "0"] + list(extra), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


def test_separate_with_a_model_rate_resamples_in_and_out(tmp_path, checkpoint):
    """a 16 kHz wav through an 8 kHz checkpoint: the outputs have the input's length and rate and equal resample -> separate_long -> resample by hand"""
    from recipes import audio_io
    from sepkernels.longform import separate_long
    model, path = checkpoint
    x = 0.2 * torch.randn(1, 2001, generator=torch.Generator().manual_seed(4))
    audio_io.write_wav(str(tmp_path / "talk.wav"), x, 16000)
    _separate(tmp_path, path, "talk.wav", "out", "--model_rate", "8000")
    read, sr = audio_io.read_wav(str(tmp_path / "talk.wav"))
    assert sr == 16000
    low = resample(read, 16000, 8000)
    est = separate_long(model, low, 400)                                     # 0.05 s at the MODEL's rate
    assert low.shape[-1] == 1001 and est.shape[-1] == 1001
    back = resample(est.contiguous(), 8000, 16000)
    assert back.shape[-1] == 2002                                            # one more than the input: cropped
    for k in range(2):
        got, sr = audio_io.read_wav(str(tmp_path / "out" / "talk_{}.wav".format(k + 1)))
        assert sr == 16000 and tuple(got.shape) == (1, 2001)
        assert (got[0] - back[k, :2001].clamp(-1, 1)).abs().max().item() <= 1.0 / 32768
    audio_io.write_wav(str(tmp_path / "odd.wav"), x[:, :1999], 16000)       # 1999 at 16 k -> 1000 at 8 k -> 2000 at 16 k: cropped to 1999
    _separate(tmp_path, path, "odd.wav", "out", "--model_rate", "8000")
    assert audio_io.wav_info(str(tmp_path / "out" / "odd_1.wav"))[:3] == (1999, 1, 16000)
    audio_io.write_wav(str(tmp_path / "third.wav"), x[:, :1000], 12000)     # 1000 at 12 k -> 667 at 8 k -> 1001 at 12 k: cropped to 1000
    _separate(tmp_path, path, "third.wav", "out", "--model_rate", "8000")
    assert audio_io.wav_info(str(tmp_path / "out" / "third_2.wav"))[:3] == (1000, 1, 12000)


def test_separate_without_the_flag_writes_the_same_bytes_as_before(tmp_path, checkpoint):
    """the default is the command as it was: the wav goes to the model at its own rate, whatever that is, and the files are byte for byte those of
    the statements the command consisted of before the flag existed; --model_rate equal to the wav's rate is the same again"""
    from recipes import audio_io
    from sepkernels.longform import separate_long
    model, path = checkpoint
    x = 0.2 * torch.randn(1, 2001, generator=torch.Generator().manual_seed(6))
    audio_io.write_wav(str(tmp_path / "talk.wav"), x, 16000)
    _separate(tmp_path, path, "talk.wav", "plain")
    _separate(tmp_path, path, "talk.wav", "same", "--model_rate", "16000")
    mixture, sample_rate = audio_io.read_wav(str(tmp_path / "talk.wav"))
    window = int(round(0.05 * sample_rate))
    estimates = separate_long(model, mixture, window, hop=window // 2, batch_windows=16).cpu()
    for k, est in enumerate(estimates):
        audio_io.write_wav(str(tmp_path / "want.wav"), est, sample_rate, 16)
        want = open(str(tmp_path / "want.wav"), "rb").read()
        for out in ("plain", "same"):
            assert open(str(tmp_path / out / "talk_{}.wav".format(k + 1)), "rb").read() == want
