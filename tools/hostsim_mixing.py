"""Development tool: the dynamic-mixing kernels (csrc/mixing.hip: sep_mix_draw, sep_mix_render; csrc/runtime.hip beside them holds the library's
error slot and the kernel-name observable) compiled for the host (tools/hostsim.py::host_copy, the stand-in HIP header of tools/hostsim/include)
and linked with tools/hostsim/mixing_main.cpp into ONE PROGRAM that draws and renders the test corpus of tests/test_dynamic_mixing_gpu.py in both
sample kinds on exactly-sized buffers against the rule of include/sepkernels.h restated in plain loops -- and renders HOSTILE plans (an utterance
index out of range either way, start >= len, lead negative or >= T, NaN gains), which run only here and never on a device.  With --asan the
program is built with -fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no Python is involved in the run): a read
outside the corpus's storage, a write outside an output, undefined arithmetic on a hostile plan.

    python tools/hostsim_mixing.py [--asan] [--speed]

--speed builds and runs tools/hostsim/mixing_speed_main.cpp instead: the same for sep_mix_draw_speed and sep_mix_render_speed -- the speed cases against the
definition in plain loops, and hostile speed indices (out of range either way), start >= len', leads, a one-sample utterance and descriptor fields out
of bounds on exactly-sized filter buffers.

build_library(workdir) gives tests/test_dynamic_mixing_cpu.py a host-simulation library of csrc/mixing.hip and csrc/runtime.hip alone (the
recorded-sequence case there needs csrc/sequence.hip and with it every file: tools/hostsim.py::build)."""
import os
import subprocess
import sys
import tempfile

import hostsim
from hostsim_bss import HOSTSIM_DIR, _includes

FILES = ("mixing", "runtime")


def _sources(d):
    """the host copies of mixing.hip and runtime.hip in `d`, plus the simulation's runtime"""
    out = []
    for f in FILES:
        out.append(os.path.join(d, f + ".cpp"))
        open(out[-1], "w").write(hostsim.host_copy(f + ".hip"))
    return out + [os.path.join(HOSTSIM_DIR, "sim_main.cpp")]


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/mixing.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    cxx = hostsim.compiler()
    if cxx is None:
        raise RuntimeError("hostsim needs clang++")
    so = os.path.join(workdir, "libsepkernels_hostsim_mixing.so")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-fPIC", "-pthread", "-shared"] + _includes(workdir) + _sources(workdir) + ["-o", so])
    return so


def main():
    kind = "address,undefined" if "--asan" in sys.argv else None
    cxx = hostsim.compiler()
    if cxx is None:
        print("needs clang++")
        return 1
    flags = ["-std=c++17", "-O1", "-pthread"] + (["-g", "-fsanitize=" + kind, "-fno-omit-frame-pointer"] if kind else [])
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "mixing_host")
        driver = "mixing_speed_main.cpp" if "--speed" in sys.argv else "mixing_main.cpp"
        subprocess.check_call([cxx] + flags + _includes(d) + _sources(d) + [os.path.join(HOSTSIM_DIR, driver), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=900)
    markers = ("ERROR: AddressSanitizer", "runtime error:") if kind else ()
    reports = sum(r.stderr.count(mk) for mk in markers)
    print(r.stdout[-3000:])
    if reports or r.returncode:
        print(r.stderr[-6000:])
    print("{}: exit status {}, sanitizer reports: {}".format(kind or "plain", r.returncode, reports))
    return 1 if reports or r.returncode else 0


if __name__ == "__main__":
    raise SystemExit(main())
