"""Development tool: the BSS-eval kernels (csrc/loss.hip: sep_bss_xcorr, sep_bss_energies) compiled for the host (tools/hostsim.py::host_copy,
the stand-in HIP header of tools/hostsim/include) and linked with tools/hostsim/bss_main.cpp into ONE PROGRAM that runs the kernel cases of
tests/test_bss_eval_gpu.py on exactly-sized buffers against plain double loops.  With --asan the program is built with
-fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no Python is involved in the run): reads beyond a row's
length or the buffers' ends, writes beyond the scratch, undefined arithmetic.

    python tools/hostsim_bss.py [--asan]

build_library(workdir) gives tests/test_bss_eval_cpu.py a host-simulation library of csrc/loss.hip and csrc/runtime.hip alone (a few seconds instead of the
minute the whole of csrc/ takes)."""
import os
import subprocess
import sys
import tempfile

import hostsim

HOSTSIM_DIR = os.path.join(hostsim.ROOT, "tools", "hostsim")


def _sources(d):
    """the host copies of loss.hip (the kernels) and runtime.hip (the library's error slot) in `d`, plus the simulation's runtime"""
    out = []
    for f in ("loss", "runtime"):
        out.append(os.path.join(d, f + ".cpp"))
        open(out[-1], "w").write(hostsim.host_copy(f + ".hip"))
    return out + [os.path.join(HOSTSIM_DIR, "sim_main.cpp")]


def _includes(d):
    return ["-I", d, "-I", os.path.join(HOSTSIM_DIR, "include"), "-I", hostsim.CSRC, "-I", os.path.join(hostsim.ROOT, "include")]


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/loss.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    cxx = hostsim.compiler()
    if cxx is None:
        raise RuntimeError("hostsim needs clang++")
    so = os.path.join(workdir, "libsepkernels_hostsim_loss.so")
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
        exe = os.path.join(d, "bss_host")
        subprocess.check_call([cxx] + flags + _includes(d) + _sources(d) + [os.path.join(HOSTSIM_DIR, "bss_main.cpp"), "-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        r = subprocess.run([exe], env=env, capture_output=True, text=True)
    markers = ("ERROR: AddressSanitizer", "runtime error:") if kind else ()
    reports = sum(r.stderr.count(mk) for mk in markers)
    print(r.stdout[-3000:])
    if reports or r.returncode:
        print(r.stderr[-6000:])
    print("{}: exit status {}, sanitizer reports: {}".format(kind or "plain", r.returncode, reports))
    return 1 if reports or r.returncode else 0


if __name__ == "__main__":
    raise SystemExit(main())
