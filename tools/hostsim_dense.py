"""Development tool: the dilated unfold kernels (csrc/causal.hip, csrc/online.hip) compiled for the host (tools/hostsim.py::host_copy, the
stand-in HIP header of tools/hostsim/include) and linked with tools/hostsim/dense_tcn_main.cpp into ONE PROGRAM that runs the kernel cases of
tests/test_dense_tcn_gpu.py on exactly-sized buffers.  With --asan / --tsan the program is built under that sanitizer (its runtime linked
in; nothing is preloaded and no Python is involved in the run): out-of-bounds accesses of global buffers and LDS, and races between the
lanes of a workgroup (every lane is a host thread; only barriers order them).

    python tools/hostsim_dense.py [--asan | --tsan]
"""
import os
import subprocess
import sys
import tempfile

import hostsim

FILES = ("causal", "online", "runtime")     # runtime.hip holds the library's error slot (sep_set_error / sep_last_error)


def main():
    kind = "address" if "--asan" in sys.argv else "thread" if "--tsan" in sys.argv else None
    cxx = hostsim.compiler()
    if cxx is None:
        print("needs clang++")
        return 1
    inc = os.path.join(hostsim.ROOT, "tools", "hostsim", "include")
    flags = ["-std=c++17", "-O1", "-pthread"] + (["-g", "-fsanitize=" + kind, "-fno-omit-frame-pointer"] if kind else [])
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "gemm_common.hpp"), "w").write(hostsim.host_copy("gemm_common.hpp"))
        srcs = []
        for f in FILES:
            srcs.append(os.path.join(d, f + ".cpp"))
            open(srcs[-1], "w").write(hostsim.host_copy(f + ".hip"))
        srcs += [os.path.join(hostsim.ROOT, "tools", "hostsim", "sim_main.cpp"), os.path.join(hostsim.ROOT, "tools", "hostsim", "dense_tcn_main.cpp")]
        exe = os.path.join(d, "dense_tcn_host")
        subprocess.check_call([cxx] + flags + ["-I", d, "-I", inc, "-I", hostsim.CSRC, "-I", os.path.join(hostsim.ROOT, "include")] + srcs + ["-o", exe])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=0", TSAN_OPTIONS="halt_on_error=0 report_signal_unsafe=0")
        r = subprocess.run([exe], env=env, capture_output=True, text=True)
    marker = {"address": "ERROR: AddressSanitizer", "thread": "WARNING: ThreadSanitizer", None: "\0"}[kind]
    reports = r.stderr.count(marker)
    print(r.stdout[-3000:])
    if reports or r.returncode:
        print(r.stderr[-6000:])
    print("{}: exit status {}, sanitizer reports: {}".format(kind or "plain", r.returncode, reports))
    return 1 if reports or r.returncode else 0


if __name__ == "__main__":
    raise SystemExit(main())
