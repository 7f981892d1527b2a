"""Development tool: the optimal-permutation kernels (csrc/loss.hip: sep_pair_gram, sep_assign, sep_pair_assign, sep_pair_bwd) compiled for the host
(tools/hostsim.py::host_copy, the stand-in HIP header of tools/hostsim/include) and linked with tools/hostsim/hungarian_main.cpp into ONE PROGRAM
that runs the four kernels at n in {1, 9, 64} and T in {1, 2 SEP_PAIR_SLAB + 17} on exactly-sized buffers against plain double loops and a
plain O(n^3) solver, matrices of NaN and +-Inf included.  With --asan the program is built with -fsanitize=address,undefined (the runtime is
linked in; nothing is preloaded and no Python is involved in the run): reads beyond a row's end, writes beyond the scratch or the outputs,
an index from a poisoned comparison, undefined arithmetic.

    python tools/hostsim_hungarian.py [--asan]

build_library(workdir) gives tests/test_hungarian_cpu.py a host-simulation library of csrc/loss.hip and csrc/runtime.hip alone."""
import os
import subprocess
import sys
import tempfile

import hostsim
from hostsim_bss import HOSTSIM_DIR, _includes, _sources, build_library      # noqa: F401  (the same translation units: csrc/loss.hip, csrc/runtime.hip)


def main():
    kind = "address,undefined" if "--asan" in sys.argv else None
    cxx = hostsim.compiler()
    if cxx is None:
        print("needs clang++")
        return 1
    flags = ["-std=c++17", "-O1", "-pthread"] + (["-g", "-fsanitize=" + kind, "-fno-omit-frame-pointer"] if kind else [])
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "hungarian_host")
        subprocess.check_call([cxx] + flags + _includes(d) + _sources(d) + [os.path.join(HOSTSIM_DIR, "hungarian_main.cpp"), "-o", exe])
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
