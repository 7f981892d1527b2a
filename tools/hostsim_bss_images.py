"""Development tool: the BSS-eval v4 ("images") kernel (csrc/loss.hip: sep_bss_image_energies) compiled for the host (tools/hostsim.py::host_copy,
the stand-in HIP header of tools/hostsim/include) and linked with tools/hostsim/bss_images_main.cpp into ONE PROGRAM that runs the shapes of
tests/test_bss_images_gpu.py on exactly-sized buffers against plain double loops.  With --asan the program is built with
-fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no Python is involved in the run): reads beyond a row's
length, a frame's end or the buffers' ends, writes beyond the scratch, undefined arithmetic.

    python tools/hostsim_bss_images.py [--asan]

The host-simulation library for tests/test_bss_images_cpu.py is tools/hostsim_bss.py::build_library (csrc/loss.hip and csrc/runtime.hip alone)."""
import os
import subprocess
import sys
import tempfile

import hostsim
import hostsim_bss

CASES = 6                      # what bss_images_main.cpp runs: the five shapes and the refused calls


def main():
    kind = "address,undefined" if "--asan" in sys.argv else None
    cxx = hostsim.compiler()
    if cxx is None:
        print("needs clang++")
        return 1
    flags = ["-std=c++17", "-O1", "-pthread"] + (["-g", "-fsanitize=" + kind, "-fno-omit-frame-pointer"] if kind else [])
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "bss_images_host")
        subprocess.check_call([cxx] + flags + hostsim_bss._includes(d) + hostsim_bss._sources(d) + [os.path.join(hostsim_bss.HOSTSIM_DIR, "bss_images_main.cpp"), "-o", exe])
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
