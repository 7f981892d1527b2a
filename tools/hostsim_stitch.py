"""Development tool: the stitching kernels (csrc/stitch.hip: sep_stitch_cost, sep_stitch_chain, sep_stitch_ola) and sep_assign beside them
(csrc/assign.hip; csrc/runtime.hip holds the library's error slot) compiled for the host (tools/hostsim.py::host_copy, the stand-in HIP header of
tools/hostsim/include) and linked with tools/hostsim/stitch_main.cpp into ONE PROGRAM that runs the three kernels over the window geometries of
tests/test_longform_gpu.py at n in {1, 3, 9, 20, 64} on exactly-sized buffers against plain double loops, and the four launches in a row on
scrambled windows.  With --asan the program is built with -fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no
Python is involved in the run): reads beyond a window's row or the overlap, writes beyond cost / perm_abs / out, an index from a bad
permutation entry, undefined arithmetic.

    python tools/hostsim_stitch.py [--asan]

build_library(workdir) gives tests/test_longform_cpu.py a host-simulation library of csrc/stitch.hip, csrc/assign.hip and csrc/runtime.hip alone."""
import sys

import hostsim

FILES = ("stitch", "assign", "runtime")


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/stitch.hip, csrc/assign.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    return hostsim.build_units(workdir, FILES, "stitch")


def main():
    return hostsim.run_program(FILES, "stitch_main.cpp", "stitch_host", "--asan" in sys.argv)


if __name__ == "__main__":
    raise SystemExit(main())
