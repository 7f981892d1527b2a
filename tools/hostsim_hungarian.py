"""Development tool: the optimal-permutation kernels (csrc/assign.hip: sep_pair_gram, sep_assign, sep_pair_assign, sep_pair_bwd) compiled for the host
(tools/hostsim.py::host_copy, the stand-in HIP header of tools/hostsim/include) and linked with tools/hostsim/hungarian_main.cpp into ONE PROGRAM
that runs the four kernels at n in {1, 9, 64} and T in {1, 2 SEP_PAIR_SLAB + 17} on exactly-sized buffers against plain double loops and a
plain O(n^3) solver, matrices of NaN and +-Inf included.  With --asan the program is built with -fsanitize=address,undefined (the runtime is
linked in; nothing is preloaded and no Python is involved in the run): reads beyond a row's end, writes beyond the scratch or the outputs,
an index from a poisoned comparison, undefined arithmetic.

    python tools/hostsim_hungarian.py [--asan]

build_library(workdir) gives tests/test_hungarian_cpu.py a host-simulation library of csrc/assign.hip, csrc/loss.hip (the criterion test there sets the
result next to sep_sisdr_dots) and csrc/runtime.hip alone."""
import sys

import hostsim

FILES = ("assign", "loss", "runtime")      # the kernels; sep_sisdr_dots and its siblings, which the criterion test compares with; the library's error slot


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/assign.hip, csrc/loss.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    return hostsim.build_units(workdir, FILES, "assign")


def main():
    return hostsim.run_program(FILES, "hungarian_main.cpp", "hungarian_host", "--asan" in sys.argv)


if __name__ == "__main__":
    raise SystemExit(main())
