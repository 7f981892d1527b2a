"""Development tool: the MixIT kernels (csrc/mixit.hip: sep_mixit_gram, sep_mixit_search, sep_mixit_bwd) compiled for the host (tools/hostsim.py::host_copy,
the stand-in HIP header of tools/hostsim/include) and linked with tools/hostsim/mixit_main.cpp into ONE PROGRAM that runs the three kernels at
R = M + N in {2, 10, 24} and T in {1, 2 SEP_MIXIT_SLAB + 17} on exactly-sized buffers against plain double loops.  With --asan the program is
built with -fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no Python is involved in the run): reads beyond a
row's end, writes beyond the scratch or the outputs, undefined arithmetic.

    python tools/hostsim_mixit.py [--asan]

build_library(workdir) gives tests/test_mixit_cpu.py a host-simulation library of csrc/mixit.hip, csrc/bss.hip and csrc/runtime.hip alone."""
import sys

import hostsim

FILES = ("mixit", "bss", "runtime")      # the kernels; bss_reduce_kernel, which adds the Gram pass's slabs; the library's error slot


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/mixit.hip, csrc/bss.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    return hostsim.build_units(workdir, FILES, "mixit")


def main():
    return hostsim.run_program(FILES, "mixit_main.cpp", "mixit_host", "--asan" in sys.argv)


if __name__ == "__main__":
    raise SystemExit(main())
