"""Development tool: the resampling kernels (csrc/resample.hip: sep_resample_fwd, sep_resample_stream_fwd; csrc/runtime.hip beside them holds the
library's error slot and the kernel-name observable) compiled for the host (tools/hostsim.py::host_copy, the stand-in HIP header of
tools/hostsim/include) and linked with tools/hostsim/resample_main.cpp into ONE PROGRAM that runs both kernels over the rate pairs and lengths of
tests/test_resample_gpu.py on exactly-sized buffers against plain double loops over the full table, and every stream against the offline call
bit for bit.  With --asan the program is built with -fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no Python
is involved in the run): reads outside [0, T) of a row or beyond the table, first[] and the history, writes beyond T_out, undefined arithmetic.

    python tools/hostsim_resample.py [--asan]

build_library(workdir) gives tests/test_resample_cpu.py a host-simulation library of csrc/resample.hip and csrc/runtime.hip alone."""
import sys

import hostsim

FILES = ("resample", "runtime")


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/resample.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    return hostsim.build_units(workdir, FILES, "resample")


def main():
    return hostsim.run_program(FILES, "resample_main.cpp", "resample_host", "--asan" in sys.argv)


if __name__ == "__main__":
    raise SystemExit(main())
