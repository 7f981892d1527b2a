"""Development tool: the BSS-eval kernels (csrc/bss.hip: sep_bss_xcorr, sep_bss_energies) compiled for the host (tools/hostsim.py::host_copy,
the stand-in HIP header of tools/hostsim/include) and linked with tools/hostsim/bss_main.cpp into ONE PROGRAM that runs the kernel cases of
tests/test_bss_eval_gpu.py on exactly-sized buffers against plain double loops.  With --asan the program is built with
-fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no Python is involved in the run): reads beyond a row's
length or the buffers' ends, writes beyond the scratch, undefined arithmetic.

    python tools/hostsim_bss.py [--asan]

build_library(workdir) gives tests/test_bss_eval_cpu.py a host-simulation library of csrc/bss.hip and csrc/runtime.hip alone (a few seconds instead of the
minute the whole of csrc/ takes)."""
import sys

import hostsim

FILES = ("bss", "runtime")      # the kernels; the library's error slot


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/bss.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    return hostsim.build_units(workdir, FILES, "bss")


def main():
    return hostsim.run_program(FILES, "bss_main.cpp", "bss_host", "--asan" in sys.argv)


if __name__ == "__main__":
    raise SystemExit(main())
