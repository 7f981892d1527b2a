"""Development tool: the BSS-eval v4 ("images") kernel (csrc/bss.hip: sep_bss_image_energies) compiled for the host (tools/hostsim.py::host_copy,
the stand-in HIP header of tools/hostsim/include) and linked with tools/hostsim/bss_images_main.cpp into ONE PROGRAM that runs the shapes of
tests/test_bss_images_gpu.py on exactly-sized buffers against plain double loops.  With --asan the program is built with
-fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no Python is involved in the run): reads beyond a row's
length, a frame's end or the buffers' ends, writes beyond the scratch, undefined arithmetic.

    python tools/hostsim_bss_images.py [--asan]

The host-simulation library for tests/test_bss_images_cpu.py is tools/hostsim_bss.py::build_library (csrc/bss.hip and csrc/runtime.hip alone)."""
import sys

import hostsim

FILES = ("bss", "runtime")     # the kernels; the library's error slot
CASES = 6                      # what bss_images_main.cpp runs: the five shapes and the refused calls


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/bss.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    return hostsim.build_units(workdir, FILES, "bss")


def main():
    return hostsim.run_program(FILES, "bss_images_main.cpp", "bss_images_host", "--asan" in sys.argv)


if __name__ == "__main__":
    raise SystemExit(main())
