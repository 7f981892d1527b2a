"""Development tool: the dynamic-mixing kernels (csrc/mixing.hip: sep_mix_draw, sep_mix_render; csrc/runtime.hip beside them holds the library's
error slot and the kernel-name observable) compiled for the host (tools/hostsim.py::host_copy, the stand-in HIP header of tools/hostsim/include)
and linked with tools/hostsim/mixing_main.cpp into ONE PROGRAM that draws and renders the test corpus of tests/test_dynamic_mixing_gpu.py in both
sample kinds on exactly-sized buffers against the rule of include/sepkernels.h restated in plain loops -- and renders HOSTILE plans (an utterance
index out of range either way, start >= len, lead negative or >= T, NaN gains), which run only here and never on a device.  With --asan the
program is built with -fsanitize=address,undefined (the runtime is linked in; nothing is preloaded and no Python is involved in the run): a read
outside the corpus's storage, a write outside an output, undefined arithmetic on a hostile plan.

    python tools/hostsim_mixing.py [--asan] [--speed]

--speed builds and runs tools/hostsim/mixing_speed_main.cpp instead: the same for sep_mix_draw_speed and sep_mix_render_speed -- the speed cases against the
definition in plain loops, and hostile speed indices (out of range either way), start >= len', leads, a one-sample utterance and descriptor fields out
of bounds on exactly-sized filter buffers.

build_library(workdir) gives tests/test_dynamic_mixing_cpu.py a host-simulation library of csrc/mixing.hip and csrc/runtime.hip alone (the
recorded-sequence case there needs csrc/sequence.hip and with it every file: tools/hostsim.py::build)."""
import sys

import hostsim

FILES = ("mixing", "runtime")


def build_library(workdir):
    """-> path of a shared library with the entry points of csrc/mixing.hip and csrc/runtime.hip, for hostsim.HostSimBackend"""
    return hostsim.build_units(workdir, FILES, "mixing")


def main():
    driver = "mixing_speed_main.cpp" if "--speed" in sys.argv else "mixing_main.cpp"
    return hostsim.run_program(FILES, driver, "mixing_host", "--asan" in sys.argv)


if __name__ == "__main__":
    raise SystemExit(main())
