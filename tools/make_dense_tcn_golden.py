"""
ORACLE TOOLING -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/convtasnet_causal16_dense.npz and convtasnet_causal16_dense_joint.npz, the fixtures of tests/test_dense_tcn_cpu.py /
test_dense_tcn_gpu.py: the UNMODIFIED reference's ConvTasNet(causal=True, separable=False) in the configurations of
tests/dense_tcn_configs.py -- forward in fp32 and fp64, PIT(NegSI-SDR), every gradient in fp64 -- with the keys and the seeds of
oracle/make_golden.py::model_golden (whose function is used as it is).  A fixture that would exceed the repository's limit of 1 MiB per file
is stored as two: its `grad/*` keys move to convtasnet_<name>_grads.npz (tests/test_dense_tcn_gpu.py::load_fixture reads both).  Needs the reference tree (build container only), imported the way
oracle/make_golden.py does; not needed at test time:

    python tools/make_dense_tcn_golden.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle.make_golden as MG                 # noqa: E402
from dense_tcn_configs import CONFIGS, SHAPES   # noqa: E402


LIMIT = 1 << 20


def main():
    ConvTasNet, NegSISDR, _, PIT1d, _ = MG.import_reference()
    MG.CONFIGS.update(CONFIGS)                  # (this process only: model_golden looks its configuration up by name)
    MG.SHAPES.update(SHAPES)
    for name in CONFIGS:
        MG.model_golden(name, ConvTasNet, NegSISDR, PIT1d)
        path = os.path.join(MG.OUT, "convtasnet_{}.npz".format(name))
        if os.path.getsize(path) > LIMIT:
            blob = dict(np.load(path))
            grads = {k: blob.pop(k) for k in list(blob) if k.startswith("grad/")}
            np.savez_compressed(path, **blob)
            np.savez_compressed(path[:-4] + "_grads.npz", **grads)
        for q in (path, path[:-4] + "_grads.npz"):
            if os.path.exists(q):
                assert os.path.getsize(q) <= LIMIT, q
                print(q, os.path.getsize(q), "bytes")


if __name__ == "__main__":
    main()
