"""
ORACLE TOOLING -- TEST INFRASTRUCTURE ONLY.

Writes tests/golden/convtasnet_causal_online.npz, the fixture of tests/test_online_cpu.py / test_online_gpu.py: for the causal configurations
`causal16` (P = 3, softmax mask, 3 sources, L = 20, S = 10) and `causal16_p5` (P = 5, sigmoid mask, encoder ReLU) the UNMODIFIED reference
model, with the parameters of tests/golden/convtasnet_<name>.npz (not stored again here), run on that fixture's mixtures zero-prefixed by
L - S samples and right-padded to a multiple of S -- the input for which streaming chunk by chunk and then flushing must give the offline
output (sepkernels/online.py).  Stored per configuration: `<name>/input`, `<name>/output_f64` (fp64 run of the same module tree) and
`<name>/output_f32` (the reference as shipped).  Needs the reference tree (build container only), imported the way oracle/make_golden.py does:

    python tools/make_online_golden.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.make_golden import CONFIGS, import_reference      # noqa: E402

NAMES = ("causal16", "causal16_p5")
OUT = os.path.join(ROOT, "tests", "golden", "convtasnet_causal_online.npz")


def online_input(mixture, L, S):
    """(B, 1, T) -> zero prefix of L - S samples, zeros on the right up to a multiple of S (before the prefix)"""
    T = mixture.shape[-1]
    return F.pad(mixture, (L - S, (S - T % S) % S))


def main():
    ConvTasNet = import_reference()[0]
    blob = {}
    for name in NAMES:
        cfg = CONFIGS[name]
        g = np.load(os.path.join(ROOT, "tests", "golden", "convtasnet_{}.npz".format(name)))
        model = ConvTasNet(**cfg)
        model.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("param/")})
        model.eval()
        x = online_input(torch.from_numpy(g["mixture"]), cfg["kernel_size"], cfg["stride"])
        assert (x.shape[-1] - cfg["kernel_size"]) % cfg["stride"] == 0         # the offline forward pads nothing
        with torch.no_grad():
            out32 = model(x)
            out64 = model.double()(x.double())
        blob[name + "/input"] = x.numpy()
        blob[name + "/output_f32"] = out32.numpy()
        blob[name + "/output_f64"] = out64.numpy()
        print(name, tuple(x.shape), "->", tuple(out64.shape))
    np.savez_compressed(OUT, **blob)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
