"""CPU: the two oracle statements (oracle/convtasnet_oracle.py: elementary tensor algebra; oracle/fast_port.py: the same path on
torch.nn.functional) against the unmodified reference at the PAPER-BEST configuration (N512 L16 B128 H512 Sc128 P3 X8 R3:
dilations up to 128, three repeats, the last layer without output head), forward, PIT loss, permutation and every parameter
gradient in fp64 -- the other golden fixtures pin them only up to R=2, X=3.  The reference's values are
tests/golden/convtasnet_paper_t20003.npz (oracle/make_golden.py::paper_t20003_golden: the whole output, the loss, the permutation and,
per parameter gradient, its norm, largest magnitude and 64 sampled elements).  The port is what the full-size GPU parity tests and
bench.py's cpu_baseline rely on, which is why this equality is pinned here."""
import os

import numpy as np
import torch

from oracle import convtasnet_oracle as O
from oracle import fast_port as FP
from oracle.make_golden import PAPER_CFG as PAPER, paper_t20003_setup, sample_index


def test_oracle_and_port_equal_the_live_reference_at_paper_best(golden_dir):
    from models.conv_tasnet import ConvTasNet
    fx = np.load(os.path.join(golden_dir, "convtasnet_paper_t20003.npz"))
    model, mixture, sources = paper_t20003_setup(ConvTasNet)
    # the fixture stores no parameters (5 M): the product's class under the fixture's seeds must BE the reference's model -- same keys,
    # same values (fingerprints), same seeded input
    assert np.array_equal(mixture.numpy()[0, 0, :16], fx["mixture_head"])
    assert sorted(k[4:] for k in fx.files if k.startswith("pfp/")) == sorted(model.state_dict().keys())
    for k, v in model.state_dict().items():
        fp = fx["pfp/" + k]
        assert abs(v.sum().item() - fp[0]) <= 1e-12 * (fp[1] + 1e-30) and abs(v.abs().sum().item() - fp[1]) <= 1e-12 * (fp[1] + 1e-30), k
    names = [k for k, _ in model.named_parameters()]
    assert sorted(k[4:] for k in fx.files if k.startswith("gfp/")) == sorted(names)
    p = {k: v.detach().clone() for k, v in model.state_dict().items()}
    out, loss, pattern = torch.from_numpy(fx["output"]), float(fx["loss"]), torch.from_numpy(fx["pattern"])

    for name, step in (("fast_port", FP.train_step), ("algebra oracle", O.train_step)):
        o, l, pat, gr = step(p, PAPER, mixture, sources, dtype=torch.float64)
        assert (o - out).abs().max() <= 1e-12 * out.abs().max(), name
        assert abs(l.item() - loss) <= 1e-12 * abs(loss), name
        assert torch.equal(torch.as_tensor(pat), pattern), name
        for k in names:
            fp, g = fx["gfp/" + k], gr[k].reshape(-1)
            gmax = max(float(fp[1]), 1e-30)
            err = max(abs(g.norm().item() - fp[0]), abs(g.abs().max().item() - fp[1]),
                      (g[sample_index(g.numel())] - torch.from_numpy(fp[2:])).abs().max().item())
            assert err <= 1e-10 * gmax, "{}: {} {:.2e}".format(name, k, err / gmax)
