"""CPU: every kernel instance sep_pw_wgrad / sep_pw_wgrad_batch can launch -- 27 names -- reached BY NAME on the host simulation of the
kernel sources (tools/hostsim.py), one smallest case per name: B = 2, T = 130, ldt = 256, nsplit = 2, the shape and arithmetic that
family's acceptance rule asks for.  Each case asserts sepkernels.last_kernel() and compares with the CPU emulator through the kernel
tests' own helper and tolerance (tests/test_gpu_kernels.py: _wgrad_both).  The dispatch is host code, identical on the host simulation
and on the device, so this file has no device tier on purpose: it pins which descriptor lands on which instance."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                         # noqa: E402
import test_gpu_kernels as GK          # noqa: E402

pytestmark = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++ (ext_vector_type)")

B, T, LDT, NS = 2, 130, 256, 2
XMODES = ["SEP_PRO_NONE", "SEP_PRO_PRELU", "SEP_PRO_GLN", "SEP_PRO_GLN_PRELU"]

# family -> (name format, arithmetic, M, N, x_modes, form); form: how the call is made (below)
FAMILIES = [
    ("wgrad_direct<{}>", "f32", 32, 4, XMODES, "plain"),
    ("wgrad_split<{}>", "bf16x6", 192, 64, XMODES, "plain"),
    ("wgrad_pc<4,1,{}>", "bf16x6", 256, 128, XMODES, "plain"),
    ("wgrad_pc<2,2,{}>", "bf16x6", 128, 256, XMODES, "plain"),
    ("wgrad_pc16<4,1,{}>", "f16x3", 256, 128, XMODES, "plain"),
    ("wgrad_pc16_pre<4,1,{}>", "f16x3", 256, 128, XMODES[:2], "pre"),
    ("wgrad_pc16_batch<4,1,{}>", "f16x3", 256, 128, XMODES, "batch"),
]
CASES = [("wgrad", "f32", 32, 4, "SEP_PRO_NONE", "g_mul")] + \
        [(fmt.format(xm), arith, M, N, xm, form) for fmt, arith, M, N, xms, form in FAMILIES for xm in xms]
assert len(CASES) == len(set(c[0] for c in CASES)) == 27


@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim.build(str(tmp_path_factory.mktemp("hostsim_wgrad")))


@pytest.fixture()
def on_host(sim_library):
    """the kernel tests' device hooks pointed at the host simulation"""
    saved = (GK.HIP, GK.to_device, GK.device_sync, GK.device_name)
    with hostsim.HostSimBackend(sim_library) as K:
        GK.HIP, GK.to_device, GK.device_sync, GK.device_name = K, (lambda t: t.clone()), (lambda: None), (lambda: "cpu")
        try:
            yield K
        finally:
            GK.HIP, GK.to_device, GK.device_sync, GK.device_name = saved


def _product(M, N, xm, two_sources=False):
    """keyword arguments of one weight gradient with the prologue `xm` (emulator and device take the same ones)"""
    part, pb = GK._wg_out(NS, M, N)
    X = GK.padded(B, N, T, LDT)
    kw = dict(B=B, M=M, N=N, T=T, ldt=LDT, X=X, x_mode=XMODES.index(xm), partial=part, partial_bias=pb, nsplit=NS)
    if two_sources:
        kw.update(G=GK.padded(B, M // 2, T, LDT), G2=GK.padded(B, M // 2, T, LDT, scale=3.0), g_split=M // 2)
    else:
        kw.update(G=GK.padded(B, M, T, LDT))
    if xm.endswith("PRELU"):
        kw.update(x_alpha=torch.tensor([0.2]))
    if "GLN" in xm:
        u = torch.where(X > 0, X, 0.2 * X) if xm.endswith("PRELU") else X
        kw.update(x_stats=GK.stats_of(u, T), x_gamma=GK.rnd(N) + 1, x_beta=GK.rnd(N), count=N * T, eps=1e-12)
    return kw


class _Via:
    """stands in for the device backend inside _wgrad_both: the product goes out in the form under test, everything else is the backend's"""

    def __init__(self, K, send):
        self.K, self.send = K, send

    def pw_wgrad(self, **kw):
        self.send(self.K, kw)


@pytest.mark.parametrize("name,arith,M,N,xm,form", CASES, ids=[c[0] for c in CASES])
def test_the_descriptor_lands_on_the_named_instance_and_matches_the_emulator(on_host, name, arith, M, N, xm, form):
    import sepkernels
    GK.G.manual_seed(4000 + CASES.index((name, arith, M, N, xm, form)))
    prev = sepkernels.set_gemm_arith(arith)
    try:
        if form == "plain":
            GK._wgrad_both(_product(M, N, xm))
        elif form == "g_mul":                      # the latent product: G is multiplied by Gaux on the fly, which only the plain kernel does
            kw = _product(M, N, xm)
            kw.update(Gaux=GK.padded(B, M, T, LDT), g_mul=1, g_div=1)
            GK._wgrad_both(kw)
        elif form == "pre":                        # the second G source handed over pre-split, as test_wgrad_with_a_presplit_second_source builds it
            kw = _product(M, N, xm, two_sources=True)
            GK.HIP = _Via(on_host, lambda K, q: K.pw_wgrad(G2_pre=K.split_rows(q["G2"], T, NS // B), **q))
            GK._wgrad_both(kw)
        else:                                      # two products in one grid (they share the prologue's tensors); the one under comparison first, then second
            for slot in (0, 1):
                part, pb = GK._wg_out(NS, M, N)
                other = dict(G=GK.padded(B, M, T, LDT), X=GK.padded(B, N, T, LDT), partial=part, partial_bias=pb)
                GK.HIP = _Via(on_host, lambda K, q: K.pw_wgrad_batch([q, dict(q, **other)][::1 - 2 * slot]))
                GK._wgrad_both(_product(M, N, xm))
        assert sepkernels.last_kernel() == name
    finally:
        sepkernels.set_gemm_arith(prev)
