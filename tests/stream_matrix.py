"""Helper module (not a test file): the ledger of the kernel instances behind the streaming (non-GEMM) entry points of csrc/filterbank.hip,
csrc/tcn.hip, csrc/gln.hip, csrc/depthwise.hip, csrc/cln.hip and csrc/causal.hip, a case matrix that reaches every one of them BY NAME (sep_last_kernel), a float64 restatement of every
call's contract, and a metric local enough that one wrong row or one wrong halo frame cannot hide.  tests/test_stream_instances_cpu.py runs
the matrix on the host simulation of the kernel sources, tests/test_stream_instances_gpu.py on the MI355X; the children of the latter start

    python tests/stream_matrix.py --env NAME --out FILE [--backend hostsim:<library>]

once per A/B switch, because the dispatchers read their SEPK_* switches once per process.

THE LEDGER.  INSTANCES is every name the dispatchers in scope can emit: the kernel function and its template arguments as spelled at the launch,
with a run-time value that selects behaviour without a template argument behind a "/" (the nz of the decoder backward's grid, the LDS-free
`aligned` form of the three-tap row kernels, the sliced form of the token gLN).  dispatch(env, case) restates the dispatch tables in Python:
under a switch the expected name of a case is the forced instance.  cases() refuses to return a matrix that misses an instance.

THE METRIC.  reference() evaluates the contract of include/sepkernels.h in torch float64 on the same fp32 inputs and describes every output as
  rows   an elementwise output, laid out in rows of frames: for every row, max_t |got - ref| <= bound * max_t |ref| over the row's valid frames
         (a loud row cannot mask a quiet one: every channel row of the inputs carries its own magnitude, 2^-6 .. 2^6); pad frames must be
         exactly zero (or, for the cLN's mean / rstd, untouched) where the header says so;
  sums   a reduction output: |got - ref| <= bound * sum |addends| (the reference returns the same sum over the magnitudes of the addends);
         slot and tile distributions are summed first.  (One sum has a nested addend: the PReLU2 slope sum of dwconv_bwd, sum du2 z [z <= 0].
         Where the kernel reads z, the addend is du2 z.  Where it forms z = bd + sum_k wd_k v1 again from `a`, z's own terms are addends
         of the sum the kernel evaluates, du2 bd and du2 wd_k v1: a row whose z nearly cancels would otherwise be asked for more digits
         than an fp32 z has.)
  ints   exact equality (exponents, the fp16 planes of sep_split_rows, arrival counters).
Every device buffer sits between two guard bands of a fixed value, every pure output and every pad region starts as NaN; after the call the
guards and the inputs must be untouched.

THE BOUND is measured, per family: FAMILIES[f]["e32"] is the worst figure, in the metric above, of the fp32 CPU emulator (tests/emulator.py --
torch on the CPU, not the code under test) against the float64 reference over the family's cases (`python tests/stream_matrix.py --measure`),
and FAMILIES[f]["bound"] = min(2e-4, 4 * e32 rounded up to a power of two): the factor 4 because the device sums in wave trees and float4
lanes where torch sums serially, and never looser than the 2e-4 the older tests grant.  tests/test_stream_instances_cpu.py recomputes e32 and
holds the table to this rule.

SIGN-SENSITIVE BACKWARD KERNELS.  dwconv_bwd_row<.,.,true> forms z again from `a` and gates on its sign: an argument that fp32 and fp64 place on
different sides of zero gives an O(1) difference that is no error.  No element is exempted: the generator draws the case's operands from up to
8 seeds and takes the first for which no z of the float64 reference lies closer to zero than the bound times the magnitude sum of its addends
(|bd| + sum_k |wd_k v1|); the seed used is recorded with the case, and cases() fails if a case finds none.  (The ReLU / PReLU gates of the other
kernels in scope read their argument from an INPUT tensor, identical on both sides.)"""
import argparse
import json
import math
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "dnn-based_source_separation_amd", "src"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SLOTS, ARRIVE = 16, 17
DW_TT = 1024                                     # frames per tile of the depthwise tile kernels and of rowpart
GUARD = 256                                      # elements in front of and behind every device buffer
GUARD_VALUE = 12345.0
EPS = 1e-12
SEEDS = 8

# family: the fp32 emulator's worst figure against the float64 reference over the family's cases, and the bound that follows from it
FAMILIES = {
    "encoder": dict(e32=3.8e-07, bound=2.0 ** -19),
    "dwconv_fwd": dict(e32=4.0e-06, bound=2.0 ** -15),
    "dwconv_bwd": dict(e32=7.5e-07, bound=2.0 ** -18),
    "decoder_fwd": dict(e32=8.1e-07, bound=2.0 ** -18),
    "decoder_bwd": dict(e32=6.3e-07, bound=2.0 ** -18),
    "depthwise": dict(e32=1.4e-07, bound=2.0 ** -20),
    "split_rows": dict(e32=5.2e-08, bound=2.0 ** -22),
    "gln_tokens": dict(e32=5.0e-06, bound=2.0 ** -15),
    "cln": dict(e32=6.1e-06, bound=2.0 ** -15),
    "causal": dict(e32=2.4e-07, bound=2.0 ** -19),
}


def bound_rule(e32):
    """4 x the emulator's figure, rounded up to a power of two, never looser than the 2e-4 of the older tests"""
    return min(2e-4, 2.0 ** math.ceil(math.log2(4 * e32))) if e32 > 0 else 2e-4


ENVS = {
    "default": {},
    "dwconv_lds": {"SEPK_DWCONV_LDS": "1"},
    "dwb_no_recompute": {"SEPK_DWB_RECOMPUTE": "0"},
    "cln_three": {"SEPK_CLN_CHAIN": "0"},
    "depthwise_generic": {"SEPK_DEPTHWISE_ROWS": "0"},
}
SWITCHES = ("SEPK_DWCONV_LDS", "SEPK_DWB_RECOMPUTE", "SEPK_CLN_CHAIN", "SEPK_DEPTHWISE_ROWS")
ENV_FAMILIES = {"default": tuple(FAMILIES), "dwconv_lds": ("dwconv_fwd", "dwconv_bwd"), "dwb_no_recompute": ("dwconv_bwd",), "cln_three": ("cln",),
                "depthwise_generic": ("depthwise",)}

BOOL = {False: "false", True: "true"}
INSTANCES = sorted(
    ["encoder_l16s8", "encoder<16>", "encoder<0>"] +
    ["dwconv_fwd_direct<{},{}>".format(dm, r) for dm in (0, 1, 2) for r in (1, 2)] + ["dwconv_fwd_tiles"] +
    ["dwconv_bwd_row<{},{},{}>".format(al, nit, BOOL[rc]) for al in (0, 1, 2, 3) for nit in (4, 8) for rc in (False, True)] + ["dwconv_bwd_tiles"] +
    ["decoder_fwd16<2>", "decoder_fwd16<4>", "decoder_fwd<16>", "decoder_fwd<0>"] +
    ["decoder_bwd<{}>/nz{}".format(t, nz) for t in ("16,2", "16,4", "0,0") for nz in (1, 8)] +
    ["depthwise3_row<{}>/{}".format(k, f) for k in (0, 1) for f in ("aligned", "lds")] + ["depthwise3_wgrad_row", "depthwise_fwd", "depthwise_bwd_input",
                                                                                         "depthwise_bwd_weight"] +
    ["split_rows<4>", "split_rows<8>"] +
    ["gln_tokens_fwd", "gln_tokens_fwd/sliced", "gln_tokens_bwd", "gln_tokens_bwd/sliced"] +
    ["cln_chain_fwd<{},{}>".format(rr, BOOL[y]) for rr in (1, 2, 4, 8) for y in (False, True)] + ["cln_chain_bwd<{},8>".format(rr) for rr in (1, 2, 4, 8)] +
    ["cln_three_fwd", "cln_three_stats", "cln_three_bwd"] +
    ["cd_depthwise_{}<{},{}>".format(k, kw, BOOL[st]) for k in ("fwd", "wgrad") for kw in (3, 0) for st in (False, True)])


# ---------------------------------------------------------------------------------------------------------------- the dispatch tables, restated
def gln_tokens_nsplit(nseq, n):
    if nseq >= 128:
        return 1
    trips = (n + 1023) // 1024
    return max(1, min((512 + nseq - 1) // nseq, trips // 16, 64))


def dispatch(env, c):
    """the instance name the entry point gives the case under the environment `env` (a dict of the SEPK_* switches)"""
    op = c["op"]
    if op == "encoder_fwd":
        if (c["Cin"], c["L"], c["S"]) == (1, 16, 8):
            return "encoder_l16s8"
        return "encoder<16>" if c["Cin"] * c["L"] == 16 else "encoder<0>"
    if op == "dwconv_fwd":
        d = c["d"]
        if "SEPK_DWCONV_LDS" not in env and (d in (1, 2) or d % 4 == 0):
            return "dwconv_fwd_direct<{},{}>".format(0 if d % 4 == 0 else d, 2 if c["C"] % 2 == 0 else 1)
        return "dwconv_fwd_tiles"
    if op == "dwconv_bwd":
        d = c["d"]
        if "SEPK_DWCONV_LDS" not in env and c["ldt"] <= 8192:
            rc = bool(c["bias"]) and env.get("SEPK_DWB_RECOMPUTE") != "0"
            return "dwconv_bwd_row<{},{},{}>".format(0 if d % 4 == 0 else d if d <= 2 else 3, 4 if c["ldt"] <= 4096 else 8, BOOL[rc])
        return "dwconv_bwd_tiles"
    if op == "decoder_fwd":
        LC = c["Cout"] * c["L"]
        if LC == 16 and c["L"] == 16 and c["S"] == 8 and c["n_src"] <= 4 and c["ldt"] % 64 == 0:
            return "decoder_fwd16<2>" if c["n_src"] <= 2 else "decoder_fwd16<4>"
        return "decoder_fwd<16>" if LC == 16 else "decoder_fwd<0>"
    if op == "decoder_bwd":
        LC = c["Cout"] * c["L"]
        t = "16,2" if LC == 16 and c["n_src"] <= 2 else "16,4" if LC == 16 and c["n_src"] <= 4 else "0,0"
        return "decoder_bwd<{}>/nz{}".format(t, 8 if c["N"] >= 64 else 1)
    if op in ("depthwise_fwd", "depthwise_bwd_input", "depthwise_bwd_weight"):
        rows = (env.get("SEPK_DEPTHWISE_ROWS") != "0" and c["Kw"] == 3 and c["stride"] == 1 and c["Tin"] == c["Tout"] and c["Tin"] % 4 == 0 and
                c["Tin"] * 4 <= 128 * 1024)
        if not rows:
            return op
        if op == "depthwise_bwd_weight":
            return "depthwise3_wgrad_row"
        p, d = c["pad"], c["dil"]
        al = ((p | (d - p) | (2 * d - p)) & 3) == 0 if op == "depthwise_fwd" else ((p | (p - d) | (p - 2 * d)) & 3) == 0
        return "depthwise3_row<{}>/{}".format(0 if op == "depthwise_fwd" else 1, "aligned" if al else "lds")
    if op == "split_rows":
        return "split_rows<4>" if c["ldt"] <= 4096 else "split_rows<8>"
    if op in ("gln_tokens_fwd", "gln_tokens_bwd"):
        return op + ("/sliced" if gln_tokens_nsplit(c["nseq"], c["L"] * c["C"]) > 1 else "")
    if op in ("cln_fwd", "cln_stats", "cln_bwd"):
        C = c["C"]
        if C > 512 or env.get("SEPK_CLN_CHAIN") == "0":
            return {"cln_fwd": "cln_three_fwd", "cln_stats": "cln_three_stats", "cln_bwd": "cln_three_bwd"}[op]
        rr = 1 if C <= 64 else 2 if C <= 128 else 4 if C <= 256 else 8
        return "cln_chain_bwd<{},8>".format(rr) if op == "cln_bwd" else "cln_chain_fwd<{},{}>".format(rr, BOOL[op == "cln_fwd"])
    if op in ("depthwise_cln_fwd", "depthwise_cln_bwd_weight"):
        return "cd_depthwise_{}<{},{}>".format("fwd" if op == "depthwise_cln_fwd" else "wgrad", 3 if c["Kw"] == 3 else 0, BOOL[c["ldt"] * 4 <= 64 * 1024])
    raise KeyError(op)


# ---------------------------------------------------------------------------------------------------------------- the case matrix
def _enc_frames(Tin, L, S, pad_left):
    return (Tin + 2 * pad_left - L) // S + 1


def _all_cases():
    cs = []
    add = lambda family, op, **kw: cs.append(dict(family=family, op=op, **kw))
    # encoder: the three instances and the two generic shapes, relu off / on, input padding 0 / 3; once without pad frames (F == ldt)
    for (Cin, L, S) in [(1, 16, 8), (2, 8, 4), (1, 16, 4), (2, 20, 10), (1, 2, 1)]:
        for relu in (0, 1):
            for pad_left in (0, 3):
                Tin = S * 299 + L - 2 * pad_left
                add("encoder", "encoder_fwd", B=2, Cin=Cin, L=L, S=S, N=7, relu=relu, pad_left=pad_left, Tin=Tin, F=_enc_frames(Tin, L, S, pad_left), ldt=384)
        add("encoder", "encoder_fwd", B=2, Cin=Cin, L=L, S=S, N=6, relu=1, pad_left=0, Tin=S * 127 + L, F=128, ldt=128)
    # depthwise pair of the TCN layers, forward: six direct instances, the tile kernel, T < d, no pad frames, the accepted maxima
    for d in (1, 2, 4, 3, 6):
        for C in (6, 7):
            for T in (300, 1100):
                add("dwconv_fwd", "dwconv_fwd", B=2, C=C, T=T, ldt=(T + 127) // 128 * 128, d=d)
    for (C, T, ldt, d) in [(6, 100, 128, 128), (7, 100, 128, 128), (7, 384, 384, 2), (6, 384, 384, 3), (6, 300, 384, 4096), (7, 300, 384, 4095)]:
        add("dwconv_fwd", "dwconv_fwd", B=2, C=C, T=T, ldt=ldt, d=d)
    # ... backward: 16 row instances (AL x NIT x RC), the tile kernel up to its 160 KiB of LDS, T < d, and B = 3, C = 17 for the slots;
    # each in the three modes of the gLN1 outputs
    for mode in ("publish", "sums", "none"):
        for i, d in enumerate((4, 1, 2, 3, 6)):
            for j, (T, ldt) in enumerate([(300, 384), (4096, 4096), (4100, 4224), (8192, 8192)]):
                for bias in (1, 0):
                    add("dwconv_bwd", "dwconv_bwd", B=2, C=6 + (i + j) % 2, T=T, ldt=ldt, d=d, bias=bias, mode=mode)
        for d in (1, 3, 128, 2048):
            add("dwconv_bwd", "dwconv_bwd", B=2, C=6 + d % 2, T=8200, ldt=8320, d=d, bias=1, mode=mode)
        add("dwconv_bwd", "dwconv_bwd", B=2, C=7, T=100, ldt=128, d=128, bias=1, mode=mode)
        add("dwconv_bwd", "dwconv_bwd", B=2, C=6, T=100, ldt=128, d=128, bias=0, mode=mode)
        add("dwconv_bwd", "dwconv_bwd", B=3, C=17, T=300, ldt=384, d=1, bias=1, mode=mode)
    add("dwconv_bwd", "dwconv_bwd", B=3, C=17, T=8200, ldt=8320, d=3, bias=1, mode="publish")
    # decoder: four forward / three backward instances x N in {16, 64} x {F = 300 of ldt = 384, F = ldt = 256}
    geo = {"16/2": dict(n_src=2, Cout=1, L=16, S=8), "16/4": dict(n_src=3, Cout=1, L=16, S=8), "16/5": dict(n_src=5, Cout=1, L=16, S=8),
           "2x8": dict(n_src=2, Cout=2, L=8, S=4), "4x8": dict(n_src=4, Cout=2, L=8, S=4), "0": dict(n_src=2, Cout=2, L=20, S=10)}
    for N in (16, 64):
        for (F, ldt) in ((300, 384), (256, 256)):
            for k, (g, pad_left) in enumerate([("16/2", 0), ("16/4", 3), ("16/5", 0), ("2x8", 3), ("0", 3)]):
                for latent in (1, 0):
                    add("decoder_fwd", "decoder_fwd", B=2, N=N, F=F, ldt=ldt, pad_left=pad_left, latent=latent, **geo[g])
            for k, (g, pad_left) in enumerate([("16/2", 0), ("2x8", 3), ("16/4", 3), ("4x8", 0), ("16/5", 0), ("0", 3)]):
                for raw_mask in (0, 1):
                    add("decoder_bwd", "decoder_bwd", B=2, N=N, F=F, ldt=ldt, pad_left=pad_left, raw_mask=raw_mask, **geo[g])
    # depthwise convolution of the staged layers: three taps aligned / through LDS, five taps and stride 2 on the generic kernels
    for (Kw, stride, pad, dil, Tin, C) in [(3, 1, 8, 4, 300, 7), (3, 1, 2, 1, 300, 6), (3, 1, 6, 3, 300, 7), (3, 1, 3, 3, 1100, 6), (5, 1, 8, 2, 300, 7),
                                           (3, 2, 1, 1, 257, 6), (3, 2, 2, 2, 600, 7)]:
        Tout = Tin if stride == 1 else (Tin + 2 * pad - dil * (Kw - 1) - 1) // stride + 1
        for op in ("depthwise_fwd", "depthwise_bwd_input", "depthwise_bwd_weight"):
            for bias in ((1, 0) if op == "depthwise_fwd" else (0,)):
                add("depthwise", op, B=2, C=C, Tin=Tin, Tout=Tout, Kw=Kw, stride=stride, pad=pad, dil=dil, bias=bias)
    # operand split of the heads' weight gradient: both row lengths at one slab and at the most slabs the entry point takes
    for (T, ldt) in ((4000, 4096), (8100, 8192)):
        for k in (1, 64):
            add("split_rows", "split_rows", B=2, C=6, T=T, ldt=ldt, k=k)
    # token gLN: the largest L * C of the single form and the smallest of the sliced one
    for (nseq, L, C) in [(3, 1984, 16), (3, 1985, 16), (2, 37, 4), (2, 31, 1024)]:
        for op in ("gln_tokens_fwd", "gln_tokens_bwd"):
            add("gln_tokens", op, nseq=nseq, L=L, C=C)
    # cLN: RR 1, 2, 4, 8 and the three-launch form; T astride the 32-frame tile; B in {1, 3}
    for C in (24, 100, 200, 300, 520):
        for T in (31, 33, 203):
            for B in (1, 3):
                ldt = (T + 3) // 4 * 4 + (4 if T == 33 else 0)
                for op, alpha in (("cln_fwd", 0), ("cln_fwd", 1), ("cln_stats", B % 2), ("cln_bwd", 0), ("cln_bwd", 1)):
                    add("cln", op, B=B, C=C, T=T, ldt=ldt, alpha=alpha)
    # first norm folded into its depthwise convolution: Kw in {3, 5}, the staged and the unstaged row, pad in {0, (Kw - 1) d}
    for Kw, dil in ((3, 3), (5, 2)):
        for (B, C, T, ldt) in ((2, 7, 300, 384), (1, 2, 16300, 16388)):
            for pad in (0, (Kw - 1) * dil):
                for op in ("depthwise_cln_fwd", "depthwise_cln_bwd_weight"):
                    add("causal", op, B=B, C=C, T=T, ldt=ldt, Kw=Kw, dil=dil, pad=pad, alpha=int(pad > 0), bias=int(pad > 0))
    return cs


_CASES = {}


def cases(env="default"):
    """every case of the environment with the instance it is meant to reach under "name" and the seed of its operands under "seed"; fails if an
    instance has no case (default environment) or a sign-sensitive case finds no seed"""
    if env not in _CASES:
        out = []
        for i, c in enumerate(_all_cases()):
            if c["family"] in ENV_FAMILIES[env]:
                c = dict(c, id=i, name=dispatch(ENVS[env], c))
                out.append(c)
        if env == "default":
            missing = sorted(set(INSTANCES) - set(c["name"] for c in out))
            assert not missing, "no case reaches {}".format(missing)
        for c in out:
            c["seed"] = find_seed(c)
        _CASES[env] = out
    return _CASES[env]


# ---------------------------------------------------------------------------------------------------------------- operands
def _t():
    import torch
    return torch


def _rn(g, *s):
    torch = _t()
    return torch.randn(*s, generator=g, dtype=torch.float64)


def _mags(g, *s):
    torch = _t()
    return 2.0 ** torch.randint(-6, 7, s, generator=g).double()


def _rows(g, B, C, ldt, T, mean=0.0):
    """(B, C, ldt) fp32, every (b, c) row with a magnitude of its own, pad frames zero"""
    x = (_rn(g, B, C, ldt) + mean) * _mags(g, B, C, 1)
    x[..., T:] = 0
    return x.float().contiguous()


def _nan(*s, dtype=None):
    torch = _t()
    return torch.full(s, float("nan"), dtype=dtype or torch.float32)


def _slotted(g, tot):
    """(B, 2) totals -> (B, SLOTS, 2) fp64, spread unevenly over the slots"""
    torch = _t()
    w = torch.rand(SLOTS, generator=g, dtype=torch.float64)
    return (tot.unsqueeze(1) * (w / w.sum()).view(1, SLOTS, 1)).contiguous()


def _prelu(x, a):
    torch = _t()
    return torch.where(x > 0, x, a * x)


def _stats_of(g, u, T):
    torch = _t()
    v = u[..., :T].double()
    return _slotted(g, torch.stack([v.sum((1, 2)), (v * v).sum((1, 2))], 1))


def _shift(v, s):
    """out[..., t] = v[..., t + s] inside the row, zero outside"""
    torch = _t()
    T = v.shape[-1]
    out = torch.zeros_like(v)
    if 0 <= s < T:
        out[..., :T - s] = v[..., s:]
    elif -T < s < 0:
        out[..., -s:] = v[..., :T + s]
    return out


def _mu_rstd(stats, count):
    st = stats.double().reshape(-1, SLOTS, 2).sum(1)
    m = st[:, 0] / count
    var = (st[:, 1] / count - m * m).clamp_min(0.0)
    return m.view(-1, 1, 1), (1.0 / (var + EPS).sqrt()).view(-1, 1, 1)


def operands(c, seed):
    """-> ordered list of (argument name, role, value) in the order of the backend method; role: "in" (must come back untouched), "out" (written),
    "scratch" (workspace), "val" (scalar or None)"""
    torch = _t()
    g = torch.Generator().manual_seed(seed)
    op = c["op"]
    V = lambda n, v: (n, "val", v)
    if op == "encoder_fwd":
        B, Cin, Tin, N, L, S, F, ldt = (c[k] for k in ("B", "Cin", "Tin", "N", "L", "S", "F", "ldt"))
        x = (_rn(g, B, Cin, Tin) * _mags(g, B, Cin, 1)).float()
        E = (_rn(g, N, Cin, L) * _mags(g, N, 1, 1)).float()
        return [("x", "in", x), ("E", "in", E), ("w", "out", _nan(B, N, ldt)), ("stats", "out", _slotted(g, _rn(g, B, 2).abs() * 10)), V("B", B), V("Cin", Cin),
                V("Tin", Tin), V("N", N), V("L", L), V("S", S), V("F", F), V("ldt", ldt), V("pad_left", c["pad_left"]), V("relu", c["relu"])]
    if op in ("dwconv_fwd", "dwconv_bwd"):
        B, C, T, ldt, d = (c[k] for k in ("B", "C", "T", "ldt", "d"))
        a = _rows(g, B, C, ldt, T, mean=0.2)
        a1, a2 = torch.tensor([0.25]), torch.tensor([0.1])
        st1 = _stats_of(g, _prelu(a, a1), T)
        g1, b1, wd, bd = (_rn(g, C) + 1.5).float(), _rn(g, C).float(), _rn(g, C, 1, 3).float(), _rn(g, C).float()
        if op == "dwconv_fwd":
            return [("a", "in", a), ("stats1", "in", st1), ("gamma1", "in", g1), ("beta1", "in", b1), ("alpha1", "in", a1), ("wd", "in", wd), ("bd", "in", bd),
                    ("alpha2", "in", a2), ("z", "out", _nan(B, C, ldt)), ("stats2", "out", _slotted(g, _rn(g, B, 2).abs() * 10)), V("B", B), V("C", C), V("T", T),
                    V("ldt", ldt), V("dilation", d), V("eps", EPS)]
        fw = _ref_dwconv_fwd(c, dict(a=a, stats1=st1, gamma1=g1, beta1=b1, alpha1=a1, wd=wd, bd=bd, alpha2=a2, stats2=torch.zeros(B, SLOTS, 2, dtype=torch.float64)))
        z = fw["z"]["ref"].float().contiguous()                      # the forward's z, rounded to the buffer's fp32 like any stored activation
        st2 = _slotted(g, fw["stats2"]["ref"])
        dv2 = _rows(g, B, C, ldt, T)
        g2, bs2 = (_rn(g, C) + 1.5).float(), (_rn(g, B, 2) * 0.01).float()
        ntile = (ldt + DW_TT - 1) // DW_TT
        mode = c["mode"]
        bacc = torch.zeros(B, SLOTS, 2, dtype=torch.float64) if mode != "none" else None
        arr = torch.zeros(B, ARRIVE, dtype=torch.int32) if mode == "publish" else None
        bs1 = _nan(B, 2) if mode == "publish" else None
        return [("dv2", "in", dv2), ("z", "in", z), ("a", "in", a), ("stats1", "in", st1), ("gamma1", "in", g1), ("beta1", "in", b1), ("alpha1", "in", a1),
                ("stats2", "in", st2), ("gamma2", "in", g2), ("alpha2", "in", a2), ("bsum2", "in", bs2), ("wd", "in", wd), ("bd", "in" if c["bias"] else "val", bd if c["bias"] else None),
                ("dv1", "out", _nan(B, C, ldt)), ("rowpart", "out", _nan(B, C, ntile, 8)), ("bacc1", "out" if bacc is not None else "val", bacc),
                ("arrive1", "out" if arr is not None else "val", arr), ("bsum1", "out" if bs1 is not None else "val", bs1), V("B", B), V("C", C), V("T", T), V("ldt", ldt),
                V("dilation", d), V("eps", EPS)]
    if op in ("decoder_fwd", "decoder_bwd"):
        B, n_src, N, Cout, L, S, F, ldt, pad_left = (c[k] for k in ("B", "n_src", "N", "Cout", "L", "S", "F", "ldt", "pad_left"))
        Tout = S * (F - 1) + L - 2 * pad_left
        w = _rows(g, B, N, ldt, F)
        m = torch.rand(B, n_src, N, ldt, generator=g, dtype=torch.float64)
        m[..., F:] = 0
        m = m.float()
        D = (_rn(g, N, Cout, L) * _mags(g, N, 1, 1)).float()
        geo = [V("B", B), V("n_src", n_src), V("N", N), V("Cout", Cout), V("L", L), V("S", S), V("F", F), V("ldt", ldt), V("Tout", Tout), V("pad_left", pad_left)]
        if op == "decoder_fwd":
            lat = _nan(B, n_src, N, ldt) if c["latent"] else None
            return [("w", "in", w), ("m", "in", m), ("D", "in", D), ("est", "out", _nan(B, n_src, Cout, Tout)), ("latent", "out" if c["latent"] else "val", lat)] + geo
        d_est = (_rn(g, B, n_src, Cout, Tout) * _mags(g, B, n_src, Cout, 1)).float()
        return [("d_est", "in", d_est), ("w", "in", w), ("m", "in", m), ("D", "in", D), ("dpre", "out", _nan(B, n_src * N, ldt)), ("dwm", "out", _nan(B, N, ldt))] + geo + \
               [V("raw_mask", c["raw_mask"])]
    if op in ("depthwise_fwd", "depthwise_bwd_input", "depthwise_bwd_weight"):
        B, C, Tin, Tout, Kw = (c[k] for k in ("B", "C", "Tin", "Tout", "Kw"))
        geo = [V("B", B), V("C", C), V("Tin", Tin), V("Tout", Tout), V("Kw", Kw), V("stride", c["stride"]), V("pad", c["pad"]), V("dil", c["dil"])]
        x, w, bias = _rows(g, B, C, Tin, Tin), _rn(g, C, 1, Kw).float(), _rn(g, C).float()
        dy = _rows(g, B, C, Tout, Tout)
        if op == "depthwise_fwd":
            return [("x", "in", x), ("w", "in", w), ("bias", "in" if c["bias"] else "val", bias if c["bias"] else None), ("y", "out", _nan(B, C, Tout))] + geo
        if op == "depthwise_bwd_input":
            return [("dy", "in", dy), ("w", "in", w), ("dx", "out", _nan(B, C, Tin))] + geo
        return [("dy", "in", dy), ("x", "in", x), ("partial", "out", _nan(B, C, Kw + 1))] + geo
    if op == "split_rows":
        B, C, T, ldt, k = (c[k] for k in ("B", "C", "T", "ldt", "k"))
        x = _rows(g, B, C, ldt, T)
        x[0, 1] = 0                                                     # an all-zero row: exponent 0
        return [("x", "in", x), ("out", "out", torch.full((B, C, ldt), -1, dtype=torch.int32)), ("exps", "out", torch.full((B, C), -77, dtype=torch.int32)),
                ("sums", "out", _nan(B * k, C)), V("B", B), V("C", C), V("T", T), V("ldt", ldt), V("k", k)]
    if op in ("gln_tokens_fwd", "gln_tokens_bwd"):
        nseq, L, C = c["nseq"], c["L"], c["C"]
        x = ((_rn(g, nseq, L, C) + 0.3) * _mags(g, 1, 1, C)).float()
        gamma, beta = (_rn(g, C) + 1.5).float(), _rn(g, C).float()
        import sepkernels
        ws = torch.zeros(max(1, (sepkernels.load().sep_gln_tokens_ws_bytes(nseq, L, C) + 7) // 8), dtype=torch.float64)
        if op == "gln_tokens_fwd":
            return [("x", "in", x), ("gamma", "in", gamma), ("beta", "in", beta), ("y", "out", _nan(nseq, L, C)), ("stats", "out", _nan(nseq, 2)), V("nseq", nseq), V("L", L),
                    V("C", C), V("eps", 1e-8), ("ws", "scratch", ws)]
        v = x.double().reshape(nseq, -1)
        mu = v.mean(1)
        stats = torch.stack([mu, 1.0 / ((v * v).mean(1) - mu * mu + 1e-8).sqrt()], 1).float()
        dy = (_rn(g, nseq, L, C) * _mags(g, 1, 1, C)).float()
        return [("dy", "in", dy), ("x", "in", x), ("gamma", "in", gamma), ("stats", "in", stats), ("dx", "out", _nan(nseq, L, C)), ("part", "out", _nan(nseq, 2, C)),
                V("nseq", nseq), V("L", L), V("C", C), ("ws", "scratch", ws)]
    if op in ("cln_fwd", "cln_stats", "cln_bwd", "depthwise_cln_fwd", "depthwise_cln_bwd_weight"):
        B, C, T, ldt = (c[k] for k in ("B", "C", "T", "ldt"))
        x = _rows(g, B, C, ldt, T, mean=0.4)
        gamma, beta = (_rn(g, C) + 1.5).float(), _rn(g, C).float()
        alpha = torch.tensor([0.25]) if c["alpha"] else None
        A = ("alpha", "in" if c["alpha"] else "val", alpha)
        import sepkernels
        ws = torch.zeros((sepkernels.load().sep_cln_ws_bytes(B, C, T, ldt) + 7) // 8, dtype=torch.float64)
        geo = [V("B", B), V("C", C), V("T", T), V("ldt", ldt)]
        if op == "cln_fwd":
            return [("x", "in", x), ("gamma", "in", gamma), ("beta", "in", beta), ("y", "out", _nan(B, C, ldt)), ("mean", "out", _nan(B, ldt)), ("rstd", "out", _nan(B, ldt)),
                    ("ws", "scratch", ws)] + geo + [V("eps", EPS), A]
        if op == "cln_stats":
            return [("x", "in", x), ("mean", "out", _nan(B, ldt)), ("rstd", "out", _nan(B, ldt)), ("ws", "scratch", ws)] + geo + [V("eps", EPS), A]
        m, r = _cln_stats64(x, alpha, B, C, T, ldt)
        mean, rstd = torch.zeros(B, ldt), torch.zeros(B, ldt)
        mean[:, :T], rstd[:, :T] = m.float(), r.float()
        dy = _rows(g, B, C, ldt, T)
        if op == "cln_bwd":
            return [("dy", "in", dy), ("x", "in", x), ("gamma", "in", gamma), ("mean", "in", mean), ("rstd", "in", rstd), ("dx", "out", _nan(B, C, ldt)),
                    ("dgamma_part", "out", _nan(B, C)), ("dbeta_part", "out", _nan(B, C)), ("ws", "scratch", ws)] + geo + \
                   [V("eps", EPS), A, ("dalpha_part", "out" if c["alpha"] else "val", _nan(B, C) if c["alpha"] else None)]
        Kw = c["Kw"]
        w, bias = _rn(g, C, Kw).float(), _rn(g, C).float()
        tail = geo + [V("Kw", Kw), V("pad", c["pad"]), V("dil", c["dil"])]
        norm = [("x", "in", x), A, ("gamma", "in", gamma), ("beta", "in", beta), ("mean", "in", mean), ("rstd", "in", rstd)]
        if op == "depthwise_cln_fwd":
            return norm + [("w", "in", w), ("bias", "in" if c["bias"] else "val", bias if c["bias"] else None), ("y", "out", _nan(B, C, ldt))] + tail
        return [("dy", "in", dy)] + norm + [("partial", "out", _nan(B, C, Kw + 1))] + tail
    raise KeyError(op)


# ---------------------------------------------------------------------------------------------------------------- the contracts in float64
def _rowsout(ref, valid, pad):
    return dict(kind="rows", ref=ref, valid=valid, pad=pad)


def _sums(ref, mag, pre=None):
    return dict(kind="sums", ref=ref, abs=mag, pre=pre)


def _slot_totals(t):
    return t.double().reshape(-1, SLOTS, 2).sum(1)


def _ref_encoder(c, a):
    torch = _t()
    B, Cin, Tin, N, L, S, F, ldt, pad_left = (c[k] for k in ("B", "Cin", "Tin", "N", "L", "S", "F", "ldt", "pad_left"))
    xp = torch.zeros(B, Cin, max(S * (F - 1) + L, pad_left + Tin), dtype=torch.float64)
    xp[:, :, pad_left:pad_left + Tin] = a["x"].double()
    idx = (torch.arange(F) * S).view(1, F) + torch.arange(L).view(L, 1)
    y = torch.einsum("nq,bqf->bnf", a["E"].double().reshape(N, Cin * L), xp[:, :, idx].reshape(B, Cin * L, F))
    if c["relu"]:
        y = y.clamp_min(0)
    w = torch.zeros(B, N, ldt, dtype=torch.float64)
    w[..., :F] = y
    prior = _slot_totals(a["stats"])
    return dict(w=_rowsout(w, F, "zero"),
                stats=_sums(prior + torch.stack([y.sum((1, 2)), (y * y).sum((1, 2))], 1), prior.abs() + torch.stack([y.abs().sum((1, 2)), (y * y).sum((1, 2))], 1), _slot_totals))


def _v1(c, a):
    """gLN1(PReLU(a)) on the valid frames, float64"""
    C, T = c["C"], c["T"]
    mu, r = _mu_rstd(a["stats1"], float(C * T))
    u1 = _prelu(a["a"].double()[..., :T], a["alpha1"].double())
    sc = a["gamma1"].double().view(1, C, 1) * r
    return u1, u1 * sc + (a["beta1"].double().view(1, C, 1) - mu * sc)


def _ref_dwconv_fwd(c, a):
    torch = _t()
    B, C, T, ldt, d = (c[k] for k in ("B", "C", "T", "ldt", "d"))
    _, v = _v1(c, a)
    wk = a["wd"].double().reshape(C, 3)
    w0, w1, w2 = (wk[:, k].view(1, C, 1) for k in range(3))
    vm, vp = _shift(v, -d), _shift(v, d)
    bd = a["bd"].double().view(1, C, 1)
    zz = bd + w0 * vm + w1 * v + w2 * vp
    z = torch.zeros(B, C, ldt, dtype=torch.float64)
    z[..., :T] = zz
    u = _prelu(zz, a["alpha2"].double())
    prior = _slot_totals(a["stats2"])
    return dict(z=dict(_rowsout(z, T, "zero"), scale=bd.abs() + w0.abs() * vm.abs() + w1.abs() * v.abs() + w2.abs() * vp.abs()),
                stats2=_sums(prior + torch.stack([u.sum((1, 2)), (u * u).sum((1, 2))], 1), prior.abs() + torch.stack([u.abs().sum((1, 2)), (u * u).sum((1, 2))], 1), _slot_totals))


def _ref_dwconv_bwd(c, a):
    torch = _t()
    B, C, T, ldt, d = (c[k] for k in ("B", "C", "T", "ldt", "d"))
    cnt = float(C * T)
    u1, v1 = _v1(c, a)
    recompute = c["name"].endswith(",true>")
    if recompute:            # the kernel forms z = bd + depthwise(v1) again from `a`
        fw = _ref_dwconv_fwd(c, dict(a, stats2=torch.zeros(B, SLOTS, 2, dtype=torch.float64)))
        zz, zscale = fw["z"]["ref"][..., :T], fw["z"]["scale"]
    else:
        zz, zscale = a["z"].double()[..., :T], None
    mu2, r2 = _mu_rstd(a["stats2"], cnt)
    al2 = a["alpha2"].double()
    g = a["dv2"].double()[..., :T]
    xh = (_prelu(zz, al2) - mu2) * r2
    bs2 = a["bsum2"].double()
    du2 = r2 * (a["gamma2"].double().view(1, C, 1) * g - bs2[:, 0].view(B, 1, 1) - xh * bs2[:, 1].view(B, 1, 1))
    dz = du2 * torch.where(zz > 0, torch.ones_like(zz), al2 * torch.ones_like(zz))
    wk = a["wd"].double().reshape(C, 3)
    w0, w1, w2 = (wk[:, k].view(1, C, 1) for k in range(3))
    dv = w0 * _shift(dz, d) + w1 * dz + w2 * _shift(dz, -d)            # dv1[t] = w0 dz[t+d] + w1 dz[t] + w2 dz[t-d]
    dv1 = torch.zeros(B, C, ldt, dtype=torch.float64)
    dv1[..., :T] = dv
    neg = zz <= 0
    terms = [dv, dv * u1, dz, dz * _shift(v1, -d), dz * v1, dz * _shift(v1, d), torch.where(neg, du2 * zz, torch.zeros_like(zz)), torch.zeros_like(zz)]
    rp = torch.stack([t.sum(2) for t in terms], 2)
    mags = [t.abs() for t in terms]
    if recompute:            # z is itself a sum formed inside the kernel: the addends of sum du2 z are du2 bd and du2 wd_k v1[t + (k-1) d]
        mags[6] = torch.where(neg, du2.abs() * zscale, torch.zeros_like(zz))
    rpa = torch.stack([t.sum(2) for t in mags], 2)
    out = dict(dv1=_rowsout(dv1, T, "zero"), rowpart=_sums(rp, rpa, lambda t: t.double().reshape(B, C, -1, 8).sum(2)))
    if c["mode"] != "none":
        g1 = a["gamma1"].double().view(1, C)
        ba = torch.stack([(g1 * rp[..., 0]).sum(1), (g1 * rp[..., 1]).sum(1)], 1)
        baa = torch.stack([(g1.abs() * rpa[..., 0]).sum(1), (g1.abs() * rpa[..., 1]).sum(1)], 1)
        out["bacc1"] = _sums(ba, baa, _slot_totals)
        if c["mode"] == "publish":
            mu1, r1 = _mu_rstd(a["stats1"], cnt)
            mu1, r1 = mu1.view(B), r1.view(B)
            out["bsum1"] = _sums(torch.stack([ba[:, 0] / cnt, r1 * (ba[:, 1] - mu1 * ba[:, 0]) / cnt], 1),
                                 torch.stack([baa[:, 0] / cnt, r1 * (baa[:, 1] + mu1.abs() * baa[:, 0]) / cnt], 1))
            units = C if c["name"] != "dwconv_bwd_tiles" else C * ((ldt + DW_TT - 1) // DW_TT)
            out["arrive1"] = dict(kind="arrive", units=units)
    if recompute:
        out["_sign"] = (zz.abs(), zscale)          # the gate's argument and the magnitude sum of its addends
    out["_taps"] = (w0 * _shift(dz, d), w2 * _shift(dz, -d))      # (for the halo control of tests/test_stream_instances_cpu.py)
    return out


def _decoder_geo(c):
    Tout = c["S"] * (c["F"] - 1) + c["L"] - 2 * c["pad_left"]
    return tuple(c[k] for k in ("B", "n_src", "N", "Cout", "L", "S", "F", "ldt", "pad_left")) + (Tout,)


def _ref_decoder_fwd(c, a):
    torch = _t()
    B, n_src, N, Cout, L, S, F, ldt, pad_left, Tout = _decoder_geo(c)
    wh = a["w"].double().reshape(B, 1, N, ldt) * a["m"].double().reshape(B, n_src, N, ldt)
    wh[..., F:] = 0
    fr = torch.einsum("bsnf,nck->bsckf", wh[..., :F], a["D"].double().reshape(N, Cout, L))
    out = torch.zeros(B, n_src, Cout, S * (F - 1) + L, dtype=torch.float64)
    idx = ((torch.arange(F) * S).view(1, F) + torch.arange(L).view(L, 1)).reshape(-1)
    out.index_add_(3, idx, fr.reshape(B, n_src, Cout, L * F))
    r = dict(est=_rowsout(out[..., pad_left:pad_left + Tout].contiguous(), Tout, None))
    if c["latent"]:
        r["latent"] = _rowsout(wh, F, "zero")
    return r


def _ref_decoder_bwd(c, a):
    torch = _t()
    B, n_src, N, Cout, L, S, F, ldt, pad_left, Tout = _decoder_geo(c)
    xp = torch.zeros(B * n_src, Cout, S * (F - 1) + L + pad_left + Tout, dtype=torch.float64)
    xp[:, :, pad_left:pad_left + Tout] = a["d_est"].double().reshape(B * n_src, Cout, Tout)
    idx = (torch.arange(F) * S).view(1, F) + torch.arange(L).view(L, 1)
    fr = xp[:, :, idx].reshape(B * n_src, Cout * L, F)
    dl = torch.zeros(B, n_src, N, ldt, dtype=torch.float64)
    dl[..., :F] = torch.einsum("nq,bqf->bnf", a["D"].double().reshape(N, Cout * L), fr).reshape(B, n_src, N, F)
    mv, wv = a["m"].double().reshape(B, n_src, N, ldt), a["w"].double().reshape(B, 1, N, ldt)
    dp = dl * wv if c["raw_mask"] else dl * wv * mv * (1 - mv)
    dw = (dl * mv).sum(1)
    dp[..., F:] = 0
    dw[..., F:] = 0
    return dict(dpre=_rowsout(dp, F, "zero"), dwm=_rowsout(dw, F, "zero"))


def _depthwise64(x, w, bias, c):
    torch = _t()
    C, Tin, Tout, Kw, stride, pad, dil = (c[k] for k in ("C", "Tin", "Tout", "Kw", "stride", "pad", "dil"))
    need = (Tout - 1) * stride + (Kw - 1) * dil + 1
    xp = torch.nn.functional.pad(x, (pad, max(0, need - pad - Tin)))
    return torch.nn.functional.conv1d(xp, w.reshape(C, 1, Kw), bias, stride=stride, dilation=dil, groups=C)[:, :, :Tout]


def _ref_depthwise(c, a):
    torch = _t()
    B, C, Tin, Tout, Kw, stride, pad, dil = (c[k] for k in ("B", "C", "Tin", "Tout", "Kw", "stride", "pad", "dil"))
    if c["op"] == "depthwise_fwd":
        return dict(y=_rowsout(_depthwise64(a["x"].double(), a["w"].double(), a["bias"].double() if a["bias"] is not None else None, c), Tout, None))
    if c["op"] == "depthwise_bwd_input":
        with torch.enable_grad():
            x0 = torch.zeros(B, C, Tin, dtype=torch.float64, requires_grad=True)
            gx = torch.autograd.grad(_depthwise64(x0, a["w"].double(), None, c), x0, a["dy"].double())[0]
        return dict(dx=_rowsout(gx, Tin, None))
    g = a["dy"].double()
    xp = torch.zeros(B, C, Tin + 2 * pad + Kw * dil + Tout * stride, dtype=torch.float64)
    xp[:, :, pad:pad + Tin] = a["x"].double()
    to = torch.arange(Tout)
    terms = [g * xp[:, :, to * stride + k * dil] for k in range(Kw)] + [g]
    return dict(partial=_sums(torch.stack([t.sum(2) for t in terms], 2), torch.stack([t.abs().sum(2) for t in terms], 2)))


def _f16_toward_zero(v):
    """float64 -> the fp16 value nearest to v that is not larger in magnitude: (its 16 bits as int64, its value as float64)"""
    torch = _t()
    h = v.to(torch.float16)
    bits = h.view(torch.int16).to(torch.int64) & 0xFFFF
    bits = torch.where(h.double().abs() > v.abs(), bits - 1, bits)            # sign and magnitude: one step down in the bits is one step toward zero
    return bits, torch.where(bits >= 0x8000, bits - 0x10000, bits).to(torch.int16).view(torch.float16).double()


def _ref_split_rows(c, a):
    torch = _t()
    B, C, T, ldt, k = (c[k] for k in ("B", "C", "T", "ldt", "k"))
    x = a["x"].double().clone()
    x[..., T:] = 0
    m = x.abs().amax(2)
    ex = torch.where(m > 0, 13 - torch.frexp(m)[1], torch.zeros_like(m, dtype=torch.int32)).to(torch.int32)
    wv = x * 2.0 ** ex.double().unsqueeze(2)
    hb, hv = _f16_toward_zero(wv)
    lb, _ = _f16_toward_zero(wv - hv)
    pack = lambda b: (b[..., 0::2] | (b[..., 1::2] << 16)).reshape(B, C, ldt // 32, 16)       # frame t in the low half of its word
    words = torch.cat([pack(hb), pack(lb)], 3).reshape(B, C, ldt)
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words)
    xs = x.reshape(B, C, k, ldt // k)
    sums = xs.sum(3).permute(0, 2, 1).reshape(B * k, C)
    return dict(out=dict(kind="ints", ref=words.to(torch.int32)), exps=dict(kind="ints", ref=ex),
                sums=_sums(sums, xs.abs().sum(3).permute(0, 2, 1).reshape(B * k, C)))


def _ref_gln_tokens(c, a):
    torch = _t()
    nseq, L, C = c["nseq"], c["L"], c["C"]
    x = a["x"].double()
    tok = lambda t: t.permute(0, 2, 1).contiguous()                     # (nseq, L, C) -> rows (nseq, C) of L frames
    pre = lambda t: tok(t.double().reshape(nseq, L, C))
    if c["op"] == "gln_tokens_fwd":
        v = x.reshape(nseq, -1)
        m = v.mean(1)
        r = 1.0 / ((v * v).mean(1) - m * m + 1e-8).sqrt()
        y = (x - m.view(nseq, 1, 1)) * r.view(nseq, 1, 1) * a["gamma"].double().view(1, 1, C) + a["beta"].double().view(1, 1, C)
        return dict(y=dict(_rowsout(tok(y), L, None), pre=pre), stats=_sums(torch.stack([m, r], 1), torch.stack([v.abs().mean(1), r], 1)))
    mu, rs = a["stats"].double()[:, 0].view(nseq, 1, 1), a["stats"].double()[:, 1].view(nseq, 1, 1)
    g = a["dy"].double()
    xh = (x - mu) * rs
    gg = g * a["gamma"].double().view(1, 1, C)
    m1, m2 = gg.mean((1, 2), keepdim=True), (gg * xh).mean((1, 2), keepdim=True)
    dx = rs * (gg - m1 - xh * m2)
    return dict(dx=dict(_rowsout(tok(dx), L, None), pre=pre),
                part=_sums(torch.stack([(g * xh).sum(1), g.sum(1)], 1), torch.stack([(g * xh).abs().sum(1), g.abs().sum(1)], 1)))


def _cln_stats64(x, alpha, B, C, T, ldt):
    torch = _t()
    v = x.double().reshape(B, C, ldt)[..., :T]
    if alpha is not None:
        v = _prelu(v, alpha.double())
    n = torch.arange(1, T + 1, dtype=torch.float64) * C
    m = v.sum(1).cumsum(1) / n
    var = ((v * v).sum(1).cumsum(1) / n - m * m).clamp_min(0)
    return m, 1.0 / (var.sqrt() + EPS)


def _padded(v, ldt):
    torch = _t()
    out = torch.zeros(v.shape[:-1] + (ldt,), dtype=torch.float64)
    out[..., :v.shape[-1]] = v
    return out


def _ref_cln(c, a):
    torch = _t()
    B, C, T, ldt = (c[k] for k in ("B", "C", "T", "ldt"))
    al = a["alpha"].double() if a.get("alpha") is not None else None
    x = a["x"].double()[..., :T]
    if c["op"] in ("cln_fwd", "cln_stats"):
        m, r = _cln_stats64(a["x"], a.get("alpha"), B, C, T, ldt)
        out = dict(mean=_rowsout(_padded(m, ldt), T, "keep"), rstd=_rowsout(_padded(r, ldt), T, "keep"))
        if c["op"] == "cln_fwd":
            u = _prelu(x, al) if al is not None else x
            out["y"] = _rowsout(_padded((u - m.unsqueeze(1)) * r.unsqueeze(1) * a["gamma"].double().view(1, C, 1) + a["beta"].double().view(1, C, 1), ldt), T, "zero")
        return out
    g = a["dy"].double()[..., :T]
    v = _prelu(x, al) if al is not None else x
    m, r = a["mean"].double()[:, :T].unsqueeze(1), a["rstd"].double()[:, :T].unsqueeze(1)
    gh = g * a["gamma"].double().view(1, C, 1)
    A, Bq = gh.sum(1), (gh * (v - m)).sum(1)
    n = torch.arange(1, T + 1, dtype=torch.float64) * C
    sigma = 1.0 / r[:, 0] - EPS
    Dq = torch.where(sigma > 0, -Bq * r[:, 0] ** 2 / (2 * sigma.clamp_min(1e-300)), torch.zeros_like(Bq))
    Dm = -r[:, 0] * A - 2 * m[:, 0] * Dq
    P = (Dm / n).flip(1).cumsum(1).flip(1).unsqueeze(1)
    Q = (Dq / n).flip(1).cumsum(1).flip(1).unsqueeze(1)
    du = gh * r + P + 2 * v * Q
    out = {}
    if al is not None:
        t = torch.where(x <= 0, du * x, torch.zeros_like(du))
        out["dalpha_part"] = _sums(t.sum(2), t.abs().sum(2))
        du = du * torch.where(x > 0, torch.ones_like(x), al * torch.ones_like(x))
    out["dx"] = _rowsout(_padded(du, ldt), T, "zero")
    t = g * (v - m) * r
    out["dgamma_part"] = _sums(t.sum(2), t.abs().sum(2))
    out["dbeta_part"] = _sums(g.sum(2), g.abs().sum(2))
    return out


def _ref_causal(c, a):
    torch = _t()
    B, C, T, ldt, Kw, pad, dil = (c[k] for k in ("B", "C", "T", "ldt", "Kw", "pad", "dil"))
    x = a["x"].double()[..., :T]
    u = _prelu(x, a["alpha"].double()) if a.get("alpha") is not None else x
    v1 = a["gamma"].double().view(1, C, 1) * (u - a["mean"].double()[:, :T].unsqueeze(1)) * a["rstd"].double()[:, :T].unsqueeze(1) + a["beta"].double().view(1, C, 1)
    taps = [_shift(v1, k * dil - pad) for k in range(Kw)]
    w = a["w"].double().reshape(C, Kw) if "w" in a else None
    if c["op"] == "depthwise_cln_fwd":
        y = sum(w[:, k].view(1, C, 1) * taps[k] for k in range(Kw))
        if a.get("bias") is not None:
            y = y + a["bias"].double().view(1, C, 1)
        return dict(y=_rowsout(_padded(y, ldt), T, "zero"))
    g = a["dy"].double()[..., :T]
    terms = [g * t for t in taps] + [g]
    return dict(partial=_sums(torch.stack([t.sum(2) for t in terms], 2), torch.stack([t.abs().sum(2) for t in terms], 2)))


REFERENCE = {"encoder_fwd": _ref_encoder, "dwconv_fwd": _ref_dwconv_fwd, "dwconv_bwd": _ref_dwconv_bwd, "decoder_fwd": _ref_decoder_fwd, "decoder_bwd": _ref_decoder_bwd,
             "depthwise_fwd": _ref_depthwise, "depthwise_bwd_input": _ref_depthwise, "depthwise_bwd_weight": _ref_depthwise, "split_rows": _ref_split_rows,
             "gln_tokens_fwd": _ref_gln_tokens, "gln_tokens_bwd": _ref_gln_tokens, "cln_fwd": _ref_cln, "cln_stats": _ref_cln, "cln_bwd": _ref_cln,
             "depthwise_cln_fwd": _ref_causal, "depthwise_cln_bwd_weight": _ref_causal}


def reference(c, args):
    """the contract in float64 on the operands as they are BEFORE the call -> {output name: description}"""
    return REFERENCE[c["op"]](c, {n: v for (n, _, v) in args})


def sign_margin(c, ref):
    """smallest |argument| / (bound * magnitude sum of its addends) over the sign-sensitive gate arguments of the case; inf where it has none"""
    if "_sign" not in ref:
        return float("inf")
    z, scale = ref["_sign"]
    return float((z / (FAMILIES[c["family"]]["bound"] * scale + 1e-300)).min())


_PREPARED = {}


def prepare(c, seed):
    key = (c["id"], c["name"], seed)
    if key not in _PREPARED:
        if len(_PREPARED) > 4:
            _PREPARED.clear()
        args = operands(c, seed)
        _PREPARED[key] = (args, reference(c, args))
    return _PREPARED[key]


def find_seed(c):
    """the first of SEEDS seeds whose operands keep every sign-sensitive argument clear of zero"""
    if not c["name"].endswith(",true>"):
        return zlib.crc32("stream/{}".format(c["id"]).encode())
    for k in range(SEEDS):
        seed = zlib.crc32("stream/{}/{}".format(c["id"], k).encode())
        if sign_margin(c, prepare(c, seed)[1]) >= 1.0:
            return seed
    raise AssertionError("no seed in {} keeps the gate arguments of case {} clear of zero".format(SEEDS, c))


# ---------------------------------------------------------------------------------------------------------------- the check
def measure(desc, got):
    """one output in the metric of its kind -> dict(err, pads_ok)"""
    torch = _t()
    kind = desc["kind"]
    if desc.get("pre") is not None:
        got = desc["pre"](got)
    if kind == "ints":
        return dict(err=0.0 if torch.equal(got.reshape(desc["ref"].shape).to(desc["ref"].dtype), desc["ref"]) else float("inf"), pads_ok=True)
    if kind == "arrive":
        arr = got.reshape(-1, ARRIVE)
        units = arr[:, :SLOTS].sum(1)                 # every workgroup of a sample arrived exactly once; the last arrival of every used slot went up
        ok = bool((units == desc["units"]).all()) and bool((arr[:, SLOTS] == min(SLOTS, desc["units"])).all())
        return dict(err=0.0 if ok else float("inf"), pads_ok=True)
    ref = desc["ref"]
    got = got.double().reshape(ref.shape)
    if kind == "sums":
        if not torch.isfinite(got).all():
            return dict(err=float("inf"), pads_ok=True)
        diff, mag = (got - ref).abs(), desc["abs"]
        ratio = torch.where(mag > 0, diff / mag.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
        return dict(err=float(ratio.max()), pads_ok=True)
    W, V = ref.shape[-1], desc["valid"]
    g2, r2 = got.reshape(-1, W), ref.reshape(-1, W)
    pads_ok = True
    if desc["pad"] == "zero":
        pads_ok = bool((g2[:, V:] == 0).all())
    elif desc["pad"] == "keep":
        pads_ok = bool(torch.isnan(g2[:, V:]).all())
    gv, rv = g2[:, :V], r2[:, :V]
    if not torch.isfinite(gv).all():
        return dict(err=float("inf"), pads_ok=pads_ok)
    diff, den = (gv - rv).abs().amax(1), rv.abs().amax(1)
    ratio = torch.where(den > 0, diff / den.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))
    return dict(err=float(ratio.max()), row=int(ratio.argmax()), pads_ok=pads_ok)


def global_max_metric(desc, got):
    """the figure of the older kernel tests (both() of tests/test_gpu_kernels.py): max |got - ref| over the global maximum of the reference"""
    if desc.get("pre") is not None:
        got = desc["pre"](got)
    ref = desc["ref"]
    return float((got.double().reshape(ref.shape) - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------- running a case
def _guarded(t, to_device):
    """the device's copy of `t` between two guard bands -> (whole buffer, view of the middle)"""
    torch = _t()
    flat = torch.full((t.numel() + 2 * GUARD,), GUARD_VALUE if t.dtype.is_floating_point else int(GUARD_VALUE), dtype=t.dtype)
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1)
    flat = to_device(flat)
    return flat, flat[GUARD:GUARD + t.numel()].view(t.shape)


def _guards_intact(flat):
    f = flat.cpu()
    g = GUARD_VALUE if f.dtype.is_floating_point else int(GUARD_VALUE)
    return bool((f[:GUARD] == g).all()) and bool((f[-GUARD:] == g).all())


def call(K, op, values):
    """the entry point through the backend K (sep_split_rows: through the library handle, the binding's method allocates its own outputs)"""
    if op != "split_rows":
        return getattr(K, op)(*values)
    import sepkernels
    torch = _t()
    x, out, exps, sums, B, C, T, ldt, k = values
    if getattr(K, "name", "") == "emulator":
        xs = x.reshape(B, C, ldt).clone()
        xs[..., T:] = 0
        sums.copy_(xs.reshape(B, C, k, ldt // k).sum(3).permute(0, 2, 1).reshape(B * k, C))
        ref = _ref_split_rows(dict(B=B, C=C, T=T, ldt=ldt, k=k), dict(x=x))          # (the integer outputs have no fp32 arithmetic to emulate)
        out.copy_(ref["out"]["ref"])
        exps.copy_(ref["exps"]["ref"])
        return None
    P = sepkernels._ptr
    sepkernels._check(sepkernels.load().sep_split_rows(P(x, torch.float32), P(out, torch.int32), P(exps, torch.int32), P(sums, torch.float32), B, C, T, ldt, k,
                                                       sepkernels._stream()), "sep_split_rows")


def emulator():
    """tests/emulator.py plus the three calls it lacks, composed from its own pieces in the buffers' dtype"""
    torch = _t()
    from emulator import EmuBackend, _prelu as eprelu

    class Emu(EmuBackend):
        def cln_stats(self, x, mean, rstd, ws, B, C, T, ldt, eps, alpha=None):
            EmuBackend.cln_fwd(self, x, torch.ones(C, dtype=x.dtype), torch.zeros(C, dtype=x.dtype), torch.empty(B, C, ldt, dtype=x.dtype), mean, rstd, ws, B, C, T, ldt, eps,
                               alpha=alpha)

        @staticmethod
        def _v1(x, alpha, gamma, beta, mean, rstd, B, C, T, ldt):
            u = eprelu(x, alpha) if alpha is not None else x
            v = torch.zeros(B, C, ldt, dtype=x.dtype)
            v[:, :, :T] = ((u.reshape(B, C, ldt) - mean.reshape(B, 1, ldt)) * rstd.reshape(B, 1, ldt) * gamma.view(1, C, 1) + beta.view(1, C, 1))[:, :, :T]
            return v

        def depthwise_cln_fwd(self, x, alpha, gamma, beta, mean, rstd, w, bias, y, B, C, T, ldt, Kw, pad, dil):
            out = self._depthwise(self._v1(x, alpha, gamma, beta, mean, rstd, B, C, T, ldt), w, bias, C, ldt, ldt, Kw, 1, pad, dil).clone()
            out[:, :, T:] = 0
            y.reshape(B, C, ldt).copy_(out)

        def depthwise_cln_bwd_weight(self, dy, x, alpha, gamma, beta, mean, rstd, partial, B, C, T, ldt, Kw, pad, dil):
            g = dy.reshape(B, C, ldt).clone()
            g[:, :, T:] = 0
            EmuBackend.depthwise_bwd_weight(self, g, self._v1(x, alpha, gamma, beta, mean, rstd, B, C, T, ldt), partial, B, C, ldt, ldt, Kw, 1, pad, dil)
    return Emu()


def _another_name(K, to_device, avoid):
    """a tiny call of another family in front of every case, so that a case whose dispatcher stores no name cannot inherit the right one"""
    torch = _t()
    if avoid != "encoder<0>":
        K.encoder_fwd(to_device(torch.zeros(1, 1, 8)), to_device(torch.zeros(1, 1, 2)), to_device(torch.zeros(1, 1, 128)), to_device(torch.zeros(1, SLOTS, 2, dtype=torch.float64)),
                      1, 1, 8, 1, 2, 1, 7, 128, 0, 0)
    else:
        K.depthwise_fwd(to_device(torch.zeros(1, 1, 8)), to_device(torch.zeros(1, 1, 2)), None, to_device(torch.zeros(1, 1, 4)), 1, 1, 8, 4, 2, 2, 0, 1)


def run_case(K, c, to_device, sync, tamper=None):
    """one case through the backend K -> its record.  `tamper(outputs, args, ref)`: the controls of the checker alter the device's results"""
    torch = _t()
    import sepkernels
    args, ref = prepare(c, c["seed"])
    held, values = {}, []
    for (n, role, v) in args:
        if role == "val":
            values.append(v)
        else:
            held[n] = _guarded(v, to_device)
            values.append(held[n][1])
    emu = getattr(K, "name", "") == "emulator"
    if not emu:
        _another_name(K, to_device, c["name"])
    call(K, c["op"], values)
    kernel = c["name"] if emu else sepkernels.last_kernel()
    sync()
    rec = dict(case={k: v for k, v in c.items()}, kernel=kernel, outputs={}, pads_zero=True, inputs_intact=True, guards_intact=True)
    got = {n: held[n][1].cpu() for (n, role, _) in args if role == "out"}
    if tamper is not None:
        tamper(got, {n: v for (n, _, v) in args}, ref)
    bound = FAMILIES[c["family"]]["bound"]
    for name, g in got.items():
        m = measure(ref[name], g)
        rec["outputs"][name] = dict(err=m["err"], bound=bound)
        rec["pads_zero"] = rec["pads_zero"] and m["pads_ok"]
    for (n, role, v) in args:
        if role == "val":
            continue
        rec["guards_intact"] = rec["guards_intact"] and _guards_intact(held[n][0])
        if role == "in" and not torch.equal(held[n][1].cpu(), v):
            rec["inputs_intact"] = False
    rec["ok"] = (kernel == c["name"] and rec["pads_zero"] and rec["inputs_intact"] and rec["guards_intact"] and all(o["err"] <= o["bound"] for o in rec["outputs"].values()))
    return rec


def run(env, K, to_device, sync, log=None, families=None):
    """every case of cases(env) (of the families given) through the backend K, which must live in a process started with ENVS[env]"""
    for k in SWITCHES:
        assert os.environ.get(k) == ENVS[env].get(k), "the process environment is not that of '{}' ({})".format(env, k)
    recs = []
    for c in cases(env):
        if families is not None and c["family"] not in families:
            continue
        rec = run_case(K, c, to_device, sync)
        recs.append(rec)
        if log:
            worst = max([o["err"] / o["bound"] for o in rec["outputs"].values()] or [0.0])
            log("{:4s} {:30s} {}  worst err/bound {:.3f}".format("ok" if rec["ok"] else "FAIL", rec["kernel"], shape_of(c), worst))
    return recs


def shape_of(c):
    return " ".join("{}={}".format(k, v) for k, v in c.items() if k not in ("family", "name", "id", "seed"))


def failures(recs):
    """one line per record that is not ok"""
    out = []
    for r in recs:
        if not r["ok"]:
            c = r["case"]
            bad = {k: v["err"] for k, v in r["outputs"].items() if not v["err"] <= v["bound"]}
            out.append("{} (meant {}) {}: pads_zero={} inputs_intact={} guards_intact={} over the bound {}: {}".format(
                r["kernel"], c["name"], shape_of(c), r["pads_zero"], r["inputs_intact"], r["guards_intact"], FAMILIES[c["family"]]["bound"], bad))
    return out


def emulator_figures(families=None):
    """family -> the fp32 emulator's worst figure against the float64 reference over the family's cases (the e32 of FAMILIES)"""
    emu, worst = emulator(), {}
    for c in cases("default"):
        if families is not None and c["family"] not in families:
            continue
        rec = run_case(emu, c, (lambda t: t.clone()), (lambda: None))
        assert rec["pads_zero"] and rec["inputs_intact"] and rec["guards_intact"], rec
        for name, o in rec["outputs"].items():
            if ref_kind(c, name) in ("rows", "sums"):
                worst[c["family"]] = max(worst.get(c["family"], 0.0), o["err"])
    return worst


def ref_kind(c, name):
    return prepare(c, c["seed"])[1][name]["kind"]


def child_command(env, out, backend=None):
    """(argv, process environment) of the child that runs one environment"""
    penv = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    penv.update(ENVS[env])
    argv = [sys.executable, os.path.abspath(__file__), "--env", env, "--out", out]
    return argv + (["--backend", backend] if backend else []), penv


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", default="default", choices=sorted(ENVS))
    ap.add_argument("--out", default=None)
    ap.add_argument("--backend", default="hip", help="hip (default) or hostsim:<path of the host-simulation library>")
    ap.add_argument("--measure", action="store_true", help="print the fp32 emulator's worst figure per family and the bound that follows (FAMILIES)")
    args = ap.parse_args()
    for k in SWITCHES:                            # the switches are read once per process, at the first call
        os.environ.pop(k, None)
    os.environ.update(ENVS[args.env])
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import sepkernels
    if args.measure:
        for f, e in emulator_figures().items():
            print("{:12s} e32 = {:.3e}  bound = {!r}  (in the ledger: {})".format(f, e, bound_rule(e), FAMILIES[f]))
        return 0
    log = lambda s: print(s, flush=True)
    if args.backend.startswith("hostsim:"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import hostsim
        with hostsim.HostSimBackend(args.backend[8:]) as K:
            recs = run(args.env, K, (lambda t: t.clone()), (lambda: None), log)
    else:
        recs = run(args.env, sepkernels.HipBackend(), (lambda t: t.cuda()), torch.cuda.synchronize, log)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(recs, fh)
    bad = failures(recs)
    for line in bad:
        print("FAIL", line)
    print("{}: {} cases, {} failures; reached: {}".format(args.env, len(recs), len(bad), " ".join(sorted(set(r["kernel"] for r in recs)))))
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
