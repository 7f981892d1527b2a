"""Helper module (not a test file): the ledger of the kernel instances behind the entry points of the dual-path separators (DPRNN-TasNet, DPTNet,
GALRNet, SepFormer) -- csrc/linear.hip, csrc/lstm.hip, csrc/attn.hip and csrc/rownorm.hip --, a case matrix that reaches every one of them BY NAME
(sep_last_kernel), a restatement of every call's contract as ONE function of a dtype, and a metric local enough that one wrong token row, one wrong
sequence or one wrong weight-gradient slab cannot hide behind a louder one.  tests/test_dualpath_instances_cpu.py runs the matrix on the host
simulation of the kernel sources, tests/test_dualpath_instances_gpu.py on the MI355X; the children of either start

    python tests/dualpath_matrix.py --env NAME --out FILE [--backend hostsim:<library>]

once per value of SEPK_LSTM_NS4, which the LSTM dispatcher reads once per process.  Built on the plan of tests/stream_matrix.py.

THE LEDGER.  INSTANCES is every name the four dispatchers can emit, the kernel and its template arguments as spelled at the launch (attn_bwd<D,ML,NW>
is ONE name for the q / kv pair of launches).  dispatch(env, case) restates the four dispatch tables by hand; cases() refuses a matrix that misses
an instance.  Under the default environment the LSTM cases reach both sweep kernels through the SEP_LSTM_FORCE16 / SEP_LSTM_FORCE4 bits; cases
without a force bit pin the automatic rule at its boundary (256 four-sequence workgroups) and are what the two SEPK_LSTM_NS4 environments move.

THE REFERENCE.  contract(case, inputs, dtype) evaluates the contract of include/sepkernels.h in torch on the fp32 inputs: its float64 run is the
reference, its float32 run is e32 (NOT tests/emulator.py: its attention and parts of its rownorm already compute in double).  The dropout masks are
restated from the two hashes (keep_attn, keep_flat).  The inputs a backward call takes from its forward (gates and cell states, o and lse, s and
stat) are the float64 forward's results rounded to fp32 -- identical on both sides.

THE METRIC (after DESIGN.md 4.2: a contraction's error is relative to the sum of the magnitudes of its addends).  Every output is described as
  elem   |got - ref| <= bound * scale, element by element, where scale is the magnitude sum of the element's own contraction:
           linear      sum_k |a||b| + |bias| + |bias2| + |prior dx|; every weight-gradient slab by itself with its own scale, a slab beyond the
                       last token (scale 0) exactly zero; partial_bias against sum |dy| of the slab
           attention   o against sum_k P~ |v| (P~: the probabilities after the dropout scaling); dq, dk, dv against scale sum |dS|~ |k|,
                       scale sum |dS|~ |q|, sum P~ |dO|; lse against 1 + max_k |s|; delta is scratch: finite and inside its guards.
                       (|dS|~ = P (sum_d |dO||v| / (1 - p) [kept] + sum_d |dO||O|): dS = P (dP~ - delta) is formed inside the kernel from a
                       difference that cancels where the softmax is peaked and is exactly zero at L = 1, so its own addends are what an fp32
                       evaluation is relative to -- with |dS| itself the float32 run of the contract misses every peaked case by orders.)
           rownorm     y against |gamma| rstd (|s| + |mu|) + |beta|; s against |x| + |drop(res)|; stat against |mu| + max |s| and against rstd;
                       ds, dres against rstd (|dy gamma| + mean_c |dy gamma| + |xhat| mean_c |dy gamma xhat|) -- element by element, never more
                       than the row's rstd sum_c |dy gamma| (1 + |xhat|); dres exactly zero where the mask drops; part summed over the slabs
                       against the sum of the addends' magnitudes, every slab finite and fully written
         a place whose scale is zero must hold the reference exactly.
  seq    the LSTM outputs, per sequence (and direction): max_(t,u) |got - ref| <= bound * max_(t,u) |ref|
  same   bit for bit the result of the saving call (gates = cstate = NULL, s = NULL)
  exact  chunk_tokens: the permutation; relu_drop: the mask exact and the values within ONE fp32 rounding (2^-24) of the float64 formula
Every device buffer sits between two guard bands of a fixed value (token rows >= ntok and sequences >= nseq lie there), every pure output starts as
NaN; after the call the guards and the inputs must be untouched.  Every token row, weight row, sequence and attention key row carries its own
magnitude, 2^-6 .. 2^6 (the LSTM's xg 2^-3 .. 2^3, so that it is not all saturated): a loud row cannot mask a quiet one.

THE BOUND, per family and output: min(the tolerance the older test of tests/test_gpu_kernels.py grants that output (OLD), 4 * e32 rounded up to a
power of two), e32 being the float32 run's worst figure against the float64 run over the family's cases (`--measure`), written into FAMILIES;
tests/test_dualpath_instances_cpu.py recomputes it and holds the table to the rule (stream_matrix.bound_rule).

HOST TIER.  Every instance is reached on the host simulation too.  Cases flagged device-only: the relu_drop case that wraps the grid (a million
float4s on host threads) and the L = 40 LSTM case; no other case proved too slow.  The attention cases of L >= 257 run with N = H = 1 there."""
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

GUARD = 1024                                     # elements in front of and behind every device buffer
GUARD_VALUE = 12345.0
FORCE16, FORCE4, INTERLEAVED = 0x100, 0x200, 0x400
ONE_ROUNDING = 2.0 ** -24
ROWNORM_EPS = 1e-5

# family: the float32 run's worst figure against the float64 run over the family's cases, and the bound that follows from it
FAMILIES = {
    "linear": dict(e32=1.3e-06, bound=2.0 ** -17),
    "lstm": dict(e32=7.5e-07, bound=2.0 ** -18),
    "attn": dict(e32=1.3e-05, bound=5e-5),
    "rownorm": dict(e32=2.8e-06, bound=2.0 ** -16),
    "relu_drop": dict(e32=None, bound=ONE_ROUNDING),      # one fp32 rounding: the precision of the format, not a measured figure
    "chunk_tokens": dict(e32=None, bound=0.0),            # a permutation
}
# what the older tests (tests/test_gpu_kernels.py) grant each output
OLD = {"linear": {None: 2e-4}, "lstm": {None: 2e-4}, "attn": {"o": 2e-5, "lse": 2e-5, "dqkv": 5e-5},
       "rownorm": {"y": 2e-5, "stat": 2e-5, "s": 1e-6, "ds": 5e-5, "dres": 5e-5, "part": 5e-5}}


def bound_rule(e32, old):
    """4 x the float32 run's figure, rounded up to a power of two, never looser than what the older test grants"""
    return min(old, 2.0 ** math.ceil(math.log2(4 * e32))) if e32 > 0 else old


def bound_of(family, output):
    f = FAMILIES[family]
    if f["e32"] is None:
        return f["bound"]
    old = OLD[family]
    return min(old.get(output, old.get(None, max(old.values()))), f["bound"])


ENVS = {"default": {}, "lstm_ns4_0": {"SEPK_LSTM_NS4": "0"}, "lstm_ns4_1": {"SEPK_LSTM_NS4": "1"}}
SWITCHES = ("SEPK_LSTM_NS4",)
ENV_FAMILIES = {"default": tuple(FAMILIES), "lstm_ns4_0": ("lstm",), "lstm_ns4_1": ("lstm",)}

INSTANCES = sorted(
    ["linear<{},{},{}>".format(m, ti, tj) for m, tiles in (("fwd", ((128, 128), (128, 64))), ("bwd_input", ((128, 128), (128, 64))),
                                                           ("bwd_weight", ((128, 128), (128, 64), (64, 128), (64, 64)))) for ti, tj in tiles] +
    ["chunk_tokens<true>", "chunk_tokens<false>"] +
    ["lstm_{}<{}>".format(k, H) for k in ("fwd", "fwd4", "bwd", "bwd4") for H in (16, 32, 64, 128)] +
    ["attn_{}<{},{},{}>".format(k, D, ml, nw) for k in ("fwd", "bwd") for D in (8, 16, 32) for ml, nw in ((64, 2), (128, 4), (256, 8), (320, 8))] +
    ["rownorm_{}<{}>".format(k, nj) for k in ("fwd", "bwd") for nj in (1, 2, 3, 4)] +
    ["relu_drop_fwd", "relu_drop_bwd"])


# ---------------------------------------------------------------------------------------------------------------- the dispatch tables, restated
def dispatch(env, c):
    """the instance name the entry point gives the case under the environment `env` (a dict of the SEPK_* switches)"""
    op = c["op"]
    if op == "linear_fwd":
        return "linear<fwd,128,{}>".format(128 if c["N"] % 128 == 0 else 64)
    if op == "linear_bwd_input":
        return "linear<bwd_input,128,{}>".format(128 if c["K"] % 128 == 0 else 64)
    if op == "linear_bwd_weight":
        return "linear<bwd_weight,{},{}>".format(128 if c["N"] % 128 == 0 else 64, 128 if c["K"] % 128 == 0 else 64)
    if op in ("chunk_to_tokens", "tokens_to_chunk"):
        return "chunk_tokens<{}>".format("true" if op == "chunk_to_tokens" else "false")
    if op in ("lstm_fwd", "lstm_bwd"):
        force, rev = (c["reverse"] >> 8) & 3, c["reverse"] & 0xff
        if force:
            four = force == 2
        elif env.get("SEPK_LSTM_NS4") in ("0", "1"):
            four = env["SEPK_LSTM_NS4"] == "1"
        else:
            four = (c["nseq"] + 3) // 4 * (2 if rev == 2 else 1) <= 256
        return "lstm_{}{}<{}>".format(op[5:], "4" if four else "", c["H"])
    if op in ("attn_fwd", "attn_bwd"):
        L = c["L"]
        ml, nw = (64, 2) if L <= 64 else (128, 4) if L <= 128 else (256, 8) if L <= 256 else (320, 8)
        return "attn_{}<{},{},{}>".format(op[5:], c["D"], ml, nw)
    if op in ("rownorm_fwd", "rownorm_bwd"):
        return "rownorm_{}<{}>".format(op[8:], (c["C"] + 255) // 256)
    if op in ("relu_drop_fwd", "relu_drop_bwd"):
        return op
    raise KeyError(op)


# ---------------------------------------------------------------------------------------------------------------- the case matrix
def _all_cases():
    cs = []
    add = lambda family, op, **kw: cs.append(dict(family=family, op=op, **kw))
    # linear, forward and input gradient: ntok astride the 128-token tile x every contraction length the argument check takes (32 and 96 are no
    # multiple of 64; 192 is three 64-wide column tiles), the output width and the bias combination (accumulate) rotating
    NTOK, WIDTHS = (1, 127, 128, 129, 300), (32, 64, 96, 128, 192)
    for i, ntok in enumerate(NTOK):
        for j, kk in enumerate(WIDTHS):
            out = (64, 128, 192)[(i + j) % 3]
            add("linear", "linear_fwd", ntok=ntok, K=kk, N=out, bias=(i + j) % 2, bias2=((i + 2 * j) // 2) % 2)
            add("linear", "linear_bwd_input", ntok=ntok, K=out, N=kk, accumulate=(i + j) % 2)
    for b, b2 in ((0, 0), (1, 0), (0, 1), (1, 1)):                         # every bias combination at one shape with a ragged tile
        add("linear", "linear_fwd", ntok=129, K=32, N=128, bias=b, bias2=b2)
    # ... weight gradient: shift x L (a sequence boundary inside a chunk, on a chunk edge, every shifted row zero), the four tiles and three 64-wide
    # tiles, nslab in {1, 3, more than there are chunks}, x as the right half of a wider matrix, partial_bias NULL
    TILES = ((128, 128), (128, 64), (64, 128), (64, 64), (192, 192))
    i = 0
    for shift in (-1, 0, 1):
        for L, nseq in ((1, 45), (7, 11), (32, 3)):
            N, K = TILES[i % 5]
            add("linear", "linear_bwd_weight", nseq=nseq, L=L, ntok=nseq * L, K=K, N=N, shift=shift, nslab=(1, 3, 7)[(i + i // 3) % 3], wide=i % 2, pb=int(i % 4 != 3))
            i += 1
    for (N, K), nslab in zip(TILES, (3, 7, 1, 3, 7)):                        # every tile with a shifted x and a boundary inside a chunk
        add("linear", "linear_bwd_weight", nseq=43, L=7, ntok=301, K=K, N=N, shift=(-1, 1)[nslab % 2], nslab=nslab, wide=1, pb=1)
    # chunk_tokens: the shapes of test_chunk_tokens_layout_pair, both sequence axes
    for (B, F, S, K) in [(2, 64, 5, 250), (1, 48, 3, 33), (3, 7, 2, 1), (2, 64, 257, 50)]:
        for inter in (0, 1):
            for op in ("chunk_to_tokens", "tokens_to_chunk"):
                add("chunk_tokens", op, B=B, F=F, S=S, K=K, inter=inter)
    # lstm: every H x {sixteen, four} x every direction mode, forward and backward, nseq and L rotating through {1, 3, 5, 17} x {1, 2, 9}
    NSEQ, LS = (1, 3, 5, 17), (1, 2, 9)
    i = 0
    for H in (16, 32, 64, 128):
        for force in (FORCE16, FORCE4):
            for rev in (0, 1, 2, 2 | INTERLEAVED):
                nseq, L = NSEQ[(i + i // 4) % 4], LS[(i + i // 8) % 3]          # (every direction mode meets every nseq, every H every L)
                for op in ("lstm_fwd", "lstm_bwd"):
                    add("lstm", op, H=H, nseq=nseq, L=L, reverse=rev | force)
                i += 1
    for force in (FORCE16, FORCE4):                                              # (device only: forty steps of 512 host threads)
        for op in ("lstm_fwd", "lstm_bwd"):
            add("lstm", op, H=128, nseq=17, L=40, reverse=2 | force, device_only=1)
    for H, rev in ((16, 0), (32, 2), (64, 1), (128, 2 | INTERLEAVED)):           # gates = cstate = NULL; no force bit: the automatic rule, few sequences
        add("lstm", "lstm_fwd", H=H, nseq=5, L=9, reverse=rev, null=1)
    for H, rev in ((16, 2), (64, 0)):                                            # an xg column block at +-100: both exp2 paths overflow and underflow
        add("lstm", "lstm_fwd", H=H, nseq=5, L=9, reverse=rev, sat=1)
    for nseq, rev in ((1024, 0), (1025, 0), (512, 2), (513, 2)):                 # the automatic rule at its boundary of 256 workgroups
        for op in ("lstm_fwd", "lstm_bwd"):
            add("lstm", op, H=16, nseq=nseq, L=2, reverse=rev)
    # attention: per D the lengths that reach all four ML, with a ragged second block and a wave with a single live query; three score profiles,
    # the dropout rate alternating so that every instance sees both
    for D in (8, 16, 32):
        for i, L in enumerate((33, 64, 65, 129, 257, 320)):
            for j, profile in enumerate(("unit", "spread", "lastmax")):
                for op in ("attn_fwd", "attn_bwd"):
                    add("attn", op, N=2, H=3, L=L, D=D, p_drop=(0.0, 0.1)[(i + j) % 2], profile=profile)
    for L in (1, 31, 32):
        for op in ("attn_fwd", "attn_bwd"):
            add("attn", op, N=2, H=3, L=L, D=16, p_drop=(0.1 if L == 31 else 0.0), profile="unit")
    # rownorm: C astride every 256-feature trip x {no branch, branch, branch with dropout}, rows rotating; the grid-stride case at two widths
    for i, C in enumerate((4, 252, 256, 260, 512, 516, 768, 772, 1024)):
        for j, (res, p) in enumerate(((0, 0.0), (1, 0.0), (1, 0.25))):
            rows = (1, 3, 5)[(i + j) % 3]
            add("rownorm", "rownorm_fwd", rows=rows, C=C, res=res, p_drop=p, null=int(res and (i + j) % 2 == 0))
            add("rownorm", "rownorm_bwd", rows=rows, C=C, res=res, p_drop=p)
    for C in (4, 260):
        add("rownorm", "rownorm_fwd", rows=8197, C=C, res=1, p_drop=0.25, null=0)
        add("rownorm", "rownorm_bwd", rows=8197, C=C, res=1, p_drop=0.25)
    # relu_drop: one float4, a ragged grid, and more float4s than the grid's 4096 x 256 threads
    for n in (4, 1028, 4 * 1048576 + 4096):
        for p in (0.0, 0.1):
            for op in ("relu_drop_fwd", "relu_drop_bwd"):
                add("relu_drop", op, n=n, p_drop=p, device_only=int(n > 4 * 1048576))
    return cs


_CASES = {}


def cases(env="default", tier="device"):
    """every case of the environment on the tier ("device" or "host") with the instance it is meant to reach under "name"; fails if an instance
    has no case (default environment, either tier)"""
    key = (env, tier)
    if key not in _CASES:
        out = []
        for i, c in enumerate(_all_cases()):
            if c["family"] not in ENV_FAMILIES[env] or (tier == "host" and c.get("device_only")):
                continue
            if env != "default" and ((c["reverse"] >> 8) & 3 or c.get("device_only")):      # under a switch: the cases the switch moves
                continue
            if tier == "host" and c["family"] == "attn" and c["L"] >= 257:
                c = dict(c, N=1, H=1)
            c = dict(c, id=i, name=dispatch(ENVS[env], c), seed=zlib.crc32("dualpath/{}".format(i).encode()))
            out.append(c)
        if env == "default":
            missing = sorted(set(INSTANCES) - set(c["name"] for c in out))
            assert not missing, "no case reaches {}".format(missing)
        _CASES[key] = out
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------- operands
def _t():
    import torch
    return torch


def _rn(g, *s):
    torch = _t()
    return torch.randn(*s, generator=g, dtype=torch.float64)


def _mags(g, *s, lo=-6, hi=6):
    torch = _t()
    return 2.0 ** torch.randint(lo, hi + 1, s, generator=g).double()


def _nan(*s):
    torch = _t()
    return torch.full(s, float("nan"), dtype=torch.float32)


def _hash_keep(idx, p_drop, seed):
    """dropout_hash of csrc/common.hpp on 64-bit element indices (int64 tensor) -> keep mask; None without dropout"""
    if not p_drop > 0:
        return None
    M = 0xFFFFFFFF
    thr = max(1, min(int(float(_f32(p_drop)) * 4294967296.0), M))
    s0, s1 = seed & M, (seed >> 32) & M
    x = (idx & M) ^ s0
    x = (x * 0x9E3779B1) & M
    x = x ^ (x >> 15)
    x = (x * 0x85EBCA6B) & M
    x = x ^ (x >> 13)
    x = (x + s1 + (((idx >> 32) & M) * 0x9E3779B1)) & M
    x = (x * 0xC2B2AE35) & M
    x = x ^ (x >> 16)
    return x >= thr


def _f32(v):
    torch = _t()
    return torch.tensor(v, dtype=torch.float32)


def keep_inv(p_drop):
    """1 / (1 - p) as the libraries form it, in fp32"""
    return float(_f32(1.0) / (_f32(1.0) - _f32(p_drop))) if p_drop > 0 else 1.0


def keep_attn(N, L, H, p_drop, seed):
    """csrc/attn.hip: the hash of the element index ((n H + h) L + q) L + key -> (N, H, L, L) keep mask"""
    torch = _t()
    n, h, q, k = torch.meshgrid(torch.arange(N), torch.arange(H), torch.arange(L), torch.arange(L), indexing="ij")
    return _hash_keep(((n * H + h) * L + q) * L + k, p_drop, seed)


def keep_flat(n, p_drop, seed):
    """csrc/rownorm.hip: the same hash on the flat element index"""
    return _hash_keep(_t().arange(n), p_drop, seed)


def _elem(ref, scale, **kw):
    return dict(kind="elem", ref=ref, scale=scale, **kw)


def _shifted(x, nseq, L, shift):
    torch = _t()
    if not shift:
        return x
    xv = x.reshape(nseq, L, -1)
    xs = torch.zeros_like(xv)
    if shift < 0:
        xs[:, 1:] = xv[:, :-1]
    else:
        xs[:, :-1] = xv[:, 1:]
    return xs.reshape(x.shape)


# Every op: setup(c, g) -> (buffers, invoke, contract)
#   buffers   ordered {name: (role, fp32 tensor)}; role "in" (must come back untouched), "out" (NaN, written), "inout"
#   invoke    (K, V) -> None: the call(s) through the backend K on the device views V[name]
#   contract  (a, dt) -> {output: description}: the contract evaluated in dtype dt on the buffers' values a[name] as they are BEFORE the call
def _setup_linear(c, g):
    torch = _t()
    op, ntok, K, N = c["op"], c["ntok"], c["K"], c["N"]
    rows = lambda n, w: (_rn(g, n, w) * _mags(g, n, 1)).float()
    if op == "linear_fwd":
        bufs = dict(x=("in", rows(ntok, K)), w=("in", (rows(N, K) * K ** -0.5).float()), y=("out", _nan(ntok, N)))
        for b in ("bias", "bias2"):
            if c[b]:
                bufs[b] = ("in", (_rn(g, N) * _mags(g, N)).float())

        def invoke(Kb, V):
            Kb.linear_fwd(V["x"], V["w"], V.get("bias"), V.get("bias2"), V["y"], ntok, K, N)

        def contract(a, dt):
            x, w = a["x"].to(dt), a["w"].to(dt)
            y, sc = x @ w.t(), x.abs() @ w.abs().t()
            for b in ("bias", "bias2"):
                if b in a:
                    y, sc = y + a[b].to(dt), sc + a[b].to(dt).abs()
            return dict(y=_elem(y, sc))
        return bufs, invoke, contract
    if op == "linear_bwd_input":
        acc = c["accumulate"]
        bufs = dict(dy=("in", rows(ntok, N)), w=("in", (rows(N, K) * N ** -0.5).float()), dx=("inout", rows(ntok, K)) if acc else ("out", _nan(ntok, K)))

        def invoke(Kb, V):
            Kb.linear_bwd_input(V["dy"], V["w"], V["dx"], ntok, K, N, acc)

        def contract(a, dt):
            dy, w = a["dy"].to(dt), a["w"].to(dt)
            dx, sc = dy @ w, dy.abs() @ w.abs()
            if acc:
                dx, sc = dx + a["dx"].to(dt), sc + a["dx"].to(dt).abs()
            return dict(dx=_elem(dx, sc))
        return bufs, invoke, contract
    nseq, L, shift, nslab = c["nseq"], c["L"], c["shift"], c["nslab"]
    ldx = 2 * K + 4 if c["wide"] else K
    bufs = dict(dy=("in", rows(ntok, N)), xw=("in", rows(ntok, ldx)), partial=("out", _nan(nslab, N, K)))
    if c["pb"]:
        bufs["partial_bias"] = ("out", _nan(nslab, N))

    def invoke(Kb, V):
        Kb.linear_bwd_weight(V["dy"], V["xw"][:, ldx - K:], ldx, V["partial"], V.get("partial_bias"), ntok, K, N, L, shift, nslab)

    def contract(a, dt):
        dy, xs = a["dy"].to(dt), _shifted(a["xw"][:, ldx - K:].to(dt), nseq, L, shift)
        per = ((ntok + 31) // 32 + nslab - 1) // nslab * 32
        part, psc, pb, pbsc = (torch.zeros(nslab, N, K, dtype=dt), torch.zeros(nslab, N, K, dtype=dt), torch.zeros(nslab, N, dtype=dt), torch.zeros(nslab, N, dtype=dt))
        for s in range(nslab):
            lo, hi = min(ntok, s * per), min(ntok, (s + 1) * per)
            part[s], psc[s] = dy[lo:hi].t() @ xs[lo:hi], dy[lo:hi].abs().t() @ xs[lo:hi].abs()
            pb[s], pbsc[s] = dy[lo:hi].sum(0), dy[lo:hi].abs().sum(0)
        out = dict(partial=_elem(part, psc))
        if c["pb"]:
            out["partial_bias"] = _elem(pb, pbsc)
        return out
    return bufs, invoke, contract


def _setup_chunk(c, g):
    B, F, S, K, inter = (c[k] for k in ("B", "F", "S", "K", "inter"))
    to_tokens = c["op"] == "chunk_to_tokens"
    x = _rn(g, B, F, S, K).float()
    tok = (x.permute(0, 3, 2, 1) if inter else x.permute(0, 2, 3, 1)).contiguous()
    bufs = dict(src=("in", x if to_tokens else tok), dst=("out", _nan(*(tok.shape if to_tokens else x.shape))))

    def invoke(Kb, V):
        getattr(Kb, c["op"])(V["src"], V["dst"], B, F, S, K, inter)

    def contract(a, dt):
        return dict(dst=dict(kind="exact", ref=tok if to_tokens else x))
    return bufs, invoke, contract


def _lstm_dirs(reverse):
    rev = reverse & 0xff
    return [0, 1] if rev == 2 else [rev]


def _lstm_forward(xg, whh, revs, dt):
    """(D, nseq, L, 4H), (D, 4H, H) -> h (D, nseq, L, H), gates (D, nseq, L, 4H), c (D, nseq, L, H) in dtype dt"""
    torch = _t()
    D, nseq, L, H4 = xg.shape
    H = H4 // 4
    hs, gs, cs = torch.zeros(D, nseq, L, H, dtype=dt), torch.zeros(D, nseq, L, H4, dtype=dt), torch.zeros(D, nseq, L, H, dtype=dt)
    for d, rev in enumerate(revs):
        h, cc = torch.zeros(nseq, H, dtype=dt), torch.zeros(nseq, H, dtype=dt)
        for step in range(L):
            t = L - 1 - step if rev else step
            a = xg[d, :, t] + h @ whh[d].t()
            i, f, gg, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            cc = f * cc + i * gg
            h = o * torch.tanh(cc)
            hs[d, :, t], gs[d, :, t], cs[d, :, t] = h, torch.cat([i, f, gg, o], 1), cc
    return hs, gs, cs


def _lstm_backward(dh, gates, cst, whh, revs, dt):
    torch = _t()
    D, nseq, L, H = cst.shape
    out = torch.zeros(D, nseq, L, 4 * H, dtype=dt)
    for d, rev in enumerate(revs):
        dhr, dc = torch.zeros(nseq, H, dtype=dt), torch.zeros(nseq, H, dtype=dt)
        for step in range(L):
            t = step if rev else L - 1 - step
            tp = t + 1 if rev else t - 1
            cp = cst[d, :, tp] if 0 <= tp < L else torch.zeros(nseq, H, dtype=dt)
            G = gates[d, :, t]
            i, f, gg, o = G[:, :H], G[:, H:2 * H], G[:, 2 * H:3 * H], G[:, 3 * H:]
            v = dh[d, :, t] + dhr
            tc = torch.tanh(cst[d, :, t])
            dcc = v * o * (1 - tc * tc) + dc
            da = torch.cat([dcc * gg * i * (1 - i), dcc * cp * f * (1 - f), dcc * i * (1 - gg * gg), v * tc * o * (1 - o)], 1)
            out[d, :, t] = da
            dc = dcc * f
            dhr = da @ whh[d]
    return out


def _setup_lstm(c, g):
    torch = _t()
    op, H, nseq, L, reverse = c["op"], c["H"], c["nseq"], c["L"], c["reverse"]
    revs = _lstm_dirs(reverse)
    D, inter = len(revs), bool(reverse & INTERLEAVED)
    xg = _rn(g, D, nseq, L, 4 * H) * _mags(g, D, nseq, 1, 1, lo=-3, hi=3)
    if c.get("sat"):              # units 0 .. 3 of every gate: i, o at +100, f at -100, g at +100 / -100 -- c stays 0 +- 1 there, everything finite
        for gate, v in ((0, 100.0), (1, -100.0), (3, 100.0)):
            xg[..., gate * H:gate * H + 4] = v
        xg[..., 2 * H:2 * H + 2], xg[..., 2 * H + 2:2 * H + 4] = 100.0, -100.0
        xg[:, 1] *= -1            # ... and one sequence with every sign turned round
    xg = xg.float()
    whh = (_rn(g, D, 4 * H, H) * H ** -0.5).float()
    slabs = lambda t: t.reshape(nseq, L, 2, H).permute(2, 0, 1, 3) if inter else t.reshape(D, nseq, L, H)       # h / dh as (D, nseq, L, H)
    seq = lambda ref, pre=None: dict(kind="seq", ref=ref, rows=D * nseq, pre=pre)
    if op == "lstm_fwd":
        hshape = (nseq, L, 2 * H) if inter else (D, nseq, L, H)
        bufs = dict(xg=("in", xg), whh=("in", whh), h=("out", _nan(*hshape)), gates=("out", _nan(D, nseq, L, 4 * H)), cstate=("out", _nan(D, nseq, L, H)))
        if c.get("null"):
            bufs["h_null"] = ("out", _nan(*hshape))

        def invoke(Kb, V):
            Kb.lstm_fwd(V["xg"], V["whh"], V["h"], V["gates"], V["cstate"], nseq, L, H, reverse)
            if c.get("null"):
                Kb.lstm_fwd(V["xg"], V["whh"], V["h_null"], None, None, nseq, L, H, reverse)

        def contract(a, dt):
            h, gt, cs = _lstm_forward(a["xg"].to(dt), a["whh"].to(dt), revs, dt)
            out = dict(h=seq(h, slabs), gates=seq(gt), cstate=seq(cs))
            if c.get("null"):
                out["h_null"] = dict(kind="same", to="h")
            return out
        return bufs, invoke, contract
    _, gt, cs = _lstm_forward(xg.double(), whh.double(), revs, torch.float64)
    dh = (_rn(g, D, nseq, L, H) * _mags(g, D, nseq, 1, 1)).float()
    if inter:
        dh = dh.permute(1, 2, 0, 3).reshape(nseq, L, 2 * H).contiguous()
    bufs = dict(dh=("in", dh), gates=("in", gt.float()), cstate=("in", cs.float()), whh=("in", whh), dxg=("out", _nan(D, nseq, L, 4 * H)))

    def invoke(Kb, V):
        Kb.lstm_bwd(V["dh"], V["gates"], V["cstate"], V["whh"], V["dxg"], nseq, L, H, reverse)

    def contract(a, dt):
        return dict(dxg=seq(_lstm_backward(slabs(a["dh"]).to(dt), a["gates"].to(dt), a["cstate"].to(dt), a["whh"].to(dt), revs, dt)))
    return bufs, invoke, contract


def _attn_forward(qkv, keep, kinv, scale, dt):
    """(N, L, 3, H, D) -> s, lse, pr, pd (N, H, L, L / L) and q, k, v (N, H, L, D) in dt"""
    torch = _t()
    t = qkv.to(dt)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = scale * (q @ k.transpose(-1, -2))
    lse = torch.logsumexp(s, dim=-1)
    pr = torch.exp(s - lse.unsqueeze(-1))
    pd = pr if keep is None else torch.where(keep, pr * kinv, torch.zeros_like(pr))
    return q, k, v, s, lse, pr, pd


def _setup_attn(c, g):
    torch = _t()
    op, N, L, H, D, p, profile = (c[k] for k in ("op", "N", "L", "H", "D", "p_drop", "profile"))
    scale, seed = D ** -0.5, 0x1234ABCD5678 + c["id"]
    if profile == "unit":
        q, k = _rn(g, N, L, H, D) * 1.3, _rn(g, N, L, H, D) * 1.3
    elif profile == "spread":                    # scores of standard deviation 10: spread over about +-30, a peaked softmax
        q, k = _rn(g, N, L, H, D) * 10 ** 0.5, _rn(g, N, L, H, D) * 10 ** 0.5
    else:                                        # keys of increasing norm along one direction: the scores rise to about 30 at the LAST key, every block rescales
        u = _rn(g, N, 1, H, D)
        u = u / u.norm(dim=-1, keepdim=True)
        amp = (30 * D ** 0.5) ** 0.5
        ramp = (torch.arange(1, L + 1, dtype=torch.float64) / L).view(1, L, 1, 1)
        q, k = amp * u + 0.3 * _rn(g, N, L, H, D), amp * ramp * u + 0.3 * _rn(g, N, L, H, D)
    v = _rn(g, N, L, H, D) * _mags(g, N, L, H, 1)
    qkv = torch.stack([q, k, v], 2).float().contiguous()
    keep, kinv = keep_attn(N, L, H, p, seed), keep_inv(p)
    if op == "attn_fwd":
        bufs = dict(qkv=("in", qkv), o=("out", _nan(N, L, H, D)), lse=("out", _nan(N, H, L)))

        def invoke(Kb, V):
            Kb.attn_fwd(V["qkv"], V["o"], V["lse"], N, L, H, D, scale, p, seed)

        def contract(a, dt):
            _, _, vv, s, lse, _, pd = _attn_forward(a["qkv"], keep, kinv, scale, dt)
            return dict(o=_elem((pd @ vv).permute(0, 2, 1, 3), (pd @ vv.abs()).permute(0, 2, 1, 3)), lse=_elem(lse, 1 + s.abs().amax(-1)))
        return bufs, invoke, contract
    _, _, vv, _, lse, _, pd = _attn_forward(qkv, keep, kinv, scale, torch.float64)
    o = (pd @ vv).permute(0, 2, 1, 3).float().contiguous()
    dout = (_rn(g, N, L, H, D) * _mags(g, N, L, H, 1)).float()
    bufs = dict(qkv=("in", qkv), o=("in", o), dout=("in", dout), lse=("in", lse.float().contiguous()), delta=("out", _nan(N, H, L)), dqkv=("out", _nan(N, L, 3, H, D)))

    def invoke(Kb, V):
        Kb.attn_bwd(V["qkv"], V["o"], V["dout"], V["lse"], V["delta"], V["dqkv"], N, L, H, D, scale, p, seed)

    def contract(a, dt):
        t = a["qkv"].to(dt)
        qq, kk, vv = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        gg, oo = a["dout"].to(dt).permute(0, 2, 1, 3), a["o"].to(dt).permute(0, 2, 1, 3)
        pr = torch.exp(scale * (qq @ kk.transpose(-1, -2)) - a["lse"].to(dt).unsqueeze(-1))
        dl = (gg * oo).sum(-1, keepdim=True)
        dpd = gg @ vv.transpose(-1, -2)
        pd, dp = (pr, dpd) if keep is None else (torch.where(keep, pr * kinv, torch.zeros_like(pr)), torch.where(keep, dpd * kinv, torch.zeros_like(dpd)))
        ds = pr * (dp - dl)
        # dS is itself formed in the kernel, from a difference that cancels where the softmax is peaked (dP -> delta; at L = 1 it is zero): its addends
        # are P dP~ and P delta, whose own addends are the |dO||v| and |dO||O| -- the nested addend of stream_matrix's sums
        dpa = gg.abs() @ vv.abs().transpose(-1, -2) * kinv
        dsa = pr * ((dpa if keep is None else torch.where(keep, dpa, torch.zeros_like(dpa))) + (gg * oo).abs().sum(-1, keepdim=True))
        pack = lambda a3: torch.stack(a3, 0).permute(1, 3, 0, 2, 4)          # (3, N, H, L, D) -> (N, L, 3, H, D)
        ref = pack([scale * (ds @ kk), scale * (ds.transpose(-1, -2) @ qq), pd.transpose(-1, -2) @ gg])
        sc = pack([scale * (dsa @ kk.abs()), scale * (dsa.transpose(-1, -2) @ qq.abs()), pd.transpose(-1, -2) @ gg.abs()])
        return dict(dqkv=_elem(ref, sc), delta=dict(kind="finite"))
    return bufs, invoke, contract


def _rownorm_forward(x, res, keep, kinv, gamma, beta, dt):
    torch = _t()
    s, q = x.to(dt), None
    if res is not None:
        q = res.to(dt)
        if keep is not None:
            q = torch.where(keep, q * kinv, torch.zeros_like(q))
        s = s + q
    mu = s.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((s - mu) ** 2).mean(1, keepdim=True) + ROWNORM_EPS)
    return s, q, mu, rstd, (s - mu) * rstd * gamma.to(dt) + beta.to(dt)


def _setup_rownorm(c, g):
    torch = _t()
    op, rows, C, with_res, p = (c[k] for k in ("op", "rows", "C", "res", "p_drop"))
    seed = 0x1234567 * (rows + 1) + (C << 40) + c["id"]
    x = (_rn(g, rows, C) + 0.3) * _mags(g, rows, 1)
    res = _rn(g, rows, C) * 0.8 * _mags(g, rows, 1) if with_res else None
    if rows >= 3:                 # a constant row (variance 0: y = beta) and a row at offset 1000 with unit spread (the two-pass variance)
        x[1] = float(x[1, 0])
        x[2] = 1000.0 + _rn(g, C)
        if with_res:
            res[1] = 0.0
            res[2] = 0.0         # (a sum rounded to fp32 at offset 1000 moves by 2^-15 of the row's spread: s = x there, exact on both sides)
    x, res = x.float(), (res.float() if with_res else None)
    gamma, beta = (_rn(g, C) + 1).float(), _rn(g, C).float()
    keep, kinv = keep_flat(rows * C, p, seed), keep_inv(p)
    keep = keep.view(rows, C) if keep is not None else None
    if op == "rownorm_fwd":
        bufs = dict(x=("in", x), gamma=("in", gamma), beta=("in", beta), y=("out", _nan(rows, C)), stat=("out", _nan(rows, 2)))
        if with_res:
            bufs.update(res=("in", res), s=("out", _nan(rows, C)))
        if c.get("null"):
            bufs.update(y_null=("out", _nan(rows, C)), stat_null=("out", _nan(rows, 2)))

        def invoke(Kb, V):
            Kb.rownorm_fwd(V["x"], V.get("res"), V["gamma"], V["beta"], V.get("s"), V["y"], V["stat"], rows, C, ROWNORM_EPS, p, seed)
            if c.get("null"):
                Kb.rownorm_fwd(V["x"], V["res"], V["gamma"], V["beta"], None, V["y_null"], V["stat_null"], rows, C, ROWNORM_EPS, p, seed)

        def contract(a, dt):
            s, q, mu, rstd, y = _rownorm_forward(a["x"], a.get("res"), keep, kinv, a["gamma"], a["beta"], dt)
            out = dict(y=_elem(y, a["gamma"].to(dt).abs() * rstd * (s.abs() + mu.abs()) + a["beta"].to(dt).abs()),
                       stat=_elem(torch.cat([mu, rstd], 1), torch.cat([mu.abs() + s.abs().amax(1, keepdim=True), rstd], 1)))
            if with_res:
                out["s"] = _elem(s, a["x"].to(dt).abs() + q.abs())
            if c.get("null"):
                out.update(y_null=dict(kind="same", to="y"), stat_null=dict(kind="same", to="stat"))
            return out
        return bufs, invoke, contract
    s64, _, mu64, rstd64, _ = _rownorm_forward(x, res, keep, kinv, gamma, beta, torch.float64)
    dy = (_rn(g, rows, C) * _mags(g, rows, 1)).float()
    nparts = min((rows + 3) // 4, 2048)
    bufs = dict(dy=("in", dy), s=("in", s64.float()), gamma=("in", gamma), stat=("in", torch.cat([mu64, rstd64], 1).float()), ds=("out", _nan(rows, C)),
                part=("out", _nan(nparts, 2, C)))
    if p > 0:
        bufs["dres"] = ("out", _nan(rows, C))

    def invoke(Kb, V):
        assert Kb.rownorm_parts(rows, C) == nparts
        Kb.rownorm_bwd(V["dy"], V["s"], V["gamma"], V["stat"], V["ds"], V.get("dres"), V["part"], rows, C, p, seed)

    def contract(a, dt):
        gdy, st = a["dy"].to(dt), a["stat"].to(dt)
        mu, rstd = st[:, :1], st[:, 1:]
        xh = (a["s"].to(dt) - mu) * rstd
        gg = gdy * a["gamma"].to(dt)
        m1, m2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
        ds = rstd * (gg - m1 - xh * m2)
        sc = rstd * (gg.abs() + gg.abs().mean(1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(1, keepdim=True))
        out = dict(ds=_elem(ds, sc),
                   part=_elem(torch.stack([(gdy * xh).sum(0), gdy.sum(0)]), torch.stack([(gdy * xh).abs().sum(0), gdy.abs().sum(0)]), pre=lambda t: t.double().sum(0)))
        if p > 0:
            out["dres"] = _elem(torch.where(keep, ds * kinv, torch.zeros_like(ds)), sc * kinv, zero=~keep)
        return out
    return bufs, invoke, contract


def _setup_relu_drop(c, g):
    torch = _t()
    op, n, p = c["op"], c["n"], c["p_drop"]
    seed = 0xABCDEF0123 + n
    h = (_rn(g, n) * _mags(g, n)).float()
    keep, kinv = keep_flat(n, p, seed), keep_inv(p)
    live = (h > 0) if keep is None else (h > 0) & keep
    fwd = lambda hh, dt: torch.where(live, hh.to(dt) * kinv, torch.zeros(n, dtype=dt))
    one = lambda ref: _elem(ref, ref.abs(), zero=ref == 0, bound=ONE_ROUNDING)
    if op == "relu_drop_fwd":
        bufs = dict(h=("in", h), a=("out", _nan(n)))

        def invoke(Kb, V):
            Kb.relu_drop_fwd(V["h"], V["a"], n, p, seed)

        def contract(a, dt):
            return dict(a=one(fwd(a["h"], dt)))
        return bufs, invoke, contract
    act = fwd(h, torch.float64).float()
    bufs = dict(dy=("in", (_rn(g, n) * _mags(g, n)).float()), a=("in", act), dh=("out", _nan(n)))

    def invoke(Kb, V):
        Kb.relu_drop_bwd(V["dy"], V["a"], V["dh"], n, p)

    def contract(a, dt):
        return dict(dh=one(torch.where(a["a"] != 0, a["dy"].to(dt) * kinv, torch.zeros(n, dtype=dt))))
    return bufs, invoke, contract


SETUP = {"linear": _setup_linear, "chunk_tokens": _setup_chunk, "lstm": _setup_lstm, "attn": _setup_attn, "rownorm": _setup_rownorm, "relu_drop": _setup_relu_drop}
_PREPARED = {}


def prepare(c):
    """-> (buffers, invoke, contract, the float64 run of the contract); the last few cases are kept"""
    torch = _t()
    key = (c["id"], c["name"], c.get("N"), c.get("H"))
    if key not in _PREPARED:
        if len(_PREPARED) > 4:
            _PREPARED.clear()
        bufs, invoke, contract = SETUP[c["family"]](c, torch.Generator().manual_seed(c["seed"]))
        _PREPARED[key] = (bufs, invoke, contract, contract({n: v for n, (_, v) in bufs.items()}, torch.float64))
    return _PREPARED[key]


# ---------------------------------------------------------------------------------------------------------------- the check
def _ratio(diff, scale):
    torch = _t()
    return torch.where(scale > 0, diff / scale.clamp_min(1e-300), torch.where(diff > 0, torch.full_like(diff, float("inf")), torch.zeros_like(diff)))


def measure(desc, got, others):
    """one output in the metric of its kind -> its figure (to be held against the bound); inf where a condition without a tolerance fails"""
    torch = _t()
    kind = desc["kind"]
    inf = float("inf")
    if kind == "same":
        return 0.0 if torch.equal(got, others[desc["to"]]) else inf
    if kind == "finite":
        return 0.0 if torch.isfinite(got).all() else inf
    if kind == "exact":
        return 0.0 if torch.equal(got.reshape(desc["ref"].shape), desc["ref"]) else inf
    if not torch.isfinite(got).all():                # (before any slabs are summed: every slab finite and fully written)
        return inf
    if desc.get("pre") is not None:
        got = desc["pre"](got)
    ref = desc["ref"].double()
    got = got.double().reshape(ref.shape)
    if kind == "seq":
        g2, r2 = got.reshape(desc["rows"], -1), ref.reshape(desc["rows"], -1)
        return float(_ratio((g2 - r2).abs().amax(1), r2.abs().amax(1)).max())
    if desc.get("zero") is not None and not bool((got[desc["zero"]] == 0).all() and (got[~desc["zero"]] != 0).logical_or(ref[~desc["zero"]] == 0).all()):
        return inf
    return float(_ratio((got - ref).abs(), desc["scale"].double().expand_as(ref)).max())


# ---------------------------------------------------------------------------------------------------------------- running a case
def _guarded(t, to_device):
    """the device's copy of `t` between two guard bands -> (whole buffer, view of the middle)"""
    torch = _t()
    flat = torch.full((t.numel() + 2 * GUARD,), GUARD_VALUE, dtype=t.dtype)
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1)
    flat = to_device(flat)
    return flat, flat[GUARD:GUARD + t.numel()].view(t.shape)


def _guards_intact(flat):
    f = flat.cpu()
    return bool((f[:GUARD] == GUARD_VALUE).all()) and bool((f[-GUARD:] == GUARD_VALUE).all())


class FloatRun:
    """the contract's float32 run standing in for a device: the e32 of FAMILIES"""
    name = "float32"


def _another_name(K, to_device, family):
    """a tiny call of another family in front of every case, so that a case whose dispatcher stores no name cannot inherit the right one"""
    torch = _t()
    if family != "relu_drop":
        K.relu_drop_fwd(to_device(torch.zeros(4)), to_device(torch.zeros(4)), 4, 0.0, 0)
    else:
        K.chunk_to_tokens(to_device(torch.zeros(1, 1, 1, 1)), to_device(torch.zeros(1, 1, 1)), 1, 1, 1, 1, 0)


def run_case(K, c, to_device, sync, tamper=None):
    """one case through the backend K -> its record.  `tamper(outputs, inputs, ref)`: the controls of the checker alter the device's results"""
    torch = _t()
    import sepkernels
    bufs, invoke, contract, ref = prepare(c)
    a = {n: v for n, (_, v) in bufs.items()}
    rec = dict(case=dict(c), outputs={}, inputs_intact=True, guards_intact=True)
    if isinstance(K, FloatRun):
        got = {n: (d["ref"].float() if "ref" in d else None) for n, d in contract(a, torch.float32).items()}
        got = {n: (v if v is not None else (got[ref[n]["to"]] if ref[n]["kind"] == "same" else torch.zeros(1))) for n, v in got.items()}
        rec["kernel"] = c["name"]
    else:
        held = {n: _guarded(v, to_device) for n, v in a.items()}
        _another_name(K, to_device, c["family"])
        invoke(K, {n: h[1] for n, h in held.items()})
        rec["kernel"] = sepkernels.last_kernel()
        sync()
        got = {n: held[n][1].cpu() for n, (role, _) in bufs.items() if role != "in"}
        for n, (role, v) in bufs.items():
            rec["guards_intact"] = rec["guards_intact"] and _guards_intact(held[n][0])
            if role == "in" and not torch.equal(held[n][1].cpu(), v):
                rec["inputs_intact"] = False
    if tamper is not None:
        tamper(got, a, ref)
    assert sorted(got) == sorted(ref), (sorted(got), sorted(ref))
    for name, g in got.items():
        desc = dict(ref[name], pre=None) if isinstance(K, FloatRun) else ref[name]          # (the float32 run's results are in the reference's own layout)
        rec["outputs"][name] = dict(err=measure(desc, g, got), bound=ref[name].get("bound", bound_of(c["family"], name)))
    rec["ok"] = rec["kernel"] == c["name"] and rec["inputs_intact"] and rec["guards_intact"] and all(o["err"] <= o["bound"] for o in rec["outputs"].values())
    return rec


def run(env, K, to_device, sync, log=None, families=None, tier="device"):
    """every case of cases(env, tier) (of the families given) through the backend K, which must live in a process started with ENVS[env]"""
    for k in SWITCHES:
        assert os.environ.get(k) == ENVS[env].get(k), "the process environment is not that of '{}' ({})".format(env, k)
    recs = []
    for c in cases(env, tier):
        if families is not None and c["family"] not in families:
            continue
        rec = run_case(K, c, to_device, sync)
        recs.append(rec)
        if log:
            log("{:4s} {:28s} {}  worst err/bound {:.3f}".format("ok" if rec["ok"] else "FAIL", rec["kernel"], shape_of(c), worst_of(rec)))
    return recs


def worst_of(rec):
    """the record's worst err / bound over the outputs that have a tolerance"""
    return max([o["err"] / o["bound"] for o in rec["outputs"].values() if o["bound"] > 0] + [0.0 if all(o["err"] <= o["bound"] for o in rec["outputs"].values()) else float("inf")])


def shape_of(c):
    return " ".join("{}={}".format(k, hex(v) if k == "reverse" else v) for k, v in c.items() if k not in ("family", "name", "id", "seed"))


def failures(recs):
    """one line per record that is not ok"""
    out = []
    for r in recs:
        if not r["ok"]:
            c = r["case"]
            bad = {k: (v["err"], v["bound"]) for k, v in r["outputs"].items() if not v["err"] <= v["bound"]}
            out.append("{} (meant {}) {}: inputs_intact={} guards_intact={} over the bound (err, bound): {}".format(
                r["kernel"], c["name"], shape_of(c), r["inputs_intact"], r["guards_intact"], bad))
    return out


def float32_figures(families=None):
    """family -> the contract's float32 run's worst figure against its float64 run over the family's cases (the e32 of FAMILIES): the outputs
    with a measured bound only (not `same`, `finite`, `exact` or the one-rounding outputs)"""
    worst = {}
    for c in cases("default", "device"):
        if FAMILIES[c["family"]]["e32"] is None or (families is not None and c["family"] not in families):
            continue
        rec = run_case(FloatRun(), c, None, None)
        ref = prepare(c)[3]
        for name, o in rec["outputs"].items():
            if ref[name]["kind"] in ("elem", "seq"):
                worst[c["family"]] = max(worst.get(c["family"], 0.0), o["err"])
    return worst


def by_instance(recs):
    """instance -> worst err and worst err / bound over its records (profiles/r22_dualpath_instances.json)"""
    out = {}
    for r in recs:
        e = out.setdefault(r["kernel"], dict(cases=0, worst_err=0.0, worst_err_over_bound=0.0))
        e["cases"] += 1
        e["worst_err"] = max([e["worst_err"]] + [o["err"] for o in r["outputs"].values() if o["bound"] > 0])
        e["worst_err_over_bound"] = max(e["worst_err_over_bound"], worst_of(r))
    return out


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
    ap.add_argument("--backend", default="hip", help="hip (default), hostsim:<path of the host-simulation library> or float32 (the contract's float32 run)")
    ap.add_argument("--measure", action="store_true", help="print the float32 run's worst figure per family and the bound that follows (FAMILIES)")
    args = ap.parse_args()
    for k in SWITCHES:                            # the switch is read once per process, at the first call
        os.environ.pop(k, None)
    os.environ.update(ENVS[args.env])
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    if args.measure:
        for f, e in float32_figures().items():
            print("{:12s} e32 = {:.3e}  bound = {!r}  (in the ledger: {})".format(f, e, bound_rule(e, max(OLD[f].values())), FAMILIES[f]))
        return 0
    log = lambda s: print(s, flush=True)
    if args.backend == "float32":
        recs = run(args.env, FloatRun(), None, None, log)
    elif args.backend.startswith("hostsim:"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import hostsim
        with hostsim.HostSimBackend(args.backend[8:]) as K:
            recs = run(args.env, K, (lambda t: t.clone()), (lambda: None), log, tier="host")
    else:
        import sepkernels
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
