"""Helper module (not a test file): the ledger of sep_pw_gemm's kernel instances, a case matrix that reaches every one of them by name,
and a float64 restatement of the call's contract with the error model's own scale.  tests/test_gemm_instances_cpu.py runs the "host"
tier on the host simulation of the kernel sources, tests/test_gemm_instances_gpu.py the "device" tier on the MI355X; both start

    python tests/gemm_matrix.py --env NAME --tier host|device --out FILE [--backend hostsim:<library>]

once per environment, because the dispatchers read their switches once per process.

THE LEDGER.  One sep_pw_gemm call lands on one of five kernel families (csrc/gemm.hip, gemm_coop.hip, gemm_pc.hip); sep_last_kernel()
names the instance, spelled by the launch macro from the template arguments it instantiates:
    pc<WR,WC,prologue,two-source,epilogue>          14 combinations x {<4,1> (M % 256 == 0), <2,2>}
    coop<MI,prologue,two-source,epilogue,ns=N>      14 combinations x MI in {1, 2}, three MI = 4 forms (M % 512 == 0), ring depth N in {2, 3}
    direct<trans_a,prologue,two-source,epilogue,arith=A>   16 combinations x 3 arithmetics (GLN_BWD: fp32 MFMA only), M % 128 == 0
    direct_rt<trans_a,prologue,two-source>          everything else the direct kernel takes (epilogue flags read at run time, fp32 MFMA)
    staged                                          register-staged fallback
`dispatch(env, case)` restates the dispatch tables in Python; ENV_INSTANCES lists, per process environment, the instances that
environment is responsible for (an instance reachable under several environments is listed under each one whose switch changes the
shapes that reach it); INSTANCES is their union, and cases() refuses to return a matrix that misses one of them.

THE BOUND (the error of a contraction is relative to sum |a||x| per output, not elementwise).  reference() returns,
with every output, a SCALE of the same shape: the output's formula with every term replaced by its magnitude,
    sum_k |a||x'| + |bias| + |res| + |prior Y2|,   |x'| = |gamma| rstd (|u| + |mean|) + |beta| behind a gLN prologue,
    rstd (|gamma||x| + |mg| + rstd (|u| + |mean|) |mgx|) |PReLU'(a)| behind the gLN-backward prologue, sums: the sum of their terms' scales.
err = max |got - ref| / scale over the valid frames.  e32 is the same figure for the CPU emulator's fp32 evaluation (tests/emulator.py) of
the same operands -- the reference's own error -- and the bound per output is
    err <= 4 * e32 + a(arith) + r(output).
  4 x    the project's margin for a split product (22 + 22 significand bits) beside an fp32 one (24 + 24):
         test_gemm_split_arithmetic_is_as_accurate_as_fp32_mfma.
  a      f32, bf16x6: 0 (exact fp32 products / an exact three-part split).  f16x3: x 2^s = hi + lo, hi = fp16(x 2^s) TOWARD ZERO, so the
         remainder is below one unit of hi's last place, 2^-10 |x|; lo = fp16(remainder) toward zero leaves less than 2^-10 of THAT: each
         operand is represented to 2^-21 relative (section 4.2's "11 + 11 bits"; its 2^-22 for the dropped lo*lo term holds for round to
         nearest, truncation gives |lo| < 2^-10 |x| and lo_a lo_x < 2^-20 |ax|).  a = 2^-21 + 2^-21 + 2^-20 = 2^-19 of sum |a||x'|.
  r      outputs behind a non-linear epilogue or a sum.  Sigmoid: Lipschitz constant 1/4, so its scale is scale_in / 4 + |out| and
         r = 8 * 2^-24: rounding the argument of exp (|y| 2^-24 relative, times sigmoid's slope: below 4 * 2^-24 of that scale), exp,
         reciprocal, the addition and the stored value one unit each.  PReLU is Lipschitz with max(1, |alpha|): a pre-activation within
         rounding of zero moves the output by no more than its own error whichever branch the device took, so no branch is counted as
         an error; its derivative (PRELU_BWD, ROWSUMS_PRELU, the prologues) is taken from INPUT tensors, identical on both sides.
         Sums (epi_stats, epi_rowpart, epi_dalpha, pro_dalpha): no lane of any family adds more than 128 values in fp32 before the
         partial goes to double (a 64-frame piece of a row; a thread's share of a 256 x 128 or 512 x 64 tile), and n fp32 additions in
         any order err by at most (n - 1) 2^-24 of the sum of magnitudes: r = 128 * 2^-24.  The sum of squares' scale is
         sum 2 |u| scale(u) + u^2 (the derivative of the square times the error of u, plus the square's own rounding).
A dropped cross term (hi*lo) is an error of ~2^-11 of the scale; the largest bound above is ~2^-17.  The negative control of
tests/test_gemm_instances_cpu.py perturbs a device result by 2^-14 of the scale and the check must reject it.

OPERANDS follow test_gemm_packed_weights_model_shapes: rows of X spread by exp(3 N(0,1)), rows of A by exp(4 N(0,1)) -- except on
direct<..., arith=2>, whose contract is ONE power-of-two scale for all of A from the caller's bound a_amax (include/sepkernels.h: values
far below it lose low bits by design; its rows are drawn alike, as test_gemm_split_arithmetic_is_as_accurate_as_fp32_mfma draws them).
A gLN prologue sees data with a non-zero mean."""
import argparse
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "dnn-based_source_separation_amd", "src"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

F32, BF16X6, F16X3 = 0, 1, 2
NONE, PRELU, GLN, GLN_PRELU, GLN_BWD = 0, 1, 2, 3, 4
STATS, RES, SIG, PBWD, ROWS, ROWSP = 1, 2, 4, 8, 16, 48
PRO_NAME = {NONE: "SEP_PRO_NONE", PRELU: "SEP_PRO_PRELU", GLN: "SEP_PRO_GLN", GLN_PRELU: "SEP_PRO_GLN_PRELU", GLN_BWD: "SEP_PRO_GLN_BWD"}
EPI_NAME = {0: "0", STATS: "SEP_EPI_STATS_PRELU", RES: "SEP_EPI_RESIDUAL", SIG: "SEP_EPI_SIGMOID", PBWD: "SEP_EPI_PRELU_BWD",
            ROWS: "SEP_EPI_ROWSUMS", ROWSP: "SEP_EPI_ROWSUMS | SEP_EPI_ROWSUMS_PRELU"}
BOOL = {0: "false", 1: "true", False: "false", True: "true"}
SLOTS = 16

# (prologue, two-source, epilogue) of the packed-weight kernels (gemm_pc.hip, gemm_coop.hip): the PK rows of SEP_FUSED_COMBOS in
# csrc/gemm_common.hpp, restated by hand -- this file is what the device is compared against and is not generated from that table
PACKED_COMBOS = [(NONE, 0, STATS), (GLN_PRELU, 0, RES), (GLN_PRELU, 0, 0), (PRELU, 0, SIG), (PRELU, 0, 0), (GLN, 0, 0), (NONE, 0, 0), (NONE, 0, PBWD),
                 (NONE, 1, 0), (NONE, 1, ROWSP), (NONE, 0, ROWSP), (NONE, 0, ROWS), (GLN_BWD, 0, RES), (GLN_BWD, 0, 0)]
COOP_MI4 = [(NONE, 0, STATS), (NONE, 1, 0), (NONE, 0, 0)]          # bits 0, 1, 2 of SEPK_COOP_MI4 (default 2)
# (trans_a, prologue, two-source, epilogue) of the direct kernel's compile-time instances: all rows of that table, PK and DIRECT
DIRECT_COMBOS = [(0, NONE, 0, STATS), (0, GLN_PRELU, 0, RES), (0, GLN_PRELU, 0, 0), (0, PRELU, 0, SIG), (0, PRELU, 0, 0), (0, GLN, 0, 0), (0, NONE, 0, 0),
                 (0, NONE, 0, RES), (1, NONE, 1, 0), (1, NONE, 0, 0), (1, NONE, 0, PBWD), (1, NONE, 1, ROWSP), (1, NONE, 0, ROWSP), (1, NONE, 0, ROWS),
                 (1, GLN_BWD, 0, RES), (1, GLN_BWD, 0, 0)]
# the orientation in which the Conv-TasNet step uses each packed combination (the packed kernels themselves never look at trans_a)
BACKWARD = {(NONE, 0, PBWD), (NONE, 1, 0), (NONE, 1, ROWSP), (NONE, 0, ROWSP), (NONE, 0, ROWS), (GLN_BWD, 0, RES), (GLN_BWD, 0, 0)}

ENVS = {
    "default": {},
    "pc": {"SEPK_GEMM_KERNEL": "pc"},
    "coop": {"SEPK_GEMM_KERNEL": "coop"},
    "coop_mi1": {"SEPK_COOP_MI": "1"},
    "coop_mi4": {"SEPK_COOP_MI": "4"},
    "pc_22": {"SEPK_PC_22": "1"},
    "no_coop": {"SEPK_COOP": "0"},
    "staged": {"SEPK_FORCE_STAGED": "1"},
    "coop_ns3": {"SEPK_COOP_NS": "3", "SEPK_COOP_MI4": "7", "SEPK_GEMM_KERNEL": "coop"},      # the three-stage ring of every cooperative instance
}
SWITCHES = ("SEPK_GEMM_KERNEL", "SEPK_PC_MINK", "SEPK_PC_22", "SEPK_COOP", "SEPK_COOP_MI", "SEPK_COOP_MI4", "SEPK_COOP_NS", "SEPK_FORCE_STAGED")


def pc_name(wr, wc, pro, sp, ef):
    return "pc<{},{},{},{},{}>".format(wr, wc, PRO_NAME[pro], BOOL[sp], EPI_NAME[ef])


def coop_name(mi, pro, sp, ef, ns=2):
    return "coop<{},{},{},{},ns={}>".format(mi, PRO_NAME[pro], BOOL[sp], EPI_NAME[ef], ns)


def direct_name(tr, pro, sp, ef, ar):
    return "direct<{},{},{},{},arith={}>".format(BOOL[tr], PRO_NAME[pro], BOOL[sp], EPI_NAME[ef], ar)


def direct_rt_name(tr, pro, sp):
    return "direct_rt<{},{},{}>".format(BOOL[tr], PRO_NAME[pro], BOOL[sp])


def _direct_arith(pro, arith):
    return 0 if pro == GLN_BWD else arith      # the binding always hands a_amax over with F16X3, so F16X3 never runs as BF16X6 here


PC_ALL = [pc_name(wr, wc, *c) for (wr, wc) in ((4, 1), (2, 2)) for c in PACKED_COMBOS]
COOP_12 = [coop_name(mi, *c) for mi in (2, 1) for c in PACKED_COMBOS]
DIRECT_ALL = sorted(set(direct_name(*c, _direct_arith(c[1], ar)) for c in DIRECT_COMBOS for ar in (F32, BF16X6, F16X3)))
DIRECT_RT_ALL = [direct_rt_name(tr, pro, sp) for pro in (NONE, PRELU, GLN, GLN_PRELU) for tr in (0, 1) for sp in (0, 1)] + \
                [direct_rt_name(tr, GLN_BWD, 0) for tr in (0, 1)]
ENV_INSTANCES = {
    "default": PC_ALL + COOP_12 + [coop_name(4, NONE, 1, 0)] + DIRECT_ALL + DIRECT_RT_ALL + ["staged"],
    "pc": PC_ALL,                                                         # ... at the short contractions the default gives to coop
    "coop": COOP_12 + [coop_name(4, NONE, 1, 0)],                         # ... at the long contractions the default gives to pc
    "coop_mi1": [coop_name(1, *c) for c in PACKED_COMBOS],                # ... at M % 256 == 0
    "coop_mi4": [coop_name(4, *c) for c in COOP_MI4],
    "pc_22": [pc_name(2, 2, *c) for c in PACKED_COMBOS],                  # ... at M % 256 == 0
    "no_coop": sorted(set(direct_name(int(c in BACKWARD), *c, _direct_arith(c[0], F16X3)) for c in PACKED_COMBOS)),      # packed weights handed over, unused
    "staged": ["staged"],
    "coop_ns3": [coop_name(mi, *c, ns=3) for mi in (2, 1) for c in PACKED_COMBOS] + [coop_name(4, *c, ns=3) for c in COOP_MI4],
}
INSTANCES = sorted(set(n for v in ENV_INSTANCES.values() for n in v))


# ---------------------------------------------------------------------------------------------------------------- the dispatch tables, restated
def dispatch(env, c):
    """the instance name sep_pw_gemm gives the case under the environment `env` (a dict of the SEPK_* switches), or "error" where its
    argument checks refuse the call"""
    M, K, ldt, pro, ef, tr = c["M"], c["K"], c["ldt"], c["pro"], c["epi"], c["tr"]
    sp = 1 if c["k_split"] else 0
    big_gln = pro >= GLN and K > 512              # the per-row affine tables of the gLN prologues hold 512 rows in every family
    if c["arith"] == F16X3 and c["packed"] and env.get("SEPK_COOP") != "0":
        kern = env.get("SEPK_GEMM_KERNEL", "")
        curated = (pro, sp, ef) in PACKED_COMBOS
        if not kern.startswith("c") and (kern.startswith("p") or K >= int(env.get("SEPK_PC_MINK", 512)) or M >= 1024):
            if M % 128 == 0 and K % 64 == 0 and c["k_split"] % 16 == 0 and c["m_split"] % 128 == 0 and ldt % 256 == 0 and not big_gln and curated:
                tall = M % 256 == 0 and not int(env.get("SEPK_PC_22", 0))
                return pc_name(4 if tall else 2, 1 if tall else 2, pro, sp, ef)
        if M % 128 == 0 and not big_gln and curated:
            force_mi = int(env.get("SEPK_COOP_MI", 0))
            ns = 3 if env.get("SEPK_COOP_NS") == "3" else 2
            mi4 = 7 if force_mi == 4 else int(env.get("SEPK_COOP_MI4", 2))
            if force_mi not in (1, 2) and M % 512 == 0 and (pro, sp, ef) in COOP_MI4 and (mi4 >> COOP_MI4.index((pro, sp, ef))) & 1:
                return coop_name(4, pro, sp, ef, ns)
            return coop_name(1 if (force_mi == 1 or M % 256 != 0) else 2, pro, sp, ef, ns)
    if "SEPK_FORCE_STAGED" not in env and M >= 4 and M % 4 == 0 and not big_gln:
        if M % 128 == 0 and (tr, pro, sp, ef) in DIRECT_COMBOS:
            return direct_name(tr, pro, sp, ef, _direct_arith(pro, c["arith"]))
        return direct_rt_name(tr, pro, sp)
    return "staged" if K % 32 == 0 and c["k_split"] % 32 == 0 else "error"


def kernel_arith(name):
    """the arithmetic the named instance multiplies in"""
    if name.startswith(("pc<", "coop<")):
        return F16X3
    if name.startswith("direct<"):
        return int(name[name.index("arith=") + 6])
    return F32


# ---------------------------------------------------------------------------------------------------------------- the case matrix
def _case(regime, pro, sp, ef, *, tr, B, M, K, T, ldt, arith=F16X3, packed=True, k_split=None, m_split=0, accumulate=0):
    if sp and K < 32:
        K = 32                                    # two sources need two ring stages
    if k_split is None:
        k_split = 0 if not sp else (K // 2 if (K // 2) % 32 == 0 else 32 if K > 32 else 16)
    assert bool(k_split) == bool(sp) and T <= ldt and ldt % 128 == 0
    return dict(regime=regime, pro=pro, epi=ef, tr=int(tr), B=B, M=M, K=K, T=T, ldt=ldt, arith=arith, packed=bool(packed), k_split=k_split,
                m_split=m_split, accumulate=accumulate)


# the instances of the paper-best step (N = 512, B = 128, H = 512, Sc = 128; sepkernels/net.py) at their real (M, K): (prologue, two-source, epilogue, extras)
MODEL_STEP = [
    (GLN, 0, 0, dict(M=128, K=512)),                                           # bottleneck
    (NONE, 0, STATS, dict(M=512, K=128)),                                      # TCN conv1
    (GLN_PRELU, 0, RES, dict(M=256, K=512, m_split=128, accumulate=1)),        # heads [Wo; Ws]
    (GLN_PRELU, 0, 0, dict(M=128, K=512)),                                     # last layer: skip head only
    (PRELU, 0, SIG, dict(M=1024, K=128)),                                      # mask, two speakers
    (NONE, 0, PBWD, dict(M=128, K=1024)),                                      # mask^T
    (NONE, 1, 0, dict(M=512, K=256, k_split=128)),                             # heads^T
    (NONE, 0, 0, dict(M=512, K=128)),                                          # last layer's skip^T
    (GLN_BWD, 0, RES, dict(M=128, K=512)),                                     # conv1^T
    (NONE, 0, ROWS, dict(M=512, K=128)),                                       # bottleneck^T
]


def _shapes(tier, ldt_unit, kmin, kmid):
    """(regime, B, K, T, ldt) of one instance: one small shape on the host; on the device the smallest shape it takes, a ragged one (B = 3,
    T = ldt - 1, B * ldt / 128 not a multiple of 8: dead workgroups in the 8 * NR * ceil(NC / 8) grids) and one without pad frames"""
    if tier == "host":
        return [("host", 1, kmin, 200, 256)]
    rag = 384 if ldt_unit == 128 else 512
    return [("min", 1, kmin, 100, ldt_unit), ("ragged", 3, kmid, rag - 1, rag), ("nopad", 2, kmid, 256, 256)]


def _packed_cases(tier, family, tile, combos, kmin, kmid, M):
    out = []
    for (pro, sp, ef) in combos:
        for (regime, B, K, T, ldt) in _shapes(tier, 256 if family == "pc" else 128, kmin, kmid):
            out.append(_case(regime, pro, sp, ef, tr=(pro, sp, ef) in BACKWARD, B=B, M=M, K=K, T=T, ldt=ldt))
    return out


def _all_cases(env, tier):
    dev = tier == "device"
    cs = []
    if env in ("default", "pc", "pc_22"):
        kmin, kmid = (64, 128) if env == "pc" else (512, 512)
        if env != "pc_22":
            cs += _packed_cases(tier, "pc", (4, 1), PACKED_COMBOS, kmin, kmid, 256)
            cs += _packed_cases(tier, "pc", (2, 2), PACKED_COMBOS, kmin, kmid, 128)
        else:
            cs += _packed_cases(tier, "pc", (2, 2), PACKED_COMBOS, kmin, kmid, 256)
    if env in ("default", "coop", "coop_mi1", "coop_ns3"):
        kmin, kmid = (512, 512) if env == "coop" else (16, 128) if dev else (64, 64)
        if env != "coop_mi1":
            cs += _packed_cases(tier, "coop", 2, PACKED_COMBOS, kmin, kmid, 256)
            cs += _packed_cases(tier, "coop", 1, PACKED_COMBOS, kmin, kmid, 128)
            cs += _packed_cases(tier, "coop", 4, COOP_MI4 if env == "coop_ns3" else [(NONE, 1, 0)], kmin, kmid, 512)
        else:
            cs += _packed_cases(tier, "coop", 1, PACKED_COMBOS, kmin, kmid, 256)
    if env == "coop_mi4":
        cs += _packed_cases(tier, "coop", 4, COOP_MI4, 16 if dev else 64, 128, 512)
    if env == "no_coop":            # the weights arrive packed, the library is told not to use the packed kernels: the direct kernel on A / A2
        for (pro, sp, ef) in PACKED_COMBOS:
            for (regime, B, K, T, ldt) in _shapes(tier, 128, 16 if dev else 64, 128):
                cs.append(_case(regime, pro, sp, ef, tr=(pro, sp, ef) in BACKWARD, B=B, M=128, K=K, T=T, ldt=ldt))
    if env == "default":
        for (tr, pro, sp, ef) in DIRECT_COMBOS:
            for ar in ((F32,) if pro == GLN_BWD else (F32, BF16X6, F16X3)):
                for (regime, B, K, T, ldt) in _shapes(tier, 128, 16 if dev else 64, 128):
                    cs.append(_case(regime, pro, sp, ef, tr=tr, B=B, M=128, K=K, T=T, ldt=ldt, arith=ar, packed=False))
        for i, name in enumerate(DIRECT_RT_ALL):                       # rows off the 128 grid, and epilogues no compile-time instance exists for
            tr, pro, sp = [(t, p, s) for p in PRO_NAME for t in (0, 1) for s in (0, 1) if direct_rt_name(t, p, s) == name][0]
            for (regime, B, K, T, ldt) in _shapes(tier, 128, 16 if dev else 64, 128):
                ef = [0, RES, SIG, 0][i % 4] if pro != GLN_BWD else RES
                cs.append(_case(regime, pro, sp, ef, tr=tr, B=B, M=[192, 64, 36][i % 3], K=K, T=T, ldt=ldt, arith=[F16X3, F32, BF16X6][i % 3], packed=False))
        cs.append(_case("host" if not dev else "min", NONE, 0, 0, tr=0, B=1, M=66, K=32, T=100, ldt=128, arith=F32, packed=False))      # M % 4 != 0: staged
    if env == "staged":
        for (tr, pro, sp, ef, M, K, extra) in [(0, NONE, 0, 0, 128, 32, {}), (1, NONE, 1, ROWSP, 128, 192, dict(k_split=128)), (0, GLN_PRELU, 0, RES, 256, 64, dict(m_split=128, accumulate=1)),
                                               (0, PRELU, 0, SIG, 64, 64, {}), (1, GLN_BWD, 0, RES, 128, 64, {}), (0, NONE, 0, STATS, 192, 64, {}), (1, NONE, 0, PBWD, 64, 128, {}),
                                               (0, GLN, 0, 0, 128, 1024 if dev else 128, {})]:
            for (regime, B, _, T, ldt) in _shapes(tier, 128, K, K):
                cs.append(_case(regime, pro, sp, ef, tr=tr, B=B, M=M, K=K, T=T, ldt=ldt, arith=F32, packed=False, **extra))
    if dev:
        cs += _family_edges(env)
    return cs


def _family_edges(env):
    """device tier, once per family: K at the family's minimum (the "min" regime above) and K = 1024; a gLN prologue at the K = 512 limit of
    the affine tables and beyond it (K = 528 is refused by the argument checks -- no family takes it: the fallback needs K % 32 == 0 --,
    K = 544 lands on the register-staged kernel); M = 384, M = 192 (leaves the packed path), M = 1024; a two-source contraction with unequal
    halves (k_split = 128 of K = 192); m_split with accumulate; and the paper-best step's instances at B = 16, T = 3999, ldt = 4096"""
    e = []
    big = dict(B=2, T=300, ldt=512)
    heads = dict(m_split=128, accumulate=1)
    if env == "default":
        e += [_case("k1024", NONE, 0, 0, tr=0, M=128, K=1024, **big), _case("k1024", NONE, 0, PBWD, tr=1, M=256, K=1024, **big),
              _case("gln512", GLN, 0, 0, tr=0, M=128, K=512, **big), _case("gln528", GLN, 0, 0, tr=0, M=128, K=528, **big),
              _case("gln544", GLN_PRELU, 0, 0, tr=0, M=128, K=544, **big), _case("m384", NONE, 0, STATS, tr=0, M=384, K=512, **big),
              _case("m384", NONE, 0, STATS, tr=0, M=384, K=128, **big), _case("m192", NONE, 0, STATS, tr=0, M=192, K=128, **big),
              _case("m192", PRELU, 0, SIG, tr=0, M=192, K=512, **big), _case("m1024", PRELU, 0, SIG, tr=0, M=1024, K=128, **big),
              _case("ksplit128of192", NONE, 1, 0, tr=1, M=256, K=192, k_split=128, **big), _case("ksplit128of192", NONE, 1, ROWSP, tr=1, M=128, K=192, k_split=128, **big),
              _case("msplit_acc", GLN_PRELU, 0, RES, tr=0, M=256, K=512, **heads, **big), _case("msplit_acc", GLN_PRELU, 0, RES, tr=0, M=256, K=128, **heads, **big),
              _case("msplit_acc", GLN_PRELU, 0, RES, tr=0, M=384, K=256, m_split=256, accumulate=1, **big)]
        for ar in (F32, BF16X6, F16X3):
            un = dict(arith=ar, packed=False)
            e += [_case("k1024", NONE, 0, 0, tr=1, M=128, K=1024, **un, **big), _case("gln512", GLN, 0, 0, tr=0, M=128, K=512, **un, **big),
                  _case("gln544", GLN, 0, 0, tr=0, M=128, K=544, **un, **big), _case("m384", PRELU, 0, SIG, tr=0, M=384, K=64, **un, **big),
                  _case("m1024", NONE, 0, STATS, tr=0, M=1024, K=64, **un, **big), _case("ksplit128of192", NONE, 1, ROWSP, tr=1, M=128, K=192, k_split=128, **un, **big),
                  _case("msplit_acc", NONE, 0, RES, tr=0, M=256, K=128, **heads, **un, **big), _case("msplit_acc", GLN_PRELU, 0, RES, tr=0, M=256, K=128, **heads, **un, **big),
                  _case("msplit_acc", NONE, 0, RES, tr=0, M=192, K=128, **heads, **un, **big), _case("acc", NONE, 0, 0, tr=0, M=64, K=64, accumulate=1, **un, **big),
                  _case("k1024", PRELU, 1, SIG, tr=0, M=64, K=1024, **un, **big), _case("gln512", GLN_PRELU, 1, 0, tr=1, M=192, K=512, k_split=128, **un, **big)]
        for (pro, sp, ef, kw) in MODEL_STEP:
            e.append(_case("model", pro, sp, ef, tr=(pro, sp, ef) in BACKWARD, B=16, T=3999, ldt=4096, **kw))
    if env == "pc":
        e += [_case("ksplit128of192", NONE, 1, 0, tr=1, M=256, K=192, k_split=128, **big), _case("ksplit128of192", NONE, 1, ROWSP, tr=1, M=128, K=192, k_split=128, **big),
              _case("msplit_acc", GLN_PRELU, 0, RES, tr=0, M=256, K=64, **heads, **big), _case("m384", NONE, 0, ROWS, tr=1, M=384, K=64, **big),
              _case("m1024", NONE, 0, STATS, tr=0, M=1024, K=64, **big), _case("k1024", GLN_BWD, 0, 0, tr=1, M=128, K=1024, **big)]
    if env == "coop":
        e += [_case("k1024", NONE, 0, 0, tr=0, M=128, K=1024, **big), _case("k1024", NONE, 1, ROWSP, tr=1, M=256, K=1024, **big),
              _case("gln512", GLN_PRELU, 0, RES, tr=0, M=256, K=512, **heads, **big), _case("gln544", GLN, 0, 0, tr=0, M=128, K=544, **big),
              _case("m384", GLN_BWD, 0, RES, tr=1, M=384, K=512, **big), _case("m1024", PRELU, 0, SIG, tr=0, M=1024, K=128, **big)]
        for (pro, sp, ef, kw) in MODEL_STEP:
            e.append(_case("model", pro, sp, ef, tr=(pro, sp, ef) in BACKWARD, B=16, T=3999, ldt=4096, **kw))
    if env == "staged":
        e += [_case("k1024", NONE, 1, 0, tr=1, M=128, K=1024, arith=F32, packed=False, **big), _case("gln544", GLN, 0, 0, tr=0, M=128, K=544, **big),
              _case("model", GLN_PRELU, 0, RES, tr=0, B=16, T=3999, ldt=4096, M=256, K=512, arith=F32, packed=False, **heads)]
    return e


def cases(env, tier):
    """every case of the environment with the instance it is meant to reach under "name"; fails if an instance of ENV_INSTANCES[env] has none"""
    out = _all_cases(env, tier)
    for i, c in enumerate(out):
        c["name"] = dispatch(ENVS[env], c)
        c["seed"] = zlib.crc32("{}/{}/{}".format(env, tier, i).encode())
    missing = sorted(set(ENV_INSTANCES[env]) - set(c["name"] for c in out))
    assert not missing, "no case reaches {}".format(missing)
    return out


# ---------------------------------------------------------------------------------------------------------------- operands
def operands(c):
    """-> (kwargs of pw_gemm as CPU fp32 / fp64 tensors, names of the tensors the call writes)"""
    import torch
    g = torch.Generator().manual_seed(c["seed"])
    B, M, K, T, ldt, pro, ef, tr = c["B"], c["M"], c["K"], c["T"], c["ldt"], c["pro"], c["epi"], c["tr"]
    k1, Mf = c["k_split"] or K, c["m_split"] or M

    def rn(*s):
        return torch.randn(*s, generator=g, dtype=torch.float64)

    def padded(C, spread=0.0, mean=0.0):
        x = (rn(B, C, ldt) + mean) * torch.exp(spread * rn(B, C, 1))
        x[..., T:] = 0
        return x.float().contiguous()

    def slots(tot):                                   # (B, 2) totals spread unevenly over the slots
        w = torch.rand(SLOTS, generator=g, dtype=torch.float64)
        return (tot.unsqueeze(1) * (w / w.sum()).view(1, SLOTS, 1)).contiguous()

    def stats_of(u):
        v = u[..., :T].double()
        return slots(torch.stack([v.sum((1, 2)), (v * v).sum((1, 2))], 1))
    shared_scale = (not c["name"].startswith(("pc<", "coop<"))) and c["arith"] == F16X3
    Am = (rn(M, K) * K ** -0.5 * torch.exp((0.0 if shared_scale else 4.0) * rn(M, 1))).float()
    Xf = padded(K, 3.0, mean=0.7 if pro in (GLN, GLN_PRELU) else 0.0)
    kw = dict(B=B, M=M, K=K, T=T, ldt=ldt, trans_a=tr, k_split=c["k_split"], m_split=c["m_split"], pro_mode=pro, epi_flags=ef, accumulate=c["accumulate"],
              arith=c["arith"], eps=1e-12)
    kw["A"] = (Am[:, :k1].t() if tr else Am[:, :k1]).contiguous()
    kw["X"] = Xf[:, :k1].contiguous()
    if c["k_split"]:
        kw["A2"] = (Am[:, k1:].t() if tr else Am[:, k1:]).contiguous()
        kw["X2"] = Xf[:, k1:].contiguous()
    if not tr:
        kw["bias"] = rn(M).float()
    written = ["Y"]
    al = torch.tensor([0.25])
    if pro in (PRELU, GLN_PRELU, GLN_BWD):
        kw["pro_alpha"] = al
    if pro in (GLN, GLN_PRELU):
        u = torch.where(Xf > 0, Xf, al * Xf) if pro == GLN_PRELU else Xf
        kw.update(pro_stats=stats_of(u), pro_gamma=(rn(K) + 1).float(), pro_beta=rn(K).float(), count=float(K * T))
    if pro == GLN_BWD:
        a = padded(K, 1.0, mean=0.3)
        kw.update(pro_stats=stats_of(torch.where(a > 0, a, al * a)), pro_gamma=(rn(K) + 1).float(), pro_aux=a, count=float(K * T),
                  pro_store=torch.full((B, K, ldt), float("nan")), pro_dalpha=torch.full((1,), 100.0, dtype=torch.float64))
        if ef & RES:                                   # the means formed by the kernel from a producer's slots
            kw["pro_bacc"] = slots(rn(B, 2) * 0.01 * K * T)
        else:
            kw["pro_bsum"] = (rn(B, 2) * 0.01).float()
        written += ["pro_store", "pro_dalpha"]
    if ef & STATS:
        kw.update(epi_alpha=torch.tensor([0.2]), epi_stats=slots(rn(B, 2).abs() * 3.0))
        written.append("epi_stats")
    if ef & RES:
        kw["epi_res"] = padded(Mf)
    if ef & PBWD:
        kw.update(epi_aux=padded(M), epi_alpha=torch.tensor([0.2]), epi_dalpha=torch.full((1,), -3.0, dtype=torch.float64))
        written.append("epi_dalpha")
    if ef & ROWS:
        kw.update(epi_aux=padded(M, 0.0, 0.2), epi_rowpart=torch.full((B, M, ldt // 64, 2), float("nan")))
        if ef & 32:
            kw["epi_alpha"] = torch.tensor([0.2])
        written.append("epi_rowpart")
    if c["m_split"]:
        kw["Y"] = torch.full((B, Mf, ldt), float("nan"))
        kw["Y2"] = padded(M - Mf) if c["accumulate"] else torch.full((B, M - Mf, ldt), float("nan"))
        written.append("Y2")
    else:
        kw["Y"] = padded(M) if c["accumulate"] else torch.full((B, M, ldt), float("nan"))
    return kw, written


# ---------------------------------------------------------------------------------------------------------------- the contract in float64
def reference(c, kw):
    """include/sepkernels.h, sep_gemm_desc: prologue -> contraction -> bias -> epilogue, in float64 on the operands of `kw` (as they are
    BEFORE the call).  -> {output name: (value, scale)}; epi_stats as (B, 2) totals over the slots"""
    import torch
    B, M, K, T, ldt, pro, ef, tr = c["B"], c["M"], c["K"], c["T"], c["ldt"], c["pro"], c["epi"], c["tr"]
    k1, Mf = c["k_split"] or K, c["m_split"] or M
    f = lambda name: kw[name].double()
    Am = f("A").reshape(k1, M).t() if tr else f("A").reshape(M, k1)
    X = f("X").reshape(B, k1, ldt)
    if c["k_split"]:
        Am = torch.cat([Am, f("A2").reshape(K - k1, M).t() if tr else f("A2").reshape(M, K - k1)], 1)
        X = torch.cat([X, f("X2").reshape(B, K - k1, ldt)], 1)
    valid = (torch.arange(ldt) < T).view(1, 1, ldt)
    zero = torch.zeros((), dtype=torch.float64)
    prelu = lambda x, a: torch.where(x > 0, x, a * x)
    out = {}
    if pro >= GLN:
        st = kw["pro_stats"].sum(1)
        mean = (st[:, 0] / kw["count"]).view(B, 1, 1)
        rstd = 1.0 / torch.sqrt((st[:, 1].view(B, 1, 1) / kw["count"] - mean * mean).clamp_min(0.0) + kw["eps"])
    if pro == NONE:
        xp, axp = X, X.abs()
    elif pro == PRELU:
        xp = prelu(X, f("pro_alpha"))
        axp = xp.abs()
    elif pro in (GLN, GLN_PRELU):
        u = prelu(X, f("pro_alpha")) if pro == GLN_PRELU else X
        sc = f("pro_gamma").view(1, K, 1) * rstd
        xp = (u - mean) * sc + f("pro_beta").view(1, K, 1)
        axp = sc.abs() * (u.abs() + mean.abs()) + f("pro_beta").abs().view(1, K, 1)
    else:
        a, al = f("pro_aux").reshape(B, K, ldt), f("pro_alpha")
        u = prelu(a, al)
        if kw.get("pro_bacc") is not None:
            ba = kw["pro_bacc"].sum(1)
            mg = (ba[:, 0] / kw["count"]).view(B, 1, 1)
            mgx = rstd * ((ba[:, 1] - mean.view(B) * ba[:, 0]) / kw["count"]).view(B, 1, 1)
        else:
            mg, mgx = f("pro_bsum")[:, 0].view(B, 1, 1), f("pro_bsum")[:, 1].view(B, 1, 1)
        gam = f("pro_gamma").view(1, K, 1)
        du = rstd * (gam * X - mg - (u - mean) * rstd * mgx)
        adu = rstd * (gam.abs() * X.abs() + mg.abs() + (u.abs() + mean.abs()) * rstd * mgx.abs())
        slope = torch.where(a > 0, torch.ones_like(a), al * torch.ones_like(a))
        xp, axp = torch.where(valid, du * slope, zero), torch.where(valid, adu * slope.abs(), zero)
        neg = valid & (a <= 0)
        out["pro_store"] = (xp, axp)
        out["pro_dalpha"] = (f("pro_dalpha") + torch.where(neg, du * a, zero).sum(), f("pro_dalpha").abs() + torch.where(neg, adu * a.abs(), zero).sum())
    y = torch.einsum("mk,bkt->bmt", Am, xp)
    s = torch.einsum("mk,bkt->bmt", Am.abs(), axp)
    if kw.get("bias") is not None:
        y, s = y + f("bias").view(1, M, 1), s + f("bias").abs().view(1, M, 1)
    if ef & STATS:
        al = f("epi_alpha")
        u = torch.where(valid, prelu(y, al), zero)
        su = torch.where(valid, s * max(1.0, abs(float(al))), zero)
        prior = kw["epi_stats"].sum(1)
        out["epi_stats"] = (prior + torch.stack([u.sum((1, 2)), (u * u).sum((1, 2))], 1),
                            prior.abs() + torch.stack([su.sum((1, 2)), (2 * u.abs() * su + u * u).sum((1, 2))], 1))
    if ef & RES:
        r = f("epi_res").reshape(B, Mf, ldt)
        y = torch.cat([y[:, :Mf] + r, y[:, Mf:]], 1)
        s = torch.cat([s[:, :Mf] + r.abs(), s[:, Mf:]], 1)
    if ef & SIG:
        y = 1.0 / (1.0 + torch.exp(-y))
        s = s / 4 + y
    if ef & PBWD:
        aux, al = f("epi_aux").reshape(B, M, ldt), f("epi_alpha")
        neg = valid & (aux <= 0)
        out["epi_dalpha"] = (f("epi_dalpha") + torch.where(neg, y * aux, zero).sum(), f("epi_dalpha").abs() + torch.where(neg, s * aux.abs(), zero).sum())
        slope = torch.where(aux > 0, torch.ones_like(aux), al * torch.ones_like(aux))
        y, s = y * slope, s * slope.abs()
    if ef & ROWS:
        u = f("epi_aux").reshape(B, M, ldt)
        if ef & 32:
            u = prelu(u, f("epi_alpha"))
        yv, sv = torch.where(valid, y, zero), torch.where(valid, s, zero)
        pieces = lambda v: v.reshape(B, M, ldt // 64, 64).sum(-1)
        out["epi_rowpart"] = (torch.stack([pieces(yv), pieces(yv * u)], -1), torch.stack([pieces(sv), pieces(sv * u.abs())], -1))
    y, s = torch.where(valid, y, zero), torch.where(valid, s, zero)
    if c["m_split"]:
        out["Y"] = (y[:, :Mf], s[:, :Mf])
        prior = f("Y2").reshape(B, M - Mf, ldt) if c["accumulate"] else zero
        out["Y2"] = (y[:, Mf:] + prior, s[:, Mf:] + prior.abs())
    else:
        prior = f("Y").reshape(B, M, ldt) if c["accumulate"] else zero
        out["Y"] = (y + prior, s + prior.abs())
    return out


FRAMES = ("Y", "Y2", "pro_store")                # tensors laid out (B, rows, ldt): compared over [0, T), pad frames must be exactly zero
SUMS = ("epi_stats", "epi_rowpart", "epi_dalpha", "pro_dalpha")
A_ARITH = {F32: 0.0, BF16X6: 0.0, F16X3: 2.0 ** -19}


def measure(c, name, got, ref, scale):
    """max |got - ref| / scale of one output (epi_stats: the totals over the slots; frame tensors: the valid frames)"""
    import torch
    got = got.double()
    if name == "epi_stats":
        got = got.sum(1)
    got = got.reshape(ref.shape)
    if name in FRAMES:
        got, ref, scale = got[..., :c["T"]], ref[..., :c["T"]], scale[..., :c["T"]]
    if not torch.isfinite(got).all():
        return float("inf")
    return float(((got - ref).abs() / (scale + 1e-300)).max())


def bound(c, kernel, name, e32):
    r = 128 * 2.0 ** -24 if name in SUMS else 8 * 2.0 ** -24 if (c["epi"] & SIG and name in ("Y", "Y2")) else 0.0
    return 4 * e32 + A_ARITH[kernel_arith(kernel)] + r


GUARD = 1024                                     # floats behind every written buffer that must come back untouched


def run_case(K, c, to_device, sync, perturb=0.0):
    """one case through the backend K -> its record.  `perturb`: the negative control adds perturb * scale to the device's Y"""
    import torch
    import sepkernels
    from emulator import EmuBackend
    kw, written = operands(c)
    before = {k: v.clone() for k, v in kw.items() if torch.is_tensor(v)}
    # the device's copies: written buffers sit in front of a guard area
    dkw, guards = {}, {}
    for k, v in kw.items():
        if torch.is_tensor(v) and k in written:
            flat = torch.full((v.numel() + GUARD,), 12345.0, dtype=v.dtype)
            flat[:v.numel()] = v.reshape(-1)
            flat = to_device(flat)
            guards[k] = flat
            dkw[k] = flat[:v.numel()].view(v.shape)
        elif torch.is_tensor(v):
            dkw[k] = to_device(v)
        else:
            dkw[k] = v
    if c["packed"]:
        k1 = c["k_split"] or c["K"]
        Am = dkw["A"].reshape(k1, c["M"]).t() if c["tr"] else dkw["A"].reshape(c["M"], k1)
        if c["k_split"]:
            Am = torch.cat([Am, dkw["A2"].reshape(c["K"] - k1, c["M"]).t() if c["tr"] else dkw["A2"].reshape(c["M"], c["K"] - k1)], 1)
        dkw["A_pk"] = K.pack_weights([(Am.contiguous(), c["M"], c["K"], 0)])[0]
    if c["name"] == "error":
        try:
            K.pw_gemm(**dkw)
            return dict(case=c, kernel=sepkernels.last_kernel(), ok=False, why="the call was expected to be refused")
        except sepkernels.SepKernelsError as e:
            return dict(case=c, kernel="error", ok=True, message=str(e)[-120:], outputs={})
    ref = reference(c, kw)
    ekw = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in kw.items()}      # the reference's own fp32 evaluation
    EmuBackend().pw_gemm(**ekw)
    K.pw_gemm(**dkw)
    kernel = sepkernels.last_kernel()
    sync()
    rec = dict(case=c, kernel=kernel, outputs={}, pads_zero=True, inputs_intact=True, guards_intact=True)
    for name in written:
        got = dkw[name].cpu()
        r, s = ref[name]
        if perturb and name == "Y":
            got = got.double() + perturb * s.reshape(got.shape)
        err, e32 = measure(c, name, got, r, s), measure(c, name, ekw[name], r, s)
        rec["outputs"][name] = dict(err=err, e32=e32, bound=bound(c, kernel, name, e32))
        if name in FRAMES and not bool((got[..., c["T"]:] == 0).all()):
            rec["pads_zero"] = False
        tail = guards[name].cpu()[dkw[name].numel():]
        if not bool((tail == 12345.0).all()):
            rec["guards_intact"] = False
    for k, v in before.items():
        if k not in written and not torch.equal(dkw[k].cpu(), v):
            rec["inputs_intact"] = False
    rec["ok"] = (kernel == c["name"] and rec["pads_zero"] and rec["inputs_intact"] and rec["guards_intact"] and
                 all(o["err"] <= o["bound"] for o in rec["outputs"].values()))
    return rec


def run(env, tier, K, to_device, sync, log=None):
    """every case of cases(env, tier) through the backend K, which must live in a process started with ENVS[env]"""
    for k in SWITCHES:
        assert os.environ.get(k) == ENVS[env].get(k), "the process environment is not that of '{}' ({})".format(env, k)
    recs = []
    for c in cases(env, tier):
        rec = run_case(K, c, to_device, sync)
        recs.append(rec)
        if log:
            worst = max([o["err"] / o["bound"] for o in rec["outputs"].values()] or [0.0])
            log("{:4s} {:66s} {:14s} B={} M={} K={} T={} ldt={}  worst err/bound {:.3f}".format("ok" if rec["ok"] else "FAIL", rec["kernel"], c["regime"], c["B"],
                                                                                                c["M"], c["K"], c["T"], c["ldt"], worst))
    return recs


def failures(recs):
    """one line per record that is not ok"""
    out = []
    for r in recs:
        if not r["ok"]:
            c = r["case"]
            bad = {k: v for k, v in r.get("outputs", {}).items() if not v["err"] <= v["bound"]}
            out.append("{} (meant {}) {} B={} M={} K={} T={} ldt={} arith={} packed={}: pads_zero={} inputs_intact={} guards_intact={} over bound: {} {}".format(
                r["kernel"], c["name"], c["regime"], c["B"], c["M"], c["K"], c["T"], c["ldt"], c["arith"], c["packed"], r.get("pads_zero"), r.get("inputs_intact"),
                r.get("guards_intact"), bad, r.get("why", "")))
    return out


def summary(recs):
    """-> one row per (instance, shape regime): the worst err / bound over the cases and outputs, with that output's err, e32 and bound"""
    rows = {}
    for r in recs:
        for name, o in (r.get("outputs") or {"-": dict(err=0.0, e32=0.0, bound=1.0)}).items():
            key = (r["kernel"], r["case"]["regime"])
            ratio = o["err"] / o["bound"]
            if key not in rows or ratio > rows[key]["ratio"]:
                c = r["case"]
                rows[key] = dict(instance=r["kernel"], regime=c["regime"], output=name, err=o["err"], e32=o["e32"], bound=o["bound"], ratio=ratio,
                                 shape=dict(B=c["B"], M=c["M"], K=c["K"], T=c["T"], ldt=c["ldt"]))
    return [rows[k] for k in sorted(rows)]


def child_command(env, tier, out, backend=None):
    """(argv, process environment) of the child that runs one environment"""
    penv = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    penv.update(ENVS[env])
    argv = [sys.executable, os.path.abspath(__file__), "--env", env, "--tier", tier, "--out", out]
    return argv + (["--backend", backend] if backend else []), penv


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--env", required=True, choices=sorted(ENVS))
    ap.add_argument("--tier", required=True, choices=["host", "device"])
    ap.add_argument("--out", required=True)
    ap.add_argument("--backend", default="hip", help="hip (default) or hostsim:<path of the host-simulation library>")
    ap.add_argument("--profile", default=None, help="JSON file whose [tier][env] entry is replaced by this run's summary (profiles/r11_gemm_instances.json)")
    args = ap.parse_args()
    for k in SWITCHES:                            # the switches are read once per process, at the first call
        os.environ.pop(k, None)
    os.environ.update(ENVS[args.env])
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    import sepkernels
    log = lambda s: print(s, flush=True)
    if args.backend.startswith("hostsim:"):
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import hostsim
        with hostsim.HostSimBackend(args.backend[8:]) as K:
            recs = run(args.env, args.tier, K, (lambda t: t.clone()), (lambda: None), log)
    else:
        recs = run(args.env, args.tier, sepkernels.backend(), (lambda t: t.cuda()), torch.cuda.synchronize, log)
    with open(args.out, "w") as fh:
        json.dump(recs, fh)
    if args.profile:
        prof = json.load(open(args.profile)) if os.path.exists(args.profile) else {}
        prof.setdefault(args.tier, {})[args.env] = summary(recs)
        with open(args.profile, "w") as fh:
            json.dump(prof, fh, indent=1)
    bad = failures(recs)
    for line in bad:
        print("FAIL", line)
    print("{}: {} cases, {} failures".format(args.env, len(recs), len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    raise SystemExit(main())
