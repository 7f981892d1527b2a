"""CPU: every kernel instance behind the entry points of the dual-path separators -- csrc/linear.hip, csrc/lstm.hip, csrc/attn.hip and
csrc/rownorm.hip --, reached BY NAME on the host simulation of the kernel sources and compared with the float64 run of the call's contract, token
row by token row, slab by slab and sequence by sequence (tests/dualpath_matrix.py: the ledger, the case matrix, the reference, the metric and the
measured bounds).  The default environment runs in this process, family by family; each value of SEPK_LSTM_NS4 in a child process -- the
dispatcher reads the switch once per process."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                         # noqa: E402
import dualpath_matrix as DM           # noqa: E402

pytestmark = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++ (ext_vector_type)")
CSRC = os.path.join(ROOT, "dnn-based_source_separation_amd", "csrc")
HOST = ((lambda t: t.clone()), (lambda: None))


@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim.build(str(tmp_path_factory.mktemp("hostsim_dualpath")))


@pytest.fixture(scope="module")
def reached():
    """instance names the families' runs reported, filled in by the per-family test below"""
    return {}


def _check(recs, expected):
    assert len(recs) == len(expected)
    assert not DM.failures(recs), "\n".join(DM.failures(recs))
    for rec in recs:
        assert rec["kernel"] == rec["case"]["name"] and rec["kernel"] in DM.INSTANCES, rec      # the case reached the instance it names
        assert rec["inputs_intact"] and rec["guards_intact"], rec
        for name, o in rec["outputs"].items():
            assert o["err"] <= o["bound"], (rec["kernel"], name, o)


@pytest.mark.parametrize("family", list(DM.FAMILIES))
def test_every_instance_of_the_family_is_reached_and_within_its_bound(sim_library, reached, family):
    for k in DM.SWITCHES:
        assert k not in os.environ
    with hostsim.HostSimBackend(sim_library) as K:
        recs = DM.run("default", K, *HOST, families=(family,), tier="host")
    _check(recs, [c for c in DM.cases("default", "host") if c["family"] == family])
    reached[family] = set(rec["kernel"] for rec in recs)


def test_the_union_over_the_families_is_the_ledger(reached):
    """no instance of the dispatch tables unreached, no name emitted that the ledger does not know (needs the per-family runs above)"""
    assert sorted(reached) == sorted(DM.FAMILIES), "a family's run is missing: {}".format(sorted(set(DM.FAMILIES) - set(reached)))
    union = set().union(*reached.values())
    assert sorted(union) == DM.INSTANCES, (sorted(set(DM.INSTANCES) - union), sorted(union - set(DM.INSTANCES)))


@pytest.mark.parametrize("env", [e for e in DM.ENVS if e != "default"])
def test_under_the_switch_every_unforced_case_reaches_the_forced_sweep(sim_library, tmp_path, env):
    out = str(tmp_path / "records.json")
    argv, penv = DM.child_command(env, out, backend="hostsim:" + sim_library)
    r = subprocess.run(argv, env=penv, capture_output=True, text=True, timeout=3600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
    recs = json.load(open(out))
    _check(recs, DM.cases(env, "host"))
    four = env == "lstm_ns4_1"
    assert all(rec["kernel"].startswith(("lstm_fwd4<", "lstm_bwd4<")) == four for rec in recs)
    assert {rec["kernel"] for rec in recs} == {"lstm_{}{}<{}>".format(k, "4" if four else "", H) for k, hs in (("fwd", (16, 32, 64, 128)), ("bwd", (16,))) for H in hs}


def test_the_ledger_lists_every_launch_line_of_the_dispatchers():
    """INSTANCES against the four sources: every sep_set_kernel statement contributes the string literals it chooses between; a statement inside
    a launch macro is spelled out from the arguments of every use of the macro"""
    src = {f: open(os.path.join(CSRC, f + ".hip")).read() for f in ("linear", "lstm", "attn", "rownorm")}
    stmts = {f: re.findall(r"sep_set_kernel\(([^;]*)\);", s) for f, s in src.items()}
    plain = {f: [lit for s in v if "#" not in s for lit in re.findall(r'"([^"]*)"', s)] for f, v in stmts.items()}
    assert {f: (len(v), sum("#" in s for s in v)) for f, v in stmts.items()} == {"linear": (2, 1), "lstm": (4, 0), "attn": (2, 2), "rownorm": (4, 2)}
    uses = lambda f, pattern: re.findall(pattern, src[f])
    names = []
    # linear: SEP_LIN(TI, TJ) spells one name per MODE; the forward and the input gradient are launched with TI = 128 only
    tiles = uses("linear", r"SEP_LIN\((\d+), (\d+)\);")
    assert len(tiles) == 4
    names += ["linear<{},{},{}>".format(m, ti, tj) for m in ("fwd", "bwd_input", "bwd_weight") for ti, tj in tiles if m == "bwd_weight" or ti == "128"]
    assert len(re.findall(r"lin_launch<LIN_(?:FWD|BWD_INPUT)>\(p, 128, tj,", src["linear"])) == 2
    # attention: SEP_ATF(DD) / SEP_ATB(DD) use SEP_AT?_ONE(DD, ML, NW) four times each and are used once per head width
    for k, one, outer in (("fwd", "SEP_ATF_ONE", "SEP_ATF"), ("bwd", "SEP_ATB_ONE", "SEP_ATB")):
        sizes, widths = re.findall(one + r"\(DD, (\d+), (\d+)\);", src["attn"]), re.findall(outer + r"\((\d+)\);", src["attn"])
        assert len(sizes) == 4 and len(widths) == 3
        names += ["attn_{}<{},{},{}>".format(k, D, ml, nw) for D in widths for ml, nw in sizes]
    for k, macro in (("fwd", "SEP_RNF"), ("bwd", "SEP_RNB")):
        njs = re.findall(macro + r"\((\d)\);", src["rownorm"])
        assert len(njs) == 4
        names += ["rownorm_{}<{}>".format(k, nj) for nj in njs]
    assert (len(plain["linear"]), len(plain["lstm"]), len(plain["attn"]), len(plain["rownorm"])) == (2, 16, 0, 2)
    names += [lit for v in plain.values() for lit in v]
    assert len(names) == len(set(names)) == len(DM.INSTANCES) == 8 + 2 + 16 + 24 + 8 + 2
    assert sorted(names) == DM.INSTANCES


def test_every_case_names_an_instance_and_the_matrix_is_the_one_agreed():
    """cases() itself refuses a matrix that misses an instance; here: every environment builds on either tier, no case dropped quietly, the
    boundary cases of the automatic LSTM rule expect what the rule says, and the shapes the matrix was planned with are in"""
    for env in DM.ENVS:
        for tier in ("device", "host"):
            cs = DM.cases(env, tier)
            assert cs and all(c["name"] in DM.INSTANCES for c in cs)
    counts = lambda tier: {f: sum(c["family"] == f for c in DM.cases("default", tier)) for f in DM.FAMILIES}
    assert counts("device") == {"linear": 68, "lstm": 82, "attn": 114, "rownorm": 58, "relu_drop": 12, "chunk_tokens": 16}
    assert counts("host") == {"linear": 68, "lstm": 78, "attn": 114, "rownorm": 58, "relu_drop": 8, "chunk_tokens": 16}
    assert {e: len(DM.cases(e, "device")) for e in DM.ENVS} == {"default": 350, "lstm_ns4_0": 14, "lstm_ns4_1": 14}
    auto = {(c["nseq"], c["reverse"], c["name"]) for c in DM.cases("default") if c["op"] == "lstm_fwd" and c["L"] == 2 and c["nseq"] >= 512}
    assert auto == {(1024, 0, "lstm_fwd4<16>"), (1025, 0, "lstm_fwd<16>"), (512, 2, "lstm_fwd4<16>"), (513, 2, "lstm_fwd<16>")}
    att = [c for c in DM.cases("default") if c["family"] == "attn"]
    assert {c["L"] for c in att if c["D"] == 8} == {33, 64, 65, 129, 257, 320} and {c["L"] for c in att} >= {1, 31, 32}
    for inst in (n for n in DM.INSTANCES if n.startswith("attn_")):                       # per instance: the three profiles and both dropout rates
        mine = [c for c in att if c["name"] == inst]
        assert {c["profile"] for c in mine} == {"unit", "spread", "lastmax"} and {c["p_drop"] for c in mine} == {0.0, 0.1}, inst
    assert {c["C"] for c in DM.cases("default") if c["family"] == "rownorm"} == {4, 252, 256, 260, 512, 516, 768, 772, 1024}
    lstm = [c for c in DM.cases("default") if c["family"] == "lstm" and (c["reverse"] >> 8) & 3]
    assert {(c["H"], c["reverse"] & 0x4ff, c["reverse"] >> 8 & 3, c["op"]) for c in lstm} == {(H, r, f, op) for H in (16, 32, 64, 128) for r in (0, 1, 2, 0x402) for f in (1, 2)
                                                                                                for op in ("lstm_fwd", "lstm_bwd")}


def test_the_bounds_in_the_ledger_follow_from_the_float32_run():
    """FAMILIES: e32 is (an upper bound of) the worst figure of the contract's float32 run against its float64 run, the bound follows by the
    rule; the float32 run itself passes every case within the bound (a case it cannot pass would be a wrong case)"""
    worst = DM.float32_figures()
    for f, entry in DM.FAMILIES.items():
        if entry["e32"] is None:
            continue
        assert worst[f] <= entry["e32"], (f, worst[f], entry)
        assert entry["e32"] <= 1.5 * worst[f], (f, worst[f], entry)      # ... and not padded
        assert entry["bound"] == DM.bound_rule(entry["e32"], max(DM.OLD[f].values())), (f, entry)
        for out, old in DM.OLD[f].items():
            assert DM.bound_of(f, out) == min(old, entry["bound"]) <= old
    recs = [DM.run_case(DM.FloatRun(), c, None, None) for c in DM.cases("default", "device")]
    assert not DM.failures(recs), "\n".join(DM.failures(recs))


# ------------------------------------------------------------------------------------------------- controls of the checker
def _case(op, also=lambda c: True, **kw):
    return [c for c in DM.cases("default", "host") if c["op"] == op and all(c.get(k) == v for k, v in kw.items()) and also(c)][0]


def _quiet_row(got, a, ref):
    """every element of the quietest token row of y moved by 2^-14 of its own scale"""
    sc = ref["y"]["scale"]
    row = int(sc.amax(1).argmin())
    got["y"][row] += (2.0 ** -14 * sc[row]).float()
    _quiet_row.global_max = float((got["y"].double() - ref["y"]["ref"]).abs().max() / ref["y"]["ref"].abs().max())


def _swap_slabs(got, a, ref):
    got["partial"][[0, 1]] = got["partial"][[1, 0]].clone()


def _other_sequence(got, a, ref):
    got["h"][0, 1] = got["h"][0, 0].clone()


def _keep_a_dropped(got, a, ref):
    """one dropped element of dres takes the value it would have had if kept"""
    idx = tuple(int(i) for i in ref["dres"]["zero"].nonzero()[0])
    got["dres"][idx] = got["ds"][idx] * DM.keep_inv(0.25) + 1e-30


def _drop_a_kept(got, a, ref):
    idx = tuple(int(i) for i in ((~ref["dres"]["zero"]) & (ref["dres"]["ref"] != 0)).nonzero()[0])
    got["dres"][idx] = 0.0


CONTROLS = {
    "token_row": (lambda: _case("linear_fwd", ntok=300, K=64), "y", _quiet_row),
    "slab_swap": (lambda: _case("linear_bwd_weight", ntok=301, nslab=3), "partial", _swap_slabs),
    "sequence": (lambda: _case("lstm_fwd", also=lambda c: c["reverse"] in (DM.FORCE16, DM.FORCE4) and c["nseq"] >= 3 and c["L"] >= 2), "h", _other_sequence),
    "dropout_kept": (lambda: _case("rownorm_bwd", p_drop=0.25, also=lambda c: c["rows"] >= 3 and c["C"] >= 252), "dres", _keep_a_dropped),
    "dropout_dropped": (lambda: _case("rownorm_bwd", p_drop=0.25, also=lambda c: c["rows"] >= 3 and c["C"] >= 252), "dres", _drop_a_kept),
}


@pytest.mark.parametrize("which", list(CONTROLS))
def test_the_checker_rejects_a_wrong_result(sim_library, which):
    """the unperturbed result passes; the check rejects one token row moved by 2^-14 of its scale (2e-4 of the output's GLOBAL maximum, the figure
    both() of tests/test_gpu_kernels.py looks at, would have let it through), one weight-gradient slab swapped with its neighbour (their sum, which
    the older test also looks at, is unchanged), one sequence's h replaced by another's, and one dropout decision flipped either way"""
    make, out, tamper = CONTROLS[which]
    c = make()
    with hostsim.HostSimBackend(sim_library) as K:
        good = DM.run_case(K, c, *HOST)
        assert good["ok"], good
        bad = DM.run_case(K, c, *HOST, tamper=tamper)
    assert not bad["ok"] and bad["outputs"][out]["err"] > bad["outputs"][out]["bound"], bad
    assert bad["kernel"] == good["kernel"] and bad["inputs_intact"] and bad["guards_intact"]
    assert all(o["err"] <= o["bound"] for n, o in bad["outputs"].items() if n != out)
    if which == "token_row":
        assert _quiet_row.global_max <= 2e-4


def test_a_length_beyond_the_tiles_is_refused(sim_library):
    with hostsim.HostSimBackend(sim_library) as K:
        qkv, o, lse = torch.zeros(1, 321, 3, 1, 8), torch.zeros(1, 321, 1, 8), torch.zeros(1, 1, 321)
        with pytest.raises(Exception):
            K.attn_fwd(qkv, o, lse, 1, 321, 1, 8, 1.0, 0.0, 0)
        with pytest.raises(Exception):
            K.attn_bwd(qkv, o, o, lse, lse.clone(), qkv.clone(), 1, 321, 1, 8, 1.0, 0.0, 0)
