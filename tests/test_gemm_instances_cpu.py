"""CPU: every kernel instance sep_pw_gemm can launch, reached BY NAME on the host simulation of the kernel sources and compared with a
float64 restatement of the call's contract in the error model's own metric (tests/gemm_matrix.py: the ledger, the case matrix, the
reference and the bound).  One child process per environment -- the dispatchers read their SEPK_* switches once per process."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import hostsim                         # noqa: E402
import gemm_matrix as GM               # noqa: E402

pytestmark = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++ (ext_vector_type)")


@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim.build(str(tmp_path_factory.mktemp("hostsim_gemm")))


@pytest.fixture(scope="module")
def reached():
    """instance names the environments' children reported, filled in by the per-environment test below"""
    return {}


@pytest.mark.parametrize("env", list(GM.ENVS))
def test_every_instance_of_the_environment_is_reached_and_within_its_bound(sim_library, reached, tmp_path, env):
    out = str(tmp_path / "records.json")
    argv, penv = GM.child_command(env, "host", out, backend="hostsim:" + sim_library)
    r = subprocess.run(argv, env=penv, capture_output=True, text=True, timeout=3600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
    recs = json.load(open(out))
    assert len(recs) == len(GM.cases(env, "host"))
    assert not GM.failures(recs)
    for rec in recs:
        assert rec["kernel"] == rec["case"]["name"], rec                 # the case reached the instance it names
        assert rec["pads_zero"] and rec["inputs_intact"] and rec["guards_intact"], rec
        for name, o in rec["outputs"].items():
            assert o["err"] <= o["bound"], (rec["kernel"], name, o)
    names = set(rec["kernel"] for rec in recs)
    assert names >= set(GM.ENV_INSTANCES[env]), sorted(set(GM.ENV_INSTANCES[env]) - names)
    reached[env] = names


def test_the_union_over_the_environments_is_the_ledger(reached):
    """no instance of the dispatch tables unreached, no name emitted that the ledger does not know (needs the per-environment runs above)"""
    assert sorted(reached) == sorted(GM.ENVS), "an environment's run is missing: {}".format(sorted(set(GM.ENVS) - set(reached)))
    union = set().union(*reached.values())
    assert sorted(union) == GM.INSTANCES, (sorted(set(GM.INSTANCES) - union), sorted(union - set(GM.INSTANCES)))


def test_the_ledger_lists_every_launch_line_of_the_dispatchers():
    """INSTANCES against the sources: the dispatchers' one table of fused products (SEP_FUSED_COMBOS, csrc/gemm_common.hpp: a PK row exists in
    the packed families and the direct kernel, a DIRECT row in the direct kernel alone) and one list of prologues (SEP_GEMM_PROLOGUES:
    direct_rt), each row restated by hand in tests/gemm_matrix.py; every dispatcher expands the table once and spells no combination itself"""
    import re
    csrc = os.path.join(ROOT, "dnn-based_source_separation_amd", "csrc")
    text = lambda f: open(os.path.join(csrc, f)).read()
    val = {"false": 0, "true": 1, "0": 0, **{v: k for k, v in GM.PRO_NAME.items()}, **{v: k for k, v in GM.EPI_NAME.items()}}
    rows = [(kind, val[t], val[p], val[s], val[e], int(bit)) for kind, t, p, s, e, bit in
            re.findall(r"^ +(PK|DIRECT)\((false|true), (SEP_PRO_\w+), (false|true), ([^,]+), (\d)\)", text("gemm_common.hpp"), re.M)]
    packed = [r for r in rows if r[0] == "PK"]
    assert len(packed) == len(GM.PACKED_COMBOS) == 14 and set(r[2:5] for r in packed) == set(GM.PACKED_COMBOS)
    assert set(r[2:5] for r in packed if r[1]) == GM.BACKWARD                      # the orientation the step uses each packed combination in
    mi4 = sorted((r[5], r[2:5]) for r in rows if r[5])
    assert len(mi4) == len(GM.COOP_MI4) == 3 and mi4 == [(1 << i, c) for i, c in enumerate(GM.COOP_MI4)] and all(r[0] == "PK" for r in rows if r[5])
    assert len(rows) == len(GM.DIRECT_COMBOS) == 16 and set(r[1:5] for r in rows) == set(GM.DIRECT_COMBOS)
    pros = re.search(r"^#define SEP_GEMM_PROLOGUES\(X\)(.*)$", text("gemm_common.hpp"), re.M).group(1)
    pros = [(val[p], int(two)) for p, two in re.findall(r"X\((SEP_PRO_\w+), ([01])\)", pros)]
    rt = [GM.direct_rt_name(tr, p, sp) for p, two in pros for tr in (0, 1) for sp in range(1 + two)]
    assert len(rt) == len(GM.DIRECT_RT_ALL) == 18 and sorted(rt) == sorted(GM.DIRECT_RT_ALL)
    for f in ("gemm_pc.hip", "gemm_coop.hip", "gemm.hip"):
        assert text(f).count("SEP_FUSED_COMBOS(") == 1, f
        assert not re.search(r"\(\s*(?:(?:false|true)\s*,\s*)?SEP_PRO_\w+\s*,\s*(?:false|true)\s*,", text(f)), f      # (prologue, two-source, ... spelled out
    assert text("gemm.hip").count("SEP_GEMM_PROLOGUES(") == 1
    assert text("wgrad.hip").count("SEP_WGRAD_XMODES(") == 2 and "SEP_WGRAD_XMODES(" not in text("gemm.hip")      # the weight gradients' switch: wgrad_split, wgrad_direct
    assert len(GM.INSTANCES) == 28 + 2 * (28 + 3) + (14 * 3 + 2) + 18 + 1


def test_the_launch_lines_of_the_products_the_weight_gradients_and_the_reductions_sit_in_their_files():
    """sep_set_kernel statements per file (a statement inside a launch macro counted once): gemm.hip, wgrad.hip and reduce.hip hold together
    the eight that the one file they were cut from held, and each of the two fallbacks is named in its own file alone.  The kernel behind
    "wgrad" stays in gemm.hip beside pw_gemm_kernel (its generated code changes without it) and is launched through sep_pw_wgrad_staged"""
    import re
    csrc = os.path.join(ROOT, "dnn-based_source_separation_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith(".hip")}
    stmts = {f: re.findall(r"sep_set_kernel\(([^;]*)\);", texts[f]) for f in ("gemm.hip", "wgrad.hip", "reduce.hip")}
    assert {f: len(s) for f, s in stmts.items()} == {"gemm.hip": 5, "wgrad.hip": 3, "reduce.hip": 0}
    assert sum(len(s) for s in stmts.values()) == 8
    assert [s for s in stmts["gemm.hip"] if "#" not in s and "NAME" not in s] == ['"staged"']
    assert [s for s in stmts["wgrad.hip"] if "#" not in s] == ['"wgrad"']
    for lit, home in (('"staged"', "gemm.hip"), ('"wgrad"', "wgrad.hip")):
        assert [f for f, t in texts.items() if lit in t] == [home], lit
    assert [f for f, t in texts.items() if "void pw_wgrad_kernel(" in t] == [f for f, t in texts.items() if "void pw_gemm_kernel(" in t] == ["gemm.hip"]
    assert {f: t.count("sep_pw_wgrad_staged(") for f, t in texts.items() if "sep_pw_wgrad_staged(" in t} == {"gemm.hip": 1, "wgrad.hip": 1}


def test_the_split_arithmetic_and_the_block_decode_are_spelled_in_one_file():
    """the primitives of SEP_ARITH_F16X3 / SEP_ARITH_BF16X6 (the mixed-precision FMA of the two-part split, the two MFMA builtins, the byte
    selector of the three-part split) and the XCD-aware block decode occur in csrc/gemm_common.hpp and in no other file of csrc/ -- as
    code or as comment --, the float4 load in csrc/common.hpp alone: a second copy under another name would be found here.  The one
    exception: pw_wgrad_split_kernel and pw_wgrad_direct_kernel (wgrad.hip) spell the decode out, once each, because their generated code
    changes behind the helper -- exactly two occurrences there, so a third copy is still found.  The chunk products that the kernels of
    gemm.hip and wgrad.hip share are defined in the header and in no .hip file"""
    csrc = os.path.join(ROOT, "dnn-based_source_separation_amd", "csrc")
    texts = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if os.path.isfile(os.path.join(csrc, f))}
    assert {"common.hpp", "gemm_common.hpp", "gemm.hip", "wgrad.hip", "reduce.hip", "gemm_coop.hip", "gemm_pc.hip", "wgrad_pc.hip", "wgrad_pc16.hip", "filterbank.hip", "tcn.hip", "gln.hip", "depthwise.hip", "cln.hip"} <= set(texts)
    once = {"v_fma_mix_f32": "gemm_common.hpp",
            "__builtin_amdgcn_mfma_f32_32x32x16_f16(": "gemm_common.hpp",
            "__builtin_amdgcn_mfma_f32_32x32x16_bf16(": "gemm_common.hpp",
            "0x07060302u": "gemm_common.hpp",
            "float4 ld4(": "common.hpp"}
    for spelling, home in once.items():
        assert [f for f, t in texts.items() if spelling in t] == [home], spelling
    assert {f: t.count("bid & 7") for f, t in texts.items() if "bid & 7" in t} == {"gemm_common.hpp": 1, "wgrad.hip": 2}
    for kernel in ("pw_wgrad_direct_kernel", "pw_wgrad_split_kernel"):          # ... and the two are where they are said to be
        body = texts["wgrad.hip"].split("void %s(const sep_wgrad_desc d) {" % kernel)[1]
        assert "bid & 7" in body[:body.index("__syncthreads()")], kernel
    for helper in ("mfma_chunk32(", "split3_frag(", "mfma_split6("):
        assert [f for f, t in texts.items() if "void " + helper in t] == ["gemm_common.hpp"], helper


def _one_case(sim_library, perturb):
    import sepkernels
    c = dict(GM.cases("default", "host")[1])          # the heads' form on the producer / consumer kernel
    assert c["name"] == "pc<4,1,SEP_PRO_GLN_PRELU,false,SEP_EPI_RESIDUAL>"
    with hostsim.HostSimBackend(sim_library) as K:
        return GM.run_case(K, c, (lambda t: t.clone()), (lambda: None), perturb=perturb)


def test_the_bound_rejects_a_result_off_by_2_to_the_minus_14_of_the_scale(sim_library):
    """numerical control of the checker: a dropped hi*lo cross term is ~2^-11 of the scale; a device result perturbed by 2^-14 of it must
    already fail, the unperturbed one passes (the in-process dispatch is the default environment's)"""
    for k in GM.SWITCHES:
        assert k not in os.environ
    good = _one_case(sim_library, 0.0)
    assert good["ok"] and good["outputs"]["Y"]["err"] <= good["outputs"]["Y"]["bound"] < 2.0 ** -16, good
    bad = _one_case(sim_library, 2.0 ** -14)
    assert not bad["ok"] and bad["outputs"]["Y"]["err"] > bad["outputs"]["Y"]["bound"], bad
    assert bad["kernel"] == good["kernel"] and bad["pads_zero"] and bad["inputs_intact"]


def test_a_gln_prologue_beyond_the_affine_tables_is_refused_or_staged():
    """K = 528 behind a gLN prologue: no family takes it (the packed kernels and the direct kernel hold 512 table rows, the register-staged
    fallback needs K % 32 == 0) and the call is refused with a message, not launched somewhere else; K = 544 runs on the fallback"""
    got = {c["K"]: c["name"] for c in GM.cases("default", "device") if c["regime"] in ("gln528", "gln544") and c["packed"]}
    assert got == {528: "error", 544: "staged"}
