"""CPU: every kernel instance behind the streaming entry points of csrc/filterbank.hip, csrc/tcn.hip, csrc/gln.hip, csrc/depthwise.hip,
csrc/cln.hip and csrc/causal.hip, reached BY NAME on the host simulation of the kernel sources and compared with a float64 restatement of
the call's contract, row by row and sum by sum (tests/stream_matrix.py: the ledger, the case matrix, the reference, the metric and the
measured bounds).  The default environment runs in this process, family by family; each A/B switch in a child process -- the dispatchers
read their SEPK_* switches once per process."""
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
import stream_matrix as SM             # noqa: E402

pytestmark = pytest.mark.skipif(hostsim.compiler() is None, reason="needs clang++ (ext_vector_type)")
CSRC = os.path.join(ROOT, "dnn-based_source_separation_amd", "csrc")
HOST = ((lambda t: t.clone()), (lambda: None))


@pytest.fixture(scope="module")
def sim_library(tmp_path_factory):
    return hostsim.build(str(tmp_path_factory.mktemp("hostsim_stream")))


@pytest.fixture(scope="module")
def reached():
    """instance names the families' runs reported, filled in by the per-family test below"""
    return {}


def _check(recs, expected):
    assert len(recs) == len(expected)
    assert not SM.failures(recs), "\n".join(SM.failures(recs))
    for rec in recs:
        assert rec["kernel"] == rec["case"]["name"], rec                 # the case reached the instance it names
        assert rec["pads_zero"] and rec["inputs_intact"] and rec["guards_intact"], rec
        for name, o in rec["outputs"].items():
            assert o["err"] <= o["bound"], (rec["kernel"], name, o)


@pytest.mark.parametrize("family", list(SM.FAMILIES))
def test_every_instance_of_the_family_is_reached_and_within_its_bound(sim_library, reached, family):
    for k in SM.SWITCHES:
        assert k not in os.environ
    with hostsim.HostSimBackend(sim_library) as K:
        recs = SM.run("default", K, *HOST, families=(family,))
    _check(recs, [c for c in SM.cases("default") if c["family"] == family])
    reached[family] = set(rec["kernel"] for rec in recs)


def test_the_union_over_the_families_is_the_ledger(reached):
    """no instance of the dispatch tables unreached, no name emitted that the ledger does not know (needs the per-family runs above)"""
    assert sorted(reached) == sorted(SM.FAMILIES), "a family's run is missing: {}".format(sorted(set(SM.FAMILIES) - set(reached)))
    union = set().union(*reached.values())
    assert sorted(union) == SM.INSTANCES, (sorted(set(SM.INSTANCES) - union), sorted(union - set(SM.INSTANCES)))


@pytest.mark.parametrize("env", [e for e in SM.ENVS if e != "default"])
def test_under_a_switch_every_case_reaches_the_forced_instance(sim_library, tmp_path, env):
    out = str(tmp_path / "records.json")
    argv, penv = SM.child_command(env, out, backend="hostsim:" + sim_library)
    r = subprocess.run(argv, env=penv, capture_output=True, text=True, timeout=3600)
    assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
    recs = json.load(open(out))
    _check(recs, SM.cases(env))
    forced = {"dwconv_lds": {"dwconv_fwd_tiles", "dwconv_bwd_tiles"}, "cln_three": {"cln_three_fwd", "cln_three_stats", "cln_three_bwd"},
              "depthwise_generic": {"depthwise_fwd", "depthwise_bwd_input", "depthwise_bwd_weight"},
              "dwb_no_recompute": {n for n in SM.INSTANCES if n.startswith("dwconv_bwd") and not n.endswith(",true>")}}[env]
    assert set(rec["kernel"] for rec in recs) == forced


def test_the_ledger_lists_every_launch_line_of_the_dispatchers():
    """INSTANCES against the sources: every sep_set_kernel statement of the six files, a statement inside a launch macro counted once per use
    of the macro, contributes the string literals it chooses between"""
    def names(fname, macros):
        src = open(os.path.join(CSRC, fname)).read()
        stmts = re.findall(r"sep_set_kernel\(([^;]*)\);", src)
        plain = sum(len(re.findall(r'"[^"]*"', s)) for s in stmts if "#" not in s and "NAME" not in s)
        in_macros = [s for s in stmts if "#" in s or "NAME" in s]
        assert len(in_macros) == len(macros), (fname, in_macros)
        uses = sum(per_use * (len(re.findall(r"\b" + m + r"\(", src)) - 1) for m, per_use in macros.items())      # (- 1: the #define itself)
        return plain, uses
    stream = {"filterbank.hip": names("filterbank.hip", {"SEP_DEB": 2}), "tcn.hip": names("tcn.hip", {"SEP_DWF": 2, "SEP_DWB2": 2}),
              "gln.hip": names("gln.hip", {}), "depthwise.hip": names("depthwise.hip", {})}
    assert stream == {"filterbank.hip": (7, 3 * 2), "tcn.hip": (4, 3 * 2 + 8 * 2), "gln.hip": (4, 0), "depthwise.hip": (8, 0)}
    assert tuple(sum(v[i] for v in stream.values()) for i in (0, 1)) == (23, 3 * 2 + 8 * 2 + 3 * 2)      # the four together: as many as the one file they were cut from
    assert names("cln.hip", {"SEP_CLF": 1, "SEP_CLS": 1, "SEP_CLB": 1}) == (3, 12)
    assert names("causal.hip", {"SEP_CDF": 1, "SEP_CDW": 1}) == (0, 8)
    assert len(SM.INSTANCES) == len(set(SM.INSTANCES)) == 23 + 28 + 3 + 12 + 8
    for f in tuple(stream) + ("cln.hip", "causal.hip"):                # and every literal name in the sources is one of the ledger's
        for lit in re.findall(r'"([^"]*)"', " ".join(s for s in re.findall(r"sep_set_kernel\(([^;]*)\);", open(os.path.join(CSRC, f)).read()) if "#" not in s and "NAME" not in s)):
            assert lit in SM.INSTANCES, lit


def test_every_case_names_an_instance_and_the_sign_guard_finds_a_seed():
    """cases() itself refuses a matrix that misses an instance or a sign-sensitive case without a seed; here: every environment builds, every
    recompute case kept clear of zero, and the forward's accepted maxima are in"""
    for env in SM.ENVS:
        cs = SM.cases(env)
        assert cs and all(c["name"] in SM.INSTANCES for c in cs)
    counts = {f: sum(c["family"] == f for c in SM.cases("default")) for f in SM.FAMILIES}          # the matrix as it was agreed: no case dropped quietly
    assert counts == {"encoder": 25, "dwconv_fwd": 26, "dwconv_bwd": 142, "decoder_fwd": 40, "decoder_bwd": 48, "depthwise": 28, "split_rows": 4, "gln_tokens": 8,
                      "cln": 150, "causal": 16}
    assert {e: len(SM.cases(e)) for e in SM.ENVS} == {"default": 487, "dwconv_lds": 168, "dwb_no_recompute": 142, "cln_three": 150, "depthwise_generic": 28}
    guarded = [c for c in SM.cases("default") if c["name"].endswith(",true>")]
    assert len(guarded) >= 3 * 20
    for c in guarded[::7]:
        assert SM.sign_margin(c, SM.prepare(c, c["seed"])[1]) >= 1.0
    assert {(c["d"], c["name"]) for c in SM.cases("default") if c["op"] == "dwconv_fwd" and c["d"] >= 4095} == {(4096, "dwconv_fwd_direct<0,2>"), (4095, "dwconv_fwd_tiles")}


def test_the_bounds_in_the_ledger_follow_from_the_emulator():
    """FAMILIES: e32 is (an upper bound of) the fp32 emulator's worst figure against the float64 reference, the bound follows by the rule"""
    worst = SM.emulator_figures()
    for f, entry in SM.FAMILIES.items():
        assert worst[f] <= entry["e32"], (f, worst[f], entry)
        assert entry["e32"] <= 1.5 * worst[f], (f, worst[f], entry)      # ... and not padded
        assert entry["bound"] == SM.bound_rule(entry["e32"]) <= 2e-4, (f, entry)


# ------------------------------------------------------------------------------------------------- controls of the checker
def _control_case(op, name, **kw):
    return [c for c in SM.cases("default") if c["op"] == op and c["name"] == name and all(c[k] == v for k, v in kw.items())][0]


CONTROLS = {   # case -> the elementwise output the controls alter
    "dwconv_bwd": (lambda: _control_case("dwconv_bwd", "dwconv_bwd_row<3,4,true>", mode="sums"), "dv1"),
    "decoder_bwd": (lambda: _control_case("decoder_bwd", "decoder_bwd<16,2>/nz1", raw_mask=0, F=300), "dwm"),
    "cln_fwd": (lambda: _control_case("cln_fwd", "cln_chain_fwd<1,true>", T=203, B=3, alpha=0), "y"),
}


def _rows_of(desc, t):
    return t.reshape(-1, desc["ref"].shape[-1])


def _tamper(kind, out):
    def fn(got, args, ref):
        desc = ref[out]
        bound = SM.FAMILIES[fn.family]["bound"]
        g, r = _rows_of(desc, got[out]), _rows_of(desc, desc["ref"])
        V = desc["valid"]
        peak = r[:, :V].abs().amax(1)
        quiet = int(torch.where(peak > 0, peak, torch.full_like(peak, float("inf"))).argmin())
        fn.quiet_over_loud = float(peak[quiet] / peak.max())
        if kind == "element":                      # one element of one row moved by 8 x its bound
            g[1, V // 2] += 8 * bound * float(peak[1])
        elif kind == "quiet_row":                  # the quietest row scaled by 1 + 2^-10
            g[quiet, :V] *= 1 + 2.0 ** -10
        elif kind == "ends":
            if "_taps" in ref:                     # the d frames at either end of the quietest row, the tap that reaches d frames into the row dropped
                d, (plus, minus) = fn.d, ref["_taps"]
                p, m = plus.reshape(-1, plus.shape[-1])[quiet], minus.reshape(-1, minus.shape[-1])[quiet]
                g[quiet, :d] -= p[:d].float()
                g[quiet, V - d:V] -= m[V - d:V].float()
            else:                                  # no dilated tap in this kernel: the frame index off by one at either end of the quietest row
                g[quiet, 0], g[quiet, V - 1] = g[quiet, 1].clone(), g[quiet, V - 2].clone()
        fn.global_max = SM.global_max_metric(desc, got[out])
    return fn


@pytest.mark.parametrize("which", list(CONTROLS))
def test_the_checker_rejects_what_the_global_maximum_metric_lets_through(sim_library, which):
    """the unperturbed result passes; it fails with one element moved by 8 x its bound, with the quietest row scaled by 1 + 2^-10, and with the
    frames at either end of the quietest row wrong (depthwise backward: the d frames at either end recomputed with the tap that reaches d frames
    into the row dropped -- a halo error; decoder and cLN have no dilated tap: their first and last frame take the neighbouring frame's value).
    The last two stay below 2e-4 of the output's GLOBAL maximum, the figure both() of tests/test_gpu_kernels.py looks at: both() would have let
    the scaled quiet row through in all three cases, and the wrong end frames in the depthwise and the decoder case (in the cLN case the rows of
    y are all of the size of gamma and beta, and the end frames stand out globally too)."""
    make, out = CONTROLS[which]
    c = make()
    with hostsim.HostSimBackend(sim_library) as K:
        good = SM.run_case(K, c, *HOST)
        assert good["ok"] and good["outputs"][out]["err"] <= good["outputs"][out]["bound"], good
        seen = {}
        for kind in ("element", "quiet_row", "ends"):
            t = _tamper(kind, out)
            t.family, t.d = c["family"], c.get("d", 1)
            bad = SM.run_case(K, c, *HOST, tamper=t)
            assert not bad["ok"] and bad["outputs"][out]["err"] > bad["outputs"][out]["bound"], (kind, bad)
            assert bad["kernel"] == good["kernel"] and bad["pads_zero"] and bad["inputs_intact"] and bad["guards_intact"]
            assert all(o["err"] <= o["bound"] for n, o in bad["outputs"].items() if n != out)
            seen[kind] = t.global_max
    assert seen["quiet_row"] <= 2e-4, seen                     # what both() grants: it would have passed
    if which != "cln_fwd":
        assert seen["ends"] <= 2e-4, seen
