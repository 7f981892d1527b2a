"""GPU: every kernel instance behind the streaming entry points of csrc/filterbank.hip, csrc/tcn.hip, csrc/gln.hip, csrc/depthwise.hip,
csrc/cln.hip and csrc/causal.hip, reached BY NAME on the MI355X and compared with a float64 restatement of the call's contract, row by row and sum by sum (tests/stream_matrix.py: the ledger, the
case matrix -- the same cases tests/test_stream_instances_cpu.py runs on the host simulation --, the reference, the metric and the measured
bounds).  The default environment runs in this process, one pytest case per family; each of the four A/B switches, read once per process, gets
one child process that runs the affected families' cases under it: one after another, each under its own time limit; the first child that
exits non-zero ends the run and is reported -- nothing is started behind it and nothing is tried twice."""
import json
import os
import subprocess
import time

import pytest
import torch

import sepkernels
import stream_matrix as SM

pytestmark = pytest.mark.gpu

# seconds per child: 3 x the time the child took on the MI355X, process start, the import of torch and the library load included (3 s, 3 s, 2 s
# and 3 s), rounded up to 20 s.  (Before the first device run the limits were sized from the CPU emulator standing in for the device: the
# references, the emulation and the bookkeeping of an environment take 2.4 s (dwconv_lds, 168 cases), 2.3 s (dwb_no_recompute, 142), 0.7 s
# (cln_three, 150) and 0.1 s (depthwise_generic, 28) on 8 threads, three times that plus 20 s of start-up: 60, 60, 30, 30.)
LIMITS = {"dwconv_lds": 20, "dwb_no_recompute": 20, "cln_three": 20, "depthwise_generic": 20}


@pytest.fixture(scope="module")
def reached():
    """instance names the families' runs reported, filled in by the per-family test below"""
    return {}


def _check(recs, expected):
    assert len(recs) == len(expected)
    assert not SM.failures(recs), "\n".join(SM.failures(recs))
    for rec in recs:
        assert rec["kernel"] == rec["case"]["name"], rec
        assert rec["pads_zero"] and rec["inputs_intact"] and rec["guards_intact"], rec
        for name, o in rec["outputs"].items():
            assert o["err"] <= o["bound"], (rec["kernel"], name, o)


@pytest.mark.parametrize("family", list(SM.FAMILIES))
def test_every_instance_of_the_family_is_reached_on_the_device_and_within_its_bound(reached, family):
    for k in SM.SWITCHES:
        assert k not in os.environ
    recs = SM.run("default", sepkernels.HipBackend(), (lambda t: t.cuda()), torch.cuda.synchronize, families=(family,))
    worst = {}
    for rec in recs:
        worst[rec["kernel"]] = max([worst.get(rec["kernel"], 0.0)] + [o["err"] / o["bound"] for o in rec["outputs"].values()])
    for name in sorted(worst):
        print("reached {:30s} worst err / bound {:.3f}".format(name, worst[name]))
    _check(recs, [c for c in SM.cases("default") if c["family"] == family])
    reached[family] = set(worst)


def test_the_union_over_the_families_is_the_ledger(reached):
    """no instance of the dispatch tables unreached on the device, no name emitted that the ledger does not know (needs the runs above)"""
    assert sorted(reached) == sorted(SM.FAMILIES), "a family's run is missing: {}".format(sorted(set(SM.FAMILIES) - set(reached)))
    union = set().union(*reached.values())
    print("reached:", " ".join(sorted(union)))
    assert sorted(union) == SM.INSTANCES, (sorted(set(SM.INSTANCES) - union), sorted(union - set(SM.INSTANCES)))


def test_under_every_switch_the_cases_reach_the_forced_instance_and_stay_within_the_bound(tmp_path):
    assert sorted(LIMITS) == sorted(e for e in SM.ENVS if e != "default")
    for env in LIMITS:
        out = str(tmp_path / (env + ".json"))
        argv, penv = SM.child_command(env, out)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[env])] + argv, env=penv, capture_output=True, text=True)
        print("environment '{}': {:.0f} s of {} allowed".format(env, time.time() - t0, LIMITS[env]))
        if r.returncode != 0:          # a fault, a time limit or a failed check: report this child, start no other
            pytest.fail("environment '{}' exited with {}:\n{}\n{}".format(env, r.returncode, r.stdout[-8000:], r.stderr[-4000:]))
        recs = json.load(open(out))
        _check(recs, SM.cases(env))
        assert all(rec["case"]["family"] in SM.ENV_FAMILIES[env] for rec in recs)
