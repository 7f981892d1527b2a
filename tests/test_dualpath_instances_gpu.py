"""GPU: every kernel instance behind the entry points of the dual-path separators -- csrc/linear.hip, csrc/lstm.hip, csrc/attn.hip and
csrc/rownorm.hip --, reached BY NAME on the MI355X and compared with the float64 run of the call's contract, token row by token row, slab by slab
and sequence by sequence (tests/dualpath_matrix.py: the ledger, the case matrix -- the cases tests/test_dualpath_instances_cpu.py runs on the host
simulation, plus the two that are too large for it --, the reference, the metric and the measured bounds).  The default environment runs in this
process, one pytest case per family; each value of SEPK_LSTM_NS4, read once per process, gets one child process that runs the unforced LSTM cases
under it: one after the other, each under its own time limit; the first child that exits non-zero ends the run and is reported -- nothing is
started behind it and nothing is tried twice."""
import json
import os
import subprocess
import time

import pytest
import torch

import sepkernels
import dualpath_matrix as DM

pytestmark = pytest.mark.gpu

# seconds per child: 3 x the time the child took on the MI355X, process start, the import of torch and the library load included (2 s and 2 s),
# rounded up to 10 s and never below 20 s.  (Before the first device run the limits were sized from the contract's float32 run standing in for the
# device: the references, that run and the bookkeeping of either environment (14 cases) take 3.2 s on 8 threads, three times that plus 20 s of
# start-up: 30 and 30.)
LIMITS = {"lstm_ns4_0": 20, "lstm_ns4_1": 20}


@pytest.fixture(scope="module")
def reached():
    """instance names the families' runs reported, filled in by the per-family test below"""
    return {}


def _check(recs, expected):
    assert len(recs) == len(expected)
    assert not DM.failures(recs), "\n".join(DM.failures(recs))
    for rec in recs:
        assert rec["kernel"] == rec["case"]["name"] and rec["kernel"] in DM.INSTANCES, rec
        assert rec["inputs_intact"] and rec["guards_intact"], rec
        for name, o in rec["outputs"].items():
            assert o["err"] <= o["bound"], (rec["kernel"], name, o)


@pytest.mark.parametrize("family", list(DM.FAMILIES))
def test_every_instance_of_the_family_is_reached_on_the_device_and_within_its_bound(reached, family):
    for k in DM.SWITCHES:
        assert k not in os.environ
    recs = DM.run("default", sepkernels.HipBackend(), (lambda t: t.cuda()), torch.cuda.synchronize, families=(family,))
    for name, e in sorted(DM.by_instance(recs).items()):
        print("reached {:28s} worst err / bound {:.3f}".format(name, e["worst_err_over_bound"]))
    _check(recs, [c for c in DM.cases("default") if c["family"] == family])
    reached[family] = set(rec["kernel"] for rec in recs)


def test_the_union_over_the_families_is_the_ledger(reached):
    """no instance of the dispatch tables unreached on the device, no name emitted that the ledger does not know (needs the runs above)"""
    assert sorted(reached) == sorted(DM.FAMILIES), "a family's run is missing: {}".format(sorted(set(DM.FAMILIES) - set(reached)))
    union = set().union(*reached.values())
    print("reached:", " ".join(sorted(union)))
    assert sorted(union) == DM.INSTANCES, (sorted(set(DM.INSTANCES) - union), sorted(union - set(DM.INSTANCES)))


def test_under_either_value_of_the_switch_the_unforced_cases_reach_the_forced_sweep_and_stay_within_the_bound(tmp_path):
    assert sorted(LIMITS) == sorted(e for e in DM.ENVS if e != "default")
    for env in LIMITS:
        out = str(tmp_path / (env + ".json"))
        argv, penv = DM.child_command(env, out)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[env])] + argv, env=penv, capture_output=True, text=True)
        print("environment '{}': {:.0f} s of {} allowed".format(env, time.time() - t0, LIMITS[env]))
        if r.returncode != 0:          # a fault, a time limit or a failed check: report this child, start no other
            pytest.fail("environment '{}' exited with {}:\n{}\n{}".format(env, r.returncode, r.stdout[-8000:], r.stderr[-4000:]))
        recs = json.load(open(out))
        _check(recs, DM.cases(env))
        assert all(rec["kernel"].startswith(("lstm_fwd4<", "lstm_bwd4<")) == (env == "lstm_ns4_1") for rec in recs)
