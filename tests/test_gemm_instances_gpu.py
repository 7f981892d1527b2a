"""GPU: every kernel instance sep_pw_gemm can launch, reached BY NAME on the MI355X at its smallest shape, a ragged one, one without pad
frames, the family's edges and -- for the instances of the paper-best step -- their real (M, K) at B = 16, T = 3999, and compared with a
float64 restatement of the call's contract in the error model's own metric (tests/gemm_matrix.py).  One child process per environment
(the dispatchers read their SEPK_* switches once per process), one after another, each under its own time limit; the first child that
exits non-zero ends the run and is reported -- nothing is started behind it and nothing is tried twice."""
import json
import subprocess
import time

import pytest

import gemm_matrix as GM

pytestmark = pytest.mark.gpu

# seconds per child.  No device run has been timed yet: with the CPU emulator standing in for the device the references, the emulation and
# the bookkeeping of an environment take 40 s (default, coop: the paper-best shapes at B = 16) or under 5 s (the others) on 8 threads; three
# times that plus process start and library load, rounded up.  To be re-sized from the first device run the same way (3 x measured).
LIMITS = {"default": 300, "pc": 120, "coop": 300, "coop_mi1": 120, "coop_mi4": 120, "pc_22": 120, "no_coop": 120, "staged": 120, "coop_ns3": 120}

def test_every_instance_is_reached_on_the_device_and_within_its_bound(tmp_path):
    assert sorted(LIMITS) == sorted(GM.ENVS)
    reached = set()
    for env in GM.ENVS:
        out = str(tmp_path / (env + ".json"))
        argv, penv = GM.child_command(env, "device", out)
        t0 = time.time()
        r = subprocess.run(["timeout", "-k", "10", str(LIMITS[env])] + argv, env=penv, capture_output=True, text=True)
        print("environment '{}': {:.0f} s of {} allowed".format(env, time.time() - t0, LIMITS[env]))
        if r.returncode != 0:          # a fault, a time limit or a failed check: report this child, start no other
            pytest.fail("environment '{}' exited with {}:\n{}\n{}".format(env, r.returncode, r.stdout[-8000:], r.stderr[-4000:]))
        recs = json.load(open(out))
        assert len(recs) == len(GM.cases(env, "device"))
        assert not GM.failures(recs)
        for rec in recs:
            assert rec["kernel"] == rec["case"]["name"], rec
            assert rec["kernel"] == "error" or (rec["pads_zero"] and rec["inputs_intact"] and rec["guards_intact"]), rec
            for name, o in rec["outputs"].items():
                assert o["err"] <= o["bound"], (rec["kernel"], name, o)
        names = set(rec["kernel"] for rec in recs) - {"error"}
        assert names >= set(GM.ENV_INSTANCES[env]), sorted(set(GM.ENV_INSTANCES[env]) - names)
        reached |= names
    assert sorted(reached) == GM.INSTANCES, (sorted(set(GM.INSTANCES) - reached), sorted(reached - set(GM.INSTANCES)))

