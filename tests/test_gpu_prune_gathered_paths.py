"""The pruned sweep with its gathered sets' cross-kernel split over the whole chip (csrc/sweep_pruned.hpp contract_rows:
up to Np / 128 splits of the training points instead of the plan's 8), through the library: winner
value, index and n_clamped are the unpruned sweep's and the same on a second run, with last_prune() unchanged, on small
problems where candidates outside the lb set survive -- some tens under the bounds as they are, all of them under
TGP_PRUNE_MARGIN=1000 (f32 RBF at N x D, one Matern-5/2 f32 and one f64 handle: the cross-kernel's split serves every dtype
and kernel family)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _prune_gathered_child as child          # noqa: E402


def _child(which):
    e = {k: v for k, v in os.environ.items() if k not in child.SWITCHES}
    out = subprocess.run([sys.executable, os.path.join(HERE, "_prune_gathered_child.py"), which], env=e, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "prune-gathered ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return {tuple(r["case"]): r for r in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{"))}


@pytest.fixture(scope="module")
def few():
    return _child("few")


@pytest.fixture(scope="module")
def many():
    return _child("many")


def same_winner_and_schedule(r):
    assert r["pruned"] == r["again"] == r["unpruned"], r
    assert r["p_pruned"] == r["p_again"], r
    assert r["p_pruned"]["state"] == 0 and r["p_pruned"]["lb_set"] == 16, r["p_pruned"]
    assert r["p_unpruned"]["state"] == -1, r["p_unpruned"]


CASE_IDS = ["-".join(str(x) for x in c) for c in child.CASES]


@pytest.mark.parametrize("case", child.CASES, ids=CASE_IDS)
def test_winner_is_the_unpruned_sweeps(few, case):
    r = few[tuple(case)]
    print(r)
    same_winner_and_schedule(r)
    # an lb set of 16 out of 4096: at N = 300, D = 8 its best value leaves some tens of the other candidates' bounds above
    # the bar (tests/test_gpu_prune_paths.py found the same at N = 300, D = 5); the larger shapes' bounds separate fully
    if case[2] == 300 and case[3] == 8:
        assert r["p_pruned"]["survivors"] > 0, r["p_pruned"]


@pytest.mark.parametrize("case", child.CASES, ids=CASE_IDS)
def test_every_candidate_outside_the_lb_set_contracted(many, case):
    r = many[tuple(case)]
    print(r)
    same_winner_and_schedule(r)
    assert r["p_pruned"]["survivors"] == child.M - 16, r["p_pruned"]
