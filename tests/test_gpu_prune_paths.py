"""Every branch of the pruned sweep's schedule (turbo_amd/csrc/sweep_pruned.hpp) by the launches it
makes, with the gathered contraction spanning more than one launch pair.

One handle and batch per case (N = 300, M = 4099, the problem of tests/_prune_screen_child.py) in a child process with
TGP_CHUNK=1024 and a slab of one chunk, so a launch pair takes 1024 candidates: G(n) = ceil(n / 1024) pairs for n gathered
rows, 5 for the full schedule.  A profiled segment of kind "cross-kernel" is counted per bound pass and per cross-kernel
launch, one of kind "contraction" per contraction; the screen's launches are a kind of their own and are not counted.

* the winner's index, value bytes and n_clamped are those of the same handle under TGP_SWEEP_PRUNE=0;
* the schedule took the stated branch (state, screen, screen_arith, survivors > 0: no case passes by not pruning);
* kstar_launches and trmm_launches are the branch's formula.
* TGP_PRUNE_MARGIN=1000 (a second child: the margin is read once): the bar is below zero and EI >= 0, so every candidate
  outside the lb set survives, and the survivors' contraction takes G(3857) = 4 launch pairs."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _prune_paths_child as child              # noqa: E402

M, NPICK, FULL = child.M, 242, 5                # TGP_PRUNE_TOP = 256: groups of 17 candidates, 242 of them; 5 pairs of 1024


def G(n):
    return -(-n // 1024)


# name -> (state, screen_arith, cross-kernel launches, contractions) with s = the survivors read back
EXPECT = {
    "tight": (0, 0, lambda s: 1 + G(NPICK) + G(s), lambda s: G(NPICK) + G(s)),
    "direct": (0, 1, lambda s: G(NPICK) + G(s), lambda s: G(NPICK) + G(s)),
    "gathered": (0, 1, lambda s: G(NPICK) + 1 + G(s), lambda s: G(NPICK) + G(s)),
    "tight_all": (1, 1, lambda s: G(NPICK) + 1 + FULL, lambda s: G(NPICK) + FULL),
    "h2": (0, 2, lambda s: G(NPICK) + G(s), lambda s: G(NPICK) + G(s)),
    "fallback": (1, 0, lambda s: 1 + G(NPICK) + FULL, lambda s: G(NPICK) + FULL),
    "many_f32": (0, 1, lambda s: G(NPICK) + 1 + G(s), lambda s: G(NPICK) + G(s)),
    "many_f64": (0, 0, lambda s: 1 + G(NPICK) + G(s), lambda s: G(NPICK) + G(s)),
}


def _child(which):
    e = {k: v for k, v in os.environ.items() if k not in child.SWITCHES}
    out = subprocess.run([sys.executable, os.path.join(HERE, "_prune_paths_child.py"), which], env=e, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "prune-paths ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return {r["case"]: r for r in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{"))}


@pytest.fixture(scope="module")
def paths():
    return _child("paths")


@pytest.fixture(scope="module")
def many():
    return _child("many")


def _check(r):
    print(r)
    state, arith, kstar, trmm = EXPECT[r["case"]]
    p, s = r["p_pruned"], r["p_pruned"]["survivors"]
    assert r["chunk"] == 1024                                   # (and the slab holds one chunk: launch_rows = 1024)
    assert r["pruned"] == r["unpruned"], r
    assert r["p_unpruned"]["state"] == -1 and r["launches_unpruned"] == dict(kstar=FULL, trmm=FULL), r
    assert p["state"] == state and p["screen_arith"] == arith and p["lb_set"] == NPICK and s > 0, p
    assert (p["screen"] > 0) if arith else (p["screen"] == -1), p
    assert r["launches"] == dict(kstar=kstar(s), trmm=trmm(s)), (r["launches"], kstar(s), trmm(s))
    return p


@pytest.mark.parametrize("name", list(child.PATHS))
def test_branch_makes_its_launches_and_keeps_the_winner(paths, name):
    p = _check(paths[name])
    if name in ("direct", "h2"):
        assert p["survivors"] == p["screen"], p                # contracted as they are
    elif name == "gathered":
        assert p["survivors"] <= p["screen"], p                # filtered once more


@pytest.mark.parametrize("name", list(child.MANY))
def test_whole_batch_survives_and_spans_four_launch_pairs(many, name):
    p = _check(many[name])
    assert p["survivors"] == M - NPICK == 3857 and G(p["survivors"]) == 4, p
