"""The pruned sweep's speculative round (turbo_amd/csrc/sweep_pruned.hpp, TGP_PRUNE_SPEC): the lb set's
exact round also contracts the largest runner-ups of its groups, and when they cover every survivor the sweep ends there.

One handle and batch per configuration (N = 300, M = 4099, the problem of tests/_prune_screen_child.py) in child processes
with TGP_PRUNE_MIN_WORK=0, TGP_PRUNE_FRAC=1 and TGP_PRUNE_DIRECT=100000 (every survivor set is contracted as it is):
the fp16 screen (f32 RBF, D = 16, ARD), the f32 screen (f32 RBF, D = 5) and the tight bound pass alone (f64 Matern-5/2),
each with EI, PI and UCB and both senses.  TGP_PRUNE_TOP = 256 gives 242 picks and 724 runner-ups.

* always speculating (TGP_PRUNE_SPEC=2), the winner's index, value bytes and n_clamped are those of TGP_PRUNE_SPEC=0 and of
  TGP_SWEEP_PRUNE=0 on the same handle, and last_prune() reads as under TGP_PRUNE_SPEC=0;
* the profile counts one cross-kernel and one contraction segment per launch pair of the one round on a hit; a miss adds
  the survivors' round (tests/test_gpu_prune_paths.py's formula);
* which case gives which outcome (seen on an MI355X when the test was written): every case of the grid hits, with 128
  extras and with TGP_PRUNE_SPEC_CAP=1 alike -- EI / "max" (all three configurations) and PI / "max" (fp16 screen) with
  ONE survivor, which is the largest runner-up of all, the other cases with none or one.  One extra cannot cover two survivors,
  but this problem has no such case, so the misses come from a second child with TGP_PRUNE_MARGIN=1000 (read once per
  process): all 3857 candidates outside the lb set survive and 128 extras cannot cover them -- every case there misses;
* launch pairs of 1024 rows and TGP_PRUNE_TOP=512 (456 picks + 1000 extras): the one round spans two launch pairs;
* TGP_PRUNE_SPEC=1: a handle's first sweep and the sweep after one without survivors do not speculate, the sweep after one
  with 1 .. cap survivors does, and the record's bytes are the same every time;
* with a winner record attached (tgp_set_winner_out) it holds the final arg-max's winner on a hit and on a miss."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _prune_spec_child as child              # noqa: E402

NOT_TRIED, HIT, MISS = 0, 1, 2


def _child(which):
    e = {k: v for k, v in os.environ.items() if k not in child.SWITCHES}
    out = subprocess.run([sys.executable, os.path.join(HERE, "_prune_spec_child.py"), which], env=e, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "prune-spec ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


@pytest.fixture(scope="module")
def grid():
    return _child("grid")


@pytest.fixture(scope="module")
def miss():
    return _child("miss")


def _picks_and_extras(M, top, cap):
    gs = -(-M // top)
    npick = -(-M // gs)
    last = M - (npick - 1) * gs
    return npick, min(cap, (npick - 1) * min(3, gs - 1) + min(3, last - 1))


def _check(r, top=256, rows_per_pair=None):
    """one sweep three ways: same record, same last_prune(), the launches of its outcome"""
    print(r["case"], r["spec2"]["spec"], r["spec2"]["prune"], r["spec2"]["launches"])
    name, cap = r["case"][0], r["case"][3]
    s2, s0, off = r["spec2"], r["spec0"], r["unpruned"]
    assert s2["rec"] == s0["rec"] == off["rec"], r
    assert s2["prune"] == s0["prune"] and s0["prune"]["state"] == 0 and off["prune"]["state"] == -1, r
    assert s0["spec"] == NOT_TRIED and off["spec"] == NOT_TRIED and s2["spec"] in (HIT, MISS), r
    G = (lambda n: -(-n // rows_per_pair)) if rows_per_pair else (lambda n: 1 if n else 0)
    npick, nx = _picks_and_extras(child.M, top, cap)
    assert s0["prune"]["lb_set"] == npick
    s = s0["prune"]["survivors"]
    bound = 1 if name == "f64" else 0                          # the tight bound pass is a cross-kernel launch; the screens are not
    assert s0["launches"] == dict(kstar=bound + G(npick) + G(s), trmm=G(npick) + G(s)), r
    rest = G(s) if s2["spec"] == MISS else 0
    assert s2["launches"] == dict(kstar=bound + G(npick + nx) + rest, trmm=G(npick + nx) + rest), r
    if s2["spec"] == HIT:
        assert s <= nx
    return s2["spec"], s


def test_same_winner_and_counters_and_the_launches_of_the_outcome(grid):
    cases = [r for r in grid if r["case"][0] != "winner"]
    assert len(cases) == 3 * (3 * 2 + 3)
    seen = [(_check(r), r["case"]) for r in cases]
    assert {c[0] for _, c in seen} == set(child.CONFIGS)
    assert any(o == HIT and s > 0 for (o, s), _ in seen), seen          # a hit that is not the trivial one
    for (o, s), c in seen:
        if c[3] == 1 and s >= 2:
            assert o == MISS, (c, o, s)                                 # one extra cannot cover two survivors
        if s == 0:
            assert o == HIT, (c, o, s)


def test_every_candidate_survives_and_the_round_misses(miss):
    cases = [r for r in miss if r["case"][0] != "winner"]
    assert len(cases) == 3 * 2
    for r in cases:
        assert _check(r) == (MISS, child.M - 242), r


def test_winner_record_on_the_device_is_the_final_argmaxs(grid, miss):
    cases = [r for r in grid + miss if r["case"][0] == "winner"]
    assert len(cases) == 6
    outcomes = set()
    for r in cases:
        s2, off = r["spec2"], r["unpruned"]
        outcomes.add(s2["spec"])
        assert s2["rec"] == off["rec"], r
        for x in (s2, off):
            assert x["winner"] == dict(val=x["rec"]["best_val"], idx=float(7000 + x["rec"]["best_idx"]), row_ok=True), r
    assert outcomes == {HIT, MISS}, cases


def test_one_round_across_two_launch_pairs():
    cases = _child("pairs")
    assert len(cases) == 3
    for r in cases:
        assert r["chunk"] == 1024
        npick, nx = _picks_and_extras(child.M, 512, 1000)
        assert (npick, nx) == (456, 1000) and -(-(npick + nx) // 1024) == 2
        _check(r, top=512, rows_per_pair=1024)


def test_default_trigger_follows_the_previous_pruned_sweep():
    cases = _child("trigger")
    assert len(cases) == 3
    for r in cases:
        seq, cap = r["seq"], r["cap"]
        print(r["case"], [(x["spec"], x["prune"]) for x in seq])
        first = lambda x: x["prune"]["screen"] if x["prune"]["screen"] >= 0 else x["prune"]["survivors"]
        assert seq[0]["spec"] == NOT_TRIED                                  # a handle's first pruned sweep
        assert 1 <= first(seq[0]) <= cap and first(seq[3]) == 0, r          # (the two situations the case is built on)
        for prev, x in zip(seq, seq[1:]):
            tried = prev["prune"]["state"] == 0 and 1 <= first(prev) <= cap
            assert (x["spec"] != NOT_TRIED) == tried, (prev, x)
        assert seq[1]["spec"] in (HIT, MISS) and seq[4]["spec"] == NOT_TRIED and seq[5]["spec"] in (HIT, MISS)
        for x in (seq[1], seq[2], seq[4], seq[5]):
            assert x["rec"] == seq[0]["rec"] == r["unpruned"]["rec"]         # the history chooses a schedule, never a result
            assert x["prune"] == seq[0]["prune"]
