"""CPU: the pruned sweep's speculative round (tests/prune_spec_reference.py, the NumPy restatement of prune_pick4_kernel,
prune_extras_kernel and sweep_pruned's hit / miss branch) on random bounds with random exact values below them:
whether the round hits or misses, the winner (value, lowest index) is the brute-force arg-max, the bar and the survivor count
are those of tests/prune_reference.py, and every candidate whose bound reaches the bar was contracted."""
import math

import numpy as np
import pytest

import prune_reference as pr
import prune_spec_reference as ps


def _case(seed, M, kind):
    """ub (M,) and exact values a <= ub; kind: smooth | ties | inf | flat"""
    rng = np.random.RandomState(seed)
    ub = rng.normal(size=M)
    if kind == "ties":
        ub = np.round(ub * 2) / 2                               # many equal bounds, inside and across groups
    if kind == "flat":
        ub = np.full(M, 0.25)
    slack = rng.exponential(0.3, size=M) * (rng.uniform(size=M) < 0.8)    # a fifth of the bounds are attained
    if kind == "ties":
        slack = np.round(slack * 2) / 2
    a = ub - slack
    if kind == "inf":
        where = rng.choice(M, size=max(1, M // 50), replace=False)
        ub[where] = math.inf                                    # NaN bounds are stored as +inf; their values may be anything
        a[where] = rng.normal(size=len(where))
        a[where[0]] = math.nan
        ub[rng.choice(M, size=3, replace=False)] = -math.inf
        a = np.where(np.isneginf(ub), -math.inf, a)
    return ub, a


def _brute(a):
    vals = np.where(np.isnan(a), -np.inf, a)
    return float(vals.max()), int(np.argmax(vals))


SHAPES = [(4099, 256), (1000, 256), (777, 300), (259, 256), (513, 256), (50, 20), (41, 40), (4099, 4099)]


@pytest.mark.parametrize("kind", ["smooth", "ties", "inf", "flat"])
@pytest.mark.parametrize("M,top", SHAPES)
@pytest.mark.parametrize("cap", [0, 1, 7, 128, 100000])
def test_winner_bar_and_survivors_are_the_two_round_schedules(M, top, cap, kind):
    seen = set()
    for seed in range(3):
        ub, a = _case(1000 * seed + M + cap, M, kind)
        r = ps.spec_argmax(a, ub, top=top, cap=cap)
        bv, bi = _brute(a)
        assert (r["value"], r["index"]) == (bv, bi), (r, bv, bi)
        v0, i0, n0 = pr.pruned_argmax(a, ub, top=top)
        assert (v0, i0, n0) == (r["value"], r["index"], r["survivors"])
        picks = pr.lb_set(ub, top)
        ok = ~np.isnan(a[picks])
        lb = float(a[picks][ok].max()) if ok.any() else -math.inf
        assert r["lb"] == lb
        assert ps.covered(ub, r["lb"], r["contracted"])
        seen.add(r["outcome"])
    if cap == 0:
        assert seen == {ps.NOT_TRIED}


def test_picks_are_the_lb_set_and_groups_shorter_than_four_leave_gaps():
    for M, top in SHAPES:
        for kind in ("smooth", "ties", "inf", "flat"):
            ub, _ = _case(M, M, kind)
            picks, runner = ps.picks_and_runner_ups(ub, top)
            assert np.array_equal(picks, pr.lb_set(ub, top))
            gs = -(-M // top)
            sizes = np.array([min(g + gs, M) - g for g in range(0, M, gs)])
            assert np.array_equal((runner >= 0).sum(1), np.minimum(sizes - 1, 3))
            for g, row in enumerate(runner):
                real = row[row >= 0]
                assert np.all(row[len(real):] == -1)            # the unused places are the last ones
                members = np.arange(g * gs, min((g + 1) * gs, M))
                four = np.concatenate([[picks[g]], real])
                rest = np.setdiff1d(members, four)
                key = lambda i: (-ub[i], i)
                assert [key(i) for i in four] == sorted(key(i) for i in four)
                assert all(key(four[-1]) < key(i) for i in rest) or len(four) < 4


def test_extras_are_the_largest_runner_ups_largest_first():
    ub, _ = _case(5, 4099, "inf")
    _, runner = ps.picks_and_runner_ups(ub, 256)
    real = runner[runner >= 0]
    for cap in (0, 1, 60, 128, 10 ** 6):
        ex = ps.extras(ub, runner, cap)
        assert len(ex) == min(cap, len(real)) and len(set(ex.tolist())) == len(ex)
        keys = [(-ub[i], i) for i in ex]
        assert keys == sorted(keys)
        out = np.setdiff1d(real, ex)
        if len(ex) and len(out):
            worst = max((-ub[i], i) for i in ex)
            assert all(worst < (-ub[i], i) for i in out)
        if len(ex):
            assert np.isinf(ub[real]).any() <= np.isposinf(ub[ex]).any()     # an infinite bound ranks first


def test_both_outcomes_occur_and_a_miss_ignores_the_extras():
    ub = _case(11, 4099, "smooth")[0]
    a = ub - 1.0                                                # no bound is attained: the bar lies a unit below the best pick
    full = ps.spec_argmax(a, ub, cap=100000)
    one = ps.spec_argmax(a, ub, cap=1)
    assert full["survivors"] == one["survivors"] > 1
    assert one["outcome"] == ps.MISS
    picks = pr.lb_set(ub)
    surv = pr.survivors(ub, picks, one["lb"])
    assert np.array_equal(one["contracted"], np.sort(np.concatenate([picks, surv])))
    # a hit needs every survivor among the extras: build bounds whose survivors are their groups' second places
    ub2 = np.full(4099, -5.0)
    ub2[::17] = 1.0                                             # the picks (groups of 17)
    ub2[1::17] = 0.9                                            # the runner-ups reach the bar below
    a2 = ub2 - 0.5
    r = ps.spec_argmax(a2, ub2, cap=100000)
    assert r["outcome"] == ps.HIT and r["survivors"] == len(ub2[1::17]) and (r["value"], r["index"]) == _brute(a2)
    r = ps.spec_argmax(a2, ub2, cap=100000, direct=10)          # more survivors than the screen hands on directly
    assert r["outcome"] == ps.MISS and (r["value"], r["index"]) == _brute(a2)
