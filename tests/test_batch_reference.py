"""CPU: the rank-update restatement of tgp_sweep_batch's greedy loop (tests/batch_reference.py) against LITERAL refits --
oracle.fit on the augmented, pre-normalised data with normalize_y=False and the kernel held, then predict and the
acquisition at every step (include/turbogp.h states the contract; old_library/bayesian_optimiser.py:527-566 the method)."""
import numpy as np
import pytest

from oracle import gp_oracle as o
import batch_reference as br


def _problem(kind, D, N, M, noise, ard, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X.sum(1)) + 0.3 * ((X - 0.4) ** 2).sum(1) + 0.02 * rng.normal(size=N)
    ls = 0.35 * (0.7 + 0.6 * np.arange(D) / max(D - 1, 1)) if ard else 0.4
    return X, y, ls, rng.uniform(0, 1, (M, D)), rng.uniform(0, 1, (3, D))


def _check_against_refits(om, yn, Xc, strategy, lie, Xp, acq, desired, param, inc, q):
    ref = br.select_batch(om, Xc, q, strategy, lie, Xp, acq, desired, param, inc)
    assert not ref["not_pd"]
    P = 0 if Xp is None else len(Xp)
    Zs = [] if Xp is None else list(Xp)
    fant = list(ref["fantasies"][:P])
    best = inc
    for f in fant:
        best = max(best, f) if desired == "max" else min(best, f)
    chosen = []
    for k in range(q):
        mu, sg = br.refit_posterior(om, yn, Zs, fant, Xc)
        a = o.acquisition(acq, mu, sg, desired, param, best)
        a = np.where(np.isnan(a), -np.inf, a)
        a[chosen] = -np.inf
        np.testing.assert_allclose(ref["acq"][k], a, rtol=1e-9, atol=1e-12 * max(1.0, np.abs(a[np.isfinite(a)]).max()))
        i = int(np.argmax(a))
        assert ref["idx"][k] == i, (k, ref["idx"][k], i)
        chosen.append(i)
        if strategy == br.KB:   # the fantasy of a believer: the refit's mean at the chosen row
            np.testing.assert_allclose(ref["fantasies"][P + k], mu[i], rtol=1e-9, atol=1e-12)
        else:
            assert ref["fantasies"][P + k] == lie
        Zs.append(Xc[i])
        fant.append(ref["fantasies"][P + k])
        best = max(best, fant[-1]) if desired == "max" else min(best, fant[-1])
    mu, sg = br.refit_posterior(om, yn, Zs, fant, Xc)
    np.testing.assert_allclose(ref["mu"], mu, rtol=1e-9, atol=1e-12 * om.y_std)
    # (variances: near a conditioned point of a noise-free model sigma is of the order of sqrt(jitter) and only the
    # cancellation-bounded absolute error of the variance is meaningful, as in tests/test_gpu_parity.py)
    np.testing.assert_allclose(ref["sigma"] ** 2, sg ** 2, rtol=1e-9, atol=1e-13 * (om.constant + om.noise) * om.y_std ** 2)
    assert len(set(ref["idx"].tolist())) == q
    return ref


# every acquisition in both directions, each with a lie: "opp" = the opposite extreme of y, the mean, or "below" = a float
# under every observation; ("ucb", inf) is TGP_ACQ_SIGMA (UCB(beta=inf), acquisition_functions.py)
ACQ_ROWS = (("ei", "min", 0.01, "opp"), ("pi", "max", 0.0, "opp"), ("ucb", "max", 2.0, "opp"),
            ("ei", "max", 0.01, "mean"), ("pi", "min", 0.0, "below"), ("ucb", "min", 2.0, "mean"),
            ("ucb", "max", np.inf, "below"))


# (kind, ard) -> (constant, normalize_y)
SETTINGS = {("rbf", True): (1.2, True), ("matern52", True): (1.2, True), ("rbf", False): (1.2, True),
            ("matern12", True): (0.3, True), ("matern32", False): (4.0, True), ("matern12", False): (4.0, False),
            ("matern32", True): (0.3, False)}


@pytest.mark.parametrize("kind,ard", list(SETTINGS))
@pytest.mark.parametrize("noise", [1e-3, 0.0])
@pytest.mark.parametrize("strategy", [br.KB, br.CL])
@pytest.mark.parametrize("pending", [False, True])
def test_rank_updates_equal_literal_refits(kind, ard, noise, strategy, pending):
    constant, normalize_y = SETTINGS[(kind, ard)]
    X, y, ls, Xc, Xp = _problem(kind, 3, 25, 400, noise, ard, 3)
    jitter = 1e-10 if noise > 0 else 1e-8
    om = o.fit(X, y, kind, constant, ls, noise, jitter, normalize_y)
    yn = (y - om.y_mean) / om.y_std
    for acq, desired, param, lie in ACQ_ROWS:
        inc = float(y.min() if desired == "min" else y.max())
        lie = br.resolve_lie({"opp": "max" if desired == "min" else "min", "below": float(y.min()) - 1.0}.get(lie, lie), y)
        _check_against_refits(om, yn, Xc, strategy, lie, Xp if pending else None, acq, desired, param, inc, 5)


@pytest.mark.parametrize("strategy", [br.KB, br.CL])
def test_sixty_four_conditioned_points_equal_literal_refits(strategy):
    """P + q = 64 (BT_MAXP): 40 pending points, then 24 selections -- 64 refits of the augmented data"""
    rng = np.random.RandomState(21)
    X, y, ls, Xc, _ = _problem("matern52", 3, 25, 400, 1e-3, True, 4)
    Xp = rng.uniform(0, 1, (40, 3))
    om = o.fit(X, y, "matern52", 1.2, ls, 1e-3, 1e-10, True)
    yn = (y - om.y_mean) / om.y_std
    ref = _check_against_refits(om, yn, Xc, strategy, float(np.mean(y)), Xp, "ei", "min", 0.01, float(y.min()), 24)
    assert len(ref["fantasies"]) == 64


def test_duplicate_rows_lowest_index_first_and_the_duplicate_is_not_next():
    """ties: every candidate row twice (row i + 20 duplicates row i) gives identical values; the lower index is taken
    first, and once a row is conditioned on, its duplicate's sigma falls to the noise level, so SIGMA does not take it
    next"""
    X, y, ls, C, _ = _problem("rbf", 2, 15, 20, 1e-3, False, 5)
    Xc = np.vstack([C, C])
    om = o.fit(X, y, "rbf", 1.0, ls, 1e-3, 1e-10, True)
    yn = (y - om.y_mean) / om.y_std
    for acq, desired, param in (("ucb", "max", np.inf), ("ei", "min", 0.01), ("ucb", "max", 2.0)):
        ref = br.select_batch(om, Xc, 6, br.KB, 0.0, None, acq, desired, param, float(y.min()))
        a0 = ref["acq"][0]
        assert a0[:20].tobytes() == a0[20:].tobytes()
        assert ref["idx"][0] < 20
        assert all(i < 20 or i - 20 in ref["idx"][:k] for k, i in enumerate(ref["idx"])), ref["idx"]
        if np.isinf(param):
            dup = ref["idx"][0] + 20
            assert ref["idx"][1] != dup
            assert ref["acq"][1][dup] < 2 * np.sqrt(om.noise + om.jitter) * om.y_std
        _check_against_refits(om, yn, Xc, br.KB, 0.0, None, acq, desired, param, float(y.min()), 6)


def test_lies_masking_and_the_incumbent_rule():
    X, y, ls, Xc, Xp = _problem("rbf", 2, 15, 300, 1e-3, False, 9)
    assert br.resolve_lie("min", y) == y.min() and br.resolve_lie("max", y) == y.max()
    assert br.resolve_lie("mean", y) == pytest.approx(y.mean()) and br.resolve_lie(0.25, y) == 0.25
    om = o.fit(X, y, "rbf", 1.0, ls, 1e-3, 1e-10, True)
    # a lie far below every observation, minimising with EI: after the first fantasy the incumbent IS the lie
    lie = float(y.min()) - 5.0
    ref = br.select_batch(om, Xc, 4, br.CL, lie, None, "ei", "min", 0.0, float(y.min()))
    yn = (y - om.y_mean) / om.y_std
    mu, sg = br.refit_posterior(om, yn, [Xc[ref["idx"][0]]], [lie], Xc)
    a = o.acquisition("ei", mu, sg, "min", 0.0, lie)
    a[ref["idx"][0]] = -np.inf
    np.testing.assert_allclose(ref["acq"][1], a, rtol=1e-9, atol=1e-14)
    # with the real incumbent the second step would rank differently
    a_old = o.acquisition("ei", mu, sg, "min", 0.0, float(y.min()))
    assert not np.allclose(a_old[np.isfinite(a)], a[np.isfinite(a)])
    # masking: a constant liar at the believer's value of a row whose variance barely moves never picks a row twice
    ref = br.select_batch(om, Xc[:5], 5, br.CL, float(y.max()), None, "ucb", "max", 2.0, 0.0)
    assert sorted(ref["idx"].tolist()) == [0, 1, 2, 3, 4]
    assert all(np.isneginf(ref["acq"][k][ref["idx"][:k]]).all() for k in range(5))
