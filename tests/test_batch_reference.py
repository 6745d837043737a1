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


@pytest.mark.parametrize("kind,ard", [("rbf", True), ("matern52", True), ("rbf", False)])
@pytest.mark.parametrize("noise", [1e-3, 0.0])
@pytest.mark.parametrize("strategy", [br.KB, br.CL])
@pytest.mark.parametrize("pending", [False, True])
def test_rank_updates_equal_literal_refits(kind, ard, noise, strategy, pending):
    X, y, ls, Xc, Xp = _problem(kind, 3, 25, 400, noise, ard, 3)
    jitter = 1e-10 if noise > 0 else 1e-8
    om = o.fit(X, y, kind, 1.2, ls, noise, jitter, True)
    yn = (y - om.y_mean) / om.y_std
    for acq, desired, param in (("ei", "min", 0.01), ("pi", "max", 0.0), ("ucb", "max", 2.0)):
        inc = float(y.min() if desired == "min" else y.max())
        lie = br.resolve_lie("max" if desired == "min" else "min", y)
        _check_against_refits(om, yn, Xc, strategy, lie, Xp if pending else None, acq, desired, param, inc, 5)


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
