"""CPU: the pruned sweep's bound and margin logic (tests/prune_reference.py, the NumPy restatement of sweep_pruned) on an
f64 posterior -- every bound is at or above the exact acquisition, the monotonicity it rests on holds, the pruned arg-max
is the full one, and the clamp gate opens and closes where DESIGN.md §4 says."""
import math

import numpy as np
import pytest

import prune_reference as pr


def _posterior(seed=0, N=200, D=3, M=3000, noise=1e-2, constant=1.0, ls=0.4):
    """RBF posterior in f64: normalised mean K*.alpha, |K*|.|alpha|, variance c + s^2 - q, y mean / std"""
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, size=(N, D))
    y = np.sin(3 * X.sum(1)) + 0.01 * rng.normal(size=N)
    Xc = rng.uniform(0, 1, size=(M, D))
    Xc[:50] = X[:50]                                # candidates at training points: the smallest variances
    ym, ys = y.mean(), y.std()
    yn = (y - ym) / ys
    k = lambda A, B: constant * np.exp(-0.5 * (((A[:, None, :] - B[None, :, :]) / ls) ** 2).sum(-1))
    K = k(X, X) + noise * np.eye(N)
    L = np.linalg.cholesky(K)
    alpha = np.linalg.solve(L.T, np.linalg.solve(L, yn))
    Ks = k(Xc, X)
    V = np.linalg.solve(L, Ks.T)
    var = constant + noise - (V * V).sum(0)
    return Ks @ alpha, np.abs(Ks) @ np.abs(alpha), var, ym, ys, N, y


CASES = [(pr.ACQ_EI, -1.0, 0.01), (pr.ACQ_EI, 1.0, 0.0), (pr.ACQ_PI, -1.0, 0.01), (pr.ACQ_PI, 1.0, 0.0),
         (pr.ACQ_UCB, 1.0, 2.0), (pr.ACQ_UCB, -1.0, 2.0), (pr.ACQ_UCB, 1.0, -1.0)]


def _exact_and_bounds(acq, sf, param, noise=1e-2, constant=1.0, jitter_mean=0.0):
    mun, s, var, ym, ys, N, y = _posterior(noise=noise, constant=constant)
    inc = float(y.min() if sf < 0 else y.max())
    mun_x = mun + jitter_mean * pr.err_scale(N) * s * 0.5       # another summation order of the same products
    exact = np.array([pr.acq_value(acq, sf, inc, param, ys * m + ym, math.sqrt(max(v, 0.0) * ys * ys))
                      for m, v in zip(mun_x, var)])
    ub = np.array([pr.upper_bound(acq, sf, inc, param, m, a, N, constant, noise, ym, ys) for m, a in zip(mun, s)])
    return exact, ub, var, noise


@pytest.mark.parametrize("acq,sf,param", CASES)
@pytest.mark.parametrize("jitter", [-1.0, 0.0, 1.0])
def test_every_bound_is_above_the_exact_value(acq, sf, param, jitter):
    exact, ub, var, noise = _exact_and_bounds(acq, sf, param, jitter_mean=jitter)
    assert var.min() >= 0.99 * noise                    # the interval's lower end holds for this posterior
    assert np.all(ub >= exact), np.max(exact - ub)


@pytest.mark.parametrize("acq,sf,param", CASES)
def test_the_pruned_argmax_is_the_full_argmax(acq, sf, param):
    exact, ub, _, _ = _exact_and_bounds(acq, sf, param)
    val, idx, nsurv = pr.pruned_argmax(exact, ub)
    j = int(np.argmax(exact))
    assert (val, idx) == (float(exact[j]), j)
    assert nsurv < len(exact)


def test_ties_survive_and_the_lowest_index_wins():
    exact, ub, _, _ = _exact_and_bounds(pr.ACQ_EI, -1.0, 0.01)
    j = int(np.argmax(exact))
    for t in (j // 2, j + 5):
        exact[t], ub[t] = exact[j], ub[j]
    val, idx, _ = pr.pruned_argmax(exact, ub)
    assert idx == j // 2 and val == exact[j]


def test_acquisitions_are_monotone_in_sigma():
    sig = np.linspace(1e-3, 3.0, 400)
    for mu in (-2.0, -0.3, 0.0, 0.4, 2.5):
        ei = [pr.acq_value(pr.ACQ_EI, -1.0, 0.1, 0.01, mu, s) for s in sig]
        assert np.all(np.diff(ei) >= -1e-15)
        pi = np.array([pr.acq_value(pr.ACQ_PI, -1.0, 0.1, 0.01, mu, s) for s in sig])
        diff = -(mu - 0.1) - 0.01
        assert np.all(np.diff(pi) <= 1e-15) if diff > 0 else np.all(np.diff(pi) >= -1e-15)
        for param in (2.0, -1.0):
            ucb = np.diff([pr.acq_value(pr.ACQ_UCB, 1.0, 0.0, param, mu, s) for s in sig])
            assert np.all(ucb > 0) if param > 0 else np.all(ucb < 0)


def test_bar_and_margin():
    assert pr.bar(1.0) == 1.0 - 1e-6
    assert pr.bar(-2.0) == -2.0 - 2e-6
    assert pr.bar(-math.inf) == -math.inf and pr.bar(math.inf) == math.inf
    ub = np.array([0.5, 1.0 - 1e-7, 0.999, 2.0])
    assert list(pr.survivors(ub, [3], 1.0)) == [1]


def test_lb_set_is_one_best_bound_per_group():
    ub = np.array([3.0, 1.0, 3.0, 0.0, 5.0, 5.0, -np.inf])
    assert list(pr.lb_set(ub, top=3)) == [0, 4, 6]
    assert list(pr.lb_set(ub, top=100)) == list(range(7))


def test_the_clamp_gate():
    # the BASELINE configs: C1 / C2 f64 with noise 1e-4, C3 / C4 f32 with noise 1e-2 -- all open
    assert pr.gate(1e-4, 1.0, "f64") and pr.gate(1e-2, 1.0, "f32")
    # f32 with noise 1e-4 (a candidate at a training point may clamp): closed; f64 holds it down to ~1e-12
    assert not pr.gate(1e-4, 1.0, "f32")
    assert pr.gate(1e-10, 1.0, "f64") and not pr.gate(1e-13, 1.0, "f64")
    assert not pr.gate(0.0, 1.0, "f64")
