"""CPU: the rank-update restatement of tgp_sweep_batch_mc's greedy loop (tests/mc_reference.py) against S LITERAL refits
per step -- one oracle.fit per simulation on the real data plus that simulation's fantasies, pre-normalised, with
normalize_y=False and the kernel held (batch_reference.refit_posterior), then predict, the acquisition with that
simulation's incumbent, and the average (include/turbogp.h states the contract; old_library/bayesian_optimiser.py:568-624
the method)."""
import numpy as np
import pytest

from oracle import gp_oracle as o
import batch_reference as br
import mc_reference as mr


def _problem(N, D, kind, noise, M, seed, ard=False, ls_scale=1.0):
    """the generator of tests/test_gpu_batch.py"""
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    w = rng.normal(size=D) / np.sqrt(D)
    y = np.sin(3 * X @ w) + 0.5 * ((X - 0.5) ** 2).sum(1) + 0.01 * rng.normal(size=N)
    iso = float(np.sqrt(D / 6.0)) * ls_scale
    ls = iso * (0.5 + np.arange(D) / max(D - 1.0, 1.0)) if ard else iso
    Xc = rng.uniform(0, 1, (M, D))
    Xp = rng.uniform(0, 1, (4, D))
    return X, y, ls, Xc, Xp


# N, D, kind, noise, S, P, q   (the noise-free case at the shorter length scale tests/test_gpu_batch.py uses for it)
PROBLEMS = [
    (32, 2, "matern52", 1e-4, 4, 2, 3),
    (128, 4, "rbf", 1e-3, 6, 3, 4),
    (200, 4, "rbf", 0.0, 4, 2, 3),
    (512, 8, "matern32", 1e-4, 8, 4, 4),
]
ACQ_ROWS = (("ei", "min", 0.01), ("pi", "max", 0.0), ("ucb", "max", 2.0), ("ei", "max", 0.01), ("ucb", "min", 2.0))


@pytest.mark.parametrize("prob", PROBLEMS, ids=["-".join(str(v) for v in p) for p in PROBLEMS])
def test_rank_updates_equal_S_literal_refits(prob):
    """every candidate's averaged acquisition at every step within 1e-9 of the step's best value"""
    N, D, kind, noise, S, P, q = prob
    X, y, ls, Xc, Xp = _problem(N, D, kind, noise, 300, 7 + N, ard=(kind == "matern52"), ls_scale=1.0 if noise > 0 else 0.4)
    jitter = 1e-10 if noise > 0 else 1e-8
    om = o.fit(X, y, kind, 1.0, ls, noise, jitter, True)
    yn = (y - om.y_mean) / om.y_std
    Xp = Xp[:P]
    eps = mr.normals(11 + N, S, P + q)
    worst = 0.0
    for acq, desired, param in ACQ_ROWS:
        inc0 = float(y.min() if desired == "min" else y.max())
        ref = mr.select_batch(om, Xc, q, eps, Xp, acq, desired, param, inc0)
        assert not ref["not_pd"]
        assert len(set(ref["idx"].tolist())) == q
        Z, fant = ref["Z"], ref["fantasies"]
        pick = np.maximum if desired == "max" else np.minimum
        for k in range(q):
            j = P + k
            tot = np.zeros(len(Xc))
            for s in range(S):
                mu, sg = br.refit_posterior(om, yn, Z[:j], fant[s, :j], Xc)
                inc_s = float(pick.reduce(np.concatenate([[inc0], fant[s, :j]])))
                tot = tot + o.acquisition(acq, mu, sg, desired, param, inc_s)
            a = tot / S
            a[ref["idx"][:k]] = -np.inf
            got = ref["acq"][k]
            live = np.isfinite(a)
            assert np.array_equal(live, np.isfinite(got))
            best = np.abs(a[live]).max()
            err = np.abs(got[live] - a[live]).max() / best
            worst = max(worst, err)
            assert err <= 1e-9, (acq, desired, k, err)
            assert ref["idx"][k] == int(np.argmax(a)), (acq, desired, k)
            # the fantasy of simulation s at the point taken: a draw of y around the refit's mean there, R[j,j] wide
            for s in range(S):
                mu, sg = br.refit_posterior(om, yn, Z[:j], fant[s, :j], Xc[ref["idx"][k]][None, :])
                sd_y = np.sqrt(sg[0] ** 2 + om.y_std ** 2 * jitter)     # predict's variance holds the noise, not the jitter
                np.testing.assert_allclose((fant[s, j] - mu[0]) / sd_y, eps[s, j], rtol=1e-6, atol=1e-6)
    print("worst |rank update - literal refits| / step's best: %.3g" % worst)


@pytest.mark.parametrize("pending", [False, True])
@pytest.mark.parametrize("S", [1, 3, 16])
def test_zero_eps_is_kriging_believer(S, pending):
    X, y, ls, Xc, Xp = _problem(60, 3, "matern52", 1e-4, 400, 5, ard=True)
    om = o.fit(X, y, "matern52", 1.0, ls, 1e-4, 1e-10, True)
    Xp = Xp[:3] if pending else None
    P = 3 if pending else 0
    for acq, desired, param in ACQ_ROWS:
        inc = float(y.min() if desired == "min" else y.max())
        kb = br.select_batch(om, Xc, 5, br.KB, 0.0, Xp, acq, desired, param, inc)
        ref = mr.select_batch(om, Xc, 5, np.zeros((S, P + 5)), Xp, acq, desired, param, inc)
        np.testing.assert_array_equal(ref["idx"], kb["idx"])
        np.testing.assert_allclose(ref["val"], kb["val"], rtol=1e-12, atol=0)
        for k in range(5):
            live = np.isfinite(kb["acq"][k])
            np.testing.assert_allclose(ref["acq"][k][live], kb["acq"][k][live], rtol=1e-12, atol=1e-300)
        for s in range(S):
            np.testing.assert_allclose(ref["fantasies"][s], kb["fantasies"], rtol=1e-12, atol=0)
        np.testing.assert_allclose(ref["sigma"], kb["sigma"], rtol=1e-12, atol=0)


def test_sigma_does_not_depend_on_the_simulations():
    X, y, ls, Xc, Xp = _problem(60, 3, "rbf", 1e-4, 400, 6)
    om = o.fit(X, y, "rbf", 1.0, ls, 1e-4, 1e-10, True)
    kb = br.select_batch(om, Xc, 5, br.KB, 0.0, Xp, "ucb", "max", np.inf, 0.0)
    ref = mr.select_batch(om, Xc, 5, mr.normals(3, 7, 9), Xp, "ucb", "max", np.inf, 0.0)
    np.testing.assert_array_equal(ref["idx"], kb["idx"])
    np.testing.assert_array_equal(ref["val"], kb["val"])


def test_pending_fantasies_have_the_joint_predictive_covariance_of_y():
    """the draw is JOINT: over many simulations the pending fantasies' sample mean and covariance are the model's
    predictive mean and covariance of y at the pending points (nearby points, so the off-diagonal terms are large).
    Bars: 5 standard errors -- of a mean sqrt(C_ii / S), of a sample covariance of Gaussians sqrt((C_ii C_jj + C_ij^2) / (S - 1))"""
    S = 20000
    X, y, ls, Xc, _ = _problem(40, 2, "matern52", 1e-2, 20, 9, ard=True)
    om = o.fit(X, y, "matern52", 1.0, ls, 1e-2, 1e-10, True)
    base = np.array([0.31, 0.62])
    Xp = base + np.array([[0.0, 0.0], [0.03, -0.02], [-0.25, 0.2], [0.02, 0.04]])
    eps = mr.normals(2024, S, 5)
    ref = mr.select_batch(om, Xc, 1, eps, Xp, "ei", "min", 0.01, float(y.min()))
    F = ref["fantasies"][:, :4]
    C = mr.pending_y_covariance(om, Xp)
    mean, _ = o.predict(om, Xp)
    se_mean = np.sqrt(np.diag(C) / S)
    assert np.all(np.abs(F.mean(0) - mean) <= 5 * se_mean), (F.mean(0) - mean) / se_mean
    Chat = np.cov(F.T, ddof=1)
    se = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C ** 2) / (S - 1))
    z = np.abs(Chat - C) / se
    assert z.max() <= 5.0, z
    # the test has teeth: the neighbours' correlation is far from the zero that independent draws would give
    corr01 = C[0, 1] / np.sqrt(C[0, 0] * C[1, 1])
    assert corr01 > 0.3 and abs(0.0 - C[0, 1]) / se[0, 1] > 20


def test_normals_layout():
    """simulation s does not depend on S, the draw for point j not on J; the moments are a standard normal's"""
    a, b = mr.normals(5, 4, 7), mr.normals(5, 64, 12)
    assert a.tobytes() == b[:4, :7].copy().tobytes()
    assert not np.array_equal(mr.normals(6, 4, 7), a)
    z = mr.normals(1, 4000, 64).reshape(-1)
    n = z.size
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2.0 / n)
