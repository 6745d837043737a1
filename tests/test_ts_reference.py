"""CPU: tests/ts_reference.py -- the NumPy restatement tests/test_gpu_thompson.py holds the GPU to -- held to the
mathematics of pathwise conditioning with random Fourier features.  Tolerances are multiples of the Monte Carlo
standard error of each estimate, not tuned constants."""
import numpy as np
import pytest

from oracle import gp_oracle as o
import ts_reference as tr

KINDS = ["rbf", "matern12", "matern32", "matern52"]


def _fit(kind, noise=1e-2, N=20, D=2, seed=0, normalize_y=True):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    y = 2.0 + np.sin(4 * X[:, 0]) + np.cos(3 * X[:, 1 % D]) + 0.05 * rng.normal(size=N)
    ls = np.array([0.35, 0.5][:D]) if D <= 2 else 0.5
    return o.fit(X, y, kind, 1.3, ls, noise, 1e-10, normalize_y), rng


@pytest.mark.parametrize("kind", KINDS)
def test_feature_kernel_tends_to_the_exact_kernel(kind):
    """(2c/F) sum cos(w u + b) cos(w u' + b) -> c k0(u - u'): each term has variance <= c^2 (2/F)... so the error at
    F features is within a few sqrt(2/F) c, and shrinks as F grows"""
    rng = np.random.RandomState(1)
    U1, U2 = rng.uniform(0, 2, (15, 2)), rng.uniform(0, 2, (15, 2))
    c = 1.3
    exact = o.cross_kernel(U1, U2, kind, c, 1.0)
    errs = []
    for F in (256, 2048, 16384):
        d = tr.draw(123, 1, F, 2, 1, kind, 0.0)
        est = tr.mc_kernel(d["omega"], d["b"], U1, U2, c)
        err = np.abs(est - exact).max()
        assert err <= 5.0 * c * np.sqrt(2.0 / F), (F, err)
        errs.append(err)
    assert errs[-1] < errs[0]


def test_the_draw_is_what_the_layout_says():
    """uniforms of 53 bits from two words, b = 2 pi u; streams independent; Matern omega = z sqrt(2 nu / chi2)"""
    d = tr.draw(7, 3, 128, 4, 5, "matern32", 0.25)
    assert d["omega"].shape == (128, 4) and d["b"].shape == (128,) and d["W"].shape == (3, 128) and d["eps"].shape == (3, 5)
    assert np.all((d["b"] >= 0) & (d["b"] < 2 * np.pi))
    r = tr.philox4x32_10(np.uint64(5), 0, tr.S_B, tr.TAG, 7, 0)
    u = ((int(r[0]) >> 5) * 67108864.0 + (int(r[1]) >> 6)) / 9007199254740992.0
    assert d["b"][5] == tr.TWO_PI * u
    z = tr.normals(np.arange(3 * 5, dtype=np.uint64), tr.S_EPS, 7).reshape(3, 5)
    np.testing.assert_array_equal(d["eps"], 0.5 * z)
    rbf = tr.draw(7, 3, 128, 4, 5, "rbf", 0.25)
    n = tr.normals(np.uint64(8 * 9) + np.arange(3, dtype=np.uint64), tr.S_CHI2, 7)
    np.testing.assert_allclose(d["omega"][9], rbf["omega"][9] * np.sqrt(3.0 / (n ** 2).sum()), rtol=1e-15)
    big = tr.normals(np.arange(200000, dtype=np.uint64), tr.S_W, 99)
    se = 1.0 / np.sqrt(big.size)
    assert abs(big.mean()) < 5 * se and abs(big.var() - 1.0) < 5 * np.sqrt(2.0) * se


@pytest.mark.parametrize("kind", KINDS)
def test_mean_and_covariance_match_the_posterior(kind):
    """over S = 4000 paths at 30 held-out points: the empirical mean is the posterior mean and the empirical covariance
    the LATENT posterior covariance (the oracle's sigma^2 minus the WhiteKernel noise), within the Monte Carlo error
    plus the F-feature kernel error"""
    m, rng = _fit(kind)
    S, F = 4000, 4096
    Xt = rng.uniform(0, 1, (30, 2))
    p = tr.Paths(m, 2024, S, F)
    f = p.values(Xt)                                                    # (30, S)
    mu, sd = o.predict(m, Xt)
    var_f = sd ** 2 - m.noise * m.y_std ** 2                            # latent
    se_mean = np.sqrt(np.maximum(var_f, 0) / S)
    feat = m.y_std ** 2 * m.constant * 5.0 * np.sqrt(2.0 / F)          # the prior's kernel error, raw units
    assert np.all(np.abs(f.mean(1) - mu) <= 5.0 * se_mean + np.sqrt(feat) * 5.0 / np.sqrt(S)), kind
    emp = np.cov(f)
    Ks = o.cross_kernel(Xt, m.X, kind, m.constant, m.length_scale)
    V = np.linalg.solve(m.L, Ks.T)
    post = (o.cross_kernel(Xt, Xt, kind, m.constant, m.length_scale) - V.T @ V) * m.y_std ** 2
    np.testing.assert_allclose(np.diag(post), var_f, rtol=1e-6, atol=1e-10)
    se_cov = np.sqrt((post ** 2 + np.outer(np.diag(post), np.diag(post))) / S)
    assert np.all(np.abs(emp - post) <= 5.0 * se_cov + feat), (kind, float(np.abs(emp - post).max()))


def test_the_mean_is_exact_whatever_F():
    """E[f_s] = mu for every F: with W and eps averaged out analytically the path is the posterior mean"""
    m, rng = _fit("matern52")
    p = tr.Paths(m, 5, 1, 64)
    Xt = rng.uniform(0, 1, (10, 2))
    Ks = o.cross_kernel(Xt, m.X, m.kind, m.constant, m.length_scale)
    np.testing.assert_allclose(m.y_mean + m.y_std * (Ks @ m.alpha), o.predict(m, Xt)[0], rtol=1e-12)
    # the path = mean + (prior - K* K^-1 (prior(X) + eps)): linear in (W, eps), zero at W = eps = 0
    p.d["W"][:] = 0.0
    p.d["eps"][:] = 0.0
    pX = p.prior_scaled(p.Xs)
    from scipy.linalg import cho_solve
    p.V = (m.alpha[:, None] - cho_solve((m.L, True), pX + p.d["eps"].T)).T
    np.testing.assert_allclose(p.values(Xt)[:, 0], o.predict(m, Xt)[0], rtol=1e-12)


@pytest.mark.parametrize("kind", KINDS)
def test_a_path_through_a_training_point_reproduces_it(kind):
    m, _ = _fit(kind, noise=1e-10)
    p = tr.Paths(m, 11, 4, 1024)
    f = p.values(m.X)
    y = m.y_mean + m.y_std * m.L @ (m.L.T @ m.alpha)     # the raw targets, rebuilt from the fit
    # f(X_n) = y~_n - eps_n up to the noise-free part of the posterior there: within a few sd of eps
    np.testing.assert_allclose(f, np.repeat(y[:, None], 4, 1), rtol=0, atol=6.0 * np.sqrt(m.noise + m.jitter) * m.y_std)


def test_sample_s_does_not_depend_on_S():
    m, rng = _fit("rbf")
    Xt = rng.uniform(0, 1, (7, 2))
    one = tr.Paths(m, 3, 1, 512).values(Xt)
    many = tr.Paths(m, 3, 64, 512).values(Xt)
    np.testing.assert_allclose(many[:, :1], one, rtol=1e-13)
    assert np.abs(many[:, 1] - one[:, 0]).max() > 1e-3


@pytest.mark.parametrize("kind", KINDS)
def test_gradient_is_the_central_difference(kind):
    m, rng = _fit(kind, N=15, D=2)
    p = tr.Paths(m, 8, 3, 256)
    X = rng.uniform(0, 1, (6, 2))
    g = p.grad(X)
    h = 1e-6
    for d in range(2):
        e = np.zeros(2)
        e[d] = h
        fd = (p.values(X + e) - p.values(X - e)) / (2 * h)
        np.testing.assert_allclose(g[:, :, d], fd, rtol=1e-5, atol=1e-6)


def test_distinct_selection():
    f = np.array([[1.0, 1.0, 0.0], [1.0, 5.0, np.nan], [0.5, 5.0, 2.0]])
    idx, val = tr.select(f, 1.0, False)
    np.testing.assert_array_equal(idx, [0, 1, 2])
    idx, val = tr.select(f, 1.0, True)
    np.testing.assert_array_equal(idx, [0, 1, 2])
    idx, _ = tr.select(np.array([[3.0, 3.0], [2.0, 2.0]]), 1.0, True)
    np.testing.assert_array_equal(idx, [0, 1])
    idx, _ = tr.select(np.array([[3.0, 3.0], [2.0, 2.0]]), -1.0, False)
    np.testing.assert_array_equal(idx, [1, 1])
