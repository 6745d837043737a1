"""CPU: tests/cov_reference.py -- the restatement the ABI and GPU tests hold the library to -- against the reference's
sklearn model (the goldens, and sklearn itself on fuzzed cases) and against the closed-form EI."""
import os

import numpy as np
import pytest

import cov_reference as cr
from conftest import golden_path
from oracle import gp_oracle as G

GOLDENS = ("cov_matern52_white_2d", "cov_rbf_ard_3d")


def load_golden(name):
    with np.load(golden_path(name), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    ls = d["length_scale"]
    d["ls"] = float(ls[0]) if ls.size == 1 else ls
    d["kind"] = str(d["kind"])
    return d


def golden_model(d):
    return G.fit(d["X"], d["y"], d["kind"], float(d["constant"]), d["ls"], float(d["noise"]), float(d["jitter"]),
                 bool(d["normalize_y"]))


@pytest.mark.parametrize("name", GOLDENS)
def test_reference_equals_the_golden(name):
    d = load_golden(name)
    model = golden_model(d)
    mu, cov, neg = cr.predict_cov(model, d["Xq"], latent=False)
    vs, ms = cr.scales(model)
    # two f64 implementations of the same formulas: the project's measured class, far inside the 1e-5 bar
    assert np.abs(mu - d["y_mean"]).max() <= 1e-9 * ms
    assert np.abs(cov - d["y_cov"]).max() <= 1e-9 * vs
    assert neg == int((np.diag(d["y_cov"]) < 0).sum())
    assert np.abs(np.sqrt(np.maximum(np.diag(cov), 0)) - d["sigmas"]).max() <= 1e-7 * ms
    lat = cr.predict_cov(model, d["Xq"], latent=True)[1]
    assert np.abs((cov - lat) - model.y_std ** 2 * float(d["noise"]) * np.eye(len(mu))).max() <= 1e-12 * vs


@pytest.mark.parametrize("kind", ["rbf", "matern12", "matern32", "matern52"])
def test_reference_equals_sklearn_on_a_fuzzed_case(kind):
    import sklearn.gaussian_process as skgp
    K = skgp.kernels
    rng = np.random.RandomState({"rbf": 1, "matern12": 2, "matern32": 3, "matern52": 4}[kind])
    N, D, m = 25, 3, 14
    X, Xq = rng.uniform(0, 1, (N, D)), rng.uniform(-0.2, 1.2, (m, D))
    Xq[3] = Xq[2]                                   # duplicated query rows: the noise stays on the diagonal
    y = 1.0 + np.cos(4 * X[:, 0]) * X[:, 1] + 0.1 * rng.normal(size=N)
    c, ls, noise = 1.3, np.array([0.5, 0.8, 0.3]), 2e-3
    base = K.RBF(length_scale=ls) if kind == "rbf" else K.Matern(length_scale=ls, nu={"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}[kind])
    gpr = skgp.GaussianProcessRegressor(kernel=c * base + K.WhiteKernel(noise), optimizer=None, normalize_y=True, alpha=1e-10)
    gpr.fit(X, y)
    want_mu, want_cov = gpr.predict(Xq, return_cov=True)
    model = G.fit(X, y, kind, c, ls, noise, 1e-10, True)
    mu, cov, _ = cr.predict_cov(model, Xq)
    vs, ms = cr.scales(model)
    assert np.abs(mu - want_mu).max() <= 1e-9 * ms
    assert np.abs(cov - want_cov).max() <= 1e-9 * vs
    assert cov[2, 3] < cov[2, 2] and abs(cov[2, 2] - cov[2, 3] - model.y_std ** 2 * noise) <= 1e-9 * vs
    # samples given eps reproduce the covariance's factor: y - mu = y_std Lc eps
    eps = rng.standard_normal((5, m))
    yv, mu2 = cr.sample_joint(model, Xq, eps, nugget=1e-10)
    Lc = np.linalg.cholesky(cov + model.y_std ** 2 * 1e-10 * np.eye(m))
    assert np.array_equal(mu, mu2) and np.abs((yv - mu) - eps @ Lc.T).max() <= 1e-9 * ms


def test_duplicated_rows_need_a_nugget():
    d = load_golden("cov_rbf_ard_3d")
    model = golden_model(d)
    Xq = np.vstack([d["Xq"][2:5], d["Xq"][3:4]])
    eps = np.zeros((1, 4))
    with pytest.raises(np.linalg.LinAlgError):
        cr.sample_joint(model, Xq, eps, latent=True, nugget=0.0)
    cr.sample_joint(model, Xq, eps, latent=True, nugget=1e-6)


def test_joint_ei_of_one_point_is_the_closed_form_ei():
    """q = 1, S = 4096 fixed normals: within 4 standard errors (from the sample) of oracle.gp_oracle's closed form"""
    SEED = 20240607          # chosen here, on the CPU, with the reference alone
    d = load_golden("cov_matern52_white_2d")
    model = golden_model(d)
    eps = np.random.RandomState(SEED).standard_normal((4096, 1))
    for ext in ("min", "max"):
        inc = float(d["y"].min() if ext == "min" else d["y"].max())
        # points next to the incumbent's own location: mu is near the incumbent there, so a good share of the samples
        # improves on it and the sample's standard error means something (far from it no sample improves: se = 0)
        x_inc = d["X"][int(np.argmin(d["y"]) if ext == "min" else np.argmax(d["y"]))]
        for k in (1, 2, 3, 4):
            x = x_inc + 0.03 * k
            yv, _ = cr.sample_joint(model, x[None, :], eps, nugget=1e-10)
            terms = cr.joint_ei_terms(yv, ext, inc, 0.01)
            mu, sg = G.predict(model, x[None, :])
            want = float(G.acquisition("ei", mu, sg, ext, 0.01, inc)[0])
            se = terms.std(ddof=1) / np.sqrt(len(terms))
            assert abs(terms.mean() - want) <= 4.0 * se + 1e-12, (ext, terms.mean(), want, se)
            assert cr.joint_ei(model, x[None, :], eps, ext, inc, 0.01) == terms.mean()


def test_normals_are_indexed_by_sample_and_point():
    a, b = cr.normals(7, 3, 17), cr.normals(7, 8, 65)
    assert np.array_equal(a, b[:3, :17]) and not np.array_equal(a, cr.normals(8, 3, 17))
    big = cr.normals(5, 64, 512)
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1.0) < 0.02
