"""The problems the tgp_hyper_sample tests walk (CPU host handle and GPU handles) and the comparison with the NumPy reference
chain of tests/slice_reference.py.  Test helper, not product code."""
import math

import numpy as np

import slice_reference as sr

MARGIN = 1e-6      # a reference walk must keep every LML this far from its slice level (the stated condition on the walks)


def problem(N, D, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3.0 * X.sum(1)) + 0.5 * X[:, 0] + 0.05 * rng.normal(size=N)
    return X, y


def case(name):
    """dict(X, y, kind, n_ls, theta0, lo, hi, jitter, normalize_y, width, seed): the seeds were picked on the CPU so that the
    reference walk's margin exceeds MARGIN (asserted again by every test that uses them)"""
    if name == "rbf_iso_noise_n12":          # P = 3, everything free
        X, y = problem(12, 1, 0)
        return dict(X=X, y=y, kind="rbf", n_ls=1, theta0=np.log([1.0, 0.3, 1e-2]), lo=np.log([1e-2, 1e-2, 1e-5]),
                    hi=np.log([1e2, 1e1, 1.0]), jitter=1e-10, normalize_y=True, width=None, seed=2)
    if name == "matern52_ard_fixed_noise_n40":   # P = 5, the noise fixed
        X, y = problem(40, 3, 1)
        return dict(X=X, y=y, kind="matern52", n_ls=3, theta0=np.log([1.0, 0.5, 0.7, 0.9, 1e-3]),
                    lo=np.log([1e-2, 5e-2, 5e-2, 5e-2, 1e-3]), hi=np.log([1e2, 1e1, 1e1, 1e1, 1e-3]), jitter=1e-10,
                    normalize_y=True, width=[1.0, 0.5, 0.5, 0.5, 1.0], seed=3)
    if name == "matern32_iso_fixed_constant_n15":
        X, y = problem(15, 2, 2)
        return dict(X=X, y=y, kind="matern32", n_ls=1, theta0=np.log([1.0, 0.4, 1e-2]), lo=np.log([1.0, 2e-2, 1e-5]),
                    hi=np.log([1.0, 1e1, 1.0]), jitter=1e-10, normalize_y=False, width=2.0, seed=3)
    # the GPU sizes: one-workgroup fit, its two-block path, the blocked fit
    if name == "gpu_n12":
        c = case("rbf_iso_noise_n12")
        c["seed"] = 3
        return c
    if name in ("gpu_n100", "gpu_n300"):
        n = int(name[5:])
        X, y = problem(n, 2, n)
        return dict(X=X, y=y, kind="matern52", n_ls=1, theta0=np.log([1.0, 0.4, 1e-2]), lo=np.log([1e-2, 2e-2, 1e-4]),
                    hi=np.log([1e2, 1e1, 1.0]), jitter=1e-10, normalize_y=True, width=None, seed=4)
    raise KeyError(name)


def reference(c, S, burn, thin):
    lml = sr.oracle_lml(c["X"], c["y"], c["kind"], c["n_ls"], c["jitter"], c["normalize_y"])
    return sr.slice_sample(lml, c["theta0"], c["lo"], c["hi"], S, burn, thin, width=c["width"], seed=c["seed"])


def native(gp, c, S, burn, thin):
    return gp.hyper_sample(c["X"], c["y"], c["kind"], c["theta0"], c["n_ls"], np.stack([c["lo"], c["hi"]], 1), c["jitter"],
                           c["normalize_y"], n_samples=S, burn=burn, thin=thin, width=c["width"], seed=c["seed"])


def assert_same_walk(gp, c, S, burn, thin):
    ref = reference(c, S, burn, thin)
    # the stated condition, on the reference alone: no comparison of the walk was within rounding of its slice level
    assert ref["margin"] > MARGIN, ref["margin"]
    theta, lml, evaluations, not_pd = native(gp, c, S, burn, thin)
    print("margin %.3g  evaluations %d / %d  max |dtheta| %.3g  max |dlml| %.3g"
          % (ref["margin"], evaluations, ref["evaluations"], np.abs(theta - ref["theta"]).max(), np.abs(lml - ref["lml"]).max()))
    assert evaluations == ref["evaluations"] and not_pd == ref["not_pd"]
    np.testing.assert_allclose(theta, ref["theta"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(lml, ref["lml"], rtol=1e-9, atol=1e-8)
    return ref, theta, lml
