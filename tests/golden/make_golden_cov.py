#!/usr/bin/env python3
"""Golden vectors for the joint posterior (tests/golden/cov_*.npz), generated from the reference's own
SciKitGPSurrogate (turbo/modules/surrogates.py:225-365): its ModelInstance wraps a scikit-learn
GaussianProcessRegressor, and ``predict(X, return_cov=True)`` on that object (sklearn _gpr.py:454-469) is what
tgp_predict_cov replaces.  Runs in the build container only (needs /root/reference); data only."""
import os
import sys
import warnings

import numpy as np

REF = "/root/reference"
if not os.path.isdir(os.path.join(REF, "turbo")):
    sys.exit("needs /root/reference; the committed .npz fixtures are what travels")
sys.path.insert(0, REF)
import sklearn.gaussian_process as sk_gp  # noqa: E402

if not hasattr(np, "asscalar"):
    np.asscalar = lambda a: np.asarray(a).item()

import turbo.modules as tm  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
K = sk_gp.kernels


def run_case(name, seed, N, D, m, kernel, kind, constant, ls, noise, normalize_y, jitter=1e-10):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, size=(N, D))
    y = 3.0 + 2.0 * np.sin(3 * X.sum(1)) + 0.05 * rng.normal(size=N)
    Xq = rng.uniform(0, 1, size=(m, D))
    Xq[0] = X[0]                      # a training point: variance ~ noise
    Xq[1] = 40.0                      # far away: the prior
    sur = tm.SciKitGPSurrogate(model_params=dict(kernel=kernel, optimizer=None, normalize_y=normalize_y, alpha=jitter),
                               training_iterations=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model, _ = sur.construct_model(0, X, y)
        y_mean, y_cov = model.model.predict(Xq, return_cov=True)
        mus, sigmas = model.predict(Xq, return_std_dev=True)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), X=X, y=y, Xq=Xq, kind=kind, constant=constant,
                        length_scale=np.atleast_1d(ls), noise=noise, jitter=jitter, normalize_y=normalize_y,
                        y_mean=np.asarray(y_mean).reshape(-1), y_cov=np.asarray(y_cov), sigmas=np.asarray(sigmas).reshape(-1))
    print(name, "diag range", np.diag(y_cov).min(), np.diag(y_cov).max())


if __name__ == "__main__":
    run_case("cov_matern52_white_2d", 11, 20, 2, 15, 1.5 * K.Matern(length_scale=0.4, nu=2.5) + K.WhiteKernel(1e-3),
             "matern52", 1.5, 0.4, 1e-3, True)
    ls = np.array([0.3, 0.6, 1.1])
    run_case("cov_rbf_ard_3d", 12, 12, 3, 9, 0.8 * K.RBF(length_scale=ls), "rbf", 0.8, ls, 0.0, False)
