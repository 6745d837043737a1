"""NumPy/SciPy f64 restatement of the joint posterior (tgp_predict_cov, tgp_sample_joint; include/turbogp.h) and of
``turbo_amd.joint_ei`` -- TEST INFRASTRUCTURE, written from the definitions, not from the library.

Built on oracle.gp_oracle like the other references (fit, cross_kernel).  In normalised units:
    Ks = c k0(Xq, X);  V = L^-1 Ks^T;  Sigma = c k0(Xq, Xq) + [latent ? 0 : noise] I - V^T V
    mu = y_mean + y_std Ks alpha;  raw covariance = y_std^2 Sigma
    y[s, j] = mu[j] + y_std (Lc eps[s, :])[j],  Lc = chol(Sigma + nugget I)
The noise sits on the diagonal only (duplicated rows included), the jitter is not in Sigma, nothing is clamped.
tests/test_cov_reference.py holds this module to the reference's sklearn model; the ABI and GPU tests hold the library to it.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

from oracle import gp_oracle as G
from philox_ref import philox4x32_10

TAG = 0x434F564A          # "COVJ"
STRIDE = 4096             # element s 4096 + j
TWO_PI = 6.283185307179586
EPS = 2.220446049250313e-16


def _sigma(model, Xq, latent):
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    Ks = G.cross_kernel(Xq, model.X, model.kind, model.constant, model.length_scale)
    V = solve_triangular(model.L, Ks.T, lower=True, check_finite=False)
    Kqq = G.cross_kernel(Xq, Xq, model.kind, model.constant, model.length_scale)
    Sigma = Kqq - V.T @ V
    if not latent:
        Sigma = Sigma + model.noise * np.eye(Xq.shape[0])
    mu = model.y_mean + model.y_std * (Ks @ model.alpha)
    return mu, Sigma


def predict_cov(model, Xq, latent=False):
    """mu (m,), cov (m, m) raw units, number of negative diagonal entries"""
    mu, Sigma = _sigma(model, Xq, latent)
    cov = model.y_std ** 2 * Sigma
    return mu, cov, int((np.diag(cov) < 0).sum())


def sample_joint(model, Xq, eps, latent=False, nugget=0.0):
    """y (S, m), mu (m,) for eps (S, m); numpy.linalg.LinAlgError under the pivot rule of the entry: a pivot whose square
    is <= 8 eps x (that diagonal entry of Sigma + nugget I), or not finite"""
    mu, Sigma = _sigma(model, Xq, latent)
    A = 0.5 * (Sigma + Sigma.T) + nugget * np.eye(Sigma.shape[0])
    Lc = cholesky(A, lower=True, check_finite=False)      # (raises LinAlgError at a pivot <= 0)
    d = np.diag(Lc)
    if not np.all(np.isfinite(d)) or np.any(d * d <= 8.0 * EPS * np.diag(A)):
        raise np.linalg.LinAlgError("pivot below 8 eps of its diagonal entry")
    eps = np.atleast_2d(np.asarray(eps, dtype=np.float64))
    return mu[None, :] + model.y_std * (eps @ Lc.T), mu


def _u53(a, b):
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def normals(seed, S, m):
    """eps (S, m) of tgp_sample_joint(eps_in = NULL): one Box-Muller branch per element s 4096 + j, counter
    (element lo, element hi, 0, TAG): sqrt(-2 log(1 - u1)) cos(2 pi u2), u1 from words (0, 1), u2 from (2, 3)"""
    seed = int(seed) % (1 << 64)
    e = (np.arange(S, dtype=np.uint64)[:, None] * np.uint64(STRIDE) + np.arange(m, dtype=np.uint64)[None, :]).reshape(-1)
    r = philox4x32_10(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), 0, TAG, seed & 0xFFFFFFFF, seed >> 32)
    u1, u2 = _u53(r[0], r[1]), _u53(r[2], r[3])
    return (np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(TWO_PI * u2)).reshape(S, m)


def joint_ei_terms(y, desired_extremum, incumbent, xi):
    """(S,) the per-sample improvements max(0, max_j (sf (y_sj - incumbent) - xi)) for y (S, q)"""
    sf = 1.0 if desired_extremum == "max" else -1.0
    return np.maximum((sf * (np.asarray(y) - incumbent) - xi).max(axis=1), 0.0)


def joint_ei(model, Xb, eps, desired_extremum, incumbent, xi=0.01, latent=False, nugget=1e-10):
    y, _ = sample_joint(model, Xb, eps, latent, nugget)
    return float(joint_ei_terms(y, desired_extremum, incumbent, xi).mean())


def scales(model):
    """(covariance scale, value scale): the prior variance y_std^2 (c + noise) and its root -- what the parity bar 1e-5 of
    tests/test_gpu_parity.py is multiplied by for covariance entries and for mu / sample values"""
    v = model.y_std ** 2 * (model.constant + model.noise)
    return v, np.sqrt(v)
