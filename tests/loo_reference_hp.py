"""Extended-precision (x87 80-bit, numpy.longdouble) closed form of leave-one-out cross-validation and of the gradient of
its score with respect to the LOG hyper-parameters (tgp_loo, tgp_fit_loo_grad; include/turbogp.h), and an f64 NumPy/SciPy
restatement of the same formulas that can be made to slip -- TEST INFRASTRUCTURE, written from the definitions below
(Rasmussen & Williams section 5.4.2, eqs. 5.10-5.13), not from the kernels.  The 80-bit form sits on
tests/cov_reference_hp.py's Fit (L and alpha in long double) and tests/lml_grad_reference_hp.py's pairwise sums.

    K = c k0, its diagonal SET to c + noise + jitter;  yn the normalised targets;  alpha = K^-1 yn;  L^-1 = forward(L, I)
    kappa_i = (K^-1)_ii = sum_{k >= i} (L^-1)_ki^2
    resid_i = y_i - mu_-i = y_std alpha_i / kappa_i         (raw units)
    sigma_i = y_std / sqrt(kappa_i)                         (raw units; the held-out OBSERVATION: noise and jitter inside)
    lpd_i   = 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log(2 pi);   L_LOO = sum_i lpd_i        (normalised units)
    p = alpha / kappa;  w = 1/2 (1 / kappa + p^2);  b = K^-1 p;  B = K^-1 diag(w) K^-1;  G = b alpha^T + alpha b^T - 2 B
    grad = 1/2 sum G o dK/dlog theta, with dK as in tests/lml_grad_reference_hp.py
y_mean, y_std and the hyper-parameters are HELD across the folds: the closed form is the literal leave-one-out with the
normalisation of all N points (tests/test_loo_reference.py refits N times to show it).

Scales: the sum of the absolute values of a quantity's terms, as tests/lml_grad_reference_hp.py has them.
    a_i = sum_j |K^-1_ij yn_j|                              (the terms of alpha_i)
    resid: y_std a_i / kappa_i;   sigma: itself (one positive term);   kappa: itself (a sum of squares)
    lpd:   1/2 |log kappa_i| + 1/2 a_i^2 / kappa_i + 1/2 log(2 pi);   L_LOO: their sum
    grad:  the gradient's sums with S = |b| |alpha|^T + |alpha| |b|^T + 2 |K^-1| diag(w) |K^-1| in place of G

A platform whose long double is not at least the 64-bit-mantissa format makes the import fail, and with it every test
that uses the module.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

import cov_reference_hp as hp
import lml_grad_reference_hp as lr
from oracle import gp_oracle as G

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not an extended format here (eps %g): no reference" % np.finfo(LD).eps

PI = LD(4) * np.arctan(LD(1))
TILE = 64             # the column tile of the kappa kernel
CHUNK = 256           # its row chunk (LOO_ROWS of csrc/tgp_internal.hpp)
NPAD = 256            # N is padded to a multiple of this

SLIPS = ("padding rows counted in B",
         "a row chunk dropped",
         "the diagonal tile counted twice",
         "the jitter left out of sigma",
         "w without its 1/2",
         "G without symmetrisation")
GRAD_ONLY = ("padding rows counted in B", "w without its 1/2", "G without symmetrisation")


def _assemble(T, n, alpha, yn, Kinv, kappa, y_std, c, noise, Xs, kind, ard, w_factor=None, unsym=False, pad=0):
    """everything behind kappa, in the type T: dict of the quantities and their scales"""
    half = T(1) / T(2)
    log2pi = np.log(T(2) * PI) if T is LD else T(math.log(2 * math.pi))
    a_abs = np.abs(Kinv * yn[None, :]).sum(axis=1)
    p = alpha / kappa
    resid = y_std * p
    sigma = y_std / np.sqrt(kappa)
    lpd = half * np.log(kappa) - half * alpha * alpha / kappa - half * log2pi
    lpd_scale = half * np.abs(np.log(kappa)) + half * a_abs * a_abs / kappa + half * log2pi
    w = (half if w_factor is None else T(w_factor)) * (T(1) / kappa + p * p)
    b = Kinv @ p
    B = (Kinv * w[None, :]) @ Kinv
    Ka = np.abs(Kinv).astype(np.float64)           # (a scale is a denominator: f64 carries it, and BLAS forms it at once)
    Babs = ((Ka * w.astype(np.float64)[None, :]) @ Ka).astype(Kinv.dtype)
    if unsym:          # the lower triangle's b_i alpha_j taken for both halves
        i, j = np.indices((n, n))
        hi, lo = np.maximum(i, j), np.minimum(i, j)
        Gm = T(2) * b[hi] * alpha[lo] - T(2) * B
    else:
        Gm = np.outer(b, alpha) + np.outer(alpha, b) - T(2) * B
    S = np.outer(np.abs(b), np.abs(alpha)) + np.outer(np.abs(alpha), np.abs(b)) + T(2) * Babs
    (gc, gl, gt), (sc, sl, st) = lr._sums(Gm, S, Xs, kind, ard)
    if pad:            # a padding row has kappa = 1, alpha = 0, K^-1 = I there: w = 1/2, G_ii = -2 B_ii = -1, on k0_ii = 1
        gc, gt = gc - T(pad), gt - T(pad)
    grad = np.concatenate([[half * c * gc], half * c * gl, [half * noise * gt]]).astype(T)
    scale = np.concatenate([[half * c * sc], half * c * sl, [half * noise * st]]).astype(T)
    return dict(kappa=kappa, resid=resid, sigma=sigma, lpd=lpd, loo=lpd.sum(), grad=grad,
                kappa_scale=kappa, resid_scale=y_std * a_abs / kappa, sigma_scale=sigma, lpd_scale=lpd_scale,
                loo_scale=lpd_scale.sum(), grad_scale=scale)


def loo_and_grad(fit, y):
    """the dict of _assemble in long double, of the model in fit (a cov_reference_hp.Fit: ARD where it holds more than one
    length scale) with the raw targets y it was made of"""
    n = fit.L.shape[0]
    yn = (np.asarray(y, dtype=np.float64).astype(LD) - fit.y_mean) / fit.y_std
    Li = hp.forward(fit.L, np.eye(n, dtype=LD))
    kappa = (Li * Li).sum(axis=0)
    return _assemble(LD, n, fit.alpha, yn, Li.T @ Li, kappa, fit.y_std, fit.c, fit.noise, fit.Xs, fit.kind, fit.ls.shape[0] > 1)


def loo(X, y, kind, constant, length_scale, noise, jitter, normalize_y=True):
    """the 80-bit L_LOO alone with the normalisation HELD at that of (y, normalize_y) -- what the central differences are
    taken of: the hyper-parameters move, y_mean and y_std do not depend on them"""
    fit = hp.Fit(X, y, kind, constant, length_scale, noise, jitter, normalize_y)
    n = fit.L.shape[0]
    Li = hp.forward(fit.L, np.eye(n, dtype=LD))
    kappa = (Li * Li).sum(axis=0)
    half = LD(1) / LD(2)
    return (half * np.log(kappa) - half * fit.alpha * fit.alpha / kappa - half * np.log(LD(2) * PI)).sum()


def central_differences(X, y, kind, constant, length_scale, noise, jitter, normalize_y=True, step=2e-3):
    """d L_LOO / d log theta as lml_grad_reference_hp.central_differences takes the LML's: steps of step and step / 2,
    Richardson-extrapolated; theta = [constant, length scale(s), noise (left out where it is 0)]"""
    ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64))
    theta = np.concatenate([[float(constant)], ls, [float(noise)] if noise > 0 else []])
    out = np.zeros(len(theta), LD)

    def diff(p, h):
        v, t = [], []
        for sgn in (1.0, -1.0):
            th = theta.copy()
            th[p] = float(np.exp(np.log(LD(theta[p])) + LD(sgn * h)))
            t.append(np.log(LD(th[p])))
            l = th[1:1 + len(ls)]
            v.append(loo(X, y, kind, th[0], l if len(ls) > 1 else l[0], th[-1] if noise > 0 else 0.0, jitter, normalize_y))
        return (v[0] - v[1]) / (t[0] - t[1])

    for p in range(len(theta)):
        out[p] = (LD(4) * diff(p, step / 2) - diff(p, step)) / LD(3)
    return out


# ---- the same formulas in f64: NumPy and SciPy, with the slips the bars must reject ------------------------------------
def loo_and_grad_f64(X, y, kind, constant, length_scale, noise, jitter, normalize_y=True, slip=None):
    """the dict of _assemble in f64.  slip: one of SLIPS, the mutation the tests inject to show that the bars reject it;
    None is the honest computation."""
    assert slip is None or slip in SLIPS
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64))
    n = X.shape[0]
    yn, _, y_std = G.normalise_y(y, normalize_y)
    K = G.kernel_matrix(X, kind, constant, length_scale, noise, jitter)
    L = cholesky(K, lower=True, check_finite=False)
    alpha = solve_triangular(L.T, solve_triangular(L, yn, lower=True, check_finite=False), lower=False, check_finite=False)
    Li = np.tril(solve_triangular(L, np.eye(n), lower=True, check_finite=False))
    Kinv = Li.T @ Li
    sq = Li * Li
    kappa = sq.sum(axis=0)
    if slip == "a row chunk dropped":                  # the last chunk of 256 rows never reaches the partial sums
        kappa = sq[:(n - 1) // CHUNK * CHUNK].sum(axis=0)
    if slip == "the diagonal tile counted twice":
        t = np.arange(n) // TILE
        kappa = kappa + np.where(t[:, None] == t[None, :], sq, 0.0).sum(axis=0)
    if slip == "the jitter left out of sigma":         # the held-out deviation of a K without its jitter
        L0 = cholesky(K - jitter * np.eye(n), lower=True, check_finite=False)
        Li0 = solve_triangular(L0, np.eye(n), lower=True, check_finite=False)
        k0 = (Li0 * Li0).sum(axis=0)
    pad = (-n) % NPAD if slip == "padding rows counted in B" else 0
    with np.errstate(divide="ignore", invalid="ignore"):
        out = _assemble(np.float64, n, alpha, yn, Kinv, kappa, np.float64(y_std), np.float64(constant), np.float64(noise),
                        X / ls, kind, ls.shape[0] > 1, w_factor=1.0 if slip == "w without its 1/2" else None,
                        unsym=slip == "G without symmetrisation", pad=pad)
        if slip == "the jitter left out of sigma":
            out["sigma"] = np.float64(y_std) / np.sqrt(k0)
    return out
