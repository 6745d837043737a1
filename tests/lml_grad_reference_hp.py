"""Extended-precision (x87 80-bit, numpy.longdouble) closed form of the log marginal likelihood and its gradient with
respect to the LOG hyper-parameters (tgp_fit_grad; include/turbogp.h), and an f64 NumPy/SciPy restatement of the same
formulas that can be made to slip -- TEST INFRASTRUCTURE, written from the definitions below, not from the kernels.  The
80-bit form sits on tests/cov_reference_hp.py's Fit (L and alpha in long double) and tests/acq_grad_reference_hp.py's
h_weight.

    xs = x / l;  d2_ij = sum_d (xs_id - xs_jd)^2, dimension by dimension;  k0 = the unit kernel of d2, its diagonal 1
    K = c k0, its diagonal SET to c + noise + jitter;  L = chol(K);  yn the normalised targets;  alpha = K^-1 yn
    LML = -1/2 yn.alpha - sum_i log L_ii - N/2 log(2 pi)
    K^-1 = L^-T L^-1 (L^-1 = forward(L, I));  G = alpha alpha^T - K^-1
    dK/dlog c = c k0;   dK/dlog noise = noise I;   dK/dlog l (isotropic) = c h(r) d2;   dK/dlog l_d (ARD) = c h(r) (xs_id - xs_jd)^2
        h = exp(-d2 / 2) (RBF),  exp(-r) / r (Matern-1/2),  3 exp(-sqrt(3) r) (Matern-3/2),
            5/3 (1 + sqrt(5) r) exp(-sqrt(5) r) (Matern-5/2)
    grad = [1/2 c sum G o k0,   1/2 c sum G o h o d2   or, per d,   1/2 c sum G o h o (xs_d - xs'_d)^2,   1/2 noise tr G]
    A term with d2 = 0 contributes nothing to the length-scale sums: the diagonal, and a duplicated training row.  For
    three of the kernels that is what the formula says (the factor d2 is 0); for Matern-1/2, whose h is infinite there, it is
    the convention (ls_weight of the library; scikit-learn's K_gradient[~isfinite] = 0).

Scales.  Near an optimum every entry of the gradient is a cancellation: the sum of the absolute terms is 1e3 ... 1e6 times
the entry.  So an error is quoted as a fraction of the entry's SCALE, the same sum with |alpha_i alpha_j| + |K^-1_ij| in
place of G_ij (every other factor is non-negative), and the LML's as a fraction of
1/2 |yn.alpha| + sum_i |log L_ii| + N/2 log(2 pi).  A lost or twice-counted tile is then worth its share of the terms,
not its share of what is left after the cancellation.

A platform whose long double is not at least the 64-bit-mantissa format makes the import fail, and with it every test
that uses the module.
"""
import math

import numpy as np
from scipy.linalg import cholesky, solve_triangular

import acq_grad_reference_hp as ar
import cov_reference_hp as hp
from oracle import gp_oracle as G

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not an extended format here (eps %g): no reference" % np.finfo(LD).eps

PI = LD(4) * np.arctan(LD(1))
TILE = 64                                       # the pairwise tile of the library's gradient kernels (what two of the slips are about)

SLIPS = ("off-diagonal tiles counted once instead of twice",
         "the last training row left out of the sums",
         "dimensions >= 16 dropped from the ARD sums",
         "the last tile's rows beyond N - (N mod 64) dropped",
         "K^-1 from an f32-rounded inverse factor",
         "ls[0] for every dimension",
         "the diagonal in the length-scale sums with weight h(0)",
         "1/2 noise tr G with noise + jitter")
ARD_ONLY = ("dimensions >= 16 dropped from the ARD sums", "ls[0] for every dimension")


def _sums(Gm, S, Xs, kind, ard):
    """(sum G o k0, [sum G o h o d2] or [sum G o h o (xs_d - xs'_d)^2 for every d], tr G) and the same three with S in place of G;
    everything in the type of Xs"""
    T = Xs.dtype.type
    n, D = Xs.shape
    d2 = np.zeros((n, n), Xs.dtype)
    for d in range(D):
        t = Xs[:, d][:, None] - Xs[:, d][None, :]
        d2 += t * t
    k0 = hp.unit_kernel(d2, kind) if T is LD else ar._unit_kernel_f64(d2, kind)
    k0[np.diag_indices(n)] = T(1)
    h = ar.h_weight(d2, kind)                    # 0 where d2 is 0
    out = []
    for M in (Gm, S):
        w = M * h
        if ard:
            ls_sums = np.zeros(D, Xs.dtype)
            for d in range(D):
                t = Xs[:, d][:, None] - Xs[:, d][None, :]
                ls_sums[d] = (w * (t * t)).sum()
        else:
            ls_sums = np.array([(w * d2).sum()], dtype=Xs.dtype)
        out.append(((M * k0).sum(), ls_sums, np.trace(M)))
    return out


def lml_and_grad(fit, y):
    """dict(lml, grad (2 + n_ls,), lml_scale, grad_scale (2 + n_ls,)) in long double, of the model in fit (a
    cov_reference_hp.Fit: ARD where it holds more than one length scale) with the raw targets y it was made of"""
    n = fit.L.shape[0]
    half = LD(1) / LD(2)
    yn = (np.asarray(y, dtype=np.float64).astype(LD) - fit.y_mean) / fit.y_std
    logs = np.log(np.diag(fit.L))
    const = LD(n) / LD(2) * np.log(LD(2) * PI)
    ya = yn @ fit.alpha
    Li = hp.forward(fit.L, np.eye(n, dtype=LD))
    Kinv = Li.T @ Li
    aa = np.outer(fit.alpha, fit.alpha)
    ard = fit.ls.shape[0] > 1
    (gc, gl, gt), (sc, sl, st) = _sums(aa - Kinv, np.abs(aa) + np.abs(Kinv), fit.Xs, fit.kind, ard)
    grad = np.concatenate([[half * fit.c * gc], half * fit.c * gl, [half * fit.noise * gt]]).astype(LD)
    scale = np.concatenate([[half * fit.c * sc], half * fit.c * sl, [half * fit.noise * st]]).astype(LD)
    return dict(lml=-half * ya - logs.sum() - const, grad=grad,
                lml_scale=half * np.abs(ya) + np.abs(logs).sum() + const, grad_scale=scale)


def lml(X, y, kind, constant, length_scale, noise, jitter, normalize_y=True):
    """the 80-bit LML alone (what the central differences are taken of)"""
    fit = hp.Fit(X, y, kind, constant, length_scale, noise, jitter, normalize_y)
    yn = (np.asarray(y, dtype=np.float64).astype(LD) - fit.y_mean) / fit.y_std
    n = fit.L.shape[0]
    return -(yn @ fit.alpha) / LD(2) - np.log(np.diag(fit.L)).sum() - LD(n) / LD(2) * np.log(LD(2) * PI)


def central_differences(X, y, kind, constant, length_scale, noise, jitter, normalize_y=True, step=2e-3):
    """d LML / d log theta, theta = [constant, length scale(s), noise (left out where it is 0)], from the 80-bit LML:
    central differences of step and step / 2, Richardson-extrapolated (the error is of the order step^4).  The displaced
    hyper-parameters are f64 numbers; the difference is divided by the distance of their logarithms as they are."""
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
            v.append(lml(X, y, kind, th[0], l if len(ls) > 1 else l[0], th[-1] if noise > 0 else 0.0, jitter, normalize_y))
        return (v[0] - v[1]) / (t[0] - t[1])

    for p in range(len(theta)):
        out[p] = (LD(4) * diff(p, step / 2) - diff(p, step)) / LD(3)
    return out


# ---- the same formulas in f64: NumPy and SciPy, with the slips the bars must reject ------------------------------------
def _tile_weights(n, off_diagonal):
    """(n, n) of ones, off_diagonal on the entries whose two indices fall into different tiles of 64"""
    t = np.arange(n) // TILE
    return np.where(t[:, None] == t[None, :], 1.0, off_diagonal)


def lml_and_grad_f64(X, y, kind, constant, length_scale, noise, jitter, normalize_y=True, slip=None, with_scale=False):
    """(lml, grad (2 + n_ls,)) in f64 -- and (lml scale, grad scale) behind them where with_scale.  slip: one of SLIPS, the
    mutation the tests inject into the gradient's sums to show that the bars reject it; None is the honest computation."""
    assert slip is None or slip in SLIPS
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64))
    ard = ls.shape[0] > 1
    assert ard or slip not in ARD_ONLY
    n, D = X.shape
    yn, _, _ = G.normalise_y(y, normalize_y)
    K = G.kernel_matrix(X, kind, constant, length_scale, noise, jitter)
    L = cholesky(K, lower=True, check_finite=False)
    z = solve_triangular(L, yn, lower=True, check_finite=False)
    alpha = solve_triangular(L.T, z, lower=False, check_finite=False)
    logs = np.log(np.diag(L))
    const = n / 2 * math.log(2 * math.pi)
    ya = float(yn @ alpha)
    Li = solve_triangular(L, np.eye(n), lower=True, check_finite=False)
    if slip == "K^-1 from an f32-rounded inverse factor":
        Li = Li.astype(np.float32).astype(np.float64)
    Kinv = Li.T @ Li
    aa = np.outer(alpha, alpha)
    Gm, S = aa - Kinv, np.abs(aa) + np.abs(Kinv)
    Xs = X / (ls[0] if slip == "ls[0] for every dimension" else ls)
    if slip == "off-diagonal tiles counted once instead of twice":
        Gm = Gm * _tile_weights(n, 0.5)
    keep = n
    if slip == "the last training row left out of the sums":
        keep = n - 1
    if slip == "the last tile's rows beyond N - (N mod 64) dropped":
        keep = n - n % TILE
    (gc, gl, gt), (sc, sl, st) = _sums(Gm[:keep, :keep], S[:keep, :keep], Xs[:keep], kind, ard)
    if slip == "the diagonal in the length-scale sums with weight h(0)":
        with np.errstate(divide="ignore", invalid="ignore"):
            h0 = {"rbf": 1.0, "matern12": np.inf, "matern32": 3.0, "matern52": 5.0 / 3.0}[kind]
            gl = gl + np.trace(Gm) * h0 * 0.0              # h(0) times the term's own d2 = 0
    if slip == "dimensions >= 16 dropped from the ARD sums":
        gl = np.where(np.arange(D) < 16, gl, 0.0)
    tr_noise = noise + jitter if slip == "1/2 noise tr G with noise + jitter" else noise
    grad = np.concatenate([[0.5 * constant * gc], 0.5 * constant * gl, [0.5 * tr_noise * gt]])
    lml_value = -0.5 * ya - float(logs.sum()) - const
    if not with_scale:
        return lml_value, grad
    scale = np.concatenate([[0.5 * constant * sc], 0.5 * constant * sl, [0.5 * noise * st]])
    return lml_value, grad, 0.5 * abs(ya) + float(np.abs(logs).sum()) + const, scale
