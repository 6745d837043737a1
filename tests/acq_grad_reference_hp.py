"""Extended-precision (x87 80-bit, numpy.longdouble) closed form of the acquisition value and its gradient with respect
to the query point (tgp_acq_grad; include/turbogp.h), and an f64 NumPy/SciPy restatement of the same formulas -- TEST
INFRASTRUCTURE, written from the definitions below, not from the library.  The 80-bit form sits on
tests/cov_reference_hp.py's Fit (L and alpha in long double); the f64 one takes oracle.gp_oracle.fit's model.

    u = x / l;  d2_j = sum_d (u_d - xs_jd)^2;  r_j = sqrt(d2_j);  k_j = c k0(d2_j)
    dk_j/dx_d = -c h(r_j) (u_d - xs_jd) / l_d
        h = exp(-d2 / 2) (RBF),  exp(-r) / r (Matern-1/2),  3 exp(-sqrt(3) r) (Matern-3/2),
            5/3 (1 + sqrt(5) r) exp(-sqrt(5) r) (Matern-5/2)
    A term with r_j = 0 contributes nothing.  For three of the kernels that is what the formula says ((u_d - xs_jd) = 0);
    for Matern-1/2, whose k has a kink at a training point, it is the documented convention (csrc/query_math.hpp): the
    gradient there is the gradient of the sum of the other terms.
    mu = y_mean + y_std k.alpha                 dmu/dx_d  = -y_std / l_d sum_j alpha_j c h_j (u_d - xs_jd)
    v = L^-1 k;  w = L^-T v;  var = (c + noise) - v.v   (OBSERVED: the noise is in, the jitter is not -- what
                                                         oracle.gp_oracle.predict does; a negative var is 0)
                                                dvar/dx_d = +2 / l_d sum_j w_j c h_j (u_d - xs_jd)
    sigma = y_std sqrt(var)                     dsigma    = y_std dvar / (2 sqrt(var))   (0 where var is 0)

Acquisitions as oracle.gp_oracle.acquisition defines the values, sf = +1 (max) or -1 (min), with their partials:
d acq = cm dmu + cs dsigma.
    "mu"     mu                                         cm = 1,               cs = 0
    "sigma"  sigma  (UCB with beta = inf)               cm = 0,               cs = 1
    "ucb"    sf mu + beta sigma                         cm = sf,              cs = beta
    "pi"     Phi(Z), Z = (sf (mu - inc) - xi) / sigma   cm = sf pdf(Z)/sigma, cs = -pdf(Z) Z / sigma    (0 at sigma = 0)
    "ei"     diff Phi(Z) + sigma pdf(Z)                 cm = sf Phi(Z),       cs = pdf(Z)               (0 at sigma = 0)

Phi in long double is this module's own erfc (NumPy has none): the all-positive series of erf below |x| = 1, the
continued fraction of erfc beyond.  tests/test_acq_grad_reference.py holds it to scipy.special.ndtr and to mpmath.

A platform whose long double is not at least the 64-bit-mantissa format makes the import fail, and with it every test
that uses the module.
"""
import math

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import ndtr

import cov_reference_hp as hp

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not an extended format here (eps %g): no reference" % np.finfo(LD).eps

QUANTITIES = ("mu", "sigma", "ucb", "pi", "ei")
SLIPS = ("query points rounded to f32", "ls[0] for every dimension", "the last training point left out of the gradient sums",
         "w from an f32-rounded inverse factor", "the latent variance", "cs of PI without its Z", "the sign of dvar flipped")

PI = LD(4) * np.arctan(LD(1))
SQRT_PI, SQRT2, SQRT_2PI = np.sqrt(PI), np.sqrt(LD(2)), np.sqrt(LD(2) * PI)
_SERIES_TERMS, _CF_TERMS, _SWITCH = 60, 400, LD(1)


def erfc(x):
    """erfc of a long double array, to a few long double ulps of the result for |x| below the underflow of exp(-x^2)
    (relative to erfc, the tails included; a rounding of the argument is worth 2 x^2 of them and is not in that figure)
        |x| <  1   1 - erf,  erf(x) = 2 / sqrt(pi) exp(-x^2) sum_n 2^n x^(2n+1) / (1 3 5 ... (2n+1)): every term positive
        |x| >= 1   exp(-x^2) / sqrt(pi) / (x + (1/2) / (x + (2/2) / (x + (3/2) / (x + ...)))), evaluated from its tail
                   (400 terms: 800 give the same bits at x = 1, where it converges slowest)
        x < 0      2 - erfc(-x)"""
    x = np.atleast_1d(np.asarray(x, dtype=LD))
    a = np.abs(x)
    out = np.empty(a.shape, LD)
    near = a < _SWITCH
    if near.any():
        z = a[near]
        z2 = z * z
        term = z.copy()
        s = z.copy()
        for n in range(1, _SERIES_TERMS):
            term = term * (LD(2) * z2) / LD(2 * n + 1)
            s = s + term
        out[near] = LD(1) - LD(2) / SQRT_PI * np.exp(-z2) * s
    far = ~near
    if far.any():
        z = a[far]
        f = z.copy()
        for n in range(_CF_TERMS, 0, -1):
            f = z + (LD(n) / LD(2)) / f
        out[far] = np.exp(-z * z) / SQRT_PI / f
    neg = x < 0
    out[neg] = LD(2) - out[neg]
    return out


def Phi(z):
    """the standard normal distribution function in long double"""
    z = np.asarray(z, dtype=LD)
    return (erfc((-z / SQRT2).reshape(-1)) / LD(2)).reshape(z.shape)


def pdf(z):
    z = np.asarray(z, dtype=LD)
    return np.exp(-(z * z) / LD(2)) / SQRT_2PI


def h_weight(d2, kind):
    """h(r) of the module docstring for an array of d2 (long double or f64: the constants take the array's type);
    0 where d2 is 0"""
    T = d2.dtype.type
    if kind == "rbf":
        h = np.exp(T(-0.5) * d2)
    else:
        r = np.sqrt(d2)
        if kind == "matern12":
            h = np.exp(-r) / np.where(r > 0, r, T(1))
        elif kind == "matern32":
            h = T(3) * np.exp(-np.sqrt(T(3)) * r)
        elif kind == "matern52":
            t = np.sqrt(T(5)) * r
            h = T(5) / T(3) * (T(1) + t) * np.exp(-t)
        else:
            raise ValueError(kind)
    return np.where(d2 > 0, h, T(0))


def backward_columns(L, B):
    """L^-T B for B (n, k) in long double, row by row from the last"""
    X = np.zeros(B.shape, LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (B[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def _ls_full(ls, D):
    return np.broadcast_to(ls, (D,)) if ls.shape[0] == 1 else ls


def posterior_values(fit, Xq):
    """(mu, sigma) (m,) in long double: the values alone (what the central differences are taken of)"""
    Q = np.atleast_2d(np.asarray(Xq, dtype=LD)) / fit.ls
    k = fit.c * hp.unit_kernel(hp.sqdist(Q, fit.Xs), fit.kind)
    V = hp.forward(fit.L, np.ascontiguousarray(k.T))
    var = (fit.c + fit.noise) - (V * V).sum(0)
    var = np.where(var > 0, var, LD(0))
    return fit.y_mean + fit.y_std * (k @ fit.alpha), fit.y_std * np.sqrt(var)


def posterior(fit, Xq):
    """dict(mu, sigma (m,), dmu, dsigma (m, D)) in long double"""
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    m, D = Xq.shape
    l = _ls_full(fit.ls, D)
    Q = Xq.astype(LD) / fit.ls
    d2 = hp.sqdist(Q, fit.Xs)
    k = fit.c * hp.unit_kernel(d2, fit.kind)
    ch = fit.c * h_weight(d2, fit.kind)
    V = hp.forward(fit.L, np.ascontiguousarray(k.T))                 # (N, m)
    W = backward_columns(fit.L, V)
    var = (fit.c + fit.noise) - (V * V).sum(0)
    pos = var > 0
    var = np.where(pos, var, LD(0))
    sn = np.sqrt(var)
    ta, tw = ch * fit.alpha[None, :], ch * W.T                       # (m, N)
    dmu, dvar = np.zeros((m, D), LD), np.zeros((m, D), LD)
    for d in range(D):
        diff = Q[:, d][:, None] - fit.Xs[:, d][None, :]
        dmu[:, d] = -fit.y_std / l[d] * (ta * diff).sum(1)
        dvar[:, d] = LD(2) / l[d] * (tw * diff).sum(1)
    dsigma = np.where(pos[:, None], fit.y_std * dvar / (LD(2) * np.where(pos, sn, LD(1)))[:, None], LD(0))
    return dict(mu=fit.y_mean + fit.y_std * (k @ fit.alpha), sigma=fit.y_std * sn, dmu=dmu, dsigma=dsigma)


def acquisition(q, mu, sigma, sf=1.0, incumbent=0.0, param=0.0, dmu=None, dsigma=None):
    """value (m,) and, where dmu and dsigma are given, gradient (m, D) of quantity q in long double (gradient None
    otherwise); param is beta (ucb; inf: sigma) or xi (pi, ei)"""
    mu, sigma = np.asarray(mu, dtype=LD), np.asarray(sigma, dtype=LD)
    sf = LD(sf)
    one, zero = np.ones(mu.shape, LD), np.zeros(mu.shape, LD)
    if q == "mu":
        a, cm, cs = mu, one, zero
    elif q == "sigma" or (q == "ucb" and math.isinf(param)):
        a, cm, cs = sigma, zero, one
    elif q == "ucb":
        a, cm, cs = sf * mu + LD(param) * sigma, sf * one, LD(param) * one
    elif q in ("pi", "ei"):
        on = sigma != 0
        s = np.where(on, sigma, LD(1))
        diff = sf * (mu - LD(incumbent)) - LD(param)
        Z = diff / s
        cdf, p = Phi(Z), pdf(Z)
        if q == "pi":
            a, cm, cs = cdf, sf * p / s, -p * Z / s
        else:
            a, cm, cs = diff * cdf + s * p, sf * cdf, p
        a, cm, cs = np.where(on, a, zero), np.where(on, cm, zero), np.where(on, cs, zero)
    else:
        raise ValueError(q)
    if dmu is None:
        return a, None
    return a, cm[:, None] * dmu + cs[:, None] * dsigma


def central_differences(fit, Xq, step=1e-5):
    """(dmu, dsigma) (m, D) as central differences, step in x, of the 80-bit VALUES -- and the values (mup, mum, sgp, sgm)
    (m, D) at the displaced points, so that every acquisition's own difference can be formed from them"""
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64)).astype(LD)
    m, D = Xq.shape
    P = np.repeat(Xq[:, None, :], 2 * D, axis=1)                     # (m, 2 D, D)
    for d in range(D):
        P[:, 2 * d, d] += LD(step)
        P[:, 2 * d + 1, d] -= LD(step)
    mu, sg = posterior_values(fit, P.reshape(-1, D))
    mu, sg = mu.reshape(m, D, 2), sg.reshape(m, D, 2)
    return mu[..., 0], mu[..., 1], sg[..., 0], sg[..., 1]


# ---- the same formulas in f64: NumPy, solve_triangular, ndtr, on oracle.gp_oracle.fit's model -----------------------------
def posterior_f64(model, Xq, slip=None):
    """dict(mu, sigma, dmu, dsigma) in f64.  slip: one of SLIPS (but PI's) -- the mutation the tests inject to show
    that the bars reject it; None is the honest computation."""
    assert slip is None or slip in SLIPS
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    if slip == "query points rounded to f32":
        Xq = Xq.astype(np.float32).astype(np.float64)
    m, D = Xq.shape
    c, ys = model.constant, model.y_std
    l = np.broadcast_to(model.length_scale, (D,)) if model.length_scale.shape[0] == 1 else model.length_scale
    Q, Xs = Xq / l, model.X / l
    diff = Q[:, None, :] - Xs[None, :, :]                            # (m, N, D)
    d2 = (diff * diff).sum(-1)
    k = c * _unit_kernel_f64(d2, model.kind)
    ch = c * h_weight(d2, model.kind)
    V = solve_triangular(model.L, k.T, lower=True, check_finite=False)
    if slip == "w from an f32-rounded inverse factor":
        Li = solve_triangular(model.L, np.eye(model.L.shape[0]), lower=True, check_finite=False)
        W = Li.astype(np.float32).astype(np.float64).T @ V
    else:
        W = solve_triangular(model.L.T, V, lower=False, check_finite=False)
    kss = c if slip == "the latent variance" else c + model.noise
    var = kss - (V * V).sum(0)
    pos = var > 0
    var = np.where(pos, var, 0.0)
    sn = np.sqrt(var)
    ta, tw = ch * model.alpha[None, :], ch * W.T
    if slip == "the last training point left out of the gradient sums":
        ta, tw, diff = ta[:, :-1], tw[:, :-1], diff[:, :-1]
    ld = np.full(D, l[0]) if slip == "ls[0] for every dimension" else l
    dmu = -ys / ld * np.einsum("qj,qjd->qd", ta, diff)
    dvar = 2.0 / ld * np.einsum("qj,qjd->qd", tw, diff)
    if slip == "the sign of dvar flipped":
        dvar = -dvar
    dsigma = np.where(pos[:, None], ys * dvar / (2.0 * np.where(pos, sn, 1.0))[:, None], 0.0)
    return dict(mu=model.y_mean + ys * (k @ model.alpha), sigma=ys * sn, dmu=dmu, dsigma=dsigma)


def _unit_kernel_f64(d2, kind):
    if kind == "rbf":
        return np.exp(-0.5 * d2)
    r = np.sqrt(d2)
    if kind == "matern12":
        return np.exp(-r)
    t = r * math.sqrt(3.0 if kind == "matern32" else 5.0)
    return (1.0 + t) * np.exp(-t) if kind == "matern32" else (1.0 + t + t * t / 3.0) * np.exp(-t)


def acquisition_f64(q, post, sf=1.0, incumbent=0.0, param=0.0, slip=None):
    """(value (m,), gradient (m, D)) of quantity q in f64 from posterior_f64's dict"""
    mu, sigma = post["mu"], post["sigma"]
    one, zero = np.ones_like(mu), np.zeros_like(mu)
    if q == "mu":
        a, cm, cs = mu, one, zero
    elif q == "sigma" or (q == "ucb" and math.isinf(param)):
        a, cm, cs = sigma, zero, one
    elif q == "ucb":
        a, cm, cs = sf * mu + param * sigma, sf * one, param * one
    elif q in ("pi", "ei"):
        on = sigma != 0
        s = np.where(on, sigma, 1.0)
        diff = sf * (mu - incumbent) - param
        Z = diff / s
        cdf, p = ndtr(Z), np.exp(-Z * Z / 2.0) / math.sqrt(2.0 * math.pi)
        if q == "pi":
            a, cm, cs = cdf, sf * p / s, (-p / s if slip == "cs of PI without its Z" else -p * Z / s)
        else:
            a, cm, cs = diff * cdf + s * p, sf * cdf, p
        a, cm, cs = np.where(on, a, 0.0), np.where(on, cm, 0.0), np.where(on, cs, 0.0)
    else:
        raise ValueError(q)
    return a, cm[:, None] * post["dmu"] + cs[:, None] * post["dsigma"]
