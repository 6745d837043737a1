"""Extended-precision (x87 80-bit, numpy.longdouble) statement of max-value entropy search -- TEST INFRASTRUCTURE, written
from the definition, sharing nothing with tests/mes_reference.py (the f64 restatement of the device's branches) but that
definition:

    sigma_f^2 = sigma^2 - noise_var  (a row with sigma_f^2 <= 0 has a = da/dmu = da/dsigma = 0)
    gamma_s   = sf (y*_s - mu) / sigma_f
    h(gamma)  = gamma phi / (2 Phi) - log Phi,     dh/dgamma = -(r / 2)(1 + gamma^2 + gamma r),  r = phi / Phi
    a = (1/S) sum_s h(gamma_s),   da/dmu = -sf / (S sigma_f) sum_s dh_s,   da/dsigma = -sigma / (S sigma_f^2) sum_s gamma_s dh_s

How h and dh are formed, so that neither loses more than a few long double ulps anywhere:
    gamma <  -1   x = -gamma and Laplace's continued fraction T_k = x + k / T_(k+1), from its tail (CF_TERMS = 1600 terms: T_2 and
                  T_3 converge more slowly than T_1, and with 400 dh is 87 ulps off at x = 1.05; with 1600 it is 0.3):  r = T_1,
                  1 + gamma^2 + gamma r = 2 / (T_2 T_3),  so   dh = -(T_1 / T_2) / T_3   and
                  h = log sqrt(2 pi) + log T_1 - x / (2 T_2).   The textbook forms lose gamma^2 (h) and gamma^4 (dh) ulps
                  in long double too -- 3e-13 of dh at gamma = -50, 4e-16 at -8 -- so the fraction is used from -1 down
                  (between -8 and -1 it is the better of two valid forms).
                  It needs no exp, so it holds to -1e300 and beyond.
    -1 <= gamma <= 0   Phi = erfc(-gamma / sqrt 2) / 2 (tests/acq_grad_reference_hp.py's erfc), the textbook forms: there
                  1 + gamma^2 + gamma r >= 0.47 and nothing cancels.
    gamma >  0    Q = 1 - Phi,  log Phi = log1p(-Q)  (log(1 - Q) would lose Q beyond gamma = 9),  r = phi / (1 - Q):
                  h = gamma r / 2 + (-log1p(-Q)) and dh = -(r / 2)(1 + gamma^2 + gamma r) are sums of positive terms.
                  Q = erfc(gamma / sqrt 2) / 2 up to gamma = 1.  Beyond, erfc's own exp(-z^2) at the ROUNDED z = gamma / sqrt 2
                  would cost gamma^2 / 2 ulps (700 at gamma = 38), so Q = phi(gamma) / T_1(gamma) -- the fraction erfc itself
                  uses there -- with phi from an exact square: gamma = a + b with a of 24 bits, a^2 / 2 exact, and
                  phi = exp(-a^2 / 2) exp(-(a b + b^2 / 2)) / sqrt(2 pi).
                  Beyond gamma = 150 phi underflows in long double and h = dh = 0: the true values are below 1e-4900.

Every function returns long double.  coefficients() also returns the per-row scales the bars are fractions of
(tests/mes_edge_cases.py):  a itself (every h_s >= 0),  (1 / (S sigma_f)) sum |dh_s|,  (sigma / (S sigma_f^2)) sum |gamma_s dh_s|.
"""
import numpy as np

import acq_grad_reference_hp as ar

LD = ar.LD
CF_TERMS = 1600
CF_FROM = LD(-1)
LOG_SQRT_2PI = np.log(ar.SQRT_2PI)


def _cf(x):
    """(T_1, T_2, T_3) of Laplace's continued fraction at x > 1, from T_(n+1) = x with n = CF_TERMS below x = 3, 256 below
    8 and 64 beyond (the truncation falls like exp(-2 x sqrt(2 n)): below 1e-50 in each tier)"""
    t1, t2, t3 = (np.empty(x.shape, LD) for _ in range(3))
    for lo, hi, n in ((LD(0), LD(3), CF_TERMS), (LD(3), LD(8), 256), (LD(8), LD(np.inf), 64)):
        m = (x >= lo) & (x < hi) if np.isfinite(hi) else (x >= lo)
        if not m.any():
            continue
        xm = x[m]
        t = xm.copy()
        for k in range(n, 3, -1):
            t = xm + LD(k) / t
        c = xm + LD(3) / t
        b = xm + LD(2) / c
        t1[m], t2[m], t3[m] = xm + LD(1) / b, b, c
    return t1, t2, t3


def _pdf(g):
    """phi(g) for f64-valued g in long double, to a few ulps at any size: the square is formed exactly"""
    a = g.astype(np.float32).astype(LD)
    b = g - a
    return np.exp(-(a * a) / LD(2)) * np.exp(-(a * b + b * b / LD(2))) / ar.SQRT_2PI


def h_dh(gamma):
    """(h, dh/dgamma), elementwise, long double"""
    g = np.atleast_1d(np.asarray(gamma, dtype=LD))
    shape = g.shape
    g = g.reshape(-1)
    h, dh = np.zeros(g.shape, LD), np.zeros(g.shape, LD)
    with np.errstate(all="ignore"):
        low = g < CF_FROM
        if low.any():
            x = -g[low]
            t1, t2, t3 = _cf(x)
            dh[low] = -(t1 / t2) / t3
            h[low] = LOG_SQRT_2PI + np.log(t1) - (x / t2) / LD(2)
        mid = ~low & (g <= 0)
        if mid.any():
            gm = g[mid]
            P = ar.Phi(gm)
            r = ar.pdf(gm) / P
            h[mid] = gm * r / LD(2) - np.log(P)
            dh[mid] = -(r / LD(2)) * (LD(1) + gm * gm + gm * r)
        pos = g > 0
        if pos.any():
            gp = g[pos]
            far = gp > LD(150)                       # phi underflows: h = dh = 0 (erfc's own domain ends here)
            gq = np.where(far, LD(1), gp)
            near = gq <= LD(1)
            p = _pdf(gq)
            Q = np.where(near, ar.erfc(np.where(near, gq, LD(1)) / ar.SQRT2) / LD(2), p / _cf(np.where(near, LD(2), gq))[0])
            r = p / (LD(1) - Q)
            hv = gq * r / LD(2) + (-np.log1p(-Q))
            dv = -(r / LD(2)) * (LD(1) + gq * gq + gq * r)
            h[pos] = np.where(far, LD(0), hv)
            dh[pos] = np.where(far, LD(0), dv)
    return h.reshape(shape), dh.reshape(shape)


def gammas(mu, sigma, ystar, sf, noise_var):
    """(gamma (M, S), sigma_f^2 (M,), live (M,)) in long double; gamma is 0 in the rows that are not live"""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1).astype(LD)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1).astype(LD)
    ys = np.asarray(ystar, dtype=np.float64).astype(LD)
    ys = np.broadcast_to(ys.reshape(1, -1), (mu.shape[0], ys.size)) if ys.ndim <= 1 else ys      # (M, S): maxima per row allowed
    v = sigma * sigma - np.asarray(noise_var, dtype=np.float64).astype(LD)
    live = v > 0
    sl = np.sqrt(np.where(live, v, LD(1)))
    with np.errstate(all="ignore"):
        g = LD(sf) * (ys - mu[:, None]) / sl[:, None]
    return np.where(live[:, None], g, LD(0)), v, live


def coefficients(mu, sigma, ystar, sf, noise_var):
    """(a, da/dmu, da/dsigma), (scale_a, scale_dmu, scale_dsigma), gamma (M, S) -- long double; noise_var is
    noise y_std^2 (a scalar or one per row), ystar (S,) or one set per row (M, S)"""
    g, v, live = gammas(mu, sigma, ystar, sf, noise_var)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1).astype(LD)
    S = LD(g.shape[1])
    h, dh = h_dh(g)
    vs = np.where(live, v, LD(1))
    sl = np.sqrt(vs)
    zero = np.zeros(live.shape, LD)
    a = np.where(live, h.sum(1) / S, zero)
    cm = np.where(live, -LD(sf) * dh.sum(1) / (sl * S), zero)
    cs = np.where(live, -(g * dh).sum(1) * sigma / (vs * S), zero)
    s_m = np.where(live, np.abs(dh).sum(1) / (sl * S), zero)
    s_s = np.where(live, np.abs(g * dh).sum(1) * sigma / (vs * S), zero)
    return (a, cm, cs), (a, s_m, s_s), g


def mes(mu, sigma, ystar, sf, noise_var):
    """a (M,) in long double"""
    return coefficients(mu, sigma, ystar, sf, noise_var)[0][0]
