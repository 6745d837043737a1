"""NumPy reference of the constrained / cost-aware acquisition (tgp_sweep_weighted, tgp_weighted_grad; include/turbogp.h)
-- TEST INFRASTRUCTURE, written from the definitions in the header, not from the library.  Everything here is a pure
function of per-model posteriors (mu, sigma and, for the gradient, their partials) and works in the arrays' own precision:
float64 arrays take log Phi from ``scipy.special.log_ndtr``, numpy.longdouble arrays from tests/acq_grad_reference_hp.py's
80-bit erfc.  ``logphi_mp`` is the mpmath form the f64 one is held to (tests/test_weighted_reference.py; its worst
relative error e_ref is tests/golden/weighted_eref.json, written by tests/golden/make_golden_weighted.py).

    GE:    log f = log Phi((mu - level) / sigma)        LE:  log f = log Phi((level - mu) / sigma)
           sigma == 0: 0 where the inequality holds (equality included), else -inf
    COST:  log f = -mu
    logw  = sum_k log f_k (k = 0, 1, ...);  a = the objective's EI / PI
    value = a exp(logw) (EI / PI; exactly 0 where a == 0 or logw == -inf),  logw (ACQ_NONE);  NaN where any mu / sigma is NaN
    grad  = (prod f) grad a + a sum_k (prod_{j != k} f_j) grad f_k   (EI / PI),   sum_k (phi / Phi)(z_k) grad z_k   (NONE)
"""
import math

import numpy as np
from scipy.special import log_ndtr

GE, LE, COST = 0, 1, 2
ACQ_NONE, ACQ_PI, ACQ_EI = 0, 2, 3
LD = np.longdouble
U = 2.0 ** -53            # the f64 unit roundoff
TINY = float(np.finfo(np.float64).tiny)   # a magnitude below the smallest normal double has no f64 representation: errors are
                                          # taken relative to max(|reference|, TINY)
FACTOR = 64.0             # the project's margin (tests/test_gpu_lml_grad_edges.py)
Z_SET = (-1e150, -1e5, -40.0, -38.5, -10.0, -1.0, 0.0, 1.0, 9.0, 40.0)


def logphi_mp(z):
    """log Phi(z) by mpmath at 60 digits, as an mpf (z > 0 through log1p of the other tail)"""
    import mpmath as mp
    with mp.workdps(60):
        z = mp.mpf(float(z))
        return mp.log1p(-mp.ncdf(-z)) if z > 0 else mp.log(mp.ncdf(z))


def _erfcx_cf(x):
    """exp(x^2) erfc(x) for long double x >= 1: the continued fraction of tests/acq_grad_reference_hp.py's erfc without its
    exponential"""
    import acq_grad_reference_hp as ah
    f = x.copy()
    for n in range(ah._CF_TERMS, 0, -1):
        f = x + (LD(n) / LD(2)) / f
    return LD(1) / (ah.SQRT_PI * f)


def logphi(z):
    """(log Phi(z), phi(z) / Phi(z)) in z's precision"""
    z = np.asarray(z)
    if z.dtype == LD:
        # Phi(-|z|), the tail that is small, as t exp(-z^2 / 2) with t = erfcx(|z| / sqrt 2) / 2: nothing underflows
        import acq_grad_reference_hp as ah
        a = np.abs(z)
        with np.errstate(over="ignore", under="ignore", divide="ignore", invalid="ignore"):
            t = np.where(a < LD(2), ah.Phi(-np.minimum(a, LD(2))) * np.exp(np.minimum(a, LD(2)) ** 2 / LD(2)), _erfcx_cf(np.maximum(a, LD(2)) / ah.SQRT2) / LD(2))
            ltail = np.log(t) - a * a / LD(2)
            lp = np.where(z > 0, np.log1p(-np.exp(ltail)), ltail)
            ratio = np.where(z > 0, ah.pdf(z) / np.exp(lp), LD(1) / (t * ah.SQRT_2PI))
        return lp, ratio
    z = z.astype(np.float64)
    from scipy.special import erfcx, ndtr
    lp = log_ndtr(z)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):      # (exp(-z^2 / 2 - log Phi) would lose z^2 ulps)
        ratio = np.where(z <= 0, math.sqrt(2.0 / math.pi) / erfcx(-np.minimum(z, 0.0) / math.sqrt(2.0)),
                         np.exp(-0.5 * z * z) / (math.sqrt(2.0 * math.pi) * ndtr(np.maximum(z, 0.0))))
    return lp, ratio


def side_z(kind, level, mu, sigma):
    T = np.asarray(mu).dtype.type
    s = np.where(sigma != 0, sigma, T(1))
    return ((mu - T(level)) if kind == GE else (T(level) - mu)) / s


def side_logf(kind, level, mu, sigma):
    """log f_k (M,) of one side from its posterior"""
    mu, sigma = np.asarray(mu), np.asarray(sigma)
    T = mu.dtype.type
    bad = np.isnan(mu) | np.isnan(sigma)
    if kind == COST:
        out = -mu
    else:
        lp, _ = logphi(side_z(kind, level, mu, sigma))
        holds = (mu >= T(level)) if kind == GE else (mu <= T(level))
        step = np.where(holds, T(0), T(-np.inf))
        out = np.where(sigma == 0, step, lp)
    return np.where(bad, T(np.nan), out)


def acq_value(acq, sf, incumbent, param, mu, sigma):
    """the objective's unweighted EI / PI (0 for ACQ_NONE), 0 where sigma == 0"""
    mu, sigma = np.asarray(mu), np.asarray(sigma)
    T = mu.dtype.type
    if acq == ACQ_NONE:
        return np.zeros(mu.shape, mu.dtype)
    if mu.dtype == LD:
        import acq_grad_reference_hp as ah
        return ah.acquisition("ei" if acq == ACQ_EI else "pi", mu, sigma, sf, incumbent, param)[0]
    from scipy.special import ndtr
    on = sigma != 0
    s = np.where(on, sigma, T(1))
    diff = sf * (mu - incumbent) - param
    Z = diff / s
    a = ndtr(Z) if acq == ACQ_PI else diff * ndtr(Z) + s * np.exp(-Z * Z / 2.0) / math.sqrt(2.0 * math.pi)
    return np.where(on, a, 0.0)


def value_of(acq, a, logw, mu, sigma):
    T = np.asarray(logw).dtype.type
    bad = np.isnan(mu) | np.isnan(sigma) | np.isnan(logw) | np.isnan(a)
    if acq == ACQ_NONE:
        v = np.asarray(logw).copy()
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.where((a == 0) | (logw == -np.inf), T(0), a * np.exp(logw))
    return np.where(bad, T(np.nan), v)


def argmax(value):
    """the library-wide rule: the largest value, the lowest index on ties, NaN never wins (all NaN: index 0, -inf)"""
    v = np.where(np.isnan(value), -np.inf, np.asarray(value, dtype=np.float64))
    i = int(np.argmax(v))
    return i, float(v[i])


def sweep(acq, sf, incumbent, param, mu, sigma, sides):
    """sides: [(kind, level, mu_k (M,), sigma_k (M,)), ...] -> dict(logf (K, M), logw, acq, value (M,), best_idx, best_val)"""
    mu, sigma = np.asarray(mu), np.asarray(sigma)
    logf = np.zeros((len(sides), mu.shape[0]), mu.dtype)
    logw = np.zeros(mu.shape, mu.dtype)
    for k, (kind, level, mk, sk) in enumerate(sides):
        logf[k] = side_logf(kind, level, np.asarray(mk, dtype=mu.dtype), np.asarray(sk, dtype=mu.dtype))
        logw = logf[k].copy() if k == 0 else logw + logf[k]
    a = acq_value(acq, sf, incumbent, param, mu, sigma)
    value = value_of(acq, a, logw, mu, sigma)
    bi, bv = argmax(value)
    return dict(logf=logf, logw=logw, acq=a, value=value, best_idx=bi, best_val=bv)


def bound(logf, e_ref):
    """the pure-function bar on logw (M,): 64 max(e_ref, u) sum_k (1 + |log f_k|) -- z carries about 2 u of relative error,
    which costs at most 4 u |log Phi| in the tail and about u elsewhere; value is held to value (that + 4 u)"""
    lf = np.abs(np.where(np.isfinite(logf), logf, 0.0)).astype(np.float64)
    return FACTOR * max(e_ref, U) * (1.0 + lf).sum(0)


def acq_coef(acq, sf, incumbent, param, mu, sigma):
    """(a, cm, cs): the objective's value and its partials in mu and sigma"""
    T = mu.dtype.type
    if mu.dtype == LD:
        import acq_grad_reference_hp as ah
        cdf_pdf = lambda Z: (ah.Phi(Z), ah.pdf(Z))
    else:
        from scipy.special import ndtr
        cdf_pdf = lambda Z: (ndtr(Z), np.exp(-Z * Z / 2.0) / math.sqrt(2.0 * math.pi))
    on = sigma != 0
    s = np.where(on, sigma, T(1))
    diff = T(sf) * (mu - T(incumbent)) - T(param)
    Z = diff / s
    cdf, p = cdf_pdf(Z)
    if acq == ACQ_PI:
        a, cm, cs = cdf, T(sf) * p / s, -p * Z / s
    else:
        a, cm, cs = diff * cdf + s * p, T(sf) * cdf, p
    z0 = np.zeros(mu.shape, mu.dtype)
    return np.where(on, a, z0), np.where(on, cm, z0), np.where(on, cs, z0)


def grad(acq, sf, incumbent, param, obj, sides):
    """obj: dict(mu, sigma (m,), dmu, dsigma (m, D)); sides: [(kind, level, dict), ...] with the same dicts.
    -> (value (m,), grad (m, D), absolute (m, D): the sum of the absolute values of the gradient's terms)"""
    mu, sigma = obj["mu"], obj["sigma"]
    T = mu.dtype.type
    m, D = obj["dmu"].shape
    K = len(sides)
    lf = np.zeros((K, m), mu.dtype)
    dlf = np.zeros((K, m, D), mu.dtype)           # grad log f_k
    dfl = np.full((K, m), T(-np.inf))             # grad f_k = exp(dfl_k) df_k
    df = np.zeros((K, m, D), mu.dtype)
    for k, (kind, level, p) in enumerate(sides):
        lf[k] = side_logf(kind, level, p["mu"], p["sigma"])
        if kind == COST:
            dlf[k], dfl[k], df[k] = -p["dmu"], lf[k], -p["dmu"]
            continue
        on = (p["sigma"] != 0) & ~np.isnan(lf[k])
        s = np.where(on, p["sigma"], T(1))
        z = side_z(kind, level, p["mu"], p["sigma"])
        _, ratio = logphi(z)
        dz = ((p["dmu"] if kind == GE else -p["dmu"]) - z[:, None] * p["dsigma"]) / s[:, None]
        dz = np.where(on[:, None], dz, T(0))
        dlf[k] = np.where(on[:, None], ratio[:, None] * dz, T(0))
        dfl[k] = np.where(on, -z * z / T(2), T(-np.inf))
        df[k] = dz / T(math.sqrt(2.0 * math.pi)) if mu.dtype != LD else dz / np.sqrt(LD(2) * LD(4) * np.arctan(LD(1)))
    logw = np.zeros(m, mu.dtype)
    for k in range(K):
        logw = lf[k].copy() if k == 0 else logw + lf[k]
    if acq == ACQ_NONE:
        val = value_of(acq, np.zeros(m, mu.dtype), logw, mu, sigma)
        g = np.zeros((m, D), mu.dtype)
        absolute = np.zeros((m, D), mu.dtype)
        for k in range(K):
            g = g + dlf[k]
            absolute = absolute + np.abs(dlf[k])
    else:
        a, cm, cs = acq_coef(acq, sf, incumbent, param, mu, sigma)
        val = value_of(acq, a, logw, mu, sigma)
        with np.errstate(over="ignore", invalid="ignore"):
            w = np.exp(logw)[:, None]
            g = w * (cm[:, None] * obj["dmu"] + cs[:, None] * obj["dsigma"])
            absolute = w * (np.abs(cm[:, None] * obj["dmu"]) + np.abs(cs[:, None] * obj["dsigma"]))
            for k in range(K):
                rest = dfl[k].copy()
                for j in range(K):
                    if j != k:
                        rest = rest + lf[j]
                live = (df[k] != 0) & (a != 0)[:, None]
                term = np.where(live, (a * np.exp(rest))[:, None] * df[k], T(0))
                g = g + term
                absolute = absolute + np.abs(term)
    g = np.where(np.isnan(val)[:, None], T(np.nan), g)
    return val, g, absolute
