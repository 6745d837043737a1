"""NumPy reference of the two-objective expected hypervolume improvement (tgp_ehvi_set_front, tgp_sweep_ehvi,
tgp_ehvi_grad; include/turbogp.h) -- TEST INFRASTRUCTURE, written from the definitions in the header, not from the library.
Everything here is a pure function of per-model posteriors (mu, sigma and, for the gradient, their partials) and works in
the arrays' own precision: float64 arrays take erfcx / ndtr from SciPy, numpy.longdouble arrays take Phi and the continued
fraction of erfc from tests/acq_grad_reference_hp.py.  ``H_mp`` is the mpmath form the f64 one is held to (its worst error
e_ref is tests/golden/ehvi_eref.json, written by tests/golden/make_golden_ehvi.py).

    u_j = sf_j y_j,  r = (sf_1 ref_1, sf_2 ref_2);  the front: the non-dominated pairs with u_1 > r_1 and u_2 > r_2, sorted by
    u_1 ascending (u_2 strictly descending);  a_0 = r_1, a_i = u_1^(i), a_{P+1} = +inf;  c_i = u_2^(i+1) (i < P), c_P = r_2
    e_j(t) = sigma_j H((m_j - t) / sigma_j),  H(z) = phi(z) + z Phi(z);  sigma_j == 0: max(m_j - t, 0);  e_j(+inf) = 0
    EHVI   = sum_{i = 0 .. P} max(e_1(a_i) - e_1(a_{i+1}), 0) e_2(c_i)

The pure-function bar (``bound``).  Strip i is the product (e_1(a_i) - e_1(a_{i+1})) e_2(c_i) of factors computed from the
posterior bits.  A factor e = sigma H(z) carries the rounding of z = (m - t) / sigma, about 2 u relative, which H turns into
|z Phi(z) / H(z)| 2 u <= (2 + z_-^2) 2 u of H (z_- = min(z, 0): for z >= 0 the ratio is at most 1), plus the error of H's own
evaluation, e_ref in the same unit; the difference of two e_1 is taken of rounded values, so its absolute error is the SUM of
theirs.  Hence per strip an absolute error of a few max(e_ref, u) times
    (e_1(a_i) + e_1(a_{i+1})) e_2(c_i) (3 + z_1(a_i)_-^2 + z_1(a_{i+1})_-^2 + z_2(c_i)_-^2)
(terms at t = +inf are 0), and the bar is FACTOR = 64 times max(e_ref, u) times their sum over the strips.  A reference value
below the smallest normal double may come back as exactly 0.
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53            # the f64 unit roundoff
TINY = float(np.finfo(np.float64).tiny)
FACTOR = 64.0             # the project's margin (tests/test_gpu_lml_grad_edges.py)
MAX_FRONT = 256
Z_SET = (-38.0, -30.0, -20.0, -10.0, -5.0, -2.0, -1.0, -0.5, -1e-3, 0.0, 1e-3, 0.5, 1.0, 2.0, 5.0, 10.0, 40.0)


# ---- the front -----------------------------------------------------------------------------------------------------
def front(Y, sf, ref):
    """-> (U (P, 2) oriented, sorted by u_1 ascending; raw (P, 2); trial indices (P,) -- the first row of Y that holds the
    point; hv).  A quadratic dominance filter: a pair stays when it strictly beats r in both coordinates and no DIFFERENT
    pair is at least as good in both."""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    sf = np.asarray(sf, dtype=np.float64)
    r = sf * np.asarray(ref, dtype=np.float64)
    Uo = Y * sf
    keep = []
    for i in range(Uo.shape[0]):
        p = Uo[i]
        if not (p[0] > r[0] and p[1] > r[1]):
            continue
        dominated = False
        for j in range(Uo.shape[0]):
            q = Uo[j]
            if (q[0] >= p[0] and q[1] >= p[1]) and (q[0] != p[0] or q[1] != p[1]):
                dominated = True
                break
        if not dominated and not any((Uo[k] == p).all() for k in keep):
            keep.append(i)
    keep.sort(key=lambda i: Uo[i, 0])
    idx = np.array(keep, dtype=np.int64)
    F = Uo[idx].reshape(-1, 2)
    return F, F * sf, idx, hypervolume(F, r)


def hypervolume(points, r):
    """the area dominated by oriented points over r, by a sort: sweep u_1 from the right, the running maximum of u_2 is the
    height of each slab"""
    pts = [(float(p[0]), float(p[1])) for p in np.asarray(points, dtype=np.float64).reshape(-1, 2) if p[0] > r[0] and p[1] > r[1]]
    pts.sort(key=lambda p: -p[0])
    area, top = 0.0, float(r[1])
    for k, (x, y) in enumerate(pts):
        top = max(top, y)
        left = pts[k + 1][0] if k + 1 < len(pts) else float(r[0])
        area += (x - left) * (top - float(r[1]))
    return area


def strips(F, r, dtype=np.float64):
    """a (P + 2,) with a_{P+1} = +inf, c (P + 1,) from the oriented sorted front F (P, 2) and the oriented reference r"""
    F = np.asarray(F, dtype=np.float64).reshape(-1, 2)
    a = np.concatenate([[r[0]], F[:, 0], [np.inf]]).astype(dtype)
    c = np.concatenate([F[:, 1], [r[1]]]).astype(dtype)
    return a, c


# ---- H, e and the strips ---------------------------------------------------------------------------------------------
def H_mp(z):
    """H(z) = phi(z) + z Phi(z) by mpmath at 80 digits, as an mpf"""
    import mpmath as mp
    with mp.workdps(80):
        z = mp.mpf(float(z))
        return mp.npdf(z) + z * mp.ncdf(z)


def _erfcx_ld(x):
    """exp(x^2) erfc(x) for long double x >= 0"""
    import acq_grad_reference_hp as ah
    x = np.asarray(x, dtype=LD)
    big = np.maximum(x, LD(1))
    f = big.copy()
    for n in range(ah._CF_TERMS, 0, -1):
        f = big + (LD(n) / LD(2)) / f
    small = np.minimum(x, LD(1))
    return np.where(x >= 1, LD(1) / (ah.SQRT_PI * f), ah.erfc(small.reshape(-1)).reshape(x.shape) * np.exp(small * small))


def cdf_pdf(z):
    """(Phi(z), phi(z)) in z's precision, the left tail through erfcx"""
    z = np.asarray(z)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if z.dtype == LD:
            import acq_grad_reference_hp as ah
            x = -np.minimum(z, LD(0)) / ah.SQRT2
            g = np.exp(-x * x)
            left = _erfcx_ld(x) * g / LD(2)
            return np.where(z <= 0, left, ah.Phi(np.maximum(z, LD(0)))), ah.pdf(z)
        from scipy.special import erfcx, ndtr
        z = z.astype(np.float64)
        x = -np.minimum(z, 0.0) / math.sqrt(2.0)
        g = np.exp(-x * x)
        return np.where(z <= 0, 0.5 * erfcx(x) * g, ndtr(np.maximum(z, 0.0))), np.exp(-z * z / 2.0) / math.sqrt(2.0 * math.pi)


def H(z):
    """H(z) in z's precision: z <= 0 as exp(-x^2) (1 / sqrt(2 pi) - x erfcx(x) / sqrt 2), x = -z / sqrt 2; z > 0 as phi + z Phi"""
    z = np.asarray(z)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if z.dtype == LD:
            import acq_grad_reference_hp as ah
            x = -np.minimum(z, LD(0)) / ah.SQRT2
            left = np.exp(-x * x) * (LD(1) / ah.SQRT_2PI - x * _erfcx_ld(x) / ah.SQRT2)
            zp = np.maximum(z, LD(0))
            return np.where(z <= 0, left, ah.pdf(zp) + zp * ah.Phi(zp))
        from scipy.special import erfcx, ndtr
        z = z.astype(np.float64)
        x = -np.minimum(z, 0.0) / math.sqrt(2.0)
        left = np.exp(-x * x) * (1.0 / math.sqrt(2.0 * math.pi) - x * erfcx(x) / math.sqrt(2.0))
        zp = np.maximum(z, 0.0)
        return np.where(z <= 0, left, np.exp(-zp * zp / 2.0) / math.sqrt(2.0 * math.pi) + zp * ndtr(zp))


def e_parts(m, s, t):
    """(e, Phi(z), phi(z), z_-^2) of one model at breakpoint t (a scalar; +inf: all 0); m, s (M,) in their precision"""
    m, s = np.asarray(m), np.asarray(s)
    T = m.dtype.type
    zero = np.zeros(m.shape, m.dtype)
    if np.isinf(t):
        return zero, zero, zero, zero
    d = m - T(t)
    on = s != 0
    ss = np.where(on, s, T(1))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        z = d / ss
        cdf, pdf = cdf_pdf(z)
        e = np.where(on, ss * H(z), np.where(d > 0, d, zero))
        cdf = np.where(on, cdf, np.where(d > 0, T(1), T(0)))
        pdf = np.where(on, pdf, zero)
        zm = np.where(on, np.minimum(z, T(0)) ** 2, zero)
    return e, cdf, pdf, zm


def partials(a, c, m1, s1, m2, s2):
    """-> dict(val, cm1, cs1, cm2, cs2, scale (all (M,)), abs_c (4, M)): the value, its partials in (m_1, sigma_1, m_2,
    sigma_2), the bar's sum over the strips and, per coefficient, the sum of the absolute values of its terms.  m_j are
    ORIENTED means (sf_j mu_j).  NaN where any input is NaN."""
    m1, s1, m2, s2 = (np.asarray(v) for v in (m1, s1, m2, s2))
    T = m1.dtype.type
    P = len(c) - 1
    out = {k: np.zeros(m1.shape, m1.dtype) for k in ("val", "cm1", "cs1", "cm2", "cs2", "scale")}
    abs_c = np.zeros((4,) + m1.shape, m1.dtype)
    lo = e_parts(m1, s1, a[0])
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(P + 1):
            hi = e_parts(m1, s1, a[i + 1])
            w = e_parts(m2, s2, c[i])
            de = lo[0] - hi[0]
            out["val"] = out["val"] + np.maximum(de, T(0)) * w[0]
            terms = ((lo[1] - hi[1]) * w[0], (lo[2] - hi[2]) * w[0], de * w[1], de * w[2])
            for k, name in enumerate(("cm1", "cs1", "cm2", "cs2")):
                out[name] = out[name] + terms[k]
            abs_c[0] += (lo[1] + hi[1]) * w[0]
            abs_c[1] += (lo[2] + hi[2]) * w[0]
            abs_c[2] += (lo[0] + hi[0]) * w[1]
            abs_c[3] += (lo[0] + hi[0]) * w[2]
            out["scale"] = out["scale"] + (lo[0] + hi[0]) * w[0] * (T(3) + lo[3] + hi[3] + w[3])
            lo = hi
    bad = np.isnan(m1) | np.isnan(s1) | np.isnan(m2) | np.isnan(s2)
    for k in out:
        out[k] = np.where(bad, T(np.nan), out[k])
    out["abs_c"] = abs_c
    return out


def value(a, c, m1, s1, m2, s2):
    return partials(a, c, m1, s1, m2, s2)["val"]


def value_mp(a, c, m1, s1, m2, s2):
    """the same sum for ONE row in mpmath (80 digits) from f64 posterior bits, as an mpf"""
    import mpmath as mp
    with mp.workdps(80):
        def e(m, s, t):
            if math.isinf(t):
                return mp.mpf(0)
            d = mp.mpf(float(m)) - mp.mpf(float(t))
            if s == 0:
                return d if d > 0 else mp.mpf(0)
            z = d / mp.mpf(float(s))
            return mp.mpf(float(s)) * (mp.npdf(z) + z * mp.ncdf(z))
        P = len(c) - 1
        total = mp.mpf(0)
        lo = e(m1, s1, a[0])
        for i in range(P + 1):
            hi = e(m1, s1, a[i + 1])
            total += max(lo - hi, mp.mpf(0)) * e(m2, s2, c[i])
            lo = hi
        return total


def bound(scale, e_ref):
    """the absolute pure-function bar per row from ``partials(...)['scale']`` (module docstring)"""
    return FACTOR * max(e_ref, U) * np.asarray(scale, dtype=np.float64)


def sweep(a, c, sf, mu1, sg1, mu2, sg2):
    """-> dict(value (M,), scale (M,), best_idx, best_val) from RAW posteriors"""
    T = np.asarray(mu1).dtype.type
    p = partials(a, c, T(sf[0]) * np.asarray(mu1), sg1, T(sf[1]) * np.asarray(mu2), sg2)
    bi, bv = argmax(p["val"])
    return dict(value=p["val"], scale=p["scale"], best_idx=bi, best_val=bv)


def argmax(value):
    """the library-wide rule: the largest value, the lowest index on ties, NaN never wins (all NaN: index 0, -inf)"""
    v = np.where(np.isnan(value), -np.inf, np.asarray(value, dtype=np.float64))
    i = int(np.argmax(v))
    return i, float(v[i])


def grad(a, c, sf, obj1, obj2):
    """obj_j: dict(mu, sigma (m,), dmu, dsigma (m, D)), raw units -> (value (m,), grad (m, D), absolute (m, D): the sum of
    the absolute values of the gradient's terms, each coefficient's own absolute sum in place of the coefficient)
        grad = sf_1 C_m1 dmu_1 + C_s1 dsigma_1 + sf_2 C_m2 dmu_2 + C_s2 dsigma_2;   sigma_j == 0: no sigma term"""
    T = obj1["mu"].dtype.type
    p = partials(a, c, T(sf[0]) * obj1["mu"], obj1["sigma"], T(sf[1]) * obj2["mu"], obj2["sigma"])
    g = np.zeros(obj1["dmu"].shape, obj1["mu"].dtype)
    absolute = np.zeros(obj1["dmu"].shape, obj1["mu"].dtype)
    for j, o in enumerate((obj1, obj2)):
        cm, cs = p["cm%d" % (j + 1)], p["cs%d" % (j + 1)]
        ds = np.where((o["sigma"] != 0)[:, None], o["dsigma"], T(0))
        g = g + T(sf[j]) * cm[:, None] * o["dmu"] + cs[:, None] * ds
        absolute = absolute + p["abs_c"][2 * j][:, None] * np.abs(o["dmu"]) + p["abs_c"][2 * j + 1][:, None] * np.abs(ds)
    g = np.where(np.isnan(p["val"])[:, None], T(np.nan), g)
    return p["val"], g, absolute


def default_ref(Y, sf):
    """the plugin's default reference point: per objective the worst observed value moved away from the front by 0.1 of the
    observed range (a zero range counts as 1.0), raw units"""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    sf = np.asarray(sf, dtype=np.float64)
    Uo = Y * sf
    rng = Uo.max(0) - Uo.min(0)
    rng = np.where(rng > 0, rng, 1.0)
    return sf * (Uo.min(0) - 0.1 * rng)
