"""The Kumaraswamy input warp, its derivatives and its inverse in mpmath at 50 digits, and the f64 NumPy restatement of the
stable form (csrc/warp_math.hpp's formulas, restated from include/turbogp.h) -- TEST INFRASTRUCTURE.

    w = 1 - (1 - u^a)^b;   dw/du = a b u^(a-1) (1-u^a)^(b-1);   dw/da = b (1-u^a)^(b-1) u^a log u;
    dw/db = -(1-u^a)^b log(1-u^a);   u = (1 - (1-w)^(1/b))^(1/a)
    dw/da and dw/db are 0 at u = 0 and u = 1 (their limits); dw/du at u = 0 is 0 (a > 1), b (a = 1), +inf (a < 1), at u = 1
    it is 0 (b > 1), a (b = 1), +inf (b < 1).

GRID: the points and shapes every warp test runs over.  Errors: w absolute; a derivative relative to max(|value|, the
smallest normal double); an infinite value must be matched exactly.
"""
import numpy as np
from mpmath import mp, mpf

mp.dps = 50
TINY = float(np.finfo(np.float64).tiny)
U = 2.0 ** -53
US = (0.0, 5e-324, 1e-300, 1e-16, 1e-8, 0.1, 0.5, 0.9, 1 - 1e-8, 1 - 2.0 ** -53, 1.0)
SHAPES = (0.25, 0.5, 1.0, 2.0, 4.0)
GRID = [(u, a, b) for u in US for a in SHAPES for b in SHAPES]


def warp_mp(u, a, b):
    """(w, dw/du, dw/da, dw/db) as mpf (or +inf) at the f64 numbers u, a, b"""
    u, a, b = mpf(u), mpf(a), mpf(b)
    inf = mpf("inf")
    if u == 0:
        return mpf(0), (mpf(0) if a > 1 else (b if a == 1 else inf)), mpf(0), mpf(0)
    if u == 1:
        return mpf(1), (mpf(0) if b > 1 else (a if b == 1 else inf)), mpf(0), mpf(0)
    ua = u ** a
    q, lq = 1 - ua, mp.log1p(-ua)        # (1 - u^a is 1 to 50 digits where u^a < 1e-50: its logarithm and 1 - q^b are taken directly)
    return -mp.expm1(b * lq), a * b * u ** (a - 1) * q ** (b - 1), b * q ** (b - 1) * ua * mp.log(u), -(q ** b) * lq


def inverse_mp(w, a, b):
    w, a, b = mpf(w), mpf(a), mpf(b)
    return (-mp.expm1(mp.log1p(-w) / b)) ** (1 / a)


def _log1mexp(x):
    with np.errstate(divide="ignore"):
        return np.where(x > -np.log(2.0), np.log(-np.expm1(x)), np.log1p(-np.exp(x)))


def warp_f64(u, a, b):
    """(w, dw/du, dw/da, dw/db) in f64 NumPy for arrays u, a, b of one shape"""
    u, a, b = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(u, a, b))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lu = np.log(u)
        x = a * lu
        t = _log1mexp(x)
        inner = (u > 0) & (u < 1)
        ea = np.where(a == 1, 0.0, (a - 1) * lu)
        eb = np.where(b == 1, 0.0, (b - 1) * t)
        du = a * b * np.exp(ea + eb)
        da = np.where(inner, b * lu * np.exp(eb + x), 0.0)
        db = np.where(inner, -t * np.exp(b * t), 0.0)
        w = np.where((a == 1) & (b == 1), u, -np.expm1(b * t))
    return w, du, da, db


def inverse_f64(w, a, b):
    w, a, b = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(w, a, b))
    with np.errstate(divide="ignore", invalid="ignore"):
        y = np.log1p(-w) / b
        return np.where((a == 1) & (b == 1), w, np.exp(_log1mexp(y) / a))


def errors(u, a, b, got):
    """(w error absolute, the three derivatives' errors relative to max(|value|, TINY)) of got = (w, du, da, db) floats at
    one grid point; an infinite reference must be matched exactly (error 0 or inf); a NaN is inf"""
    want = warp_mp(u, a, b)
    out = []
    for k, (g, r) in enumerate(zip(got, want)):
        g = float(g)
        if np.isnan(g):
            out.append(np.inf)
        elif mp.isinf(r) or np.isinf(g):
            out.append(0.0 if (mp.isinf(r) and np.isinf(g) and g > 0) else np.inf)
        elif k == 0:
            out.append(float(abs(mpf(g) - r)))
        else:
            out.append(float(abs(mpf(g) - r) / max(abs(r), mpf(TINY))))
    return out
