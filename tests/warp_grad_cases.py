"""The models and the one comparison of the warped fit's gradient tests -- TEST INFRASTRUCTURE shared by
tests/test_warp_grad_reference.py (CPU) and tests/test_gpu_warp.py (tgp_fit_warp_grad).

A case: N points in the box [-1, 2]^D, shapes a, b per dimension, an ARD kernel on w(X).  The REFERENCE of the 2 D warp
entries is the chain rule in 80 bits:  d LML / d log a_d = a_d sum_i g_id (dw/da)(u_id), g = input_grad_reference_hp.dlml_dx of
the model fitted on the f64 numbers w(X) it is handed (the caller's: NumPy's on the CPU, the device's own on the GPU, so the
model is the same to the bit), dw/da and dw/db from mpmath.  SCALE of an entry: a_d sum_i scale_id |dw/da|.  The CPU test
holds that reference to central differences of the 80-bit LML over NumPy-warped X, and records the error of the f64
restatement (dlml_dx_f64 and warp_f64) against it as e_ref (tests/golden/warp_grad_eref.json); bars as everywhere:
min(64 max(e_ref, N u), 1e-9) of the scale.
"""
import json
import os

import numpy as np

import cov_edge_cases as ec
import input_grad_reference_hp as ir
import warp_reference as wr
from cov_reference_hp import Fit

LD = np.longdouble
LO, HI = -1.0, 2.0
C, NOISE, JITTER = 1.3, 1e-3, 1e-10
CASES = {
    "N40-D2": dict(N=40, D=2, kind="matern52", a=(3.0, 1.0), b=(1.0, 0.4)),
    "N129-D3": dict(N=129, D=3, kind="rbf", a=(0.5, 2.0, 1.5), b=(2.0, 0.7, 1.0)),
    "N257-D17": dict(N=257, D=17, kind="matern32", a=tuple(0.6 + 0.1 * d for d in range(17)), b=tuple(1.9 - 0.08 * d for d in range(17))),
    "identity": dict(N=40, D=2, kind="matern52", a=(1.0, 1.0), b=(1.0, 1.0)),
}
EREF_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "warp_grad_eref.json")
_cache = {}


def data(case):
    """(X raw (N, D), y, lo (D), hi (D), a (D), b (D), length scales (D) in warped units)"""
    if case not in _cache:
        c = CASES[case]
        rng = np.random.RandomState(700 + c["N"])
        X = rng.uniform(LO, HI, size=(c["N"], c["D"]))
        U = (X - LO) / (HI - LO)
        y = np.sin(6.0 * U[:, 0] ** 3) + (U ** 2).sum(axis=1) / c["D"] + 0.01 * rng.standard_normal(c["N"])
        ls = rng.uniform(0.3, 0.6, size=c["D"]) * np.sqrt(c["D"] / 2.0)
        out = (X, y, np.full(c["D"], LO), np.full(c["D"], HI), np.array(c["a"]), np.array(c["b"]), ls)
        for v in out:
            v.setflags(write=False)
        _cache[case] = out
    return _cache[case]


def unit(case):
    X, _, lo, hi, _, _, _ = data(case)
    return np.clip((X - lo) / (hi - lo), 0.0, 1.0)


def fit_args(case, Wx):
    _, y, _, _, _, _, ls = data(case)
    return (Wx, y, CASES[case]["kind"], C, ls, NOISE, JITTER, True)


def reference(case, Wx):
    """(the 2 D entries [d/dlog a | d/dlog b], their scales) in long double for the model fitted on Wx"""
    _, _, _, _, a, b, _ = data(case)
    g, s = ir.dlml_dx(Fit(*fit_args(case, Wx)))
    u = unit(case)
    n, D = u.shape
    da, db = np.zeros((n, D), LD), np.zeros((n, D), LD)
    for i in range(n):
        for d in range(D):
            _, _, va, vb = wr.warp_mp(u[i, d], a[d], b[d])
            da[i, d], db[i, d] = LD(wr.mp.nstr(va, 25)), LD(wr.mp.nstr(vb, 25))
    val = np.concatenate([a * (g * da).sum(axis=0), b * (g * db).sum(axis=0)])
    sc = np.concatenate([a * (s * np.abs(da)).sum(axis=0), b * (s * np.abs(db)).sum(axis=0)])
    return val, sc


def restatement(case):
    """the same entries in f64 NumPy, on NumPy's own w(X)"""
    _, _, _, _, a, b, _ = data(case)
    w, _, da, db = wr.warp_f64(unit(case), a[None, :], b[None, :])
    g = ir.dlml_dx_f64(*fit_args(case, w))
    return w, np.concatenate([a * (g * da).sum(axis=0), b * (g * db).sum(axis=0)])


def fractions(got, val, sc):
    d = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - val)
    return (d / sc).astype(np.float64)


def e_ref_recorded(case):
    with open(EREF_JSON) as f:
        return float(json.load(f)["cases"][case])


def bar(case, e_ref):
    return ec._bar(e_ref, CASES[case]["N"], ec.CAP_VAL)
