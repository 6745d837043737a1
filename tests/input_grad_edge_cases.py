"""The cases, bars and the one comparison of the input gradient's edge tests -- TEST INFRASTRUCTURE shared by
tests/test_input_grad_reference.py (CPU: the 80-bit closed form against central differences and its identities, the f64
restatement's e_ref, the proof that the bars reject the slips) and tests/test_gpu_input_grad_edges.py (tgp_fit_input_grad).

Cases: tests/lml_grad_edge_cases.py's models, imported and not edited, each isotropic and ARD -- tile edges N = 64, 65, 128,
129, 192, 193, 256, 257; Dp and pass edges D = 1, 3, 16, 17, 61, 63, 65; an f32 handle; no noise; raw targets; a duplicated
row under Matern-1/2.  G (N = 1100) is left out: its 80-bit K^-1 = Linv^T Linv alone takes minutes here.

Bar per ENTRY, as cov_edge_cases._bar makes it:  min(64 max(e_ref, N u), 1e-9) of the entry's scale
(tests/input_grad_reference_hp.py), e_ref the f64 restatement's own worst entry against the 80-bit form on that case,
recorded in tests/golden/input_grad_eref.json (the GPU test reads the record, never the code under test).  The cap is a
condition: _bar asserts 10 max(e_ref, N u) <= 1e-9, and a case that does not meet it would be dropped from CASES with the
reason written here (none had to be).  A scale of exactly 0 (N = 1) asks for an exact 0.
"""
import json
import os

import numpy as np

import cov_edge_cases as ec
import input_grad_reference_hp as ir
import lml_grad_edge_cases as lc
from cov_reference_hp import Fit

LD = np.longdouble
MODELS = ("S1", "S2", "S3", "A", "S5", "W", "B", "T192", "T193", "C", "D", "E", "F", "T193-noise0", "T193-raw", "T193-dup")
CASES = ["%s/%s" % (m, mode) for m in MODELS for mode in ("iso", "ard")]
EREF_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "input_grad_eref.json")

_cache = {}


def hp_reference(case):
    """(gradient, scale) of input_grad_reference_hp.dlml_dx: made once per case, never modified"""
    if ("hp", case) not in _cache:
        X, y, kind, c, ls, noise, jitter, norm = lc.call_args(case)
        g, s = ir.dlml_dx(Fit(X, y, kind, c, ls, noise, jitter, norm))
        g.setflags(write=False); s.setflags(write=False)
        _cache[("hp", case)] = (g, s)
    return _cache[("hp", case)]


def fractions(case, dX):
    """|dX - reference| / scale entry by entry (N, D), the difference formed in long double; a scale of exactly 0 asks for
    an exact 0; a NaN never passes"""
    g, s = hp_reference(case)
    dX = np.asarray(dX, dtype=np.float64)
    assert dX.shape == g.shape, (case, dX.shape, g.shape)
    d = np.abs(dX.astype(LD) - g)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(s == 0, np.where(d == 0, LD(0), LD(np.inf)), d / np.where(s == 0, LD(1), s)).astype(np.float64)
    return np.where(np.isfinite(f), f, np.inf)


def error(case, dX):
    """the worst entry's error as a fraction of its scale"""
    return float(fractions(case, dX).max())


def f64_result(case, slip=None):
    return ir.dlml_dx_f64(*lc.call_args(case), slip=slip)


def e_ref_fresh(case):
    if ("eref", case) not in _cache:
        _cache[("eref", case)] = error(case, f64_result(case))
    return _cache[("eref", case)]


def e_ref_recorded(case):
    if "record" not in _cache:
        with open(EREF_JSON) as f:
            _cache["record"] = json.load(f)["cases"]
    return float(_cache["record"][case])


def bar(case, e_ref):
    return ec._bar(e_ref, lc.config(case)["N"], ec.CAP_VAL)


def identities(case, dX, grad):
    """the two identities of a result (dX, tgp_fit_grad's grad) as fractions of their scales: sum_i dX[i][d] over
    sum_i scale[i][d], and sum_i x_id dX[i][d] + grad_ls[d] (isotropic: summed over d) over sum_i |x_id| scale[i][d] plus the
    length-scale entry's own scale.  (zero, first moment); a scale of 0 asks for an exact 0"""
    X = np.asarray(lc.call_args(case)[0], dtype=np.float64).astype(LD)
    _, s = hp_reference(case)
    dl = np.asarray(dX, dtype=np.float64).astype(LD)
    ref = lc.hp_reference(case)
    gls, sls = np.asarray(grad, dtype=np.float64).astype(LD)[1:-1], ref["grad_scale"][1:-1]
    zero_n, zero_s = np.abs(dl.sum(axis=0)), s.sum(axis=0)
    mom_n, mom_s = (X * dl).sum(axis=0), (np.abs(X) * s).sum(axis=0)
    if len(gls) == 1:
        mom_n, mom_s = np.array([mom_n.sum()]), np.array([mom_s.sum()])
    mom_n, mom_s = np.abs(mom_n + gls), mom_s + sls

    def frac(n, sc):
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(sc == 0, np.where(n == 0, LD(0), LD(np.inf)), n / np.where(sc == 0, LD(1), sc)).astype(np.float64)
        return float(np.where(np.isfinite(f), f, np.inf).max())

    return frac(zero_n, zero_s), frac(mom_n, mom_s)
