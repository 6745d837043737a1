"""The cases, bars and the one comparison of the leave-one-out tests -- TEST INFRASTRUCTURE shared by
tests/test_loo_reference.py (CPU: the 80-bit closed form against literal leave-one-out and its own central differences, the
proof that the bars reject the slips they are there for, the host backend) and tests/test_gpu_loo.py with its child
tests/_loo_child.py (tgp_loo and tgp_fit_loo_grad).

Cases: tests/lml_grad_edge_cases.py's, every model isotropic and ARD -- N = 1; 64 / 65 and 128 / 129 (the one-workgroup
fit against the blocked one, the first and the second 64-block); 192 / 193 (a full and a partial pairwise tile); 256 / 257
(Np = 256 -> 512, one and two row chunks of the kappa kernel); 300 and 384 (the latter on an f32 handle: the result is
f64); 1100 (Np = 1280, five row chunks); the 193 x 17 model without noise, without normalize_y and with a duplicated row.

Quantities (KEYS): resid, sigma and lpd (per point: judged entry by entry, each as a fraction of its OWN scale, the worst
entry reported), L_LOO, and the gradient's constant, length-scale (the worst of them) and noise entries.  Scales:
tests/loo_reference_hp.py.  A scale of exactly 0 asks for an exact 0.

Bars, u = 2^-53, exactly cov_edge_cases._bar:   bar = min(64 max(e_ref, N u), 1e-9)
  e_ref   the error of loo_reference_hp.loo_and_grad_f64 (NumPy / SciPy in f64) against the 80-bit closed form on that case
          and quantity: computed here on the CPU, recorded in tests/golden/loo_eref.json, never taken from the code under test;
  the cap is a condition: where 10 max(e_ref, N u) is above it the reference judges nothing, which is an error here
  (_bar asserts it; every case meets it with the noise of 1e-3 the models have, so none needed a larger one).
"""
import numpy as np

import cov_edge_cases as ec
import lml_grad_edge_cases as lc
import loo_reference_hp as lo
from cov_reference_hp import Fit

LD = np.longdouble
U, FACTOR, CAP = ec.U, ec.FACTOR, ec.CAP_VAL
POINT_KEYS = ("resid", "sigma", "lpd")
LOO_KEYS = POINT_KEYS + ("loo",)                      # what tgp_loo returns
GRAD_KEYS = ("constant", "length_scale", "noise")
KEYS = LOO_KEYS + GRAD_KEYS
CASES = lc.CASES
config, call_args, equal_ard_args, padded = lc.config, lc.call_args, lc.equal_ard_args, lc.padded

_cache = {}


def hp_reference(case):
    """loo_reference_hp.loo_and_grad's dict: made once per case, never modified"""
    if ("hp", case) not in _cache:
        X, y, kind, c, ls, noise, jitter, norm = call_args(case)
        ref = lo.loo_and_grad(Fit(X, y, kind, c, ls, noise, jitter, norm), y)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[("hp", case)] = ref
    return _cache[("hp", case)]


def f64_result(case, slip=None):
    return lo.loo_and_grad_f64(*call_args(case), slip=slip)


def errors(case, res, keys=KEYS):
    """{key: error as a fraction of the scale} of a result (a dict with resid, sigma, lpd, loo and, for the gradient's
    keys, grad) against the 80-bit reference; per-point keys and length_scale: the worst entry"""
    ref = hp_reference(case)
    e = {}
    for k in keys:
        if k in LOO_KEYS:
            got = np.atleast_1d(np.asarray(res[k], dtype=np.float64))
            assert got.shape == np.atleast_1d(ref[k]).shape, (case, k, got.shape)
            e[k] = float(lc._fraction(got, np.atleast_1d(ref[k]), np.atleast_1d(ref[k + "_scale"])).max())
    if any(k in GRAD_KEYS for k in keys):
        grad = np.asarray(res["grad"], dtype=np.float64)
        assert grad.shape == ref["grad"].shape, (case, grad.shape, ref["grad"].shape)
        g = lc._fraction(grad, ref["grad"], ref["grad_scale"])
        e.update(constant=float(g[0]), length_scale=float(g[1:-1].max()), noise=float(g[-1]))
    return {k: (e[k] if np.isfinite(e[k]) else float("inf")) for k in keys}     # (a NaN never passes)


def e_ref(case):
    if ("eref", case) not in _cache:
        _cache[("eref", case)] = errors(case, f64_result(case))
    return _cache[("eref", case)]


def bars(case):
    N = config(case)["N"]
    return {k: ec._bar(e, N, CAP) for k, e in e_ref(case).items()}


def judge(case, res, keys=KEYS):
    """THE comparison of a result with the 80-bit reference: {key: dict(e_ref, bar, err, ratio, ok)} and, under "ok",
    whether every key passed"""
    err, bar, ere = errors(case, res, keys), bars(case), e_ref(case)
    out = {k: dict(e_ref=ere[k], bar=bar[k], err=err[k], ratio=err[k] / bar[k], ok=bool(err[k] <= bar[k])) for k in keys}
    out["ok"] = all(out[k]["ok"] for k in keys)
    return out


def show(case, what, j):
    """the figures of a judge() result on one line (printed before anything is asserted)"""
    print("%s %s: " % (case, what) + "  ".join("%s %.3g (bar %.3g, e_ref %.3g, ratio %.3g)" % (k, j[k]["err"], j[k]["bar"], j[k]["e_ref"], j[k]["ratio"])
                                               for k in KEYS if k in j))


def fit_loo_grad(gp, case, args=None):
    """dict(lml, loo, grad) of NativeGP.fit_loo_grad"""
    lml, loo, grad = gp.fit_loo_grad(*(call_args(case) if args is None else args))
    return dict(lml=float(lml), loo=float(loo), grad=np.array(grad, dtype=np.float64, copy=True))


def fit_and_loo(gp, case):
    """NativeGP.loo()'s dict behind a plain fit of the case"""
    gp.fit(*call_args(case))
    return gp.loo()


def loo_bytes(r):
    return b"".join(np.ascontiguousarray(r[k], dtype=np.float64).tobytes() for k in LOO_KEYS)


def grad_bytes(r):
    return b"".join(np.ascontiguousarray(r[k], dtype=np.float64).tobytes() for k in ("lml", "loo", "grad"))
