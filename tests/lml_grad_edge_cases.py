"""The models, bars and the one comparison of the LML gradient's edge tests -- TEST INFRASTRUCTURE shared by
tests/test_lml_grad_reference.py (CPU: the 80-bit closed form against the f64 oracle, the golden cases and its own central
differences, and the proof that the bars reject the slips they are there for) and tests/test_gpu_lml_grad_edges.py with its
child tests/_lml_grad_child.py (tgp_fit_grad's three implementations).

Models: the data recipe of tests/cov_edge_cases.py (X, y of seed 100 + N; c = 1.3, noise 1e-3, jitter 1e-10, normalize_y;
length scales uniform(0.4, 0.9) sqrt(D / 3) (ARD) or 0.6 sqrt(D / 3)), its A-G where they fit (the same X and y), and
what the gradient's kernels need beyond them.  A CASE is "model/iso" or "model/ard"; both are registered in
cov_edge_cases.EXTRA, so its data() serves them.  Three variants of the 193 x 17 model: without noise (the noise entry is
exactly 0.0), without normalize_y, and with row 7 a bit-for-bit copy of row 3 under Matern-1/2 (an off-diagonal d2 = 0).

Quantities (KEYS): the LML, the constant's entry, the length-scale entries (the worst of them, each as a fraction of its
OWN scale), the noise entry.  Scales: tests/lml_grad_reference_hp.py.  A scale of exactly 0 (the length-scale entry of one
training point, the noise entry without noise) asks for an exact 0.

Bars, u = 2^-53, as cov_edge_cases._bar makes them:   bar = min(FACTOR max(e_ref, N u), CAP)
  e_ref   the error of oracle.gp_oracle.lml_and_grad (f64, K^-1 by cho_solve) against the 80-bit closed form on that case
          and quantity, computed here, never taken from the code under test;
  FACTOR  cov_edge_cases.FACTOR (64) and its reason: room for an explicit inverse factor and fixed-order MFMA sums over a
          backward-stable solve;
  CAP     cov_edge_cases.CAP_VAL (1e-9), a condition, not a measurement: where 10 max(e_ref, N u) is above it the reference
          judges nothing, which is an error here.
Measured (tests/golden/lml_grad_eref.json holds every case): the oracle's largest e_ref is the noise entry's, tr K^-1 --
A 4.4e-13 (iso) / 2.8e-13 (ARD), D 2.9e-13, E 1.7e-14, G 1.2e-12 / 5.3e-13 -- and the LML's on G, 2.6e-13; the constant's
and the length-scale entries stay at 1e-18 ... 3e-16, so their bars are the floor 64 N u (7e-15 for one point, 9e-13 at
N = 128, 7.8e-12 at N = 1100).  The largest bar is 7.3e-11 (G/iso, noise): every case is a factor of 80 inside the cap's
condition.  Scale / |entry| reaches 1.2e6 on A and 8.6e5 on G.
"""
import numpy as np

import cov_edge_cases as ec
import lml_grad_reference_hp as lr
from cov_reference_hp import Fit
from oracle import gp_oracle as G

LD = np.longdouble
U, FACTOR, CAP = ec.U, ec.FACTOR, ec.CAP_VAL
KEYS = ("lml", "constant", "length_scale", "noise")

# path: what tgp_fit_grad takes by default (small: N <= 128 and D padded to a multiple of 4 at most 64)
MODELS = {
    "S1": dict(N=1, D=1, kind="rbf", path="small"),
    "S2": dict(N=64, D=64, kind="matern52", path="small"),          # one block pair, every lane a dimension
    "S3": dict(N=65, D=63, kind="matern12", path="small"),          # three block pairs, one padding lane
    "A": dict(N=128, D=2, kind="rbf", path="small"),
    "S5": dict(N=128, D=61, kind="matern32", path="small"),         # Dp = 64, four ARD passes
    "W": dict(N=97, D=65, kind="matern12", path="blocked"),         # Dp = 68 forces the blocked path; five ARD passes, the last partial
    "B": dict(N=129, D=3, kind="matern32", path="blocked"),         # the third tile holds one real row
    "T192": dict(N=192, D=16, kind="rbf", path="blocked"),          # exactly three tiles, exactly one pass
    "T193": dict(N=193, D=17, kind="matern52", path="blocked"),     # a partial tile, a partial second pass
    "C": dict(N=256, D=4, kind="matern12", path="blocked"),         # NV = Np
    "D": dict(N=257, D=3, kind="rbf", path="blocked"),              # Np = 512
    "E": dict(N=300, D=17, kind="matern52", path="blocked"),
    "F": dict(N=384, D=33, kind="rbf", path="blocked", dtype="f32"),   # an f32 handle: the gradient is f64 whatever the dtype
    "G": dict(N=1100, D=6, kind="rbf", path="blocked"),             # Np = 1280
    "T193-noise0": dict(N=193, D=17, kind="matern52", path="blocked", noise=0.0),
    "T193-raw": dict(N=193, D=17, kind="matern52", path="blocked", normalize_y=False),
    "T193-dup": dict(N=193, D=17, kind="matern12", path="blocked", dup=(7, 3)),
}
for _m, _c in MODELS.items():
    _c.setdefault("dtype", "f64")
    for _ard in (False, True):
        ec.EXTRA["%s/%s" % (_m, "ard" if _ard else "iso")] = dict(_c, ard=_ard)
    if _m in ec.MODELS:                          # "its A-G where they fit": the same sizes and kernel, so the same X and y
        assert all(ec.MODELS[_m][k] == _c[k] for k in ("N", "D", "kind", "dtype")), _m
# the size at which the default takes the 128-tile K^-1 product (Np = 4352 > TGP_KINV64 = 4096).  No case of CASES: the
# 80-bit reference would take an hour here, so it is held to the f64 oracle and to the 64-tile product (test (d))
SWITCH = "X4097/iso"
SWITCH_CLASS = ("T192/iso", "D/iso", "G/iso")    # the blocked isotropic RBF cases that do have an 80-bit reference: its e_ref class
ec.EXTRA[SWITCH] = dict(N=4097, D=2, kind="rbf", ard=False, dtype="f64", path="blocked")
CASES = ["%s/%s" % (m, mode) for m in MODELS for mode in ("iso", "ard")]     # (EXTRA also holds other suites' models)
SMALL = [c for c in CASES if MODELS[c.split("/")[0]]["path"] == "small"]
BLOCKED = [c for c in CASES if MODELS[c.split("/")[0]]["path"] == "blocked"]

_cache = {}


def config(case):
    return ec.EXTRA[case]


def padded(case):
    """Np of the blocked path: N rounded up to a multiple of 256"""
    return (config(case)["N"] + 255) // 256 * 256


def call_args(case):
    """(X, y, kind, constant, length scale(s), noise, jitter, normalize_y): the arguments of fit_grad and of every
    reference; an ARD call carries D length scales (one where D = 1), an isotropic one a float"""
    if ("args", case) not in _cache:
        c = config(case)
        X, y, ls, _ = ec.data(case)
        X, y = X.copy(), y.copy()
        if c.get("dup"):
            X[c["dup"][0]] = X[c["dup"][1]]
        X.setflags(write=False); y.setflags(write=False)
        ls = np.array(ls, dtype=np.float64, copy=True) if c["ard"] else float(ls)
        _cache[("args", case)] = (X, y, c["kind"], ec.C, ls, c.get("noise", ec.NOISE), ec.JITTER, c.get("normalize_y", True))
    return _cache[("args", case)]


def equal_ard_args(case):
    """the isotropic case's arguments with its length scale written D times: the ARD sums of the same model"""
    assert not config(case)["ard"]
    a = call_args(case)
    return a[:4] + (np.full(config(case)["D"], a[4]),) + a[5:]


def fit_grad(gp, case, args=None):
    """(lml, grad) of NativeGP.fit_grad"""
    lml, grad = gp.fit_grad(*(call_args(case) if args is None else args))
    return float(lml), np.array(grad, dtype=np.float64, copy=True)


def hp_reference(case):
    """lml_grad_reference_hp.lml_and_grad's dict: made once per case, never modified"""
    if ("hp", case) not in _cache:
        X, y, kind, c, ls, noise, jitter, norm = call_args(case)
        ref = lr.lml_and_grad(Fit(X, y, kind, c, ls, noise, jitter, norm), y)
        for a in ("grad", "grad_scale"):
            ref[a].setflags(write=False)
        _cache[("hp", case)] = ref
    return _cache[("hp", case)]


def oracle_result(case):
    if ("oracle", case) not in _cache:
        _cache[("oracle", case)] = G.lml_and_grad(*call_args(case))
    return _cache[("oracle", case)]


def f64_result(case, slip=None):
    """(lml, grad) of lml_grad_reference_hp.lml_and_grad_f64 (slip: one of its SLIPS)"""
    return lr.lml_and_grad_f64(*call_args(case), slip=slip)


def _fraction(got, want, scale):
    """|got - want| / scale entry by entry, the difference formed in long double; a scale of exactly 0 asks for an exact 0"""
    d = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = np.where(scale == 0, np.where(d == 0, LD(0), LD(np.inf)), d / np.where(scale == 0, LD(1), scale))
    return f.astype(np.float64)


def errors(case, lml, grad):
    """{key: error as a fraction of the scale} of a result against the 80-bit reference; length_scale: the worst entry"""
    ref = hp_reference(case)
    grad = np.asarray(grad, dtype=np.float64)
    assert grad.shape == ref["grad"].shape, (case, grad.shape, ref["grad"].shape)
    g = _fraction(grad, ref["grad"], ref["grad_scale"])
    e = dict(lml=float(_fraction([lml], ref["lml"], ref["lml_scale"])[0]), constant=float(g[0]),
             length_scale=float(g[1:-1].max()), noise=float(g[-1]))
    return {k: (v if np.isfinite(v) else float("inf")) for k, v in e.items()}     # (a NaN never passes)


def e_ref(case):
    if ("eref", case) not in _cache:
        _cache[("eref", case)] = errors(case, *oracle_result(case))
    return _cache[("eref", case)]


def bars(case):
    N = config(case)["N"]
    return {k: ec._bar(e, N, CAP) for k, e in e_ref(case).items()}


def judge(case, lml, grad):
    """THE comparison of tgp_fit_grad's result (or anything that claims to be one) with the 80-bit reference:
    {key: dict(e_ref, bar, err, ratio, ok)} and, under "ok", whether every key passed"""
    err, bar, ere = errors(case, lml, grad), bars(case), e_ref(case)
    out = {k: dict(e_ref=ere[k], bar=bar[k], err=err[k], ratio=err[k] / bar[k], ok=bool(err[k] <= bar[k])) for k in KEYS}
    out["ok"] = all(out[k]["ok"] for k in KEYS)
    return out


def cancellation(case):
    """the largest scale / |entry| over the gradient's non-zero entries (how much of the terms cancels)"""
    ref = hp_reference(case)
    nz = ref["grad"] != 0
    return float((ref["grad_scale"][nz] / np.abs(ref["grad"][nz])).max()) if nz.any() else 0.0


def show(case, what, j):
    """the figures of a judge() result on one line (printed before anything is asserted)"""
    print("%s %s: " % (case, what) + "  ".join("%s %.3g (bar %.3g, e_ref %.3g, ratio %.3g)" % (k, j[k]["err"], j[k]["bar"], j[k]["e_ref"], j[k]["ratio"]) for k in KEYS))


def result_bytes(lml, grad):
    return np.float64(lml).tobytes() + np.ascontiguousarray(grad, dtype=np.float64).tobytes()
