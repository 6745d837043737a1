"""The problems of the expected hypervolume improvement's GPU tests (tests/test_gpu_ehvi.py, tests/test_gpu_ehvi_grad.py):
two objectives' models with their own training inputs, a front of exactly P points laid through the range of the observed
values, a candidate batch or query points.  Everything is a pure function of a case's name; the 80-bit fits are made once
per process and shared."""
import numpy as np

import ehvi_reference as er

C, LS, NOISE, JITTER = 1.3, 0.4, 2e-3, 1e-10

# N so that h and g take different sweep paths: one workgroup (N <= 128), one launch (<= 256), general (300); M around the
# value kernel's block (256) and several blocks; the last case lies beyond its capped grid (768 blocks of 256 = 196 608)
#   name                    N1    N2   D  M       P    dtypes          kernel      sf
CASES = {
    "n12x200_m1_p0":       (12,   200, 3, 1,      0,   ("f64", "f64"), "rbf",      (1.0, 1.0)),
    "n200x300_m777_p0":    (200,  300, 3, 777,    0,   ("f64", "f64"), "matern52", (-1.0, 1.0)),
    "n128x300_m255_p1":    (128,  300, 3, 255,    1,   ("f64", "f64"), "matern52", (1.0, -1.0)),
    "n200x12_m257_p2":     (200,  12,  3, 257,    2,   ("f64", "f64"), "rbf",      (-1.0, 1.0)),
    "n300x200_m777_p255":  (300,  200, 3, 777,    255, ("f32", "f64"), "matern32", (-1.0, -1.0)),
    "n300x300_m777_p256":  (300,  300, 3, 777,    256, ("f64", "f32"), "rbf",      (1.0, -1.0)),
    "n30x30_m262444_p2":   (30,   30,  2, 262444, 2,   ("f64", "f64"), "rbf",      (1.0, 1.0)),
}
# tgp_ehvi_grad: M = m query points
GRAD_CASES = {
    "g30x128_d1_m1_p0":     (30,   128,  1, 1,  0,   ("f64", "f64"), "rbf",      (1.0, 1.0)),
    "g128x300_d6_m3_p1":    (128,  300,  6, 3,  1,   ("f64", "f64"), "matern52", (1.0, -1.0)),
    "g300x30_d6_m64_p2":    (300,  30,   6, 64, 2,   ("f64", "f64"), "matern32", (-1.0, 1.0)),
    "g1000x300_d1_m3_p255": (1000, 300,  1, 3,  255, ("f64", "f64"), "matern52", (-1.0, -1.0)),
    "g300x1000_d6_m64_p256": (300, 1000, 6, 64, 256, ("f64", "f64"), "rbf",      (1.0, -1.0)),
    "g300x300_d6_m3_p2_f32": (300, 300,  6, 3,  2,   ("f32", "f32"), "rbf",      (1.0, 1.0)),
}
_problems, _hp, _refs = {}, {}, {}


def y1(X, rng):
    return np.sin(3.0 * X.sum(1)) + 0.3 * X[:, 0] + 0.05 * rng.normal(size=X.shape[0])


def y2(X, rng):
    return np.cos(2.0 * X[:, 0] + 1.0) + 0.5 * X.mean(1) + 0.05 * rng.normal(size=X.shape[0])


def staircase(P, sf, lo, hi, rng, dominated=True):
    """raw pairs Y whose front over the raw reference `lo`-side corner has exactly P points: a concave staircase between
    the oriented corners lo and hi, each stair followed by a point it dominates, shuffled"""
    t = (np.arange(P) + 0.5) / max(P, 1)
    u1 = lo[0] + (hi[0] - lo[0]) * t
    u2 = lo[1] + (hi[1] - lo[1]) * (1.0 - t * t)
    U = np.stack([u1, u2], 1)
    if dominated and P:
        worse = U - rng.uniform(0.0, 0.5, (P, 2)) * (np.asarray(hi) - np.asarray(lo)) / P
        U = np.concatenate([U, worse, U[: P // 2]])                    # (and duplicates)
    return (U * np.asarray(sf))[rng.permutation(U.shape[0])]


def problem(name):
    """dict(X1, y1, X2, y2, Xc (M, D), Y (n, 2) raw pairs, ref (2,) raw, sf, P, kind, ls, dtypes)"""
    if name in _problems:
        return _problems[name]
    N1, N2, D, M, P, dtypes, kind, sf = (CASES if name in CASES else GRAD_CASES)[name]
    rng = np.random.RandomState(N1 * 1000 + N2 + 7 * P + M % 1000)
    X1, X2 = rng.uniform(0, 1, (N1, D)), rng.uniform(0, 1, (N2, D))     # each objective has its own training inputs
    ya, yb = y1(X1, rng), y2(X2, rng)
    Xc = rng.uniform(-0.2, 1.2, (M, D))
    sfa = np.asarray(sf)
    # the oriented range of the observations: the reference point a tenth of it below the worst, the staircase inside it
    lo = np.array([(sfa[0] * ya).min(), (sfa[1] * yb).min()])
    hi = np.array([(sfa[0] * ya).max(), (sfa[1] * yb).max()])
    r = lo - 0.1 * (hi - lo)
    Y = staircase(P, sf, lo + 0.05 * (hi - lo), hi - 0.05 * (hi - lo), rng) if P else np.zeros((0, 2))
    p = dict(name=name, X1=X1, y1=ya, X2=X2, y2=yb, Xc=Xc, Y=Y, ref=r * sfa, sf=sf, P=P, kind=kind,
             ls=np.full(1, LS) if D < 6 else LS * (1.0 + 0.25 * np.arange(D)), dtypes=dtypes, D=D)
    _problems[name] = p
    return p


def fit_handle(L, dtype, X, y, kind, ls, noise=NOISE, jitter=JITTER):
    gp = L.NativeGP(0, dtype)
    gp.fit(X, y, kind, C, ls, noise, jitter, True)
    return gp


def handles(L, name, private=False, candidates=True):
    """(h with the batch resident and the front set, g); private: g on a private stream"""
    p = problem(name)
    h = fit_handle(L, p["dtypes"][0], p["X1"], p["y1"], p["kind"], p["ls"])
    g = fit_handle(L, p["dtypes"][1], p["X2"], p["y2"], p["kind"], p["ls"])
    if private:
        g.set_private_stream(True)
    if candidates:
        h.set_candidates(p["Xc"])
    front, hv = h.ehvi_set_front(p["Y"], p["ref"], p["sf"])
    assert front.shape[0] == p["P"], (front.shape, p["P"])
    return h, g


def strips_of(name, dtype=np.float64):
    p = problem(name)
    F, _, _, _ = er.front(p["Y"], p["sf"], p["ref"])
    return er.strips(F, np.asarray(p["sf"]) * p["ref"], dtype)


def hp_fits(name):
    """the two models in long double (tests/cov_reference_hp.py), once per case"""
    import cov_reference_hp as hp
    if name not in _hp:
        p = problem(name)
        _hp[name] = [hp.Fit(p["X1"], p["y1"], p["kind"], C, p["ls"], NOISE, JITTER, True),
                     hp.Fit(p["X2"], p["y2"], p["kind"], C, p["ls"], NOISE, JITTER, True)]
    return _hp[name]


def grad_references(name, f64=False):
    """(value (m,), grad (m, D), absolute (m, D)) of the case at its query points: the 80-bit closed form (every model's
    posterior and partials from tests/acq_grad_reference_hp.py on the long double fits) or, f64=True, the f64 restatement
    on oracle.gp_oracle's fits"""
    import acq_grad_reference_hp as ah
    p = problem(name)
    if f64:
        from oracle import gp_oracle as o
        posts = [ah.posterior_f64(o.fit(X, y, p["kind"], C, p["ls"], NOISE, JITTER, True), p["Xc"])
                 for X, y in ((p["X1"], p["y1"]), (p["X2"], p["y2"]))]
        a, c = strips_of(name)
    elif name in _refs:
        return _refs[name]
    else:
        posts = [ah.posterior(f, p["Xc"]) for f in hp_fits(name)]
        a, c = strips_of(name, er.LD)
    out = er.grad(a, c, p["sf"], posts[0], posts[1])
    if not f64:
        _refs[name] = out
    return out


def grad_error(name, grad):
    """the worst entry of |grad - 80-bit| over that entry's sum of absolute terms (magnitudes below the smallest normal
    double count as that) of anything that claims to be the case's gradient"""
    _, rg, ra = grad_references(name)
    return float((np.abs(np.asarray(grad, dtype=er.LD) - rg) / np.maximum(ra, er.LD(er.TINY))).max())
