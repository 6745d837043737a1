"""The problems of the constrained / cost-aware acquisition's tests (tests/test_gpu_weighted.py, tests/test_gpu_weighted_grad.py,
tests/test_weighted_reference.py, tests/golden/make_golden_weighted.py): an objective model and K side models, each with
its own training inputs, a candidate batch, and the comparisons.  Everything is a pure function of a case's name; oracle
fits and 80-bit fits are made once per process and shared."""
import math

import numpy as np

import weighted_reference as wr

GE, LE, COST = wr.GE, wr.LE, wr.COST
NONE, PI, EI = wr.ACQ_NONE, wr.ACQ_PI, wr.ACQ_EI
C, LS, NOISE, JITTER = 1.3, 0.4, 2e-3, 1e-10
D = 3
RTOL, VAR_ATOL = 1e-5, 1e-9      # tests/test_gpu_parity.py: mean / variance of a single f64 sweep against the oracle

# objective N x side N: 12 x 12 (one workgroup), 200 x 12 (one launch x one workgroup), 300 x 200 (general x one launch),
# 300 x 300 (general), and all three mixed within one call
#   name                     No   Ns                                      M    kinds                                  dtypes          kernel      ard    acq   sf
CASES = {
    "n12x12_m1_k1":         (12,  [12],                                   1,   [GE],                                  ("f64", "f64"), "rbf",      False, EI,   -1.0),
    "n200x12_m33_k2":       (200, [12, 12],                               33,  [LE, COST],                            ("f64", "f64"), "matern52", True,  PI,   +1.0),
    "n300x200_m777_k8":     (300, [200, 12, 300, 200, 12, 300, 200, 12],  777, [GE, LE, COST, GE, LE, COST, GE, LE],  ("f64", "f64"), "rbf",      True,  EI,   -1.0),
    "n300x300_m777_k2_f32": (300, [300, 300],                             777, [GE, COST],                            ("f32", "f32"), "matern52", False, EI,   +1.0),
    "n300x200_m33_k1_mix":  (300, [200],                                  33,  [LE],                                  ("f64", "f32"), "matern32", False, EI,   -1.0),
    "n300x300_m33_k1_mix":  (300, [300],                                  33,  [GE],                                  ("f64", "f32"), "rbf",      False, PI,   -1.0),
    "n200_m777_k0":         (200, [],                                     777, [],                                    ("f64", "f64"), "rbf",      False, EI,   -1.0),
    "n12x12_m777_k2_none":  (12,  [12, 12],                               777, [GE, LE],                              ("f64", "f64"), "matern52", False, NONE, +1.0),
}
# tgp_weighted_grad: the same tuple with M = m query points (the batch's rows); the *_underflow case's GE level lies 45 of the
# side's posterior deviations above its mean on every query point (set from the oracle in problem())
GRAD_CASES = {
    "g12_k1_m1":            (12,  [12],                                   1,   [GE],                                  ("f64", "f64"), "rbf",      False, EI,   -1.0),
    "g200_k2_m7":           (200, [200, 12],                              7,   [LE, COST],                            ("f64", "f64"), "matern52", True,  PI,   +1.0),
    "g300_k8_m64":          (300, [12, 12, 200, 12, 12, 12, 300, 12],     64,  [GE, LE, COST, GE, LE, COST, GE, LE],  ("f64", "f64"), "rbf",      True,  EI,   -1.0),
    "g300_k2_m7_f32obj":    (300, [200, 12],                              7,   [GE, COST],                            ("f32", "f64"), "matern32", False, EI,   -1.0),
    "g200_k2_m7_none":      (200, [12, 200],                              7,   [GE, LE],                              ("f64", "f64"), "matern52", False, NONE, +1.0),
    "g200_k1_m7_underflow": (200, [12],                                   7,   [GE],                                  ("f64", "f64"), "rbf",      False, NONE, +1.0),
}
XI = 0.01
_problems, _oracle, _hp = {}, {}, {}


def ls_of(ard):
    return LS * (1.0 + 0.25 * np.arange(D)) if ard else np.array([LS])


def objective_y(X, rng):
    return np.sin(3.0 * X.sum(1)) + 0.3 * X[:, 0] + 0.05 * rng.normal(size=X.shape[0])


def side_y(X, j, rng):
    return np.cos(2.0 * X[:, j % D] + j) + 0.5 * X.mean(1) + 0.05 * rng.normal(size=X.shape[0])


def problem(name):
    """dict(X, y, sides [(X_k, y_k, kind, level)], Xc (M, D), kind, ls, acq, sf, incumbent, param, dtypes)"""
    if name in _problems:
        return _problems[name]
    No, Ns, M, kinds, dtypes, kind, ard, acq, sf = (CASES if name in CASES else GRAD_CASES)[name]
    rng = np.random.RandomState(No * 1000 + M + 7 * len(Ns))
    X = rng.uniform(0, 1, (No, D))
    y = objective_y(X, rng)
    sides = []
    for j, (n, k) in enumerate(zip(Ns, kinds)):
        Xk = rng.uniform(0, 1, (n, D))              # each side has its own training inputs
        yk = side_y(Xk, j, rng)
        level = 0.0 if k == COST else float(np.median(yk) + (-0.2 if k == GE else 0.2))
        sides.append((Xk, yk, k, level))
    Xc = rng.uniform(-0.2, 1.2, (M, D))
    p = dict(name=name, X=X, y=y, sides=sides, Xc=Xc, kind=kind, ls=ls_of(ard), acq=acq, sf=sf, param=XI if acq != NONE else 0.0,
             incumbent=float(y.max() if sf > 0 else y.min()), dtypes=dtypes)
    _problems[name] = p
    if name.endswith("_underflow"):
        from oracle import gp_oracle as o
        Xk, yk, k, _ = sides[0]
        mu, sg = o.predict(o.fit(Xk, yk, kind, C, p["ls"], NOISE, JITTER, True), Xc)
        sides[0] = (Xk, yk, k, float((mu + 45.0 * sg).max()))
    return p


def fit_handle(L, dtype, X, y, kind, ls, noise=NOISE, jitter=JITTER):
    gp = L.NativeGP(0, dtype)
    gp.fit(X, y, kind, C, ls, noise, jitter, True)
    return gp


def handles(L, name, private=()):
    """the objective's handle with the batch resident and the sides' handles (those listed in `private` on a private stream);
    -> (h, [(g, kind, level), ...])"""
    p = problem(name)
    h = fit_handle(L, p["dtypes"][0], p["X"], p["y"], p["kind"], p["ls"])
    h.set_candidates(p["Xc"])
    sides = []
    for j, (Xk, yk, k, level) in enumerate(p["sides"]):
        g = fit_handle(L, p["dtypes"][1], Xk, yk, p["kind"], p["ls"])
        if j in private:
            g.set_private_stream(True)
        sides.append((g, k, level))
    return h, sides


def close(h, sides):
    for g, _, _ in sides:
        g.close()
    h.close()


def oracle_models(name):
    """[objective, side 0, ...] fitted by oracle.gp_oracle (NumPy / SciPy), once per case"""
    from oracle import gp_oracle as o
    if name not in _oracle:
        p = problem(name)
        _oracle[name] = [o.fit(p["X"], p["y"], p["kind"], C, p["ls"], NOISE, JITTER, True)] + \
                        [o.fit(Xk, yk, p["kind"], C, p["ls"], NOISE, JITTER, True) for Xk, yk, _, _ in p["sides"]]
    return _oracle[name]


def hp_fits(name):
    """the same models in long double (tests/cov_reference_hp.py), once per case"""
    import cov_reference_hp as hp
    if name not in _hp:
        p = problem(name)
        _hp[name] = [hp.Fit(p["X"], p["y"], p["kind"], C, p["ls"], NOISE, JITTER, True)] + \
                    [hp.Fit(Xk, yk, p["kind"], C, p["ls"], NOISE, JITTER, True) for Xk, yk, _, _ in p["sides"]]
    return _hp[name]


def oracle_sweep(name, Xc):
    """weighted_reference.sweep on the oracle's per-model posteriors at Xc, with those posteriors under 'post'"""
    from oracle import gp_oracle as o
    p = problem(name)
    post = [o.predict(m, Xc) for m in oracle_models(name)]
    sides = [(k, level, mu, sg) for (_, _, k, level), (mu, sg) in zip(p["sides"], post[1:])]
    r = wr.sweep(p["acq"], p["sf"], p["incumbent"], p["param"], post[0][0], post[0][1], sides)
    r["post"] = post
    return r


def partials_of_value(acq, sf, incumbent, param, post, kinds_levels):
    """(m, 2 (K + 1)): d value / d mu_j and d value / d sigma_j of every model j (objective first), by the reference's own
    gradient formula fed with unit partials"""
    K = len(kinds_levels)
    m = post[0][0].shape[0]
    dims = 2 * (K + 1)

    def unit(j, mu, sg):
        dmu, dsg = np.zeros((m, dims)), np.zeros((m, dims))
        dmu[:, 2 * j], dsg[:, 2 * j + 1] = 1.0, 1.0
        return dict(mu=np.asarray(mu, dtype=np.float64), sigma=np.asarray(sg, dtype=np.float64), dmu=dmu, dsigma=dsg)
    obj = unit(0, *post[0])
    sides = [(k, level, unit(1 + j, *post[1 + j])) for j, (k, level) in enumerate(kinds_levels)]
    return wr.grad(acq, sf, incumbent, param, obj, sides)[1]


def oracle_value_tolerance(name, r):
    """(m,) the tolerance on value against the oracle tier: tests/test_gpu_parity.py's mean and variance tolerances of every
    model (RTOL |mu| + 1e-9; RTOL var + VAR_ATOL (c + noise) y_std^2, as a deviation var_tol / (2 sigma)) propagated through
    the reference's own partial derivatives of value.  No new constant."""
    p = problem(name)
    models = oracle_models(name)
    kl = [(k, level) for _, _, k, level in p["sides"]]
    dv = np.abs(partials_of_value(p["acq"], p["sf"], p["incumbent"], p["param"], r["post"], kl))
    tol = np.zeros(r["post"][0][0].shape[0])
    for j, (mu, sg) in enumerate(r["post"]):
        mu_tol = RTOL * np.abs(mu) + 1e-9
        var_tol = RTOL * sg * sg + VAR_ATOL * (C + NOISE) * float(models[j].y_std) ** 2
        sg_tol = np.where(sg > 0, var_tol / (2.0 * np.where(sg > 0, sg, 1.0)), np.sqrt(var_tol))
        tol += dv[:, 2 * j] * mu_tol + dv[:, 2 * j + 1] * sg_tol
    return tol


def pooled_batch(name, M, score, need, pool_factor=3):
    """M rows chosen from a pool so that the reference's best score leads every other row kept by more than need(best):
    -> (Xc, position of the winner), as tests/test_gpu_integrated.py::_case builds its batches.  score(pool) -> (P,) and
    need(pool, scores, best) -> float are evaluated on the reference only."""
    rng = np.random.RandomState(4242 + M)
    pool = rng.uniform(-0.2, 1.2, (max(pool_factor * M, 128), D))
    s = score(pool)
    best = int(np.argmax(np.where(np.isnan(s), -np.inf, s)))
    gap = need(pool, s, best)
    others = [i for i in range(pool.shape[0]) if i != best and s[i] < s[best] - gap]
    assert len(others) >= M - 1, "pool too small for the required gap (%d of %d)" % (len(others), M - 1)
    keep = others[:M - 1]
    pos = (M - 1) // 3
    order = np.array(keep[:pos] + [best] + keep[pos:], dtype=np.int64)
    return np.ascontiguousarray(pool[order]), pos, gap


def logw_mp(kinds_levels, side_mu, side_sigma):
    """(logw (M,) rounded to f64, log f (K, M) rounded to f64) of the mpmath formula applied to the given bits: z and the
    sum are formed in mpmath too (60 digits)"""
    import mpmath as mp
    K, M = len(kinds_levels), side_mu.shape[1]
    logf = np.zeros((K, M))
    logw = np.zeros(M)
    with mp.workdps(60):
        for i in range(M):
            tot = mp.mpf(0)
            for k, (kind, level) in enumerate(kinds_levels):
                mu, sg = mp.mpf(float(side_mu[k, i])), mp.mpf(float(side_sigma[k, i]))
                if kind == COST:
                    lf = -mu
                elif sg == 0:
                    holds = mu >= level if kind == GE else mu <= level
                    lf = mp.mpf(0) if holds else mp.mpf("-inf")
                else:
                    z = ((mu - mp.mpf(level)) if kind == GE else (mp.mpf(level) - mu)) / sg
                    lf = mp.log1p(-mp.ncdf(-z)) if z > 0 else mp.log(mp.ncdf(z))
                logf[k, i] = float(lf)
                tot += lf
            logw[i] = float(tot)
    return logw, logf


def value_mp(acq, a, logw_ref):
    """a exp(logw) with the exponential in mpmath (0 where a == 0 or logw == -inf); logw itself for ACQ_NONE"""
    import mpmath as mp
    if acq == NONE:
        return logw_ref.copy()
    out = np.zeros(a.shape[0])
    with mp.workdps(60):
        for i in range(a.shape[0]):
            if a[i] != 0 and logw_ref[i] != -math.inf:
                out[i] = float(mp.mpf(float(a[i])) * mp.exp(mp.mpf(float(logw_ref[i]))))
    return out


def grad_references(name, f64=False):
    """(value (m,), grad (m, D), absolute (m, D)) of the case at its query points: the 80-bit closed form (every model's
    posterior and partials from tests/acq_grad_reference_hp.py on the long double fits, Phi from its erfc) or, f64=True,
    the f64 restatement on the oracle's models"""
    import acq_grad_reference_hp as ah
    p = problem(name)
    if f64:
        posts = [ah.posterior_f64(m, p["Xc"]) for m in oracle_models(name)]
    else:
        posts = [ah.posterior(f, p["Xc"]) for f in hp_fits(name)]
    sides = [(k, level, post) for (_, _, k, level), post in zip(p["sides"], posts[1:])]
    return wr.grad(p["acq"], p["sf"], p["incumbent"], p["param"], posts[0], sides)


def grad_errors(name, val, grad):
    """(worst |val - 80-bit| over max(|80-bit value|, tiny), worst entry of |grad - 80-bit| / that entry's sum of absolute
    terms; magnitudes below the smallest normal double count as that) of anything that claims to be the case's value and
    gradient"""
    rv, rg, ra = grad_references(name)
    ev = np.abs(np.asarray(val, dtype=wr.LD) - rv) / np.maximum(np.abs(rv), wr.LD(wr.TINY))
    eg = np.abs(np.asarray(grad, dtype=wr.LD) - rg) / np.maximum(ra, wr.LD(wr.TINY))
    return float(ev.max()), float(eg.max())


def grad_bar(name, e_ref):
    """64 max(e_ref, N u): the rule of tests/test_gpu_acq_grad_edges.py, N the largest model of the case"""
    No, Ns = GRAD_CASES[name][0], GRAD_CASES[name][1]
    return wr.FACTOR * max(e_ref, max([No] + list(Ns)) * wr.U)
