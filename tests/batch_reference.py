"""NumPy f64 restatement of tgp_sweep_batch's greedy loop (include/turbogp.h) -- TEST INFRASTRUCTURE.

Built on oracle.gp_oracle.  ``select_batch`` conditions by the rank-1 updates the kernels implement (normalised units,
hyper-parameters and y_mean / y_std held); ``refit_posterior`` is the literal refit the contract defines them by: fit on
the real points plus the fantasised ones, pre-normalised, with normalize_y=False and the kernel held.
tests/test_batch_reference.py holds the first to the second; tests/test_gpu_batch.py holds the GPU to the first.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import gp_oracle as G

KB, CL = "kriging_believer", "constant_liar"


def resolve_lie(lie, y):
    """'min' / 'max' / 'mean' of the observed raw y, or the float itself"""
    if isinstance(lie, str):
        return float({"min": np.min, "max": np.max, "mean": np.mean}[lie](np.asarray(y, dtype=np.float64)))
    return float(lie)


def _best(inc, f, desired_extremum):
    return max(inc, f) if desired_extremum == "max" else min(inc, f)


def select_batch(model, Xc, q, strategy, lie, pending, acq_kind, desired_extremum, param, incumbent, forced=None):
    """The greedy loop.  ``forced`` (q,): teacher forcing -- take these candidate rows instead of this loop's own
    arg-max (the acquisition of every step is still recorded).  Returns a dict: idx (q,), val (q,) = acquisition at
    each taken row, best (q,) = the step's best unmasked acquisition, acq (list of q (M,) vectors, masked rows -inf),
    fantasies (P + q,), mu / sigma (M,) after all P + q points, not_pd (bool), n_clamped_steps = the (candidate, point)
    pairs of the P + q updates whose variance fell below 0 before the clamp (the first sweep's clamps not included),
    min_abs_prevar = the smallest |variance before the clamp| of those updates (normalised units): where it is far above
    the rounding of the variance, the count does not depend on the arithmetic's last digits."""
    Xc = np.atleast_2d(np.asarray(Xc, dtype=np.float64))
    M = Xc.shape[0]
    pending = np.zeros((0, Xc.shape[1])) if pending is None else np.atleast_2d(np.asarray(pending, dtype=np.float64))
    P = pending.shape[0]
    c, noise, jit = model.constant, model.noise, model.jitter
    ym, ys = model.y_mean, model.y_std
    Ks = G.cross_kernel(Xc, model.X, model.kind, c, model.length_scale)
    mu_n = Ks @ model.alpha
    V = solve_triangular(model.L, Ks.T, lower=True, check_finite=False)
    var = (c + noise) - np.einsum("ij,ij->j", V, V)
    var[var < 0] = 0.0
    Gc = np.zeros((M, P + q))
    R = np.zeros((P + q, P + q))
    e = np.zeros(P + q)
    Z, kZ, fant = [], [], []
    inc = float(incumbent) if incumbent is not None else 0.0
    mask = np.zeros(M, dtype=bool)
    out = dict(idx=[], val=[], best=[], acq=[], not_pd=False, n_clamped_steps=0, min_abs_prevar=np.inf)

    def condition(z):
        j = len(Z)
        kz = G.cross_kernel(z[None, :], model.X, model.kind, c, model.length_scale)[0]
        w = cho_solve((model.L, True), kz, check_finite=False)
        S = np.empty(j + 1)
        for i in range(j):
            S[i] = G.cross_kernel(z[None, :], Z[i][None, :], model.kind, c, model.length_scale)[0, 0] - kZ[i] @ w
        S[j] = (c + noise) + jit - kz @ w
        m = kz @ model.alpha
        piv = S[j]
        for i in range(j):
            t = (S[i] - R[j, :i] @ R[i, :i]) / R[i, i]
            R[j, i] = t
            piv -= t * t
            m += t * e[i]
        if not (piv > 0) or not np.isfinite(piv):
            out["not_pd"] = True
            piv = np.nan
        R[j, j] = np.sqrt(piv)
        f = ys * m + ym if strategy == KB else float(lie)
        e[j] = 0.0 if strategy == KB else ((f - ym) / ys - m) / R[j, j]
        cx = G.cross_kernel(Xc, z[None, :], model.kind, c, model.length_scale)[:, 0] - Ks @ w - Gc[:, :j] @ R[j, :j]
        g = cx / R[j, j]
        Gc[:, j] = g
        var[:] = var - g * g
        out["n_clamped_steps"] += int(np.count_nonzero(var < 0))
        out["min_abs_prevar"] = min(out["min_abs_prevar"], float(np.min(np.abs(var))))
        var[var < 0] = 0.0
        mu_n[:] = mu_n + g * e[j]
        Z.append(z.copy())
        kZ.append(kz)
        fant.append(f)
        return f

    for z in pending:
        inc = _best(inc, condition(z), desired_extremum)
    for k in range(q):
        mu = ys * mu_n + ym
        sg = np.sqrt(var * ys ** 2)
        a = G.acquisition(acq_kind, mu, sg, desired_extremum, param, inc)
        a = np.where(np.isnan(a), -np.inf, a)
        a[mask] = -np.inf
        # (the lowest unmasked index among the largest values: a masked row never wins, even when every value is -inf)
        free = np.flatnonzero(~mask)
        i = int(free[np.argmax(a[free])]) if forced is None else int(forced[k])
        out["acq"].append(a)
        out["best"].append(float(np.max(a)))
        out["idx"].append(i)
        out["val"].append(float(a[i]))
        mask[i] = True
        inc = _best(inc, condition(Xc[i]), desired_extremum)
    out["idx"] = np.array(out["idx"], dtype=np.int64)
    out["val"] = np.array(out["val"])
    out["best"] = np.array(out["best"])
    out["fantasies"] = np.array(fant)
    out["mu"] = ys * mu_n + ym
    out["sigma"] = np.sqrt(var * ys ** 2)
    return out


def refit_posterior(model, yn, Zs, fant, Xc):
    """The literal refit: oracle.fit on [X; Z] with [yn; (fant - y_mean) / y_std], normalize_y=False, the kernel and
    jitter held; returns (mu, sigma) at Xc in raw units."""
    X = np.vstack([model.X] + [np.atleast_2d(z) for z in Zs]) if len(Zs) else model.X
    y = np.concatenate([yn, (np.asarray(fant, dtype=np.float64) - model.y_mean) / model.y_std])
    m2 = G.fit(X, y, model.kind, model.constant, model.length_scale, model.noise, model.jitter, normalize_y=False)
    mu, sg = G.predict(m2, Xc)
    return model.y_std * mu + model.y_mean, model.y_std * sg
