"""NumPy f64 restatement of tgp_sweep_batch_mc's greedy loop (include/turbogp.h) -- TEST INFRASTRUCTURE.

Built on oracle.gp_oracle like tests/batch_reference.py: ``select_batch`` conditions by the rank-1 updates the kernels
implement, S simulations at once -- the variance update is shared, every simulation's mean is mu0 + G eps_s -- and
averages the S acquisition functions in the order s = 0, 1, ...  ``normals`` are the Philox-4x32-10 normals of
csrc/batch_kernels.hip (counter (element lo, element hi, 0, TAG), element s 64 + j), written like ts_reference.normals.
tests/test_mc_reference.py holds the loop to S literal refits, tests/test_gpu_batch_mc.py holds the GPU to the loop.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import gp_oracle as G
from philox_ref import philox4x32_10

TAG = 0x4D435349          # "MCSI"
TWO_PI = 6.283185307179586
MAXP = 64


def _u53(a, b):
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def normals(seed, S, J):
    """eps (S, J): one Box-Muller branch per element s 64 + j: sqrt(-2 log(1 - u1)) cos(2 pi u2), u1 from words (0, 1),
    u2 from (2, 3)"""
    seed = int(seed) % (1 << 64)
    e = (np.arange(S, dtype=np.uint64)[:, None] * np.uint64(MAXP) + np.arange(J, dtype=np.uint64)[None, :]).reshape(-1)
    r = philox4x32_10(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), 0, TAG, seed & 0xFFFFFFFF, seed >> 32)
    u1, u2 = _u53(r[0], r[1]), _u53(r[2], r[3])
    return (np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(TWO_PI * u2)).reshape(S, J)


def mean_acquisition(acq_kind, mu_s, sg, desired_extremum, param, inc_s):
    """(M,) the average over the rows of mu_s (S, M) of the acquisition with incumbent inc_s[s], summed in the order
    s = 0, 1, ...; ('ucb', inf) -- TGP_ACQ_SIGMA -- is sigma itself"""
    if acq_kind == "ucb" and np.isinf(param):
        return sg.copy()
    tot = np.zeros(mu_s.shape[1])
    for s in range(mu_s.shape[0]):
        tot = tot + G.acquisition(acq_kind, mu_s[s], sg, desired_extremum, param, inc_s[s])
    return tot / float(mu_s.shape[0])


def select_batch(model, Xc, q, eps, pending, acq_kind, desired_extremum, param, incumbent, forced=None):
    """The greedy loop for eps (S, P + q).  ``forced`` (q,): teacher forcing, as batch_reference.select_batch.  Returns a
    dict: idx (q,), val (q,), best (q,), acq (list of q (M,) vectors, masked rows -inf), fantasies (S, P + q) raw units,
    sigma (M,) after all points, Z (list of the P + q conditioned points), not_pd, n_clamped_steps"""
    Xc = np.atleast_2d(np.asarray(Xc, dtype=np.float64))
    M = Xc.shape[0]
    pending = np.zeros((0, Xc.shape[1])) if pending is None else np.atleast_2d(np.asarray(pending, dtype=np.float64))
    P = pending.shape[0]
    eps = np.atleast_2d(np.asarray(eps, dtype=np.float64))
    S = eps.shape[0]
    assert eps.shape == (S, P + q)
    c, noise, jit = model.constant, model.noise, model.jitter
    ym, ys = model.y_mean, model.y_std
    Ks = G.cross_kernel(Xc, model.X, model.kind, c, model.length_scale)
    mu0 = Ks @ model.alpha
    V = solve_triangular(model.L, Ks.T, lower=True, check_finite=False)
    var = (c + noise) - np.einsum("ij,ij->j", V, V)
    var[var < 0] = 0.0
    Gc = np.zeros((M, P + q))
    R = np.zeros((P + q, P + q))
    fant = np.zeros((S, P + q))
    Z, kZ = [], []
    inc = np.full(S, float(incumbent) if incumbent is not None else 0.0)
    mask = np.zeros(M, dtype=bool)
    out = dict(idx=[], val=[], best=[], acq=[], not_pd=False, n_clamped_steps=0)

    def condition(z):
        j = len(Z)
        kz = G.cross_kernel(z[None, :], model.X, model.kind, c, model.length_scale)[0]
        w = cho_solve((model.L, True), kz, check_finite=False)
        Sj = np.empty(j + 1)
        for i in range(j):
            Sj[i] = G.cross_kernel(z[None, :], Z[i][None, :], model.kind, c, model.length_scale)[0, 0] - kZ[i] @ w
        Sj[j] = (c + noise) + jit - kz @ w
        piv = Sj[j]
        for i in range(j):
            t = (Sj[i] - R[j, :i] @ R[i, :i]) / R[i, i]
            R[j, i] = t
            piv -= t * t
        if not (piv > 0) or not np.isfinite(piv):
            out["not_pd"] = True
            piv = np.nan
        R[j, j] = np.sqrt(piv)
        m = kz @ model.alpha + eps[:, :j] @ R[j, :j]              # (S,) each simulation's mean at z before its draw
        f = ys * (m + R[j, j] * eps[:, j]) + ym                   # a draw of the observation y, raw units
        fant[:, j] = f
        cx = G.cross_kernel(Xc, z[None, :], model.kind, c, model.length_scale)[:, 0] - Ks @ w - Gc[:, :j] @ R[j, :j]
        g = cx / R[j, j]
        Gc[:, j] = g
        var[:] = var - g * g
        out["n_clamped_steps"] += int(np.count_nonzero(var < 0))
        var[var < 0] = 0.0
        Z.append(z.copy())
        kZ.append(kz)
        inc[:] = np.maximum(inc, f) if desired_extremum == "max" else np.minimum(inc, f)

    for z in pending:
        condition(z)
    for k in range(q):
        j = len(Z)
        mu_s = ym + ys * (mu0[None, :] + eps[:, :j] @ Gc[:, :j].T)      # (S, M)
        sg = np.sqrt(var * ys ** 2)
        a = mean_acquisition(acq_kind, mu_s, sg, desired_extremum, param, inc)
        a = np.where(np.isnan(a), -np.inf, a)
        a[mask] = -np.inf
        free = np.flatnonzero(~mask)
        i = int(free[np.argmax(a[free])]) if forced is None else int(forced[k])
        out["acq"].append(a)
        out["best"].append(float(np.max(a)))
        out["idx"].append(i)
        out["val"].append(float(a[i]))
        mask[i] = True
        condition(Xc[i])
    out["idx"] = np.array(out["idx"], dtype=np.int64)
    out["val"] = np.array(out["val"])
    out["best"] = np.array(out["best"])
    out["fantasies"] = fant
    out["sigma"] = np.sqrt(var * ys ** 2)
    out["Z"] = Z
    return out


def pending_y_covariance(model, Z):
    """the model's joint predictive covariance of the OBSERVATIONS y at the points Z, raw units: the posterior
    covariance of f plus (noise + jitter) on the diagonal"""
    Z = np.atleast_2d(np.asarray(Z, dtype=np.float64))
    c = model.constant
    Kzz = G.cross_kernel(Z, Z, model.kind, c, model.length_scale)
    Kzx = G.cross_kernel(Z, model.X, model.kind, c, model.length_scale)
    V = solve_triangular(model.L, Kzx.T, lower=True, check_finite=False)
    return model.y_std ** 2 * (Kzz - V.T @ V + (model.noise + model.jitter) * np.eye(len(Z)))
