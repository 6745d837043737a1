"""The cases of test_gpu_fit_paths.py, importable (the default switches, in the test's own process) and runnable as a
child process: csrc/tuning.hpp reads the TGP_* switches once per process, so every other selection of the fit's paths
gets a process of its own.  `python _fit_paths_child.py GROUP...` prints one JSON line with a key per group.
Test helper, not product code."""
import ctypes
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

THETA = dict(kind="rbf", constant=1.0, ls=1.0, noise=0.0, jitter=0.0)   # of the not-PD constructions


def _call(gp, entry, X, y, kind, constant, ls, noise, jitter, normalize_y=True, outputs=True, n_ls=None):
    """tgp_fit / tgp_fit_append through the C ABI itself: (status, last error, lml, y_mean, y_std, appended)"""
    L = sys.modules["turbo_amd"]._lib
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    ls = np.ascontiguousarray(np.atleast_1d(ls), dtype=np.float64)
    out = [ctypes.c_double(math.nan) for _ in range(3)]
    refs = [ctypes.byref(v) if outputs else None for v in out]
    args = [gp._h, L._ptr(X), X.shape[0], X.shape[1], L._ptr(y), L.KERNELS[kind], float(constant), L._ptr(ls),
            ls.shape[0] if n_ls is None else n_ls, float(noise), float(jitter), 1 if normalize_y else 0] + refs
    flag = ctypes.c_int(-1)
    if entry == "append":
        rc = gp.lib.tgp_fit_append(*args, ctypes.byref(flag))
    else:
        rc = gp.lib.tgp_fit(*args)
    return rc, gp.lib.tgp_last_error(gp._h).decode(), out[0].value, out[1].value, out[2].value, flag.value


def _sweep_status(gp):
    """what tgp_sweep answers on the handle as it stands"""
    L = sys.modules["turbo_amd"]._lib
    rc = gp.lib.tgp_sweep(gp._h, L.ACQ_NONE, 1.0, 0.0, 0.0, None, None, None, None, None, None)
    return rc, gp.lib.tgp_last_error(gp._h).decode()


def far_apart(N, D, dup=None, seed=0):
    """N points 100 length scales apart -- every off-diagonal kernel value underflows to exactly 0, K = I -- and,
    dup = (i, j), row j a copy of row i: then L[j, i] = 1 and pivot j = 1 - 1 = 0 EXACTLY, whatever the blocking and the
    order of the sums (every other term is an exact zero)"""
    X = np.zeros((N, D))
    X[:, 0] = 100.0 * np.arange(N)
    X[:, 1:] = np.random.RandomState(seed).uniform(0, 1, (N, D - 1))
    if dup is not None:
        X[dup[1]] = X[dup[0]]
    y = np.random.RandomState(seed + 1).normal(size=N)
    return X, y


def not_pd():
    """every fit path's refusal: [status, error text, status and text of the tgp_sweep behind it]"""
    import turbo_amd as ta
    t = THETA
    res = {}
    gp = ta.NativeGP(0, "f64")
    for name, N, dup in (("small", 6, (2, 4)), ("blocked", 130, (70, 129))):
        X, y = far_apart(N, 2, dup)
        rc, err = _call(gp, "fit", X, y, t["kind"], t["constant"], t["ls"], t["noise"], t["jitter"])[:2]
        res[name] = [rc, err, *_sweep_status(gp)]
    # a copy of row 3 appended to a healthy small fit
    X, y = far_apart(7, 2, (3, 6))
    ok = _call(gp, "fit", X[:6], y[:6], t["kind"], t["constant"], t["ls"], t["noise"], t["jitter"])
    rc, err, _, _, _, appended = _call(gp, "append", X, y, t["kind"], t["constant"], t["ls"], t["noise"], t["jitter"])
    res["append"] = [rc, err, *_sweep_status(gp), ok[0], appended]
    # the second model of a batch
    Xg, yg = far_apart(5, 2)
    Xb, yb = far_apart(6, 2, (2, 4))
    spec = dict(kind=t["kind"], constant=t["constant"], length_scale=t["ls"], noise=t["noise"], jitter=t["jitter"], normalize_y=True)
    try:
        gp.predict_batch([dict(X=Xg, y=yg, **spec), dict(X=Xb, y=yb, **spec)], np.random.RandomState(3).uniform(0, 1, (9, 2)))
        res["predict_batch"] = ["no error", ""]
    except np.linalg.LinAlgError:
        res["predict_batch"] = ["LinAlgError", gp.lib.tgp_last_error(gp._h).decode()]
    gp.close()
    return res


def _problem(N, D, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X.sum(1)) + 0.05 * rng.normal(size=N)
    return X, y


def timings():
    """last_timings() after each kind of fit call: name -> [fit_ms, the three gradient stage times]"""
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    res = {}

    def note(name):
        t = gp.last_timings()
        res[name] = [float(t["fit_ms"]), float(t["grad_kinv_ms"]), float(t["grad_pairwise_ms"]), float(t["grad_ard_ms"])]

    for tag, N in (("small", 40), ("blocked", 130)):
        X, y = _problem(N + 1, 3, N)
        gp.fit(X[:N], y[:N], "matern52", 1.0, 0.7, 1e-2, 1e-10, True)
        note(tag + " fit")
        gp.fit_grad(X[:N], y[:N], "matern52", 1.0, 0.7, 1e-2, 1e-10, True)
        note(tag + " fit_grad iso")
        gp.fit_grad(X[:N], y[:N], "matern52", 1.0, np.array([0.5, 0.7, 0.9]), 1e-2, 1e-10, True)
        note(tag + " fit_grad ard")
        gp.fit(X[:N], y[:N], "matern52", 1.0, 0.7, 1e-2, 1e-10, True)
        gp.fit(X, y, "matern52", 1.0, 0.7, 1e-2, 1e-10, True, append=True)
        assert gp.appended
        note(tag + " append")
    gp.close()
    return res


def integrated_tail():
    """tgp_sweep_integrated's record with a winner buffer attached: S = 2 samples, N = 12, M = 64 candidates of which the
    first 12 ARE the training points (a tiny noise term: variances there cancel to rounding, some below 0)"""
    import torch
    import turbo_amd as ta
    L = ta._lib
    N, D, M = 12, 2, 64
    X, y = _problem(N, D, 5)
    rng = np.random.RandomState(6)
    Xc = np.vstack([X, rng.uniform(0, 1, (M - N, D))])
    thetas = np.log(np.array([[1.0, 0.4, 1e-13], [1.5, 0.7, 1e-12]]))
    gp = ta.NativeGP(0, "f64")
    gp.fit(X, y, "rbf", 1.0, 0.4, 1e-13, 1e-10, True)
    gp.set_candidates(Xc)
    per = 0                                   # the samples' own clamp counts, one plain sweep each
    for th in thetas:
        k, ls, noise = np.exp(th)
        gp.fit(X, y, "rbf", k, ls, noise, 1e-10, True)
        per += gp.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)["n_clamped"]
    rec = torch.full((D + 2,), -7.25, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    gp.set_winner_out(rec.data_ptr(), 1000, keepalive=rec)
    r = gp.sweep_integrated(X, y, "rbf", thetas, 1, 1e-10, True, acq=L.ACQ_UCB, sf=1.0, incumbent=0.0, param=2.0,
                            want_mu=True, want_sigma=True, want_acq=True)
    gp.winner_wait(None)
    torch.cuda.synchronize()
    winner = rec.cpu().numpy()
    r2 = gp.sweep_integrated(X, y, "rbf", thetas, 1, 1e-10, True, acq=L.ACQ_UCB, sf=1.0, incumbent=0.0, param=2.0)
    gp.close()
    return dict(acq=r["acq"].tobytes().hex(), mu=r["mu"].tobytes().hex(), sigma=r["sigma"].tobytes().hex(),
                best_val=float(r["best_val"]).hex(), best_idx=int(r["best_idx"]), n_clamped=int(r["n_clamped"]),
                argmax=int(np.argmax(r["acq"])), clamped_per_sample=int(per), winner=winner.tobytes().hex(),
                record_only=[float(r2["best_val"]).hex(), int(r2["best_idx"]), int(r2["n_clamped"])],
                winner_row=Xc[int(r["best_idx"])].tobytes().hex())


GROUPS = dict(not_pd=not_pd, timings=timings, integrated_tail=integrated_tail)

if __name__ == "__main__":
    print("fit-paths " + json.dumps({g: GROUPS[g]() for g in sys.argv[1:]}))
