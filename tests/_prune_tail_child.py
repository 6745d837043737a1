"""Child process of tests/test_gpu_prune_tail.py: TGP_PRUNE_TOP is read once per process, so the forced-survivor cases
(a small lb set, every survivor taken) run here.  Prints one JSON line per case: the full-vector sweep, the pruned sweep
and the unpruned arg-max-only sweep of the same handle, and what the pruned schedule did."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import turbo_amd as ta                      # noqa: E402

ACQ = {"ucb": 1, "pi": 2, "ei": 3}


def bits(v):
    return np.float64(v).tobytes().hex()


def rec(r):
    return dict(best_idx=int(r["best_idx"]), best_val=bits(r["best_val"]), n_clamped=int(r["n_clamped"]))


def problem(seed, N, D, M):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, size=(N, D))
    w = rng.normal(size=D) / np.sqrt(D)
    y = np.sin(3 * X @ w) + 0.5 * ((X - 0.5) ** 2).sum(1) + 0.01 * rng.normal(size=N)
    return X, y, float(np.sqrt(D / 6.0)), rng.uniform(0, 1, size=(M, D))


# kind, dtype, N, D, M, acq, sf, param, noise, tie
CASES = [
    ("rbf", "f32", 1000, 6, 9000, "ei", -1, 0.01, 1e-2, False),
    ("matern52", "f64", 300, 4, 6000, "ucb", 1, 2.0, 1e-4, False),
    ("matern32", "f32", 4096, 8, 12000, "ei", -1, 0.01, 1e-2, True),
    ("rbf", "f64", 1000, 5, 8000, "pi", -1, 0.01, 1e-3, True),
]
top = int(os.environ["TGP_PRUNE_TOP"])
for kind, dtype, N, D, M, acq, sf, param, noise, tie in CASES:
    X, y, ls, Xc = problem(N + M, N, D, M)
    gp = ta.NativeGP(0, dtype)
    gp.fit(X, y, kind, 1.0, ls, noise, 1e-10, True)
    gp.set_candidates(Xc)
    a = (ACQ[acq], float(sf), float(y.min() if sf < 0 else y.max()), float(param))
    copies = []
    if tie:
        # copies of the winner's row inside its own group of the lb set, below and above it: the group's pick is the
        # lowest copy (equal bounds, lowest index), the other copies survive with the very same exact value
        w = gp.sweep(*a, want_acq=True)["best_idx"]
        gs = (M + top - 1) // top
        g0, g1 = (w // gs) * gs, min((w // gs + 1) * gs, M)
        copies = sorted({g0 + (w - g0) // 2, w, min(w + 7, g1 - 1)})
        for j in copies:
            Xc[j] = Xc[w]
        gp.set_candidates(Xc)
    full = gp.sweep(*a, want_acq=True)
    os.environ["TGP_SWEEP_PRUNE"] = "1"
    pr = gp.sweep(*a)
    st = gp.last_prune()
    os.environ["TGP_SWEEP_PRUNE"] = "0"
    off = gp.sweep(*a)
    st_off = gp.last_prune()
    acqv = np.where(np.isnan(full["acq"]), -np.inf, full["acq"])
    print(json.dumps(dict(case=[kind, dtype, N, D, M, acq], tie=tie, copies=[int(j) for j in copies], prune=st, prune_off=st_off,
                          argmax=int(np.argmax(acqv)), full=rec(full), pruned=rec(pr), unpruned=rec(off))))
print("prune-tail ok")
