"""Child process of tests/test_gpu_prune_screen.py (the pruned sweep's switches are read per call or once per process, and a
child keeps the parent's environment out of it).  One JSON line per case: the winner record of the same handle and batch under
TGP_PRUNE_SCREEN=1 (twice), TGP_PRUNE_SCREEN=0 and TGP_SWEEP_PRUNE=0, and what the pruned schedule did each time.

    _prune_screen_child.py grid      the shape x acquisition x sense x length-scale grid
    _prune_screen_child.py giveway   the cases where the screen must give way"""
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACQ = {"ucb": 1, "pi": 2, "ei": 3}
NS, MS, DS = (257, 300, 1000), (1000, 4099), (1, 5, 32, 40)
CONSTANT, NOISE = 0.1, 1e-2
# every switch of the pruned sweep's schedule (csrc/tuning.hpp): the parent strips them, run() sets them per call
SWITCHES = ("TGP_SWEEP_PRUNE", "TGP_PRUNE_SCREEN", "TGP_PRUNE_FRAC", "TGP_PRUNE_DIRECT", "TGP_PRUNE_MIN_WORK", "TGP_PRUNE_TOP",
            "TGP_PRUNE_TAU", "TGP_PRUNE_MARGIN")


def bits(v):
    return np.float64(v).tobytes().hex()


def rec(r):
    return dict(best_idx=int(r["best_idx"]), best_val=bits(r["best_val"]), n_clamped=int(r["n_clamped"]))


def problem(N, D, M, ard, const_y=False):
    """a smooth target with a wide spread of means, and a length scale under which most of the batch lies between the
    training points: the bounds then separate the batch (checked on the CPU with the oracle when the grid was chosen)"""
    rng = np.random.RandomState(7919 * N + 31 * D + M + (1 if ard else 0))
    X = rng.uniform(0, 0.4 if D == 1 else 1, size=(N, D))     # (one dimension: the data cover part of the batch's range only)
    w = rng.normal(size=D) / np.sqrt(D)
    bump = lambda x0: np.exp(-((X - x0) ** 2).sum(1) / (2 * 0.0625 * D))
    y = np.sin(3 * X @ w) + 4.0 * (bump(0.3 if D == 1 else 0.7) - bump(0.1 if D == 1 else 0.3)) + 0.01 * rng.normal(size=N)     # one deep well, one high peak
    if const_y:
        y = np.full(N, 0.5)
    ls = np.sqrt(D / 6.0) * (np.logspace(-0.5, 0.5, D) if ard and D > 1 else np.ones(D))
    if D == 1:
        ls = np.array([0.05 if ard else 0.08])
    return X, y, ls, rng.uniform(0, 1, size=(M, D))


def grid_cases():
    for N, M, D, acq, sense, ard in itertools.product(NS, MS, DS, ("ei", "pi", "ucb"), ("min", "max"), (False, True)):
        yield N, M, D, acq, sense, ard


def acq_args(acq, sense, y):
    sf = -1.0 if sense == "min" else 1.0
    return ACQ[acq], sf, float(y.min() if sf < 0 else y.max()), (0.5 if acq == "ucb" else 0.01)


def run(gp, a, env):
    for k in SWITCHES[:4]:
        os.environ.pop(k, None)
    os.environ.update(env)
    r = gp.sweep(*a)
    return rec(r), gp.last_prune()


def main(which):
    import turbo_amd as ta
    os.environ["TGP_PRUNE_MIN_WORK"] = "0"
    if which == "grid":
        for N, M, D, acq, sense, ard in grid_cases():
            X, y, ls, Xc = problem(N, D, M, ard)
            gp = ta.NativeGP(0, "f32")
            gp.fit(X, y, "rbf", CONSTANT, ls if ard else float(ls[0]), NOISE, 1e-10, True)
            gp.set_candidates(Xc)
            a = acq_args(acq, sense, y)
            s1, p1 = run(gp, a, {"TGP_PRUNE_SCREEN": "1"})
            s1b, p1b = run(gp, a, {"TGP_PRUNE_SCREEN": "1"})
            s0, p0 = run(gp, a, {"TGP_PRUNE_SCREEN": "0"})
            off, poff = run(gp, a, {"TGP_SWEEP_PRUNE": "0"})
            print(json.dumps(dict(case=[N, M, D, acq, sense, ard], screen=s1, again=s1b, noscreen=s0, unpruned=off,
                                  p_screen=p1, p_again=p1b, p_noscreen=p0, p_unpruned=poff)), flush=True)
    else:
        N, M, D = 1000, 4099, 5
        X, y, ls, Xc = problem(N, D, M, False)
        # (name, kind, dtype, const_y, environment of the screened run)
        for name, kind, dtype, const_y, env in (
                ("ties", "rbf", "f32", True, {}),
                ("matern", "matern52", "f32", False, {}),
                ("f64", "rbf", "f64", False, {}),
                ("direct", "rbf", "f32", False, {"TGP_PRUNE_FRAC": "1", "TGP_PRUNE_DIRECT": "100000"}),
                ("gathered", "rbf", "f32", False, {"TGP_PRUNE_FRAC": "1", "TGP_PRUNE_DIRECT": "0"}),
                ("tight_all", "rbf", "f32", False, {"TGP_PRUNE_FRAC": "0.0001", "TGP_PRUNE_DIRECT": "0"})):
            yy = problem(N, D, M, False, const_y)[1]
            gp = ta.NativeGP(0, dtype)
            gp.fit(X, yy, kind, CONSTANT, float(ls[0]), NOISE, 1e-10, True)
            gp.set_candidates(Xc)
            a = acq_args("ei", "min", yy)
            e1 = dict(env, TGP_PRUNE_SCREEN="1")
            s1, p1 = run(gp, a, e1)
            s1b, p1b = run(gp, a, e1)
            s0, p0 = run(gp, a, dict(env, TGP_PRUNE_SCREEN="0"))
            off, poff = run(gp, a, {"TGP_SWEEP_PRUNE": "0"})
            print(json.dumps(dict(case=name, screen=s1, again=s1b, noscreen=s0, unpruned=off, p_screen=p1, p_again=p1b,
                                  p_noscreen=p0, p_unpruned=poff)), flush=True)
    print("prune-screen ok")


if __name__ == "__main__":
    main(sys.argv[1])
