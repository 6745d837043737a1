"""Time the integrated acquisition: ``tgp_sweep_integrated`` at S = 8 against what a caller of the plain API must do for the
same result -- S x (``tgp_fit`` + ``tgp_sweep`` with ``acq_out``), a NumPy mean and an arg-max -- and one ``tgp_hyper_sample``
chain per size.  One JSON line per case, appended to profiles/integrated_select.jsonl.

    python tools/bench_integrated.py [--reps 20] [--out profiles/integrated_select.jsonl]

Cases: N = 32, D = 2, M = 10^4 (turbo's everyday regime) and C3 (N = 4096, D = 32, M = 262 144, f32 sweep)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [dict(name="n32_m1e4", N=32, D=2, M=10000, dtype="f64", reps_scale=1.0),
         dict(name="c3", N=4096, D=32, M=262144, dtype="f32", reps_scale=0.25)]


def run_case(L, case, S, reps):
    rng = np.random.RandomState(0)
    N, D, M = case["N"], case["D"], case["M"]
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X.sum(1) / np.sqrt(D)) + 0.01 * rng.normal(size=N)
    Xc = rng.uniform(0, 1, (M, D))
    base = np.log([1.0, 0.5 * np.sqrt(D), 1e-3])
    thetas = base + 0.1 * rng.normal(size=(S, 3))
    inc = float(y.min())
    gp = L.NativeGP(0, case["dtype"])
    gp.fit(X, y, "matern52", 1.0, 0.5 * np.sqrt(D), 1e-3, 1e-10, True)
    gp.set_candidates(Xc)

    def integrated():
        return gp.sweep_integrated(X, y, "matern52", thetas, 1, 1e-10, True, L.ACQ_EI, -1.0, inc, 0.01)

    def by_hand():
        total = None
        for th in thetas:
            gp.fit(X, y, "matern52", math.exp(th[0]), math.exp(th[1]), math.exp(th[2]), 1e-10, True)
            a = gp.sweep(L.ACQ_EI, -1.0, inc, 0.01, want_acq=True)["acq"]
            total = a.copy() if total is None else total + a
        total /= S
        i = int(np.argmax(np.where(np.isnan(total), -np.inf, total)))
        return i, float(total[i])

    reps = max(3, int(reps * case["reps_scale"]))
    out = {}
    for name, fn in (("integrated_ms", integrated), ("by_hand_ms", by_hand)):
        fn()
        fn()                                   # warm: allocations, code objects
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)), reps=reps)
    r, (i, v) = integrated(), by_hand()
    out["same_winner"] = bool(r["best_idx"] == i)
    out["winner_rel_diff"] = float(abs(r["best_val"] - v) / max(abs(v), 1e-300))
    lb = np.stack([base - 3.0, base + 3.0], 1)
    t0 = time.perf_counter()
    _, _, evals, not_pd = gp.hyper_sample(X, y, "matern52", base, 1, lb, 1e-10, True, n_samples=S, burn=20, thin=5, seed=1)
    out["hyper_sample"] = dict(wall_ms=(time.perf_counter() - t0) * 1e3, evaluations=int(evals), not_pd=int(not_pd),
                               n_samples=S, burn=20, thin=5)
    gp.close()
    return dict(case=case["name"], N=N, D=D, M=M, S=S, dtype=case["dtype"], acq="ei", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--cases", default="n32_m1e4,c3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "integrated_select.jsonl"))
    a = ap.parse_args()
    import turbo_amd._lib as L
    with open(a.out, "a") as f:
        for case in CASES:
            if case["name"] not in a.cases.split(","):
                continue
            line = json.dumps(run_case(L, case, a.samples, a.reps))
            print(line)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
