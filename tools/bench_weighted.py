#!/usr/bin/env python3
"""Cost of tgp_sweep_weighted at C3 (N = 4096, M = 262 144, D = 32, f32 handles; the K sides fitted on the same
X) for K in {1, 2, 4}, beside what a caller does without it: K + 1 predict-only tgp_sweep calls with their (M,) mu / sigma
vectors read back, the product in NumPy (acquisition_functions._weighted_from_posteriors) and its arg-max.
   (a) weighted_ms   one tgp_sweep_weighted (arg-max only)
   (b) baseline_ms   the K + 1 sweeps + NumPy
Host clock around calls that end in a stream synchronisation; after --warmup rounds, --reps rounds with (a) and (b)
alternating inside each; medians and each side's spread (max - min over the rounds).  Acceptance (profiles/README.md):
(a)'s median is no larger than (b)'s median plus (b)'s own round-to-round spread.
--bytes: the byte counts the script computes from the shapes -- 32 B per candidate and side for the accumulation (mu, sigma
read, logw read and written), 2 x 8 M D per side for the device-to-device copy -- to set beside a kernel trace.
--grad: tgp_weighted_grad at m = 10 and m = 64, at C1 and C3 (f64), against K + 1 tgp_acq_grad calls.
One JSON line each; --out appends them to a file (profiles/weighted.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"C1": (512, 8, 16384, "rbf"), "C3": (4096, 32, 262144, "rbf")}


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)), spread=float(np.max(t) - np.min(t)))


def alternating(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return out


def models(L, shape, dtype, K, seed=0):
    N, D, M, kind = SHAPES[shape]
    rng = np.random.RandomState(N + seed)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(X.sum(1)) + 0.01 * rng.normal(size=N)
    ls = 0.5 * np.sqrt(D)
    h = L.NativeGP(0, dtype)
    h.fit(X, y, kind, 1.0, ls, 1e-3, 1e-10, True)
    sides = []
    for k in range(K):
        g = L.NativeGP(0, dtype)
        yk = np.cos(X[:, k % D] * 3.0 + k) + 0.1 * X.sum(1) + 0.01 * rng.normal(size=N)
        g.fit(X, yk, kind, 1.0, ls, 1e-3, 1e-10, True)
        sides.append((g, ("ge", "le", "cost")[k % 3], 0.0 if k % 3 == 2 else float(np.median(yk))))
    return h, sides, X, y, rng


def sweep_lines(a, L, lines):
    from turbo_amd.acquisition_functions import _weighted_from_posteriors
    N, D, M, kind = SHAPES["C3"]
    for K in (int(v) for v in a.sides.split(",")):
        h, sides, X, y, rng = models(L, "C3", "f32", K)
        lo, hi = np.zeros(D), np.ones(D)
        h.gen_candidates(7, 0, M, lo, hi)
        for g, _, _ in sides:                       # the baseline caller keeps the batch resident on every handle
            g.gen_candidates(7, 0, M, lo, hi)
        inc = float(y.min())
        got = {}

        def weighted():
            got["a"] = h.sweep_weighted(sides, L.ACQ_EI, -1.0, inc, 0.01)

        def baseline():
            o = h.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
            post = []
            for g, kind_k, level in sides:
                s = g.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
                post.append((L.SIDE_KINDS[kind_k], level, s["mu"], s["sigma"]))
            v = _weighted_from_posteriors(L.ACQ_EI, -1.0, inc, 0.01, o["mu"], o["sigma"], post)
            v = np.where(np.isnan(v), -np.inf, v)
            got["b"] = int(np.argmax(v))
        t = alternating({"a": weighted, "b": baseline}, a.reps, a.warmup)
        sa, sb = stats(t["a"]), stats(t["b"])
        line = dict(workload="sweep_weighted", date=time.strftime("%Y-%m-%d"), shape="C3", N=N, D=D, M=M, K=K, dtype="f32", reps=a.reps,
                    weighted_ms=sa, baseline_ms=sb, same_winner=bool(got["a"]["best_idx"] == got["b"]),
                    accepted=bool(sa["median"] <= sb["median"] + sb["spread"]),
                    accumulate_bytes_per_side=32 * M, copy_bytes_per_side=2 * 8 * M * D)
        s = json.dumps(line)
        print(s, flush=True)
        lines.append(s)
        for g, _, _ in sides:
            g.close()
        h.close()


def grad_lines(a, L, lines):
    for shape in ("C1", "C3"):
        N, D, M, kind = SHAPES[shape]
        for K in (int(v) for v in a.sides.split(",")):
            h, sides, X, y, rng = models(L, shape, "f64", K)
            inc = float(y.min())
            for m in (10, 64):
                Xq = rng.uniform(0, 1, (m, D))

                def weighted():
                    h.weighted_grad(Xq, sides, L.ACQ_EI, -1.0, inc, 0.01)

                def separate():
                    h.acq_grad(Xq, L.ACQ_EI, -1.0, inc, 0.01)
                    for g, _, _ in sides:
                        g.acq_grad(Xq, L.ACQ_NONE)
                t = alternating({"a": weighted, "b": separate}, a.reps, a.warmup)
                line = dict(workload="weighted_grad", date=time.strftime("%Y-%m-%d"), shape=shape, N=N, D=D, K=K, m=m, dtype="f64",
                            reps=a.reps, weighted_grad_ms=stats(t["a"]), acq_grad_calls_ms=stats(t["b"]))
                s = json.dumps(line)
                print(s, flush=True)
                lines.append(s)
            for g, _, _ in sides:
                g.close()
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sides", default="1,2,4")
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd._lib as L
    lines = []
    if not a.no_sweep:
        sweep_lines(a, L, lines)
    if a.grad:
        grad_lines(a, L, lines)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
