#!/usr/bin/env python3
"""Times of tgp_fit_input_grad and tgp_fit_warp_grad beside tgp_fit_grad on the blocked route at N = 512, 2048, 4096 with
D = 8 and 32 (Matern-5/2, ARD), and of tgp_warp_candidates beside the tgp_sweep it precedes at C3's batch (262 144 x 32,
N = 4096, f32 handle); one JSON line per shape; --out appends them to a file (profiles/input_grad.jsonl).

  * the three fit entries are taken in INTERLEAVED rounds -- fit_grad, fit_input_grad, fit_warp_grad, then again -- so that
    whatever else the host and the card are doing falls on all three alike; `*_wall_ms` are medians of --reps synchronous
    calls on the host clock after --warmup rounds (every call ends in the library's own synchronisation), min and max
    beside them: the spread;
  * tgp_fit_grad is called with the one-workgroup route off (N >= 512 takes the blocked route anyway), so the differences
    are the input-gradient pass, its D2H copy, and the warp's kernel, copies and chain-rule reduction;
  * the kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script (--trace-shape N,D: one shape,
    few repetitions, no candidate part), where input_grad_kernel stands beside lml_weights_kernel at the same (N, D).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stat(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def fit_shapes(L, N, D, reps, warmup):
    rng = np.random.RandomState(N + D)
    lo, hi = np.zeros(D), np.ones(D)
    X = np.ascontiguousarray(rng.uniform(0, 1, (N, D)))
    y = np.sin(3 * X.sum(1)) + 0.01 * rng.normal(size=N)
    ls = np.full(D, 0.6 * np.sqrt(D)) * (1.0 + 0.02 * np.arange(D))
    a, b = np.linspace(0.7, 1.6, D), np.linspace(1.4, 0.8, D)
    gp = L.NativeGP(0, "f64")
    args = (X, y, "matern52", 1.0, ls, 1e-3, 1e-10, True)
    calls = dict(fit_grad=lambda: gp.fit_grad(*args), fit_input_grad=lambda: gp.fit_input_grad(*args),
                 fit_warp_grad=lambda: gp.fit_warp_grad(*args, lo, hi, a, b))
    t = {k: [] for k in calls}
    for r in range(warmup + reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            if r >= warmup:
                t[k].append((time.perf_counter() - t0) * 1e3)
    gp.close()
    rec = dict(what="fit", N=N, D=D, kind="matern52", ard=True, reps=reps, poll_us=os.environ.get("TGP_POLL_US", "default"))
    for k in calls:
        rec[k + "_wall_ms"] = stat(t[k])
    rec["input_grad_over_fit_grad"] = rec["fit_input_grad_wall_ms"]["median"] / rec["fit_grad_wall_ms"]["median"]
    rec["warp_grad_over_fit_grad"] = rec["fit_warp_grad_wall_ms"]["median"] / rec["fit_grad_wall_ms"]["median"]
    return rec


def candidate_shape(L, reps, warmup, N=4096, D=32, M=262144):
    rng = np.random.RandomState(3)
    X = np.ascontiguousarray(rng.uniform(0, 1, (N, D)))
    y = np.sin(3 * X.sum(1)) + 0.01 * rng.normal(size=N)
    lo, hi = np.zeros(D), np.ones(D)
    gp = L.NativeGP(0, "f32")
    gp.fit(X, y, "rbf", 1.0, 0.6 * np.sqrt(D), 1e-3, 1e-10, True)        # (C3: 32-D RBF, EI)
    gp.generate(7, 0, M, lo, hi)
    a, b = np.linspace(0.7, 1.6, D), np.linspace(1.4, 0.8, D)
    t = dict(warp_candidates=[], sweep=[])
    for r in range(warmup + reps):
        t0 = time.perf_counter()
        gp.warp_candidates(lo, hi, a * (1.0 + 0.01 * r), b)          # (a re-warp from the raw rows: what a trial with a prefetched batch pays)
        t1 = time.perf_counter()
        gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01)
        t2 = time.perf_counter()
        if r >= warmup:
            t["warp_candidates"].append((t1 - t0) * 1e3)
            t["sweep"].append((t2 - t1) * 1e3)
    gp.close()
    rec = dict(what="candidates", N=N, D=D, M=M, kind="rbf", dtype="f32", reps=reps, warp_candidates_wall_ms=stat(t["warp_candidates"]), sweep_wall_ms=stat(t["sweep"]))
    rec["warp_over_sweep"] = rec["warp_candidates_wall_ms"]["median"] / rec["sweep_wall_ms"]["median"]
    rec["warp_bytes"] = 2 * M * D * 8
    rec["warp_tbs_over_wall"] = rec["warp_bytes"] / (rec["warp_candidates_wall_ms"]["median"] * 1e-3) / 1e12
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="512,2048,4096")
    ap.add_argument("--dims", default="8,32")
    ap.add_argument("--trace-shape", default=None, help="N,D: that one fit shape only (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd._lib as L
    L.load()
    lines = []
    if a.trace_shape:
        N, D = map(int, a.trace_shape.split(","))
        lines.append(json.dumps(fit_shapes(L, N, D, a.reps, a.warmup)))
        print(lines[-1], flush=True)
    else:
        for N in map(int, a.sizes.split(",")):
            for D in map(int, a.dims.split(",")):
                lines.append(json.dumps(fit_shapes(L, N, D, a.reps, a.warmup)))
                print(lines[-1], flush=True)
        lines.append(json.dumps(candidate_shape(L, a.reps, a.warmup)))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
