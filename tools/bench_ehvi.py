#!/usr/bin/env python3
"""Cost of tgp_sweep_ehvi at C1 (N = 512, M = 16 384, D = 8) and C3 (N = 4096, M = 262 144, D = 32), f32
handles, the second objective fitted on the same X, for fronts of P in {8, 64, 256}, beside what a caller does without it:
two predict-only tgp_sweep calls with their (M,) mu / sigma vectors read back, the strip sum in NumPy
(acquisition_functions._ehvi_from_posteriors) and its arg-max.
   (a) ehvi_ms       one tgp_sweep_ehvi (arg-max only)
   (b) baseline_ms   the two sweeps + NumPy
Host clock around calls that end in a stream synchronisation; after --warmup rounds, --reps rounds with (a) and (b)
alternating inside each; medians and each side's spread (max - min over the rounds).  Acceptance (profiles/README.md): (a)'s
median is below (b)'s in every cell and both name the same winner.
--grad: tgp_ehvi_grad at m = 10 and m = 64, at C1 and C3 (f64), against two tgp_acq_grad calls.
--trace: nothing is timed; the (a) side alone runs --reps times per cell, for a kernel trace of its own
(rocprofv3 --kernel-trace --stats -- python tools/bench_ehvi.py --trace --fronts 256): ehvi_value_kernel's time per launch
over (P + 1) M gives the time per strip and candidate.
One JSON line each; --out appends them to a file (profiles/ehvi.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"C1": (512, 8, 16384, "rbf"), "C3": (4096, 32, 262144, "rbf")}
SF = (-1.0, -1.0)


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


def models(L, shape, dtype):
    N, D, M, kind = SHAPES[shape]
    rng = np.random.RandomState(N)
    X = rng.uniform(0, 1, (N, D))
    y1 = np.sin(X.sum(1)) + 0.01 * rng.normal(size=N)
    y2 = np.cos(X[:, 0] * 3.0) + 0.1 * X.sum(1) + 0.01 * rng.normal(size=N)
    ls = 0.5 * np.sqrt(D)
    h, g = L.NativeGP(0, dtype), L.NativeGP(0, dtype)
    h.fit(X, y1, kind, 1.0, ls, 1e-3, 1e-10, True)
    g.fit(X, y2, kind, 1.0, ls, 1e-3, 1e-10, True)
    return h, g, y1, y2, rng


def front_of(P, y1, y2):
    """(Y, ref): a staircase of exactly P points through the observed ranges (both minimised), ref beyond the worst"""
    lo, hi = np.array([y1.min(), y2.min()]), np.array([y1.max(), y2.max()])
    t = (np.arange(P) + 0.5) / P
    Y = np.stack([lo[0] + (hi[0] - lo[0]) * t, lo[1] + (hi[1] - lo[1]) * (1.0 - t) ** 2], 1)
    return Y, hi + 0.1 * (hi - lo)


def sweep_lines(a, L, lines):
    from turbo_amd.acquisition_functions import _ehvi_from_posteriors
    for shape in a.shapes.split(","):
        N, D, M, kind = SHAPES[shape]
        h, g, y1, y2, rng = models(L, shape, "f32")
        lo, hi = np.zeros(D), np.ones(D)
        h.gen_candidates(7, 0, M, lo, hi)
        g.gen_candidates(7, 0, M, lo, hi)            # the baseline caller keeps the batch resident on both handles
        for P in (int(v) for v in a.fronts.split(",")):
            Y, ref = front_of(P, y1, y2)
            front, hv = h.ehvi_set_front(Y, ref, SF)
            assert front.shape[0] == P
            got = {}

            def ehvi():
                got["a"] = h.sweep_ehvi(g)

            def baseline():
                o1 = h.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
                o2 = g.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
                v = _ehvi_from_posteriors(front, SF, ref, o1["mu"], o1["sigma"], o2["mu"], o2["sigma"])
                v = np.where(np.isnan(v), -np.inf, v)
                got["b"] = int(np.argmax(v))
            if a.trace:
                for _ in range(a.reps):
                    ehvi()
                continue
            t = alternating({"a": ehvi, "b": baseline}, a.reps, a.warmup)
            sa, sb = stats(t["a"]), stats(t["b"])
            line = dict(workload="sweep_ehvi", date=time.strftime("%Y-%m-%d"), shape=shape, N=N, D=D, M=M, P=P, dtype="f32", reps=a.reps,
                        ehvi_ms=sa, baseline_ms=sb, same_winner=bool(got["a"]["best_idx"] == got["b"]),
                        accepted=bool(sa["median"] < sb["median"] and got["a"]["best_idx"] == got["b"]), strip_candidates=(P + 1) * M)
            s = json.dumps(line)
            print(s, flush=True)
            lines.append(s)
        g.close()
        h.close()


def grad_lines(a, L, lines):
    for shape in a.shapes.split(","):
        N, D, M, kind = SHAPES[shape]
        h, g, y1, y2, rng = models(L, shape, "f64")
        for P in (int(v) for v in a.fronts.split(",")):
            Y, ref = front_of(P, y1, y2)
            h.ehvi_set_front(Y, ref, SF)
            for m in (10, 64):
                Xq = rng.uniform(0, 1, (m, D))

                def ehvi():
                    h.ehvi_grad(Xq, g)

                def separate():
                    h.acq_grad(Xq, L.ACQ_EI, SF[0], float(ref[0]), 0.0)
                    g.acq_grad(Xq, L.ACQ_EI, SF[1], float(ref[1]), 0.0)
                if a.trace:
                    for _ in range(a.reps):
                        ehvi()
                    continue
                t = alternating({"a": ehvi, "b": separate}, a.reps, a.warmup)
                sa, sb = stats(t["a"]), stats(t["b"])
                line = dict(workload="ehvi_grad", date=time.strftime("%Y-%m-%d"), shape=shape, N=N, D=D, P=P, m=m, dtype="f64", reps=a.reps,
                            ehvi_grad_ms=sa, acq_grad_calls_ms=sb, accepted=bool(sa["median"] < sb["median"]))
                s = json.dumps(line)
                print(s, flush=True)
                lines.append(s)
        g.close()
        h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="C1,C3")
    ap.add_argument("--fronts", default="8,64,256")
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd._lib as L
    lines = []
    if not a.no_sweep:
        sweep_lines(a, L, lines)
    if a.grad:
        grad_lines(a, L, lines)
    if a.out and lines:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
