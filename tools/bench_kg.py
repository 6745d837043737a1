#!/usr/bin/env python3
"""Cost of tgp_sweep_kg at C1-C3-like shapes for A in {16, 64, 256} discretisation points, beside the
unpruned predict-only sweep of the SAME handle on the SAME batch -- the call's own step 1 and the baseline the ratio is
quoted against.  One JSON line per (shape, dtype, A); --out appends them to a file (profiles/kg.jsonl).  Times are
medians of --reps calls after --warmup:
  kg_call_ms            the whole synchronous tgp_sweep_kg on the host clock (arg-max only: no (M,) output copied back)
  kg_kernels_device_ms  tgp_last_timings slot 20: cross-kernel + cross-covariance + envelope between events, chunk by chunk
  predict_sweep_ms      tgp_sweep(TGP_ACQ_NONE, mu and sigma asked for) on the host clock, its device time beside it
  set_points_ms         tgp_kg_set_points on the host clock (once per fit and point set)
  cross_cov_fraction_of_attainable_f64   2 M Np A flops over slot 20's time against the f64 MFMA rate
                        tools/microbench/mfma_f64_peak measured (66.8 TFLOP/s) -- the whole slot, so the cross-kernel
                        (M Np (3 D + ~20) flops on the vector pipe) and the envelope are in the denominator too."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ATTAINABLE_F64_TFLOPS = 66.8
SHAPES = {"C1": (512, 8, 65536, "rbf"), "C2": (2048, 16, 131072, "matern52"), "C3": (4096, 32, 262144, "rbf")}


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="C1,C2,C3")
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--points", default="16,64,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd._lib as L
    lines = []
    for shape in a.shapes.split(","):
        N, D, M, kind = SHAPES[shape]
        rng = np.random.RandomState(N)
        X = rng.uniform(0, 1, (N, D))
        y = np.sin(X.sum(1)) + 0.01 * rng.normal(size=N)
        for dtype in a.dtypes.split(","):
            gp = L.NativeGP(0, dtype)
            gp.fit(X, y, kind, 1.0, 0.5 * np.sqrt(D), 1e-3, 1e-10, True)
            gp.generate(1, 0, M, [0.0] * D, [1.0] * D)
            _, Np = gp.sweep_geometry()
            sweep_dev = []
            sweep_ms = median_ms(lambda: (gp.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True),
                                          sweep_dev.append(gp.last_timings()["sweep_ms"])), a.reps, a.warmup)
            Np = gp.sweep_geometry()[1]
            for A in (int(v) for v in a.points.split(",")):
                Xa = np.ascontiguousarray(X[np.argsort(y, kind="stable")[:A]])
                set_ms = median_ms(lambda: gp.kg_set_points(Xa), max(a.reps // 2, 1), 1)
                dev = []
                call_ms = median_ms(lambda: dev.append(gp.sweep_kg(1.0)["kg_ms"]), a.reps, a.warmup)
                kg_dev = float(np.median(dev[a.warmup:]))
                flops = 2.0 * M * Np * A
                line = dict(workload="sweep_kg", date=time.strftime("%Y-%m-%d"), shape=shape, N=N, Np=int(Np), D=D, M=M, A=A,
                            kernel=kind, dtype=dtype, kg_call_ms=call_ms, kg_kernels_device_ms=kg_dev,
                            predict_sweep_ms=sweep_ms, predict_sweep_device_ms=float(np.median(sweep_dev[a.warmup:])),
                            kg_call_over_predict_sweep=call_ms / sweep_ms, set_points_ms=set_ms,
                            cross_cov_gflop=flops / 1e9,
                            cross_cov_fraction_of_attainable_f64=flops / (kg_dev * 1e-3) / (ATTAINABLE_F64_TFLOPS * 1e12))
                s = json.dumps(line)
                print(s, flush=True)
                lines.append(s)
            gp.close()
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
