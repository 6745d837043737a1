#!/usr/bin/env python3
"""Device time of tgp_predict_cov / tgp_sample_joint at three shapes, with what there is to compare them to -- nothing on
the parent commit does this job:
  * the same matrices from SciPy on the host's threads (solve_triangular + V^T V; cholesky + a product),
  * the groups-of-16 route of tgp_acq_grad's kernels for V (its launch_query front, timed through tgp_acq_grad over the
    same points: the GEMV-shaped path the stored product replaces) -- the plain GEMM that would follow it is MODELLED at
    the attainable f64 MFMA rate, not run,
  * the fraction of the attainable f64 MFMA rate (66.8 TFLOP/s: tools/microbench/mfma_f64_peak) the algorithmic flops
    (m N^2 for the triangular product + m^2 N for the symmetric update; + m^3 / 3 + S m^2 for the samples) come to.
One JSON line per shape; --out appends them to a file (profiles/predict_cov.jsonl).  Times are medians of --reps calls
after --warmup; `*_device_ms` is tgp_last_timings slot 15 (the kernels between two events, copies left out), `*_wall_ms`
the whole synchronous call on the host clock (H2D of the points, D2H of the (m, m) matrix included)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ATTAINABLE_F64_TFLOPS = 66.8


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=512)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd._lib as L
    from scipy.linalg import cholesky, solve_triangular
    from oracle import gp_oracle as G
    lines = []
    for N, D, m in ((4096, 32, 4096), (4096, 32, 512), (512, 32, 512)):
        rng = np.random.RandomState(N + m)
        X = rng.uniform(0, 1, (N, D))
        y = np.sin(X.sum(1)) + 0.01 * rng.normal(size=N)
        Xq = rng.uniform(0, 1, (m, D))
        gp = L.NativeGP(0, "f64")
        gp.fit(X, y, "matern52", 1.0, 1.5, 1e-3, 1e-10, True)
        S = a.samples
        dev = lambda: float(np.asarray(_timings(gp))[15])
        cov_dev, smp_dev = [], []
        cov_wall = median_ms(lambda: (gp.predict_cov(Xq), cov_dev.append(dev())), a.reps, a.warmup)
        smp_wall = median_ms(lambda: (gp.sample_joint(Xq, S, seed=1, nugget=1e-8), smp_dev.append(dev())), a.reps, a.warmup)
        grad_wall = median_ms(lambda: gp.acq_grad(Xq, L.ACQ_NONE), a.reps, a.warmup)
        cov_ms, smp_ms = float(np.median(cov_dev[a.warmup:])), float(np.median(smp_dev[a.warmup:]))
        f_cov = m * float(N) ** 2 + float(m) ** 2 * N
        f_smp = f_cov + float(m) ** 3 / 3.0 + S * float(m) ** 2
        line = dict(workload="predict_cov", date=time.strftime("%Y-%m-%d"), N=N, D=D, m=m, S=S, kernel="matern52",
                    predict_cov_device_ms=cov_ms, predict_cov_wall_ms=cov_wall, sample_joint_device_ms=smp_ms,
                    sample_joint_wall_ms=smp_wall, predict_cov_algorithmic_gflop=f_cov / 1e9,
                    predict_cov_fraction_of_attainable_f64=f_cov / (cov_ms * 1e-3) / (ATTAINABLE_F64_TFLOPS * 1e12),
                    sample_joint_fraction_of_attainable_f64=f_smp / (smp_ms * 1e-3) / (ATTAINABLE_F64_TFLOPS * 1e12),
                    groups_of_16_route_wall_ms=grad_wall,
                    groups_of_16_note="tgp_acq_grad(TGP_ACQ_NONE) over the same points: v = Linv k* AND w = Linv^T v per point on "
                                      "q_rows_mfma_kernel / q_cols_mfma_kernel, measured; V is half of it",
                    plain_gemm_after_it_model_ms=float(m) ** 2 * N * 2 / (ATTAINABLE_F64_TFLOPS * 1e12) * 1e3,
                    plain_gemm_note="MODEL, not a run: 2 m^2 N flops (both triangles) at the attainable rate")
        if not a.no_scipy:
            model = G.fit(X, y, "matern52", 1.0, 1.5, 1e-3, 1e-10, True)

            def scipy_cov():
                Ks = G.cross_kernel(Xq, model.X, model.kind, model.constant, model.length_scale)
                V = solve_triangular(model.L, Ks.T, lower=True, check_finite=False)
                return G.cross_kernel(Xq, Xq, model.kind, model.constant, model.length_scale) + 1e-3 * np.eye(m) - V.T @ V
            line["scipy_predict_cov_wall_ms"] = median_ms(scipy_cov, max(a.reps // 2, 1), 1)
            Sg = scipy_cov() + 1e-8 * np.eye(m)
            eps = rng.standard_normal((S, m))
            line["scipy_factor_and_sample_wall_ms"] = median_ms(lambda: eps @ cholesky(Sg, lower=True, check_finite=False).T,
                                                                max(a.reps // 2, 1), 1)
            line["scipy_threads"] = os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"])
        gp.close()
        s = json.dumps(line)
        print(s, flush=True)
        lines.append(s)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _timings(gp):
    import ctypes
    v = np.zeros(16)
    gp._check(gp.lib.tgp_last_timings(gp._h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 16))
    return v


if __name__ == "__main__":
    main()
