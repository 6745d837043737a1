#!/usr/bin/env python3
"""Cost of tgp_kg_grad at the C1 / C3 models for A in {16, 64, 256} discretisation points and m in {10, 64}
query points, beside what it stands next to on the SAME handle: tgp_acq_grad (EI) at the same m, and the finite-difference
alternative it replaces -- 2 D calls of tgp_sweep_kg on m rows (tgp_set_candidates + tgp_sweep_kg each).  Then one whole KG
trial through the plugin: CandidateSweep(num_random=1000, grad_restarts=10) over ta.KG(gradient=True), beside the same trial
without the gradient stage.  One JSON line each; --out appends them to a file (profiles/kg_grad.jsonl).  Every time is
{median, min, max} over --reps rounds after --warmup; a round times a block of --inner calls of each entry in turn (the
finite-difference loop and the trials: one), so the entries compared alternate; the host clock around calls that end in a
stream synchronisation, except
  kg_grad_device_ms     tgp_last_timings slot 20: the call's own kernels between events (the predict-only sweep of the m
                        points in front of them and the copies left out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SHAPES = {"C1": (512, 8, "rbf"), "C3": (4096, 32, "rbf")}


def alternating(fns, reps, warmup, inner):
    """{name: [ms per call]}: ``reps`` rounds, each timing a block of ``inner`` calls of every entry in turn, so that what
    else runs on the machine meets all of them alike; a short call is timed ``inner`` at a time"""
    for _ in range(warmup):
        for fn, _ in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, (fn, n) in fns.items():
            n = inner if n is None else n
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            out[k].append((time.perf_counter() - t0) * 1e3 / n)
    return out


def stats(t):
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def slot20(gp, L):
    v = np.zeros(21)
    gp.lib.tgp_last_timings(gp._h, v.ctypes.data_as(L._dp), 21)
    return float(v[20])


def entries(a, L, lines):
    for shape in a.shapes.split(","):
        N, D, kind = SHAPES[shape]
        rng = np.random.RandomState(N)
        X = rng.uniform(0, 1, (N, D))
        y = np.sin(X.sum(1)) + 0.01 * rng.normal(size=N)
        gp = L.NativeGP(0, "f64")
        gp.fit(X, y, kind, 1.0, 0.5 * np.sqrt(D), 1e-3, 1e-10, True)
        for A in (int(v) for v in a.points.split(",")):
            gp.kg_set_points(np.ascontiguousarray(X[np.argsort(y, kind="stable")[:A]]))
            for m in (int(v) for v in a.batch.split(",")):
                Xq = rng.uniform(0, 1, (m, D))
                dev = []

                def finite_differences():
                    for d in range(D):
                        for sgn in (1.0, -1.0):
                            P = Xq.copy()
                            P[:, d] += sgn * 1e-6
                            gp.set_candidates(P)
                            gp.sweep_kg(1.0, want_kg=True)
                t = alternating({"kg": (lambda: (gp.kg_grad(Xq, 1.0), dev.append(slot20(gp, L))), None),
                                 "ei": (lambda: gp.acq_grad(Xq, L.ACQ_EI, -1.0, float(y.min()), 0.01), None),
                                 "fd": (finite_differences, 1)}, a.reps, a.warmup, a.inner)
                kg, ei, fd = stats(t["kg"]), stats(t["ei"]), stats(t["fd"])
                line = dict(workload="kg_grad", date=time.strftime("%Y-%m-%d"), shape=shape, N=N, D=D, A=A, m=m, kernel=kind,
                            dtype="f64", reps=a.reps, calls_per_timing=a.inner, kg_grad_call_ms=kg, kg_grad_device_ms=stats(dev[a.warmup:]),
                            acq_grad_ei_call_ms=ei, sweep_kg_2D_calls_ms=fd, kg_grad_over_acq_grad=kg["median"] / ei["median"],
                            finite_differences_over_kg_grad=fd["median"] / kg["median"])
                s = json.dumps(line)
                print(s, flush=True)
                lines.append(s)
        gp.close()


def trial(a, lines):
    import turbo_amd as ta
    N, D, kind = SHAPES["C1"]
    rng = np.random.RandomState(N)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(X.sum(1)) + 0.01 * rng.normal(size=N)
    b = ta.Bounds([("x%d" % d, 0.0, 1.0) for d in range(D)])
    sur = ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel(kind, 1.0, 0.5 * np.sqrt(D), 1e-3), optimizer=None,
                                              normalize_y=True), training_iterations=0)
    model, _ = sur.construct_model(0, X, y)
    kg, _ = ta.KG(n_points=64, gradient=True).construct_function(0, model, "min")
    ei, _ = ta.EI(0.01).construct_function(0, model, "min", float(y.min()))
    info = {}

    def run(key, acq, restarts):
        def one():
            np.random.seed(3)
            _, info[key] = ta.CandidateSweep(num_random=1000, grad_restarts=restarts, start_from_best=2 if restarts else 0)(b, acq)
        return one
    t = alternating({"kg_trial_grad_restarts_10_ms": (run("kg_trial_grad_restarts_10_ms", kg, 10), 1),
                     "kg_trial_sweep_only_ms": (run("kg_trial_sweep_only_ms", kg, 0), None),
                     "ei_trial_grad_restarts_10_ms": (run("ei_trial_grad_restarts_10_ms", ei, 10), 1)}, a.reps, a.warmup, a.inner)
    out = {k: stats(v) for k, v in t.items()}
    line = dict(workload="kg_trial", date=time.strftime("%Y-%m-%d"), N=N, D=D, A=64, kernel=kind, num_random=1000, **out,
                kg_gradient_evaluations=int(info["kg_trial_grad_restarts_10_ms"].get("gradient_evaluations", -1)),
                kg_max_acq_refined=float(info["kg_trial_grad_restarts_10_ms"]["max_acq"]),
                kg_max_acq_sweep_only=float(info["kg_trial_sweep_only_ms"]["max_acq"]))
    s = json.dumps(line)
    print(s, flush=True)
    lines.append(s)
    sur.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="C1,C3")
    ap.add_argument("--points", default="16,64,256")
    ap.add_argument("--batch", default="10,64")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd._lib as L
    lines = []
    entries(a, L, lines)
    trial(a, lines)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
