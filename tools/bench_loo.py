#!/usr/bin/env python3
"""Times of tgp_loo and tgp_fit_loo_grad beside tgp_fit_grad at N = 128, 512, 2048 and 4096 (D = 16, Matern-5/2,
isotropic and ARD), one JSON line per shape and mode; --out appends them to a file (profiles/loo.jsonl).

  * `*_wall_ms`: medians of --reps synchronous calls on the host clock after --warmup (every call ends in the library's own
    synchronisation), min and max beside them: the spread;
  * `loo_device_ms`: tgp_last_timings slot 19, the three kernels of tgp_loo between two events (copies left out), and what
    that is in bytes per second of the N^2 / 2 doubles of Linv the kappa kernel has to read, against the attainable HBM
    rate (ATTAINABLE_HBM_TBS) -- where Linv fits the caches (and a fit has just written it) the figure is not an
    HBM figure, and at small N it measures three launches;
  * `loo_grad_stages_ms`: tgp_last_timings slots 2-4 after tgp_fit_loo_grad -- [K^-1, kappa, b, A, B = A A^T | pairwise pass |
    tile sums]; a polled call (the default up to Np = 4096) records none, so run once more with TGP_POLL_US=0 for them;
  * --ab-library PATH: another build of libturbogp.so (the parent commit's), whose tgp_fit_grad is timed in the SAME process,
    the two builds alternating call by call: `fit_grad_ab`.  Both are called through bare ctypes, the same way.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ATTAINABLE_HBM_TBS = 6.3      # what a streaming read attains of the 8 TB/s HBM3E peak (measured float4 copy: 6.29 TB/s)


class RawFitGrad:
    """tgp_fit_grad of the library at `path` on a handle of its own, through ctypes alone"""

    def __init__(self, path):
        c = ctypes
        self.lib = c.CDLL(path)
        dp = c.POINTER(c.c_double)
        self.lib.tgp_create.argtypes = [c.c_int, c.c_int, c.POINTER(c.c_void_p)]
        self.lib.tgp_fit_grad.argtypes = [c.c_void_p, dp, c.c_int64, c.c_int64, dp, c.c_int, c.c_double, dp, c.c_int64,
                                          c.c_double, c.c_double, c.c_int, dp, dp, dp, dp]
        self.lib.tgp_destroy.argtypes = [c.c_void_p]
        self.h = c.c_void_p()
        assert self.lib.tgp_create(0, 0, c.byref(self.h)) == 0, path

    def __call__(self, X, y, kind_id, constant, ls, noise):
        dp = ctypes.POINTER(ctypes.c_double)
        grad = np.zeros(2 + len(ls))
        lml = ctypes.c_double()
        rc = self.lib.tgp_fit_grad(self.h, X.ctypes.data_as(dp), X.shape[0], X.shape[1], y.ctypes.data_as(dp), kind_id, constant,
                                   ls.ctypes.data_as(dp), len(ls), noise, 1e-10, 1, ctypes.byref(lml), None, None, grad.ctypes.data_as(dp))
        assert rc == 0, rc
        return lml.value, grad

    def close(self):
        self.lib.tgp_destroy(self.h)


def times(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sizes", default="128,512,2048,4096")
    ap.add_argument("--ab-library", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd._lib as L
    L.load()
    kind = "matern52"
    lines = []
    for N in map(int, a.sizes.split(",")):
        D = 16
        rng = np.random.RandomState(N)
        X = np.ascontiguousarray(rng.uniform(0, 1, (N, D)))
        y = np.sin(X.sum(1)) + 0.01 * rng.normal(size=N)
        for ard in (False, True):
            ls = np.full(D if ard else 1, 1.5) * (1.0 + 0.05 * np.arange(D if ard else 1))
            gp = L.NativeGP(0, "f64")
            args = (X, y, kind, 1.0, ls if ard else float(ls[0]), 1e-3, 1e-10, True)
            rec = dict(N=N, D=D, kind=kind, ard=ard, reps=a.reps, poll_us=os.environ.get("TGP_POLL_US", "default"))
            rec["fit_wall_ms"] = times(lambda: gp.fit(*args), a.reps, a.warmup)
            dev = []
            rec["loo_wall_ms"] = times(lambda: (gp.loo(), dev.append(_slot(gp, 19))), a.reps, a.warmup)
            rec["loo_device_ms"] = float(np.median(dev[a.warmup:]))
            nbytes = N * (N + 1) / 2 * 8
            rec["kappa_bytes"] = nbytes
            rec["kappa_tbs_over_loo_device"] = nbytes / (rec["loo_device_ms"] * 1e-3) / 1e12
            rec["attainable_hbm_tbs"] = ATTAINABLE_HBM_TBS
            rec["fit_grad_wall_ms"] = times(lambda: gp.fit_grad(*args), a.reps, a.warmup)
            rec["fit_grad_stages_ms"] = [_slot(gp, i) for i in (2, 3, 4)]
            rec["fit_loo_grad_wall_ms"] = times(lambda: gp.fit_loo_grad(*args), a.reps, a.warmup)
            rec["loo_grad_stages_ms"] = [_slot(gp, i) for i in (2, 3, 4)]
            rec["loo_grad_over_fit_grad"] = rec["fit_loo_grad_wall_ms"]["median"] / rec["fit_grad_wall_ms"]["median"]
            gp.close()
            if a.ab_library:
                this, other = RawFitGrad(L.LIB_PATH), RawFitGrad(a.ab_library)
                raw = (X, np.ascontiguousarray(y), L.KERNELS[kind], 1.0, np.ascontiguousarray(ls), 1e-3)
                ga, gb = this(*raw), other(*raw)
                rec["fit_grad_ab_same_bytes"] = bool(np.float64(ga[0]).tobytes() + ga[1].tobytes() == np.float64(gb[0]).tobytes() + gb[1].tobytes())
                ta, tb = [], []
                for i in range(a.warmup + a.reps):              # alternating, call by call
                    for fn, t in ((this, ta), (other, tb)) if i % 2 == 0 else ((other, tb), (this, ta)):
                        t0 = time.perf_counter()
                        fn(*raw)
                        t.append((time.perf_counter() - t0) * 1e3)
                stat = lambda t: dict(median=float(np.median(t[a.warmup:])), min=float(np.min(t[a.warmup:])), max=float(np.max(t[a.warmup:])))
                rec["fit_grad_ab"] = dict(this=stat(ta), other=stat(tb), other_library=os.path.basename(a.ab_library))
                rec["fit_grad_ab"]["this_over_other"] = rec["fit_grad_ab"]["this"]["median"] / rec["fit_grad_ab"]["other"]["median"]
                this.close(); other.close()
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


def _slot(gp, i):
    v = np.zeros(20)
    gp._check(gp.lib.tgp_last_timings(gp._h, v.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 20))
    return float(v[i])


if __name__ == "__main__":
    main()
