#!/usr/bin/env python3
"""Greedy batch selection (tgp_sweep_batch, Kriging Believer) against the ways to get q points without it.

    python tools/bench_batch.py [--configs branin,c1,c2,c3] [--q 1,2,4,8,16] [--pending 0,4] [--reps 3] [--out FILE]

One JSON line per (config, q, pending): the median wall time of one tgp_sweep_batch call, of the naive loop that gets
the same q points by q x (tgp_fit_append of the fantasised point + tgp_sweep) after appending the pending points, and
(Branin size only) of the same loop as a NumPy / SciPy refit on the host.  One tgp_sweep of the same batch is timed as
the yardstick (batch_over_sweep, per_point_over_sweep = (batch - sweep) / (P + q - 1) / sweep).

    python tools/bench_batch.py --mc 1,16,64 [--mc-literal-S 16] [--configs branin,c2,c3] --q 8 [--out profiles/batch_mc.jsonl]

The Monte Carlo mode: one JSON line per (config, q, pending, S) with the median wall time of one tgp_sweep_batch_mc call
of S simulations beside one Kriging Believer call on the same handle and candidates (mc_over_kb).  --mc-literal-S S adds,
once per config without pending points, what the old library's loop costs on the same handle: S x (tgp_fit_append of
one fantasised point + tgp_sweep) for ONE selection after the first (the refit back to the real data between two
simulations is timed on its own and subtracted), beside the same step inside tgp_sweep_batch_mc (q = 2 minus q = 1).
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.special import ndtr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import CONFIGS, synth_train   # noqa: E402

ACQ = {"ucb": 1, "pi": 2, "ei": 3}
BRANIN = dict(D=2, N=32, M=10000, kind="matern52", ard=False, acq="ei", param=0.01, dtype="f64", noise=1e-4, cfg=0)


def branin_train(n=32, seed=0):
    rng = np.random.RandomState(seed)
    X = np.column_stack([rng.uniform(-5, 10, n), rng.uniform(0, 15, n)])
    y = (X[:, 1] - 5.1 / (4 * np.pi ** 2) * X[:, 0] ** 2 + 5 / np.pi * X[:, 0] - 6) ** 2 \
        + 10 * (1 - 1 / (8 * np.pi)) * np.cos(X[:, 0]) + 10
    return X, y, np.array([3.0, 4.0])


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def host_refit_loop(X, y, Xc, Xp, q, ls, noise, jitter, param):
    """the same greedy loop as literal refits on the host (NumPy / SciPy; Matern-5/2, the Branin model's kernel)"""
    def k52(A, B):
        d = np.sqrt(np.maximum(((A[:, None, :] - B[None, :, :]) / ls) ** 2, 0).sum(-1)) * np.sqrt(5.0)
        return (1 + d + d * d / 3.0) * np.exp(-d)
    Xa, ya = X.copy(), y.copy()
    ym, ys = y.mean(), y.std()
    inc = y.min()
    chosen = []
    for z in list(Xp):
        Xa = np.vstack([Xa, z])
        K = k52(Xa[:-1], Xa[:-1]) + (noise + jitter) * np.eye(len(Xa) - 1)
        f = ym + ys * (k52(z[None], Xa[:-1]) @ cho_solve(cho_factor(K, lower=True), (ya - ym) / ys))[0]
        ya = np.append(ya, f)
    for _ in range(q):
        K = k52(Xa, Xa) + (noise + jitter) * np.eye(len(Xa))
        cf = cho_factor(K, lower=True)
        Ks = k52(Xc, Xa)
        mu = ym + ys * (Ks @ cho_solve(cf, (ya - ym) / ys))
        var = np.maximum(1 + noise - np.einsum("ij,ji->i", Ks, cho_solve(cf, Ks.T)), 0)
        sg = ys * np.sqrt(var)
        diff = -(mu - inc) - param
        Z = np.where(sg > 0, diff / np.where(sg > 0, sg, 1), 0)
        a = np.where(sg > 0, diff * ndtr(Z) + sg * np.exp(-Z * Z / 2) / np.sqrt(2 * np.pi), 0)
        a[chosen] = -np.inf
        i = int(np.argmax(a))
        chosen.append(i)
        Xa = np.vstack([Xa, Xc[i]])
        ya = np.append(ya, mu[i])
        inc = min(inc, mu[i])
    return chosen


def mc_mode(a, st, emit):
    """tgp_sweep_batch_mc beside Kriging Believer, same handle, same candidates, warm.  st: the per-config state main
    builds (gp, L, fit, X, y, Xc, Xp_all, acq, sf, inc, par, t_sweep, base)"""
    gp, L, call = st.gp, st.L, (st.acq, st.sf, st.inc, st.par)
    for P in [int(v) for v in a.pending.split(",")]:
        Xp = st.Xp_all[:P] if P else None
        for q in [int(v) for v in a.q.split(",")]:
            gp.sweep_batch(q, L.BATCH_KB, 0.0, Xp, *call)
            t_kb = _median_ms(lambda: gp.sweep_batch(q, L.BATCH_KB, 0.0, Xp, *call), a.reps)
            kb_dev = gp.profile_read()["last_sweep_ms"]
            for S in [int(v) for v in a.mc.split(",")]:
                gp.sweep_batch_mc(q, S, 1, None, Xp, *call)
                t_mc = _median_ms(lambda: gp.sweep_batch_mc(q, S, 1, None, Xp, *call), a.reps)
                emit(dict(st.base, workload="batch_select_mc", strategy="monte_carlo", q=q, pending=P, S=S,
                          sweep_ms=round(st.t_sweep, 4), kb_ms=round(t_kb, 4), kb_device_ms=round(kb_dev, 4),
                          mc_ms=round(t_mc, 4), mc_device_ms=round(gp.profile_read()["last_sweep_ms"], 4),
                          mc_over_kb=round(t_mc / t_kb, 3)))
    if a.mc_literal_S > 0:
        # the old library's loop for ONE selection after the first: per simulation append the fantasised point and sweep.
        # Each simulation starts from the real data again; that refit is not part of the method, so S x its median time
        # is subtracted from the loop's.
        S = a.mc_literal_S
        res = gp.sweep_batch_mc(2, S, 1, None, None, *call)
        Xa, fants = np.vstack([st.X, res["x"][0]]), res["fantasies"][:, 0]

        def literal():
            for s_ in range(S):
                st.fit(Xa, np.append(st.y, fants[s_]), append=True)
                gp.sweep(*call, want_acq=True)
                st.fit(st.X, st.y)
        t_lit = _median_ms(literal, a.reps) - S * _median_ms(lambda: st.fit(st.X, st.y), a.reps)
        gp.set_candidates(st.Xc)
        t_step = _median_ms(lambda: gp.sweep_batch_mc(2, S, 1, None, None, *call), a.reps) \
            - _median_ms(lambda: gp.sweep_batch_mc(1, S, 1, None, None, *call), a.reps)
        emit(dict(st.base, workload="batch_select_mc", strategy="monte_carlo_literal", S=S,
                  literal_one_selection_ms=round(t_lit, 3), mc_one_selection_ms=round(t_step, 4),
                  literal_over_mc=round(t_lit / max(t_step, 1e-9), 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="branin,c1,c2,c3")
    ap.add_argument("--q", default="1,2,4,8,16")
    ap.add_argument("--pending", default="0,4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-naive", action="store_true", help="time tgp_sweep_batch and tgp_sweep only")
    ap.add_argument("--mc", default=None, help="Monte Carlo mode: the simulation counts, e.g. 1,16,64")
    ap.add_argument("--mc-literal-S", type=int, default=0, metavar="S",
                    help="with --mc: also time the literal alternative for one selection, S x (tgp_fit_append + tgp_sweep)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd as ta
    L = ta._lib
    out = open(a.out, "a") if a.out else None

    def emit(line):
        s = json.dumps(line)
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()
    for name in a.configs.split(","):
        cfg = BRANIN if name == "branin" else CONFIGS[name]
        if name == "branin":
            X, y, ls = branin_train(cfg["N"])
            rng = np.random.RandomState(1)
            Xc = np.column_stack([rng.uniform(-5, 10, cfg["M"]), rng.uniform(0, 15, cfg["M"])])
            Xp_all = np.column_stack([rng.uniform(-5, 10, 4), rng.uniform(0, 15, 4)])
        else:
            X, y, ls = synth_train(cfg)
            rng = np.random.RandomState(3000 + cfg["cfg"])
            Xc = rng.uniform(0, 1, (cfg["M"], cfg["D"]))
            Xp_all = rng.uniform(0, 1, (4, cfg["D"]))
        kind, noise, jitter = cfg["kind"], cfg["noise"], 1e-10
        acq, par = ACQ[cfg["acq"]], cfg["param"]
        sf = -1.0 if cfg["acq"] in ("ei", "pi") else 1.0
        inc = float(y.min())
        gp = ta.NativeGP(0, cfg["dtype"])
        fit = lambda Xf, yf, append=False: gp.fit(Xf, yf, kind, 1.0, ls, noise, jitter, True, append=append)   # noqa: E731
        fit(X, y)
        gp.set_candidates(Xc)
        gp.sweep(acq, sf, inc, par)
        t_sweep = _median_ms(lambda: gp.sweep(acq, sf, inc, par), a.reps)
        if a.mc:
            base = dict(config=name, N=cfg["N"], D=cfg["D"], M=cfg["M"], dtype=cfg["dtype"], acq=cfg["acq"])
            mc_mode(a, SimpleNamespace(gp=gp, L=L, fit=fit, X=X, y=y, Xc=Xc, Xp_all=Xp_all, acq=acq, sf=sf, inc=inc, par=par,
                                       t_sweep=t_sweep, base=base), emit)
            continue
        for P in [int(v) for v in a.pending.split(",")]:
            Xp = Xp_all[:P] if P else None
            for q in [int(v) for v in a.q.split(",")]:
                fit(X, y)
                gp.set_candidates(Xc)
                res = gp.sweep_batch(q, L.BATCH_KB, 0.0, Xp, acq, sf, inc, par)     # warm-up (buffers)
                t_batch = _median_ms(lambda: gp.sweep_batch(q, L.BATCH_KB, 0.0, Xp, acq, sf, inc, par), a.reps)
                dev_ms = gp.profile_read()["last_sweep_ms"]
                line = dict(workload="batch_select", config=name, N=cfg["N"], D=cfg["D"], M=cfg["M"], dtype=cfg["dtype"],
                            acq=cfg["acq"], strategy="kriging_believer", q=q, pending=P, sweep_ms=round(t_sweep, 4),
                            batch_ms=round(t_batch, 4), batch_device_ms=round(dev_ms, 4),
                            batch_over_sweep=round(t_batch / t_sweep, 3),
                            per_point_over_sweep=round((t_batch - t_sweep) / max(P + q - 1, 1) / t_sweep, 4))
                if not a.no_naive:
                    fants = res["fantasies"]

                    def naive():
                        Xa, ya = X, y
                        for j in range(P):
                            Xa, ya = np.vstack([Xa, Xp[j]]), np.append(ya, fants[j])
                            fit(Xa, ya, append=True)
                        for k in range(q):
                            r = gp.sweep(acq, sf, inc, par)
                            Xa, ya = np.vstack([Xa, Xc[r["best_idx"]]]), np.append(ya, fants[P + k])
                            if k < q - 1:
                                fit(Xa, ya, append=True)
                        fit(X, y)      # (restores the model: its time is subtracted below)
                    t_naive = _median_ms(naive, a.reps) - _median_ms(lambda: fit(X, y), a.reps)
                    line.update(naive_ms=round(t_naive, 4), speedup_vs_naive=round(t_naive / t_batch, 2))
                    if name == "branin":
                        t_host = _median_ms(lambda: host_refit_loop(X, y, Xc, Xp_all[:P], q, ls, noise, jitter, par), a.reps)
                        line.update(host_refit_ms=round(t_host, 3))
                emit(line)
    if out:
        out.close()


if __name__ == "__main__":
    main()
