#!/usr/bin/env python3
"""Max-value entropy search selection (tgp_mes_draw + tgp_sweep with the MES acquisition) beside tgp_sweep(EI) and the
Thompson draw + sweep on one handle.

    python tools/bench_mes.py [--configs branin,c2,c3] [--S 8,64] [--F 2048] [--reps 9] [--out FILE]
    python tools/bench_mes.py --ei-only --tag parent|new [--package DIR] [--configs c3] [--reps 21] [--out FILE]

One JSON line per (config, S): median host wall times of one mes_draw, one MES sweep (arg-max only: the trial's call),
their sum, one EI sweep as the library runs it (pruned where eligible), one EI sweep with TGP_SWEEP_PRUNE=0 (the
schedule MES takes) and one Thompson draw + sweep of the same S.  Every timed call returns with its results on the host.
--ei-only: the EI sweep alone, for the A/B against another build: --package names the checkout (built) whose turbo_amd
package and library are timed, one process each, the two builds alternating.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench import CONFIGS, synth_train          # noqa: E402
from bench_batch import BRANIN, branin_train    # noqa: E402


def _times_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def _median_ms(fn, reps):
    return float(np.median(_times_ms(fn, reps)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="branin,c2,c3")
    ap.add_argument("--S", default="8,64")
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--ei-only", action="store_true")
    ap.add_argument("--tag", default="new")
    ap.add_argument("--package", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.package:
        sys.path.insert(0, os.path.abspath(a.package))
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
        else:
            X, y, ls = synth_train(cfg)
            rng = np.random.RandomState(3000 + cfg["cfg"])
            Xc = rng.uniform(0, 1, (cfg["M"], cfg["D"]))
        sf, inc = -1.0, float(y.min())
        gp = ta.NativeGP(0, cfg["dtype"])
        gp.fit(X, y, cfg["kind"], 1.0, ls, cfg["noise"], 1e-10, True)
        gp.set_candidates(Xc)
        base = dict(config=name, N=cfg["N"], D=cfg["D"], M=cfg["M"], dtype=cfg["dtype"], kernel=cfg["kind"])
        for _ in range(3):
            gp.sweep(L.ACQ_EI, sf, inc, 0.01)
        if a.ei_only:
            ts = _times_ms(lambda: gp.sweep(L.ACQ_EI, sf, inc, 0.01), a.reps)
            emit(dict(workload="ei_sweep_ab", build=a.tag, ei_sweep_ms=round(float(np.median(ts)), 4), ei_sweep_min_ms=round(float(np.min(ts)), 4),
                      prune_state=gp.last_prune()["state"], reps=a.reps, **base))
            continue
        t_ei = _median_ms(lambda: gp.sweep(L.ACQ_EI, sf, inc, 0.01), a.reps)
        ei_state = gp.last_prune()["state"]
        os.environ["TGP_SWEEP_PRUNE"] = "0"
        gp.sweep(L.ACQ_EI, sf, inc, 0.01)
        t_ei_full = _median_ms(lambda: gp.sweep(L.ACQ_EI, sf, inc, 0.01), a.reps)
        del os.environ["TGP_SWEEP_PRUNE"]
        for S in [int(v) for v in a.S.split(",")]:
            gp.mes_draw(1, S, a.F, sf, inc)
            gp.sweep(L.ACQ_MES, sf)                                   # warm-up (buffers, code object)
            t_draw = _median_ms(lambda: gp.mes_draw(1, S, a.F, sf, inc), a.reps)
            t_mes = _median_ms(lambda: gp.sweep(L.ACQ_MES, sf), a.reps)
            dev_ms = gp.profile_read()["last_sweep_ms"]
            mes_state = gp.last_prune()["state"]

            def select():
                gp.mes_draw(2, S, a.F, sf, inc)
                gp.sweep(L.ACQ_MES, sf)

            def thompson():
                gp.ts_draw(2, S, a.F)
                gp.ts_sweep(sf, False)
            t_sel = _median_ms(select, a.reps)
            t_ts = _median_ms(thompson, a.reps)
            emit(dict(workload="mes_select", S=S, F=a.F, mes_draw_ms=round(t_draw, 4), mes_sweep_ms=round(t_mes, 4),
                      mes_sweep_device_ms=round(dev_ms, 4), mes_select_ms=round(t_sel, 4), ei_sweep_ms=round(t_ei, 4),
                      ei_prune_state=ei_state, ei_sweep_unpruned_ms=round(t_ei_full, 4), mes_prune_state=mes_state,
                      ts_draw_plus_sweep_ms=round(t_ts, 4), mes_sweep_over_ei_unpruned=round(t_mes / t_ei_full, 4),
                      mes_sweep_over_ei=round(t_mes / t_ei, 4), mes_select_over_ei=round(t_sel / t_ei, 4),
                      mes_select_over_thompson=round(t_sel / t_ts, 4), **base))
    if out:
        out.close()


if __name__ == "__main__":
    main()
