#!/usr/bin/env python3
"""Thompson-sampling batch selection (tgp_ts_draw + tgp_ts_sweep) beside tgp_sweep and tgp_sweep_batch (KB) on one handle.

    python tools/bench_thompson.py [--configs branin,c2,c3] [--S 1,8,64] [--F 2048] [--reps 5] [--out FILE]

One JSON line per (config, S): median host wall times of one tgp_ts_draw, one tgp_ts_sweep (distinct) and their sum,
of one tgp_sweep and of one tgp_sweep_batch with Kriging Believer at q = 8 on the same handle and candidates.  Every
timed call returns after its stream has synchronised (each entry waits for its own results).
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
from bench_batch import BRANIN, branin_train, ACQ   # noqa: E402


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="branin,c2,c3")
    ap.add_argument("--S", default="1,8,64")
    ap.add_argument("--F", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import turbo_amd as ta
    L = ta._lib
    out = open(a.out, "a") if a.out else None
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
        acq, par = ACQ[cfg["acq"]], cfg["param"]
        sf = -1.0 if cfg["acq"] in ("ei", "pi") else 1.0
        inc = float(y.min())
        gp = ta.NativeGP(0, cfg["dtype"])
        gp.fit(X, y, cfg["kind"], 1.0, ls, cfg["noise"], 1e-10, True)
        gp.set_candidates(Xc)
        gp.sweep(acq, sf, inc, par)
        t_sweep = _median_ms(lambda: gp.sweep(acq, sf, inc, par), a.reps)
        gp.sweep_batch(8, L.BATCH_KB, 0.0, None, acq, sf, inc, par)
        t_kb = _median_ms(lambda: gp.sweep_batch(8, L.BATCH_KB, 0.0, None, acq, sf, inc, par), a.reps)
        for S in [int(v) for v in a.S.split(",")]:
            distinct = S <= cfg["M"]
            gp.ts_draw(1, S, a.F)
            gp.ts_sweep(sf, distinct)                                  # warm-up (buffers)
            t_draw = _median_ms(lambda: gp.ts_draw(1, S, a.F), a.reps)
            t_ts = _median_ms(lambda: gp.ts_sweep(sf, distinct), a.reps)
            dev_ms = gp.profile_read()["last_sweep_ms"]

            def both():
                gp.ts_draw(2, S, a.F)
                gp.ts_sweep(sf, distinct)
            t_both = _median_ms(both, a.reps)
            line = dict(workload="thompson_select", config=name, N=cfg["N"], D=cfg["D"], M=cfg["M"], dtype=cfg["dtype"],
                        kernel=cfg["kind"], S=S, F=a.F, distinct=distinct, ts_draw_ms=round(t_draw, 4),
                        ts_sweep_ms=round(t_ts, 4), ts_sweep_device_ms=round(dev_ms, 4), ts_draw_plus_sweep_ms=round(t_both, 4),
                        sweep_ms=round(t_sweep, 4), kb_q8_ms=round(t_kb, 4), ts_over_sweep=round(t_both / t_sweep, 4),
                        ts_over_kb_q8=round(t_both / t_kb, 4))
            s = json.dumps(line)
            print(s, flush=True)
            if out:
                out.write(s + "\n")
                out.flush()
    if out:
        out.close()


if __name__ == "__main__":
    main()
