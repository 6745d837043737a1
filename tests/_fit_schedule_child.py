"""Child process of test_gpu_fit_schedule.py: csrc/tuning.hpp reads the TGP_* switches once per process, so every selection
of the blocked fit's schedule (csrc/fit_plan.hpp, csrc/fit_blocked.hpp) gets a process of its own.

    python _fit_schedule_child.py [private] [tail] [serial]

Fits, on ONE f64 handle and in this order (each smaller than the one before: Linv must be clean where the new fit skips):
N = 1100 (Np = 1280), N = 600 (Np = 768), N = 129 (Np = 256, Nr = 192: the padding panels are skipped); with `tail` one
more at N = 1700 (Np = 1792: TGP_OB=1024 would leave a tail of 768).  `private`: that handle on a private stream.  Then an
f32 handle at N = 600 with 2048 resident candidates and tgp_set_overlap(2), and its sweep; with `serial` once more with
tgp_set_overlap(0).  Every fit is held against the oracle with the comparisons and tolerances of _alt_paths_child.py and
leaves one line `fit-schedule {json}` with the digests of what it wrote.  Test helper, not product code."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import turbo_amd as ta                      # noqa: E402
from oracle import gp_oracle as o            # noqa: E402

L = ta._lib
F64_FITS = [(1100, 6, "matern52"), (600, 3, "rbf"), (129, 2, "matern32")]
TAIL_FIT = (1700, 4, "matern52")


def dig(*arrays):   # (tools/stress_round3.py's)
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def problem(N, D, M):
    rng = np.random.RandomState(N)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X.sum(1)) + 0.05 * rng.normal(size=N)
    return X, y, rng.uniform(0, 1, (M, D)), float(np.sqrt(D / 6.0))


def check_sweep(r, om, Xc, tol):
    mu, sg = o.predict(om, Xc)
    np.testing.assert_allclose(r["mu"], mu, rtol=tol, atol=tol * om.y_std)
    np.testing.assert_allclose(r["sigma"] ** 2, sg ** 2, rtol=tol, atol=tol * 1.001 * om.y_std ** 2)
    assert r["best_idx"] == int(np.argmax(r["acq"]))


def fit_f64(gp, N, D, kind):
    X, y, Xc, ls = problem(N, D, 512)
    om = o.fit(X, y, kind, 1.0, ls, 1e-3, 1e-10, True)
    lml, _, _ = gp.fit(X, y, kind, 1.0, ls, 1e-3, 1e-10, True)
    Lf = gp.debug_read(L.BUF_L)
    print("N=%d lml rel err %.3g, L max abs err %.3g" % (N, abs(lml - om.lml) / abs(om.lml), np.abs(Lf - om.L).max()), flush=True)
    assert abs(lml - om.lml) <= 1e-9 * abs(om.lml), (lml, om.lml)
    np.testing.assert_allclose(Lf, om.L, rtol=1e-8, atol=1e-11)
    rec = dict(fit="f64 N=%d" % N, L=dig(Lf), Linv=dig(gp.debug_read(L.BUF_LINV)), alpha=dig(gp.debug_read(L.BUF_ALPHA)), lml=repr(lml))
    gp.set_candidates(Xc)
    r = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)
    check_sweep(r, om, Xc, 1e-7)
    rec["sweep"] = dig(r["mu"], r["sigma"], r["acq"])
    print("fit-schedule " + json.dumps(rec), flush=True)


def fit_f32(modes):
    N, D, kind = 600, 3, "rbf"
    X, y, Xc, ls = problem(N, D, 2048)
    om = o.fit(X, y, kind, 1.0, ls, 1e-3, 1e-10, True)
    gp = ta.NativeGP(0, "f32")
    gp.fit(X, y, kind, 1.0, ls, 1e-3, 1e-10, True)
    gp.set_candidates(Xc)                      # resident before the fits below: they start its sweep
    for mode in modes:
        gp.set_overlap(mode)
        lml, _, _ = gp.fit(X, y, kind, 1.0, ls, 1e-3, 1e-10, True)
        assert abs(lml - om.lml) <= 1e-9 * abs(om.lml), (lml, om.lml)
        r = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)
        check_sweep(r, om, Xc, 5e-3)
        print("fit-schedule " + json.dumps(dict(fit="f32 N=%d overlap=%d" % (N, mode), sweep=dig(r["mu"], r["sigma"], r["acq"]),
                                                winner=[int(r["best_idx"]), repr(float(r["best_val"]))], lml=repr(lml))), flush=True)
    print("third stream beside the others: %d" % gp.stream_status()["third_overlaps"], flush=True)
    gp.close()


if __name__ == "__main__":
    flags = sys.argv[1:]
    gp = ta.NativeGP(0, "f64")
    if "private" in flags:
        gp.set_private_stream(True)
    for case in F64_FITS + ([TAIL_FIT] if "tail" in flags else []):
        fit_f64(gp, *case)
    gp.close()
    fit_f32([2, 0] if "serial" in flags else [2])
    print("fit-schedule done")
