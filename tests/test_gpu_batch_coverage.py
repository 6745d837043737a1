"""tgp_sweep_batch on the GPU, the axes tests/test_gpu_batch.py leaves out: every kernel, constant != 1, normalize_y=False,
TGP_ACQ_SIGMA and both directions of every acquisition, the pass's partial D-chunks at f64 limits, the size limits (P + q
= 64, M = q, tile and path boundaries of N), every first-sweep path (f32 families, TGP_CHUNK, TGP_MID_MAXM, the read-once
switches in a child process, a front left by an overlapped fit), every handle state (appended, received factor,
imported state, reused across shapes), n_clamped, ties, and the plugin layer.  The reference is tests/batch_reference.py
(held to literal refits by tests/test_batch_reference.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gp_oracle as o
import batch_reference as br

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# f32-family handles: the bars of tests/test_gpu_configs.py (the first sweep is f32, the steps f64)
REGRET_TOL, F32_MU_TOL, F32_VAR_TOL = 1e-3, 5e-4, 5e-5
ACQ_CODE = {"ei": 3, "pi": 2, "ucb": 1, "sigma": 4}


def _problem(N, D, M, seed, ard=False, ls_scale=1.0, n_pending=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    w = rng.normal(size=D) / np.sqrt(D)
    y = np.sin(3 * X @ w) + 0.5 * ((X - 0.5) ** 2).sum(1) + 0.01 * rng.normal(size=N)
    iso = float(np.sqrt(D / 6.0)) * ls_scale
    ls = iso * (0.5 + np.arange(D) / max(D - 1.0, 1.0)) if ard else iso
    return X, y, ls, rng.uniform(0, 1, (M, D)), rng.uniform(0, 1, (n_pending, D))


def _gp(dtype, X, y, kind, c, ls, noise, jitter, normalize_y, Xc):
    import turbo_amd as ta
    gp = ta.NativeGP(0, dtype)
    gp.fit(X, y, kind, c, ls, noise, jitter, normalize_y)
    gp.set_candidates(Xc)
    return gp


def _lie(spec, y):
    """'min' / 'max' / 'mean', or 'below': a float under every observation"""
    return float(y.min()) - 1.0 if spec == "below" else br.resolve_lie(spec, y)


def _ref_acq(acq):
    """the reference's (kind, param override): TGP_ACQ_SIGMA is UCB(beta=inf)"""
    return ("ucb", np.inf) if acq == "sigma" else (acq, None)


def _check_parity(gp, om, Xc, q, strategy, lie, Xp, acq, sf, inc, par, f64=True, clamps=True):
    """teacher-forced parity with the reference (the limits of test_parity_with_the_reference_under_teacher_forcing),
    the GPU's own picks against the reference's own greedy picks while the reference's step is decisive, n_clamped"""
    import turbo_amd as ta
    L = ta._lib
    kind, p = _ref_acq(acq)
    rpar = par if p is None else p
    desired = "max" if sf > 0 else "min"
    first = gp.sweep(ACQ_CODE[acq], sf, inc, par)
    res = gp.sweep_batch(q, L.BATCH_KB if strategy == br.KB else L.BATCH_CL, lie, Xp, ACQ_CODE[acq], sf, inc, par,
                         want_posterior=True)
    idx = res["idx"]
    assert len(set(idx.tolist())) == q
    ref = br.select_batch(om, Xc, q, strategy, lie, Xp, kind, desired, rpar, inc, forced=idx)
    assert not ref["not_pd"]
    for k in range(q):
        best, got = ref["best"][k], ref["acq"][k][idx[k]]
        regret = (best - got) / max(abs(best), 1e-300)
        assert regret <= (1e-9 if f64 else REGRET_TOL), (k, best, got)
        # (f32: the first value comes from the f32 sweep; EI far below its scale moves by a few 1e-3 relative)
        np.testing.assert_allclose(res["val"][k], got, rtol=1e-9 if f64 else 1e-2, atol=1e-12 if f64 else 1e-6 * abs(best))
    np.testing.assert_array_equal(res["x"], Xc[idx])
    np.testing.assert_allclose(res["fantasies"], ref["fantasies"], rtol=1e-9 if f64 else 1e-6, atol=1e-12)
    s_y, cn = om.y_std, om.constant + om.noise
    if f64:
        np.testing.assert_allclose(res["mu"], ref["mu"], rtol=1e-5, atol=1e-9 * s_y)
        # (the variance's absolute error scales with the prior variance c + noise, in raw units)
        np.testing.assert_allclose(res["sigma"] ** 2, ref["sigma"] ** 2, rtol=1e-5, atol=1e-9 * cn * s_y ** 2)
    else:
        assert np.max(np.abs(res["mu"] - ref["mu"])) <= F32_MU_TOL * s_y
        assert np.max(np.abs(res["sigma"] ** 2 - ref["sigma"] ** 2)) <= F32_VAR_TOL * cn * s_y ** 2
    if f64:
        # the arg-max and the mask directly: while the reference's top two values of a step are more than 1e-6 apart
        # (relative), the GPU's own pick is the reference's own greedy pick
        own = br.select_batch(om, Xc, q, strategy, lie, Xp, kind, desired, rpar, inc)
        for k in range(q):
            a = np.sort(own["acq"][k][np.isfinite(own["acq"][k])])
            if a.size >= 2 and not (a[-1] - a[-2] > 1e-6 * max(abs(a[-1]), 1e-300)):
                break
            assert idx[k] == own["idx"][k], (k, idx[:k + 1], own["idx"][:k + 1])
    if clamps and f64 and ref["min_abs_prevar"] > 1e-12 * cn:
        # (every pre-clamp variance of the steps is far from 0: the count does not depend on the last digits)
        assert res["n_clamped"] == first["n_clamped"] + ref["n_clamped_steps"], (res["n_clamped"], first["n_clamped"],
                                                                                ref["n_clamped_steps"])
    return res, ref


# One row per case; between them the rows cover every axis of the batch entry:
#   kernel rbf / matern12 / matern32 / matern52, iso and ARD;  constant 1.0 / 0.3 / 4.0;  normalize_y True / False;
#   EI, PI, UCB(2), SIGMA with sf = +1 and -1;  KB, CL with lie min / max / mean / below every y;
#   N: 1, 2, 127, 128 (N <= 128: one-workgroup sweep), 129, 256 (mid sweep), 257, 383, 384, 385, 1025 (general sweep;
#      128-row tiles of the pass, jt_live < njt, js splits of bt_pass_splits);
#   D: 1, 15, 16, 17, 32, 33, 100 (the pass's DC = 16 chunks: full, partial, several);
#   M: 1, q (every row taken), 63, 64, 65, 255, 256, 257, 20480 (js = 1);  (P, q): (0, 1), (5, 1), (63, 1), (0, 64), (40, 24)
CASES = [
    # N,   D,  kind,      ard,   c,   norm,  noise, M,     P,  q,  strategy, lie,     acq,     sf
    (1,    2,  "rbf",      False, 1.0, False, 1e-3, 1,     0,  1,  br.KB, None,    "ei",    -1.0),
    (2,    3,  "matern12", False, 0.3, True,  1e-3, 63,    5,  1,  br.CL, "min",   "pi",    1.0),
    (127,  15, "matern32", True,  4.0, True,  1e-4, 64,    0,  8,  br.KB, None,    "ucb",   -1.0),
    (128,  16, "matern52", True,  1.0, False, 1e-4, 65,    3,  8,  br.CL, "max",   "sigma", 1.0),
    (128,  2,  "matern12", True,  1.0, True,  1e-3, 4000,  2,  8,  br.KB, None,    "ei",    1.0),
    (129,  17, "rbf",      True,  0.3, True,  1e-3, 255,   2,  8,  br.CL, "mean",  "ei",    1.0),
    (129,  15, "rbf",      False, 4.0, False, 0.0,  500,   0,  8,  br.KB, None,    "pi",    -1.0),
    (256,  33, "matern12", True,  4.0, True,  1e-3, 256,   0,  8,  br.KB, None,    "ei",    -1.0),
    (257,  32, "matern32", False, 1.0, True,  1e-4, 257,   4,  6,  br.CL, "below", "ucb",   1.0),
    (257,  16, "matern52", True,  1.0, True,  1e-4, 256,   5,  1,  br.CL, "below", "ei",    -1.0),
    (383,  1,  "matern52", False, 0.3, False, 1e-3, 2000,  63, 1,  br.KB, None,    "pi",    -1.0),
    (384,  100, "rbf",     True,  1.0, True,  1e-2, 3000,  0,  64, br.CL, "min",   "ei",    -1.0),
    (385,  17, "matern12", False, 1.0, True,  1e-3, 24,    0,  24, br.KB, None,    "sigma", -1.0),
    (1025, 33, "matern32", True,  4.0, True,  1e-3, 20480, 40, 24, br.CL, "mean",  "pi",    1.0),
]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(v) for v in c[:10]) + "-" + c[12] for c in CASES])
def test_f64_parity_matrix(case):
    N, D, kind, ard, c, norm, noise, M, P, q, strategy, lie_spec, acq, sf = case
    # (noise-free: shorter length scales, as in test_gpu_batch.py -- with jitter alone the conditioning decides)
    X, y, ls, Xc, Xp = _problem(N, D, M, 100 + N + D, ard=ard, ls_scale=1.0 if noise > 0 else 0.4, n_pending=P)
    jitter = 1e-10 if noise > 0 else 1e-8
    gp = _gp("f64", X, y, kind, c, ls, noise, jitter, norm, Xc)
    om = o.fit(X, y, kind, c, ls, noise, jitter, norm)
    inc = float(y.max() if sf > 0 else y.min())
    lie = _lie(lie_spec, y) if strategy == br.CL else 0.0
    res, _ = _check_parity(gp, om, Xc, q, strategy, lie, Xp if P else None, acq, sf, inc, 2.0 if acq == "ucb" else 0.01)
    if M == q:
        assert sorted(res["idx"].tolist()) == list(range(M))


def test_p_plus_q_above_64_is_a_bad_argument():
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, Xc, Xp = _problem(40, 3, 500, 1, n_pending=40)
    gp = _gp("f64", X, y, "rbf", 1.0, ls, 1e-3, 1e-10, True, Xc)
    for P, q in ((40, 25), (0, 65), (1, 64)):
        with pytest.raises(ValueError, match="P \\+ q <= 64"):
            gp.sweep_batch(q, L.BATCH_KB, 0.0, Xp[:P] if P else None, L.ACQ_EI, -1.0, float(y.min()), 0.01)
    assert len(gp.sweep_batch(24, L.BATCH_KB, 0.0, Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01)["idx"]) == 24


# ---- the first sweep's paths ----------------------------------------------------------------------------------------

def _assert_q1_is_the_sweep(gp, y):
    import turbo_amd as ta
    L = ta._lib
    for acq, sf, par in ((L.ACQ_EI, -1.0, 0.01), (L.ACQ_UCB, 1.0, 2.0), (L.ACQ_PI, -1.0, 0.0), (L.ACQ_SIGMA, 1.0, 0.0)):
        inc = float(y.min() if sf < 0 else y.max())
        ref = gp.sweep(acq, sf, inc, par)
        res = gp.sweep_batch(1, L.BATCH_KB, 0.0, None, acq, sf, inc, par)
        assert int(res["idx"][0]) == ref["best_idx"], (acq, res["idx"], ref["best_idx"])
        assert np.float64(res["val"][0]).tobytes() == np.float64(ref["best_val"]).tobytes()
        assert res["n_clamped"] == ref["n_clamped"]


@pytest.mark.parametrize("dtype", ["f32h2", "f32x3"])
@pytest.mark.parametrize("N", [100, 200, 700])
def test_q1_is_the_sweep_for_f32_families(dtype, N):
    X, y, ls, Xc, _ = _problem(N, 6, 4000, 7 * N)
    _assert_q1_is_the_sweep(_gp(dtype, X, y, "matern52", 1.0, ls, 1e-3, 1e-10, True, Xc), y)


@pytest.mark.parametrize("env", [("TGP_CHUNK", "1024"), ("TGP_MID_MAXM", "100000")])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_q1_is_the_sweep_under_per_call_switches(env, dtype, monkeypatch):
    # (both switches are read at every call; 256 < N <= 512 is where TGP_MID_MAXM opts in the mid sweep)
    monkeypatch.setenv(*env)
    X, y, ls, Xc, _ = _problem(400, 5, 5000, 3)
    gp = _gp(dtype, X, y, "rbf", 1.0, ls, 1e-3, 1e-10, True, Xc)
    _assert_q1_is_the_sweep(gp, y)
    if dtype == "f64":
        om = o.fit(X, y, "rbf", 1.0, ls, 1e-3, 1e-10, True)
        _check_parity(gp, om, Xc, 6, br.CL, float(y.mean()), None, "ei", -1.0, float(y.min()), 0.01)


@pytest.mark.parametrize("dtype", ["f32h2", "f32x3"])
def test_f32_family_parity(dtype):
    X, y, ls, Xc, Xp = _problem(700, 8, 5000, 70, ard=True, n_pending=3)
    gp = _gp(dtype, X, y, "matern52", 1.0, ls, 1e-3, 1e-10, True, Xc)
    om = o.fit(X, y, "matern52", 1.0, ls, 1e-3, 1e-10, True)
    _check_parity(gp, om, Xc, 8, br.KB, 0.0, Xp, "ei", -1.0, float(y.min()), 0.01, f64=False)
    _check_parity(gp, om, Xc, 8, br.CL, float(y.min()), None, "ucb", 1.0, float(y.max()), 2.0, f64=False)


def test_read_once_switches_in_a_child_process():
    """TGP_SMALL / TGP_MID / TGP_TILE / TGP_SLAB_GB + TGP_KS_JS are read once per process: a fresh child per setting"""
    for env in ({"TGP_SMALL": "0"}, {"TGP_MID": "0"}, {"TGP_TILE": "128"}, {"TGP_SLAB_GB": "0.001", "TGP_KS_JS": "1"}):
        e = dict(os.environ)
        e.update(env)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_batch_paths_child.py")], env=e, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0 and "batch-paths ok" in r.stdout, (env, r.stdout[-3000:])


def test_a_front_left_by_an_overlapped_fit():
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, Xc, Xp = _problem(600, 6, 6000, 5, n_pending=3)
    a, b = ta.NativeGP(0, "f64"), ta.NativeGP(0, "f64")
    if a.stream_status()["third_overlaps"] == 0:
        pytest.skip("no third stream on this device: tgp_set_overlap is a no-op")
    a.set_overlap(2)
    b.set_overlap(0)
    inc = float(y.min())

    def fit(g):   # (the candidates resident before the fit: the fit starts their sweep)
        g.fit(X, y, "matern52", 1.0, ls, 1e-3, 1e-10, True)

    for g in (a, b):
        fit(g)
        g.set_candidates(Xc)
        fit(g)
    r1 = a.sweep_batch(1, L.BATCH_KB, 0.0, None, L.ACQ_EI, -1.0, inc, 0.01)
    s1 = b.sweep(L.ACQ_EI, -1.0, inc, 0.01)
    assert int(r1["idx"][0]) == s1["best_idx"] and np.float64(r1["val"][0]).tobytes() == np.float64(s1["best_val"]).tobytes()
    for g in (a, b):
        fit(g)
    ra = a.sweep_batch(8, L.BATCH_CL, float(y.mean()), Xp, L.ACQ_EI, -1.0, inc, 0.01, want_posterior=True)
    rb = b.sweep_batch(8, L.BATCH_CL, float(y.mean()), Xp, L.ACQ_EI, -1.0, inc, 0.01, want_posterior=True)
    _assert_same(ra, rb)
    a.close()


def _assert_same(ra, rb, keys=("idx", "val", "x", "fantasies", "mu", "sigma", "n_clamped")):
    for k in keys:
        if isinstance(ra[k], np.ndarray):
            assert ra[k].tobytes() == rb[k].tobytes(), k
        else:
            assert ra[k] == rb[k], k


# ---- handle states --------------------------------------------------------------------------------------------------

def test_after_an_appended_observation():
    import turbo_amd as ta
    X, y, ls, Xc, Xp = _problem(300, 5, 3000, 13, n_pending=2)
    gp = ta.NativeGP(0, "f64")
    gp.fit(X[:299], y[:299], "matern32", 1.3, ls, 1e-3, 1e-10, True)
    gp.set_candidates(Xc)
    gp.sweep_batch(4, 0, 0.0, Xp, 3, -1.0, float(y.min()), 0.01)
    gp.fit(X, y, "matern32", 1.3, ls, 1e-3, 1e-10, True, append=True)
    assert gp.appended
    gp.set_candidates(Xc)
    om = o.fit(X, y, "matern32", 1.3, ls, 1e-3, 1e-10, True)
    # (append is not bit-equal to a refit: held to the reference on the appended data)
    _check_parity(gp, om, Xc, 8, br.KB, 0.0, Xp, "ei", -1.0, float(y.min()), 0.01)


@pytest.mark.parametrize("N,dtype,M", [(40, "f64", 3000), (700, "f64", 5000), (1300, "f32", 6000)])
def test_a_receiver_handle_selects_what_the_giver_selects(N, dtype, M):
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, Xc, Xp = _problem(N, 6, M, N, n_pending=3)
    a = _gp(dtype, X, y, "rbf", 1.1, ls, 1e-2, 1e-10, True, Xc)
    args = (8, L.BATCH_CL, float(y.min()), Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01)
    ra = a.sweep_batch(*args, want_posterior=True)
    f = a.export_factor()
    for blocks in (None, 128):
        b = ta.NativeGP(0, dtype)
        if blocks is None:
            assert b.import_factor(f)
        else:
            for r0 in range(0, f.Np, blocks):
                b.import_factor(f, r0, blocks)
        b.set_candidates(Xc)
        _assert_same(ra, b.sweep_batch(*args, want_posterior=True))


def test_after_import_state():
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, Xc, Xp = _problem(300, 4, 4000, 17, ard=True, n_pending=2)
    a = _gp("f64", X, y, "matern12", 0.3, ls, 1e-3, 1e-10, False, Xc)
    b = ta.NativeGP(0, "f64")
    b.import_state(a.export_state())
    b.set_candidates(Xc)
    for args in ((6, L.BATCH_KB, 0.0, Xp, L.ACQ_PI, 1.0, float(y.max()), 0.0),
                 (6, L.BATCH_CL, float(y.max()), None, L.ACQ_SIGMA, -1.0, 0.0, 0.0)):
        _assert_same(a.sweep_batch(*args, want_posterior=True), b.sweep_batch(*args, want_posterior=True))


def test_handle_reuse_across_shapes():
    """one handle, growing and shrinking M, D, N, q and P, ordinary sweeps in between: every result is a fresh handle's
    (the grow-only d_bt / d_btm / d_bti buffers, their per-call layout, the mask / flag / clamp resets)"""
    import turbo_amd as ta
    L = ta._lib
    seq = [  # N, D, M, q, P, kind
        (300, 6, 5000, 8, 2, "rbf"), (60, 3, 800, 3, 0, "matern52"), (700, 20, 9000, 16, 10, "matern32"),
        (200, 17, 300, 30, 0, "matern12"), (300, 6, 5000, 8, 2, "rbf"), (1030, 2, 200, 64, 0, "rbf"),
        (40, 33, 3000, 1, 63, "matern52"),
    ]
    h = ta.NativeGP(0, "f64")
    for n, (N, D, M, q, P, kind) in enumerate(seq):
        X, y, ls, Xc, Xp = _problem(N, D, M, 1000 + n, n_pending=P)
        inc = float(y.min())
        acq = (L.ACQ_EI, L.ACQ_UCB, L.ACQ_SIGMA)[n % 3]
        args = (q, n % 2, float(y.mean()), Xp if P else None, acq, -1.0, inc, 0.01 if acq == L.ACQ_EI else 2.0)
        h.fit(X, y, kind, 1.0, ls, 1e-3, 1e-10, True)
        h.set_candidates(Xc)
        if n % 2:
            h.sweep(L.ACQ_EI, -1.0, inc, 0.01, want_mu=True, want_sigma=True)
        r = h.sweep_batch(*args, want_posterior=True)
        fresh = _gp("f64", X, y, kind, 1.0, ls, 1e-3, 1e-10, True, Xc)
        _assert_same(r, fresh.sweep_batch(*args, want_posterior=True))
        fresh.close()
        s = h.sweep(L.ACQ_EI, -1.0, inc, 0.01, want_mu=True, want_sigma=True, want_acq=True)
        assert int(np.argmax(s["acq"])) == s["best_idx"]


def _raw(gp, q, strategy, lie, Xp, acq, sf, inc, par, x=True, fant=True, nc=True, post=True):
    """tgp_sweep_batch with chosen nullable outputs left NULL"""
    import turbo_amd as ta
    L = ta._lib
    P = 0 if Xp is None else len(Xp)
    out = dict(idx=np.full(q, -1, dtype=np.int64), val=np.full(q, np.nan))
    out["x"] = np.full((q, gp.D), np.nan) if x else None
    out["fantasies"] = np.full(P + q, np.nan) if fant else None
    out["mu"] = np.full(gp.M, np.nan) if post else None
    out["sigma"] = np.full(gp.M, np.nan) if post else None
    n = ctypes.c_int64(-1)
    p = lambda a: None if a is None else a.ctypes.data_as(L._dp)   # noqa: E731
    Xp = None if Xp is None else np.ascontiguousarray(Xp, dtype=np.float64)
    rc = gp.lib.tgp_sweep_batch(gp._h, q, strategy, lie, p(Xp), P, acq, sf, inc, par, out["idx"].ctypes.data_as(L._i64p),
                                p(out["val"]), p(out["x"]), p(out["fantasies"]), p(out["mu"]), p(out["sigma"]),
                                ctypes.byref(n) if nc else None)
    assert rc == L.OK
    out["n_clamped"] = n.value if nc else None
    return out


@pytest.mark.parametrize("N", [100, 200, 600])
def test_same_inputs_same_outputs(N):
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, Xc, Xp = _problem(N, 5, 4000, 3 * N, n_pending=3)
    gp = _gp("f64", X, y, "matern52", 1.0, ls, 1e-3, 1e-10, True, Xc)
    args = (8, L.BATCH_KB, 0.0, Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01)
    full = _raw(gp, *args)
    _assert_same(full, _raw(gp, *args))                         # twice: the same bytes
    nopost = _raw(gp, *args, post=False)                        # no posterior (the last pass skipped): the same picks
    _assert_same(full, nopost, ("idx", "val", "x", "fantasies"))
    _assert_same(full, _raw(gp, *args, x=False, fant=False, nc=False), ("idx", "val", "mu", "sigma"))
    _assert_same(full, _raw(gp, *args, x=False), ("idx", "val", "fantasies", "mu", "sigma", "n_clamped"))
    # (without the posterior the last point's update does not run, and neither do its clamps: compared among such calls)
    _assert_same(nopost, _raw(gp, *args, x=False, fant=False, post=False), ("idx", "val", "n_clamped"))


def test_n_clamped():
    import turbo_amd as ta
    L = ta._lib
    # noisy: the reference sees no negative variance at all, so the count is 0
    X, y, ls, Xc, Xp = _problem(300, 4, 3000, 23, n_pending=3)
    gp = _gp("f64", X, y, "rbf", 1.0, ls, 1e-2, 1e-10, True, Xc)
    om = o.fit(X, y, "rbf", 1.0, ls, 1e-2, 1e-10, True)
    res, ref = _check_parity(gp, om, Xc, 8, br.KB, 0.0, Xp, "ei", -1.0, float(y.min()), 0.01)
    assert ref["n_clamped_steps"] == 0 and res["n_clamped"] == 0
    # noise-free, jitter only, pending points that ARE candidate rows: each row's variance after its own conditioning is
    # zero up to rounding (var - var), so clamps must happen; the count is the first sweep's plus the steps'
    X, y, ls, Xc, _ = _problem(60, 2, 400, 29, ls_scale=0.5)
    gp = _gp("f64", X, y, "rbf", 1.0, ls, 0.0, 0.0, False, Xc)
    Xp = Xc[:20]
    first = gp.sweep(L.ACQ_SIGMA, 1.0, 0.0, 0.0)
    res = gp.sweep_batch(4, L.BATCH_KB, 0.0, Xp, L.ACQ_SIGMA, 1.0, 0.0, 0.0, want_posterior=True)
    assert res["n_clamped"] > first["n_clamped"], (res["n_clamped"], first["n_clamped"])
    assert not set(res["idx"].tolist()) & set(range(20))       # (a pending row has sigma 0: never the SIGMA pick)


@pytest.mark.parametrize("N", [100, 200])
def test_ties_on_duplicate_rows(N):
    """duplicate candidate rows (row i + M0 duplicates row i): identical bits in the first sweep on the small (N <= 128)
    and mid (128 < N <= 256) paths, the lower index first, and under SIGMA with KB the duplicate is not the next pick"""
    import turbo_amd as ta
    L = ta._lib
    M0 = 1500
    X, y, ls, C, _ = _problem(N, 4, M0, 41 + N)
    Xc = np.vstack([C, C])
    gp = _gp("f64", X, y, "matern52", 1.0, ls, 1e-3, 1e-10, True, Xc)
    s = gp.sweep(L.ACQ_SIGMA, 1.0, 0.0, 0.0, want_mu=True, want_sigma=True, want_acq=True)
    for k in ("mu", "sigma", "acq"):
        assert s[k][:M0].tobytes() == s[k][M0:].tobytes(), k
    assert s["best_idx"] < M0
    for acq, sf, par in ((L.ACQ_SIGMA, 1.0, 0.0), (L.ACQ_EI, -1.0, 0.01), (L.ACQ_UCB, 1.0, 2.0)):
        r = gp.sweep_batch(8, L.BATCH_KB, 0.0, None, acq, sf, float(y.min()), par)
        idx = r["idx"].tolist()
        assert idx[0] < M0
        assert all(i < M0 or i - M0 in idx[:k] for k, i in enumerate(idx)), idx
        if acq == L.ACQ_SIGMA:
            assert idx[1] != idx[0] + M0


# ---- the plugin layer -----------------------------------------------------------------------------------------------

def _model(X, y, kind="matern52"):
    import turbo_amd as ta
    kern = ta.GPKernel(kind, 1.0, 0.4, 1e-3)
    sur = ta.HipGPSurrogate(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=1)
    return sur.construct_model(0, X, y)[0]


@pytest.mark.parametrize("design", ["uniform", "lhs"])
def test_device_rng_select_batch_equals_the_host_fed_batch(design):
    import turbo_amd as ta
    from turbo_amd.auxiliary_optimisers import CandidateSweep
    from turbo_amd.acquisition_functions import EI
    lb = ta.Bounds([("a", -1.0, 2.0), ("b", 0.0, 1.0), ("c", 3.0, 5.0)])
    rng = np.random.RandomState(2)
    lo, hi = np.array([-1.0, 0.0, 3.0]), np.array([2.0, 1.0, 5.0])
    X = lo + (hi - lo) * rng.uniform(0, 1, (150, 3))
    y = np.sin(X.sum(1)) + 0.1 * X[:, 0] ** 2
    model = _model(X, y)
    acq, _ = EI(0.01).construct_function(0, model, 'min', float(y.min()))
    opt = CandidateSweep(num_random=3000, device_rng_seed=11, device_design=design)
    xs, info = opt.select_batch(lb, acq, 6, strategy='constant_liar', lie='mean', pending=X[:2] + 0.05)
    ctx = model._ensure_resident()
    Xc = ctx.read_candidates()
    assert Xc.shape == (3000, 3)
    res = acq.maximise_batch(Xc, 6, 'constant_liar', 'mean', X[:2] + 0.05)
    np.testing.assert_array_equal(res["idx"], info["candidate_indices"])
    np.testing.assert_array_equal(res["val"], info["max_acq"])
    np.testing.assert_array_equal(res["x"], xs)


def test_a_worker_loop_with_prefetch_chooses_what_it_chooses_without():
    """the W-worker loop of INTEGRATION.md, __call__ and select_batch in turn: with prefetch_next=True the next trial's
    fit starts the sweep of the prefetched batch (a front a batch call then uses); the batches are the same"""
    import turbo_amd as ta
    from turbo_amd.auxiliary_optimisers import CandidateSweep
    from turbo_amd.acquisition_functions import EI
    lb = ta.Bounds([("a", 0.0, 1.0), ("b", 0.0, 1.0), ("c", 0.0, 1.0), ("d", 0.0, 1.0)])
    f = lambda x: float(np.sin(3 * x.sum()) + ((x - 0.3) ** 2).sum())    # noqa: E731

    def loop(prefetch):
        rng = np.random.RandomState(5)
        X = list(rng.uniform(0, 1, (300, 4)))
        y = [f(x) for x in X]
        kern = ta.GPKernel("matern52", 1.0, 0.5, 1e-3)
        sur = ta.HipGPSurrogate(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=1)
        opt = CandidateSweep(num_random=6000, device_rng_seed=3, prefetch_next=prefetch)
        running, out = [], []
        for it in range(6):
            model, _ = sur.construct_model(len(y), np.array(X), np.array(y))
            acq, _ = EI(0.01).construct_function(len(y), model, 'min', min(y))
            if it % 2 == 0:
                x, _ = opt(lb, acq)
                xs = np.asarray(x).reshape(1, -1)
            else:
                xs, _ = opt.select_batch(lb, acq, 3, strategy='kriging_believer',
                                         pending=np.array(running) if running else None)
            out.append(xs.copy())
            running.extend(list(xs))
            while len(running) > 2:             # the oldest trials finish
                x = running.pop(0)
                X.append(x)
                y.append(f(x))
        return out

    a, b = loop(True), loop(False)
    for xa, xb in zip(a, b):
        assert xa.tobytes() == xb.tobytes()


@pytest.mark.parametrize("kind", ["rbf", "matern12"])
def test_ucb_inf_through_select_batch_is_sigma(kind):
    import turbo_amd as ta
    from turbo_amd.auxiliary_optimisers import CandidateSweep
    from turbo_amd.acquisition_functions import UCB
    lb = ta.Bounds([("a", 0.0, 1.0), ("b", 0.0, 1.0)])
    rng = np.random.RandomState(8)
    X = rng.uniform(0, 1, (40, 2))
    y = np.cos(4 * X[:, 0]) + X[:, 1]
    model = _model(X, y, kind)
    acq, _ = UCB(float('inf')).construct_function(0, model, 'max')
    opt = CandidateSweep(num_random=2000, device_rng_seed=4)
    xs, info = opt.select_batch(lb, acq, 5, strategy='constant_liar', lie=0.25)
    Xc = model._ensure_resident().read_candidates()
    om = o.fit(X, y, kind, 1.0, 0.4, 1e-3, 1e-10, True)
    ref = br.select_batch(om, Xc, 5, br.CL, 0.25, None, "ucb", "max", np.inf, float(y.max()),
                          forced=info["candidate_indices"])
    for k in range(5):
        assert (ref["best"][k] - ref["acq"][k][info["candidate_indices"][k]]) <= 1e-9 * ref["best"][k]
    np.testing.assert_allclose(info["max_acq"], [ref["acq"][k][i] for k, i in enumerate(info["candidate_indices"])],
                               rtol=1e-9)


@pytest.mark.parametrize("lie", ["max", "mean", -0.7])
def test_maximise_batch_maximising_with_every_lie(lie):
    import turbo_amd as ta
    from turbo_amd.acquisition_functions import EI
    rng = np.random.RandomState(9)
    X = rng.uniform(0, 1, (150, 3))
    y = np.sin(3 * X.sum(1))
    model = _model(X, y)
    acq, _ = EI(0.01).construct_function(0, model, 'max', float(y.max()))
    Xc = rng.uniform(0, 1, (3000, 3))
    Xp = rng.uniform(0, 1, (2, 3))
    res = acq.maximise_batch(Xc, 6, 'constant_liar', lie, Xp, want_posterior=True)
    lv = br.resolve_lie(lie, y)
    assert res["lie"] == lv
    np.testing.assert_array_equal(res["fantasies"], np.full(8, lv))
    om = o.fit(X, y, "matern52", 1.0, 0.4, 1e-3, 1e-10, True)
    ref = br.select_batch(om, Xc, 6, br.CL, lv, Xp, "ei", "max", 0.01, float(y.max()), forced=res["idx"])
    for k in range(6):
        best = ref["best"][k]
        assert (best - ref["acq"][k][res["idx"][k]]) / max(abs(best), 1e-300) <= 1e-9
    np.testing.assert_allclose(res["mu"], ref["mu"], rtol=1e-5, atol=1e-9 * om.y_std)
