"""Thompson sampling on the GPU (tgp_ts_draw / tgp_ts_sweep / tgp_ts_eval / tgp_ts_read, the TS plugin), held to
tests/ts_reference.py -- the NumPy restatement of the draw and of the pathwise update on SciPy's Cholesky of K --
and to oracle.gp_oracle."""
import numpy as np
import pytest

from oracle import gp_oracle as o
import ts_reference as tr

pytestmark = pytest.mark.gpu

F_TOL = 1e-9        # |f_gpu - f_ref| <= F_TOL * y_std * (1 + scale of the update term), see _f_tol


def _problem(N, D, kind, noise, M, seed, ard=False, constant=1.0, normalize_y=True):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    w = rng.normal(size=D) / np.sqrt(D)
    y = 3.0 + 2.0 * np.sin(3 * X @ w) + 0.5 * ((X - 0.5) ** 2).sum(1) + 0.01 * rng.normal(size=N)
    iso = float(np.sqrt(D / 6.0))
    ls = iso * (0.5 + np.arange(D) / max(D - 1.0, 1.0)) if ard else iso
    Xc = rng.uniform(0, 1, (M, D))
    return X, y, ls, Xc


def _gp(dtype, X, y, kind, constant, ls, noise, normalize_y, Xc=None, jitter=1e-10):
    import turbo_amd as ta
    gp = ta.NativeGP(0, dtype)
    gp.fit(X, y, kind, constant, ls, noise, jitter, normalize_y)
    if Xc is not None:
        gp.set_candidates(Xc)
    return gp


def _f_tol(ref, Xq):
    """the rounding scale of f: y_std times the size of the terms that cancel in the update (|k| |v| summed)"""
    Ks = o.cross_kernel(np.atleast_2d(Xq), ref.m.X, ref.m.kind, ref.m.constant, ref.ls)
    mag = np.abs(Ks) @ np.abs(ref.V).T + np.abs(ref.d["W"]).sum(1)[None, :] * ref.scale
    return F_TOL * ref.m.y_std * (1.0 + mag)


CASES = [
    # N, D, kind, ard, constant, normalize_y, noise, S, F, M, sf, distinct
    (1, 3, "rbf", False, 1.0, True, 1e-2, 1, 64, 1, 1.0, False),
    (32, 1, "matern12", False, 0.3, True, 1e-2, 8, 2048, 10000, -1.0, True),
    (128, 3, "matern32", True, 4.0, False, 1e-5, 64, 64, 5000, 1.0, True),
    (129, 17, "matern52", True, 0.3, True, 1e-2, 8, 2048, 20000, -1.0, False),
    (256, 32, "rbf", False, 4.0, True, 1e-5, 1, 2048, 65536, 1.0, False),
    (257, 100, "matern12", True, 1.0, False, 1e-2, 64, 2048, 3000, -1.0, True),
    (1025, 17, "matern32", False, 1.0, True, 1e-2, 8, 64, 16384, 1.0, True),
    (4096, 32, "matern52", True, 0.3, True, 1e-2, 8, 2048, 16384, -1.0, True),
    (64, 3, "rbf", True, 1.0, True, 1e-5, 64, 2048, 64, 1.0, True),              # S = M, distinct
]


@pytest.mark.parametrize("case", CASES, ids=["N%d-D%d-%s-S%d-F%d-M%d" % (c[0], c[1], c[2], c[7], c[8], c[9]) for c in CASES])
def test_sweep_matches_the_reference(case):
    N, D, kind, ard, const, ny, noise, S, F, M, sf, distinct = case
    X, y, ls, Xc = _problem(N, D, kind, noise, M, N + D, ard, const, ny)
    gp = _gp("f64", X, y, kind, const, ls, noise, ny, Xc)
    seed = 1234567 + N
    gp.ts_draw(seed, S, F)
    m = o.fit(X, y, kind, const, ls, noise, 1e-10, ny)
    ref = tr.Paths(m, seed, S, F)
    # the draw itself
    got = gp.ts_read()
    d = ref.d
    assert got["b"].tobytes() == d["b"].tobytes()
    np.testing.assert_allclose(got["omega"], d["omega"], rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(got["W"], d["W"], rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(got["eps"], d["eps"], rtol=1e-14, atol=1e-15 * np.sqrt(noise))
    # every sampled value, then the selections
    res = gp.ts_sweep(sf, distinct, want_f=True)
    want = ref.values(Xc, chunk=2048)
    tol = _f_tol(ref, Xc)
    err = np.abs(res["f"] - want)
    assert np.all(err <= tol), (float(err.max()), float((err / tol).max()))
    idx, val = tr.select(want, sf, distinct)
    gidx = res["idx"]
    for s in range(S):
        if gidx[s] != idx[s]:       # only a tie below the rounding may differ: regret 0 to that scale
            assert sf * (want[idx[s], s] - want[gidx[s], s]) <= 2 * max(tol[idx[s], s], tol[gidx[s], s]), s
    np.testing.assert_array_equal(res["val"], res["f"][gidx, np.arange(S)])
    np.testing.assert_array_equal(res["x"], Xc[gidx])
    if distinct:
        assert len(set(gidx.tolist())) == S


@pytest.mark.parametrize("kind,ard,N,D", [("rbf", False, 40, 3), ("matern12", True, 300, 5), ("matern32", True, 129, 17),
                                          ("matern52", False, 1025, 2)])
def test_eval_values_and_gradients(kind, ard, N, D):
    X, y, ls, _ = _problem(N, D, kind, 1e-3, 1, 7, ard)
    gp = _gp("f64", X, y, kind, 1.0, ls, 1e-3, True)
    S, F = 8, 2048
    gp.ts_draw(99, S, F)
    ref = tr.Paths(o.fit(X, y, kind, 1.0, ls, 1e-3, 1e-10, True), 99, S, F)
    rng = np.random.RandomState(3)
    Xq = np.vstack([rng.uniform(0, 1, (37, D)), X[:3] + 1e-3])
    f, g = gp.ts_eval(Xq, want_grad=True)
    tol = _f_tol(ref, Xq)
    assert np.all(np.abs(f - ref.values(Xq)) <= tol)
    gw = ref.grad(Xq)
    np.testing.assert_allclose(g, gw, rtol=1e-9, atol=1e-9 * float(np.abs(gw).max()))
    f2, g2 = gp.ts_eval(Xq)
    assert g2 is None and f2.tobytes() == f.tobytes()


def test_same_seed_is_bit_identical_and_f32_handle_equals_f64():
    X, y, ls, Xc = _problem(600, 8, "matern52", 1e-3, 20000, 5, True)
    a = _gp("f64", X, y, "matern52", 1.0, ls, 1e-3, True, Xc)
    b = _gp("f32", X, y, "matern52", 1.0, ls, 1e-3, True, Xc)
    outs = []
    for gp in (a, a, b):
        gp.ts_draw(2024, 8, 2048)
        r = gp.ts_sweep(-1.0, True, want_f=True)
        outs.append((gp.ts_read(), r))
    for (d, r) in outs[1:]:
        for k in ("omega", "b", "W", "eps"):
            assert d[k].tobytes() == outs[0][0][k].tobytes(), k
        assert r["f"].tobytes() == outs[0][1]["f"].tobytes()
        np.testing.assert_array_equal(r["idx"], outs[0][1]["idx"])


def test_sample_s_does_not_depend_on_S():
    X, y, ls, Xc = _problem(200, 4, "rbf", 1e-3, 5000, 9)
    gp = _gp("f64", X, y, "rbf", 1.0, ls, 1e-3, True, Xc)
    gp.ts_draw(77, 1, 1024)
    f1 = gp.ts_sweep(1.0, want_f=True)
    gp.ts_draw(77, 64, 1024)
    f64 = gp.ts_sweep(1.0, True, want_f=True)
    np.testing.assert_allclose(f64["f"][:, 0], f1["f"][:, 0], rtol=0, atol=1e-12 * float(np.abs(f1["f"]).max()))
    assert f64["idx"][0] == f1["idx"][0]


def test_handle_is_untouched():
    L = __import__("turbo_amd")._lib
    X, y, ls, Xc = _problem(300, 6, "matern52", 1e-4, 8000, 11)
    for dtype in ("f64", "f32"):
        gp = _gp(dtype, X, y, "matern52", 1.0, ls, 1e-4, True, Xc)
        s0 = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True)
        b0 = gp.sweep_batch(4, L.BATCH_KB, 0.0, None, L.ACQ_EI, -1.0, float(y.min()), 0.01)
        gp.ts_draw(5, 16, 2048)
        gp.ts_sweep(1.0, True)
        gp.ts_eval(Xc[:10], want_grad=True)
        s1 = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True)
        b1 = gp.sweep_batch(4, L.BATCH_KB, 0.0, None, L.ACQ_EI, -1.0, float(y.min()), 0.01)
        assert s0["mu"].tobytes() == s1["mu"].tobytes() and s0["sigma"].tobytes() == s1["sigma"].tobytes()
        assert (s0["best_idx"], s0["best_val"]) == (s1["best_idx"], s1["best_val"])
        np.testing.assert_array_equal(b0["idx"], b1["idx"])
        assert b0["val"].tobytes() == b1["val"].tobytes()


def _refused(fn):
    with pytest.raises(Exception) as ei:
        fn()
    assert "draw" in str(ei.value) or "fitted" in str(ei.value)


def test_refits_appends_and_imports_invalidate_the_draw():
    X, y, ls, Xc = _problem(100, 3, "rbf", 1e-3, 500, 13)
    gp = _gp("f64", X, y, "rbf", 1.0, ls, 1e-3, True, Xc)
    _refused(lambda: gp.ts_sweep(1.0))                 # no draw yet
    checks = (lambda: gp.ts_sweep(1.0), lambda: gp.ts_eval(Xc[:2]), lambda: gp.ts_read())
    gp.ts_draw(1, 2, 64)
    gp.ts_sweep(1.0)
    gp.fit(X, y, "rbf", 1.0, ls, 1e-3, 1e-10, True)     # the same data again: still a new fit
    for c in checks:
        _refused(c)
    gp.ts_draw(1, 2, 64)
    X2, y2 = np.vstack([X, Xc[:1]]), np.append(y, 0.5)
    gp.fit(X2, y2, "rbf", 1.0, ls, 1e-3, 1e-10, True, append=True)
    assert gp.appended
    for c in checks:
        _refused(c)
    gp.ts_draw(1, 2, 64)
    gp.import_state(gp.export_state())
    for c in checks:
        _refused(c)
    other = _gp("f64", X, y, "rbf", 1.0, ls, 1e-3, True)
    gp.ts_draw(1, 2, 64)
    gp.import_factor(other.export_factor())
    for c in checks:
        _refused(c)
    gp.ts_draw(1, 2, 64)                                # a received factor draws (alpha, no y~ needed)
    gp.set_candidates(Xc)
    r_imp = gp.ts_sweep(1.0, want_f=True)
    other.set_candidates(Xc)
    other.ts_draw(1, 2, 64)
    r_own = other.ts_sweep(1.0, want_f=True)
    assert r_imp["f"].tobytes() == r_own["f"].tobytes()


def test_plugin_end_to_end():
    import turbo_amd as ta
    from turbo_amd.bounds import Bounds
    rng = np.random.RandomState(21)
    D = 3
    X = rng.uniform(0, 1, (40, D))
    y = np.sin(3 * X.sum(1)) + 0.01 * rng.normal(size=40)
    kern = ta.GPKernel("matern52", 1.0, 0.7, 1e-4)
    sur = ta.HipGPSurrogate(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=1)
    model, _ = sur.construct_model(0, X, y)
    lb = Bounds([("x%d" % i, 0.0, 1.0) for i in range(D)])
    fac = ta.TS(seed=11, n_features=1024)
    assert fac.get_type() == "optimism"
    acq, info = fac.construct_function(3, model, "min")
    assert acq.get_name() == "TS" and info["seed"] == (11 + 3 * 0x9E3779B97F4A7C15) % (1 << 64)
    om = o.fit(X, y, "matern52", 1.0, 0.7, 1e-4, 1e-10, True)
    ref = tr.Paths(om, info["seed"], 1, 1024)
    Xq = rng.uniform(0, 1, (200, D))
    np.testing.assert_allclose(acq(Xq), -ref.values(Xq)[:, 0], rtol=0, atol=1e-8)
    np.testing.assert_allclose(acq(Xq[:5]), -ref.values(Xq[:5])[:, 0], rtol=0, atol=1e-8)
    v, g = acq.value_and_grad(Xq[:4])
    np.testing.assert_allclose(g, -ref.grad(Xq[:4])[:, 0, :], rtol=1e-8, atol=1e-8)
    # CandidateSweep q = 1 on a host batch, and the gradient stage with lockstep='scipy'
    np.random.seed(5)
    x1, i1 = ta.CandidateSweep(num_random=4000)(lb, acq)
    np.random.seed(5)
    Xc = ta.random_selector()(4000, lb)
    want = -ref.values(Xc)[:, 0]
    assert abs(i1["max_acq"] - want.max()) <= 1e-8
    np.testing.assert_array_equal(x1[0], Xc[int(np.argmax(want))])
    x2, i2 = ta.CandidateSweep(num_random=2000, grad_restarts=3, start_from_best=1, lockstep="scipy")(lb, acq)
    assert i2["max_acq"] >= want[:2000].max() - 1e-8 or i2["max_acq"] >= -ref.values(x2)[0, 0] - 1e-8
    assert abs(i2["max_acq"] - (-ref.values(x2)[0, 0])) <= 1e-7
    with pytest.raises(NotImplementedError):
        ta.CandidateSweep(num_random=100, grad_restarts=2, lockstep=True)(lb, acq)
    with pytest.raises(NotImplementedError):
        ta.CandidateSweep(num_random=100, grad_restarts=2, on_device=True)(lb, acq)
    # device draw
    xg, ig = ta.CandidateSweep(num_random=3000, device_rng_seed=8)(lb, acq)
    assert np.isfinite(ig["max_acq"])
    with pytest.raises(NotImplementedError):
        ta.CandidateSweep(num_random=3000, device_rng_seed=8, prefetch_next=True)(lb, acq)
    # select_batch: q = 8 with pending points; the first selection is the q = 1 selection
    pend = rng.uniform(0, 1, (3, D))
    np.random.seed(6)
    xb, ib = ta.CandidateSweep(num_random=5000).select_batch(lb, acq, 8, strategy="thompson", pending=pend)
    np.random.seed(6)
    x1b, i1b = ta.CandidateSweep(num_random=5000).select_batch(lb, acq, 1, strategy="thompson")
    assert ib["pending_ignored"] == 3 and ib["strategy"] == "thompson" and ib["n_features"] == 1024
    assert len(set(ib["candidate_indices"].tolist())) == 8
    assert ib["candidate_indices"][0] == i1b["candidate_indices"][0]
    np.testing.assert_array_equal(xb[0], x1b[0])
    np.testing.assert_array_equal(ib["max_acq"], -ib["sample_values"])
    np.random.seed(6)
    Xc = ta.random_selector()(5000, lb)
    ref8 = tr.Paths(om, info["seed"], 8, 1024)
    idx, _ = tr.select(ref8.values(Xc), -1.0, True)
    np.testing.assert_array_equal(ib["candidate_indices"], idx)
    with pytest.raises(ValueError):
        ta.CandidateSweep(num_random=100).select_batch(lb, acq, 2, strategy="kriging_believer")
    ei, _ = ta.EI(0.01).construct_function(0, model, "min", float(y.min()))
    with pytest.raises(ValueError):
        ta.CandidateSweep(num_random=100).select_batch(lb, ei, 2, strategy="thompson")


def test_bad_arguments():
    X, y, ls, Xc = _problem(50, 2, "rbf", 1e-3, 10, 17)
    gp = _gp("f64", X, y, "rbf", 1.0, ls, 1e-3, True, Xc)
    lib, h, BAD = gp.lib, gp._h, 2   # TGP_BAD_ARG
    for S, F in ((0, 64), (65, 64), (1, 0), (1, 100), (1, 16448)):
        assert lib.tgp_ts_draw(h, 1, S, F) == BAD
    gp.ts_draw(1, 11, 64)
    with pytest.raises(Exception, match="distinct"):
        gp.ts_sweep(1.0, True)                       # S = 11 > M = 10
    with pytest.raises(Exception, match="sf"):
        gp.ts_sweep(0.5)
    assert lib.tgp_ts_sweep(h, 1.0, 0, None, None, None, None) == BAD
    assert lib.tgp_ts_eval(h, None, 1, None, None) == BAD
    with pytest.raises(Exception):
        gp.ts_eval(np.zeros((4097, 2)))
    gp.ts_sweep(1.0)                                  # the draw survives refused calls
