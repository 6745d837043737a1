"""tgp_sweep_batch on the GPU: greedy batch selection with Kriging Believer / Constant Liar (include/turbogp.h), held to
tests/batch_reference.py (whose rank-1 updates tests/test_batch_reference.py holds to literal refits)."""
import numpy as np
import pytest

from oracle import gp_oracle as o
import batch_reference as br

pytestmark = pytest.mark.gpu

REGRET_TOL = 1e-3      # f32 sweeps (tests/test_gpu_configs.py)
ACQS = {"ei": 3, "pi": 2, "ucb": 1}


def _problem(N, D, kind, noise, M, seed, ard=False, ls_scale=1.0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    w = rng.normal(size=D) / np.sqrt(D)
    y = np.sin(3 * X @ w) + 0.5 * ((X - 0.5) ** 2).sum(1) + 0.01 * rng.normal(size=N)
    iso = float(np.sqrt(D / 6.0)) * ls_scale
    ls = iso * (0.5 + np.arange(D) / max(D - 1.0, 1.0)) if ard else iso
    Xc = rng.uniform(0, 1, (M, D))
    Xp = rng.uniform(0, 1, (4, D))
    return X, y, ls, Xc, Xp


def _gp(dtype, X, y, kind, ls, noise, Xc, jitter=1e-10):
    import turbo_amd as ta
    gp = ta.NativeGP(0, dtype)
    gp.fit(X, y, kind, 1.0, ls, noise, jitter, True)
    gp.set_candidates(Xc)
    return gp


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [32, 200, 512, 2048])
def test_q1_without_pending_is_the_sweep_bit_for_bit(dtype, N):
    L = __import__("turbo_amd")._lib
    X, y, ls, Xc, _ = _problem(N, 6, "matern52", 1e-4, 3000, N)
    gp = _gp(dtype, X, y, "matern52", ls, 1e-4, Xc)
    for acq, sf, par in ((L.ACQ_EI, -1.0, 0.01), (L.ACQ_UCB, 1.0, 2.0), (L.ACQ_PI, 1.0, 0.0)):
        ref = gp.sweep(acq, sf, float(y.min() if sf < 0 else y.max()), par)
        for strategy in (L.BATCH_KB, L.BATCH_CL):
            res = gp.sweep_batch(1, strategy, float(y.mean()), None, acq, sf, float(y.min() if sf < 0 else y.max()), par)
            assert int(res["idx"][0]) == ref["best_idx"]
            assert np.float64(res["val"][0]).tobytes() == np.float64(ref["best_val"]).tobytes()
            np.testing.assert_array_equal(res["x"][0], Xc[ref["best_idx"]])


CASES = [
    # N, D, kind, noise, M, dtype, strategy, pending, acq, sf
    (32, 2, "matern52", 1e-4, 10000, "f64", br.KB, False, "ei", -1.0),
    (32, 2, "matern52", 1e-4, 10000, "f64", br.CL, True, "ei", -1.0),
    (200, 4, "rbf", 1e-3, 8192, "f64", br.KB, True, "ucb", 1.0),
    (200, 4, "rbf", 0.0, 8192, "f64", br.CL, False, "pi", 1.0),          # noise-free: jitter only
    (512, 8, "rbf", 1e-4, 8192, "f64", br.CL, True, "ei", 1.0),
    (512, 8, "matern32", 1e-4, 8192, "f64", br.KB, False, "ei", -1.0),
    (2048, 16, "matern52", 1e-4, 16384, "f64", br.KB, True, "ei", -1.0),
    (2048, 16, "matern52", 1e-4, 16384, "f64", br.CL, False, "ucb", 1.0),
    (4096, 32, "rbf", 1e-2, 65536, "f32", br.KB, True, "ei", -1.0),
    (4096, 32, "rbf", 1e-2, 65536, "f32", br.CL, False, "ei", -1.0),
]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(v) for v in c) for c in CASES])
def test_parity_with_the_reference_under_teacher_forcing(case):
    import turbo_amd as ta
    L = ta._lib
    N, D, kind, noise, M, dtype, strategy, pend, acq_name, sf = case
    # (the noise-free case at shorter length scales: with jitter alone on the diagonal the problem's own conditioning,
    # not the arithmetic, would decide the last digits of both sides)
    X, y, ls, Xc, Xp = _problem(N, D, kind, noise, M, 7 + N, ard=(kind == "matern52"), ls_scale=1.0 if noise > 0 else 0.4)
    jitter = 1e-10 if noise > 0 else 1e-8
    gp = _gp(dtype, X, y, kind, ls, noise, Xc, jitter)
    om = o.fit(X, y, kind, 1.0, ls, noise, jitter, True)
    q = 8
    Xp = Xp if pend else None
    desired = "max" if sf > 0 else "min"
    inc = float(y.max() if sf > 0 else y.min())
    par = 2.0 if acq_name == "ucb" else 0.01
    lie = float(y.min()) if strategy == br.CL else 0.0
    res = gp.sweep_batch(q, L.BATCH_KB if strategy == br.KB else L.BATCH_CL, lie, Xp, ACQS[acq_name], sf, inc, par,
                         want_posterior=True)
    idx = res["idx"]
    assert len(set(idx.tolist())) == q
    ref = br.select_batch(om, Xc, q, strategy, lie, Xp, acq_name, desired, par, inc, forced=idx)
    assert not ref["not_pd"]
    f64 = dtype == "f64"
    for k in range(q):
        best, got = ref["best"][k], ref["acq"][k][idx[k]]
        regret = (best - got) / max(abs(best), 1e-300)
        assert regret <= (1e-9 if f64 else REGRET_TOL), (k, best, got)
        # (f32: the first value comes from the f32 sweep; EI far below its scale moves by a few 1e-3 relative)
        np.testing.assert_allclose(res["val"][k], got, rtol=1e-9 if f64 else 1e-2, atol=1e-12 if f64 else 1e-6 * abs(best))
    np.testing.assert_array_equal(res["x"], Xc[idx])
    np.testing.assert_allclose(res["fantasies"], ref["fantasies"], rtol=1e-9 if f64 else 1e-6, atol=1e-12)
    s_y = om.y_std
    if f64:
        np.testing.assert_allclose(res["mu"], ref["mu"], rtol=1e-5, atol=1e-9 * s_y)
        np.testing.assert_allclose(res["sigma"] ** 2, ref["sigma"] ** 2, rtol=1e-5, atol=1e-9 * (1.0 + noise) * s_y ** 2)
    else:
        assert np.max(np.abs(res["mu"] - ref["mu"])) <= 5e-4 * s_y
        dvar = np.abs(res["sigma"] ** 2 - ref["sigma"] ** 2)
        assert np.max(dvar) <= 5e-5 * (1.0 + noise) * s_y ** 2


def test_the_handle_is_left_untouched():
    import turbo_amd as ta
    L = ta._lib
    for N in (32, 300, 1024):
        X, y, ls, Xc, Xp = _problem(N, 5, "rbf", 1e-4, 5000, 3 + N)
        gp = _gp("f64", X, y, "rbf", ls, 1e-4, Xc)
        before = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)
        gp.sweep_batch(6, L.BATCH_CL, float(y.min()), Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01, want_posterior=True)
        after = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)
        for k in ("mu", "sigma", "acq"):
            assert before[k].tobytes() == after[k].tobytes(), (N, k)
        assert (before["best_idx"], before["best_val"]) == (after["best_idx"], after["best_val"])


def test_not_pd_and_bad_arguments():
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, Xc, _ = _problem(40, 3, "rbf", 0.0, 500, 11)
    # one training point, noise 0, jitter 0, a pending duplicate of it: the augmented pivot is c - c^2 / c = 0 exactly
    gp = _gp("f64", X[:1], y[:1], "rbf", ls, 0.0, Xc, jitter=0.0)
    with pytest.raises(Exception) as ei:
        gp.sweep_batch(2, L.BATCH_KB, 0.0, X[:1], L.ACQ_EI, -1.0, float(y.min()), 0.01)
    assert "positive definite" in str(ei.value)
    assert gp._h is not None
    gp2 = _gp("f64", X, y, "rbf", ls, 1e-4, Xc)
    code = lambda *a: gp2.lib.tgp_sweep_batch(gp2._h, *a)   # noqa: E731
    import ctypes
    idx = np.zeros(64, dtype=np.int64)
    val = np.zeros(64)
    ip, vp = idx.ctypes.data_as(L._i64p), val.ctypes.data_as(L._dp)
    Xp = np.zeros((60, 3))
    nul = None
    assert code(5, L.BATCH_KB, 0.0, Xp.ctypes.data_as(L._dp), 60, L.ACQ_EI, 1.0, 0.0, 0.0, ip, vp, nul, nul, nul, nul, nul) == L.BAD_ARG
    assert code(501, L.BATCH_KB, 0.0, nul, 0, L.ACQ_EI, 1.0, 0.0, 0.0, ip, vp, nul, nul, nul, nul, nul) == L.BAD_ARG
    assert code(2, L.BATCH_KB, 0.0, nul, 0, L.ACQ_NONE, 1.0, 0.0, 0.0, ip, vp, nul, nul, nul, nul, nul) == L.BAD_ARG
    assert code(0, L.BATCH_KB, 0.0, nul, 0, L.ACQ_EI, 1.0, 0.0, 0.0, ip, vp, nul, nul, nul, nul, nul) == L.BAD_ARG
    assert code(2, L.BATCH_KB, 0.0, nul, 0, L.ACQ_EI, 1.0, 0.0, 0.0, ip, vp, nul, nul, nul, nul, ctypes.POINTER(ctypes.c_int64)()) == L.OK
    # the handle still serves ordinary calls after the refusals
    r = gp2.sweep(L.ACQ_EI, 1.0, 0.0, 0.0)
    assert 0 <= r["best_idx"] < 500


def test_select_batch_end_to_end_on_branin():
    import turbo_amd as ta
    from turbo_amd.auxiliary_optimisers import CandidateSweep
    from turbo_amd.acquisition_functions import EI
    lb = ta.Bounds([("x", -5.0, 10.0), ("y", 0.0, 15.0)])
    bounds = [(b[1], b[2]) for b in lb.ordered]
    rng = np.random.RandomState(0)
    X = np.column_stack([rng.uniform(lo, hi, 12) for lo, hi in bounds])
    y = (X[:, 1] - 5.1 / (4 * np.pi ** 2) * X[:, 0] ** 2 + 5 / np.pi * X[:, 0] - 6) ** 2 \
        + 10 * (1 - 1 / (8 * np.pi)) * np.cos(X[:, 0]) + 10
    kern = ta.GPKernel("matern52", 1.0, 3.0, 1e-4)
    sur = ta.HipGPSurrogate(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=1)
    model, _ = sur.construct_model(0, X, y)
    acq, _ = EI(0.01).construct_function(0, model, 'min', float(y.min()))
    opt = CandidateSweep(num_random=2000)
    np.random.seed(123)
    x1, info1 = opt(lb, acq)
    state_after_call = np.random.get_state()[1].copy()
    np.random.seed(123)
    xs, info = opt.select_batch(lb, acq, 4, strategy='constant_liar', lie='min', pending=X[:2] + 0.01)
    assert np.array_equal(np.random.get_state()[1], state_after_call)     # the RNG consumed as by one __call__
    assert xs.shape == (4, 2)
    assert len({tuple(r) for r in xs}) == 4
    for d, (lo, hi) in enumerate(bounds):
        assert np.all(xs[:, d] >= lo) and np.all(xs[:, d] <= hi)
    assert set(info) >= {'max_acq', 'candidate_indices', 'fantasies', 'pending_fantasies', 'strategy'}
    assert info['strategy'] == 'constant_liar'
    np.testing.assert_array_equal(info['fantasies'], np.full(4, y.min()))
    assert len(info['pending_fantasies']) == 2
    # KB without pending: its first pick is __call__'s winner
    np.random.seed(123)
    xk, infok = opt.select_batch(lb, acq, 3)
    np.testing.assert_array_equal(xk[0], np.asarray(x1).reshape(-1))
    assert infok['max_acq'][0] == info1['max_acq']
