"""tgp_sweep_batch_mc on the GPU: greedy batch selection by the Monte Carlo strategy (include/turbogp.h), held to
tests/mc_reference.py (whose rank-1 updates tests/test_mc_reference.py holds to S literal refits per step)."""
import ctypes

import numpy as np
import pytest

from oracle import gp_oracle as o
import batch_reference as br
import mc_reference as mr

pytestmark = pytest.mark.gpu

REGRET_TOL = 1e-3      # f32 sweeps (tests/test_gpu_configs.py)
ACQS = {"ei": 3, "pi": 2, "ucb": 1}


def _problem(N, D, kind, noise, M, seed, ard=False, ls_scale=1.0):
    """the generator of tests/test_gpu_batch.py"""
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
        inc = float(y.min() if sf < 0 else y.max())
        ref = gp.sweep(acq, sf, inc, par)
        for S, want_acq in ((1, False), (5, True), (64, False)):
            res = gp.sweep_batch_mc(1, S, 9, None, None, acq, sf, inc, par, want_acq=want_acq)
            assert int(res["idx"][0]) == ref["best_idx"]
            assert np.float64(res["val"][0]).tobytes() == np.float64(ref["best_val"]).tobytes()
            np.testing.assert_array_equal(res["x"][0], Xc[ref["best_idx"]])
            assert res["fantasies"].shape == (S, 1) and np.all(np.isfinite(res["fantasies"]))


@pytest.mark.parametrize("N", [32, 200, 2048])
@pytest.mark.parametrize("S", [3, 16])
def test_zero_eps_is_kriging_believer(N, S):
    """the mean of S equal numbers is exact only for S a power of two: values at rtol 1e-12, indices equal"""
    L = __import__("turbo_amd")._lib
    X, y, ls, Xc, Xp = _problem(N, 5, "rbf", 1e-4, 6000, 2 + N)
    gp = _gp("f64", X, y, "rbf", ls, 1e-4, Xc)
    for acq, sf, par, pend in ((L.ACQ_EI, -1.0, 0.01, Xp), (L.ACQ_PI, 1.0, 0.0, None), (L.ACQ_UCB, 1.0, 2.0, Xp),
                               (L.ACQ_EI, 1.0, 0.01, None)):
        inc = float(y.min() if sf < 0 else y.max())
        P = 0 if pend is None else len(pend)
        kb = gp.sweep_batch(6, L.BATCH_KB, 0.0, pend, acq, sf, inc, par, want_posterior=True)
        res = gp.sweep_batch_mc(6, S, 0, np.zeros((S, P + 6)), pend, acq, sf, inc, par, want_sigma=True)
        np.testing.assert_array_equal(res["idx"], kb["idx"])
        np.testing.assert_allclose(res["val"], kb["val"], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(res["x"], kb["x"])
        for s in range(S):
            np.testing.assert_allclose(res["fantasies"][s], kb["fantasies"], rtol=1e-12, atol=0)
        np.testing.assert_array_equal(res["eps"], np.zeros((S, P + 6)))
        assert res["sigma"].tobytes() == kb["sigma"].tobytes()
        assert res["n_clamped"] == kb["n_clamped"]


@pytest.mark.parametrize("N", [5, 130])
def test_one_zero_simulation_is_kriging_believer_to_the_bit(N):
    """what the two strategies share (the R row, the rank-1 step, the block arg-max and its partials), at the smallest
    shapes that reach every part: N one below and one above the pass's 128-row split, M = 300 = two update blocks (the
    second partial), pending points before the selections.  With S = 1 and eps = 0 the mean of one number is that
    number, so unlike test_zero_eps_is_kriging_believer the values are equal to the bit too.  No ties: the candidates
    are distinct uniform draws."""
    L = __import__("turbo_amd")._lib
    X, y, ls, Xc, Xp = _problem(N, 3, "rbf", 1e-4, 300, 40 + N)
    gp = _gp("f64", X, y, "rbf", ls, 1e-4, Xc)
    for acq, sf, par in ((L.ACQ_EI, -1.0, 0.01), (L.ACQ_PI, 1.0, 0.0), (L.ACQ_UCB, 1.0, 2.0)):
        inc = float(y.min() if sf < 0 else y.max())
        kb = gp.sweep_batch(3, L.BATCH_KB, 0.0, Xp[:2], acq, sf, inc, par, want_posterior=True)
        res = gp.sweep_batch_mc(3, 1, 0, np.zeros((1, 5)), Xp[:2], acq, sf, inc, par, want_sigma=True)
        np.testing.assert_array_equal(res["idx"], kb["idx"])
        np.testing.assert_array_equal(res["x"], kb["x"])
        assert res["sigma"].tobytes() == kb["sigma"].tobytes()
        assert res["n_clamped"] == kb["n_clamped"]
        assert np.asarray(res["val"], dtype=np.float64).tobytes() == np.asarray(kb["val"], dtype=np.float64).tobytes()


CASES = [
    # N, D, kind, noise, M, dtype, pending, acq, sf, S, q
    (32, 2, "matern52", 1e-4, 10000, "f64", False, "ei", -1.0, 1, 8),
    (32, 2, "matern12", 1e-4, 10000, "f64", True, "pi", -1.0, 16, 8),
    (100, 3, "matern32", 1e-4, 8192, "f64", True, "ucb", -1.0, 5, 8),
    (200, 4, "rbf", 1e-3, 8192, "f64", True, "ucb", 1.0, 64, 8),
    (200, 4, "rbf", 0.0, 8192, "f64", False, "pi", 1.0, 5, 8),           # noise-free: jitter only
    (512, 8, "rbf", 1e-4, 8192, "f64", True, "ei", 1.0, 16, 8),
    (512, 8, "matern32", 1e-4, 8192, "f64", False, "ei", -1.0, 64, 8),
    (2048, 16, "matern52", 1e-4, 16384, "f64", True, "ei", -1.0, 5, 8),
    (2048, 16, "matern12", 1e-4, 16384, "f64", False, "ucb", 1.0, 16, 8),
    (300, 5, "matern52", 1e-3, 4096, "f64", True, "ei", -1.0, 64, 60),   # P + q = 64
    (4096, 32, "rbf", 1e-2, 65536, "f32", True, "ei", -1.0, 16, 8),      # C3-shaped: only the first sweep is f32
]


@pytest.mark.parametrize("case", CASES, ids=["-".join(str(v) for v in c) for c in CASES])
def test_parity_with_the_reference_under_teacher_forcing(case):
    """bars: the project's own from tests/test_gpu_batch.py (f64 regret <= 1e-9, val rtol 1e-9 / atol 1e-12; f32 handle
    regret <= 1e-3, val rtol 1e-2); f64 also acq_out within 1e-9 x the step's best on every unmasked row and
    fantasy_out at rtol 1e-9.  eps is taken from eps_out, so the reference sees the numbers the GPU used."""
    import turbo_amd as ta
    L = ta._lib
    N, D, kind, noise, M, dtype, pend, acq_name, sf, S, q = case
    X, y, ls, Xc, Xp = _problem(N, D, kind, noise, M, 7 + N, ard=(kind == "matern52"), ls_scale=1.0 if noise > 0 else 0.4)
    jitter = 1e-10 if noise > 0 else 1e-8
    gp = _gp(dtype, X, y, kind, ls, noise, Xc, jitter)
    om = o.fit(X, y, kind, 1.0, ls, noise, jitter, True)
    Xp = Xp if pend else None
    P = 4 if pend else 0
    desired = "max" if sf > 0 else "min"
    inc = float(y.max() if sf > 0 else y.min())
    par = 2.0 if acq_name == "ucb" else 0.01
    f64 = dtype == "f64"
    res = gp.sweep_batch_mc(q, S, 1234 + N, None, Xp, ACQS[acq_name], sf, inc, par, want_acq=True, want_sigma=True)
    idx, eps = res["idx"], res["eps"]
    assert eps.shape == (S, P + q)
    assert len(set(idx.tolist())) == q
    ref = mr.select_batch(om, Xc, q, eps, Xp, acq_name, desired, par, inc, forced=idx)
    assert not ref["not_pd"]
    worst_regret = worst_acq = 0.0
    for k in range(q):
        best, got = ref["best"][k], ref["acq"][k][idx[k]]
        regret = (best - got) / max(abs(best), 1e-300)
        worst_regret = max(worst_regret, regret)
        assert regret <= (1e-9 if f64 else REGRET_TOL), (k, best, got)
        np.testing.assert_allclose(res["val"][k], got, rtol=1e-9 if f64 else 1e-2, atol=1e-12 if f64 else 1e-6 * abs(best))
        if f64 or k > 0 or P > 0:     # (an f32 handle's first sweep gives row 0 in f32 when nothing is pending)
            a_ref, a_got = ref["acq"][k], res["acq"][k]
            live = np.isfinite(a_ref)
            assert np.all(np.isneginf(a_got[idx[:k]]))
            scale = np.abs(a_ref[live]).max()
            err = np.abs(a_got[live] - a_ref[live]).max() / scale
            worst_acq = max(worst_acq, err)
            if f64:
                assert err <= 1e-9, (k, err)
    print("worst regret %.3g, worst |acq_out - reference| / step's best %.3g" % (worst_regret, worst_acq))
    np.testing.assert_array_equal(res["x"], Xc[idx])
    # (fantasy_out: f64 at the issue's rtol 1e-9.  The f32 handle's fantasy bar and the sigma bars below are not this
    # feature's own: they are the ones tests/test_gpu_batch.py applies to tgp_sweep_batch's fantasies and sigma^2 --
    # the variance update is that call's, and only the first sweep of an f32 handle is f32)
    np.testing.assert_allclose(res["fantasies"], ref["fantasies"], rtol=1e-9 if f64 else 1e-6, atol=1e-12)
    s_y = om.y_std
    if f64:
        np.testing.assert_allclose(res["sigma"] ** 2, ref["sigma"] ** 2, rtol=1e-5, atol=1e-9 * (1.0 + noise) * s_y ** 2)
    else:
        assert np.max(np.abs(res["sigma"] ** 2 - ref["sigma"] ** 2)) <= 5e-5 * (1.0 + noise) * s_y ** 2


def test_philox_normals_and_their_layout():
    L = __import__("turbo_amd")._lib
    X, y, ls, Xc, Xp = _problem(64, 3, "rbf", 1e-4, 2000, 5)
    gp = _gp("f64", X, y, "rbf", ls, 1e-4, Xc)
    for seed in (0, 1, 2**64 - 1, 0x9E3779B97F4A7C15):
        res = gp.sweep_batch_mc(5, 64, seed, None, Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01)
        np.testing.assert_allclose(res["eps"], mr.normals(seed, 64, 9), rtol=0, atol=1e-14)
    # simulation s does not depend on S; the draw for point j not on q
    a = gp.sweep_batch_mc(1, 4, 77, None, Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01)
    b = gp.sweep_batch_mc(1, 64, 77, None, Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01)
    assert a["eps"].tobytes() == b["eps"][:4].copy().tobytes()
    assert a["fantasies"].tobytes() == b["fantasies"][:4].copy().tobytes()
    c = gp.sweep_batch_mc(3, 4, 77, None, Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01)
    assert c["eps"][:, :5].copy().tobytes() == a["eps"].tobytes()
    # eps_in is used as it is and handed back
    e = np.random.RandomState(1).normal(size=(6, 7))
    d = gp.sweep_batch_mc(3, 6, 0, e, Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01)
    assert d["eps"].tobytes() == e.tobytes()


def test_sigma_acquisition_returns_kriging_believers_indices_whatever_eps_is():
    L = __import__("turbo_amd")._lib
    for N in (32, 300):
        X, y, ls, Xc, Xp = _problem(N, 4, "matern52", 1e-4, 5000, 13 + N, ard=True)
        gp = _gp("f64", X, y, "matern52", ls, 1e-4, Xc)
        kb = gp.sweep_batch(7, L.BATCH_KB, 0.0, Xp, L.ACQ_SIGMA, 1.0, 0.0, 0.0)
        for seed, S in ((1, 1), (2, 16), (3, 64)):
            res = gp.sweep_batch_mc(7, S, seed, None, Xp, L.ACQ_SIGMA, 1.0, 0.0, 0.0)
            np.testing.assert_array_equal(res["idx"], kb["idx"])
            assert res["val"].tobytes() == kb["val"].tobytes()


def test_the_handle_is_left_untouched():
    import turbo_amd as ta
    L = ta._lib
    for N in (32, 300, 1024):
        X, y, ls, Xc, Xp = _problem(N, 5, "rbf", 1e-4, 5000, 3 + N)
        gp = _gp("f64", X, y, "rbf", ls, 1e-4, Xc)
        before = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)
        gp.sweep_batch_mc(6, 16, 5, None, Xp, L.ACQ_EI, -1.0, float(y.min()), 0.01, want_acq=True, want_sigma=True)
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
        gp.sweep_batch_mc(2, 8, 1, None, X[:1], L.ACQ_EI, -1.0, float(y.min()), 0.01)
    assert "positive definite" in str(ei.value)
    assert gp.lib.tgp_sweep_batch_mc(gp._h, 2, 8, 1, None, X[:1].ctypes.data_as(L._dp), 1, L.ACQ_EI, -1.0, 0.0, 0.01,
                                     np.zeros(2, dtype=np.int64).ctypes.data_as(L._i64p), np.zeros(2).ctypes.data_as(L._dp),
                                     None, None, None, None, None, None) == L.NOT_PD
    assert gp._h is not None
    gp2 = _gp("f64", X, y, "rbf", ls, 1e-4, Xc)
    idx = np.zeros(64, dtype=np.int64)
    val = np.zeros(64)
    ip, vp = idx.ctypes.data_as(L._i64p), val.ctypes.data_as(L._dp)
    Xp = np.zeros((64, 3))
    xp = Xp.ctypes.data_as(L._dp)
    nul = None

    def code(q, S, eps, xp_, P, acq):
        return gp2.lib.tgp_sweep_batch_mc(gp2._h, q, S, 1, eps, xp_, P, acq, 1.0, 0.0, 0.0, ip, vp, nul, nul, nul, nul, nul,
                                          ctypes.POINTER(ctypes.c_int64)())
    assert code(2, 0, nul, nul, 0, L.ACQ_EI) == L.BAD_ARG
    assert code(2, 65, nul, nul, 0, L.ACQ_EI) == L.BAD_ARG
    assert code(0, 4, nul, nul, 0, L.ACQ_EI) == L.BAD_ARG
    assert code(5, 4, nul, xp, 60, L.ACQ_EI) == L.BAD_ARG          # P + q = 65
    assert code(2, 4, nul, nul, 0, L.ACQ_NONE) == L.BAD_ARG
    for bad in (np.nan, np.inf):
        e = np.zeros((4, 2))
        e[3, 1] = bad
        assert code(2, 4, e.ctypes.data_as(L._dp), nul, 0, L.ACQ_EI) == L.BAD_ARG
    assert code(2, 4, nul, nul, 0, L.ACQ_EI) == L.OK
    # the handle still serves ordinary calls after the refusals
    r = gp2.sweep(L.ACQ_EI, 1.0, 0.0, 0.0)
    assert 0 <= r["best_idx"] < 500


def test_select_batch_monte_carlo_end_to_end_on_branin():
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
    xs, info = opt.select_batch(lb, acq, 4, strategy='monte_carlo', pending=X[:2] + 0.01, n_sim=8, seed=42)
    # the RNG consumed as by one __call__ -- with a seed GIVEN; seed=None takes one more np.random.randint after the
    # candidates, as TS takes its seed (checked at the end of this test)
    assert np.array_equal(np.random.get_state()[1], state_after_call)
    assert xs.shape == (4, 2)
    assert len({tuple(r) for r in xs}) == 4
    for d, (lo, hi) in enumerate(bounds):
        assert np.all(xs[:, d] >= lo) and np.all(xs[:, d] <= hi)
    assert set(info) >= {'max_acq', 'candidate_indices', 'fantasies', 'pending_fantasies', 'strategy', 'n_sim', 'seed'}
    assert info['strategy'] == 'monte_carlo' and info['n_sim'] == 8 and info['seed'] == 42
    assert info['fantasies'].shape == (8, 4) and info['pending_fantasies'].shape == (8, 2)
    # the same seed gives the same batch; another seed other fantasies
    np.random.seed(123)
    xs2, info2 = opt.select_batch(lb, acq, 4, strategy='monte_carlo', pending=X[:2] + 0.01, n_sim=8, seed=42)
    np.testing.assert_array_equal(xs, xs2)
    assert info2['fantasies'].tobytes() == info['fantasies'].tobytes()
    np.random.seed(123)
    _, info3 = opt.select_batch(lb, acq, 4, strategy='monte_carlo', pending=X[:2] + 0.01, n_sim=8, seed=43)
    assert not np.array_equal(info3['pending_fantasies'], info['pending_fantasies'])
    # without pending points the first pick is __call__'s winner
    np.random.seed(123)
    xk, infok = opt.select_batch(lb, acq, 3, strategy='monte_carlo', n_sim=16, seed=1)
    np.testing.assert_array_equal(xk[0], np.asarray(x1).reshape(-1))
    assert infok['max_acq'][0] == info1['max_acq']
    # one simulation with a pending point runs; seed=None takes its seed from NumPy's RNG, as TS does
    np.random.seed(5)
    xa, infoa = opt.select_batch(lb, acq, 2, strategy='monte_carlo', pending=X[:1] + 0.01, n_sim=1)
    assert xa.shape == (2, 2) and infoa['fantasies'].shape == (1, 2) and 0 <= infoa['seed'] < 2**63
    state_none = np.random.get_state()[1].copy()
    np.random.seed(5)
    xb, infob = opt.select_batch(lb, acq, 2, strategy='monte_carlo', pending=X[:1] + 0.01, n_sim=1)
    assert infob['seed'] == infoa['seed']
    np.testing.assert_array_equal(xa, xb)
    np.random.seed(5)
    opt(lb, acq)
    want_seed = int(np.random.randint(0, 2**63))            # the draw that follows the candidates'
    assert infoa['seed'] == want_seed
    assert np.array_equal(np.random.get_state()[1], state_none)
    # the other strategies take no notice of the new arguments
    np.random.seed(123)
    xc1, _ = opt.select_batch(lb, acq, 3)
    np.random.seed(123)
    xc2, _ = opt.select_batch(lb, acq, 3, n_sim=3, seed=9)
    np.testing.assert_array_equal(xc1, xc2)


def test_select_batch_monte_carlo_with_candidates_drawn_on_the_device():
    """device_rng_seed keys the CANDIDATES (seed + call number); the `seed` argument keys the fantasies and reaches the
    library unchanged: info['seed'] is the one asked for, two seeds give the same candidates' first pick but different
    fantasies, the same seed the same batch, and seed=None takes its seed from NumPy's RNG"""
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
    pend = X[:2] + 0.01
    for design in ('uniform', 'lhs'):
        def run(seed):
            opt = CandidateSweep(num_random=2000, device_rng_seed=7, device_design=design)     # call 0: the same candidates
            return opt.select_batch(lb, acq, 4, strategy='monte_carlo', pending=pend, n_sim=8, seed=seed)
        xa, ia = run(42)
        xb, ib = run(42)
        xc, ic = run(43)
        assert ia['seed'] == 42 and ic['seed'] == 43 and ia['n_sim'] == 8
        np.testing.assert_array_equal(xa, xb)
        assert ia['fantasies'].tobytes() == ib['fantasies'].tobytes()
        assert not np.array_equal(ia['pending_fantasies'], ic['pending_fantasies'])
        # the normals are the reference's for the seed asked for, and the plugin's call is the library's with that seed
        eps = mr.normals(42, 8, 6)
        assert ia['fantasies'].shape == (8, 4) and ia['pending_fantasies'].shape == (8, 2)
        ctx = model._ensure_resident()
        direct = ctx.sweep_batch_mc(4, 8, 42, None, pend, ta._lib.ACQ_EI, -1.0, float(y.min()), 0.01)
        np.testing.assert_allclose(direct['eps'], eps, rtol=0, atol=1e-14)
        assert direct['fantasies'].tobytes() == np.column_stack([ia['pending_fantasies'], ia['fantasies']]).tobytes()
        assert len({tuple(r) for r in xa}) == 4
        for d, (lo, hi) in enumerate(bounds):
            assert np.all(xa[:, d] >= lo) and np.all(xa[:, d] <= hi)
        # seed=None: one np.random.randint(0, 2**63), as TS; the candidates do not touch NumPy's RNG on this path
        np.random.seed(11)
        _, inone = run(None)
        np.random.seed(11)
        assert inone['seed'] == int(np.random.randint(0, 2**63))
