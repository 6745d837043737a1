"""GPU: learned input warping in the C-ABI (csrc/warp_kernels.hip, csrc/api_warp.hpp).
 (a) tgp_warp_points on the device against mpmath on the grid of tests/warp_reference.py, at 64 max(e_ref, u) -- absolute for
     w, relative to max(|value|, the smallest normal) for the derivatives -- e_ref from tests/golden/warp_eref.json; exact
     endpoints and identity; the inverse brings the points back;
 (b) tgp_warp_candidates at M in {1, 255, 256, 257, 70 001} x D in {1, 3, 33}: the rows are tgp_warp_points' bytes, the raw
     rows come back unchanged, a borrowed buffer is unchanged, a re-warp with new shapes equals a fresh warp, a new
     tgp_set_candidates drops both buffers, tgp_sweep behind the warp returns the bytes of tgp_sweep over the uploaded warped
     rows (and the winner is the warped row);
 (c) tgp_fit_warp_grad is the composition of tgp_warp_points and tgp_fit_input_grad to the byte, and its 2 D warp entries are
     held to the 80-bit chain rule of tests/warp_grad_cases.py (which tests/test_warp_grad_reference.py holds to central
     differences of the 80-bit LML) at min(64 max(e_ref, N u), 1e-9) of the entry's scale -- on an identity warp too;
 (d) tgp_fit_warp_lbfgsb against SciPy's L-BFGS-B driving fit_warp_grad from Python on the same starts, by the three criteria
     of test_the_default_hyper_parameter_fit_walks_what_scipy_walks; with every warp entry fixed at 0 it returns what
     tgp_fit_lbfgsb returns on tgp_warp_points' identity output; the prior enters the objective;
 (e) the argument checks answer TGP_BAD_ARG, host handles refuse the GPU-only entries.

Every comparison prints its figures before it asserts."""
import faulthandler
import json
import os

import numpy as np
import pytest

import warp_grad_cases as wc
import warp_reference as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def gp():
    import turbo_amd as ta
    return ta.NativeGP(0, "f64")


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def test_warp_points_on_the_device_against_mpmath(gp):
    g = np.array(wr.GRID, dtype=np.float64)
    u, a, b = g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()
    n = len(u)
    # one row of len(GRID) dimensions, each with its own shapes, in the unit box
    got = gp.warp_points(u[None, :], np.zeros(n), np.ones(n), a, b, derivatives=True)
    with open(os.path.join(ROOT, "tests", "golden", "warp_eref.json")) as f:
        rec = json.load(f)["e_ref"]
    worst = dict.fromkeys(rec, 0.0)
    for k in range(n):
        for key, e in zip(("w", "dw_du", "dw_da", "dw_db"), wr.errors(u[k], a[k], b[k], [x[0, k] for x in got])):
            worst[key] = max(worst[key], e)
    for key in worst:
        bar = 64 * max(rec[key], wr.U)
        print("%s: device %.3g (bar %.3g, e_ref %.3g)" % (key, worst[key], bar, rec[key]))
    for key in worst:
        assert worst[key] <= 64 * max(rec[key], wr.U), (key, worst[key])
    w = got[0][0]
    assert np.all(w[u == 0] == 0) and not np.any(np.signbit(w[u == 0])) and np.all(w[u == 1] == 1)
    ident = (a == 1) & (b == 1)
    assert w[ident].tobytes() == u[ident].tobytes()
    assert gp.warp_points(u[None, :], np.zeros(n), np.ones(n), a, b).tobytes() == got[0].tobytes()
    back = gp.warp_inverse(got[0], np.zeros(n), np.ones(n), a, b)[0]
    w2 = gp.warp_points(back[None, :], np.zeros(n), np.ones(n), a, b, derivatives=True)
    with np.errstate(invalid="ignore"):
        slope = np.where(np.isfinite(w2[1][0]), w2[1][0] * back, 1.0)
    assert np.all(np.abs(w2[0][0] - w) <= 64 * wr.U * np.maximum(1.0, slope))     # (the bar of tests/test_warp_reference.py's round trip)


# ---- (b) ----------------------------------------------------------------------------------------------------------------
def _small_model(gp, D):
    rng = np.random.RandomState(D)
    X = rng.uniform(0, 1, (24, D))
    y = np.sin(3 * X.sum(axis=1))
    gp.fit(X, y, "matern52", 1.0, 0.7 * np.sqrt(D), 1e-3, 1e-10, True)


@pytest.mark.parametrize("D", [1, 3, 33])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 70001])
def test_the_batch_warp(M, D):
    import turbo_amd as ta
    from turbo_amd import _lib
    gp = ta.NativeGP(0, "f64")
    _small_model(gp, D)
    rng = np.random.RandomState(1000 * D + M % 997)
    lo, hi = -1.0 - 0.1 * np.arange(D), 2.0 + 0.05 * np.arange(D)
    Xc = rng.uniform(-1.2, 2.2, (M, D))                         # (some rows outside the box: clipped)
    Xc[0, 0], Xc[-1, -1] = lo[0], hi[-1]
    a, b = rng.uniform(0.3, 3.0, D), rng.uniform(0.3, 3.0, D)
    a2, b2 = rng.uniform(0.3, 3.0, D), rng.uniform(0.3, 3.0, D)
    want, want2 = gp.warp_points(Xc, lo, hi, a, b), gp.warp_points(Xc, lo, hi, a2, b2)
    gp.set_candidates(Xc)
    gp.warp_candidates(lo, hi, a, b)
    assert gp.read_candidates().tobytes() == want.tobytes()
    assert gp.warp_read_raw().tobytes() == Xc.tobytes()
    assert gp.get_candidate(M - 1).tobytes() == want[M - 1].tobytes()
    if M > 1:
        assert gp.warp_read_raw(M - 1, 1).tobytes() == Xc[M - 1:].tobytes()
    s_warp = gp.sweep(_lib.ACQ_EI, -1.0, 0.0, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    gp.warp_candidates(lo, hi, a2, b2)                           # a re-warp: from the raw rows
    assert gp.read_candidates().tobytes() == want2.tobytes() and gp.warp_read_raw().tobytes() == Xc.tobytes()
    gp.set_candidates(want)                                      # a new batch drops both
    with pytest.raises(ValueError):
        gp.warp_read_raw()
    assert gp.read_candidates().tobytes() == want.tobytes()
    s_up = gp.sweep(_lib.ACQ_EI, -1.0, 0.0, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    for key in ("mu", "sigma", "acq"):
        assert s_warp[key].tobytes() == s_up[key].tobytes(), key
    assert (s_warp["best_idx"], s_warp["best_val"], s_warp["n_clamped"]) == (s_up["best_idx"], s_up["best_val"], s_up["n_clamped"])
    gp.close()


def test_a_borrowed_buffer_is_never_written_to():
    torch = pytest.importorskip("torch")
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    D, M = 3, 4099
    _small_model(gp, D)
    Xc = np.random.RandomState(5).uniform(0, 1, (M, D))
    t = torch.from_numpy(Xc).to("cuda:0")
    gp.set_candidates_dev(t.data_ptr(), M, keepalive=t)
    gp.warp_candidates(np.zeros(D), np.ones(D), 2.0, 0.5)
    gp.warp_candidates(np.zeros(D), np.ones(D), 0.5, 2.0)
    torch.cuda.synchronize()
    assert t.cpu().numpy().tobytes() == Xc.tobytes()
    assert gp.warp_read_raw().tobytes() == Xc.tobytes()
    assert gp.read_candidates().tobytes() == gp.warp_points(Xc, np.zeros(D), np.ones(D), 0.5, 2.0).tobytes()
    gp.close()


def test_a_generated_batch_is_warped_where_it_is(gp):
    D, M = 3, 5000
    _small_model(gp, D)
    lo, hi = np.full(D, -2.0), np.full(D, 3.0)
    gp.generate(11, 0, M, lo, hi)
    raw = gp.read_candidates()
    gp.warp_candidates(lo, hi, [0.5, 1.0, 2.0], [1.0, 1.0, 0.7])
    assert gp.warp_read_raw().tobytes() == raw.tobytes()
    assert gp.read_candidates().tobytes() == gp.warp_points(raw, lo, hi, [0.5, 1.0, 2.0], [1.0, 1.0, 0.7]).tobytes()


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(wc.CASES))
def test_fit_warp_grad_is_the_composition_and_its_warp_entries_hold(case, gp):
    X, y, lo, hi, a, b, ls = wc.data(case)
    D = len(a)
    Wx = gp.warp_points(X, lo, hi, a, b)
    args = wc.fit_args(case, Wx)
    l1, g1, dX = gp.fit_input_grad(*args)
    l2, g2 = gp.fit_warp_grad(X, *args[1:], lo, hi, a, b)
    assert np.float64(l1).tobytes() == np.float64(l2).tobytes() and g1.tobytes() == g2[:2 + D].tobytes()
    assert gp.fit_warp_grad(X, *args[1:], lo, hi, a, b)[1].tobytes() == g2.tobytes()
    val, sc = wc.reference(case, Wx)
    e_ref = wc.e_ref_recorded(case)
    bar = wc.bar(case, e_ref)
    err = wc.fractions(g2[2 + D:], val, sc)
    print("%s: worst warp entry %.3g of its scale (bar %.3g, e_ref %.3g); entries %s" % (case, err.max(), bar, e_ref, np.array2string(g2[2 + D:], precision=4)))
    assert np.all(np.isfinite(g2)) and err.max() <= bar, (case, err)
    if case == "identity":
        assert np.all(g2[2 + D:] != 0) and Wx.tobytes() == ((X - lo) / (hi - lo)).tobytes()
    # the handle is left fitted on w(X): it sweeps a warped batch
    gp.set_candidates(Wx[:5])
    mu = gp.sweep(want_mu=True)["mu"]
    assert np.all(np.isfinite(mu))


# ---- (d) ----------------------------------------------------------------------------------------------------------------
def _warp_problem(N, D):
    rng = np.random.RandomState(N + D)
    lo, hi = np.zeros(D), np.ones(D)
    X = rng.uniform(0, 1, (N, D))
    T = wr.warp_f64(X, np.array([3.0, 1.0, 0.6][:D])[None, :], np.array([1.0, 0.4, 1.5][:D])[None, :])[0]
    y = np.sin(6 * T[:, 0]) + (T[:, 1:] ** 2).sum(axis=1) + 0.02 * rng.standard_normal(N)
    P0 = 2 + D
    theta0 = np.concatenate([np.log([1.0]), np.log(np.full(D, 0.5)), np.log([1e-2]), np.zeros(2 * D)])
    bounds = np.array([[np.log(1e-3), np.log(1e3)]] + [[np.log(1e-2), np.log(1e2)]] * D + [[np.log(1e-6), np.log(1e1)]] + [[np.log(0.25), np.log(4.0)]] * (2 * D))
    return X, y, lo, hi, theta0, bounds, P0


@pytest.mark.parametrize("N,D", [(30, 2), (200, 3)])
def test_fit_warp_lbfgsb_walks_what_scipy_walks(N, D, gp):
    import scipy.optimize
    X, y, lo, hi, theta0, bounds, P0 = _warp_problem(N, D)
    sigma = 0.5
    evals = [0]

    def objective(th):
        evals[0] += 1
        try:
            lml, grad = gp.fit_warp_grad(X, y, "matern52", np.exp(th[0]), np.exp(th[1:1 + D]), np.exp(th[1 + D]), 1e-10, True, lo, hi,
                                         np.exp(th[P0:P0 + D]), np.exp(th[P0 + D:]))
        except np.linalg.LinAlgError:
            return np.inf, np.zeros_like(th)
        wpart = th[P0:]
        f = -lml + 0.5 * (wpart ** 2).sum() / sigma ** 2
        g = -grad
        g[P0:] += wpart / sigma ** 2
        return f, g
    ref = scipy.optimize.minimize(objective, theta0, method="L-BFGS-B", jac=True, bounds=bounds)
    theta, f, st, ev = gp.fit_warp_optimise(X, y, "matern52", lo, hi, theta0, D, bounds, 1e-10, True, prior_sigma=sigma, max_iter=15000)
    print("N %d D %d: SciPy f %.10g in %d evaluations, library f %.10g in %d (status %d); theta %s vs %s" % (N, D, ref.fun, evals[0], f[0], ev, st[0], np.array2string(theta[0], precision=4), np.array2string(ref.x, precision=4)))
    assert 0.6 * evals[0] - 10 <= ev <= 1.5 * evals[0] + 25, (ev, evals[0])
    assert abs(f[0] - ref.fun) <= 1e-8 * max(1.0, abs(ref.fun)), (f[0], ref.fun)
    np.testing.assert_allclose(theta[0], ref.x, atol=5e-3)
    # f_out is the minimised objective: -LML plus the prior's term at theta_out
    t = theta[0]
    lml, _ = gp.fit_warp_grad(X, y, "matern52", np.exp(t[0]), np.exp(t[1:1 + D]), np.exp(t[1 + D]), 1e-10, True, lo, hi, np.exp(t[P0:P0 + D]), np.exp(t[P0 + D:]))
    assert abs(f[0] - (-lml + 0.5 * (t[P0:] ** 2).sum() / sigma ** 2)) <= 1e-12 * max(1.0, abs(f[0]))
    assert np.any(np.abs(t[P0:]) > 0.05)                         # (the warp moved: the data are warped)


def test_fit_warp_lbfgsb_with_the_warp_fixed_is_fit_lbfgsb_on_the_identity_output(gp):
    N, D = 200, 3
    X, y, lo, hi, theta0, bounds, P0 = _warp_problem(N, D)
    lo, hi = lo - 1.0, hi + 2.0
    Xr = lo + X * (hi - lo)
    bounds = bounds.copy()
    bounds[P0:] = 0.0                                            # every warp entry fixed at log 1
    starts = np.stack([theta0, theta0 + np.concatenate([[0.3], np.full(D, -0.4), [1.0], np.zeros(2 * D)])])
    theta, f, st, ev = gp.fit_warp_optimise(Xr, y, "matern52", lo, hi, starts, D, bounds, 1e-10, True, prior_sigma=0.5)
    Wx = gp.warp_points(Xr, lo, hi, 1.0, 1.0)
    t_ref, f_ref, st_ref, ev_ref = gp.fit_optimise(Wx, y, "matern52", starts[:, :P0], D, bounds[:P0], 1e-10, True, lbfgsb=True)
    assert theta[:, :P0].tobytes() == t_ref.tobytes() and np.all(theta[:, P0:] == 0)
    assert f.tobytes() == f_ref.tobytes() and ev == ev_ref and np.array_equal(st, st_ref)


# ---- (e) ----------------------------------------------------------------------------------------------------------------
def test_the_argument_checks(gp):
    import turbo_amd as ta
    D = 2
    X = np.random.RandomState(0).uniform(0, 1, (20, D))
    y = X.sum(axis=1)
    lo, hi = np.zeros(D), np.ones(D)
    for bad in (dict(hi=np.zeros(D)), dict(a=[1.0, 0.0]), dict(b=[np.nan, 1.0]), dict(a=[np.inf, 1.0]), dict(lo=[0.0, -np.inf])):
        kw = dict(lo=lo, hi=hi, a=np.ones(D), b=np.ones(D))
        kw.update(bad)
        with pytest.raises(ValueError):
            gp.warp_points(X, kw["lo"], kw["hi"], kw["a"], kw["b"])
        with pytest.raises(ValueError):
            gp.warp_inverse(X, kw["lo"], kw["hi"], kw["a"], kw["b"])
        with pytest.raises(ValueError):
            gp.fit_warp_grad(X, y, "rbf", 1.0, 0.5, 1e-3, 1e-10, True, kw["lo"], kw["hi"], kw["a"], kw["b"])
    fresh = ta.NativeGP(0, "f64")
    fresh.D, fresh.M = D, 0
    with pytest.raises(ValueError):
        fresh.warp_candidates(lo, hi, 1.0, 1.0)                  # no resident batch
    with pytest.raises(ValueError):
        fresh.warp_read_raw(0, 1)
    fresh.fit(X, y, "rbf", 1.0, 0.5, 1e-3, 1e-10, True)
    fresh.set_candidates(X)
    with pytest.raises(ValueError):
        fresh.warp_candidates(lo, lo, 1.0, 1.0)
    with pytest.raises(ValueError):
        fresh.warp_read_raw()                                    # a refused warp leaves the batch as it was
    assert fresh.read_candidates().tobytes() == X.tobytes()
    fresh.warp_candidates(lo, hi, 2.0, 2.0)
    with pytest.raises(ValueError):
        fresh.warp_read_raw(5, 100)
    theta0 = np.zeros(2 + 1 + 2 * D)
    bounds = np.array([[-3.0, 3.0]] * len(theta0))
    with pytest.raises(ValueError):
        fresh.fit_warp_optimise(X, y, "rbf", lo, lo, theta0, 1, bounds, 1e-10, True)
    with pytest.raises(ValueError):
        fresh.fit_warp_optimise(X, y, "rbf", lo, hi, theta0, 1, bounds, 1e-10, True, prior_sigma=-1.0)
    bad_bounds = bounds.copy()
    bad_bounds[-1] = [1.0, -1.0]
    with pytest.raises(ValueError):
        fresh.fit_warp_optimise(X, y, "rbf", lo, hi, theta0, 1, bad_bounds, 1e-10, True)
    fresh.close()
    host = ta.NativeGP(ta._lib.DEVICE_HOST)
    host.D, host.M = D, 0
    assert host.warp_points(X, lo, hi, 2.0, 0.5).shape == X.shape          # the host serves the warp itself ...
    for call in (lambda: host.warp_candidates(lo, hi, 1.0, 1.0), lambda: host.warp_read_raw(0, 1),
                 lambda: host.fit_warp_grad(X, y, "rbf", 1.0, 0.5, 1e-3, 1e-10, True, lo, hi, 1.0, 1.0),
                 lambda: host.fit_warp_optimise(X, y, "rbf", lo, hi, theta0, 1, bounds, 1e-10, True)):
        with pytest.raises(ValueError):                                     # ... and refuses what needs the GPU
            call()
