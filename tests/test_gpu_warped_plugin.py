"""GPU: learned input warping through the plugin layer (turbo_amd/warped.py).
 (a) recovery: y = sin(6 t0) + t1^2 with t = w_true(x), a_true = (3, 1), b_true = (1, 0.4), N = 60 -- the fitted warped
     model's LML exceeds the unwarped optimum's and its RMSE on 2000 held-out points is below the unwarped model's, both
     against HipGPSurrogate on the same data and seeds; optimizer='scipy' reaches the library's optimum;
     training_iterations=0 keeps the current warp;
 (b) WarpedHipGPSurrogate -> EI -> CandidateSweep(num_random=4096, device_rng_seed=...) over five trials: the chosen x is a
     drawn candidate bit for bit; RandomAndQuasiNewton over five trials: refined points lie inside the raw box; the value
     reported is the acquisition at the chosen raw point; value_and_grad is the gradient in raw coordinates (its own test);
 (c) the refused entries raise."""
import faulthandler
import warnings

import numpy as np
import pytest

import warp_reference as wr

pytestmark = pytest.mark.gpu
A_TRUE, B_TRUE = np.array([3.0, 1.0]), np.array([1.0, 0.4])
LO, HI = np.array([-2.0, 1.0]), np.array([2.0, 3.0])


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _objective(X):
    t = wr.warp_f64(np.clip((X - LO) / (HI - LO), 0.0, 1.0), A_TRUE[None, :], B_TRUE[None, :])[0]
    return np.sin(6 * t[:, 0]) + t[:, 1] ** 2


def _bounds(ta):
    return ta.Bounds([("x0", LO[0], HI[0]), ("x1", LO[1], HI[1])])


def _params(ta, optimizer="fmin_l_bfgs_b"):
    return dict(kernel=ta.GPKernel("matern52", 1.0, np.array([0.5, 0.5]), 1e-2), normalize_y=True, random_state=0, optimizer=optimizer)


def _quiet(fn, *args):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*args)


def test_the_warp_is_recovered_against_the_unwarped_surrogate():
    import turbo_amd as ta
    rng = np.random.RandomState(60)
    X, Xt = rng.uniform(LO, HI, (60, 2)), rng.uniform(LO, HI, (2000, 2))
    y, yt = _objective(X), _objective(Xt)
    out = {}
    for name, make in (("plain", lambda: ta.HipGPSurrogate(model_params=_params(ta), training_iterations=3, param_continuity=False)),
                       ("warped", lambda: ta.WarpedHipGPSurrogate(_bounds(ta), model_params=_params(ta), training_iterations=3, param_continuity=False)),
                       ("warped-scipy", lambda: ta.WarpedHipGPSurrogate(_bounds(ta), model_params=_params(ta, "scipy"), training_iterations=3, param_continuity=False))):
        sur = make()
        model, info = _quiet(sur.construct_model, 0, X, y)
        rmse = float(np.sqrt(np.mean((_quiet(model.predict, Xt) - yt) ** 2)))
        out[name] = (model.get_log_likelihood(), rmse, info)
        print("%s: LML %.6f, RMSE %.4g, %s evaluations%s" % (name, out[name][0], rmse, info.get("lml_evaluations"),
                                                             "" if name == "plain" else ", a %s b %s" % (info["warp_a"], info["warp_b"])))
        if name == "warped":      # training_iterations=0 keeps the current warp (param_continuity carries it on)
            keep = ta.WarpedHipGPSurrogate(_bounds(ta), model_params=_params(ta), training_iterations=0)
            keep.warp_a, keep.warp_b = info["warp_a"].copy(), info["warp_b"].copy()
            _, kept = _quiet(keep.construct_model, 0, X, y)
            assert np.array_equal(kept["warp_a"], info["warp_a"]) and np.array_equal(kept["warp_b"], info["warp_b"])
            keep.close()
        sur.close()
    assert out["warped"][0] > out["plain"][0], (out["warped"][0], out["plain"][0])
    assert out["warped"][1] < out["plain"][1], (out["warped"][1], out["plain"][1])
    # optimizer='scipy' drives the same objective from the same starts: the warp it ends at is the library's to the theta
    # criterion of test_the_default_hyper_parameter_fit_walks_what_scipy_walks (log entries within 5e-3)
    for key in ("warp_a", "warp_b"):
        np.testing.assert_allclose(np.log(out["warped-scipy"][2][key]), np.log(out["warped"][2][key]), atol=5e-3)


def _trials(ta, aux, n_trials=5, check=None):
    rng = np.random.RandomState(5)
    X = rng.uniform(LO, HI, (30, 2))
    y = _objective(X)
    sur = ta.WarpedHipGPSurrogate(_bounds(ta), model_params=_params(ta), training_iterations=2)
    for trial in range(n_trials):
        model, info = _quiet(sur.construct_model, trial, X, y)
        assert isinstance(model, ta.WarpedModel) and info["warp_a"].shape == (2,)
        acq, _ = ta.EI(0.01).construct_function(trial, model, "min", float(y.min()))
        x, ainfo = _quiet(aux, _bounds(ta), acq)
        assert x.shape == (1, 2) and np.all(x >= LO) and np.all(x <= HI)
        direct = float(np.asarray(acq(x)).reshape(-1)[0])
        print("trial %d: x %s, max_acq %.6g (direct %.6g), a %s b %s" % (trial, x, ainfo["max_acq"], direct, info["warp_a"], info["warp_b"]))
        assert abs(direct - ainfo["max_acq"]) <= 1e-9 * max(1.0, abs(direct))
        if check is not None:
            check(trial, x, model, acq)
        X, y = np.vstack([X, x]), np.append(y, _objective(x))
    sur.close()


def test_the_sweep_only_route_chooses_a_drawn_candidate_bit_for_bit():
    import turbo_amd as ta
    seed, M = 17, 4096
    ref = ta.NativeGP(0, "f64")
    ref.fit(np.zeros((2, 2)) + [[0.0], [1.0]], np.array([0.0, 1.0]), "rbf", 1.0, 1.0, 1e-2, 1e-10, True)    # (D for the generator)

    def check(trial, x, model, acq):
        ref.generate(seed + trial, 0, M, LO, HI)
        rows = ref.read_candidates()
        hit = np.nonzero((rows == x).all(axis=1))[0]
        assert len(hit) >= 1, (trial, x)
        vals = np.asarray(acq(rows))                       # the raw batch through the warped model, row by row
        assert int(np.argmax(vals)) == int(hit[0])
    _trials(ta, ta.CandidateSweep(num_random=M, device_rng_seed=seed), check=check)
    ref.close()


def test_value_and_grad_is_the_gradient_in_raw_coordinates():
    """against central differences of the acquisition in x, on a model with fixed hyper-parameters and a noise term (as
    tests/test_gpu_parity.py's test_acquisition_gradient_vs_finite_differences, and to its tolerances: a near-interpolating
    model's values carry too much rounding for a difference over 1e-6 of the box)"""
    import turbo_amd as ta
    rng = np.random.RandomState(9)
    X = rng.uniform(LO, HI, (40, 2))
    y = _objective(X) + 0.05 * rng.standard_normal(40)
    params = dict(kernel=ta.GPKernel("matern52", 1.6, np.array([0.5, 0.8]), 5e-3), optimizer=None, normalize_y=True)
    sur = ta.WarpedHipGPSurrogate(_bounds(ta), model_params=params, training_iterations=0)
    sur.warp_a, sur.warp_b = A_TRUE.copy(), B_TRUE.copy()
    model, info = _quiet(sur.construct_model, 0, X, y)
    assert np.array_equal(info["warp_a"], A_TRUE) and np.array_equal(info["warp_b"], B_TRUE)
    Xq = rng.uniform(LO + 0.05 * (HI - LO), HI - 0.05 * (HI - LO), (7, 2))
    for fac, args in ((ta.EI(0.01), [float(y.min())]), (ta.UCB(2.0), [])):
        f, _ = fac.construct_function(0, model, "min", *args)
        val, grad = f.value_and_grad(Xq)
        np.testing.assert_allclose(val, f(Xq), rtol=1e-9, atol=1e-13)
        fd = np.empty_like(grad)
        for d in range(2):
            e = np.zeros(2); e[d] = 1e-6 * (HI - LO)[d]
            fd[:, d] = (f(Xq + e) - f(Xq - e)) / (2 * e[d])
        scale = np.abs(fd).max() + 1e-12
        print("%s: gradient against differences, worst %.3g of %.3g" % (f.get_name(), np.abs(grad - fd).max(), scale))
        np.testing.assert_allclose(grad, fd, rtol=2e-4, atol=max(2e-6 * scale, 2e-9))
    sur.close()


def test_the_gradient_stage_stays_inside_the_raw_box():
    import turbo_amd as ta
    np.random.seed(3)
    _trials(ta, ta.RandomAndQuasiNewton(num_random=1000, grad_restarts=6, start_from_best=2))
    np.random.seed(4)
    _trials(ta, ta.RandomAndQuasiNewton(num_random=300, grad_restarts=3, start_from_best=1, lockstep="scipy"), n_trials=2)


def test_predict_many_is_the_per_model_predict():
    """several WarpedModels of one factory, each with its own warp (N <= 128 and 128 < N <= 256, the sizes the parent batches):
    predict_many returns every model's own predict, bit for bit -- and not the posterior of the unwarped model"""
    import turbo_amd as ta
    rng = np.random.RandomState(21)
    sur = ta.WarpedHipGPSurrogate(_bounds(ta), model_params=dict(kernel=ta.GPKernel("matern52", 1.3, np.array([0.3, 0.4]), 1e-3),
                                                                  optimizer=None, normalize_y=True), training_iterations=0)
    grid = rng.uniform(LO, HI, (300, 2))
    models = []
    for n, a, b in ((40, (3.0, 1.0), (1.0, 0.4)), (128, (0.5, 2.0), (2.0, 1.0)), (129, (1.0, 1.0), (1.0, 1.0)), (200, (2.5, 0.7), (0.6, 1.5)), (300, (3.0, 1.0), (1.0, 0.4))):
        X = rng.uniform(LO, HI, (n, 2))
        sur.warp_a, sur.warp_b = np.array(a), np.array(b)
        models.append(_quiet(sur.construct_model, len(models), X, _objective(X) + 0.01 * rng.standard_normal(n))[0])
    mus, sgs = _quiet(sur.predict_many, models, grid, True)
    assert mus.shape == sgs.shape == (len(models), 300)
    assert _quiet(sur.predict_many, models, grid).tobytes() == mus.tobytes()
    plain = ta.HipGPSurrogate(model_params=sur.model_params, training_iterations=0)
    for t, m in enumerate(models):
        mu, sg = _quiet(m.predict, grid, True)
        assert mus[t].tobytes() == mu.tobytes() and sgs[t].tobytes() == sg.tobytes(), t
        if not (np.all(m.warp_a == 1) and np.all(m.warp_b == 1)):     # ... which the unwarped model of the same rows is far from
            raw, _ = _quiet(plain.construct_model, t, m.X, m.y)
            assert np.abs(_quiet(raw.predict, grid) - mu).max() > 1e-3
    plain.close()
    sur.close()


def test_the_scipy_routes_get_a_finite_gradient_on_a_wall_of_infinite_slope():
    """a < 1 at lo and b < 1 at hi: dw/du is +inf there; value_and_grad, which SciPy's L-BFGS-B walks in raw coordinates, stays
    finite on the walls, and the SciPy gradient stage ends inside the box with a finite value"""
    import turbo_amd as ta
    rng = np.random.RandomState(31)
    X = rng.uniform(LO, HI, (40, 2))
    y = _objective(X) + 0.05 * rng.standard_normal(40)
    sur = ta.WarpedHipGPSurrogate(_bounds(ta), model_params=dict(kernel=ta.GPKernel("matern52", 1.6, np.array([0.5, 0.8]), 5e-3),
                                                                  optimizer=None, normalize_y=True), training_iterations=0)
    sur.warp_a, sur.warp_b = np.array([0.5, 0.6]), np.array([0.5, 0.7])
    model, _ = _quiet(sur.construct_model, 0, X, y)
    f, _ = ta.UCB(2.0).construct_function(0, model, "min")
    walls = np.array([[LO[0], LO[1]], [HI[0], HI[1]], [LO[0], 2.0], [0.5, HI[1]]])
    val, grad = f.value_and_grad(walls)
    print("on the walls: values %s, gradients %s" % (val, grad.tolist()))
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    np.random.seed(8)
    for lockstep in ("scipy", False):
        x, info = _quiet(ta.RandomAndQuasiNewton(num_random=200, grad_restarts=4, start_from_best=2, lockstep=lockstep), _bounds(ta), f)
        assert np.all(x >= LO) and np.all(x <= HI) and np.isfinite(info["max_acq"])
    sur.close()


def test_the_refused_entries_raise():
    import turbo_amd as ta
    rng = np.random.RandomState(5)
    X = rng.uniform(LO, HI, (30, 2))
    sur = ta.WarpedHipGPSurrogate(_bounds(ta), model_params=_params(ta), training_iterations=1)
    model, _ = _quiet(sur.construct_model, 0, X, _objective(X))
    for acq in (ta.TS(), ta.MES(), ta.KG()):
        with pytest.raises(ValueError, match="warped model"):
            acq.construct_function(0, model, "min")
    ei, _ = ta.EI(0.01).construct_function(0, model, "min", 0.0)
    with pytest.raises(ValueError, match="warped model"):
        ta.CandidateSweep(num_random=64).select_batch(_bounds(ta), ei, 2)
    ctx = model._ensure_resident()
    for name in ("sweep_batch", "ts_draw", "mes_draw", "kg_set_points", "set_winner_out"):
        with pytest.raises(ValueError, match="warped model"):
            getattr(ctx, name)
    sur.close()
