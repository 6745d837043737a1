"""CPU: a pickled WarpedModel, reloaded and served by a HOST handle, predicts the bytes of a host fit on host-warped X and lies
within 1e-9 of oracle.gp_oracle on NumPy-warped X (tests/warp_reference.py's f64 restatement); its hyper-parameters carry
the warp; what input warping does not serve is refused with a ValueError."""
import pickle
import warnings

import numpy as np
import pytest

import warp_reference as wr
from oracle import gp_oracle as G


def _model(ta):
    rng = np.random.RandomState(11)
    N, D = 50, 3
    lo, hi = np.array([-1.0, 0.0, 2.0]), np.array([1.0, 5.0, 2.5])
    X = rng.uniform(lo, hi, (N, D))
    y = np.sin(4 * (X[:, 0] + X[:, 1])) + X[:, 2] + 0.01 * rng.standard_normal(N)
    kern = ta.GPKernel("matern52", 1.3, np.array([0.4, 0.7, 0.5]), 1e-3)
    fac = ta.WarpedHipGPSurrogate(ta.Bounds([("p", lo[0], hi[0]), ("q", lo[1], hi[1]), ("r", lo[2], hi[2])]),
                                  model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=0)
    a, b = np.array([3.0, 1.0, 0.5]), np.array([1.0, 0.4, 2.0])
    return ta.WarpedModel(fac, X, y, kern.copy(), 1e-10, True, lo, hi, a, b), rng.uniform(lo - 0.1, hi + 0.1, (200, D))


def test_a_reloaded_warped_model_predicts_on_a_host_handle():
    import turbo_amd as ta
    model, Xq = _model(ta)
    back = pickle.loads(pickle.dumps(model))
    assert back._factory._reloaded and back._factory._native is None
    back._factory._native = ta.NativeGP(ta._lib.DEVICE_HOST, "f64")          # the handle a process without a GPU ends up with
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mu, sg = back.predict(Xq, return_std_dev=True)
    k, lo, hi, a, b = model.kernel, model.warp_lo, model.warp_hi, model.warp_a, model.warp_b
    host = ta.NativeGP(ta._lib.DEVICE_HOST, "f64")
    host.fit(host.warp_points(model.X, lo, hi, a, b), model.y, k.kind, k.constant, k.length_scale, k.noise_level, 1e-10, True)
    host.set_candidates(host.warp_points(Xq, lo, hi, a, b))
    want = host.sweep(want_mu=True, want_sigma=True)
    assert mu.tobytes() == want["mu"].tobytes() and sg.tobytes() == want["sigma"].tobytes()
    unit = lambda Z: np.clip((Z - lo) / (hi - lo), 0.0, 1.0)
    Wx, Wq = wr.warp_f64(unit(model.X), a[None, :], b[None, :])[0], wr.warp_f64(unit(Xq), a[None, :], b[None, :])[0]
    om = G.fit(Wx, model.y, k.kind, k.constant, k.length_scale, k.noise_level, 1e-10, True)
    omu, osg = G.predict(om, Wq)
    print("against the oracle on NumPy-warped X: mu %.3g, sigma %.3g" % (np.abs(mu - omu).max(), np.abs(sg - osg).max()))
    assert np.abs(mu - omu).max() <= 1e-9 and np.abs(sg - osg).max() <= 1e-9
    assert abs(back.get_log_likelihood() - om.lml) <= 1e-9 * abs(om.lml)
    names = back.get_hyper_param_names()
    assert names[-6:] == ["warp_a_0", "warp_a_1", "warp_a_2", "warp_b_0", "warp_b_1", "warp_b_2"]
    assert np.array_equal(back.get_hyper_params()[-6:], np.concatenate([a, b])) and len(names) == len(back.get_hyper_params())


def test_predict_many_warps_every_model_with_its_own_warp():
    """on host handles too: predict_many over warped models is the per-model predict, bit for bit"""
    import turbo_amd as ta
    model, Xq = _model(ta)
    fac = model._factory
    fac._reloaded, fac._native = True, ta.NativeGP(ta._lib.DEVICE_HOST, "f64")
    other = ta.WarpedModel(fac, model.X[:30], model.y[:30], model.kernel.copy(), 1e-10, True, model.warp_lo, model.warp_hi,
                           np.array([0.5, 2.0, 1.0]), np.array([1.5, 1.0, 1.0]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mus, sgs = fac.predict_many([model, other], Xq, return_std_dev=True)
        for t, m in enumerate((model, other)):
            mu, sg = m.predict(Xq, return_std_dev=True)
            assert mus[t].tobytes() == mu.tobytes() and sgs[t].tobytes() == sg.tobytes()
    assert np.abs(mus[0] - mus[1]).max() > 1e-6


def test_what_input_warping_does_not_serve_is_refused():
    import turbo_amd as ta
    model, _ = _model(ta)
    for acq in (ta.TS(), ta.MES(), ta.KG()):
        with pytest.raises(ValueError, match="warped model"):
            acq.construct_function(0, model, "min")
    ei, _ = ta.EI(0.01).construct_function(0, model, "min", 0.0)
    bounds = ta.Bounds([("p", -1.0, 1.0), ("q", 0.0, 5.0), ("r", 2.0, 2.5)])
    with pytest.raises(ValueError, match="warped model"):
        ta.CandidateSweep(num_random=16).select_batch(bounds, ei, 2)
    with pytest.raises(ValueError, match="warped model"):
        ei.maximise_batch(np.zeros((4, 3)), 2)
    with pytest.raises(ValueError, match="warped model"):
        ei.winner_record(0)
    with pytest.raises(ValueError):
        ta.WarpedHipGPSurrogate(np.array([[0.0, 0.0]]))                      # an empty box
    with pytest.raises(ValueError):
        ta.WarpedHipGPSurrogate(np.array([[0.0, 1.0]]), warp_bounds=(2.0, 4.0))   # the identity warp outside
    with pytest.raises(ValueError):
        ta.WarpedHipGPSurrogate(np.array([[0.0, 1.0]]), criterion="loo")
