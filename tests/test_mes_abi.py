"""CPU: max-value entropy search in the C-ABI (declared, exported, bound), on host handles (the reload path), and what
the MES plugin refuses before anything reaches a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import mes_reference as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 2   # TGP_BAD_ARG


def _args_of(header, name):
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header)
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_entries_are_declared_exported_and_bound():
    import turbo_amd._lib as L
    h = open(os.path.join(ROOT, "include", "turbogp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    lib = L.load()
    c = ctypes
    ctype_of = {"tgp_handle": c.c_void_p, "const double *": L._dp, "double *": L._dp, "int64_t": c.c_int64,
                "uint64_t": c.c_uint64, "double": c.c_double, "int": c.c_int}
    for name in ("tgp_mes_set_maxima", "tgp_mes_draw"):
        assert name in L.SYMBOLS, name
        assert re.search(r"\bT %s\b" % name, nm), name
        want = []
        for a in _args_of(h, name):
            ty = re.sub(r"\s*\b\w+$", "", a).strip()        # drop the parameter's name
            want.append(ctype_of[ty if not ty.endswith("*") else ty.replace(" *", " *")])
        assert getattr(lib, name).argtypes == want, (name, want)
    assert re.search(r"\b[A-Z]+_ACQ_MES\s*=\s*5\b", h) and L.ACQ_MES == 5
    # the host-only library serves the maxima too (a reloaded MES instance), the draw is GPU only
    host = subprocess.run(["nm", "-D", "--defined-only", L.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bT tgp_mes_set_maxima\b", host) and not re.search(r"\bT tgp_mes_draw\b", host)


def _host_gp(noise=1e-3, normalize_y=True):
    import turbo_amd._lib as L
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (30, 3))
    y = 2.0 + np.sin(3 * X.sum(1)) + 0.01 * rng.normal(size=30)
    gp.fit(X, y, "matern52", 1.0, 0.6, noise, 1e-10, normalize_y)
    return gp, X, y, rng.uniform(0, 1, (500, 3))


def test_host_handle_rules():
    import turbo_amd._lib as L
    gp, X, y, Xc = _host_gp()
    gp.set_candidates(Xc)
    lib, h = gp.lib, gp._h
    dp = lambda a: a.ctypes.data_as(L._dp)
    with pytest.raises(ValueError, match="maxima"):
        gp.sweep(L.ACQ_MES)                                       # no maxima yet
    one = np.array([3.0])
    assert lib.tgp_mes_set_maxima(h, dp(one), 0) == BAD
    assert lib.tgp_mes_set_maxima(h, dp(np.zeros(65)), 65) == BAD
    assert lib.tgp_mes_set_maxima(h, dp(np.array([1.0, np.nan])), 2) == BAD
    assert lib.tgp_mes_set_maxima(h, None, 1) == BAD
    assert lib.tgp_mes_set_maxima(None, dp(one), 1) == BAD
    with pytest.raises(ValueError, match="maxima"):
        gp.sweep(L.ACQ_MES)                                       # the refused calls stored nothing
    gp.mes_set_maxima(one)
    assert gp.sweep(L.ACQ_MES)["best_val"] > 0
    gp.fit(X, y, "matern52", 1.0, 0.6, 1e-3, 1e-10, True)         # a refit drops them
    with pytest.raises(ValueError, match="maxima"):
        gp.sweep(L.ACQ_MES)
    gp.mes_set_maxima(one)
    gp.import_state(gp.export_state())                            # ... and so does a state import
    with pytest.raises(ValueError, match="maxima"):
        gp.evaluate(Xc, L.ACQ_MES)
    with pytest.raises(Exception, match="host"):
        gp.mes_draw(1, 4, 64)                                     # GPU only
    with pytest.raises(ValueError):
        gp.sweep(6)                                               # beyond the enum


@pytest.mark.parametrize("noise,ny", [(1e-3, True), (0.0, True), (1e-2, False)])
def test_host_evaluate_equals_the_reference(noise, ny):
    """tgp_evaluate(MES) on a host handle against the reference fed the host backend's own mu / sigma: the bar of the
    GPU epilogues, 1e-9 x the best value (the host's erfcx is its own: a continued fraction from z = 3 on)"""
    import turbo_amd._lib as L
    gp, X, y, Xc = _host_gp(noise, ny)
    Xc[:5] = X[:5]
    y_std = float(y.std()) if ny else 1.0
    for sf in (1.0, -1.0):
        for ys in (np.array([y.max() if sf > 0 else y.min()]), (y.mean() + sf * np.linspace(-2.0, 3.0, 7)),
                   np.array([y.mean() - sf * 40.0])):
            gp.mes_set_maxima(ys)
            r = gp.evaluate(Xc, L.ACQ_MES, sf, 7.0, 9.0, want_mu=True, want_sigma=True, want_acq=True)
            want = mr.mes(r["mu"], r["sigma"], ys, sf, noise, y_std)
            assert np.all(np.isfinite(r["acq"]))
            assert np.abs(r["acq"] - want).max() <= 1e-9 * want.max()
            assert r["best_idx"] == int(np.argmax(r["acq"])) and r["best_val"] == r["acq"].max()


class _Native:
    X = np.zeros((1, 1))

    def _sweep(self, *a, **k):
        raise AssertionError("never reached")


def test_plugin_contract_and_refusals():
    import turbo_amd as ta

    class Foreign:
        def predict(self, X, return_std_dev=False):
            raise AssertionError("never reached")

    assert ta.MES().get_type() == "optimism"
    with pytest.raises(ValueError, match="native models only"):
        ta.MES(seed=1).construct_function(0, Foreign(), "min")
    for bad in (dict(n_samples=0), dict(n_samples=65), dict(n_features=100)):
        with pytest.raises(ValueError):
            ta.MES(**bad)
    acq, info = ta.MES(n_samples=4, seed=2**64 - 1).construct_function(5, _Native(), "min")
    assert info["seed"] == (2**64 - 1 + 5 * 0x9E3779B97F4A7C15) % 2**64 and info["n_samples"] == 4
    assert acq.get_name() == "MES" and acq.scale_factor == -1 and acq.maxima is None
    np.random.seed(3)
    _, a = ta.MES().construct_function(2, _Native(), "max")
    np.random.seed(3)
    assert a["seed"] == (int(np.random.randint(0, 2**63)) + 2 * 0x9E3779B97F4A7C15) % 2**64
    with pytest.raises(NotImplementedError, match="MES"):
        acq.maximise_batch(None, 2)
    with pytest.raises(NotImplementedError, match="MES"):
        acq.refine(None, None)


def test_dill_round_trip_through_the_host_backend():
    """an instance that carries its maxima is evaluated where there is no GPU: the Recorder's plot path"""
    import warnings
    import dill
    import turbo_amd as ta
    from turbo_amd.acquisition_functions import MES
    rng = np.random.RandomState(1)
    X = rng.uniform(0, 1, (25, 2))
    y = np.cos(4 * X[:, 0]) + X[:, 1]
    sur = ta.HipGPSurrogate.__new__(ta.HipGPSurrogate)
    sur.__setstate__(dict(model_params=dict(kernel=ta.GPKernel("rbf", 1.0, 0.4, 1e-3), optimizer=None, normalize_y=True),
                          training_iterations=0, param_continuity=True, dtype="f64", device=ta._lib.DEVICE_HOST,
                          incremental=False, _last_model_params=None))
    model = ta.HipGPSurrogate.ModelInstance(sur, X, y, ta.GPKernel("rbf", 1.0, 0.4, 1e-3), 1e-10, True)
    acq = MES.FunctionInstance(model, "max", 1, 3, 64, maxima=[1.9, 2.0, 2.4])
    again = dill.loads(dill.dumps(acq))
    assert again.maxima.tobytes() == acq.maxima.tobytes()
    g = rng.uniform(0, 1, (200, 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = again(g)
        mu, sg = again.model.predict(g, return_std_dev=True)
        i, v = again.maximise(g)
    want = mr.mes(mu, sg, acq.maxima, 1.0, 1e-3, float(y.std()))
    assert np.abs(got - want).max() <= 1e-9 * want.max()
    assert i == int(np.argmax(got)) and v == got[i]
    fresh = MES.FunctionInstance(again.model, "max", 1, 3, 64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="drawn on the GPU"):
            fresh(g)
