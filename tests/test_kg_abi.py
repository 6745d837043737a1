"""CPU: the knowledge gradient in the C-ABI (declared, exported, bound), what a host handle answers, and what the KG
plugin checks before anything reaches a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

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
                "int64_t *": L._i64p, "double": c.c_double}
    for name in ("tgp_kg_set_points", "tgp_sweep_kg"):
        assert name in L.SYMBOLS, name
        assert re.search(r"\bT %s\b" % name, nm), name
        want = [ctype_of[re.sub(r"\s*\b\w+$", "", a).strip()] for a in _args_of(h, name)]
        assert getattr(lib, name).argtypes == want, (name, want)
    # GPU only: the host-only library does not carry them
    host = subprocess.run(["nm", "-D", "--defined-only", L.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert not re.search(r"\bT tgp_(kg_set_points|sweep_kg)\b", host)
    assert "Slot [20]" in h


def test_host_handle_answers_bad_arg():
    import turbo_amd._lib as L
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (30, 3))
    y = 2.0 + np.sin(3 * X.sum(1))
    gp.fit(X, y, "matern52", 1.0, 0.6, 1e-3, 1e-10, True)
    gp.set_candidates(rng.uniform(0, 1, (50, 3)))
    lib, h = gp.lib, gp._h
    Xa = np.ascontiguousarray(X[:4])
    assert lib.tgp_kg_set_points(h, Xa.ctypes.data_as(L._dp), 4, None) == BAD
    assert b"host backend" in lib.tgp_last_error(h)
    assert lib.tgp_sweep_kg(h, 1.0, None, None, None, None, None, None, None) == BAD
    assert b"host backend" in lib.tgp_last_error(h)
    assert lib.tgp_kg_set_points(None, Xa.ctypes.data_as(L._dp), 4, None) == BAD
    assert lib.tgp_sweep_kg(None, 1.0, None, None, None, None, None, None, None) == BAD
    with pytest.raises(Exception, match="host"):
        gp.kg_set_points(Xa)
    t = np.zeros(21)
    assert lib.tgp_last_timings(h, t.ctypes.data_as(L._dp), 21) == 0 and t[20] == 0.0


class _Native:
    def __init__(self, X, y):
        self.X, self.y = X, y

    def _sweep(self, *a, **k):
        raise AssertionError("never reached")


def test_plugin_contract_and_refusals():
    import turbo_amd as ta

    class Foreign:
        def predict(self, X, return_std_dev=False):
            raise AssertionError("never reached")

    class Mixture(_Native):
        is_marginalised = True

    assert ta.KG().get_type() == "optimism"
    for bad in (dict(n_points=0), dict(n_points=257), dict(points=np.zeros((0, 2))), dict(points=np.zeros((257, 2))),
                dict(points=np.zeros(3)), dict(points=np.array([[0.0, np.nan]]))):
        with pytest.raises(ValueError):
            ta.KG(**bad)
    X = np.arange(12.0).reshape(6, 2)
    y = np.array([3.0, 1.0, 3.0, 0.5, 1.0, 2.0])
    with pytest.raises(ValueError, match="native models only"):
        ta.KG().construct_function(0, Foreign(), "min")
    with pytest.raises(ValueError, match="marginalised"):
        ta.KG().construct_function(0, Mixture(X, y), "min")
    with pytest.raises(ValueError, match=r"\(A, 2\)"):
        ta.KG(points=np.zeros((3, 5))).construct_function(0, _Native(X, y), "min")
    # the default points: the best observed y in the direction of the extremum, the earlier trial on ties; no RNG
    state = np.random.get_state()[1].copy()
    acq, info = ta.KG(n_points=3).construct_function(0, _Native(X, y), "min")
    assert acq.points.tolist() == X[[3, 1, 4]].tolist() and info == {"n_points": 3, "default_points": True}
    acq, info = ta.KG(n_points=4).construct_function(0, _Native(X, y), "max")
    assert acq.points.tolist() == X[[0, 2, 5, 1]].tolist()
    acq, info = ta.KG(n_points=64).construct_function(0, _Native(X, y), "max")
    assert info["n_points"] == 6 and acq.points.shape == (6, 2)
    assert (np.random.get_state()[1] == state).all()
    given = np.array([[0.5, 0.5]])
    acq, info = ta.KG(points=given).construct_function(0, _Native(X, y), "max")
    assert info == {"n_points": 1, "default_points": False} and acq.points.tolist() == given.tolist()
    assert acq.get_name() == "KG" and acq.scale_factor == 1 and acq.sweep_dtype == "f64"
    assert acq.maximise_host_stream(10, [0, 0], [1, 1]) is None
    for call in (lambda: acq.maximise_batch(None, 2), lambda: acq.refine(None, None), lambda: acq.lbfgsb(None, None),
                 lambda: acq.value_and_grad(X)):
        with pytest.raises(NotImplementedError, match="KG: .* use "):
            call()
