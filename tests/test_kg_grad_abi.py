"""CPU: the knowledge gradient's gradient in the C-ABI (tgp_kg_grad, tgp_kg_lbfgsb: declared, exported, bound), what a host
handle answers, and what ``ta.KG(gradient=True)`` offers and refuses before anything reaches a GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 2   # TGP_BAD_ARG
ENTRIES = ("tgp_kg_grad", "tgp_kg_lbfgsb")


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
    for name in ENTRIES:
        assert name in L.SYMBOLS, name
        assert re.search(r"\bT %s\b" % name, nm), name
        want = [ctype_of[re.sub(r"\s*\b\w+$", "", a).strip()] for a in _args_of(h, name)]
        assert getattr(lib, name).argtypes == want, (name, want)
    assert hasattr(L.NativeGP, "kg_grad") and hasattr(L.NativeGP, "kg_lbfgsb")
    # GPU only: the host-only library does not carry them
    host = subprocess.run(["nm", "-D", "--defined-only", L.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert not re.search(r"\bT tgp_kg_(grad|lbfgsb)\b", host)


def test_host_handle_answers_bad_arg():
    import turbo_amd._lib as L
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (30, 3))
    y = 2.0 + np.sin(3 * X.sum(1))
    gp.fit(X, y, "matern52", 1.0, 0.6, 1e-3, 1e-10, True)
    lib, h = gp.lib, gp._h
    dp = lambda a: a.ctypes.data_as(L._dp)
    Xq, val, grad = np.ascontiguousarray(X[:2]), np.zeros(2), np.zeros((2, 3))
    lo, hi = np.zeros(3), np.ones(3)
    assert lib.tgp_kg_grad(h, dp(Xq), 2, 1.0, dp(val), dp(grad)) == BAD
    assert b"host backend" in lib.tgp_last_error(h)
    assert lib.tgp_kg_lbfgsb(h, dp(Xq), 2, dp(lo), dp(hi), 1.0, 10, dp(grad), dp(val), None, None) == BAD
    assert b"host backend" in lib.tgp_last_error(h)
    assert lib.tgp_kg_grad(None, dp(Xq), 2, 1.0, dp(val), dp(grad)) == BAD
    assert lib.tgp_kg_lbfgsb(None, dp(Xq), 2, dp(lo), dp(hi), 1.0, 10, dp(grad), dp(val), None, None) == BAD
    with pytest.raises(Exception, match="host"):
        gp.kg_grad(Xq)
    with pytest.raises(Exception, match="host"):
        gp.kg_lbfgsb(Xq, lo, hi)


class _Native:
    def __init__(self, X, y):
        self.X, self.y = X, y

    def _sweep(self, *a, **k):
        raise AssertionError("never reached")

    def _ensure_resident(self):
        raise AssertionError("reached the model")


def test_gradient_instance_offers_two_methods_and_refuses_two():
    import turbo_amd as ta
    X = np.arange(12.0).reshape(6, 2)
    y = np.array([3.0, 1.0, 3.0, 0.5, 1.0, 2.0])
    acq, info = ta.KG(n_points=3, gradient=True).construct_function(0, _Native(X, y), "min")
    assert info == {"n_points": 3, "default_points": True, "gradient": True}
    assert isinstance(acq, ta.KG.FunctionInstance) and acq.get_name() == "KG" and acq.sweep_dtype == "f64"
    assert acq.points.tolist() == X[[3, 1, 4]].tolist()
    # offered: they go for the model's context (this stand-in has none)
    for call in (lambda: acq.value_and_grad(X[:2]), lambda: acq.lbfgsb(X[:2], [(0, 12), (0, 12)])):
        with pytest.raises(AssertionError, match="reached the model"):
            call()
    # refused, with a text of their own
    for call in (lambda: acq.maximise_batch(None, 2), lambda: acq.refine(None, None)):
        with pytest.raises(NotImplementedError, match=r"KG: .*gradient=True serves.* use "):
            call()
    assert acq.maximise_host_stream(10, [0, 0], [1, 1]) is None
    from turbo_amd.auxiliary_optimisers import _offers
    assert all(_offers(acq, name) for name in ("value_and_grad", "lbfgsb", "maximise_topk"))


def test_the_default_instance_is_unchanged():
    import turbo_amd as ta
    X = np.arange(12.0).reshape(6, 2)
    y = np.array([3.0, 1.0, 3.0, 0.5, 1.0, 2.0])
    assert ta.KG().gradient is False and ta.KG(gradient=False).gradient is False
    acq, info = ta.KG(n_points=3).construct_function(0, _Native(X, y), "min")
    assert type(acq) is ta.KG.FunctionInstance and info == {"n_points": 3, "default_points": True}
    for call in (lambda: acq.maximise_batch(None, 2), lambda: acq.refine(None, None), lambda: acq.lbfgsb(None, None),
                 lambda: acq.value_and_grad(X)):
        with pytest.raises(NotImplementedError, match="its gradient is not implemented"):
            call()
