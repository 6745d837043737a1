"""CPU: the Thompson-sampling entries are part of the C-ABI (declared, exported, bound), GPU-only (host handles refuse
them), and the plugin refuses what it does not do before anything reaches the GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tgp_ts_draw", "tgp_ts_sweep", "tgp_ts_eval", "tgp_ts_read")


def test_entries_are_declared_exported_and_bound():
    import turbo_amd._lib as L
    h = open(os.path.join(ROOT, "include", "turbogp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    lib = L.load()
    for name in ENTRIES:
        assert re.search(r"\bint %s\s*\(" % name, h), name
        assert name in L.SYMBOLS, name
        assert re.search(r"\bT %s\b" % name, nm), name
        assert hasattr(lib, name), name


def test_host_handles_and_bad_arguments_are_refused():
    import ctypes
    import turbo_amd._lib as L
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (10, 2))
    gp.fit(X, np.sin(X.sum(1)), "rbf", 1.0, 0.5, 1e-4, 1e-10, True)
    gp.set_candidates(rng.uniform(0, 1, (50, 2)))
    lib, h = gp.lib, gp._h
    i64 = np.zeros(64, dtype=np.int64)
    d = np.zeros(64 * 64)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    ip = i64.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    BAD = 2   # TGP_BAD_ARG
    assert lib.tgp_ts_draw(h, 1, 1, 64) == BAD
    assert b"host backend" in lib.tgp_last_error(h)
    assert lib.tgp_ts_sweep(h, 1.0, 0, ip, dp, None, None) == BAD
    assert lib.tgp_ts_eval(h, dp, 1, dp, None) == BAD
    assert lib.tgp_ts_read(h, dp, None, None, None) == BAD
    assert lib.tgp_ts_draw(None, 1, 1, 64) == BAD
    with pytest.raises(Exception, match="host backend"):
        gp.ts_draw(1, 1, 64)


def test_plugin_refuses_what_it_does_not_do():
    import turbo_amd as ta
    from turbo_amd.bounds import Bounds

    class Foreign:
        def predict(self, X, return_std_dev=False):
            raise AssertionError("never reached")

    with pytest.raises(NotImplementedError, match="HipGPSurrogate"):
        ta.TS(seed=1).construct_function(0, Foreign(), "min")
    for bad in (0, 63, 100, 16448):
        with pytest.raises(ValueError):
            ta.TS(n_features=bad)
    assert ta.TS().get_type() == "optimism"
    ei, _ = ta.EI(0.01).construct_function(0, Foreign(), "min", 0.0)
    lb = Bounds([("x", 0.0, 1.0)])
    with pytest.raises(ValueError, match="TS acquisition"):
        ta.CandidateSweep(num_random=10).select_batch(lb, ei, 2, strategy="thompson")


def test_seed_rule():
    """trial t draws with (seed + t * 0x9E3779B97F4A7C15) mod 2**64; seed=None takes one draw of NumPy's global RNG"""
    import turbo_amd as ta
    from turbo_amd.acquisition_functions import TS

    class Native:
        X = np.zeros((1, 1))

        def _sweep(self, *a, **k):
            raise AssertionError("never reached")

    _, info = TS(seed=2**64 - 1).construct_function(5, Native(), "max")
    assert info["seed"] == (2**64 - 1 + 5 * 0x9E3779B97F4A7C15) % 2**64
    np.random.seed(3)
    _, a = TS().construct_function(2, Native(), "max")
    np.random.seed(3)
    base = int(np.random.randint(0, 2**63))
    assert a["seed"] == (base + 2 * 0x9E3779B97F4A7C15) % 2**64
    acq, _ = ta.TS(seed=1).construct_function(0, Native(), "min")
    assert acq.get_name() == "TS" and acq.scale_factor == -1
    with pytest.raises(ValueError):
        acq.maximise_batch(None, 2, strategy="kriging_believer")
    for meth in (lambda: acq.refine(None, None), lambda: acq.lbfgsb(None, None), lambda: acq.winner_record(0)):
        with pytest.raises(NotImplementedError):
            meth()
