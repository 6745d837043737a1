"""CPU: tgp_sweep_batch_mc is part of the C-ABI (declared, exported, bound) and GPU-only (host handles refuse it), and the
plugin refuses what the Monte Carlo strategy does not do before anything reaches the GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_batch_mc_is_declared_exported_and_bound():
    import turbo_amd._lib as L
    h = open(os.path.join(ROOT, "include", "turbogp.h")).read()
    assert re.search(r"\bint tgp_sweep_batch_mc\s*\(", h)
    assert "tgp_sweep_batch_mc" in L.SYMBOLS
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bT tgp_sweep_batch_mc\b", nm)
    assert hasattr(L.load(), "tgp_sweep_batch_mc")
    assert hasattr(L.NativeGP, "sweep_batch_mc")


def test_host_handles_refuse_the_monte_carlo_entry():
    import turbo_amd._lib as L
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (10, 2))
    gp.fit(X, np.sin(X.sum(1)), "rbf", 1.0, 0.5, 1e-4, 1e-10, True)
    gp.set_candidates(rng.uniform(0, 1, (50, 2)))
    with pytest.raises(Exception) as ei:
        gp.sweep_batch_mc(2, 4, 1, None, None, L.ACQ_EI, -1.0, 0.0, 0.01)
    assert "host backend" in str(ei.value)
    idx, val = np.zeros(64, dtype=np.int64), np.zeros(64)
    nul = None
    rc = gp.lib.tgp_sweep_batch_mc(gp._h, 2, 4, 1, nul, nul, 0, L.ACQ_EI, -1.0, 0.0, 0.01, idx.ctypes.data_as(L._i64p),
                                   val.ctypes.data_as(L._dp), nul, nul, nul, nul, nul, nul)
    assert rc == L.BAD_ARG
    assert b"host backend" in gp.lib.tgp_last_error(gp._h)
    assert gp.lib.tgp_sweep_batch_mc(None, 2, 4, 1, nul, nul, 0, L.ACQ_EI, -1.0, 0.0, 0.01, idx.ctypes.data_as(L._i64p),
                                     val.ctypes.data_as(L._dp), nul, nul, nul, nul, nul, nul) == L.BAD_ARG


def test_select_batch_monte_carlo_refuses_what_it_does_not_do():
    import turbo_amd as ta
    from turbo_amd.auxiliary_optimisers import CandidateSweep
    from turbo_amd.bounds import Bounds

    class Foreign:
        def predict(self, X, return_std_dev=False):
            raise AssertionError("never reached")

    acq, _ = ta.EI(0.01).construct_function(0, Foreign(), "min", 0.0)
    lb = Bounds([("x", 0.0, 1.0)])
    with pytest.raises(NotImplementedError, match="grad_restarts"):
        CandidateSweep(num_random=10, grad_restarts=1).select_batch(lb, acq, 2, strategy="monte_carlo")
    with pytest.raises(NotImplementedError, match="HipGPSurrogate"):
        CandidateSweep(num_random=10).select_batch(lb, acq, 2, strategy="monte_carlo", n_sim=8, seed=3)
    with pytest.raises(NotImplementedError, match="HipGPSurrogate"):
        acq.maximise_batch(np.zeros((4, 1)), 2, strategy="monte_carlo", n_sim=8, seed=3)

    class Native:
        X = np.zeros((1, 1))
        y = np.zeros(1)

        def _sweep(self, *a, **k):
            raise AssertionError("never reached")

        def _ensure_resident(self):
            raise AssertionError("never reached")

    ei, _ = ta.EI(0.01).construct_function(0, Native(), "min", 0.0)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="n_sim"):
            ei.maximise_batch(np.zeros((4, 1)), 2, strategy="monte_carlo", n_sim=bad, seed=1)
    with pytest.raises(ValueError, match="strategy"):
        ei.maximise_batch(np.zeros((4, 1)), 2, strategy="marginalise")
    # a TS acquisition still selects batches with 'thompson' only
    ts, _ = ta.TS(seed=1).construct_function(0, Native(), "min")
    with pytest.raises(ValueError, match="thompson"):
        ts.maximise_batch(None, 2, strategy="monte_carlo")
    with pytest.raises(ValueError, match="thompson"):
        CandidateSweep(num_random=10).select_batch(lb, ts, 2, strategy="monte_carlo")
