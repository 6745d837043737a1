"""CPU: tgp_sweep_batch is part of the C-ABI (declared, exported, bound) and GPU-only (host handles refuse it)."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_batch_is_declared_exported_and_bound():
    import turbo_amd._lib as L
    h = open(os.path.join(ROOT, "include", "turbogp.h")).read()
    assert re.search(r"\bint tgp_sweep_batch\s*\(", h)
    assert "tgp_sweep_batch" in L.SYMBOLS
    assert (L.BATCH_KB, L.BATCH_CL) == (0, 1)
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bT tgp_sweep_batch\b", nm)
    assert hasattr(L.load(), "tgp_sweep_batch")


def test_host_handles_refuse_the_batch_entry():
    import turbo_amd._lib as L
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (10, 2))
    gp.fit(X, np.sin(X.sum(1)), "rbf", 1.0, 0.5, 1e-4, 1e-10, True)
    gp.set_candidates(rng.uniform(0, 1, (50, 2)))
    with pytest.raises(Exception) as ei:
        gp.sweep_batch(2, L.BATCH_KB, 0.0, None, L.ACQ_EI, -1.0, 0.0, 0.01)
    assert "host backend" in str(ei.value)


def test_select_batch_refuses_what_it_does_not_do():
    from turbo_amd.auxiliary_optimisers import CandidateSweep
    from turbo_amd.bounds import Bounds

    class Foreign:
        def predict(self, X, return_std_dev=False):
            raise AssertionError("never reached")

    from turbo_amd.acquisition_functions import EI
    acq, _ = EI(0.01).construct_function(0, Foreign(), "min", 0.0)
    lb = Bounds([("x", 0.0, 1.0)])
    with pytest.raises(NotImplementedError, match="grad_restarts"):
        CandidateSweep(num_random=10, grad_restarts=1).select_batch(lb, acq, 2)
    with pytest.raises(NotImplementedError, match="HipGPSurrogate"):
        CandidateSweep(num_random=10).select_batch(lb, acq, 2)
    with pytest.raises(NotImplementedError, match="HipGPSurrogate"):
        acq.maximise_batch(np.zeros((4, 1)), 2)
