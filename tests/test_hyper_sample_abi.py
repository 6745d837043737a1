"""CPU (host handle): tgp_hyper_sample walks the chain of the NumPy reference (tests/slice_reference.py) -- the same
evaluations, the same samples -- refuses bad arguments, and hands a non-PD start back."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import hyper_sample_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import turbo_amd._lib as lib
    return lib


def test_entries_are_declared_exported_and_bound(L):
    h = open(os.path.join(ROOT, "include", "turbogp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    for name in ("tgp_hyper_sample", "tgp_sweep_integrated"):
        assert re.search(r"\bint %s\s*\(" % name, h)
        assert name in L.SYMBOLS and hasattr(L.load(), name)
        assert re.search(r"\bT %s\b" % name, nm)
    assert hasattr(L.NativeGP, "hyper_sample") and hasattr(L.NativeGP, "sweep_integrated")
    # the host-only library serves the sampler too (a reloaded model's hyper-parameters can be sampled without ROCm)
    nm_host = subprocess.run(["nm", "-D", "--defined-only", L.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert re.search(r"\bT tgp_hyper_sample\b", nm_host) and not re.search(r"\bT tgp_sweep_integrated\b", nm_host)


@pytest.mark.parametrize("name", ["rbf_iso_noise_n12", "matern52_ard_fixed_noise_n40", "matern32_iso_fixed_constant_n15"])
def test_host_handle_walks_the_reference_chain(L, name):
    c = hc.case(name)
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    ref, theta, lml = hc.assert_same_walk(gp, c, S=6, burn=3, thin=2)
    fixed = ~(c["lo"] < c["hi"])
    assert np.all(theta[:, fixed] == c["lo"][fixed])
    assert np.all(theta >= c["lo"]) and np.all(theta <= c["hi"])
    # the same seed again: the same bytes; another seed: another walk
    again = hc.native(gp, c, 6, 3, 2)
    assert again[0].tobytes() == theta.tobytes() and again[1].tobytes() == lml.tobytes()
    other = gp.hyper_sample(c["X"], c["y"], c["kind"], c["theta0"], c["n_ls"], np.stack([c["lo"], c["hi"]], 1), c["jitter"],
                            c["normalize_y"], n_samples=6, burn=3, thin=2, width=c["width"], seed=c["seed"] + 1000)
    assert other[0].tobytes() != theta.tobytes()
    gp.close()


def test_host_only_library_walks_the_same_chain(L):
    """libturbogp_host.so exports the entry: loaded on its own (no HIP), it returns the full library's bytes"""
    c = hc.case("rbf_iso_noise_n12")
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    want = hc.native(gp, c, 3, 1, 1)
    gp.close()
    lib = ctypes.CDLL(L.HOST_LIB_PATH)
    h = ctypes.c_void_p()
    assert lib.tgp_create(-1, 0, ctypes.byref(h)) == 0
    lib.tgp_hyper_sample.argtypes = L._argtypes()["tgp_hyper_sample"]
    th, lm = np.empty((3, 3)), np.empty(3)
    ev, npd = ctypes.c_int64(0), ctypes.c_int64(0)
    X, y = np.ascontiguousarray(c["X"]), np.ascontiguousarray(c["y"])
    t0, lo, hi = (np.ascontiguousarray(c[k]) for k in ("theta0", "lo", "hi"))
    rc = lib.tgp_hyper_sample(h, L._ptr(X), 12, 1, L._ptr(y), L.KERNELS["rbf"], L._ptr(t0), 1, L._ptr(lo), L._ptr(hi), 1e-10, 1,
                              3, 1, 1, None, c["seed"], L._ptr(th), L._ptr(lm), ctypes.byref(ev), ctypes.byref(npd))
    assert rc == 0 and th.tobytes() == want[0].tobytes() and ev.value == want[2]
    lib.tgp_destroy.argtypes = [ctypes.c_void_p]
    lib.tgp_destroy(h)


def test_bad_arguments_and_a_non_pd_start(L):
    c = hc.case("rbf_iso_noise_n12")
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    lb = np.stack([c["lo"], c["hi"]], 1)

    def call(**kw):
        a = dict(theta0=c["theta0"], lb=lb, S=4, burn=1, thin=1, width=None, X=c["X"], jitter=1e-10)
        a.update(kw)
        return gp.hyper_sample(a["X"], c["y"], "rbf", a["theta0"], 1, a["lb"], a["jitter"], True, n_samples=a["S"], burn=a["burn"],
                               thin=a["thin"], width=a["width"], seed=1)

    for kw in (dict(S=0), dict(S=65), dict(thin=0), dict(burn=-1), dict(width=[1.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match="tgp_hyper_sample"):
            call(**kw)
    swapped = lb.copy()
    swapped[1] = swapped[1, ::-1]
    with pytest.raises(ValueError, match="lo <= hi"):
        call(lb=swapped)
    outside = c["theta0"].copy()
    outside[1] = c["hi"][1] + 0.5
    with pytest.raises(ValueError, match="inside the box"):
        call(theta0=outside)
    nul = None
    assert gp.lib.tgp_hyper_sample(None, nul, 1, 1, nul, 0, nul, 1, nul, nul, 0.0, 1, 1, 0, 1, nul, 0, nul, nul, nul, nul) == L.BAD_ARG
    assert gp.lib.tgp_hyper_sample(gp._h, nul, 1, 1, nul, 0, nul, 1, nul, nul, 0.0, 1, 1, 0, 1, nul, 0, nul, nul, nul, nul) == L.BAD_ARG
    # duplicated rows, no jitter, no noise term: the start itself is not positive definite -> TGP_NOT_PD
    Xd = np.vstack([c["X"][:6], c["X"][:6]])
    nonoise = lb.copy()
    nonoise[2] = -np.inf
    with pytest.raises(np.linalg.LinAlgError, match="theta0"):
        call(X=Xd, lb=nonoise, jitter=0.0)
    gp.close()
