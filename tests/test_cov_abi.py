"""CPU: the joint posterior in the C-ABI (declared, exported, bound), on host handles (the reload path) against
tests/cov_reference.py, and through ModelInstance after a dill round trip with no GPU visible."""
import ctypes
import os
import re
import subprocess
import warnings

import numpy as np
import pytest

import cov_reference as cr
from oracle import gp_oracle as G
from test_cov_reference import GOLDENS, golden_model, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_PD, BAD, NOT_FITTED = 0, 1, 2, 4
TOL = 1e-5      # the project's bar for fp64 through the C-ABI (tests/test_gpu_parity.py), times the prior scale


def _args_of(header, name):
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header)
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_entries_are_declared_exported_and_bound():
    import turbo_amd._lib as L
    h = open(os.path.join(ROOT, "include", "turbogp.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    host = subprocess.run(["nm", "-D", "--defined-only", L.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    lib = L.load()
    c = ctypes
    ctype_of = {"tgp_handle": c.c_void_p, "const double *": L._dp, "double *": L._dp, "int64_t": c.c_int64,
                "int64_t *": L._i64p, "uint64_t": c.c_uint64, "double": c.c_double, "int": c.c_int}
    for name in ("tgp_predict_cov", "tgp_sample_joint"):
        assert name in L.SYMBOLS, name
        assert re.search(r"\bT %s\b" % name, nm), name
        assert re.search(r"\bT %s\b" % name, host), name            # the host-only library serves both
        want = [ctype_of[re.sub(r"\s*\b\w+$", "", a).strip()] for a in _args_of(h, name)]
        assert getattr(lib, name).argtypes == want, (name, want)


def _host_gp(X, y, kind, c, ls, noise, jitter, ny):
    import turbo_amd._lib as L
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    gp.fit(X, y, kind, c, ls, noise, jitter, ny)
    return gp


def _fuzzed():
    rng = np.random.RandomState(5)
    X = rng.uniform(0, 1, (30, 3))
    y = 2.0 + np.sin(3 * X.sum(1)) + 0.01 * rng.normal(size=30)
    Xq = rng.uniform(-0.1, 1.1, (21, 3))
    return dict(X=X, y=y, Xq=Xq, kind="matern32", constant=1.2, ls=0.6, noise=1e-3, jitter=1e-10, normalize_y=True)


def _cases():
    return [load_golden(n) for n in GOLDENS] + [_fuzzed()]


@pytest.mark.parametrize("i", range(3))
@pytest.mark.parametrize("latent", [False, True])
def test_host_handle_equals_the_reference(i, latent):
    d = _cases()[i]
    model = golden_model(d)
    gp = _host_gp(d["X"], d["y"], d["kind"], float(d["constant"]), d["ls"], float(d["noise"]), float(d["jitter"]), bool(d["normalize_y"]))
    vs, ms = cr.scales(model)
    mu, cov, neg = gp.predict_cov(d["Xq"], latent)
    wmu, wcov, wneg = cr.predict_cov(model, d["Xq"], latent)
    print("host predict_cov case %d latent %d: mu err %.3g cov err %.3g (scaled)" % (i, latent, np.abs(mu - wmu).max() / ms, np.abs(cov - wcov).max() / vs))
    assert np.abs(mu - wmu).max() <= TOL * ms and np.abs(cov - wcov).max() <= TOL * vs
    assert np.array_equal(cov, cov.T)                               # symmetric bit for bit
    assert neg == int((np.diag(cov) < 0).sum())
    if not latent:                                                  # the diagonal is tgp_predict's sigma^2 before its clamp
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sg = gp.evaluate(d["Xq"], want_sigma=True)["sigma"]
        assert np.abs(np.maximum(np.diag(cov), 0.0) - sg ** 2).max() <= TOL * vs
    eps = np.random.RandomState(3).standard_normal((6, len(d["Xq"])))
    nug = 1e-8
    r = gp.sample_joint(d["Xq"], 6, eps=eps, latent=latent, nugget=nug)
    wy, _ = cr.sample_joint(model, d["Xq"], eps, latent, nug)
    print("host sample_joint: y err %.3g (scaled)" % (np.abs(r["y"] - wy).max() / ms))
    # (Lc's rounding is amplified by the conditioning of Sigma + nugget I; these cases stay far inside the bar)
    assert np.abs(r["y"] - wy).max() <= TOL * ms
    assert np.array_equal(r["eps"], eps) and np.array_equal(r["mu"], mu)


def test_negative_diagonal_entries_are_counted_not_clamped():
    """a noise-free, jitter-free model queried AT its training points: the latent variance there is rounding noise of
    either sign (with a jitter it is the jitter, to the last digit)"""
    rng = np.random.RandomState(2)
    X = rng.uniform(0, 1, (40, 2))
    y = np.sin(5 * X[:, 0])
    gp = _host_gp(X, y, "matern12", 1.0, 0.5, 0.0, 0.0, False)
    mu, cov, neg = gp.predict_cov(X, latent=True)
    d = np.diag(cov)
    assert neg == int((d < 0).sum()) and np.abs(d).max() < 1e-12
    assert neg > 0, "this case is meant to have entries below zero: pick another if the arithmetic changed"
    assert np.array_equal(cov, cov.T)


def test_bad_arguments():
    import turbo_amd._lib as L
    d = _fuzzed()
    lib = L.load()
    fresh = L.NativeGP(L.DEVICE_HOST, "f64")
    dp = lambda a: a.ctypes.data_as(L._dp)
    Xq = np.ascontiguousarray(d["Xq"][:4])
    cov, y, eps = np.empty((4, 4)), np.empty((3, 4)), np.zeros((3, 4))
    assert lib.tgp_predict_cov(fresh._h, dp(Xq), 4, 0, None, dp(cov), None) == NOT_FITTED
    assert lib.tgp_sample_joint(fresh._h, dp(Xq), 4, 3, 0, 0.0, 0, dp(eps), dp(y), None, None) == NOT_FITTED
    gp = _host_gp(d["X"], d["y"], d["kind"], d["constant"], d["ls"], d["noise"], d["jitter"], True)
    h = gp._h
    big = np.zeros((4097, 3))
    assert lib.tgp_predict_cov(None, dp(Xq), 4, 0, None, dp(cov), None) == BAD
    assert lib.tgp_predict_cov(h, dp(Xq), 0, 0, None, dp(cov), None) == BAD
    assert lib.tgp_predict_cov(h, dp(big), 4097, 0, None, dp(cov), None) == BAD
    assert lib.tgp_predict_cov(h, None, 4, 0, None, dp(cov), None) == BAD
    assert lib.tgp_predict_cov(h, dp(Xq), 4, 0, None, None, None) == BAD
    bad = Xq.copy(); bad[1, 2] = np.inf
    assert lib.tgp_predict_cov(h, dp(bad), 4, 0, None, dp(cov), None) == BAD
    assert lib.tgp_predict_cov(h, dp(Xq), 4, 0, None, dp(cov), None) == OK       # mu_out and the count are nullable
    sj = lambda Xp=Xq, m=4, S=3, nug=0.0, e=eps, yo=y: lib.tgp_sample_joint(h, dp(Xp) if Xp is not None else None, m, S, 0, nug, 1,
                                                                           dp(e) if e is not None else None,
                                                                           dp(yo) if yo is not None else None, None, None)
    assert sj() == OK
    assert sj(e=None) == BAD                                          # the host backend cannot draw
    assert sj(S=0) == BAD and sj(S=4097) == BAD and sj(m=0) == BAD and sj(m=4097) == BAD
    assert sj(nug=-1e-12) == BAD and sj(nug=np.inf) == BAD and sj(nug=np.nan) == BAD
    assert sj(Xp=None) == BAD and sj(yo=None) == BAD and sj(Xp=bad) == BAD
    e2 = eps.copy(); e2[2, 3] = np.nan
    assert sj(e=e2) == BAD
    with pytest.raises(ValueError, match="eps_in"):
        gp.sample_joint(Xq, 3)


def test_duplicated_rows_need_a_nugget():
    d = _fuzzed()
    gp = _host_gp(d["X"], d["y"], d["kind"], d["constant"], d["ls"], d["noise"], d["jitter"], True)
    Xq = np.vstack([d["Xq"][:5], d["Xq"][2:3]])
    eps = np.random.RandomState(0).standard_normal((2, 6))
    with pytest.raises(np.linalg.LinAlgError):
        gp.sample_joint(Xq, 2, eps=eps, latent=True, nugget=0.0)
    r = gp.sample_joint(Xq, 2, eps=eps, latent=True, nugget=1e-6)
    assert np.all(np.isfinite(r["y"]))
    assert np.all(np.isfinite(gp.sample_joint(Xq, 2, eps=eps, latent=False, nugget=0.0)["y"]))   # the noise separates them


def test_model_instance_after_a_dill_round_trip_without_a_gpu():
    """the Recorder's reload path: predict_cov, sample_y and joint_ei of an unpickled model through the host backend"""
    import dill
    import turbo_amd as ta
    d = _fuzzed()
    kern = ta.GPKernel(d["kind"], d["constant"], d["ls"], d["noise"])
    sur = ta.HipGPSurrogate.__new__(ta.HipGPSurrogate)
    sur.__setstate__(dict(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=0,
                          param_continuity=True, dtype="f64", device=ta._lib.DEVICE_HOST, incremental=False,
                          _last_model_params=None))
    model = dill.loads(dill.dumps(ta.HipGPSurrogate.ModelInstance(sur, d["X"], d["y"], kern, 1e-10, True)))
    ref = G.fit(d["X"], d["y"], d["kind"], d["constant"], d["ls"], d["noise"], 1e-10, True)
    vs, ms = cr.scales(ref)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mu, cov = model.predict_cov(d["Xq"])
        wmu, wcov, _ = cr.predict_cov(ref, d["Xq"])
        assert mu.shape == (21, 1) and cov.shape == (21, 21)
        assert np.abs(mu[:, 0] - wmu).max() <= TOL * ms and np.abs(cov - wcov).max() <= TOL * vs
        eps = np.random.RandomState(9).standard_normal((5, 21))
        ys = model.sample_y(d["Xq"], n_samples=5, eps=eps)
        assert ys.shape == (21, 5)
        assert np.abs(ys.T - cr.sample_joint(ref, d["Xq"], eps, False, 1e-10)[0]).max() <= TOL * ms
        # seed on the host backend: NumPy's RandomState(seed) draws eps (documented to differ from the device draw)
        a = model.sample_y(d["Xq"], n_samples=4, seed=11)
        want_eps = np.random.RandomState(11).standard_normal((4, 21))
        assert np.abs(a.T - cr.sample_joint(ref, d["Xq"], want_eps, False, 1e-10)[0]).max() <= TOL * ms
        got = ta.joint_ei(model, d["Xq"][:4], "min", float(d["y"].min()), xi=0.01, eps=eps[:, :4])
        want = cr.joint_ei(ref, d["Xq"][:4], eps[:, :4], "min", float(d["y"].min()), 0.01)
        assert abs(got - want) <= TOL * ms
        dup = np.vstack([d["Xq"][:3], d["Xq"][:1]])
        with pytest.raises(np.linalg.LinAlgError):
            model.sample_y(dup, eps=np.zeros((1, 4)), latent=True, nugget=0.0)

    class Foreign:
        def predict(self, X, return_std_dev=False):
            raise AssertionError("never reached")
    with pytest.raises(ValueError, match="native models only"):
        ta.joint_ei(Foreign(), d["Xq"][:2], "min", 0.0)


def test_host_backend_joint_posterior_under_sanitizers(tmp_path):
    """AddressSanitizer + UBSan over the host backend's two entries: a stand-alone program, nothing loaded into python"""
    csrc = os.path.join(ROOT, "turbo_amd", "csrc")
    exe = str(tmp_path / "host_cov_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-I" + csrc, os.path.join(ROOT, "tests", "host_cov_sanitizer_driver.cpp"),
           os.path.join(csrc, "host_backend.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if built.returncode != 0 and ("asan" in built.stderr.lower() or "sanitize" in built.stderr.lower()):
        pytest.skip("this g++ has no sanitizer runtime: " + built.stderr[-200:])
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], env=dict(os.environ, TGP_HOST_THREADS="3"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
