"""CPU: the references of tests/test_gpu_loo.py judged before they judge anything, and the host backend's tgp_loo.
 (a) the 80-bit closed form (tests/loo_reference_hp.py) equals LITERAL leave-one-out: for the cases of at most 65 points, N
     refits on N - 1 points through oracle.gp_oracle with the hyper-parameters, y_mean and y_std held;
 (b) its gradient equals central differences in log theta of the 80-bit L_LOO itself;
 (c) every case can judge: the f64 restatement's errors are the e_ref the bars are built from, recorded in
     tests/golden/loo_eref.json (written where LOO_WRITE=1), and every case meets the cap's condition;
 (d) the bars reject the slips they exist for, each injected into the f64 restatement;
 (e) the host backend (tgp_loo on a TGP_DEVICE_HOST handle, and libturbogp_host.so) is held to the bars on every case of at
     most 384 points;
 (f) argument checks that need no GPU;
 (g) the host backend's tgp_loo under AddressSanitizer + UBSan, as a stand-alone program."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import loo_edge_cases as le
import loo_reference_hp as lo
from oracle import gp_oracle as G

LD = np.longdouble
EREF_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loo_eref.json")
LITERAL_CASES = [c for c in le.CASES if le.config(c)["N"] <= 65]
LITERAL_TOL = 1e-9
# every case of at most 300 points and five hyper-parameters, and one wide ARD one (each hyper-parameter costs four 80-bit fits)
FD_CASES = [c for c in le.CASES if le.config(c)["N"] <= 300 and (not le.config(c)["ard"] or le.config(c)["D"] <= 3)] + ["S2/ard"]
FD_STEP = 2e-3
# as tests/test_lml_grad_reference.py reasons for the LML: the extrapolated difference is off by the order of step^4 = 1.6e-11
# times a fifth derivative of the order of the scale at most, and a wrong formula is of order 1 of the ENTRY
FD_CEILING_SCALE, FD_CEILING_ENTRY = 1e-10, 1e-6
SLIP_CASES = ["S3/iso", "S3/ard", "T193/iso", "T193/ard", "T193-noise0/ard", "D/iso", "E/ard"]
HOST_CASES = [c for c in le.CASES if le.config(c)["N"] <= 384]


def _record():
    with open(EREF_JSON) as f:
        return json.load(f)


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LITERAL_CASES)
def test_the_closed_form_is_literal_leave_one_out(case):
    """N models of N - 1 points each, fitted and queried by the f64 oracle on the targets normalised ONCE with all N points
    (normalize_y off in the refits: y_mean and y_std are held), the held-out observation's variance with the jitter K
    carries.  mu_-i, sigma_-i (normalised units) and L_LOO to 1e-9."""
    X, y, kind, c, ls, noise, jitter, norm = le.call_args(case)
    ref = le.hp_reference(case)
    n = len(y)
    yn, y_mean, y_std = G.normalise_y(y, norm)
    if n == 1:                  # nothing is left to condition on: the prior, mean 0 and variance c + noise + jitter
        mu, var = np.zeros(1), np.array([c + noise + jitter])
    else:
        mu, var = np.zeros(n), np.zeros(n)
        for i in range(n):
            keep = np.arange(n) != i
            m = G.fit(X[keep], yn[keep], kind, c, ls, noise, jitter, False)
            mi, si = G.predict(m, X[i:i + 1])
            mu[i], var[i] = mi[0], si[0] ** 2 + jitter
    lpd = -0.5 * np.log(var) - 0.5 * (yn - mu) ** 2 / var - 0.5 * np.log(2 * np.pi)
    want_mu = (yn.astype(LD) - ref["resid"] / ref["resid"].dtype.type(y_std)).astype(np.float64)
    want_sigma = (ref["sigma"] / LD(y_std)).astype(np.float64)
    d = (np.abs(mu - want_mu).max(), np.abs(np.sqrt(var) - want_sigma).max(), abs(lpd.sum() - float(ref["loo"])))
    print("%s literal leave-one-out against the closed form: mu %.3g  sigma %.3g  L_LOO %.3g" % ((case,) + d))
    assert max(d) <= LITERAL_TOL


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FD_CASES)
def test_the_gradient_against_central_differences(case):
    ref = le.hp_reference(case)
    fd = lo.central_differences(*le.call_args(case), step=FD_STEP)
    n = len(fd)
    assert n == len(ref["grad"]) - (1 if le.call_args(case)[5] == 0.0 else 0)
    d = np.abs(fd - ref["grad"][:n])
    sc = ref["grad_scale"][:n]
    of_scale = float((d / np.where(sc == 0, LD(1), sc)).max())
    of_entry = float(d.max() / max(np.abs(ref["grad"][:n]).max(), LD(1e-300)))
    print("%s closed form against Richardson-extrapolated central differences (h = %g): %.3g of the scale, %.3g of the largest entry"
          % (case, FD_STEP, of_scale, of_entry))
    assert of_scale <= FD_CEILING_SCALE and of_entry <= FD_CEILING_ENTRY


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", le.CASES)
def test_the_case_can_judge(case):
    e, ref = le.e_ref(case), le.hp_reference(case)
    print("%s e_ref %s" % (case, "  ".join("%s %.3g" % kv for kv in e.items())))
    bars = le.bars(case)                                      # (asserts the cap's condition for every quantity)
    assert all(b <= le.CAP for b in bars.values())
    assert np.all(np.isfinite(ref["grad"].astype(np.float64))) and ref["loo_scale"] > 0 and np.all(ref["kappa"] > 0)
    zero = ref["grad_scale"] == 0                             # an exact zero is asked for exactly where the definition gives one
    want = np.zeros(len(zero), dtype=bool)
    if le.config(case)["N"] == 1:
        want[1:-1] = True
    if le.call_args(case)[5] == 0.0:
        want[-1] = True
    assert np.array_equal(zero, want) and np.all(ref["grad"][zero] == 0)
    j = le.judge(case, le.f64_result(case))                   # the honest f64 restatement passes
    le.show(case, "f64 restatement", j)
    assert j["ok"], j


def test_the_recorded_e_ref():
    """tests/golden/loo_eref.json is the record; a fresh value is at most 4 x the recorded one (more would mean the
    reference, the data or the arithmetic under them changed).  Below 8 u of the scale a value is last-bit noise of the
    BLAS underneath and is compared as 8 u."""
    fresh = {case: le.e_ref(case) for case in le.CASES}
    if os.environ.get("LOO_WRITE") == "1":
        with open(EREF_JSON, "w") as f:
            json.dump(dict(unit="fraction of the quantity's scale (tests/loo_reference_hp.py); resid, sigma, lpd, length_scale: the worst entry",
                           cases=fresh), f, indent=1, sort_keys=True)
    rec = _record()["cases"]
    assert sorted(rec) == sorted(fresh)
    floor = 8 * le.U
    for case in fresh:
        for k in le.KEYS:
            assert max(fresh[case][k], floor) <= 4 * max(rec[case][k], floor), (case, k, fresh[case], rec[case])
            assert 10 * max(rec[case][k], le.config(case)["N"] * le.U) <= le.CAP, (case, k)


# ---- (d) the bars have teeth -------------------------------------------------------------------------------------------
def _applies(slip, case):
    """whether the slip changes anything on this case at all"""
    c = le.config(case)
    if slip == "a row chunk dropped":
        return c["N"] > lo.CHUNK                      # one chunk: nothing is "the last of several"
    if slip == "padding rows counted in B":
        return c["N"] % lo.NPAD != 0
    return True


def test_the_bars_reject_the_slips():
    """Every slip of loo_reference_hp.SLIPS, injected into the f64 restatement, is rejected by judge() on every case of
    SLIP_CASES it applies to.  The slips of the gradient's chain (GRAD_ONLY) leave what tgp_loo returns alone, byte for
    byte; "padding rows counted in B" reaches the constant's and the noise entry only (a padding row's K^-1 is the
    identity: it adds -1 to the trace and to the diagonal of the constant's sum), so without noise only the constant's."""
    seen = {slip: 0 for slip in lo.SLIPS}
    for case in SLIP_CASES:
        honest = le.f64_result(case)
        for slip in lo.SLIPS:
            if not _applies(slip, case):
                continue
            res = le.f64_result(case, slip)
            j = le.judge(case, res)
            worst = max(le.KEYS, key=lambda k: j[k]["ratio"])
            print("%s with %s: %.3g of its bar (%s)" % (case, slip, j[worst]["ratio"], worst))
            assert not j["ok"], (case, slip, j)
            if slip in lo.GRAD_ONLY:
                assert le.loo_bytes(res) == le.loo_bytes(honest), (case, slip)
                assert not all(j[k]["ok"] for k in le.GRAD_KEYS), (case, slip, j)
            if slip == "the jitter left out of sigma":
                assert [k for k in le.KEYS if not j[k]["ok"]] == ["sigma"], (case, j)
            seen[slip] += 1
    assert all(n >= 2 for n in seen.values()), seen


# ---- (e) the host backend ------------------------------------------------------------------------------------------------
def _host_loo(lib_path, case):
    """tgp_loo of a TGP_DEVICE_HOST handle of the library at lib_path, through ctypes alone"""
    import turbo_amd._lib as tl
    lib = ctypes.CDLL(lib_path)
    X, y, kind, c, ls, noise, jitter, norm = le.call_args(case)
    X, y = np.ascontiguousarray(X), np.ascontiguousarray(y)
    ls = np.ascontiguousarray(np.atleast_1d(ls), dtype=np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = lambda a: a.ctypes.data_as(dp)
    h = ctypes.c_void_p()
    assert lib.tgp_create(tl.DEVICE_HOST, tl.F64, ctypes.byref(h)) == tl.OK
    try:
        n = len(y)
        out = dict(resid=np.zeros(n), sigma=np.zeros(n), lpd=np.zeros(n))
        loo = ctypes.c_double()
        assert lib.tgp_loo(h, None, None, None, None) == tl.NOT_FITTED
        rc = lib.tgp_fit(h, ptr(X), ctypes.c_int64(n), ctypes.c_int64(X.shape[1]), ptr(y), tl.KERNELS[kind], ctypes.c_double(c),
                         ptr(ls), ctypes.c_int64(len(ls)), ctypes.c_double(noise), ctypes.c_double(jitter), 1 if norm else 0, None, None, None)
        assert rc == tl.OK
        assert lib.tgp_loo(h, None, None, None, None) == tl.OK          # all-NULL outputs
        assert lib.tgp_loo(h, ptr(out["resid"]), ptr(out["sigma"]), ptr(out["lpd"]), ctypes.byref(loo)) == tl.OK
        out["loo"] = loo.value
        return out
    finally:
        lib.tgp_destroy(h)


@pytest.mark.parametrize("case", HOST_CASES)
def test_the_host_backend_meets_the_bars(case):
    import turbo_amd as ta
    gp = ta.NativeGP(ta._lib.DEVICE_HOST)
    res = le.fit_and_loo(gp, case)
    j = le.judge(case, res, le.LOO_KEYS)
    le.show(case, "host backend", j)
    assert all(np.all(np.isfinite(res[k])) for k in le.LOO_KEYS) and j["ok"], j
    assert le.loo_bytes(gp.loo()) == le.loo_bytes(res)


@pytest.mark.parametrize("case", ["S1/iso", "S3/ard", "D/iso"])
def test_the_host_only_library_meets_the_bars(case):
    import turbo_amd as ta
    res = _host_loo(ta._lib.HOST_LIB_PATH, case)
    j = le.judge(case, res, le.LOO_KEYS)
    le.show(case, "libturbogp_host.so", j)
    assert j["ok"], j
    if not ta._lib.HOST_ONLY:                               # the same source in both libraries: the same bytes
        assert le.loo_bytes(res) == le.loo_bytes(le.fit_and_loo(ta.NativeGP(ta._lib.DEVICE_HOST), case))


# ---- (f) arguments -------------------------------------------------------------------------------------------------------
def test_argument_checks_on_a_host_handle():
    import turbo_amd as ta
    gp = ta.NativeGP(ta._lib.DEVICE_HOST)
    lib = gp.lib
    assert lib.tgp_loo(gp._h, None, None, None, None) == ta._lib.NOT_FITTED
    with pytest.raises(RuntimeError):
        gp.N = 1
        gp.loo()
    args = le.call_args("S3/iso")
    with pytest.raises((ValueError, ta._lib.TurboGPLibraryError)):       # TGP_BAD_ARG on a host handle (GPU only)
        gp.fit_loo_grad(*args)
    if not ta._lib.HOST_ONLY:
        assert b"tgp_fit_loo_grad" in lib.tgp_last_error(gp._h)
    gp.fit(*args)
    assert lib.tgp_loo(gp._h, None, None, None, None) == ta._lib.OK
    only = np.zeros(65)
    assert lib.tgp_loo(gp._h, None, only.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None) == ta._lib.OK
    assert np.array_equal(only, gp.loo()["sigma"])


# ---- (g) ----------------------------------------------------------------------------------------------------------------
def test_host_backend_loo_under_sanitizers(tmp_path):
    """AddressSanitizer + UBSan over HostGP::loo at N = 1, 65 and 257: a stand-alone program, nothing loaded into python"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "turbo_amd", "csrc")
    exe = str(tmp_path / "host_loo_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-pthread", "-I" + csrc, os.path.join(root, "tests", "host_loo_sanitizer_driver.cpp"),
           os.path.join(csrc, "host_backend.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if built.returncode != 0 and ("asan" in built.stderr.lower() or "sanitize" in built.stderr.lower()):
        pytest.skip("this g++ has no sanitizer runtime: " + built.stderr[-200:])
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], env=dict(os.environ, TGP_HOST_THREADS="3"), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
