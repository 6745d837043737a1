"""CPU: the two-objective expected hypervolume improvement in the C-ABI (tgp_ehvi_set_front, tgp_sweep_ehvi, tgp_ehvi_grad,
tgp_ehvi_lbfgsb: declared, exported, bound with the header's argument types; absent from the host-only library), every
TGP_BAD_ARG line that can be reached without a device (NULL and host handles), and the front builder (csrc/host_front.hpp)
walked by a stand-alone program under AddressSanitizer + UBSan."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 2   # TGP_BAD_ARG
ENTRIES = ("tgp_ehvi_set_front", "tgp_sweep_ehvi", "tgp_ehvi_grad", "tgp_ehvi_lbfgsb")


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
    ctype_of = {"tgp_handle": c.c_void_p, "const double *": L._dp, "double *": L._dp, "int64_t": c.c_int64, "int64_t *": L._i64p,
                "double": c.c_double, "int": c.c_int}
    for name in ENTRIES:
        assert name in L.SYMBOLS, name
        assert re.search(r"\bT %s\b" % name, nm), name
        want = [ctype_of[re.sub(r"\s*\b\w+$", "", a).strip()] for a in _args_of(h, name)]
        assert getattr(lib, name).argtypes == want, (name, want)
    assert all(hasattr(L.NativeGP, m) for m in ("ehvi_set_front", "sweep_ehvi", "ehvi_grad", "ehvi_lbfgsb"))
    assert int(re.search(r"#define \w+_EHVI_MAX_FRONT (\d+)", h).group(1)) == L.EHVI_MAX_FRONT == 256       # (the header's macro)
    # GPU only: the host-only library does not carry them
    host = subprocess.run(["nm", "-D", "--defined-only", L.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert not re.search(r"\bT tgp_\w*ehvi\w*\b", host)


def test_what_needs_no_device_answers_bad_arg():
    import turbo_amd._lib as L
    gp = L.NativeGP(L.DEVICE_HOST, "f64")
    other = L.NativeGP(L.DEVICE_HOST, "f64")
    rng = np.random.RandomState(0)
    X = rng.uniform(0, 1, (30, 3))
    y = 2.0 + np.sin(3 * X.sum(1))
    for g in (gp, other):
        g.fit(X, y, "matern52", 1.0, 0.6, 1e-3, 1e-10, True)
    gp.set_candidates(X)
    lib, h, g = gp.lib, gp._h, other._h
    dp = lambda a: a.ctypes.data_as(L._dp)
    Xq, val, grad = np.ascontiguousarray(X[:2]), np.zeros(2), np.zeros((2, 3))
    lo, hi = np.zeros(3), np.ones(3)
    Y, ref = np.array([[1.0, 2.0], [2.0, 1.0]]), np.zeros(2)
    for second in (g, None, h):
        # a host objective: every entry, whatever the second handle
        assert lib.tgp_ehvi_set_front(h, dp(Y), 2, 1.0, 1.0, dp(ref), None, None, None) == BAD
        assert b"host backend" in lib.tgp_last_error(h)
        assert lib.tgp_sweep_ehvi(h, second, *([None] * 8)) == BAD
        assert b"host backend" in lib.tgp_last_error(h)
        assert lib.tgp_ehvi_grad(h, second, dp(Xq), 2, dp(val), dp(grad)) == BAD
        assert b"host backend" in lib.tgp_last_error(h)
        assert lib.tgp_ehvi_lbfgsb(h, second, dp(Xq), 2, dp(lo), dp(hi), 10, dp(grad), dp(val), None, None) == BAD
        assert b"host backend" in lib.tgp_last_error(h)
        # no handle at all
        assert lib.tgp_ehvi_set_front(None, dp(Y), 2, 1.0, 1.0, dp(ref), None, None, None) == BAD
        assert lib.tgp_sweep_ehvi(None, second, *([None] * 8)) == BAD
        assert lib.tgp_ehvi_grad(None, second, dp(Xq), 2, dp(val), dp(grad)) == BAD
        assert lib.tgp_ehvi_lbfgsb(None, second, dp(Xq), 2, dp(lo), dp(hi), 10, dp(grad), dp(val), None, None) == BAD
    with pytest.raises(Exception, match="host"):
        gp.ehvi_set_front(Y, ref)
    with pytest.raises(Exception, match="host"):
        gp.sweep_ehvi(other)
    with pytest.raises(Exception, match="host"):
        gp.ehvi_grad(Xq, other)
    with pytest.raises(Exception, match="host"):
        gp.ehvi_lbfgsb(Xq, lo, hi, other)


def test_front_builder_under_sanitizers(tmp_path):
    """AddressSanitizer + UBSan over csrc/host_front.hpp: a stand-alone program, nothing loaded into python"""
    csrc = os.path.join(ROOT, "turbo_amd", "csrc")
    exe = str(tmp_path / "host_front_san")
    san = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.cpp"           # "no sanitizer runtime" is decided on a program of its own: a compile error in the
    probe.write_text("int main() { return 0; }\n")      # code under test is a failure, never a skip
    probed = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if probed.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime: " + probed.stderr[-200:])
    cmd = ["g++"] + san + ["-Wall", "-I" + csrc, os.path.join(ROOT, "tests", "host_front_sanitizer_driver.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
