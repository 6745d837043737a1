"""CPU: the input warp's references judged, and the HOST backend's tgp_warp_points / tgp_warp_inverse (through
libturbogp_host.so) held to them, on the grid of tests/warp_reference.py:
 (a) the f64 NumPy restatement against mpmath at 50 digits; its worst errors are the e_ref of the GPU test's bars, recorded in
     tests/golden/warp_eref.json (written where WARP_WRITE=1);
 (b) the host backend against mpmath at 64 max(e_ref, u): absolute for w, relative to max(|value|, the smallest normal) for
     the derivatives; an infinite dw/du matched exactly;
 (c) exact endpoints, the exact identity at a = b = 1, monotonicity in u on adjacent doubles, the round trip through the
     inverse; the argument checks answer TGP_BAD_ARG;
 (d) the stand-alone sanitizer driver (tests/host_warp_sanitizer_driver.cpp: ASan + UBSan, nothing loaded into python)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import warp_reference as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EREF_JSON = os.path.join(ROOT, "tests", "golden", "warp_eref.json")
KEYS = ("w", "dw_du", "dw_da", "dw_db")
_dp = ctypes.POINTER(ctypes.c_double)


def _recorded():
    with open(EREF_JSON) as f:
        return json.load(f)["e_ref"]


def _grid_arrays():
    g = np.array(wr.GRID, dtype=np.float64)
    return g[:, 0].copy(), g[:, 1].copy(), g[:, 2].copy()


def _worst(got):
    """{key: worst error over the grid} of got = four arrays over the grid"""
    worst = dict.fromkeys(KEYS, 0.0)
    for k, (u, a, b) in enumerate(wr.GRID):
        for key, e in zip(KEYS, wr.errors(u, a, b, [x[k] for x in got])):
            worst[key] = max(worst[key], e)
    return worst


class HostLib:
    """libturbogp_host.so loaded on its own (the library a machine without ROCm has) and one TGP_DEVICE_HOST handle"""

    def __init__(self):
        import __graft_entry__ as g
        from turbo_amd import _lib
        if not os.path.exists(_lib.HOST_LIB_PATH):
            g.build()
        self.lib = ctypes.CDLL(_lib.HOST_LIB_PATH)
        self.h = ctypes.c_void_p()
        assert self.lib.tgp_create(-1, 0, ctypes.byref(self.h)) == 0
        self.lib.tgp_warp_points.argtypes = [ctypes.c_void_p, _dp, ctypes.c_int64, ctypes.c_int64] + [_dp] * 8
        self.lib.tgp_warp_inverse.argtypes = [ctypes.c_void_p, _dp, ctypes.c_int64, ctypes.c_int64] + [_dp] * 5

    @staticmethod
    def _p(a):
        return None if a is None else a.ctypes.data_as(_dp)

    def warp(self, u, a, b, lo=0.0, hi=1.0, derivatives=True):
        """every grid point as a one-dimensional, one-row problem of its own: (rc, [w, du, da, db])"""
        n = len(u)
        out = [np.full(n, np.nan) for _ in range(4)]
        rc = 0
        for k in range(n):
            x, l, h, aa, bb = (np.array([v], dtype=np.float64) for v in (u[k], lo, hi, a[k], b[k]))
            o = [np.zeros(1) for _ in range(4)]
            rc |= self.lib.tgp_warp_points(self.h, self._p(x), 1, 1, self._p(l), self._p(h), self._p(aa), self._p(bb), self._p(o[0]),
                                           *[self._p(v) if derivatives else None for v in o[1:]])
            for j in range(4):
                out[j][k] = o[j][0]
        return rc, out

    def inverse(self, w, a, b):
        out = np.full(len(w), np.nan)
        for k in range(len(w)):
            x, l, h, aa, bb, o = (np.array([v], dtype=np.float64) for v in (w[k], 0.0, 1.0, a[k], b[k], 0.0))
            assert self.lib.tgp_warp_inverse(self.h, self._p(x), 1, 1, self._p(l), self._p(h), self._p(aa), self._p(bb), self._p(o)) == 0
            out[k] = o[0]
        return out


@pytest.fixture(scope="module")
def host():
    return HostLib()


def test_the_restatement_against_mpmath_and_the_recorded_e_ref():
    """the f64 restatement's worst errors over the grid are the record; a fresh value is at most 4 x the recorded one (a
    value below 8 u is compared as 8 u), and the record is small enough to judge with: 64 e_ref <= 1e-9"""
    u, a, b = _grid_arrays()
    fresh = _worst(wr.warp_f64(u, a, b))
    if os.environ.get("WARP_WRITE") == "1":
        with open(EREF_JSON, "w") as f:
            json.dump(dict(unit="worst error of tests/warp_reference.py's f64 restatement over its GRID against mpmath (50 digits): w absolute, the derivatives relative to max(|value|, the smallest normal double)",
                           e_ref=fresh), f, indent=1, sort_keys=True)
    rec = _recorded()
    for key in KEYS:
        print("%s: e_ref %.3g (recorded %.3g)" % (key, fresh[key], rec[key]))
        assert max(fresh[key], 8 * wr.U) <= 4 * max(rec[key], 8 * wr.U), key
        assert 64 * rec[key] <= 1e-9, key


def test_the_host_backend_against_mpmath(host):
    u, a, b = _grid_arrays()
    rc, got = host.warp(u, a, b)
    assert rc == 0
    worst, rec = _worst(got), _recorded()
    for key in KEYS:
        bar = 64 * max(rec[key], wr.U)
        print("%s: host %.3g (bar %.3g, e_ref %.3g)" % (key, worst[key], bar, rec[key]))
        assert worst[key] <= bar, (key, worst[key], bar)
    rc, alone = host.warp(u, a, b, derivatives=False)
    assert rc == 0 and alone[0].tobytes() == got[0].tobytes()          # w does not depend on what else is asked for


@pytest.mark.parametrize("which", ["restatement", "host"])
def test_endpoints_identity_and_monotonicity(which, host):
    u, a, b = _grid_arrays()
    f = (lambda uu: wr.warp_f64(np.clip(uu, 0.0, 1.0), a, b)) if which == "restatement" else (lambda uu: host.warp(uu, a, b)[1])
    w, du, da, db = f(u)
    assert np.all(w[u == 0] == 0) and not np.any(np.signbit(w[u == 0])) and np.all(w[u == 1] == 1)
    assert np.all(da[(u == 0) | (u == 1)] == 0) and np.all(db[(u == 0) | (u == 1)] == 0)
    ident = (a == 1) & (b == 1)
    assert w[ident].tobytes() == u[ident].tobytes() and np.all(du[ident] == 1)
    assert np.all((w >= 0) & (w <= 1)) and np.all(du >= 0) and np.all(da <= 0) and np.all(db >= 0)
    up = np.nextafter(u, 2.0)
    inside = up <= 1.0
    w_up = f(np.where(inside, up, 1.0))[0]
    assert np.all(w_up[inside] >= w[inside]), [wr.GRID[k] for k in np.nonzero(inside & (w_up < w))[0]]
    # outside the box the point is clipped
    assert f(np.full_like(u, -3.0))[0].max() == 0 and f(np.full_like(u, 7.0))[0].min() == 1


@pytest.mark.parametrize("which", ["restatement", "host"])
def test_the_round_trip_through_the_inverse(which, host):
    """u -> w -> u' -> w': the inverse carries at least the rounding of its result, u' (1 +- u), which the warp maps to
    |dw/du| u' u of w; so w' is within 64 u max(1, dw/du u') of w (the factor as everywhere), and the ends are exact"""
    u, a, b = _grid_arrays()
    if which == "restatement":
        w = wr.warp_f64(u, a, b)[0]
        back = wr.inverse_f64(w, a, b)
        w2, du2 = wr.warp_f64(back, a, b)[:2]
    else:
        w = host.warp(u, a, b)[1][0]
        back = host.inverse(w, a, b)
        w2, du2 = host.warp(back, a, b)[1][:2]
    assert np.all((back >= 0) & (back <= 1)) and np.all(back[w == 0] == 0) and np.all(back[w == 1] == 1)
    for k in range(len(u)):
        want = float(wr.inverse_mp(w[k], a[k], b[k]))
        assert abs(back[k] - want) <= 64 * wr.U * max(want, wr.TINY) * max(1.0, abs(np.log(max(want, wr.TINY)))) or want < 1e-290, (wr.GRID[k], back[k], want)
    with np.errstate(invalid="ignore"):
        slope = np.where(np.isfinite(du2), du2 * back, 1.0)
    assert np.all(np.abs(w2 - w) <= 64 * wr.U * np.maximum(1.0, slope)), np.abs(w2 - w).max()


def test_the_argument_checks(host):
    one, u = np.array([1.0]), np.array([0.5])
    for lo, hi, a, b in [(1.0, 1.0, 1.0, 1.0), (0.0, np.inf, 1.0, 1.0), (0.0, 1.0, 0.0, 1.0), (0.0, 1.0, 1.0, -1.0), (0.0, 1.0, np.nan, 1.0), (0.0, 1.0, 1.0, np.inf)]:
        rc, _ = host.warp(u, np.array([a]), np.array([b]), lo=lo, hi=hi)
        assert rc == 2, (lo, hi, a, b)
    p = host._p
    assert host.lib.tgp_warp_points(host.h, p(u), 0, 1, p(one * 0), p(one), p(one), p(one), p(one.copy()), None, None, None) == 2
    assert host.lib.tgp_warp_points(host.h, None, 1, 1, p(one * 0), p(one), p(one), p(one), p(one.copy()), None, None, None) == 2
    assert host.lib.tgp_warp_inverse(host.h, p(u), 1, 1, p(one), p(one), p(one), p(one), p(one.copy())) == 2


def test_host_warp_under_sanitizers(tmp_path):
    """AddressSanitizer + UBSan over the host warp and its inverse: a stand-alone program, nothing loaded into python"""
    csrc = os.path.join(ROOT, "turbo_amd", "csrc")
    exe = str(tmp_path / "host_warp_san")
    san = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-pthread"]
    probe = tmp_path / "probe.cpp"           # "no sanitizer runtime" is decided on a program of its own: a compile error in the
    probe.write_text("int main() { return 0; }\n")      # code under test is a failure, never a skip
    probed = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True, timeout=300)
    if probed.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime: " + probed.stderr[-200:])
    cmd = ["g++"] + san + ["-I" + csrc, os.path.join(ROOT, "tests", "host_warp_sanitizer_driver.cpp"), os.path.join(csrc, "host_backend.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert built.returncode == 0, built.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ERROR" not in run.stderr and "runtime error" not in run.stderr, run.stdout[-2000:] + run.stderr[-3000:]
    assert run.stdout.strip().splitlines()[-1] == "ok", run.stdout
