"""CPU: the constrained / cost-aware acquisition in the C-ABI (tgp_sweep_weighted, tgp_weighted_grad, tgp_weighted_lbfgsb:
declared, exported, bound; the header with its struct still C99) and every TGP_BAD_ARG line that can be reached without a
device: NULL and host handles, K = 9."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = 2   # TGP_BAD_ARG
ENTRIES = ("tgp_sweep_weighted", "tgp_weighted_grad", "tgp_weighted_lbfgsb")


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
    ctype_of = {"tgp_handle": c.c_void_p, "const tgp_side *": c.POINTER(L.Side), "const double *": L._dp, "double *": L._dp,
                "int64_t": c.c_int64, "int64_t *": L._i64p, "double": c.c_double, "int": c.c_int}
    for name in ENTRIES:
        assert name in L.SYMBOLS, name
        assert re.search(r"\bT %s\b" % name, nm), name
        want = [ctype_of[re.sub(r"\s*\b\w+$", "", a).strip()] for a in _args_of(h, name)]
        assert getattr(lib, name).argtypes == want, (name, want)
    assert all(hasattr(L.NativeGP, m) for m in ("sweep_weighted", "weighted_grad", "weighted_lbfgsb"))
    assert (L.SIDE_GE, L.SIDE_LE, L.SIDE_COST) == (0, 1, 2)
    kinds = re.search(r"enum tgp_side_kind \{([^}]*)\};", h).group(1)
    assert [tuple(v.strip().lower() for v in e.split("=")) for e in kinds.split(",")] == \
        [("tgp_side_ge", "0"), ("tgp_side_le", "1"), ("tgp_side_cost", "2")]
    # GPU only: the host-only library does not carry them
    host = subprocess.run(["nm", "-D", "--defined-only", L.HOST_LIB_PATH], stdout=subprocess.PIPE, text=True).stdout
    assert not re.search(r"\bT tgp_(sweep_weighted|weighted_grad|weighted_lbfgsb)\b", host)


def test_the_struct_is_plain_c99(tmp_path):
    """the header compiles as C99 with the struct, whose layout is the one the ctypes binding assumes"""
    import turbo_amd._lib as L
    src = tmp_path / "side.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "turbogp.h"\n'
                   'int main(void) { tgp_side s; s.g = 0; s.kind = (enum tgp_side_kind)2; s.reserved = 0; s.level = 0.0;\n'
                   ' printf("%d %d %d %d %d\\n", (int)sizeof(tgp_side), (int)offsetof(tgp_side, kind), (int)offsetof(tgp_side, reserved),\n'
                   ' (int)offsetof(tgp_side, level), s.kind); return 0; }\n')
    exe = str(tmp_path / "side")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-o", exe])
    out = subprocess.check_output([exe], timeout=60).decode().split()
    assert [int(v) for v in out] == [ctypes.sizeof(L.Side), L.Side.kind.offset, L.Side.reserved.offset, L.Side.level.offset, 2]


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
    lib, h = gp.lib, gp._h
    dp = lambda a: a.ctypes.data_as(L._dp)
    Xq, val, grad = np.ascontiguousarray(X[:2]), np.zeros(2), np.zeros((2, 3))
    lo, hi = np.zeros(3), np.ones(3)
    arr, K = gp._sides([(other, "ge", 0.0)])
    nine = (L.Side * 9)()
    sweep_tail = [None] * 10
    for sides, k in ((arr, K), (None, 0), (nine, 9), (None, 1)):
        # a host objective: every entry, whatever the sides
        assert lib.tgp_sweep_weighted(h, sides, k, L.ACQ_EI, 1.0, 0.0, 0.01, *sweep_tail) == BAD
        assert b"host backend" in lib.tgp_last_error(h)
        assert lib.tgp_weighted_grad(h, sides, k, dp(Xq), 2, L.ACQ_EI, 1.0, 0.0, 0.01, dp(val), dp(grad)) == BAD
        assert b"host backend" in lib.tgp_last_error(h)
        assert lib.tgp_weighted_lbfgsb(h, sides, k, dp(Xq), 2, dp(lo), dp(hi), L.ACQ_EI, 1.0, 0.0, 0.01, 10, dp(grad), dp(val), None, None) == BAD
        assert b"host backend" in lib.tgp_last_error(h)
        # no handle at all
        assert lib.tgp_sweep_weighted(None, sides, k, L.ACQ_EI, 1.0, 0.0, 0.01, *sweep_tail) == BAD
        assert lib.tgp_weighted_grad(None, sides, k, dp(Xq), 2, L.ACQ_EI, 1.0, 0.0, 0.01, dp(val), dp(grad)) == BAD
        assert lib.tgp_weighted_lbfgsb(None, sides, k, dp(Xq), 2, dp(lo), dp(hi), L.ACQ_EI, 1.0, 0.0, 0.01, 10, dp(grad), dp(val), None, None) == BAD
    with pytest.raises(Exception, match="host"):
        gp.sweep_weighted([(other, "ge", 0.0)])
    with pytest.raises(Exception, match="host"):
        gp.weighted_grad(Xq, [])
    with pytest.raises(Exception, match="host"):
        gp.weighted_lbfgsb(Xq, lo, hi, [])
    with pytest.raises(KeyError):
        gp._sides([(other, "between", 0.0)])
