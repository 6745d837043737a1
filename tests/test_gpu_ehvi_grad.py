"""GPU: tgp_ehvi_grad and tgp_ehvi_lbfgsb -- the expected hypervolume improvement and its gradient with respect to the
query point -- against the 80-bit closed form (tests/ehvi_reference.py::grad fed from tests/acq_grad_reference_hp.py's long
double posteriors), entry by entry within 64 max(e_ref, N u) of the entry's sum of absolute terms (the rule of
tests/test_gpu_acq_grad_edges.py; e_ref: per case the f64 NumPy restatement's own error and H's, tests/golden/ehvi_eref.json), and against tgp_sweep_ehvi's value, bit for bit on
f64 handles.  Problems: tests/ehvi_cases.py.  Every figure is printed before it is asserted."""
import faulthandler
import json
import os

import numpy as np
import pytest

import ehvi_cases as ec
import ehvi_reference as er

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ehvi_eref.json")) as _f:
    _golden = json.load(_f)
E_REF, E_REF_GRAD = float(_golden["e_ref"]), _golden["grad"]


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def L():
    import turbo_amd._lib as lib
    return lib


@pytest.mark.parametrize("name", list(ec.GRAD_CASES))
def test_value_and_gradient_against_the_80_bit_form(L, name):
    p = ec.problem(name)
    h, g = ec.handles(L, name)
    val, grad = h.ehvi_grad(p["Xc"], g)
    rv = ec.grad_references(name)[0]
    N = max(p["X1"].shape[0], p["X2"].shape[0])
    e_ref = max(E_REF, float(E_REF_GRAD[name]))
    bar = er.FACTOR * max(e_ref, N * er.U)
    eg = ec.grad_error(name, grad)
    ev = float((np.abs(val.astype(er.LD) - rv) / np.maximum(np.abs(rv), er.LD(er.TINY))).max())
    print("%s: value %.3g relative to the 80-bit value (printed only: the value's own statement is the sweep's bits, below), gradient %.3g of the entry's sum of absolute terms (bar %.3g, e_ref %.3g); |grad| max %.3g"
          % (name, ev, eg, bar, e_ref, float(np.abs(grad).max())))
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    assert eg <= bar                  # (f32 handles too: the fit and the query kernels are f64 whatever the sweep's dtype)
    # the same bits from run to run
    v2, g2 = h.ehvi_grad(p["Xc"], g)
    assert v2.tobytes() == val.tobytes() and g2.tobytes() == grad.tobytes()
    # bit for bit tgp_sweep_ehvi's value for the same rows where both sweeps run in f64
    if p["dtypes"] == ("f64", "f64"):
        h.set_candidates(p["Xc"])
        r = h.sweep_ehvi(g, want_value=True)
        assert r["value"].tobytes() == val.tobytes()
    g.close()
    h.close()


def test_a_points_bits_depend_neither_on_m_nor_on_its_row(L):
    name = "g300x1000_d6_m64_p256"
    p = ec.problem(name)
    h, g = ec.handles(L, name, candidates=False)
    X = p["Xc"]
    v, gr = h.ehvi_grad(X, g)
    for m in (1, 3, 17):
        vm, gm = h.ehvi_grad(X[:m], g)
        assert vm.tobytes() == v[:m].tobytes() and gm.tobytes() == gr[:m].tobytes(), m
    vt, gt = h.ehvi_grad(X[-16:], g)                                  # the last 16 rows as rows 0 .. 15
    assert vt.tobytes() == v[-16:].tobytes() and gt.tobytes() == gr[-16:].tobytes()
    perm = np.random.RandomState(0).permutation(X.shape[0])
    vp, gp_ = h.ehvi_grad(X[perm], g)
    assert vp.tobytes() == v[perm].tobytes() and gp_.tobytes() == gr[perm].tobytes()
    # a private stream on the second objective: the same bits
    g.set_private_stream(True)
    for _ in range(2):
        v2, g2 = h.ehvi_grad(X, g)
        assert v2.tobytes() == v.tobytes() and g2.tobytes() == gr.tobytes()
    g.close()
    h.close()


def test_the_resident_batches_are_not_touched_and_degenerate_points(L):
    name = "g300x30_d6_m64_p2"
    p = ec.problem(name)
    h, g = ec.handles(L, name)
    other = np.random.RandomState(1).uniform(0, 1, (40, p["D"]))
    g.set_candidates(other)
    before = h.sweep(L.ACQ_EI, 1.0, 0.1, 0.01, want_acq=True)
    X = p["Xc"].copy()
    X[5] = np.nan
    val, grad = h.ehvi_grad(X, g)
    assert np.isnan(val[5]) and np.isnan(grad[5]).all() and np.isfinite(np.delete(grad, 5, 0)).all()
    assert np.array_equal(h.read_candidates(), p["Xc"]) and np.array_equal(g.read_candidates(), other)
    after = h.sweep(L.ACQ_EI, 1.0, 0.1, 0.01, want_acq=True)
    assert after["acq"].tobytes() == before["acq"].tobytes()
    g.close()
    h.close()


def test_lbfgsb(L):
    """a 2-D problem with a three-point front: no restart ends below its start, a flat region returns the start, the
    argument checks are tgp_acq_lbfgsb's"""
    rng = np.random.RandomState(11)
    X = rng.uniform(0, 1, (40, 2))
    ya = -10.0 * ((X - 0.3) ** 2).sum(1) + 0.01 * rng.normal(size=40)
    yb = -10.0 * ((X - 0.7) ** 2).sum(1) + 0.01 * rng.normal(size=40)
    h, g = L.NativeGP(0, "f64"), L.NativeGP(0, "f64")
    h.fit(X, ya, "rbf", 1.0, [0.25], 1e-3, 1e-10, True)
    g.fit(X, yb, "matern52", 1.0, [0.5], 1e-3, 1e-10, True)
    Y = np.stack([ya, yb], 1)
    ref = er.default_ref(Y, (1.0, 1.0))
    front, hv = h.ehvi_set_front(Y, ref, (1.0, 1.0))
    F, raw, _, rhv = er.front(Y, (1.0, 1.0), ref)
    assert front.tolist() == raw.tolist() and abs(hv - rhv) <= 64 * er.U * rhv
    starts = np.ascontiguousarray(rng.uniform(0.2, 0.8, (6, 2)))
    lo, hi = np.zeros(2), np.ones(2)
    v0, g0 = h.ehvi_grad(starts, g)
    x, v, st, ev = h.ehvi_lbfgsb(starts, lo, hi, g)
    vx, _ = h.ehvi_grad(x, g)
    print("EHVI L-BFGS-B: %s -> %s, status %s, %d evaluations (front of %d)" % (v0, v, st, ev, front.shape[0]))
    assert vx.tobytes() == v.tobytes() and np.all(v >= v0) and np.any(v > v0) and np.all(x >= lo) and np.all(x <= hi) and ev >= 6
    assert set(st.tolist()) <= {0, 1, 2}
    # a flat region: the reference point 60 deviations above everything the first model can reach -- value and gradient are
    # exact zeros, the walk returns its start
    h.ehvi_set_front(np.zeros((0, 2)), (float(ya.max()) + 100.0, float(ref[1])), (1.0, 1.0))
    x, v, st, ev = h.ehvi_lbfgsb(starts, lo, hi, g)
    print("flat: values %s status %s evaluations %d" % (v, st, ev))
    assert np.array_equal(x, starts) and not v.any()
    h.ehvi_set_front(Y, ref, (1.0, 1.0))
    with pytest.raises(ValueError):
        h.ehvi_lbfgsb(starts, hi, lo, g)                              # lo > hi
    with pytest.raises(ValueError, match="max_iter"):
        h.ehvi_lbfgsb(starts, lo, hi, g, max_iter=0)
    dp = lambda a: a.ctypes.data_as(L._dp)
    assert h.lib.tgp_ehvi_lbfgsb(h._h, g._h, dp(starts), 0, dp(lo), dp(hi), 10, dp(x), dp(v), None, None) == 2
    assert h.lib.tgp_ehvi_lbfgsb(h._h, g._h, dp(starts), 3, dp(lo), dp(hi), 10, None, dp(v), None, None) == 2
    assert h.lib.tgp_ehvi_lbfgsb(h._h, h._h, dp(starts), 3, dp(lo), dp(hi), 10, dp(x), dp(v), None, None) == 2
    x2, v2, _, _ = h.ehvi_lbfgsb(np.array([[5.0, 5.0], [-3.0, -3.0]]), lo, hi, g)      # starts outside the box are clipped
    assert np.all(x2 >= lo) and np.all(x2 <= hi)
    x1, v1, st1, ev1 = h.ehvi_lbfgsb(starts, lo, hi, g, max_iter=1)
    assert np.all(v1 >= v0)
    g.close()
    h.close()
