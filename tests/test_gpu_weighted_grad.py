"""GPU: tgp_weighted_grad and tgp_weighted_lbfgsb -- the weighted value and its gradient with respect to the query point --
against the 80-bit closed form (tests/weighted_reference.py::grad fed from tests/acq_grad_reference_hp.py's long double
posteriors), entry by entry within 64 max(e_ref, N u) of the entry's sum of absolute terms (the rule of
tests/test_gpu_acq_grad_edges.py with the sides' terms in the sum; e_ref: tests/golden/weighted_grad_eref.json), against
tgp_sweep_weighted's value, and against SciPy's L-BFGS-B.  Every figure is printed before it is asserted."""
import faulthandler
import json
import os

import numpy as np
import pytest

import kg_grad_cases as gc
import weighted_cases as wc
import weighted_reference as wr

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN, "weighted_grad_eref.json")) as _f:
    E_REF = json.load(_f)["cases"]
with open(os.path.join(GOLDEN, "weighted_eref.json")) as _f:
    E_REF_LOGPHI = float(json.load(_f)["e_ref"])


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


def _grad(h, sides, p, X=None):
    return h.weighted_grad(p["Xc"] if X is None else X, sides, p["acq"], p["sf"], p["incumbent"], p["param"])


@pytest.mark.parametrize("name", list(wc.GRAD_CASES))
def test_value_and_gradient_against_the_80_bit_form(L, name):
    p = wc.problem(name)
    h, sides = wc.handles(L, name)
    val, grad = _grad(h, sides, p)
    ev, eg = wc.grad_errors(name, val, grad)
    bar_g, bar_v = wc.grad_bar(name, E_REF[name]["grad"]), wc.grad_bar(name, E_REF[name]["value"])
    print("%s: value %.3g (bar %.3g), gradient %.3g of the entry's sum of absolute terms (bar %.3g, e_ref %.3g)"
          % (name, ev, bar_v, eg, bar_g, E_REF[name]["grad"]))
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
    assert eg <= bar_g
    if p["acq"] == wr.ACQ_NONE:          # (logw is a sum with its own absolute scale: sum_k (1 + |log f_k|), as in the sweep's tier)
        rv = wc.grad_references(name)[0]
        assert np.all(np.abs(val - rv.astype(np.float64)) <= bar_v * (len(sides) + np.abs(rv.astype(np.float64))))
    else:
        assert ev <= bar_v
    # the same bits from run to run
    v2, g2 = _grad(h, sides, p)
    assert v2.tobytes() == val.tobytes() and g2.tobytes() == grad.tobytes()
    if name.endswith("_underflow"):
        assert val.max() < -745.0 and np.abs(grad).max() > 1.0       # a feasibility of 1e-400 and more, a finite slope
    wc.close(h, sides)


@pytest.mark.parametrize("name", ["g200_k2_m7", "g300_k8_m64", "g200_k2_m7_none", "g200_k1_m7_underflow"])
def test_val_against_the_sweep(L, name):
    """rows of the batch passed as Xq on f64 handles: val equals tgp_sweep_weighted's value_out within the pure-function
    bound of tests/weighted_reference.py"""
    p = wc.problem(name)
    h, sides = wc.handles(L, name)
    r = h.sweep_weighted(sides, p["acq"], p["sf"], p["incumbent"], p["param"], want_logw=True, want_value=True, want_sides=True)
    val, _ = _grad(h, sides, p)
    logf = np.stack([wr.side_logf(k, lv, r["side_mu"][j], r["side_sigma"][j]) for j, (_, k, lv) in enumerate(sides)])
    bar = wr.bound(logf, E_REF_LOGPHI)
    tol = bar if p["acq"] == wr.ACQ_NONE else np.abs(r["value"]) * (bar + 4 * wr.U)
    err = np.abs(val - r["value"])
    print("%s: max |val - value_out| / bound %.3g (max err %.3g)" % (name, float((err / np.maximum(tol, wr.TINY)).max()), err.max()))
    assert np.all(err <= tol)
    wc.close(h, sides)


def test_a_points_bits_depend_neither_on_m_nor_on_its_row(L):
    name = "g300_k8_m64"
    p = wc.problem(name)
    h, sides = wc.handles(L, name)
    X = p["Xc"]
    v, g = _grad(h, sides, p)
    for m in (1, 7, 17):
        vm, gm = _grad(h, sides, p, X[:m])
        assert vm.tobytes() == v[:m].tobytes() and gm.tobytes() == g[:m].tobytes(), m
    vt, gt = _grad(h, sides, p, X[-16:])                             # the last 16 rows as rows 0 .. 15
    assert vt.tobytes() == v[-16:].tobytes() and gt.tobytes() == g[-16:].tobytes()
    perm = np.random.RandomState(0).permutation(X.shape[0])
    vp, gp_ = _grad(h, sides, p, X[perm])
    assert vp.tobytes() == v[perm].tobytes() and gp_.tobytes() == g[perm].tobytes()
    for i in (0, 33, 63):
        v1, g1 = _grad(h, sides, p, X[i:i + 1])
        assert v1[0] == v[i] and g1[0].tobytes() == g[i].tobytes()
    wc.close(h, sides)


def test_sides_on_private_streams_return_the_same_bits(L):
    """the events that order a private stream behind the query points and in front of the combination: a one-workgroup, a
    one-launch and a general side on private streams return the bits of the shared-stream handles"""
    name = "g300_k8_m64"
    p = wc.problem(name)
    h, sides = wc.handles(L, name)
    v, g = _grad(h, sides, p)
    h2, sides2 = wc.handles(L, name, private=(0, 2, 6))              # N = 12, 200 and 300
    for _ in range(3):                                               # (a grown workspace, then warm ones)
        v2, g2 = _grad(h2, sides2, p)
        assert v2.tobytes() == v.tobytes() and g2.tobytes() == g.tobytes()
    wc.close(h, sides)
    wc.close(h2, sides2)


def _lbfgsb_problem():
    """a 2-D problem whose weighted EI and its gradient are well above L-BFGS-B's pgtol at every start: a rough objective
    model (length scale 0.12 under 40 points of 10 |x - 0.3|^2) and a GE side that cuts the unconstrained optimum off"""
    rng = np.random.RandomState(11)
    X = rng.uniform(0, 1, (40, 2))
    y = 10.0 * ((X - 0.3) ** 2).sum(1) + 0.01 * rng.normal(size=40)
    Xk = rng.uniform(0, 1, (30, 2))
    yk = Xk[:, 0] + Xk[:, 1] + 0.01 * rng.normal(size=30)
    starts = np.ascontiguousarray(rng.uniform(0.35, 0.65, (5, 2)))
    return X, y, Xk, yk, starts


LBFGSB_OBJ = ("rbf", 1.0, [0.12], 1e-3)
LBFGSB_SIDE = ("matern52", 1.0, [0.7], 1e-3)


def test_lbfgsb_against_scipy(L):
    """five starts on a 2-D problem: the same x, value, status and evaluation count as SciPy's L-BFGS-B on -value driven
    through tgp_weighted_grad one start at a time, to the tolerance tests/test_gpu_kg_grad.py holds tgp_kg_lbfgsb to
    (kg_grad_cases.LBFGSB_TOL: points 1e-9, values 1e-12 of max(1, |value|)).  On the NumPy reference first: every start
    takes several iterations, so the walk itself is what is compared."""
    import scipy.optimize
    import acq_grad_reference_hp as ah
    from oracle import gp_oracle as o
    X, y, Xk, yk, starts = _lbfgsb_problem()
    lo, hi = np.zeros(2), np.ones(2)
    om = o.fit(X, y, LBFGSB_OBJ[0], LBFGSB_OBJ[1], LBFGSB_OBJ[2], LBFGSB_OBJ[3], 1e-10, True)
    sm = o.fit(Xk, yk, LBFGSB_SIDE[0], LBFGSB_SIDE[1], LBFGSB_SIDE[2], LBFGSB_SIDE[3], 1e-10, True)

    def ref_neg_f(q):
        q = q.reshape(1, -1)
        v, g, _ = wr.grad(wr.ACQ_EI, -1.0, float(y.min()), 0.01, ah.posterior_f64(om, q), [(wr.GE, 0.9, ah.posterior_f64(sm, q))])
        return -float(v[0]), -g[0]
    ref_walks = [scipy.optimize.minimize(ref_neg_f, s, jac=True, bounds=list(zip(lo, hi)), method="L-BFGS-B", options=dict(maxiter=15000))
                 for s in starts]
    print("reference walks: iterations %s, evaluations %s" % ([r.nit for r in ref_walks], [r.nfev for r in ref_walks]))
    assert all(r.success and r.nit > 3 and r.nfev > r.nit for r in ref_walks)
    h = L.NativeGP(0, "f64")
    h.fit(X, y, LBFGSB_OBJ[0], LBFGSB_OBJ[1], LBFGSB_OBJ[2], LBFGSB_OBJ[3], 1e-10, True)
    g = L.NativeGP(0, "f64")
    g.fit(Xk, yk, LBFGSB_SIDE[0], LBFGSB_SIDE[1], LBFGSB_SIDE[2], LBFGSB_SIDE[3], 1e-10, True)
    sides = [(g, "ge", 0.9)]                                         # the unconstrained optimum (0.3, 0.3) is cut off
    kw = dict(acq=L.ACQ_EI, sf=-1.0, incumbent=float(y.min()), param=0.01)
    x, v, st, ev = h.weighted_lbfgsb(starts, lo, hi, sides, **kw)
    vx, _ = h.weighted_grad(x, sides, **kw)
    v0, _ = h.weighted_grad(starts, sides, **kw)
    print("weighted L-BFGS-B: %s -> %s, status %s, %d evaluations" % (v0, v, st, ev))
    assert vx.tobytes() == v.tobytes() and np.all(v > v0) and np.all(x >= lo) and np.all(x <= hi)
    total = 0
    for j in range(5):
        def neg_f(q):
            val, gr = h.weighted_grad(q.reshape(1, -1), sides, **kw)
            return -float(val[0]), -gr[0]
        ref = scipy.optimize.minimize(neg_f, starts[j], jac=True, bounds=list(zip(lo, hi)), method="L-BFGS-B", options=dict(maxiter=15000))
        dx, dv = float(np.abs(x[j] - ref.x).max()), abs(v[j] + ref.fun) / max(1.0, abs(ref.fun))
        print("    start %d: |x - scipy| %.3g, value %.17g (scipy %.17g, %d iterations, %d evaluations; reference walk %.6g)"
              % (j, dx, v[j], -ref.fun, ref.nit, ref.nfev, -ref_walks[j].fun))
        assert ref.nit > 3
        assert (st[j] == 1) == bool(ref.success), (j, st[j], ref.message)
        assert dx <= gc.LBFGSB_TOL[0] and dv <= gc.LBFGSB_TOL[1], (j, dx, dv)
        total += ref.nfev
    assert ev == total
    with pytest.raises(ValueError):
        h.weighted_lbfgsb(starts, hi, lo, sides, **kw)               # lo > hi
    with pytest.raises(ValueError, match="max_iter"):
        h.weighted_lbfgsb(starts, lo, hi, sides, max_iter=0, **kw)
    with pytest.raises(ValueError, match="acquisition"):
        h.weighted_lbfgsb(starts, lo, hi, sides, acq=L.ACQ_UCB, sf=-1.0)
    g.close()
    h.close()
