"""GPU: ``ta.Constrained`` through ``CandidateSweep`` and ``RandomAndQuasiNewton`` on a 2-D toy -- a quadratic objective whose
unconstrained optimum an LE constraint cuts off, N = 30 observations, 1000 candidates, five gradient restarts.  Every fact
about the selection is first asserted on the NumPy reference (tests/weighted_reference.py over the oracle's posteriors), so
the inputs are known to discriminate."""
import faulthandler
import warnings

import numpy as np
import pytest

import weighted_reference as wr
from oracle import gp_oracle as o

pytestmark = pytest.mark.gpu
N, M = 30, 1000
KERNEL = ("rbf", 1.0, 0.5, 1e-4)
LEVEL = 0.0


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _factory(ta):
    return ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel(*KERNEL), normalize_y=True, optimizer=None), training_iterations=1)


def _toy():
    rng = np.random.RandomState(21)
    X = rng.uniform(0, 1, (N, 2))
    y = ((X - 0.3) ** 2).sum(1)                       # the unconstrained optimum: (0.3, 0.3)
    c = 0.9 - X.sum(1)                                # feasible where c <= 0: x0 + x1 >= 0.9, which cuts it off
    Xc = rng.uniform(0, 1, (M, 2))
    return X, y, c, Xc


def _oracle(X, v):
    return o.fit(X, v, KERNEL[0], KERNEL[1], KERNEL[2], KERNEL[3], 1e-10, True)


def _pof(side_model, x):
    mu, sg = o.predict(side_model, np.atleast_2d(x))
    return float(np.exp(wr.side_logf(wr.LE, LEVEL, mu, sg))[0])


def _build(ta, X, y, side_values, kind="le", level=LEVEL, cost=None):
    model, _ = _factory(ta).construct_model(0, X, y)
    acq = ta.Constrained(ta.EI(0.01), constraints=[ta.Constraint("c", _factory(ta), kind, level)] if side_values is not None else [],
                         cost=ta.Cost(_factory(ta), source="seconds") if cost is not None else None)
    for t in range(X.shape[0]):
        info = {}
        if side_values is not None:
            info["c"] = float(side_values[t])
        if cost is not None:
            info["seconds"] = float(cost[t])
        acq.evaluation_started(t)
        acq.evaluation_finished(t, float(y[t]), info)
    inst, info = acq.construct_function(0, model, "min", float(y.min()))
    return model, acq, inst, info


def test_the_selection_is_feasible_where_plain_ei_is_not():
    import turbo_amd as ta
    X, y, c, Xc = _toy()
    feas = c <= LEVEL
    om, sm = _oracle(X, y), _oracle(X, c)
    # on the reference first: plain EI picks an infeasible candidate, the weighted value a feasible one
    mu, sg = o.predict(om, Xc)
    smu, ssg = o.predict(sm, Xc)
    plain = wr.sweep(wr.ACQ_EI, -1.0, float(y.min()), 0.01, mu, sg, [])
    ref = wr.sweep(wr.ACQ_EI, -1.0, float(y[feas].min()), 0.01, mu, sg, [(wr.LE, LEVEL, smu, ssg)])
    assert feas.any() and y[feas].min() > y.min()
    assert _pof(sm, Xc[plain["best_idx"]]) < 0.5 and _pof(sm, Xc[ref["best_idx"]]) >= 0.5
    model, acq, inst, info = _build(ta, X, y, c)
    assert info["n_feasible"] == int(feas.sum()) and info["feasible_incumbent"] == y[feas].min() and inst.acq == wr.ACQ_EI
    # the instance itself over the same batch
    vals = inst(Xc)
    i, v = inst.maximise(Xc)
    assert (i, v) == wr.argmax(vals) and _pof(sm, Xc[i]) >= 0.5
    np.testing.assert_allclose(vals, ref["value"], rtol=1e-4, atol=1e-9 * max(1.0, float(np.abs(ref["value"]).max())))
    # value_and_grad is the sweep's value and has a slope
    vg, gg = inst.value_and_grad(Xc[:7])
    np.testing.assert_allclose(vg, vals[:7], rtol=1e-9, atol=1e-300)
    assert np.all(np.isfinite(gg)) and np.abs(gg).max() > 0
    bounds = ta.Bounds([("a", 0.0, 1.0), ("b", 0.0, 1.0)])
    plain_inst, _ = ta.EI(0.01).construct_function(0, model, "min", float(y.min()))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for aux in (ta.CandidateSweep(num_random=M, grad_restarts=5, start_from_best=0),
                    ta.RandomAndQuasiNewton(num_random=M, grad_restarts=5, start_from_best=2)):
            np.random.seed(5)
            x, minfo = aux(bounds, inst)
            np.random.seed(5)
            xp, _ = aux(bounds, plain_inst)
            print("%s: constrained -> %s (PoF %.3f, value %.4g), plain EI -> %s (PoF %.3f)" % (
                type(aux).__name__, x, _pof(sm, x), minfo["max_acq"], xp, _pof(sm, xp)))
            assert _pof(sm, x) >= 0.5 and _pof(sm, xp) < 0.5
            assert "gradient_evaluations" in minfo           # the in-library L-BFGS-B ran (tgp_weighted_lbfgsb)
            assert minfo["max_acq"] >= v * (1 - 1e-9) or aux.num_random != M
    for call in (lambda: inst.maximise_batch(Xc, 2), lambda: inst.refine(Xc[:2], [(0, 1), (0, 1)]), lambda: inst.winner_record(0)):
        with pytest.raises(NotImplementedError, match="Constrained"):
            call()
    with pytest.raises(AttributeError, match="Constrained"):
        inst.maximise_topk(Xc, 2)


def test_no_feasible_trial_maximises_the_log_feasibility():
    import turbo_amd as ta
    X, y, c, Xc = _toy()
    level = float(c.min() - 0.5)                      # no observed value is <= level
    sm = _oracle(X, c)
    smu, ssg = o.predict(sm, Xc)
    ref = wr.sweep(wr.ACQ_NONE, -1.0, 0.0, 0.0, np.zeros(M), np.ones(M), [(wr.LE, level, smu, ssg)])
    srt = np.sort(ref["logw"])
    assert srt[-1] - srt[-2] > 1e-3 * abs(srt[-1])    # on the reference: a winner that leads clearly
    model, acq, inst, info = _build(ta, X, y, c, level=level)
    assert info["n_feasible"] == 0 and info["feasible_incumbent"] is None and inst.acq == wr.ACQ_NONE
    vals = inst(Xc)
    i, v = inst.maximise(Xc)
    print("no feasible trial: arg-max of logw %d (reference %d), logw %.6g (reference %.6g)" % (i, ref["best_idx"], v, ref["best_val"]))
    assert i == ref["best_idx"] and (i, v) == wr.argmax(vals)
    np.testing.assert_allclose(vals, ref["logw"], rtol=1e-4, atol=1e-6)


def test_a_cost_moves_the_winner_to_the_cheap_side():
    """an objective symmetric about x0 = 0.5 observed at mirrored points: EI is symmetric, so the mirrored candidate batch
    has two equal maxima; a cost that grows with x0 picks the left one"""
    import turbo_amd as ta
    rng = np.random.RandomState(8)
    half = rng.uniform(0, 1, (N // 2, 2)) * [0.5, 1.0]
    X = np.vstack([half, np.column_stack([1.0 - half[:, 0], half[:, 1]])])
    y = (np.abs(X[:, 0] - 0.5) - 0.25) ** 2 + (X[:, 1] - 0.5) ** 2
    seconds = np.exp(2.0 * X[:, 0])                   # log cost = 2 x0: cheap on the left
    ch = rng.uniform(0, 1, (M // 2, 2)) * [0.5, 1.0]
    Xc = np.vstack([np.column_stack([1.0 - ch[:, 0], ch[:, 1]]), ch])     # the right-hand copies first: they win ties
    om, cm = _oracle(X, y), _oracle(X, np.log(seconds))
    mu, sg = o.predict(om, Xc)
    cmu, csg = o.predict(cm, Xc)
    plain = wr.sweep(wr.ACQ_EI, -1.0, float(y.min()), 0.01, mu, sg, [])
    ref = wr.sweep(wr.ACQ_EI, -1.0, float(y.min()), 0.01, mu, sg, [(wr.COST, 0.0, cmu, csg)])
    # on the reference first: EI is symmetric to rounding, and the cost decides for the left
    np.testing.assert_allclose(plain["value"][:M // 2], plain["value"][M // 2:], rtol=1e-6, atol=1e-12)
    assert Xc[ref["best_idx"], 0] < 0.5 and ref["best_idx"] >= M // 2
    mirror = ref["best_idx"] - M // 2
    assert ref["value"][ref["best_idx"]] > 1.5 * ref["value"][mirror]
    model, acq, inst, info = _build(ta, X, y, None, cost=seconds)
    assert set(info["side_fitting_info"]) == {"cost"} and info["n_feasible"] == N
    i, v = inst.maximise(Xc)
    ip, _ = ta.EI(0.01).construct_function(0, model, "min", float(y.min()))[0].maximise(Xc)
    print("cost: weighted winner %d at x0 = %.3f (reference %d), plain EI winner %d at x0 = %.3f" % (i, Xc[i, 0], ref["best_idx"], ip, Xc[ip, 0]))
    assert i == ref["best_idx"] and Xc[i, 0] < 0.5
    assert inst(Xc)[i] > 1.5 * inst(Xc)[mirror]
