"""CPU, build container only: ``ta.Constrained`` -- acquisition factory and listener in one -- under the UNMODIFIED reference
``turbo.Optimiser`` (turbo/optimiser.py:227-357), as tests/test_dropin_reference_optimiser.py runs the other plugins: the
ctypes context is replaced by tests/oracle_context.py's stand-in, here with the three weighted methods answered from
tests/weighted_reference.py.  Under test is the plugin contract: the records per trial, the feasible incumbent handed to
the library, TGP_ACQ_NONE before any feasible trial, acq_info, the dill round trip with the host formula behind it, and
the refusals."""
import os
import sys
import warnings

import numpy as np
import pytest

import weighted_reference as wr
from oracle import gp_oracle as o
from oracle_context import OracleBackedContext

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "turbo")),
                                reason="needs the reference checkout (build container only)")
CALLS = []
KIND = {"ge": wr.GE, "le": wr.LE, "cost": wr.COST}


class WeightedOracleContext(OracleBackedContext):
    """the stand-in with ``sweep_weighted`` / ``weighted_grad`` / ``weighted_lbfgsb`` from the NumPy reference"""

    def _posts(self, sides, X):
        out = []
        for g, kind, level in sides:
            assert g is not self and g.model is not None
            out.append((KIND.get(kind, kind), level) + tuple(o.predict(g.model, X)))
        return out

    def sweep_weighted(self, sides, acq=3, sf=1.0, incumbent=0.0, param=0.0, want_mu=False, want_sigma=False, want_acq=False,
                       want_logw=False, want_value=False, want_sides=False):
        mu, sg = o.predict(self.model, self.Xc)
        r = wr.sweep(acq, sf, incumbent, param, mu, sg, self._posts(sides, self.Xc))
        for g, _, _ in sides:
            g.set_candidates(self.Xc)
        CALLS.append(dict(entry="sweep_weighted", acq=acq, sf=sf, incumbent=incumbent, param=param, K=len(sides), M=len(self.Xc)))
        return dict(mu=mu if want_mu else None, sigma=sg if want_sigma else None, acq=r["acq"] if want_acq else None,
                    logw=r["logw"] if want_logw else None, value=r["value"] if want_value else None, side_mu=None, side_sigma=None,
                    best_idx=r["best_idx"], best_val=r["best_val"], n_clamped=0)

    def weighted_grad(self, Xq, sides, acq=3, sf=1.0, incumbent=0.0, param=0.0):
        import acq_grad_reference_hp as ah
        Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
        obj = ah.posterior_f64(self.model, Xq)
        sd = [(KIND.get(kind, kind), level, ah.posterior_f64(g.model, Xq)) for g, kind, level in sides]
        CALLS.append(dict(entry="weighted_grad", acq=acq, incumbent=incumbent, m=len(Xq)))
        v, g, _ = wr.grad(acq, sf, incumbent, param, obj, sd)
        return v, g

    def weighted_lbfgsb(self, X0, lo, hi, sides, acq=3, sf=1.0, incumbent=0.0, param=0.0, max_iter=15000):
        import scipy.optimize
        X0 = np.atleast_2d(np.asarray(X0, dtype=np.float64))
        CALLS.append(dict(entry="weighted_lbfgsb", acq=acq, incumbent=incumbent, R=len(X0)))
        xs, vs, st, ev = [], [], [], 0
        for x0 in X0:
            def neg_f(q):
                v, g = self.weighted_grad(q.reshape(1, -1), sides, acq, sf, incumbent, param)
                return -float(v[0]), -g[0]
            res = scipy.optimize.minimize(neg_f, np.clip(x0, lo, hi), jac=True, bounds=list(zip(lo, hi)), method="L-BFGS-B",
                                          options=dict(maxiter=max_iter))
            xs.append(res.x); vs.append(-res.fun); st.append(1 if res.success else 0); ev += res.nfev
        return np.array(xs), np.array(vs), np.array(st, dtype=np.int64), ev


@pytest.fixture
def reference(monkeypatch):
    sys.path.insert(0, REF)
    if not hasattr(np, "asscalar"):                      # harness-side shim
        monkeypatch.setattr(np, "asscalar", lambda a: np.asarray(a).item(), raising=False)
    import turbo as tb
    import turbo.modules as tm
    import turbo_amd as ta
    real = (ta._lib.NativeGP, ta._lib.load)
    monkeypatch.setattr(ta._lib, "NativeGP", WeightedOracleContext)
    monkeypatch.setattr(ta._lib, "load", lambda: None)
    del CALLS[:]
    yield tb, tm, ta, real
    sys.path.remove(REF)


def branin(x, y):
    from math import pi
    return float((y - (5.1 / (4 * pi ** 2)) * x ** 2 + 5 * x / pi - 6) ** 2 + 10 * (1 - 1 / (8 * pi)) * np.cos(x) + 10)


def _factory(ta):
    return ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel("matern52", 1.0, 1.0, 1.0), normalize_y=True, optimizer=None),
                             training_iterations=1)


def test_constrained_under_the_unmodified_optimiser(reference, monkeypatch):
    tb, tm, ta, real = reference

    def objective(x, y):
        return branin(x, y), {"xy": float(x * y)}
    np.random.seed(7)
    op = tb.Optimiser(objective, 'min', [('x', -5., 10.), ('y', 0., 15.)], pre_phase_trials=4, settings_preset=None)
    op.latent_space = tm.NoLatentSpace()
    op.pre_phase_select = tm.LHS_selector(num_total=4)
    op.fallback = tm.Fallback(selector=tm.random_selector())
    op.surrogate = _factory(ta)
    acq = ta.Constrained(ta.EI(xi=0.01), constraints=[ta.Constraint("xy", _factory(ta), kind="le", level=40.0)])
    op.acquisition = acq
    op.register_listener(acq)                             # duck-typed: registered / evaluation_finished / ...
    op.aux_optimiser = ta.CandidateSweep(num_random=256, grad_restarts=2, start_from_best=0)
    assert acq.optimiser is op and acq.get_type() == "improvement"
    selected = []

    class Spy(tm.Listener):
        def selection_finished(self, trial_num, x, selection_info):
            selected.append((trial_num, dict(selection_info), len(acq.records)))
    op.register_listener(Spy())
    n_trials = 10
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        op.run(max_trials=n_trials)
    xs, ys = np.vstack(op.rt.trial_xs), np.array(op.rt.trial_ys)
    # one record per trial, in step with the data the models are fitted to
    assert sorted(acq.records) == list(range(n_trials))
    np.testing.assert_allclose([acq.records[t]["xy"] for t in range(n_trials)], xs[:, 0] * xs[:, 1], rtol=1e-12)
    bayes = [s for s in selected if s[1]["type"] != "pre_phase"]
    assert [s[0] for s in bayes] == list(range(4, n_trials))
    sweeps = [c for c in CALLS if c["entry"] == "sweep_weighted"]
    stages = [c for c in CALLS if c["entry"] == "weighted_lbfgsb"]
    assert len(sweeps) == len(bayes) and len(stages) == len(bayes) and all(c["K"] == 1 and c["M"] == 256 for c in sweeps)
    for (t, info, n_rec), call, stage in zip(bayes, sweeps, stages):
        assert n_rec == t                                 # the records the instance was built from: one per row of model.X
        ai = info["acq_info"]
        assert set(ai) == {"xi", "feasible_incumbent", "n_feasible", "side_fitting_info"} and ai["xi"] == 0.01
        assert set(ai["side_fitting_info"]) == {"xy"} and "iterations" in ai["side_fitting_info"]["xy"]
        feas = xs[:t, 0] * xs[:t, 1] <= 40.0
        assert ai["n_feasible"] == int(feas.sum())
        if feas.any():                                    # the incumbent handed to the library: the best FEASIBLE y
            assert ai["feasible_incumbent"] == ys[:t][feas].min()
            assert call["acq"] == wr.ACQ_EI and call["incumbent"] == ys[:t][feas].min() and call["param"] == 0.01 and call["sf"] == -1
            assert stage["acq"] == wr.ACQ_EI and stage["incumbent"] == ys[:t][feas].min() and stage["R"] == 2
        else:
            assert ai["feasible_incumbent"] is None and call["acq"] == wr.ACQ_NONE
        assert "max_acq" in info["maximisation_info"]
    op.unregister_listener(acq)
    assert acq.optimiser is None

    # the dill round trip of an instance, and __call__ on the host formula behind it: no GPU here, so the reloaded models
    # are served by the library's host backend and the instance follows the formula from every model's predict
    import dill
    model = bayes[-1][1]["model"]
    last = acq.records.pop(n_trials - 1)                  # (that model was fitted to the first n_trials - 1 rows)
    inst, _ = acq.construct_function(n_trials, model, "min", float(ys.min()))
    acq.records[n_trials - 1] = last
    blob = dill.dumps(inst)
    monkeypatch.setattr(ta._lib, "NativeGP", real[0])
    monkeypatch.setattr(ta._lib, "load", real[1])
    inst2 = dill.loads(blob)
    grid = np.random.RandomState(0).uniform([-5, 0], [10, 15], size=(50, 2))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = inst2(grid)
        i, v = inst2.maximise(grid)
    assert inst2.get_name() == inst.get_name() and inst2.acq == inst.acq and inst2.incumbent_cost == inst.incumbent_cost
    om = o.fit(model.X, model.y, "matern52", 1.0, 1.0, 1.0, 1e-10, True)
    sm = o.fit(model.X, model.X[:, 0] * model.X[:, 1], "matern52", 1.0, 1.0, 1.0, 1e-10, True)
    a, inc, par = inst._native_args()
    want = wr.sweep(a, -1.0, inc, par, *o.predict(om, grid), [(wr.LE, 40.0) + tuple(o.predict(sm, grid))])
    np.testing.assert_allclose(got, want["value"], rtol=1e-6, atol=1e-12)
    assert i == want["best_idx"] and v == pytest.approx(want["best_val"], rel=1e-6)


def _records(acq, xy, cost=None):
    for t, v in enumerate(xy):
        info = {"xy": float(v)}
        if cost is not None:
            info["seconds"] = float(cost[t])
        acq.evaluation_started(t)
        acq.evaluation_finished(t, 0.0, info)


def test_no_feasible_trial_cost_and_the_refusals(reference):
    tb, tm, ta, real = reference
    rng = np.random.RandomState(3)
    X = rng.uniform(0, 1, (12, 2))
    y = ((X - 0.5) ** 2).sum(1)
    model, _ = _factory(ta).construct_model(0, X, y)
    acq = ta.Constrained(ta.PI(xi=0.02), constraints=[ta.Constraint("xy", _factory(ta), "ge", 5.0)],
                         cost=ta.Cost(_factory(ta), source="seconds"))
    with pytest.raises(ValueError, match="one record per row"):
        acq.construct_function(0, model, "min", float(y.min()))
    _records(acq, X[:, 0] * X[:, 1], cost=1.0 + X[:, 0])            # no trial reaches xy >= 5
    inst, info = acq.construct_function(0, model, "min", float(y.min()))
    assert inst.acq == wr.ACQ_NONE and info["n_feasible"] == 0 and info["feasible_incumbent"] is None
    assert set(info["side_fitting_info"]) == {"xy", "cost"} and inst.get_name() == "feasibility"
    np.testing.assert_allclose([acq.records[t]["cost"] for t in range(12)], np.log(1.0 + X[:, 0]), rtol=1e-15)
    grid = rng.uniform(0, 1, (40, 2))
    i, v = inst.maximise(grid)
    assert CALLS[-1]["acq"] == wr.ACQ_NONE and CALLS[-1]["K"] == 2
    vals = inst(grid)
    assert (i, v) == wr.argmax(vals)
    # the duration source: the wall time since evaluation_started, as its log
    timed = ta.Constrained(ta.EI(0.01), cost=ta.Cost(_factory(ta)))
    timed.evaluation_started(0)
    timed.evaluation_finished(0, 1.0, None)
    assert np.isfinite(timed.records[0]["cost"]) and timed.records[0]["cost"] < 0.0      # far below a second
    with pytest.raises(KeyError, match="evaluation_started"):
        timed.evaluation_finished(1, 1.0, None)
    with pytest.raises(KeyError, match="eval_info"):
        acq.evaluation_finished(12, 0.0, {"seconds": 1.0})
    # refused, each with a text of its own
    for call in (lambda: inst.maximise_batch(grid, 2), lambda: inst.refine(grid[:2], [(0, 1), (0, 1)]), lambda: inst.winner_record(0)):
        with pytest.raises(NotImplementedError, match="Constrained: .* use "):
            call()
    with pytest.raises(AttributeError, match="Constrained: maximise_topk"):
        inst.maximise_topk(grid, 3)
    from turbo_amd.auxiliary_optimisers import _offers
    assert not _offers(inst, "maximise_topk") and _offers(inst, "lbfgsb") and _offers(inst, "value_and_grad")
    assert inst.maximise_host_stream(10, [0, 0], [1, 1], topk=4) is None
    with pytest.raises(TypeError, match="EI or PI"):
        ta.Constrained(ta.UCB(1.0))
    with pytest.raises(ValueError, match="own factory"):
        shared = _factory(ta)
        m2, _ = shared.construct_model(0, X, y)
        bad = ta.Constrained(ta.EI(0.01), constraints=[ta.Constraint("xy", shared, "le", 0.5)])
        _records(bad, X[:, 0] * X[:, 1])
        bad.construct_function(0, m2, "min", float(y.min()))[0].maximise(grid)

    with pytest.raises(ValueError, match="warped"):
        acq.construct_function(0, type("Warped", (), dict(is_warped=True, X=X, y=y))(), "min", 0.0)
    with pytest.raises(ValueError, match="marginalised"):
        acq.construct_function(0, type("Marginalised", (), dict(is_marginalised=True, X=X, y=y))(), "min", 0.0)
