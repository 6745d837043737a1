"""CPU: ``ta.EHVI`` and ``ta.Objective`` -- acquisition factory and listener in one -- without a device: the records per
trial, the default reference point, acq_info, the refusals, and the NumPy ``__call__`` on foreign models against
tests/ehvi_reference.py.  Where a native model is needed (the shared-factory refusal) the ctypes context is replaced by
tests/oracle_context.py's stand-in, as tests/test_constrained_plugin_host.py does."""
import numpy as np
import pytest

import ehvi_reference as er
from oracle import gp_oracle as o


class Foreign:
    """a model that is not HipGPSurrogate's: X, y and predict from the NumPy oracle"""

    def __init__(self, X, y):
        self.X, self.y = X, y
        self.m = o.fit(X, y, "matern52", 1.0, 0.5, 1e-3, 1e-10, True)

    def predict(self, X, return_std_dev=False):
        mu, sg = o.predict(self.m, np.atleast_2d(X))
        return (mu, sg) if return_std_dev else mu


class ForeignSurrogate:
    def construct_model(self, trial_num, X, y):
        return Foreign(X, y), {"foreign": True}


def _toy(n=14):
    rng = np.random.RandomState(4)
    X = rng.uniform(0, 1, (n, 2))
    return X, X[:, 0] + 0.1 * X[:, 1], 1.0 - np.sqrt(X[:, 0]) + 0.5 * X[:, 1], rng


def _acq(ta, X, y2, ref=None, extremum="min", surrogate=None, name="f2"):
    acq = ta.EHVI(ta.Objective(name, surrogate or ForeignSurrogate(), extremum), ref=ref)
    for t in range(X.shape[0]):
        acq.evaluation_started(t)
        acq.evaluation_finished(t, 0.0, {name: float(y2[t])})
    return acq


def test_records_default_reference_point_and_acq_info():
    import turbo_amd as ta
    X, y1, y2, rng = _toy()
    acq = ta.EHVI(ta.Objective("f2", ForeignSurrogate(), "min"))
    assert acq.get_type() == "optimism"
    marker = object()
    acq.registered(marker)
    assert acq.optimiser is marker
    acq.unregistered()
    assert acq.optimiser is None
    model = Foreign(X, y1)
    with pytest.raises(ValueError, match="one record per row"):
        acq.construct_function(0, model, "min")
    with pytest.raises(KeyError, match="eval_info"):
        acq.evaluation_finished(0, 0.0, {"other": 1.0})
    with pytest.raises(KeyError, match="eval_info"):
        acq.evaluation_finished(0, 0.0, None)
    with pytest.raises(ValueError, match="finite"):
        acq.evaluation_finished(0, 0.0, {"f2": float("nan")})
    for t in np.random.RandomState(0).permutation(len(y2)):          # (any order: the trial number is the key)
        acq.evaluation_finished(int(t), float(y1[t]), {"f2": float(y2[t]), "more": 3})
    assert sorted(acq.records) == list(range(len(y2))) and [acq.records[t] for t in range(len(y2))] == [float(v) for v in y2]
    for ext1, ext2 in (("min", "min"), ("max", "min"), ("min", "max")):
        acq.second.extremum = ext2
        inst, info = acq.construct_function(3, model, ext1)
        sf = (1.0 if ext1 == "max" else -1.0, 1.0 if ext2 == "max" else -1.0)
        Y = np.stack([y1, y2], 1)
        assert set(info) == {"ref", "pareto_front", "pareto_trials", "hypervolume", "second_fitting_info"}
        assert info["second_fitting_info"] == {"foreign": True}
        assert np.array_equal(info["ref"], er.default_ref(Y, sf))
        F, raw, idx, hv = er.front(Y, sf, info["ref"])
        assert info["pareto_front"].tolist() == raw.tolist() and info["pareto_trials"] == idx.tolist()
        assert abs(info["hypervolume"] - hv) <= 64 * er.U * hv
        assert inst.get_name() == "EHVI" and inst.sf == sf
    # a zero range counts as 1.0; an explicit reference point is used as given
    flat = _acq(ta, X[:3], np.full(3, 2.0))
    _, info = flat.construct_function(0, Foreign(X[:3], np.array([1.0, 1.0, 1.0])), "min")
    assert info["ref"].tolist() == [1.1, 2.1] and info["pareto_front"].tolist() == [[1.0, 2.0]] and info["pareto_trials"] == [0]
    given = _acq(ta, X, y2, ref=(5.0, 6.0))
    assert given.construct_function(0, model, "min")[1]["ref"].tolist() == [5.0, 6.0]
    with pytest.raises(ValueError, match="2 finite"):
        ta.EHVI(ta.Objective("f2", ForeignSurrogate()), ref=(1.0, np.inf))
    with pytest.raises(TypeError, match="Objective"):
        ta.EHVI(ForeignSurrogate())
    with pytest.raises(ValueError, match="extremum"):
        ta.Objective("f2", ForeignSurrogate(), "least")


def test_numpy_call_on_foreign_models_follows_the_reference():
    import turbo_amd as ta
    X, y1, y2, rng = _toy()
    model = Foreign(X, y1)
    grid = np.vstack([rng.uniform(-0.2, 1.2, (60, 2)), X[:3]])
    for ext1, ext2 in (("min", "min"), ("max", "min"), ("min", "max"), ("max", "max")):
        acq = _acq(ta, X, y2, extremum=ext2)
        inst, info = acq.construct_function(0, model, ext1)
        sf = inst.sf
        got = inst(grid)
        F, _, _, _ = er.front(np.stack([y1, y2], 1), sf, info["ref"])
        a, c = er.strips(F, np.asarray(sf) * info["ref"])
        m2 = o.fit(X, y2, "matern52", 1.0, 0.5, 1e-3, 1e-10, True)
        ref = er.sweep(a, c, sf, *o.predict(model.m, grid), *o.predict(m2, grid))
        err = np.abs(got - ref["value"])
        bar = 2 * er.bound(ref["scale"], 16 * er.U)
        print("%s/%s: front of %d, max err / bar %.3g" % (ext1, ext2, len(F), float((err / np.maximum(bar, er.TINY)).max())))
        assert np.all(err <= bar) and got.max() > 0
        assert inst.maximise(grid) == er.argmax(got)
        assert inst(np.zeros((0, 2))).shape == (0,)
        assert inst.maximise_host_stream(10, [0, 0], [1, 1]) is None
    # GPU-only routes say so; the refusals have texts of their own
    for call in (lambda: inst.value_and_grad(grid[:2]), lambda: inst.lbfgsb(grid[:2], [(0, 1), (0, 1)]),
                 lambda: inst.maximise_generated(10, [0, 0], [1, 1], 1)):
        with pytest.raises(TypeError, match="EHVI: .* GPU only"):
            call()
    for call in (lambda: inst.maximise_batch(grid, 2), lambda: inst.refine(grid[:2], [(0, 1), (0, 1)]), lambda: inst.winner_record(0)):
        with pytest.raises(NotImplementedError, match="EHVI: .* use "):
            call()
    with pytest.raises(AttributeError, match="EHVI: maximise_topk"):
        inst.maximise_topk(grid, 3)
    from turbo_amd.auxiliary_optimisers import _offers
    assert not _offers(inst, "maximise_topk") and hasattr(inst, "lbfgsb") and hasattr(inst, "value_and_grad")
    assert not _offers(inst, "lbfgsb")                   # (a foreign model: the gradient stage takes finite differences)
    acq = _acq(ta, X, y2)
    with pytest.raises(ValueError, match="warped"):
        acq.construct_function(0, type("Warped", (), dict(is_warped=True, X=X, y=y1))(), "min")
    with pytest.raises(ValueError, match="marginalised"):
        acq.construct_function(0, type("Marginalised", (), dict(is_marginalised=True, X=X, y=y1))(), "min")

    class WarpedSurrogate:
        def construct_model(self, trial_num, X, y):
            return type("Warped", (), dict(is_warped=True, X=X, y=y))(), {}
    with pytest.raises(ValueError, match="warped"):
        _acq(ta, X, y2, surrogate=WarpedSurrogate()).construct_function(0, model, "min")


def test_a_second_objective_on_the_first_ones_factory_is_refused(monkeypatch):
    import turbo_amd as ta
    from oracle_context import OracleBackedContext
    monkeypatch.setattr(ta._lib, "NativeGP", OracleBackedContext)
    monkeypatch.setattr(ta._lib, "load", lambda: None)
    X, y1, y2, rng = _toy()
    shared = ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel("matern52", 1.0, 1.0, 1e-3), normalize_y=True, optimizer=None),
                               training_iterations=1)
    model, _ = shared.construct_model(0, X, y1)
    with pytest.raises(ValueError, match="own factory"):
        _acq(ta, X, y2, surrogate=shared).construct_function(0, model, "min")
