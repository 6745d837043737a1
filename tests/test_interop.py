"""Interoperability with models / selectors that are not this package's (CPU):

  * ta.EI / PI / UCB with a FOREIGN model fall back to ``model.predict`` + the formula in NumPy, as the
    reference's factories work with any ``Surrogate.ModelInstance``
    (turbo/modules/acquisition_functions.py:147-158, :225-247, :336-358) -- held to the acquisition vectors the
    reference itself produced (tests/golden/*.npz);
  * ``LHS_selector`` without a device seed gives the reference's points for the same seed (one construction, no hand-over)."""
import numpy as np
import pytest

import turbo_amd as ta
from conftest import golden_path


class _StoredPosterior:
    """a foreign Surrogate.ModelInstance: answers predict() from the reference's recorded mu / sigma"""

    def __init__(self, case):
        self.case = case

    def predict(self, X, return_std_dev=False):
        assert X is self.case["Xc"]
        return (self.case["mus"], self.case["sigmas"]) if return_std_dev else self.case["mus"]


def test_foreign_model_falls_back_to_predict_and_matches_the_reference(golden_case):
    m = _StoredPosterior(golden_case)
    Xc = golden_case["Xc"]
    for ext in ("min", "max"):
        inc = float(golden_case["incumbent_" + ext])
        for key, factory, args in (("ei", ta.EI(0.01), (inc,)), ("pi", ta.PI(0.01), (inc,)),
                                   ("ucb2", ta.UCB(2.0), ()), ("ucbinf", ta.UCB(float("inf")), ())):
            f, _ = factory.construct_function(3, m, ext, *args)
            assert f.get_name() == str(golden_case["name_%s_%s" % (key, ext)])
            want = golden_case["acq_%s_%s" % (key, ext)]
            got = f(Xc)
            assert got.shape == want.shape and got.dtype == np.float64
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300)
            i, v = f.maximise(Xc)
            assert v == want.max() and i == int(np.flatnonzero(want == want.max())[0])


def test_foreign_model_zero_sigma_nan_and_gpu_only_calls():
    class M:
        def predict(self, X, return_std_dev=False):
            return X[:, 0].copy(), np.abs(X[:, 1])
    X = np.random.RandomState(0).normal(size=(12, 2))
    X[3, 1] = 0.0
    X[5, 0] = np.nan
    for factory in (ta.EI(0.01), ta.PI(0.01)):
        f, _ = factory.construct_function(0, M(), "min", 0.1)
        v = f(X)
        assert v[3] == 0.0 and np.isnan(v[5])
        i, best = f.maximise(X)
        assert i != 5 and best == np.nanmax(v)
    for name, args in (("maximise_topk", (X, 3)), ("refine", (X, [(0, 1)] * 2)), ("value_and_grad", (X,)),
                       ("maximise_generated", (10, [0, 0], [1, 1], 1)), ("winner_record", (0,))):
        with pytest.raises(TypeError, match="GPU only"):
            getattr(f, name)(*args)
    with pytest.raises(TypeError, match="GPU only"):
        f.lbfgsb(X, [(0, 1)] * 2)
    with pytest.raises(AssertionError):
        ta.EI(0.01).construct_function(0, object(), "min", 0.0)


def test_gradient_stage_over_a_foreign_model_uses_finite_differences_like_the_reference():
    """CandidateSweep(grad_restarts > 0) with one of our acquisition instances over a foreign model: no closed-form
    gradient, no library optimiser -- SciPy's L-BFGS-B over 1-point calls differentiated by finite differences, the
    reference's own gradient stage (turbo/modules/auxiliary_optimisers.py:80-99), whatever `lockstep` / `on_device` say"""
    class Bowl:
        def predict(self, X, return_std_dev=False):
            mu = ((X - 0.3) ** 2).sum(1)
            return (mu, np.full(len(X), 0.1)) if return_std_dev else mu
    bounds = ta.Bounds([("a", 0.0, 1.0), ("b", 0.0, 1.0)]) if hasattr(ta, "Bounds") else None
    if bounds is None:
        pytest.skip("no Bounds stand-in")
    f, _ = ta.UCB(0.0).construct_function(0, Bowl(), "min")      # -LCB with beta = 0: maximise -mu
    for kw in (dict(), dict(lockstep="scipy"), dict(lockstep=False), dict(on_device=True)):
        np.random.seed(3)
        x, info = ta.CandidateSweep(num_random=50, grad_restarts=3, start_from_best=1, **kw)(bounds, f)
        np.testing.assert_allclose(x, [[0.3, 0.3]], atol=1e-5)
        assert abs(info["max_acq"]) < 1e-9


def test_lhs_selector_host_design_is_a_latin_hypercube():
    b = ta.Bounds([("a", 0.0, 1.0), ("b", -5.0, 10.0), ("c", 3.0, 4.0)])
    lo, hi = np.array([0.0, -5.0, 3.0]), np.array([1.0, 10.0, 4.0])
    np.random.seed(5)
    sel = ta.LHS_selector(num_total=16)
    pts = np.vstack([sel(6, b), sel(10, b)])
    with pytest.raises(AssertionError):
        sel(1, b)
    strata = np.floor((pts - lo) / (hi - lo) * 16).astype(int)
    assert all(sorted(strata[:, d].tolist()) == list(range(16)) for d in range(3))


def test_lhs_selector_host_design_is_the_references_for_the_same_seed():
    """held to the reference's own LHS_selector(9)(9, bounds) after np.random.seed(3) and the three np.random.rand
    numbers that follow it, recorded in tests/golden/lhs_selector_seed3.npz"""
    import dill
    with np.load(golden_path("lhs_selector_seed3"), allow_pickle=False) as z:
        want, rand_after = z["design"], z["rand_after"]
    b = ta.Bounds([("a", 0.0, 1.0), ("b", -5.0, 10.0)])
    np.random.seed(3)
    sel = ta.LHS_selector(9)
    first = sel(4, b)
    sel = dill.loads(dill.dumps(sel))
    rest = sel(5, b)
    assert np.array_equal(np.vstack([first, rest]), want) and sel.index == 9
    assert not hasattr(sel, "_delegate")     # one construction everywhere: nothing is handed over
    assert np.array_equal(np.random.rand(3), rand_after)     # the RNG is left where the reference leaves it
