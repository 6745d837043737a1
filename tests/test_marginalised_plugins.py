"""The marginalised plugin classes: MarginalisedHipGPSurrogate -> EI -> CandidateSweep picks the integrated reference's point,
the gradient stage's value and gradient are the mean of the samples' closed forms (GPU), a pickled model predicts the mixture's
moments where no GPU is visible, and what works on ONE fitted model refuses a mixture (CPU)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import integrated_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _branin(X):
    x1, x2 = 15.0 * X[:, 0] - 5.0, 15.0 * X[:, 1]
    return (x2 - 5.1 / (4 * math.pi ** 2) * x1 ** 2 + 5 / math.pi * x1 - 6) ** 2 + 10 * (1 - 1 / (8 * math.pi)) * np.cos(x1) + 10


def _data(n=20, seed=3):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (n, 2))
    return X, _branin(X)


def _kernel(ta):
    return ta.GPKernel("matern52", 1.0, 0.5, 1e-3, bounds=dict(constant=(1e-2, 1e2), length_scale=(5e-2, 1e1), noise=(1e-5, 1e-1)))


def _candidates(n, seed):
    """the batch CandidateSweep's default random_selector draws after np.random.seed(seed): a column per parameter"""
    np.random.seed(seed)
    return np.hstack([np.random.uniform(0.0, 1.0, size=(n, 1)) for _ in range(2)])


# ---------------------------------------------------------------------------------------------------- GPU


@pytest.fixture(scope="module")
def fitted():
    import turbo_amd as ta
    X, y = _data()
    # (fixed point estimate: the chain then starts at the kernel's own values, whatever the optimiser would have found)
    sur = ta.MarginalisedHipGPSurrogate(model_params=dict(kernel=_kernel(ta), normalize_y=True, optimizer=None),
                                        training_iterations=1, n_hyper_samples=6, burn=5, thin=2, hyper_seed=17)
    model, info = sur.construct_model(0, X, y)
    return ta, sur, model, info, X, y


@pytest.mark.gpu
def test_surrogate_ei_candidate_sweep_picks_the_references_point(fitted):
    ta, sur, model, info, X, y = fitted
    assert isinstance(model, ta.MarginalisedModel) and model.thetas.shape == (6, 3)
    assert info["hyper_samples"].shape == (6, 3) and info["evaluations"] > 6 and info["not_pd"] >= 0
    Xc = _candidates(1000, 3)      # (seed picked on the CPU -- the host handle walks the same chain -- for a clear winner)
    ref = ir.integrated(X, y, "matern52", model.thetas, 1, 1e-10, True, Xc, "ei", -1.0, float(y.min()), 0.01)
    acq, _ = ta.EI(0.01).construct_function(0, model, "min", float(y.min()))
    # the single-sweep tolerances of tests/test_gpu_parity.py at the samples' largest constant + noise
    kss = float(np.exp(model.thetas[:, 0]).max() + np.exp(model.thetas[:, -1]).max())
    s_floor = math.sqrt(1e-9 * kss) * float(np.std(y))
    tol = 4 * s_floor + 1e-9 * max(1.0, ref["best_val"])
    np.testing.assert_allclose(acq(Xc), ref["acq"], rtol=1e-5, atol=tol)
    mu, sg = model.predict(Xc, return_std_dev=True)
    np.testing.assert_allclose(mu, ref["mu"], rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(sg ** 2, ref["sigma"] ** 2, rtol=1e-5, atol=s_floor ** 2)
    assert ref["gap"] > 100 * (tol + 1e-5 * ref["best_val"]), "the reference's winner must lead clearly"
    from turbo_amd.bounds import Bounds
    lb = Bounds([("a", 0.0, 1.0), ("b", 0.0, 1.0)])
    np.random.seed(3)                       # the sweep draws the same 1000 candidates
    x, minfo = ta.CandidateSweep(num_random=1000)(lb, acq)
    np.testing.assert_array_equal(x, Xc[ref["best_idx"]].reshape(1, 2))
    assert minfo["max_acq"] == pytest.approx(ref["best_val"], rel=1e-5)
    # the sharded sweep's hook: the winner record is attached for a mixture too, and the integrated sweep packs it
    import torch
    rec = acq.winner_record(7000)
    bi, bv = acq.maximise(Xc)
    sur._context().winner_wait(None)
    torch.cuda.synchronize()
    got = rec.cpu().numpy()
    assert bi == ref["best_idx"] and got[0] == bv and got[1] == 7000 + bi
    np.testing.assert_array_equal(got[2:], Xc[bi])
    sur._context().set_winner_out(None)
    # a second trial starts its chain at this trial's last sample; with the optimiser on, the parent's fit runs first
    model2, info2 = sur.construct_model(1, X, y)
    assert info2["hyper_seed"] != info["hyper_seed"] and model2.thetas.shape == (6, 3)
    opt = ta.MarginalisedHipGPSurrogate(model_params=dict(kernel=_kernel(ta), normalize_y=True), training_iterations=2,
                                        n_hyper_samples=3, burn=2, thin=1, hyper_seed=1)
    model3, info3 = opt.construct_model(0, X, y)
    assert info3["lml_evaluations"] > 0 and model3.thetas.shape == (3, 3)
    lo, hi = _kernel(ta).theta_bounds[:, 0], _kernel(ta).theta_bounds[:, 1]
    assert np.all(model3.thetas >= lo) and np.all(model3.thetas <= hi)


@pytest.mark.gpu
def test_gradient_stage_value_and_gradient(fitted):
    ta, sur, model, info, X, y = fitted
    acq, _ = ta.EI(0.01).construct_function(0, model, "min", float(y.min()))
    rng = np.random.RandomState(1)
    Xq = rng.uniform(0.05, 0.95, (5, 2))

    def ref_value(P):
        return ir.integrated(X, y, "matern52", model.thetas, 1, 1e-10, True, P, "ei", -1.0, float(y.min()), 0.01)["acq"]

    v, g = acq.value_and_grad(Xq)
    want = ref_value(Xq)
    np.testing.assert_allclose(v, want, rtol=1e-8, atol=1e-8 * np.abs(want).max())
    # The issue's rule, ENTRY BY ENTRY: |g - fd| <= 1e-5 |fd| with fd the central difference of the reference's value at step
    # 1e-6 (tests/test_gpu_round3.py / test_gpu_round4.py hold no finite-difference check to take other figures from; the one
    # in tests/test_gpu_parity.py differentiates the library's own value at rtol 2e-4).  A purely relative bound cannot hold
    # for an entry near zero, so each entry also gets the finite difference's OWN error as an absolute term, estimated on the
    # reference alone: |fd(h) - fd(2h)| (truncation of either step and the rounding noise of the oracle's value divided by h).
    h = 1e-6

    def central(i, d, step):
        e = np.zeros(2)
        e[d] = step
        return (ref_value(Xq[i:i + 1] + e)[0] - ref_value(Xq[i:i + 1] - e)[0]) / (2 * step)

    for i in range(Xq.shape[0]):
        for d in range(2):
            fd, fd2 = central(i, d, h), central(i, d, 2 * h)
            own = abs(fd - fd2)
            print("point %d dim %d: g %.9g fd %.9g |g - fd| %.3g  rel %.3g  fd's own error %.3g" % (
                i, d, g[i, d], fd, abs(g[i, d] - fd), abs(g[i, d] - fd) / max(abs(fd), 1e-300), own))
            assert abs(g[i, d] - fd) <= 1e-5 * abs(fd) + own, (i, d, g[i, d], fd, own)
    # the stage itself: SciPy driven, never worse than the sweep it starts from
    from turbo_amd.bounds import Bounds
    lb = Bounds([("a", 0.0, 1.0), ("b", 0.0, 1.0)])
    np.random.seed(2)
    x0, i0 = ta.CandidateSweep(num_random=200)(lb, acq)
    np.random.seed(2)
    x1, i1 = ta.RandomAndQuasiNewton(num_random=200, grad_restarts=3, start_from_best=2)(lb, acq)
    assert i1["max_acq"] >= i0["max_acq"] - 1e-12
    assert i1["max_acq"] == pytest.approx(ref_value(x1)[0], rel=1e-5)      # (the single-sweep tolerance: the winner may be a swept candidate)
    with pytest.raises(ValueError, match="on_device"):
        ta.RandomAndQuasiNewton(num_random=50, grad_restarts=2, start_from_best=1, on_device=True)(lb, acq)
    # the gradient stage's contexts are the factory's: a second model refits them, it does not add to them
    assert len(sur._grad_handles) == 6 and sur._grad_owner is model
    before = [id(gp) for gp in sur._grad_handles]
    model2, _ = sur.construct_model(1, X, y)
    acq2, _ = ta.EI(0.01).construct_function(1, model2, "min", float(y.min()))
    v2, _ = acq2.value_and_grad(Xq)
    assert [id(gp) for gp in sur._grad_handles] == before and sur._grad_owner is model2
    want2 = ir.integrated(X, y, "matern52", model2.thetas, 1, 1e-10, True, Xq, "ei", -1.0, float(y.min()), 0.01)["acq"]
    np.testing.assert_allclose(v2, want2, rtol=1e-8, atol=1e-8 * np.abs(want2).max())
    v1, _ = acq.value_and_grad(Xq)                       # ... and the first model gets them back on demand
    np.testing.assert_allclose(v1, v, rtol=0, atol=0)


# ---------------------------------------------------------------------------------------------------- CPU


def _bare_model(ta):
    """a MarginalisedModel over hand-made samples, its factory a MarginalisedHipGPSurrogate from the real constructor (which
    loads the library and creates no GPU context) with a chain state to carry across the pickle"""
    from turbo_amd.surrogates import HipGPSurrogate, MarginalisedModel
    X, y = _data(12, 4)
    factory = ta.MarginalisedHipGPSurrogate(model_params=dict(kernel=_kernel(ta), normalize_y=True, optimizer=None),
                                            training_iterations=1, n_hyper_samples=4, burn=3, thin=2, hyper_seed=11)
    point = HipGPSurrogate.ModelInstance(factory, X, y, _kernel(ta), 1e-10, True)
    rng = np.random.RandomState(0)
    thetas = np.log([1.2, 0.5, 2e-3]) + 0.3 * rng.normal(size=(4, 3))
    factory._last_sample = thetas[-1].copy()
    return MarginalisedModel(factory, point, thetas, np.zeros(4), 1), X, y


_CHILD = r"""
import sys, warnings
import numpy as np, dill
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import integrated_reference as ir
model = dill.load(open(sys.argv[2], "rb"))
Xc = np.random.RandomState(1).uniform(0, 1, (40, 2))
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    mu, sg = model.predict(Xc, return_std_dev=True)
ref = ir.integrated(model.X, model.y, "matern52", model.thetas, 1, 1e-10, True, Xc, "none", 1.0, 0.0, 0.0)
print("max |dmu| %.3g max |dsigma| %.3g" % (np.abs(mu - ref["mu"]).max(), np.abs(sg - ref["sigma"]).max()))
np.testing.assert_allclose(mu, ref["mu"], rtol=0, atol=1e-9)
np.testing.assert_allclose(sg, ref["sigma"], rtol=0, atol=1e-9)
print("ok")
"""


def test_pickled_model_predicts_the_mixture_without_a_gpu(tmp_path):
    import dill
    import turbo_amd as ta
    model, X, y = _bare_model(ta)
    blob = dill.dumps(model)
    assert len(blob) < 20000                                # X, y, kernel, thetas: no factor
    back = dill.loads(blob)
    assert back.thetas.tobytes() == model.thetas.tobytes() and back.X.tobytes() == X.tobytes()
    assert back.point.X is back.X and back.is_marginalised
    f0, f1 = model._factory, back._factory
    assert type(f1) is ta.MarginalisedHipGPSurrogate and f1._reloaded and back.point._factory is f1
    assert (f1.n_hyper_samples, f1.burn, f1.thin, f1.hyper_seed) == (4, 3, 2, 11)
    assert f1._last_sample.tobytes() == f0._last_sample.tobytes() and f1._grad_handles == [] and f1._grad_owner is None
    path = tmp_path / "model.dill"
    path.write_bytes(blob)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    run = subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(path)], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().splitlines()[-1] == "ok", run.stdout + run.stderr


def test_what_needs_one_fitted_model_refuses_a_mixture():
    import turbo_amd as ta
    from turbo_amd.bounds import Bounds
    model, X, y = _bare_model(ta)
    lb = Bounds([("a", 0.0, 1.0), ("b", 0.0, 1.0)])
    ei, _ = ta.EI(0.01).construct_function(0, model, "min", float(y.min()))
    assert ei.get_name() == "EI"
    for fac in (ta.UCB(2.0), ):
        f, _ = fac.construct_function(0, model, "min")
        assert f.model is model
    with pytest.raises(ValueError, match="marginalised"):
        ta.CandidateSweep(num_random=10).select_batch(lb, ei, 2)
    with pytest.raises(ValueError, match="marginalised"):
        ta.TS(seed=1).construct_function(0, model, "min")
    with pytest.raises(ValueError, match="marginalised"):
        ta.MES(n_samples=4, seed=1).construct_function(0, model, "min")
    with pytest.raises(ValueError, match="on_device"):
        ta.CandidateSweep(num_random=10, grad_restarts=2, start_from_best=1, on_device=True)(lb, ei)
    for call in (lambda: ei.maximise_topk(np.zeros((4, 2)), 2), lambda: ei.maximise_batch(np.zeros((4, 2)), 2),
                 lambda: ei.refine(np.zeros((1, 2)), [(0, 1), (0, 1)]), lambda: ei.lbfgsb(np.zeros((1, 2)), [(0, 1), (0, 1)])):
        with pytest.raises(ValueError, match="marginalised"):
            call()
    with pytest.raises(ValueError):
        ta.MarginalisedHipGPSurrogate.__init__(ta.MarginalisedHipGPSurrogate.__new__(ta.MarginalisedHipGPSurrogate),
                                               n_hyper_samples=65)


def test_gradient_contexts_belong_to_the_factory_and_do_not_multiply(monkeypatch):
    """every model of a factory shares the factory's S gradient contexts: two models alive do not double them, a model with
    more samples grows them to its S, close() releases them.  (A counting stand-in for the GPU context: no device needed.)"""
    import turbo_amd as ta
    from turbo_amd import surrogates
    from turbo_amd.surrogates import MarginalisedModel
    live, fits = [], []

    class FakeGP:
        host = False

        def __init__(self, device, dtype):
            assert dtype == "f64"
            live.append(self)

        def fit(self, X, y, kind, c, ls, noise, jitter, normalize_y):
            self.theta = (c, float(np.atleast_1d(ls)[0]), noise)
            fits.append(self)
            return 0.0, 0.0, 1.0

        def acq_grad(self, X, acq, sf, incumbent, param):
            X = np.atleast_2d(X)
            return np.full(X.shape[0], self.theta[0]), np.full(X.shape, self.theta[1])

        def close(self):
            live.remove(self)

    monkeypatch.setattr(surrogates._lib, "NativeGP", FakeGP)
    m1, X, y = _bare_model(ta)
    factory = m1._factory
    monkeypatch.setattr(factory, "_context", lambda: FakeGP.__new__(FakeGP))
    m2 = MarginalisedModel(factory, m1.point, m1.thetas[:3] + 0.1, np.zeros(3), 1)
    Xq = np.zeros((2, 2))
    v1, g1 = m1.value_and_grad(Xq, 3, -1.0, 0.0, 0.01)
    assert len(live) == 4 and len(fits) == 4
    np.testing.assert_allclose(v1, np.exp(m1.thetas[:, 0]).mean())
    np.testing.assert_allclose(g1, np.exp(m1.thetas[:, 1]).mean())
    m1.value_and_grad(Xq, 3, -1.0, 0.0, 0.01)
    assert len(fits) == 4                                   # fitted once per model, not per call
    v2, _ = m2.value_and_grad(Xq, 3, -1.0, 0.0, 0.01)
    assert len(live) == 4 and len(fits) == 7                # the second model refits three of the same four contexts
    np.testing.assert_allclose(v2, np.exp(m2.thetas[:, 0]).mean())
    m1.value_and_grad(Xq, 3, -1.0, 0.0, 0.01)
    assert len(live) == 4 and len(fits) == 11
    factory.close()
    assert live == [] and factory._grad_handles == [] and factory._grad_owner is None
