"""GPU: tgp_hyper_sample on a device handle walks the reference chain on every fit path -- the one-workgroup fit (N = 12), its
two-block path (N = 100) and the blocked fit (N = 300) --, is a pure function of its arguments, and rejects and counts a
proposal whose kernel matrix is not positive definite."""
import math

import numpy as np
import pytest

import hyper_sample_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gp():
    import turbo_amd._lib as L
    g = L.NativeGP(0, "f64")
    yield g
    g.close()


@pytest.mark.parametrize("name", ["gpu_n12", "gpu_n100", "gpu_n300"])
def test_device_handle_walks_the_reference_chain(gp, name):
    c = hc.case(name)
    ref, theta, lml = hc.assert_same_walk(gp, c, S=4, burn=2, thin=1)
    again = hc.native(gp, c, 4, 2, 1)
    assert again[0].tobytes() == theta.tobytes() and again[1].tobytes() == lml.tobytes() and again[2] == ref["evaluations"]
    # the handle is left fitted at the last evaluation, with this problem's shape
    assert gp.N == c["X"].shape[0] and gp.D == c["X"].shape[1]


def test_a_non_pd_proposal_is_rejected_and_counted(gp):
    """jitter 0, no noise term (the noise entry fixed at -inf) and every row duplicated: with the rows duplicated EXACTLY the
    start itself is not positive definite (tests/test_hyper_sample_abi.py has that case), so the copies sit 1e-9 away -- at a
    length scale of 1e-8 the pair is 0.1 apart in scaled units and the matrix is fine, at any length scale above ~1e-2 the
    pair's second pivot has no significant digit left and the fit refuses"""
    rng = np.random.RandomState(5)
    X0 = rng.uniform(0, 1, (8, 1))
    X = np.vstack([X0, X0 + 1e-9])
    y0 = np.sin(4 * X0[:, 0])
    y = np.concatenate([y0, y0])
    lb = np.array([[0.0, 0.0], [math.log(1e-9), math.log(10.0)], [-np.inf, -np.inf]])
    theta0 = np.array([0.0, math.log(1e-8), -np.inf])
    theta, lml, evaluations, not_pd = gp.hyper_sample(X, y, "rbf", theta0, 1, lb, 0.0, True, n_samples=4, burn=1, thin=1,
                                                      width=[1.0, 6.0, 1.0], seed=9)
    print("evaluations %d not_pd %d  log ls %s" % (evaluations, not_pd, theta[:, 1]))
    assert not_pd > 0 and evaluations > not_pd
    assert np.all(np.isfinite(lml)) and np.all(theta[:, 1] >= lb[1, 0]) and np.all(theta[:, 1] <= lb[1, 1])
    assert np.all(theta[:, 0] == 0.0) and np.all(np.isneginf(theta[:, 2]))
    # every kept sample is a point the fit accepts, with the LML the chain recorded
    for t, f in zip(theta, lml):
        got = gp.fit(X, y, "rbf", 1.0, math.exp(t[1]), 0.0, 0.0, True)[0]
        assert abs(got - f) <= 1e-9 * abs(f)
    # a start that is not positive definite is handed back
    with pytest.raises(np.linalg.LinAlgError, match="theta0"):
        gp.hyper_sample(X, y, "rbf", np.array([0.0, 0.0, -np.inf]), 1, lb, 0.0, True, n_samples=2, burn=0, thin=1, seed=9)
