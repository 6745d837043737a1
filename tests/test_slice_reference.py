"""CPU: the NumPy slice sampler of tests/slice_reference.py samples the density it claims to -- exp(LML) on the box -- checked
against quadrature of that same oracle LML on a 1-D problem with one free coordinate."""
import math

import numpy as np

import slice_reference as sr


def _problem():
    rng = np.random.RandomState(4)
    X = rng.uniform(0, 1, (8, 1))
    y = np.sin(5 * X[:, 0]) + 0.1 * rng.normal(size=8)
    return X, y


def _standard_error(z):
    """standard error of mean(z) for a correlated chain: sqrt(var / n * tau) with the integrated autocorrelation time
    tau = 1 + 2 sum_k rho_k, the sum cut by Geyer's initial positive sequence (pairs rho_2k + rho_2k+1 while positive)"""
    z = np.asarray(z, dtype=np.float64)
    n = z.shape[0]
    d = z - z.mean()
    var = float(d @ d) / n
    tau = 1.0
    for k in range(1, n // 4, 2):
        pair = (float(d[:-k] @ d[k:]) + float(d[:-(k + 1)] @ d[k + 1:])) / (n * var)
        if pair <= 0.0:
            break
        tau += 2.0 * pair
    return math.sqrt(var * tau / n), tau


def test_long_chain_matches_quadrature_of_the_same_lml():
    X, y = _problem()
    lml = sr.oracle_lml(X, y, "rbf", 1, 1e-10, True)
    # constant and noise fixed, the length scale free on [log 0.02, log 5]
    lo = np.array([0.0, math.log(0.02), math.log(1e-2)])
    hi = np.array([0.0, math.log(5.0), math.log(1e-2)])
    # posterior mean and variance of the free coordinate by Simpson's rule on the box, from the same LML
    g = np.linspace(lo[1], hi[1], 2001)
    f = np.array([lml(np.array([0.0, t, lo[2]])) for t in g])
    w = np.ones_like(g)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    dens = w * np.exp(f - f.max())
    dens /= dens.sum()
    q_mean = float(dens @ g)
    q_var = float(dens @ (g - q_mean) ** 2)

    S = 4000
    out = sr.slice_sample(lml, np.array([0.0, math.log(0.3), lo[2]]), lo, hi, S, burn=50, thin=1, width=1.0, seed=11)
    assert out["theta"].shape == (S, 3) and out["not_pd"] == 0
    assert np.all(out["theta"][:, 0] == 0.0) and np.all(out["theta"][:, 2] == lo[2])      # fixed entries never move
    t = out["theta"][:, 1]
    assert t.min() >= lo[1] and t.max() <= hi[1]
    np.testing.assert_allclose(out["lml"][-1], lml(out["theta"][-1]), rtol=0, atol=0)
    se_mean, tau_m = _standard_error(t)
    se_var, tau_v = _standard_error((t - t.mean()) ** 2)
    print("quadrature mean %.5f var %.5f | chain mean %.5f +- %.5f (tau %.2f) var %.5f +- %.5f (tau %.2f) | evaluations %d"
          % (q_mean, q_var, t.mean(), se_mean, tau_m, t.var(), se_var, tau_v, out["evaluations"]))
    assert abs(t.mean() - q_mean) <= 4.0 * se_mean
    assert abs(t.var() - q_var) <= 4.0 * se_var


def test_the_walk_is_a_pure_function_of_its_inputs_and_of_the_seed():
    X, y = _problem()
    lml = sr.oracle_lml(X, y, "rbf", 1, 1e-10, True)
    lo = np.log([1e-2, 1e-2, 1e-5])
    hi = np.log([1e2, 1e1, 1.0])
    a = sr.slice_sample(lml, np.log([1.0, 0.3, 1e-2]), lo, hi, 5, 2, 2, seed=3)
    b = sr.slice_sample(lml, np.log([1.0, 0.3, 1e-2]), lo, hi, 5, 2, 2, seed=3)
    c = sr.slice_sample(lml, np.log([1.0, 0.3, 1e-2]), lo, hi, 5, 2, 2, seed=4)
    assert a["theta"].tobytes() == b["theta"].tobytes() and a["evaluations"] == b["evaluations"]
    assert a["theta"].tobytes() != c["theta"].tobytes()
    assert np.all(a["theta"] >= lo) and np.all(a["theta"] <= hi)
    # the first uniforms of the stream are the documented Philox words
    from philox_ref import philox4x32_10
    r = philox4x32_10(0, 0, sr.SLICE_TAG, 0, 3, 0)
    u0 = (float(int(r[0]) >> 5) * 67108864.0 + float(int(r[1]) >> 6)) / 9007199254740992.0
    assert sr.Stream(3).next() == u0
