"""CPU: tests/mes_reference.py -- the NumPy / SciPy statement of max-value entropy search the GPU tests compare against
-- is itself held to scipy.stats (the entropy of a truncated normal), to finite differences and to its own rules."""
import numpy as np
import pytest
from scipy import stats

import mes_reference as mr


def test_h_is_the_entropy_lost_by_truncation():
    """h(gamma) = H[N(0,1)] - H[N(0,1) truncated above at gamma], on [-8, 8] at 1e-10"""
    g = np.linspace(-8.0, 8.0, 321)
    # (the lower end at -40 instead of -inf, where scipy's entropy forms -inf * 0: the mass below it is 1e-350)
    want = stats.norm.entropy() - np.array([stats.truncnorm(-40.0, gi).entropy() for gi in g])
    got = mr.h(g)
    assert np.max(np.abs(got - want)) <= 1e-10, float(np.max(np.abs(got - want)))


def test_h_is_positive_and_decreasing():
    g = np.linspace(-35.0, 12.0, 4701)
    v = mr.h(g)
    assert np.all(v >= 0.0)
    assert np.all(np.diff(v) <= 0.0)


def test_dh_matches_central_differences():
    g = np.linspace(-6.0, 6.0, 241)
    e = 1e-5
    fd = (mr.h(g + e) - mr.h(g - e)) / (2 * e)
    _, dh = mr.h_and_dh(g)
    # central differences: e^2 / 6 |h'''| truncation + eps / e rounding, both ~1e-10 against |dh| up to 6
    np.testing.assert_allclose(dh, fd, rtol=1e-8, atol=1e-9)


def test_the_tail_branch_joins_the_erfcx_branch():
    """the expansion of h used below gamma = -50 continues the erfcx route: the series' next term there is 4e2 / 50^8 = 1e-11
    (2.6e-12 of h, measured against the 80-bit reference), the erfcx route's cancellation 50^2 / 2 ulps.  dh/dgamma is the
    continued fraction on both sides of -50 (below -10), so it does not see that seam at all; the form it replaced,
    -(r / 2)(1 + gamma^2 + gamma r), was off by 8.9e-10 of dh at gamma = -49.4 (measured; 50^4 ulps would be 7e-10), and
    the series that served below -50 by 9e-11.  At its own seam, -10, the two forms of dh agree to the cancelling form's
    10^4 ulps.  tests/test_mes_reference_hp.py holds both branches to the 80-bit reference class by class."""
    a, da = mr.h_and_dh(np.array([-50.0]))                   # the erfcx route's last point
    b, db = mr.h_and_dh(np.array([np.nextafter(-50.0, -np.inf)]))
    assert abs(a[0] - b[0]) <= 1e-10
    assert abs(da[0] - db[0]) <= 1e-17                       # (dh = -0.02 there: three of its ulps)
    _, dc = mr.h_and_dh(np.array([mr.DH_SEAM, np.nextafter(mr.DH_SEAM, -np.inf)]))
    assert abs(dc[0] - dc[1]) <= 2e-12 * abs(dc[0])
    g = np.array([-1e4, -1e6, -1e12, -1e150, -1e300])
    v = mr.h(g)
    np.testing.assert_allclose(v, np.log(-g) + 0.5 * np.log(2 * np.pi) - 0.5, rtol=0, atol=1e-7)


def test_finite_at_extreme_arguments():
    g = np.array([-1e308, -1e300, -1e10, -40.0, -38.5, -1000.0, 0.0, 5e-324, 26.0, 37.0, 40.0, 1e10, 1e300, 1e308])
    v, d = mr.h_and_dh(g)
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(d))
    assert v[-1] == 0.0 and v[g == 40.0][0] >= 0.0
    assert v[g == 0.0][0] == pytest.approx(np.log(2.0), abs=1e-15)


def test_mask_where_the_latent_deviation_is_zero():
    mu = np.array([0.0, 1.0, 3.0, 3.0])
    noise, y_std = 0.25, 2.0                                 # noise y_std^2 = 1
    sigma = np.array([1.0, 0.5, np.nextafter(1.0, 2.0), 2.0])
    a = mr.mes(mu, sigma, [3.0, 4.0], 1.0, noise, y_std)
    assert a[0] == 0.0 and a[1] == 0.0 and a[2] > 0.0 and a[3] > 0.0
    a0 = mr.mes(mu, np.array([0.0, 1.0, 0.0, 2.0]), [3.0], 1.0, 0.0, 1.0)     # noise 0: the sigma != 0 mask of EI / PI
    assert a0[0] == 0.0 and a0[2] == 0.0 and a0[1] > 0.0
    _, cm, cs = mr.mes_coefficients(mu, sigma, [3.0, 4.0], 1.0, noise, y_std)
    assert cm[0] == 0.0 and cs[1] == 0.0


def test_the_sum_runs_in_sample_order():
    rng = np.random.RandomState(0)
    mu, sigma = rng.normal(size=50), rng.uniform(0.5, 2.0, 50)
    ys = rng.normal(size=7) * 3 + 2
    got = mr.mes(mu, sigma, ys, 1.0, 0.01, 1.0)
    sl = np.sqrt(sigma * sigma - 0.01)
    acc = np.zeros(50)
    for s in range(7):
        acc = acc + mr.h((ys[s] - mu) / sl)
    assert got.tobytes() == (acc / 7.0).tobytes()
    # direction: minimisation mirrors the problem
    mirrored = mr.mes(-mu, sigma, -ys, -1.0, 0.01, 1.0)
    assert mirrored.tobytes() == got.tobytes()


def test_coefficients_match_finite_differences():
    rng = np.random.RandomState(1)
    mu, sigma = rng.normal(size=40), rng.uniform(0.4, 2.0, 40)
    ys = np.sort(rng.normal(size=5)) + 2.5
    for sf in (1.0, -1.0):
        a, cm, cs = mr.mes_coefficients(mu, sigma, sf * ys, sf, 0.04, 1.5)
        assert a.tobytes() == mr.mes(mu, sigma, sf * ys, sf, 0.04, 1.5).tobytes()
        e = 1e-6
        fm = (mr.mes(mu + e, sigma, sf * ys, sf, 0.04, 1.5) - mr.mes(mu - e, sigma, sf * ys, sf, 0.04, 1.5)) / (2 * e)
        fs = (mr.mes(mu, sigma + e, sf * ys, sf, 0.04, 1.5) - mr.mes(mu, sigma - e, sf * ys, sf, 0.04, 1.5)) / (2 * e)
        np.testing.assert_allclose(cm, fm, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(cs, fs, rtol=1e-7, atol=1e-9)
