"""CPU tests of the knowledge gradient's references (tests/kg_reference.py, tests/kg_reference_hp.py) and of the cases and
bars tests/test_gpu_kg.py judges the kernels with (tests/kg_cases.py).  Nothing here touches the library."""
import numpy as np
import pytest

import kg_cases as kc
import kg_reference as kr
import kg_reference_hp as krh
from oracle import gp_oracle as G

LD = np.longdouble
U = 2.0 ** -53


def _line_sets():
    """random line sets, and the shapes the definition singles out: equal slopes, dominated lines, three lines through
    one point, a single line, all slopes equal"""
    rng = np.random.RandomState(2009)
    sets = []
    for k in range(30):
        L = 2 + k % 9
        sets.append((rng.normal(size=L), rng.normal(size=L) * (0.1 + 0.3 * (k % 4))))
    a, b = rng.normal(size=6), rng.normal(size=6)
    b[3] = b[1]; b[5] = b[1]                                   # three lines of one slope: the largest intercept counts
    sets.append((a, b))
    sets.append((np.array([0.0, -5.0, 0.3, -4.0]), np.array([-1.0, 0.0, 1.0, 0.5])))     # two lines under the envelope
    sets.append((np.array([0.0, 0.0, 0.0]), np.array([-1.0, 0.0, 1.0])))                 # three lines through one point
    sets.append((np.array([0.7]), np.array([0.3])))                                      # one line: KG = 0
    sets.append((np.array([0.1, 0.9, 0.5]), np.array([0.2, 0.2, 0.2])))                  # one slope: KG = 0
    a = rng.normal(size=5)
    sets.append((np.concatenate([a, a]), np.concatenate([a * 0.3, a * 0.3])))            # every line twice
    return sets


def _quadrature(a, b, nodes):
    """E_Z[max_i (a_i + b_i Z)] - max_i a_i by the trapezoid rule on [-10, 10]"""
    z = np.linspace(-10.0, 10.0, nodes)
    g = (a[:, None] + b[:, None] * z[None, :]).max(0) * np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)
    h = z[1] - z[0]
    return h * (g.sum() - 0.5 * (g[0] + g[-1])) - a.max()


def test_envelope_form_against_quadrature():
    worst = 0.0
    for a, b in _line_sets():
        q1, q2 = _quadrature(a, b, 200001), _quadrature(a, b, 100001)
        # the bar: the quadrature's own change when its step is halved (its error is a third of that for a kinked
        # integrand), over the worst-case rounding of a 200 001-term sum of this magnitude
        bar = abs(q1 - q2) + 200001 * U * (np.abs(a).max() + 10.0 * np.abs(b).max())
        for val in (kr.envelope_kg(a[None, :], b[None, :])[0], float(krh.envelope_kg(a[None, :], b[None, :])[0])):
            assert val >= 0.0
            assert abs(val - q1) <= bar, (a, b, val, q1, bar)
            worst = max(worst, abs(val - q1))
    assert worst < 1e-6      # (what the prototype measured over its 200 sets)
    print("envelope vs quadrature: worst |difference| %.3g" % worst)


def test_two_line_closed_form():
    rng = np.random.RandomState(2)
    for _ in range(50):
        a, b = rng.normal(size=2), rng.normal(size=2)
        db = abs(b[1] - b[0])
        want = db * kr.f_neg(np.array(abs(a[0] - a[1]) / db))
        assert kr.envelope_kg(a[None, :], b[None, :])[0] == want        # the same operations: the same bits


def test_far_tail_is_finite_and_zero():
    a = np.array([[0.0, -1e6, 3.0, 3.0 - 1e-300]])
    b = np.array([[0.0, 1.0, 1e-300, 0.0]])
    v = kr.envelope_kg(a, b)[0]
    assert np.isfinite(v) and v >= 0.0
    assert kr.f_neg(np.array([0.0, 39.0, 40.0, 1e300, np.inf])).tolist()[2:] == [0.0, 0.0, 0.0]


def test_lines_against_a_literal_refit():
    N, D, A = 30, 3, 7
    rng = np.random.RandomState(30)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X.sum(1)) + 0.05 * rng.normal(size=N)
    noise, jitter = 1e-2, 1e-6
    om = G.fit(X, y, "matern52", kc.C, 0.6, noise, jitter, True)
    Xa, Xc = rng.uniform(0, 1, (A, D)), rng.uniform(0, 1, (4, D))
    mu_a, mu, sigma, cov = kr.posterior(om, Xa, Xc)
    a, b, live = kr.lines_from_outputs(mu_a, mu, sigma, cov, noise * om.y_std ** 2, (noise + jitter) * om.y_std ** 2, -1.0)
    assert live.all()
    # both sides solve with K (cond <= (c N + noise + jitter) / (noise + jitter)) in f64
    bar = 64 * ((kc.C * N + noise + jitter) / (noise + jitter)) * U * kr.prior_scale(om)
    for i in range(len(Xc)):
        ra, rb = kr.refit_lines(om, y, Xa, Xc[i], -1.0)
        err = max(np.abs(ra - a[i]).max(), np.abs(rb - b[i]).max())
        print("refit vs lines, candidate %d: %.3g (bar %.3g)" % (i, err, bar))
        assert err <= bar


@pytest.mark.parametrize("name", kc.HP_CASES)
def test_f64_reference_against_80_bit(name):
    e = kc.e_ref(name)
    print("e_ref %s: %s" % (name, {k: "%.3g" % v for k, v in e.items()}))
    for k, v in e.items():
        cap = kc.CAP_COV if k == "cov" else kc.CAP_VAL
        assert kc.FACTOR * v <= cap, "64 e_ref of %s in %s is %.3g, over the cap %.3g" % (k, name, kc.FACTOR * v, cap)
    assert (np.asarray(kc.hp_reference(name)["kg"]) >= 0).all() and (kc.reference(name)["kg"] >= 0).all()


@pytest.mark.parametrize("name", list(kc.CASES))
def test_case_conditions(name):
    """asserted here so that no GPU test can hide behind them: the arg-max of every case is decided by a margin the
    f64 reference resolves"""
    best, gap = kc.argmax_conditions(name)
    print("case %s: best KG %.3g of the prior scale, top-two gap %.3g of the best" % (name, best, gap))
    assert best >= kc.ARGMAX_MIN_BEST
    assert gap > kc.ARGMAX_MIN_GAP


def test_coincidence_case_is_what_it_says():
    X, _, _, Xa, Xc = kc.data("n40")
    assert kc.CASES["n40"]["noise"] == 0.0
    assert (Xc[5] == X[0]).all() and (Xc[7] == Xa[3]).all() and (Xa[4] == Xa[1]).all()
    e = kc.e_ref("n40")
    assert max(e.values()) < 1e-12


def _faulty(name, fault):
    _, _, _, Xa, Xc = kc.data(name)
    return kr.kg(kc.model(name), Xa, Xc[:kc.hp_rows(name)], kc.CASES[name]["sf"], fault)


@pytest.mark.parametrize("fault", kr.FAULTS)
def test_bars_reject_the_faults(fault):
    """bar (b) of the GPU file must fail an f64 reference that makes the fault; the honest one passes everywhere"""
    rejected = []
    for name in kc.HP_CASES:
        assert kc.judge_b(name, kc.reference(name))["ok"]
        j = kc.judge_b(name, _faulty(name, fault))
        if not j["ok"]:
            rejected.append(name)
    print("%s: rejected on %s" % (fault, rejected))
    assert "n300" in rejected and "n256" in rejected, (fault, rejected)
    # (the observed covariance changes nothing where the noise is 0: case n40 cannot see that one)
    exempt = {"n40"} if fault == kr.FAULTS[1] else set()
    assert set(kc.HP_CASES) - exempt <= set(rejected), (fault, rejected)
