"""CPU: the NumPy reference of the expected hypervolume improvement (tests/ehvi_reference.py) against definitions that do not
share its decomposition -- Monte Carlo of the area's growth (the area by a sort), the row-strip form (objectives swapped),
the product of two EIs at P = 0, central differences in long double -- and its front builder's edge cases."""
import json
import math
import os

import numpy as np
import pytest
from scipy.special import ndtr

import ehvi_reference as er

HERE = os.path.dirname(os.path.abspath(__file__))
LD = er.LD


def _e_ref():
    return json.load(open(os.path.join(HERE, "golden", "ehvi_eref.json")))["e_ref"]


def test_golden_e_ref_is_the_reference_own_error():
    import mpmath as mp
    per = {}
    with mp.workdps(80):
        for z in er.Z_SET:
            ref = er.H_mp(z)
            got = mp.mpf(float(er.H(np.array([z]))[0]))
            per[z] = float(abs(got - ref) / ((2 + min(z, 0.0) ** 2) * max(ref, mp.mpf(er.TINY))))
    worst = max(per.values())
    print("e_ref measured %.3e, golden %.3e" % (worst, _e_ref()))
    assert min(er.Z_SET) <= -38 and max(er.Z_SET) >= 40 and 0.0 in er.Z_SET
    assert worst <= _e_ref() * (1 + 1e-12)
    assert _e_ref() < 16 * er.U


def _areas_with(F, r, V):
    """hv(F u {v}) for every row v of V (n, 2), by a sort along the points: descending u_1, the running maximum of u_2 is
    the slab's height; a coordinate that does not beat r is moved onto r, where it adds no area"""
    n = V.shape[0]
    pts = np.concatenate([np.broadcast_to(F[None], (n,) + F.shape), V[:, None, :]], axis=1)
    pts = np.maximum(pts, np.asarray(r)[None, None, :])
    order = np.argsort(-pts[:, :, 0], axis=1, kind="stable")
    x = np.take_along_axis(pts[:, :, 0], order, 1)
    y = np.take_along_axis(pts[:, :, 1], order, 1)
    top = np.maximum.accumulate(y, axis=1)
    left = np.concatenate([x[:, 1:], np.full((n, 1), r[0])], axis=1)
    return ((x - left) * (top - r[1])).sum(1)


# (front size, seed, m_1, sigma_1, m_2, sigma_2): oriented posteriors placed inside, above and beside the front
MC_CASES = [(0, 1, 0.3, 0.5, 0.2, 0.4), (1, 2, 0.5, 0.3, 0.5, 0.3), (3, 3, 0.6, 0.25, 0.4, 0.35), (8, 4, 0.5, 0.4, 0.5, 0.4),
            (8, 5, 1.1, 0.2, 0.1, 0.3), (5, 6, 0.2, 0.6, 0.9, 0.1)]


def _front_of(P, seed):
    rng = np.random.RandomState(seed)
    u1 = np.sort(rng.uniform(0.1, 1.0, P))
    u2 = np.sort(rng.uniform(0.1, 1.0, P))[::-1]
    Y = np.stack([u1, u2], 1)
    extra = Y * rng.uniform(0.3, 0.95, (P, 2)) if P else np.zeros((0, 2))      # dominated points
    return np.concatenate([Y, extra])


@pytest.mark.parametrize("case", MC_CASES)
def test_closed_form_is_the_expected_growth_of_the_area(case):
    P, seed, m1, s1, m2, s2 = case
    Y = _front_of(P, seed)
    r = np.array([0.0, 0.0])
    F, _, _, hv = er.front(Y, (1.0, 1.0), r)
    assert F.shape[0] == P
    a, c = er.strips(F, r)
    want = float(er.value(a, c, np.array([m1]), np.array([s1]), np.array([m2]), np.array([s2]))[0])
    rng = np.random.RandomState(100 + seed)
    n = 150000
    V = np.stack([m1 + s1 * rng.normal(size=n), m2 + s2 * rng.normal(size=n)], 1)
    gain = _areas_with(F, r, V) - er.hypervolume(F, r)
    est, se = gain.mean(), gain.std(ddof=1) / math.sqrt(n)
    print("P=%d closed %.6g  mc %.6g +- %.2g  (%.2f se)" % (P, want, est, se, (want - est) / se))
    assert abs(want - est) <= 4 * se


def test_row_strips_agree_with_column_strips():
    rng = np.random.RandomState(7)
    e_ref = _e_ref()
    for P in (0, 1, 2, 9, 40):
        Y = _front_of(P, 20 + P)
        r = np.array([-0.1, 0.05])
        M = 200
        m1, m2 = rng.uniform(-0.5, 1.5, M), rng.uniform(-0.5, 1.5, M)
        s1, s2 = rng.uniform(0.01, 0.6, M), rng.uniform(0.01, 0.6, M)
        F, _, _, hv = er.front(Y, (1.0, 1.0), r)
        Ft, _, _, hvt = er.front(Y[:, ::-1], (1.0, 1.0), r[::-1])
        assert abs(hv - hvt) <= 8 * er.U * hv * max(P, 1)
        p = er.partials(*er.strips(F, r), m1, s1, m2, s2)
        q = er.partials(*er.strips(Ft, r[::-1]), m2, s2, m1, s1)
        err = np.abs(p["val"] - q["val"])
        bar = er.bound(p["scale"], e_ref) + er.bound(q["scale"], e_ref)
        print("P=%d worst err / bar %.3g" % (P, (err / bar).max()))
        assert (err <= bar).all()


def test_empty_front_is_the_product_of_two_eis():
    rng = np.random.RandomState(3)
    M = 500
    mu1, mu2 = rng.normal(size=M), rng.normal(size=M)
    s1, s2 = rng.uniform(0.05, 2.0, M), rng.uniform(0.05, 2.0, M)
    for sf in ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0)):
        ref = np.array([-sf[0] * 4.0, -sf[1] * 4.0])          # z > 0 throughout: both forms are conditioned
        a, c = er.strips(np.zeros((0, 2)), np.asarray(sf) * ref)
        got = er.sweep(a, c, sf, mu1, s1, mu2, s2)["value"]
        ei = []
        for mu, s, f, inc in ((mu1, s1, sf[0], ref[0]), (mu2, s2, sf[1], ref[1])):
            d = f * (mu - inc)
            Z = d / s
            ei.append(d * ndtr(Z) + s * np.exp(-Z * Z / 2) / math.sqrt(2 * math.pi))
        want = ei[0] * ei[1]
        assert (np.abs(got - want) <= 8 * er.U * want).all()


def test_partials_against_central_differences_in_long_double():
    rng = np.random.RandomState(11)
    for P in (0, 2, 9):
        F, _, _, _ = er.front(_front_of(P, 40 + P), (1.0, 1.0), (0.0, 0.0))
        a, c = er.strips(F, (0.0, 0.0), LD)
        M = 40
        x = [rng.uniform(-0.3, 1.3, M).astype(LD), rng.uniform(0.2, 0.5, M).astype(LD),
             rng.uniform(-0.3, 1.3, M).astype(LD), rng.uniform(0.2, 0.5, M).astype(LD)]
        p = er.partials(a, c, *x)
        h = LD(1e-7)
        for k, name in enumerate(("cm1", "cs1", "cm2", "cs2")):
            up, dn = list(x), list(x)
            up[k] = x[k] + h
            dn[k] = x[k] - h
            fd = (er.value(a, c, *up) - er.value(a, c, *dn)) / (2 * h)
            err = np.abs(fd - p[name])
            # the difference's truncation, h^2 / 6 of the third derivative: in sigma that is a polynomial of degree 6 in z
            # times phi / sigma^3 -- at most a few hundred times the coefficient's own terms for sigma >= 0.2, so 1e-14 / 6
            # of it stays below 1e-8 of them -- and its rounding noise: 2^-64 |value| / h = 5e-13 |value|
            scale = 1e-8 * np.abs(p["abs_c"][k]) + 1e-11 * np.abs(p["val"])
            print("P=%d %s worst %.3g" % (P, name, float((err / scale).max())))
            assert (err <= scale).all()


def test_zero_sigma_and_nan_rows():
    F, _, _, _ = er.front(np.array([[0.3, 0.8], [0.7, 0.4]]), (1.0, 1.0), (0.0, 0.0))
    a, c = er.strips(F, (0.0, 0.0))
    # sigma == 0 on both: the exact area a point adds
    v = er.value(a, c, np.array([0.5, 0.2, 1.0]), np.zeros(3), np.array([0.6, 0.3, 1.0]), np.zeros(3))
    want = [0.2 * 0.2, 0.0, 1.0 - (0.3 * 0.8 + 0.4 * 0.4)]
    assert np.allclose(v, want, rtol=0, atol=4 * er.U)
    v = er.value(a, c, np.array([np.nan, 0.5]), np.array([0.1, np.nan]), np.array([0.5, 0.5]), np.array([0.1, 0.1]))
    assert np.isnan(v).all()
    assert er.argmax(np.array([np.nan, 0.0, 0.0])) == (1, 0.0)


def test_front_edge_cases():
    sf = (1.0, 1.0)
    # duplicates merge, ties in one coordinate keep the better point, the reference's boundary is outside
    Y = np.array([[1.0, 3.0], [1.0, 3.0], [2.0, 2.0], [2.0, 1.5], [1.5, 2.0], [3.0, 1.0], [0.0, 5.0], [5.0, 0.0], [0.5, 0.5]])
    F, raw, idx, hv = er.front(Y, sf, (0.0, 0.0))
    assert F.tolist() == [[1.0, 3.0], [2.0, 2.0], [3.0, 1.0]]
    assert idx.tolist() == [0, 2, 5]
    assert hv == 1.0 * 3.0 + 1.0 * 2.0 + 1.0 * 1.0
    # every point dropped; n = 0
    for Yn in (np.array([[0.0, 1.0], [-1.0, -1.0]]), np.zeros((0, 2))):
        F, raw, idx, hv = er.front(Yn, sf, (0.0, 0.0))
        assert F.shape == (0, 2) and hv == 0.0
        a, c = er.strips(F, (0.0, 0.0))
        assert a.tolist() == [0.0, np.inf] and c.tolist() == [0.0]
    # all four sign pairs: the same oriented front
    base = np.array([[1.0, 3.0], [2.0, 2.0], [3.0, 1.0], [1.5, 1.5]])
    for s in ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0)):
        F, raw, idx, hv = er.front(base * np.array(s), s, (0.0, 0.0))
        assert F.tolist() == base[:3].tolist() and hv == 6.0
        assert raw.tolist() == (base[:3] * np.array(s)).tolist()


def test_front_is_invariant_under_permutation_and_dominated_points():
    rng = np.random.RandomState(5)
    Y = rng.uniform(0, 1, (60, 2))
    r = (0.1, 0.1)
    F, _, _, hv = er.front(Y, (1.0, -1.0), r)
    perm = rng.permutation(60)
    F2, _, _, hv2 = er.front(Y[perm], (1.0, -1.0), r)
    assert F.tolist() == F2.tolist() and hv == hv2
    worse = Y * np.array([0.9, 1.1])                       # smaller u_1, larger y_2 (= smaller u_2): dominated
    F3, _, _, hv3 = er.front(np.concatenate([worse, Y]), (1.0, -1.0), r)
    assert F.tolist() == F3.tolist() and hv == hv3


def test_hypervolume_of_a_staircase_by_hand():
    steps = np.array([[1.0, 4.0], [2.0, 3.0], [3.0, 2.0], [4.0, 1.0]])
    assert er.hypervolume(steps, (0.0, 0.0)) == 4.0 + 3.0 + 2.0 + 1.0
    assert er.front(steps, (1.0, 1.0), (0.5, 0.5))[3] == 0.5 * 3.5 + 1.0 * 2.5 + 1.0 * 1.5 + 1.0 * 0.5
    assert er.default_ref(steps, (1.0, 1.0)).tolist() == [1.0 - 0.3, 1.0 - 0.3]
    assert er.default_ref(np.array([[2.0, 5.0]]), (-1.0, 1.0)).tolist() == [2.1, 4.9]
