"""CPU: the NumPy reference of the constrained / cost-aware acquisition (tests/weighted_reference.py) held to mpmath, to its
own 80-bit form and to central differences of its own value -- what the GPU tests' bars are made of."""
import json
import os

import numpy as np
import pytest

import weighted_cases as wc
import weighted_reference as wr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def test_log_phi_against_mpmath_on_the_set():
    """f64 (scipy.special.log_ndtr) and the 80-bit form, on z in Z_SET; the committed e_ref is what the generator measures"""
    import mpmath as mp
    committed = _json("weighted_eref.json")
    worst = 0.0
    for z in wr.Z_SET:
        ref = wr.logphi_mp(z)
        got = float(wr.logphi(np.array([z]))[0][0])
        assert np.isfinite(got)
        with mp.workdps(60):
            e = float(abs(mp.mpf(got) - ref) / max(abs(ref), mp.mpf(wr.TINY)))
        assert e == pytest.approx(committed["per_z"][repr(z)], rel=1e-6, abs=1e-300), z
        worst = max(worst, e)
        if abs(z) <= 1e5:                                             # (z^2 / 2 is beyond the long double's own tail only at 1e150)
            hp = wr.logphi(np.array([z], dtype=wr.LD))[0][0]
            with mp.workdps(60):
                assert float(abs(mp.mpf(float(hp)) - ref) / max(abs(ref), mp.mpf(wr.TINY))) < 4 * wr.U, z
    assert worst == pytest.approx(committed["e_ref"], rel=1e-6) and worst < 1e-13


def test_ratio_against_mpmath():
    import mpmath as mp
    for z in (-1e5, -40.0, -10.0, -1.0, 0.0, 1.0, 9.0):
        with mp.workdps(60):
            ref = float(mp.npdf(z) / mp.ncdf(z))
        for dt in (np.float64, wr.LD):
            got = float(wr.logphi(np.array([z], dtype=dt))[1][0])
            assert got == pytest.approx(ref, rel=1e-13), (z, dt)


def test_step_function_cost_and_nan_rows():
    mu = np.array([0.0, 1.0, 2.0, np.nan, 1.0])
    sg = np.array([0.0, 0.0, 0.0, 0.0, np.nan])
    assert np.array_equal(wr.side_logf(wr.GE, 1.0, mu, sg)[:3], [-np.inf, 0.0, 0.0])
    assert np.array_equal(wr.side_logf(wr.LE, 1.0, mu, sg)[:3], [0.0, 0.0, -np.inf])
    assert np.isnan(wr.side_logf(wr.GE, 1.0, mu, sg)[3:]).all() and np.isnan(wr.side_logf(wr.COST, 0.0, mu, sg)[3:]).all()
    assert np.array_equal(wr.side_logf(wr.COST, 0.0, mu, sg)[:3], [-0.0, -1.0, -2.0])
    r = wr.sweep(wr.ACQ_EI, 1.0, 0.0, 0.0, np.array([1.0, 1.0, np.nan]), np.array([1.0, 1.0, 1.0]),
                 [(wr.GE, 0.0, np.array([-1.0, 5.0, 5.0]), np.array([0.0, 1.0, 1.0]))])
    assert r["value"][0] == 0.0 and r["value"][1] > 0 and np.isnan(r["value"][2]) and r["best_idx"] == 1
    assert wr.argmax(np.array([np.nan, np.nan])) == (0, -np.inf) and wr.argmax(np.array([1.0, 2.0, 2.0])) == (1, 2.0)
    # a 1e-400 feasibility: the product is 0, the logs still order
    far = wr.sweep(wr.ACQ_NONE, 1.0, 0.0, 0.0, np.zeros(2), np.ones(2), [(wr.GE, 45.0, np.zeros(2), np.array([1.0, 0.9]))])
    assert np.all(np.isfinite(far["logw"])) and far["best_idx"] == 0
    assert not wr.sweep(wr.ACQ_EI, 1.0, -1.0, 0.0, np.zeros(2), np.ones(2), [(wr.GE, 45.0, np.zeros(2), np.array([1.0, 0.9]))])["value"].any()


@pytest.mark.parametrize("name", list(wc.GRAD_CASES))
def test_the_f64_gradient_against_the_80_bit_form_and_the_committed_e_ref(name):
    v, g, _ = wc.grad_references(name, f64=True)
    ev, eg = wc.grad_errors(name, v, g)
    committed = _json("weighted_grad_eref.json")["cases"][name]
    print(name, ev, eg, committed)
    assert ev == pytest.approx(committed["value"], rel=1e-3, abs=1e-18) and eg == pytest.approx(committed["grad"], rel=1e-3, abs=1e-18)
    assert wc.grad_bar(name, eg) <= 1e-6, "the reference judges nothing at this conditioning"
    rv, rg, ra = wc.grad_references(name)
    assert np.all(np.isfinite(rg.astype(np.float64))) and float(np.abs(rg).max()) > 0


@pytest.mark.parametrize("name", ["g200_k2_m7", "g300_k2_m7_f32obj", "g200_k2_m7_none", "g200_k1_m7_underflow"])
def test_the_gradient_against_central_differences_of_its_own_value(name):
    """the 80-bit gradient against central differences of the 80-bit value, entry by entry over the entry's sum of absolute
    terms.  Step 1e-7: the difference's truncation error falls as the step squared (4e-4 at 1e-5 on a far-tail row of
    g200_k2_m7, 4e-6 at 1e-6) and the long double's rounding, 1e-19 / step, is still far below it"""
    import acq_grad_reference_hp as ah
    p = wc.problem(name)
    fits = wc.hp_fits(name)
    _, rg, ra = wc.grad_references(name)
    step = 1e-7
    m, D = p["Xc"].shape
    num = np.zeros((m, D), wr.LD)
    for d in range(D):
        vals = []
        for sgn in (+1, -1):
            Xq = p["Xc"].astype(wr.LD).copy()
            Xq[:, d] += wr.LD(sgn * step)
            posts = [ah.posterior_values(f, Xq) for f in fits]
            sides = [(k, lv, mu, sg) for (_, _, k, lv), (mu, sg) in zip(p["sides"], posts[1:])]
            vals.append(wr.sweep(p["acq"], p["sf"], p["incumbent"], p["param"], posts[0][0], posts[0][1], sides)["value"])
        num[:, d] = (vals[0] - vals[1]) / wr.LD(2 * step)
    err = float((np.abs(num - rg) / np.maximum(ra, wr.LD(wr.TINY))).max())
    print(name, "central differences:", err)
    assert err < 1e-6
