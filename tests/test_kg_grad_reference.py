"""CPU: the references of the knowledge gradient's gradient (tests/kg_grad_reference.py, tests/kg_grad_reference_hp.py) and
the cases, bar and conditions tests/test_gpu_kg_grad.py judges the kernels with (tests/kg_grad_cases.py).

(i)   the 80-bit closed form against central differences (step 1e-7) of the 80-bit VALUE, kg_reference_hp.kg: under 1e-8 of
      the batch's maximum.  What the difference itself is good to: its truncation, (h / l)^2 ~ 1e-13 relative, and the
      rounding of two 80-bit values over 2 h, 2^-64 kappa / h -- 1e-10 or so with kappa ~ 1e6; a term of the closed form
      that is missing or has the wrong sign shows at 1e-3 and more (iv).  Measured: 2e-29 (a flat corner) .. 3e-11.
(ii)  the f64 form against the 80-bit one is e_ref, and 64 e_ref stays under the cap of the bar;
(iii) every case meets the conditions the bar rests on;
(iv)  the bar rejects the deliberate slips of kg_grad_reference.SLIPS;
(v)   the starts of the L-BFGS-B comparison are the first three judged rows, by the reference's KG, from which SciPy's own
      walk on the f64 reference is well conditioned (kg_grad_cases' docstring).
"""
import numpy as np
import pytest

import kg_grad_cases as gc
import kg_grad_reference as gr
import kg_grad_reference_hp as grh
import kg_reference_hp as krh

CD_ROWS = 12


@pytest.mark.parametrize("name", list(gc.CASES))
def test_closed_form_against_central_differences_of_the_80_bit_value(name):
    Xa, Xq = gc.points(name)
    k = len(Xq) if name == "kink" else min(CD_ROWS, len(Xq))      # (kink: both sides of the indicator)
    want = gc.hp_reference(name)
    cd = grh.central_differences(gc.hp_fit(name), Xa, Xq[:k], gc.CASES[name]["sf"], step=gc.CD_STEP)
    err = float(np.abs(cd - want["grad"][:k]).max() / np.abs(want["grad"]).max())
    print("%s: closed form against central differences %.3g (bar %.3g), %d rows" % (name, err, gc.CD_BAR, k))
    assert err <= gc.CD_BAR
    # the value beside the gradient is kg_reference_hp.kg's
    val = krh.kg(gc.hp_fit(name), Xa, Xq, gc.CASES[name]["sf"])["kg"]
    assert np.array_equal(val, want["kg"])


@pytest.mark.parametrize("name", list(gc.CASES))
def test_e_ref_and_the_conditions_of_the_bar(name):
    c = gc.conditions(name)
    print("%s: %s  bar %.3g" % (name, c, gc.bar(name)))
    assert gc.FACTOR * c["e_ref"] <= gc.CAP
    assert c["max_grad"] >= gc.MIN_GRAD
    if name != "n1":                      # (N = 1: grad mu == 0, the tie is exact and moot)
        assert c["min_kink"] >= gc.MIN_KINK
    assert np.all(np.isfinite(gc.reference(name)["grad"]))
    # the f64 reference walks the envelope the 80-bit one walks
    for key in ("on_env", "strict", "n_env"):
        assert np.array_equal(gc.reference(name)[key], gc.hp_reference(name)[key]), key


def test_one_case_judges_both_sides_of_the_indicator():
    c = gc.conditions("kink")
    print("kink: %d rows with the candidate's line the strict maximum intercept, %d without" % (c["strict"], c["not_strict"]))
    assert c["strict"] >= gc.MIN_SIDE and c["not_strict"] >= gc.MIN_SIDE


@pytest.mark.parametrize("slip", gr.SLIPS)
def test_the_bar_rejects(slip):
    for name in gc.CASES:
        if slip == gr.SLIPS[0] and gc.conditions(name)["strict"] == 0:
            continue                      # (the term is zero on every row of the case)
        Xa, Xq = gc.points(name)
        g = gr.kg_grad(gc.model(name), Xa, Xq, gc.CASES[name]["sf"], slip=slip)["grad"]
        j = gc.judge(name, g)
        print("%s, %s: %.3g (bar %.3g)" % (slip, name, j["err"], j["bar"]))
        assert not j["ok"], (slip, name, j)


@pytest.mark.parametrize("name", list(gc.LBFGSB_STARTS))
def test_the_lbfgsb_starts_are_the_first_well_conditioned_ones(name):
    starts, over = gc.LBFGSB_STARTS[name], gc.LBFGSB_PASSED_OVER[name]
    ranked = [int(i) for i in gc.ranked_rows(name)]
    taken = [i for i in ranked if i in starts or i in over][:len(starts) + len(over)]
    assert ranked[:len(taken)] == taken and sorted(taken) == sorted(starts + over)      # nothing ranked higher is left out
    assert [i for i in taken if i in starts] == list(starts)
    for i in taken:
        sens = gc.walk_sensitivity(name, i)
        print("%s row %d: one ulp at the start moves SciPy's end by %.3g (points), %.3g (values)" % (name, i, sens[0], sens[1]))
        assert gc.well_conditioned(sens) == (i in starts), (name, i, sens)
