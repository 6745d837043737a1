"""CPU: the references of tests/test_gpu_input_grad_edges.py judged before they judge anything.
 (a) the 80-bit closed form of d LML / d X (tests/input_grad_reference_hp.py) against Richardson-extrapolated central
     differences of the 80-bit LML itself (lml_grad_reference_hp.lml): the independent check of the formula and its sign;
 (b) its two identities: sum_i d LML / d x_id = 0, and sum_i x_id d LML / d x_id = -d LML / d log l_d against
     lml_grad_reference_hp.lml_and_grad;
 (c) the f64 restatement's error e_ref on every case of tests/input_grad_edge_cases.py, recorded in
     tests/golden/input_grad_eref.json (written where INPUT_GRAD_WRITE=1), and every case meets the cap's condition
     10 max(e_ref, N u) <= 1e-9;
 (d) the bars reject every slip, each injected into the f64 restatement, on at least one case."""
import json
import os

import numpy as np
import pytest

import cov_edge_cases as ec
import input_grad_edge_cases as ic
import input_grad_reference_hp as ir
import lml_grad_edge_cases as lc
import lml_grad_reference_hp as lr

LD = np.longdouble
# (case, the entries (row, dimension) differenced): every kernel; tile-interior, tile-edge and last rows; the duplicated
# pair of T193-dup is left alone (Matern-1/2 has a kink at d2 = 0: no derivative to difference there)
FD_ENTRIES = {
    "B/iso": [(0, 0), (63, 1), (64, 2), (128, 0)],
    "A/ard": [(5, 0), (127, 1)],
    "S3/iso": [(1, 0), (64, 62)],
    "T193/ard": [(100, 16), (192, 3)],
}
FD_STEP = 5e-4      # in units of the length scale: the displaced coordinate is x_id + step l_d
# The extrapolated difference is off by step^4 = 6e-14 times the LML's fifth derivative along s_id, whose polynomial
# factors (the fifth Hermite polynomial's coefficients reach 15) keep it within some tens of the entry's scale, and by the
# rounding of the 80-bit LML over the step (1e-15 of the scale): 1e-9 of the scale is the ceiling.  A wrong sign or factor
# is of order 1 of the entry.
FD_CEILING = 1e-9
SLIP_CASES = ["S3/iso", "S3/ard", "B/ard", "T193/iso", "T193/ard", "E/ard"]


def _lml_at(case, i, d, delta):
    X, y, kind, c, ls, noise, jitter, norm = lc.call_args(case)
    Xd = np.array(X, dtype=np.float64, copy=True)
    Xd[i, d] = X[i, d] + delta
    return lr.lml(Xd, y, kind, c, ls, noise, jitter, norm), LD(Xd[i, d])


@pytest.mark.parametrize("case", sorted(FD_ENTRIES))
def test_the_closed_form_against_central_differences(case):
    g, s = ic.hp_reference(case)
    ls = np.broadcast_to(np.atleast_1d(lc.call_args(case)[4]), (g.shape[1],))
    for i, d in FD_ENTRIES[case]:
        def diff(h):
            (vp, xp), (vm, xm) = _lml_at(case, i, d, h), _lml_at(case, i, d, -h)
            return (vp - vm) / (xp - xm)
        h = FD_STEP * float(ls[d])
        fd = (LD(4) * diff(h / 2) - diff(h)) / LD(3)
        err = float(abs(fd - g[i, d]) / s[i, d])
        print("%s entry (%d, %d): closed form %.6e, differences %.6e, %.3g of the scale (entry / scale %.3g)" % (case, i, d, float(g[i, d]), float(fd), err, float(abs(g[i, d]) / s[i, d])))
        assert err <= FD_CEILING, (case, i, d, err)


@pytest.mark.parametrize("case", ["S1/iso", "S3/iso", "S3/ard", "B/iso", "T193/ard", "T193-dup/ard", "T193-noise0/iso"])
def test_the_two_identities_of_the_closed_form(case):
    """in 80 bits both hold to the rounding of N terms of the format (2^-64 each, taken as N 2^-63 of the scales)"""
    g, _ = ic.hp_reference(case)
    ref = lc.hp_reference(case)
    zero, moment = ic.identities(case, g.astype(np.float64), ref["grad"].astype(np.float64))
    # (the gradient is rounded to f64 on the way in: u of every entry's size, far below N u of its scale)
    n = lc.config(case)["N"]
    print("%s: sum over the rows %.3g, first moment %.3g of their scales" % (case, zero, moment))
    assert zero <= 2 * n * ec.U and moment <= 2 * n * ec.U, (case, zero, moment)


def test_one_point_has_no_gradient():
    g, s = ic.hp_reference("S1/ard")
    assert g.shape == (1, 1) and g[0, 0] == 0 and s[0, 0] == 0
    assert ir.dlml_dx_f64(*lc.call_args("S1/ard"))[0, 0] == 0.0


def test_the_recorded_e_ref_and_the_caps_condition():
    """tests/golden/input_grad_eref.json is the record; a fresh value is at most 4 x the recorded one.  Below 8 u of the
    scale a value is last-bit noise of the BLAS underneath and is compared as 8 u.  ic.bar asserts the cap's condition."""
    fresh = {case: ic.e_ref_fresh(case) for case in ic.CASES}
    if os.environ.get("INPUT_GRAD_WRITE") == "1":
        with open(ic.EREF_JSON, "w") as f:
            json.dump(dict(unit="the f64 restatement's worst entry of d LML / d X against the 80-bit closed form, as a fraction of the entry's scale (tests/input_grad_reference_hp.py)",
                           cases=fresh), f, indent=1, sort_keys=True)
        ic._cache.pop("record", None)
    floor = 8 * ec.U
    for case in ic.CASES:
        rec = ic.e_ref_recorded(case)
        n = lc.config(case)["N"]
        print("%s: e_ref %.3g (recorded %.3g), bar %.3g" % (case, fresh[case], rec, ic.bar(case, rec)))
        assert max(fresh[case], floor) <= 4 * max(rec, floor), (case, fresh[case], rec)
        assert 10 * max(rec, n * ec.U) <= ec.CAP_VAL, case


def test_the_bars_reject_every_slip():
    """every slip, injected into the f64 restatement, misses the bar of at least one case it can show on -- and the honest
    restatement meets every one of them"""
    caught = {s: [] for s in ir.SLIPS}
    for case in SLIP_CASES:
        bar = ic.bar(case, ic.e_ref_recorded(case))
        assert ic.error(case, ic.f64_result(case)) <= bar, case
        for slip in ir.SLIPS:
            if slip in ir.ARD_ONLY and not lc.config(case)["ard"]:
                continue
            err = ic.error(case, ic.f64_result(case, slip))
            if err > bar:
                caught[slip].append((case, err))
    for slip, hits in caught.items():
        print("%s: %s" % (slip, ", ".join("%s %.3g" % h for h in hits) or "NOT CAUGHT"))
    assert all(caught.values()), [s for s, h in caught.items() if not h]
