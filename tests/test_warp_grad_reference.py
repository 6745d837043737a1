"""CPU: the reference of tgp_fit_warp_grad's 2 D warp entries (tests/warp_grad_cases.py) judged before it judges anything.
 (a) the 80-bit chain rule against Richardson-extrapolated central differences in log a_d and log b_d of the 80-bit LML
     (lml_grad_reference_hp.lml) over NumPy-warped X -- on the identity warp too, where the entries are the true gradient,
     not 0;
 (b) the f64 restatement's error against it, e_ref, recorded in tests/golden/warp_grad_eref.json (written where
     WARP_GRAD_WRITE=1), and the cap's condition on every case."""
import json
import os

import numpy as np
import pytest

import cov_edge_cases as ec
import lml_grad_reference_hp as lr
import warp_grad_cases as wc
import warp_reference as wr

LD = np.longdouble
FD_STEP = 1e-3
# step^4 = 1e-12 times the fifth derivative of the LML in log a, some tens of the entry's scale at most (every derivative of
# u^a in log a brings a factor a log u, |a log u| u^a <= 1 / e ... 5! / e^5 on the way): 1e-9 of the scale is the ceiling; the
# model differenced is fitted on NumPy's w(X), the closed form on the same numbers
FD_CEILING = 1e-9
FD_CASES = {"N40-D2": None, "identity": None, "N129-D3": [0, 2, 4], "N257-D17": [3, 33]}    # None: every entry


@pytest.mark.parametrize("case", sorted(FD_CASES))
def test_the_chain_rule_against_central_differences(case):
    X, y, lo, hi, a, b, ls = wc.data(case)
    D = len(a)
    w, _ = wc.restatement(case)
    val, sc = wc.reference(case, w)
    if case == "identity":
        assert np.all(val != 0)
    for p in (range(2 * D) if FD_CASES[case] is None else FD_CASES[case]):
        def lml_at(h):
            aa, bb = a.copy(), b.copy()
            (aa if p < D else bb)[p % D] = float(np.exp(np.log(LD((a if p < D else b)[p % D])) + LD(h)))
            wd = wr.warp_f64(wc.unit(case), aa[None, :], bb[None, :])[0]
            return lr.lml(*wc.fit_args(case, wd)), np.log(LD((aa if p < D else bb)[p % D]))

        def diff(h):
            (vp, tp), (vm, tm) = lml_at(h), lml_at(-h)
            return (vp - vm) / (tp - tm)
        fd = (LD(4) * diff(FD_STEP / 2) - diff(FD_STEP)) / LD(3)
        err = float(abs(fd - val[p]) / sc[p])
        print("%s entry %d: chain rule %.6e, differences %.6e, %.3g of the scale" % (case, p, float(val[p]), float(fd), err))
        assert err <= FD_CEILING, (case, p, err)


def test_the_recorded_e_ref_and_the_caps_condition():
    fresh = {}
    for case in wc.CASES:
        w, got = wc.restatement(case)
        fresh[case] = float(wc.fractions(got, *wc.reference(case, w)).max())
    if os.environ.get("WARP_GRAD_WRITE") == "1":
        with open(wc.EREF_JSON, "w") as f:
            json.dump(dict(unit="the f64 restatement's worst warp entry against the 80-bit chain rule, as a fraction of the entry's scale (tests/warp_grad_cases.py)", cases=fresh), f, indent=1, sort_keys=True)
    for case in wc.CASES:
        rec = wc.e_ref_recorded(case)
        print("%s: e_ref %.3g (recorded %.3g), bar %.3g" % (case, fresh[case], rec, wc.bar(case, rec)))
        assert max(fresh[case], 8 * ec.U) <= 4 * max(rec, 8 * ec.U), case
