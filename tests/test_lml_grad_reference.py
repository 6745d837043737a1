"""CPU: the references of tests/test_gpu_lml_grad_edges.py judged before they judge anything.
 (a) the 80-bit closed form (tests/lml_grad_reference_hp.py) against oracle.gp_oracle.lml_and_grad on every case of
     tests/lml_grad_edge_cases.py: the oracle's errors are the e_ref the bars are built from, recorded in
     tests/golden/lml_grad_eref.json (written where LML_GRAD_WRITE=1), and every case meets the cap's condition;
 (b) against the committed golden grad_* cases (scikit-learn's values through the reference project);
 (c) against central differences in log theta of the 80-bit LML itself: the independent check of the formulas;
 (d) the bars reject the slips they exist for, each injected into the f64 restatement."""
import json
import os

import numpy as np
import pytest

import cov_edge_cases as ec
import lml_grad_edge_cases as lc
import lml_grad_reference_hp as lr
from conftest import golden_path
from cov_reference_hp import Fit
from oracle import gp_oracle as G

LD = np.longdouble
EREF_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lml_grad_eref.json")
GOLDEN_CASES = ["grad_rbf_iso_3d", "grad_rbf_ard_3d", "grad_matern52_ard_5d", "grad_matern32_iso_5d",
                "grad_matern12_iso_5d_nowhite", "grad_default_matern52_white"]
# every case of at most 300 points and five hyper-parameters, and two wide ARD ones (each hyper-parameter costs four 80-bit fits)
FD_CASES = [c for c in lc.CASES if lc.config(c)["N"] <= 300 and (not lc.config(c)["ard"] or lc.config(c)["D"] <= 3)] + ["S2/ard", "T193/ard"]
FD_STEP = 2e-3
# The extrapolated difference is off by the order of step^4 = 1.6e-11 times the LML's fifth derivative in log theta, which is
# of the order of the scale at most, and by the rounding of the 80-bit LML over the step (1e-16 of the scale): 1e-10 of the
# scale is the ceiling (measured: 2.6e-13 at most).  A wrong formula (a sign, a factor, h of another kernel) is of order 1
# of the ENTRY, and the entry is a cancellation to 1e-6 of its scale on model A: so the second ceiling, 1e-6 of the largest
# entry (measured: 9e-10 at most, on A).
FD_CEILING_SCALE, FD_CEILING_ENTRY = 1e-10, 1e-6
SLIP_CASES = ["S3/iso", "S3/ard", "S5/ard", "T193/iso", "T193/ard", "E/ard", "C/iso"]


def _record():
    with open(EREF_JSON) as f:
        return json.load(f)


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def test_the_table():
    """every kernel on either path, every case twice (isotropic and ARD), A-G the joint posterior's models"""
    for path in ("small", "blocked"):
        assert {m["kind"] for m in lc.MODELS.values() if m["path"] == path} == set(G.KINDS)
    assert len(lc.CASES) == 2 * len(lc.MODELS) and sorted(lc.SMALL + lc.BLOCKED) == sorted(lc.CASES)
    for case in lc.CASES:
        c = lc.config(case)
        small = c["N"] <= 128 and (c["D"] + 3) // 4 * 4 <= 64
        assert (c["path"] == "small") == small, case
    X, y = lc.call_args("T193-dup/iso")[:2]
    assert X[7].tobytes() == X[3].tobytes() and y[7] != y[3]
    assert lc.call_args("T193-noise0/ard")[5] == 0.0 and lc.call_args("T193-raw/iso")[7] is False
    for m in "ABCDEFG":                                       # the same X and y as tests/cov_edge_cases.py's
        assert np.array_equal(lc.call_args(m + "/iso")[0], ec.data(m)[0]) and np.array_equal(lc.call_args(m + "/ard")[1], ec.data(m)[1])


@pytest.mark.parametrize("case", lc.CASES)
def test_the_case_can_judge(case):
    e, ref = lc.e_ref(case), lc.hp_reference(case)
    print("%s e_ref %s; scale / |entry| up to %.3g" % (case, "  ".join("%s %.3g" % kv for kv in e.items()), lc.cancellation(case)))
    bars = lc.bars(case)                                      # (asserts the cap's condition for every quantity)
    assert all(b <= lc.CAP for b in bars.values())
    assert np.all(np.isfinite(ref["grad"].astype(np.float64))) and ref["lml_scale"] > 0
    zero = ref["grad_scale"] == 0                             # an exact zero is asked for exactly where the definition gives one
    want = np.zeros(len(zero), dtype=bool)
    if lc.config(case)["N"] == 1:
        want[1:-1] = True
    if lc.call_args(case)[5] == 0.0:
        want[-1] = True
    assert np.array_equal(zero, want) and np.all(ref["grad"][zero] == 0)
    j = lc.judge(case, *lc.f64_result(case))                  # the honest f64 restatement passes
    lc.show(case, "f64 restatement", j)
    assert j["ok"], j
    lml, grad, ls, gs = lr.lml_and_grad_f64(*lc.call_args(case), with_scale=True)     # and its scales are the 80-bit ones
    assert abs(ls - float(ref["lml_scale"])) <= 1e-6 * ls and np.allclose(gs, ref["grad_scale"].astype(np.float64), rtol=1e-6, atol=0)


def test_the_recorded_e_ref():
    """tests/golden/lml_grad_eref.json is the record; a fresh value is at most 4 x the recorded one (more would mean the
    reference, the data or the arithmetic under them changed).  Below 8 u of the scale a value is last-bit noise of the
    BLAS underneath and is compared as 8 u."""
    fresh = {case: dict(e_ref=lc.e_ref(case), scale_over_entry=lc.cancellation(case)) for case in lc.CASES}
    if os.environ.get("LML_GRAD_WRITE") == "1":
        with open(EREF_JSON, "w") as f:
            json.dump(dict(unit="fraction of the quantity's scale (tests/lml_grad_reference_hp.py); length_scale: the worst entry; scale_over_entry: the largest scale / |entry| of the gradient",
                           cases=fresh), f, indent=1, sort_keys=True)
    rec = _record()["cases"]
    assert sorted(rec) == sorted(fresh)
    floor = 8 * lc.U
    for case in fresh:
        for k in lc.KEYS:
            assert max(fresh[case]["e_ref"][k], floor) <= 4 * max(rec[case]["e_ref"][k], floor), (case, k, fresh[case], rec[case])


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_the_closed_form_against_the_golden_cases(name):
    """scikit-learn's LML and gradient are an honest f64 computation of the same definition: they are held to the bar an
    f64 result gets, 64 max(e_ref, N u) of the scale with e_ref the oracle's error on that case.  (A case without a
    WhiteKernel has noise 0 here and no noise entry there.)"""
    with np.load(golden_path(name), allow_pickle=False) as z:
        c = {k: z[k] for k in z.files}
    white = float(c["noise"]) >= 0
    noise = float(c["noise"]) if white else 0.0
    ls = c["length_scale"] if len(c["length_scale"]) > 1 else float(c["length_scale"][0])
    args = (c["X"], c["y"], str(c["kind"]), float(c["constant"]), ls, noise, float(c["jitter"]), True)
    ref = lr.lml_and_grad(Fit(*args), c["y"])
    n = len(c["grad"])
    assert n == len(ref["grad"]) - (0 if white else 1)
    olml, ograd = G.lml_and_grad(*args)
    N = len(c["y"])
    for what, got, want, scale in (("lml", [float(c["lml"])], ref["lml"], ref["lml_scale"]),
                                   ("grad", c["grad"], ref["grad"][:n], ref["grad_scale"][:n])):
        ogot = [olml] if what == "lml" else ograd[:n]
        err, e = lc._fraction(got, want, scale).max(), lc._fraction(ogot, want, scale).max()
        bar = ec._bar(float(e), N, lc.CAP)
        print("%s %s: scikit-learn %.3g of the scale (bar %.3g, e_ref %.3g)" % (name, what, err, bar, e))
        assert err <= bar, (name, what, err, bar)


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FD_CASES)
def test_the_closed_form_against_central_differences(case):
    ref = lc.hp_reference(case)
    fd = lr.central_differences(*lc.call_args(case), step=FD_STEP)
    n = len(fd)
    assert n == len(ref["grad"]) - (1 if lc.call_args(case)[5] == 0.0 else 0)
    d = np.abs(fd - ref["grad"][:n])
    sc = ref["grad_scale"][:n]
    of_scale = float((d / np.where(sc == 0, LD(1), sc)).max())
    of_entry = float(d.max() / max(np.abs(ref["grad"][:n]).max(), LD(1e-300)))
    print("%s closed form against Richardson-extrapolated central differences (h = %g): %.3g of the scale, %.3g of the largest entry"
          % (case, FD_STEP, of_scale, of_entry))
    assert of_scale <= FD_CEILING_SCALE and of_entry <= FD_CEILING_ENTRY


# ---- (d) the bars have teeth -------------------------------------------------------------------------------------------
def _applies(slip, case):
    """whether the slip changes anything on this case at all (a slip that leaves every term where it was is no slip)"""
    c = lc.config(case)
    if slip in lr.ARD_ONLY and not (c["ard"] and c["D"] > 1):
        return False
    if slip == "dimensions >= 16 dropped from the ARD sums":
        return c["D"] > 16
    if slip == "the last tile's rows beyond N - (N mod 64) dropped":
        return c["N"] % 64 != 0
    if slip == "off-diagonal tiles counted once instead of twice":
        return c["N"] > 64
    if slip == "the diagonal in the length-scale sums with weight h(0)":
        return c["kind"] == "matern12"
    return True


def test_the_bars_reject_the_slips():
    """Every slip of lml_grad_reference_hp.SLIPS, injected into the f64 restatement, is rejected by judge() on every case
    of SLIP_CASES it applies to -- at least one small and one blocked model each -- and only the gradient falls, never
    the LML.

    FINDING, stated rather than hidden: "the diagonal in the length-scale sums with weight h(0)" cannot be rejected for
    the RBF, Matern-3/2 and Matern-5/2 kernels, by these bars or any: the term is G_ii h(0) d2_ii with d2_ii = 0 and h(0)
    finite (1, 3, 5/3), an exact 0, so the slipped result is the honest one byte for byte (asserted below).  It is an error
    only for Matern-1/2, whose h(0) is infinite: there inf x 0 makes the length-scale entries NaN, which no bar passes
    (S3, C).  The other conditions of _applies are arithmetic too: a slip about tiles needs a second tile, one about
    dimensions >= 16 a seventeenth dimension, one about N mod 64 a remainder."""
    rejected = {slip: set() for slip in lr.SLIPS}
    for case in SLIP_CASES:
        honest = lc.f64_result(case)
        for slip in lr.SLIPS:
            if slip in lr.ARD_ONLY and not lc.config(case)["ard"]:
                continue
            res = lc.f64_result(case, slip)
            j = lc.judge(case, *res)
            worst = max(lc.KEYS, key=lambda k: j[k]["ratio"])
            print("%s with %s: %.3g of its bar (%s)%s" % (case, slip, j[worst]["ratio"], worst, "" if _applies(slip, case) else "  [changes nothing here]"))
            if not _applies(slip, case):
                assert lc.result_bytes(*res) == lc.result_bytes(*honest), (case, slip)
                continue
            assert not j["ok"], (case, slip, j)
            assert j["lml"]["ok"], (case, slip)
            if slip == "1/2 noise tr G with noise + jitter":       # a relative 1e-7 of one entry, and only that entry falls
                assert [k for k in lc.KEYS if not j[k]["ok"]] == ["noise"], (case, j)
            if slip in lr.ARD_ONLY or slip.startswith("the diagonal"):
                assert not j["length_scale"]["ok"] and j["noise"]["ok"], (case, slip, j)
            rejected[slip].add(lc.config(case)["path"])
    for slip, paths in rejected.items():
        assert paths == {"small", "blocked"}, (slip, paths)
