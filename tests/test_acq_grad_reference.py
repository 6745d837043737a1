"""CPU: the references of tests/test_gpu_acq_grad_edges.py judged before they judge anything.
 (a) Phi in long double (tests/acq_grad_reference_hp.py's own erfc) against scipy.special.ndtr and, where mpmath imports,
     against mpmath at 30 digits;
 (b) the 80-bit closed form of every acquisition's gradient against 80-bit central differences of the 80-bit value: the
     independent check of the formulas;
 (c) the f64 restatement against the 80-bit form on every batch of tests/acq_grad_edge_cases.py -- its errors are the e_ref
     the bars are built from, recorded in tests/golden/acq_grad_eref.json (written where ACQ_GRAD_WRITE=1) -- and the
     conditions a batch must meet to judge anything (the caps, no flat acquisition);
 (d) the bars reject the slips they exist for, each injected into the f64 restatement."""
import json
import os

import numpy as np
import pytest
from scipy.special import ndtr

import acq_grad_edge_cases as ac
import acq_grad_reference_hp as ar
import cov_edge_cases as ec

LD = np.longdouble
EREF_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acq_grad_eref.json")
BATCHES = [(name, "base") for name in ac.NAMES] + [("D", "tail%d" % m) for m in ac.M_FINAL] + [("F", "limit")]
FD_MODELS = [name for name in ac.NAMES if ac.MODELS[name]["N"] <= 300]
FD_STEP = 1e-5
# a central difference of step h is off by h^2 f''' / 6: some (h / l)^2 = 1e-9 of the gradient for the length scales here,
# times what the kernel's higher derivatives are worth near a training point.  The record holds what was measured (at most
# 8 x that passes); this ceiling holds whatever the record says, and a wrong formula (a sign, a factor, 1 / l_d) is of order 1.
FD_CEILING = 1e-6
SLIP_MODELS = ("D", "S2", "E", "G")           # ARD on the general path, the one-launch path, a wide model, the two-step judgement


def _record():
    with open(EREF_JSON) as f:
        return json.load(f)


# ---- (a) ----------------------------------------------------------------------------------------------------------------
def _grid():
    return np.concatenate([np.linspace(-30.0, 30.0, 2401), [-1e-300, 0.0, 1e-20, -1.4142135, -1.4142136, 1.4142135, 1.4142136, -37.5, 8.3]])


def test_phi_against_ndtr():
    """to a few f64 ulps of the value, where "a few" grows with z^2 in the lower tail: ndtr forms z / sqrt(2) (two
    roundings, 2 u relative) and its square (one more), and d log Phi / d log z is -z^2 there, so 2.5 z^2 u of the
    difference is ndtr's own argument: the bar is (8 + 4 z^2) u, 8 u at the centre"""
    z = _grid()
    got, want = ar.Phi(z), ndtr(z)
    rel = np.abs(want.astype(LD) - got) / got
    worst = float((rel / ((8 + 4 * z * z) * ac.U)).max())
    print("Phi against ndtr: at most %.3g of (8 + 4 z^2) u; %.3g u over |z| <= 1" % (worst, float(rel[np.abs(z) <= 1].max() / ac.U)))
    assert worst <= 1.0
    assert np.all(np.diff(got[:1201]) > 0) and np.all(np.diff(got[:2401]) >= 0) and got[2400] <= 1 and float(ar.Phi(np.array([0.0]))[0]) == 0.5


def test_phi_against_mpmath():
    mp = pytest.importorskip("mpmath")        # (judges the reference, not the library)
    mp.mp.dps = 40
    z = _grid()
    got = ar.Phi(z)
    want = np.array([LD(mp.nstr(mp.ncdf(mp.mpf(float(x))), 30)) for x in z])
    rel = np.abs(got - want) / want
    eps = float(np.finfo(LD).eps)
    worst = float((rel / ((16 + 4 * z * z) * eps)).max())      # the same argument one format up
    print("Phi against mpmath: at most %.3g of (16 + 4 z^2) eps; %.3g eps over |z| <= 3" % (worst, float(rel[np.abs(z) <= 3].max() / eps)))
    assert worst <= 1.0
    p = ar.pdf(z)
    wantp = np.array([LD(mp.nstr(mp.npdf(mp.mpf(float(x))), 30)) for x in z])
    assert float((np.abs(p - wantp) / wantp / ((16 + 4 * z * z) * eps)).max()) <= 1.0


# ---- (b) ----------------------------------------------------------------------------------------------------------------
_fd = {}


def fd_agreement(name):
    """{key: max |closed form - central difference| over the batch's maximum of |gradient|}, base batch, 80 bits
    throughout; Matern-1/2 without row 5 (the function has a kink at a training point; the closed form's convention
    there is stated in tests/acq_grad_reference_hp.py)"""
    if name not in _fd:
        fit, Xq = ec.hp_fit(name), ac.points(name)
        keep = np.arange(len(Xq)) != 5 if ac.MODELS[name]["kind"] == "matern12" else np.ones(len(Xq), dtype=bool)
        mup, mum, sgp, sgm = ar.central_differences(fit, Xq, FD_STEP)
        ref, sc = ac.hp_reference(name), ac.scales(name)
        out = {}
        for key, (q, _, sf, which, param) in ac.CASES.items():
            inc = ac.incumbent(name, which)
            fp, fm = ar.acquisition(q, mup, sgp, sf, inc, param)[0], ar.acquisition(q, mum, sgm, sf, inc, param)[0]
            out[key] = ac._fraction(((fp - fm) / (LD(2) * LD(FD_STEP)))[keep], ref[key][1][keep], sc[key][1])
        _fd[name] = out
    return _fd[name]


@pytest.mark.parametrize("name", FD_MODELS)
def test_the_closed_form_against_central_differences(name):
    got = fd_agreement(name)
    rec = _record()["central_differences"].get(name, {}) if os.environ.get("ACQ_GRAD_WRITE") != "1" else got
    for key, v in got.items():
        print("%s %-7s closed form against central differences (h = %g): %.3g of the batch maximum" % (name, key, FD_STEP, v))
    for key, v in got.items():
        assert v <= FD_CEILING, (name, key, v)
        assert v <= 8 * max(rec[key], 1e-12), (name, key, v, rec[key])     # (below 1e-12 the difference is rounding of the 80-bit values over 2 h)


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,batch", BATCHES)
def test_the_batch_can_judge(name, batch):
    e, fl, sc = ac.e_ref(name, batch), ac.flatness(name, batch), ac.scales(name, batch)
    m, I = ac.rows(batch)
    assert len(I) == len(set(I.tolist())) and I.max() < m
    assert (5 in I) == (batch == "base")                     # the training point among the queries stays in
    beyond = ac.BEYOND_THE_CAP.get(name, ())
    for key in ac.KEYS:
        print("%s %s %-7s e_ref value %.3g gradient %.3g; max |gradient| %.3g of prior scale / smallest length scale"
              % (name, batch, key, e[key][0], e[key][1], fl[key]))
        if (name, key) == ("S1", "mu"):                      # identically zero (the module's docstring): exact zeros are asked for
            assert sc[key][1] == 0.0 and e[key][1] == 0.0
        else:
            assert fl[key] >= ac.FLAT, (name, batch, key, fl[key])
        assert sc[key][0] > 0
        if key in beyond:                                    # listed because it IS beyond the cap, not for convenience
            assert 10 * max(e[key]) > ac.CAP, (name, key, e[key])
    bars = ac.bars(name, batch)                              # (asserts the cap's condition for every case it returns)
    assert sorted(bars) == sorted(k for k in ac.KEYS if k not in beyond)
    assert all(b <= (ac.APPEND_BAR if ac.MODELS[name].get("append") else ac.CAP) for bb in bars.values() for b in bb)
    j = ac.judge(name, batch, ac.f64_results(name, batch))  # the honest f64 computation passes, the two-step cases included
    ac.show(name, batch + " f64 restatement", j)
    assert j["ok"], j
    assert all(j[key]["bar_value"] <= ac.CAP and j[key]["bar_grad"] <= ac.CAP for key in ac.KEYS)


def test_the_recorded_e_ref():
    """tests/golden/acq_grad_eref.json is the record; a fresh value is at most 4 x the recorded one (more would mean the
    reference, the data or the arithmetic under them changed).  Below 8 u of the scale a value is last-bit noise of
    the BLAS underneath and is compared as 8 u."""
    fresh = {}
    for name, batch in BATCHES:
        fresh.setdefault(name, {})[batch] = {key: list(v) for key, v in ac.e_ref(name, batch).items()}
    if os.environ.get("ACQ_GRAD_WRITE") == "1":
        with open(EREF_JSON, "w") as f:
            json.dump(dict(unit="fraction of the batch's 80-bit maximum of the quantity's magnitude (the value of mu: of the prior scale); [value, gradient]",
                           e_ref=fresh, central_differences={name: fd_agreement(name) for name in FD_MODELS},
                           central_differences_unit="max |80-bit closed form - 80-bit central difference, h = 1e-5| over the base batch's maximum of |gradient|"),
                      f, indent=1, sort_keys=True)
    rec = _record()["e_ref"]
    assert sorted(rec) == sorted(fresh)
    floor = 8 * ac.U
    for name in fresh:
        assert sorted(rec[name]) == sorted(fresh[name])
        for batch in fresh[name]:
            assert sorted(rec[name][batch]) == sorted(fresh[name][batch])
            for key, v in fresh[name][batch].items():
                for a, b in zip(v, rec[name][batch][key]):
                    assert max(a, floor) <= 4 * max(b, floor), (name, batch, key, v, rec[name][batch][key])


# ---- (d) the bars have teeth -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SLIP_MODELS)
def test_the_bars_reject_the_slips(name):
    for slip in ar.SLIPS:
        j = ac.judge(name, "base", ac.f64_results(name, "base", slip))
        worst = max(((j[k]["ratio_value"], k + " value") for k in ac.KEYS), key=lambda t: t[0])
        worstg = max(((j[k]["ratio_grad"], k + " gradient") for k in ac.KEYS), key=lambda t: t[0])
        print("%s with %s: %.3g of its bar (%s), %.3g (%s)" % (name, slip, worst[0], worst[1], worstg[0], worstg[1]))
        assert not j["ok"], (name, slip)
        if slip == "cs of PI without its Z":                 # only PI's gradient is wrong, and only that fails
            assert [k for k in ac.KEYS if not j[k]["ok"]] == ["pi_min", "pi_max"], j
            assert all(j[k]["ratio_value"] <= 1.0 for k in ac.KEYS)
        if slip == "ls[0] for every dimension":              # the values stand; every gradient judged by the 80-bit posterior falls
            assert all(j[k]["ratio_value"] <= 1.0 for k in ac.KEYS), j
            assert all(j[k]["ratio_grad"] > 1.0 for k in ac.KEYS if k not in ac.BEYOND_THE_CAP.get(name, ())), j
