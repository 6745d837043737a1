"""GPU: tgp_ehvi_set_front and tgp_sweep_ehvi -- the two-objective expected hypervolume improvement over the resident
batch -- in tiers: identity (mu, sigma, mu2, sigma2 are the bits of the handles' own predict-only sweeps), the pure-function
tier (the mpmath formula applied to those bits, under the derived bar of tests/ehvi_reference.py::bound), cross-entry
(P = 0 against the product of two tgp_sweep EIs; the arg-max rule), bits (a value depends on its posterior bits alone; the
front may come from a permuted Y with dominated points added) and the degenerate rows.  Problems: tests/ehvi_cases.py.
Every figure is printed before it is asserted; the last test writes them where EHVI_PARITY_JSON names a file
(profiles/ehvi_parity.json)."""
import faulthandler
import json
import math
import os

import numpy as np
import pytest

import ehvi_cases as ec
import ehvi_reference as er

pytestmark = pytest.mark.gpu
RECORD = {}
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ehvi_eref.json")) as _f:
    E_REF = float(json.load(_f)["e_ref"])
MP_ROWS = 12      # rows per case the mpmath form is applied to where 2 (P + 1) M evaluations of it would take minutes


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def L():
    import turbo_amd._lib as lib
    return lib


def _call(h, g, **kw):
    a = dict(want_mu=True, want_sigma=True, want_second=True, want_value=True)
    a.update(kw)
    return h.sweep_ehvi(g, **a)


def _pure_function(name, a, c, sf, r, beyond=0):
    """every row against the f64 reference at the returned bits (both sides of that comparison carry the bar), and the
    mpmath form on all rows (small P and M) or on MP_ROWS of them: the first, the last, the winner, rows past `beyond`
    (the capped grid's second trip) and an even spread"""
    M = r["value"].shape[0]
    ref = er.sweep(a, c, sf, r["mu"], r["sigma"], r["mu2"], r["sigma2"])
    bar = er.bound(ref["scale"], E_REF)
    err = np.abs(r["value"] - ref["value"])
    ratio = float((err / np.maximum(2 * bar, er.TINY)).max())
    rows = np.arange(M) if M * len(c) <= 4000 else np.unique(np.concatenate(
        [[0, M - 1, r["best_idx"], min(beyond, M - 1), min(beyond + 257, M - 1)], np.linspace(0, M - 1, MP_ROWS - 5).astype(int)]))
    worst = 0.0
    for i in rows:
        want = er.value_mp(a, c, sf[0] * r["mu"][i], r["sigma"][i], sf[1] * r["mu2"][i], r["sigma2"][i])
        got = float(r["value"][i])
        if got == 0.0 and want < er.TINY:
            continue
        e = abs(float(want - got))
        worst = max(worst, e / max(bar[i], er.TINY))
        assert e <= bar[i], (name, i, got, float(want), e, bar[i])
    print("%s: value in [%.3g, %.3g]; against f64 reference max err / (2 bar) %.3g; against mpmath on %d rows max err / bar %.3g; e_ref %.3g"
          % (name, np.nanmin(r["value"]), np.nanmax(r["value"]), ratio, len(rows), worst, E_REF))
    RECORD[name] = dict(f64_err_over_2bar=ratio, mp_err_over_bar=worst, mp_rows=int(len(rows)), value_max=float(np.nanmax(r["value"])))
    assert np.all(err <= 2 * bar)


@pytest.mark.parametrize("name", list(ec.CASES))
def test_identity_and_the_pure_function_tier(L, name):
    p = ec.problem(name)
    h, g = ec.handles(L, name)
    M = p["Xc"].shape[0]
    before = h.sweep(L.ACQ_EI, 1.0, 0.1, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    r = _call(h, g)
    # identity, in every dtype: the same handles' own predict-only sweeps of the same rows
    own = h.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
    assert own["mu"].tobytes() == r["mu"].tobytes() and own["sigma"].tobytes() == r["sigma"].tobytes()
    assert g.M == M
    s = g.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
    assert s["mu"].tobytes() == r["mu2"].tobytes() and s["sigma"].tobytes() == r["sigma2"].tobytes()
    assert r["n_clamped"] == own["n_clamped"] + s["n_clamped"]
    # h's state is untouched
    after = h.sweep(L.ACQ_EI, 1.0, 0.1, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    for key in ("mu", "sigma", "acq"):
        assert after[key].tobytes() == before[key].tobytes(), key
    assert (after["best_idx"], after["best_val"]) == (before["best_idx"], before["best_val"])
    if M <= 1000:
        assert np.array_equal(h.read_candidates(), p["Xc"]) and np.array_equal(g.read_candidates(), p["Xc"])
    a, c = ec.strips_of(name)
    _pure_function(name, a, c, p["sf"], r, beyond=768 * 256)
    # the arg-max of the returned values under the library-wide rule; arg-max only gives the same record
    assert (r["best_idx"], r["best_val"]) == er.argmax(r["value"])
    r2 = _call(h, g, want_mu=False, want_sigma=False, want_second=False, want_value=False)
    assert (r2["best_idx"], r2["best_val"], r2["n_clamped"]) == (r["best_idx"], r["best_val"], r["n_clamped"])
    assert r["value"].max() > 0.0
    g.close()
    h.close()


def test_empty_front_is_the_product_of_two_eis(L):
    """P = 0 on f64 handles: e_1(r_1) e_2(r_2) against the product of the handles' tgp_sweep EI at incumbent ref_j, xi = 0,
    within 4 u.  The reference point lies a whole observed range below the worst observation, so that every candidate has
    z > 0 on both models (asserted): tgp_sweep's EI forms its two halves separately for z < 0 and carries z^2 u there, which
    is that entry's error, not this one's."""
    name = "n200x300_m777_p0"
    p = ec.problem(name)
    h, g = ec.handles(L, name)
    sf = np.asarray(p["sf"])
    lo = np.array([(sf[0] * p["y1"]).min(), (sf[1] * p["y2"]).min()])
    hi = np.array([(sf[0] * p["y1"]).max(), (sf[1] * p["y2"]).max()])
    ref = sf * (lo - (hi - lo))
    front, hv = h.ehvi_set_front(np.zeros((0, 2)), ref, p["sf"])
    assert front.shape == (0, 2) and hv == 0.0
    r = _call(h, g)
    z1, z2 = sf[0] * (r["mu"] - ref[0]) / r["sigma"], sf[1] * (r["mu2"] - ref[1]) / r["sigma2"]
    assert z1.min() > 0 and z2.min() > 0
    e1 = h.sweep(L.ACQ_EI, p["sf"][0], float(ref[0]), 0.0, want_acq=True)["acq"]
    e2 = g.sweep(L.ACQ_EI, p["sf"][1], float(ref[1]), 0.0, want_acq=True)["acq"]
    want = e1 * e2
    rel = float((np.abs(r["value"] - want) / want).max())
    print("P = 0: max relative difference to EI_1 EI_2 %.3g u (z in [%.2f, %.2f])" % (rel / er.U, min(z1.min(), z2.min()), max(z1.max(), z2.max())))
    RECORD["p0 product of EIs"] = dict(rel_over_u=rel / er.U)
    assert rel <= 4 * er.U
    g.close()
    h.close()


def test_second_objective_on_a_private_stream_returns_the_same_bits(L):
    name = "n300x200_m777_p255"
    h, g = ec.handles(L, name)
    base = _call(h, g)
    h2, g2 = ec.handles(L, name, private=True)
    for _ in range(2):
        got = _call(h2, g2)
        for key in ("mu", "sigma", "mu2", "sigma2", "value"):
            assert got[key].tobytes() == base[key].tobytes(), key
        assert (got["best_idx"], got["best_val"], got["n_clamped"]) == (base["best_idx"], base["best_val"], base["n_clamped"])
    for x in (g, h, g2, h2):
        x.close()


def test_a_values_bits_depend_on_its_posterior_bits_alone(L):
    """the same rows at another M and other positions: wherever the four posterior values are the same bits (they are the
    sweeps' business), so is the value; and a front set from a permuted Y with more dominated points gives every bit again"""
    name = "n300x300_m777_p256"
    p = ec.problem(name)
    h, g = ec.handles(L, name)
    base = _call(h, g)
    key = lambda r, i: (r["mu"][i].tobytes(), r["sigma"][i].tobytes(), r["mu2"][i].tobytes(), r["sigma2"][i].tobytes())
    known = {key(base, i): base["value"][i].tobytes() for i in range(777)}
    for rows in (np.arange(776, 519, -1), np.array([5]), np.arange(255)):
        h.set_candidates(p["Xc"][rows])
        r = _call(h, g)
        hit = [i for i in range(len(rows)) if key(r, i) in known]
        print("M = %d: %d rows with the posterior bits of the M = 777 batch" % (len(rows), len(hit)))
        assert all(known[key(r, i)] == r["value"][i].tobytes() for i in hit)
        ref = er.sweep(*ec.strips_of(name), p["sf"], r["mu"], r["sigma"], r["mu2"], r["sigma2"])
        assert np.all(np.abs(r["value"] - ref["value"]) <= 2 * er.bound(ref["scale"], E_REF))
    h.set_candidates(p["Xc"])
    rng = np.random.RandomState(9)
    sf = np.asarray(p["sf"])
    more = np.concatenate([p["Y"], p["Y"] - sf * rng.uniform(0.0, 0.3, p["Y"].shape)])        # worse in both oriented coordinates
    front, hv = h.ehvi_set_front(more[rng.permutation(more.shape[0])], p["ref"], p["sf"])
    assert front.shape[0] == p["P"]
    again = _call(h, g)
    assert again["value"].tobytes() == base["value"].tobytes()
    g.close()
    h.close()


def test_set_front_against_the_reference_builder(L):
    h = L.NativeGP(0, "f64")                                          # no fitted model needed
    rng = np.random.RandomState(2)
    cases = [np.array([[1.0, 3.0], [1.0, 3.0], [2.0, 2.0], [2.0, 1.5], [1.5, 2.0], [3.0, 1.0], [0.0, 5.0], [5.0, 0.0], [0.5, 0.5]]),
             np.array([[0.0, 1.0], [-1.0, -1.0]]), np.zeros((0, 2)), rng.normal(size=(400, 2)) + 1.0]
    for Y in cases:
        for sf in ((1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0)):
            Ys = Y * np.asarray(sf)
            F, raw, idx, hv = er.front(Ys, sf, (0.0, 0.0))
            front, got_hv = h.ehvi_set_front(Ys, (0.0, 0.0), sf)
            assert front.tolist() == raw.tolist(), (Y.shape, sf)
            assert abs(got_hv - hv) <= 8 * er.U * max(len(F), 1) * hv
    # refusals: the previous front is untouched
    p = ec.problem("n200x12_m257_p2")
    hh, g = ec.handles(L, "n200x12_m257_p2")
    base = _call(hh, g)
    Y257 = ec.staircase(257, (1.0, 1.0), (0.0, 0.0), (1.0, 1.0), rng)
    for args, text in (((np.array([[1.0, np.nan]]), (0.0, 0.0), (1.0, 1.0)), "finite"), ((p["Y"], (0.0, np.inf), (1.0, 1.0)), "ref"),
                       ((p["Y"], (0.0, 0.0), (0.5, 1.0)), "sf"), ((p["Y"], (0.0, 0.0), (1.0, 0.0)), "sf"), ((Y257, (-1.0, -1.0), (1.0, 1.0)), "256")):
        with pytest.raises(ValueError, match=text):
            hh.ehvi_set_front(*args)
    assert _call(hh, g)["value"].tobytes() == base["value"].tobytes()
    Y256 = ec.staircase(256, (1.0, 1.0), (0.0, 0.0), (1.0, 1.0), rng)
    front, _ = hh.ehvi_set_front(Y256, (-1.0, -1.0), (1.0, 1.0))
    assert front.shape == (256, 2)
    # the front survives a refit and a new batch
    hh.fit(p["X1"], p["y1"], p["kind"], ec.C, p["ls"], ec.NOISE, ec.JITTER, True)
    hh.set_candidates(p["Xc"][:50])
    r = _call(hh, g)
    F, _, _, _ = er.front(Y256, (1.0, 1.0), (-1.0, -1.0))
    ref = er.sweep(*er.strips(F, (-1.0, -1.0)), (1.0, 1.0), r["mu"], r["sigma"], r["mu2"], r["sigma2"])
    assert np.all(np.abs(r["value"] - ref["value"]) <= 2 * er.bound(ref["scale"], E_REF))
    for x in (h, hh, g):
        x.close()


def _two_models(L, noise2=ec.NOISE, jitter2=ec.JITTER, kind="matern12"):
    rng = np.random.RandomState(5)
    X1, X2 = rng.uniform(0, 1, (40, 3)), rng.uniform(0, 1, (12, 3))
    ya, yb = ec.y1(X1, rng), ec.y2(X2, rng)
    h = ec.fit_handle(L, "f64", X1, ya, kind, np.full(1, ec.LS))
    g = ec.fit_handle(L, "f64", X2, yb, kind, np.full(1, ec.LS), noise=noise2, jitter=jitter2)
    return h, g, X1, X2, ya, yb, rng


def test_zero_sigma_rows_and_a_nan_row(L):
    """objective 2 with noise 0 and jitter 0 (Matern-1/2: K is factored as it is) and a batch that contains its training
    points: sigma_2 == 0 there, e_2 = max(m_2 - t, 0); a NaN row never wins"""
    h, g, X1, X2, ya, yb, rng = _two_models(L, 0.0, 0.0)
    Xc = np.vstack([X2, rng.uniform(0, 1, (20, 3)), np.full((1, 3), np.nan)])
    h.set_candidates(Xc)
    Y = np.array([[0.2, 0.9], [0.6, 0.5], [0.9, 0.1]])
    ref = (float(ya.min()) - 0.5, float(yb.min()) - 0.5)
    h.ehvi_set_front(Y, ref, (1.0, 1.0))
    r = _call(h, g)
    zero = r["sigma2"] == 0.0
    print("zero sigma: sigma_2 == 0 at %d of the 12 training points, %d clamped" % (int(zero[:12].sum()), r["n_clamped"]))
    assert zero[:12].any(), "the clamp was not reached: this case judges nothing"
    F, _, _, _ = er.front(Y, (1.0, 1.0), ref)
    a, c = er.strips(F, ref)
    _pure_function("zero sigma", a, c, (1.0, 1.0), dict(r, value=r["value"][:-1], mu=r["mu"][:-1], sigma=r["sigma"][:-1], mu2=r["mu2"][:-1],
                                                       sigma2=r["sigma2"][:-1], best_idx=min(r["best_idx"], 31)))
    assert r["value"][:-1][zero[:-1]].max() > 0.0
    assert math.isnan(r["value"][-1]) and r["best_idx"] != Xc.shape[0] - 1
    assert (r["best_idx"], r["best_val"]) == er.argmax(r["value"])
    g.close()
    h.close()


def test_forty_sigma_below_the_reference_point_and_an_all_zero_batch(L):
    h, g, X1, X2, ya, yb, rng = _two_models(L, kind="rbf")
    Xc = np.vstack([X1[:3], rng.uniform(-0.2, 1.2, (60, 3))])
    h.set_candidates(Xc)
    own = h.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
    i0 = int(np.argmin(own["sigma"]))
    r2 = float(yb.min()) - 0.5
    # row i0 lies 41 of its deviations below r_1; a row with a deviation ten times that is 4.1 below
    h.ehvi_set_front(np.zeros((0, 2)), (float(own["mu"][i0] + 41.0 * own["sigma"][i0]), r2), (1.0, 1.0))
    r = _call(h, g)
    z = (r["mu"] - (own["mu"][i0] + 41.0 * own["sigma"][i0])) / r["sigma"]
    print("40 sigma: z_1 in [%.1f, %.1f], values in [%.3g, %.3g]" % (z.min(), z.max(), r["value"].min(), r["value"].max()))
    assert z[i0] <= -40.0 and r["value"][i0] == 0.0
    assert r["value"].max() > 0.0 and r["best_idx"] != i0 and (r["best_idx"], r["best_val"]) == er.argmax(r["value"])
    # every row 41 deviations below: exact zeros, index 0 wins
    h.ehvi_set_front(np.zeros((0, 2)), (float((own["mu"] + 41.0 * own["sigma"]).max()), r2), (1.0, 1.0))
    r = _call(h, g)
    assert not r["value"].any() and (r["best_idx"], r["best_val"]) == (0, 0.0)
    g.close()
    h.close()


def test_the_error_lines_that_need_a_device(L):
    name = "n12x200_m1_p0"
    p = ec.problem(name)
    h, g = ec.handles(L, name)

    def refused(hh, gg, status, text):
        rc = hh.lib.tgp_sweep_ehvi(hh._h, gg._h if gg is not None else None, *([None] * 8))
        assert rc == status, (rc, status, text)
        assert text in hh.lib.tgp_last_error(hh._h).decode(), hh.lib.tgp_last_error(hh._h).decode()
    other_d = L.NativeGP(0, "f64")
    other_d.fit(p["X2"][:, :2], p["y2"], "rbf", 1.0, [0.4], 1e-3, 1e-10, True)
    unfitted = L.NativeGP(0, "f64")
    nofront = ec.fit_handle(L, "f64", p["X1"], p["y1"], p["kind"], p["ls"])
    nofront.set_candidates(p["Xc"])
    refused(nofront, g, 2, "no front set")
    refused(h, h, 2, "two handles")
    refused(h, None, 2, "NULL")
    refused(h, other_d, 2, "D differs")
    refused(h, unfitted, 4, "no fitted model")
    unfitted.ehvi_set_front(p["Y"], p["ref"], p["sf"])
    refused(unfitted, g, 4, "no fitted model")
    lo, hi = np.full(3, -0.2), np.full(3, 1.2)
    h.warp_candidates(lo, hi, np.full(3, 1.5), np.full(3, 0.8))
    refused(h, g, 2, "warped")
    fresh = ec.fit_handle(L, "f64", p["X1"], p["y1"], p["kind"], p["ls"])          # fitted, a front, no candidates
    fresh.ehvi_set_front(p["Y"], p["ref"], p["sf"])
    refused(fresh, g, 2, "no candidates")
    with pytest.raises(ValueError, match="m <= 4096"):
        h.ehvi_grad(np.zeros((4097, 3)), g)
    with pytest.raises(ValueError, match="no front"):
        nofront.ehvi_grad(p["Xc"], g)
    h.set_candidates(p["Xc"])
    assert np.all(np.isfinite(_call(h, g)["value"]))                 # and the handles still work
    for x in (other_d, unfitted, nofront, fresh, g, h):
        x.close()


def test_record_the_figures():
    """(last in the file) where EHVI_PARITY_JSON names a file, the figures seen above go there"""
    out = os.environ.get("EHVI_PARITY_JSON")
    if out and RECORD:
        with open(out, "w") as f:
            json.dump(dict(unit="value: absolute error at the returned posterior bits as a fraction of the bar 64 max(e_ref, u) sum_i "
                                "(e_1(a_i) + e_1(a_{i+1})) e_2(c_i) (3 + z_-^2 ...) -- against mpmath on mp_rows rows, against the f64 "
                                "reference (twice the bar) on all", e_ref=E_REF, cases=RECORD), f, indent=1, sort_keys=True)
    for name, rec in RECORD.items():
        for key in ("f64_err_over_2bar", "mp_err_over_bar"):
            assert rec.get(key, 0.0) <= 1.0, (name, key, rec)
