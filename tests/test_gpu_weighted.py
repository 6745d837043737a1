"""GPU: tgp_sweep_weighted -- the objective's EI / PI weighted by the side models' feasibility and cost -- in four tiers:
identity (mu, sigma, side_mu, side_sigma are the bits of the handles' own predict-only sweeps), the pure-function tier (the
mpmath formula applied to those bits, under the derived bar of tests/weighted_reference.py::bound), the independent tier
(per-model oracle fit + predict) and the state every handle is left in.  Problems: tests/weighted_cases.py.  Every figure
is printed before it is asserted; the last test writes them where WEIGHTED_PARITY_JSON names a file
(profiles/weighted_parity.json)."""
import faulthandler
import json
import math
import os

import numpy as np
import pytest

import weighted_cases as wc
import weighted_reference as wr

pytestmark = pytest.mark.gpu
RECORD = {}
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "weighted_eref.json")) as _f:
    E_REF = float(json.load(_f)["e_ref"])


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


def _call(h, sides, p, **kw):
    a = dict(acq=p["acq"], sf=p["sf"], incumbent=p["incumbent"], param=p["param"], want_mu=True, want_sigma=True, want_acq=True,
             want_logw=True, want_value=True, want_sides=True)
    a.update(kw)
    return h.sweep_weighted(sides, **a)


def _pure_function(name, p, r, kinds_levels):
    """the mpmath formula applied to the bits the library returned for the sides' mu and sigma (and, for the value, to the
    unweighted acquisition it returned: that one's own accuracy is the plain sweep's tests' business)"""
    ref_logw, ref_logf = wc.logw_mp(kinds_levels, r["side_mu"], r["side_sigma"])
    bar = wr.bound(ref_logf, E_REF) if len(kinds_levels) else np.zeros(r["logw"].shape[0])
    fin = np.isfinite(ref_logw)
    assert np.array_equal(np.isfinite(r["logw"]), fin) and np.array_equal(r["logw"][~fin], ref_logw[~fin])
    err = np.abs(r["logw"][fin] - ref_logw[fin])
    ratio = float((err / np.maximum(bar[fin], 1e-300)).max()) if fin.any() and len(kinds_levels) else 0.0
    ref_val = wc.value_mp(p["acq"], r["acq"], ref_logw)
    if p["acq"] == wr.ACQ_NONE:
        verr, vbar = np.abs(r["value"][fin] - ref_val[fin]), bar[fin]
    else:
        verr, vbar = np.abs(r["value"] - ref_val), np.abs(ref_val) * (bar + 4 * wr.U)
    vratio = float((verr / np.maximum(vbar, 1e-300)).max()) if (verr > 0).any() else 0.0
    print("%s: logw max err %.3g (max err / bar %.3g), value max err / bar %.3g, e_ref %.3g" % (name, err.max() if err.size else 0.0, ratio, vratio, E_REF))
    RECORD[name] = dict(logw_max_err=float(err.max()) if err.size else 0.0, logw_err_over_bar=ratio, value_err_over_bar=vratio)
    assert np.all(err <= bar[fin]) and np.all(verr <= vbar)


@pytest.mark.parametrize("name", list(wc.CASES))
def test_identity_and_the_pure_function_tier(L, name):
    p = wc.problem(name)
    h, sides = wc.handles(L, name)
    K, M = len(sides), p["Xc"].shape[0]
    r = _call(h, sides, p)
    # identity, in every dtype: the same handles' own predict-only sweeps of the same rows
    own = h.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
    assert own["mu"].tobytes() == r["mu"].tobytes() and own["sigma"].tobytes() == r["sigma"].tobytes()
    clamped = own["n_clamped"]
    for k, (g, _, _) in enumerate(sides):
        assert g.M == M
        s = g.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
        assert s["mu"].tobytes() == r["side_mu"][k].tobytes() and s["sigma"].tobytes() == r["side_sigma"][k].tobytes(), k
        clamped += s["n_clamped"]
    assert r["n_clamped"] == clamped
    if p["dtypes"][0] == "f64" and p["acq"] != wr.ACQ_NONE:         # the unweighted acquisition, as tgp_sweep returns it
        a = h.sweep(p["acq"], p["sf"], p["incumbent"], p["param"], want_acq=True)
        assert a["acq"].tobytes() == r["acq"].tobytes()
        if K == 0:                                                   # K = 0: tgp_sweep's winner, bit for bit
            assert (a["best_idx"], a["best_val"]) == (r["best_idx"], r["best_val"])
            assert r["value"].tobytes() == r["acq"].tobytes() and not r["logw"].any()
    _pure_function(name, p, r, [(k, lv) for _, k, lv in sides])
    # the arg-max of the returned values under the library-wide rule; arg-max only gives the same record
    bi, bv = wr.argmax(r["value"])
    assert (r["best_idx"], r["best_val"]) == (bi, bv)
    r2 = _call(h, sides, p, want_mu=False, want_sigma=False, want_acq=False, want_logw=False, want_value=False, want_sides=False)
    assert (r2["best_idx"], r2["best_val"], r2["n_clamped"]) == (r["best_idx"], r["best_val"], r["n_clamped"])
    wc.close(h, sides)


def test_a_side_on_a_private_stream_returns_the_same_bits(L):
    name = "n300x200_m777_k8"
    p = wc.problem(name)
    h, sides = wc.handles(L, name)
    base = _call(h, sides, p)
    h2, sides2 = wc.handles(L, name, private=(1, 2, 3))              # a one-workgroup, a general and a one-launch side
    got = _call(h2, sides2, p)
    for key in ("mu", "sigma", "acq", "logw", "value", "side_mu", "side_sigma"):
        assert got[key].tobytes() == base[key].tobytes(), key
    assert (got["best_idx"], got["best_val"], got["n_clamped"]) == (base["best_idx"], base["best_val"], base["n_clamped"])
    wc.close(h, sides)
    wc.close(h2, sides2)


@pytest.mark.parametrize("name", ["n200x12_m33_k2", "n300x200_m777_k8"])
def test_the_independent_oracle_tier(L, name):
    """per-model oracle fit + predict on f64 handles: the winner on a batch whose reference winner leads by more than 100 x
    the tolerance, and best_val within the parity tolerances propagated through the reference's own partials"""
    p = wc.problem(name)
    M = p["Xc"].shape[0]

    def score(pool):
        return wc.oracle_sweep(name, pool)["value"]

    def need(pool, s, best):
        r = wc.oracle_sweep(name, pool)
        return 100.0 * float(wc.oracle_value_tolerance(name, r)[best])
    Xc, pos, gap = wc.pooled_batch(name, M, score, need)
    ref = wc.oracle_sweep(name, Xc)
    tol = float(wc.oracle_value_tolerance(name, ref)[pos])
    srt = np.sort(ref["value"])
    assert ref["best_idx"] == pos and srt[-1] - srt[-2] > 100.0 * tol            # on the reference first
    h, sides = wc.handles(L, name)
    h.set_candidates(Xc)
    r = _call(h, sides, p)
    print("%s: oracle tier |best_val - ref| %.3g (tol %.3g), gap %.3g" % (name, abs(r["best_val"] - ref["best_val"]), tol, srt[-1] - srt[-2]))
    RECORD[name + " oracle"] = dict(best_val_err=abs(r["best_val"] - ref["best_val"]), tol=tol)
    assert r["best_idx"] == ref["best_idx"]
    assert abs(r["best_val"] - ref["best_val"]) <= tol
    wc.close(h, sides)


def _underflow_problem(L):
    """one GE side whose level lies 45 of its posterior deviations above its mean on every row of the pool"""
    from oracle import gp_oracle as o
    name = "n200x12_m33_k2"
    p = wc.problem(name)
    Xk, yk = p["sides"][0][0], p["sides"][0][1]
    om = o.fit(Xk, yk, p["kind"], wc.C, p["ls"], wc.NOISE, wc.JITTER, True)
    state = {}

    def score(pool):
        mu, sg = o.predict(om, pool)
        state.setdefault("level", float((mu + 45.0 * sg).max()))     # (the pool is drawn once: the level is the pool's)
        return wr.side_logf(wr.GE, state["level"], mu, sg)

    def need(pool, s, best):
        mu, sg = o.predict(om, pool)
        z = (mu - state["level"]) / sg
        # the bar on logw, and the oracle's own posterior tolerances through d log Phi / d z = phi / Phi ~ |z|
        dz = (wc.RTOL * np.abs(mu) + 1e-9) / sg + np.abs(z) * (wc.RTOL * sg * sg + wc.VAR_ATOL * (wc.C + wc.NOISE) * om.y_std ** 2) / (2 * sg * sg)
        ratio = wr.logphi(z)[1]
        return 100.0 * float(wr.bound(s[None, :], E_REF)[best] + (ratio * dz)[best])
    Xc, pos, gap = wc.pooled_batch("underflow", 33, score, need, pool_factor=8)
    mu, sg = o.predict(om, Xc)
    return p, Xk, yk, state["level"], Xc, pos, (mu - state["level"]) / sg


def test_underflow_a_feasibility_of_1e_400_still_orders_the_batch(L):
    p, Xk, yk, level, Xc, pos, z = _underflow_problem(L)
    assert np.all(z <= -40.0)                                        # on the reference first
    h = wc.fit_handle(L, "f64", p["X"], p["y"], p["kind"], p["ls"])
    g = wc.fit_handle(L, "f64", Xk, yk, p["kind"], p["ls"])
    h.set_candidates(Xc)
    sides = [(g, "ge", level)]
    ei = h.sweep_weighted(sides, L.ACQ_EI, -1.0, float(p["y"].min()), wc.XI, want_logw=True, want_value=True, want_sides=True, want_acq=True)
    ref_logw, ref_logf = wc.logw_mp([(wr.GE, level)], ei["side_mu"], ei["side_sigma"])
    bar = wr.bound(ref_logf, E_REF)
    print("underflow: logw in [%.4g, %.4g], max err / bar %.3g" % (ei["logw"].min(), ei["logw"].max(), float((np.abs(ei["logw"] - ref_logw) / bar).max())))
    RECORD["underflow"] = dict(logw_min=float(ei["logw"].min()), logw_max=float(ei["logw"].max()), logw_err_over_bar=float((np.abs(ei["logw"] - ref_logw) / bar).max()))
    assert np.all(np.isfinite(ei["logw"])) and np.all(np.abs(ei["logw"] - ref_logw) <= bar)
    assert ei["logw"].max() < -745.0 and not ei["value"].any() and ei["acq"].any()       # exactly 0 under EI
    none = h.sweep_weighted(sides, L.ACQ_NONE, want_value=True)
    assert none["value"].tobytes() == ei["logw"].tobytes()
    assert none["best_idx"] == pos and none["best_val"] == ei["logw"][pos]
    wc.close(h, sides)


def test_a_step_function_side_and_a_nan_row(L):
    """a side with noise 0 and jitter 0 (Matern-1/2: K is factored as it is) and a batch that contains its training points:
    sigma_k == 0 there, so f_k is 1 at or above the level and 0 below; a NaN row never wins"""
    p = wc.problem("n12x12_m1_k1")
    rng = np.random.RandomState(5)
    Xk = rng.uniform(0, 1, (12, wc.D))
    yk = wc.side_y(Xk, 0, rng)
    level = float(np.sort(yk)[5:7].mean())                           # between two observed values
    h = wc.fit_handle(L, "f64", p["X"], p["y"], "matern12", p["ls"])
    g = wc.fit_handle(L, "f64", Xk, yk, "matern12", p["ls"], noise=0.0, jitter=0.0)
    Xc = np.vstack([Xk, rng.uniform(0, 1, (20, wc.D)), np.full((1, wc.D), np.nan)])
    h.set_candidates(Xc)
    r = h.sweep_weighted([(g, "ge", level)], L.ACQ_EI, -1.0, float(p["y"].min()), wc.XI, want_logw=True, want_value=True,
                         want_sides=True, want_acq=True)
    sg, mu = r["side_sigma"][0], r["side_mu"][0]
    zero = sg == 0.0
    print("step function: sigma_k == 0 at %d of the 12 training points" % int(zero[:12].sum()))
    assert zero[:12].any(), "the clamp was not reached: this case judges nothing"
    below = zero & (mu < level)
    assert below.any() and (zero & (mu >= level)).any()
    assert np.all(r["logw"][below] == -np.inf) and np.all(r["value"][below] == 0.0)
    assert np.all(r["logw"][zero & (mu >= level)] == 0.0)
    assert np.array_equal(r["value"][zero & (mu >= level)], r["acq"][zero & (mu >= level)])
    # the clamp counts of the K + 1 sweeps arrive as their sum: this side's is known not to be zero
    own_h = h.sweep(L.ACQ_NONE, want_sigma=True)["n_clamped"]
    own_g = g.sweep(L.ACQ_NONE, want_sigma=True)["n_clamped"]
    print("step function: clamped variances: objective %d, side %d, reported %d" % (own_h, own_g, r["n_clamped"]))
    assert own_g > 0 and r["n_clamped"] == own_h + own_g
    assert math.isnan(r["value"][-1]) and r["best_idx"] != Xc.shape[0] - 1
    assert (r["best_idx"], r["best_val"]) == wr.argmax(r["value"])
    wc.close(h, [(g, 0, 0)])


def test_after_the_call(L):
    """the sides own a copy of the objective's rows and behave as after tgp_set_candidates with them; a buffer a side had
    borrowed is released, never written; the objective's later sweep is unchanged bit for bit"""
    import torch
    name = "n300x200_m33_k1_mix"
    p = wc.problem(name)
    h, sides = wc.handles(L, name)
    g = sides[0][0]
    before = h.sweep(p["acq"], p["sf"], p["incumbent"], p["param"], want_mu=True, want_sigma=True, want_acq=True)
    other = np.random.RandomState(3).uniform(0, 1, (50, wc.D))
    buf = torch.tensor(other, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    g.set_candidates_dev(buf.data_ptr(), 50, keepalive=buf)
    _call(h, sides, p)
    assert np.array_equal(buf.cpu().numpy(), other)                  # the borrowed buffer: unchanged
    assert g.M == p["Xc"].shape[0] and np.array_equal(g.read_candidates(), p["Xc"])
    assert np.array_equal(h.read_candidates(), p["Xc"])
    s1 = g.sweep(L.ACQ_EI, 1.0, 0.3, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    g.set_candidates(p["Xc"])
    s2 = g.sweep(L.ACQ_EI, 1.0, 0.3, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    for key in ("mu", "sigma", "acq"):
        assert s1[key].tobytes() == s2[key].tobytes(), key
    assert (s1["best_idx"], s1["best_val"], s1["n_clamped"]) == (s2["best_idx"], s2["best_val"], s2["n_clamped"])
    after = h.sweep(p["acq"], p["sf"], p["incumbent"], p["param"], want_mu=True, want_sigma=True, want_acq=True)
    for key in ("mu", "sigma", "acq"):
        assert after[key].tobytes() == before[key].tobytes(), key
    assert (after["best_idx"], after["best_val"]) == (before["best_idx"], before["best_val"])
    wc.close(h, sides)


def test_the_error_lines_that_need_a_device(L):
    p = wc.problem("n12x12_m1_k1")
    h, sides = wc.handles(L, "n12x12_m1_k1")
    g = sides[0][0]
    kw = dict(acq=L.ACQ_EI, sf=-1.0, incumbent=0.0, param=0.01)

    def refused(sd, status, text, **over):
        a = dict(kw)
        a.update(over)
        arr, K = h._sides(sd)
        rc = h.lib.tgp_sweep_weighted(h._h, arr, K, a["acq"], a["sf"], a["incumbent"], a["param"], *([None] * 10))
        assert rc == status, (rc, status, text)
        assert text in h.lib.tgp_last_error(h._h).decode(), h.lib.tgp_last_error(h._h).decode()
    other_d = L.NativeGP(0, "f64")
    other_d.fit(p["X"][:, :2], p["y"], "rbf", 1.0, [0.4], 1e-3, 1e-10, True)
    unfitted = L.NativeGP(0, "f64")
    refused([(g, "ge", 0.0), (other_d, "le", 0.0)], 2, "side 1: D differs")
    refused([(g, "ge", 0.0), (g, "le", 0.0)], 2, "side 1: the same handle as side 0")
    refused([(h, "ge", 0.0)], 2, "side 0: the objective's own handle")
    refused([(g, "ge", 0.0), (unfitted, "ge", 0.0)], 4, "side 1: no fitted model")
    refused([(g, 7, 0.0)], 2, "side 0: unknown kind")
    refused([(g, "ge", float("nan"))], 2, "side 0: the level must be finite")
    refused([(g, "cost", 1.0)], 2, "side 0: a cost side's level must be 0")
    refused([(g, "ge", 0.0)], 2, "sf must be", sf=0.5)
    for acq in (L.ACQ_UCB, L.ACQ_SIGMA, L.ACQ_MES):
        refused([(g, "ge", 0.0)], 2, "acquisition must be", acq=acq)
    arr, _ = h._sides([(g, "ge", 0.0)] * 1)
    assert h.lib.tgp_sweep_weighted(h._h, arr, 9, 3, -1.0, 0.0, 0.01, *([None] * 10)) == 2
    assert h.lib.tgp_sweep_weighted(h._h, None, 1, 3, -1.0, 0.0, 0.01, *([None] * 10)) == 2
    lo, hi = np.full(wc.D, -0.2), np.full(wc.D, 1.2)
    h.warp_candidates(lo, hi, np.full(wc.D, 1.5), np.full(wc.D, 0.8))
    refused([(g, "ge", 0.0)], 2, "warped")
    h.set_candidates(p["Xc"])
    fresh = wc.fit_handle(L, "f64", p["X"], p["y"], p["kind"], p["ls"])          # fitted, no candidates
    arr, K = fresh._sides([(g, "ge", 0.0)])
    assert fresh.lib.tgp_sweep_weighted(fresh._h, arr, K, 3, -1.0, 0.0, 0.01, *([None] * 10)) == 2
    assert "no candidates" in fresh.lib.tgp_last_error(fresh._h).decode()
    r = _call(h, sides, p)                                           # and the handles still work
    assert np.all(np.isfinite(r["value"]))
    for x in (other_d, unfitted, fresh):
        x.close()
    wc.close(h, sides)


def test_record_the_figures():
    """(last in the file) where WEIGHTED_PARITY_JSON names a file, the figures seen above go there"""
    out = os.environ.get("WEIGHTED_PARITY_JSON")
    if out and RECORD:
        with open(out, "w") as f:
            json.dump(dict(unit="logw: absolute error against the mpmath formula at the returned bits, and its fraction of the bar "
                                "64 max(e_ref, u) sum_k (1 + |log f_k|); value: fraction of value (bar + 4 u)",
                           e_ref=E_REF, cases=RECORD), f, indent=1, sort_keys=True)
    for name, rec in RECORD.items():
        for key in ("logw_err_over_bar", "value_err_over_bar"):
            assert rec.get(key, 0.0) <= 1.0, (name, key, rec)
