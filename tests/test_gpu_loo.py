"""GPU: leave-one-out cross-validation -- tgp_loo (loo_kappa_partial_kernel, loo_points_kernel of csrc/loo_kernels.hip) and
tgp_fit_loo_grad (launch_loo_grad: K^-1, kappa, b, A, B = A A^T, then lml_weights_kernel with the LOO pair weight) -- held to
an 80-bit closed form (tests/loo_reference_hp.py).  Cases, bars and the comparison: tests/loo_edge_cases.py (bars of
64 max(e_ref, N u) of each entry's SCALE under a cap of 1e-9; tests/test_loo_reference.py shows on the CPU that they reject
a dropped row chunk, a diagonal tile counted twice, the jitter left out of sigma, padding rows in B, w without its 1/2 and
an unsymmetrised G).

 (a) every case: tgp_loo behind a fit (resid, sigma, lpd, L_LOO) and tgp_fit_loo_grad (L_LOO, every gradient entry) against
     the reference; the same bytes on a second call; everything finite; the noise entry exactly +0.0 without noise;
 (b) *loo of tgp_fit_loo_grad is tgp_loo's on that handle, and its lml is tgp_fit_grad's under TGP_SMALL=0 (a child process);
     TGP_KINV64=0 (another child): the 128-tile products at Np = 256, 512 and 1280;
 (c) ARD with every length scale equal sums to the isotropic entry;
 (d) one handle through six shapes: every result a fresh handle's, byte for byte;
 (e) behind tgp_fit_append (299 -> 300) tgp_loo meets the 300-point model's bars;
 (f) a handle that received a factor returns the giver's bytes;
 (g) tgp_loo leaves the fit, the sweep, the MES maxima and a Thompson draw alone;
 (h) the plugin classes on Branin, N = 30, and the starts side by side on worker handles at N = 80.

Every case prints its figures before it asserts; the last test writes them where LOO_JSON names a file
(profiles/loo_parity.json)."""
import faulthandler
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

import cov_edge_cases as ec
import loo_edge_cases as le
import loo_reference_hp as lo
from cov_reference_hp import Fit

pytestmark = pytest.mark.gpu

RECORD = {}
_base = {}


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _handle(case, dtype=None):
    import turbo_amd as ta
    return ta.NativeGP(0, dtype or le.config(case)["dtype"])


def _base_calls(case):
    """(tgp_loo's dict behind a fit on one fresh handle, tgp_fit_loo_grad's dict on another, that other handle): made
    once, shared, never modified"""
    if case not in _base:
        plain = le.fit_and_loo(_handle(case), case)
        gp = _handle(case)
        grad = le.fit_loo_grad(gp, case)
        for r in (plain, grad):
            for v in r.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
        _base[case] = (plain, grad, gp)
    return _base[case]


def _judge(case, what, res, keys):
    j = le.judge(case, res, keys)
    le.show(case, what, j)
    RECORD.setdefault(case, {})[what] = {k: {f: float(v) for f, v in j[k].items() if f != "ok"} for k in keys}
    return j


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", le.CASES)
def test_every_case_against_the_80_bit_reference(case):
    """(model F is an f32 handle: tgp_loo reads the f64 inverse factor whatever the dtype, so it is held to the f64 bar)"""
    plain, grad, gp = _base_calls(case)
    jp = _judge(case, "tgp_loo", plain, le.LOO_KEYS)
    jg = _judge(case, "tgp_fit_loo_grad", grad, ("loo",) + le.GRAD_KEYS)
    again = le.fit_loo_grad(gp, case)
    N = le.config(case)["N"]
    assert grad["grad"].shape == (2 + (le.config(case)["D"] if le.config(case)["ard"] else 1),)
    assert all(plain[k].shape == (N,) and np.all(np.isfinite(plain[k])) for k in le.POINT_KEYS) and np.isfinite(plain["loo"])
    assert np.isfinite(grad["lml"]) and np.isfinite(grad["loo"]) and np.all(np.isfinite(grad["grad"]))
    assert jp["ok"], jp
    assert jg["ok"], jg
    assert le.grad_bytes(again) == le.grad_bytes(grad)                    # the same bits from run to run
    fresh = _handle(case)
    assert le.loo_bytes(le.fit_and_loo(fresh, case)) == le.loo_bytes(plain) and le.loo_bytes(fresh.loo()) == le.loo_bytes(plain)
    if le.call_args(case)[5] == 0.0:
        assert grad["grad"][-1] == 0.0 and not np.signbit(grad["grad"][-1])


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", le.CASES)
def test_the_score_is_tgp_loo_s_on_that_handle(case):
    _, grad, gp = _base_calls(case)
    after = gp.loo()
    print("%s L_LOO: tgp_fit_loo_grad %r, tgp_loo on the handle %r" % (case, grad["loo"], after["loo"]))
    assert np.float64(grad["loo"]).tobytes() == np.float64(after["loo"]).tobytes()
    j = _judge(case, "tgp_loo behind tgp_fit_loo_grad", after, le.LOO_KEYS)      # (the blocked fit's factor for every N)
    assert j["ok"], j


def _child(env, mode, cases):
    """{case: list of floats} of tests/_loo_child.py under env"""
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_loo_child.py"), mode] + list(cases),
                         env=e, capture_output=True, text=True, timeout=110)
    lines = [l for l in out.stdout.splitlines() if l.startswith("loo-child ")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(lines[0][len("loo-child "):])
    assert sorted(res) == sorted(cases)
    return {c: [float.fromhex(x) for x in v] for c, v in res.items()}


def test_the_lml_is_the_blocked_fit_s():
    """tgp_fit_loo_grad takes the blocked route for every N: its lml has the bytes of tgp_fit_grad under TGP_SMALL=0"""
    res = _child({"TGP_SMALL": "0"}, "lml", le.CASES)
    for case in le.CASES:
        assert res[case][0].hex() == float(_base_calls(case)[1]["lml"]).hex(), case


def test_the_128_tile_products():
    """TGP_KINV64=0: K^-1 = U U^T and B = A A^T on 128 x 128 tiles (g.on128<KN_UPPER_A / KN_FULL, TM_LOWER>), what the
    default takes above Np = 4096 -- here at Np = 256, 512 and 1280, held to the same bars"""
    cases = ["T193/ard", "C/iso", "D/ard", "E/iso", "G/iso"]
    assert {le.padded(c) for c in cases} == {256, 512, 1280}
    res = _child({"TGP_KINV64": "0"}, "loo", cases)
    for c in cases:
        r = dict(lml=res[c][0], loo=res[c][1], grad=np.array(res[c][2:]))
        j = _judge(c, "TGP_KINV64=0", r, ("loo",) + le.GRAD_KEYS)
        assert np.all(np.isfinite(r["grad"])) and j["ok"], (c, j)
        assert np.float64(r["loo"]).tobytes() == np.float64(_base_calls(c)[1]["loo"]).tobytes()      # (kappa never sees the product)


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in le.CASES if not le.config(c)["ard"] and le.config(c)["D"] > 1])
def test_equal_ard_length_scales_sum_to_the_isotropic_entry(case):
    """d2 = sum_d (xs_d - xs'_d)^2: the D ARD entries of a model whose length scales are all equal add up to its isotropic
    entry, as a fraction of that entry's scale; everything else in the two calls is the same arithmetic on the same numbers"""
    grad = _base_calls(case)[1]
    a = le.fit_loo_grad(_handle(case), case, le.equal_ard_args(case))
    ref = le.hp_reference(case)
    total = np.sum(a["grad"][1:-1].astype(le.LD))
    err = float(abs(total - le.LD(grad["grad"][1])) / ref["grad_scale"][1])
    err_ref = float(abs(total - ref["grad"][1]) / ref["grad_scale"][1])
    bar = le.bars(case)["length_scale"]
    print("%s equal ARD length scales: sum of the entries %.3g from the isotropic entry, %.3g from the 80-bit one (bar %.3g)" % (case, err, err_ref, bar))
    RECORD.setdefault(case, {})["equal ARD sum"] = dict(err=err, err_to_reference=err_ref, bar=bar, ratio=err / bar)
    assert a["grad"].shape == (2 + le.config(case)["D"],) and np.all(np.isfinite(a["grad"]))
    assert err <= bar and err_ref <= bar
    same = lambda r: np.float64(r["lml"]).tobytes() + np.float64(r["loo"]).tobytes() + r["grad"][[0, -1]].tobytes()
    assert same(a) == same(grad)


# ---- (d) ----------------------------------------------------------------------------------------------------------------
def test_one_handle_many_shapes():
    """1100 x 6 isotropic, 129 x 3 ARD, 384 x 33 ARD, 300 x 17 isotropic, 128 x 61 ARD, 257 x 3 ARD on ONE f64 handle: the
    LOO workspace grows along Np and then (the pairwise partials) along Dp, and Linv, W, A and the vectors hold what the
    larger fit left.  Every result -- tgp_fit_loo_grad's and tgp_loo's behind it -- is a fresh f64 handle's, byte for byte."""
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    for case in ("G/iso", "B/ard", "F/ard", "E/iso", "S5/ard", "D/ard"):
        got = le.fit_loo_grad(gp, case)
        after = gp.loo()
        if le.config(case)["dtype"] == "f64":
            fresh, fgp = _base_calls(case)[1:]
        else:
            fgp = _handle(case, "f64")
            fresh = le.fit_loo_grad(fgp, case)
        print("%s on the travelled handle: lml %r loo %r grad[:3] %r" % (case, got["lml"], got["loo"], got["grad"][:3]))
        assert le.grad_bytes(got) == le.grad_bytes(fresh), (case, got, fresh)
        assert le.loo_bytes(after) == le.loo_bytes(fgp.loo()), case


# ---- (e) ----------------------------------------------------------------------------------------------------------------
def test_tgp_loo_after_an_append():
    """tests/cov_edge_cases.py's model H: 299 rows, the one-row extension to 300, then tgp_loo -- held to the bars of the
    300-point model itself (the reference and the f64 restatement on all 300 rows, made here by the recipe of the cases)"""
    import turbo_amd as ta
    X, y, ls, _ = ec.data("H")
    kind = ec.MODELS["H"]["kind"]
    gp = ec.fit_handle(ta.NativeGP(0, "f64"), "H")
    assert gp.appended
    got = gp.loo()
    args = (X, y, kind, ec.C, ls, ec.NOISE, ec.JITTER, True)
    ref = lo.loo_and_grad(Fit(*args), y)
    f64 = lo.loo_and_grad_f64(*args)
    rec = {}
    for k in le.LOO_KEYS:
        frac = lambda r: float(le.lc._fraction(np.atleast_1d(r[k]), np.atleast_1d(ref[k]), np.atleast_1d(ref[k + "_scale"])).max())
        e, err = frac(f64), frac(got)
        bar = ec._bar(e, len(y), le.CAP)
        rec[k] = dict(e_ref=e, bar=bar, err=err, ratio=err / bar)
        print("H after the append, %s: %.3g (bar %.3g, e_ref %.3g)" % (k, err, bar, e))
    RECORD["H (appended)"] = {"tgp_loo": rec}
    assert all(v["err"] <= v["bar"] for v in rec.values()), rec
    assert le.loo_bytes(gp.loo()) == le.loo_bytes(got)


# ---- (f) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A/iso", "D/iso"])
def test_a_received_factor_returns_the_giver_s_bytes(case):
    """such a handle holds Linv and alpha but no y: what tgp_loo returns is the residual, and it is the giver's"""
    giver, taker = _handle(case), _handle(case)
    want = le.fit_and_loo(giver, case)
    assert taker.import_factor(giver.export_factor())
    got = taker.loo()
    assert le.loo_bytes(got) == le.loo_bytes(want)
    assert le.loo_bytes(want) == le.loo_bytes(_base_calls(case)[0])


# ---- (g) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["A/iso", "E/ard"])
def test_tgp_loo_leaves_the_model_alone(case):
    import turbo_amd as ta
    L = ta._lib
    gp = _handle(case)
    gp.fit(*le.call_args(case))
    Xc = np.random.RandomState(7).uniform(0, 1, (700, le.config(case)["D"]))
    gp.set_candidates(Xc)
    inc = float(le.call_args(case)[1].min())

    def state():
        s = gp.sweep(L.ACQ_EI, -1.0, inc, 0.01, want_mu=True, want_sigma=True, want_acq=True)
        m = gp.sweep(L.ACQ_MES, -1.0, inc, 0.0, want_acq=True)
        t = gp.ts_sweep(sf=-1.0, want_f=True)
        d = gp.ts_read()
        return b"".join(np.ascontiguousarray(a).tobytes() for a in (
            s["mu"], s["sigma"], s["acq"], np.float64(s["best_val"]), np.int64(s["best_idx"]), m["acq"], np.int64(m["best_idx"]),
            t["idx"], t["val"], t["f"], d["W"], d["eps"], gp.debug_read(L.BUF_L), gp.debug_read(L.BUF_ALPHA)))

    gp.mes_draw(11, S=4, F=256, sf=-1.0, incumbent=inc)          # (leaves its Thompson draw and the maxima in the handle)
    before = state()
    first = gp.loo()
    assert state() == before
    assert le.loo_bytes(gp.loo()) == le.loo_bytes(first)


# ---- (h) ----------------------------------------------------------------------------------------------------------------
def _branin(n=30):
    rng = np.random.RandomState(3)
    X = np.stack([rng.uniform(-5, 10, n), rng.uniform(0, 15, n)], axis=1)
    x1, x2 = X[:, 0], X[:, 1]
    y = (x2 - 5.1 / (4 * np.pi ** 2) * x1 ** 2 + 5 / np.pi * x1 - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10
    return X, y


def test_the_plugin_classes_on_branin():
    """HipGPSurrogate(criterion='loo') ends at hyper-parameters whose L_LOO is at least that of the 'lml' optimum (both
    start from the same kernel and draw the same restarts); fitting_info carries the criterion
    and the score; the pickled and reloaded model's loo() through the host backend is the GPU's to 1e-9; the marginalised
    surrogate refuses the criterion."""
    import turbo_amd as ta
    X, y = _branin()
    models = {}
    for crit in ("lml", "loo"):
        sur = ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel("matern52", 1.0, 1.0, 1e-2), normalize_y=True, random_state=0),
                                training_iterations=3, criterion=crit)
        models[crit] = sur.construct_model(0, X, y)
    (m_lml, i_lml), (m_loo, i_loo) = models["lml"], models["loo"]
    s_lml, s_loo = m_lml.get_loo_log_likelihood(), m_loo.get_loo_log_likelihood()
    print("Branin N = 30: L_LOO %.6f at the LML optimum, %.6f at the LOO optimum (LML %.6f / %.6f)"
          % (s_lml, s_loo, m_lml.get_log_likelihood(), m_loo.get_log_likelihood()))
    RECORD["Branin N = 30"] = dict(loo_at_lml_optimum=s_lml, loo_at_loo_optimum=s_loo)
    assert i_loo["criterion"] == "loo" and i_loo["loo"] == s_loo and "criterion" not in i_lml
    assert s_loo >= s_lml
    mu, sigma = m_loo.loo()
    assert mu.shape == sigma.shape == (30,) and np.all(sigma > 0)
    host = pickle.loads(pickle.dumps(m_loo))
    host._factory._native = ta.NativeGP(ta._lib.DEVICE_HOST, "f64")       # what a process without a GPU ends up with
    hmu, hsigma = host.loo()
    scale = np.abs(y).max()
    assert np.abs(hmu - mu).max() <= 1e-9 * scale and np.abs(hsigma - sigma).max() <= 1e-9 * scale
    assert abs(host.get_loo_log_likelihood() - s_loo) <= 1e-9 * abs(s_loo)
    with pytest.raises(ValueError):
        ta.MarginalisedHipGPSurrogate(criterion="loo")
    with pytest.raises(ValueError):
        ta.HipGPSurrogate(criterion="k-fold")


def test_the_threaded_starts_maximise_the_loo_score():
    """N = 80 > 64: three starts side by side on the device's worker handles, each walking tgp_fit_loo_grad -- none may
    silently optimise the LML.  The same starts one after the other on the factory's own handle end at the same
    hyper-parameters, bit for bit, and that optimum's L_LOO is at least the LML optimum's."""
    import turbo_amd as ta
    X, y = _branin(80)
    res = {}
    for name, crit, above in (("threads", "loo", "auto"), ("serial", "loo", None), ("lml", "lml", "auto")):
        sur = ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel("matern52", 1.0, 1.0, 1e-2), normalize_y=True, random_state=0),
                                training_iterations=3, criterion=crit, parallel_restarts_above=above)
        model, info = sur.construct_model(0, X, y)
        res[name] = (model, info, sur.last_worker_count)
    print("Branin N = 80: theta %r, L_LOO %.6f (threads) / %.6f (serial) / %.6f (at the LML optimum)"
          % (res["threads"][0].kernel.theta, res["threads"][1]["loo"], res["serial"][1]["loo"], res["lml"][0].get_loo_log_likelihood()))
    assert res["threads"][2] == 3 and res["serial"][2] == 0
    assert res["threads"][0].kernel.theta.tobytes() == res["serial"][0].kernel.theta.tobytes()
    assert res["threads"][1]["loo"] == res["serial"][1]["loo"] and res["threads"][1]["criterion"] == "loo"
    assert res["threads"][1]["loo"] >= res["lml"][0].get_loo_log_likelihood()


def test_status_codes_on_the_gpu():
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    assert gp.lib.tgp_loo(gp._h, None, None, None, None) == ta._lib.NOT_FITTED
    gp.fit(*le.call_args("S3/iso"))
    assert gp.lib.tgp_loo(gp._h, None, None, None, None) == ta._lib.OK


def test_record_the_figures():
    """(last in the file) where LOO_JSON names a file the figures seen above go there: profiles/loo_parity.json"""
    out = os.environ.get("LOO_JSON")
    if out and RECORD:
        with open(out, "w") as f:
            json.dump(dict(unit="fraction of the quantity's scale: the sum of the absolute terms (tests/loo_reference_hp.py); resid, sigma, lpd, length_scale: the worst entry",
                           factor=le.FACTOR, cap=le.CAP, cases=RECORD), f, indent=1, sort_keys=True)
    for case, rec in RECORD.items():
        for what, keys in rec.items():
            if not isinstance(keys, dict):
                continue
            for k, v in (keys.items() if "ratio" not in keys else [(what, keys)]):
                assert v["ratio"] <= 1.0 and v["bar"] <= le.CAP, (case, what, k, v)
