"""GPU: the gradient of the knowledge gradient (tgp_kg_grad, tgp_kg_lbfgsb, ``ta.KG(gradient=True)``) against the 80-bit
closed form of tests/kg_grad_reference_hp.py, on the cases and under the bar of tests/kg_grad_cases.py.  Every figure is
printed before it is asserted; where KG_GRAD_PARITY_JSON names a file the last test writes them there
(profiles/kg_grad_parity.json)."""
import json
import os

import numpy as np
import pytest

import kg_cases as kc
import kg_grad_cases as gc
import kg_grad_reference as gr
import kg_grad_reference_hp as grh

pytestmark = pytest.mark.gpu

RECORD = {}
_runs = {}


def _L():
    import turbo_amd._lib as L
    return L


def _batch(name):
    """the rows the case's call is made on: the leading 48 (or all there are); n600m: the leading 4096"""
    c = gc.CASES[name]
    return gc.data(name)[4][:c["tail"][0] if "tail" in c else gc.BASE]


def _run(name):
    """the case's one call: (handle, val, grad) over _batch(name); made once, the handle left open"""
    if name not in _runs:
        L = _L()
        gp = L.NativeGP(0, gc.CASES[name].get("dtype", "f64"))
        gp.fit(*gc.fit_args(name))
        gp.kg_set_points(gc.data(name)[3])
        val, grad = gp.kg_grad(_batch(name), gc.CASES[name]["sf"])
        t = np.zeros(21)
        gp.lib.tgp_last_timings(gp._h, t.ctypes.data_as(L._dp), 21)
        RECORD[name] = dict(kg_grad_ms=float(t[20]))
        _runs[name] = (gp, val, grad)
    return _runs[name]


@pytest.mark.parametrize("name", list(gc.CASES))
def test_gradient_against_the_80_bit_closed_form(name):
    gp, val, grad = _run(name)
    sf = gc.CASES[name]["sf"]
    assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad)) and np.all(val >= 0.0)
    j = gc.judge(name, grad[gc.rows(name)])
    want = gc.hp_reference(name)
    ev = float(np.abs(val[gc.rows(name)] - want["kg"]).max()) / gc.scale(name)
    print("%s: gradient error %.3g of the batch maximum (bar %.3g, e_ref %.3g); value error %.3g of the scale"
          % (name, j["err"], j["bar"], gc.e_ref(name), ev))
    RECORD[name].update(err=j["err"], bar=j["bar"], e_ref=gc.e_ref(name), val_err=ev)
    assert j["ok"], j
    assert ev <= kc.CAP_VAL
    # the value is tgp_sweep_kg's for the same points: bit for bit where the sweep is f64
    gp.set_candidates(_batch(name))
    swept = gp.sweep_kg(sf, want_kg=True)["kg"]
    if gc.CASES[name].get("dtype", "f64") == "f64":
        assert val.tobytes() == swept.tobytes()
    else:      # (the sweep's sigma is f32 there, this call's is f64: tests/test_gpu_kg.py holds kg_out to its own f32 bar)
        print("    f32 handle: tgp_sweep_kg's value differs by %.3g of the scale" % (float(np.abs(val - swept).max()) / gc.scale(name)))


def test_coincident_rows_of_n40():
    """Rows 5 (ON training point 0) and 7 (ON discretisation point 3) with noise 0: the f64 reference itself is good to
    about 2e-6 there, so they are held to 64 e_ref of THESE rows without the cap -- and to the closed form at the call's own
    value: the sweep's bits."""
    name = "n40"
    gp, val, grad = _run(name)
    Xa, Xc = gc.data(name)[3], gc.data(name)[4]
    rows = np.array(gc.CASES[name]["skip"])
    want = grh.kg_grad(gc.hp_fit(name), Xa, Xc[rows], gc.CASES[name]["sf"])["grad"]
    ref = gr.kg_grad(gc.model(name), Xa, Xc[rows], gc.CASES[name]["sf"])["grad"]
    top = np.abs(gc.hp_reference(name)["grad"]).max()
    e_ref = float(np.abs(ref.astype(gc.LD) - want).max() / top)
    err = float(np.abs(grad[rows].astype(gc.LD) - want).max() / top)
    bar = gc.FACTOR * max(e_ref, gc.CASES[name]["N"] * gc.U)
    print("n40 rows 5, 7: error %.3g of the batch maximum (e_ref %.3g, bar %.3g)" % (err, e_ref, bar))
    RECORD["n40 rows 5, 7"] = dict(err=err, e_ref=e_ref, bar=bar)
    assert np.all(np.isfinite(grad[rows])) and np.all(np.isfinite(val[rows]))
    assert err <= bar


def test_f32_handle_against_the_f64_handle():
    g32, v32, d32 = _run("f32")
    g64, v64, d64 = _run("n600m")
    same = d32.tobytes() == d64[:len(d32)].tobytes() and v32.tobytes() == v64[:len(v32)].tobytes()
    j = gc.judge("f32", d32[gc.rows("f32")])
    print("f32 handle: the f64 handle's bits: %s; error %.3g (bar %.3g)" % (same, j["err"], j["bar"]))
    RECORD["f32"]["same_bits_as_f64"] = bool(same)
    assert same or j["ok"]


def test_bits_do_not_depend_on_m_or_row_and_repeat():
    name = "n600m"
    gp, val, grad = _run(name)
    sf = gc.CASES[name]["sf"]
    X = _batch(name)
    v2, g2 = gp.kg_grad(X, sf)
    assert v2.tobytes() == val.tobytes() and g2.tobytes() == grad.tobytes()          # run to run
    for m in (255, 256, 257):
        v, g = gp.kg_grad(X[:m], sf)
        assert v.tobytes() == val[:m].tobytes() and g.tobytes() == grad[:m].tobytes(), m
    v, g = gp.kg_grad(X[:gc.BASE], sf)                                               # the base rows in a small call
    assert v.tobytes() == val[:gc.BASE].tobytes() and g.tobytes() == grad[:gc.BASE].tobytes()
    v, g = gp.kg_grad(X[-16:], sf)                                                   # the last 16 rows as rows 0 .. 15
    assert v.tobytes() == val[-16:].tobytes() and g.tobytes() == grad[-16:].tobytes()
    for i in (0, 255, 256, 4095):
        v, g = gp.kg_grad(X[i:i + 1], sf)
        assert v[0] == val[i] and g[0].tobytes() == grad[i].tobytes(), i
    perm = np.random.RandomState(2).permutation(300)
    v, g = gp.kg_grad(X[perm], sf)
    assert v.tobytes() == val[perm].tobytes() and g.tobytes() == np.ascontiguousarray(grad[perm]).tobytes()


def test_the_call_leaves_the_handle_as_it_was():
    import torch
    L = _L()
    name = "n300"
    gp, val, _ = _run(name)
    X, y, _, Xa, Xc = gc.data(name)
    sf = gc.CASES[name]["sf"]
    gp.set_candidates(Xc)
    rec = torch.zeros(Xc.shape[1] + 2, dtype=torch.float64, device="cuda:0")
    gp.set_winner_out(rec.data_ptr(), 500, keepalive=rec)

    def state():
        ei = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)
        gp.winner_wait(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        w_ei = rec.cpu().numpy().copy()
        kg = gp.sweep_kg(sf, want_kg=True, want_mu=True, want_sigma=True)
        ts = gp.ts_sweep(1.0, want_f=True)
        mes = gp.sweep(L.ACQ_MES, 1.0, want_acq=True)
        return ei, w_ei, kg, ts, mes, gp.read_candidates(), gp.sweep_geometry()

    gp.ts_draw(3, 2, 256)
    gp.mes_set_maxima(np.array([y.max(), y.max() + 0.1]))
    before = state()
    torch.cuda.synchronize()
    w0 = rec.cpu().numpy().copy()
    v, g = gp.kg_grad(Xc[:gc.BASE], sf)
    torch.cuda.synchronize()
    assert rec.cpu().numpy().tobytes() == w0.tobytes()              # the winner record: not touched by the call itself
    assert v.tobytes() == val.tobytes()
    after = state()
    for a, b in ((before[0], after[0]), (before[2], after[2])):
        for key in ("mu", "sigma", "acq"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert (a["best_idx"], a["best_val"], a["n_clamped"]) == (b["best_idx"], b["best_val"], b["n_clamped"])
    assert before[1].tobytes() == after[1].tobytes()
    assert before[3]["f"].tobytes() == after[3]["f"].tobytes() and (before[3]["idx"] == after[3]["idx"]).all()
    assert before[4]["acq"].tobytes() == after[4]["acq"].tobytes()
    assert before[5].tobytes() == after[5].tobytes() and before[6] == after[6]
    gp.set_winner_out(None)


@pytest.mark.parametrize("name", ["n1", "n40", "n129", "n256", "f32"])
def test_the_other_sweep_paths_are_left_as_they_were(name):
    """the one-workgroup sweep (n1, n40), the one-launch sweep (n129, n256) and an f32 handle (no sweep inside the call): an
    EI sweep and a KG sweep of the resident batch -- outputs, winner, clamp count --, the batch itself, the sweep geometry
    and what the last sweep reported are the same before and after a tgp_kg_grad"""
    L = _L()
    gp, val, _ = _run(name)
    X, y, _, Xa, Xc = gc.data(name)
    sf = gc.CASES[name]["sf"]
    gp.set_candidates(Xc)

    def state():
        ei = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)
        report = (gp.last_timings()["sweep_f64"], gp.last_prune(), gp.sweep_geometry())
        kg = gp.sweep_kg(sf, want_kg=True, want_mu=True, want_sigma=True)
        return ei, kg, report, gp.read_candidates()

    before = state()
    gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01)
    told = (gp.last_timings()["sweep_f64"], gp.last_prune(), gp.sweep_geometry())
    v, _ = gp.kg_grad(_batch(name), sf)
    assert (gp.last_timings()["sweep_f64"], gp.last_prune(), gp.sweep_geometry()) == told     # right behind the call
    assert v.tobytes() == val.tobytes()
    after = state()
    for a, b in ((before[0], after[0]), (before[1], after[1])):
        for key in ("mu", "sigma", "acq"):
            assert a[key].tobytes() == b[key].tobytes(), key
        assert (a["best_idx"], a["best_val"], a["n_clamped"]) == (b["best_idx"], b["best_val"], b["n_clamped"])
    assert before[2] == after[2] and before[3].tobytes() == after[3].tobytes()


def test_points_belong_to_one_fit_and_argument_rules():
    L = _L()
    name = "n300"
    X, y, ls, Xa, Xc = gc.data(name)
    c = gc.CASES[name]
    sf, D = c["sf"], X.shape[1]
    dp = lambda a: a.ctypes.data_as(L._dp)
    Xq, val, grad = np.ascontiguousarray(Xc[:4]), np.zeros(4), np.zeros((4, D))
    big = np.zeros((4097, D))
    gp = L.NativeGP(0, "f64")
    assert gp.lib.tgp_kg_grad(gp._h, dp(Xq), 4, sf, dp(val), dp(grad)) == 4                 # TGP_NOT_FITTED
    gp.fit(X[:-1], y[:-1], c["kind"], kc.C, ls, c["noise"], c["jitter"], True)
    with pytest.raises(ValueError, match="tgp_kg_set_points"):
        gp.kg_grad(Xq, sf)                                                                  # no points yet
    gp.kg_set_points(Xa)
    bad = Xq.copy()
    bad[1, 2] = np.nan
    for args in ((dp(Xq), 4, 0.5, dp(val), dp(grad)), (dp(Xq), 0, sf, dp(val), dp(grad)), (dp(big), 4097, sf, dp(val), dp(grad)),
                 (dp(bad), 4, sf, dp(val), dp(grad)), (None, 4, sf, dp(val), dp(grad)), (dp(Xq), 4, sf, None, dp(grad)),
                 (dp(Xq), 4, sf, dp(val), None)):
        assert gp.lib.tgp_kg_grad(gp._h, *args) == 2
    with pytest.raises(ValueError, match="sf"):
        gp.kg_grad(Xq, 0.5)
    first, _ = gp.kg_grad(Xq, sf)
    gp.fit(X, y, c["kind"], kc.C, ls, c["noise"], c["jitter"], True)                        # a refit drops the points
    with pytest.raises(ValueError, match="tgp_kg_set_points"):
        gp.kg_grad(Xq, sf)
    with pytest.raises(ValueError, match="tgp_kg_set_points"):
        gp.kg_lbfgsb(Xq, np.zeros(D), np.ones(D), sf)
    gp.kg_set_points(Xa)
    mine, gmine = gp.kg_grad(Xq, sf)
    full = _run(name)
    assert mine.tobytes() == full[1][:4].tobytes() and gmine.tobytes() == full[2][:4].tobytes()
    assert not np.array_equal(first, mine)
    gp.close()


@pytest.mark.parametrize("name", ["n40", "n300"])
def test_lbfgsb_in_the_library(name):
    """tgp_kg_lbfgsb, three restarts in the unit box with SciPy's default limits: no end below its start, val_out is
    tgp_kg_grad at x_out, and the ends are those of SciPy's L-BFGS-B driving tgp_kg_grad from the same starts -- to the
    tolerance tests/test_gpu_parity.py holds tgp_acq_lbfgsb to against SciPy (points 1e-9, values 1e-12 of max(1, |value|)),
    with the same success flags.  The starts are kg_grad_cases.LBFGSB_STARTS: the best rows of the case under the f64
    reference from which the walk is well conditioned, a property of the walk measured with SciPy alone on the CPU (that
    module's docstring; from row 42 of n300 SciPy's own end moves 2.6e-8 when the start moves by one ulp)."""
    import scipy.optimize
    gp = _run(name)[0]
    sf = gc.CASES[name]["sf"]
    D = gc.data(name)[0].shape[1]
    starts = np.ascontiguousarray(gc.points(name)[1][list(gc.LBFGSB_STARTS[name])])
    lo, hi = np.zeros(D), np.ones(D)
    v0, _ = gp.kg_grad(np.clip(starts, lo, hi), sf)               # (a start outside the box is clipped into it first)
    x, v, st, ev = gp.kg_lbfgsb(starts, lo, hi, sf)
    vx, _ = gp.kg_grad(x, sf)
    print("%s: KG %s -> %s, status %s, %d evaluations" % (name, v0, v, st, ev))
    assert np.all(v >= v0) and np.all(x >= lo) and np.all(x <= hi) and ev >= 3
    assert vx.tobytes() == v.tobytes()
    worst = [0.0, 0.0]
    for j in range(3):
        def neg_f(p):
            val, g = gp.kg_grad(p.reshape(1, -1), sf)
            return -float(val[0]), -g[0]
        ref = scipy.optimize.minimize(neg_f, starts[j], jac=True, bounds=list(zip(lo, hi)), method="L-BFGS-B", options=dict(maxiter=15000))
        dx, dv = float(np.abs(x[j] - ref.x).max()), abs(v[j] + ref.fun) / max(1.0, abs(ref.fun))
        worst = [max(worst[0], dx), max(worst[1], dv)]
        print("    restart %d: |x - scipy| %.3g, value %.17g (scipy %.17g, %d evaluations)" % (j, dx, v[j], -ref.fun, ref.nfev))
        assert (st[j] == 1) == bool(ref.success), (j, st[j], ref.message)
        assert dx <= gc.LBFGSB_TOL[0] and dv <= gc.LBFGSB_TOL[1], (j, dx, dv)
    RECORD["lbfgsb " + name] = dict(points=worst[0], values=worst[1], evaluations=int(ev))
    # argument checks as tgp_acq_lbfgsb's
    with pytest.raises(ValueError):
        gp.kg_lbfgsb(starts, hi, lo, sf)                          # lo > hi
    with pytest.raises(ValueError, match="sf"):
        gp.kg_lbfgsb(starts, lo, hi, 0.5)
    with pytest.raises(ValueError, match="max_iter"):
        gp.kg_lbfgsb(starts, lo, hi, sf, max_iter=0)
    dp = lambda a: a.ctypes.data_as(_L()._dp)
    assert gp.lib.tgp_kg_lbfgsb(gp._h, dp(starts), 0, dp(lo), dp(hi), sf, 10, dp(x), dp(v), None, None) == 2
    assert gp.lib.tgp_kg_lbfgsb(gp._h, dp(starts), 3, dp(lo), dp(hi), sf, 10, None, dp(v), None, None) == 2
    x2, v2, _, _ = gp.kg_lbfgsb(np.array([[5.0] * D, [-3.0] * D]), lo, hi, sf)       # starts outside the box are clipped
    assert np.all(x2 >= lo) and np.all(x2 <= hi)


def test_plugin_refines_a_kg_trial_through_the_library():
    import turbo_amd as ta
    from turbo_amd.bounds import Bounds
    L = _L()
    rng = np.random.RandomState(0)
    lb = Bounds([("x", -5.0, 10.0), ("y", 0.0, 15.0)])
    X = np.column_stack([rng.uniform(-5, 10, 30), rng.uniform(0, 15, 30)])
    x1, x2 = X[:, 0], X[:, 1]
    y = (x2 - 5.1 / (4 * np.pi ** 2) * x1 ** 2 + 5 / np.pi * x1 - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10
    kern = ta.GPKernel("matern52", 1.0, 3.0, 1e-4)
    sur = ta.HipGPSurrogate(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=0)
    model, _ = sur.construct_model(0, X, y)
    acq, info = ta.KG(n_points=16, gradient=True).construct_function(0, model, "min")
    assert info == {"n_points": 16, "default_points": True, "gradient": True}
    ctx = model._ensure_resident()
    calls = []

    class Recording:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name.startswith("tgp_"):
                calls.append(name)
            return getattr(self._lib, name)

    real = ctx.lib
    ctx.lib = Recording(real)
    try:
        np.random.seed(5)
        x, info = ta.CandidateSweep(num_random=1000, grad_restarts=4, start_from_best=2)(lb, acq)
    finally:
        ctx.lib = real
    np.random.seed(5)
    batch = ta.random_selector()(1000, lb)
    swept = float(acq(batch).max())
    at_x = float(acq.value_and_grad(np.asarray(x).reshape(1, -1))[0][0])
    print("plugin: the sweep's best %.6g, the refined point %.6g (max_acq %.6g); entries %s" % (swept, at_x, info["max_acq"], sorted(set(calls))))
    assert "tgp_kg_lbfgsb" in calls and "tgp_sweep_kg" in calls
    assert at_x >= swept and info["max_acq"] >= swept
    # lockstep='scipy' goes through value_and_grad; on_device=True reports the refusal
    np.random.seed(5)
    xs, infos = ta.CandidateSweep(num_random=1000, grad_restarts=4, start_from_best=2, lockstep="scipy")(lb, acq)
    assert abs(infos["max_acq"] - info["max_acq"]) <= 1e-7 * max(1.0, abs(info["max_acq"]))
    with pytest.raises(NotImplementedError, match="gradient=True serves"):
        ta.CandidateSweep(num_random=1000, grad_restarts=4, on_device=True)(lb, acq)
    # the default instance still refuses the stage
    plain, _ = ta.KG(n_points=16).construct_function(0, model, "min")
    with pytest.raises(NotImplementedError):
        ta.CandidateSweep(num_random=1000, grad_restarts=4, start_from_best=2)(lb, plain)
    sur.close()


def test_write_the_parity_record():
    """(last in the file) where KG_GRAD_PARITY_JSON names a file, the figures seen above go there: profiles/kg_grad_parity.json"""
    for gp, _, _ in _runs.values():
        gp.close()
    _runs.clear()
    out = os.environ.get("KG_GRAD_PARITY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
            f.write("\n")
