"""GPU: the knowledge gradient (tgp_kg_set_points / tgp_sweep_kg, the KG plugin) against tests/kg_reference.py and the
80-bit tests/kg_reference_hp.py, on the cases and under the bars of tests/kg_cases.py.  Every figure is printed before it
is asserted; where KG_PARITY_JSON names a file the last test writes them there (profiles/kg_parity.json)."""
import json
import os

import numpy as np
import pytest

import kg_cases as kc
import kg_reference as kr

pytestmark = pytest.mark.gpu

RECORD = {}
_runs = {}


def _L():
    import turbo_amd._lib as L
    return L


def _fit(name, gp=None):
    L = _L()
    gp = gp or L.NativeGP(0, kc.CASES[name].get("dtype", "f64"))
    gp.fit(*kc.fit_args(name))
    return gp


def _run(name):
    """the case's one full call: (handle, mu_a, result dict); made once, the handle left open for the tests that go on"""
    if name not in _runs:
        _, _, _, Xa, Xc = kc.data(name)
        gp = _fit(name)
        mu_a = gp.kg_set_points(Xa)
        gp.set_candidates(Xc)
        old = os.environ.get("TGP_CHUNK")
        if name == "n600":
            os.environ["TGP_CHUNK"] = "8192"          # three chunks, the last one partial
        try:
            r = gp.sweep_kg(kc.CASES[name]["sf"], want_kg=True, want_mu=True, want_sigma=True, want_cov=True)
        finally:
            if name == "n600":
                os.environ.pop("TGP_CHUNK") if old is None else os.environ.__setitem__("TGP_CHUNK", old)
        _runs[name] = (gp, mu_a, r)
    return _runs[name]


@pytest.mark.parametrize("name", kc.HP_CASES)
def test_end_to_end_against_the_80_bit_reference(name):
    gp, mu_a, r = _run(name)
    j = kc.judge_b(name, dict(kg=r["kg"], mu_a=mu_a, mu=r["mu"], cov=r["cov"]))
    print("(b) %s: err %s  bar %s" % (name, {k: "%.3g" % v for k, v in j["err"].items()}, {k: "%.3g" % v for k, v in j["bar"].items()}))
    # ... and the library's own joint posterior over [Xa; x] (latent): the same covariance by another route
    _, _, _, Xa, Xc = kc.data(name)
    A, m = len(Xa), kc.hp_rows(name)
    _, cov, _ = gp.predict_cov(np.vstack([Xa, Xc[:m]]), latent=True)
    own = float(np.abs(r["cov"][:m] - cov[A:, :A]).max()) / kc.scale(name) ** 2
    print("    cov_out against tgp_predict_cov(latent=1): %.3g (bar %.3g)" % (own, j["bar"]["cov"]))
    RECORD.setdefault(name, {}).update(b_err=j["err"], b_bar=j["bar"], e_ref=kc.e_ref(name), cov_vs_predict_cov=own)
    assert j["ok"], j
    assert own <= j["bar"]["cov"]
    assert np.all(np.isfinite(r["kg"])) and np.all(r["kg"] >= 0.0)


@pytest.mark.parametrize("name", list(kc.CASES))
def test_envelope_alone_and_the_argmax(name):
    gp, mu_a, r = _run(name)
    j = kc.judge_a(name, mu_a, r["mu"], r["sigma"], r["cov"], r["kg"])
    ref = kc.reference(name)["kg"]
    print("(a) %s: err %.3g  e_lines %.3g  bar %.3g;  best %d (numpy %d, reference %d)" % (
        name, j["err"], j["e_lines"], j["bar"], r["best_idx"], int(np.argmax(r["kg"])), int(np.argmax(ref))))
    RECORD.setdefault(name, {}).update(a_err=j["err"], a_e_lines=j["e_lines"], a_bar=j["bar"], kg_ms=r["kg_ms"])
    assert j["ok"], j
    assert r["best_val"] == r["kg"][r["best_idx"]]
    assert r["best_idx"] == int(np.argmax(r["kg"]))
    if kc.CASES[name].get("dtype", "f64") == "f64":
        assert r["best_idx"] == int(np.argmax(ref))          # unconditional: test_kg_reference.py holds the gap


def test_f32_handle():
    """The sweep in f32, everything behind it in f64: regret of best_idx under the f64 reference < 1e-3 relative and
    kg_out within 1e-5 of the prior scale.

    MEASURED on an MI355X, case "f32" (N = 600, D = 4, Matern 5/2, noise 1e-3, A = 64, M = 4096): regret 0, kg_out 9.7e-6
    of the scale.  That is the f32 sweep's sigma alone (3.5e-5 of the scale off the f64 reference; v(x) is the sweep's
    own by definition): the mean of a handle whose sweep is not f64 is re-formed in f64 from the chunk's cross-kernel.
    With the f32 sweep's mean as well (5.2e-5 off) kg_out was 1.9e-5, over the bar.  The `mu` the call returns is that
    f64 mean: held here under the cap of bar (b), which no f32 mean comes near."""
    name = "f32"
    gp, mu_a, r = _run(name)
    want = kc.reference(name)
    ref = want["kg"]
    best = float(ref.max())
    regret = (best - float(ref[r["best_idx"]])) / best
    err = float(np.abs(r["kg"] - ref).max()) / kc.scale(name)
    emu = float(np.abs(r["mu"] - want["mu"]).max()) / kc.scale(name)
    esg = float(np.abs(r["sigma"] - want["sigma"]).max()) / kc.scale(name)
    print("f32 handle: regret %.3g, kg error %.3g, mu error %.3g, sigma error %.3g of the scale" % (regret, err, emu, esg))
    RECORD.setdefault(name, {}).update(f32_regret=regret, f32_kg_err=err, f32_mu_err=emu, f32_sigma_err=esg)
    assert regret < kc.F32_REGRET
    assert err <= kc.F32_KG
    assert emu <= kc.CAP_VAL


def test_bits_run_to_run_rows_alone_and_permuted_points(monkeypatch):
    name = "n600"
    gp, mu_a, r = _run(name)
    sf = kc.CASES[name]["sf"]
    _, _, _, Xa, Xc = kc.data(name)
    monkeypatch.setenv("TGP_CHUNK", "8192")
    again = gp.sweep_kg(sf, want_kg=True, want_cov=True)
    assert again["kg"].tobytes() == r["kg"].tobytes() and again["cov"].tobytes() == r["cov"].tobytes()
    assert (again["best_idx"], again["best_val"]) == (r["best_idx"], r["best_val"])
    for i in (0, 8191, 8192, 16383, 16384, len(Xc) - 1):     # both sides of the chunk boundaries, the last row
        gp.set_candidates(Xc[i:i + 1])
        one = gp.sweep_kg(sf, want_kg=True, want_cov=True)
        assert one["cov"].tobytes() == r["cov"][i:i + 1].tobytes(), i
        assert one["kg"].tobytes() == r["kg"][i:i + 1].tobytes(), i
        assert one["best_idx"] == 0 and one["best_val"] == r["kg"][i]
    monkeypatch.delenv("TGP_CHUNK")
    gp.set_candidates(Xc)
    whole = gp.sweep_kg(sf, want_kg=True, want_cov=True)      # the default chunk: other chunk boundaries, the same bits
    assert whole["kg"].tobytes() == r["kg"].tobytes() and whole["cov"].tobytes() == r["cov"].tobytes()
    perm = np.random.RandomState(1).permutation(len(Xa))
    mu_p = gp.kg_set_points(Xa[perm])
    p = gp.sweep_kg(sf, want_kg=True, want_mu=True, want_sigma=True, want_cov=True)
    assert mu_p.tobytes() == mu_a[perm].tobytes()
    assert p["cov"].tobytes() == np.ascontiguousarray(r["cov"][:, perm]).tobytes()
    bar = kc.judge_a(name, mu_a, r["mu"], r["sigma"], r["cov"], r["kg"])["bar"]
    d = float(np.abs(p["kg"] - r["kg"]).max())
    print("permuted points: kg changes by %.3g (bar (a) %.3g)" % (d, bar))
    RECORD.setdefault(name, {}).update(permuted_kg_change=d)
    assert d <= bar
    gp.kg_set_points(Xa)


def test_the_call_leaves_the_handle_as_it_was():
    import torch
    L = _L()
    name = "n300"
    gp, _, r = _run(name)
    X, y, _, Xa, Xc = kc.data(name)
    sf = kc.CASES[name]["sf"]
    gp.set_candidates(Xc)
    rec = torch.zeros(Xc.shape[1] + 2, dtype=torch.float64, device="cuda:0")
    gp.set_winner_out(rec.data_ptr(), 500, keepalive=rec)

    def ei():
        out = gp.sweep(L.ACQ_EI, -1.0, float(y.min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)
        gp.winner_wait(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out, rec.cpu().numpy().copy()

    gp.ts_draw(3, 2, 256)
    ts0 = gp.ts_sweep(1.0, want_f=True)
    gp.mes_set_maxima(np.array([y.max(), y.max() + 0.1]))
    mes0 = gp.sweep(L.ACQ_MES, 1.0, want_acq=True)
    e0, w0 = ei()
    k = gp.sweep_kg(sf, want_kg=True)
    gp.winner_wait(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    wk = rec.cpu().numpy().copy()
    assert k["kg"].tobytes() == r["kg"].tobytes()
    assert wk[0] == k["best_val"] and wk[1] == 500 + k["best_idx"] and (wk[2:] == Xc[k["best_idx"]]).all()
    e1, w1 = ei()
    for key in ("mu", "sigma", "acq"):
        assert e1[key].tobytes() == e0[key].tobytes(), key
    assert (e1["best_idx"], e1["best_val"], e1["n_clamped"]) == (e0["best_idx"], e0["best_val"], e0["n_clamped"])
    assert w1.tobytes() == w0.tobytes()
    ts1 = gp.ts_sweep(1.0, want_f=True)
    assert ts1["f"].tobytes() == ts0["f"].tobytes() and (ts1["idx"] == ts0["idx"]).all()
    assert gp.sweep(L.ACQ_MES, 1.0, want_acq=True)["acq"].tobytes() == mes0["acq"].tobytes()
    gp.set_winner_out(None)


def test_points_belong_to_one_fit_and_argument_rules():
    L = _L()
    name = "n300"
    X, y, ls, Xa, Xc = kc.data(name)
    c = kc.CASES[name]
    sf = c["sf"]
    gp = L.NativeGP(0, "f64")
    with pytest.raises(RuntimeError):
        gp.D = X.shape[1]
        gp.kg_set_points(Xa)                                   # no model
    gp.fit(X[:-1], y[:-1], c["kind"], kc.C, ls, c["noise"], c["jitter"], True)
    gp.set_candidates(Xc[:100])
    with pytest.raises(ValueError, match="tgp_kg_set_points"):
        gp.sweep_kg(sf)                                        # no points yet
    dp = lambda a: a.ctypes.data_as(L._dp)
    big = np.zeros((257, X.shape[1]))
    bad = Xa.copy()
    bad[2, 1] = np.inf
    assert gp.lib.tgp_kg_set_points(gp._h, dp(big), 0, None) == 2
    assert gp.lib.tgp_kg_set_points(gp._h, dp(big), 257, None) == 2
    assert gp.lib.tgp_kg_set_points(gp._h, dp(bad), len(bad), None) == 2
    assert gp.lib.tgp_kg_set_points(gp._h, None, 3, None) == 2
    with pytest.raises(ValueError):
        gp.sweep_kg(sf)                                        # the refused calls stored nothing
    gp.kg_set_points(Xa)
    with pytest.raises(ValueError, match="sf"):
        gp.sweep_kg(0.5)
    first = gp.sweep_kg(sf, want_kg=True)
    gp.fit(X, y, c["kind"], kc.C, ls, c["noise"], c["jitter"], True, append=True)      # the one-row extension
    assert gp.appended
    gp.set_candidates(Xc[:100])
    with pytest.raises(ValueError, match="tgp_kg_set_points"):
        gp.sweep_kg(sf)
    gp.kg_set_points(Xa)
    app = gp.sweep_kg(sf, want_kg=True, want_cov=True)
    # an appended fit is served: its result is the full fit's to the figure DESIGN.md gives for an append (1e-9 of the scale)
    full = _run(name)[2]
    assert np.abs(app["kg"] - full["kg"][:100]).max() <= 1e-9 * kc.scale(name)
    assert not np.array_equal(first["kg"], app["kg"])
    gp.fit(X, y, c["kind"], kc.C, ls, c["noise"], c["jitter"], True)                   # a refit drops them
    gp.set_candidates(Xc[:100])
    with pytest.raises(ValueError, match="tgp_kg_set_points"):
        gp.sweep_kg(sf)
    gp.kg_set_points(Xa)
    mine = gp.sweep_kg(sf, want_kg=True, want_cov=True)
    assert mine["kg"].tobytes() == full["kg"][:100].tobytes()
    # a handle that received the factor: refused until it has points of its own, then the giver's bytes
    b = L.NativeGP(0, "f64")
    assert b.import_factor(gp.export_factor())
    b.set_candidates(Xc[:100])
    with pytest.raises(ValueError, match="tgp_kg_set_points"):
        b.sweep_kg(sf)
    b.kg_set_points(Xa)
    theirs = b.sweep_kg(sf, want_kg=True, want_cov=True)
    assert theirs["kg"].tobytes() == mine["kg"].tobytes() and theirs["cov"].tobytes() == mine["cov"].tobytes()
    b.import_factor(gp.export_factor())                        # ... and an import drops them again
    with pytest.raises(ValueError, match="tgp_kg_set_points"):
        b.sweep_kg(sf)
    b.close()
    g2 = L.NativeGP(0, "f64")                                  # no resident candidates
    g2.fit(X, y, c["kind"], kc.C, ls, c["noise"], c["jitter"], True)
    g2.kg_set_points(Xa)
    assert g2.lib.tgp_sweep_kg(g2._h, sf, None, None, None, None, None, None, None) == 2
    g2.close()
    gp.close()


def test_plugin_through_candidate_sweep():
    import torch
    import turbo_amd as ta
    from turbo_amd.bounds import Bounds
    from oracle import gp_oracle as o
    rng = np.random.RandomState(0)
    lb = Bounds([("x", -5.0, 10.0), ("y", 0.0, 15.0)])
    X = np.column_stack([rng.uniform(-5, 10, 30), rng.uniform(0, 15, 30)])
    x1, x2 = X[:, 0], X[:, 1]
    y = (x2 - 5.1 / (4 * np.pi ** 2) * x1 ** 2 + 5 / np.pi * x1 - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10
    kern = ta.GPKernel("matern52", 1.0, 3.0, 1e-4)
    sur = ta.HipGPSurrogate(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=0)
    model, _ = sur.construct_model(0, X, y)
    om = o.fit(X, y, "matern52", 1.0, 3.0, 1e-4, 1e-10, True)      # (the surrogate's default jitter)
    acq, info = ta.KG(n_points=16).construct_function(0, model, "min")
    assert info == {"n_points": 16, "default_points": True} and acq.get_name() == "KG"
    assert acq.points.tobytes() == X[np.argsort(y, kind="stable")[:16]].tobytes()      # the documented default
    # a host-drawn batch
    np.random.seed(5)
    x, info = ta.CandidateSweep(num_random=4096, grad_restarts=0)(lb, acq)
    np.random.seed(5)
    batch = ta.random_selector()(4096, lb)
    ref = kr.kg(om, acq.points, batch, -1.0)["kg"]
    i = int(np.argmax(ref))
    best, second = np.sort(ref)[::-1][:2]
    print("plugin, host batch: row %d, KG %.6g (library %.6g), gap %.3g" % (i, ref[i], info["max_acq"], (best - second) / best))
    assert (best - second) / best > kc.ARGMAX_MIN_GAP
    assert np.asarray(x).reshape(-1).tobytes() == batch[i].tobytes()
    assert abs(info["max_acq"] - ref[i]) <= 1e-9 * kr.prior_scale(om)
    vals = acq(batch[:300])
    assert np.abs(vals - ref[:300]).max() <= 1e-9 * kr.prior_scale(om)
    idx, v = acq.maximise_topk(batch, 5)
    assert idx.tolist() == np.argsort(-ref, kind="stable")[:5].tolist()
    # a device-generated batch
    x, info = ta.CandidateSweep(num_random=4096, grad_restarts=0, device_rng_seed=11)(lb, acq)
    ctx = model._ensure_resident()
    gen = ctx.read_candidates()
    refg = kr.kg(om, acq.points, gen, -1.0)["kg"]
    ig = int(np.argmax(refg))
    best, second = np.sort(refg)[::-1][:2]
    assert (best - second) / best > kc.ARGMAX_MIN_GAP
    assert np.asarray(x).reshape(-1).tobytes() == gen[ig].tobytes()
    # another instance's points displace this one's; this one sends its own again
    other, _ = ta.KG(points=X[:3]).construct_function(0, model, "min")
    other(batch[:10])
    assert acq(batch[:300]).tobytes() == vals.tobytes()
    for call in (lambda: acq.maximise_batch(batch, 2), lambda: acq.refine(batch[:2], [(-5, 10), (0, 15)]),
                 lambda: acq.lbfgsb(batch[:2], [(-5, 10), (0, 15)]), lambda: acq.value_and_grad(batch[:2])):
        with pytest.raises(NotImplementedError):
            call()
    assert acq.maximise_host_stream(4096, [-5.0, 0.0], [10.0, 15.0]) is None
    # a shard's winner record: [value, global index, row]
    rec = acq.winner_record(1000)
    bi, bv = acq.maximise(batch)
    ctx.winner_wait(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    w = rec.cpu().numpy()
    assert bi == i and w[0] == bv and w[1] == 1000 + i and w[2:].tobytes() == batch[i].tobytes()
    ctx.set_winner_out(None)


def test_write_the_parity_record():
    """(last in the file) where KG_PARITY_JSON names a file, the figures seen above go there: profiles/kg_parity.json"""
    for gp, _, _ in _runs.values():
        gp.close()
    _runs.clear()
    out = os.environ.get("KG_PARITY_JSON")
    if out:
        with open(out, "w") as f:
            json.dump(RECORD, f, indent=1, sort_keys=True)
            f.write("\n")
