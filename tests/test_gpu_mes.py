"""Max-value entropy search on the GPU (ACQ_MES, tgp_mes_set_maxima, tgp_mes_draw, the MES plugin), held to
tests/mes_reference.py and oracle.gp_oracle.

Bar (a): acq_out against the reference fed the call's OWN mu / sigma outputs -- the new arithmetic alone -- every row
within 1e-9 x the sweep's best value (tests/test_gpu_batch_mc.py's bar for averaged acquisitions).
Bar (b): end to end against the oracle's predict + the reference, f64 handles: regret <= 1e-9 relative and the same
index where the reference's top two differ by more than that (tests/test_gpu_batch.py's bar); the f32 handle: the f32
bars of tests/test_gpu_configs.py (rtol 1e-5 on the vector against the f64 handle's neighbourhood is not applicable to
an entropy whose gamma divides by sigma_f, so its REGRET bar is used: regret < 1e-3 relative).
Gradient: the bar for tgp_acq_grad's ACQ_NONE / ACQ_SIGMA / UCB / PI / EI gradients themselves is
tests/test_gpu_acq_grad_edges.py's (an 80-bit closed form, 64 max(e_ref, N u) of the batch maximum under a cap of 1e-9).
The MES gradient is held here to its closed form over the device's own ACQ_NONE / ACQ_SIGMA gradients -- which that
file pins -- and to central differences at tests/test_gpu_parity.py's bar (rtol 2e-4, atol max(2e-6 scale, 2e-9),
h = 1e-6).
Row by row, on every branch of h and dh (gamma from -1e300 to the underflow) and at bars built from an 80-bit reference:
tests/test_gpu_mes_edges.py."""
import numpy as np
import pytest

from oracle import gp_oracle as o
import mes_reference as mr

pytestmark = pytest.mark.gpu

A_TOL = 1e-9
REGRET_F32 = 1e-3
_cache = {}


def _problem(N, D, M, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    w = rng.normal(size=D) / np.sqrt(D)
    y = 3.0 + 2.0 * np.sin(3 * X @ w) + 0.5 * ((X - 0.5) ** 2).sum(1) + 0.01 * rng.normal(size=N)
    ls = float(np.sqrt(D / 6.0))
    Xc = rng.uniform(0, 1, (M, D))
    return X, y, ls, Xc


def _gp(dtype, X, y, kind, ls, noise, normalize_y=True, Xc=None):
    import turbo_amd as ta
    gp = ta.NativeGP(0, dtype)
    gp.fit(X, y, kind, 1.0, ls, noise, 1e-10, normalize_y)
    if Xc is not None:
        gp.set_candidates(Xc)
    return gp


def _oracle(key, X, y, kind, ls, noise, ny, Xc):
    """the oracle's posterior over a case's batch, computed once and shared (read-only)"""
    if key not in _cache:
        m = o.fit(X, y, kind, 1.0, ls, noise, 1e-10, ny)
        mu, sg = o.predict(m, Xc, chunk=4096)
        mu.setflags(write=False)
        sg.setflags(write=False)
        _cache[key] = (m, mu, sg)
    return _cache[key]


def _maxima(y, S, sf, seed):
    """caller-supplied maxima around and beyond the best observation (teacher forcing)"""
    rng = np.random.RandomState(seed)
    best = y.max() if sf > 0 else y.min()
    return best + sf * np.abs(rng.normal(size=S)) * 0.5 * y.std()


def _mes():
    import turbo_amd as ta
    return ta._lib.ACQ_MES


# N, D, M, kind, dtype, noise, normalize_y: the one-workgroup, the one-launch and the general sweep (last chunk partial), f32
SHAPES = [
    (40, 2, 3000, "matern52", "f64", 1e-3, True),
    (200, 4, 8192, "rbf", "f64", 1e-4, True),
    (600, 8, 20000, "matern32", "f64", 1e-3, False),
    (600, 8, 20000, "matern12", "f64", 0.0, True),
    (600, 8, 20000, "matern52", "f32", 1e-3, True),
]


@pytest.mark.parametrize("S", [1, 5, 64])
@pytest.mark.parametrize("shape", SHAPES, ids=["N%d-%s-%s-noise%g" % (s[0], s[3], s[4], s[5]) for s in SHAPES])
def test_every_sweep_path_with_given_maxima(shape, S, monkeypatch):
    N, D, M, kind, dtype, noise, ny = shape
    monkeypatch.setenv("TGP_CHUNK", "8192")            # N = 600: 20 000 candidates end in a partial chunk
    X, y, ls, Xc = _problem(N, D, M, N + D)
    gp = _gp(dtype, X, y, kind, ls, noise, ny, Xc)
    worst = 0.0
    for sf in (1.0, -1.0):
        ys = _maxima(y, S, sf, S)
        gp.mes_set_maxima(ys)
        r = gp.sweep(_mes(), sf, 0.0, 0.0, want_mu=True, want_sigma=True, want_acq=True)
        y_std = float(y.std()) if ny else 1.0
        if ny:
            m, _, _ = _oracle((shape[:4], noise, ny), X, y, kind, ls, noise, ny, Xc)
            y_std = m.y_std
        # (a) the new arithmetic alone
        want = mr.mes(r["mu"], r["sigma"], ys, sf, noise, y_std)
        best = float(want.max())
        err = float(np.abs(r["acq"] - want).max())
        worst = max(worst, err / best)
        print("bar (a) N=%d %s S=%d sf=%+d: max |a - ref| / best = %.3e" % (N, dtype, S, sf, err / best))
        assert err <= A_TOL * best, (err, best)
        assert np.all(np.isfinite(r["acq"])) and np.all(r["acq"] >= 0.0)
        assert r["best_val"] == r["acq"][r["best_idx"]] and r["best_idx"] == int(np.argmax(r["acq"]))
        # (b) end to end against the oracle
        m, omu, osg = _oracle((shape[:4], noise, ny), X, y, kind, ls, noise, ny, Xc)
        ref = mr.mes(omu, osg, ys, sf, noise, m.y_std)
        rb = float(ref.max())
        regret = (rb - float(ref[r["best_idx"]])) / rb
        print("bar (b) N=%d %s S=%d sf=%+d: regret = %.3e" % (N, dtype, S, sf, regret))
        if dtype == "f64":
            assert regret <= 1e-9, regret
            top2 = np.sort(ref)[-2:]
            if top2[1] - top2[0] > 1e-9 * rb:
                assert r["best_idx"] == int(np.argmax(ref))
        else:
            assert regret < REGRET_F32, regret


@pytest.mark.parametrize("N,D,M,kind", [(40, 2, 3000, "matern52"), (200, 4, 8192, "rbf"), (600, 8, 20000, "matern32")])
def test_evaluate_topk_winner_and_prune_state(N, D, M, kind):
    import torch
    X, y, ls, Xc = _problem(N, D, M, N + D)
    gp = _gp("f64", X, y, kind, ls, 1e-3, True, Xc)
    ys = _maxima(y, 5, -1.0, 2)
    gp.mes_set_maxima(ys)
    rec = torch.zeros(D + 2, dtype=torch.float64, device="cuda:0")
    gp.set_winner_out(rec.data_ptr(), 1000, keepalive=rec)
    r = gp.sweep(_mes(), -1.0, 0.0, 0.0, want_acq=True)
    only = gp.sweep(_mes(), -1.0, 123.0, 4.0)               # arg-max only; incumbent and param are ignored
    assert gp.last_prune()["state"] == -1                   # the unpruned schedule, TGP_SWEEP_PRUNE at its default
    assert (only["best_idx"], only["best_val"]) == (r["best_idx"], r["best_val"])
    gp.winner_wait(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    w = rec.cpu().numpy()
    assert w[0] == r["best_val"] and w[1] == 1000 + r["best_idx"]
    np.testing.assert_array_equal(w[2:], Xc[r["best_idx"]])
    idx, vals = gp.sweep_topk(8, _mes(), -1.0)
    order = np.argsort(-r["acq"], kind="stable")[:8]
    np.testing.assert_array_equal(idx, order)
    assert vals.tobytes() == r["acq"][order].tobytes()
    e = gp.evaluate(Xc, _mes(), -1.0, want_acq=True)
    assert e["acq"].tobytes() == r["acq"].tobytes() and e["best_idx"] == r["best_idx"]


@pytest.mark.parametrize("N,D,kind", [(40, 2, "matern52"), (600, 8, "rbf")])
@pytest.mark.parametrize("m", [1, 3, 64])
def test_value_and_gradient(N, D, kind, m):
    """The 1e-12 relative agreement of tgp_acq_grad's value with the sweep's is between two kernel families that sum mu
    and the variance in different orders, so the query points are taken where the value is well conditioned in them:
    h's relative condition number in gamma is ~gamma^2 in its upper tail, and gamma's in the variance is
    kss / (2 sigma_f^2) -- the latent variance is what is left of kss = c + noise after k^T K^-1 k AND the noise are
    taken off.  The m points are the first of a uniform pool with |gamma_s| <= 4 for every maximum and
    sigma_f^2 >= kss y_std^2 / 20 (the length scale is a quarter of the other tests', so that such points exist): a few
    ulps of difference in mu and the variance times 16 x 10 stay an order below the bar.  (Measured on points taken
    without that rule at N = 40: 9.0e-12 relative at a value of 3.3e-18 (gamma = 8.7, sigma_f^2 / kss ~ 1e-3) and
    6.3e-12 at 5.3e-22 -- 1e-17 of the sweep's best value and less; bar (a) covers such rows at 1e-9 x best.)"""
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, _ = _problem(N, D, 1, N + D)
    ls = 0.25 * ls
    noise = 1e-3
    pool = np.random.RandomState(m).uniform(0.05, 0.95, (4000, D))
    gp = _gp("f64", X, y, kind, ls, noise, True, pool)
    post = gp.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
    y_std = o.fit(X, y, kind, 1.0, ls, noise, 1e-10, True).y_std
    for sf in (1.0, -1.0):
        ys = _maxima(y, 5, sf, 9)
        v = mr.latent_var(post["sigma"], noise, y_std)
        ok = v >= (1.0 + noise) * y_std ** 2 / 20.0
        gam = sf * (ys[None, :] - post["mu"][:, None]) / np.sqrt(np.where(ok, v, 1.0))[:, None]
        ok &= np.abs(gam).max(1) <= 4.0
        assert ok.sum() >= m, int(ok.sum())
        Xq = pool[ok][:m]
        gp.set_candidates(Xq)
        gp.mes_set_maxima(ys)
        val, grad = gp.acq_grad(Xq, L.ACQ_MES, sf)
        sw = gp.sweep(L.ACQ_MES, sf, want_acq=True)["acq"]
        print("acq_grad vs sweep N=%d m=%d sf=%+d: max relative difference %.3e" % (N, m, sf, float(np.max(np.abs(val - sw) / sw))))
        np.testing.assert_allclose(val, sw, rtol=1e-12, atol=0)
        # central differences of the device's own value
        h = 1e-6
        fd = np.empty_like(grad)
        for d in range(D):
            e = np.zeros(D)
            e[d] = h
            fd[:, d] = (gp.acq_grad(Xq + e, L.ACQ_MES, sf)[0] - gp.acq_grad(Xq - e, L.ACQ_MES, sf)[0]) / (2 * h)
        scale = np.abs(fd).max() + 1e-12
        np.testing.assert_allclose(grad, fd, rtol=2e-4, atol=max(2e-6 * scale, 2e-9))
        # the reference's closed form: da = cm dmu + cs dsigma with the device's own mu, sigma and their gradients
        mu, gmu = gp.acq_grad(Xq, L.ACQ_NONE, sf)
        sg, gsg = gp.acq_grad(Xq, L.ACQ_SIGMA, sf)
        a, cm, cs = mr.mes_coefficients(mu, sg, ys, sf, noise, y_std)
        np.testing.assert_allclose(val, a, rtol=0, atol=A_TOL * float(a.max()))
        want = cm[:, None] * gmu + cs[:, None] * gsg
        np.testing.assert_allclose(grad, want, rtol=0, atol=1e-9 * float(np.abs(want).max()))


@pytest.mark.parametrize("N,D", [(40, 2), (600, 8)])
def test_lbfgsb_never_ends_below_its_start(N, D):
    import turbo_amd as ta
    X, y, ls, _ = _problem(N, D, 1, N + D)
    gp = _gp("f64", X, y, "matern52", ls, 1e-3, True)
    gp.mes_set_maxima(_maxima(y, 8, 1.0, 4))
    X0 = np.random.RandomState(0).uniform(0.1, 0.9, (4, D))
    v0, _ = gp.acq_grad(X0, ta._lib.ACQ_MES, 1.0)
    x, v, st, ev = gp.acq_refine(X0, [0.0] * D, [1.0] * D, ta._lib.ACQ_MES, 1.0, lbfgsb=True)
    assert np.all(v >= v0) and np.all(x >= 0) and np.all(x <= 1) and ev >= 4
    np.testing.assert_allclose(gp.acq_grad(x, ta._lib.ACQ_MES, 1.0)[0], v, rtol=1e-12, atol=0)


@pytest.mark.parametrize("N,D,M", [(40, 2, 3000), (600, 8, 20000)])
def test_mes_draw_is_the_thompson_sweep(N, D, M):
    X, y, ls, Xc = _problem(N, D, M, N + D)
    gp = _gp("f64", X, y, "matern52", ls, 1e-3, True, Xc)
    other = _gp("f64", X, y, "matern52", ls, 1e-3, True, Xc)
    for sf in (1.0, -1.0):
        other.ts_draw(77, 8, 256)
        val = other.ts_sweep(sf)["val"]
        got = gp.mes_draw(77, 8, 256, sf)                   # NaN incumbent: the sampled maxima as they are
        assert got.tobytes() == val.tobytes()
        inc = float(np.sort(val)[4])                        # an incumbent better than some of them
        got2 = gp.mes_draw(77, 8, 256, sf, inc)
        want = np.where(sf * inc > sf * val, inc, val)
        assert got2.tobytes() == want.tobytes() and np.any(got2 != val)
        a = gp.sweep(_mes(), sf, want_acq=True)
        other.mes_set_maxima(want)
        b = other.sweep(_mes(), sf, want_acq=True)
        assert a["acq"].tobytes() == b["acq"].tobytes() and a["best_idx"] == b["best_idx"]
        assert gp.ts_sweep(sf)["val"].tobytes() == val.tobytes()      # the Thompson draw stays in the handle


def test_rules():
    import ctypes
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, Xc = _problem(300, 3, 2000, 1)
    gp = _gp("f64", X, y, "matern52", ls, 1e-3, True, Xc)
    with pytest.raises(ValueError, match="maxima"):
        gp.sweep(L.ACQ_MES)
    gp.mes_set_maxima([y.max()])
    gp.sweep(L.ACQ_MES)
    gp.fit(X, y, "matern52", 1.0, ls, 1e-3, 1e-10, True)                  # a refit drops them
    with pytest.raises(ValueError, match="maxima"):
        gp.sweep(L.ACQ_MES)
    gp.mes_set_maxima([y.max()])
    X2 = np.vstack([X, [[0.5, 0.5, 0.5]]])
    gp.fit(X2, np.append(y, 3.0), "matern52", 1.0, ls, 1e-3, 1e-10, True, append=True)
    assert gp.appended
    with pytest.raises(ValueError, match="maxima"):
        gp.acq_grad(Xc[:2], L.ACQ_MES)
    giver = _gp("f64", X, y, "matern52", ls, 1e-3, True)
    gp.mes_set_maxima([y.max()])
    gp.import_factor(giver.export_factor())
    gp.set_candidates(Xc)
    with pytest.raises(ValueError, match="maxima"):
        gp.sweep_topk(4, L.ACQ_MES)
    gp.mes_set_maxima([y.max(), y.max() + 1.0])
    # the three refusing entries
    with pytest.raises(ValueError):
        gp.sweep_batch(2, acq=L.ACQ_MES)
    with pytest.raises(ValueError):
        gp.sweep_batch_mc(2, 4, acq=L.ACQ_MES)
    with pytest.raises(ValueError):
        gp.acq_refine(Xc[:2], [0] * 3, [1] * 3, L.ACQ_MES)
    for bad in ([], list(range(65)), [1.0, float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            gp.mes_set_maxima(bad)
    assert gp.sweep(L.ACQ_MES)["best_val"] > 0          # the failed calls left the maxima in place


def test_degenerate_inputs_stay_finite():
    import turbo_amd as ta
    L = ta._lib
    for N, D in ((40, 2), (600, 8)):
        X, y, ls, Xc = _problem(N, D, 1000, 3)
        Xc[:20] = X[:20]                                    # copies of training points
        gp = _gp("f64", X, y, "matern52", ls, 1e-3, True, Xc)
        gp.mes_set_maxima(_maxima(y, 5, 1.0, 1))
        r = gp.sweep(L.ACQ_MES, 1.0, want_acq=True)
        assert np.all(np.isfinite(r["acq"])) and np.all(r["acq"] >= 0)
        # y* 50 sigma below every mu
        p = gp.sweep(L.ACQ_NONE, want_mu=True, want_sigma=True)
        gp.mes_set_maxima([float(p["mu"].min() - 50.0 * p["sigma"].max())])
        r = gp.sweep(L.ACQ_MES, 1.0, want_acq=True)
        assert np.all(np.isfinite(r["acq"])) and 0 <= r["best_idx"] < 1000
        # S = 1, y* far above everything: values underflow, the index stays valid
        gp.mes_set_maxima([1e6])
        r = gp.sweep(L.ACQ_MES, 1.0, want_acq=True)
        assert np.all(r["acq"] < 1e-300) and np.all(r["acq"] >= 0) and 0 <= r["best_idx"] < 1000
        # noise 0: rows whose variance clamps to 0 give exactly 0
        g0 = _gp("f64", X, y, "rbf", 3.0 * ls, 0.0, True, Xc)
        g0.mes_set_maxima(_maxima(y, 5, 1.0, 1))
        r0 = g0.sweep(L.ACQ_MES, 1.0, want_sigma=True, want_acq=True)
        zero = r0["sigma"] == 0.0
        assert np.all(r0["acq"][zero] == 0.0) and np.all(np.isfinite(r0["acq"]))


def test_other_acquisitions_do_not_see_the_maxima():
    import turbo_amd as ta
    L = ta._lib
    X, y, ls, Xc = _problem(600, 8, 20000, 11)
    a = _gp("f64", X, y, "matern52", ls, 1e-3, True, Xc)
    b = _gp("f64", X, y, "matern52", ls, 1e-3, True, Xc)
    b.mes_set_maxima(_maxima(y, 64, -1.0, 5))
    for acq, par in ((L.ACQ_EI, 0.01), (L.ACQ_PI, 0.01), (L.ACQ_UCB, 2.0), (L.ACQ_SIGMA, 0.0)):
        ra = a.sweep(acq, -1.0, float(y.min()), par, want_acq=True)
        rb = b.sweep(acq, -1.0, float(y.min()), par, want_acq=True)
        assert ra["acq"].tobytes() == rb["acq"].tobytes()
        assert (ra["best_idx"], ra["best_val"]) == (rb["best_idx"], rb["best_val"])
        assert a.sweep(acq, -1.0, float(y.min()), par)["best_idx"] == b.sweep(acq, -1.0, float(y.min()), par)["best_idx"]


def test_plugin_through_candidate_sweep():
    import dill
    import turbo_amd as ta
    from turbo_amd.bounds import Bounds
    rng = np.random.RandomState(0)
    lb = Bounds([("x", -5.0, 10.0), ("y", 0.0, 15.0)])
    X = np.column_stack([rng.uniform(-5, 10, 30), rng.uniform(0, 15, 30)])
    x1, x2 = X[:, 0], X[:, 1]
    y = (x2 - 5.1 / (4 * np.pi ** 2) * x1 ** 2 + 5 / np.pi * x1 - 6) ** 2 + 10 * (1 - 1 / (8 * np.pi)) * np.cos(x1) + 10
    kern = ta.GPKernel("matern52", 1.0, 3.0, 1e-4)
    sur = ta.HipGPSurrogate(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=0)
    model, _ = sur.construct_model(0, X, y)
    picks = []
    for _ in range(2):
        acq, info = ta.MES(n_samples=8, seed=3).construct_function(0, model, "min")
        assert acq.get_name() == "MES" and info["n_samples"] == 8
        np.random.seed(5)
        x, info = ta.CandidateSweep(num_random=4096, grad_restarts=3)(lb, acq)
        picks.append((np.asarray(x, dtype=np.float64).reshape(-1).copy(), float(info["max_acq"]), acq))
    assert picks[0][0].tobytes() == picks[1][0].tobytes() and picks[0][1] == picks[1][1]
    x, v, acq = picks[0]
    assert -5.0 <= x[0] <= 10.0 and 0.0 <= x[1] <= 15.0 and acq.maxima.shape == (8,)
    mu, sg = model.predict(x.reshape(1, -1), return_std_dev=True)
    want = mr.mes(mu, sg, acq.maxima, -1.0, 1e-4, model.y_std)[0]
    assert abs(v - want) <= A_TOL * max(want, float(acq(x.reshape(1, -1))[0]))
    np.random.seed(5)
    _, i0 = ta.CandidateSweep(num_random=4096, grad_restarts=0)(lb, ta.MES(8, seed=3).construct_function(0, model, "min")[0])
    assert v >= i0["max_acq"] * (1 - 1e-12)          # the same batch, the same maxima: the gradient stage only improves
    g = np.stack(np.meshgrid(np.linspace(-5, 10, 50), np.linspace(0, 15, 50)), -1).reshape(-1, 2)
    before = acq(g)
    again = dill.loads(dill.dumps(acq))
    assert again.maxima.tobytes() == acq.maxima.tobytes()
    assert again(g).tobytes() == before.tobytes()
    with pytest.raises(NotImplementedError):
        acq.maximise_batch(g, 2)
    with pytest.raises(NotImplementedError):
        acq.refine(g[:2], [(-5, 10), (0, 15)])
