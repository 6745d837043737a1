"""Round 4 (GPU): regressions the round-3 review found, and the round's new kernels against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(N, D=8, seed=0):
    rng = np.random.RandomState(seed + N + D)
    X = rng.uniform(0, 1, (N, D))
    return X, np.sin(3 * X.sum(1)) + 0.01 * rng.normal(size=N)


def _fit_ms(gp, X, y, reps=12):
    ts = []
    for _ in range(reps + 3):
        gp.fit(X, y, "matern52", 1.0, 1.1, 1e-4, 1e-10, True)
        ts.append(gp.profile_read()["last_fit_ms"])
    return float(np.median(ts[3:]))


def _ab_mode(mode):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ab_private_streams.py"), mode],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    return [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]


def test_fits_are_not_slower_after_a_side_by_side_hyper_parameter_fit():
    """Round 3's regression: after one threaded hyper-parameter fit at N <= 512 -- three handles on private
    streams, created BEFORE any fit large enough to want the background stream -- every later fit of the
    process took 2x (N = 2048: 1.00 -> 2.02 ms): the background stream, created as the process's 5th stream,
    shared a hardware queue with the main stream.  The reference's normal run is exactly this order: one
    factory, theta optimised at every trial with N growing (turbo/modules/surrogates.py:313-324,
    turbo/optimiser.py:335-336).  Each order runs in a process of its own (tools/ab_private_streams.py)."""
    base = _ab_mode("pair_first")[0]
    for mode in ("private_first_kept", "private_first_released", "plugin"):
        for rec in _ab_mode(mode):
            for key in ("fit_ms_n1000", "fit_ms_n2048"):
                assert rec[key] <= 1.3 * base[key], (mode, rec["stage"], key, rec[key], base[key])   # (the regression was 2x)


def test_fits_in_the_same_process_after_a_threaded_hyper_parameter_fit():
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    X, y = _data(2048)
    before = _fit_ms(gp, X, y)
    Xs, ys = _data(400)
    for opt in ("scipy", "fmin_l_bfgs_b"):      # the starts' threads in Python (rounds 3-4) | inside the library (the default)
        sur = ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel("matern52", 1.0, 1.0, 1e-2), normalize_y=True, optimizer=opt),
                                training_iterations=3, param_continuity=False, incremental=False)
        np.random.seed(11)
        _, info = sur.construct_model(0, Xs, ys)
        assert info["lml_evaluations"] > 3
        assert opt != "scipy" or (sur.last_worker_count == 3 and sur._workers == [])      # the starts did run side by side, and the borrowed views did not outlive the fit
        after = _fit_ms(gp, X, y)
        assert after <= 1.3 * before, (opt, before, after)   # (the regression was 2x)
        sur.close()


def test_bench_gpus2_launches_its_own_ranks_on_the_gpu_box():
    """`python bench.py --gpus 2` with no RANK in the environment: two gloo ranks share this box's one card
    (BENCH_BACKEND=gloo; the driver's runs use RCCL, one rank per GPU) -- the whole N > 1 step on device memory."""
    env = dict(os.environ, BENCH_BACKEND="gloo", OMP_NUM_THREADS="4")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "c1", "--steps", "2",
                          "--warmup", "1", "--no-opt-in"], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and "standin" not in out
    assert out["config"]["M_per_gpu"] == 32768 and out["scaling"] == "strong"
    assert out["roofline"]["launches"] > 0


def test_bench_plain_run_dumps_the_last_timed_step(tmp_path):
    """`python bench.py --config c1 --steps 3 --warmup 1 --dump-outputs DIR` on one GPU: the plain line (no --full legs),
    `steps` timed steps, and the dumped winner and fit scalars held to the oracle on the same synthetic inputs"""
    sys.path.insert(0, ROOT)
    import bench
    from oracle import gp_oracle as o
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "c1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0 and out["dtype"] == "f64"
    assert not {"cpu_baseline", "plugin", "opt_in"} & set(out) and out["overlapped_schedule"] is None
    d = {k: np.load(str(tmp_path / (k + ".npy"))) for k in ("best_val", "best_idx", "best_row", "n_clamped", "lml", "y_mean", "y_std")}
    assert all(a.dtype == np.float64 for a in d.values())
    cfg = dict(bench.CONFIGS["c1"])
    X, y, Xc, ls = bench.synth(cfg, 0, cfg["M"])
    om = o.fit(X, y, cfg["kind"], 1.0, ls, cfg["noise"], 1e-10, True)
    mu, sg = o.predict(om, Xc, True, chunk=16384)
    acq = o.acquisition(cfg["acq"], mu, sg, "min", cfg["param"], float(y.min()))
    bi = int(d["best_idx"][0])
    np.testing.assert_array_equal(d["best_row"], Xc[bi])
    assert d["best_val"][0] == pytest.approx(acq[bi], rel=1e-6) and d["best_val"][0] >= acq.max() - 1e-6 * abs(acq.max())
    assert d["lml"][0] == pytest.approx(om.lml, rel=1e-8)
    assert d["y_mean"][0] == pytest.approx(float(y.mean()), rel=1e-12) and d["y_std"][0] == pytest.approx(float(y.std()), rel=1e-12)


# ---- the one-launch sweep for 128 < N <= 512 (mid_sweep_kernel: 64 candidates per workgroup up to N = 256, 32 above) ----
RTOL = 1e-5          # BASELINE.json north_star: 1e-5 rtol (fp64) on mean / variance / acquisition
VAR_ATOL = 1e-9      # x (c + noise) y_std^2: the variance cancels near observed points


def _synth(seed, N, D, M):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, size=(N, D))
    w = rng.normal(size=D) / np.sqrt(D)
    y = np.sin(3 * X @ w) + 0.5 * ((X - 0.5) ** 2).sum(1) + 0.01 * rng.normal(size=N)
    return X, y, rng.uniform(0, 1, size=(M, D))


@pytest.mark.parametrize("kind,N,D,M,ard", [("rbf", 129, 2, 1000, False), ("matern52", 150, 5, 63, True),
                                            ("matern32", 192, 17, 64, False), ("matern12", 193, 3, 65, False),
                                            ("matern52", 200, 8, 10000, False), ("rbf", 255, 33, 777, True),
                                            ("matern52", 256, 8, 10000, True), ("rbf", 256, 70, 1, False),
                                            ("matern52", 257, 4, 33, False), ("rbf", 300, 6, 31, True),
                                            ("matern32", 384, 9, 2000, False), ("matern12", 385, 2, 32, False),
                                            ("matern52", 500, 8, 10000, False), ("rbf", 512, 20, 4097, True)])
def test_mid_sweep_vs_oracle(kind, N, D, M, ard, monkeypatch):
    """posterior mean / variance, every acquisition, arg-max, top-k and the zero-copy one-call form at the sizes the
    one-launch kernel serves (turbo/modules/surrogates.py:332-338 -> sklearn _gpr.py:443-494; acquisition_functions.py
    :147-158, :225-247, :336-358), against the oracle; M either side of the 64-candidate tile, N either side of the
    64-row blocks, candidates that ARE training points (variance -> clamp path)"""
    import turbo_amd as ta
    from oracle import gp_oracle as o
    if N > 256:
        monkeypatch.setenv("TGP_MID_MAXM", "16384")        # above N = 256 the one-launch sweep is opt-in (read at every call)
    X, y, Xc = _synth(5 + N + D, N, D, M)
    Xc[: min(M, 3)] = X[: min(M, 3)]                       # exact copies of training points
    ls = np.sqrt(D / 6.0) * ((0.5 + np.arange(D) / max(D - 1.0, 1.0)) if ard else 1.0)
    noise = 1e-4
    om = o.fit(X, y, kind, 1.3, ls, noise, 1e-10, True)
    omu, osig = o.predict(om, Xc)
    gp = ta.NativeGP(0, "f64")
    lml, _, _ = gp.fit(X, y, kind, 1.3, ls, noise, 1e-10, True)
    assert lml == pytest.approx(om.lml, rel=1e-9)
    var_atol = VAR_ATOL * (1.3 + noise) * om.y_std ** 2
    inc = float(y.min())
    gp.set_candidates(Xc)
    for acq_id, name, ext, sf, param in ((ta._lib.ACQ_EI, "ei", "min", -1.0, 0.01), (ta._lib.ACQ_PI, "pi", "max", 1.0, 0.01),
                                         (ta._lib.ACQ_UCB, "ucb", "min", -1.0, 2.0)):
        want = o.acquisition(name, omu, osig, ext, param, inc)
        r = gp.sweep(acq_id, sf, inc, param, want_mu=True, want_sigma=True, want_acq=True)
        np.testing.assert_allclose(r["mu"], omu, rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(r["sigma"] ** 2, osig ** 2, rtol=RTOL, atol=var_atol)
        np.testing.assert_allclose(r["acq"], want, rtol=RTOL, atol=1e-9 * max(1.0, float(np.abs(want).max())))
        assert r["best_idx"] == int(np.flatnonzero(r["acq"] == r["acq"].max())[0]) and r["best_val"] == r["acq"].max()
        r2 = gp.sweep(acq_id, sf, inc, param)                          # arg-max only: same winner, nothing copied back
        assert (r2["best_idx"], r2["best_val"]) == (r["best_idx"], r["best_val"])
        e = gp.evaluate(Xc, acq_id, sf, inc, param, want_mu=True, want_sigma=True, want_acq=True)   # zero-copy, one launch
        for k in ("mu", "sigma", "acq"):
            np.testing.assert_array_equal(e[k], r[k])
        assert (e["best_idx"], e["best_val"]) == (r["best_idx"], r["best_val"])
        gp.set_candidates(Xc)
        k = min(7, M)
        idx, vals = gp.sweep_topk(k, acq_id, sf, inc, param)
        order = np.lexsort((np.arange(M), -r["acq"]))[:k]
        np.testing.assert_array_equal(idx[:k], order)
        np.testing.assert_array_equal(vals[:k], r["acq"][order])
    p = gp.sweep(ta._lib.ACQ_NONE, 1.0, 0.0, 0.0, want_mu=True, want_sigma=True)     # predict
    np.testing.assert_array_equal(p["mu"], r["mu"])
    np.testing.assert_array_equal(p["sigma"], r["sigma"])
    s = gp.sweep(ta._lib.ACQ_SIGMA, 1.0, 0.0, 0.0, want_acq=True)
    np.testing.assert_array_equal(s["acq"], r["sigma"])


def test_mid_sweep_equals_the_four_launch_sweep_and_packs_the_winner_record(monkeypatch):
    """A/B against the general path (TGP_MID=0 in a child process: prep + cross-kernel + contraction + finalize),
    and the device-resident winner record of the sharded arg-max (tgp_set_winner_out) written by the LAST workgroup"""
    _mid_ab(230)
    monkeypatch.setenv("TGP_MID_MAXM", "16384")
    _mid_ab(450)


def _mid_ab(N):
    import torch
    import turbo_amd as ta
    X, y, Xc = _synth(77, N, 6, 5000)
    gp = ta.NativeGP(0, "f64")
    gp.fit(X, y, "matern52", 1.0, 0.9, 1e-3, 1e-10, True)
    gp.set_candidates(Xc)
    rec = torch.zeros(6 + 2, dtype=torch.float64, device="cuda:0")
    gp.set_winner_out(rec.data_ptr(), 1000000, keepalive=rec)
    inc = float(y.min())
    r = gp.sweep(ta._lib.ACQ_EI, -1.0, inc, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    h = rec.cpu().numpy()
    assert h[0] == r["best_val"] and h[1] == 1000000 + r["best_idx"]
    np.testing.assert_array_equal(h[2:], Xc[r["best_idx"]])
    for _ in range(20):                                        # the ticket counter is handed back at zero every time
        assert gp.sweep(ta._lib.ACQ_EI, -1.0, inc, 0.01)["best_idx"] == r["best_idx"]
    child = ("import sys, numpy as np; sys.path.insert(0, %r); import turbo_amd as ta\n"
             "z = np.load(sys.argv[1]); gp = ta.NativeGP(0, 'f64')\n"
             "gp.fit(z['X'], z['y'], 'matern52', 1.0, 0.9, 1e-3, 1e-10, True); gp.set_candidates(z['Xc'])\n"
             "r = gp.sweep(ta._lib.ACQ_EI, -1.0, float(z['y'].min()), 0.01, want_mu=True, want_sigma=True, want_acq=True)\n"
             "np.savez(sys.argv[2], mu=r['mu'], sigma=r['sigma'], acq=r['acq'], bi=r['best_idx'])\n" % ROOT)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        np.savez(os.path.join(d, "in.npz"), X=X, y=y, Xc=Xc)
        out = subprocess.run([sys.executable, "-c", child, os.path.join(d, "in.npz"), os.path.join(d, "out.npz")],
                             env=dict(os.environ, TGP_MID="0"), capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-3000:]
        z = np.load(os.path.join(d, "out.npz"))
        np.testing.assert_allclose(r["mu"], z["mu"], rtol=1e-11, atol=1e-12)
        np.testing.assert_allclose(r["sigma"] ** 2, z["sigma"] ** 2, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(r["acq"], z["acq"], rtol=1e-8, atol=1e-14)
        assert int(z["bi"]) == r["best_idx"]


def test_mid_sweep_through_the_plugins_and_latency(monkeypatch):
    """the plugin path at N = 200 / 256: predict(10^4) and an EI sweep of 10^4 candidates are one launch each, device
    time <= 0.12 ms; N = 500 with a plot-sized batch (4096 points: one round of 32-candidate
    workgroups) likewise"""
    import turbo_amd as ta
    from oracle import gp_oracle as o
    for N, M, bound in ((200, 10000, 0.12), (256, 10000, 0.12), (500, 4096, 0.14)):
        if N > 256:
            monkeypatch.setenv("TGP_MID_MAXM", "16384")
        X, y, Xc = _synth(N, N, 8, M)
        sur = ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel("matern52", 1.0, 1.1, 1e-4), optimizer=None,
                                                  normalize_y=True), training_iterations=1, incremental=False)
        model, _ = sur.construct_model(0, X, y)
        om = o.fit(X, y, "matern52", 1.0, 1.1, 1e-4, 1e-10, True)
        omu, osig = o.predict(om, Xc)
        mu, sg = model.predict(Xc, return_std_dev=True)
        np.testing.assert_allclose(mu, omu, rtol=RTOL, atol=1e-9)
        np.testing.assert_allclose(sg ** 2, osig ** 2, rtol=RTOL, atol=VAR_ATOL * om.y_std ** 2)
        f, _ = ta.EI(0.01).construct_function(0, model, "min", float(y.min()))
        want = o.acquisition("ei", omu, osig, "min", 0.01, float(y.min()))
        np.testing.assert_allclose(f(Xc), want, rtol=RTOL, atol=1e-12)
        ts = []
        for _ in range(12):
            bi, _ = f.maximise(Xc)
            ts.append(f.last_sweep_ms)
        assert bi == int(np.argmax(want))
        assert float(np.median(ts[2:])) <= bound, ts


def test_predict_many_stored_models_of_up_to_256_points():
    """tgp_predict_batch with stored models of 128 < N <= 256 (the plot path: one grid, every trial's model --
    turbo/plotting/trials.py:371, 448, 574-577): T fits as ONE launch of T workgroups (mid_fit_batch_kernel), T sweeps as
    one launch; rows equal the per-model predict to rounding and the oracle to the north_star tolerance; LML as the
    per-model fit's; a not-PD model is named"""
    import turbo_amd as ta
    from oracle import gp_oracle as o
    rng = np.random.RandomState(21)
    D, M = 3, 3000
    Xall = rng.uniform(0, 1, (256, D))
    yall = np.sin(4 * Xall[:, 0]) + 0.5 * Xall[:, 1] ** 2 + 0.02 * rng.normal(size=256)
    grid = rng.uniform(0, 1, (M, D))
    grid[:4] = Xall[:4]
    for kind, ls in (("matern52", 0.6), ("rbf", np.array([0.4, 0.9, 1.3]))):
        sur = ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel(kind, 1.2, ls, 1e-3), optimizer=None, normalize_y=True),
                                training_iterations=1, incremental=False)
        sizes = [129, 150, 191, 192, 193, 200, 230, 255, 256, 64, 128, 17]      # two size classes in one call
        models = [sur.construct_model(t, Xall[:n], yall[:n])[0] for t, n in enumerate(sizes)]
        mus, sgs = sur.predict_many(models, grid, return_std_dev=True)
        assert mus.shape == sgs.shape == (len(sizes), M)
        for t, (n, m) in enumerate(zip(sizes, models)):
            mu1, sg1 = m.predict(grid, return_std_dev=True)
            np.testing.assert_allclose(mus[t], mu1, rtol=1e-9, atol=1e-10)
            np.testing.assert_allclose(sgs[t] ** 2, sg1 ** 2, rtol=1e-7, atol=1e-11)
            if n in (129, 193, 256):
                om = o.fit(Xall[:n], yall[:n], kind, 1.2, ls, 1e-3, 1e-10, True)
                omu, osg = o.predict(om, grid)
                np.testing.assert_allclose(mus[t], omu, rtol=RTOL, atol=1e-9)
                np.testing.assert_allclose(sgs[t] ** 2, osg ** 2, rtol=RTOL, atol=VAR_ATOL * (1.2 + 1e-3) * om.y_std ** 2)
                assert m.get_log_likelihood() == pytest.approx(om.lml, rel=1e-9)
        # LML from the batch itself (models that have not been fitted one by one)
        fresh = [ta.HipGPSurrogate.ModelInstance(sur, Xall[:n], yall[:n], m.kernel.copy(), 1e-10, True) for n, m in zip(sizes, models)]
        sur.predict_many(fresh, grid[:10])
        for f, m in zip(fresh, models):
            assert f.log_likelihood == pytest.approx(m.get_log_likelihood(), rel=1e-9)
        sur.close()
    # a model that is not positive definite is named
    gp = ta.NativeGP(0, "f64")
    Xd = np.vstack([Xall[:150], Xall[:50]])                      # duplicated points, no noise, no jitter
    specs = [dict(X=Xall[:140], y=yall[:140], kind="rbf", constant=1.0, length_scale=0.5, noise=1e-3, jitter=1e-10, normalize_y=True),
             dict(X=Xd, y=np.r_[yall[:150], yall[:50]], kind="rbf", constant=1.0, length_scale=0.5, noise=0.0, jitter=0.0, normalize_y=True)]
    with pytest.raises(np.linalg.LinAlgError, match="model 1"):
        gp.predict_batch(specs, grid[:100], want_sigma=True)


def test_seeded_fuzz_128_to_256_points_vs_oracle():
    """24 seeded random problems in the range of the one-launch sweep and the one-workgroup batch fit (N 129 .. 256,
    D 1 .. 40, M 1 .. 3000, every kernel family, iso / ARD, noise 1e-6 .. 1e-1, with and without y normalisation):
    tgp_fit + tgp_sweep, tgp_evaluate and tgp_predict_batch against the oracle"""
    import turbo_amd as ta
    from oracle import gp_oracle as o
    rng = np.random.RandomState(20261004)
    gp = ta.NativeGP(0, "f64")
    kinds = ["rbf", "matern12", "matern32", "matern52"]
    for case in range(24):
        N = int(rng.randint(129, 257))
        D = int(rng.choice([1, 2, 3, 5, 8, 13, 17, 32, 40]))
        M = int(rng.choice([1, 7, 63, 64, 65, 500, 3000]))
        kind = kinds[case % 4]
        ard = bool(rng.randint(2)) and D > 1
        ls = rng.uniform(0.3, 2.0, D) * np.sqrt(D / 3.0) if ard else float(rng.uniform(0.3, 2.0) * np.sqrt(D / 3.0))
        const = float(rng.uniform(0.2, 5.0))
        noise = float(10 ** rng.uniform(-6, -1))
        norm = bool(rng.randint(2))
        X = rng.uniform(-1, 2, (N, D))
        y = np.sin(X @ rng.normal(size=D)) * 3.0 + 10.0 * norm + 0.1 * rng.normal(size=N)
        Xc = rng.uniform(-1, 2, (M, D))
        om = o.fit(X, y, kind, const, ls, noise, 1e-10, norm)
        omu, osg = o.predict(om, Xc)
        lml, ym, ys = gp.fit(X, y, kind, const, ls, noise, 1e-10, norm)
        assert lml == pytest.approx(om.lml, rel=1e-8, abs=1e-8), (case, N, D, kind)
        var_atol = VAR_ATOL * (const + noise) * om.y_std ** 2 * 10
        inc = float(y.min())
        want = o.acquisition("ei", omu, osg, "min", 0.01, inc)
        for r in (gp.evaluate(Xc, ta._lib.ACQ_EI, -1.0, inc, 0.01, want_mu=True, want_sigma=True, want_acq=True),):
            np.testing.assert_allclose(r["mu"], omu, rtol=RTOL, atol=1e-8 * om.y_std, err_msg=str((case, N, D, kind)))
            np.testing.assert_allclose(r["sigma"] ** 2, osg ** 2, rtol=RTOL, atol=var_atol, err_msg=str((case, N, D, kind)))
            np.testing.assert_allclose(r["acq"], want, rtol=1e-4, atol=1e-7 * max(1.0, float(np.abs(want).max())))
            assert r["best_val"] == r["acq"].max()
        spec = dict(X=X, y=y, kind=kind, constant=const, length_scale=ls, noise=noise, jitter=1e-10, normalize_y=norm)
        bmu, bsg, blml, _ = gp.predict_batch([spec, spec], Xc, want_sigma=True)
        np.testing.assert_array_equal(bmu[0], bmu[1])
        np.testing.assert_allclose(bmu[0], omu, rtol=RTOL, atol=1e-8 * om.y_std, err_msg=str((case, N, D, kind)))
        np.testing.assert_allclose(bsg[0] ** 2, osg ** 2, rtol=RTOL, atol=var_atol, err_msg=str((case, N, D, kind)))
        assert blml[0] == pytest.approx(om.lml, rel=1e-8, abs=1e-8)


def test_a_fit_beside_the_background_stream_repeats_bit_for_bit():
    """The same fit 150 times per size on one handle returns ONE log-likelihood.  Between N = 3700 and 6000 the
    trailing updates of the factorisation share the chip with the background stream's inverse; the direct-to-LDS
    k-loop of gemm64_glds.hpp once let a DMA write overtake a pending LDS read there and one fit in ten came out
    different at N = 5000 (tools/repeat_fit.py; LAPACK's dpotrf behind _gpr.py:349 has no such mood).  The sweep's
    k-loops carry the same wait: a sweep repeated beside nothing else is covered by the parity tests, here it is
    repeated right behind fits"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import repeat_fit
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    for N in (3700, 5000, 5500):
        r = repeat_fit.repeat(gp, N, 150)
        assert r["disagreeing"] == 0 and r["distinct"] == 1, r
    rng = np.random.RandomState(5)
    Xc = rng.uniform(0, 1, (20000, 7))
    gp.set_candidates(Xc)
    ref = None
    for _ in range(30):
        r = gp.sweep(ta._lib.ACQ_EI, -1.0, 0.0, 0.01, want_mu=True, want_sigma=True)
        cur = (r["best_idx"], r["mu"].tobytes(), r["sigma"].tobytes())
        ref = ref or cur
        assert cur == ref


def test_every_call_repeats_bit_for_bit_beside_other_threads():
    """tools/repeat_paths.py: fit + sweep in every sweep arithmetic, fit_grad, top-k + evaluate, the hyper-parameter
    fits and the batched predict, each repeated alone and then beside three threads that drive fits and sweeps on
    private streams -- the same bytes every time (with the f64 GEMM's old k-loop this run reports differences in
    the N >= 2304 fits: profiles/r04_repeat_paths.txt)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "repeat_paths.py"), "--quick", "--reps", "8"],
                         capture_output=True, text=True, timeout=900)
    lines = [json.loads(l) for l in out.stdout.splitlines() if l.startswith("{")]
    assert out.returncode == 0 and len(lines) > 30, out.stdout[-3000:] + out.stderr[-3000:]
    assert all(not np.any(l["differing"]) for l in lines)


@pytest.mark.parametrize("N", [6200, 6500, 6700, 7800, 8900])
def test_fit_with_a_ragged_last_outer_block_of_1024(N):
    """From Np = 6144 on the factorisation works in outer blocks of 1024 columns; Np is a multiple of 256, so the last
    block can be 256, 512 or 768 long.  Its own inverse is built by merging halves, which 768 is not: N = 6657 ... 6912,
    7681 ... 7936 and 8705 ... 8960 failed with `invalid configuration argument` (found by tools/repeat_fit.py over a
    ladder of sizes) and now take blocks of 512.  L, alpha and the likelihood against the oracle (dpotrf / cho_solve
    behind _gpr.py:349-360)"""
    import turbo_amd as ta
    from oracle import gp_oracle as o
    X, y = _data(N, 6)
    gp = ta.NativeGP(0, "f64")
    lml, _, _ = gp.fit(X, y, "matern52", 1.1, 0.8, 1e-3, 1e-10, True)
    om = o.fit(X, y, "matern52", 1.1, 0.8, 1e-3, 1e-10, True)
    assert abs(lml - om.lml) <= 1e-9 * abs(om.lml), (lml, om.lml)
    np.testing.assert_allclose(gp.debug_read(ta._lib.BUF_ALPHA), om.alpha, rtol=1e-6, atol=1e-7 * np.abs(om.alpha).max())
    Xc = np.random.RandomState(N).uniform(0, 1, (2000, 6))
    mu, sg = o.predict(om, Xc)
    gp.set_candidates(Xc)
    r = gp.sweep(ta._lib.ACQ_NONE, want_mu=True, want_sigma=True)
    np.testing.assert_allclose(r["mu"], mu, rtol=1e-7, atol=1e-7 * om.y_std)
    np.testing.assert_allclose(r["sigma"] ** 2, sg ** 2, rtol=1e-6, atol=1e-7 * om.y_std ** 2)


def test_fits_in_random_order_on_one_handle_equal_fresh_handles():
    """tools/order_fit.py: what an earlier fit of another size left in the handle's buffers does not matter
    (the inverse factor is only zero-filled when needed since round 4)"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "order_fit.py"), "--count", "40", "--max-n", "5000"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert json.loads(out.stdout.splitlines()[-1])["differing"] == []
