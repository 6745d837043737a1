"""GPU: tgp_predict_cov / tgp_sample_joint (csrc/cov_kernels.hip) against tests/cov_reference.py, one case per place the
kernels can go wrong: the three size classes of the fit, a ragged blocked factor, an f32 handle (results still f64), and
m = one point / a ragged MFMA tile / a second 64-tile / several 128-tiles with a tail.

Every case prints its error as a fraction of the prior scale before it asserts, and the last test writes the worst per
case where COV_PARITY_JSON names a file (profiles/cov_parity.json); the bar is 1e-5."""
import json
import os

import numpy as np
import pytest

import cov_reference as cr
from oracle import gp_oracle as G

pytestmark = pytest.mark.gpu

TOL = 1e-5      # the project's bar for fp64 through the C-ABI (tests/test_gpu_parity.py), times the prior scale
# The nugget of the sample-parity cases.  Two Cholesky factors of one matrix differ by about cond(A) eps |Lc| in the
# directions of A's small eigenvalues; with the largest eigenvalue at most trace(A) = m (c + noise) = 390 here and the
# smallest at least the nugget, cond <= 4e8 and the difference in a sample stays below 4e8 x 2.2e-16 x |Lc| (<= 20) = 2e-6
# of the prior scale, inside the bar of 1e-5 (the latent covariance of 300 points in a unit square is singular to
# rounding without it: a smaller nugget would measure the conditioning, not the kernels).
NUGGET = 1e-6
CASES = {
    "one_workgroup": dict(N=5, D=2, kind="rbf", ard=False, dtype="f64"),
    "second_size_class": dict(N=200, D=3, kind="matern32", ard=False, dtype="f64"),
    "ragged_blocked": dict(N=300, D=5, kind="matern52", ard=True, dtype="f64"),
    "several_blocks_f32": dict(N=700, D=4, kind="matern12", ard=False, dtype="f32"),
}
MS = (1, 17, 65, 300)
WORST = {}


def _data(name):
    c = CASES[name]
    rng = np.random.RandomState(100 + c["N"])
    X = rng.uniform(0, 1, (c["N"], c["D"]))
    y = 1.5 + np.sin(3 * X.sum(1)) + 0.3 * X[:, 0] + 0.02 * rng.normal(size=c["N"])
    ls = rng.uniform(0.4, 0.9, c["D"]) if c["ard"] else 0.6
    Xq = rng.uniform(-0.05, 1.05, (300, c["D"]))
    Xq[5] = X[0]                              # a training point among the queries
    return X, y, ls, Xq


_cache = {}


def _fitted(name):
    """(handle, reference model, Xq): the fit and the reference are made once per case and shared"""
    if name not in _cache:
        import turbo_amd as ta
        c = CASES[name]
        X, y, ls, Xq = _data(name)
        gp = ta.NativeGP(0, c["dtype"])
        gp.fit(X, y, c["kind"], 1.3, ls, 1e-3, 1e-10, True)
        _cache[name] = (gp, G.fit(X, y, c["kind"], 1.3, ls, 1e-3, 1e-10, True), Xq, y)
    return _cache[name]


def _note(name, key, val):
    w = WORST.setdefault(name, {})
    w[key] = max(w.get(key, 0.0), float(val))


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("latent", [False, True])
def test_covariance_and_mean(name, m, latent):
    import turbo_amd._lib as L
    gp, model, Xq, y = _fitted(name)
    vs, ms = cr.scales(model)
    Xm = Xq[:m]
    mu, cov, neg = gp.predict_cov(Xm, latent)
    wmu, wcov, _ = cr.predict_cov(model, Xm, latent)
    emu, ecov = np.abs(mu - wmu).max() / ms, np.abs(cov - wcov).max() / vs
    print("%s m=%d latent=%d: mu %.3g cov %.3g of the prior scale" % (name, m, latent, emu, ecov))
    _note(name, "mu", emu); _note(name, "cov", ecov)
    assert emu <= TOL and ecov <= TOL
    assert np.array_equal(cov, cov.T)                                     # symmetric bit for bit
    assert neg == int((np.diag(cov) < 0).sum())
    mu2, cov2, _ = gp.predict_cov(Xm, latent)                             # the same bits from run to run
    assert mu2.tobytes() == mu.tobytes() and cov2.tobytes() == cov.tobytes()
    if not latent:                                                        # the diagonal is tgp_predict's sigma^2
        sg = gp.evaluate(Xm, want_sigma=True)["sigma"]
        ed = np.abs(np.maximum(np.diag(cov), 0.0) - sg ** 2).max() / vs
        _note(name, "diag_vs_predict", ed)
        assert ed <= TOL


@pytest.mark.parametrize("name", list(CASES))
def test_an_entry_depends_on_its_own_two_points_only(name):
    gp, model, Xq, y = _fitted(name)
    mu2, c2, _ = gp.predict_cov(Xq[:2])
    mu300, c300, _ = gp.predict_cov(Xq[:300])
    assert c2.tobytes() == c300[:2, :2].tobytes() and mu2.tobytes() == mu300[:2].tobytes()
    c65 = gp.predict_cov(Xq[:65])[1]
    assert c65.tobytes() == np.ascontiguousarray(c300[:65, :65]).tobytes()


@pytest.mark.parametrize("name", list(CASES))
def test_the_fit_and_the_next_sweep_are_untouched(name):
    import turbo_amd._lib as L
    gp, model, Xq, y = _fitted(name)
    rng = np.random.RandomState(1)
    Xc = rng.uniform(0, 1, (3000, Xq.shape[1]))
    gp.set_candidates(Xc)
    args = (L.ACQ_EI, -1.0, float(y.min()), 0.01)
    before = gp.sweep(*args, want_mu=True, want_sigma=True, want_acq=True)
    linv, alpha = gp.debug_read(L.BUF_LINV), gp.debug_read(L.BUF_ALPHA)
    gp.predict_cov(Xq[:65])
    gp.sample_joint(Xq[:65], 3, seed=5, nugget=NUGGET)
    after = gp.sweep(*args, want_mu=True, want_sigma=True, want_acq=True)
    for k in ("mu", "sigma", "acq"):
        assert before[k].tobytes() == after[k].tobytes(), k
    assert (before["best_idx"], before["best_val"]) == (after["best_idx"], after["best_val"])
    assert gp.debug_read(L.BUF_LINV).tobytes() == linv.tobytes() and gp.debug_read(L.BUF_ALPHA).tobytes() == alpha.tobytes()
    assert gp.read_candidates(0, 10).tobytes() == Xc[:10].tobytes()


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("m", MS)
def test_samples_given_the_normals(name, m):
    gp, model, Xq, y = _fitted(name)
    vs, ms = cr.scales(model)
    for latent in (False, True):
        eps = np.random.RandomState(m).standard_normal((5, m))
        r = gp.sample_joint(Xq[:m], 5, eps=eps, latent=latent, nugget=NUGGET)
        wy, wmu = cr.sample_joint(model, Xq[:m], eps, latent, NUGGET)
        ey = np.abs(r["y"] - wy).max() / ms
        print("%s m=%d latent=%d: samples %.3g of the prior scale" % (name, m, latent, ey))
        _note(name, "samples", ey)
        assert ey <= TOL and np.abs(r["mu"] - wmu).max() <= TOL * ms
        assert np.array_equal(r["eps"], eps)
        again = gp.sample_joint(Xq[:m], 5, eps=eps, latent=latent, nugget=NUGGET)
        assert again["y"].tobytes() == r["y"].tobytes()


@pytest.mark.parametrize("name", ["one_workgroup", "ragged_blocked"])
def test_the_device_draw(name):
    gp, model, Xq, y = _fitted(name)
    for seed in (0, 3, 2**64 - 1):
        r = gp.sample_joint(Xq[:17], 3, seed=seed, nugget=NUGGET)
        np.testing.assert_allclose(r["eps"], cr.normals(seed, 3, 17), rtol=0, atol=1e-14)
    a = gp.sample_joint(Xq[:17], 3, seed=3, nugget=NUGGET)
    b = gp.sample_joint(Xq[:65], 8, seed=3, nugget=NUGGET)
    assert a["eps"].tobytes() == np.ascontiguousarray(b["eps"][:3, :17]).tobytes()   # sample s depends neither on S nor on m
    vs, ms = cr.scales(model)
    wy, _ = cr.sample_joint(model, Xq[:65], b["eps"], False, NUGGET)
    assert np.abs(b["y"] - wy).max() <= TOL * ms
    S4096 = gp.sample_joint(Xq[:2], 4096, seed=1, nugget=NUGGET)          # the largest S: several 128-row tiles of normals
    assert abs(S4096["eps"].mean()) < 0.05 and abs(S4096["eps"].std() - 1) < 0.05
    wy, _ = cr.sample_joint(model, Xq[:2], S4096["eps"], False, NUGGET)
    assert np.abs(S4096["y"] - wy).max() <= TOL * ms


def test_duplicated_rows_need_a_nugget_also_on_a_received_factor():
    import turbo_amd as ta
    gp, model, Xq, y = _fitted("ragged_blocked")                         # N = 300
    other = ta.NativeGP(0, "f64")
    other.import_factor(gp.export_factor())
    dup = np.vstack([Xq[:70], Xq[3:4]])                                   # the duplicate sits in the second 64-block
    eps = np.random.RandomState(0).standard_normal((2, 71))
    vs, ms = cr.scales(model)
    for h in (gp, other):
        with pytest.raises(np.linalg.LinAlgError):
            h.sample_joint(dup, 2, eps=eps, latent=True, nugget=0.0)
        r = h.sample_joint(dup, 2, eps=eps, latent=True, nugget=1e-6)
        wy, _ = cr.sample_joint(model, dup, eps, True, 1e-6)
        assert np.abs(r["y"] - wy).max() <= TOL * ms
    mu_a, cov_a, _ = gp.predict_cov(Xq[:65])
    mu_b, cov_b, _ = other.predict_cov(Xq[:65])
    assert cov_a.tobytes() == cov_b.tobytes() and mu_a.tobytes() == mu_b.tobytes()


def test_bad_arguments_and_not_fitted():
    import turbo_amd as ta
    import turbo_amd._lib as L
    gp, model, Xq, y = _fitted("second_size_class")
    lib, h = gp.lib, gp._h
    dp = lambda a: a.ctypes.data_as(L._dp)
    X4 = np.ascontiguousarray(Xq[:4]); cov = np.empty((4, 4)); yo = np.empty((3, 4)); eps = np.zeros((3, 4))
    fresh = ta.NativeGP(0, "f64")                                         # no fit yet: TGP_NOT_FITTED -> RuntimeError
    assert lib.tgp_predict_cov(fresh._h, dp(X4), 4, 0, None, dp(cov), None) == 4
    assert lib.tgp_sample_joint(fresh._h, dp(X4), 4, 3, 0, 0.0, 1, None, dp(yo), None, None) == 4
    with pytest.raises(RuntimeError):
        fresh._check(4)
    bad = X4.copy(); bad[0, 0] = np.nan
    assert lib.tgp_predict_cov(h, dp(X4), 0, 0, None, dp(cov), None) == 2
    assert lib.tgp_predict_cov(h, dp(np.zeros((4097, 3))), 4097, 0, None, dp(cov), None) == 2
    assert lib.tgp_predict_cov(h, dp(bad), 4, 0, None, dp(cov), None) == 2
    assert lib.tgp_predict_cov(h, dp(X4), 4, 0, None, None, None) == 2
    assert lib.tgp_sample_joint(h, dp(X4), 4, 0, 0, 0.0, 1, None, dp(yo), None, None) == 2
    assert lib.tgp_sample_joint(h, dp(X4), 4, 4097, 0, 0.0, 1, None, dp(yo), None, None) == 2
    assert lib.tgp_sample_joint(h, dp(X4), 4, 3, 0, -1.0, 1, None, dp(yo), None, None) == 2
    assert lib.tgp_sample_joint(h, dp(X4), 4, 3, 0, float("nan"), 1, None, dp(yo), None, None) == 2
    eps[1, 1] = np.inf
    assert lib.tgp_sample_joint(h, dp(X4), 4, 3, 0, 0.0, 1, dp(eps), dp(yo), None, None) == 2
    assert lib.tgp_sample_joint(h, dp(X4), 4, 3, 0, 0.0, 1, None, dp(yo), None, None) == 0   # the nullable outputs


def test_joint_ei_and_the_model_instance():
    import turbo_amd as ta
    X, y, ls, Xq = _data("second_size_class")
    kern = ta.GPKernel("matern32", 1.3, ls, 1e-3)
    sur = ta.HipGPSurrogate(model_params=dict(kernel=kern, optimizer=None, normalize_y=True), training_iterations=1)
    model, _ = sur.construct_model(0, X, y)
    ref = G.fit(X, y, "matern32", 1.3, ls, 1e-3, 1e-10, True)
    vs, ms = cr.scales(ref)
    mu, cov = model.predict_cov(Xq[:17])
    assert mu.shape == (17, 1) and np.abs(cov - cr.predict_cov(ref, Xq[:17])[1]).max() <= TOL * vs
    eps = np.random.RandomState(4).standard_normal((512, 6))
    for ext in ("min", "max"):
        inc = float(y.min() if ext == "min" else y.max())
        got = ta.joint_ei(model, Xq[:6], ext, inc, xi=0.01, eps=eps)
        want = cr.joint_ei(ref, Xq[:6], eps, ext, inc, 0.01)
        assert abs(got - want) <= TOL * ms
    ys = model.sample_y(Xq[:17], n_samples=4, seed=9)
    assert ys.shape == (17, 4)
    assert ys.tobytes() == model.sample_y(Xq[:17], n_samples=4, seed=9).tobytes()
    wy, _ = cr.sample_joint(ref, Xq[:17], cr.normals(9, 4, 17), False, 1e-10)
    assert np.abs(ys.T - wy).max() <= TOL * ms


def test_record_the_worst_errors():
    """(last in the file) where COV_PARITY_JSON names a file, the worst errors seen above go there: profiles/cov_parity.json"""
    out = os.environ.get("COV_PARITY_JSON")
    if out and WORST:
        with open(out, "w") as f:
            json.dump(dict(bar=TOL, unit="fraction of the prior scale y_std^2 (c + noise) (cov) or its root (mu, samples)", worst=WORST), f, indent=1, sort_keys=True)
    for name, w in WORST.items():
        assert all(v <= TOL for v in w.values()), (name, w)
