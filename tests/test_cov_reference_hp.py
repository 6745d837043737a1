"""CPU: (a) the f64 reference of the joint posterior (tests/cov_reference.py) against the 80-bit one
(tests/cov_reference_hp.py) on every model of tests/cov_edge_cases.py -- its errors are the e_ref the tight bars are built
from, recorded in tests/golden/cov_hp_eref.json (written where COV_HP_WRITE=1); (b) the bars reject, on every model, the
slips they exist for -- an f32 factor, f32 query points, a k-range one tile short, the noise left on a latent diagonal --
and the backward check rejects a stale trailing block and a non-zero above the diagonal; (c) the same comparisons run end
to end on the library's host backend (which says nothing about the kernels: tests/test_gpu_cov_edges.py does)."""
import json
import os
import warnings

import numpy as np
import pytest
from scipy.linalg import solve_triangular

import cov_edge_cases as ec
import cov_reference as cr
from oracle import gp_oracle as G

EREF_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cov_hp_eref.json")
NAMES = list(ec.MODELS)


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_f64_reference_against_the_80_bit_one(name):
    e = ec.e_ref(name)
    print("%s: e_ref mu %.3g cov observed %.3g latent %.3g of the scale" % (name, e["mu"], e["cov_observed"], e["cov_latent"]))
    assert e["cov_observed"] < 1e-12 and e["cov_latent"] < 1e-12 and e["mu"] < 1e-10
    if not ec.MODELS[name].get("append"):
        for latent in (False, True):
            bmu, bcov = ec.bars(name, latent)                 # (asserts the caps)
            assert bmu <= ec.CAP_VAL and bcov <= ec.CAP_COV


def test_the_recorded_e_ref():
    """tests/golden/cov_hp_eref.json is the record; a fresh value is at most 4 x the recorded one (more would mean the
    reference, the data or the arithmetic under them changed).  Below 8 u of the scale a value is last-bit noise of
    the BLAS underneath and is compared as 8 u."""
    fresh = {name: ec.e_ref(name) for name in NAMES}
    if os.environ.get("COV_HP_WRITE") == "1":
        with open(EREF_JSON, "w") as f:
            json.dump(dict(unit="fraction of the prior scale y_std^2 (c + noise) (cov) or its root (mu); m = 300", e_ref=fresh), f,
                      indent=1, sort_keys=True)
    with open(EREF_JSON) as f:
        rec = json.load(f)["e_ref"]
    assert sorted(rec) == sorted(NAMES)
    floor = 8 * ec.U
    for name in NAMES:
        assert sorted(rec[name]) == sorted(fresh[name])
        for k, v in fresh[name].items():
            assert max(v, floor) <= 4 * max(rec[name][k], floor), (name, k, v, rec[name][k])


# ---- (b) the bars have teeth -------------------------------------------------------------------------------------------
def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _copy_with_L(model, L):
    return G.GPModel(model.X, model.kind, model.constant, model.length_scale, model.noise, model.jitter, model.y_mean,
                     model.y_std, L, model.alpha, model.lml)


@pytest.mark.parametrize("name", NAMES)
def test_the_bars_reject_the_slips(name):
    model, Xq = ec.reference(name), ec.data(name)[3]
    for latent in (False, True):
        mu, cov, _ = cr.predict_cov(model, Xq, latent)
        ok = ec.judge_cov(name, mu, cov, latent)
        assert ok["ok"], ok                                    # the honest f64 computation passes ...
        slips = {}
        slips["factor rounded to f32"] = cr.predict_cov(_copy_with_L(model, _f32(model.L)), Xq, latent)[:2]
        slips["query points rounded to f32"] = cr.predict_cov(model, _f32(Xq), latent)[:2]
        Ks = G.cross_kernel(Xq, model.X, model.kind, model.constant, model.length_scale)
        V = solve_triangular(model.L, Ks.T, lower=True, check_finite=False)[:-16]
        Sigma = G.cross_kernel(Xq, Xq, model.kind, model.constant, model.length_scale) - V.T @ V
        if not latent:
            Sigma = Sigma + model.noise * np.eye(len(Xq))
        slips["the k-range one 16-wide tile short"] = (mu, model.y_std ** 2 * Sigma)
        if latent:
            slips["the noise left on the latent diagonal"] = cr.predict_cov(model, Xq, False)[:2]
        for what, (smu, scov) in slips.items():
            r = ec.judge_cov(name, smu, scov, latent)
            print("%s latent=%d %s: cov %.3g (bar %.3g) mu %.3g (bar %.3g)" % (name, latent, what, r["cov"], r["bar_cov"], r["mu"], r["bar_mu"]))
            assert not r["ok"], (what, r)                      # ... and each slip does not


@pytest.mark.parametrize("name", ec.SAMPLE_MODELS)
def test_the_backward_check_rejects_a_wrong_factor(name):
    m = 256                                                    # four full 64-blocks
    model = ec.reference(name)
    A, a_err = ec.factor_inputs(name, m)
    mu = cr.predict_cov(model, ec.data(name)[3][:m])[0]
    Af = np.asarray(A, dtype=np.float64)
    out = lambda Lc: mu[None, :] + model.y_std * Lc.T           # what sample_joint(eps = I) returns for this factor
    own = model.y_std ** 2 * Af                                 # (the matrix these factors are factors of, as a covariance)
    good = ec.judge_factor(out(ec.blocked_cholesky(Af)), mu, model.y_std, A, a_err, ec.A_ERR_FACTOR, own_cov=own)
    print("%s: blocked f64 factor %.3g of the bound (%.3g of the textbook bound against its own matrix), SciPy's %.3g"
          % (name, good["ratio"], good["own"], good["scipy_ratio"]))
    assert good["ok"] and good["scipy_ratio"] <= 1.0, good
    # the last diagonal block misses the last panel's update (it stays positive definite, so the factorisation goes through)
    stale = ec.judge_factor(out(ec.blocked_cholesky(Af, skip=(2, 3, 3))), mu, model.y_std, A, a_err, ec.A_ERR_FACTOR, own_cov=own)
    print("%s: with a stale trailing block %.3g of the bound" % (name, stale["ratio"]))
    assert stale["zeros"] and stale["diag"] and stale["ratio"] > 1.0 and stale["own"] > 1.0 and not stale["ok"], stale
    Lc = ec.blocked_cholesky(Af)
    Lc[70, 100] = 1e-3                                          # above the diagonal inside the second diagonal 64-block
    above = ec.judge_factor(out(Lc), mu, model.y_std, A, a_err, ec.A_ERR_FACTOR)
    assert not above["zeros"] and not above["ok"], above


# ---- (c) the harness end to end on the host backend --------------------------------------------------------------------
_host = {}


def _host_gp(name):
    if name not in _host:
        import turbo_amd._lib as L
        _host[name] = ec.fit_handle(L.NativeGP(L.DEVICE_HOST, "f64"), name)
    return _host[name]


@pytest.mark.parametrize("name", ec.HOST_MODELS)
@pytest.mark.parametrize("latent", [False, True])
def test_host_backend_covariance(name, latent):
    gp, Xq = _host_gp(name), ec.data(name)[3]
    mu, cov, neg = gp.predict_cov(Xq[:129], latent)
    r = ec.judge_cov(name, mu, cov, latent)
    print("host %s latent=%d: mu %.3g (bar %.3g) cov %.3g (bar %.3g)" % (name, latent, r["mu"], r["bar_mu"], r["cov"], r["bar_cov"]))
    assert r["ok"], r
    assert np.array_equal(cov, cov.T) and neg == int((np.diag(cov) < 0).sum())
    mu2, cov2, _ = gp.predict_cov(Xq[:129], latent)                       # the same bits from run to run
    assert mu2.tobytes() == mu.tobytes() and cov2.tobytes() == cov.tobytes()
    if not latent:                                                        # the diagonal is tgp_predict's sigma^2
        vs, _ = cr.scales(ec.reference(name))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sg = gp.evaluate(Xq[:129], want_sigma=True)["sigma"]
        assert np.abs(np.maximum(np.diag(cov), 0.0) - sg ** 2).max() <= 1e-5 * vs


@pytest.mark.parametrize("name", ec.HOST_MODELS)
def test_host_backend_samples_and_factor(name):
    gp, Xq, m = _host_gp(name), ec.data(name)[3], 129
    y = gp.sample_joint(Xq[:m], 5, eps=ec.sample_eps(m), latent=False, nugget=0.0)["y"]
    r = ec.judge_samples(name, m, y)
    print("host %s samples: %.3g (bar %.3g, e_ref %.3g)" % (name, r["err"], r["bar"], r["e_ref"]))
    assert r["ok"], r
    s = gp.sample_joint(Xq[:m], m, eps=np.eye(m), latent=False, nugget=0.0)
    A, a_err = ec.factor_inputs(name, m)
    f = ec.judge_factor(s["y"], s["mu"], ec.reference(name).y_std, A, a_err, ec.A_ERR_FACTOR, own_cov=gp.predict_cov(Xq[:m])[1])
    print("host %s factor: %.3g of the bound (%.3g of the textbook bound against its own matrix), SciPy's %.3g" % (name, f["ratio"], f["own"], f["scipy_ratio"]))
    assert f["ok"], f
