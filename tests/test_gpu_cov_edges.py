"""GPU: tgp_predict_cov / tgp_sample_joint (csrc/cov_kernels.hip) held to an 80-bit reference (tests/cov_reference_hp.py)
at the edges the kernels are made of.  Models, bars and comparisons: tests/cov_edge_cases.py (the bars are
64 max(e_ref, N u) of the prior scale under caps of 1e-10 / 1e-9 -- four to five orders under tests/test_gpu_cov.py's 1e-5,
and tests/test_cov_reference_hp.py shows on the CPU that they reject an f32 factor, f32 query points, a k-range one tile
short and a stale trailing block).

 (a) one call of m = 300 per model, observed and latent, against the 80-bit reference;
 (b) every m edge (the 64-block count against mpad, a live tile with no identity padding, an all-padding tile under a
     live block) returns the BYTES of that call's leading block -- with (a) this pins every edge at the tight bar;
 (c) samples forwards against cov_reference.sample_joint; (d) the Cholesky factor itself backwards: Lc Lc^T against
     the reference's Sigma, and against the library's own, under Higham's bound: no nugget, no argument about conditioning;
 (e) m = S = 4096, the documented limit; (f) the workspace's aliased regions reused after a larger call.

Every case prints its figures before it asserts; the last test writes them where COV_EDGES_JSON names a file
(profiles/cov_parity_edges.json)."""
import json
import os
import time

import numpy as np
import pytest

import cov_edge_cases as ec
import cov_reference as cr
import cov_reference_hp as hp

pytestmark = pytest.mark.gpu

TOL_F32_PATHS = 1e-5     # tests/test_gpu_cov.py's bar, kept where it applies: against evaluate() (f32 on an f32 handle) and
NUGGET = 1e-6            # for latent samples, whose factor is conditioned by this nugget alone (see NUGGET there)
NAMES = list(ec.MODELS)
RECORD = {}
_handles, _base = {}, {}


def _fresh(name):
    import turbo_amd as ta
    return ec.fit_handle(ta.NativeGP(0, ec.MODELS[name]["dtype"]), name)


def _gp(name):
    """the model's handle, fitted once per module"""
    if name not in _handles:
        _handles[name] = _fresh(name)
    return _handles[name]


def _base_call(name, latent):
    """predict_cov of the 300 base rows: made once, shared, never modified"""
    if (name, latent) not in _base:
        mu, cov, neg = _gp(name).predict_cov(ec.data(name)[3], latent)
        mu.setflags(write=False); cov.setflags(write=False)
        _base[(name, latent)] = (mu, cov, neg)
    return _base[(name, latent)]


def _note(name, key, **kw):
    RECORD.setdefault(name, {})[key] = {k: float(v) for k, v in kw.items()}


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("latent", [False, True])
def test_one_large_call_against_the_80_bit_reference(name, latent):
    gp, Xq = _gp(name), ec.data(name)[3]
    mu, cov, neg = _base_call(name, latent)
    r = ec.judge_cov(name, mu, cov, latent)
    e = ec.e_ref(name)
    which = "cov_latent" if latent else "cov_observed"
    print("%s latent=%d: mu %.3g (bar %.3g, e_ref %.3g) cov %.3g (bar %.3g, e_ref %.3g) of the prior scale"
          % (name, latent, r["mu"], r["bar_mu"], e["mu"], r["cov"], r["bar_cov"], e[which]))
    _note(name, which, e_ref=e[which], bar=r["bar_cov"], err=r["cov"], ratio=r["cov"] / r["bar_cov"])
    _note(name, "mu_latent" if latent else "mu_observed", e_ref=e["mu"], bar=r["bar_mu"], err=r["mu"], ratio=r["mu"] / r["bar_mu"])
    assert r["ok"], r
    assert np.array_equal(cov, cov.T)                                     # symmetric bit for bit
    assert neg == int((np.diag(cov) < 0).sum())
    mu2, cov2, _ = gp.predict_cov(Xq, latent)                             # the same bits from run to run
    assert mu2.tobytes() == mu.tobytes() and cov2.tobytes() == cov.tobytes()
    if not latent:                                                        # the diagonal is tgp_predict's sigma^2
        vs, _ = cr.scales(ec.reference(name))
        sg = gp.evaluate(Xq, want_sigma=True)["sigma"]
        assert np.abs(np.maximum(np.diag(cov), 0.0) - sg ** 2).max() <= TOL_F32_PATHS * vs


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("m", ec.M_EDGES)
def test_every_m_edge_returns_the_bytes_of_the_large_call(name, m):
    gp, Xq = _gp(name), ec.data(name)[3]
    for latent in (False, True):
        mu300, cov300, _ = _base_call(name, latent)
        mu, cov, neg = gp.predict_cov(Xq[:m], latent)
        assert cov.tobytes() == np.ascontiguousarray(cov300[:m, :m]).tobytes(), (name, m, latent)
        assert mu.tobytes() == mu300[:m].tobytes(), (name, m, latent)
        assert neg == int((np.diag(cov) < 0).sum())


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.SAMPLE_MODELS)
@pytest.mark.parametrize("m", ec.SAMPLE_MS)
def test_samples_forwards(name, m):
    gp, Xq, model = _gp(name), ec.data(name)[3], ec.reference(name)
    vs, ms = cr.scales(model)
    eps = ec.sample_eps(m)
    r = gp.sample_joint(Xq[:m], 5, eps=eps, latent=False, nugget=0.0)     # observed: the noise conditions the factor
    j = ec.judge_samples(name, m, r["y"])
    emu = float(np.abs(r["mu"].astype(ec.LD) - ec.hp_posterior(name)[0][:m]).max()) / ms
    bmu = ec.bars(name, False)[0]
    print("%s m=%d observed samples: %.3g (bar %.3g, e_ref %.3g) mu %.3g (bar %.3g)" % (name, m, j["err"], j["bar"], j["e_ref"], emu, bmu))
    _note(name, "samples_observed_m%d" % m, e_ref=j["e_ref"], bar=j["bar"], err=j["err"], ratio=j["err"] / j["bar"])
    assert j["ok"], j
    assert emu <= bmu and np.array_equal(r["eps"], eps)
    assert r["mu"].tobytes() == _base_call(name, False)[0][:m].tobytes()
    r = gp.sample_joint(Xq[:m], 5, eps=eps, latent=True, nugget=NUGGET)
    wy, _ = cr.sample_joint(model, Xq[:m], eps, True, NUGGET)
    ey = np.abs(r["y"] - wy).max() / ms
    print("%s m=%d latent samples (nugget %g): %.3g (bar %.3g)" % (name, m, NUGGET, ey, TOL_F32_PATHS))
    _note(name, "samples_latent_m%d" % m, e_ref=0.0, bar=TOL_F32_PATHS, err=ey, ratio=ey / TOL_F32_PATHS)
    assert ey <= TOL_F32_PATHS


# ---- (d) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.SAMPLE_MODELS)
@pytest.mark.parametrize("m", ec.SAMPLE_MS)
def test_the_factor_backwards(name, m):
    gp, Xq = _gp(name), ec.data(name)[3]
    s = gp.sample_joint(Xq[:m], m, eps=np.eye(m), latent=False, nugget=0.0)
    A, a_err = ec.factor_inputs(name, m)
    own = gp.predict_cov(Xq[:m])[1]                                       # the matrix Lc is the factor of
    f = ec.judge_factor(s["y"], s["mu"], ec.reference(name).y_std, A, a_err, ec.A_ERR_FACTOR, own_cov=own)
    print("%s m=%d: |Lc Lc^T - A| is %.3g of its bound (%.3g with the reference's error once; SciPy's factor: %.3g), against its own Sigma %.3g of the textbook bound, zeros above %s, diagonal positive %s"
          % (name, m, f["ratio"], f["ratio_at_factor_1"], f["scipy_ratio"], f["own"], f["zeros"], f["diag"]))
    _note(name, "factor_m%d" % m, residual_over_bound=f["ratio"], residual_over_bound_at_factor_1=f["ratio_at_factor_1"],
          own_sigma_residual_over_textbook_bound=f["own"], scipy_residual_over_bound=f["scipy_ratio"])
    assert f["zeros"] and f["diag"] and f["ratio"] <= 1.0 and f["own"] <= 1.0, f


# ---- (e) the limit, on model D ------------------------------------------------------------------------------------------
_limit = {}


def _limit_reference():
    """f64 reference over all 4096 rows, the 80-bit block on the index set, and the f64 reference's own error there"""
    if "ref" not in _limit:
        Xq = ec.data("D", ec.M_LIMIT)[3]
        model = ec.reference("D")
        mu, cov, _ = cr.predict_cov(model, Xq, False)
        I = ec.limit_index_set()
        hmu, hobs, _ = hp.sigma_block(ec.hp_fit("D"), Xq, I)
        vs, ms = cr.scales(model)
        e_cov = float(np.abs(cov[np.ix_(I, I)].astype(ec.LD) - hobs).max())     # raw units
        e_mu = float(np.abs(mu[I].astype(ec.LD) - hmu).max())
        _limit["ref"] = dict(Xq=Xq, mu=mu, cov=cov, I=I, hmu=hmu, hobs=hobs, e_cov=e_cov, e_mu=e_mu)
    return _limit["ref"]


def _limit_sample():
    """sample_joint(m = S = 4096, eps = I) as the FIRST call of a fresh handle, which (f) then goes on using"""
    if "sample" not in _limit:
        gp = _fresh("D")
        Xq = ec.data("D", ec.M_LIMIT)[3]
        t = time.perf_counter()
        s = gp.sample_joint(Xq, ec.M_LIMIT, eps=np.eye(ec.M_LIMIT), latent=False, nugget=0.0)
        _limit["sample"] = (gp, s, time.perf_counter() - t)
    return _limit["sample"]


def test_the_limit_covariance():
    ref = _limit_reference()
    gp, model = _gp("D"), ec.reference("D")
    vs, ms = cr.scales(model)
    t = time.perf_counter()
    mu, cov, neg = gp.predict_cov(ref["Xq"], False)
    dt = time.perf_counter() - t
    cov.setflags(write=False)
    _limit["cov"] = cov                                                   # (the limit's factor is held to it)
    bmu, bcov = ec.bars("D", False)
    I = ref["I"]
    eb = float(np.abs(cov[np.ix_(I, I)].astype(ec.LD) - ref["hobs"]).max()) / vs
    ebm = float(np.abs(mu[I].astype(ec.LD) - ref["hmu"]).max()) / ms
    # the whole matrix has only the f64 reference: its own error (4 x the largest seen on the 80-bit block) joins the bar
    ef, efm = np.abs(cov - ref["cov"]).max() / vs, np.abs(mu - ref["mu"]).max() / ms
    bf, bfm = bcov + 4 * ref["e_cov"] / vs, bmu + 4 * ref["e_mu"] / ms
    print("D m=4096 (%.2f s with the copies): 80-bit block cov %.3g (bar %.3g) mu %.3g (bar %.3g); whole matrix against f64 cov %.3g (bar %.3g) mu %.3g (bar %.3g)"
          % (dt, eb, bcov, ebm, bmu, ef, bf, efm, bfm))
    _note("D", "limit_cov_block", e_ref=ref["e_cov"] / vs, bar=bcov, err=eb, ratio=eb / bcov)
    _note("D", "limit_mu_block", e_ref=ref["e_mu"] / ms, bar=bmu, err=ebm, ratio=ebm / bmu)
    _note("D", "limit_cov_whole_vs_f64", e_ref=ref["e_cov"] / vs, bar=bf, err=ef, ratio=ef / bf, seconds=dt)
    assert eb <= bcov and ebm <= bmu and ef <= bf and efm <= bfm
    assert np.array_equal(cov, cov.T) and neg == int((np.diag(cov) < 0).sum())
    mu300, cov300, _ = _base_call("D", False)                             # the leading block: the bytes of (a)'s call
    assert np.ascontiguousarray(cov[:300, :300]).tobytes() == cov300.tobytes() and mu[:300].tobytes() == mu300.tobytes()


def test_the_limit_factor():
    ref = _limit_reference()
    model = ec.reference("D")
    gp, s, dt = _limit_sample()
    A = ref["cov"] / model.y_std ** 2
    a_err = 4 * ref["e_cov"] / model.y_std ** 2                           # A's own error: 4 x the largest seen on the 80-bit block
    own = _limit["cov"] if "cov" in _limit else _gp("D").predict_cov(ref["Xq"], False)[1]
    f = ec.judge_factor(s["y"], s["mu"], model.y_std, A, a_err, extended=False, own_cov=own)
    print("D m=S=4096 (%.2f s with the copies): |Lc Lc^T - A| is %.3g of its bound (SciPy's factor: %.3g), against its own Sigma %.3g of the textbook bound, zeros above %s, diagonal positive %s"
          % (dt, f["ratio"], f["scipy_ratio"], f["own"], f["zeros"], f["diag"]))
    _note("D", "factor_m4096", residual_over_bound=f["ratio"], own_sigma_residual_over_textbook_bound=f["own"],
          scipy_residual_over_bound=f["scipy_ratio"], seconds=dt)
    assert f["zeros"] and f["diag"] and f["ratio"] <= 1.0 and f["own"] <= 1.0, f
    assert np.array_equal(s["eps"], np.eye(ec.M_LIMIT))
    assert s["mu"][:300].tobytes() == _base_call("D", False)[0].tobytes()


# ---- (f) ----------------------------------------------------------------------------------------------------------------
def test_the_workspace_after_a_larger_call():
    """one handle makes the m = S = 4096 call and then four smaller ones of every shape the workspace's aliased regions
    take; each result is, byte for byte, what a fresh handle of the same fit returns when it makes only that call"""
    Xq = ec.data("D", ec.M_LIMIT)[3]
    gp, big, _ = _limit_sample()
    eps = np.random.RandomState(7).standard_normal((3, 129))
    calls = [
        ("predict_cov m=1", lambda h: h.predict_cov(Xq[:1])),
        ("sample_joint m=129 S=3", lambda h: h.sample_joint(Xq[:129], 3, eps=eps)),
        ("predict_cov m=300 latent", lambda h: h.predict_cov(Xq[:300], latent=True)),
        ("sample_joint m=65 S=4096 drawn", lambda h: h.sample_joint(Xq[:65], 4096, seed=1, nugget=NUGGET)),
    ]
    flat = lambda r: b"".join(np.ascontiguousarray(v).tobytes() for v in (r.values() if isinstance(r, dict) else r[:2])) + \
        (b"" if isinstance(r, dict) else bytes([r[2] & 0xFF]))
    # (the large call itself: the module's long-used handle grows into it and must return the fresh handle's bytes)
    other = _gp("D").sample_joint(Xq, ec.M_LIMIT, eps=np.eye(ec.M_LIMIT), latent=False, nugget=0.0)
    assert flat(other) == flat(big), "sample_joint m=S=4096"
    del other
    for what, call in calls:
        assert flat(call(gp)) == flat(call(_fresh("D"))), what


def test_record_the_figures():
    """(last in the file) where COV_EDGES_JSON names a file the figures seen above go there: profiles/cov_parity_edges.json"""
    out = os.environ.get("COV_EDGES_JSON")
    if out and RECORD:
        with open(out, "w") as f:
            json.dump(dict(unit="fraction of the prior scale y_std^2 (c + noise) (cov) or its root (mu, samples); factor_*: max |Lc Lc^T - A| over its bound",
                           factor=ec.FACTOR, cap_cov=ec.CAP_COV, cap_value=ec.CAP_VAL, models=RECORD), f, indent=1, sort_keys=True)
    for name, rec in RECORD.items():
        for key, v in rec.items():                           # (model H's bar is the appended fit's 1e-9, not the formula's)
            assert v.get("ratio", 0.0) <= 1.0 and v.get("residual_over_bound", 0.0) <= 1.0, (name, key, v)
            assert v.get("own_sigma_residual_over_textbook_bound", 0.0) <= 1.0, (name, key, v)
            if "bar" in v and not key.startswith("samples_latent") and not key.endswith("whole_vs_f64") and not ec.MODELS[name].get("append"):
                assert v["bar"] <= (ec.CAP_COV if "cov" in key else ec.CAP_VAL), (name, key, v)
