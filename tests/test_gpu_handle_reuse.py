"""GPU: a handle whose buffers have grown, been released and been reused gives the answers a fresh handle gives
(csrc/dev_mem.hpp's owners behind tgp_internal.hpp's Context).  One handle fits models of every size class in turn and
sweeps batches that grow and shrink again; a fresh handle per (model, batch) is the reference, made once and shared.

Every comparison is bit for bit, because the suite already holds each entry compared here to the same bytes:
  tgp_fit (lml, Linv), tgp_sweep    handle to handle, 'f32h2' included: test_gpu_round6.py::test_a_handle_sweeps_with_a_factor_it_received
  tgp_evaluate, tgp_sweep_topk      against the sweep's own values: test_gpu_round4.py (array_equal on mu / sigma / acq, the top k)
  tgp_sweep_batch                   run to run, idx / val / x / fantasies at N = 600: test_gpu_batch_coverage.py::test_same_inputs_same_outputs
  tgp_ts_draw + tgp_ts_sweep        run to run and handle to handle: test_gpu_thompson.py::test_same_seed_is_bit_identical_and_f32_handle_equals_f64
  tgp_predict_cov                   run to run: test_gpu_cov.py::test_covariance_and_mean

Each test runs under a time limit of its own (the fixture below: no plugin needed)."""
import faulthandler

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()

# one-workgroup fit | one-launch sweep | general path (Np 256 -> 768, Dp 4 -> 8: the whole fit set is allocated anew and
# the resident candidates are dropped) | the first again, in buffers larger than it needs (linv_extent)
MODELS = [(100, 3), (300, 3), (600, 5), (100, 3)]
BATCHES = (300, 5000, 300)      # the workspace grows, then is reused with a smaller leading dimension
KIND, CONST, NOISE, JITTER = "matern52", 1.2, 1e-3, 1e-10


def _model(N, D):
    rng = np.random.RandomState(7 * N + D)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X.sum(1)) + 0.3 * ((X - 0.5) ** 2).sum(1) + 0.02 * rng.normal(size=N)
    return X, y, float(np.sqrt(D / 6.0))


def _batch(M, D):
    return np.random.RandomState(1000 + M + D).uniform(0, 1, (M, D))


def _fit(gp, N, D):
    X, y, ls = _model(N, D)
    return gp.fit(X, y, KIND, CONST, ls, NOISE, JITTER, True)[0], float(y.min())


def _sweeps(gp, M, D, inc):
    """tgp_set_candidates + tgp_sweep, then tgp_evaluate (pinned candidates on the small models): EI, all three outputs"""
    import turbo_amd._lib as L
    Xc = _batch(M, D)
    gp.set_candidates(Xc)
    s = gp.sweep(L.ACQ_EI, -1.0, inc, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    e = gp.evaluate(Xc, L.ACQ_EI, -1.0, inc, 0.01, want_mu=True, want_sigma=True, want_acq=True)
    return s, e


_fresh = {}


def _reference(dtype, N, D, M):
    """what a handle that has done nothing else answers: (lml, Linv, sweep, evaluate)"""
    key = (dtype, N, D, M)
    if key not in _fresh:
        import turbo_amd as ta
        gp = ta.NativeGP(0, dtype)
        lml, inc = _fit(gp, N, D)
        linv = gp.debug_read(ta._lib.BUF_LINV)
        _fresh[key] = (lml, linv) + _sweeps(gp, M, D, inc)
        gp.close()
    return _fresh[key]


def _same(got, want, what):
    for k in ("mu", "sigma", "acq"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)
    assert got["best_idx"] == want["best_idx"] and got["best_idx"] == int(np.argmax(got["acq"])), what
    assert np.float64(got["best_val"]).tobytes() == np.float64(want["best_val"]).tobytes(), what
    assert got["n_clamped"] == want["n_clamped"], what


@pytest.mark.parametrize("dtype", ["f64", "f32h2"])     # 'f32h2': Linv32, the fp16 planes of Linv and their scales as well
def test_models_and_batches_in_turn_on_one_handle(dtype):
    import turbo_amd as ta
    gp = ta.NativeGP(0, dtype)
    for N, D in MODELS:
        lml, inc = _fit(gp, N, D)
        for M in BATCHES:
            want_lml, want_linv, want_s, want_e = _reference(dtype, N, D, M)
            assert lml == want_lml
            s, e = _sweeps(gp, M, D, inc)
            _same(s, want_s, (dtype, N, M, "sweep"))
            _same(e, want_e, (dtype, N, M, "evaluate"))
        assert gp.debug_read(ta._lib.BUF_LINV).tobytes() == want_linv.tobytes(), (dtype, N)
    gp.close()


def _other_entries(gp, inc):
    """one call of each entry that keeps a workspace of its own, on the resident model and candidates"""
    import turbo_amd._lib as L
    out = {}
    out["topk_idx"], out["topk_val"] = gp.sweep_topk(4, L.ACQ_EI, -1.0, inc, 0.01)
    b = gp.sweep_batch(2, L.BATCH_KB, 0.0, None, L.ACQ_EI, -1.0, inc, 0.01)
    out.update(batch_idx=b["idx"], batch_val=b["val"], batch_x=b["x"], batch_fant=b["fantasies"])
    gp.ts_draw(11, 4, 64)
    t = gp.ts_sweep(-1.0, True, want_f=True)
    out.update(ts_idx=t["idx"], ts_val=t["val"], ts_x=t["x"], ts_f=t["f"])
    mu, cov, neg = gp.predict_cov(_batch(5, gp.D))
    out.update(cov_mu=mu, cov=cov, cov_neg=np.int64(neg))
    return out


def test_the_other_workspaces_on_a_reused_handle():
    """tgp_sweep_topk (k = 4), tgp_sweep_batch (q = 2), tgp_ts_draw (S = 4, F = 64) + tgp_ts_sweep and tgp_predict_cov
    (m = 5) at N = 600 on an f64 handle that has fitted two smaller models and swept three batches before"""
    import turbo_amd as ta
    N, D, M = 600, 5, 5000
    reused = ta.NativeGP(0, "f64")
    for n, d in MODELS[:2]:
        _, inc = _fit(reused, n, d)
        _sweeps(reused, 300, d, inc)
    _, inc = _fit(reused, N, D)
    for m in BATCHES:
        _sweeps(reused, m, D, inc)
    fresh = ta.NativeGP(0, "f64")
    _fit(fresh, N, D)
    for gp in (reused, fresh):
        gp.set_candidates(_batch(M, D))
    got, want = _other_entries(reused, inc), _other_entries(fresh, inc)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    assert got["topk_idx"][0] == _reference("f64", N, D, M)[2]["best_idx"]
    reused.close()
    fresh.close()


def test_ten_handles_created_and_destroyed_then_one_more():
    """the destructor path and the shared streams' reference count: ten handles, a small fit and sweep in each, then one
    more that still answers as the first did"""
    import turbo_amd as ta
    N, D, M = 100, 3, 300
    first = None
    for i in range(11):
        gp = ta.NativeGP(0, "f64")
        lml, inc = _fit(gp, N, D)
        s, _ = _sweeps(gp, M, D, inc)
        if first is None:
            first = (lml, s)
        gp.close()
    assert lml == first[0]
    _same(s, first[1], "the eleventh handle")
    _same(s, _reference("f64", N, D, M)[2], "a fresh handle")
