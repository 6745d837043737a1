"""What the fit entries (tgp_fit, tgp_fit_grad, tgp_fit_append, tgp_predict_batch, tgp_sweep_integrated) do around their
kernels, on every path the host code takes -- small and fused, small and unfused, blocked and staged, polled and
event-timed: the refusal of a matrix that is not positive definite (status, exact text, pivot), the handle after a
rejected call, last_timings(), the append's outputs, optional outputs and the integrated sweep's record.

The cases live in _fit_paths_child.py.  csrc/tuning.hpp reads the TGP_* switches once per process, so the default
selection runs here and every other one in a child process: TGP_POLL_US=0 TGP_SMALL_FUSED=0 (event-timed completion,
the small fit and its gradient as two launches) and TGP_SWEEP_ZC=0 (the sweep's record by D2H copies)."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _fit_paths_child as cases      # noqa: E402

NOT_PD_TEXT = "kernel matrix is not positive definite (pivot %d of %d <= 0)"
_child_results = {}


def _child(groups, **env):
    """the groups' results from a child process under `env` (one process per selection of switches, shared by the tests)"""
    key = (tuple(groups), tuple(sorted(env.items())))
    if key not in _child_results:
        e = dict(os.environ)
        e.update(env)
        out = subprocess.run([sys.executable, os.path.join(HERE, "_fit_paths_child.py"), *groups], env=e, capture_output=True,
                             text=True, timeout=300)
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("fit-paths ")]
        assert out.returncode == 0 and lines, out.stdout[-2000:] + out.stderr[-4000:]
        _child_results[key] = json.loads(lines[-1][len("fit-paths "):])
    return _child_results[key]


EVENT_TIMED = dict(TGP_POLL_US="0", TGP_SMALL_FUSED="0")


def _event_timed():
    return _child(("not_pd", "timings"), **EVENT_TIMED)


def _check_not_pd(res):
    from turbo_amd import _lib as L
    print(res)
    for name, pivot, n in (("small", 4, 6), ("blocked", 129, 130), ("append", 6, 7)):
        rc, err, sweep_rc, sweep_err = res[name][:4]
        assert rc == L.NOT_PD and err == NOT_PD_TEXT % (pivot, n), (name, rc, err)
        assert sweep_rc == L.NOT_FITTED and sweep_err == "tgp_sweep: no fitted model", (name, sweep_rc, sweep_err)
    assert res["append"][4] == L.OK and res["append"][5] == 0        # the fit it extends was healthy; nothing was appended
    assert res["predict_batch"] == ["LinAlgError", "model 1 of the batch: " + NOT_PD_TEXT % (4, 6)]


def test_not_positive_definite_on_every_fit_path():
    """status TGP_NOT_PD and the text with the pivot's number from the small fit, the blocked fit (polled), the append
    and tgp_predict_batch; after each, tgp_sweep answers TGP_NOT_FITTED"""
    _check_not_pd(cases.not_pd())


def test_not_positive_definite_event_timed():
    """the same refusals with TGP_POLL_US=0: the blocked fit's event-timed completion"""
    _check_not_pd(_event_timed()["not_pd"])


def test_a_rejected_call_leaves_the_handle_unfitted():
    """tgp_fit clears the fitted flag before it looks at its arguments"""
    import turbo_amd as ta
    L = ta._lib
    gp = ta.NativeGP(0, "f64")
    X, y = cases._problem(8, 3, 1)
    assert cases._call(gp, "fit", X, y, "rbf", 1.0, 0.7, 1e-2, 1e-10)[0] == L.OK
    assert cases._sweep_status(gp) == (L.BAD_ARG, "tgp_sweep: no candidates set")        # (fitted: the next check speaks)
    rc, err = cases._call(gp, "fit", X, y, "rbf", 1.0, np.array([0.7, 0.8]), 1e-2, 1e-10, n_ls=2)[:2]
    assert (rc, err) == (L.BAD_ARG, "tgp_fit: n_ls must be 1 or D")
    assert cases._sweep_status(gp) == (L.NOT_FITTED, "tgp_sweep: no fitted model")
    gp.close()


def _check_timings(res, polled):
    print(res)
    assert sorted(res) == sorted(t + c for t in ("small", "blocked") for c in (" fit", " fit_grad iso", " fit_grad ard", " append"))
    for name, (fit_ms, *stages) in res.items():
        assert math.isfinite(fit_ms) and fit_ms > 0.0, (name, fit_ms)
        if "fit_grad" not in name:
            continue
        if name.startswith("small") or polled:
            assert stages == [0.0, 0.0, 0.0], (name, stages)      # (all of it inside fit_ms)
        else:
            assert all(math.isfinite(s) and s >= 0.0 for s in stages), (name, stages)


def test_fit_time_is_reported_after_every_kind_of_fit():
    """last_timings()["fit_ms"] is finite and > 0 after a small fit, a small fit + gradient (iso, ARD), a blocked fit, a
    blocked fit + gradient and an append; the gradient's stage times are 0 where the call is polled or small"""
    _check_timings(cases.timings(), polled=True)


def test_fit_time_is_reported_event_timed():
    """... and under TGP_POLL_US=0 TGP_SMALL_FUSED=0, where the blocked gradient's stages are timed by events"""
    _check_timings(_event_timed()["timings"], polled=False)


def test_append_returns_what_a_fresh_fit_returns():
    import turbo_amd as ta
    L = ta._lib
    X, y = cases._problem(41, 3, 2)
    th = ("matern52", 1.3, 0.7, 1e-2, 1e-10)
    fresh = ta.NativeGP(0, "f64")
    rc, _, lml, ym, ys, _ = cases._call(fresh, "fit", X, y, *th)
    assert rc == L.OK
    gp = ta.NativeGP(0, "f64")
    assert cases._call(gp, "fit", X[:40], y[:40], *th)[0] == L.OK
    rc, _, a_lml, a_ym, a_ys, appended = cases._call(gp, "append", X, y, *th)
    print("append lml %r, fresh %r" % (a_lml, lml))
    assert rc == L.OK and appended == 1
    assert abs(a_lml - lml) <= 1e-10 * abs(lml)
    assert (a_ym, a_ys) == (ym, ys)
    # another length scale: nothing to extend, the call IS a fresh fit
    th2 = ("matern52", 1.3, 0.8, 1e-2, 1e-10)
    rc, _, lml2, ym2, ys2, _ = cases._call(fresh, "fit", X, y, *th2)
    assert rc == L.OK
    assert cases._call(gp, "fit", X[:40], y[:40], *th)[0] == L.OK
    rc, _, *got = cases._call(gp, "append", X, y, *th2)
    assert rc == L.OK and got == [lml2, ym2, ys2, 0]
    fresh.close()
    gp.close()


@pytest.mark.parametrize("N", [8, 130], ids=["small", "blocked"])
def test_fit_outputs_are_optional(N):
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    X, y = cases._problem(N, 3, 3)
    assert cases._call(gp, "fit", X, y, "rbf", 1.0, 0.7, 1e-2, 1e-10, outputs=False)[0] == ta._lib.OK
    assert cases._sweep_status(gp)[1] == "tgp_sweep: no candidates set"       # fitted
    gp.close()


def test_integrated_sweep_record_with_and_without_zero_copy():
    """tgp_sweep_integrated with a winner buffer attached: best_idx is the arg-max of the returned acq_out, n_clamped
    the samples' clamp counts, the winner record [value, global index, row] -- and all of it, bit for bit, again under
    TGP_SWEEP_ZC=0 (the record by D2H copies)"""
    here = cases.integrated_tail()
    there = _child(("integrated_tail",), TGP_SWEEP_ZC="0")["integrated_tail"]
    print(here["best_idx"], here["n_clamped"], here["clamped_per_sample"])
    for r in (here, there):
        assert r["best_idx"] == r["argmax"]
        assert r["n_clamped"] == r["clamped_per_sample"]
        acq = np.frombuffer(bytes.fromhex(r["acq"]))
        assert float.fromhex(r["best_val"]) == acq[r["best_idx"]]
        assert r["record_only"] == [r["best_val"], r["best_idx"], r["n_clamped"]]
        winner = np.frombuffer(bytes.fromhex(r["winner"]))
        assert winner[0] == acq[r["best_idx"]] and winner[1] == 1000 + r["best_idx"]
        assert winner[2:].tobytes().hex() == r["winner_row"]
    assert here == there
