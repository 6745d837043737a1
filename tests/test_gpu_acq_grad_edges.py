"""GPU: tgp_acq_grad (csrc/query_kernels.hip, small_query_kernel of csrc/refine_kernels.hip, csrc/query_math.hpp) held to
an 80-bit closed form (tests/acq_grad_reference_hp.py) at the edges its kernels are made of.  Models, batches, bars and the
comparison: tests/acq_grad_edge_cases.py (bars of 64 max(e_ref, N u) of the batch maximum under a cap of 1e-9 -- five to
seven orders under the 2e-4 against central differences that held the gradient before; tests/test_acq_grad_reference.py
shows on the CPU that they reject f32 query points, ls[0] for every dimension, a training point left out, an f32 inverse
factor, the latent variance, PI's cs without its Z and a flipped dvar).

 (a) every model, the 48-row base batch, every acquisition and sf, value and gradient, against the 80-bit reference:
     small_query_kernel (A, S1, S2, S3; Np = 64 and 128, D = 63 / 64) and the general kernels q_kvec, q_rows_mfma /
     q_cols_mfma in their 4-, 8- and 16-wave classes and q_reduce with its last workgroup's finalisation (the others);
 (b) calls of m around the groups of sixteen points return the BYTES of that call's leading rows (general path);
 (c) m = 255, 256, 257: the second pass of the last workgroup's finalisation loop;
 (d) m = 4096 with D = 33: more than the pinned staging holds, so q_finalize_kernel and the copies run;
 (e) the kernels behind TGP_QUERY_MFMA=0, TGP_SMALL_QUERY=0 and TGP_POLL_US=0, one fresh child process each;
 (f) one handle through three fits of different sizes: the query workspace grows and is reused;
 (g) at the variance clamp nothing is NaN and a zero sigma has a zero gradient.

Every case prints its figures before it asserts; the last test writes them where ACQ_GRAD_JSON names a file
(profiles/acq_grad_parity.json)."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import acq_grad_edge_cases as ac
import cov_edge_cases as ec

pytestmark = pytest.mark.gpu

RECORD = {}
_handles, _base = {}, {}


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _fresh(name):
    import turbo_amd as ta
    return ec.fit_handle(ta.NativeGP(0, ac.MODELS[name]["dtype"]), name)


def _gp(name):
    """the model's handle, fitted once per module"""
    if name not in _handles:
        _handles[name] = _fresh(name)
    return _handles[name]


def _base_call(name):
    """every quantity at the 48 base rows, the first queries of the model's handle: made once, shared, never modified"""
    if name not in _base:
        res = ac.query_all(_gp(name), name, ac.points(name))
        for v, g in res.values():
            v.setflags(write=False); g.setflags(write=False)
        _base[name] = res
    return _base[name]


def _note(name, what, j):
    for key, r in j.items():
        if key != "ok":
            RECORD.setdefault(name, {}).setdefault(what, {})[key] = {k: float(v) for k, v in r.items() if k != "ok"}


def _judge(name, batch, what, results):
    j = ac.judge(name, batch, results)
    ac.show(name, what, j)
    _note(name, what, j)
    return j


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.NAMES)
def test_the_base_call_against_the_80_bit_reference(name):
    """(model F is an f32 handle: the query path is all f64 -- d_Linv, d_Xs and d_alpha are the f64 fit -- so it is held
    to the f64 bar like the others)"""
    res = _base_call(name)
    j = _judge(name, "base", "base", res)
    assert j["ok"], j
    again = ac.query_all(_gp(name), name, ac.points(name))                # the same bits from run to run
    assert ac.flat_bytes(again) == ac.flat_bytes(res)
    assert all(np.all(np.isfinite(v)) and np.all(np.isfinite(g)) for v, g in res.values())


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["D", "I"])
@pytest.mark.parametrize("m", ac.M_EDGES)
def test_every_m_edge_returns_the_bytes_of_the_base_call(name, m):
    base = _base_call(name)
    got = ac.query_all(_gp(name), name, ac.points(name)[:m])
    for key in ac.KEYS:
        assert ac.flat_bytes({key: got[key]}) == ac.flat_bytes(ac.leading({key: base[key]}, m)), (name, m, key)


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", ac.M_FINAL)
def test_the_second_pass_of_the_finalisation(m):
    """q_reduce_kernel's last workgroup takes 256 points per pass: point 256 is the first of the second"""
    base = _base_call("D")
    batch = "tail%d" % m
    mm, I = ac.rows(batch)
    assert mm == m and I[-1] == m - 1
    got = ac.query_all(_gp("D"), "D", ec.data("D")[3][:m])
    j = _judge("D", batch, "m=%d" % m, {key: (v[I], g[I]) for key, (v, g) in got.items()})
    assert j["ok"], j
    assert ac.flat_bytes(ac.leading(got, ac.M_BASE)) == ac.flat_bytes(base)


# ---- (d) ----------------------------------------------------------------------------------------------------------------
def test_the_copying_path_at_the_limit():
    """m D 8 bytes = 4096 x 33 x 8 is above the 1 MiB of pinned staging: H2D copy, q_finalize_kernel, D2H copies.  No bytes
    are compared with the base call: the finalisation is another kernel's."""
    m, I = ac.rows("limit")
    assert m * ac.MODELS["F"]["D"] * 8 > (1 << 20) and I[0] == 0 and I[-1] == m - 1
    got = ac.query_all(_gp("F"), "F", ec.data("F", m)[3])
    assert all(v.shape == (m,) and g.shape == (m, 33) and np.all(np.isfinite(v)) and np.all(np.isfinite(g)) for v, g in got.values())
    j = _judge("F", "limit", "m=%d" % m, {key: (v[I], g[I]) for key, (v, g) in got.items()})
    assert j["ok"], j


# ---- (e) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,cases", [
    ({"TGP_QUERY_MFMA": "0"}, ["D:8", "D:9", "I:8", "I:9"]),      # the wave-per-row / split-column kernels, both QROWS_QB classes
    ({"TGP_SMALL_QUERY": "0"}, ["A:48", "S2:48", "S3:48"]),       # the general kernels at N <= 128
    ({"TGP_POLL_US": "0"}, ["A:48", "D:48"]),                     # no doorbell: copies and q_finalize_kernel (D), the stream synchronised
], ids=["query_mfma_0", "small_query_0", "poll_us_0"])
def test_the_alternate_paths(env, cases):
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_acq_grad_child.py")] + cases,
                         env=e, capture_output=True, text=True, timeout=300)
    lines = [l for l in out.stdout.splitlines() if l.startswith("acq-grad-child ")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(lines[0][len("acq-grad-child "):])
    assert sorted(res) == sorted(cases)
    what = ",".join("%s=%s" % kv for kv in env.items())
    for case in cases:
        name, m = case.split(":")
        ac.show(name, "%s m=%s" % (what, m), res[case])
        _note(name, "%s m=%s" % (what, m), res[case])
    for case in cases:
        j = res[case]
        assert j["ok"] and all(j[k]["err_value"] <= j[k]["bar_value"] and j[k]["err_grad"] <= j[k]["bar_grad"] for k in ac.KEYS), (case, j)
        assert all(j[k]["bar_value"] <= ac.CAP and j[k]["bar_grad"] <= ac.CAP for k in ac.KEYS)


# ---- (f) ----------------------------------------------------------------------------------------------------------------
def test_one_handle_in_turn():
    """one handle fits S2 (one launch, no workspace), G (the largest workspace), then S3 and queries each: every result is,
    byte for byte, what the model's own handle returned"""
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    for name in ("S2", "G", "S3"):
        ec.fit_handle(gp, name)
        assert ac.flat_bytes(ac.query_all(gp, name, ac.points(name))) == ac.flat_bytes(_base_call(name)), name


# ---- (g) ----------------------------------------------------------------------------------------------------------------
# model A as it stands but for its noise: there var = c - v.v at a training point is the jitter (1e-10) to rounding, so
# sigma is small and positive -- the first half of the property.  Without the jitter too, on the two Matern-1/2 models (their
# K is well enough conditioned to be factored as it is), var at a training point is rounding noise around an exact 0 and
# the clamp decides: C on the general kernels, S3 in small_query_kernel.
@pytest.mark.parametrize("name,jitter", [("A", ec.JITTER), ("C", 0.0), ("S3", 0.0)])
def test_a_zero_sigma_has_a_zero_gradient(name, jitter):
    """no tolerance: the model refitted without noise, queried at 16 of its own training points.  Everything is finite;
    wherever sigma is exactly 0 its gradient row is exactly 0 (q_finalize_point, SmallEval::finish) and PI / EI are 0 with
    a zero gradient (acq_coef)."""
    import turbo_amd as ta
    X, y, ls, _ = ec.data(name)
    gp = ta.NativeGP(0, "f64")
    gp.fit(X, y, ac.MODELS[name]["kind"], ec.C, ls, 0.0, jitter, True)
    res = ac.query_all(gp, name, X[:16])
    sv, sg = res["sigma"]
    zero = sv == 0.0
    print("%s without noise (jitter %g) at 16 training points: sigma is exactly 0 at %d of them, at most %.3g elsewhere"
          % (name, jitter, int(zero.sum()), sv[~zero].max() if (~zero).any() else 0.0))
    RECORD.setdefault(name, {})["noise=0 jitter=%g at training points" % jitter] = dict(zero_sigma=float(zero.sum()), points=16.0)
    for key, (v, g) in res.items():
        assert np.all(np.isfinite(v)) and np.all(np.isfinite(g)), key
    assert np.all(sv >= 0.0) and np.all(sg[zero] == 0.0)
    for key in ("pi_min", "pi_max", "ei_min", "ei_max"):
        v, g = res[key]
        assert np.all(v[zero] == 0.0) and np.all(g[zero] == 0.0), key
    for key in ("ucb_min", "ucb_max"):                                    # sf mu + beta 0: mu's own gradient, to the bit
        sf = ac.CASES[key][2]
        assert np.array_equal(res[key][1][zero], sf * res["mu"][1][zero]), key
    if jitter == 0.0:
        assert zero.any() and not zero.all(), "the clamp was not reached: this case judges nothing"


def test_record_the_figures():
    """(last in the file) where ACQ_GRAD_JSON names a file the figures seen above go there: profiles/acq_grad_parity.json"""
    out = os.environ.get("ACQ_GRAD_JSON")
    if out and RECORD:
        with open(out, "w") as f:
            json.dump(dict(unit="fraction of the batch's 80-bit maximum of the quantity's magnitude (the value of mu: of the prior scale y_std sqrt(c + noise)); model G's pi_* / ei_*: against the 80-bit acquisition at the returned posterior",
                           factor=ac.FACTOR, cap=ac.CAP, append_bar=ac.APPEND_BAR, models=RECORD), f, indent=1, sort_keys=True)
    for name, rec in RECORD.items():
        for what, keys in rec.items():
            for key, v in keys.items():
                if isinstance(v, dict):
                    assert v["ratio_value"] <= 1.0 and v["ratio_grad"] <= 1.0, (name, what, key, v)
                    assert max(v["bar_value"], v["bar_grad"]) <= (ac.APPEND_BAR if ac.MODELS[name].get("append") else ac.CAP), (name, what, key, v)
