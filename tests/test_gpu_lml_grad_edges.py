"""GPU: tgp_fit_grad's log marginal likelihood and its gradient (small_fit_grad_kernel / small_grad_body of
csrc/small_grad.hpp; launch_lml_grad, lml_weights_kernel and sum_partials_kernel of csrc/grad_kernels.hip;
lml_grad_from_sums of csrc/tgp_api.hip) held to an 80-bit closed form (tests/lml_grad_reference_hp.py) at the size and path
edges its three implementations are made of.  Models, bars and the comparison: tests/lml_grad_edge_cases.py (bars of
64 max(e_ref, N u) of each entry's SCALE, the sum of its absolute terms, under a cap of 1e-9;
tests/test_lml_grad_reference.py shows on the CPU that they reject a tile counted once, a row, a tile's remainder or the
dimensions from 16 on left out, an f32 inverse factor, ls[0] for every dimension and the jitter in the noise entry).

 (a) every case, isotropic and ARD: the LML and every entry of the gradient against the 80-bit reference; the same bytes
     on a second call; everything finite; a noise entry of exactly 0.0 without noise;
 (b) the two sum paths against each other: ARD with every length scale equal sums to the isotropic entry, and the LML, the
     constant's and the noise entry are the isotropic call's bytes;
 (c) the other templates, one fresh child process per setting (tests/_lml_grad_child.py): TGP_KINV64=0 (the 128-tile
     K^-1 product at Np = 256, 512, 1280), TGP_SMALL=0 (the small models down the blocked path), TGP_SMALL_FUSED=0 (two
     launches) and TGP_POLL_US=0 (event-timed stages) -- the last two also the default's bytes;
 (d) N = 4097, where the default takes the 128-tile product: against the f64 oracle, and against the 64-tile product
     (TGP_KINV64=8192) to the oracle's e_ref class;
 (e) one handle through six shapes: the gradient workspace grows along either axis and holds a larger fit's leavings;
 (f) fit_grad behind an appended fit refits in full.

Every case prints its figures before it asserts; the last test writes them where LML_GRAD_JSON names a file
(profiles/lml_grad_parity.json)."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cov_edge_cases as ec
import lml_grad_edge_cases as lc
import lml_grad_reference_hp as lr
from oracle import gp_oracle as G

pytestmark = pytest.mark.gpu

RECORD = {}
_base = {}


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _handle(case, dtype=None):
    import turbo_amd as ta
    return ta.NativeGP(0, dtype or lc.config(case)["dtype"])


def _base_call(case):
    """(lml, grad, handle) of the default path on a fresh handle of the model's dtype: made once, shared, never modified"""
    if case not in _base:
        gp = _handle(case)
        lml, grad = lc.fit_grad(gp, case)
        grad.setflags(write=False)
        _base[case] = (lml, grad, gp)
    return _base[case]


def _judge(case, what, lml, grad):
    j = lc.judge(case, lml, grad)
    lc.show(case, what, j)
    RECORD.setdefault(case, {})[what] = {k: {f: float(v) for f, v in j[k].items() if f != "ok"} for k in lc.KEYS}
    return j


def _child(env, cases):
    """{case: (lml, grad)} of tests/_lml_grad_child.py under env"""
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lml_grad_child.py")] + list(cases),
                         env=e, capture_output=True, text=True, timeout=110)
    lines = [l for l in out.stdout.splitlines() if l.startswith("lml-grad-child ")]
    assert out.returncode == 0 and len(lines) == 1, out.stdout[-2000:] + out.stderr[-4000:]
    res = json.loads(lines[0][len("lml-grad-child "):])
    assert sorted(res) == sorted(cases)
    return {c: (float.fromhex(v[0]), np.array([float.fromhex(x) for x in v[1:]])) for c, v in res.items()}


# ---- (a) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", lc.CASES)
def test_the_base_call_against_the_80_bit_reference(case):
    """(model F is an f32 handle: the factor under the gradient is the f64 fit whatever the dtype, so it is held to the f64
    bar like the others)"""
    lml, grad, gp = _base_call(case)
    j = _judge(case, "base", lml, grad)
    again = lc.fit_grad(gp, case)
    assert grad.shape == (2 + (lc.config(case)["D"] if lc.config(case)["ard"] else 1),)
    assert np.isfinite(lml) and np.all(np.isfinite(grad))
    assert j["ok"], j
    assert lc.result_bytes(*again) == lc.result_bytes(lml, grad)          # the same bits from run to run
    if lc.call_args(case)[5] == 0.0:
        assert grad[-1] == 0.0 and not np.signbit(grad[-1])


# ---- (b) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in lc.CASES if not lc.config(c)["ard"] and lc.config(c)["D"] > 1])
def test_equal_ard_length_scales_sum_to_the_isotropic_entry(case):
    """d2 = sum_d (xs_d - xs'_d)^2, so the D ARD entries of a model whose length scales are all equal add up to its
    isotropic entry: the per-dimension passes against the one sum over d2, as a fraction of the isotropic entry's scale.
    Everything else in the two calls is the same arithmetic on the same numbers."""
    lml, grad, _ = _base_call(case)
    alml, agrad = lc.fit_grad(_handle(case), case, lc.equal_ard_args(case))
    ref = lc.hp_reference(case)
    total = np.sum(agrad[1:-1].astype(lc.LD))
    err = float(abs(total - lc.LD(grad[1])) / ref["grad_scale"][1])
    bar = lc.bars(case)["length_scale"]
    err_ref = float(abs(total - ref["grad"][1]) / ref["grad_scale"][1])
    print("%s equal ARD length scales: sum of the entries %.3g from the isotropic entry, %.3g from the 80-bit one (bar %.3g)" % (case, err, err_ref, bar))
    RECORD.setdefault(case, {})["equal ARD sum"] = dict(err=err, err_to_reference=err_ref, bar=bar, ratio=err / bar)
    assert agrad.shape == (2 + lc.config(case)["D"],) and np.all(np.isfinite(agrad))
    assert err <= bar and err_ref <= bar
    assert lc.result_bytes(alml, agrad[[0, -1]]) == lc.result_bytes(lml, grad[[0, -1]])


# ---- (c) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,cases,same_bytes", [
    ({"TGP_KINV64": "0"}, lc.BLOCKED, False),                       # g.on128<KN_UPPER_A, TM_LOWER>: Np = 256, 512 and 1280
    ({"TGP_SMALL": "0"}, lc.SMALL, False),                          # N <= 128 through launch_lml_grad
    ({"TGP_SMALL_FUSED": "0"}, lc.SMALL, True),                     # small fit, then small_grad_kernel
    ({"TGP_POLL_US": "0"}, ["S3/ard", "T193/ard"], True),           # no doorbell: the stages between event records
], ids=["kinv64_0", "small_0", "small_fused_0", "poll_us_0"])
def test_the_other_templates(env, cases, same_bytes):
    what = ",".join("%s=%s" % kv for kv in env.items())
    res = _child(env, cases)
    if "TGP_KINV64" in env:
        assert {lc.padded(c) for c in cases} == {256, 512, 1280}
    judged = {c: _judge(c, what, *res[c]) for c in cases}
    for c in cases:
        assert np.all(np.isfinite(res[c][1])) and judged[c]["ok"], (c, judged[c])
    if same_bytes:
        for c in cases:
            assert lc.result_bytes(*res[c]) == lc.result_bytes(*_base_call(c)[:2]), (what, c, res[c], _base_call(c)[:2])


# ---- (d) ----------------------------------------------------------------------------------------------------------------
def test_the_native_switch_over():
    """N = 4097, D = 2, isotropic RBF: Np = 4352 is the first size above TGP_KINV64 = 4096, so the default forms K^-1 on
    128 x 128 tiles; the child with TGP_KINV64=8192 forms it on 64 x 64 tiles.  No 80-bit reference at this size:
      - either run against oracle.gp_oracle.lml_and_grad at the relative tolerances of test_gpu_parity.py's
        test_lml_gradient_larger_vs_oracle (LML 1e-9; gradient 1e-6 of each entry, without that test's absolute term:
        measured 1.6e-9 at most, on the constant's entry, whose terms cancel to 1e-10 of their sum);
      - the two runs against each other, as fractions of the f64 scales, under the bar the cases with an 80-bit
        reference get: 64 max(e_ref, N u), e_ref the oracle's largest measured error over the blocked isotropic RBF
        cases (lml_grad_edge_cases.SWITCH_CLASS).  The differences and the margin the bar leaves over the larger of them
        are recorded; no figure of this case's own made the bar.  (Measured on an MI355X: the two products return the
        same bits -- either sums over k in the same order -- so the recorded margin is null.)"""
    case = lc.SWITCH
    args = lc.call_args(case)
    N = lc.config(case)["N"]
    assert lc.padded(case) == 4352 and N == 4097
    runs = {"default (128-tile)": lc.fit_grad(_handle(case), case), "TGP_KINV64=8192 (64-tile)": _child({"TGP_KINV64": "8192"}, [case])[case]}
    olml, ograd = G.lml_and_grad(*args)
    _, _, lml_scale, grad_scale = lr.lml_and_grad_f64(*args, with_scale=True)
    scale = np.concatenate([[lml_scale], grad_scale])
    flat = {k: np.concatenate([[v[0]], v[1]]) for k, v in runs.items()}
    oflat = np.concatenate([[olml], ograd])
    rec = RECORD.setdefault(case, {})
    for k, v in flat.items():
        d = np.abs(v - oflat)
        rec[k + " against the f64 oracle"] = dict(zip(lc.KEYS, (d / scale).tolist()))
        print("%s %s against the f64 oracle: relative %s; of the scale %s" % (case, k, d / np.abs(oflat), d / scale))
    a, b = flat.values()
    diff = np.abs(a - b) / scale
    cls = {k: max(lc.e_ref(c)[k] for c in lc.SWITCH_CLASS) for k in lc.KEYS}
    bar = {k: ec._bar(cls[k], N, lc.CAP) for k in lc.KEYS}
    rec["128-tile against 64-tile"] = {k: dict(diff=float(diff[i]), e_ref_class=cls[k], bar=bar[k]) for i, k in enumerate(lc.KEYS)}
    worst = max(range(len(lc.KEYS)), key=lambda i: diff[i] / bar[lc.KEYS[i]])
    rec["margin of the bar over the larger difference"] = float(bar[lc.KEYS[worst]] / diff[worst]) if diff[worst] > 0 else None   # (None: the same bits)
    print("%s 128-tile against 64-tile, of the scale: %s; bars %s" % (case, dict(zip(lc.KEYS, diff.tolist())), bar))
    for k, (lml, grad) in runs.items():
        assert np.all(np.isfinite(grad)), k
        assert lml == pytest.approx(olml, rel=1e-9), k
        np.testing.assert_allclose(grad, ograd, rtol=1e-6, atol=0, err_msg=k)
    for i, k in enumerate(lc.KEYS):
        assert diff[i] <= bar[k], (k, diff[i], bar[k])


# ---- (e) ----------------------------------------------------------------------------------------------------------------
def test_one_handle_many_shapes():
    """1100 x 6 isotropic, 129 x 3 ARD, 384 x 33 ARD, 300 x 17 isotropic, 128 x 61 ARD, 257 x 3 ARD on ONE f64 handle:
    ensure_grad_workspace grows along Dp after it grew along Np, the small path runs between blocked ones, and W and
    d_gpart hold what the larger fit left.  Every result is a fresh f64 handle's, byte for byte."""
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    for case in ("G/iso", "B/ard", "F/ard", "E/iso", "S5/ard", "D/ard"):
        got = lc.fit_grad(gp, case)
        fresh = _base_call(case)[:2] if lc.config(case)["dtype"] == "f64" else lc.fit_grad(_handle(case, "f64"), case)
        print("%s on the travelled handle: lml %r grad[:3] %r" % (case, got[0], got[1][:3]))
        assert lc.result_bytes(*got) == lc.result_bytes(*fresh), (case, got, fresh)


# ---- (f) ----------------------------------------------------------------------------------------------------------------
def test_fit_grad_after_an_append():
    """tests/cov_edge_cases.py's model H: 299 rows, the one-row extension to 300, then fit_grad of the 300 on that handle.
    The gradient path refits in full, so the bytes are a fresh handle's."""
    import turbo_amd as ta
    X, y, ls, _ = ec.data("H")
    kind = ec.MODELS["H"]["kind"]
    gp = ec.fit_handle(ta.NativeGP(0, "f64"), "H")
    assert gp.appended
    got = gp.fit_grad(X, y, kind, ec.C, ls, ec.NOISE, ec.JITTER, True)
    fresh = ta.NativeGP(0, "f64").fit_grad(X, y, kind, ec.C, ls, ec.NOISE, ec.JITTER, True)
    print("H after the append: lml %r grad %r" % (got[0], got[1]))
    assert np.all(np.isfinite(got[1])) and lc.result_bytes(*got) == lc.result_bytes(*fresh)
    olml, ograd = G.lml_and_grad(X, y, kind, ec.C, ls, ec.NOISE, ec.JITTER, True)
    assert got[0] == pytest.approx(olml, rel=1e-9)
    np.testing.assert_allclose(got[1], ograd, rtol=1e-6, atol=1e-6)


def test_record_the_figures():
    """(last in the file) where LML_GRAD_JSON names a file the figures seen above go there: profiles/lml_grad_parity.json"""
    out = os.environ.get("LML_GRAD_JSON")
    if out and RECORD:
        with open(out, "w") as f:
            json.dump(dict(unit="fraction of the quantity's scale: the sum of the absolute terms of the entry (tests/lml_grad_reference_hp.py); length_scale: the worst entry",
                           factor=lc.FACTOR, cap=lc.CAP, cases=RECORD), f, indent=1, sort_keys=True)
    for case, rec in RECORD.items():
        for what, keys in rec.items():
            if case == lc.SWITCH or not isinstance(keys, dict) or "lml" not in keys:
                continue
            for k, v in keys.items():
                assert v["ratio"] <= 1.0 and v["bar"] <= lc.CAP, (case, what, k, v)
