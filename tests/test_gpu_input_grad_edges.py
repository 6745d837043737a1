"""GPU: tgp_fit_input_grad's d LML / d X (input_grad_kernel and input_grad_sum_kernel of csrc/warp_kernels.hip behind the
blocked fit's LML gradient) held to an 80-bit closed form (tests/input_grad_reference_hp.py) at its tile, pass and size
edges.  Cases, bars and the comparison: tests/input_grad_edge_cases.py -- every ENTRY within min(64 max(e_ref, N u), 1e-9) of
its scale, e_ref read from tests/golden/input_grad_eref.json; tests/test_input_grad_reference.py shows on the CPU that these
bars reject a dropped column side, tiles counted once, a row, a tile's remainder or the dimensions from 16 on left out,
ls[0] for every dimension, an f32 inverse factor and a flipped sign.

 (a) every case, isotropic and ARD: every entry against the 80-bit reference; N = 1 gives exact zeros; everything finite;
     both identities (sum over the rows 0, first moment = -d LML / d log l) to the same bars; the same bytes on a second
     call and again after an unrelated fit on the handle; dX = NULL is the same lml and grad;
 (b) lml and grad are tgp_fit_grad's bytes under TGP_SMALL=0, taken in a child process (tests/_lml_grad_child.py);
 (c) a host handle answers TGP_BAD_ARG.

Every case prints its figures before it asserts."""
import faulthandler
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import input_grad_edge_cases as ic
import lml_grad_edge_cases as lc

pytestmark = pytest.mark.gpu

_results = {}


@pytest.fixture(autouse=True)
def _time_limit():
    """a hung GPU call never returns to the interpreter: after 120 s the watchdog thread dumps the stacks and ends the run"""
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _call(gp, case):
    lml, grad, dX = gp.fit_input_grad(*lc.call_args(case))
    return float(lml), np.array(grad, copy=True), np.array(dX, copy=True)


def _result(case):
    """(lml, grad, dX, handle) on a fresh handle of the model's dtype: made once, shared, never modified"""
    if case not in _results:
        import turbo_amd as ta
        gp = ta.NativeGP(0, lc.config(case)["dtype"])
        _results[case] = _call(gp, case) + (gp,)
    return _results[case]


@pytest.mark.parametrize("case", ic.CASES)
def test_every_entry_against_the_80_bit_reference(case):
    lml, grad, dX, gp = _result(case)
    n = lc.config(case)["N"]
    e_ref = ic.e_ref_recorded(case)
    bar = ic.bar(case, e_ref)
    err = ic.error(case, dX)
    zero, moment = ic.identities(case, dX, grad)
    bar_id = max(bar, lc.bars(case)["length_scale"])
    print("%s: worst entry %.3g of its scale (bar %.3g, e_ref %.3g); sum over the rows %.3g, first moment %.3g (bar %.3g)" % (case, err, bar, e_ref, zero, moment, bar_id))
    assert np.all(np.isfinite(dX)) and dX.shape == (n, lc.config(case)["D"])
    if n == 1:
        assert dX.tobytes() == np.zeros_like(dX).tobytes()       # +0.0, not -0.0
    assert err <= bar, (case, err, bar)
    assert zero <= bar and moment <= bar_id, (case, zero, moment, bar, bar_id)
    assert lc.judge(case, lml, grad)["ok"]                       # (the hyper-parameter entries are tgp_fit_grad's own)


@pytest.mark.parametrize("case", ["S3/ard", "B/iso", "T193/ard", "T193-dup/iso", "F/ard"])
def test_the_same_bytes_again_and_after_an_unrelated_fit(case):
    lml, grad, dX, gp = _result(case)
    want = lc.result_bytes(lml, grad) + dX.tobytes()
    l2, g2, d2 = _call(gp, case)
    assert lc.result_bytes(l2, g2) + d2.tobytes() == want
    other = "W/ard" if case != "W/ard" else "B/iso"
    _call(gp, other)                                             # another N, D and kernel: the workspaces hold its leavings
    l3, g3, d3 = _call(gp, case)
    assert lc.result_bytes(l3, g3) + d3.tobytes() == want
    l4, g4, none = gp.fit_input_grad(*lc.call_args(case), want_dX=False)
    assert none is None and lc.result_bytes(float(l4), g4) == lc.result_bytes(lml, grad)


def test_lml_and_grad_are_fit_grads_bytes_on_the_blocked_route():
    """tgp_fit_grad under TGP_SMALL=0 in a child process (the switch is read once per process)"""
    env = dict(os.environ, TGP_SMALL="0")
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_lml_grad_child.py")
    out = subprocess.run([sys.executable, child] + ic.CASES, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("lml-grad-child ")][-1]
    theirs = json.loads(line[len("lml-grad-child "):])
    for case in ic.CASES:
        lml, grad, _, _ = _result(case)
        mine = [float(v).hex() for v in [lml] + list(grad)]
        assert mine == theirs[case], case


def test_a_host_handle_refuses():
    import turbo_amd as ta
    gp = ta.NativeGP(ta._lib.DEVICE_HOST)
    with pytest.raises(ValueError):
        gp.fit_input_grad(*lc.call_args("B/iso"))
