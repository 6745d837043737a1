"""CPU: the host backend's max-value entropy search (csrc/host_backend.cpp: its own mes_h over its own erfcx_pos) held, row
by row, to the 80-bit reference at the bars of tests/mes_edge_cases.py -- the judgement tests/test_gpu_mes_edges.py
applies to the kernels.  A TGP_DEVICE_HOST handle at N = 40; the maxima are placed so that a marked candidate's gamma_s
cover every class, then so that they walk across erfcx_pos's switch at z = 3 (|gamma| = 3 sqrt 2 = 4.2426...) in steps
of a few ulps, on both sides of 0."""
import numpy as np
import pytest

import mes_edge_cases as me

N, M = me.PATHS["one-workgroup"]
SWITCH = 3.0 * np.sqrt(2.0)


@pytest.fixture(scope="module")
def host():
    from turbo_amd import _lib
    X, y, ls, Xc = me.library_problem(N, M)
    gp = _lib.NativeGP(_lib.DEVICE_HOST, "f64")
    _, _, y_std = gp.fit(X, y, "matern52", 1.0, ls, me.NOISE_LIB, 1e-10, True)
    gp.set_candidates(Xc)
    post = gp.sweep(_lib.ACQ_NONE, want_mu=True, want_sigma=True)
    nv = me.NOISE_LIB * y_std * y_std
    assert me.well_conditioned(post["sigma"], nv)
    return _lib, gp, Xc, post["mu"].copy(), post["sigma"].copy(), nv


def _check(host, ys, sf, what):
    _lib, gp, Xc, mu, sigma, nv = host
    gp.mes_set_maxima(ys)
    r = gp.sweep(_lib.ACQ_MES, sf, want_mu=True, want_sigma=True, want_acq=True)
    assert r["mu"].tobytes() == mu.tobytes() and r["sigma"].tobytes() == sigma.tobytes()
    j = me.judge(mu, sigma, ys, sf, nv, a=r["acq"])
    print("host %s sf=%+d: worst %.3g of its bar; by class %s; tiny %d" % (what, sf, j["worst"]["a"], {k: "%.2g" % v for k, v in j["by_class"]["a"].items()}, j["tiny"]))
    assert j["ok"], j["bad"]
    e = gp.evaluate(Xc, _lib.ACQ_MES, sf, want_acq=True)
    assert e["acq"].tobytes() == r["acq"].tobytes() and e["best_idx"] == r["best_idx"] == int(np.argmax(r["acq"]))
    return j


@pytest.mark.parametrize("sf", [1.0, -1.0])
def test_every_class_at_a_marked_candidate(host, sf):
    _, _, _, mu, sigma, nv = host
    j = _check(host, me.placed_maxima(mu[me.MARK], sigma[me.MARK], nv, sf, me.MARK_GAMMAS), sf, "S=64")
    assert all(v > 0.0 for v in j["by_class"]["a"].values())
    for g in me.SINGLE_GAMMAS:
        _check(host, me.placed_maxima(mu[me.MARK], sigma[me.MARK], nv, sf, [g]), sf, "S=1 gamma=%g" % g)


@pytest.mark.parametrize("sf", [1.0, -1.0])
def test_across_the_switch_of_erfcx_pos(host, sf):
    """64 maxima: gamma_s = -/+ 3 sqrt 2 (1 + k 2^-50), k = -16 .. 15, at the marked candidate -- the product
    exp(z^2) erfc(z) on one side of z = 3, the 50-term fraction on the other, for gamma <= 0 and for gamma > 0"""
    _, _, _, mu, sigma, nv = host
    k = np.arange(-16, 16)
    gam = np.concatenate([-SWITCH * (1.0 + k * 2.0 ** -50), SWITCH * (1.0 + k * 2.0 ** -50)])
    j = _check(host, me.placed_maxima(mu[me.MARK], sigma[me.MARK], nv, sf, gam), sf, "switch")
    # the marked row alone, one maximum at a time: each side of the switch judged by itself
    worst = 0.0
    for g in gam[::4]:
        jj = _check(host, me.placed_maxima(mu[me.MARK], sigma[me.MARK], nv, sf, [g]), sf, "S=1 gamma=%.17g" % g)
        worst = max(worst, jj["rows"]["a"][me.MARK])
    print("marked row across the switch: at most %.3g of its bar" % worst)
