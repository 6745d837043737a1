"""The proved error term of the pruned sweep's screen (turbo_amd/csrc/prune_screen.hpp), on the CPU:
the float32 expansion under four summation orders, with the matrix core's products and partial sums rounded to nearest and
toward zero, and with v_exp_f32's last bit pushed against the bound on either side, stays within E(c) of the exact path's
mean for EVERY candidate of the adversarial inputs (candidates on training points, rows far outside the cube, ARD length
scales spanning 100x, underflowing kernel values, constant 1 and 50, alpha of mixed signs with |alpha|_1 = 1e4)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_screen_reference as ref            # noqa: E402

DS = (1, 5, 32, 40)


@pytest.fixture(scope="module")
def exact():
    """the exact path's mean of every case, once: {(D, config): (inputs, mean, mean with k one ulp down, ... up)}"""
    out = {}
    for D in DS:
        for cfg in ref.CONFIGS:
            case = ref.adversarial_case(D, cfg)
            out[(D, cfg)] = (case, [ref.exact_mean(*case, bump=b) for b in (0, -1, 1)])
    return out


@pytest.mark.parametrize("cfg", ref.CONFIGS)
@pytest.mark.parametrize("D", DS)
def test_expansion_stays_within_the_proved_error(exact, D, cfg):
    (Cs, Xs, alpha, constant), (mu, mu_dn, mu_up) = exact[(D, cfg)]
    assert Cs.shape == (512, D) and Xs.shape == (300, D)
    assert abs(np.abs(alpha).sum() - 1e4) < 1e-6 and (alpha > 0).any() and (alpha < 0).any()
    E = ref.error_bound(Cs, Xs, alpha, constant, D)
    assert np.isfinite(E).all() and (E > 0).all()
    worst = 0.0
    for order in ref.ORDERS:
        for trunc in (False, True):
            ms = ref.screen_mean(Cs, Xs, alpha, constant, order, trunc)
            r = np.abs(ms - mu) / E
            worst = max(worst, float(r.max()))
            assert (np.abs(ms - mu) <= E).all(), (D, cfg, order, trunc, float(r.max()))
    # v_exp_f32's last bit, against the bound: the screen's k up and the exact path's down, and the other way round
    for bs, m in ((1, mu_dn), (-1, mu_up)):
        ms = ref.screen_mean(Cs, Xs, alpha, constant, "chunks2", True, bump=bs)
        r = np.abs(ms - m) / E
        worst = max(worst, float(r.max()))
        assert (np.abs(ms - m) <= E).all(), (D, cfg, "bump", bs, float(r.max()))
    print("D=%d %s: largest |mu_s - mu~| / E = %.3g, E in [%.3g, %.3g]" % (D, cfg, worst, E.min(), E.max()))
    assert worst > 0.0 or cfg == "underflow_c1"      # (the two paths are not the same arithmetic: a zero would mean the model compares a path with itself)


def test_cancellation_cases_are_really_there():
    Cs, Xs, alpha, constant = ref.adversarial_case(32, "iso_c1")
    d2 = ((Cs[::7, None, :].astype(np.float64) - Xs[None, :, :].astype(np.float64)) ** 2).sum(-1)
    assert (d2.min(1) == 0.0).all()                  # every 7th candidate IS a training point
    assert ref.sq_norms(Cs[::11]).mean() > 20 * ref.sq_norms(Cs[1::11]).mean()
    Cu, Xu, _, cu = ref.adversarial_case(5, "underflow_c1")
    k = ref.kernel_value(np.float32(((Cu[1, None, :] - Xu) ** 2).sum(-1)), cu)
    assert (k == 0).any()


def test_error_terms_match_the_header():
    """the constants of screen_error_terms() are restated in the model: hold the two texts together"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "turbo_amd", "csrc", "prune_screen.hpp")).read()
    for piece in ("1.5 * D + 6.0", "0.5 * (D + 3) + 1.4 * fabs(log2(constant)) + 11.2", "8.0 * (double)(N + 8) * 0x1p-53", "0x1p-120",
                  "1.001 * constant", "1.001 * sa[0]"):
        assert piece in src, piece
