"""The proved error term of the fp16 screen (turbo_amd/csrc/prune_screen_h2.hpp), on the CPU: the
two-plane fp16 dot product under four summation orders, with the matrix core's partial sums rounded to nearest and toward
zero and v_exp_f32's last bit pushed against the bound, the sign-partitioned sums and E = min(closed, weighted) stay within
E of the exact path's mean for EVERY candidate of prune_screen_reference's adversarial inputs and of the extra cases
(one-signed alpha, a positive count of exactly 128, N = 1 / 127 / 128 / 129, inputs that fail the range conditions).  The
error the dispatcher ends up with is nowhere looser than the f32 screen's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prune_screen_reference as ref            # noqa: E402
import prune_screen_h2_reference as h2          # noqa: E402

DS = (1, 5, 32, 40)


def check(Cs, Xs, alpha, constant, D, tag):
    """every candidate, every order / rounding / pushed last bit; returns the largest |mu_s - mu~| / E"""
    mus = [ref.exact_mean(Cs, Xs, alpha, constant, bump=b) for b in (0, -1, 1)]
    worst = 0.0
    runs = [(o, t, 0, mus[0]) for o in ref.ORDERS for t in (False, True)] + [("chunks2", True, 1, mus[1]), ("chunks2", True, -1, mus[2])]
    for order, trunc, bump, mu in runs:
        ms, W = h2.screen_mean(Cs, Xs, alpha, constant, order, trunc, bump)
        E, closed = h2.error_bound(Cs, Xs, alpha, constant, D, W)
        fin = np.isfinite(E)
        assert (E[fin] > 0).all() and (E <= closed).all()
        # W is the weight the proof speaks of: sum k_s |alpha| >= |mu_s|, and at most constant |alpha|_1 (1 + rounding)
        assert (np.abs(ms[fin]) <= W[fin] * (1 + 1e-12)).all()
        assert (W[fin] <= 1.001 * constant * np.abs(alpha).sum()).all()
        r = np.abs(ms[fin] - mu[fin]) / E[fin]
        assert (np.abs(ms[fin] - mu[fin]) <= E[fin]).all(), (tag, order, trunc, bump, float(r.max()))
        worst = max(worst, float(r.max()) if r.size else 0.0)
        # the error the default dispatch ends up with (the f32 screen's below MIN_D) is nowhere above the f32 screen's
        En = h2.dispatched_error(Cs, Xs, alpha, constant, D, W)
        Eo = ref.error_bound(Cs, Xs, alpha, constant, D)
        fin = np.isfinite(En)
        assert (En[fin] <= Eo[fin]).all(), (tag, order, trunc, float((En[fin] / Eo[fin]).max()))
    return worst, E, closed


@pytest.mark.parametrize("cfg", ref.CONFIGS)
@pytest.mark.parametrize("D", DS)
def test_fp16_screen_stays_within_the_proved_error(D, cfg):
    Cs, Xs, alpha, constant = ref.adversarial_case(D, cfg)
    worst, E, closed = check(Cs, Xs, alpha, constant, D, (D, cfg))
    assert np.isfinite(E).all()
    print("D=%d %s: largest |mu_s - mu~| / E = %.3g, E in [%.3g, %.3g], E / closed in [%.3g, %.3g], E / E_f32 median %.3g"
          % (D, cfg, worst, E.min(), E.max(), (E / closed).min(), (E / closed).max(),
             np.median(E / ref.error_bound(Cs, Xs, alpha, constant, D))))
    assert worst > 0.0 or cfg == "underflow_c1"


@pytest.mark.parametrize("name", sorted(h2.extra_cases()))
def test_extra_cases(name):
    Cs, Xs, alpha, constant, D = h2.extra_cases()[name]
    worst, E, closed = check(Cs, Xs, alpha, constant, D, name)
    print("%s: largest |mu_s - mu~| / E = %.3g, finite E on %d of %d" % (name, worst, np.isfinite(E).sum(), len(E)))
    if name == "x_out_of_range":
        assert np.isinf(E).all()                    # no candidate is screened: the tight bound pass takes them all
    elif name == "c_out_of_range":
        assert np.isinf(E[::5]).all() and np.isfinite(np.delete(E, np.s_[::5])).all()
    else:
        assert np.isfinite(E).all()
    if name == "positives_128":
        perm, ntp = h2.partition(alpha)
        assert ntp == 1 and (perm[:128] >= 0).all() and len(perm) == 128 + 256      # no padding row in the positive block
    if name == "all_positive":
        assert h2.partition(alpha)[1] * 128 == len(h2.partition(alpha)[0])
    if name == "all_negative":
        assert h2.partition(alpha)[1] == 0


def test_weighted_form_is_what_tightens_it():
    """on the unit-cube inputs the kernel values average well below the constant: the weighted form is the smaller one"""
    Cs, Xs, alpha, constant = ref.adversarial_case(32, "iso_c1")
    ms, W = h2.screen_mean(Cs, Xs, alpha, constant)
    E, closed = h2.error_bound(Cs, Xs, alpha, constant, 32, W)
    assert np.median(E / closed) < 0.8


def test_planes_carry_22_bits():
    rng = np.random.RandomState(3)
    v = (rng.normal(size=4096) * 10.0 ** rng.uniform(-3, 3, size=4096)).astype(np.float32)
    s = h2.scale(np.abs(v).max())
    v1, v2 = h2.split2(v * s)
    assert np.abs(v1).max() < 2.0 ** 14 and np.abs(v1).max() >= 2.0 ** 13
    big = np.abs(v * s) >= 2.0 ** -14
    assert (np.abs(v1 + v2 / 2048.0 - (v * s).astype(np.float64))[big] <= 2.0 ** -22 * np.abs(v * s)[big]).all()


def test_error_terms_match_the_header():
    """the constants of screen_h2_error_terms() are restated in the model: hold the two texts together"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "turbo_amd", "csrc", "prune_screen_h2.hpp")).read()
    for piece in ("2.01 * D + 25.0 + 0.26 * sqrt((double)D)", "ce * u * 0.5 * t.dcoef", "ce * (0.7 * L * u + 0x1p-41)",
                  "ce * u * (2.4 + 1.4 * L)", "1.001 * expm1(0.5001 * delta)", "0x1p-24 * R + 0x1p-40", "1.001 * sa[0]",
                  "SCRH_MIN_D = 15", "R < 0x1p46", "xm2 < 0x1p54f"):
        assert piece in src, piece
