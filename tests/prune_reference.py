"""NumPy restatement of the pruned sweep's bound and margin logic (csrc/sweep_pruned.hpp, sweep_pruned).

An arg-max-only sweep needs a candidate's variance only when the candidate can still win.  With q = k^T K^-1 k in [0, c]
the variance c + s^2 - q lies in [s^2, c + s^2], and EI / PI / UCB are monotone in sigma for a fixed mean, so the mean
alone bounds every candidate's acquisition from above: the mean moved by its rounding-error bound e the way that raises
the acquisition, at the larger of the values at the two ends of the sigma interval.  Under the clamp gate the computed
variance of every candidate stays above 0.99 s^2, which is the interval's lower end."""
import math

import numpy as np

ACQ_UCB, ACQ_PI, ACQ_EI = 1, 2, 3
UNIT_ROUNDOFF = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
TAU = 2e4          # TGP_PRUNE_TAU
MARGIN = 1e-6      # TGP_PRUNE_MARGIN
TOP = 256          # TGP_PRUNE_TOP


def ndtr(a):
    """cephes ndtr as finalize_kernel evaluates it"""
    x = a * 0.70710678118654752440
    z = abs(x)
    if z < 0.70710678118654752440:
        return 0.5 + 0.5 * math.erf(x)
    y = 0.5 * math.erfc(z)
    return 1.0 - y if x > 0 else y


def acq_value(acq, sf, incumbent, param, mu, sigma):
    """finalize_kernel's acquisition of one candidate"""
    if acq == ACQ_UCB:
        return sf * mu + param * sigma
    if sigma == 0.0:
        return 0.0
    diff = sf * (mu - incumbent) - param
    z = diff / sigma
    if acq == ACQ_PI:
        return ndtr(z)
    return diff * ndtr(z) + sigma * math.exp(-(z * z) / 2.0) / 2.5066282746310002


def gate(noise, constant, dtype, tau=TAU):
    """the pruned schedule runs only when s^2 / (c + s^2) >= tau * u"""
    return noise > 0.0 and noise / (constant + noise) >= tau * UNIT_ROUNDOFF[dtype]


def err_scale(N):
    """e = err_scale(N) * sum_j |k_j| |alpha_j| bounds |exact mean - bound pass's mean| (two sums of the same N products)"""
    return 4.0 * (N + 8) * 2.0 ** -53


def sigma_range(constant, noise, y_std):
    return math.sqrt((0.99 * noise) * (y_std * y_std)), math.sqrt((constant + noise) * (y_std * y_std))


def upper_bound(acq, sf, incumbent, param, mun, abs_sum, N, constant, noise, y_mean, y_std, margin=MARGIN):
    """prune_bound_kernel: the inflated upper bound of one candidate's acquisition (NaN -> +inf: it always survives)"""
    e = err_scale(N) * abs_sum
    mu = y_std * (mun + e if sf > 0 else mun - e) + y_mean
    lo, hi = sigma_range(constant, noise, y_std)
    a_lo = acq_value(acq, sf, incumbent, param, mu, lo)
    a_hi = acq_value(acq, sf, incumbent, param, mu, hi)
    if math.isnan(a_lo) or math.isnan(a_hi):
        return math.inf
    a = max(a_lo, a_hi)
    scale = abs(a) + ((abs(mu) + abs(param) * hi) if acq == ACQ_UCB else 0.0)
    return a + margin * scale


def bar(lb, margin=MARGIN):
    """the value a bound must reach for its candidate to survive"""
    return lb if math.isinf(lb) else lb - margin * abs(lb)


def lb_set(ub, top=TOP):
    """the largest bound (lowest index on ties) of each group of ceil(M / top) consecutive candidates"""
    M = len(ub)
    gs = -(-M // top)
    return np.array([g + int(np.argmax(ub[g:g + gs])) for g in range(0, M, gs)], dtype=np.int64)


def survivors(ub, picks, lb, margin=MARGIN):
    """every candidate outside the lb set whose bound reaches the bar, in index order"""
    keep = np.asarray(ub) >= bar(lb, margin)
    keep[np.asarray(picks)] = False
    return np.nonzero(keep)[0]


def pruned_argmax(exact, ub, top=TOP, margin=MARGIN):
    """the pruned schedule on host arrays: (value, index) from the lb set and the survivors, and the survivor count"""
    exact = np.asarray(exact, dtype=np.float64)
    picks = lb_set(ub, top)
    ok = ~np.isnan(exact[picks])
    lb = float(exact[picks][ok].max()) if ok.any() else -math.inf
    surv = survivors(ub, picks, lb, margin)
    idx = np.sort(np.concatenate([picks, surv]))
    vals = exact[idx]
    vals = np.where(np.isnan(vals), -np.inf, vals)
    j = int(np.argmax(vals))
    return float(vals[j]), int(idx[j]), len(surv)
