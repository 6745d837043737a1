"""NumPy reference of tgp_sweep_integrated: per hyper-parameter sample oracle.fit + oracle.predict + oracle.acquisition, then
the mean of the acquisitions and the moments of the equal-weight mixture.  Test helper, not product code."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import gp_oracle as o            # noqa: E402


def unpack(theta, n_ls):
    """theta -> (constant, length scale(s), noise) exactly as the library forms them (csrc/host_slice.hpp slice_unpack): the C
    library's exp, entry by entry.  NumPy's vectorised exp differs from it in the last bit for about one argument in sixteen,
    and a caller who fits "at theta_k" with a length scale one ulp away fits another model: in f64 nobody sees it, in an f32
    sweep the cast of the factor flips a rounding here and there (seen once in a development run, not recorded: 3.1e-12 x max |acq| at N = 300, S = 64)"""
    theta = np.asarray(theta, dtype=np.float64)
    ls = np.array([math.exp(float(t)) for t in theta[1:1 + n_ls]])
    return math.exp(float(theta[0])), (ls if n_ls > 1 else float(ls[0])), math.exp(float(theta[-1]))


def acquisition(acq, mu, sigma, sf, incumbent, param):
    """acq: 'ei' / 'pi' / 'ucb' / 'sigma' / 'none'"""
    ext = "max" if sf > 0 else "min"
    if acq == "sigma":
        return np.asarray(sigma, dtype=np.float64).copy()
    if acq == "none":
        return np.zeros_like(mu)
    return o.acquisition(acq, mu, sigma, ext, param, incumbent)


def integrated(X, y, kind, thetas, n_ls, jitter, normalize_y, Xc, acq, sf, incumbent, param):
    """dict(mu, sigma, acq, best_idx, best_val, gap, per_sample=[(mu_k, sigma_k)]): gap = best - second best value"""
    thetas = np.atleast_2d(thetas)
    S = thetas.shape[0]
    a = m1 = m2 = None
    per = []
    for k in range(S):
        c, ls, noise = unpack(thetas[k], n_ls)
        model = o.fit(X, y, kind, c, ls, noise, jitter, normalize_y)
        mu, sg = o.predict(model, Xc, True)
        ak = acquisition(acq, mu, sg, sf, incumbent, param)
        per.append((mu, sg))
        if k == 0:
            a, m1, m2 = ak.copy(), mu.copy(), sg * sg + mu * mu
        else:
            a += ak
            m1 += mu
            m2 += sg * sg + mu * mu
    a, mu = a / S, m1 / S
    sigma = np.sqrt(np.maximum(0.0, m2 / S - mu * mu))
    bi = int(np.argmax(a))
    srt = np.sort(a)
    gap = float(srt[-1] - srt[-2]) if a.shape[0] > 1 else math.inf
    return dict(mu=mu, sigma=sigma, acq=a, best_idx=bi, best_val=float(a[bi]), gap=gap, per_sample=per)
