"""NumPy restatement of the hyper-parameter slice sampler behind ``tgp_hyper_sample`` (csrc/host_slice.hpp): coordinate-wise
slice sampling with stepping-out and shrinkage (Neal 2003, figs. 3 and 5) of exp(LML(theta)) on a box in log space, driven by
the Philox stream of tests/philox_ref.py and the oracle's log marginal likelihood.  Test helper, not product code."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import gp_oracle as o            # noqa: E402
from philox_ref import philox4x32_10         # noqa: E402

SLICE_TAG = 0x534C4943      # "SLIC"
SLICE_STEPS = 8
SLICE_SHRINKS = 1000


class Stream:
    """the j-th uniform of a call: philox_u53 of words 0, 1 of philox4x32_10(j lo, j hi, TAG, 0, seed lo, seed hi)"""

    def __init__(self, seed, block=4096):
        self.seed, self.j, self.block = int(seed), 0, block
        self.buf, self.base = None, 0

    def next(self):
        if self.buf is None or self.j >= self.base + self.block:
            self.base = self.j
            e = np.arange(self.base, self.base + self.block, dtype=np.uint64)
            r = philox4x32_10(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), SLICE_TAG, 0,
                              self.seed & 0xFFFFFFFF, self.seed >> 32)
            self.buf = ((r[0] >> np.uint64(5)).astype(np.float64) * 67108864.0
                        + (r[1] >> np.uint64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)
        u = float(self.buf[self.j - self.base])
        self.j += 1
        return u


def oracle_lml(X, y, kind, n_ls, jitter, normalize_y):
    """theta -> LML through oracle.fit, -inf (and a count) where the matrix is not positive definite"""
    def f(theta):
        theta = np.asarray(theta, dtype=np.float64)
        ls = np.array([math.exp(float(t)) for t in theta[1:1 + n_ls]])      # (the C library's exp, as the sampler forms them)
        try:
            return o.fit(X, y, kind, math.exp(theta[0]), ls if n_ls > 1 else float(ls[0]), math.exp(theta[-1]),
                         jitter, normalize_y).lml
        except np.linalg.LinAlgError:
            return None
    return f


def slice_sample(lml, theta0, lo, hi, S, burn, thin, width=None, seed=0):
    """returns dict(theta (S, P), lml (S,), evaluations, not_pd, margin): `margin` is the smallest |LML - slice level| over
    every comparison the walk made -- a walk can only differ between two implementations of the LML where it is within
    their rounding"""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    P = lo.shape[0]
    width = np.ones(P) if width is None else np.broadcast_to(np.asarray(width, dtype=np.float64), (P,))
    x = np.where(lo < hi, np.asarray(theta0, dtype=np.float64), lo)
    st = dict(evals=0, not_pd=0, margin=math.inf)

    def value_at(p, v, level):
        xt = x.copy()
        xt[p] = v
        f = lml(xt)
        st["evals"] += 1
        if f is None:
            st["not_pd"] += 1
            return -math.inf
        st["margin"] = min(st["margin"], abs(f - level))
        return f

    f = lml(x)
    st["evals"] += 1
    if f is None:
        raise np.linalg.LinAlgError("theta0 is not positive definite")
    rng = Stream(seed)
    out_t, out_f = [], []
    for sw in range(1, burn + S * thin + 1):
        for p in range(P):
            if not lo[p] < hi[p]:
                continue
            w = float(width[p])
            u = rng.next()
            level = f + (math.log(u) if u > 0.0 else -math.inf)
            L = x[p] - w * rng.next()
            R = L + w
            for _ in range(SLICE_STEPS):
                if L <= lo[p]:
                    break
                if not value_at(p, L, level) > level:
                    break
                L -= w
            L = max(L, lo[p])
            for _ in range(SLICE_STEPS):
                if R >= hi[p]:
                    break
                if not value_at(p, R, level) > level:
                    break
                R += w
            R = min(R, hi[p])
            for _ in range(SLICE_SHRINKS):
                x1 = L + rng.next() * (R - L)
                f1 = value_at(p, x1, level)
                if f1 > level:
                    x[p], f = x1, f1
                    break
                if x1 < x[p]:
                    L = x1
                else:
                    R = x1
        if sw > burn and (sw - burn) % thin == 0:
            out_t.append(x.copy())
            out_f.append(f)
    return dict(theta=np.array(out_t), lml=np.array(out_f), evaluations=st["evals"], not_pd=st["not_pd"],
                margin=st["margin"])
