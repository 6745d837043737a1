"""NumPy f64 restatement of the Thompson-sampling draw (tgp_ts_draw / tgp_ts_sweep / tgp_ts_eval) -- TEST INFRASTRUCTURE.

The random numbers follow the counter layout of csrc/ts_kernels.hip (Philox-4x32-10 keyed by the seed, counter
(element lo, element hi, stream, TAG)); the path is pathwise conditioning with random Fourier features on an
``oracle.gp_oracle`` fit, the update solved with SciPy's Cholesky of K (independent of the library's inverse factor).
tests/test_ts_reference.py holds this to the mathematics, tests/test_gpu_thompson.py holds the GPU to this.
"""
import numpy as np
from scipy.linalg import cho_solve

from oracle import gp_oracle as G
from philox_ref import philox4x32_10

TAG = 0x54534D50
TWO_PI = 6.283185307179586
GOLDEN = 0x9E3779B97F4A7C15
NU2 = {"rbf": 0, "matern12": 1, "matern32": 3, "matern52": 5}
S_OMEGA, S_CHI2, S_B, S_W, S_EPS = 0, 1, 2, 3, 4


def _words(e, stream, seed):
    e = np.asarray(e, dtype=np.uint64)
    return philox4x32_10(e & np.uint64(0xFFFFFFFF), e >> np.uint64(32), stream, TAG, seed & 0xFFFFFFFF, seed >> 32)


def _u53(a, b):
    return ((a >> np.uint64(5)).astype(np.float64) * 67108864.0 + (b >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0


def normals(e, stream, seed):
    """one Box-Muller branch per element: sqrt(-2 log(1 - u1)) cos(2 pi u2), u1 from words (0, 1), u2 from (2, 3)"""
    r = _words(e, stream, seed)
    u1, u2 = _u53(r[0], r[1]), _u53(r[2], r[3])
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(TWO_PI * u2)


def draw(seed, S, F, D, N, kind, noise_plus_jitter):
    """omega (F, D) in scaled coordinates, b (F,), W (S, F), eps (S, N)"""
    seed = int(seed) % (1 << 64)
    i = np.arange(F, dtype=np.uint64)
    z = normals((i[:, None] * np.uint64(D) + np.arange(D, dtype=np.uint64)[None, :]).reshape(-1), S_OMEGA, seed).reshape(F, D)
    nu2 = NU2[kind]
    if nu2 > 0:
        n = normals((i[:, None] * np.uint64(8) + np.arange(nu2, dtype=np.uint64)[None, :]).reshape(-1), S_CHI2, seed)
        chi = (n.reshape(F, nu2) ** 2).sum(1)
        z = z * np.sqrt(nu2 / chi)[:, None]
    r = _words(i, S_B, seed)
    b = TWO_PI * _u53(r[0], r[1])
    W = normals(np.arange(S * F, dtype=np.uint64), S_W, seed).reshape(S, F)
    eps = np.sqrt(noise_plus_jitter) * normals(np.arange(S * N, dtype=np.uint64), S_EPS, seed).reshape(S, N)
    return dict(omega=z, b=b, W=W, eps=eps)


class Paths:
    """S sample paths of the latent function of ``model`` (a gp_oracle.GPModel), in raw units"""

    def __init__(self, model, seed, S, F):
        self.m = model
        self.S, self.F = int(S), int(F)
        X = np.asarray(model.X, dtype=np.float64)
        self.ls = np.broadcast_to(model.length_scale, (X.shape[1],)).astype(np.float64)
        self.Xs = X / self.ls
        self.d = draw(seed, S, F, X.shape[1], X.shape[0], model.kind, model.noise + model.jitter)
        self.scale = np.sqrt(2.0 * model.constant / F)
        pX = self.prior_scaled(self.Xs)                                   # (N, S)
        self.V = (model.alpha[:, None] - cho_solve((model.L, True), pX + self.d["eps"].T, check_finite=False)).T   # (S, N)

    def prior_scaled(self, U):
        return self.scale * np.cos(U @ self.d["omega"].T + self.d["b"]) @ self.d["W"].T

    def latent(self, Xq, chunk=4096):
        """f_s at the rows of Xq, normalised units: (m, S)"""
        Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
        out = np.empty((Xq.shape[0], self.S))
        for a in range(0, Xq.shape[0], chunk):
            x = Xq[a:a + chunk]
            Ks = G.cross_kernel(x, self.m.X, self.m.kind, self.m.constant, self.ls)
            out[a:a + chunk] = self.prior_scaled(x / self.ls) + Ks @ self.V.T
        return out

    def values(self, Xq, chunk=4096):
        """raw sampled values (m, S)"""
        return self.m.y_mean + self.m.y_std * self.latent(Xq, chunk)

    def grad(self, Xq):
        """d raw value / d x: (m, S, D)"""
        Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
        om, b, W = self.d["omega"], self.d["b"], self.d["W"]
        U = Xq / self.ls
        sn = np.sin(U @ om.T + b)                                       # (m, F)
        gp = -self.scale * np.einsum("mf,sf,fd->msd", sn, W, om)
        diff = U[:, None, :] - self.Xs[None, :, :]                      # (m, N, D)
        d2 = (diff ** 2).sum(-1)
        h = self.m.constant * h_weight(self.m.kind, d2)                 # (m, N)
        gu = -np.einsum("mn,mnd,sn->msd", h, diff, self.V)
        return self.m.y_std * (gp + gu) / self.ls


def h_weight(kind, d2):
    """dk0/dx_d = -h (u_d - xs_d) / l_d (csrc/query_math.hpp); Matern 1/2 takes 0 at r = 0"""
    if kind == "rbf":
        return np.exp(-0.5 * d2)
    r = np.sqrt(d2)
    if kind == "matern12":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, np.exp(-r) / np.where(r > 0, r, 1.0), 0.0)
    if kind == "matern32":
        return 3.0 * np.exp(-np.sqrt(3.0 * d2))
    t = np.sqrt(5.0 * d2)
    return 5.0 / 3.0 * (t + 1.0) * np.exp(-t)


def select(f, sf, distinct):
    """per sample the arg-max of sf * f (M, S): lowest index on ties, NaN never wins; distinct: skip earlier picks"""
    f = np.asarray(f, dtype=np.float64)
    M, S = f.shape
    taken = np.zeros(M, dtype=bool)
    idx = np.empty(S, dtype=np.int64)
    for s in range(S):
        v = sf * f[:, s]
        v = np.where(np.isnan(v), -np.inf, v)
        v = np.where(taken, -np.inf, v)
        cand = np.nonzero(~taken)[0]
        i = int(cand[np.argmax(v[cand])])
        idx[s] = i
        if distinct:
            taken[i] = True
    return idx, f[idx, np.arange(S)]


def mc_kernel(omega, b, U1, U2, constant):
    """the F-feature Monte Carlo estimate of c k0(U1, U2): (2c/F) sum_i cos(omega_i u1 + b_i) cos(omega_i u2 + b_i)"""
    F = omega.shape[0]
    return (2.0 * constant / F) * np.cos(U1 @ omega.T + b) @ np.cos(U2 @ omega.T + b).T
