"""Extended-precision (x87 80-bit, numpy.longdouble) closed form of the gradient of the log marginal likelihood with respect
to the TRAINING INPUTS (tgp_fit_input_grad; include/turbogp.h), and an f64 NumPy/SciPy restatement of the same formula that
can be made to slip -- TEST INFRASTRUCTURE, written from the definitions below, not from the kernels.  The conventions are
tests/lml_grad_reference_hp.py's; the 80-bit form sits on tests/cov_reference_hp.py's Fit.

    s = x / l;  d2_ij = sum_d (s_id - s_jd)^2;  G = alpha alpha^T - K^-1;  h(r) that module's length-scale weight, so
    dK_ij / dlog l_d = c h_ij (s_id - s_jd)^2  and, d2 depending on x_id through 2 (s_id - s_jd) / l_d,
    dK_ij / dx_id = -c h_ij (s_id - s_jd) / l_d  (row i and column i of K move together: the trace's 1/2 goes)

        d LML / d x_id = -(c / l_d) sum_{j != i} G_ij h_ij (s_id - s_jd)

    A pair with d2 = 0 (the diagonal, a duplicated training row) contributes nothing, under Matern-1/2 included.
    SCALE of an entry: the same sum with (|alpha_i alpha_j| + |K^-1_ij|) |s_id - s_jd| in place of G_ij (s_id - s_jd).

Two identities follow (G and h are symmetric, s_id - s_jd antisymmetric):
    sum_i d LML / d x_id = 0;      sum_i x_id d LML / d x_id = -d LML / d log l_d  (ARD; isotropic: summed over d, the one entry).
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

import acq_grad_reference_hp as ar
import cov_reference_hp as hp
from oracle import gp_oracle as G

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not an extended format here (eps %g): no reference" % np.finfo(LD).eps
TILE = 64

SLIPS = ("a tile's column-side contribution dropped",
         "off-diagonal tiles counted once",
         "the last row left out",
         "dimensions >= 16 dropped",
         "rows of the partial last tile dropped",
         "ls[0] for every dimension",
         "K^-1 from an f32-rounded factor",
         "a sign flip of (s_i - s_j)")
ARD_ONLY = ("ls[0] for every dimension",)


def _rows(Gm, S, Xs, ls, c, kind):
    """(gradient (n, D), scale (n, D)) in the type of Xs from the pair weights Gm, their absolute twin S, the scaled inputs
    and the D length scales"""
    n, D = Xs.shape
    d2 = np.zeros((n, n), Xs.dtype)
    for d in range(D):
        t = Xs[:, d][:, None] - Xs[:, d][None, :]
        d2 += t * t
    h = ar.h_weight(d2, kind)                    # 0 where d2 is 0
    g, sc = np.zeros((n, D), Xs.dtype), np.zeros((n, D), Xs.dtype)
    for d in range(D):
        t = Xs[:, d][:, None] - Xs[:, d][None, :]
        g[:, d] = -(c / ls[d]) * (Gm * h * t).sum(axis=1)
        sc[:, d] = (c / ls[d]) * (S * h * np.abs(t)).sum(axis=1)
    return g, sc


def dlml_dx(fit):
    """(d LML / d X (N, D), its scales (N, D)) in long double, of the model in fit (a cov_reference_hp.Fit), raw X units"""
    n, D = fit.Xs.shape
    Li = hp.forward(fit.L, np.eye(n, dtype=LD))
    Kinv = Li.T @ Li
    aa = np.outer(fit.alpha, fit.alpha)
    ls = np.broadcast_to(fit.ls, (D,))
    return _rows(aa - Kinv, np.abs(aa) + np.abs(Kinv), fit.Xs, ls, fit.c, fit.kind)


def dlml_dx_f64(X, y, kind, constant, length_scale, noise, jitter, normalize_y=True, slip=None):
    """d LML / d X (N, D) in f64.  slip: one of SLIPS, the mutation the tests inject to show that the bars reject it; None is
    the honest computation."""
    assert slip is None or slip in SLIPS
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n, D = X.shape
    ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64))
    assert ls.shape[0] > 1 or slip not in ARD_ONLY
    ls = np.broadcast_to(ls, (D,)).copy()
    yn, _, _ = G.normalise_y(y, normalize_y)
    K = G.kernel_matrix(X, kind, constant, length_scale, noise, jitter)
    L = cholesky(K, lower=True, check_finite=False)
    alpha = solve_triangular(L.T, solve_triangular(L, yn, lower=True, check_finite=False), lower=False, check_finite=False)
    Li = solve_triangular(L, np.eye(n), lower=True, check_finite=False)
    if slip == "K^-1 from an f32-rounded factor":
        Li = Li.astype(np.float32).astype(np.float64)
    Kinv = Li.T @ Li
    aa = np.outer(alpha, alpha)
    Gm, S = aa - Kinv, np.abs(aa) + np.abs(Kinv)
    Xs = X / (ls[0] if slip == "ls[0] for every dimension" else ls)
    t = np.arange(n) // TILE
    if slip == "a tile's column-side contribution dropped":      # row i hears only of the tiles at or left of its own
        Gm = Gm * (t[None, :] <= t[:, None])
    if slip == "off-diagonal tiles counted once":
        Gm = Gm * np.where(t[:, None] == t[None, :], 1.0, 0.5)
    keep = n
    if slip == "the last row left out":
        keep = n - 1
    if slip == "rows of the partial last tile dropped":
        keep = n - n % TILE
    if slip == "a sign flip of (s_i - s_j)":
        Gm = -Gm
    g = np.zeros((n, D))
    g[:keep], _ = _rows(Gm[:keep, :keep], S[:keep, :keep], Xs[:keep], ls, float(constant), kind)
    if slip == "dimensions >= 16 dropped":
        g[:, 16:] = 0.0
    return g
