"""Extended-precision (x87 80-bit, numpy.longdouble) restatement of the joint posterior -- TEST INFRASTRUCTURE, written
from the definitions in tests/cov_reference.py's docstring, not from the library and not from SciPy:

    u = x / l;  d2(a, b) = sum_d (a_d - b_d)^2, dimension by dimension;  k0 = the unit kernel of d2
    K = c k0(X, X), its diagonal SET to c + noise + jitter;  L = chol(K) (column by column)
    yn = (y - mean) / std, population mean and standard deviation (an exactly zero std -> 1)
    z = L^-1 yn;  alpha = L^-T z;  Ks = c k0(Xq, X);  V = L^-1 Ks^T
    Sigma = c k0(Xq, Xq) + [latent ? 0 : noise] I - V^T V;  mu = y_mean + y_std Ks alpha;  raw covariance = y_std^2 Sigma

Every intermediate is long double: the f64 NumPy/SciPy reference (tests/cov_reference.py) and the library are both
measured against this, so the parity bars can be a few ulps of f64 times the conditioning instead of 1e-5.

A platform whose long double is not at least the 64-bit-mantissa format makes the import fail, and with it every test
that uses the module -- a reference no better than what it judges must not pass for one.
"""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not an extended format here (eps %g): no reference" % np.finfo(LD).eps

KINDS = ("rbf", "matern12", "matern32", "matern52")


def unit_kernel(d2, kind):
    if kind == "rbf":
        return np.exp(LD(-0.5) * d2)
    d = np.sqrt(d2)
    if kind == "matern12":
        return np.exp(-d)
    if kind == "matern32":
        k = d * np.sqrt(LD(3))
        return (LD(1) + k) * np.exp(-k)
    if kind == "matern52":
        k = d * np.sqrt(LD(5))
        return (LD(1) + k + k * k / LD(3)) * np.exp(-k)
    raise ValueError(kind)


def sqdist(A, B):
    out = np.zeros((A.shape[0], B.shape[0]), LD)
    for d in range(A.shape[1]):
        t = A[:, d][:, None] - B[:, d][None, :]
        out += t * t
    return out


def cholesky(A):
    """lower factor, column by column (each column's rows in one vectorised step); numpy.linalg.LinAlgError at a pivot <= 0"""
    A = np.array(A, dtype=LD, copy=True)
    n = A.shape[0]
    for j in range(n):
        p = A[j, j] - A[j, :j] @ A[j, :j]
        if not p > 0:
            raise np.linalg.LinAlgError("pivot %d is not positive" % j)
        A[j, j] = np.sqrt(p)
        if j + 1 < n:
            A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, :j] @ A[j, :j]) / A[j, j]
    return np.tril(A)


def forward(L, B):
    """L^-1 B for B (n, k): row by row"""
    X = np.zeros(B.shape, LD)
    for i in range(L.shape[0]):
        X[i] = (B[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def backward(L, b):
    """L^-T b for b (n,)"""
    x = np.zeros(b.shape, LD)
    for i in range(L.shape[0] - 1, -1, -1):
        x[i] = (b[i] - L[i + 1:, i] @ x[i + 1:]) / L[i, i]
    return x


class Fit:
    """the fitted state in long double: scaled training points, L, alpha, the normalisation of y"""

    def __init__(self, X, y, kind, constant, length_scale, noise, jitter, normalize_y=True):
        assert kind in KINDS
        self.kind = kind
        self.c, self.noise, self.jitter = LD(constant), LD(noise), LD(jitter)
        self.ls = np.atleast_1d(np.asarray(length_scale, dtype=np.float64)).astype(LD)
        self.Xs = np.atleast_2d(np.asarray(X, dtype=np.float64)).astype(LD) / self.ls
        yl = np.asarray(y, dtype=np.float64).astype(LD)
        if normalize_y:
            self.y_mean = yl.sum() / LD(yl.shape[0])
            self.y_std = np.sqrt(((yl - self.y_mean) ** 2).sum() / LD(yl.shape[0]))
            if self.y_std == 0:
                self.y_std = LD(1)
        else:
            self.y_mean, self.y_std = LD(0), LD(1)
        yn = (yl - self.y_mean) / self.y_std
        K = self.c * unit_kernel(sqdist(self.Xs, self.Xs), kind)
        K[np.diag_indices_from(K)] = self.c + self.noise + self.jitter
        self.L = cholesky(K)
        self.alpha = backward(self.L, forward(self.L, yn[:, None])[:, 0])


def predict_cov(fit, Xq):
    """mu (m,), the OBSERVED raw covariance (m, m) and the LATENT one, all long double.  Sigma is formed once; the
    latent matrix is the observed one with the noise taken off its diagonal."""
    Q = np.atleast_2d(np.asarray(Xq, dtype=np.float64)).astype(LD) / fit.ls
    Ks = fit.c * unit_kernel(sqdist(Q, fit.Xs), fit.kind)
    V = forward(fit.L, np.ascontiguousarray(Ks.T))
    Kqq = fit.c * unit_kernel(sqdist(Q, Q), fit.kind)
    core = Kqq - V.T @ V
    core = (core + core.T) / LD(2)                       # (V^T V is symmetric up to the order of its sums)
    obs = core.copy()
    obs[np.diag_indices_from(obs)] += fit.noise
    v = fit.y_std * fit.y_std
    return fit.y_mean + fit.y_std * (Ks @ fit.alpha), v * obs, v * core


def sigma_block(fit, Xq, I):
    """(mu[I], observed cov[I][:, I], latent cov[I][:, I]) of predict_cov(fit, Xq) without the rest of the matrix: an entry
    depends on its own two query points only (for m = 4096, where the full long double V^T V would take minutes)"""
    return predict_cov(fit, np.asarray(Xq)[np.asarray(I)])


def sample_joint(fit, mu, cov, eps, nugget=0.0):
    """y (S, m) = mu + y_std eps Lc^T with Lc = chol(cov / y_std^2 + nugget I), all long double"""
    A = np.asarray(cov, dtype=LD) / (fit.y_std * fit.y_std)
    A = A + LD(nugget) * np.eye(A.shape[0], dtype=LD)
    Lc = cholesky(A)
    return mu[None, :] + fit.y_std * (np.asarray(eps, dtype=np.float64).astype(LD) @ Lc.T)
