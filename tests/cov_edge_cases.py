"""The models, bars and comparisons of the joint posterior's edge tests -- TEST INFRASTRUCTURE shared by
tests/test_cov_reference_hp.py (CPU: the f64 reference and the host backend against the 80-bit reference, and the proof
that the bars reject the slips they are there for) and tests/test_gpu_cov_edges.py (the kernels).

Every model: c = 1.3, noise 1e-3, jitter 1e-10, normalize_y; X, y and the 300 base query rows as tests/test_gpu_cov.py's
_data draws them (seed 100 + N, Xq[5] = X[0]); length scales uniform(0.4, 0.9) sqrt(D / 3) (ARD) or 0.6 sqrt(D / 3), so a
17- or 33-dimensional model stays correlated instead of diagonal.

Bars, as fractions of cov_reference.scales(model), u = 2^-53:   bar = FACTOR max(e_ref, n u)
  e_ref   the f64 NumPy/SciPy reference's own error against the 80-bit reference for that model and quantity (what an
          honest f64 computation on this conditioning loses), computed here, never taken from the code under test;
  FACTOR  64: room for another algorithm (an explicit inverse factor, fixed-order MFMA sums) over a backward-stable solve;
  n u     the floor where NumPy happens to land on the last bit (n = N training points; m for a sample's factor);
  caps    a condition, not a measurement: no covariance bar is above 1e-10 and no mu / sample bar above 1e-9, so the bar
          is min(formula, cap) (model G's mu, cond(K) of some 1e6, is the one case near its cap: whether the cap binds
          depends on the BLAS under the f64 reference), and a reference that is not ten times better than the cap judges
          nothing and is an error here.
          The smallest f32 slip (query points rounded to f32: 2.5e-9 in the covariance) is 25 x above the covariance cap.
"""
import numpy as np
from scipy.linalg import cholesky, solve_triangular

import cov_reference as cr
import cov_reference_hp as hp
from oracle import gp_oracle as G

LD = np.longdouble
U = 2.0 ** -53
FACTOR = 64.0
CAP_COV, CAP_VAL = 1e-10, 1e-9
APPEND_BAR = 1e-9            # DESIGN.md's figure for an appended fit against a refit (model H; its reference IS the refit)
C, NOISE, JITTER = 1.3, 1e-3, 1e-10
M_BASE = 300

MODELS = {
    "A": dict(N=128, D=2, kind="rbf", ard=False, dtype="f64"),       # upper edge of the one-workgroup fit; NV = 128, Np = 256
    "B": dict(N=129, D=3, kind="matern32", ard=False, dtype="f64"),  # lower edge of the mid class
    "C": dict(N=256, D=4, kind="matern12", ard=False, dtype="f64"),  # upper edge of the mid class; NV = Np
    "D": dict(N=257, D=3, kind="rbf", ard=True, dtype="f64"),        # lower edge of the blocked fit; NV = 384 < Np = 512
    "E": dict(N=300, D=17, kind="matern52", ard=True, dtype="f64"),  # a partial second D-chunk (Ks kernel, SYRK epilogue)
    "F": dict(N=384, D=33, kind="rbf", ard=True, dtype="f32"),       # NV = N; three D-chunks; an f32 handle answers in f64
    "G": dict(N=1100, D=6, kind="rbf", ard=True, dtype="f64"),       # several outer blocks, NV = 1152 < Np = 1280
    "H": dict(N=300, D=5, kind="matern52", ard=True, dtype="f64", append=True),   # 299 rows, then fit(append=True) with all 300
}
M_EDGES = (1, 63, 64, 65, 127, 128, 129, 192, 193, 256, 257)
SAMPLE_MODELS = ("A", "D", "E", "G")
SAMPLE_MS = (64, 65, 128, 129, 193, 300)
HOST_MODELS = ("A", "B")     # the two smallest: what the host backend is run on
M_LIMIT = 4096

# models that other edge suites build by the same recipe (tests/acq_grad_edge_cases.py adds its own here): data(),
# fit_handle(), reference() and hp_fit() serve them too; they are not in MODELS, so no covariance test runs them
EXTRA = {}

_data_cache, _ref_cache, _hp_cache = {}, {}, {}


def config(name):
    return MODELS[name] if name in MODELS else EXTRA[name]


def data(name, m=M_BASE):
    """X, y, length scale(s), Xq (m, D): m > 300 continues the same generator behind the 300 base rows"""
    key = (name, m)
    if key not in _data_cache:
        c = config(name)
        N, D = c["N"], c["D"]
        rng = np.random.RandomState(100 + N)
        X = rng.uniform(0, 1, (N, D))
        y = 1.5 + np.sin(3 * X.sum(1)) + 0.3 * X[:, 0] + 0.02 * rng.normal(size=N)
        ls = (rng.uniform(0.4, 0.9, D) if c["ard"] else 0.6) * np.sqrt(D / 3.0)
        Xq = rng.uniform(-0.05, 1.05, (M_BASE, D))
        Xq[5] = X[0]                              # a training point among the queries
        if m > M_BASE:
            Xq = np.vstack([Xq, rng.uniform(-0.05, 1.05, (m - M_BASE, D))])
        _data_cache[key] = (X, y, ls, Xq)
    return _data_cache[key]


def fit_handle(gp, name):
    """fit a NativeGP as the table says (model H: 299 rows, then the one-row extension)"""
    c = config(name)
    X, y, ls, _ = data(name)
    if c.get("append"):
        gp.fit(X[:-1], y[:-1], c["kind"], C, ls, NOISE, JITTER, True)
        gp.fit(X, y, c["kind"], C, ls, NOISE, JITTER, True, append=True)
        assert gp.appended, "the one-row extension did not run"
    else:
        gp.fit(X, y, c["kind"], C, ls, NOISE, JITTER, True)
    return gp


def reference(name):
    """the f64 model (oracle.gp_oracle.fit on all rows), made once"""
    if name not in _ref_cache:
        X, y, ls, _ = data(name)
        _ref_cache[name] = G.fit(X, y, config(name)["kind"], C, ls, NOISE, JITTER, True)
    return _ref_cache[name]


def hp_fit(name):
    if ("fit", name) not in _hp_cache:
        X, y, ls, _ = data(name)
        _hp_cache[("fit", name)] = hp.Fit(X, y, config(name)["kind"], C, ls, NOISE, JITTER, True)
    return _hp_cache[("fit", name)]


def hp_posterior(name):
    """(mu, observed covariance, latent covariance) of the 300 base rows in long double: once per model, never modified"""
    if ("post", name) not in _hp_cache:
        out = hp.predict_cov(hp_fit(name), data(name)[3])
        for a in out:
            a.setflags(write=False)
        _hp_cache[("post", name)] = out
    return _hp_cache[("post", name)]


def errors(name, mu, cov, latent, m=None):
    """(mu error, covariance error) of a result for the leading m base rows against the 80-bit reference, as
    fractions of the scales; differences formed in long double"""
    hmu, hobs, hlat = hp_posterior(name)
    m = len(mu) if m is None else m
    want = (hlat if latent else hobs)[:m, :m]
    vs, ms = cr.scales(reference(name))
    return (float(np.abs(np.asarray(mu).astype(LD) - hmu[:m]).max()) / ms,
            float(np.abs(np.asarray(cov).astype(LD) - want).max()) / vs)


def e_ref(name):
    """{"mu", "cov_observed", "cov_latent"}: the f64 reference's own error at m = 300, as fractions of the scales"""
    if ("eref", name) not in _hp_cache:
        model, Xq = reference(name), data(name)[3]
        out = {}
        for latent in (False, True):
            mu, cov, _ = cr.predict_cov(model, Xq, latent)
            emu, ecov = errors(name, mu, cov, latent)
            out["mu"] = max(out.get("mu", 0.0), emu)
            out["cov_latent" if latent else "cov_observed"] = ecov
        _hp_cache[("eref", name)] = out
    return _hp_cache[("eref", name)]


def _bar(e, n, cap):
    assert 10 * max(e, n * U) <= cap, "the reference errs by %.3g under a cap of %.3g: too loose to judge this case" % (e, cap)
    return min(FACTOR * max(e, n * U), cap)


def bars(name, latent):
    """(mu bar, covariance bar) as fractions of the scales"""
    if MODELS[name].get("append"):
        return APPEND_BAR, APPEND_BAR
    e, N = e_ref(name), MODELS[name]["N"]
    return _bar(e["mu"], N, CAP_VAL), _bar(e["cov_latent" if latent else "cov_observed"], N, CAP_COV)


def judge_cov(name, mu, cov, latent, m=None):
    """dict(mu, cov, bar_mu, bar_cov, ok): THE comparison of a predict_cov result with the 80-bit reference"""
    emu, ecov = errors(name, mu, cov, latent, m)
    bmu, bcov = bars(name, latent)
    return dict(mu=emu, cov=ecov, bar_mu=bmu, bar_cov=bcov, ok=bool(emu <= bmu and ecov <= bcov))


# ---- samples forwards (observed, nugget 0): against cov_reference.sample_joint --------------------------------------
def sample_eps(m, S=5):
    return np.random.RandomState(m).standard_normal((S, m))


def sample_e_ref(name, m):
    """the f64 reference's own error in the observed samples of the leading m base rows (nugget 0) against the 80-bit
    factor of the 80-bit covariance, as a fraction of the value scale"""
    key = ("seref", name, m)
    if key not in _hp_cache:
        hmu, hobs, _ = hp_posterior(name)
        eps = sample_eps(m)
        want = hp.sample_joint(hp_fit(name), hmu[:m], hobs[:m, :m], eps, 0.0)
        got, _ = cr.sample_joint(reference(name), data(name)[3][:m], eps, False, 0.0)
        _hp_cache[key] = float(np.abs(got.astype(LD) - want).max()) / cr.scales(reference(name))[1]
    return _hp_cache[key]


def judge_samples(name, m, y):
    """dict(err, e_ref, bar, ok): observed samples (nugget 0, sample_eps(m)) against cov_reference.sample_joint"""
    model = reference(name)
    want, _ = cr.sample_joint(model, data(name)[3][:m], sample_eps(m), False, 0.0)
    err = float(np.abs(np.asarray(y) - want).max()) / cr.scales(model)[1]
    e = sample_e_ref(name, m)
    bar = _bar(e, m, CAP_VAL)
    return dict(err=err, e_ref=e, bar=bar, ok=bool(err <= bar))


# ---- the factor itself, backwards -------------------------------------------------------------------------------------
# The multiplier on the reference's own error in A for m <= 300.  The residual Lc Lc^T - A_ref is
# (Lc Lc^T - A_lib) + (A_lib - A_ref): the first part is the factorisation's and has Higham's bound, the second is the
# error of the library's Sigma, which no rule makes smaller than the f64 reference's.  With the multiplier at 1 the
# check failed on an MI355X on the three RBF models (A, D, G) at 1.16 ... 2.0 of the bound, every m: where the
# posterior is tight A_ii is 1e-3, Higham's term 6e-17, and the bound is e_ref (3.4e-15 ... 5.5e-15 of the scale) to
# 99 %, while the library's Sigma is 5.6e-15 ... 1.2e-14 from the 80-bit one (1.6 ... 2.1 x e_ref, 0.007 of Sigma's
# bar).  4 is the next power of two over the largest recorded ratio; both ratios are recorded, and ``own`` below holds
# the factorisation itself with no such term at all.
A_ERR_FACTOR = 4.0


def judge_factor(y, mu, y_std, A, a_err, a_err_factor=1.0, extended=True, own_cov=None):
    """The backward check of y = sample_joint(Xq[:m], n_samples=m, eps=I, latent=False, nugget=0): y[s] = mu + y_std Lc[:, s].

    zeros     y[s][j] is bit-equal to mu[j] for every j < s (Lc is zero above its diagonal)
    diag      the diagonal of Lc = ((y - mu) / y_std)^T is positive
    ratio     max_ij |Lc Lc^T - A|_ij / bound_ij,
              bound_ij = 8 (m + 1) u sqrt(A_ii A_jj) + 8 u (|mu|_max / y_std) (|Lc_i|_1 + |Lc_j|_1) / m + a_err_factor a_err
    The first term is the textbook bound of an unblocked Cholesky (Higham, Accuracy and Stability, thm 10.3) times 8 for
    panels solved with an inverted diagonal block; the second the rounding of mu + y_std Lc on the way out; a_err the
    reference's own error in A (A_ERR_FACTOR above).  ``ratio_at_factor_1`` is the same maximum with a_err_factor = 1 and
    ``scipy_ratio`` SciPy's own factor of the same A under the same bound: both for the record.
    own       (where ``own_cov``, the library's predict_cov of the same points, is given) the textbook statement itself, with
              no reference in it: Lc against the matrix it is the factor OF, A_own = own_cov / y_std^2,
              max_ij |Lc Lc^T - A_own|_ij / (the first two terms + 4 u |A_own|_ij) -- the last for the scaling by y_std^2
              and back.  It separates a wrong trailing update from a wrong Sigma: Sigma's error is not in it.
    A: Sigma_ref / y_std^2 (long double where ``extended``; the product Lc Lc^T is formed in A's precision)."""
    y, mu = np.asarray(y, dtype=np.float64), np.asarray(mu, dtype=np.float64)
    m = len(mu)
    assert y.shape == (m, m)
    low = np.tril(np.ones((m, m), dtype=bool), -1)          # [s][j], j < s
    zeros = bool(np.array_equal(y.view(np.int64)[low], np.broadcast_to(mu.view(np.int64), (m, m))[low]))
    Lc = ((y - mu[None, :]) / y_std).T
    diag = bool(np.all(np.diag(Lc) > 0))
    T = LD if extended else np.float64
    A = np.asarray(A, dtype=T)
    d = np.sqrt(np.diag(A).astype(np.float64))

    def product_and_bound(F):
        """F F^T in A's precision, and the first two terms of the bound"""
        l1 = np.abs(F).sum(1)
        Ft = F.astype(T)
        return Ft @ Ft.T, 8 * (m + 1) * U * np.outer(d, d) + 8 * U * (np.abs(mu).max() / y_std) * (l1[:, None] + l1[None, :]) / m

    P, hb = product_and_bound(Lc)
    R = np.abs(P - A).astype(np.float64)
    r, r1 = float((R / (hb + a_err_factor * a_err)).max()), float((R / (hb + a_err)).max())
    own = None
    if own_cov is not None:
        Ao = np.asarray(own_cov, dtype=np.float64) / (y_std * y_std)
        own = float((np.abs(P - Ao.astype(T)).astype(np.float64) / (hb + 4 * U * np.abs(Ao))).max())
    del P, R
    Af = np.asarray(A, dtype=np.float64)
    Ps, hs = product_and_bound(cholesky(0.5 * (Af + Af.T), lower=True, check_finite=False))
    scipy_ratio = float((np.abs(Ps - A).astype(np.float64) / (hs + a_err_factor * a_err)).max())
    return dict(zeros=zeros, diag=diag, ratio=r, ratio_at_factor_1=r1, own=own, scipy_ratio=scipy_ratio,
                ok=bool(zeros and diag and r <= 1.0 and (own is None or own <= 1.0)))


def factor_inputs(name, m):
    """(A long double, a_err) for the leading m <= 300 base rows: the 80-bit observed covariance over y_std^2, and the
    f64 reference's own error in it (e_ref of the observed covariance, in A's units)"""
    fit = hp_fit(name)
    A = hp_posterior(name)[1][:m, :m] / (fit.y_std * fit.y_std)
    return A, e_ref(name)["cov_observed"] * (C + NOISE)


def blocked_cholesky(A, skip=None, nb=64):
    """right-looking Cholesky by nb-column panels in f64 -- the shape of the library's, for the mutation tests;
    skip = (panel, block row, block column): that trailing block misses that panel's update"""
    A = np.array(A, dtype=np.float64, copy=True)
    m = A.shape[0]
    n = (m + nb - 1) // nb
    blk = lambda i: slice(i * nb, min((i + 1) * nb, m))
    for j in range(n):
        s = blk(j)
        A[s, s] = cholesky(A[s, s], lower=True, check_finite=False)
        if j + 1 == n:
            break
        r = slice((j + 1) * nb, m)
        A[r, s] = solve_triangular(A[s, s], A[r, s].T, lower=True, check_finite=False).T
        for bi in range(j + 1, n):
            for bj in range(j + 1, bi + 1):
                if (j, bi, bj) != skip:
                    A[blk(bi), blk(bj)] -= A[blk(bi), s] @ A[blk(bj), s].T
    return np.tril(A)


def limit_index_set():
    """256 rows of the m = 4096 case: the tile and block edges, every multiple of 128 and of 128 - 1, the rest drawn"""
    I = {0, 63, 64, 127, 128, 129, 4031, 4032, 4095}
    I |= set(range(0, M_LIMIT, 128)) | set(range(127, M_LIMIT, 127))
    rest = np.random.RandomState(4096).permutation(M_LIMIT)
    for r in rest:
        if len(I) >= 256:
            break
        I.add(int(r))
    return np.array(sorted(I))
