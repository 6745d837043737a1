"""float64 NumPy / SciPy reference of the knowledge gradient -- TEST INFRASTRUCTURE, written from the definition in
include/turbogp.h (not from the library) on the CPU oracle (oracle/gp_oracle.py):

    mu(.)     raw posterior mean
    C(a, x)   raw LATENT posterior covariance  y_std^2 (c k0(a, x) - c k0(a, X) K^-1 c k0(X, x))
    v(x)      max(sigma(x)^2 - noise y_std^2, 0), sigma the oracle's predict (it includes the noise)
    s(x)^2    v(x) + (noise + jitter) y_std^2
    lines     i < A: a_i = sf mu(Xa_i), b_i = C(Xa_i, x) / s(x);   i = A: a_A = sf mu(x), b_A = v(x) / s(x)
    KG(x)     E_Z[max_i (a_i + b_i Z)] - max_i a_i

evaluated as Frazier, Powell & Dayanik (2009), algorithm 1: the lines sorted by slope (of equal slopes only the largest
intercept stays), the upper envelope built by the stack scan, then KG = sum over consecutive envelope lines of
(b_next - b_i) f(-|c_i|), c_i = (a_i - a_next) / (b_next - b_i), f(z) = phi(z) + z Phi(z).

``FAULTS`` are deliberate mistakes ``kg`` can be told to make: the CPU tests show that the GPU file's bars reject them.
"""
import numpy as np
from scipy.linalg import cho_solve, solve_triangular
from scipy.special import erfcx

from oracle import gp_oracle as o

FAULTS = ("the x line left out", "the observed covariance in b", "the jitter missing from s",
          "the last 16-wide k-tile of the training points dropped", "an f32 W")


def f_neg(az):
    """f(-az) = phi(az) - az Phi(-az) for az >= 0 through erfcx: exp(-az^2 / 2) (1 / sqrt(2 pi) - az erfcx(az / sqrt 2) / 2)"""
    az = np.asarray(az, dtype=np.float64)
    t = az / np.sqrt(2.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        g = np.exp(-t * t) * np.maximum(1.0 / np.sqrt(2.0 * np.pi) - 0.5 * az * erfcx(t), 0.0)
    return np.where(az < 40.0, g, 0.0)


def envelope(a, b):
    """the upper envelope of the lines a[m, i] + b[m, i] z of every row m (algorithm 1's sort and stack scan, the rows
    side by side).  Returns (order, stack, c, size): ``order`` the slope-sorted line indices, ``stack[m, :size[m]]`` the
    positions IN that order of the envelope's lines from left to right and ``c[m, k]`` the z at which stack[m, k] takes
    over from stack[m, k - 1] (c[m, 0] = -inf).  dtype follows a / b (float64 or long double)."""
    a = np.atleast_2d(a)
    b = np.atleast_2d(b)
    M, L = a.shape
    order = np.lexsort((a, b), axis=1)                  # by slope, then by intercept: the last of equal slopes has the largest
    a_s = np.take_along_axis(a, order, 1)
    b_s = np.take_along_axis(b, order, 1)
    keep = np.ones((M, L), bool)
    keep[:, :-1] = b_s[:, 1:] != b_s[:, :-1]
    stack = np.zeros((M, L), np.int64)
    c = np.full((M, L), -np.inf, dtype=a.dtype)
    size = np.zeros(M, np.int64)
    rows_all = np.arange(M)
    for i in range(L):
        todo = keep[:, i].copy()
        first = todo & (size == 0)
        stack[first, 0] = i
        size[first] = 1
        todo &= ~first
        while todo.any():
            r = rows_all[todo]
            top = stack[r, size[r] - 1]
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                z = (a_s[r, top] - a_s[r, i]) / (b_s[r, i] - b_s[r, top])
            pop = (z <= c[r, size[r] - 1]) & (size[r] > 1)
            size[r[pop]] -= 1
            push = r[~pop]
            stack[push, size[push]] = i
            c[push, size[push]] = z[~pop]
            size[push] += 1
            todo[push] = False
    return order, stack, c, size


def envelope_kg(a, b, f=f_neg):
    """KG of every row's line set (M, L): the sum over the envelope from left to right"""
    a = np.atleast_2d(a)
    b = np.atleast_2d(b)
    order, stack, c, size = envelope(a, b)
    b_s = np.take_along_axis(b, order, 1)
    out = np.zeros(a.shape[0], dtype=a.dtype)
    for k in range(1, int(size.max()) if size.size else 0):
        r = np.nonzero(size > k)[0]
        db = b_s[r, stack[r, k]] - b_s[r, stack[r, k - 1]]
        out[r] = out[r] + db * f(np.abs(c[r, k]))
    return out


def lines_from_outputs(mu_a, mu, sigma, cov, noise_var, obs_var, sf):
    """the (M, A + 1) lines from a posterior given as arrays: mu_a (A,), mu / sigma (M,), cov (M, A) raw latent;
    noise_var = noise y_std^2, obs_var = (noise + jitter) y_std^2.  Returns (a, b, live): rows with s^2 <= 0 or not
    finite are not live (their KG is 0)"""
    mu_a, mu, sigma, cov = (np.asarray(t) for t in (mu_a, mu, sigma, cov))
    v = np.maximum(sigma * sigma - noise_var, 0)
    s2 = v + obs_var
    live = (s2 > 0) & np.isfinite(s2) & np.isfinite(mu)
    s = np.sqrt(np.where(live, s2, 1))
    a = np.concatenate([np.broadcast_to(sf * mu_a, cov.shape), (sf * mu)[:, None]], axis=1)
    b = np.concatenate([cov, v[:, None]], axis=1) / s[:, None]
    return a, b, live


def kg_from_outputs(mu_a, mu, sigma, cov, noise_var, obs_var, sf):
    a, b, live = lines_from_outputs(mu_a, mu, sigma, cov, noise_var, obs_var, sf)
    return np.where(live, envelope_kg(np.where(live[:, None], a, 0.0), np.where(live[:, None], b, 0.0)), 0.0)


def posterior(om, Xa, Xc, fault=None):
    """mu_a (A,), mu (M,), sigma (M,) and the raw latent cov (M, A) of the oracle's model"""
    Xa = np.atleast_2d(np.asarray(Xa, dtype=np.float64))
    Xc = np.atleast_2d(np.asarray(Xc, dtype=np.float64))
    mu_a = o.predict(om, Xa, return_std=False)
    mu, sigma = o.predict(om, Xc)
    Kx = o.cross_kernel(Xc, om.X, om.kind, om.constant, om.length_scale)
    Ka = o.cross_kernel(Xa, om.X, om.kind, om.constant, om.length_scale)
    prior = o.cross_kernel(Xc, Xa, om.kind, om.constant, om.length_scale)
    if fault in (FAULTS[3], FAULTS[4]):
        W = cho_solve((om.L, True), Ka.T, check_finite=False)            # (N, A)
        if fault == FAULTS[3]:
            cut = ((om.X.shape[0] - 1) // 16) * 16
            corr = Kx[:, :cut] @ W[:cut]
        else:
            corr = Kx @ W.astype(np.float32).astype(np.float64)
    else:
        Vx = solve_triangular(om.L, Kx.T, lower=True, check_finite=False)
        Va = solve_triangular(om.L, Ka.T, lower=True, check_finite=False)
        corr = Vx.T @ Va
    cov = om.y_std ** 2 * (prior - corr)
    return mu_a, mu, sigma, cov


def kg(om, Xa, Xc, sf, fault=None):
    """dict(kg (M,), mu_a, mu, sigma, cov) of the f64 reference; ``fault``: one of FAULTS, made on purpose"""
    assert fault is None or fault in FAULTS
    mu_a, mu, sigma, cov = posterior(om, Xa, Xc, fault)
    nv = om.noise * om.y_std ** 2
    ov = (om.noise + (0.0 if fault == FAULTS[2] else om.jitter)) * om.y_std ** 2
    a, b, live = lines_from_outputs(mu_a, mu, sigma, cov, nv, ov, sf)
    if fault == FAULTS[1]:
        # the observed covariance: the noise on the candidate's own variance and wherever a point IS the candidate
        s = np.sqrt(np.where(live, np.maximum(sigma * sigma - nv, 0) + ov, 1))
        same = (np.atleast_2d(Xc)[:, None, :] == np.atleast_2d(Xa)[None, :, :]).all(-1)
        b = np.concatenate([cov + nv * same, (sigma * sigma)[:, None]], axis=1) / s[:, None]
    if fault == FAULTS[0]:
        a, b = a[:, :-1], b[:, :-1]
    val = np.where(live, envelope_kg(np.where(live[:, None], a, 0.0), np.where(live[:, None], b, 0.0)), 0.0)
    return dict(kg=val, mu_a=mu_a, mu=mu, sigma=sigma, cov=cov)


def prior_scale(om):
    """y_std sqrt(c + noise): what the bars are relative to"""
    return float(om.y_std * np.sqrt(om.constant + om.noise))


def refit_lines(om, y, Xa, x, sf):
    """the lines a literal refit predicts at Xa and x: the oracle fitted on (X + {x}, y + {mu(x) + s(x) Z}) with the
    hyper-parameters, jitter, y_mean and y_std HELD gives mean(Z) = intercept + slope Z; returns (a (A + 1,), b (A + 1,)).
    The held normalisation is applied by hand: the augmented model is solved in normalised units."""
    Xa = np.atleast_2d(Xa)
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    mu_x, sg_x = o.predict(om, x)
    v = max(sg_x[0] ** 2 - om.noise * om.y_std ** 2, 0.0)
    s = np.sqrt(v + (om.noise + om.jitter) * om.y_std ** 2)
    X2 = np.vstack([om.X, x])
    K2 = o.kernel_matrix(X2, om.kind, om.constant, om.length_scale, om.noise, om.jitter)
    P = np.vstack([Xa, x])
    Kp = o.cross_kernel(P, X2, om.kind, om.constant, om.length_scale)
    out = []
    for Z in (0.0, 1.0):
        y2 = np.concatenate([np.asarray(y, dtype=np.float64), [mu_x[0] + s * Z]])
        yn2 = (y2 - om.y_mean) / om.y_std
        out.append(om.y_mean + om.y_std * (Kp @ np.linalg.solve(K2, yn2)))
    return sf * out[0], out[1] - out[0]
