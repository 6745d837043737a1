"""The gradient of the knowledge gradient with respect to the candidate -- TEST INFRASTRUCTURE, written from the closed
form in include/turbogp.h at tgp_kg_grad (not from the library).  ``assemble`` is the envelope theorem on a posterior given
as arrays and works in the arrays' own precision; ``kg_grad`` feeds it from the f64 oracle (oracle/gp_oracle.py, NumPy /
SciPy), tests/kg_grad_reference_hp.py from the 80-bit fit.

    lines   i < A: a_i = sf mu(Xa_i), b_i = C(Xa_i, x) / s;   i = A: a_A = sf mu(x), b_A = v / s;   s^2 = v + (noise + jitter) y_std^2
    envelope, left to right: lines j_0 .. j_n-1, breakpoints -inf = z_0 < z_1 < .. < z_n = +inf
    P_k = Phi(z_k+1) - Phi(z_k),  E_k = phi(z_k) - phi(z_k+1)
    grad KG = sum_k E_k grad b_jk + sf grad mu ([A on the envelope] P_A - [a_A > max_{i<A} a_i])
    grad b_i = grad C_i / s - C_i grad s / s^2,  grad b_A = grad v / s - v grad s / s^2,  grad s = grad v / (2 s)
    grad_d C(Xa_i, x) = y_std^2 (d_d c k0(x, Xa_i) - sum_j d_d c k0(x, X_j) W_ji),  d_d c k0(x, X_j) = -c h(r_j) (u_d - xs_jd) / l_d
    grad v = y_std^2 dvar (tests/acq_grad_reference_hp.py), 0 where the latent variance was clamped

The indicator is a STRICT >.  Where the candidate's line is the strict maximum intercept the bracket is formed as
-(Phi(z_lo) + Phi(-z_hi)), the two tails outside its interval.  Dead rows (s^2 <= 0 or not finite, a non-finite mean): 0.

``SLIPS`` are deliberate mistakes ``kg_grad`` can be told to make: the CPU tests show that the GPU file's bars reject them.
"""
import numpy as np
from scipy.linalg import cho_solve
from scipy.special import ndtr

import acq_grad_reference_hp as ah
import kg_reference as kr
from oracle import gp_oracle as o

SLIPS = ("the -[a_A is the maximum] term dropped", "grad s dropped", "the prior term dropped", "W rounded to f32",
         "the last training point left out")


def _pdf64(z):
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


def assemble(a, b, db, dmu, sf, live, Phi=ndtr, pdf=_pdf64, drop_max_term=False):
    """grad KG (m, D) from the lines a, b (m, A + 1), the slopes' gradients db (m, A + 1, D) and grad mu (m, D) of the raw
    mean, in the arrays' precision.  Returns dict(grad, on_env (m,) the candidate's line is on the envelope, strict (m,)
    a_A > max_{i<A} a_i, kink (m,) |a_A - max_{i<A} a_i|, n_env (m,) the envelope's lines)"""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    T = a.dtype.type
    m, L = a.shape
    A = L - 1
    D = dmu.shape[1]
    az = np.where(live[:, None], a, T(0))
    bz = np.where(live[:, None], b, T(0))
    order, stack, c, size = kr.envelope(az, bz)
    grad = np.zeros((m, D), a.dtype)
    on_env, strict = np.zeros(m, bool), np.zeros(m, bool)
    kink = np.full(m, np.inf)
    for r in range(m):
        if not live[r]:
            continue
        n = int(size[r])
        lines = order[r, stack[r, :n]]
        z = np.concatenate([c[r, :n], np.array([np.inf], a.dtype)])
        E = pdf(z[:-1]) - pdf(z[1:])
        g = (E[:, None] * db[r, lines]).sum(0)
        amax = a[r, :A].max() if A > 0 else T(-np.inf)
        strict[r] = a[r, A] > amax
        kink[r] = float(abs(a[r, A] - amax))
        at = np.nonzero(lines == A)[0]
        on_env[r] = at.size > 0
        if on_env[r]:
            k = int(at[0])
            if strict[r]:
                bracket = -(Phi(z[k]) + Phi(-z[k + 1]))
                if drop_max_term:
                    bracket = Phi(z[k + 1]) - Phi(z[k])
            else:
                bracket = Phi(z[k + 1]) - Phi(z[k])
        else:
            bracket = T(-1) if strict[r] and not drop_max_term else T(0)
        grad[r] = g + T(sf) * dmu[r] * bracket
    return dict(grad=grad, on_env=on_env, strict=strict, kink=kink, n_env=np.where(live, size, 0))


def slopes_grad(cov, v, s, dC, dv, clamped, drop_ds=False):
    """db (m, A + 1, D) from C (m, A), v, s (m,), grad C (m, A, D) and grad v (m, D), in their precision"""
    T = cov.dtype.type
    dv = np.where(clamped[:, None], T(0), dv)
    ds = T(0) * dv if drop_ds else dv / (T(2) * s[:, None])
    db_i = dC / s[:, None, None] - cov[:, :, None] * ds[:, None, :] / (s * s)[:, None, None]
    db_A = dv / s[:, None] - v[:, None] * ds / (s * s)[:, None]
    return np.concatenate([db_i, db_A[:, None, :]], axis=1)


def kg_grad(om, Xa, Xq, sf, slip=None):
    """dict(kg (m,), grad (m, D), on_env, strict, kink, n_env) of the f64 reference; ``slip``: one of SLIPS, on purpose"""
    assert slip is None or slip in SLIPS
    Xa = np.atleast_2d(np.asarray(Xa, dtype=np.float64))
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    m, D = Xq.shape
    c, ys = om.constant, om.y_std
    l = np.broadcast_to(om.length_scale, (D,)) if om.length_scale.shape[0] == 1 else om.length_scale
    mu_a, mu, sigma, cov = kr.posterior(om, Xa, Xq)
    nv, ov = om.noise * ys ** 2, (om.noise + om.jitter) * ys ** 2
    a, b, live = kr.lines_from_outputs(mu_a, mu, sigma, cov, nv, ov, sf)
    v = np.maximum(sigma * sigma - nv, 0)
    s = np.sqrt(np.where(live, v + ov, 1))
    last = slip == SLIPS[4]
    post = ah.posterior_f64(om, Xq, slip="the last training point left out of the gradient sums" if last else None)
    dv = 2.0 * post["sigma"][:, None] * post["dsigma"]          # y_std^2 dvar
    # grad C: the prior term and the training points' sum against W = K^-1 c k0(X, Xa)
    Q, Xs, Ua = Xq / l, om.X / l, Xa / l
    diff = Q[:, None, :] - Xs[None, :, :]                        # (m, N, D)
    ch = c * ah.h_weight((diff * diff).sum(-1), om.kind)
    diffa = Q[:, None, :] - Ua[None, :, :]                       # (m, A, D)
    cha = c * ah.h_weight((diffa * diffa).sum(-1), om.kind)
    Ka = o.cross_kernel(Xa, om.X, om.kind, om.constant, om.length_scale)
    W = cho_solve((om.L, True), Ka.T, check_finite=False)        # (N, A)
    if slip == SLIPS[3]:
        W = W.astype(np.float32).astype(np.float64)
    if last:
        ch, diff, W = ch[:, :-1], diff[:, :-1], W[:-1]
    dC = np.einsum("qjd,ja->qad", ch[:, :, None] * diff, W, optimize=True)
    if slip != SLIPS[2]:
        dC = dC - cha[:, :, None] * diffa
    dC = ys ** 2 * dC / l
    db = slopes_grad(cov, v, s, dC, dv, ~(v > 0), drop_ds=slip == SLIPS[1])
    out = assemble(a, b, db, post["dmu"], sf, live, drop_max_term=slip == SLIPS[0])
    out["kg"] = np.where(live, kr.envelope_kg(np.where(live[:, None], a, 0.0), np.where(live[:, None], b, 0.0)), 0.0)
    return out
