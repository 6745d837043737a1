"""Max-value entropy search (Wang & Jegelka 2017) in NumPy / SciPy: the reference the ACQ_MES kernels, the host
backend and the MES plugin are held to.

    sigma_f^2 = max(sigma^2 - noise y_std^2, 0)      the y* are maxima of the LATENT function
    gamma_s   = sf (y*_s - mu) / sigma_f
    h(gamma)  = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma)
    a(x)      = (1/S) sum_s h(gamma_s), summed in the order s = 0, 1, ...;  0 where sigma_f == 0

h goes through scipy.special.erfcx at z = |gamma| / sqrt 2, e = erfcx(z):
    gamma <= 0:  log Phi = log(e / 2) - z^2,  r = phi / Phi = sqrt(2 / pi) / e
    gamma >  0:  q = e exp(-z^2) / 2 = 1 - Phi,  log Phi = log1p(-q),  r = exp(-z^2) / (sqrt(2 pi) (1 - q))
    gamma < -50: with t = 1 / gamma^2 (Mills' ratio expanded; the two halves of h are each gamma^2 / 2 there and cancel)
                 h = log(-gamma) + (log(2 pi) - 1) / 2 + 2 t - 15/2 t^2 + 148/3 t^3      (next term ~ 4e2 t^4)
dh/dgamma = -(r / 2)(1 + gamma^2 + gamma r) on gamma >= DH_SEAM = -10 (0 where r has underflowed to 0).  Below the seam
that form loses gamma^4 ulps (8.9e-10 of dh at gamma = -49.4), so there, with x = -gamma and Laplace's continued fraction
T_k = x + k / T_(k+1) evaluated backwards from T_17 = x (DH_DEPTH = 16):  dh = -T_1 / (T_2 T_3)  -- r = T_1 and
1 + gamma^2 + gamma r = 2 / (T_2 T_3), every term positive -- without a division per level (dh_tail).  This is the f64 restatement of csrc/mes_math.hpp, operation
for operation; tests/mes_reference_hp.py is the independent 80-bit statement both are judged by."""
import numpy as np
from scipy.special import erfcx

SQRT_2_OVER_PI = 0.79788456080286536
INV_SQRT_2PI = 0.3989422804014327
H_TAIL_CONST = 0.41893853320467274      # (log(2 pi) - 1) / 2
DH_SEAM, DH_DEPTH = -10.0, 16


def dh_tail(g):
    """dh/dgamma below DH_SEAM as the device forms it: T_k = x a_k / a_(k+1) with a_k = a_(k+1) + k t a_(k+2), t = 1 / x^2,
    a_17 = 1, a_16 = 1 + 16 t (T_17 = x), and dh = -T_1 / (T_2 T_3) = -a_1 a_4 / (x a_2^2)"""
    x = -np.asarray(g, dtype=np.float64)
    with np.errstate(all="ignore"):
        ix = 1.0 / x
        t = np.where(x > 50.0, ix * ix, 1.0 / (x * x))          # (below -50 the device reuses the t of h's series)
        hi, lo = np.ones_like(x), 1.0 + DH_DEPTH * t
        a4 = lo
        for k in range(DH_DEPTH - 1, 1, -1):
            hi, lo = lo, lo + (k * t) * hi
            if k == 4:
                a4 = lo
        a1 = lo + t * hi
        return -(a1 * a4) / (x * lo * lo)


def h_and_dh(gamma):
    """h and dh/dgamma, elementwise"""
    g = np.asarray(gamma, dtype=np.float64)
    h = np.empty_like(g)
    dh = np.empty_like(g)
    tail = g < -50.0
    neg = ~tail & (g <= 0.0)
    pos = g > 0.0
    with np.errstate(all="ignore"):
        ig = 1.0 / g[tail]
        t = ig * ig
        h[tail] = np.log(-g[tail]) + H_TAIL_CONST + t * (2.0 + t * (-7.5 + t * (148.0 / 3.0)))
    z = np.abs(g) * 0.70710678118654752440
    e = erfcx(z)
    r = np.zeros_like(g)
    lp = np.zeros_like(g)
    r[neg] = SQRT_2_OVER_PI / e[neg]
    lp[neg] = np.log(0.5 * e[neg]) - z[neg] * z[neg]
    with np.errstate(over="ignore"):
        ez = np.exp(-z[pos] * z[pos])
    q = 0.5 * e[pos] * ez
    r[pos] = INV_SQRT_2PI * ez / (1.0 - q)
    lp[pos] = np.log1p(-q)
    live = neg | pos
    h[live] = 0.5 * g[live] * r[live] - lp[live]
    with np.errstate(all="ignore"):
        dh[live] = np.where(r[live] == 0.0, 0.0, -0.5 * r[live] * (1.0 + g[live] * g[live] + g[live] * r[live]))
    low = g < DH_SEAM
    dh[low] = dh_tail(g[low])
    return h, dh


def h(gamma):
    return h_and_dh(gamma)[0]


def latent_var(sigma, noise, y_std):
    sigma = np.asarray(sigma, dtype=np.float64)
    return sigma * sigma - noise * (y_std * y_std)


def mes(mu, sigma, ystar, sf, noise, y_std):
    """a (M,) from the raw posterior mean / deviation (M,) and the S maxima"""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    ystar = np.asarray(ystar, dtype=np.float64).reshape(-1)
    v = latent_var(sigma, noise, y_std)
    live = v > 0.0
    sl = np.sqrt(v[live])
    acc = np.zeros(sl.shape)
    for s in range(ystar.shape[0]):                     # the order of the sum: s = 0, 1, ...
        acc = acc + h(sf * (ystar[s] - mu[live]) / sl)
    out = np.zeros_like(mu)
    out[live] = acc / float(ystar.shape[0])
    return out


def mes_coefficients(mu, sigma, ystar, sf, noise, y_std):
    """(a, da/dmu, da/dsigma): d gamma / d mu = -sf / sigma_f, d gamma / d sigma_f = -gamma / sigma_f,
    d sigma_f / d sigma = sigma / sigma_f"""
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    ystar = np.asarray(ystar, dtype=np.float64).reshape(-1)
    S = float(ystar.shape[0])
    v = latent_var(sigma, noise, y_std)
    a, cm, cs = np.zeros_like(mu), np.zeros_like(mu), np.zeros_like(mu)
    live = v > 0.0
    sl = np.sqrt(v[live])
    sa, sdh, sgdh = np.zeros(sl.shape), np.zeros(sl.shape), np.zeros(sl.shape)
    for s in range(ystar.shape[0]):
        g = sf * (ystar[s] - mu[live]) / sl
        hv, dh = h_and_dh(g)
        sa, sdh, sgdh = sa + hv, sdh + dh, sgdh + g * dh
    a[live] = sa / S
    cm[live] = -sf * sdh / (sl * S)
    cs[live] = -sgdh * sigma[live] / (v[live] * S)
    return a, cm, cs
