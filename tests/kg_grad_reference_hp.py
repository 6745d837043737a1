"""Extended-precision (numpy.longdouble) gradient of the knowledge gradient -- TEST INFRASTRUCTURE: the closed form of
tests/kg_grad_reference.py (``assemble``, ``slopes_grad``: they work in their arrays' precision) fed from
tests/cov_reference_hp.py's Fit, tests/kg_reference_hp.py's posterior and tests/acq_grad_reference_hp.py's posterior
gradient, Phi and pdf; every intermediate is long double.  ``central_differences`` differentiates the 80-bit VALUE
(kg_reference_hp.kg) instead: the closed form is held to it on the CPU."""
import numpy as np

import acq_grad_reference_hp as ah
import cov_reference_hp as hp
import kg_grad_reference as gr
import kg_reference as kr
import kg_reference_hp as krh

LD = np.longdouble


def kg_grad(fit, Xa, Xq, sf):
    """dict(kg (m,), grad (m, D), on_env, strict, kink, n_env) in long double"""
    Xa = np.atleast_2d(np.asarray(Xa, dtype=np.float64))
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    m, D = Xq.shape
    l = np.broadcast_to(fit.ls, (D,)) if fit.ls.shape[0] == 1 else fit.ls
    ys2 = fit.y_std * fit.y_std
    mu_a, mu, sigma, cov = krh.posterior(fit, Xa, Xq)
    nv, ov = fit.noise * ys2, (fit.noise + fit.jitter) * ys2
    a, b, live = kr.lines_from_outputs(mu_a, mu, sigma, cov, nv, ov, LD(sf))
    v = np.maximum(sigma * sigma - nv, LD(0))
    s = np.sqrt(np.where(live, v + ov, LD(1)))
    post = ah.posterior(fit, Xq)
    dv = LD(2) * post["sigma"][:, None] * post["dsigma"]
    Q, Ua = Xq.astype(LD) / fit.ls, Xa.astype(LD) / fit.ls
    ch = fit.c * ah.h_weight(hp.sqdist(Q, fit.Xs), fit.kind)                 # (m, N)
    cha = fit.c * ah.h_weight(hp.sqdist(Q, Ua), fit.kind)                    # (m, A)
    Ka = fit.c * hp.unit_kernel(hp.sqdist(Ua, fit.Xs), fit.kind)             # (A, N)
    W = ah.backward_columns(fit.L, hp.forward(fit.L, np.ascontiguousarray(Ka.T)))   # (N, A)
    dC = np.zeros((m, Xa.shape[0], D), LD)
    for d in range(D):
        diff = Q[:, d][:, None] - fit.Xs[:, d][None, :]
        diffa = Q[:, d][:, None] - Ua[:, d][None, :]
        dC[:, :, d] = ys2 / l[d] * ((ch * diff) @ W - cha * diffa)
    db = gr.slopes_grad(cov, v, s, dC, dv, ~(v > 0))
    out = gr.assemble(a, b, db, post["dmu"], sf, live, Phi=ah.Phi, pdf=ah.pdf)
    out["kg"] = np.where(live, krh.envelope_kg(np.where(live[:, None], a, LD(0)), np.where(live[:, None], b, LD(0))), LD(0))
    return out


def central_differences(fit, Xa, Xq, sf, step=1e-7):
    """(m, D): central differences, step in x, of the 80-bit value kg_reference_hp.kg"""
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    m, D = Xq.shape
    P = np.repeat(Xq[:, None, :], 2 * D, axis=1)
    for d in range(D):
        P[:, 2 * d, d] += step
        P[:, 2 * d + 1, d] -= step
    P = P.reshape(-1, D)
    val = krh.kg(fit, Xa, P, sf)["kg"].reshape(m, D, 2)
    h = (P.reshape(m, D, 2, D)[:, np.arange(D), 0, np.arange(D)] - P.reshape(m, D, 2, D)[:, np.arange(D), 1, np.arange(D)]).astype(LD)
    return (val[..., 0] - val[..., 1]) / h
