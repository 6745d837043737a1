"""Extended-precision (numpy.longdouble) restatement of the knowledge gradient -- TEST INFRASTRUCTURE, written from the
definition in include/turbogp.h on tests/cov_reference_hp.py's joint posterior over vstack(Xa, Xc) and
tests/acq_grad_reference_hp.py's Phi / pdf; every intermediate is long double.  The f64 reference
(tests/kg_reference.py) and the library are both measured against this.

The envelope's structure (the sort, the stack scan) is kg_reference.envelope run on long double arrays: it only compares
and divides, so it works in the arrays' own precision.  f(z) = pdf(z) + z Phi(z) is evaluated directly at z = -|c|."""
import numpy as np

import acq_grad_reference_hp as ah
import cov_reference_hp as hp
import kg_reference as kr

LD = np.longdouble


def f_neg(az):
    az = np.asarray(az, dtype=LD)
    fin = np.isfinite(az) & (az < LD(100))
    z = np.where(fin, az, LD(0))
    out = ah.pdf(-z) - z * ah.Phi(-z)
    return np.where(fin, np.maximum(out, LD(0)), LD(0))


def envelope_kg(a, b):
    """KG of line sets (M, L) given in any precision, evaluated in long double"""
    return kr.envelope_kg(np.atleast_2d(np.asarray(a)).astype(LD), np.atleast_2d(np.asarray(b)).astype(LD), f=f_neg)


def posterior(fit, Xa, Xc):
    """mu_a (A,), mu (M,), sigma (M,) observed, cov (M, A) raw latent, all long double"""
    Xa = np.atleast_2d(np.asarray(Xa, dtype=np.float64))
    Xc = np.atleast_2d(np.asarray(Xc, dtype=np.float64))
    A = Xa.shape[0]
    mu, obs, lat = hp.predict_cov(fit, np.vstack([Xa, Xc]))
    var = np.maximum(np.diag(obs)[A:], LD(0))
    return mu[:A], mu[A:], np.sqrt(var), lat[A:, :A]


def kg(fit, Xa, Xc, sf):
    """dict(kg, mu_a, mu, sigma, cov) in long double"""
    mu_a, mu, sigma, cov = posterior(fit, Xa, Xc)
    ys2 = fit.y_std * fit.y_std
    a, b, live = kr.lines_from_outputs(mu_a, mu, sigma, cov, fit.noise * ys2, (fit.noise + fit.jitter) * ys2, LD(sf))
    val = np.where(live, envelope_kg(np.where(live[:, None], a, LD(0)), np.where(live[:, None], b, LD(0))), LD(0))
    return dict(kg=val, mu_a=mu_a, mu=mu, sigma=sigma, cov=cov)
