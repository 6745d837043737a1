"""Learned input warping at the plugin boundary (Snoek, Swersky, Zemel, Adams, ICML 2014; the reference's roadmap gives the
job to the surrogate: docs/source/refactor.md:42, :55).

``WarpedHipGPSurrogate`` is a ``HipGPSurrogate`` whose models live on w(X): every input dimension goes through the
Kumaraswamy CDF of its unit interval, w = 1 - (1 - u^a)^b, and a, b are learned with the kernel's hyper-parameters from the
same marginal likelihood (``tgp_fit_warp_lbfgsb`` / ``tgp_fit_warp_grad``).  A ``WarpedModel`` is an ordinary fit on w(X);
what it hands the acquisition functions and ``CandidateSweep`` as "the context" is a ``_WarpedContext``: the factory's
``NativeGP`` with ONE step added behind every call that makes a batch resident -- ``warp_candidates`` -- and the raw
coordinates kept at its boundary:

  * a batch made resident (uploaded, generated on the GPU, the NumPy stream) is warped where it lies (``tgp_warp_candidates``)
    before anything sweeps it; the chosen row is read by its INDEX from the raw rows (``tgp_warp_read_raw``), so it is one
    of the drawn candidates bit for bit, never an inverted row;
  * points handed over for one evaluation (``evaluate``, ``acq_grad``) are warped on the way in, gradients come back in RAW
    coordinates (the native gradient times dw/dx);
  * the gradient stage of the LIBRARY routes (``acq_refine``: ``tgp_acq_lbfgsb`` / ``tgp_acq_refine``) runs in WARPED
    coordinates on the unit box from the warped starts, and its results go back through the closed-form inverse: the
    infinite dw/du at the walls never enters those walks.  The SciPy routes (``lockstep='scipy'`` / ``False``) walk in RAW
    coordinates on ``acq_grad``; for them a point on such a wall gets the slope 2^-40 of the box inside: finite;
  * what this module does not serve is refused with a ``ValueError``: batch selection, Thompson sampling, max-value entropy
    search, the knowledge gradient, the winner record of the multi-GPU sweep, the fit's early sweep of a prefetched batch.

For any other model nothing changes: the routes make the calls they make today.
"""
import warnings

import numpy as np

from . import _lib
from .kernels import GPKernel, _exp_like_numpy
from .surrogates import HipGPSurrogate

_REFUSED = {
    'sweep_batch': 'select_batch / maximise_batch', 'sweep_batch_mc': 'select_batch / maximise_batch',
    'ts_draw': 'TS', 'ts_sweep': 'TS', 'ts_eval': 'TS', 'ts_read': 'TS',
    'mes_draw': 'MES', 'mes_set_maxima': 'MES',
    'kg_set_points': 'KG', 'sweep_kg': 'KG', 'kg_grad': 'KG', 'kg_lbfgsb': 'KG',
    'set_winner_out': 'the sharded multi-GPU sweep', 'sweep_integrated': 'the marginalised surrogate',
    'hyper_sample': 'the marginalised surrogate', 'export_factor': 'the multi-GPU drivers', 'import_factor': 'the multi-GPU drivers',
}


def refuse_warped(model, what):
    """``ValueError`` where ``model`` is a ``WarpedModel``: ``what`` is outside what input warping serves"""
    if getattr(model, 'is_warped', False):
        raise ValueError('{} is not available for a warped model (WarpedHipGPSurrogate): input warping serves UCB / PI / EI '
                         'through CandidateSweep and RandomAndQuasiNewton on one GPU'.format(what))


class _WarpedContext:
    """the factory's ``NativeGP`` as a ``WarpedModel`` hands it out: raw coordinates outside, warped rows inside"""

    def __init__(self, real, model):
        object.__setattr__(self, '_real', real)
        object.__setattr__(self, '_model', model)

    def __getattr__(self, name):
        if name in _REFUSED:
            refuse_warped(self._model, _REFUSED[name])
        return getattr(self._real, name)

    def __setattr__(self, name, value):
        if name == 'prefetched':          # the fit's early sweep would sweep the rows of the LAST warp: never armed
            value = False
        setattr(self._real, name, value)

    def _box(self):
        m = self._model
        return m.warp_lo, m.warp_hi, m.warp_a, m.warp_b

    # ---- the one new step: behind every call that makes a batch resident
    def warp_candidates(self):
        self._real.warp_candidates(*self._box())

    def set_candidates(self, X):
        self._real.set_candidates(X)
        self.warp_candidates()

    def set_candidates_numpy_stream(self, *args, **kwargs):
        drawn = self._real.set_candidates_numpy_stream(*args, **kwargs)
        if drawn:
            self.warp_candidates()
        return drawn

    def generate(self, *args, **kwargs):
        drew = self._real.generate(*args, **kwargs)
        self.warp_candidates()            # (a batch left alone by reuse=True is warped from its raw rows with THIS model's shapes)
        return drew

    def set_candidates_dev(self, *args, **kwargs):
        self._real.set_candidates_dev(*args, **kwargs)
        self.warp_candidates()

    # ---- rows come back raw, by index
    def get_candidate(self, idx):
        return self._real.warp_read_raw(int(idx), 1)[0]

    def read_candidates(self, first=0, count=None):
        return self._real.warp_read_raw(first, count)

    # ---- points for one evaluation
    def evaluate(self, X, *args, **kwargs):
        return self._real.evaluate(self._real.warp_points(X, *self._box()), *args, **kwargs)

    def acq_grad(self, X, *args, **kwargs):
        lo, hi, a, b = self._box()
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        W, du, _, _ = self._real.warp_points(X, lo, hi, a, b, derivatives=True)
        if not np.all(np.isfinite(du)):
            # a point ON a wall where the warp's slope is infinite (a < 1 at lo, b < 1 at hi): SciPy's L-BFGS-B, which walks in
            # RAW coordinates on this gradient (lockstep='scipy' / False), puts iterates exactly on the bounds as a matter of
            # course and cannot take +-inf.  The slope is taken 2^-40 of the box inside instead: finite, of the right sign,
            # and large -- the projected gradient there is what SciPy reads
            t = (hi - lo) * 2.0 ** -40
            du_in = self._real.warp_points(np.clip(X, lo + t, hi - t), lo, hi, a, b, derivatives=True)[1]
            du = np.where(np.isfinite(du), du, du_in)
        v, g = self._real.acq_grad(W, *args, **kwargs)
        return v, g * (du / (hi - lo))                               # raw coordinates: dw/dx = dw/du / (hi - lo)

    def acq_refine(self, X0, lo, hi, *args, **kwargs):
        """the gradient stage in warped coordinates on the unit box; lo / hi (the raw box) only clip the starts"""
        blo, bhi, a, b = self._box()
        D = len(blo)
        W0 = self._real.warp_points(np.clip(np.atleast_2d(X0), lo, hi), blo, bhi, a, b)
        w, v, status, its = self._real.acq_refine(W0, np.zeros(D), np.ones(D), *args, **kwargs)
        return self._real.warp_inverse(w, blo, bhi, a, b), v, status, its


class WarpedModel(HipGPSurrogate.ModelInstance):
    """A GP fitted to w(X).  Holds the RAW X, y, the kernel and the warp (that is what pickles); ``predict`` and every
    acquisition over it take raw points.  Predicts through the host backend where no GPU is visible, as its parent does."""
    is_warped = True

    def __init__(self, factory, X, y, kernel, jitter, normalize_y, lo, hi, a, b):
        super().__init__(factory, X, y, kernel, jitter, normalize_y)
        self.warp_lo, self.warp_hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
        self.warp_a, self.warp_b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)

    def warp(self, X):
        """w(X) for raw points X (m, D)"""
        return self._factory._context().warp_points(np.atleast_2d(np.asarray(X, dtype=np.float64)), self.warp_lo, self.warp_hi,
                                                    self.warp_a, self.warp_b)

    def _ensure_resident(self):
        f = self._factory
        ctx = f._context()
        if f._resident is not self:
            k = self.kernel
            if np.ndim(k.length_scale) > 0:
                assert len(k.length_scale) == self.X.shape[1], 'anisotropic length scale needs one entry per dimension'
            if hasattr(ctx, 'set_overlap') and not getattr(ctx, 'host', False):
                ctx.set_overlap(0)
            # (no one-row extension: another warp moves every row of w(X))
            lml, ym, ys = ctx.fit(self.warp(self.X), self.y, k.kind, k.constant, k.length_scale, k.noise_level, self.jitter,
                                  self.normalize_y, append=False)
            self.appended = False
            self.log_likelihood, self.y_mean, self.y_std = lml, ym, ys
            self.fit_ms = ctx.profile_read()['last_fit_ms']
            f._resident = self
        return _WarpedContext(ctx, self)

    def _points(self, X):
        return self.warp(super()._points(X))

    def value_and_grad(self, X, acq, sf, incumbent, param):
        """acquisition values (m,) and gradients (m, D) in RAW coordinates: the native gradient times dw/dx"""
        return self._ensure_resident().acq_grad(np.atleast_2d(np.asarray(X, dtype=np.float64)), acq, sf, incumbent, param)

    def get_hyper_params(self):
        return np.hstack([self.kernel.hyper_params(), self.warp_a, self.warp_b])

    def get_hyper_param_names(self):
        D = len(self.warp_a)
        return self.kernel.hyper_param_names() + ['warp_a_%d' % d for d in range(D)] + ['warp_b_%d' % d for d in range(D)]


class WarpedHipGPSurrogate(HipGPSurrogate):
    """``HipGPSurrogate`` with a learned Kumaraswamy warp of every input dimension.

    Args (beyond the parent's):
        bounds: the latent box the warp maps to the unit cube: a ``Bounds`` (anything with ``.ordered``) or a (D, 2) array
        warp_bounds: (low, high) of every shape parameter a_d, b_d; (1, 1) keeps the identity warp
        warp_prior_sigma: width of the log-normal prior on a_d and b_d, centred on the identity warp, that the fit adds to
            the minimised objective (sum of log(shape)^2 / (2 sigma^2)); 0: none.  The default 0.5 is a MODELLING choice
            -- a shape beyond e^(+-1) should be paid for by the data -- not a measurement.

    ``construct_model`` optimises kernel and warp together: ``tgp_fit_warp_lbfgsb`` by default, SciPy's L-BFGS-B driving
    ``tgp_fit_warp_grad`` with ``optimizer='scipy'``.  With ``training_iterations=0`` (or ``optimizer=None``) the current
    warp is kept; ``param_continuity`` carries warp and kernel from trial to trial as the parent carries the kernel.
    Returns a ``WarpedModel``; ``fitting_info`` gains ``warp_a`` and ``warp_b``."""

    def predict_many(self, models, X, return_std_dev=False):
        """``[m.predict(X, return_std_dev) for m in models]``, model by model: the parent's batched route hands the library
        every model's X and the grid as they are, and a warped model's are RAW while its length scales are in warped units
        -- each model has a warp of its own to put both through first"""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        out = [m.predict(X, return_std_dev) for m in models]
        if not return_std_dev:
            return np.array(out, dtype=np.float64).reshape(len(models), X.shape[0])
        return (np.array([o[0] for o in out], dtype=np.float64).reshape(len(models), X.shape[0]),
                np.array([o[1] for o in out], dtype=np.float64).reshape(len(models), X.shape[0]))

    def __init__(self, bounds, *args, warp_bounds=(0.25, 4.0), warp_prior_sigma=0.5, **kwargs):
        super().__init__(*args, **kwargs)
        if self.criterion != 'lml':
            raise ValueError("a warped surrogate maximises the log marginal likelihood: criterion='lml' only")
        box = np.array([(lb[1], lb[2]) for lb in bounds.ordered] if hasattr(bounds, 'ordered') else bounds, dtype=np.float64).reshape(-1, 2)
        if not (np.all(np.isfinite(box)) and np.all(box[:, 1] > box[:, 0])):
            raise ValueError('bounds must be finite with high > low in every dimension')
        self.warp_lo, self.warp_hi = box[:, 0].copy(), box[:, 1].copy()
        lo, hi = float(warp_bounds[0]), float(warp_bounds[1])
        if not (0.0 < lo <= 1.0 <= hi and np.isfinite(hi)):
            raise ValueError('warp_bounds must be finite with 0 < low <= 1 <= high (the identity warp lies inside)')
        if not (np.isfinite(warp_prior_sigma) and warp_prior_sigma >= 0.0):
            raise ValueError('warp_prior_sigma must be finite and >= 0')
        self.warp_bounds = (lo, hi)
        self.warp_prior_sigma = float(warp_prior_sigma)
        D = len(self.warp_lo)
        self.warp_a, self.warp_b = np.ones(D), np.ones(D)       # the current warp

    def construct_model(self, trial_num, X, y):
        iterations = self._get_training_iterations(trial_num)
        fitting_info = {'iterations': iterations}
        assert 'kernel' in self.model_params, 'you must specify a kernel for the GP'
        kernel = GPKernel.from_any(self.model_params['kernel']).copy()
        optimizer = self.model_params.get('optimizer', 'fmin_l_bfgs_b')
        jitter = self.model_params.get('alpha', 1e-10)
        assert np.isscalar(jitter), 'only a scalar alpha is supported'
        normalize_y = bool(self.model_params.get('normalize_y', False))
        if self.param_continuity and self._last_model_params is not None:
            kernel.theta = np.log(self._last_model_params.copy())
        X = np.array(X, dtype=np.float64, copy=True, order='C')
        y = np.array(y, dtype=np.float64, copy=True).reshape(-1)
        assert X.ndim == 2 and X.shape[0] == y.shape[0], 'X must be (N, D) and y (N,)'
        assert X.shape[1] == len(self.warp_lo), 'X must have one column per dimension of the bounds'
        if kernel.anisotropic:
            assert len(kernel.length_scale) == X.shape[1], 'anisotropic length scale needs one entry per dimension'
        a, b = (self.warp_a.copy(), self.warp_b.copy()) if self.param_continuity else (np.ones(X.shape[1]), np.ones(X.shape[1]))
        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter('always')
            trained = iterations > 0 and optimizer is not None
            if trained:
                evals, a, b = self._optimise_warped(kernel, a, b, X, y, float(jitter), normalize_y, optimizer, iterations - 1)
                fitting_info.update({'lml_evaluations': evals})
            elif iterations == 0:
                fitting_info.update({'fixed': kernel.theta})
            model = WarpedModel(self, X, y, kernel, float(jitter), normalize_y, self.warp_lo, self.warp_hi, a, b)
            model._ensure_resident()
        if len(ws) > 0:
            fitting_info.update({'warnings': [w.message for w in ws]})
        if trained:
            self._last_model_params = np.exp(kernel.theta.copy()) if len(kernel.theta) else None
            self.warp_a, self.warp_b = a.copy(), b.copy()
        fitting_info.update({'fit_ms': model.fit_ms, 'warp_a': a.copy(), 'warp_b': b.copy()})
        return model, fitting_info

    def _optimise_warped(self, kernel, a, b, X, y, jitter, normalize_y, optimizer, n_restarts):
        """minimise -LML + the warp's prior over [theta (the kernel's free entries), log a, log b]; leaves the best theta
        in ``kernel`` and returns (objective evaluations, a, b).  The library's vector is log(constant, length scale(s),
        noise, a, b) in full; a FIXED kernel entry travels with lo == hi, as in the parent's fit."""
        D = X.shape[1]
        n_ls = len(kernel.length_scale) if kernel.anisotropic else 1
        P0 = 2 + n_ls
        bounds = kernel.theta_bounds
        if (kernel.noise is not None and not kernel.noise > 0) or (len(bounds) and not np.isfinite(bounds).all()):
            raise ValueError('a warped fit needs finite bounds on every free hyper-parameter and a noise term that is > 0 or absent')
        free = np.asarray(kernel.select_gradient(np.arange(P0, dtype=np.float64)), dtype=np.int64)
        with np.errstate(divide='ignore'):
            full = np.concatenate([np.log(np.concatenate([[kernel.constant], np.atleast_1d(np.asarray(kernel.length_scale, dtype=np.float64)),
                                                          [kernel.noise_level]])), np.log(a), np.log(b)])
        wb = np.log(self.warp_bounds)
        full_bounds = np.stack([full, full], axis=1)
        if len(free):
            full_bounds[free] = bounds
        full_bounds[P0:] = wb
        full[P0:] = np.clip(full[P0:], wb[0], wb[1])
        starts = np.tile(full, (1 + n_restarts, 1))
        if n_restarts > 0:
            rng = self._rng()
            for j in range(1, 1 + n_restarts):      # the kernel's entries as scikit-learn draws them; the warp starts where it stands
                if len(free):
                    starts[j, free] = rng.uniform(bounds[:, 0], bounds[:, 1])
        ctx = self._context()
        self._resident = None
        sigma = self.warp_prior_sigma
        if optimizer in ('fmin_l_bfgs_b', 'device'):
            theta, f, status, evals = ctx.fit_warp_optimise(X, y, kernel.kind, self.warp_lo, self.warp_hi, starts, n_ls, full_bounds,
                                                            jitter, normalize_y, prior_sigma=sigma, max_iter=15000)
            for st in status:
                if st != 1:
                    warnings.warn('lbfgs failed to converge (status={})'.format(1 if st == 0 else 2))
            f = np.where(np.isfinite(f), f, np.inf)
            best = theta[int(np.argmin(f))]
        elif optimizer == 'scipy' or callable(optimizer):
            import scipy.optimize
            moving = np.nonzero(full_bounds[:, 0] < full_bounds[:, 1])[0]
            count = [0]

            def obj(x, eval_gradient=True):
                th = full.copy()
                th[moving] = x
                count[0] += 1
                # (the C library's exp, entry by entry, as GPKernel.theta takes it: the library's own walk hands the GPU these bits)
                ex = np.array([_exp_like_numpy(t) for t in th], dtype=np.float64)
                ls = ex[1:1 + n_ls]
                try:
                    lml, grad = ctx.fit_warp_grad(X, y, kernel.kind, ex[0], ls if kernel.anisotropic else float(ls[0]),
                                                  ex[1 + n_ls], jitter, normalize_y, self.warp_lo, self.warp_hi,
                                                  ex[P0:P0 + D], ex[P0 + D:])
                except np.linalg.LinAlgError:
                    return (np.inf, np.zeros_like(x)) if eval_gradient else np.inf
                fval, g = -lml, -grad
                if sigma > 0:
                    wfree = moving[moving >= P0]
                    fval += 0.5 * float((th[wfree] ** 2).sum()) / sigma ** 2
                    g[wfree] += th[wfree] / sigma ** 2
                return (fval, g[moving]) if eval_gradient else fval

            optima = []
            for s in starts:
                if callable(optimizer):
                    optima.append(optimizer(obj, s[moving], bounds=full_bounds[moving]))
                else:
                    res = scipy.optimize.minimize(obj, s[moving], method='L-BFGS-B', jac=True, bounds=full_bounds[moving])
                    if res.status != 0:
                        warnings.warn('lbfgs failed to converge (status={}): {}'.format(res.status, res.message))
                    optima.append((res.x, res.fun))
            best = full.copy()
            best[moving] = optima[int(np.argmin([o[1] for o in optima]))][0]
            evals = count[0]
        else:
            raise ValueError('Unknown optimizer {}.'.format(optimizer))
        if len(free):
            kernel.theta = best[free]
        shapes = np.array([_exp_like_numpy(t) for t in best[P0:]], dtype=np.float64)
        return int(evals), shapes[:D], shapes[D:]
