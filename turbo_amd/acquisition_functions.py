"""Acquisition-function plugins evaluated on the GPU, fused with the posterior sweep.

Mirror of the reference's factories and function instances
(turbo/modules/acquisition_functions.py): ``AcquisitionFunction`` :12-77, ``UCB`` :80-158,
``PI`` :163-247, ``EI`` :250-358 -- same constructor arguments, ``get_type()``,
``construct_function(trial_num, model, desired_extremum[, incumbent_cost])``, ``get_name()`` and
``__call__(X (M, D)) -> (M,)``.  With a native model (``HipGPSurrogate.ModelInstance``) mean, variance
and the acquisition value are produced by one pass of the HIP kernels.  A FOREIGN model -- any other
``Surrogate.ModelInstance`` of the reference, e.g. its ``SciKitGPSurrogate`` -- is served as the reference
serves it: ``model.predict(X, return_std_dev=True)`` and the formula in NumPy
(``_from_mu_sigma`` below; interoperability only -- a native model never takes that route, and the
GPU-only extras ``maximise_topk`` / ``refine`` / ``value_and_grad`` / ``maximise_generated`` refuse it).

Beyond the reference interface each instance has ``maximise(X) -> (index, value)``, which the
``CandidateSweep`` auxiliary optimiser uses to get the arg-max without copying M values back.
"""
import uuid
from math import isinf

import numpy as np

from . import _lib


def _is_native(model):
    return hasattr(model, '_sweep')


def _is_marginalised(model):
    """a ``MarginalisedModel``: its ``_sweep`` is the integrated sweep (``tgp_sweep_integrated``), so ``__call__`` and
    ``maximise`` of UCB / PI / EI over it ARE the integrated acquisition; what works on one fitted model refuses it"""
    return bool(getattr(model, 'is_marginalised', False))


def _refuse_marginalised(model, what):
    if _is_marginalised(model):
        raise ValueError('{} is not available for a marginalised model (hyper-parameter samples): it works on one '
                         'fitted model'.format(what))


def _refuse_warped(model, what):
    """a ``WarpedModel`` (turbo_amd/warped.py) serves UCB / PI / EI over one batch or a gradient stage: the rest is refused"""
    if getattr(model, 'is_warped', False):
        raise ValueError('{} is not available for a warped model (WarpedHipGPSurrogate): input warping serves UCB / PI / EI '
                         'through CandidateSweep and RandomAndQuasiNewton on one GPU'.format(what))


def _require_native(model, what):
    _refuse_marginalised(model, what)
    if not _is_native(model):
        raise TypeError('{} needs a model built by HipGPSurrogate (got {!r}): it runs on the GPU only'
                        .format(what, type(model)))


GOLDEN = 0x9E3779B97F4A7C15


def _trial_seed(seed, trial_num):
    """the seed trial ``trial_num`` draws with (TS, MES): ``(seed + trial_num * GOLDEN) mod 2**64``; ``seed`` None takes
    one ``np.random.randint(0, 2**63)`` from NumPy's global RNG per trial"""
    base = int(np.random.randint(0, 2**63)) if seed is None else int(seed)
    return (base + int(trial_num) * GOLDEN) % (1 << 64)


def _checked_n_features(n_features):
    n_features = int(n_features)
    if n_features < 64 or n_features > 16384 or n_features % 64 != 0:
        raise ValueError('n_features must be a multiple of 64 in [64, 16384]')
    return n_features


def topk_tail(idx, vals, ranked_only=False):
    """a top-k as the library fills it (index -1 where nothing ranked; ``ranked_only``: those slots are gone already) ->
    (top = (indices, values) of the ranked slots, the winner's index, its value); nothing ranked (an all-NaN batch):
    index 0 and -inf, as ``maximise`` reports it"""
    if not ranked_only:
        keep = idx >= 0
        idx, vals = idx[keep], vals[keep]
    if len(idx) > 0:
        return (idx, vals), int(idx[0]), float(vals[0])
    return (idx, vals), 0, -np.inf


def _from_mu_sigma(acq, sf, incumbent, param, mu, sigma):
    """UCB / PI / EI / sigma from a foreign model's posterior, float64 on the host
    (turbo/modules/acquisition_functions.py:147-158, :225-247, :336-358):
        UCB  sf mu + beta sigma                       (ACQ_SIGMA, i.e. beta = inf: sigma alone)
        PI   Phi(z),                z = (sf (mu - f+) - xi) / sigma
        EI   (sigma z) Phi(z) + sigma phi(z)          both 0 wherever sigma == 0"""
    from scipy.special import ndtr
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    if acq == _lib.ACQ_SIGMA:
        return sigma
    if acq == _lib.ACQ_UCB:
        return sf * mu + param * sigma
    out = np.zeros_like(mu)
    live = np.nonzero(sigma != 0)[0]
    s = sigma[live]
    gain = sf * (mu[live] - incumbent) - param
    z = gain / s
    if acq == _lib.ACQ_PI:
        out[live] = ndtr(z)
    else:
        out[live] = gain * ndtr(z) + s * (np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi))
    return out


class AcquisitionFunction:
    """factory interface, turbo/modules/acquisition_functions.py:12-77"""

    def get_type(self):
        raise NotImplementedError()

    def construct_function(self, trial_num, model, desired_extremum, *args):
        raise NotImplementedError()

    class FunctionInstance:
        def __init__(self, model, desired_extremum):
            assert _is_native(model) or hasattr(model, 'predict'), 'not a Surrogate.ModelInstance: {!r}'.format(type(model))
            self.model = model
            assert desired_extremum in ('min', 'max')
            self.desired_extremum = desired_extremum
            self.scale_factor = 1 if desired_extremum == 'max' else -1

        def get_name(self):
            raise NotImplementedError()

        def _native_args(self):
            """(acq enum, incumbent, param)"""
            raise NotImplementedError()

        def _prepare(self, X=None):
            """Hook: called by every method below once the model is known to be native and before the library sweeps,
            evaluates or refines -- X: the points about to be handed over, None: the batch already resident.  Returns X
            as the method is to pass it on.  Nothing to do here; ``MES`` puts its maxima into the context."""
            return X

        def __call__(self, X):
            acq, incumbent, param = self._native_args()
            if not _is_native(self.model):
                mu, sigma = self.model.predict(X, return_std_dev=True)
                return _from_mu_sigma(acq, self.scale_factor, incumbent, param, mu, sigma)
            if np.size(X) > 0:      # (an empty batch has nothing to prepare for: empty results, nothing launched)
                X = self._prepare(X)
            res = self.model._sweep(X, acq, self.scale_factor, incumbent, param, want_acq=True,
                                    want_sigma=False)
            return res['acq']

        last_sweep_ms = None      # device time of the last maximise* call (hipEvents around the sweep)

        @property
        def sweep_dtype(self):
            """arithmetic of the model's candidate sweep: 'f64', or 'f32' / 'f32h2' / 'f32x3' (a foreign model: 'f64').
            Models of up to 256 points are ALWAYS swept in f64, whatever the factory's dtype: the one-workgroup kernels
            for N <= 128 and the one-launch sweep for 128 < N <= 256 (csrc/small_kernels.hip) only exist in f64 -- an
            upgrade, never a loss, and the caller need not re-form the winner's value in f64."""
            factory = getattr(self.model, '_factory', None)
            dtype = getattr(factory, 'dtype', 'f64')
            if dtype == 'f64':
                return 'f64'
            # the LIBRARY says which kernels the last sweep took (tgp_last_timings slot 6): the size rule alone is not the
            # whole condition -- TGP_SMALL=0 / TGP_MID=0, a device without the one-launch sweep's LDS opt-in, or a model
            # another one displaced send a small model down the general sweep in the handle's arithmetic
            ctx = getattr(factory, '_native', None)
            if ctx is not None and getattr(factory, '_resident', None) is self.model and hasattr(ctx, 'last_timings') \
                    and not getattr(ctx, 'host', False):
                f64 = ctx.last_timings().get('sweep_f64', -1)
                if f64 >= 0:
                    return 'f64' if f64 else dtype
            n_obs = getattr(getattr(self.model, 'X', None), 'shape', (1 << 30,))[0]
            return 'f64' if n_obs <= 256 else dtype

        def maximise(self, X):
            """arg-max over the rows of X: (index, value); lowest index wins ties"""
            acq, incumbent, param = self._native_args()
            if not _is_native(self.model):
                vals = self(X)
                vals = np.where(np.isnan(vals), -np.inf, vals)      # NaN never wins, as on the GPU
                i = int(np.argmax(vals))                            # first maximum = lowest index
                return i, float(vals[i])
            res = self.model._sweep(self._prepare(X), acq, self.scale_factor, incumbent, param)
            self.last_sweep_ms = res.get('sweep_ms')
            return res['best_idx'], res['best_val']

        def maximise_topk(self, X, k):
            """the k best rows of X: (indices (k,), values (k,)), best first, lowest index on ties;
            the (M,) acquisition vector stays on the GPU (``tgp_sweep_topk``)"""
            _require_native(self.model, 'maximise_topk')
            acq, incumbent, param = self._native_args()
            X = self._prepare(X)
            ctx = self.model._ensure_resident()
            ctx.set_candidates(X)
            return topk_tail(*ctx.sweep_topk(min(int(k), 64), acq, self.scale_factor, incumbent, param))[0]

        BATCH_STRATEGIES = {'kriging_believer': _lib.BATCH_KB, 'constant_liar': _lib.BATCH_CL}

        def maximise_batch(self, X, q, strategy='kriging_believer', lie='min', pending=None, want_posterior=False,
                           n_sim=16, seed=None):
            """q rows of X chosen greedily for q parallel workers (``tgp_sweep_batch``), conditioned first on the
            ``pending`` points (P, D) -- trials still under evaluation.  Every chosen or pending point is given a
            fantasy value -- 'kriging_believer': the posterior mean there; 'constant_liar': ``lie``, a float in raw y
            units or 'min' / 'max' / 'mean' of the model's observed y -- and the model is conditioned on it with the
            hyper-parameters held (old_library/bayesian_optimiser.py:76-103, :527-566).  X None: the batch already
            resident on the model's GPU context.  Returns the dict of ``NativeGP.sweep_batch`` (idx, val, x, fantasies,
            mu, sigma, n_clamped, sweep_ms).

            'monte_carlo' (``tgp_sweep_batch_mc``; old_library/bayesian_optimiser.py:568-624): ``n_sim`` <= 64
            simulations of the pending and chosen points' outcomes, drawn jointly from the model, and the AVERAGE of
            the acquisition over them maximised.  ``seed`` keys the fantasies' random numbers; None takes one
            ``np.random.randint(0, 2**63)`` from NumPy's global RNG, as ``TS`` does.  Returns the dict of
            ``NativeGP.sweep_batch_mc`` (fantasies (n_sim, P + q)) plus n_sim and seed; ``lie`` is not used and
            ``want_posterior`` asks for sigma alone (the S means differ).  The other strategies ignore ``n_sim`` and
            ``seed``."""
            _refuse_marginalised(self.model, 'maximise_batch')
            _refuse_warped(self.model, 'maximise_batch')
            if not _is_native(self.model):
                raise NotImplementedError('maximise_batch runs on the GPU only: it needs a model built by HipGPSurrogate '
                                          '(got {!r})'.format(type(self.model)))
            if strategy != 'monte_carlo' and strategy not in self.BATCH_STRATEGIES:
                raise ValueError('strategy must be one of {}'.format(sorted(list(self.BATCH_STRATEGIES) + ['monte_carlo'])))
            acq, incumbent, param = self._native_args()
            monte_carlo, lie_value = strategy == 'monte_carlo', 0.0
            if monte_carlo:
                n_sim = int(n_sim)
                if n_sim < 1 or n_sim > 64:
                    raise ValueError('n_sim must be in [1, 64]')
                seed = int(np.random.randint(0, 2**63)) if seed is None else int(seed) % (1 << 64)
            elif strategy == 'constant_liar':
                y = np.asarray(self.model.y, dtype=np.float64)
                if isinstance(lie, str):
                    if lie not in ('min', 'max', 'mean'):
                        raise ValueError("lie must be a float or one of 'min', 'max', 'mean'")
                    lie_value = float(getattr(np, lie)(y))
                else:
                    lie_value = float(lie)
            ctx = self.model._ensure_resident()
            if X is not None:
                ctx.set_candidates(np.asarray(X, dtype=np.float64))
            if monte_carlo:
                res = ctx.sweep_batch_mc(q, n_sim, seed, None, pending, acq, self.scale_factor, incumbent, param,
                                         want_sigma=want_posterior)
                res['n_sim'], res['seed'] = n_sim, seed
            else:
                res = ctx.sweep_batch(q, self.BATCH_STRATEGIES[strategy], lie_value, pending, acq, self.scale_factor,
                                      incumbent, param, want_posterior=want_posterior)
                res['lie'] = lie_value if strategy == 'constant_liar' else None
            self.last_sweep_ms = res.get('sweep_ms')
            return res

        def refine(self, starting_points, bounds, max_iter=200):
            """the gradient stage on the GPU (``tgp_acq_refine``): every restart refined by a projected
            L-BFGS, together (N <= 128: each in its own workgroup of one launch); returns
            (x (R, D), values (R,), evaluations of the slowest restart)"""
            _require_native(self.model, 'refine')
            import warnings
            acq, incumbent, param = self._native_args()
            ctx = self.model._ensure_resident()
            low, high = zip(*bounds)
            x, v, status, its = ctx.acq_refine(starting_points, low, high, acq, self.scale_factor,
                                               incumbent, param, max_iter)
            for j in np.nonzero(status == 0)[0]:
                warnings.warn('restart {} of the on-device optimisation stopped at max_iter'.format(j))
            return x, v, its

        def lbfgsb(self, starting_points, bounds, max_iter=15000):
            """the gradient stage as the reference runs it -- SciPy's L-BFGS-B from every start
            (turbo/modules/auxiliary_optimisers.py:80-99) -- inside the library (``tgp_acq_lbfgsb``): the restarts in
            lock-step, one batched closed-form value + gradient evaluation per round; returns
            (x (R, D), values (R,), status (R,): 1 = SciPy's success, evaluations)"""
            _require_native(self.model, 'lbfgsb')
            acq, incumbent, param = self._native_args()
            self._prepare(starting_points)
            ctx = self.model._ensure_resident()
            low, high = zip(*bounds)
            return ctx.acq_refine(starting_points, low, high, acq, self.scale_factor, incumbent, param, max_iter,
                                  lbfgsb=True)

        def winner_record(self, global_offset):
            """Attach a device-resident (D + 2,) float64 record to the model's GPU context: every
            later sweep packs [best value, global_offset + best index, candidate row] into it on
            the GPU (``tgp_set_winner_out``).  Returns the torch tensor that owns the memory -- the
            input of the sharded arg-max's all-gather over RCCL."""
            import torch
            if _is_marginalised(self.model):     # tgp_sweep_integrated packs the record as a plain sweep does
                ctx = self.model._resident_context()
            else:
                _refuse_warped(self.model, 'winner_record (the sharded multi-GPU sweep)')
                _require_native(self.model, 'winner_record')
                ctx = self.model._ensure_resident()
            D = self.model.X.shape[1]
            rec = getattr(ctx, '_winner_keepalive', None)
            if rec is None or rec.numel() != D + 2:
                rec = torch.zeros(D + 2, dtype=torch.float64, device='cuda:%d' % ctx.device)
            ctx.set_winner_out(rec.data_ptr(), global_offset, keepalive=rec)
            return rec

        def value_and_grad(self, X):
            """acquisition values (m,) and their gradients (m, D) at a small batch of points,
            in closed form on the GPU (the reference differentiates 1-point calls by finite
            differences: turbo/modules/auxiliary_optimisers.py:80-92)"""
            acq, incumbent, param = self._native_args()
            if _is_marginalised(self.model):      # the mean of the samples' closed forms
                return self.model.value_and_grad(X, acq, self.scale_factor, incumbent, param)
            _require_native(self.model, 'value_and_grad')
            X = self._prepare(X)
            ctx = self.model._ensure_resident()
            return ctx.acq_grad(X, acq, self.scale_factor, incumbent, param)

        def maximise_host_stream(self, num_points, low, high, topk=0, first=0, count=None):
            """The reference's HOST draw (``random_selector``: NumPy's global RNG, a column per parameter) made resident
            without forming the batch on the host (``tgp_set_candidates_mt19937``: the generator's sequential part in
            the library, the doubles on the GPU; ``np.random`` ends where NumPy's own calls would leave it), then swept.
            Returns None -- nothing drawn -- where the library cannot promise NumPy's numbers; otherwise
            ``(ctx, best_index, best_value, top)`` with ``top = (indices, values)`` of the ``topk`` best (None for 0);
            rows of the batch come from ``ctx.get_candidate``.  ``first`` / ``count``: only rows [first, first + count) of
            the ``num_points``-row batch are kept and swept (a rank's shard; indices are local to it) while ``np.random``
            ends behind the whole batch."""
            if not _is_native(self.model) or _is_marginalised(self.model):
                return None
            acq, incumbent, param = self._native_args()
            ctx = self.model._ensure_resident()
            if not hasattr(ctx, 'set_candidates_numpy_stream') or not ctx.set_candidates_numpy_stream(num_points, low, high, first=first, count=count):
                return None
            self._prepare(None)
            if topk > 0:
                top, best_i, best_y = topk_tail(*ctx.sweep_topk(min(int(topk), 64), acq, self.scale_factor, incumbent, param))
                return ctx, best_i, best_y, top
            res = ctx.sweep(acq, self.scale_factor, incumbent, param)
            self.last_sweep_ms = res.get('sweep_ms')
            return ctx, res['best_idx'], res['best_val'], None

        def maximise_generated(self, num_points, low, high, seed, first_candidate=0, lhs_total=None, prefetch_seed=None):
            """draw `num_points` candidates in [low, high) on the GPU -- independent uniform ones, or
            (lhs_total given) rows first_candidate.. of an lhs_total-point Latin hypercube design --
            and return the best: (x (D,), value, index).  Candidates never cross PCIe.

            ``prefetch_seed``: after this sweep, draw the batch of the NEXT call (same shape, that seed) right away and
            arm ``tgp_set_overlap``: the candidates do not depend on the model, so the next trial's fit
            (turbo/optimiser.py:336) starts their sweep inside itself -- candidate scaling, cross-kernel and the first
            row tiles of the contraction beside the Cholesky's panel chain -- and the next call of this method finds
            the batch resident and skips the draw.  Same candidates, same values, same winner as without it."""
            acq, incumbent, param = self._native_args()
            marginalised = _is_marginalised(self.model)
            if marginalised:
                if prefetch_seed is not None:
                    raise ValueError('prefetch_next is not available for a marginalised model (every sample refits)')
                ctx = self.model._resident_context()
            else:
                _require_native(self.model, 'maximise_generated')
                ctx = self.model._ensure_resident()
            # (resident already when the previous call prefetched it)
            ctx.generate(seed, first_candidate, num_points, low, high, lhs_total, reuse=True)
            if marginalised:      # the resident batch under every hyper-parameter sample (tgp_sweep_integrated)
                res = self.model._integrated(ctx, acq, self.scale_factor, incumbent, param, False, False, False)
                return ctx.get_candidate(res['best_idx']), res['best_val'], res['best_idx']
            res = ctx.sweep(acq, self.scale_factor, incumbent, param)
            self.last_sweep_ms = res.get('sweep_ms')
            best = ctx.get_candidate(res['best_idx']), res['best_val'], res['best_idx']
            if prefetch_seed is not None and hasattr(ctx, 'set_overlap') and not getattr(ctx, 'host', False):
                ctx.generate(prefetch_seed, first_candidate, num_points, low, high, lhs_total)
                ctx.prefetched = True     # ModelInstance._ensure_resident arms tgp_set_overlap for the next fit
            return best


class UCB(AcquisitionFunction):
    def __init__(self, beta):
        """beta: a constant float or a function of the trial number (:81-87)"""
        self.beta = beta

    def get_type(self):
        return 'optimism'

    def construct_function(self, trial_num, model, desired_extremum):
        beta = self.beta(trial_num) if callable(self.beta) else self.beta
        acq_info = {'beta': beta}
        return UCB.FunctionInstance(model, desired_extremum, beta), acq_info

    class FunctionInstance(AcquisitionFunction.FunctionInstance):
        """sf * mu + beta * sigma;  beta = inf -> sigma  (:147-158)"""

        def __init__(self, model, desired_extremum, beta):
            super().__init__(model, desired_extremum)
            self.beta = beta

        def get_name(self):
            return 'UCB' if self.desired_extremum == 'max' else '-LCB'

        def _native_args(self):
            if isinf(self.beta):
                return _lib.ACQ_SIGMA, 0.0, 0.0
            return _lib.ACQ_UCB, 0.0, self.beta


class _Improvement(AcquisitionFunction):
    """PI and EI: xi (a constant float or a function of the trial number) against the incumbent's cost"""

    def __init__(self, xi):
        self.xi = xi

    def get_type(self):
        return 'improvement'

    def construct_function(self, trial_num, model, desired_extremum, incumbent_cost):
        xi = self.xi(trial_num) if callable(self.xi) else self.xi
        acq_info = {'xi': xi}
        return self.FunctionInstance(model, desired_extremum, incumbent_cost, xi), acq_info

    class FunctionInstance(AcquisitionFunction.FunctionInstance):
        NAME = ACQ = None       # what PI.FunctionInstance and EI.FunctionInstance differ in

        def __init__(self, model, desired_extremum, incumbent_cost, xi):
            super().__init__(model, desired_extremum)
            self.incumbent_cost = incumbent_cost
            self.xi = xi

        def get_name(self):
            return self.NAME

        def _native_args(self):
            return self.ACQ, self.incumbent_cost, self.xi


class PI(_Improvement):
    """xi: a constant float or a function of the trial number (:164-170)"""

    class FunctionInstance(_Improvement.FunctionInstance):
        """Phi((sf * (mu - f+) - xi) / sigma), 0 where sigma == 0  (:225-247)"""
        NAME, ACQ = 'PI', _lib.ACQ_PI


class EI(_Improvement):
    """xi: a constant float or a function of the trial number (:251-257)"""

    class FunctionInstance(_Improvement.FunctionInstance):
        """diff * Phi(Z) + sigma * phi(Z), 0 where sigma == 0  (:336-358)"""
        NAME, ACQ = 'EI', _lib.ACQ_EI


class TS(AcquisitionFunction):
    """Thompson sampling: maximise ONE sample path of the GP posterior, drawn on the GPU (``tgp_ts_draw``).

    The author's older library names this acquisition (old_library/bayesian_optimiser.py:137-138, :263-264) and its
    'asyTS' batch strategy (:102-104) but leaves both as ``raise NotImplementedError()``.  A path is drawn by pathwise
    conditioning with ``n_features`` random Fourier features (csrc/ts_kernels.hip): a sample of the latent function,
    whose mean is the posterior mean.  Trial ``trial_num`` draws with seed ``(seed + trial_num * 0x9E3779B97F4A7C15) mod
    2**64``; ``seed=None`` takes one ``np.random.randint(0, 2**63)`` from NumPy's global RNG per trial, so a seeded run
    stays reproducible."""

    GOLDEN = GOLDEN

    def __init__(self, seed=None, n_features=2048):
        self.n_features = _checked_n_features(n_features)
        self.seed = seed

    def get_type(self):
        return 'optimism'

    def construct_function(self, trial_num, model, desired_extremum):
        _refuse_warped(model, 'TS')
        _refuse_marginalised(model, 'TS (a sample path belongs to one fitted model)')
        if not _is_native(model):
            raise NotImplementedError('TS draws its sample paths on the GPU: it needs a model built by HipGPSurrogate '
                                      '(got {!r})'.format(type(model)))
        seed = _trial_seed(self.seed, trial_num)
        acq_info = {'seed': seed, 'n_features': self.n_features}
        return TS.FunctionInstance(model, desired_extremum, seed, self.n_features), acq_info

    class FunctionInstance(AcquisitionFunction.FunctionInstance):
        """sf * (the sampled path's raw value): sample 0 of the draw with this instance's seed"""

        is_thompson = True
        sweep_dtype = 'f64'      # every Thompson entry is f64 whatever the handle's dtype

        def __init__(self, model, desired_extremum, seed, n_features):
            super().__init__(model, desired_extremum)
            self.seed = int(seed)
            self.n_features = int(n_features)
            self._token = object()

        def get_name(self):
            return 'TS'

        def _native_args(self):
            raise NotImplementedError('TS has no posterior-formula arguments: it maximises a sampled path')

        def _ctx(self, S=1):
            """the model's context holding THIS instance's draw of S paths (drawn again after any refit: the same seed
            gives the same paths)"""
            f = self.model._factory
            refit = f._resident is not self.model
            ctx = self.model._ensure_resident()
            key = (self._token, int(S))
            if refit or getattr(ctx, '_ts_owner', None) != key:
                ctx._ts_owner = None
                ctx.ts_draw(self.seed, S, self.n_features)
                ctx._ts_owner = key
            return ctx

        def _as_points(self, X):
            X = np.asarray(X, dtype=np.float64)
            if X.ndim == 1:
                X = X.reshape(1, -1)
            assert X.ndim == 2 and X.shape[1] == self.model.X.shape[1], \
                'X must have shape (num_points, {})'.format(self.model.X.shape[1])
            return X

        def _values(self, X):
            """raw sampled values at the rows of X"""
            X = self._as_points(X)
            if X.shape[0] == 0:
                return np.empty(0)
            ctx = self._ctx()
            if X.shape[0] <= 64:
                f, _ = ctx.ts_eval(X)
                return f[:, 0]
            ctx.set_candidates(X)
            return ctx.ts_sweep(self.scale_factor, want_f=True)['f'][:, 0]

        def __call__(self, X):
            return self.scale_factor * self._values(X)

        def value_and_grad(self, X):
            """sf * sampled value (m,) and its gradient (m, D) in closed form (``tgp_ts_eval``)"""
            X = self._as_points(X)
            ctx = self._ctx()
            vals, grads = [], []
            for i in range(0, X.shape[0], 4096):
                f, g = ctx.ts_eval(X[i:i + 4096], want_grad=True)
                vals.append(f[:, 0])
                grads.append(g[:, 0, :])
            return self.scale_factor * np.concatenate(vals), self.scale_factor * np.concatenate(grads)

        def maximise(self, X):
            """arg-max of sf * sampled value over the rows of X: (index, value); lowest index wins ties"""
            X = self._as_points(X)
            ctx = self._ctx()
            ctx.set_candidates(X)
            res = ctx.ts_sweep(self.scale_factor)
            self.last_sweep_ms = res.get('sweep_ms')
            return int(res['idx'][0]), self.scale_factor * float(res['val'][0])

        def maximise_topk(self, X, k):
            """the k best rows of X for the sampled path: (indices (k,), values (k,)), best first"""
            v = self(X)
            v = np.where(np.isnan(v), -np.inf, v)
            order = np.argsort(-v, kind='stable')[:min(int(k), 64)]
            return order.astype(np.int64), v[order]

        def maximise_generated(self, num_points, low, high, seed, first_candidate=0, lhs_total=None, prefetch_seed=None):
            """draw ``num_points`` candidates on the GPU (uniform, or rows of an ``lhs_total``-point Latin hypercube) and
            return the sampled path's best: (x (D,), sf * value, index)"""
            if prefetch_seed is not None:
                raise NotImplementedError('TS: no prefetched batch (the overlap starts an EI / UCB sweep inside the fit)')
            ctx = self._ctx()
            ctx.generate(seed, first_candidate, num_points, low, high, lhs_total)
            res = ctx.ts_sweep(self.scale_factor)
            self.last_sweep_ms = res.get('sweep_ms')
            return res['x'][0].copy(), self.scale_factor * float(res['val'][0]), int(res['idx'][0])

        def maximise_host_stream(self, num_points, low, high, topk=0, first=0, count=None):
            return None     # nothing drawn: the caller draws on the host and calls maximise / maximise_topk

        def maximise_batch(self, X, q, strategy='thompson', lie=None, pending=None, want_posterior=False, n_sim=16,
                           seed=None):
            """q distinct rows of X for q parallel workers: row s maximises sample path s of ONE draw of q paths, skipping
            the rows of paths < s (asynchronous Thompson sampling: ``pending`` trials are ignored,
            old_library/bayesian_optimiser.py:102-104).  X None: the batch already resident.  Path 0 is this instance's
            own path, so the first row is ``maximise(X)``'s.  Returns a dict: idx (q,), val (q,) raw sampled values,
            x (q, D), pending_ignored, seed, n_features, sweep_ms"""
            if strategy != 'thompson':
                raise ValueError("a TS acquisition selects batches with strategy='thompson' only")
            q = int(q)
            if q < 1 or q > 64:
                raise ValueError('q must be in [1, 64]')
            ctx = self._ctx(q)
            if X is not None:
                ctx.set_candidates(self._as_points(X))
            res = ctx.ts_sweep(self.scale_factor, distinct=True)
            self.last_sweep_ms = res.get('sweep_ms')
            P = 0 if pending is None else int(np.asarray(pending).reshape(-1, self.model.X.shape[1]).shape[0])
            return dict(idx=res['idx'], val=res['val'], x=res['x'], pending_ignored=P, seed=self.seed,
                        n_features=self.n_features, sweep_ms=res.get('sweep_ms'))

        def _refuse(self, what):
            raise NotImplementedError('TS: {} is not available for sample paths (use CandidateSweep with '
                                      "lockstep='scipy' or lockstep=False for gradient restarts)".format(what))

        def refine(self, starting_points, bounds, max_iter=200):
            self._refuse('the on-device optimiser (on_device=True, tgp_acq_refine)')

        def lbfgsb(self, starting_points, bounds, max_iter=15000):
            self._refuse('the in-library L-BFGS-B (lockstep=True, tgp_acq_lbfgsb)')

        def winner_record(self, global_offset):
            self._refuse('the sharded multi-rank sweep')


class MES(AcquisitionFunction):
    """Max-value entropy search (Wang & Jegelka 2017): the expected reduction of the entropy of the posterior at x from
    knowing the optimum's VALUE y*, averaged over ``n_samples`` <= 64 samples of y* (``TGP_ACQ_MES``, csrc/mes_math.hpp):

        sigma_f^2 = max(sigma^2 - noise y_std^2, 0),   gamma_s = sf (y*_s - mu) / sigma_f
        a(x) = (1/S) sum_s [ gamma_s phi(gamma_s) / (2 Phi(gamma_s)) - log Phi(gamma_s) ],   0 where sigma_f == 0

    The y*_s are the maxima (minima for 'min') of ``n_samples`` posterior sample paths over the batch the instance is
    FIRST asked to maximise or evaluate -- a Thompson draw of ``n_features`` random Fourier features and its sweep
    (``tgp_mes_draw``) -- none worse than the best observed y; they then stay with the instance (and travel with its
    pickle), whatever it is asked afterwards.  Seeds as ``TS``: trial ``trial_num`` draws with
    ``(seed + trial_num * 0x9E3779B97F4A7C15) mod 2**64``, ``seed=None`` takes one ``np.random.randint(0, 2**63)`` per
    trial.  Native models only: the latent deviation needs the model's noise level and the maxima its sample paths, so
    ``construct_function`` raises ``ValueError`` for a foreign model.  ``maximise_batch`` and ``refine`` are refused
    (no MES inside the batch strategies or the one-launch optimiser); an arg-max-only MES sweep is never pruned."""

    def __init__(self, n_samples=8, seed=None, n_features=2048):
        n_samples = int(n_samples)
        if n_samples < 1 or n_samples > 64:
            raise ValueError('n_samples must be in [1, 64]')
        self.n_samples = n_samples
        self.seed = seed
        self.n_features = _checked_n_features(n_features)

    def get_type(self):
        return 'optimism'

    def construct_function(self, trial_num, model, desired_extremum):
        _refuse_warped(model, 'MES')
        _refuse_marginalised(model, 'MES (its maxima belong to one fitted model)')
        if not _is_native(model):
            raise ValueError('MES serves native models only: it needs a model built by HipGPSurrogate (got {!r}) for the '
                             'noise level and the sample paths its maxima come from'.format(type(model)))
        seed = _trial_seed(self.seed, trial_num)
        acq_info = {'seed': seed, 'n_samples': self.n_samples, 'n_features': self.n_features}
        return MES.FunctionInstance(model, desired_extremum, seed, self.n_samples, self.n_features), acq_info

    class FunctionInstance(AcquisitionFunction.FunctionInstance):
        """the S-sample average of h(gamma_s); ``maxima`` (S,) once drawn or given"""

        def __init__(self, model, desired_extremum, seed, n_samples, n_features, maxima=None):
            super().__init__(model, desired_extremum)
            self.seed = int(seed)
            self.n_samples = int(n_samples)
            self.n_features = int(n_features)
            self.maxima = None if maxima is None else np.array(maxima, dtype=np.float64).reshape(-1)
            self._token = object()

        def get_name(self):
            return 'MES'

        def _native_args(self):
            return _lib.ACQ_MES, 0.0, 0.0

        def _as_points(self, X):
            X = np.asarray(X, dtype=np.float64)
            if X.ndim == 1 and X.size > 0:
                X = X.reshape(1, -1)
            return X

        def _prepare(self, X=None):
            """the base class's hook: THIS instance's maxima into the model's context.  First use: they are drawn over X
            (None: the batch already resident).  Later: re-sent only when the handle holds another fit or another
            instance's maxima.  Returns X as points."""
            if X is not None:
                X = self._as_points(X)
            ctx = self.model._ensure_resident()
            key = (self._token, getattr(ctx, 'fit_gen', 0))
            if self.maxima is None:
                if getattr(ctx, 'host', False):
                    raise ValueError('MES: the maxima are drawn on the GPU; this instance has none yet and the model is '
                                     'served by the host backend')
                if X is not None:
                    ctx.set_candidates(X)
                y = np.asarray(self.model.y, dtype=np.float64)
                best = float(y.max() if self.scale_factor > 0 else y.min())
                ctx._mes_owner = None
                self.maxima = ctx.mes_draw(self.seed, self.n_samples, self.n_features, self.scale_factor, best).copy()
                ctx._mes_owner = key
            elif getattr(ctx, '_mes_owner', None) != key:
                ctx._mes_owner = None
                ctx.mes_set_maxima(self.maxima)
                ctx._mes_owner = key
            return X

        def maximise_generated(self, num_points, low, high, seed, first_candidate=0, lhs_total=None, prefetch_seed=None):
            # Not folded into the hook: the first use draws the batch BEFORE the maxima (they are drawn over it; the base
            # method then finds it by its key and does not draw it again), every later use sends the maxima before the
            # base method draws -- the hook's one place in the base method cannot give both orders.
            if self.maxima is None:
                self.model._ensure_resident().generate(seed, first_candidate, num_points, low, high, lhs_total)
            self._prepare(None)
            return super().maximise_generated(num_points, low, high, seed, first_candidate, lhs_total, prefetch_seed)

        def _refuse(self, what):
            raise NotImplementedError('MES: {} is not available for max-value entropy search (use CandidateSweep with '
                                      'the default lockstep=True gradient stage)'.format(what))

        def maximise_batch(self, X, q, strategy='kriging_believer', lie='min', pending=None, want_posterior=False,
                           n_sim=16, seed=None):
            self._refuse('batch selection (tgp_sweep_batch / tgp_sweep_batch_mc)')

        def refine(self, starting_points, bounds, max_iter=200):
            self._refuse('the on-device optimiser (on_device=True, tgp_acq_refine)')


class KG(AcquisitionFunction):
    """The knowledge gradient (Frazier, Powell & Dayanik 2009): the expected gain of the best posterior mean over a
    discretisation set ``points`` (A, D), A <= 256, and the candidate itself from ONE more observation at the candidate
    (``tgp_kg_set_points`` / ``tgp_sweep_kg``, csrc/kg_kernels.hip):

        lines  a_i = sf mu(Xa_i), b_i = C(Xa_i, x) / s(x);  a_A = sf mu(x), b_A = v(x) / s(x)
        KG(x)  = E_Z[max_i (a_i + b_i Z)] - max_i a_i >= 0,  raw units

    with C the raw latent posterior covariance, v the latent variance at x and s^2 = v + (noise + jitter) y_std^2 (the
    hyper-parameters held, as the batch strategies condition).  ``points`` None: the ``min(n_points, N, 256)`` training
    inputs with the best observed y in the direction of the extremum, the earlier trial on ties -- deterministic, no
    random number drawn.  Native models only; a marginalised model is refused.  ``maximise_batch``, ``refine``,
    ``lbfgsb`` and ``value_and_grad`` are refused by the default instance.

    ``gradient=True``: the instance offers ``value_and_grad`` (``tgp_kg_grad``: KG and its closed-form gradient, the
    envelope theorem over the same lines) and ``lbfgsb`` (``tgp_kg_lbfgsb``), so that ``CandidateSweep(grad_restarts>0)``
    / ``RandomAndQuasiNewton`` refine a KG trial as they refine EI; ``refine`` (the on-device optimiser) and
    ``maximise_batch`` stay refused."""

    def __init__(self, points=None, n_points=64, gradient=False):
        self.gradient = bool(gradient)
        n_points = int(n_points)
        if n_points < 1 or n_points > 256:
            raise ValueError('n_points must be in [1, 256]')
        if points is not None:
            points = np.array(points, dtype=np.float64)
            if points.ndim != 2 or points.shape[0] < 1 or points.shape[0] > 256:
                raise ValueError('points must be (A, D) with 1 <= A <= 256')
            if not np.all(np.isfinite(points)):
                raise ValueError('points must be finite')
        self.points = points
        self.n_points = n_points

    def get_type(self):
        return 'optimism'

    @staticmethod
    def default_points(X, y, desired_extremum, n_points=64):
        """the ``min(n_points, N, 256)`` rows of X with the best y ('max': largest), the earlier row on ties"""
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        sf = 1.0 if desired_extremum == 'max' else -1.0
        k = min(int(n_points), X.shape[0], 256)
        order = np.argsort(-sf * y, kind='stable')[:k]
        return np.ascontiguousarray(X[order])

    def construct_function(self, trial_num, model, desired_extremum):
        _refuse_warped(model, 'KG')
        _refuse_marginalised(model, 'KG (its discretisation points belong to one fitted model)')
        if not _is_native(model):
            raise ValueError('KG serves native models only: it needs a model built by HipGPSurrogate (got {!r}) for the '
                             'posterior covariance between the candidates and its points'.format(type(model)))
        if self.points is None:
            points = KG.default_points(model.X, model.y, desired_extremum, self.n_points)
        else:
            points = self.points
            if points.shape[1] != np.asarray(model.X).shape[1]:
                raise ValueError('points must be (A, {})'.format(np.asarray(model.X).shape[1]))
        acq_info = {'n_points': int(points.shape[0]), 'default_points': self.points is None}
        if self.gradient:
            acq_info['gradient'] = True
            return KG.GradientInstance(model, desired_extremum, points), acq_info
        return KG.FunctionInstance(model, desired_extremum, points), acq_info

    class FunctionInstance(AcquisitionFunction.FunctionInstance):
        """KG(x) over ``points`` (A, D)"""

        sweep_dtype = 'f64'      # the cross-covariance and the envelope are f64 whatever the handle's dtype

        def __init__(self, model, desired_extremum, points):
            super().__init__(model, desired_extremum)
            self.points = np.ascontiguousarray(points, dtype=np.float64)
            self._token = object()

        def get_name(self):
            return 'KG'

        def _native_args(self):
            raise NotImplementedError('KG has no posterior-formula arguments: it needs the cross-covariance sweep')

        def _as_points(self, X):
            X = np.asarray(X, dtype=np.float64)
            if X.ndim == 1:
                X = X.reshape(1, -1)
            assert X.ndim == 2 and X.shape[1] == self.model.X.shape[1], \
                'X must have shape (num_points, {})'.format(self.model.X.shape[1])
            return X

        def _ctx(self):
            """the model's context holding THIS instance's points: re-sent when the handle holds another fit or another
            instance's points"""
            ctx = self.model._ensure_resident()
            if getattr(ctx, 'host', False):
                raise ValueError('KG runs on the GPU only; the model is served by the host backend')
            key = (self._token, getattr(ctx, 'fit_gen', 0))
            if getattr(ctx, '_kg_owner', None) != key:
                ctx._kg_owner = None
                ctx.kg_set_points(self.points)
                ctx._kg_owner = key
            return ctx

        def _sweep(self, ctx, **want):
            res = ctx.sweep_kg(self.scale_factor, **want)
            self.last_sweep_ms = res.get('kg_ms')
            return res

        def __call__(self, X):
            X = self._as_points(X)
            if X.shape[0] == 0:
                return np.empty(0)
            ctx = self._ctx()
            ctx.set_candidates(X)
            return self._sweep(ctx, want_kg=True)['kg']

        def maximise(self, X):
            """arg-max of KG over the rows of X: (index, value); lowest index wins ties"""
            ctx = self._ctx()
            ctx.set_candidates(self._as_points(X))
            res = self._sweep(ctx)
            return res['best_idx'], res['best_val']

        def maximise_topk(self, X, k):
            """the k best rows of X: (indices (k,), values (k,)), best first (a host argsort of the (M,) values)"""
            v = self(X)
            v = np.where(np.isnan(v), -np.inf, v)
            order = np.argsort(-v, kind='stable')[:min(int(k), 64)]
            return order.astype(np.int64), v[order]

        def maximise_generated(self, num_points, low, high, seed, first_candidate=0, lhs_total=None, prefetch_seed=None):
            """draw ``num_points`` candidates on the GPU and return the best: (x (D,), value, index)"""
            if prefetch_seed is not None:
                raise NotImplementedError('KG: no prefetched batch (the overlap starts an EI / UCB sweep inside the fit)')
            ctx = self._ctx()
            ctx.generate(seed, first_candidate, num_points, low, high, lhs_total, reuse=True)
            res = self._sweep(ctx)
            return ctx.get_candidate(res['best_idx']), res['best_val'], res['best_idx']

        def maximise_host_stream(self, num_points, low, high, topk=0, first=0, count=None):
            return None     # nothing drawn: the caller draws on the host and calls maximise / maximise_topk

        def winner_record(self, global_offset):
            self._ctx()
            return super().winner_record(global_offset)

        def _refuse(self, what, instead):
            raise NotImplementedError('KG: {} is not available for the knowledge gradient (its gradient is not '
                                      'implemented): use {}'.format(what, instead))

        def maximise_batch(self, X, q, strategy='kriging_believer', lie='min', pending=None, want_posterior=False,
                           n_sim=16, seed=None):
            self._refuse('batch selection (tgp_sweep_batch / tgp_sweep_batch_mc)',
                         'maximise_topk for q rows of one sweep, or EI / UCB with select_batch')

        def refine(self, starting_points, bounds, max_iter=200):
            self._refuse('the on-device optimiser (on_device=True, tgp_acq_refine)',
                         'CandidateSweep with grad_restarts=0 (maximise over the candidates)')

        def lbfgsb(self, starting_points, bounds, max_iter=15000):
            self._refuse('the in-library L-BFGS-B (lockstep=True, tgp_acq_lbfgsb)',
                         'CandidateSweep with grad_restarts=0 (maximise over the candidates)')

        def value_and_grad(self, X):
            self._refuse('value_and_grad',
                         'CandidateSweep with grad_restarts=0, or __call__ for values and finite differences')

    class GradientInstance(FunctionInstance):
        """KG(x) over ``points`` with its closed-form gradient (``KG(gradient=True)``)"""

        def value_and_grad(self, X):
            """KG (m,) -- ``__call__``'s value for the same point -- and its gradient (m, D) at m <= 4096 points
            (``tgp_kg_grad``)"""
            return self._ctx().kg_grad(self._as_points(X), self.scale_factor)

        def lbfgsb(self, starting_points, bounds, max_iter=15000):
            """L-BFGS-B from every start inside the library (``tgp_kg_lbfgsb``): the restarts in lock-step, one batched
            ``tgp_kg_grad`` per round; returns (x (R, D), values (R,), status (R,): 1 = SciPy's success, evaluations)"""
            low, high = zip(*bounds)
            return self._ctx().kg_lbfgsb(self._as_points(starting_points), low, high, self.scale_factor, max_iter)

        def _refuse(self, what, instead):
            raise NotImplementedError('KG: {} is not available for the knowledge gradient (gradient=True serves '
                                      'value_and_grad and the in-library L-BFGS-B only): use {}'.format(what, instead))

        def refine(self, starting_points, bounds, max_iter=200):
            self._refuse('the on-device optimiser (on_device=True, tgp_acq_refine)',
                         'CandidateSweep with the default lockstep=True gradient stage (tgp_kg_lbfgsb)')



def _weighted_from_posteriors(acq, sf, incumbent, param, mu, sigma, sides):
    """the weighted value on the host from every model's posterior -- ``tgp_sweep_weighted``'s definition in NumPy, float64:
    sides = [(kind, level, mu_k, sigma_k)]; log Phi by ``scipy.special.log_ndtr`` (never log(ndtr(z)): finite for every
    finite z), a step function where sigma_k == 0, value = a exp(logw) (EI / PI; exactly 0 where a == 0 or logw == -inf) or
    logw itself (ACQ_NONE); NaN where any mu or sigma is NaN"""
    from scipy.special import log_ndtr
    mu = np.asarray(mu, dtype=np.float64).reshape(-1)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(-1)
    logw = np.zeros_like(mu)
    for k, (kind, level, mk, sk) in enumerate(sides):
        mk = np.asarray(mk, dtype=np.float64).reshape(-1)
        sk = np.asarray(sk, dtype=np.float64).reshape(-1)
        if kind == _lib.SIDE_COST:
            lf = -mk
        else:
            live = sk != 0
            d = (mk - level) if kind == _lib.SIDE_GE else (level - mk)
            with np.errstate(invalid='ignore', divide='ignore'):
                lf = np.where(live, log_ndtr(d / np.where(live, sk, 1.0)), np.where(d >= 0, 0.0, -np.inf))
        lf = np.where(np.isnan(mk) | np.isnan(sk), np.nan, lf)
        logw = lf if k == 0 else logw + lf
    bad = np.isnan(mu) | np.isnan(sigma) | np.isnan(logw)
    if acq == _lib.ACQ_NONE:
        return np.where(bad, np.nan, logw)
    a = _from_mu_sigma(acq, sf, incumbent, param, mu, sigma)
    with np.errstate(over='ignore', invalid='ignore'):
        value = np.where((a == 0) | (logw == -np.inf), 0.0, a * np.exp(logw))
    return np.where(bad | np.isnan(a), np.nan, value)


class Constraint:
    """An unknown constraint of ``Constrained``: the objective reports ``eval_info[name]`` for every trial, a GP (its OWN
    ``HipGPSurrogate`` factory: one factory is one GPU handle, so the models do not displace each other) is fitted to
    those values, and a candidate is feasible where the value is ``<= level`` (kind 'le') or ``>= level`` ('ge')"""

    def __init__(self, name, surrogate, kind='le', level=0.0):
        if kind not in ('le', 'ge'):
            raise ValueError("kind must be 'le' or 'ge'")
        if not np.isfinite(level):
            raise ValueError('level must be finite')
        self.name, self.surrogate, self.kind, self.level = name, surrogate, kind, float(level)

    def holds(self, values):
        values = np.asarray(values, dtype=np.float64)
        return values <= self.level if self.kind == 'le' else values >= self.level


class Cost:
    """The evaluation cost of ``Constrained`` ("EI per second", Snoek, Larochelle & Adams 2012, section 3.2): a GP (its own
    ``HipGPSurrogate`` factory) on the LOG of a positive cost per trial -- ``source='duration'``: the wall time between the
    Optimiser's ``evaluation_started`` and ``evaluation_finished``; any other ``source``: ``eval_info[source]``"""
    name = 'cost'

    def __init__(self, surrogate, source='duration'):
        self.surrogate, self.source = surrogate, source


class Constrained(AcquisitionFunction):
    """``base`` (``EI`` or ``PI``) weighted by the probability that every constraint model is satisfied (Gardner et al. 2014;
    Gelbart, Snoek & Adams 2014) and divided by the predicted cost -- ``tgp_sweep_weighted`` and its gradient.  It is an
    acquisition factory AND a listener (duck-typed: it imports nothing from ``turbo``), so with an unmodified reference
    Optimiser it is put in both places::

        acq = ta.Constrained(ta.EI(0.01), constraints=[ta.Constraint('g', ta.HipGPSurrogate(...), 'le', 0.0)])
        op.acquisition = acq
        op.register_listener(acq)          # evaluation_finished(trial_num, y, eval_info) brings eval_info['g']

    The incumbent the base sees is the best observed y among the trials whose OBSERVED constraint values satisfy every
    constraint; while there is none, the instance maximises the log feasibility alone (``TGP_ACQ_NONE``)."""

    def __init__(self, base, constraints=(), cost=None):
        if not isinstance(base, (EI, PI)):
            raise TypeError('Constrained weights EI or PI (a weight on a signed or entropy-valued acquisition has no meaning); '
                            'got {!r}'.format(type(base)))
        self.base = base
        self.constraints = list(constraints)
        self.cost = cost
        if len(self.constraints) + (cost is not None) > 8:
            raise ValueError('at most 8 side models')
        names = [c.name for c in self.constraints]
        if len(set(names)) != len(names):
            raise ValueError('constraint names must be distinct')
        self.records = {}          # trial_num -> {constraint name: value, 'cost': log cost}
        self._started = {}         # trial_num -> perf_counter() at evaluation_started
        self.optimiser = None

    def get_type(self):
        return 'improvement'

    # ---- listener callbacks (turbo/modules/listener.py) ----
    def registered(self, optimiser):
        self.optimiser = optimiser

    def unregistered(self):
        self.optimiser = None

    def run_started(self, finished_trials, max_trials):
        pass

    def selection_started(self, trial_num):
        pass

    def surrogate_fitted(self, trial_num):
        pass

    def acquisition_maximised(self, trial_num):
        pass

    def selection_finished(self, trial_num, x, selection_info):
        pass

    def run_finished(self):
        pass

    def evaluation_started(self, trial_num):
        import time
        if self.cost is not None and self.cost.source == 'duration':      # (the only reader: evaluation_finished pops it)
            self._started[trial_num] = time.perf_counter()

    def evaluation_finished(self, trial_num, y, eval_info):
        import time
        now = time.perf_counter()
        rec = {}
        info = eval_info if isinstance(eval_info, dict) else {}
        for c in self.constraints:
            if c.name not in info:
                raise KeyError('Constrained: trial {} reported no eval_info[{!r}] (the objective must return (cost, eval_info) '
                               'with a value for every constraint)'.format(trial_num, c.name))
            rec[c.name] = float(info[c.name])
        if self.cost is not None:
            if self.cost.source == 'duration':
                if trial_num not in self._started:
                    raise KeyError('Constrained: no evaluation_started for trial {}: the duration is unknown'.format(trial_num))
                spent = max(now - self._started.pop(trial_num), 1e-9)
            else:
                if self.cost.source not in info:
                    raise KeyError('Constrained: trial {} reported no eval_info[{!r}] (the cost)'.format(trial_num, self.cost.source))
                spent = float(info[self.cost.source])
                if not spent > 0:
                    raise ValueError('Constrained: the cost of trial {} must be positive (it is modelled as its log)'.format(trial_num))
            rec['cost'] = float(np.log(spent))
        self.records[int(trial_num)] = rec

    # ---- factory ----
    def _side_values(self, n):
        if len(self.records) != n:
            raise ValueError('Constrained holds {} trial records for a model of {} observations: register it as a listener of '
                             'the Optimiser (op.register_listener(acq)) before the first trial, one record per row of model.X'
                             .format(len(self.records), n))
        order = sorted(self.records)
        return {c.name: np.array([self.records[t][c.name] for t in order]) for c in self.constraints}, \
            (np.array([self.records[t]['cost'] for t in order]) if self.cost is not None else None)

    def construct_function(self, trial_num, model, desired_extremum, incumbent_cost):
        _refuse_warped(model, 'Constrained')
        _refuse_marginalised(model, 'Constrained (each side is weighted under one fitted model)')
        X = np.asarray(model.X, dtype=np.float64)
        y = np.asarray(model.y, dtype=np.float64).reshape(-1)
        values, cost = self._side_values(X.shape[0])
        xi = self.base.xi(trial_num) if callable(self.base.xi) else self.base.xi
        sides, side_info = [], {}
        feasible = np.ones(X.shape[0], dtype=bool)
        for c in self.constraints:
            m, info = c.surrogate.construct_model(trial_num, X, values[c.name])
            sides.append((c.name, m, _lib.SIDE_LE if c.kind == 'le' else _lib.SIDE_GE, c.level))
            side_info[c.name] = info
            feasible &= c.holds(values[c.name])
        if self.cost is not None:
            m, info = self.cost.surrogate.construct_model(trial_num, X, cost)
            sides.append(('cost', m, _lib.SIDE_COST, 0.0))
            side_info['cost'] = info
        for name, m, _, _ in sides:
            _refuse_warped(m, 'Constrained (side {!r})'.format(name))
            _refuse_marginalised(m, 'Constrained (side {!r})'.format(name))
        n_feasible = int(feasible.sum())
        if n_feasible > 0:
            incumbent = float(y[feasible].max() if desired_extremum == 'max' else y[feasible].min())
            acq = self.base.FunctionInstance.ACQ
        else:          # no feasible observation yet: the pure feasibility search
            incumbent, acq = None, _lib.ACQ_NONE
        acq_info = {'xi': xi, 'feasible_incumbent': incumbent, 'n_feasible': n_feasible, 'side_fitting_info': side_info}
        return Constrained.FunctionInstance(model, desired_extremum, acq, incumbent, xi, sides, self.base.FunctionInstance.NAME), acq_info

    class FunctionInstance(AcquisitionFunction.FunctionInstance):
        """value(x) = base(x) prod_k f_k(x) -- or sum_k log f_k(x) while no feasible trial exists -- over ``sides``
        [(name, model, kind, level)]"""

        sweep_dtype = 'f64'      # the weight and the product are f64 whatever the handles' dtypes

        def __init__(self, model, desired_extremum, acq, incumbent, xi, sides, base_name):
            super().__init__(model, desired_extremum)
            self.acq = acq
            self.incumbent_cost = incumbent
            self.xi = xi
            self.sides = list(sides)
            self.base_name = base_name

        def get_name(self):
            return 'feasibility' if self.acq == _lib.ACQ_NONE else 'constrained ' + self.base_name

        def _native_args(self):
            return self.acq, (0.0 if self.incumbent_cost is None else self.incumbent_cost), (0.0 if self.acq == _lib.ACQ_NONE else self.xi)

        def _as_points(self, X):
            X = np.asarray(X, dtype=np.float64)
            if X.ndim == 1:
                X = X.reshape(1, -1)
            assert X.ndim == 2 and X.shape[1] == np.asarray(self.model.X).shape[1], \
                'X must have shape (num_points, {})'.format(np.asarray(self.model.X).shape[1])
            return X

        def _on_gpu(self):
            """(the objective's context, [(side context, kind, level)]) with every model resident in its own handle, or
            None where the formula is served on the host: a foreign objective or side model, or a reloaded model where
            no GPU is visible (the Recorder's plot path)"""
            if not _is_native(self.model) or not all(_is_native(m) for _, m, _, _ in self.sides):
                return None
            ctx = self.model._ensure_resident()
            if getattr(ctx, 'host', False):
                return None
            specs, seen = [], [ctx]
            for name, m, kind, level in self.sides:
                g = m._ensure_resident()
                if getattr(g, 'host', False):
                    return None
                if any(g is s for s in seen):
                    raise ValueError('Constrained: side {!r} shares its HipGPSurrogate factory (one GPU handle) with the objective '
                                     'or another side: give every Constraint / Cost its own factory'.format(name))
                seen.append(g)
                specs.append((g, kind, level))
            return ctx, specs

        def _require_gpu(self, what):
            on = self._on_gpu()
            if on is None:
                raise TypeError('Constrained: {} runs on the GPU only: it needs models built by HipGPSurrogate and a visible '
                                'device'.format(what))
            return on

        def _weighted(self, ctx, specs, **want):
            acq, incumbent, param = self._native_args()
            res = ctx.sweep_weighted(specs, acq, self.scale_factor, incumbent, param, **want)
            return res

        def __call__(self, X):
            X = self._as_points(X)
            if X.shape[0] == 0:
                return np.empty(0)
            on = self._on_gpu()
            if on is None:       # the formula from model.predict of every model, in NumPy
                acq, incumbent, param = self._native_args()
                mu, sigma = self.model.predict(X, return_std_dev=True)
                sides = [(kind, level) + tuple(m.predict(X, return_std_dev=True)) for _, m, kind, level in self.sides]
                return _weighted_from_posteriors(acq, self.scale_factor, incumbent, param, mu, sigma, sides)
            ctx, specs = on
            ctx.set_candidates(X)
            return self._weighted(ctx, specs, want_value=True)['value']

        def maximise(self, X):
            """arg-max of the weighted value over the rows of X: (index, value); lowest index wins ties"""
            on = self._on_gpu()
            if on is None:
                vals = self(X)
                vals = np.where(np.isnan(vals), -np.inf, vals)
                i = int(np.argmax(vals))
                return i, float(vals[i])
            ctx, specs = on
            ctx.set_candidates(self._as_points(X))
            res = self._weighted(ctx, specs)
            return res['best_idx'], res['best_val']

        def maximise_generated(self, num_points, low, high, seed, first_candidate=0, lhs_total=None, prefetch_seed=None):
            """draw ``num_points`` candidates on the GPU and return the best: (x (D,), value, index)"""
            if prefetch_seed is not None:
                raise NotImplementedError('Constrained: no prefetched batch (the overlap starts an unweighted sweep inside the fit)')
            ctx, specs = self._require_gpu('maximise_generated')
            ctx.generate(seed, first_candidate, num_points, low, high, lhs_total, reuse=True)
            res = self._weighted(ctx, specs)
            return ctx.get_candidate(res['best_idx']), res['best_val'], res['best_idx']

        def maximise_host_stream(self, num_points, low, high, topk=0, first=0, count=None):
            """the reference's host draw finished on the GPU, then the weighted sweep; None -- nothing drawn -- where the
            library cannot promise NumPy's numbers, or a top-k is asked for (the caller then draws on the host)"""
            if topk > 0:
                return None
            on = self._on_gpu()
            if on is None:
                return None
            ctx, specs = on
            if not hasattr(ctx, 'set_candidates_numpy_stream') or not ctx.set_candidates_numpy_stream(num_points, low, high, first=first, count=count):
                return None
            res = self._weighted(ctx, specs)
            return ctx, res['best_idx'], res['best_val'], None

        def value_and_grad(self, X):
            """the weighted value (m,) and its gradient (m, D) at m <= 4096 points (``tgp_weighted_grad``)"""
            ctx, specs = self._require_gpu('value_and_grad')
            acq, incumbent, param = self._native_args()
            return ctx.weighted_grad(self._as_points(X), specs, acq, self.scale_factor, incumbent, param)

        def lbfgsb(self, starting_points, bounds, max_iter=15000):
            """L-BFGS-B from every start inside the library (``tgp_weighted_lbfgsb``): the restarts in lock-step, one batched
            ``tgp_weighted_grad`` per round; returns (x (R, D), values (R,), status (R,): 1 = SciPy's success, evaluations)"""
            ctx, specs = self._require_gpu('lbfgsb')
            acq, incumbent, param = self._native_args()
            low, high = zip(*bounds)
            return ctx.weighted_lbfgsb(self._as_points(starting_points), low, high, specs, acq, self.scale_factor, incumbent,
                                       param, max_iter)

        def _refuse(self, what, instead):
            raise NotImplementedError('Constrained: {} is not available for the weighted acquisition: use {}'.format(what, instead))

        # maximise_topk is a PROPERTY that raises AttributeError, not a method that raises NotImplementedError: CandidateSweep asks
        # ``hasattr(acq, 'maximise_topk')`` (auxiliary_optimisers._offers) before it takes the tgp_sweep_topk route, and the base
        # class defines the method, so the only way for this instance not to offer it is for the attribute not to be there.
        # CandidateSweep then ranks the values of __call__ on the host; a direct call still fails with the text below.
        @property
        def maximise_topk(self):
            raise AttributeError('Constrained: maximise_topk (tgp_sweep_topk) is not available for the weighted acquisition: '
                                 'use __call__ and a host argsort')

        def maximise_batch(self, X, q, strategy='kriging_believer', lie='min', pending=None, want_posterior=False,
                           n_sim=16, seed=None):
            self._refuse('batch selection (tgp_sweep_batch / tgp_sweep_batch_mc)', 'one selection at a time')

        def refine(self, starting_points, bounds, max_iter=200):
            self._refuse('the on-device optimiser (on_device=True, tgp_acq_refine)',
                         'the default lockstep=True gradient stage (tgp_weighted_lbfgsb)')

        def winner_record(self, global_offset):
            self._refuse('winner_record (the sharded multi-GPU sweep)', 'one process per optimisation')


def pareto_front(Y, sf, ref):
    """the front of ``tgp_ehvi_set_front`` in NumPy: the rows of Y (n, 2) that strictly beat ``ref`` in both oriented
    coordinates u_j = sf_j y_j and that no other pair weakly dominates, duplicates merged, sorted by u_1 ascending ->
    (front (P, 2) raw units, positions (P,) of each point's first row in Y, dominated area over ref)"""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, 2)
    sf = np.asarray(sf, dtype=np.float64)
    r = sf * np.asarray(ref, dtype=np.float64)
    U = Y * sf
    order = sorted((i for i in range(U.shape[0]) if U[i, 0] > r[0] and U[i, 1] > r[1]), key=lambda i: (-U[i, 0], -U[i, 1], i))
    keep, top = [], r[1]
    for i in order:
        if U[i, 1] > top:
            keep.append(i)
            top = U[i, 1]
    keep.reverse()
    hv, left = 0.0, r[0]
    for i in keep:
        hv += (U[i, 0] - left) * (U[i, 1] - r[1])
        left = U[i, 0]
    idx = np.array(keep, dtype=np.int64)
    return Y[idx].reshape(-1, 2), idx, hv


def _ehvi_from_posteriors(front, sf, ref, mu1, sigma1, mu2, sigma2):
    """the expected hypervolume improvement on the host from both models' posteriors -- ``tgp_sweep_ehvi``'s definition in
    NumPy, float64: ``front`` (P, 2) raw units sorted as ``pareto_front`` returns it; H(z) for z <= 0 through
    ``scipy.special.erfcx``; e = max(m - t, 0) where sigma == 0; NaN where any mu or sigma is NaN"""
    from scipy.special import erfcx, ndtr
    sf = np.asarray(sf, dtype=np.float64)
    F = np.asarray(front, dtype=np.float64).reshape(-1, 2) * sf
    r = sf * np.asarray(ref, dtype=np.float64)
    a = np.concatenate([[r[0]], F[:, 0]])
    c = np.concatenate([F[:, 1], [r[1]]])
    m = [sf[0] * np.asarray(mu1, dtype=np.float64).reshape(-1), sf[1] * np.asarray(mu2, dtype=np.float64).reshape(-1)]
    s = [np.asarray(sigma1, dtype=np.float64).reshape(-1), np.asarray(sigma2, dtype=np.float64).reshape(-1)]

    def e(j, t):
        d = m[j] - t
        live = s[j] != 0
        sj = np.where(live, s[j], 1.0)
        with np.errstate(over='ignore', under='ignore', invalid='ignore'):
            z = d / sj
            x = -np.minimum(z, 0.0) / np.sqrt(2.0)
            left = np.exp(-x * x) * (1.0 / np.sqrt(2.0 * np.pi) - x * erfcx(x) / np.sqrt(2.0))
            zp = np.maximum(z, 0.0)
            right = np.exp(-0.5 * zp * zp) / np.sqrt(2.0 * np.pi) + zp * ndtr(zp)
            return np.where(live, sj * np.where(z <= 0, left, right), np.maximum(d, 0.0))
    value = np.zeros_like(m[0])
    lo = e(0, a[0])
    for i in range(len(c)):
        hi = e(0, a[i + 1]) if i + 1 < len(a) else np.zeros_like(lo)
        value = value + np.maximum(lo - hi, 0.0) * e(1, c[i])
        lo = hi
    bad = np.isnan(m[0]) | np.isnan(s[0]) | np.isnan(m[1]) | np.isnan(s[1])
    return np.where(bad, np.nan, value)


class Objective:
    """The second objective of ``EHVI``: the objective function reports ``eval_info[name]`` for every trial, and a GP (its OWN
    ``HipGPSurrogate`` factory: one factory is one GPU handle, so the two models do not displace each other) is fitted to
    those values; ``extremum``: 'min' or 'max'"""

    def __init__(self, name, surrogate, extremum='min'):
        if extremum not in ('min', 'max'):
            raise ValueError("extremum must be 'min' or 'max'")
        self.name, self.surrogate, self.extremum = name, surrogate, extremum


class EHVI(AcquisitionFunction):
    """Two-objective expected hypervolume improvement -- ``tgp_sweep_ehvi`` and its gradient: the Optimiser's own objective is
    objective 1, ``second`` (an ``Objective``) objective 2, and a candidate is scored by the expected growth of the area the
    Pareto front of the observed pairs dominates over ``ref`` (2 raw values; None: per objective the worst observed value
    moved away from the front by 0.1 of the observed range, a zero range counting as 1.0).  It is an acquisition factory AND a
    listener (duck-typed: it imports nothing from ``turbo``), so with an unmodified reference Optimiser it is put in both
    places::

        acq = ta.EHVI(ta.Objective('latency', ta.HipGPSurrogate(...), 'min'))
        op.acquisition = acq
        op.register_listener(acq)          # evaluation_finished(trial_num, y, eval_info) brings eval_info['latency']
    """

    def __init__(self, second, ref=None):
        if not isinstance(second, Objective):
            raise TypeError('EHVI takes the second objective as an Objective; got {!r}'.format(type(second)))
        if ref is not None:
            ref = np.asarray(ref, dtype=np.float64).reshape(-1)
            if ref.shape != (2,) or not np.all(np.isfinite(ref)):
                raise ValueError('ref must be 2 finite values')
        self.second = second
        self.ref = ref
        self.records = {}          # trial_num -> the second objective's value
        self.optimiser = None

    def get_type(self):
        return 'optimism'          # the Optimiser's scalar incumbent plays no part

    # ---- listener callbacks (turbo/modules/listener.py) ----
    def registered(self, optimiser):
        self.optimiser = optimiser

    def unregistered(self):
        self.optimiser = None

    def run_started(self, finished_trials, max_trials):
        pass

    def selection_started(self, trial_num):
        pass

    def surrogate_fitted(self, trial_num):
        pass

    def acquisition_maximised(self, trial_num):
        pass

    def selection_finished(self, trial_num, x, selection_info):
        pass

    def run_finished(self):
        pass

    def evaluation_started(self, trial_num):
        pass

    def evaluation_finished(self, trial_num, y, eval_info):
        info = eval_info if isinstance(eval_info, dict) else {}
        name = self.second.name
        if name not in info:
            raise KeyError('EHVI: trial {} reported no eval_info[{!r}] (the objective must return (cost, eval_info) with the '
                           'second objective\'s value)'.format(trial_num, name))
        value = float(info[name])
        if not np.isfinite(value):
            raise ValueError('EHVI: the second objective of trial {} must be finite'.format(trial_num))
        self.records[int(trial_num)] = value

    # ---- factory ----
    def _second_values(self, n):
        if len(self.records) != n:
            raise ValueError('EHVI holds {} trial records for a model of {} observations: register it as a listener of the '
                             'Optimiser (op.register_listener(acq)) before the first trial, one record per row of model.X'
                             .format(len(self.records), n))
        order = sorted(self.records)
        return order, np.array([self.records[t] for t in order])

    @staticmethod
    def default_ref(Y, sf):
        """per objective the worst observed value moved away from the front by 0.1 of the observed range (zero range: 1.0)"""
        sf = np.asarray(sf, dtype=np.float64)
        U = np.asarray(Y, dtype=np.float64).reshape(-1, 2) * sf
        span = U.max(0) - U.min(0)
        span = np.where(span > 0, span, 1.0)
        return sf * (U.min(0) - 0.1 * span)

    def construct_function(self, trial_num, model, desired_extremum):
        _refuse_warped(model, 'EHVI')
        _refuse_marginalised(model, 'EHVI (each objective is scored under one fitted model)')
        X = np.asarray(model.X, dtype=np.float64)
        y = np.asarray(model.y, dtype=np.float64).reshape(-1)
        trials, y2 = self._second_values(X.shape[0])
        second_model, second_info = self.second.surrogate.construct_model(trial_num, X, y2)
        _refuse_warped(second_model, 'EHVI (the second objective)')
        _refuse_marginalised(second_model, 'EHVI (the second objective)')
        Y = np.stack([y, y2], 1)
        sf = (1.0 if desired_extremum == 'max' else -1.0, 1.0 if self.second.extremum == 'max' else -1.0)
        ref = self.default_ref(Y, sf) if self.ref is None else self.ref.copy()
        front, idx, hv = pareto_front(Y, sf, ref)
        if front.shape[0] > _lib.EHVI_MAX_FRONT:
            raise ValueError('EHVI: the front has {} points; at most {} are scored (tgp_ehvi_set_front)'.format(front.shape[0], _lib.EHVI_MAX_FRONT))
        inst = EHVI.FunctionInstance(model, desired_extremum, second_model, self.second.name, sf, ref, Y, front)
        if inst._on_gpu() is not None:          # the library's own builder is the one the sweep uses: its front and area are reported
            front, hv = inst._library_front
            inst.front = front
        acq_info = {'ref': ref, 'pareto_front': front, 'pareto_trials': [trials[i] for i in idx], 'hypervolume': hv,
                    'second_fitting_info': second_info}
        return inst, acq_info

    class FunctionInstance(AcquisitionFunction.FunctionInstance):
        """value(x) = the expected growth of the area dominated over ``ref`` by ``front`` under the two models' independent
        posteriors at x"""

        sweep_dtype = 'f64'      # the closed form is f64 whatever the handles' dtypes

        def __init__(self, model, desired_extremum, second_model, second_name, sf, ref, Y, front):
            super().__init__(model, desired_extremum)
            self.second_model = second_model
            self.second_name = second_name
            self.sf = tuple(float(v) for v in sf)
            self.ref = np.asarray(ref, dtype=np.float64)
            self.Y = np.asarray(Y, dtype=np.float64)
            self.front = np.asarray(front, dtype=np.float64)
            self._token = uuid.uuid4().hex      # which instance's front a handle holds (a handle serves one trial after another)
            self._library_front = None          # (front, hypervolume) as tgp_ehvi_set_front reported them

        def get_name(self):
            return 'EHVI'

        def _as_points(self, X):
            X = np.asarray(X, dtype=np.float64)
            if X.ndim == 1:
                X = X.reshape(1, -1)
            assert X.ndim == 2 and X.shape[1] == np.asarray(self.model.X).shape[1], \
                'X must have shape (num_points, {})'.format(np.asarray(self.model.X).shape[1])
            return X

        def _on_gpu(self):
            """(objective 1's context, objective 2's) with both models resident, each in its own handle, and this
            instance's front on the first -- or None where the formula is served on the host: a foreign model, or a
            reloaded one where no GPU is visible (the Recorder's plot path)"""
            if not _is_native(self.model) or not _is_native(self.second_model):
                return None
            ctx = self.model._ensure_resident()
            if getattr(ctx, 'host', False):
                return None
            g = self.second_model._ensure_resident()
            if getattr(g, 'host', False):
                return None
            if g is ctx:
                raise ValueError('EHVI: the second objective shares its HipGPSurrogate factory (one GPU handle) with the first: '
                                 'give the Objective its own factory')
            if getattr(ctx, '_ehvi_owner', None) != self._token:      # another instance's front (or none) is on the handle
                self._library_front = ctx.ehvi_set_front(self.Y, self.ref, self.sf)
                ctx._ehvi_owner = self._token
            return ctx, g

        def _require_gpu(self, what):
            on = self._on_gpu()
            if on is None:
                raise TypeError('EHVI: {} runs on the GPU only: it needs models built by HipGPSurrogate and a visible '
                                'device'.format(what))
            return on

        def __call__(self, X):
            X = self._as_points(X)
            if X.shape[0] == 0:
                return np.empty(0)
            on = self._on_gpu()
            if on is None:       # the formula from model.predict of both models, in NumPy
                mu1, s1 = self.model.predict(X, return_std_dev=True)
                mu2, s2 = self.second_model.predict(X, return_std_dev=True)
                return _ehvi_from_posteriors(self.front, self.sf, self.ref, mu1, s1, mu2, s2)
            ctx, g = on
            ctx.set_candidates(X)
            return ctx.sweep_ehvi(g, want_value=True)['value']

        def maximise(self, X):
            """arg-max of the value over the rows of X: (index, value); lowest index wins ties"""
            on = self._on_gpu()
            if on is None:
                vals = self(X)
                vals = np.where(np.isnan(vals), -np.inf, vals)
                i = int(np.argmax(vals))
                return i, float(vals[i])
            ctx, g = on
            ctx.set_candidates(self._as_points(X))
            res = ctx.sweep_ehvi(g)
            return res['best_idx'], res['best_val']

        def maximise_generated(self, num_points, low, high, seed, first_candidate=0, lhs_total=None, prefetch_seed=None):
            """draw ``num_points`` candidates on the GPU and return the best: (x (D,), value, index)"""
            if prefetch_seed is not None:
                raise NotImplementedError('EHVI: no prefetched batch (the overlap starts a single-objective sweep inside the fit)')
            ctx, g = self._require_gpu('maximise_generated')
            ctx.generate(seed, first_candidate, num_points, low, high, lhs_total, reuse=True)
            res = ctx.sweep_ehvi(g)
            return ctx.get_candidate(res['best_idx']), res['best_val'], res['best_idx']

        def maximise_host_stream(self, num_points, low, high, topk=0, first=0, count=None):
            """the reference's host draw finished on the GPU, then the sweep; None -- nothing drawn -- where the library
            cannot promise NumPy's numbers, or a top-k is asked for (the caller then draws on the host)"""
            if topk > 0:
                return None
            on = self._on_gpu()
            if on is None:
                return None
            ctx, g = on
            if not hasattr(ctx, 'set_candidates_numpy_stream') or not ctx.set_candidates_numpy_stream(num_points, low, high, first=first, count=count):
                return None
            res = ctx.sweep_ehvi(g)
            return ctx, res['best_idx'], res['best_val'], None

        def value_and_grad(self, X):
            """the value (m,) and its gradient (m, D) at m <= 4096 points (``tgp_ehvi_grad``)"""
            ctx, g = self._require_gpu('value_and_grad')
            return ctx.ehvi_grad(self._as_points(X), g)

        def lbfgsb(self, starting_points, bounds, max_iter=15000):
            """L-BFGS-B from every start inside the library (``tgp_ehvi_lbfgsb``): the restarts in lock-step, one batched
            ``tgp_ehvi_grad`` per round; returns (x (R, D), values (R,), status (R,): 1 = SciPy's success, evaluations)"""
            ctx, g = self._require_gpu('lbfgsb')
            low, high = zip(*bounds)
            return ctx.ehvi_lbfgsb(self._as_points(starting_points), low, high, g, max_iter)

        def _refuse(self, what, instead):
            raise NotImplementedError('EHVI: {} is not available for the expected hypervolume improvement: use {}'.format(what, instead))

        # (a PROPERTY that raises AttributeError, as Constrained's: CandidateSweep asks hasattr(acq, 'maximise_topk'))
        @property
        def maximise_topk(self):
            raise AttributeError('EHVI: maximise_topk (tgp_sweep_topk) is not available for the expected hypervolume improvement: '
                                 'use __call__ and a host argsort')

        def maximise_batch(self, X, q, strategy='kriging_believer', lie='min', pending=None, want_posterior=False,
                           n_sim=16, seed=None):
            self._refuse('batch selection (tgp_sweep_batch / tgp_sweep_batch_mc)', 'one selection at a time')

        def refine(self, starting_points, bounds, max_iter=200):
            self._refuse('the on-device optimiser (on_device=True, tgp_acq_refine)',
                         'the default lockstep=True gradient stage (tgp_ehvi_lbfgsb)')

        def winner_record(self, global_offset):
            self._refuse('winner_record (the sharded multi-GPU sweep)', 'one process per optimisation')


def joint_ei(model, Xb, desired_extremum, incumbent, xi=0.01, n_samples=512, seed=None, eps=None, latent=False,
             nugget=1e-10):
    """The Monte Carlo q-EI of a batch: the expected improvement of the BEST of the q points of ``Xb`` (q, D), q <= 4096,
    under their joint posterior,

        mean_s max(0, max_j (sf (y_sj - incumbent) - xi)),   y_s ~ N(mu(Xb), cov(Xb)),   sf = +1 ('max') / -1 ('min')

    with the sign convention of ``EI`` (for q = 1 it converges to ``EI(xi)``'s closed form).  The samples come from
    ``model.sample_y`` (``tgp_sample_joint``: exact joint samples); the average is host arithmetic on the
    (n_samples, q) values.  ``seed`` / ``eps`` / ``latent`` / ``nugget`` as ``sample_y``; the same ``eps`` for two batches
    compares them under common random numbers.  Scores what ``CandidateSweep.select_batch`` or any other batch rule
    chose.  Native models only."""
    if not _is_native(model):
        raise ValueError('joint_ei serves native models only: it needs a model built by HipGPSurrogate (got {!r}) for '
                         'the joint posterior its samples come from'.format(type(model)))
    assert desired_extremum in ('min', 'max')
    sf = 1.0 if desired_extremum == 'max' else -1.0
    y = model.sample_y(Xb, n_samples=n_samples, seed=seed, eps=eps, latent=latent, nugget=nugget)   # (q, S)
    best = (sf * (y - float(incumbent)) - float(xi)).max(axis=0)
    return float(np.maximum(best, 0.0).mean())
