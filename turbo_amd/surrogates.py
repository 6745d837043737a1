"""Surrogate plugin: a GP fitted and queried on one MI355X through libturbogp.so.

Mirrors the reference's plugin contract so an unmodified ``turbo.Optimiser`` can use it as
``optimiser.surrogate`` (turbo/optimiser.py:43-47, :336):

    Surrogate / Surrogate.ModelInstance          turbo/modules/surrogates.py:22-81
    SciKitGPSurrogate (the semantics mirrored)   turbo/modules/surrogates.py:225-365

Hyper-parameters are either fixed (``model_params['optimizer'] = None`` or
``training_iterations = 0``) or fitted like scikit-learn does it for the reference
(sklearn/gaussian_process/_gpr.py:296-337): L-BFGS-B on the negative log marginal likelihood in
log space, started from the kernel's values (or the previous trial's, ``param_continuity``) and
from ``iterations - 1`` random restarts.  Every objective evaluation -- kernel matrix, Cholesky,
K^-1 and the gradient trace -- runs on the GPU (``tgp_fit_grad``); SciPy only drives theta.
"""
import copy
import numbers
import warnings

import numpy as np

from . import _lib
from .kernels import GPKernel



_START_THREADS = None


def _start_threads():
    """the threads that drive the concurrent starts of a hyper-parameter fit (one per worker handle of the device's
    pool, at most four), created once per process"""
    global _START_THREADS
    if _START_THREADS is None:
        from concurrent.futures import ThreadPoolExecutor
        _START_THREADS = ThreadPoolExecutor(max_workers=4, thread_name_prefix='turbo_amd-start')
    return _START_THREADS


class Surrogate:
    """A probabilistic model factory: one fitted ModelInstance per trial
    (turbo/modules/surrogates.py:22-81)."""

    def construct_model(self, trial_num, X, y):
        """Returns: (model, fitting_info)"""
        raise NotImplementedError()

    class ModelInstance:
        def predict(self, X, return_std_dev=False):
            raise NotImplementedError()

        def get_hyper_params(self):
            raise NotImplementedError()

        def get_hyper_param_names(self):
            raise NotImplementedError()

        def get_log_likelihood(self):
            raise NotImplementedError()


class HipGPSurrogate(Surrogate):
    """Drop-in for ``SciKitGPSurrogate`` with the arithmetic on the GPU.

    ``model_params`` takes the same keys the reference forwards to
    ``GaussianProcessRegressor`` (turbo/modules/surrogates.py:245-251, :315):
    ``kernel`` (a ``GPKernel`` or a scikit-learn kernel object), ``alpha`` (jitter, default
    1e-10), ``normalize_y`` (default True as in the reference's defaults, :231-243),
    ``optimizer`` (None = fixed hyper-parameters; 'fmin_l_bfgs_b' (default): L-BFGS-B as scikit-learn runs it,
    walked INSIDE the library (``tgp_fit_lbfgsb``: SciPy's algorithm restated in C++, a thread and a stream per
    start driving the GPU objective with no interpreter between two evaluations -- the same iterates, evaluation
    counts and optimum as SciPy's on the same objective; unbounded theta falls back to 'scipy'); 'scipy': SciPy's own L-BFGS-B drives the GPU objective from Python (the default of
    rounds 1-4; ``parallel_restarts_above`` applies); 'device' (opt-in): ``tgp_fit_optimise`` -- N <= 128: every
    start side by side in ONE launch with a projected L-BFGS whose iterates are not SciPy's, its optima the same
    or better; larger problems: as the default; or a callable with scikit-learn's optimizer signature),
    ``random_state`` and ``n_restarts_optimizer``.
    """

    default_model_params = {
        # 1.0 * Matern(nu=2.5) + WhiteKernel()  (turbo/modules/surrogates.py:236)
        'kernel': GPKernel('matern52', 1.0, 1.0, 1.0),
        'normalize_y': True,
    }

    def __init__(self, model_params=None, training_iterations=None, param_continuity=True,
                 dtype='f64', device=0, incremental=True, parallel_restarts_above='auto', criterion='lml'):
        """
        Args:
            model_params (dict): see class docstring
            training_iterations (None, int, or function of trial_num): as in the reference
                (surrogates.py:245-292).  With fixed hyper-parameters the value only ends up
                in ``fitting_info['iterations']``.
            param_continuity (bool): kept for signature compatibility (surrogates.py:269-271)
            dtype: 'f64', 'f32', or 'f32h2' / 'f32x3' (f32 accuracy from two scaled fp16 / three bf16
                planes on the 16-bit matrix pipe, opt-in) -- arithmetic of the candidate sweep; the fit (and the
                hyper-parameter optimisation) is always f64
            device: HIP device index
            incremental: when consecutive trials keep the hyper-parameters and only append one
                observation (the Optimiser's loop, turbo/optimiser.py:335-336), extend the
                resident factorisation by one row in O(N^2) instead of refitting in O(N^3)
            parallel_restarts_above: when the starts of the hyper-parameter fit (the warm start and the
                ``iterations - 1`` restarts) run side by side, one host thread and one GPU handle on a private
                stream each -- same iterates, same result as one after the other, bit for bit.  'auto'
                (default): where that was measured to pay, 64 < N <= 8192 on three threads (to 1536 until late in
                round 5; beyond, the workers' workspaces -- 4 N^2 doubles each -- set the limit): one evaluation
                there is a serial chain that leaves the chip idle and SciPy's own per-evaluation overhead of
                one start hides behind another start's kernels (round 4, three starts: N = 500 10.9 -> 6.5 ms,
                700 14.7 -> 7.8, 1000 27.8 -> 22.8, 1500 61 -> 57; N = 2048: no gain.  Round 5, with the start
                threads kept alive between fits -- starting three threads cost 1.2 ms per fit: N = 200 6.2 -> 4.2-5.5 ms,
                256 6.3 -> 4.9-6.5, 500 7.1 -> 5.1-6.0, 1000 23.4 -> 20.4-22.0 (host-bound: +-15 % run to run);
                N = 100 / 128 6.2 / 5.2 -> 5.8 / 4.8; below that the interpreter is the bottleneck and threads lose:
                N = 32 3.7 -> 5.8).  None: never.  A
                number: with more observations than that.
            criterion: what the hyper-parameters maximise.  'lml' (default): the log marginal likelihood, as
                scikit-learn does.  'loo': the leave-one-out log predictive density L_LOO (Rasmussen & Williams
                section 5.4.2; ``tgp_fit_loo_grad``), the criterion that does not trust the kernel family: SciPy's
                L-BFGS-B drives the GPU objective from Python for every ``optimizer`` but None (the in-library
                optimisers know the LML only and are not used); ``fitting_info`` then carries 'criterion' and the
                final 'loo'.
        """
        if criterion not in ('lml', 'loo'):
            raise ValueError("criterion must be 'lml' or 'loo'")
        self.criterion = criterion
        _lib.load()   # fail loudly, now, when the native library is missing ...
        if _lib.HOST_ONLY:
            # ... or when only the host-only build could be loaded: that one serves RELOADED models
            # (unpickling does not come through here); a new factory is the optimisation path and needs the GPU
            raise _lib.TurboGPLibraryError(
                "the GPU build of libturbogp.so could not be loaded ({}); this process loaded the host-only "
                "library, which can evaluate reloaded models but not fit new ones".format(_lib.LOAD_ERROR))
        self.model_params = model_params or self.default_model_params
        self.training_iterations = training_iterations
        assert training_iterations is None or self.model_params.get('n_restarts_optimizer') is None, \
            'cannot specify n_restarts_optimizer and training_iterations at the same time'
        self.param_continuity = param_continuity
        self.dtype = dtype
        self.device = device
        self.incremental = incremental
        self.parallel_restarts_above = parallel_restarts_above
        self.restart_threads = 3
        self._workers = []       # GPU contexts of the hyper-parameter fit's concurrent starts, while that fit runs
        self.last_worker_count = 0
        self._native = None      # one GPU context shared by every model this factory makes
        self._resident = None    # id of the model whose fit currently lives in the context
        self._last_model_params = None
        self._reloaded = False   # True once this factory came out of a pickle (Recorder.load_compressed)

    def _context(self):
        if self._native is None:
            try:
                self._native = _lib.NativeGP(self.device, self.dtype)
            except _lib.NoDeviceError:     # (also what the host-only library answers for any GPU device)
                # Only a RELOADED factory may go on without a GPU: the recorder's models are often
                # queried by the plot path in another process (turbo/recorder.py:157-163,
                # turbo/plotting/trials.py:192-195, :574-577) that owns no MI355X.  libturbogp.so's host
                # backend (csrc/host_backend.cpp) then answers predict / acquisition in float64.
                # A factory made in this process still fails loudly: the optimisation loop is GPU-only.
                if not getattr(self, '_reloaded', False):
                    raise
                warnings.warn('no HIP device in this process: the reloaded model is evaluated by the host '
                              'backend of libturbogp.so (float64; meant for plots, not for optimisation runs)')
                self._native = _lib.NativeGP(_lib.DEVICE_HOST, 'f64')
        return self._native

    def _get_training_iterations(self, trial_num):
        # turbo/modules/surrogates.py:283-292
        if self.training_iterations is None:
            iterations = self.model_params.get('n_restarts_optimizer')  # may be absent / None
        elif callable(self.training_iterations):
            iterations = self.training_iterations(trial_num)
        else:
            iterations = self.training_iterations
        assert iterations is not None, 'must specify the number of training iterations'
        assert iterations >= 0, 'invalid number of iterations: {}'.format(iterations)
        return iterations

    def construct_model(self, trial_num, X, y):
        """turbo/modules/surrogates.py:294-326"""
        iterations = self._get_training_iterations(trial_num)
        fitting_info = {'iterations': iterations}
        assert 'kernel' in self.model_params, 'you must specify a kernel for the GP'
        # don't want the initial parameter values to be changed, so make a copy
        kernel = GPKernel.from_any(self.model_params['kernel']).copy()
        optimizer = self.model_params.get('optimizer', 'fmin_l_bfgs_b')
        jitter = self.model_params.get('alpha', 1e-10)
        assert np.isscalar(jitter), 'only a scalar alpha is supported'
        normalize_y = bool(self.model_params.get('normalize_y', False))

        if self.param_continuity and self._last_model_params is not None:
            # theta is log-transformed (surrogates.py:302-304)
            kernel.theta = np.log(self._last_model_params.copy())

        # inputs are owned by the caller and may be mutated after return: copy on entry
        # (sklearn copy_X_train=True, _gpr.py:293-294)
        X = np.array(X, dtype=np.float64, copy=True, order='C')
        y = np.array(y, dtype=np.float64, copy=True).reshape(-1)
        assert X.ndim == 2 and X.shape[0] == y.shape[0], 'X must be (N, D) and y (N,)'
        if kernel.anisotropic:
            assert len(kernel.length_scale) == X.shape[1], \
                'anisotropic length scale needs one entry per dimension'

        with warnings.catch_warnings(record=True) as ws:
            warnings.simplefilter('always')
            trained = iterations > 0 and optimizer is not None and len(kernel.theta) > 0
            if trained:
                evals = self._optimise(kernel, X, y, float(jitter), normalize_y, optimizer,
                                       iterations - 1)   # for scikit: 0 restarts => 1 iteration
                fitting_info.update({'lml_evaluations': evals})
            elif iterations == 0:
                fitting_info.update({'fixed': kernel.theta})
            model = HipGPSurrogate.ModelInstance(self, X, y, kernel, float(jitter), normalize_y)
            model._ensure_resident()
        if len(ws) > 0:
            fitting_info.update({'warnings': [w.message for w in ws]})
        if trained:
            # theta is log-transformed (surrogates.py:322-324)
            self._last_model_params = np.exp(kernel.theta.copy())
        fitting_info.update({'fit_ms': model.fit_ms})
        if getattr(self, 'criterion', 'lml') == 'loo':
            fitting_info.update({'criterion': 'loo', 'loo': model.get_loo_log_likelihood()})
        return model, fitting_info

    def _criterion_grad(self, gp, k, X, y, jitter, normalize_y):
        """(score, its gradient w.r.t. log(constant, length scale(s), noise)) of the model-selection criterion at the
        hyper-parameters of kernel ``k``, on handle ``gp``: the one objective of every SciPy-driven route"""
        if getattr(self, 'criterion', 'lml') == 'loo':
            _, loo, grad = gp.fit_loo_grad(X, y, k.kind, k.constant, k.length_scale, k.noise_level, jitter, normalize_y)
            return loo, grad
        return gp.fit_grad(X, y, k.kind, k.constant, k.length_scale, k.noise_level, jitter, normalize_y)

    def _rng(self):
        # sklearn.utils.check_random_state(self.random_state), created per fit (_gpr.py:253)
        seed = self.model_params.get('random_state', None)
        if seed is None or seed is np.random:
            return np.random.mtrand._rand
        if isinstance(seed, numbers.Integral):
            return np.random.RandomState(seed)
        return seed

    def _optimise(self, kernel, X, y, jitter, normalize_y, optimizer, n_restarts):
        """maximise the log marginal likelihood over theta = log(hyper-parameters); mirrors
        GaussianProcessRegressor.fit (_gpr.py:296-337) and _constrained_optimization (:654-670).
        Leaves the best theta in ``kernel``; returns the number of GPU objective evaluations."""
        import scipy.optimize
        ctx = self._context()
        self._resident = None        # the context is about to hold other hyper-parameters
        count = [0]

        def obj_func(theta, eval_gradient=True):
            kernel.theta = theta
            count[0] += 1
            try:
                lml, grad = self._criterion_grad(ctx, kernel, X, y, jitter, normalize_y)
            except np.linalg.LinAlgError:
                # _gpr.py:586-589: not PD -> -inf likelihood, zero gradient
                return (np.inf, np.zeros_like(theta)) if eval_gradient else np.inf
            g = kernel.select_gradient(grad)
            return (-lml, -g) if eval_gradient else -lml

        def constrained_optimization(initial_theta, bounds):
            if optimizer == 'fmin_l_bfgs_b':
                res = scipy.optimize.minimize(obj_func, initial_theta, method='L-BFGS-B', jac=True,
                                              bounds=bounds)
                if res.status != 0:
                    warnings.warn('lbfgs failed to converge (status={}): {}'.format(res.status, res.message))
                return res.x, res.fun
            elif callable(optimizer):
                return optimizer(obj_func, initial_theta, bounds=bounds)
            raise ValueError('Unknown optimizer {}.'.format(optimizer))

        bounds = kernel.theta_bounds
        if optimizer in ('device', 'fmin_l_bfgs_b') and getattr(self, 'criterion', 'lml') == 'lml':   # (the library's optimisers maximise the LML)
            done = self._optimise_in_library(ctx, kernel, X, y, jitter, normalize_y, bounds, n_restarts,
                                             lbfgsb=optimizer == 'fmin_l_bfgs_b')
            if done is not None:
                return done
        if optimizer in ('device', 'scipy'):
            optimizer = 'fmin_l_bfgs_b'      # (or: unbounded theta, criterion='loo') SciPy drives tgp_fit_grad / tgp_fit_loo_grad
        starts = [kernel.theta.copy()]
        if n_restarts > 0:
            if not np.isfinite(bounds).all():
                raise ValueError('Multiple optimizer restarts (n_restarts_optimizer>0) requires '
                                 'that all bounds are finite.')
            rng = self._rng()
            for _ in range(n_restarts):
                starts.append(rng.uniform(bounds[:, 0], bounds[:, 1]))
        n_obs = X.shape[0]
        if self.parallel_restarts_above == 'auto':
            side_by_side, threads = 64 < n_obs <= 8192, 3
        elif self.parallel_restarts_above is None:
            side_by_side, threads = False, 1
        else:
            side_by_side, threads = n_obs > self.parallel_restarts_above, self.restart_threads
        if len(starts) > 1 and side_by_side and optimizer == 'fmin_l_bfgs_b':
            # Above the small-problem sizes one evaluation leaves most of the chip idle (the fit is a
            # serial panel chain): the starts run side by side, one host thread and one handle on a
            # private stream each.  Every start walks exactly the iterates it walks alone (its own
            # L-BFGS-B, its own handle), and scikit-learn draws the restarts' initial points
            # independently of the earlier results (_gpr.py:326-330), so the outcome is unchanged.
            optima = self._optimise_starts_in_threads(kernel, X, y, jitter, normalize_y, bounds, starts, count, threads)
        else:
            optima = [constrained_optimization(t0, bounds) for t0 in starts]
        best = int(np.argmin([o[1] for o in optima]))
        kernel.theta = optima[best][0]
        return count[0]

    def _optimise_starts_in_threads(self, kernel, X, y, jitter, normalize_y, bounds, starts, count, threads):
        # One handle on a private stream per start, borrowed from the DEVICE's pool of worker handles for the duration
        # of this fit (tgp_workers_acquire; round 5).  Round 4 gave every factory three of its own and kept them for its
        # lifetime (creating a stream costs the runtime ~1 ms): with two factories alive in a process the runtime's
        # hardware queues were over-subscribed -- two streams on one queue run one after the other -- and a
        # hyper-parameter fit took twice as long (N = 500: 11.6 -> 19.3 ms).  The pool keeps the streams alive too, but
        # there are at most four of them per device whatever the number of factories.  More starts than workers: the
        # starts take the workers in turn (start j on worker j mod n), each thread owning one worker.
        n = min(len(starts), threads, 4)
        with self._context().workers(n) as workers:
            self._workers = workers          # (what tools look at DURING the fit; the views are dead once the pool is released)
            self.last_worker_count = n       # ... and what stays behind: how many starts ran side by side
            try:
                return self._run_starts(workers, kernel, X, y, jitter, normalize_y, bounds, starts, count, n)
            finally:
                self._workers = []

    def _run_starts(self, workers, kernel, X, y, jitter, normalize_y, bounds, starts, count, threads):
        import scipy.optimize

        evals = [0] * len(starts)     # one cell per start: no shared read-modify-write between the threads

        def run_one(j, w):
            k = kernel.copy()

            def obj_func(theta):
                k.theta = theta
                evals[j] += 1
                try:
                    lml, grad = self._criterion_grad(w, k, X, y, jitter, normalize_y)
                except np.linalg.LinAlgError:
                    return np.inf, np.zeros_like(theta)      # _gpr.py:586-589
                return -lml, -k.select_gradient(grad)

            res = scipy.optimize.minimize(obj_func, starts[j], method='L-BFGS-B', jac=True, bounds=bounds)
            return res.x, res.fun, res.status, res.message

        def run_share(t):                     # thread t owns worker t and walks the starts t, t + n, ... one after the other
            return [(j, run_one(j, workers[t])) for j in range(t, len(starts), len(workers))]

        # (the module's ONE pool of start threads: a ThreadPoolExecutor made per fit spent ~1.2 ms of a 6.6 ms fit at
        # N = 500 starting its three threads -- Thread.start waits for each to come up)
        shares = list(_start_threads().map(run_share, range(len(workers))))
        results = [r for _, r in sorted((jr for share in shares for jr in share), key=lambda jr: jr[0])]
        count[0] += sum(evals)
        for x, f, status, message in results:
            if status != 0:
                warnings.warn('lbfgs failed to converge (status={}): {}'.format(status, message))
        return [(x, f) for x, f, _, _ in results]

    def _optimise_in_library(self, ctx, kernel, X, y, jitter, normalize_y, bounds, n_restarts, lbfgsb):
        """every start (the current theta + n_restarts drawn as scikit-learn draws them, _gpr.py:326-330) optimised
        inside the library, no SciPy and no interpreter between two evaluations.  ``lbfgsb`` (the default optimizer):
        ``tgp_fit_lbfgsb``, L-BFGS-B itself -- SciPy's iterates; otherwise (optimizer='device') ``tgp_fit_optimise``:
        N <= 128 (D <= 64) in ONE launch, a workgroup per start and a projected L-BFGS, above that the same L-BFGS-B.
        The library's vector is log(constant, length scale(s), noise) in full; a FIXED hyper-parameter travels as an entry
        with lo == hi, which the library leaves out of the optimiser's vector as scikit-learn leaves it out of theta.
        A kernel without a noise term travels with that entry fixed at log 0.
        Returns the number of objective evaluations, or None where it does not apply (unbounded theta)."""
        n_ls = len(kernel.length_scale) if kernel.anisotropic else 1
        P = 2 + n_ls
        if (kernel.noise is not None and not kernel.noise > 0) or not np.isfinite(bounds).all():
            return None
        free = np.asarray(kernel.select_gradient(np.arange(P, dtype=np.float64)), dtype=np.int64)   # positions of theta's entries in the full vector
        if len(free) != len(kernel.theta) or len(free) == 0:
            return None
        with np.errstate(divide='ignore'):      # (no noise term: the entry is fixed at log 0)
            full = np.log(np.concatenate([[kernel.constant], np.atleast_1d(np.asarray(kernel.length_scale, dtype=np.float64)),
                                          [kernel.noise_level]]))
        full_bounds = np.stack([full, full], axis=1)
        full_bounds[free] = bounds
        starts = [kernel.theta.copy()]
        if n_restarts > 0:
            rng = self._rng()
            for _ in range(n_restarts):
                starts.append(rng.uniform(bounds[:, 0], bounds[:, 1]))
        full_starts = np.tile(full, (len(starts), 1))
        full_starts[:, free] = np.array(starts)
        theta, f, status, evals = ctx.fit_optimise(X, y, kernel.kind, full_starts, n_ls, full_bounds, jitter,
                                                   normalize_y, max_iter=15000 if lbfgsb else 500, lbfgsb=lbfgsb)
        if lbfgsb:
            for st in status:     # what scikit-learn's _check_optimize_result says of SciPy's status 1 / 2
                if st != 1:
                    warnings.warn('lbfgs failed to converge (status={}): {}'.format(
                        1 if st == 0 else 2, 'STOP: TOTAL NO. OF ITERATIONS REACHED LIMIT' if st == 0
                        else 'ABNORMAL_TERMINATION_IN_LNSRCH'))
        elif np.any(status != 1):
            warnings.warn('on-device L-BFGS did not converge for start(s) {} (status {})'.format(
                np.nonzero(status != 1)[0].tolist(), status[status != 1].tolist()))
        f = np.where(np.isfinite(f), f, np.inf)
        kernel.theta = theta[int(np.argmin(f))][free]
        return int(evals)

    def predict_many(self, models, X, return_std_dev=False):
        """``[m.predict(X, return_std_dev) for m in models]`` as ONE library call per size class for the
        models that are small enough (N <= 128, and 128 < N <= 256): the plot path walks the recorder's trials and predicts
        the same grid with every trial's model (turbo/plotting/trials.py:371,448,574-577;
        turbo/plotting/surrogates.py:23-24,61-65), which otherwise re-fits every stored model in
        turn.  Returns mus (T, M) [, sigmas (T, M)]; rows equal the per-model results (bit for bit for
        N <= 128; to rounding above: the batched fit factors 64 x 64 blocks in another order)."""
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        T, M = len(models), X.shape[0]
        mus = np.empty((T, M))
        sig = np.empty((T, M)) if return_std_dev else None
        groups = {}
        for t, m in enumerate(models):
            native = isinstance(m, HipGPSurrogate.ModelInstance) and m.X.shape[1] == X.shape[1]
            # two size classes, each one library call: N <= 128 (small-problem kernels) and 128 < N <= 256.
            # (a FOREIGN model -- the reference's ModelInstance only carries .model -- has no .X: looked at only when native)
            size_class = None
            if native:
                n_obs = m.X.shape[0]
                size_class = 0 if n_obs <= 128 else (1 if n_obs <= 256 else None)
            key = (m.kernel.kind, bool(m.normalize_y), size_class) if size_class is not None else None
            groups.setdefault(key, []).append(t)
        ctx = self._context()
        for key, members in groups.items():
            if key is None or M == 0 or getattr(ctx, 'host', False):   # (the host backend has no batched entry)
                for t in members:                  # large or foreign models: one by one
                    r = models[t].predict(X, return_std_dev)
                    mus[t] = r[0] if return_std_dev else r
                    if return_std_dev:
                        sig[t] = r[1]
                continue
            specs = [dict(X=models[t].X, y=models[t].y, kind=key[0], constant=models[t].kernel.constant,
                          length_scale=models[t].kernel.length_scale, noise=models[t].kernel.noise_level,
                          jitter=models[t].jitter, normalize_y=key[1]) for t in members]
            mu, sg, lml, clamped = ctx.predict_batch(specs, X, want_sigma=return_std_dev)
            for k, t in enumerate(members):
                mus[t] = mu[k]
                if return_std_dev:
                    sig[t] = sg[k]
                if models[t].log_likelihood is None:
                    models[t].log_likelihood = float(lml[k])
            if clamped > 0 and return_std_dev:
                warnings.warn('Predicted variances smaller than 0. Setting those variances to 0.')
        return (mus, sig) if return_std_dev else mus

    def close(self):
        """release the GPU contexts this factory holds (its own and the concurrent starts' workers, each
        with N^2 fit buffers and a private stream); models re-create the main one on demand"""
        for w in self._workers:
            w.close()
        self._workers = []
        if self._native is not None:
            self._native.close()
            self._native = None
        self._resident = None

    # the GPU context is not picklable; models re-create it lazily (Recorder pickles models,
    # turbo/recorder.py:117-155)
    def __getstate__(self):
        d = dict(self.__dict__)
        d['_native'] = None
        d['_workers'] = []
        d['_resident'] = None
        return d

    def __setstate__(self, d):
        # ANY unpickle marks the factory as reloaded (Recorder.load_compressed, but also copy.deepcopy and a
        # multiprocessing hand-over): in a process without a HIP device such a factory answers predict /
        # acquisition calls from the host backend, with a warning, instead of raising.  In a process WITH a
        # GPU the flag changes nothing.
        self.__dict__.update(d)
        self._reloaded = True

    class ModelInstance(Surrogate.ModelInstance):
        """A GP fitted to one trial's data set.  Holds only host-side state (X, y, theta);
        the factorisation lives in the factory's GPU context and is rebuilt on demand when
        another model has displaced it (models are retained per trial by the Recorder:
        turbo/optimiser.py:343)."""

        def __init__(self, factory, X, y, kernel, jitter, normalize_y):
            self._factory = factory
            self.X = X
            self.y = y
            self.kernel = kernel
            self.jitter = jitter
            self.normalize_y = normalize_y
            self.log_likelihood = None
            self.y_mean = None
            self.y_std = None
            self.fit_ms = None
            self.appended = False

        # ---- native plumbing ----
        def _ensure_resident(self):
            f = self._factory
            ctx = f._context()
            if f._resident is not self:
                k = self.kernel
                ls = k.length_scale
                if np.ndim(ls) > 0:
                    assert len(ls) == self.X.shape[1], \
                        'anisotropic length scale needs one entry per dimension'
                if hasattr(ctx, 'set_overlap') and not getattr(ctx, 'host', False):
                    # the next sweep's batch is resident already (CandidateSweep(prefetch_next=True) drew it on the GPU
                    # behind the previous sweep): this fit starts that sweep inside itself.  Anything that replaced the
                    # resident batch since then cleared gen_key.
                    ctx.set_overlap(2 if (getattr(ctx, 'prefetched', False) and getattr(ctx, 'gen_key', None) is not None) else 0)
                lml, ym, ys = ctx.fit(self.X, self.y, k.kind, k.constant, ls, k.noise_level,
                                      self.jitter, self.normalize_y, append=f.incremental)
                self.appended = ctx.appended
                self.log_likelihood, self.y_mean, self.y_std = lml, ym, ys
                self.fit_ms = ctx.profile_read()['last_fit_ms']
                f._resident = self
            return ctx

        def _sweep(self, X, acq, sf=1.0, incumbent=0.0, param=0.0, want_mu=False,
                   want_sigma=False, want_acq=False):
            ctx = self._ensure_resident()
            X = np.asarray(X, dtype=np.float64)
            if X.ndim == 1 and X.size > 0:
                X = X.reshape(1, -1)
            assert X.ndim == 2 and X.shape[1] == self.X.shape[1], \
                'X must have shape (num_points, {})'.format(self.X.shape[1])
            if X.shape[0] == 0:      # an empty batch: empty results, nothing to launch
                e = np.empty(0)
                return dict(mu=e if want_mu else None, sigma=e.copy() if want_sigma else None,
                            acq=e.copy() if want_acq else None, best_val=float('nan'), best_idx=-1,
                            n_clamped=0)
            if hasattr(ctx, 'evaluate'):     # one call into the library (tgp_evaluate)
                res = ctx.evaluate(X, acq, sf, incumbent, param, want_mu, want_sigma, want_acq)
            else:
                ctx.set_candidates(X)
                res = ctx.sweep(acq, sf, incumbent, param, want_mu, want_sigma, want_acq)
            if res['n_clamped'] > 0 and want_sigma:
                # sklearn/gaussian_process/_gpr.py:480-485
                warnings.warn('Predicted variances smaller than 0. Setting those variances to 0.')
            return res

        # ---- Surrogate.ModelInstance ----
        def predict(self, X, return_std_dev=False):
            """turbo/modules/surrogates.py:332-338: mus (M,) [, sigmas (M,)]"""
            res = self._sweep(X, _lib.ACQ_NONE, want_mu=True, want_sigma=return_std_dev)
            if return_std_dev:
                return res['mu'], res['sigma']
            return res['mu']

        def _points(self, X):
            X = np.asarray(X, dtype=np.float64)
            if X.ndim == 1 and X.size > 0:
                X = X.reshape(1, -1)
            assert X.ndim == 2 and X.shape[1] == self.X.shape[1], \
                'X must have shape (num_points, {})'.format(self.X.shape[1])
            assert 1 <= X.shape[0] <= 4096, 'the joint posterior serves 1 to 4096 points per call'
            return X

        def predict_cov(self, X, latent=False):
            """The JOINT posterior at the rows of X (m <= 4096): ``(mu (m, 1), cov (m, m))``, what the sklearn model the
            reference wraps returns from ``predict(X, return_cov=True)`` (``tgp_predict_cov``).  ``latent=True`` leaves
            the WhiteKernel noise off the diagonal: the covariance of the latent function.  ``cov`` is symmetric bit for
            bit; negative diagonal entries are not clamped (sklearn does not clamp ``y_cov``) but warned about.  Works on
            a reloaded instance where no GPU is visible (the library's host backend)."""
            ctx = self._ensure_resident()
            mu, cov, neg = ctx.predict_cov(self._points(X), latent)
            if neg > 0:
                warnings.warn('{} predicted variances on the diagonal of the joint covariance are smaller than 0'.format(neg))
            return mu.reshape(-1, 1), cov

        def sample_y(self, X, n_samples=1, seed=None, eps=None, latent=False, nugget=1e-10):
            """``n_samples`` <= 4096 exact joint samples of the posterior at the rows of X (m <= 4096), shape
            ``(m, n_samples)`` -- sklearn's ``sample_y`` orientation (``tgp_sample_joint``): mu + y_std Lc eps with Lc
            the Cholesky factor of the joint covariance + ``nugget`` I (the default is the project's default jitter).

            eps:  (n_samples, m) standard normals to use as they are (quasi-random, common random numbers; their row
                  count then IS n_samples), or None:
            seed: on the GPU the normals are Philox-4x32-10 draws keyed by ``seed`` (None: one from ``np.random``), and
                  sample s depends neither on n_samples nor on m.  On a reloaded instance served by the host backend
                  there is no device draw: ``eps`` is drawn with ``np.random.RandomState(seed)`` instead, so the VALUES
                  differ from the device's for the same seed (the distribution does not).
            Raises ``numpy.linalg.LinAlgError`` when the joint covariance is not positive definite at this nugget
            (exactly duplicated rows with ``latent=True`` and ``nugget=0``)."""
            ctx = self._ensure_resident()
            X = self._points(X)
            n_samples = int(n_samples)
            if eps is not None:
                eps = np.atleast_2d(np.asarray(eps, dtype=np.float64))
                n_samples = eps.shape[0]      # (the normals given say how many samples there are)
            if eps is None and getattr(ctx, 'host', False):
                eps = np.random.RandomState(seed).standard_normal((n_samples, X.shape[0]))
            if eps is None and seed is None:
                seed = int(np.random.randint(0, 2**63))
            res = ctx.sample_joint(X, n_samples, 0 if seed is None else seed, eps, latent, nugget)
            return np.ascontiguousarray(res['y'].T)

        def get_hyper_params(self):
            return self.kernel.hyper_params()

        def get_hyper_param_names(self):
            return self.kernel.hyper_param_names()

        def get_log_likelihood(self):
            if self.log_likelihood is None:
                self._ensure_resident()
            return self.log_likelihood

        def loo(self):
            """Leave-one-out cross-validation in closed form (``tgp_loo``): ``(mu_loo (N,), sigma_loo (N,))`` in raw
            units -- the mean and the deviation of the prediction of every training observation from the other N - 1,
            with the hyper-parameters and the normalisation of y held.  sigma_loo is the deviation of the held-out
            OBSERVATION (noise and jitter inside).  Works on a reloaded instance where no GPU is visible."""
            r = self._ensure_resident().loo()
            return self.y - r['resid'], r['sigma']

        def get_loo_log_likelihood(self):
            """L_LOO, the sum of the leave-one-out log predictive densities, in the units of get_log_likelihood"""
            return self._ensure_resident().loo()['loo']

        def __getstate__(self):
            return dict(self.__dict__)


class MarginalisedHipGPSurrogate(HipGPSurrogate):
    """``HipGPSurrogate`` with the hyper-parameters MARGINALISED instead of fixed at a point estimate: the second of the
    two ways the author's older library names (old_library/bayesian_optimiser.py:53-75 'optimise' / 'marginalise', the
    latter's arguments left #TODO at :153-165; the integrated acquisition of Snoek et al. 2012).  ``construct_model``
    first does what the parent does -- the optimised (or fixed) point estimate -- then draws ``n_hyper_samples``
    samples of theta = log(constant, length scale(s), noise) from exp(LML) on the kernel's bounds with the library's slice
    sampler (``tgp_hyper_sample``: ``burn`` sweeps discarded, samples ``thin`` sweeps apart) and returns a
    ``MarginalisedModel``: predictions are the moments of the equal-weight mixture of the S posteriors, and UCB / PI / EI
    over it are the average of the S acquisitions (``tgp_sweep_integrated``).  The chain starts at the point estimate, or
    -- with ``param_continuity`` -- at the previous trial's last sample.  Hyper-parameters the kernel holds fixed stay
    fixed.  ``hyper_seed``: trial t samples with ``(hyper_seed + t * 0x9E3779B97F4A7C15) mod 2**64``; None takes one
    ``np.random.randint(0, 2**63)`` per trial."""

    GOLDEN = 0x9E3779B97F4A7C15

    def __init__(self, *args, n_hyper_samples=8, burn=20, thin=5, hyper_seed=None, **kwargs):
        super().__init__(*args, **kwargs)
        if self.criterion == 'loo':
            raise ValueError("criterion='loo' is a point estimate's criterion: the marginalised surrogate samples exp(LML)")
        n_hyper_samples, burn, thin = int(n_hyper_samples), int(burn), int(thin)
        if n_hyper_samples < 1 or n_hyper_samples > 64:
            raise ValueError('n_hyper_samples must be in [1, 64]')
        if burn < 0 or thin < 1:
            raise ValueError('burn >= 0 and thin >= 1 required')
        self.n_hyper_samples, self.burn, self.thin, self.hyper_seed = n_hyper_samples, burn, thin, hyper_seed
        self._last_sample = None
        self._grad_handles = []      # the gradient stage's float64 contexts, one per hyper-parameter sample: the FACTORY's,
        self._grad_owner = None      # ... holding the fits of this model (models are retained per trial; handles are not)

    def _gradient_handles(self, model):
        """S float64 GPU contexts fitted at ``model``'s samples.  At most ``max S`` of them exist per factory whatever the
        number of models alive: another model's request refits them, ``close()`` releases them."""
        handles = self.__dict__.setdefault('_grad_handles', [])
        if getattr(self._context(), 'host', False):
            raise ValueError('the gradient of a marginalised model needs the GPU')
        S = len(model.thetas)
        if self.__dict__.get('_grad_owner') is not model or len(handles) < S:
            self._grad_owner = None
            while len(handles) < S:
                handles.append(_lib.NativeGP(self.device, 'f64'))
            for gp, th in zip(handles, model.thetas):
                c, ls, noise = model._unpack(th)
                gp.fit(model.X, model.y, model.kernel.kind, c, ls, noise, model.jitter, model.normalize_y)
            self._grad_owner = model
        return handles[:S]

    def close(self):
        for gp in self.__dict__.get('_grad_handles', []):
            gp.close()
        self._grad_handles, self._grad_owner = [], None
        super().close()

    def __getstate__(self):
        d = super().__getstate__()
        d['_grad_handles'], d['_grad_owner'] = [], None
        return d

    def construct_model(self, trial_num, X, y):
        point, fitting_info = super().construct_model(trial_num, X, y)
        kernel = point.kernel
        n_ls = len(kernel.length_scale) if kernel.anisotropic else 1
        P = 2 + n_ls
        with np.errstate(divide='ignore'):      # (no noise term: the entry is fixed at log 0)
            full = np.log(np.concatenate([[kernel.constant], np.atleast_1d(np.asarray(kernel.length_scale, dtype=np.float64)),
                                          [kernel.noise_level]]))
        free = np.asarray(kernel.select_gradient(np.arange(P, dtype=np.float64)), dtype=np.int64)
        bounds = np.stack([full, full], axis=1)
        if len(free) > 0:
            tb = np.asarray(kernel.theta_bounds, dtype=np.float64)
            if not np.isfinite(tb).all():
                raise ValueError('MarginalisedHipGPSurrogate needs finite bounds on every free hyper-parameter')
            bounds[free] = tb
        theta0 = full.copy()
        if self.param_continuity and self._last_sample is not None and self._last_sample.shape == full.shape:
            theta0[free] = np.clip(self._last_sample[free], bounds[free, 0], bounds[free, 1])
        else:
            theta0[free] = np.clip(theta0[free], bounds[free, 0], bounds[free, 1])
        base = int(np.random.randint(0, 2**63)) if self.hyper_seed is None else int(self.hyper_seed)
        seed = (base + int(trial_num) * self.GOLDEN) % (1 << 64)
        ctx = self._context()
        self._resident = None        # the context is about to hold other hyper-parameters
        thetas, lmls, evals, not_pd = ctx.hyper_sample(point.X, point.y, kernel.kind, theta0, n_ls, bounds, point.jitter,
                                                       point.normalize_y, n_samples=self.n_hyper_samples, burn=self.burn,
                                                       thin=self.thin, seed=seed)
        self._last_sample = thetas[-1].copy()
        model = MarginalisedModel(self, point, thetas, lmls, n_ls)
        fitting_info.update({'hyper_samples': thetas.copy(), 'evaluations': int(evals), 'not_pd': int(not_pd),
                             'hyper_seed': seed})
        return model, fitting_info


class MarginalisedModel(Surrogate.ModelInstance):
    """The equal-weight mixture of S GPs that differ in their hyper-parameters ``thetas`` (S, P) = log(constant, length
    scale(s), noise); ``point`` is the point-estimate model of the same data.  ``predict`` returns the mixture's moments,
    mu = mean_k mu_k and sigma = sqrt(mean_k (sigma_k^2 + mu_k^2) - mu^2), from ``tgp_sweep_integrated``; unpickled where no
    GPU is visible it fits S host handles and averages the same moments in NumPy.  Pickles as X, y, the kernel and
    ``thetas``: O(N D + S P)."""

    is_marginalised = True

    def __init__(self, factory, point, thetas, lmls, n_ls):
        self._factory = factory
        self.point = point
        self.X, self.y = point.X, point.y
        self.kernel, self.jitter, self.normalize_y = point.kernel, point.jitter, point.normalize_y
        self.thetas = np.ascontiguousarray(thetas, dtype=np.float64)
        self.lmls = np.asarray(lmls, dtype=np.float64)
        self.n_ls = int(n_ls)

    def _unpack(self, theta):
        # (the C library's exp, entry by entry, as tgp_sweep_integrated forms them: NumPy's vectorised exp may differ in the
        # last bit, and the gradient stage's handles must hold the very models the sweep averages)
        from math import exp
        ls = np.array([exp(float(t)) for t in theta[1:1 + self.n_ls]])
        return exp(float(theta[0])), (ls if self.n_ls > 1 else float(ls[0])), exp(float(theta[-1]))

    def _ensure_resident(self):
        raise ValueError('not available for a marginalised model: this entry works on ONE fitted model '
                         '(batch strategies, Thompson sampling, MES and the on-device gradient stage over a mixture '
                         'of hyper-parameter samples are out of scope)')

    def _resident_context(self):
        """the factory's context with the point estimate's fit -- and so its D -- resident, ready for candidates"""
        ctx = self.point._ensure_resident()
        return ctx

    def _integrated(self, ctx, acq, sf, incumbent, param, want_mu, want_sigma, want_acq):
        """``tgp_sweep_integrated`` over the batch resident in ``ctx``"""
        self._factory._resident = None          # the context ends fitted at the last sample
        res = ctx.sweep_integrated(self.X, self.y, self.kernel.kind, self.thetas, self.n_ls, self.jitter, self.normalize_y,
                                   acq, sf, incumbent, param, want_mu, want_sigma, want_acq)
        if res['n_clamped'] > 0 and want_sigma:
            warnings.warn('Predicted variances smaller than 0. Setting those variances to 0.')
        return res

    def _host_mixture(self, X, acq, sf, incumbent, param, want_mu, want_sigma, want_acq):
        """no GPU in this process (a reloaded model): S host handles, the same sums in NumPy"""
        from .acquisition_functions import _from_mu_sigma
        a = m1 = m2 = None
        clamped = 0
        for th in self.thetas:
            gp = _lib.NativeGP(_lib.DEVICE_HOST, 'f64')
            try:
                c, ls, noise = self._unpack(th)
                gp.fit(self.X, self.y, self.kernel.kind, c, ls, noise, self.jitter, self.normalize_y)
                r = gp.evaluate(X, _lib.ACQ_NONE, 1.0, 0.0, 0.0, True, True, False)
            finally:
                gp.close()
            mu, sg = r['mu'], r['sigma']
            clamped += r['n_clamped']
            ak = _from_mu_sigma(acq, sf, incumbent, param, mu, sg) if acq != _lib.ACQ_NONE else np.zeros_like(mu)
            if a is None:
                a, m1, m2 = np.array(ak, dtype=np.float64), mu.copy(), sg * sg + mu * mu
            else:
                a, m1, m2 = a + ak, m1 + mu, m2 + (sg * sg + mu * mu)
        S = len(self.thetas)
        a, mu = a / S, m1 / S
        sigma = np.sqrt(np.maximum(0.0, m2 / S - mu * mu))
        vals = np.where(np.isnan(a), -np.inf, a)
        bi = int(np.argmax(vals)) if acq != _lib.ACQ_NONE else -1
        return dict(mu=mu if want_mu else None, sigma=sigma if want_sigma else None, acq=a if want_acq else None,
                    best_idx=bi, best_val=float(vals[bi]) if bi >= 0 else float('nan'), n_clamped=clamped)

    def _sweep(self, X, acq, sf=1.0, incumbent=0.0, param=0.0, want_mu=False, want_sigma=False, want_acq=False):
        X = np.asarray(X, dtype=np.float64)
        if X.ndim == 1 and X.size > 0:
            X = X.reshape(1, -1)
        assert X.ndim == 2 and X.shape[1] == self.X.shape[1], 'X must have shape (num_points, {})'.format(self.X.shape[1])
        if X.shape[0] == 0:
            e = np.empty(0)
            return dict(mu=e if want_mu else None, sigma=e.copy() if want_sigma else None, acq=e.copy() if want_acq else None,
                        best_val=float('nan'), best_idx=-1, n_clamped=0)
        if acq == _lib.ACQ_MES:
            raise ValueError('MES is not available for a marginalised model (its maxima belong to one fit)')
        ctx = self._resident_context()
        if getattr(ctx, 'host', False):
            return self._host_mixture(X, acq, sf, incumbent, param, want_mu, want_sigma, want_acq)
        ctx.set_candidates(X)
        return self._integrated(ctx, acq, sf, incumbent, param, want_mu, want_sigma, want_acq)

    def predict(self, X, return_std_dev=False):
        res = self._sweep(X, _lib.ACQ_NONE, want_mu=True, want_sigma=return_std_dev)
        if return_std_dev:
            return res['mu'], res['sigma']
        return res['mu']

    def value_and_grad(self, X, acq, sf, incumbent, param):
        """the integrated acquisition (m,) and its gradient (m, D) at a small batch of points: the mean over the samples
        of the closed form of ``tgp_acq_grad``, each sample on a float64 context that is fitted once per model.  The
        contexts belong to the FACTORY (``MarginalisedHipGPSurrogate._gradient_handles``): S of them per factory, refitted
        when another model asks, released by its ``close()`` -- the device's worker pool holds four, fewer than the samples"""
        owner = getattr(self._factory, '_gradient_handles', None)
        if owner is None:
            raise ValueError('the gradient of a marginalised model needs a MarginalisedHipGPSurrogate factory')
        handles = owner(self)
        v = g = None
        for gp in handles:
            vk, gk = gp.acq_grad(X, acq, sf, incumbent, param)
            v, g = (vk.copy(), gk.copy()) if v is None else (v + vk, g + gk)
        return v / len(handles), g / len(handles)

    def get_hyper_params(self):
        return self.point.get_hyper_params()

    def get_hyper_param_names(self):
        return self.point.get_hyper_param_names()

    def get_log_likelihood(self):
        return self.point.get_log_likelihood()

    def __getstate__(self):
        return dict(_factory=self._factory, X=self.X, y=self.y, kernel=self.kernel, jitter=self.jitter,
                    normalize_y=self.normalize_y, thetas=self.thetas, lmls=self.lmls, n_ls=self.n_ls)

    def __setstate__(self, d):
        self.__dict__.update(d)
        self.point = HipGPSurrogate.ModelInstance(self._factory, self.X, self.y, self.kernel, self.jitter, self.normalize_y)
