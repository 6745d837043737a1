"""Auxiliary optimiser: maximise the acquisition over a batch of M uniform candidates.

Mirror of stage 1 of the reference's ``RandomAndQuasiNewton``
(turbo/modules/auxiliary_optimisers.py:16-129: random stage :59-66, result :114-129) and of
``random_selector`` (turbo/modules/naive_selectors.py:39-46).  Call contract:
``aux_optimiser(latent_bounds, acq) -> (x (1, D), {'max_acq': float})`` (turbo/optimiser.py:340).

With a native acquisition instance the whole sweep (cross-kernel, triangular contraction,
acquisition, arg-max) is one call into libturbogp.so and only the winning (value, index) comes
back.  When ``torch.distributed`` is initialised with more than one rank, every rank sweeps its
own shard of the batch and the winners are combined with one all-gather (RCCL on GPUs).  With the
default ``random_selector`` the shards are rows of the ONE batch NumPy's global RNG holds for the
whole job (ranks seeded alike sweep what a single process would sweep); a generator of the
caller's own is asked for the rank's row count and decides itself what those rows are.

The gradient stage (auxiliary_optimisers.py:69-112) is mirrored too: L-BFGS-B (SciPy, as in the
reference) from the ``start_from_best`` best random candidates plus fresh random starts.  With a
native acquisition instance the gradient comes in closed form from the GPU (``tgp_acq_grad``)
instead of finite differences over 1-point calls, and the restarts advance in LOCK-STEP: each
L-BFGS-B run lives in its own thread and asks for f(x); once every still-running restart has
asked, one ``tgp_acq_grad`` call serves them all (k points per call instead of k calls).  Every
restart sees exactly the values it would see alone, so the result equals the sequential loop.
"""
import collections
import functools
import threading
import warnings

import numpy as np

from .acquisition_functions import topk_tail
from .naive_selectors import random_selector
from .distributed import allgather_argmax, allgather_records, dist_backend, dist_info, shard_plan


def _offers(acq, name):
    """Does this acquisition offer method ``name`` on a model the library holds?  The one test in front of every GPU-only
    extra (two places ask ``hasattr`` alone and say why).  False for one of OUR acquisition instances over a FOREIGN
    model (a Surrogate.ModelInstance that is not HipGPSurrogate's): its value_and_grad / refine / lbfgsb need the GPU
    model, so the gradient stage differentiates 1-point calls by finite differences instead, as the reference does
    (auxiliary_optimisers.py:80-92)"""
    if not hasattr(acq, name):
        return False
    model = getattr(acq, 'model', None)
    return model is None or hasattr(model, '_sweep')     # (no .model at all: a duck-typed instance that brings its own methods)


def _marginalised(acq):
    """an acquisition over a ``MarginalisedModel`` (hyper-parameter samples): the sweep is ``tgp_sweep_integrated``, the
    gradient stage SciPy's over the mean of the samples' closed-form gradients; what needs ONE fitted model is refused"""
    return bool(getattr(getattr(acq, 'model', None), 'is_marginalised', False))


def _warped(acq):
    """an acquisition over a ``WarpedModel`` (turbo_amd/warped.py): its context warps every batch made resident and reads the
    chosen row back raw; what needs more than one sweep of one batch on one GPU is refused"""
    return bool(getattr(getattr(acq, 'model', None), 'is_warped', False))


class _collect_warnings(warnings.catch_warnings):
    """``with _collect_warnings() as caught``: whatever the block warns about goes to the list ``caught``, every time it
    is raised, and not to the caller"""

    def __init__(self):
        super().__init__(record=True)

    def __enter__(self):
        caught = super().__enter__()
        warnings.simplefilter('always')
        return caught


def _one_row(x):
    return np.asarray(x, dtype=np.float64).reshape(1, -1)


def _resident_rows(ctx, order):
    """rows of the batch that only exists on the GPU (the MT19937 stream route)"""
    return np.vstack([ctx.get_candidate(int(i)) for i in order])


# One call of the sweep: what every stage reads.  ``one_batch``: the DEFAULT host draw (random_selector: NumPy's global RNG)
# across ranks -- every rank draws the WHOLE batch of num_random rows and keeps rows [offset, offset + m_local) of it, so
# that ranks started from the same script -- the same np.random.seed -- sweep disjoint shards of the ONE batch a single GPU
# would have swept (and end with the same RNG state), instead of each drawing the same m_local numbers.  (With seeds of
# their own the ranks still get valid, different shards.)  A generator of the caller's own keeps its contract: it is asked
# for m_local rows and decides itself what they are.
_Call = collections.namedtuple('_Call', 'latent_bounds acq bounds marginalised rank world m_local offset one_batch')

# What the random stage hands on: the winner (``best_i`` local to the shard), the ranking the gradient stage starts from --
# None, ``(indices, values)`` best first, or the NEGATED acquisition vector -- and ``rows_of(order)``, rows of the batch.
_Swept = collections.namedtuple('_Swept', 'best_x best_y best_i ranking rows_of')
_NOTHING_SWEPT = _Swept(None, -np.inf, 0, None, None)


class _Lockstep:
    """Rendezvous of k optimiser threads around one batched evaluator ``fn(X (m, D)) -> (v, g)``."""

    def __init__(self, fn, n):
        self.fn = fn
        self.cv = threading.Condition()
        self.active = n
        self.pending = {}
        self.results = {}
        self.error = None
        self.batches = []          # points per batched call (observability / tests)

    def _flush(self):
        # called with the lock held, by whichever thread completed the round
        keys = sorted(self.pending)
        X = np.vstack([self.pending[k] for k in keys])
        self.pending.clear()
        try:
            v, g = self.fn(X)
            v, g = np.asarray(v, dtype=np.float64).reshape(-1), np.asarray(g, dtype=np.float64)
            for i, k in enumerate(keys):
                self.results[k] = (float(v[i]), g[i].copy())
            self.batches.append(len(keys))
        except BaseException as e:      # every waiting restart must wake up and fail
            self.error = e
            for k in keys:
                self.results[k] = None
        self.cv.notify_all()

    def request(self, j, x):
        with self.cv:
            if self.error is not None:
                raise self.error
            self.pending[j] = np.array(x, dtype=np.float64).reshape(1, -1)
            if len(self.pending) == self.active:
                self._flush()
            else:
                self.cv.wait_for(lambda: j in self.results)
            r = self.results.pop(j)
            if r is None:
                raise self.error
            return r

    def done(self, j):
        with self.cv:
            self.active -= 1
            if self.pending and len(self.pending) == self.active:
                self._flush()


class CandidateSweep:
    _warned_host_draw = False     # the large-host-draw hint is given once per process
    STREAM_DRAW_MIN = 1 << 17     # elements of a batch from which the default host draw is finished on the GPU

    def __init__(self, num_random=1000, grad_restarts=0, start_from_best=0, gen_random=None,
                 shard=True, device_rng_seed=None, lockstep=True, on_device=False, max_iter=200,
                 device_design='uniform', prefetch_next=False):
        """
        Args:
            num_random: number of random points to sample to search for the maximum
                (whole job; each rank takes ceil(num_random / world_size) when sharded)
            grad_restarts: number of restarts of the gradient-based optimiser (0 = sweep only)
            start_from_best: how many of those start from the best points of the random stage
                (should be <= num_random and <= grad_restarts)
            gen_random: candidate generator ``(num_points, latent_bounds) -> (M, D)``;
                defaults to ``random_selector()``
            shard: split the batch over the ranks of torch.distributed when initialised
            device_rng_seed: None (default) draws candidates like the reference, on the host
                from the global NumPy RNG.  An integer draws them ON the GPU instead (Philox
                stream seed + call number; shards are disjoint pieces of one stream), so the
                batch never crosses PCIe.  Needs a native acquisition instance.
            lockstep: run the gradient restarts in lock-step over batched gradient calls (native acquisition
                instances).  True (default): L-BFGS-B walked inside the library (``tgp_acq_lbfgsb``: SciPy's algorithm in
                C++, one batched evaluation per round, each restart's walk the one SciPy would take); 'scipy': a
                Python thread and a SciPy L-BFGS-B per restart meeting at a rendezvous (rounds 2-4's default);
                False: SciPy, one restart after the other
            on_device: run the gradient stage as a batched projected L-BFGS ON the GPU
                (``tgp_acq_refine``: every restart resident; N <= 128 the whole stage in one launch,
                above one launch sequence per iteration for all restarts)
                instead of SciPy's L-BFGS-B on the host.  Needs a native acquisition instance.
            max_iter: iteration cap of the on-device optimiser
            prefetch_next: with ``device_rng_seed``: draw the NEXT call's batch right behind this call's sweep, so that
                the next trial's fit starts that batch's sweep inside itself (``tgp_set_overlap``: the candidates do
                not depend on the model; turbo/optimiser.py:336-340 runs fit and maximisation back to back).  The
                candidates, the values and the chosen points are those of ``prefetch_next=False``, bit for bit.
            device_design: with ``device_rng_seed``: 'uniform' (independent uniform candidates, the
                counterpart of ``random_selector``) or 'lhs' (the whole batch of ``num_random``
                candidates is one Latin hypercube design, the counterpart of ``LHS_selector``;
                shards are rows of that one design)
        """
        assert num_random > 0, 'the candidate sweep needs num_random > 0'
        assert start_from_best <= num_random
        assert start_from_best <= grad_restarts
        self.num_random = num_random
        self.grad_restarts = grad_restarts
        self.start_from_best = start_from_best
        self.gen_random = gen_random or random_selector()
        self.shard = shard
        self.device_rng_seed = device_rng_seed
        self.lockstep = lockstep
        self.on_device = on_device
        self.max_iter = max_iter
        assert device_design in ('uniform', 'lhs')
        self.device_design = device_design
        self.prefetch_next = bool(prefetch_next)
        self.last_batches = None
        self._calls = 0

    # ------------------------------------------------------------------------------------------------ batch selection

    def select_batch(self, latent_bounds, acq, q, strategy='kriging_believer', lie='min', pending=None, n_sim=16,
                     seed=None):
        """q points for q parallel workers from ONE batch of candidates, drawn exactly as ``__call__`` draws it, chosen
        greedily with Kriging Believer / Constant Liar and conditioned first on ``pending`` (P, D): the trials still
        running (``FunctionInstance.maximise_batch``, ``tgp_sweep_batch``).  Returns (x (q, D), info) with info =
        {'max_acq' (q,), 'candidate_indices' (q,), 'fantasies' (q,), 'pending_fantasies' (P,), 'strategy'}.

        strategy='monte_carlo' (``tgp_sweep_batch_mc``): the average of the acquisition over ``n_sim`` <= 64 joint
        simulations of the pending and chosen points' outcomes is maximised; ``seed`` keys their random numbers (None:
        one ``np.random.randint(0, 2**63)`` taken after the candidates are drawn, as ``TS`` takes its seed; with a seed
        given the NumPy RNG is consumed as by one ``__call__``).  info then holds 'fantasies' (n_sim, q),
        'pending_fantasies' (n_sim, P), 'n_sim' and 'seed'.  The other strategies ignore both arguments.

        strategy='thompson' with a ``TS`` acquisition: q distinct rows, row s the best of sample path s of one draw of q
        paths (asynchronous Thompson sampling: ``pending`` is accepted and ignored).  info = {'max_acq' (q,) sf * sampled
        value, 'candidate_indices' (q,), 'sample_values' (q,) raw, 'strategy', 'seed', 'n_features', 'pending_ignored'}."""
        self._check_select_batch(acq, strategy)
        bounds = [(lb[1], lb[2]) for lb in latent_bounds.ordered]
        if pending is not None:
            pending = np.asarray(pending, dtype=np.float64).reshape(-1, len(bounds))
        if self.device_rng_seed is not None:
            # the batch maximise_generated would draw for this call (or has prefetched), left resident
            low, high = zip(*bounds)
            acq.model._ensure_resident().generate(self.device_rng_seed + self._calls, 0, self.num_random, low, high,
                                                  self.num_random if self.device_design == 'lhs' else None, reuse=True)
            X = None
        else:
            X = self.gen_random(self.num_random, latent_bounds)
        res = acq.maximise_batch(X, q, strategy, lie, pending, n_sim=n_sim, seed=seed)
        self._calls += 1
        info = self._batch_info(acq, strategy, res, 0 if pending is None else len(pending))
        if res.get('sweep_ms') is not None:
            info['sweep_ms'] = res['sweep_ms']
        return np.asarray(res['x'], dtype=np.float64), info

    def _check_select_batch(self, acq, strategy):
        if _marginalised(acq):
            raise ValueError('select_batch is not available for a marginalised model: batch strategies over a mixture of '
                             'hyper-parameter samples are out of scope')
        if _warped(acq):
            raise ValueError('select_batch is not available for a warped model (WarpedHipGPSurrogate): batch strategies '
                             'condition on fantasies in the warped space, which is out of scope')
        thompson = bool(getattr(acq, 'is_thompson', False))
        if strategy == 'thompson' and not thompson:
            raise ValueError("strategy='thompson' needs a TS acquisition (got {!r})".format(type(acq)))
        if thompson and strategy != 'thompson':
            raise ValueError("a TS acquisition selects batches with strategy='thompson' only (got {!r})".format(strategy))
        if self.grad_restarts > 0:
            raise NotImplementedError('select_batch: no gradient refinement of the selected points (grad_restarts > 0)')
        if self.shard and dist_info()[1] > 1:
            raise NotImplementedError('select_batch: one process only (a batch sharded over ranks needs an all-gather '
                                      'per selection)')
        if not _offers(acq, 'maximise_batch') or getattr(acq, 'model', None) is None:
            raise NotImplementedError('select_batch needs a native acquisition over a model built by HipGPSurrogate '
                                      '(got {!r})'.format(type(getattr(acq, 'model', acq))))

    @staticmethod
    def _batch_info(acq, strategy, res, P):
        """the info of ``select_batch`` from ``maximise_batch``'s dict; P pending points come first among the fantasies"""
        info = {'max_acq': res['val'], 'candidate_indices': res['idx']}
        if strategy == 'thompson':
            info.update({'max_acq': acq.scale_factor * np.asarray(res['val']), 'sample_values': res['val'], 'strategy': strategy,
                         'seed': res['seed'], 'n_features': res['n_features'], 'pending_ignored': res['pending_ignored']})
        elif strategy == 'monte_carlo':
            info.update({'fantasies': res['fantasies'][:, P:], 'pending_fantasies': res['fantasies'][:, :P],
                         'strategy': strategy, 'n_sim': res['n_sim'], 'seed': res['seed']})
        else:
            info.update({'fantasies': res['fantasies'][P:], 'pending_fantasies': res['fantasies'][:P], 'strategy': strategy})
        return info

    # ------------------------------------------------------------------------------------------------ one point

    def __call__(self, latent_bounds, acq):
        """Returns: x (1, num_attribs) within the bounds, {'max_acq': value}"""
        c = self._plan(latent_bounds, acq)
        rec = self._winner_record(c)
        swept = self._random_stage(c)
        self._calls += 1
        info = {}
        if hasattr(acq, 'last_sweep_ms') and acq.last_sweep_ms is not None:
            info['sweep_ms'] = acq.last_sweep_ms
        best_x, best_y, best_i, from_sweep = swept.best_x, swept.best_y, swept.best_i, True
        if self.grad_restarts > 0:      # minimise by gradient-based optimiser (auxiliary_optimisers.py:69-112)
            best_x, best_y, best_i, from_sweep = self._gradient_stage(c, swept, info)
        if c.world > 1:
            best_x, best_y = self._exchange(c, rec if from_sweep else None, best_x, best_y, best_i, info)
        if from_sweep:
            best_y = self._report_f64(acq, best_x, best_y, info)
        # ensure that the chosen value lies within the bounds (auxiliary_optimisers.py:120-124)
        low_bounds, high_bounds = zip(*c.bounds)
        best_x = np.clip(best_x, low_bounds, high_bounds)
        info.update({'max_acq': float(best_y)})
        return best_x, info

    def _plan(self, latent_bounds, acq):
        """who sweeps which rows of the batch: contiguous shards of ONE batch of num_random candidates;
        global index = offset + local index, so the tie rule (lowest index) does not depend on the world size"""
        marginalised = _marginalised(acq)
        if marginalised and self.on_device:
            raise ValueError('on_device=True is not available for a marginalised model: the on-device gradient stage '
                             'refines ONE fitted model (the SciPy path serves the integrated acquisition)')
        rank, world = dist_info() if self.shard else (0, 1)
        if world > 1 and _warped(acq):
            raise ValueError('a warped model (WarpedHipGPSurrogate) is swept by one process only: the sharded multi-GPU sweep '
                             'is out of scope')
        m_local, offset, _ = shard_plan(self.num_random, world, rank)
        if world > 1 and getattr(acq, 'is_thompson', False):
            raise NotImplementedError('TS: one process only (the sharded multi-rank sweep is not available for sample paths)')
        one_batch = world > 1 and type(self.gen_random) is random_selector and self.device_rng_seed is None
        return _Call(latent_bounds, acq, [(lb[1], lb[2]) for lb in latent_bounds.ordered], marginalised, rank, world,
                     m_local, offset, one_batch)

    def _winner_record(self, c):
        """with RCCL the winner record [value, global index, row] is packed on the GPU by the sweep itself and
        all-gathered from there; None: the winners are exchanged from the host"""
        if c.world > 1 and c.m_local > 0 and _offers(c.acq, 'winner_record') and dist_backend() == 'nccl':
            return c.acq.winner_record(c.offset)
        return None

    # ---- the random stage: every step returns a _Swept

    def _random_stage(self, c):
        if c.m_local == 0:
            return self._pass_over(c)
        if self.device_rng_seed is not None:
            return self._sweep_generated(c)
        swept = self._sweep_host_stream(c)
        if swept is None:
            self._hint_large_host_draw(c)
            swept = self._sweep_host_batch(c)
        return swept

    def _pass_over(self, c):
        """more ranks than candidates: this rank only takes part in the exchange (and, on the default draw, passes over
        the batch so that its RNG stays in step with the other ranks')"""
        if c.one_batch:
            self.gen_random(self.num_random, c.latent_bounds)
        return _NOTHING_SWEPT

    def _sweep_generated(self, c):
        """the batch drawn ON the GPU (uniform, or rows of one Latin hypercube design), the next call's behind it"""
        # hasattr alone: the method is for every model the library can sweep -- a mixture too -- and refuses the rest itself
        assert hasattr(c.acq, 'maximise_generated'), 'device_rng_seed needs a native acquisition'
        low, high = zip(*c.bounds)
        seed = self.device_rng_seed + self._calls
        best_x, best_y, best_i = c.acq.maximise_generated(
            c.m_local, low, high, seed, first_candidate=c.offset,
            lhs_total=self.num_random if self.device_design == 'lhs' else None,
            prefetch_seed=(seed + 1) if self.prefetch_next else None)
        return _Swept(_one_row(best_x), best_y, best_i, None, None)

    def _sweep_host_stream(self, c):
        """The reference's draw (random_selector: NumPy's global RNG) for a native acquisition and a large batch: only the
        generator's sequential recurrence runs on the host, inside the library; the GPU forms the doubles and keeps the
        batch (tgp_set_candidates_mt19937) -- the numbers, the winner and np.random's state afterwards are those of the
        host loop, bit for bit (tests/test_gpu_host_stream.py).  None: not this route, or refused -- nothing was drawn."""
        if not (type(self.gen_random) is random_selector and _offers(c.acq, 'maximise_host_stream')
                and c.m_local * len(c.bounds) >= self.STREAM_DRAW_MIN
                and not (self.grad_restarts > 0 and self.start_from_best > 64)):
            return None
        k = self.start_from_best if self.grad_restarts > 0 else 0
        low, high = zip(*c.bounds)
        try:
            low, high = [float(v) for v in low], [float(v) for v in high]
            if c.one_batch:
                stream = c.acq.maximise_host_stream(self.num_random, low, high, topk=k, first=c.offset, count=c.m_local)
            else:
                stream = c.acq.maximise_host_stream(c.m_local, low, high, topk=k)
        except (TypeError, ValueError):
            return None
        if stream is None:
            return None
        ctx, best_i, best_y, top = stream
        rows_of = functools.partial(_resident_rows, ctx)
        return _Swept(_one_row(rows_of([best_i])), best_y, best_i, top, rows_of)

    def _hint_large_host_draw(self, c):
        """once per process: a candidate generator of the caller's own at BASELINE's headline sizes -- the batch is formed
        on the host and uploaded (NumPy's own loop for C3's 262 144 x 32: 45-66 ms for a 35 ms GPU step)"""
        if c.m_local * len(c.bounds) > 1000000 and not CandidateSweep._warned_host_draw and _offers(c.acq, 'maximise_generated'):
            CandidateSweep._warned_host_draw = True
            warnings.warn('CandidateSweep draws {} x {} candidates on the host with {}: at this size the draw and its upload cost '
                          'more than the GPU sweep -- the default random_selector (same numbers as the reference, finished on the '
                          'GPU) or device_rng_seed=<int> avoid that'.format(c.m_local, len(c.bounds), type(self.gen_random).__name__))

    def _sweep_host_batch(self, c):
        """the batch drawn on the host and handed over: ``maximise``, ``maximise_topk`` or the acquisition as a callable"""
        acq = c.acq
        if c.one_batch:
            random_x = self.gen_random(self.num_random, c.latent_bounds)[c.offset:c.offset + c.m_local]
        else:
            random_x = self.gen_random(c.m_local, c.latent_bounds)
        # hasattr alone: OUR instances over a foreign model do answer ``maximise`` (the formula in NumPy over its predict)
        if hasattr(acq, 'maximise') and not (self.grad_restarts > 0 and self.start_from_best > 0):
            best_i, best_y = acq.maximise(random_x)
            ranking = None
        elif _offers(acq, 'maximise_topk') and not c.marginalised and self.grad_restarts > 0 and self.start_from_best <= 64:
            # the best start_from_best candidates come back from the GPU (tgp_sweep_topk, k <= 64); the (M,) acquisition
            # vector stays there.  More starts than that take the branch below (the vector comes back and is argsorted
            # here, as the reference does).
            ranking, best_i, best_y = topk_tail(*acq.maximise_topk(random_x, self.start_from_best), ranked_only=True)
        else:
            # a foreign acquisition callable: same argsort/[0] semantics as the reference
            # (auxiliary_optimisers.py:61-66), NaNs last
            ranking = -np.asarray(acq(random_x))
            best_i = int(np.argsort(ranking, axis=0, kind='stable').flatten()[0])
            best_y = float(-ranking[best_i])
        return _Swept(_one_row(random_x[[best_i]]), best_y, best_i, ranking, random_x.__getitem__)

    # ---- the gradient stage: every route returns [(x, fun) | (None, None)] in restart order

    def _gradient_stage(self, c, swept, info):
        starting_points = self._starting_points(c, swept)
        with _collect_warnings() as caught:
            results = self._gradient_route(c)(c, starting_points, info)
        best_x, best_y, best_i, from_sweep = swept.best_x, swept.best_y, swept.best_i, True
        for j, (res_x, res_y) in enumerate(results):   # in restart order, as the reference's loop
            if res_y is not None and -res_y > best_y:
                best_x, best_y, from_sweep = _one_row(res_x), -res_y, False
                # not a member of the random batch: global indices past the batch, one block
                # of grad_restarts per rank, so no two winners of a job share an index
                best_i = (self.num_random - c.offset) + c.rank * self.grad_restarts + j
        if len(caught) > 0:
            info.update({'warnings': [w.message for w in caught]})
        return best_x, best_y, best_i, from_sweep

    def _starting_points(self, c, swept):
        """the ``start_from_best`` best rows of the batch first, fresh random points for the rest"""
        n_best = self.start_from_best if swept.ranking is not None else 0
        starts = []
        if n_best > 0:
            if isinstance(swept.ranking, tuple):
                order = np.asarray(swept.ranking[0], dtype=np.int64)[:n_best]
            else:
                order = np.argsort(swept.ranking, axis=0, kind='stable').flatten()[:n_best]
            n_best = len(order)     # (fewer when the batch ranked fewer: the rest start at random)
            starts.append(swept.rows_of(order))
        if self.grad_restarts - n_best > 0:
            starts.append(self.gen_random(self.grad_restarts - n_best, c.latent_bounds))
        starting_points = np.vstack(starts)
        assert len(starting_points) == self.grad_restarts
        return starting_points

    def _gradient_route(self, c):
        if self.on_device and _offers(c.acq, 'refine'):
            return self._restarts_on_device
        if self.lockstep and self.lockstep != 'scipy' and _offers(c.acq, 'lbfgsb') and not c.marginalised:
            return self._restarts_in_library
        if self.lockstep and _offers(c.acq, 'value_and_grad') and self.grad_restarts > 1:
            return self._restarts_in_threads
        return self._restarts_one_by_one

    def _restarts_on_device(self, c, starting_points, info):
        """all restarts advance together ON the GPU (tgp_acq_refine): no Python threads, no SciPy, one kernel sequence
        per iteration for every restart"""
        xs, vs, its = c.acq.refine(starting_points, c.bounds, max_iter=self.max_iter)
        info['refine_iterations'] = int(its)
        return [(xs[j], -float(vs[j])) for j in range(len(vs))]

    def _restarts_in_library(self, c, starting_points, info):
        """L-BFGS-B from every start as the reference runs it, walked inside the library (tgp_acq_lbfgsb): the restarts in
        lock-step on one thread, one batched gradient evaluation per round, no interpreter between two rounds -- each
        restart's walk is the one SciPy would take on the same objective"""
        xs, vs, status, evals = c.acq.lbfgsb(starting_points, c.bounds, max_iter=15000)
        results = []
        for j in range(len(vs)):
            if status[j] != 1:          # SciPy's `not result.success` (auxiliary_optimisers.py:93-97)
                warnings.warn('restart {}/{} of gradient-based optimisation failed'.format(j, self.grad_restarts))
                results.append((None, None))
            else:
                results.append((xs[j], -float(vs[j])))
        info['gradient_evaluations'] = int(evals)
        return results

    def _restarts_in_threads(self, c, starting_points, info):
        return self._bfgs_lockstep(c.acq, starting_points, c.bounds)

    def _restarts_one_by_one(self, c, starting_points, info):
        return [self._bfgs(c.acq, starting_points[j], c.bounds, j) for j in range(self.grad_restarts)]

    # ---- after the stages

    def _exchange(self, c, rec, best_x, best_y, best_i, info):
        """one all-gather of the ranks' winners: the records the sweeps packed on the GPU (``rec``), or -- a gradient
        restart won, no RCCL, no record -- (value, row, global index) from the host.  Returns the job's (x, value)"""
        if rec is not None:
            best_y, best_x, owner = allgather_records(rec, ctx=getattr(getattr(c.acq.model, '_factory', None), '_native', None))
        else:
            if best_x is None:
                best_x = np.zeros((1, len(c.bounds)))
            best_y, best_x, owner = allgather_argmax(best_y, best_x, c.offset + best_i)
        info['shards'] = c.world
        info['best_global_index'] = owner
        return best_x, best_y

    def _report_f64(self, acq, best_x, best_y, info):
        """A sweep in f32 arithmetic (dtype 'f32' / 'f32h2' / 'f32x3': BASELINE configs 3 and 4) ranks the batch with a
        mean that carries the f32 rounding of the cross-kernel (|d mu| up to 1e-4 y_std at C3).  The value REPORTED for
        the chosen point is formed once more in float64 -- cross-kernel row, mean, variance and acquisition at that one
        point (tgp_acq_grad: closed form on the f64 factor) -- so max_acq meets the fp64 bar; the sweep's own figure
        stays in the info.  Every rank holds the same model and, after the exchange, the same point: the refined value
        is the same everywhere."""
        if best_x is None or getattr(acq, 'sweep_dtype', 'f64') == 'f64' or not _offers(acq, 'value_and_grad'):
            return best_y
        v64, _ = acq.value_and_grad(_one_row(best_x))
        if np.isfinite(v64[0]):
            info['max_acq_sweep'] = float(best_y)
            return float(v64[0])
        return best_y


    def _minimise(self, neg_f, jac, starting_point, bounds, j):
        import scipy.optimize
        x0 = np.asarray(starting_point, dtype=np.float64).reshape(-1)
        result = scipy.optimize.minimize(fun=neg_f, x0=x0, jac=jac, bounds=bounds, method='L-BFGS-B',
                                         options=dict(maxiter=15000))
        if not result.success:
            warnings.warn('restart {}/{} of gradient-based optimisation failed'.format(
                j, self.grad_restarts))
            return None, None
        return result.x, float(result.fun)

    def _bfgs(self, acq, starting_point, bounds, j):
        """one L-BFGS-B run on -acq (auxiliary_optimisers.py:80-99); (x, fun) or (None, None)"""
        if _offers(acq, 'value_and_grad'):
            def neg_f(x):
                v, g = acq.value_and_grad(x.reshape(1, -1))
                return -float(v[0]), -g[0]
            jac = True
        else:
            def neg_f(x):
                return -float(np.asarray(acq(x.reshape(1, -1))).reshape(-1)[0])
            jac = None
        return self._minimise(neg_f, jac, starting_point, bounds, j)

    def _bfgs_lockstep(self, acq, starting_points, bounds):
        """all restarts at once: one thread per L-BFGS-B run, one batched gradient call per round"""
        n = len(starting_points)
        sync = _Lockstep(acq.value_and_grad, n)
        out = [(None, None)] * n
        errors = [None] * n

        def run(j):
            def neg_f(x):
                v, g = sync.request(j, x)
                return -v, -g
            try:
                out[j] = self._minimise(neg_f, True, starting_points[j], bounds, j)
            except BaseException as e:
                errors[j] = e
            finally:
                sync.done(j)

        threads = [threading.Thread(target=run, args=(j,), name='tgp-restart-%d' % j) for j in range(n)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        self.last_batches = sync.batches
        for e in errors:
            if e is not None:
                raise e
        return out


class RandomAndQuasiNewton(CandidateSweep):
    """the reference's name for this slot WITH the reference's defaults (turbo/modules/auxiliary_optimisers.py:17:
    ``num_random=1000, grad_restarts=10, start_from_best=2``), so that code and presets written against it keep their
    meaning: ``RandomAndQuasiNewton()`` runs the gradient stage, ``CandidateSweep()`` is the pure sweep.  Everything
    else is ``CandidateSweep``."""

    def __init__(self, num_random=1000, grad_restarts=10, start_from_best=2, **kwargs):
        super().__init__(num_random=num_random, grad_restarts=grad_restarts, start_from_best=start_from_best, **kwargs)
