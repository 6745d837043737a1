"""Every route of ``CandidateSweep.__call__`` and ``select_batch``, walked on a CPU with duck-typed acquisitions.

An acquisition here is an object with a chosen SUBSET of the methods the sweep probes for (``maximise``, ``maximise_topk``,
``maximise_host_stream``, ``maximise_generated``, ``value_and_grad``, ``refine``, ``lbfgsb``, ``maximise_batch``); every
method appends what it was asked to one list.  Each case pins the exact ordered call list, the returned point, every key
and value of the info, the warnings' texts and where ``np.random`` stands afterwards (key and position).  The expected
values are re-derived here from NumPy's draws and from SciPy runs of the test's own, never read back from the sweep.
"""
import warnings

import numpy as np
import pytest
import scipy.optimize

from turbo_amd.auxiliary_optimisers import CandidateSweep

CENTRE = np.array([0.3, 0.5])
LOW, HIGH = (0.0, -1.0), (1.0, 2.0)
PAIRS = [(0.0, 1.0), (-1.0, 2.0)]
SEED = 11


class _Bounds:
    ordered = [('a', 0.0, 1.0), ('b', -1.0, 2.0)]


BOUNDS = _Bounds()


def f(X):
    """the acquisition of every stub: one smooth maximum, 0 at CENTRE, inside the bounds"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    return -((X - CENTRE) ** 2).sum(axis=1)


def grad(X):
    X = np.asarray(X, dtype=np.float64).reshape(-1, 2)
    return -2.0 * (X - CENTRE)


def draw(n):
    """random_selector's draw: a column per parameter from NumPy's global RNG"""
    return np.hstack([np.random.uniform(lo, hi, size=(n, 1)) for lo, hi in PAIRS])


def state():
    st = np.random.get_state()
    return st[1].tobytes(), int(st[2])


# ---------------------------------------------------------------------------------------------------- the stubs


class _Ctx:
    def __init__(self, calls, X):
        self.calls, self.X = calls, X

    def get_candidate(self, i):
        self.calls.append(('get_candidate', int(i)))
        return self.X[int(i)].copy()


def _call(self, X):
    X = np.asarray(X)
    self.calls.append(('call', X.shape))
    return f(X)


def _maximise(self, X):
    self.calls.append(('maximise', np.asarray(X).shape))
    v = f(X)
    i = int(np.argmax(v))
    return i, float(v[i]) + self.sweep_error


def _maximise_topk(self, X, k):
    self.calls.append(('maximise_topk', np.asarray(X).shape, int(k)))
    v = f(X)
    order = np.argsort(-v, kind='stable')[:int(k)]
    return order.astype(np.int64), v[order]


def _maximise_host_stream(self, num_points, low, high, topk=0, first=0, count=None):
    self.calls.append(('maximise_host_stream', int(num_points), tuple(low), tuple(high), int(topk), int(first), count))
    if self.stream_refuses:
        return None
    X = np.hstack([np.random.uniform(lo, hi, size=(num_points, 1)) for lo, hi in zip(low, high)])
    v = f(X)
    ctx = _Ctx(self.calls, X)
    if topk > 0:
        order = np.argsort(-v, kind='stable')[:int(topk)]
        return ctx, int(order[0]), float(v[order[0]]), (order.astype(np.int64), v[order])
    i = int(np.argmax(v))
    return ctx, i, float(v[i]), None


def generated_batch(num_points, seed):
    return np.random.RandomState(int(seed)).uniform(LOW, HIGH, size=(int(num_points), 2))


def _maximise_generated(self, num_points, low, high, seed, first_candidate=0, lhs_total=None, prefetch_seed=None):
    self.calls.append(('maximise_generated', int(num_points), tuple(low), tuple(high), seed, first_candidate, lhs_total,
                       prefetch_seed))
    X = generated_batch(num_points, seed)
    v = f(X)
    i = int(np.argmax(v))
    return X[i], float(v[i]), i


def _value_and_grad(self, X):
    X = np.asarray(X)
    self.calls.append(('value_and_grad', X.shape))
    return f(X), grad(X)


def _refine(self, starting_points, bounds, max_iter=200):
    self.calls.append(('refine', np.asarray(starting_points).shape, list(bounds), max_iter))
    warnings.warn('restart 1 of the on-device optimisation stopped at max_iter')
    x = 0.5 * (np.asarray(starting_points) + CENTRE)        # half way to the maximum: better than any start
    return x, f(x), 17


def _lbfgsb(self, starting_points, bounds, max_iter=15000):
    self.calls.append(('lbfgsb', np.asarray(starting_points).shape, list(bounds), max_iter))
    x = 0.5 * (np.asarray(starting_points) + CENTRE)
    v = f(x)
    status = np.ones(len(x), dtype=np.int64)
    for j in self.failed_restarts:       # a failed restart reports the best value of all: it must not be taken
        status[j], v[j] = 0, 1.0
    return x, v, status, 23


def _maximise_batch(self, X, q, strategy='kriging_believer', lie='min', pending=None, want_posterior=False, n_sim=16, seed=None):
    self.calls.append(('maximise_batch', None if X is None else np.asarray(X).shape, q, strategy, lie,
                       None if pending is None else np.asarray(pending).shape, n_sim, seed))
    return self.batch_result


IMPL = {'maximise': _maximise, 'maximise_topk': _maximise_topk, 'maximise_host_stream': _maximise_host_stream,
        'maximise_generated': _maximise_generated, 'value_and_grad': _value_and_grad, 'refine': _refine, 'lbfgsb': _lbfgsb,
        'maximise_batch': _maximise_batch}


class _NativeModel:
    def _sweep(self, *a, **k):
        raise AssertionError('the stub model is never swept')


class _MarginalisedModel(_NativeModel):
    is_marginalised = True


class _ForeignModel:
    def predict(self, X, return_std_dev=False):
        raise AssertionError('the stub model is never asked')


def make_acq(methods, **attrs):
    """a callable with exactly these methods besides ``__call__``; ``acq.calls`` is what it was asked, in order"""
    ns = {name: IMPL[name] for name in methods}
    ns['__call__'] = _call
    acq = type('DuckAcq', (), ns)()
    acq.calls = []
    acq.sweep_error = 0.0
    acq.stream_refuses = False
    acq.failed_restarts = ()
    for k, v in attrs.items():
        setattr(acq, k, v)
    return acq


def run(sweep, acq, seed=SEED):
    np.random.seed(seed)
    with warnings.catch_warnings(record=True) as ws:
        warnings.simplefilter('always')
        x, info = sweep(BOUNDS, acq)
    return x, info, [str(w.message) for w in ws], state()


# ---------------------------------------------------------------------------------------------------- the expectations


def scipy_run(x0, closed_form):
    """one L-BFGS-B run as the reference runs it (auxiliary_optimisers.py:80-99): (x, fun, evaluations)"""
    n = [0]
    if closed_form:
        def fun(x):
            n[0] += 1
            return -float(f(x)[0]), -grad(x)[0]
    else:
        def fun(x):
            n[0] += 1
            return -float(f(x)[0])
    r = scipy.optimize.minimize(fun=fun, x0=np.asarray(x0, dtype=np.float64).reshape(-1), jac=True if closed_form else None,
                                bounds=PAIRS, method='L-BFGS-B', options=dict(maxiter=15000))
    assert r.success
    return r.x, float(r.fun), n[0]


def merged(best_x, best_y, results):
    """the reference's loop over the restarts, in order: a restart wins only with a strictly larger value"""
    for x, fun in results:
        if fun is not None and -fun > best_y:
            best_x, best_y = np.asarray(x, dtype=np.float64), -fun
    return np.clip(best_x.reshape(1, -1), LOW, HIGH), float(best_y)


def lockstep_rounds(evaluations):
    """points per batched gradient call when every restart asks once per round until it is done"""
    return [sum(1 for n in evaluations if n > r) for r in range(max(evaluations))]


def expect_host(num_random, n_best, n_fresh, seed=SEED):
    """the host draw: the batch, its ranking, the starting points (ranked rows first, fresh ones behind) and the RNG state"""
    np.random.seed(seed)
    Xc = draw(num_random)
    v = f(Xc)
    order = np.argsort(-v, kind='stable')
    starts = [Xc[order[:n_best]]] if n_best > 0 else []
    if n_fresh > 0:
        starts.append(draw(n_fresh))
    return Xc, v, order, (np.vstack(starts) if starts else None), state()


def check(got, calls, x, info, texts, st):
    gx, ginfo, gtexts, gst, gcalls = got
    assert gcalls == calls
    np.testing.assert_array_equal(gx, x)
    assert gx.shape == (1, 2) and gx.dtype == np.float64
    ginfo = dict(ginfo)
    if 'warnings' in ginfo:
        ginfo['warnings'] = [str(m) for m in ginfo['warnings']]
    assert ginfo == info
    assert all(type(ginfo[k]) is type(info[k]) for k in info)
    assert gtexts == texts
    assert gst == st


def go(sweep, acq, seed=SEED):
    x, info, texts, st = run(sweep, acq, seed)
    return x, info, texts, st, list(acq.calls)


# ---------------------------------------------------------------------------------------------------- __call__: the random stage


def test_bare_callable_sweep_only():
    Xc, v, order, _, st = expect_host(50, 0, 0)
    acq = make_acq([])
    check(go(CandidateSweep(num_random=50), acq), [('call', (50, 2))], Xc[order[:1]], {'max_acq': float(v[order[0]])}, [], st)


def test_bare_callable_with_sequential_finite_differences():
    Xc, v, order, starts, st = expect_host(50, 2, 1)
    runs = [scipy_run(s, closed_form=False) for s in starts]
    x, y = merged(Xc[order[0]], v[order[0]], [(r[0], r[1]) for r in runs])
    acq = make_acq([])
    got = go(CandidateSweep(num_random=50, grad_restarts=3, start_from_best=2), acq)
    check(got, [('call', (50, 2))] + [('call', (1, 2))] * sum(r[2] for r in runs), x, {'max_acq': y}, [], st)
    assert y > v[order[0]]       # (the gradient stage did improve on the batch: the merge was exercised)


@pytest.mark.parametrize('grad_restarts', [0, 2])
def test_maximise_alone(grad_restarts):
    """``maximise`` serves the sweep-only call and also grad_restarts > 0 with start_from_best = 0 (nothing ranked is needed)"""
    Xc, v, order, starts, st = expect_host(50, 0, grad_restarts)
    acq = make_acq(['maximise'], last_sweep_ms=1.25)
    calls, x, y = [('maximise', (50, 2))], Xc[order[:1]], float(v[order[0]])
    if grad_restarts:
        runs = [scipy_run(s, closed_form=False) for s in starts]
        calls += [('call', (1, 2))] * sum(r[2] for r in runs)
        x, y = merged(Xc[order[0]], y, [(r[0], r[1]) for r in runs])
    check(go(CandidateSweep(num_random=50, grad_restarts=grad_restarts), acq), calls, x, {'max_acq': y, 'sweep_ms': 1.25}, [], st)


@pytest.mark.parametrize('lockstep,grad_restarts,start_from_best,threaded', [
    (True, 3, 2, True), (False, 3, 2, False), ('scipy', 3, 2, True), (True, 1, 1, False)])
def test_topk_then_value_and_grad(lockstep, grad_restarts, start_from_best, threaded):
    """the k best from ``maximise_topk``; without ``lbfgsb`` the restarts meet at the rendezvous (lockstep True or 'scipy',
    more than one restart) or run one after the other"""
    Xc, v, order, starts, st = expect_host(50, start_from_best, grad_restarts - start_from_best)
    runs = [scipy_run(s, closed_form=True) for s in starts]
    x, y = merged(Xc[order[0]], v[order[0]], [(r[0], r[1]) for r in runs])
    rounds = lockstep_rounds([r[2] for r in runs]) if threaded else [1] * sum(r[2] for r in runs)
    acq = make_acq(['maximise', 'maximise_topk', 'value_and_grad'])
    sweep = CandidateSweep(num_random=50, grad_restarts=grad_restarts, start_from_best=start_from_best, lockstep=lockstep)
    check(go(sweep, acq), [('maximise_topk', (50, 2), start_from_best)] + [('value_and_grad', (m, 2)) for m in rounds],
          x, {'max_acq': y}, [], st)
    assert sweep.last_batches == (rounds if threaded else None)


def test_host_stream_sweep_only():
    Xc, v, order, _, st = expect_host(50, 0, 0)
    acq = make_acq(['maximise', 'maximise_topk', 'maximise_host_stream', 'value_and_grad', 'lbfgsb'])
    sweep = CandidateSweep(num_random=50)
    sweep.STREAM_DRAW_MIN = 1
    check(go(sweep, acq), [('maximise_host_stream', 50, LOW, HIGH, 0, 0, None), ('get_candidate', int(order[0]))],
          Xc[order[:1]], {'max_acq': float(v[order[0]])}, [], st)


def test_host_stream_topk_feeds_the_gradient_stage():
    """the ranked rows come from ``ctx.get_candidate``: the batch never was on the host"""
    Xc, v, order, starts, st = expect_host(50, 2, 1)
    xs = 0.5 * (starts + CENTRE)
    x, y = merged(Xc[order[0]], v[order[0]], [(xs[j], -float(f(xs[j])[0])) for j in range(3)])
    acq = make_acq(['maximise', 'maximise_topk', 'maximise_host_stream', 'value_and_grad', 'lbfgsb'])
    sweep = CandidateSweep(num_random=50, grad_restarts=3, start_from_best=2)
    sweep.STREAM_DRAW_MIN = 1
    calls = [('maximise_host_stream', 50, LOW, HIGH, 2, 0, None), ('get_candidate', int(order[0])),
             ('get_candidate', int(order[0])), ('get_candidate', int(order[1])), ('lbfgsb', (3, 2), PAIRS, 15000)]
    check(go(sweep, acq), calls, x, {'max_acq': y, 'gradient_evaluations': 23}, [], st)


def test_host_stream_below_its_threshold_is_not_asked():
    Xc, v, order, _, st = expect_host(50, 0, 0)
    acq = make_acq(['maximise', 'maximise_host_stream'])
    check(go(CandidateSweep(num_random=50), acq), [('maximise', (50, 2))], Xc[order[:1]], {'max_acq': float(v[order[0]])}, [], st)


def test_host_stream_refused_falls_through_to_topk():
    Xc, v, order, starts, st = expect_host(50, 2, 1)
    xs = 0.5 * (starts + CENTRE)
    x, y = merged(Xc[order[0]], v[order[0]], [(xs[j], -float(f(xs[j])[0])) for j in range(3)])
    acq = make_acq(['maximise', 'maximise_topk', 'maximise_host_stream', 'value_and_grad', 'lbfgsb'], stream_refuses=True)
    sweep = CandidateSweep(num_random=50, grad_restarts=3, start_from_best=2)
    sweep.STREAM_DRAW_MIN = 1
    calls = [('maximise_host_stream', 50, LOW, HIGH, 2, 0, None), ('maximise_topk', (50, 2), 2), ('lbfgsb', (3, 2), PAIRS, 15000)]
    check(go(sweep, acq), calls, x, {'max_acq': y, 'gradient_evaluations': 23}, [], st)


def test_more_than_64_starts_from_best_argsort_the_full_vector():
    """start_from_best = 65: neither the stream nor ``maximise_topk`` (k <= 64) -- the vector comes back and is argsorted"""
    Xc, v, order, starts, st = expect_host(80, 65, 0)
    xs = 0.5 * (starts + CENTRE)
    x, y = merged(Xc[order[0]], v[order[0]], [(xs[j], -float(f(xs[j])[0])) for j in range(65)])
    acq = make_acq(['maximise', 'maximise_topk', 'maximise_host_stream', 'value_and_grad', 'lbfgsb'])
    sweep = CandidateSweep(num_random=80, grad_restarts=65, start_from_best=65)
    sweep.STREAM_DRAW_MIN = 1
    check(go(sweep, acq), [('call', (80, 2)), ('lbfgsb', (65, 2), PAIRS, 15000)], x, {'max_acq': y, 'gradient_evaluations': 23}, [], st)


def test_device_rng_lhs_with_prefetch_advances_both_seeds():
    acq = make_acq(['maximise', 'maximise_generated'], last_sweep_ms=0.5)
    sweep = CandidateSweep(num_random=50, device_rng_seed=7, device_design='lhs', prefetch_next=True)
    np.random.seed(SEED)
    st = state()
    for call in range(2):
        X = generated_batch(50, 7 + call)
        i = int(np.argmax(f(X)))
        acq.calls = []
        check(go(sweep, acq), [('maximise_generated', 50, LOW, HIGH, 7 + call, 0, 50, 8 + call)], X[i:i + 1],
              {'max_acq': float(f(X)[i]), 'sweep_ms': 0.5}, [], st)


def test_device_rng_uniform_without_prefetch():
    acq = make_acq(['maximise_generated'])
    X = generated_batch(50, 7)
    i = int(np.argmax(f(X)))
    np.random.seed(SEED)
    st = state()
    check(go(CandidateSweep(num_random=50, device_rng_seed=7), acq), [('maximise_generated', 50, LOW, HIGH, 7, 0, None, None)],
          X[i:i + 1], {'max_acq': float(f(X)[i])}, [], st)


def test_device_rng_needs_maximise_generated():
    with pytest.raises(AssertionError, match='device_rng_seed needs a native acquisition'):
        CandidateSweep(num_random=50, device_rng_seed=7)(BOUNDS, make_acq(['maximise']))


def test_large_host_draw_of_a_foreign_generator_warns_once(monkeypatch):
    monkeypatch.setattr(CandidateSweep, '_warned_host_draw', False)

    class zeros_selector:
        def __call__(self, num_points, latent_bounds):
            return np.zeros((num_points, 2))

    acq = make_acq(['maximise', 'maximise_generated'])
    sweep = CandidateSweep(num_random=500001, gen_random=zeros_selector())
    np.random.seed(SEED)
    st = state()
    text = ('CandidateSweep draws 500001 x 2 candidates on the host with zeros_selector: at this size the draw and its upload cost '
            'more than the GPU sweep -- the default random_selector (same numbers as the reference, finished on the '
            'GPU) or device_rng_seed=<int> avoid that')
    check(go(sweep, acq), [('maximise', (500001, 2))], np.zeros((1, 2)), {'max_acq': float(f(np.zeros(2))[0])}, [text], st)
    acq.calls = []
    check(go(sweep, acq), [('maximise', (500001, 2))], np.zeros((1, 2)), {'max_acq': float(f(np.zeros(2))[0])}, [], st)


# ---------------------------------------------------------------------------------------------------- __call__: the gradient stage


def test_on_device_refine():
    Xc, v, order, starts, st = expect_host(50, 2, 1)
    xs = 0.5 * (starts + CENTRE)
    x, y = merged(Xc[order[0]], v[order[0]], [(xs[j], -float(f(xs[j])[0])) for j in range(3)])
    acq = make_acq(['maximise', 'maximise_topk', 'value_and_grad', 'refine', 'lbfgsb'])
    sweep = CandidateSweep(num_random=50, grad_restarts=3, start_from_best=2, on_device=True, max_iter=37)
    text = 'restart 1 of the on-device optimisation stopped at max_iter'
    check(go(sweep, acq), [('maximise_topk', (50, 2), 2), ('refine', (3, 2), PAIRS, 37)], x,
          {'max_acq': y, 'refine_iterations': 17, 'warnings': [text]}, [], st)


def test_lbfgsb_with_a_failed_restart():
    """status != 1 is SciPy's ``not result.success``: the warning, an empty slot, and the restart's value never taken"""
    Xc, v, order, starts, st = expect_host(50, 2, 1)
    xs = 0.5 * (starts + CENTRE)
    results = [(xs[j], -float(f(xs[j])[0])) for j in range(3)]
    results[1] = (None, None)
    x, y = merged(Xc[order[0]], v[order[0]], results)
    acq = make_acq(['maximise', 'maximise_topk', 'value_and_grad', 'lbfgsb'], failed_restarts=(1,))
    sweep = CandidateSweep(num_random=50, grad_restarts=3, start_from_best=2)
    check(go(sweep, acq), [('maximise_topk', (50, 2), 2), ('lbfgsb', (3, 2), PAIRS, 15000)], x,
          {'max_acq': y, 'gradient_evaluations': 23, 'warnings': ['restart 1/3 of gradient-based optimisation failed']}, [], st)
    assert y < 1.0


def test_f32_sweep_reports_the_f64_value():
    Xc, v, order, _, st = expect_host(50, 0, 0)
    acq = make_acq(['maximise', 'value_and_grad'], sweep_dtype='f32', sweep_error=1e-4)
    check(go(CandidateSweep(num_random=50), acq), [('maximise', (50, 2)), ('value_and_grad', (1, 2))], Xc[order[:1]],
          {'max_acq': float(v[order[0]]), 'max_acq_sweep': float(v[order[0]]) + 1e-4}, [], st)


def test_foreign_model_takes_finite_differences():
    """an instance whose ``.model`` has no ``_sweep``: its GPU-only methods are there and are not used"""
    Xc, v, order, starts, st = expect_host(50, 1, 1)
    runs = [scipy_run(s, closed_form=False) for s in starts]
    x, y = merged(Xc[order[0]], v[order[0]], [(r[0], r[1]) for r in runs])
    acq = make_acq(['maximise', 'maximise_topk', 'maximise_host_stream', 'value_and_grad', 'refine', 'lbfgsb'],
                   model=_ForeignModel(), sweep_dtype='f32')
    sweep = CandidateSweep(num_random=50, grad_restarts=2, start_from_best=1)
    sweep.STREAM_DRAW_MIN = 1
    check(go(sweep, acq), [('call', (50, 2))] + [('call', (1, 2))] * sum(r[2] for r in runs), x, {'max_acq': y}, [], st)


def test_marginalised_model_is_ranked_on_the_host_and_refined_at_the_rendezvous():
    Xc, v, order, starts, st = expect_host(50, 1, 1)
    runs = [scipy_run(s, closed_form=True) for s in starts]
    x, y = merged(Xc[order[0]], v[order[0]], [(r[0], r[1]) for r in runs])
    acq = make_acq(['maximise', 'maximise_topk', 'value_and_grad', 'lbfgsb'], model=_MarginalisedModel())
    sweep = CandidateSweep(num_random=50, grad_restarts=2, start_from_best=1)
    check(go(sweep, acq), [('call', (50, 2))] + [('value_and_grad', (m, 2)) for m in lockstep_rounds([r[2] for r in runs])],
          x, {'max_acq': y}, [], st)


def test_marginalised_model_refuses_on_device():
    acq = make_acq(['maximise', 'refine'], model=_MarginalisedModel())
    with pytest.raises(ValueError) as e:
        CandidateSweep(num_random=50, grad_restarts=2, on_device=True)(BOUNDS, acq)
    assert str(e.value) == ('on_device=True is not available for a marginalised model: the on-device gradient stage '
                            'refines ONE fitted model (the SciPy path serves the integrated acquisition)')
    assert acq.calls == []


# ---------------------------------------------------------------------------------------------------- select_batch


def test_select_batch_refusals():
    sweep = CandidateSweep(num_random=50)
    with pytest.raises(ValueError) as e:
        sweep.select_batch(BOUNDS, make_acq(['maximise_batch'], model=_MarginalisedModel()), 2)
    assert str(e.value) == ('select_batch is not available for a marginalised model: batch strategies over a mixture of '
                            'hyper-parameter samples are out of scope')
    plain = make_acq(['maximise_batch'], model=_NativeModel())
    with pytest.raises(ValueError) as e:
        sweep.select_batch(BOUNDS, plain, 2, strategy='thompson')
    assert str(e.value) == "strategy='thompson' needs a TS acquisition (got {!r})".format(type(plain))
    ts = make_acq(['maximise_batch'], model=_NativeModel(), is_thompson=True)
    with pytest.raises(ValueError) as e:
        sweep.select_batch(BOUNDS, ts, 2)
    assert str(e.value) == "a TS acquisition selects batches with strategy='thompson' only (got 'kriging_believer')"
    with pytest.raises(NotImplementedError) as e:
        CandidateSweep(num_random=50, grad_restarts=1).select_batch(BOUNDS, plain, 2)
    assert str(e.value) == 'select_batch: no gradient refinement of the selected points (grad_restarts > 0)'
    for acq, named in ((make_acq(['maximise_batch'], model=_ForeignModel()), _ForeignModel),
                       (make_acq([], model=_NativeModel()), _NativeModel)):
        with pytest.raises(NotImplementedError) as e:
            sweep.select_batch(BOUNDS, acq, 2)
        assert str(e.value) == ('select_batch needs a native acquisition over a model built by HipGPSurrogate '
                                '(got {!r})'.format(named))
    bare = make_acq(['maximise_batch'])
    with pytest.raises(NotImplementedError) as e:
        sweep.select_batch(BOUNDS, bare, 2)
    assert str(e.value) == ('select_batch needs a native acquisition over a model built by HipGPSurrogate '
                            '(got {!r})'.format(type(bare)))
    assert plain.calls == ts.calls == bare.calls == [] and sweep._calls == 0


def _select(acq, **kwargs):
    sweep = CandidateSweep(num_random=50)
    np.random.seed(SEED)
    x, info = sweep.select_batch(BOUNDS, acq, 2, **kwargs)
    after = state()
    np.random.seed(SEED)
    draw(50)
    assert after == state() and sweep._calls == 1       # one batch drawn, nothing else
    return x, info


def _same(info, expected):
    assert sorted(info) == sorted(expected)
    for k, v in expected.items():
        if isinstance(v, np.ndarray):
            np.testing.assert_array_equal(info[k], v)
        else:
            assert info[k] == v and type(info[k]) is type(v)


def test_select_batch_info_kriging_believer_and_constant_liar():
    fant = np.array([9.0, 8.0, 7.0, 6.0, 5.0])          # three pending points first, then the q = 2 chosen ones
    res = dict(idx=np.array([4, 9]), val=np.array([0.5, 0.25]), x=np.array([[0.1, 0.2], [0.3, 0.4]]), fantasies=fant,
               mu=None, sigma=None, n_clamped=0, sweep_ms=2.5, lie=None)
    pending = np.arange(6.0).reshape(3, 2) / 10
    for strategy in ('kriging_believer', 'constant_liar'):
        acq = make_acq(['maximise_batch'], model=_NativeModel(), batch_result=dict(res))
        x, info = _select(acq, strategy=strategy, lie='max', pending=pending.reshape(-1), n_sim=5, seed=3)
        assert acq.calls == [('maximise_batch', (50, 2), 2, strategy, 'max', (3, 2), 5, 3)]
        np.testing.assert_array_equal(x, res['x'])
        _same(info, {'max_acq': res['val'], 'candidate_indices': res['idx'], 'fantasies': fant[3:], 'pending_fantasies': fant[:3],
                     'strategy': strategy, 'sweep_ms': 2.5})


def test_select_batch_info_monte_carlo():
    fant = np.arange(12.0).reshape(4, 3)               # n_sim = 4 simulations of one pending and two chosen points
    res = dict(idx=np.array([4, 9]), val=np.array([0.5, 0.25]), x=np.array([[0.1, 0.2], [0.3, 0.4]]), fantasies=fant,
               n_sim=4, seed=77, sweep_ms=None)
    acq = make_acq(['maximise_batch'], model=_NativeModel(), batch_result=res)
    x, info = _select(acq, strategy='monte_carlo', pending=[[0.5, 0.5]], n_sim=4)
    assert acq.calls == [('maximise_batch', (50, 2), 2, 'monte_carlo', 'min', (1, 2), 4, None)]
    np.testing.assert_array_equal(x, res['x'])
    _same(info, {'max_acq': res['val'], 'candidate_indices': res['idx'], 'fantasies': fant[:, 1:], 'pending_fantasies': fant[:, :1],
                 'strategy': 'monte_carlo', 'n_sim': 4, 'seed': 77})


def test_select_batch_info_thompson():
    res = dict(idx=np.array([4, 9]), val=np.array([0.5, 0.25]), x=np.array([[0.1, 0.2], [0.3, 0.4]]), pending_ignored=0,
               seed=5, n_features=128, sweep_ms=1.5)
    acq = make_acq(['maximise_batch'], model=_NativeModel(), is_thompson=True, scale_factor=-1, batch_result=res)
    x, info = _select(acq, strategy='thompson')
    assert acq.calls == [('maximise_batch', (50, 2), 2, 'thompson', 'min', None, 16, None)]
    np.testing.assert_array_equal(x, res['x'])
    _same(info, {'max_acq': -res['val'], 'candidate_indices': res['idx'], 'sample_values': res['val'], 'strategy': 'thompson',
                 'seed': 5, 'n_features': 128, 'pending_ignored': 0, 'sweep_ms': 1.5})
