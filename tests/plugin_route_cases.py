"""The plugin layer's routes on real models: one case = one factory, one or two trials of ``construct_model`` +
``construct_function`` + ``CandidateSweep.__call__`` / ``select_batch``, with the name of every ``tgp_*`` entry the plugin
classes call noted in order.  Shared by tests/test_gpu_plugin_routes.py (the entry lists against
tests/golden/plugin_route_calls.json) and tools/plugin_routes_digest.py (a digest of what each case returns).

Sizes: N = 40 (the one-workgroup kernels), 200 (the one-launch sweep), 300 (the blocked fit, the general sweep); D = 3,
512 candidates, fixed hyper-parameters."""
import hashlib
import struct

import numpy as np

D, NUM_RANDOM, SEED = 3, 512, 23

# keyword arguments of CandidateSweep per route; '_stream': the MT19937 stream route is open at this batch size;
# '_trials': consecutive trials on one factory (the second model holds one observation more)
ROUTES = {
    'sweep': dict(),
    'maximise_lbfgsb': dict(grad_restarts=2, start_from_best=0),
    'topk_lbfgsb': dict(grad_restarts=3, start_from_best=2),
    'topk_threads': dict(grad_restarts=3, start_from_best=2, lockstep='scipy'),
    'topk_sequential': dict(grad_restarts=2, start_from_best=1, lockstep=False),
    'stream': dict(_stream=True),
    'stream_topk': dict(grad_restarts=3, start_from_best=2, _stream=True),
    'stream_topk_threads': dict(grad_restarts=3, start_from_best=2, lockstep='scipy', _stream=True),
    'argsort65': dict(grad_restarts=65, start_from_best=65, _stream=True),
    'device_uniform': dict(device_rng_seed=5),
    'device_lhs': dict(device_rng_seed=5, device_design='lhs', _trials=2),
    'device_lhs_prefetch': dict(device_rng_seed=5, device_design='lhs', prefetch_next=True, _trials=2),
    'device_uniform_prefetch': dict(device_rng_seed=5, prefetch_next=True, _trials=2),
    'refine': dict(grad_restarts=3, start_from_best=2, on_device=True, max_iter=50),
}
# select_batch: (CandidateSweep arguments, select_batch arguments, pending points)
BATCHES = {
    'batch_kb': (dict(), dict(q=3, strategy='kriging_believer'), 0),
    'batch_cl': (dict(), dict(q=3, strategy='constant_liar', lie='mean'), 2),
    'batch_mc': (dict(), dict(q=3, strategy='monte_carlo', n_sim=4, seed=3), 2),
    'batch_mc_unseeded': (dict(), dict(q=2, strategy='monte_carlo', n_sim=4), 0),
    'batch_kb_device': (dict(device_rng_seed=5), dict(q=3, strategy='kriging_believer'), 1),
    'batch_kb_device_lhs': (dict(device_rng_seed=5, device_design='lhs'), dict(q=2, strategy='kriging_believer'), 0),
    'batch_thompson': (dict(), dict(q=3, strategy='thompson'), 1),
    'batch_thompson_device': (dict(device_rng_seed=5), dict(q=3, strategy='thompson'), 0),
}
EVERY_ROUTE = [r for r in ROUTES] + ['batch_kb', 'batch_cl', 'batch_mc', 'batch_mc_unseeded', 'batch_kb_device',
                                     'batch_kb_device_lhs']


def case_ids():
    ids = ['ei-f64-n%d-%s' % (n, r) for n in (40, 200, 300) for r in EVERY_ROUTE]
    ids += ['ucb-f64-n200-%s' % r for r in ('sweep', 'topk_lbfgsb', 'stream_topk', 'device_uniform', 'refine', 'batch_kb')]
    ids += ['pi-f64-n40-%s' % r for r in ('sweep', 'topk_lbfgsb')]
    ids += ['ts-f64-n200-%s' % r for r in ('sweep', 'topk_threads', 'topk_sequential', 'stream', 'stream_topk_threads',
                                           'device_uniform', 'device_lhs', 'batch_thompson', 'batch_thompson_device')]
    ids += ['mes-f64-n200-%s' % r for r in ('sweep', 'maximise_lbfgsb', 'topk_lbfgsb', 'topk_threads', 'stream', 'stream_topk',
                                            'device_uniform', 'device_lhs_prefetch')]
    ids += ['mei-f64-n40-%s' % r for r in ('sweep', 'topk_lbfgsb', 'topk_sequential', 'device_uniform', 'device_lhs')]
    ids += ['ei-f32-n300-%s' % r for r in ('sweep', 'topk_lbfgsb', 'stream', 'device_uniform', 'device_lhs_prefetch')]
    return ids


class RecordingLib:
    """stands in front of the loaded library: every ``tgp_*`` entry called through it is noted by name"""

    def __init__(self, lib, log):
        self.__dict__['_lib'], self.__dict__['_log'] = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith('tgp_'):
            return fn
        log = self._log

        def entry(*args):
            log.append(name)
            return fn(*args)
        return entry


def data(n):
    rng = np.random.RandomState(1000 + n)
    X = rng.uniform(0, 1, (n + 1, D))
    y = np.sin(3 * X.sum(1)) + 0.3 * ((X - 0.4) ** 2).sum(1) + 0.02 * rng.normal(size=n + 1)
    return X, y


def _factory(ta, acq_name):
    return {'ei': lambda: ta.EI(0.01), 'mei': lambda: ta.EI(0.01), 'pi': lambda: ta.PI(0.01), 'ucb': lambda: ta.UCB(2.0),
            'ts': lambda: ta.TS(seed=9, n_features=64), 'mes': lambda: ta.MES(n_samples=4, seed=9, n_features=64)}[acq_name]()


def run_case(ta, case_id, stream_route=None, prefetch=None, keep=None):
    """Runs one case.  Returns dict(entries, x [per trial], info [per trial], state).  ``stream_route`` / ``prefetch``
    override the route's own setting (the equalities of tests/test_gpu_plugin_routes.py); ``keep(ctx)`` is called before
    the factory is closed and its result returned as 'kept'."""
    acq_name, dtype, n, route = case_id.split('-', 3)
    n = int(n[1:])
    X, y = data(n)
    kernel = ta.GPKernel('matern52', 1.0, 0.6, 1e-3)
    params = dict(kernel=kernel, normalize_y=True, optimizer=None)
    if acq_name == 'mei':
        sur = ta.MarginalisedHipGPSurrogate(model_params=dict(params, kernel=ta.GPKernel(
            'matern52', 1.0, 0.6, 1e-3, bounds=dict(constant=(1e-2, 1e2), length_scale=(5e-2, 1e1), noise=(1e-5, 1e-1)))),
            training_iterations=1, dtype=dtype, n_hyper_samples=3, burn=2, thin=1, hyper_seed=17)
    else:
        sur = ta.HipGPSurrogate(model_params=params, training_iterations=1, dtype=dtype)
    bounds = ta.Bounds([('p%d' % d, 0.0, 1.0) for d in range(D)])
    log = []
    ctx = sur._context()
    loaded = ta._lib._lib
    proxy = RecordingLib(loaded, log)
    ctx.lib = proxy
    ta._lib._lib = proxy          # (handles made during the case -- a mixture's gradient contexts -- are noted too)
    xs, infos = [], []
    try:
        if route in ROUTES:
            kwargs, select, n_pending = dict(ROUTES[route]), None, 0
        else:
            kwargs, select, n_pending = dict(BATCHES[route][0]), BATCHES[route][1], BATCHES[route][2]
        stream = kwargs.pop('_stream', False)
        if stream_route is not None:
            stream = stream_route
        trials = kwargs.pop('_trials', 1)
        if prefetch is not None:
            kwargs['prefetch_next'] = prefetch
        sweep = ta.CandidateSweep(num_random=NUM_RANDOM, **kwargs)
        if stream:
            sweep.STREAM_DRAW_MIN = 1
        np.random.seed(SEED)
        for t in range(trials):
            model, _ = sur.construct_model(t, X[:n + t], y[:n + t])
            factory = _factory(ta, acq_name)
            args = (t, model, 'min') + ((float(y[:n + t].min()),) if factory.get_type() == 'improvement' else ())
            acq, _ = factory.construct_function(*args)
            if select is None:
                x, info = sweep(bounds, acq)
            else:
                pending = np.random.RandomState(7).uniform(0, 1, (n_pending, D)) if n_pending else None
                x, info = sweep.select_batch(bounds, acq, pending=pending, **select)
            xs.append(np.array(x))
            infos.append(info)
        st = np.random.get_state()
        out = dict(entries=list(log), x=xs, info=infos, state=(st[1].tobytes(), int(st[2])))
        if keep is not None:
            out['kept'] = keep(ctx)
        return out
    finally:
        ta._lib._lib = loaded
        ctx.lib = loaded
        sur.close()


def _feed(h, v):
    if isinstance(v, dict):
        for k in sorted(v):
            if k == 'sweep_ms':       # a device time: the one figure of an info that is a measurement
                continue
            h.update(k.encode())
            _feed(h, v[k])
    elif isinstance(v, (list, tuple)):
        for e in v:
            _feed(h, e)
    elif isinstance(v, np.ndarray):
        h.update(str(v.dtype).encode() + str(v.shape).encode() + np.ascontiguousarray(v).tobytes())
    elif isinstance(v, (bool, int, np.integer)):
        h.update(b'i' + str(int(v)).encode())
    elif isinstance(v, (float, np.floating)):
        h.update(b'f' + struct.pack('<d', float(v)))
    else:
        h.update(b's' + str(v).encode())


def digest_line(case_id, out):
    hx, hi, hs = hashlib.sha256(), hashlib.sha256(), hashlib.sha256()
    _feed(hx, out['x'])
    _feed(hi, out['info'])
    hs.update(out['state'][0] + str(out['state'][1]).encode())
    first = out['info'][0]['max_acq']
    return '%-34s x=%s info=%s rng=%s entries=%d max_acq=%s' % (
        case_id, hx.hexdigest()[:16], hi.hexdigest()[:16], hs.hexdigest()[:16], len(out['entries']),
        np.array2string(np.atleast_1d(np.asarray(first, dtype=np.float64))[:2], precision=17))
