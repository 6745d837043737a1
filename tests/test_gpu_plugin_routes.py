"""The plugin layer's routes on real models (tests/plugin_route_cases.py): the ordered list of C-ABI entries behind one
``construct_model`` + ``construct_function`` + ``CandidateSweep.__call__`` / ``select_batch`` is the one recorded in
tests/golden/plugin_route_calls.json (``tools/plugin_routes_digest.py --record-calls``, from the package as it stood before
the plugin layer was cut into named steps), and three equalities the classes promise hold bit for bit."""
import json
import os

import numpy as np
import pytest

import plugin_route_cases as prc

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'plugin_route_calls.json')) as _f:
    GOLDEN = json.load(_f)


def test_the_golden_lists_are_this_modules_cases():
    assert sorted(GOLDEN) == sorted(prc.case_ids())


@pytest.mark.parametrize('case_id', prc.case_ids())
def test_entries_called_in_order(case_id):
    import turbo_amd as ta
    out = prc.run_case(ta, case_id)
    assert out['entries'] == GOLDEN[case_id]
    for x in out['x']:
        assert x.ndim == 2 and x.shape[1] == prc.D and np.all((x >= 0.0) & (x <= 1.0))


def _plain(info):
    return {k: (np.asarray(v).tolist() if isinstance(v, np.ndarray) else v) for k, v in info.items() if k != 'sweep_ms'}


@pytest.mark.parametrize('case_id', ['ei-f64-n40-device_uniform_prefetch', 'ei-f64-n300-device_lhs_prefetch',
                                     'ei-f32-n300-device_lhs_prefetch', 'mes-f64-n200-device_lhs_prefetch'])
def test_prefetch_chooses_what_no_prefetch_chooses(case_id):
    import turbo_amd as ta
    a, b = prc.run_case(ta, case_id, prefetch=True), prc.run_case(ta, case_id, prefetch=False)
    assert len(a['x']) == len(b['x']) == 2
    for t in range(2):
        np.testing.assert_array_equal(a['x'][t], b['x'][t])
        assert _plain(a['info'][t]) == _plain(b['info'][t])
    assert a['state'] == b['state']
    if not case_id.startswith('mes'):      # (a MES instance's first use draws its batch itself: nothing to skip)
        assert a['entries'].count('tgp_gen_candidates') + a['entries'].count('tgp_gen_candidates_lhs') == 3   # the second trial found its batch
        assert a['entries'].count('tgp_set_overlap') == b['entries'].count('tgp_set_overlap') == 2


@pytest.mark.parametrize('case_id', ['ei-f64-n40-stream', 'ei-f64-n200-stream_topk', 'ei-f64-n300-stream_topk',
                                     'ei-f32-n300-stream', 'mes-f64-n200-stream_topk'])
def test_stream_route_is_the_host_loop(case_id):
    """the MT19937 stream continued in the library: the host loop's point, value and ``np.random`` afterwards"""
    import turbo_amd as ta
    a, b = prc.run_case(ta, case_id, stream_route=True), prc.run_case(ta, case_id, stream_route=False)
    assert 'tgp_set_candidates_mt19937' in a['entries'] and 'tgp_set_candidates_mt19937' not in b['entries']
    np.testing.assert_array_equal(a['x'][0], b['x'][0])
    assert _plain(a['info'][0]) == _plain(b['info'][0])
    assert a['state'] == b['state']


@pytest.mark.parametrize('design', ['uniform', 'lhs'])
def test_select_batch_sweeps_the_batch_call_would_have_drawn(design):
    import turbo_amd as ta
    n = 300
    X, y = prc.data(n)
    sur = ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel('matern52', 1.0, 0.6, 1e-3), normalize_y=True, optimizer=None),
                            training_iterations=1)
    try:
        bounds = ta.Bounds([('p%d' % d, 0.0, 1.0) for d in range(prc.D)])
        model, _ = sur.construct_model(0, X[:n], y[:n])
        acq, _ = ta.EI(0.01).construct_function(0, model, 'min', float(y[:n].min()))
        x1, _ = ta.CandidateSweep(num_random=prc.NUM_RANDOM, device_rng_seed=5, device_design=design)(bounds, acq)
        drawn = sur._context().read_candidates().copy()
        sur._context().set_candidates(np.zeros((4, prc.D)))          # the batch is gone: select_batch has to draw it
        xq, infoq = ta.CandidateSweep(num_random=prc.NUM_RANDOM, device_rng_seed=5, device_design=design).select_batch(bounds, acq, 2)
        np.testing.assert_array_equal(sur._context().read_candidates(), drawn)
        np.testing.assert_array_equal(xq[0], x1[0])                 # the first pick of the greedy batch is the arg-max
        np.testing.assert_array_equal(drawn[infoq['candidate_indices'][0]], x1[0])
    finally:
        sur.close()
