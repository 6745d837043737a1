"""GPU: ``ta.EHVI`` through ``CandidateSweep`` on a ZDT1-like two-objective toy in 2-D, driven as the reference Optimiser
drives a plugin (fit, construct_function, the auxiliary optimiser, the evaluation, evaluation_finished) for a handful of
trials: the chosen point is a drawn candidate bit for bit, acq_info's front is the reference builder's, the hypervolume
over the trials never decreases, the gradient stage returns at least the sweep's best, and a pickled instance reloaded
without a visible device answers ``__call__`` within the pure-function bar."""
import faulthandler
import json
import os
import pickle
import subprocess
import sys
import warnings

import numpy as np
import pytest

import ehvi_reference as er

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ehvi_eref.json")) as _f:
    E_REF = float(json.load(_f)["e_ref"])
KERNEL = ("matern52", 1.0, 0.4, 1e-4)
M = 1000


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(120, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _factory(ta):
    return ta.HipGPSurrogate(model_params=dict(kernel=ta.GPKernel(*KERNEL), normalize_y=True, optimizer=None), training_iterations=1)


def zdt1(x):
    """ZDT1 in two dimensions: both minimised; the front is x_1 = 0, f_2 = 1 - sqrt(f_1)"""
    f1 = float(x[0])
    g = 1.0 + 9.0 * float(x[1])
    return f1, g * (1.0 - np.sqrt(f1 / g))


def test_a_handful_of_trials_on_a_two_objective_toy(tmp_path):
    import turbo_amd as ta
    rng = np.random.RandomState(3)
    X = [x for x in rng.uniform(0, 1, (6, 2))]
    ys = [zdt1(x) for x in X]
    sur = _factory(ta)
    acq = ta.EHVI(ta.Objective("f2", _factory(ta), "min"), ref=(1.1, 11.0))
    for t, (a, b) in enumerate(ys):
        acq.evaluation_started(t)
        acq.evaluation_finished(t, a, {"f2": b})
    bounds = ta.Bounds([("a", 0.0, 1.0), ("b", 0.0, 1.0)])
    sweep = ta.CandidateSweep(num_random=M, grad_restarts=0)
    refined = ta.CandidateSweep(num_random=M, grad_restarts=4, start_from_best=2)
    hvs, inst = [], None
    for t in range(6, 11):
        Xa, Y = np.vstack(X), np.array(ys)
        model, _ = sur.construct_model(t, Xa, Y[:, 0])
        inst, info = acq.construct_function(t, model, "min")
        F, raw, idx, hv = er.front(Y, (-1.0, -1.0), (1.1, 11.0))
        assert info["pareto_front"].tolist() == raw.tolist() and info["pareto_trials"] == idx.tolist()
        assert abs(info["hypervolume"] - hv) <= 64 * er.U * hv and info["ref"].tolist() == [1.1, 11.0]
        hvs.append(info["hypervolume"])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            np.random.seed(100 + t)
            x, minfo = sweep(bounds, inst)
            drawn = sur._context().read_candidates()
            np.random.seed(100 + t)
            xr, rinfo = refined(bounds, inst)
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        hit = np.nonzero((drawn == x).all(1))[0]
        vals = inst(drawn)
        print("trial %d: front of %d, hv %.6g; sweep -> %s (EHVI %.6g, candidate %s); gradient stage -> %s (EHVI %.6g)"
              % (t, len(F), hv, x, minfo["max_acq"], hit, np.asarray(xr).reshape(-1), rinfo["max_acq"]))
        assert drawn.shape == (M, 2) and len(hit) >= 1                       # a drawn candidate, bit for bit
        assert (int(hit[0]), minfo["max_acq"]) == er.argmax(vals)
        assert "gradient_evaluations" in rinfo and rinfo["max_acq"] >= minfo["max_acq"]
        xr = np.asarray(xr, dtype=np.float64).reshape(-1)
        assert np.all(xr >= 0.0) and np.all(xr <= 1.0)
        X.append(xr)
        ys.append(zdt1(xr))
        acq.evaluation_started(t)
        acq.evaluation_finished(t, ys[-1][0], {"f2": ys[-1][1]})
    hvs.append(er.front(np.array(ys), (-1.0, -1.0), (1.1, 11.0))[3])
    print("hypervolume over the trials: %s" % hvs)
    assert all(b >= a for a, b in zip(hvs, hvs[1:])) and hvs[-1] > hvs[0]

    # the last instance, pickled and reloaded by a process that sees no device: __call__ follows the formula in NumPy
    grid = np.random.RandomState(0).uniform(0, 1, (64, 2))
    on_gpu = inst(grid)
    ctx, g = inst._on_gpu()
    ctx.set_candidates(grid)
    r = ctx.sweep_ehvi(g, want_mu=True, want_sigma=True, want_second=True, want_value=True)
    assert r["value"].tobytes() == on_gpu.tobytes()
    pk, xc, out = tmp_path / "inst.pkl", tmp_path / "grid.npy", tmp_path / "out.npy"
    pk.write_bytes(pickle.dumps(inst))
    np.save(xc, grid)
    child = ("import sys, pickle, warnings, numpy as np\n"
             "sys.path.insert(0, %r)\n"
             "import turbo_amd as ta\n"
             "warnings.simplefilter('ignore')\n"
             "inst = pickle.loads(open(sys.argv[1], 'rb').read())\n"
             "vals = inst(np.load(sys.argv[2]))\n"
             "assert inst._on_gpu() is None and inst.model._factory._context().host\n"
             "np.save(sys.argv[3], vals)\n"
             "print('host-reload ok')\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    res = subprocess.run([sys.executable, "-c", child, str(pk), str(xc), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "host-reload ok" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
    host = np.load(out)
    # the bar at the GPU's posterior bits, plus what the host backend's posterior may differ by (tests/test_gpu_parity.py's
    # reload tolerances: mean 1e-9 relative + 1e-10, variance 1e-7 relative + 1e-9 (c + noise) y_std^2, as a deviation
    # var_tol / (2 sigma)) through the value's own partials
    F, _, _, _ = er.front(np.array(ys[:-1]), (-1.0, -1.0), (1.1, 11.0))
    a, c = er.strips(F, (-1.1, -11.0))
    p = er.partials(a, c, -r["mu"], r["sigma"], -r["mu2"], r["sigma2"])
    tol = 2 * er.bound(p["scale"], E_REF)
    for j, (mu, sg, m) in enumerate(((r["mu"], r["sigma"], inst.model), (r["mu2"], r["sigma2"], inst.second_model))):
        var_tol = 1e-7 * sg * sg + 1e-9 * (KERNEL[1] + KERNEL[3]) * float(m.y_std) ** 2
        tol = tol + np.abs(p["cm%d" % (j + 1)]) * (1e-9 * np.abs(mu) + 1e-10) + np.abs(p["cs%d" % (j + 1)]) * var_tol / (2 * sg)
    err = np.abs(host - on_gpu)
    print("host reload: max |host - gpu| %.3g, max err / tol %.3g" % (err.max(), float((err / np.maximum(tol, er.TINY)).max())))
    assert np.all(err <= tol)
