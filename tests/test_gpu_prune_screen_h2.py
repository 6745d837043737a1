"""The fp16 screen in front of the pruned sweep's bound pass (turbo_amd/csrc/prune_screen_h2.hpp, sweep_pruned.hpp
sweep_pruned).

* Candidate by candidate (tests/prune_screen_h2_driver.hip on the adversarial inputs of tests/prune_screen_reference.py and
  the extra cases of tests/prune_screen_h2_reference.py: N = 1 / 127 / 128 / 129, one-signed alpha, a positive count of
  exactly 128, inputs outside the range conditions): |mu_s - mu~| <= E everywhere, the largest ratio printed; the device's E
  and closed form are the model's to 1e-6 (the model fed the device's W); W = mu+ + mu- against the model's sum k |alpha|;
  two runs give the same bytes.
* Winner value, index and n_clamped byte-identical between TGP_SCREEN_ARITH=h2, f32, TGP_PRUNE_SCREEN=0 and
  TGP_SWEEP_PRUNE=0 over N x D x acquisition x sense x iso / ARD and on a batch of ties, with the schedule that ran read
  back: a case in which the screen, or the arithmetic asked for, did not run FAILS."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _prune_screen_h2_child as child          # noqa: E402
import prune_screen_reference as ref            # noqa: E402
import prune_screen_h2_reference as h2          # noqa: E402


def driver_cases():
    cases = {}
    for D in (1, 5, 32, 40):
        for cfg in ref.CONFIGS:
            cases["adv-%d-%s" % (D, cfg)] = ref.adversarial_case(D, cfg) + (D,)
    cases.update(h2.extra_cases())
    return cases


@pytest.fixture(scope="module")
def driver_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("prune_screen_h2")
    exe = str(d / "prune_screen_h2_driver")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", os.path.join(HERE, "prune_screen_h2_driver.hip"),
                           "-o", exe], timeout=900)
    args, outs = [exe, "2"], {}
    for name, (Cs, Xs, alpha, constant, D) in driver_cases().items():
        Dp = -(-D // 4) * 4
        pad = lambda A: np.ascontiguousarray(np.pad(A, ((0, 0), (0, Dp - D))), dtype=np.float32)
        fin, fout = str(d / ("in_%s.bin" % name)), str(d / ("out_%s.bin" % name))
        with open(fin, "wb") as f:
            f.write(np.array([Xs.shape[0], Cs.shape[0], Dp, D], dtype=np.int32).tobytes())
            f.write(np.float64(constant).tobytes())
            f.write(pad(Xs).tobytes()); f.write(pad(Cs).tobytes()); f.write(np.ascontiguousarray(alpha, dtype=np.float64).tobytes())
        args += [fin, fout]
        outs[name] = fout
    res = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return {k: np.fromfile(f, dtype=np.float64).reshape(9, -1) for k, f in outs.items()}


@pytest.mark.parametrize("name", sorted(driver_cases()))
def test_screen_mean_within_its_error_of_the_exact_mean(driver_out, name):
    Cs, Xs, alpha, constant, D = driver_cases()[name]
    out = driver_out[name]
    mu_s, W, E, closed, mu = out[0], out[1], out[2], out[3], out[8]
    assert out[:4].tobytes() == out[4:8].tobytes()                      # the second run's bytes
    Em, closedm = h2.error_bound(Cs, Xs, alpha, constant, D, W)         # the model's formulas on the device's W
    fin = np.isfinite(Em)
    assert (np.isfinite(E) == fin).all() and (np.isinf(E[~fin]) & (E[~fin] > 0)).all()
    if name == "x_out_of_range":
        assert not fin.any()
        return
    assert fin.all() or name == "c_out_of_range"
    assert np.isfinite(mu_s[fin]).all() and np.isfinite(W[fin]).all() and np.isfinite(mu[fin]).all()
    ratio = np.abs(mu_s[fin] - mu[fin]) / E[fin]
    print("%s: largest |mu_s - mu~| / E = %.3g (E in [%.3g, %.3g], E / closed median %.3g)"
          % (name, ratio.max(), E[fin].min(), E[fin].max(), np.median(E[fin] / closed[fin])))
    assert (np.abs(mu_s[fin] - mu[fin]) <= E[fin]).all(), float(ratio.max())
    np.testing.assert_allclose(E[fin], Em[fin], rtol=1e-6)
    np.testing.assert_allclose(closed[fin], closedm[fin], rtol=1e-6)
    # W against the model's: the two differ in the matrix core's summation order and v_exp_f32's last bit only, and E --
    # which sees alpha through |alpha| alone -- bounds the distance of either from the exact path's sum k~ |alpha|
    ms_m, W_m = h2.screen_mean(Cs, Xs, alpha, constant)
    assert (np.abs(W[fin] - W_m[fin]) <= 2.0 * E[fin]).all(), float((np.abs(W - W_m)[fin] / E[fin]).max())
    assert (np.abs(mu_s[fin] - ms_m[fin]) <= 2.0 * E[fin]).all()
    assert (np.abs(mu_s[fin]) <= W[fin] * (1 + 1e-12)).all()
    assert (np.abs(mu[fin] - ref.exact_mean(Cs, Xs, alpha, constant)[fin]) <= E[fin]).all()
    if "underflow" not in name:
        assert np.abs(mu[fin]).max() > 0.0 and W[fin].max() > 0.0


def _child(which):
    e = {k: v for k, v in os.environ.items() if k not in child.SWITCHES}
    out = subprocess.run([sys.executable, os.path.join(HERE, "_prune_screen_h2_child.py"), which], env=e, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0 and "prune-screen-h2 ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


@pytest.fixture(scope="module")
def grid():
    return {tuple(r["case"]): r for r in _child("grid")}


def same_winner_and_schedule(r, D):
    assert r["h2"] == r["f32"] == r["noscreen"] == r["unpruned"] == r["again"], r
    assert r["p_again"] == r["p_h2"], r
    # the schedule that ran: the screen under both arithmetics (the fp16 one from SCRH_MIN_D on), none where it is off
    assert r["p_h2"]["screen"] >= 0 and r["p_h2"]["screen_arith"] == (2 if D >= h2.MIN_D else 1), r["p_h2"]
    assert r["p_f32"]["screen"] >= 0 and r["p_f32"]["screen_arith"] == 1, r["p_f32"]
    assert r["p_noscreen"]["screen"] == -1 and r["p_noscreen"]["screen_arith"] == 0, r["p_noscreen"]
    assert r["p_unpruned"]["state"] == -1 and r["p_unpruned"]["screen_arith"] == 0, r["p_unpruned"]


@pytest.mark.parametrize("case", list(child.grid_cases()), ids=lambda c: "-".join(str(x) for x in c))
def test_winner_is_the_same_under_every_screen(grid, case):
    r = grid[case]
    print(r)
    same_winner_and_schedule(r, case[2])
    assert r["p_h2"]["state"] == 0 and r["p_f32"]["state"] == 0, r      # pruned under both
    assert r["p_h2"]["screen"] >= r["p_h2"]["survivors"]


def test_grid_is_complete(grid):
    assert len(grid) == 96


def test_ties():
    (r,) = _child("ties")
    print(r)
    same_winner_and_schedule(r, 32)
    # every bound ties: the screen passes the batch, the tight pass over all M too, and the full schedule takes over
    assert r["p_h2"]["state"] == 1 and r["p_h2"]["screen"] > 0.25 * child.M, r["p_h2"]
