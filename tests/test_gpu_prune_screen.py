"""The matrix-core screen in front of the pruned sweep's bound pass (turbo_amd/csrc/prune_screen.hpp, sweep_pruned.hpp
sweep_pruned).

* Winner value, index and n_clamped byte-identical between TGP_PRUNE_SCREEN=1, TGP_PRUNE_SCREEN=0 and TGP_SWEEP_PRUNE=0
  over N x M x D x acquisition x sense x iso / ARD, with the schedule that ran read back: a case in which the pruned
  schedule or the screen did not run FAILS.  Two runs of the same call return the same bytes.
* The same where the screen must give way: a batch of ties, a Matern handle, an f64 handle, and each branch behind the
  screen forced in turn.
* Candidate by candidate (tests/prune_screen_driver.hip on the adversarial inputs of tests/prune_screen_reference.py):
  |mu_s - mu~| <= E everywhere; the largest ratio is printed (about 1 would mean the proof's constants are too tight)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _prune_screen_child as child             # noqa: E402
import prune_screen_reference as ref            # noqa: E402


def _child(which):
    e = {k: v for k, v in os.environ.items() if k not in child.SWITCHES}
    out = subprocess.run([sys.executable, os.path.join(HERE, "_prune_screen_child.py"), which], env=e, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0 and "prune-screen ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


@pytest.fixture(scope="module")
def grid():
    return {tuple(r["case"]): r for r in _child("grid")}


@pytest.fixture(scope="module")
def giveway():
    return {r["case"]: r for r in _child("giveway")}


@pytest.mark.parametrize("case", list(child.grid_cases()), ids=lambda c: "-".join(str(x) for x in c))
def test_screened_winner_is_the_unscreened_and_the_unpruned_winner(grid, case):
    r = grid[case]
    print(r)
    assert r["p_screen"]["state"] == 0 and r["p_screen"]["screen"] >= 0, r["p_screen"]      # pruned, and the screen ran
    assert r["p_noscreen"]["state"] == 0 and r["p_noscreen"]["screen"] == -1, r["p_noscreen"]
    assert r["p_unpruned"]["state"] == -1 and r["p_unpruned"]["screen"] == -1, r["p_unpruned"]
    assert r["screen"] == r["noscreen"] == r["unpruned"], r
    assert r["again"] == r["screen"] and r["p_again"] == r["p_screen"], r
    assert r["p_screen"]["screen"] >= r["p_screen"]["survivors"]      # the contracted set comes out of the screen's


def test_grid_is_complete_and_the_screen_prunes(grid):
    assert len(grid) == 288
    # (the two sets are cut against different bars -- each schedule picks its lb set from its own bounds -- so they are
    # not nested; but a screen that passed most of a batch the tight bound prunes would be no screen)
    assert sum(r["p_screen"]["screen"] for r in grid.values()) < 0.1 * sum(r["case"][1] for r in grid.values())


@pytest.mark.parametrize("name", ["ties", "matern", "f64", "direct", "gathered", "tight_all"])
def test_screen_gives_way(giveway, name):
    r = giveway[name]
    print(r)
    assert r["screen"] == r["noscreen"] == r["unpruned"] == r["again"], r
    assert r["p_again"] == r["p_screen"]
    assert r["p_unpruned"]["state"] == -1
    M = 4099
    if name == "ties":
        # every bound ties: the screen passes the whole batch (less the lb set), the tight pass over all M runs and passes
        # it too, and the full schedule takes over
        assert r["p_screen"]["state"] == 1 and r["p_screen"]["screen"] > 0.25 * M, r["p_screen"]
        assert r["p_screen"]["survivors"] > 0.25 * M
    elif name in ("matern", "f64"):
        assert r["p_screen"]["screen"] == -1 and r["p_screen"]["state"] in (0, 1), r["p_screen"]       # not applicable
        assert r["p_screen"] == r["p_noscreen"]
    elif name == "direct":
        assert r["p_screen"]["state"] == 0 and r["p_screen"]["screen"] > 0
        assert r["p_screen"]["survivors"] == r["p_screen"]["screen"]                                     # contracted as they are
    elif name == "gathered":
        assert r["p_screen"]["state"] == 0 and r["p_screen"]["screen"] > 0
        assert r["p_screen"]["survivors"] <= r["p_screen"]["screen"]                                     # filtered once more
    else:
        # (prune_frac leaves room for no survivor at all: any screen survivor sends the tight pass over all M, and any
        # survivor of that the full schedule)
        assert r["p_screen"]["screen"] > 0 and r["p_screen"]["survivors"] > 0, r["p_screen"]
        assert r["p_screen"]["state"] == r["p_noscreen"]["state"] == 1


@pytest.fixture(scope="module")
def driver_out(tmp_path_factory):
    d = tmp_path_factory.mktemp("prune_screen")
    exe = str(d / "prune_screen_driver")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", os.path.join(HERE, "prune_screen_driver.hip"),
                           "-o", exe], timeout=900)
    args, cases = [exe, "2"], {}
    for D in (1, 5, 32, 40):
        for cfg in ref.CONFIGS:
            Cs, Xs, alpha, constant = ref.adversarial_case(D, cfg)
            Dp = -(-D // 4) * 4
            pad = lambda A: np.ascontiguousarray(np.pad(A, ((0, 0), (0, Dp - D))), dtype=np.float32)
            fin, fout = str(d / ("in_%d_%s.bin" % (D, cfg))), str(d / ("out_%d_%s.bin" % (D, cfg)))
            with open(fin, "wb") as f:
                f.write(np.array([Xs.shape[0], Cs.shape[0], Dp, D], dtype=np.int32).tobytes())
                f.write(np.float64(constant).tobytes())
                f.write(pad(Xs).tobytes()); f.write(pad(Cs).tobytes()); f.write(np.ascontiguousarray(alpha, dtype=np.float64).tobytes())
            args += [fin, fout]
            cases[(D, cfg)] = (fout, (Cs, Xs, alpha, constant))
    res = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return {k: (np.fromfile(f, dtype=np.float64).reshape(3, -1), case) for k, (f, case) in cases.items()}


@pytest.mark.parametrize("cfg", ref.CONFIGS)
@pytest.mark.parametrize("D", (1, 5, 32, 40))
def test_screen_mean_within_its_error_of_the_exact_mean(driver_out, D, cfg):
    (mu_s, E, mu), (Cs, Xs, alpha, constant) = driver_out[(D, cfg)]
    assert mu_s.shape == (512,) and np.isfinite(mu_s).all() and np.isfinite(E).all() and np.isfinite(mu).all()
    ratio = np.abs(mu_s - mu) / E
    print("D=%d %s: largest |mu_s - mu~| / E = %.3g (E in [%.3g, %.3g])" % (D, cfg, ratio.max(), E.min(), E.max()))
    assert (np.abs(mu_s - mu) <= E).all(), float(ratio.max())
    # the device's E is the model's, and its exact mean is the model's exact path up to v_exp_f32's last bit
    np.testing.assert_allclose(E, ref.error_bound(Cs, Xs, alpha, constant, D), rtol=1e-6)
    assert (np.abs(mu - ref.exact_mean(Cs, Xs, alpha, constant)) <= E).all()
    if cfg != "underflow_c1":
        assert np.abs(mu).max() > 0.0
