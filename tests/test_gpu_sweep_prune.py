"""The pruned arg-max-only sweep (csrc/sweep_pruned.hpp, sweep_pruned) against the full sweep on the same
handle: the winner's value and index bit for bit, and the same clamp count, with and without TGP_SWEEP_PRUNE; the
schedule that actually ran is read back (NativeGP.last_prune), so a case cannot pass by never pruning."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACQ = {"ucb": 1, "pi": 2, "ei": 3}


@pytest.fixture(autouse=True)
def _prune_small_problems(monkeypatch):
    """the cases here are far below the size the default TGP_PRUNE_MIN_WORK prunes at: open it"""
    monkeypatch.setenv("TGP_PRUNE_MIN_WORK", "0")


def _problem(seed, N, D, M, ard):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, size=(N, D))
    w = rng.normal(size=D) / np.sqrt(D)
    y = np.sin(3 * X @ w) + 0.5 * ((X - 0.5) ** 2).sum(1) + 0.01 * rng.normal(size=N)
    iso = float(np.sqrt(D / 6.0))
    ls = iso * (0.5 + np.arange(D) / max(D - 1.0, 1.0)) if ard else iso
    Xc = rng.uniform(0, 1, size=(M, D))
    return X, y, ls, Xc


def _gp(dtype, X, y, kind, ls, noise, Xc):
    import turbo_amd as ta
    gp = ta.NativeGP(0, dtype)
    gp.fit(X, y, kind, 1.0, ls, noise, 1e-10, True)
    gp.set_candidates(Xc)
    return gp


def _same(a, b):
    assert a["best_idx"] == b["best_idx"], (a["best_idx"], b["best_idx"])
    assert np.float64(a["best_val"]).tobytes() == np.float64(b["best_val"]).tobytes(), (a["best_val"], b["best_val"])
    assert a["n_clamped"] == b["n_clamped"]


def _args(acq, sf, y, param):
    return ACQ[acq], float(sf), float(y.min() if sf < 0 else y.max()), float(param)


# kind, ard, dtype, N, D, M, acq, sf, param, noise
CASES = [
    ("rbf", False, "f32", 300, 4, 5000, "ei", -1, 0.01, 1e-2),
    ("rbf", True, "f64", 257, 5, 4999, "ucb", 1, 2.0, 1e-4),
    ("matern12", False, "f32", 2048, 8, 9001, "pi", -1, 0.01, 1e-2),
    ("matern12", True, "f64", 600, 6, 7000, "ei", 1, 0.0, 1e-3),
    ("matern32", True, "f64", 2048, 8, 9001, "ei", -1, 0.01, 1e-4),
    ("matern32", False, "f32", 1024, 8, 8191, "ucb", 1, 2.0, 1e-2),
    ("matern52", False, "f32", 4096, 16, 12345, "ucb", -1, -1.0, 1e-2),
    ("matern52", True, "f64", 300, 3, 6000, "pi", 1, 0.01, 1e-3),
    ("rbf", False, "f32", 4096, 32, 20000, "ei", -1, 0.01, 1e-2),
    ("rbf", True, "f64", 4096, 12, 10007, "pi", -1, 0.01, 1e-4),
]


@pytest.mark.parametrize("kind,ard,dtype,N,D,M,acq,sf,param,noise", CASES)
def test_pruned_sweep_is_the_full_sweep_bit_for_bit(kind, ard, dtype, N, D, M, acq, sf, param, noise, monkeypatch):
    X, y, ls, Xc = _problem(N + D + M, N, D, M, ard)
    gp = _gp(dtype, X, y, kind, ls, noise, Xc)
    a = _args(acq, sf, y, param)
    full = gp.sweep(*a, want_acq=True)
    assert gp.last_prune()["state"] == -1
    assert full["best_idx"] == int(np.argmax(np.where(np.isnan(full["acq"]), -np.inf, full["acq"])))
    pr = gp.sweep(*a)
    st = gp.last_prune()
    print("prune", kind, dtype, N, M, acq, st)
    assert st["state"] in (0, 1) and 0 < st["lb_set"] <= 256, st
    assert (st["state"] == 0) == (st["survivors"] <= M // 4), st
    _same(pr, full)
    monkeypatch.setenv("TGP_SWEEP_PRUNE", "0")
    off = gp.sweep(*a)
    assert gp.last_prune()["state"] == -1
    _same(off, full)


def test_ties_go_to_the_lowest_index():
    """copies of the winner's row before and after it: the lowest copy wins, pruned or not"""
    X, y, ls, Xc = _problem(5, 1500, 6, 9000, False)
    gp = _gp("f32", X, y, "matern52", ls, 1e-2, Xc)
    a = _args("ei", -1, y, 0.01)
    w = gp.sweep(*a, want_acq=True)["best_idx"]
    for j in (w // 3, w // 2 + 1, 8998):
        Xc[j] = Xc[w]
    gp.set_candidates(Xc)
    full = gp.sweep(*a, want_acq=True)
    assert full["best_idx"] == w // 3
    pr = gp.sweep(*a)
    assert gp.last_prune()["state"] in (0, 1)
    _same(pr, full)


def test_fallback_when_too_many_survive(monkeypatch):
    X, y, ls, Xc = _problem(7, 700, 5, 6000, True)
    gp = _gp("f64", X, y, "rbf", ls, 1e-3, Xc)
    a = _args("ucb", 1, y, 2.0)
    full = gp.sweep(*a, want_acq=True)
    monkeypatch.setenv("TGP_PRUNE_FRAC", "-1")
    pr = gp.sweep(*a)
    assert gp.last_prune()["state"] == 1
    _same(pr, full)
    monkeypatch.setenv("TGP_PRUNE_FRAC", "1")
    pr = gp.sweep(*a)
    assert gp.last_prune()["state"] == 0
    _same(pr, full)


def test_clamp_case_is_gated_off():
    """f32 with noise 1e-4: s^2 / (c + s^2) is below the gate, so every candidate is contracted -- candidates that are
    training points clamp, and the count is the full sweep's"""
    X, y, ls, Xc = _problem(9, 1200, 4, 5000, False)
    Xc[:300] = X[:300]
    gp = _gp("f32", X, y, "rbf", ls, 1e-4, Xc)
    a = _args("ei", -1, y, 0.01)
    full = gp.sweep(*a, want_acq=True)
    pr = gp.sweep(*a)
    assert gp.last_prune()["state"] == -2
    _same(pr, full)


def test_candidates_at_training_points_with_the_gate_open():
    """f64, noise 1e-6 (gate open): candidates that are training points, pruned against the full sweep"""
    X, y, ls, Xc = _problem(11, 900, 3, 5000, True)
    Xc[:200] = X[:200]
    gp = _gp("f64", X, y, "matern52", ls, 1e-6, Xc)
    for acq, sf, param in (("ei", -1, 0.01), ("pi", 1, 0.0), ("ucb", -1, 2.0)):
        a = _args(acq, sf, y, param)
        full = gp.sweep(*a, want_acq=True)
        pr = gp.sweep(*a)
        assert gp.last_prune()["state"] in (0, 1)
        _same(pr, full)


@pytest.mark.parametrize("dtype", ["f32", "f64"])
def test_overlap_front_then_pruned_sweep(dtype):
    """tgp_set_overlap(2): the pruned sweep behind a fit's front (it uses the front's candidate scaling) against the full
    sweep behind the same front"""
    X, y, ls, Xc = _problem(13, 2048, 8, 20000, False)
    noise = 1e-2 if dtype == "f32" else 1e-4
    gp = _gp(dtype, X, y, "rbf", ls, noise, Xc)
    gp.set_overlap(2)
    a = _args("ei", -1, y, 0.01)
    res = []
    for want in (False, True, False):
        gp.fit(X, y, "rbf", 1.0, ls, noise, 1e-10, True)
        res.append(gp.sweep(*a, want_acq=want))
        if not want:
            assert gp.last_prune()["state"] in (0, 1)
    gp.set_overlap(0)
    _same(res[0], res[1])
    _same(res[2], res[1])


def test_small_problems_are_not_pruned_by_default(monkeypatch):
    """below TGP_PRUNE_MIN_WORK (M N^2) the full schedule runs: the pruned one's fixed cost would be more than it saves"""
    monkeypatch.delenv("TGP_PRUNE_MIN_WORK")
    X, y, ls, Xc = _problem(17, 512, 8, 6000, False)
    gp = _gp("f64", X, y, "rbf", ls, 1e-4, Xc)
    a = _args("ucb", -1, y, 2.0)
    full = gp.sweep(*a, want_acq=True)
    pr = gp.sweep(*a)
    assert gp.last_prune()["state"] == -1
    _same(pr, full)
