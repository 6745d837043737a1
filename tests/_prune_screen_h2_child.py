"""Child process of tests/test_gpu_prune_screen_h2.py (the pruned sweep's switches are read per call; a child keeps the
parent's environment out of it).  One JSON line per case: the winner record of the same handle and batch under
TGP_SCREEN_ARITH=h2 (twice), TGP_SCREEN_ARITH=f32, TGP_PRUNE_SCREEN=0 and TGP_SWEEP_PRUNE=0, and what the pruned schedule did
each time.  The problems and helpers are _prune_screen_child.py's.

    _prune_screen_h2_child.py grid    the shape x acquisition x sense x length-scale grid
    _prune_screen_h2_child.py ties    a batch whose bounds all tie"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _prune_screen_child as base             # noqa: E402  (puts the repository root on sys.path)

NS, M, DS = (300, 1100), 4099, (1, 5, 32, 40)
SWITCHES = base.SWITCHES + ("TGP_SCREEN_ARITH",)


def grid_cases():
    for N, D, acq, sense, ard in itertools.product(NS, DS, ("ei", "pi", "ucb"), ("min", "max"), (False, True)):
        yield N, M, D, acq, sense, ard


def run(gp, a, env):
    os.environ.pop("TGP_SCREEN_ARITH", None)
    return base.run(gp, a, env)


def five(gp, a):
    h, ph = run(gp, a, {"TGP_SCREEN_ARITH": "h2"})
    hb, phb = run(gp, a, {"TGP_SCREEN_ARITH": "h2"})
    f, pf = run(gp, a, {"TGP_SCREEN_ARITH": "f32"})
    s0, p0 = run(gp, a, {"TGP_PRUNE_SCREEN": "0"})
    off, poff = run(gp, a, {"TGP_SWEEP_PRUNE": "0"})
    return dict(h2=h, again=hb, f32=f, noscreen=s0, unpruned=off, p_h2=ph, p_again=phb, p_f32=pf, p_noscreen=p0, p_unpruned=poff)


def main(which):
    import turbo_amd as ta
    os.environ["TGP_PRUNE_MIN_WORK"] = "0"
    if which == "grid":
        for N, M_, D, acq, sense, ard in grid_cases():
            X, y, ls, Xc = base.problem(N, D, M_, ard)
            gp = ta.NativeGP(0, "f32")
            gp.fit(X, y, "rbf", base.CONSTANT, ls if ard else float(ls[0]), base.NOISE, 1e-10, True)
            gp.set_candidates(Xc)
            print(json.dumps(dict(case=[N, M_, D, acq, sense, ard], **five(gp, base.acq_args(acq, sense, y)))), flush=True)
    else:
        N, D = 1100, 32
        X, y, ls, Xc = base.problem(N, D, M, False, True)
        gp = ta.NativeGP(0, "f32")
        gp.fit(X, y, "rbf", base.CONSTANT, float(ls[0]), base.NOISE, 1e-10, True)
        gp.set_candidates(Xc)
        print(json.dumps(dict(case="ties", **five(gp, base.acq_args("ei", "min", y)))), flush=True)
    print("prune-screen-h2 ok")


if __name__ == "__main__":
    main(sys.argv[1])
