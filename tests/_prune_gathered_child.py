"""Child process of tests/test_gpu_prune_gathered_paths.py (the pruned sweep's switches are read per call or once per process,
and a child keeps the parent's environment out of it).  One JSON line per case: the winner record of one handle and batch under
the pruned schedule (twice) and under TGP_SWEEP_PRUNE=0, and what the pruned schedule did.

    _prune_gathered_child.py few       the bounds as they are: at N = 300, D = 8 some tens of candidates outside the lb set survive
    _prune_gathered_child.py many      TGP_PRUNE_MARGIN=1000 (read once): every candidate outside the lb set survives"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _prune_screen_child as screen            # noqa: E402

M = 4096
# process-wide: an lb set of 16 and every survivor taken, so that candidates outside
# the lb set reach the bar and both gathered sets are contracted
PROCESS_ENV = {"TGP_PRUNE_MIN_WORK": "0", "TGP_PRUNE_TOP": "16", "TGP_PRUNE_FRAC": "1"}
SWITCHES = screen.SWITCHES + ("TGP_SCREEN_ARITH", "TGP_KS_JS")   # (TGP_PRUNE_MARGIN among screen.SWITCHES)
PER_CALL = ("TGP_SWEEP_PRUNE",)

# (dtype, kernel, N, D); EI, sense "max" (the sense under which a candidate outside the lb set reaches the bar at these shapes)
# (N = 1300: twelve 128-point tiles, more than the plan's eight splits -- the lb set's cross-kernel then runs twelve)
CASES = ([("f32", "rbf", N, D) for N in (300, 700) for D in (8, 32)] + [("f32", "matern52", 300, 8), ("f64", "rbf", 300, 8)] +
         [("f32", "rbf", 1300, 8), ("f64", "matern52", 1300, 8)])


def run(gp, a, env):
    for k in PER_CALL:
        os.environ.pop(k, None)
    os.environ.update(env)
    r = gp.sweep(*a)
    return screen.rec(r), gp.last_prune()


def main(which):
    os.environ.update(PROCESS_ENV)
    if which == "many":
        os.environ["TGP_PRUNE_MARGIN"] = "1000"
    import turbo_amd as ta
    for dtype, kind, N, D in CASES:
        X, y, ls, Xc = screen.problem(N, D, M, False)
        gp = ta.NativeGP(0, dtype)
        gp.fit(X, y, kind, screen.CONSTANT, float(ls[0]), screen.NOISE, 1e-10, True)
        gp.set_candidates(Xc)
        a = screen.acq_args("ei", "max", y)
        s1, p1 = run(gp, a, {})
        s1b, p1b = run(gp, a, {})
        off, poff = run(gp, a, {"TGP_SWEEP_PRUNE": "0"})
        print(json.dumps(dict(case=[dtype, kind, N, D], pruned=s1, again=s1b, unpruned=off, p_pruned=p1, p_again=p1b,
                              p_unpruned=poff)), flush=True)
    print("prune-gathered ok")


if __name__ == "__main__":
    main(sys.argv[1])
