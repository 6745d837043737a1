"""Child process of tests/test_gpu_prune_paths.py (the pruned sweep's switches are read per call or once per process, and a
child keeps the parent's environment out of it).  One JSON line per case: the winner record of one handle and batch under
the case's switches and under TGP_SWEEP_PRUNE=0, what the pruned schedule did, and the launches the profile counted.

    _prune_paths_child.py paths     every branch of the schedule behind the bound pass
    _prune_paths_child.py many      TGP_PRUNE_MARGIN=1000 (read once): every candidate outside the lb set survives"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _prune_screen_child as screen            # noqa: E402

N, M = 300, 4099
# process-wide: launch pairs of 1024 candidates, so that a gathered set spans more than one of them
PROCESS_ENV = {"TGP_PRUNE_MIN_WORK": "0", "TGP_SLAB_GB": "0.001", "TGP_CHUNK": "1024"}
SWITCHES = screen.SWITCHES + ("TGP_SCREEN_ARITH", "TGP_SLAB_GB", "TGP_CHUNK")
PER_CALL = ("TGP_SWEEP_PRUNE", "TGP_PRUNE_FRAC", "TGP_PRUNE_DIRECT")

# name -> (dtype, kernel, D, ARD, sense, per-call environment); the acquisition is EI.
# (Sense and length scales are the ones of _prune_screen_child's grid under which a candidate OUTSIDE the lb set reaches the
# bar at this shape: with sense "min" the lb set alone holds every candidate that can win, and no case would get past step 3.)
PATHS = {
    "tight": ("f64", "matern52", 5, False, "max", {"TGP_PRUNE_FRAC": "1"}),
    "direct": ("f32", "rbf", 5, False, "max", {"TGP_PRUNE_FRAC": "1", "TGP_PRUNE_DIRECT": "100000"}),
    "gathered": ("f32", "rbf", 5, False, "max", {"TGP_PRUNE_FRAC": "1", "TGP_PRUNE_DIRECT": "0"}),
    "tight_all": ("f32", "rbf", 5, False, "max", {"TGP_PRUNE_FRAC": "0.0001", "TGP_PRUNE_DIRECT": "0"}),
    "h2": ("f32", "rbf", 16, True, "max", {"TGP_PRUNE_FRAC": "1", "TGP_PRUNE_DIRECT": "100000"}),
    "fallback": ("f64", "rbf", 5, False, "max", {"TGP_PRUNE_FRAC": "-1"}),
}
MANY = {
    "many_f32": ("f32", "rbf", 5, False, "min", {"TGP_PRUNE_FRAC": "1", "TGP_PRUNE_DIRECT": "0"}),
    "many_f64": ("f64", "matern52", 5, False, "min", {"TGP_PRUNE_FRAC": "1"}),
}


def run(gp, a, env):
    for k in PER_CALL:
        os.environ.pop(k, None)
    os.environ.update(env)
    gp.profile_reset()
    r = gp.sweep(*a)
    prof = gp.profile_read()
    return screen.rec(r), gp.last_prune(), dict(kstar=prof["kstar_launches"], trmm=prof["trmm_launches"])


def main(which):
    os.environ.update(PROCESS_ENV)
    if which == "many":
        os.environ["TGP_PRUNE_MARGIN"] = "1000"
    import turbo_amd as ta
    for name, (dtype, kind, D, ard, sense, env) in (MANY if which == "many" else PATHS).items():
        X, y, ls, Xc = screen.problem(N, D, M, ard)
        gp = ta.NativeGP(0, dtype)
        gp.fit(X, y, kind, screen.CONSTANT, ls if ard else float(ls[0]), screen.NOISE, 1e-10, True)
        gp.set_candidates(Xc)
        gp.profile_enable(True)
        a = screen.acq_args("ei", sense, y)
        s, p, n = run(gp, a, env)
        off, poff, noff = run(gp, a, {"TGP_SWEEP_PRUNE": "0"})
        print(json.dumps(dict(case=name, pruned=s, unpruned=off, p_pruned=p, p_unpruned=poff, launches=n, launches_unpruned=noff,
                              chunk=int(gp.sweep_geometry()[0]))), flush=True)
    print("prune-paths ok")


if __name__ == "__main__":
    main(sys.argv[1])
