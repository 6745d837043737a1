"""Child process of tests/test_gpu_prune_spec.py (the pruned sweep's switches are read per call or once per process, and a
child keeps the parent's environment out of it).  One JSON line per sweep or sequence of sweeps.

    _prune_spec_child.py grid       TGP_PRUNE_SPEC=2 / 0 and TGP_SWEEP_PRUNE=0 on one handle per configuration, every
                                    acquisition and sense; with TGP_PRUNE_SPEC_CAP=1 again; the winner record on the device
    _prune_spec_child.py miss       the same for EI with TGP_PRUNE_MARGIN=1000 (read once): every candidate outside the lb
                                    set survives, so the extras cannot cover them
    _prune_spec_child.py pairs      launch pairs of 1024 rows and TGP_PRUNE_TOP=512: picks + extras span two of them
    _prune_spec_child.py trigger    TGP_PRUNE_SPEC=1: which sweeps of a handle speculate"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _prune_screen_child as screen            # noqa: E402

N, M = 300, 4099
SWITCHES = screen.SWITCHES + ("TGP_SCREEN_ARITH", "TGP_SLAB_GB", "TGP_CHUNK", "TGP_PRUNE_SPEC", "TGP_PRUNE_SPEC_CAP")
PER_CALL = ("TGP_SWEEP_PRUNE", "TGP_PRUNE_SPEC", "TGP_PRUNE_SPEC_CAP")
# every survivor set is contracted as it is (the branch "direct" of tests/test_gpu_prune_paths.py), whatever its size
BASE = {"TGP_PRUNE_FRAC": "1", "TGP_PRUNE_DIRECT": "100000"}

# name -> (dtype, kernel, D, ARD): the fp16 screen, the f32 screen, the tight bound pass alone
CONFIGS = {
    "h2": ("f32", "rbf", 16, True),
    "f32": ("f32", "rbf", 5, False),
    "f64": ("f64", "matern52", 5, False),
}
ACQS, SENSES = ("ei", "pi", "ucb"), ("max", "min")


def handle(ta, name):
    dtype, kind, D, ard = CONFIGS[name]
    X, y, ls, Xc = screen.problem(N, D, M, ard)
    gp = ta.NativeGP(0, dtype)
    gp.fit(X, y, kind, screen.CONSTANT, ls if ard else float(ls[0]), screen.NOISE, 1e-10, True)
    gp.set_candidates(Xc)
    gp.profile_enable(True)
    return gp, y, Xc


def run(gp, a, env):
    for k in PER_CALL:
        os.environ.pop(k, None)
    os.environ.update(env)
    gp.profile_reset()
    r = gp.sweep(*a)
    prof = gp.profile_read()
    return dict(rec=screen.rec(r), prune=gp.last_prune(), spec=gp.last_prune_spec(),
                launches=dict(kstar=prof["kstar_launches"], trmm=prof["trmm_launches"]))


def three(gp, a, cap):
    """the same sweep speculating always, never, and unpruned"""
    return dict(spec2=run(gp, a, {"TGP_PRUNE_SPEC": "2", "TGP_PRUNE_SPEC_CAP": str(cap)}),
                spec0=run(gp, a, {"TGP_PRUNE_SPEC": "0"}),
                unpruned=run(gp, a, {"TGP_SWEEP_PRUNE": "0"}))


def main(which):
    os.environ.update(BASE)
    os.environ["TGP_PRUNE_MIN_WORK"] = "0"
    if which == "miss":
        os.environ["TGP_PRUNE_MARGIN"] = "1000"
    if which == "pairs":
        os.environ.update({"TGP_SLAB_GB": "0.001", "TGP_CHUNK": "1024", "TGP_PRUNE_TOP": "512"})
    import turbo_amd as ta
    if which in ("grid", "miss"):
        import torch
        for name in CONFIGS:
            gp, y, Xc = handle(ta, name)
            for acq in (ACQS if which == "grid" else ("ei",)):
                for sense in SENSES:
                    a = screen.acq_args(acq, sense, y)
                    for cap in (128, 1):
                        if cap == 1 and (sense == "min" or which == "miss"):
                            continue
                        print(json.dumps(dict(case=[name, acq, sense, cap], **three(gp, a, cap))), flush=True)
            # the winner record on the device
            rec = torch.zeros(Xc.shape[1] + 2, dtype=torch.float64, device="cuda:0")
            gp.set_winner_out(rec.data_ptr(), 7000, keepalive=rec)
            a = screen.acq_args("ei", "max", y)
            for cap in (128,):
                out = {}
                for key, env in (("spec2", {"TGP_PRUNE_SPEC": "2", "TGP_PRUNE_SPEC_CAP": str(cap)}), ("unpruned", {"TGP_SWEEP_PRUNE": "0"})):
                    rec.fill_(-3.0)
                    torch.cuda.synchronize()
                    r = run(gp, a, env)
                    gp.winner_wait(torch.cuda.current_stream().cuda_stream)
                    torch.cuda.synchronize()
                    w = rec.cpu().numpy()
                    i = r["rec"]["best_idx"]
                    r["winner"] = dict(val=screen.bits(w[0]), idx=float(w[1]), row_ok=bool(w[2:].tobytes() == Xc[i].tobytes()))
                    out[key] = r
                print(json.dumps(dict(case=["winner", name, cap], **out)), flush=True)
            gp.set_winner_out(None)
            gp.close()
    elif which == "pairs":
        for name in CONFIGS:
            gp, y, _ = handle(ta, name)
            a = screen.acq_args("ei", "max", y)
            runs = three(gp, a, 1000)
            print(json.dumps(dict(case=[name, "ei", "max", 1000], chunk=int(gp.sweep_geometry()[0]), **runs)), flush=True)
            gp.close()
    else:
        cap = 4096
        for name in CONFIGS:
            gp, y, _ = handle(ta, name)
            some = screen.acq_args("ei", "max", y)              # survivors outside the lb set
            none = screen.acq_args("ei", "min", y)              # the lb set holds every candidate that can win
            env = {"TGP_PRUNE_SPEC": "1", "TGP_PRUNE_SPEC_CAP": str(cap)}
            seq = [run(gp, a, env) for a in (some, some, some, none, some, some)]
            print(json.dumps(dict(case=["trigger", name], cap=cap, seq=seq, unpruned=run(gp, some, {"TGP_SWEEP_PRUNE": "0"}))), flush=True)
            gp.close()
    print("prune-spec ok")


if __name__ == "__main__":
    main(sys.argv[1])
