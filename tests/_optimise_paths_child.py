"""The cases of test_gpu_optimise_paths.py, importable (the default switches, in the test's own process) and runnable as
a child process: csrc/tuning.hpp reads the TGP_* switches once per process, so every other selection gets a process of
its own.  `python _optimise_paths_child.py GROUP...` prints one JSON line with a key per group.

Every case goes through the C ABI itself and is recorded as
    {"rc", "err" (tgp_last_error), "ev" (the evaluation count), "status" (per start), and a SHA-256 per returned array}.
`python _optimise_paths_child.py --record` writes tests/golden/optimise_paths_parent.json (recorded from the build BEFORE
the optimiser entries moved into csrc/api_optimise.hpp; the refactor has to return these bytes).
Test helper, not product code."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FIXTURE = os.path.join(ROOT, "tests", "golden", "optimise_paths_parent.json")
INF = float("inf")


def _L():
    import turbo_amd as ta
    return ta._lib


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _problem(N, D, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(0, 1, (N, D))
    y = np.sin(3 * X[:, :3].sum(1)) + 0.05 * rng.normal(size=N)
    return X, y


def _singular(N):
    """points 100 length scales apart, the last a copy of the third: K = I with two equal rows whatever the
    hyper-parameters inside the box -- a pivot that is exactly 0 without a noise term"""
    X = np.zeros((N, 2))
    X[:, 0] = 100.0 * np.arange(N)
    X[N - 1] = X[2]
    return X, np.random.RandomState(N).normal(size=N)


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def hyper_call(gp, entry, X, y, kind, theta0, n_ls, lo, hi, jitter=1e-10, normalize_y=True, max_iter=15, S=None):
    """tgp_fit_optimise / tgp_fit_lbfgsb as they stand in the C ABI"""
    L = _L()
    X, y, theta0, lo, hi = _c(X), _c(y), _c(np.atleast_2d(theta0)), _c(lo), _c(hi)
    S = theta0.shape[0] if S is None else S
    P = theta0.shape[1]
    n = max(1, min(S, 64))
    theta, f = np.full((n, P), -7.25), np.full(n, -7.25)
    st = np.full(n, -7, dtype=np.int64)
    ev = ctypes.c_int64(-7)
    rc = getattr(gp.lib, "tgp_fit_" + entry)(gp._h, L._ptr(X), X.shape[0], X.shape[1], L._ptr(y), L.KERNELS[kind], L._ptr(theta0),
                                             S, int(n_ls), L._ptr(lo), L._ptr(hi), float(jitter), 1 if normalize_y else 0,
                                             int(max_iter), L._ptr(theta), L._ptr(f), st.ctypes.data_as(L._i64p), ctypes.byref(ev))
    return dict(rc=rc, err=gp.lib.tgp_last_error(gp._h).decode(), ev=ev.value, status=st.tolist(), theta=_sha(theta), f=_sha(f))


def refine_call(gp, entry, X0, lo, hi, acq, sf=1.0, incumbent=0.0, param=0.0, max_iter=5, R=None):
    """tgp_acq_refine / tgp_acq_lbfgsb as they stand in the C ABI"""
    L = _L()
    X0, lo, hi = _c(np.atleast_2d(X0)), _c(lo), _c(hi)
    R = X0.shape[0] if R is None else R
    n = max(1, min(R, X0.shape[0]))
    x, v = np.full((n, X0.shape[1]), -7.25), np.full(n, -7.25)
    st = np.full(n, -7, dtype=np.int64)
    ev = ctypes.c_int64(-7)
    rc = getattr(gp.lib, "tgp_acq_" + entry)(gp._h, L._ptr(X0), R, L._ptr(lo), L._ptr(hi), int(acq), float(sf), float(incumbent),
                                             float(param), int(max_iter), L._ptr(x), L._ptr(v), st.ctypes.data_as(L._i64p),
                                             ctypes.byref(ev))
    return dict(rc=rc, err=gp.lib.tgp_last_error(gp._h).decode(), ev=ev.value, status=st.tolist(), x=_sha(x), v=_sha(v))


def sample_call(gp, X, y, kind, theta0, n_ls, lo, hi, S=2, burn=1, thin=1, seed=7):
    L = _L()
    X, y, theta0, lo, hi = _c(X), _c(y), _c(theta0), _c(lo), _c(hi)
    n = max(1, min(S, 64))
    theta, lml = np.full((n, theta0.shape[0]), -7.25), np.full(n, -7.25)
    ev, npd = ctypes.c_int64(-7), ctypes.c_int64(-7)
    rc = gp.lib.tgp_hyper_sample(gp._h, L._ptr(X), X.shape[0], X.shape[1], L._ptr(y), L.KERNELS[kind], L._ptr(theta0), int(n_ls),
                                 L._ptr(lo), L._ptr(hi), 1e-10, 1, S, burn, thin, None, seed, L._ptr(theta), L._ptr(lml),
                                 ctypes.byref(ev), ctypes.byref(npd))
    return dict(rc=rc, err=gp.lib.tgp_last_error(gp._h).decode(), ev=ev.value, not_pd=npd.value, theta=theta, lml=lml)


def _box(n_ls):
    lo = np.log(np.array([1e-2] + [5e-2] * n_ls + [1e-6]))
    hi = np.log(np.array([1e2] + [2e1] * n_ls + [1e0]))
    return lo, hi


def _starts(S, n_ls, seed):
    lo, hi = _box(n_ls)
    th = np.random.RandomState(seed).uniform(lo, hi, (S, 2 + n_ls))
    th[0] = np.log(np.array([1.0] + [0.7] * n_ls + [1e-2]))
    return th


# name -> (N, D, S, ard, variant, max_iter); every one runs through both entries
HYPER_CASES = [
    ("N5", 5, 2, 1, False, None, 15), ("N64", 64, 2, 3, False, None, 15), ("N65 ard", 65, 2, 3, True, None, 15),
    ("N128 S5", 128, 2, 5, False, None, 15), ("N129 S1", 129, 2, 1, False, None, 15), ("N129 S3 ard", 129, 2, 3, True, None, 15),
    ("N129 S5", 129, 2, 5, False, None, 15), ("N30 D65", 30, 65, 3, False, None, 15), ("N30 D65 ard", 30, 65, 1, True, None, 4),
    ("N30 one fixed", 30, 2, 3, True, "one fixed", 15), ("N129 one fixed", 129, 2, 3, True, "one fixed", 15),
    ("N30 all fixed", 30, 2, 3, False, "all fixed", 15), ("N129 all fixed", 129, 2, 3, False, "all fixed", 15),
    ("N30 no noise", 30, 2, 3, False, "no noise", 15), ("N129 no noise", 129, 2, 3, False, "no noise", 15),
    ("N30 max_iter 1", 30, 2, 3, False, None, 1), ("N30 max_iter 2", 30, 2, 3, True, None, 2),
    ("N129 max_iter 1", 129, 2, 3, False, None, 1), ("N129 max_iter 2", 129, 2, 3, True, None, 2),
    ("N30", 30, 2, 3, False, None, 15),
    ("not PD one launch", 6, 2, 3, False, "singular", 15), ("not PD streams", 6, 2, 3, False, "singular no noise", 15),
]


def _hyper_case(gp, entry, case):
    _, N, D, S, ard, variant, max_iter = case
    n_ls = D if ard else 1
    X, y = _singular(N) if variant and variant.startswith("singular") else _problem(N, D, N + D)
    th, (lo, hi) = _starts(S, n_ls, N + S), _box(n_ls)
    jitter = 1e-10
    if variant == "one fixed":
        lo[1] = hi[1] = np.log(0.6)
    elif variant == "all fixed":
        lo = hi = np.log(np.array([1.3] + [0.6] * n_ls + [1e-2]))
    elif variant in ("no noise", "singular no noise"):
        lo[-1] = hi[-1] = -INF
    if variant == "singular":            # a noise term below half an ulp of the diagonal
        lo[-1], hi[-1] = -60.0, -50.0
    if variant and variant.startswith("singular"):
        jitter = 0.0
        lo[0] = hi[0] = 0.0              # (the constant at 1: the pivot is 1 - 1)
        lo[1], hi[1] = np.log(0.5), np.log(2.0)
    return hyper_call(gp, entry, X, y, "matern52" if N % 2 else "rbf", th, n_ls, lo, hi, jitter=jitter, max_iter=max_iter)


def hyper(only=None):
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    res = {}
    for case in HYPER_CASES:
        if only is not None and case[0] not in only:
            continue
        for entry in ("optimise", "lbfgsb"):
            res["%s / %s" % (case[0], entry)] = _hyper_case(gp, entry, case)
    gp.close()
    return res


def hyper_n30():
    """N = 30 through both entries: what TGP_SMALL=0 sends down the same path"""
    return hyper(only=("N30",))


def _fitted(N):
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    X, y = _problem(N, 2, N)
    gp.fit(X, y, "matern52", 1.2, 0.12, 1e-2, 1e-10, True)
    gp.mes_set_maxima(np.array([y.max() + 0.05, y.max() + 0.2]))
    return gp, X, y


def refine():
    L = _L()
    res = {}
    lo, hi = np.array([0.1, 0.0]), np.array([0.9, 1.0])
    for N in (30, 200):
        gp, X, y = _fitted(N)
        # an inner start, one outside the box (clipped into it), one ON an observed point (sigma ~ 0 there)
        X0 = np.array([[0.35, 0.62], [1.4, -0.3], X[3]])
        inc = float(np.median(y))
        for entry, acqs in (("refine", ("EI", "UCB")), ("lbfgsb", ("EI", "UCB", "MES"))):
            for acq in acqs:
                param = 2.0 if acq == "UCB" else 0.01
                for R in (1, 3):
                    for max_iter in (1, 3, 4, 5, 40):
                        if max_iter == 40 and R == 1:
                            continue
                        res["N%d %s %s R%d it%d" % (N, entry, acq, R, max_iter)] = refine_call(
                            gp, entry, X0[:R], lo, hi, getattr(L, "ACQ_" + acq), 1.0, inc, param, max_iter)
        gp.close()
    return res


def refusals():
    import turbo_amd as ta
    L = _L()
    res = {}
    gp, X, y = _fitted(30)
    lo, hi = np.zeros(2), np.ones(2)
    X0 = np.full((3, 2), 0.5)
    for entry in ("refine", "lbfgsb"):
        res[entry + " R=0"] = refine_call(gp, entry, X0, lo, hi, L.ACQ_EI, R=0)
        res[entry + " R=4097"] = refine_call(gp, entry, X0, lo, hi, L.ACQ_EI, R=4097)
        res[entry + " max_iter=0"] = refine_call(gp, entry, X0, lo, hi, L.ACQ_EI, max_iter=0)
        res[entry + " lo > hi"] = refine_call(gp, entry, X0, np.array([0.0, 0.7]), np.array([1.0, 0.2]), L.ACQ_EI)
        res[entry + " NaN bound"] = refine_call(gp, entry, X0, np.array([0.0, np.nan]), hi, L.ACQ_EI)
        res[entry + " no acquisition"] = refine_call(gp, entry, X0, lo, hi, L.ACQ_NONE)
        res[entry + " sf"] = refine_call(gp, entry, X0, lo, hi, L.ACQ_EI, sf=0.5)
        # (the order of the refusals: the acquisition / own text, then max_iter, then the box)
        res[entry + " R=0, max_iter=0, lo > hi"] = refine_call(gp, entry, X0, hi, lo, L.ACQ_EI, max_iter=0, R=0)
        res[entry + " max_iter=0, lo > hi"] = refine_call(gp, entry, X0, hi, lo, L.ACQ_EI, max_iter=0)
    res["refine MES"] = refine_call(gp, "refine", X0, lo, hi, L.ACQ_MES)
    res["lbfgsb acq 6"] = refine_call(gp, "lbfgsb", X0, lo, hi, 6)
    gp.close()
    fresh = ta.NativeGP(0, "f64")
    for entry in ("refine", "lbfgsb"):
        res[entry + " not fitted"] = refine_call(fresh, entry, X0, lo, hi, L.ACQ_EI)
    Xp, yp = _problem(30, 2, 1)
    blo, bhi = _box(1)
    th = _starts(3, 1, 2)
    for entry in ("optimise", "lbfgsb"):
        res["fit_" + entry + " S=65"] = hyper_call(fresh, entry, Xp, yp, "rbf", np.repeat(th, 22, 0)[:65], 1, blo, bhi)
        res["fit_" + entry + " S=0"] = hyper_call(fresh, entry, Xp, yp, "rbf", th, 1, blo, bhi, S=0)
        res["fit_" + entry + " max_iter=0"] = hyper_call(fresh, entry, Xp, yp, "rbf", th, 1, blo, bhi, max_iter=0)
        res["fit_" + entry + " n_ls=3"] = hyper_call(fresh, entry, _problem(30, 4, 1)[0], yp, "rbf", _starts(3, 3, 2), 3, *_box(3))
        for name, at, v in (("inf", 1, INF), ("nan", 0, np.nan), ("noise hi = -inf alone", 2, -INF)):
            b = bhi.copy()
            b[at] = v
            res["fit_" + entry + " bound " + name] = hyper_call(fresh, entry, Xp, yp, "rbf", th, 1, blo, b)
        res["fit_" + entry + " lo > hi"] = hyper_call(fresh, entry, Xp, yp, "rbf", th, 1, bhi, blo)
        r = dict(rc=getattr(fresh.lib, "tgp_fit_" + entry)(fresh._h, None, 30, 2, None, 0, None, 3, 1, None, None, 1e-10, 1, 5,
                                                           None, None, None, None))
        r["err"] = fresh.lib.tgp_last_error(fresh._h).decode()
        res["fit_" + entry + " NULL"] = r
    s = sample_call(fresh, Xp, yp, "rbf", th[0], 1, blo, bhi, S=65)
    res["hyper_sample S=65"] = dict(rc=s["rc"], err=s["err"])
    s = sample_call(fresh, _problem(30, 4, 1)[0], yp, "rbf", _starts(1, 3, 2)[0], 3, *_box(3))
    res["hyper_sample n_ls=3"] = dict(rc=s["rc"], err=s["err"])
    b = bhi.copy()
    b[1] = INF
    s = sample_call(fresh, Xp, yp, "rbf", th[0], 1, blo, b)
    res["hyper_sample bound inf"] = dict(rc=s["rc"], err=s["err"])
    fresh.close()
    # the five entries on a handle of the host backend
    host = ta.NativeGP(L.DEVICE_HOST, "f64")
    host.fit(Xp, yp, "rbf", 1.0, 0.5, 1e-2, 1e-10, True)
    for entry in ("refine", "lbfgsb"):
        r = refine_call(host, entry, X0, lo, hi, L.ACQ_EI)
        res["host acq_" + entry] = dict(rc=r["rc"], err=r["err"])
    for entry in ("optimise", "lbfgsb"):
        r = hyper_call(host, entry, Xp, yp, "rbf", th, 1, blo, bhi)
        res["host fit_" + entry] = dict(rc=r["rc"], err=r["err"])
    s = sample_call(host, Xp, yp, "rbf", th[0], 1, blo, bhi)
    # (it runs there: the status, the counts' signs and finite samples; its bytes are the host's libm's)
    res["host hyper_sample"] = dict(rc=s["rc"], ran=bool(s["ev"] > 3 and s["not_pd"] >= 0),
                                    finite=bool(np.isfinite(s["theta"]).all() and np.isfinite(s["lml"]).all()))
    host.close()
    return res


def hyper_sample():
    """tgp_hyper_sample on the GPU: small fit, blocked fit, one entry fixed, and theta0 at a singular matrix"""
    import turbo_amd as ta
    gp = ta.NativeGP(0, "f64")
    res = {}
    for name, N, fixed in (("N30", 30, False), ("N130", 130, False), ("N30 one fixed", 30, True)):
        X, y = _problem(N, 2, N)
        lo, hi = _box(1)
        if fixed:
            lo[1] = hi[1] = np.log(0.6)
        s = sample_call(gp, X, y, "matern52", _starts(1, 1, 3)[0], 1, lo, hi)
        res[name] = dict(rc=s["rc"], err=s["err"], ev=s["ev"], not_pd=s["not_pd"], theta=_sha(s["theta"]), lml=_sha(s["lml"]))
    X, y = _singular(6)
    lo, hi = _box(1)
    lo[1], hi[1] = np.log(0.5), np.log(2.0)
    lo[-1] = hi[-1] = -INF
    lo[0] = hi[0] = 0.0
    th0 = np.array([0.0, 0.0, -INF])
    L = _L()
    ev, npd = ctypes.c_int64(-7), ctypes.c_int64(-7)
    out = np.full((2, 3), -7.25)
    lml = np.full(2, -7.25)
    rc = gp.lib.tgp_hyper_sample(gp._h, L._ptr(_c(X)), 6, 2, L._ptr(_c(y)), 0, L._ptr(th0), 1, L._ptr(lo), L._ptr(hi), 0.0, 1, 2, 1, 1,
                                 None, 7, L._ptr(out), L._ptr(lml), ctypes.byref(ev), ctypes.byref(npd))
    res["not PD at theta0"] = dict(rc=rc, err=gp.lib.tgp_last_error(gp._h).decode(), ev=ev.value, not_pd=npd.value)
    gp.close()
    return res


GROUPS = dict(hyper=hyper, hyper_n30=hyper_n30, refine=refine, refusals=refusals, hyper_sample=hyper_sample)
RECORDED = ("hyper", "refine", "refusals", "hyper_sample")

if __name__ == "__main__":
    if sys.argv[1:2] == ["--record"]:
        path = sys.argv[2] if len(sys.argv) > 2 else FIXTURE
        with open(path, "w") as f:
            json.dump({g: GROUPS[g]() for g in RECORDED}, f, indent=1, sort_keys=True)
            f.write("\n")
        print("recorded", path)
    else:
        print("optimise-paths " + json.dumps({g: GROUPS[g]() for g in sys.argv[1:]}))
