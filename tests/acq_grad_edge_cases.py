"""The models, batches, bars and the one comparison of the acquisition gradient's edge tests -- TEST INFRASTRUCTURE shared
by tests/test_acq_grad_reference.py (CPU: the 80-bit closed form against its own central differences, the f64
restatement against the 80-bit form, and the proof that the bars reject the slips they are there for) and
tests/test_gpu_acq_grad_edges.py with its child tests/_acq_grad_child.py (tgp_acq_grad's kernels).

Models: tests/cov_edge_cases.py's A-H unchanged (their data(), fit_handle(), hp_fit(): c = 1.3, noise 1e-3, jitter 1e-10,
normalize_y, row 5 of the queries a training point, H the appended fit judged against the refit at APPEND_BAR) and, by
the same recipe, what the query kernels need beyond them (NEW below).

A batch is a model and rows of its query points: "base" the leading 48 (three groups of 16, QM_PTS of the matrix-core
products), "tail255" / "tail256" / "tail257" (model D) sixteen rows behind them in the call of that m, its last two among them
(_tail_rows), "limit" (model F) 32 rows of the m = 4096 call.

Quantities (KEYS): mu (ACQ_NONE), sigma (ACQ_SIGMA: UCB with beta = inf), UCB with beta = 2, PI and EI with xi = 0.01 and
the incumbent y.min() (sf = -1) or y.max() (sf = +1); each as a value and as a gradient.

Bars, u = 2^-53.  An error is a fraction of the batch's 80-bit maximum of the quantity's magnitude (for the value of mu:
of the prior scale, cov_reference.scales).   bar = min(FACTOR max(e_ref, N u), CAP)
  e_ref   the f64 restatement's own error against the 80-bit closed form for that batch and quantity, computed here,
          never taken from the code under test;
  FACTOR  cov_edge_cases.FACTOR (64) and its reason: room for an explicit inverse factor and fixed-order MFMA sums over a
          backward-stable solve;
  CAP     1e-9, a condition, not a measurement: where 10 max(e_ref, N u) is above it the reference judges nothing, which
          is an error here.
A batch also judges nothing where an acquisition is flat on it: for every batch and quantity the 80-bit maximum of
|gradient| is at least FLAT (1e-6) of (prior scale / smallest length scale) -- checked on the CPU.  No entry is excluded
anywhere: row 5 stays in.

Two places where the rules above cannot hold as they stand, and what holds there instead:
  S1, gradient of mu   one training point under normalize_y has yn = 0, so alpha = 0 and mu is y_mean everywhere: the
          gradient is identically 0 in the 80-bit reference, on every batch.  A scale of exactly 0 asks for exact zeros:
          the error is 0 where every entry compared is 0 and inf otherwise.
  G, PI and EI         mu's own e_ref on G is 1e-11 of the prior scale (cond(K) of some 1e6: no f64 algorithm does better)
          and sigma is 0.02 ... 0.07, so Z = diff / sigma is uncertain by some 5e-10 and PI, EI and their gradients by
          3e-10 ... 5e-10 of their batch maxima, on any rows of G: ten times that is above the cap, the 80-bit posterior
          cannot judge them.  BEYOND_THE_CAP lists them (tests/test_acq_grad_reference.py: every listed case is indeed
          beyond the cap, and no other is), and they are judged in two steps that together say the same: mu, sigma and
          their gradients against the 80-bit reference as everywhere (the cap holds: mu's bar on G is 7e-10), and PI / EI
          against the 80-bit closed form of the acquisition AT the posterior the code itself returned (its ACQ_NONE and
          ACQ_SIGMA results), with e_ref the f64 restatement of the acquisition at those same inputs.  The conditioning
          is out of that second comparison, so its bars are the tightest of all.
"""
import numpy as np

import acq_grad_reference_hp as ar
import cov_edge_cases as ec
import cov_reference as cr

LD = np.longdouble
U, FACTOR, CAP, APPEND_BAR = ec.U, ec.FACTOR, 1e-9, ec.APPEND_BAR
FLAT = 1e-6
XI, BETA = 0.01, 2.0
M_BASE = 48

NEW = {
    "S1": dict(N=1, D=1, kind="rbf", ard=False, dtype="f64"),         # y_std exactly 0 -> 1
    "S2": dict(N=64, D=64, kind="matern52", ard=True, dtype="f64"),   # Np = 64, four threads per row, every lane a dimension
    "S3": dict(N=65, D=63, kind="matern12", ard=False, dtype="f64"),  # Np = 128, one padding lane
    "S4": dict(N=100, D=65, kind="matern32", ard=True, dtype="f64"),  # one dimension too wide for the one-launch path: the general kernels below N = 128, a partial last 16-chunk
    "I": dict(N=520, D=5, kind="matern32", ard=True, dtype="f64"),    # Np = 768: the 8-wave class of query_waves, partial last chunk
}
ec.EXTRA.update(NEW)
MODELS = dict(ec.MODELS)
MODELS.update(NEW)
NAMES = list(MODELS)

# key -> (quantity of acq_grad_reference_hp, the library's acquisition, sf, which incumbent, param)
CASES = {
    "mu": ("mu", "ACQ_NONE", 1.0, None, 0.0),
    "sigma": ("sigma", "ACQ_SIGMA", 1.0, None, 0.0),
    "ucb_min": ("ucb", "ACQ_UCB", -1.0, None, BETA),
    "ucb_max": ("ucb", "ACQ_UCB", 1.0, None, BETA),
    "pi_min": ("pi", "ACQ_PI", -1.0, "min", XI),
    "pi_max": ("pi", "ACQ_PI", 1.0, "max", XI),
    "ei_min": ("ei", "ACQ_EI", -1.0, "min", XI),
    "ei_max": ("ei", "ACQ_EI", 1.0, "max", XI),
}
KEYS = list(CASES)
M_EDGES = (1, 15, 16, 17, 32, 33, 47)          # (b): around the groups of QM_PTS = 16 points
M_FINAL = (255, 256, 257)                      # (c): the second pass of the last workgroup's finalisation starts at point 256
M_LIMIT = ec.M_LIMIT

BEYOND_THE_CAP = {"G": ("pi_min", "pi_max", "ei_min", "ei_max")}

_cache = {}


def rows(batch):
    """(m of the call the batch belongs to, the rows of it that the batch holds)"""
    if batch == "base":
        return ec.M_BASE, np.arange(M_BASE)
    if batch.startswith("tail"):                  # "tail255", "tail256", "tail257"
        m = int(batch[4:])
        assert m in M_FINAL
        return m, np.concatenate([_tail_rows(), [m - 2, m - 1]])
    if batch == "limit":
        I = {0, 255, 256, 2047, 2048, M_LIMIT - 1}
        for r in np.random.RandomState(M_LIMIT).permutation(M_LIMIT):
            if len(I) >= 32:
                break
            I.add(int(r))
        return M_LIMIT, np.array(sorted(I))
    raise ValueError(batch)


def _tail_rows():
    """model D: fourteen of rows 48 ... 252 chosen by the 80-bit reference alone -- in turn, for PI and EI and both sf,
    the row not yet taken where that gradient is largest.  With the last two rows of the call they are a tail batch.  On
    most rows of D (the last sixteen of every m in M_FINAL among them) PI and EI towards the maximum are flat to 1e-14 of
    the scale, and a flat batch judges nothing."""
    if "tail" not in _cache:
        lo, hi = M_BASE, min(M_FINAL) - 2
        post = ar.posterior(ec.hp_fit("D"), ec.data("D")[3][lo:hi])
        order = []
        for key in ("pi_min", "pi_max", "ei_min", "ei_max"):
            q, _, sf, which, param = CASES[key]
            g = ar.acquisition(q, post["mu"], post["sigma"], sf, incumbent("D", which), param, post["dmu"], post["dsigma"])[1]
            order.append(list(np.argsort(-np.abs(g).max(1).astype(np.float64), kind="stable")))
        taken = []
        while len(taken) < 14:
            for o in order:
                r = next(int(i) for i in o if int(i) not in taken)
                if len(taken) < 14:
                    taken.append(r)
        _cache["tail"] = np.array(sorted(lo + r for r in taken))
    return _cache["tail"]


def points(name, batch="base"):
    m, I = rows(batch)
    return ec.data(name, m)[3][I]


def incumbent(name, which):
    y = ec.data(name)[1]
    return 0.0 if which is None else float(y.min() if which == "min" else y.max())


def call_args(name, key):
    """(name of the library's acquisition constant, sf, incumbent, param) of tgp_acq_grad for this quantity"""
    _, acq, sf, which, param = CASES[key]
    return acq, sf, incumbent(name, which), param


def query_all(gp, name, Xq, keys=KEYS):
    """{key: (value (m,), gradient (m, D))}: one NativeGP.acq_grad call per quantity"""
    import turbo_amd._lib as L
    out = {}
    for key in keys:
        acq, sf, inc, param = call_args(name, key)
        out[key] = gp.acq_grad(Xq, getattr(L, acq), sf, inc, param)
    return out


def hp_reference(name, batch="base"):
    """{key: (value, gradient)} in long double: made once per batch, never modified"""
    k = ("hp", name, batch)
    if k not in _cache:
        post = ar.posterior(ec.hp_fit(name), points(name, batch))
        out = {}
        for key, (q, _, sf, which, param) in CASES.items():
            out[key] = ar.acquisition(q, post["mu"], post["sigma"], sf, incumbent(name, which), param, post["dmu"], post["dsigma"])
            for a in out[key]:
                a.setflags(write=False)
        _cache[k] = out
    return _cache[k]


def f64_results(name, batch="base", slip=None):
    """{key: (value, gradient)} of the f64 restatement (slip: one of acq_grad_reference_hp.SLIPS)"""
    post = ar.posterior_f64(ec.reference(name), points(name, batch), slip)
    return {key: ar.acquisition_f64(q, post, sf, incumbent(name, which), param, slip)
            for key, (q, _, sf, which, param) in CASES.items()}


def scales(name, batch="base"):
    """{key: (value scale, gradient scale)}: the batch's 80-bit maxima (the value of mu: the prior scale)"""
    ref = hp_reference(name, batch)
    ms = float(cr.scales(ec.reference(name))[1])
    return {key: (ms if key == "mu" else float(np.abs(v).max()), float(np.abs(g).max())) for key, (v, g) in ref.items()}


def errors(name, batch, results):
    """{key: (value error, gradient error)} of results against the 80-bit reference as fractions of the scales;
    differences formed in long double, over every entry.  Results of fewer rows than the batch are its LEADING rows (a
    call of m < 48 points), under the batch's scales."""
    ref, sc = hp_reference(name, batch), scales(name, batch)
    out = {}
    for key, (v, g) in results.items():
        hv, hg = ref[key]
        n = len(v)
        assert 1 <= n <= len(hv) and np.shape(v) == (n,) and np.shape(g) == (n,) + hg.shape[1:], (key, np.shape(v), np.shape(g))
        out[key] = (_fraction(v, hv[:n], sc[key][0]), _fraction(g, hg[:n], sc[key][1]))
    return out


def _fraction(got, want, scale):
    """max |got - want| / scale, formed in long double; a scale of exactly 0 (the quantity is identically 0) asks for
    exact zeros"""
    d = float(np.abs(np.asarray(got).astype(LD) - want).max())
    if scale == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / scale


def e_ref(name, batch="base"):
    k = ("eref", name, batch)
    if k not in _cache:
        _cache[k] = errors(name, batch, f64_results(name, batch))
    return _cache[k]


def _bar(e, n):
    assert 10 * max(e, n * U) <= CAP, "the reference errs by %.3g under a cap of %.3g: too loose to judge this case" % (e, CAP)
    return min(FACTOR * max(e, n * U), CAP)


def bars(name, batch="base"):
    """{key: (value bar, gradient bar)} of the comparison with the 80-bit posterior (not for BEYOND_THE_CAP's cases)"""
    if MODELS[name].get("append"):
        return {key: (APPEND_BAR, APPEND_BAR) for key in KEYS}
    N = MODELS[name]["N"]
    return {key: (_bar(ev, N), _bar(eg, N)) for key, (ev, eg) in e_ref(name, batch).items()
            if key not in BEYOND_THE_CAP.get(name, ())}


def at_own_posterior(name, batch, results, key):
    """(errors, e_ref) of results[key], each (value, gradient), against the 80-bit closed form of the acquisition at the
    posterior that results itself holds (its "mu" and "sigma" entries); e_ref: the f64 restatement of the acquisition at
    those inputs.  Fractions of the same scales as everywhere."""
    q, _, sf, which, param = CASES[key]
    inc = incumbent(name, which)
    (mu, dmu), (sg, dsg) = results["mu"], results["sigma"]
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    hv, hg = ar.acquisition(q, f64(mu), f64(sg), sf, inc, param, f64(dmu).astype(LD), f64(dsg).astype(LD))
    fv, fg = ar.acquisition_f64(q, dict(mu=f64(mu), sigma=f64(sg), dmu=f64(dmu), dsigma=f64(dsg)), sf, inc, param)
    sv, sg_ = scales(name, batch)[key]
    return ((_fraction(results[key][0], hv, sv), _fraction(results[key][1], hg, sg_)),
            (_fraction(fv, hv, sv), _fraction(fg, hg, sg_)))


def flatness(name, batch="base"):
    """{key: the 80-bit maximum of |gradient| over (prior scale / smallest length scale)}: at least FLAT, or the batch
    judges nothing"""
    ls = np.atleast_1d(ec.data(name)[2])
    unit = float(cr.scales(ec.reference(name))[1]) / float(ls.min())
    return {key: s[1] / unit for key, s in scales(name, batch).items()}


def judge(name, batch, results):
    """THE comparison of tgp_acq_grad's results (or anything that claims to be them) with the 80-bit reference:
    {key: dict(e_ref_value, bar_value, err_value, ratio_value, e_ref_grad, bar_grad, err_grad, ratio_grad, ok)} and, under
    "ok", whether every key passed"""
    err, bar, ere = errors(name, batch, results), bars(name, batch), e_ref(name, batch)
    out = {}
    for key in results:
        if key in BEYOND_THE_CAP.get(name, ()):
            (ev, eg), (rv, rg) = at_own_posterior(name, batch, results, key)
            bv, bg = _bar(rv, MODELS[name]["N"]), _bar(rg, MODELS[name]["N"])
        else:
            (ev, eg), (bv, bg), (rv, rg) = err[key], bar[key], ere[key]
        out[key] = dict(e_ref_value=rv, bar_value=bv, err_value=ev, ratio_value=ev / bv,
                        e_ref_grad=rg, bar_grad=bg, err_grad=eg, ratio_grad=eg / bg, ok=bool(ev <= bv and eg <= bg))
    out["ok"] = all(out[key]["ok"] for key in results)
    return out


def show(name, what, j):
    """the figures of a judge() result, one line per quantity (printed before anything is asserted)"""
    for key, r in j.items():
        if key != "ok":
            print("%s %s %-7s value %.3g (bar %.3g, e_ref %.3g, ratio %.3g)  gradient %.3g (bar %.3g, e_ref %.3g, ratio %.3g)"
                  % (name, what, key, r["err_value"], r["bar_value"], r["e_ref_value"], r["ratio_value"],
                     r["err_grad"], r["bar_grad"], r["e_ref_grad"], r["ratio_grad"]))


def flat_bytes(results):
    """the bytes of a {key: (value, gradient)} result, keys in sorted order"""
    return b"".join(np.ascontiguousarray(a).tobytes() for key in sorted(results) for a in results[key])


def leading(results, m):
    return {key: (v[:m], g[:m]) for key, (v, g) in results.items()}
