"""The models, shapes and bars of the knowledge-gradient tests -- TEST INFRASTRUCTURE shared by
tests/test_kg_reference.py (CPU: the references against each other, the case conditions, the proof that the bars reject
the faults they are there for) and tests/test_gpu_kg.py (the kernels).

Every model: c = 1.3, X uniform in the unit cube, y = 1.5 + sin(3 sum x) + 0.3 x_0 + 0.02 normal; length scales
0.6 sqrt(D / 3) or (ARD) uniform(0.4, 0.9) sqrt(D / 3).  The discretisation points are drawn uniform in the cube, the
candidates uniform in [-0.05, 1.05]^D.  Case "n40" has noise 0 and, on purpose: candidate 5 ON training point 0,
candidate 7 ON discretisation point 3, discretisation point 4 a copy of point 1.

Bars (u = 2^-53):
  (a) the envelope arithmetic alone, kg_out against kg_reference fed the call's own outputs, ABSOLUTE in raw units:
      64 max(e_lines, (A + 1) u max_i |a_i|) -- e_lines the f64-vs-80-bit error of the reference envelope on those same
      lines; the second term the forward bound of A breakpoints, each perturbed by u |a| / db and weighted by db Phi <= db.
  (b) end to end against the 80-bit reference, as a fraction of y_std sqrt(c + noise) (kg, mu_a, mu) or of
      y_std^2 (c + noise) (cov): min(64 max(e_ref, N u), cap), cap 1e-9 resp. 1e-10 as tests/cov_edge_cases.py; e_ref the f64
      reference's own error against the 80-bit one for that case and quantity, computed here, never from the code
      under test.  64 e_ref itself must stay under the cap (asserted on the CPU).
"""
import numpy as np

import cov_reference_hp as hp
import kg_reference as kr
import kg_reference_hp as krh
from oracle import gp_oracle as G

LD = np.longdouble
U = 2.0 ** -53
FACTOR = 64.0
CAP_VAL, CAP_COV = 1e-9, 1e-10
C = 1.3
HP_ROWS = 300                # rows of a case the 80-bit comparison runs on (all of them when M <= 300)
F32_REGRET, F32_KG = 1e-3, 1e-5
ARGMAX_MIN_BEST, ARGMAX_MIN_GAP = 1e-3, 1e-6

CASES = {
    # the one-workgroup fit
    "n1": dict(N=1, D=2, A=1, M=1, kind="rbf", sf=1.0, noise=1e-2, jitter=1e-6),
    "n40": dict(N=40, D=3, A=63, M=63, kind="matern52", sf=-1.0, noise=0.0, jitter=1e-6, coincide=True),
    "n128": dict(N=128, D=2, A=2, M=65, kind="rbf", sf=1.0, noise=1e-3, jitter=1e-10),
    # the one-launch sweep
    "n129": dict(N=129, D=3, A=64, M=300, kind="matern32", sf=-1.0, noise=1e-3, jitter=1e-10),
    "n256": dict(N=256, D=4, A=65, M=300, kind="matern12", sf=1.0, noise=1e-2, jitter=1e-6, normalize_y=False),
    # the blocked fit, a partial 128-tile, Np = 512
    "n257": dict(N=257, D=3, A=128, M=300, kind="rbf", sf=-1.0, noise=1e-3, jitter=1e-10, ard=True),
    "n300": dict(N=300, D=5, A=129, M=300, kind="matern52", sf=1.0, noise=1e-3, jitter=1e-10),
    "n300w": dict(N=300, D=6, A=256, M=8192, kind="matern52", sf=-1.0, noise=1e-2, jitter=1e-6, ard=True),
    # several chunks with TGP_CHUNK=8192, the last one partial; Np = 768; no 80-bit comparison (N > 300)
    "n600": dict(N=600, D=4, A=64, M=20000, kind="rbf", sf=1.0, noise=1e-3, jitter=1e-10),
    # an f32 handle: the sweep in f32, the rest in f64.  N = 600 because it has to be above 512: up to there the one-launch
    # sweep answers in f64 whatever the handle's dtype and an f32 handle would test nothing of its own
    "f32": dict(N=600, D=4, A=64, M=4096, kind="matern52", sf=1.0, noise=1e-3, jitter=1e-10, dtype="f32"),
}
HP_CASES = tuple(n for n, c in CASES.items() if c["N"] <= 300)
F64_CASES = tuple(n for n, c in CASES.items() if c.get("dtype", "f64") == "f64")

_cache = {}


def data(name):
    """X, y, length scale(s), Xa, Xc"""
    if ("data", name) not in _cache:
        c = CASES[name]
        N, D, A, M = c["N"], c["D"], c["A"], c["M"]
        rng = np.random.RandomState(7000 + 13 * N + A)
        X = rng.uniform(0, 1, (N, D))
        y = 1.5 + np.sin(3 * X.sum(1)) + 0.3 * X[:, 0] + 0.02 * rng.normal(size=N)
        ls = (rng.uniform(0.4, 0.9, D) if c.get("ard") else 0.6) * np.sqrt(D / 3.0)
        Xa = rng.uniform(0, 1, (A, D))
        Xc = rng.uniform(-0.05, 1.05, (M, D))
        if c.get("coincide"):
            Xa[4] = Xa[1]
            Xc[5] = X[0]
            Xc[7] = Xa[3]
        for a in (X, y, Xa, Xc):
            a.setflags(write=False)
        _cache[("data", name)] = (X, y, ls, Xa, Xc)
    return _cache[("data", name)]


def fit_args(name):
    c = CASES[name]
    X, y, ls, _, _ = data(name)
    return (X, y, c["kind"], C, ls, c["noise"], c["jitter"], c.get("normalize_y", True))


def model(name):
    """the f64 oracle model, made once"""
    if ("model", name) not in _cache:
        _cache[("model", name)] = G.fit(*fit_args(name))
    return _cache[("model", name)]


def scale(name):
    return kr.prior_scale(model(name))


def noise_vars(name):
    """(noise y_std^2, (noise + jitter) y_std^2) of the f64 model"""
    m = model(name)
    return m.noise * m.y_std ** 2, (m.noise + m.jitter) * m.y_std ** 2


def reference(name):
    """kg_reference.kg over the WHOLE batch: once per case, never modified"""
    if ("ref", name) not in _cache:
        _, _, _, Xa, Xc = data(name)
        r = kr.kg(model(name), Xa, Xc, CASES[name]["sf"])
        for a in r.values():
            a.setflags(write=False)
        _cache[("ref", name)] = r
    return _cache[("ref", name)]


def hp_rows(name):
    return min(CASES[name]["M"], HP_ROWS)


def hp_reference(name):
    """the 80-bit reference over the first hp_rows(name) candidates"""
    assert name in HP_CASES
    if ("hp", name) not in _cache:
        _, _, _, Xa, Xc = data(name)
        fit = hp.Fit(*fit_args(name))
        r = krh.kg(fit, Xa, Xc[:hp_rows(name)], CASES[name]["sf"])
        for a in r.values():
            a.setflags(write=False)
        _cache[("hp", name)] = r
    return _cache[("hp", name)]


def errors(name, got):
    """{"kg", "mu_a", "mu", "cov"}: a result's error against the 80-bit reference over its rows, as fractions of the
    scales; ``got`` holds arrays for any of those keys (rows beyond hp_rows are ignored)"""
    want, m, s = hp_reference(name), hp_rows(name), scale(name)
    out = {}
    for key in ("kg", "mu_a", "mu", "cov"):
        if got.get(key) is None:
            continue
        g = np.asarray(got[key]).astype(LD)
        g = g if key == "mu_a" else g[:m]
        out[key] = float(np.abs(g - want[key]).max()) / (s * s if key == "cov" else s)
    return out


def e_ref(name):
    """the f64 reference's own errors, as ``errors`` reports them"""
    if ("eref", name) not in _cache:
        _cache[("eref", name)] = errors(name, reference(name))
    return _cache[("eref", name)]


def bars_b(name):
    """{"kg", "mu_a", "mu", "cov"}: bar (b) as fractions of the scales"""
    e, N = e_ref(name), CASES[name]["N"]
    return {k: min(FACTOR * max(e[k], N * U), CAP_COV if k == "cov" else CAP_VAL) for k in e}


def judge_b(name, got):
    """dict(err, bar, ok): THE end-to-end comparison with the 80-bit reference"""
    err, bar = errors(name, got), bars_b(name)
    return dict(err=err, bar={k: bar[k] for k in err}, ok=all(err[k] <= bar[k] for k in err))


def judge_a(name, mu_a, mu, sigma, cov, kg_out):
    """dict(err, e_lines, bar, ok): bar (a), the envelope arithmetic alone on the call's OWN outputs (absolute, raw units)"""
    sf = CASES[name]["sf"]
    nv, ov = noise_vars(name)
    a, b, live = kr.lines_from_outputs(mu_a, mu, sigma, cov, nv, ov, sf)
    a, b = np.where(live[:, None], a, 0.0), np.where(live[:, None], b, 0.0)
    own = np.where(live, kr.envelope_kg(a, b), 0.0)
    e_lines = float(np.abs(own.astype(LD) - np.where(live, krh.envelope_kg(a, b), LD(0))).max())
    bar = FACTOR * max(e_lines, (CASES[name]["A"] + 1) * U * float(np.abs(a).max()))
    err = float(np.abs(np.asarray(kg_out) - own).max())
    return dict(err=err, e_lines=e_lines, bar=bar, ok=bool(err <= bar))


def argmax_conditions(name):
    """(best / scale, (best - second) / best) of the f64 reference over the whole batch; a one-row batch has gap inf"""
    v = reference(name)["kg"]
    order = np.argsort(-v, kind="stable")
    best = float(v[order[0]])
    gap = np.inf if len(v) < 2 else (best - float(v[order[1]])) / best
    return best / scale(name), gap
