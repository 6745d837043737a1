"""The models, batches, bar and conditions of the knowledge gradient's GRADIENT tests -- TEST INFRASTRUCTURE shared by
tests/test_kg_grad_reference.py (CPU: the closed form against central differences, the references against each other, the
case conditions, the proof that the bar rejects the slips it is there for) and tests/test_gpu_kg_grad.py (the kernels).

Models and points follow tests/kg_cases.py's recipe (its cases are taken as they are; the ones added here are drawn the same
way).  A case's batch is the leading 48 rows of its candidates unless said otherwise:
  n1      N = 1, A = 1, one row: grad mu == 0, the tie rule is moot
  n40     noise 0, WITHOUT its coincident rows 5 (on a training point) and 7 (on a discretisation point): there the reference
          itself is good to 2e-6 only; tests/test_gpu_kg_grad.py judges them apart
  n129, n256, n300, n300w as tests/kg_cases.py has them
  n257p   kg_cases' n257 with sf = +1 (with -1 its leading rows are flat to 1e-43 and judge nothing)
  a1      N = 130, D = 2, A = 1
  d33     N = 200, D = 33, A = 17, ARD Matern-3/2
  n600m   kg_cases' N = 600 Matern-5/2 model (its "f32" case; on its RBF "n600" model KG is flat to 5e-6 of the gradient's
          scale and the reference's own error alone is over the cap) on an f64 handle: the leading 48 rows and rows
          4080 .. 4095 of the 4096-row batch;  f32: the same model and leading rows on an f32 handle
  kink    N = 150, D = 3, A = 24, sf = +1 and Xa the training inputs with the WORST y: the candidate's own line is the strict
          maximum intercept on about half the rows, so both sides of the indicator are judged

Bar (u = 2^-53), as the acquisition-gradient edge tests: the error is a fraction of the batch's 80-bit maximum of |gradient|
over the judged rows and bar = min(64 max(e_ref, N u), 1e-9), e_ref the f64 reference's own error against the 80-bit one for
that case, computed here, never from the code under test.

The starts of the L-BFGS-B comparison (LBFGSB_STARTS, tgp_kg_lbfgsb against SciPy driving tgp_kg_grad, points 1e-9 and values
1e-12 of max(1, |value|)): two correct implementations of one optimiser differ by a rounding error at every evaluation, and a
walk may amplify it -- the maximiser of KG tends to sit on the kink a_A = max a_i, where L-BFGS-B walks long.  So a start can
judge only if the walk from it is well conditioned, and that is measured on the f64 REFERENCE with SciPy alone
(``walk_sensitivity``): the start is moved by ONE ulp in its first coordinate and the two ends are compared.  A start is
taken when the ends differ by at most 1 / 10 of the tolerance (1e-10, 1e-13): the ulp at the start is ONE rounding error
put through the walk's amplification, two implementations make one at each of the ~100 evaluations of a walk, and
independent errors add up to about sqrt(100) = 10 of them.  The starts are the first three judged rows, by the reference's KG (what
start_from_best hands the stage), that meet it.  n300 passes over rows 42 (152 evaluations: SciPy's own two ends 2.6e-8 and
1.3e-9 apart), 39 (7e-12, 4e-13) and 34 (3e-11, 1e-12); tests/test_kg_grad_reference.py holds the table to the rule.
"""
import numpy as np

import cov_reference_hp as hp
import kg_cases as kc
import kg_grad_reference as gr
import kg_grad_reference_hp as grh
import kg_reference as kr
from oracle import gp_oracle as G

LD = np.longdouble
U = 2.0 ** -53
FACTOR, CAP = 64.0, 1e-9
MIN_GRAD = 1e-6              # max |grad KG| of a case, of prior scale / smallest length scale
MIN_KINK = 1e-4              # |a_A - max_{i<A} a_i| of every judged row, of the prior scale
MIN_SIDE = 8                 # rows on either side of the indicator in at least one case
CD_STEP, CD_BAR = 1e-7, 1e-8

BASE = 48
OWN = {
    "a1": dict(N=130, D=2, A=1, M=64, kind="matern52", sf=-1.0, noise=1e-3, jitter=1e-10),
    "d33": dict(N=200, D=33, A=17, M=64, kind="matern32", sf=1.0, noise=1e-3, jitter=1e-10, ard=True),
    "kink": dict(N=150, D=3, A=24, M=64, kind="matern52", sf=1.0, noise=1e-3, jitter=1e-10, worst_points=True),
}
CASES = {
    "n1": dict(kc.CASES["n1"]),
    "n40": dict(kc.CASES["n40"], skip=(5, 7)),
    "n129": dict(kc.CASES["n129"]),
    "n256": dict(kc.CASES["n256"]),
    "n257p": dict(kc.CASES["n257"], sf=1.0, of="n257"),
    "n300": dict(kc.CASES["n300"]),
    "n300w": dict(kc.CASES["n300w"]),
    "a1": OWN["a1"], "d33": OWN["d33"], "kink": OWN["kink"],
    "n600m": dict(kc.CASES["f32"], dtype="f64", of="f32", tail=(4096, 16)),
    "f32": dict(kc.CASES["f32"]),
}
HP_CASES = tuple(CASES)
LBFGSB_TOL = (1e-9, 1e-12)                       # points; values, of max(1, |value|): tests/test_gpu_parity.py's
LBFGSB_STARTS = {"n40": (3, 37, 32), "n300": (26, 22, 30)}      # indices into the judged rows
LBFGSB_PASSED_OVER = {"n40": (), "n300": (42, 39, 34)}         # ranked higher, not well conditioned
_cache = {}


def data(name):
    """X, y, length scale(s), Xa, Xc"""
    c = CASES[name]
    if name not in OWN:
        return kc.data(c.get("of", name))
    if ("data", name) not in _cache:
        N, D, A, M = c["N"], c["D"], c["A"], c["M"]
        rng = np.random.RandomState(7000 + 13 * N + A)
        X = rng.uniform(0, 1, (N, D))
        y = 1.5 + np.sin(3 * X.sum(1)) + 0.3 * X[:, 0] + 0.02 * rng.normal(size=N)
        ls = (rng.uniform(0.4, 0.9, D) if c.get("ard") else 0.6) * np.sqrt(D / 3.0)
        Xa = rng.uniform(0, 1, (A, D))
        Xc = rng.uniform(-0.05, 1.05, (M, D))
        if c.get("worst_points"):
            Xa = np.ascontiguousarray(X[np.argsort(c["sf"] * y, kind="stable")[:A]])
        for a in (X, y, Xa, Xc):
            a.setflags(write=False)
        _cache[("data", name)] = (X, y, ls, Xa, Xc)
    return _cache[("data", name)]


def fit_args(name):
    c = CASES[name]
    X, y, ls, _, _ = data(name)
    return (X, y, c["kind"], kc.C, ls, c["noise"], c["jitter"], c.get("normalize_y", True))


def rows(name):
    """the judged rows of the case's candidates"""
    c = CASES[name]
    r = [i for i in range(min(BASE, c["M"])) if i not in c.get("skip", ())]
    if "tail" in c:
        m, t = c["tail"]
        r += list(range(m - t, m))
    return np.array(r)


def points(name):
    """(Xa, the judged query points)"""
    _, _, _, Xa, Xc = data(name)
    return Xa, Xc[rows(name)]


def model(name):
    if ("model", name) not in _cache:
        _cache[("model", name)] = G.fit(*fit_args(name))
    return _cache[("model", name)]


def scale(name):
    return kr.prior_scale(model(name))


def grad_scale(name):
    """prior scale / smallest length scale: what the size of a case's gradient is compared with"""
    return scale(name) / float(np.min(data(name)[2]))


def reference(name):
    """kg_grad_reference.kg_grad over the judged rows: once per case, never modified"""
    if ("ref", name) not in _cache:
        Xa, Xq = points(name)
        _cache[("ref", name)] = _frozen(gr.kg_grad(model(name), Xa, Xq, CASES[name]["sf"]))
    return _cache[("ref", name)]


def hp_fit(name):
    if ("fit", name) not in _cache:
        _cache[("fit", name)] = hp.Fit(*fit_args(name))
    return _cache[("fit", name)]


def hp_reference(name):
    """the 80-bit closed form over the judged rows"""
    if ("hp", name) not in _cache:
        Xa, Xq = points(name)
        _cache[("hp", name)] = _frozen(grh.kg_grad(hp_fit(name), Xa, Xq, CASES[name]["sf"]))
    return _cache[("hp", name)]


def _frozen(r):
    for a in r.values():
        a.setflags(write=False)
    return r


def error(name, grad):
    """a gradient's error over the judged rows (``grad``: those rows, in order) against the 80-bit closed form, as a fraction
    of the batch's 80-bit maximum of |gradient|"""
    want = hp_reference(name)["grad"]
    return float(np.abs(np.asarray(grad).astype(LD) - want).max() / np.abs(want).max())


def e_ref(name):
    if ("eref", name) not in _cache:
        _cache[("eref", name)] = error(name, reference(name)["grad"])
    return _cache[("eref", name)]


def bar(name):
    return min(FACTOR * max(e_ref(name), CASES[name]["N"] * U), CAP)


def judge(name, grad):
    """dict(err, bar, ok): THE comparison with the 80-bit closed form"""
    err, b = error(name, grad), bar(name)
    return dict(err=err, bar=b, ok=bool(err <= b))


def conditions(name):
    """dict(e_ref, max_grad (of grad_scale), min_kink (of the prior scale), strict, not_strict (rows), n_env (min, max))"""
    r = hp_reference(name)
    return dict(e_ref=e_ref(name), max_grad=float(np.abs(r["grad"]).max()) / grad_scale(name),
                min_kink=float(r["kink"].min()) / scale(name), strict=int(r["strict"].sum()),
                not_strict=int((~r["strict"]).sum()), n_env=(int(r["n_env"].min()), int(r["n_env"].max())))


def ranked_rows(name):
    """the judged rows by the f64 reference's KG, the best first"""
    return np.argsort(-reference(name)["kg"], kind="stable")


def walk_sensitivity(name, i):
    """(points, values): how far the end of SciPy's L-BFGS-B walk on the f64 REFERENCE, in the unit box from judged row i,
    moves when the start's first coordinate moves by one ulp"""
    import scipy.optimize
    om, (Xa, Xq), sf = model(name), points(name), CASES[name]["sf"]
    D = Xq.shape[1]

    def neg_f(p):
        r = gr.kg_grad(om, Xa, p.reshape(1, -1), sf)
        return -float(r["kg"][0]), -r["grad"][0]
    x0 = np.clip(Xq[i], 0.0, 1.0)
    x1 = x0.copy()
    x1[0] = np.nextafter(x1[0], 0.5)
    a, b = (scipy.optimize.minimize(neg_f, x, jac=True, bounds=[(0.0, 1.0)] * D, method="L-BFGS-B", options=dict(maxiter=15000))
            for x in (x0, x1))
    return float(np.abs(a.x - b.x).max()), abs(float(a.fun) - float(b.fun)) / max(1.0, abs(float(a.fun)))


def well_conditioned(sens):
    return sens[0] <= LBFGSB_TOL[0] / 10 and sens[1] <= LBFGSB_TOL[1] / 10
