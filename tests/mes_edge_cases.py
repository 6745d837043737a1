"""Max-value entropy search at its edges: the gamma grid, the rows, the classes, the bars and the judgement shared by
tests/test_mes_reference_hp.py (CPU: the reference and the bars judged), tests/test_gpu_mes_edges.py (the device's
arithmetic alone through tests/mes_math_driver.hip, then every library path) and tests/test_host_mes_edges.py (the host backend).

Reference: tests/mes_reference_hp.py (80-bit).  e_ref: the error of tests/mes_reference.py -- the f64 restatement of
csrc/mes_math.hpp -- against it on the grid, per quantity (h, dh) and per class of gamma:

    "below -50"      h's series                                   "(0, 8]"          the gamma > 0 forms
    "[-50, seam)"    erfcx for h, the continued fraction for dh    "(8, underflow)"  the same, exp(-gamma^2 / 2) small
    "[seam, 0]"      erfcx for both (seam = -10)

Errors are fractions of the row's own scale (mes_reference_hp.coefficients):  a: (1/S) sum h_s;  da/dmu: (1/(S sl)) sum |dh_s|;
da/dsigma: (sigma / (S v)) sum |gamma_s dh_s|.  With u = 2^-53:

    bar = min(FACTOR max(e_ref of the row's classes, u (1 + max_s gamma_s^2 over the positive gamma_s)), CAP)

FACTOR and CAP are tests/cov_edge_cases.py's (64, 1e-9).  u gamma^2 is the condition number of exp(-gamma^2 / 2) in gamma
times one rounding of gamma: derived, not measured (a gamma_s whose own h is below TINY, beyond ~36.3, does not count: its
term is invisible in the sum or the row is judged as tiny).  A row whose maxima fall in several classes takes the largest e_ref
among them.  CAP is a condition: where 10 max(e_ref, floor) exceeds it, bar() raises instead of returning.

Rows whose 80-bit scale is below TINY = 1e-290 (gamma beyond ~36.3: f64 is about to underflow) are judged for finiteness,
sign and 0 <= |got| <= 2 scale + the smallest subnormal.  Rows that are not live (sigma^2 - noise_var <= 0) must be
exactly 0 in all three quantities.
"""
import numpy as np

import cov_edge_cases as ec
import mes_reference as mr
import mes_reference_hp as hp

LD = hp.LD
U, FACTOR, CAP = ec.U, ec.FACTOR, ec.CAP_VAL
TINY = 1e-290
SUBNORMAL = 5e-324
SEAM_H, SEAM_DH = -50.0, mr.DH_SEAM
CLASSES = ("below -50", "[-50, seam)", "[seam, 0]", "(0, 8]", "(8, underflow)")
QUANTITIES = ("a", "dmu", "dsigma")
SLIPS = ("the 148/3 t^3 term dropped", "-7.5 written -7", "the h seam moved to -30", "the cancelling dh kept on [-50, seam)",
         "the gamma > 0 form used for gamma <= 0", "noise_var not subtracted", "sigma / sigma_f missing from da/dsigma",
         "the sum over S in place of the mean")
MES_MAXS = 64


def classify(g):
    """index into CLASSES, elementwise"""
    g = np.asarray(g)
    return np.where(g < SEAM_H, 0, np.where(g < SEAM_DH, 1, np.where(g <= 0, 2, np.where(g <= 8, 3, 4))))


def _ulps(x, n):
    out, lo, hi = [], x, x
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return out


def _last_before(which, threshold):
    """the largest f64 gamma at which the 80-bit |h| (which = 0) or |dh| (1) is still >= threshold, by bisection"""
    lo, hi = 30.0, 45.0
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if abs(hp.h_dh(np.array([mid]))[which][0]) >= LD(threshold):
            lo = mid
        else:
            hi = mid
    return lo


_grid = {}


def grid():
    """the gammas (f64, read-only): both tails to 1e300, both seams ulp by ulp, the underflow of h and dh"""
    if "g" not in _grid:
        parts = [-(10.0 ** np.linspace(300.0, 2.25, 60)), [-1e10, -1e4, -151.0],
                 np.linspace(-150.0, -50.0, 101), _ulps(SEAM_H, 10), [-49.4],
                 np.linspace(-50.0, SEAM_DH, 161), _ulps(SEAM_DH, 10),
                 np.linspace(SEAM_DH, 0.0, 201), [-0.0, 5e-324, 2.0 ** -1022, 1e-20],
                 np.linspace(0.0, 38.5, 155), _ulps(8.0, 2), [4.2426, 4.2427],
                 [_last_before(w, t) for w in (0, 1) for t in (TINY, 2.0 ** -1022, SUBNORMAL)],
                 [38.6, 39.0, 40.0, 1e10, 1e300]]
        g = np.concatenate([np.asarray(p, dtype=np.float64) for p in parts])
        g.setflags(write=False)
        _grid["g"] = g
    return _grid["g"]


# ---- the f64 restatement with one slip ------------------------------------------------------------------------------------
def f64_h_dh(gamma, slip=None):
    """tests/mes_reference.py's h_and_dh (slip None: the same bytes, asserted in tests/test_mes_reference_hp.py) with one of
    the slips in h or dh"""
    g = np.asarray(gamma, dtype=np.float64)
    if slip not in SLIPS[:5]:
        return mr.h_and_dh(g)
    h, dh = (a.copy() for a in mr.h_and_dh(g))
    with np.errstate(all="ignore"):
        t = 1.0 / (g * g)
        if slip == SLIPS[0]:
            tail = g < SEAM_H
            h[tail] = (np.log(-g) + mr.H_TAIL_CONST + t * (2.0 + t * -7.5))[tail]
        elif slip == SLIPS[1]:
            tail = g < SEAM_H
            h[tail] = (np.log(-g) + mr.H_TAIL_CONST + t * (2.0 + t * (-7.0 + t * (148.0 / 3.0))))[tail]
        elif slip == SLIPS[2]:
            tail = g < -30.0
            h[tail] = (np.log(-g) + mr.H_TAIL_CONST + t * (2.0 + t * (-7.5 + t * (148.0 / 3.0))))[tail]
        elif slip == SLIPS[3]:
            m = (g >= SEAM_H) & (g < SEAM_DH)
            r = mr.SQRT_2_OVER_PI / mr.erfcx(np.abs(g) * 0.70710678118654752440)
            dh[m] = (-0.5 * r * (1.0 + g * g + g * r))[m]
        else:
            m = (g >= SEAM_H) & (g <= 0.0)
            z = np.abs(g) * 0.70710678118654752440
            ez = np.exp(-z * z)
            q = 0.5 * mr.erfcx(z) * ez
            r = mr.INV_SQRT_2PI * ez / (1.0 - q)
            h[m] = (0.5 * g * r - np.log1p(-q))[m]
            dh[m] = np.where(r == 0.0, 0.0, -0.5 * r * (1.0 + g * g + g * r))[m]
    return h, dh


def f64_coefficients(mu, sigma, ystar, sf, noise_var, slip=None):
    """(a, da/dmu, da/dsigma) in f64 as tests/mes_reference.py's mes_coefficients forms them, for maxima per row
    ystar (M, S) and noise_var per row, with one of SLIPS (None: the honest computation)"""
    assert slip is None or slip in SLIPS
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    ys = np.asarray(ystar, dtype=np.float64)
    ys = np.broadcast_to(ys.reshape(1, -1), (mu.shape[0], ys.size)) if ys.ndim <= 1 else ys
    S = ys.shape[1]
    v = sigma * sigma - (0.0 if slip == SLIPS[5] else np.asarray(noise_var, dtype=np.float64))
    live = v > 0.0
    vs = np.where(live, v, 1.0)
    sl = np.sqrt(vs)
    sa, sdh, sgdh = np.zeros(mu.shape), np.zeros(mu.shape), np.zeros(mu.shape)
    with np.errstate(all="ignore"):
        for s in range(S):
            g = sf * (ys[:, s] - mu) / sl
            hv, dh = f64_h_dh(g, slip)
            sa, sdh, sgdh = sa + hv, sdh + dh, sgdh + g * dh
        n = 1.0 if slip == SLIPS[7] else float(S)
        a = sa / n
        cm = -sf * sdh / (sl * n)
        cs = -sgdh / (sl * n) if slip == SLIPS[6] else -sgdh * sigma / (vs * n)
    return np.where(live, a, 0.0), np.where(live, cm, 0.0), np.where(live, cs, 0.0)


# ---- e_ref and the bars -------------------------------------------------------------------------------------------------------
_eref = {}


def e_ref():
    """{"h" | "dh": [one figure per class]}: max over the grid of |f64 restatement - 80-bit| / |80-bit| where the 80-bit
    magnitude is at least TINY.  Computed here, never taken from the library."""
    if not _eref:
        g = grid()
        h64, d64 = mr.h_and_dh(g)
        h, dh = hp.h_dh(g)
        cls = classify(g)
        for name, got, want in (("h", h64, h), ("dh", d64, dh)):
            ok = np.abs(want) >= LD(TINY)
            rel = np.abs(got.astype(LD) - want) / np.where(ok, np.abs(want), LD(1))
            _eref[name] = [float(rel[ok & (cls == c)].max()) for c in range(len(CLASSES))]
    return _eref


def bar(quantity, classes, gpos2):
    """the bar of one row: classes a sequence of class indices present among its gamma_s, gpos2 the largest gamma_s^2
    over its positive gamma_s (0 if none)"""
    e = e_ref()["h" if quantity == "a" else "dh"]
    worst = max(max(e[c] for c in classes), U * (1.0 + gpos2))
    if 10.0 * worst > CAP:
        raise AssertionError("the cap is a condition: 10 x %.3g exceeds it (%s, classes %s, gamma^2 %.3g)" % (worst, quantity, list(classes), gpos2))
    return min(FACTOR * worst, CAP)


def judge(mu, sigma, ystar, sf, noise_var, a=None, dmu=None, dsigma=None):
    """every row of the given f64 results against the 80-bit reference fed the same f64 inputs.  Returns
    dict(ok, worst={quantity: largest err / bar}, by_class={quantity: {class: largest err / bar among the rows that have a
    gamma of the class}}, tiny, dead, rows={quantity: err / bar per row (nan where not judged by a bar)})"""
    (ra, rm, rs), scales, g = hp.coefficients(mu, sigma, ystar, sf, noise_var)
    _, _, live = hp.gammas(mu, sigma, ystar, sf, noise_var)
    cls = classify(g)
    M = g.shape[0]
    hs = hp.h_dh(g)[0]
    gpos2 = np.where((g > 0) & (hs >= LD(TINY)), g * g, LD(0)).max(1).astype(np.float64)       # (a term below TINY is no part of any bar)
    present = [sorted(set(cls[i].tolist())) for i in range(M)]
    out = dict(ok=True, worst={}, by_class={}, rows={}, tiny=0, dead=int((~live).sum()), bad=[])
    for q, got, want, sc in zip(QUANTITIES, (a, dmu, dsigma), (ra, rm, rs), scales):
        if got is None:
            continue
        got = np.asarray(got, dtype=np.float64).reshape(-1)
        ratio = np.full(M, np.nan)
        byc = {c: 0.0 for c in CLASSES}
        for i in range(M):
            if not np.isfinite(got[i]):
                out["ok"] = False
                out["bad"].append((q, i, "not finite"))
            elif not live[i]:
                if got[i] != 0.0:
                    out["ok"] = False
                    out["bad"].append((q, i, "a dead row is not 0"))
            elif sc[i] < LD(TINY):
                out["tiny"] += 1
                if not (abs(got[i]) <= 2 * float(sc[i]) + SUBNORMAL) or (q == "a" and got[i] < 0.0):
                    out["ok"] = False
                    out["bad"].append((q, i, "beyond twice a tiny reference"))
            else:
                b = bar(q, present[i], gpos2[i])
                ratio[i] = float(abs(LD(got[i]) - want[i]) / sc[i]) / b
                for c in present[i]:
                    byc[CLASSES[c]] = max(byc[CLASSES[c]], ratio[i])
                if not ratio[i] <= 1.0:
                    out["ok"] = False
                    out["bad"].append((q, i, "%.3g of its bar %.3g" % (ratio[i], b)))
        out["rows"][q] = ratio
        out["by_class"][q] = byc
        out["worst"][q] = float(np.nanmax(ratio)) if np.isfinite(ratio).any() else 0.0
    out["bad"] = out["bad"][:8]
    return out


def summary(j):
    """the part of a judgement that goes into a record"""
    return dict(worst={q: float(v) for q, v in j["worst"].items()}, tiny=int(j["tiny"]), dead=int(j["dead"]),
                by_class={q: {c: float(v) for c, v in d.items()} for q, d in j["by_class"].items()})


# ---- the rows of the arithmetic-alone tests ---------------------------------------------------------------------------------
_rows = {}


def _draw(rng, c):
    if c == 0:
        return -(10.0 ** rng.uniform(1.7, 6.0))
    if c == 1:
        return rng.uniform(SEAM_H, SEAM_DH)
    if c == 2:
        return rng.uniform(SEAM_DH, 0.0)
    if c == 3:
        return rng.uniform(0.0, 8.0)
    return rng.uniform(8.0, 37.0)


def rows():
    """dict(g0, mu, sigma, noise_var, sf (R,), S (R,) int, ys (R, MES_MAXS), kind (R,) of "grid" | "drawn" | "dead" | "ulp"),
    read-only.  grid: the gamma grid with S = 1 at mu = 0, sigma = 1, noise_var = 0, where gamma = sf y* exactly, both sf.
    drawn: 256 rows of S = 5 and 256 of S = 64, sf alternating; every third row's gamma_s all in one class, the others
    across all five; sigma^2 >= 2 noise_var.  dead / ulp: sigma^2 - noise_var exactly 0, negative, one ulp above 0."""
    if _rows:
        return _rows
    g = grid()
    R = []
    for sf in (1.0, -1.0):
        for x in g:
            R.append((x, 0.0, 1.0, 0.0, sf, 1, [sf * x], "grid"))
    rng = np.random.RandomState(20250)
    for S in (5, 64):
        for i in range(256):
            sf = 1.0 if i % 2 == 0 else -1.0
            cl = [(i // 3) % 5] * S if i % 3 == 0 else rng.randint(0, 5, S)
            gam = np.array([_draw(rng, c) for c in cl])
            mu, sigma = 3.0 * rng.normal(), rng.uniform(0.5, 2.0)
            nv = rng.uniform(0.0, 0.5) * sigma * sigma
            ys = mu + sf * gam * np.sqrt(sigma * sigma - nv)
            R.append((gam[0], mu, sigma, nv, sf, S, ys, "drawn"))
    for sf in (1.0, -1.0):
        ys = [0.5, 1.0, 2.0, -1.0, 0.0]
        R.append((0.0, 0.25, 1.0, 1.0, sf, 5, ys, "dead"))                       # exactly 0
        R.append((0.0, 0.25, 3.0, 9.0, sf, 5, ys, "dead"))
        R.append((0.0, 0.25, 1.0, 1.5, sf, 5, ys, "dead"))                       # negative
        R.append((0.0, 0.25, 0.0, 0.0, sf, 5, ys, "dead"))
        R.append((0.0, 0.25, 1.0, float(np.nextafter(1.0, 0.0)), sf, 5, ys, "ulp"))      # 2^-53: sl = 2^-26.5, |gamma| ~ 1e8
    n = len(R)
    ysm = np.zeros((n, MES_MAXS))
    for i, r in enumerate(R):
        ysm[i, :r[5]] = r[6]
    out = dict(g0=np.array([r[0] for r in R]), mu=np.array([r[1] for r in R]), sigma=np.array([r[2] for r in R]),
               noise_var=np.array([r[3] for r in R]), sf=np.array([r[4] for r in R]), S=np.array([r[5] for r in R], dtype=np.int64),
               ys=ysm, kind=np.array([r[7] for r in R]))
    # the drawn rows' first gamma as the device will form it from the f64 inputs
    d = out["kind"] == "drawn"
    out["g0"][d] = (out["sf"][d] * (ysm[d, 0] - out["mu"][d]) / np.sqrt(out["sigma"][d] ** 2 - out["noise_var"][d]))
    for v in out.values():
        v.setflags(write=False)
    _rows.update(out)
    return _rows


def row_groups():
    """[(label, row indices)] with one (S, sf) per group: what one call of judge() takes"""
    r = rows()
    groups = []
    for S in sorted(set(r["S"].tolist())):
        for sf in (1.0, -1.0):
            I = np.nonzero((r["S"] == S) & (r["sf"] == sf))[0]
            if I.size:
                groups.append(("S=%d sf=%+d" % (S, sf), I))
    return groups


def judge_rows(I, a=None, dmu=None, dsigma=None):
    r = rows()
    S, sf = int(r["S"][I[0]]), float(r["sf"][I[0]])
    return judge(r["mu"][I], r["sigma"][I], r["ys"][I][:, :S], sf, r["noise_var"][I], a, dmu, dsigma)


# ---- the library's paths at placed gammas -------------------------------------------------------------------------------------
KINDS = ("rbf", "matern12", "matern32", "matern52")
D_LIB = 3
NOISE_LIB = 1e-6
# N, M: the one-workgroup sweep, the one-launch sweep, the general sweep (M = 1500 with TGP_CHUNK = 1024: a partial last chunk)
PATHS = {"one-workgroup": (40, 300), "one-launch": (200, 300), "general": (257, 1500)}
MARK = 7                                    # the marked candidate
# the marked candidate's 64 gamma_s: every class, both seams approached from both sides
MARK_GAMMAS = np.concatenate([[-1e4, -300.0, -80.0, -60.0, -51.0, -50.001], [-49.999, -49.4], np.linspace(-45.0, -11.0, 8),
                              [-10.001, -9.999], np.linspace(-9.0, -0.25, 12), [0.0], np.linspace(0.25, 8.0, 14),
                              np.linspace(8.5, 36.0, 19)])
assert MARK_GAMMAS.shape == (MES_MAXS,) and sorted(set(classify(MARK_GAMMAS).tolist())) == [0, 1, 2, 3, 4]
SINGLE_GAMMAS = (-49.4, -9.999999, 3.0, 20.0)   # S = 1: where the cancelling dh was worst, just above the new seam, the positive classes alone


def library_problem(N, M, seed=0):
    """(X, y, length scale, candidates): a length scale short enough that every candidate keeps sigma^2 >= 2 noise_var, so
    that the conditioning of sigma^2 - noise_var stays out of the bars (asserted where the rows are judged)"""
    rng = np.random.RandomState(1000 + N + seed)
    X = rng.uniform(0, 1, (N, D_LIB))
    y = 3.0 + 2.0 * np.sin(3 * X @ np.array([0.8, -0.5, 0.3])) + 0.5 * ((X - 0.5) ** 2).sum(1)
    Xc = rng.uniform(0, 1, (M, D_LIB))
    return X, y, 0.2, Xc


def placed_maxima(mu_j, sigma_j, noise_var, sf, gammas):
    """y*_s = mu_j + sf gamma_s sl_j, so that the marked candidate's gamma_s are the given ones to a rounding of y*"""
    sl = np.sqrt(sigma_j * sigma_j - noise_var)
    return mu_j + sf * np.asarray(gammas, dtype=np.float64) * sl


def well_conditioned(sigma, noise_var):
    return bool(np.all(np.asarray(sigma) ** 2 >= 2.0 * noise_var))
