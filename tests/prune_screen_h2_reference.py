"""NumPy model of the fp16 screen (turbo_amd/csrc/prune_screen_h2.hpp; DESIGN.md section 4, "the fp16 screen's error
term"): the sign partition, the two fp16 planes per operand under the per-candidate / training-set scales, the hi and mid
accumulations under several summation orders and roundings of the matrix core's products and partial sums, the epilogue,
the sign-partitioned f64 sums and the error term E = min(closed, weighted).  The exact path, the adversarial inputs and the
f32 screen's E come from prune_screen_reference.py, unchanged.  Not a test module itself."""
import numpy as np

import prune_screen_reference as ref

U = ref.U
KAPPA = ref.KAPPA
MIN_D = 15               # SCRH_MIN_D: the dispatcher runs the fp16 screen from here on, the f32 screen below
MAXEXP = 40


def error_terms(constant, D, N):
    """screen_h2_error_terms() of prune_screen_h2.hpp, restated"""
    ce, L = 1.001 * constant, abs(np.log2(constant))
    dcoef = 2.01 * D + 25.0 + 0.26 * np.sqrt(float(D))
    P = ce * U * 0.5 * dcoef
    Qc = ref.error_terms(constant, D, N)[1] + ce * (0.7 * L * U + 2.0 ** -41)
    Qw = Qc + ce * U * (2.4 + 1.4 * L)
    return dcoef, P, Qc, Qw


def scale(m):
    """screen_h2_scale(): the power of two that puts m > 0 into [2^13, 2^14), exponent within +-MAXEXP; 1 for m = 0"""
    m = np.asarray(m, dtype=np.float32)
    e = np.frexp(np.where(m > 0, m, np.float32(1)))[1]
    return np.where(m > 0, np.ldexp(np.float32(1), np.clip(14 - e, -MAXEXP, MAXEXP)), np.float32(1)).astype(np.float32)


def split2(v):
    """float32 (already scaled) -> the two fp16 planes as float64: v ~ v1 + 2^-11 v2 (split2_f16x2)"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h1 = v.astype(np.float16)
        r = ((v - h1.astype(np.float32)) * np.float32(2048.0)).astype(np.float32)
        h2 = r.astype(np.float16)
    return h1.astype(np.float64), h2.astype(np.float64)


def sq_norms64(A):
    """|row|^2 as an f64 fma chain in dimension order (the square of an f32 is exact in f64: one rounding per step)"""
    s = np.zeros(A.shape[0], dtype=np.float64)
    for d in range(A.shape[1]):
        s = A[:, d].astype(np.float64) * A[:, d].astype(np.float64) + s
    return s


def partition(alpha):
    """order of the training points in the screen's copy: alpha >= 0 first, padded to a multiple of 128 (-1), then
    alpha < 0, padded -> (index array with -1 for padding rows, number of positive tiles)"""
    pos, neg = np.flatnonzero(alpha >= 0), np.flatnonzero(~(alpha >= 0))
    pad = lambda a: np.concatenate([a, np.full(-len(a) % 128, -1, dtype=np.int64)])
    return np.concatenate([pad(pos), pad(neg)]).astype(np.int64), (len(pos) + 127) // 128


def _accumulate(prods, order, rnd):
    add = lambda a, b: rnd(a.astype(np.float64) + b.astype(np.float64))
    prods = [p.astype(np.float32) for p in prods]      # (an fp16 x fp16 product has 22 bits: exact in f32 under any rounding)
    if order == "reversed":
        prods = prods[::-1]
    if order in ("sequential", "reversed"):
        acc = prods[0]
        for p in prods[1:]:
            acc = add(acc, p)
        return acc
    if order == "pairwise":
        while len(prods) > 1:
            nxt = [add(prods[i], prods[i + 1]) for i in range(0, len(prods) - 1, 2)]
            if len(prods) & 1:
                nxt.append(prods[-1])
            prods = nxt
        return prods[0]
    assert order == "chunks2"
    acc = None
    for i in range(0, len(prods), 2):
        t = add(prods[i], prods[i + 1]) if i + 1 < len(prods) else prods[i]
        acc = t if acc is None else add(acc, t)
    return acc


def range_ok(Cs, Xs):
    """(the training points pass, per-candidate pass): prune_screen_h2.hpp's range conditions"""
    with np.errstate(over="ignore", invalid="ignore"):
        nx, nc = sq_norms64(Xs), sq_norms64(Cs)
        xok = bool(np.all(nx < np.inf)) and bool(2.0 * np.abs(Xs).max() < 2.0 ** 54)
        nxmax = float(nx.astype(np.float32).max()) if xok else np.inf
        return xok, xok & (nc + nxmax < 2.0 ** 46)


def screen_mean(Cs, Xs, alpha, constant, order="sequential", trunc=False, bump=0):
    """(mu_s, W) as screen_h2_prep_kernel and prune_screen_h2_kernel form them; `order` / `trunc` model the matrix core's
    undocumented inside (its fp16 products are exact in f32 anyway)"""
    rnd = ref.rz32 if trunc else ref.rn32
    M, D = Cs.shape
    perm, ntp = partition(alpha)
    live = perm >= 0
    Xp = np.zeros((len(perm), D), dtype=np.float32)
    Xp[live] = Xs[perm[live]]
    ap = np.zeros(len(perm), dtype=np.float32)
    ap[live] = ref.rn32(np.abs(alpha[perm[live]]))
    nx = sq_norms64(Xp).astype(np.float32)
    nc = sq_norms64(Cs)
    sx = scale(np.float32(2.0) * np.abs(Xs).max())
    sr = scale(np.abs(Cs).max(axis=1))
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        b1, b2 = split2((np.float32(-2.0) * Xp) * sx)
        a1, a2 = split2(Cs * sr[:, None])
        hi = _accumulate([a1[:, None, d] * b1[None, :, d] for d in range(D)], order, rnd)
        mid = _accumulate([p for d in range(D) for p in (a1[:, None, d] * b2[None, :, d], a2[:, None, d] * b1[None, :, d])],
                          order, rnd)
        S = (sr * sx).astype(np.float32)[:, None]
        kS = (KAPPA / S).astype(np.float32)
        log2c = np.float64(np.float32(np.log2(np.float32(constant))))
        Lr = ref.rn32(log2c + np.float64(KAPPA) * nc)[:, None]
        clamp = -ref.rn32(S[:, 0].astype(np.float64) * nc)[:, None]
        t = ref.fma32(mid, np.broadcast_to(np.float32(2.0 ** -11), mid.shape), hi)
        s = np.maximum(ref.fma32(np.broadcast_to(nx[None, :], t.shape), np.broadcast_to(S, t.shape), t), clamp)
        arg = ref.fma32(s, np.broadcast_to(kS, s.shape), np.broadcast_to(Lr, s.shape))
        k = ref.rn32(np.exp2(arg.astype(np.float64)))
        if bump:
            k = np.maximum(np.nextafter(k, np.float32(np.inf if bump > 0 else -np.inf)), np.float32(0))      # (v_exp_f32 returns no negative)
        nt = len(perm) // 128
        kt = k.reshape(M, nt, 4, 32)
        at = np.broadcast_to(ap.reshape(1, nt, 4, 32), kt.shape)
        p = ref.rn32(kt[:, :, 0].astype(np.float64) * at[:, :, 0].astype(np.float64))
        for b in range(1, 4):
            p = ref.fma32(kt[:, :, b], at[:, :, b], p)
        p = p.astype(np.float64)
        mp, mn = p[:, :ntp].sum(axis=(1, 2)), p[:, ntp:].sum(axis=(1, 2))
    return mp - mn, mp + mn


def error_bound(Cs, Xs, alpha, constant, D, W):
    """(E, closed) of the fp16 screen for every row of Cs, W = sum k_s |alpha| as the kernel (or the model) formed it;
    +inf where the range conditions fail"""
    dcoef, P, Qc, Qw = error_terms(constant, D, Xs.shape[0])
    xok, cok = range_ok(Cs, Xs)
    if not xok:
        return np.full(Cs.shape[0], np.inf), np.full(Cs.shape[0], np.inf)
    an = 1.001 * np.abs(alpha).sum()
    nc = sq_norms64(Cs)
    nxmax = float(sq_norms64(Xs).astype(np.float32).max())
    with np.errstate(over="ignore", invalid="ignore"):
        closed = np.where(cok, an * (P * nxmax + Qc) + (an * P) * nc, np.inf)
        delta = dcoef * U * (nc + nxmax) + 2.0 ** -40
        wcoef = np.where(cok & (delta <= 1.0), 1.001 * np.expm1(0.5001 * np.minimum(delta, 1.0)), np.inf)
        return np.fmin(closed, wcoef * W + an * Qw), closed


def dispatched_error(Cs, Xs, alpha, constant, D, W):
    """E of the screen the dispatcher runs by default (TGP_SCREEN_ARITH=h2): the fp16 screen's from MIN_D on, else the f32
    screen's"""
    if D >= MIN_D:
        return error_bound(Cs, Xs, alpha, constant, D, W)[0]
    return ref.error_bound(Cs, Xs, alpha, constant, D)


def extra_cases():
    """name -> (Cs, Xs, alpha, constant, D) beyond adversarial_case: one-signed alpha, a positive count of exactly 128,
    N = 1 / 127 / 129, and inputs that fail the range conditions (a training coordinate of 1e17; candidates at 1e8)"""
    out = {}
    D = 32
    Cs, Xs, alpha, c = ref.adversarial_case(D, "iso_c1", M=128)
    out["all_positive"] = (Cs, Xs, np.abs(alpha), c, D)
    out["all_negative"] = (Cs, Xs, -np.abs(alpha), c, D)
    a = -np.abs(alpha)
    a[np.random.RandomState(5).permutation(len(a))[:128]] *= -1.0
    out["positives_128"] = (Cs, Xs, a, c, D)
    for N in (1, 127, 128, 129):
        Cs, Xs, alpha, c = ref.adversarial_case(D, "iso_c50", N=N, M=128)
        out["N%d" % N] = (Cs, Xs, alpha, c, D)
    Cs, Xs, alpha, c = ref.adversarial_case(D, "iso_c1", M=128)
    Xbig = Xs.copy()
    Xbig[3, 1] = np.float32(1e17)
    out["x_out_of_range"] = (Cs, Xbig, alpha, c, D)
    Cbig = Cs.copy()
    Cbig[::5] = np.float32(1e8)
    out["c_out_of_range"] = (Cbig, Xs, alpha, c, D)
    return out
