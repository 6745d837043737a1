"""NumPy model of the pruned sweep's screen (turbo_amd/csrc/prune_screen.hpp; DESIGN.md section 4, "the screen's error
term"): the f32 expansion  s = max(0, (|c|^2 + |x|^2) + (-2 c.x))  under several summation orders and roundings of the
matrix core's products and partial sums, the kernel's epilogue, the exact path's mean (direct-difference f32 distances, the
same exp2 sequence, an f64 sum) and the proved error term E(c).  Also the adversarial inputs the CPU test and the GPU
driver test share.  Not a test module itself."""
import numpy as np

U = 2.0 ** -24
KAPPA = np.float32(-0.72134752044448170368)
ORDERS = ("sequential", "reversed", "pairwise", "chunks2")


def rz32(x):
    """float64 -> float32 rounded toward zero"""
    x = np.asarray(x, dtype=np.float64)
    y = x.astype(np.float32)
    up = np.abs(y.astype(np.float64)) > np.abs(x)
    return np.where(up, np.nextafter(y, np.float32(0)), y).astype(np.float32)


def rn32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def fma32(a, b, c):
    """fmaf: a, b, c float32; the product is exact in float64, one rounding of the sum to float32 (the float64 rounding
    in between moves the result by at most 2^-53 relative, far inside every term of E)"""
    return rn32(a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64))


def error_terms(constant, D, N):
    """screen_error_terms() of prune_screen.hpp, restated"""
    ce = 1.001 * constant
    P = ce * U * (1.5 * D + 6.0)
    Q = ce * (U * (0.5 * (D + 3) + 1.4 * abs(np.log2(constant)) + 11.2) + 8.0 * (N + 8) * 2.0 ** -53) + 2.0 ** -120
    return P, Q


def sq_norms(A):
    """|row|^2 as the kernels form it: one fma chain per row in dimension order"""
    s = np.zeros(A.shape[0], dtype=np.float32)
    for d in range(A.shape[1]):
        s = fma32(A[:, d], A[:, d], s)
    return s


def error_bound(Cs, Xs, alpha, constant, D):
    """E(c) for every row of Cs, as screen_stats_kernel and prune_screen_kernel form it"""
    P, Q = error_terms(constant, D, Xs.shape[0])
    an = 1.001 * np.abs(alpha).sum()
    mx = float(sq_norms(Xs).max())
    return an * (P * mx + Q) + (an * P) * sq_norms(Cs).astype(np.float64)


def dot_m2(Cs, Xs, order, rnd):
    """sum_d c_d * (-2 x_d) with every product and every partial sum rounded by rnd, in the given order -> (M, N) float32"""
    M, D = Cs.shape
    prods = [rnd(Cs[:, None, d].astype(np.float64) * (-2.0 * Xs[None, :, d].astype(np.float64))) for d in range(D)]
    add = lambda a, b: rnd(a.astype(np.float64) + b.astype(np.float64))
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
    assert order == "chunks2"          # one k = 2 step after the other: acc + (p0 + p1)
    acc = None
    for i in range(0, len(prods), 2):
        t = add(prods[i], prods[i + 1]) if i + 1 < len(prods) else prods[i]
        acc = t if acc is None else add(acc, t)
    return acc


def kernel_value(d2, constant, bump=0):
    """exp2(fma(d2, -log2(e) / 2, log2(constant))) in float32; bump = +-1 moves the result one ulp up / down (v_exp_f32 is
    good to one ulp, and which way it errs is not documented)"""
    log2c = np.float32(np.log2(np.float32(constant)))
    arg = fma32(d2, np.broadcast_to(KAPPA, d2.shape), np.broadcast_to(log2c, d2.shape))
    k = rn32(np.exp2(arg.astype(np.float64)))
    if bump:
        k = np.nextafter(k, np.float32(np.inf if bump > 0 else -np.inf))
    return k


def exact_mean(Cs, Xs, alpha, constant, bump=0):
    """the exact path: direct differences summed in dimension order, f64 sum of k * alpha"""
    d2 = np.zeros((Cs.shape[0], Xs.shape[0]), dtype=np.float32)
    for d in range(Cs.shape[1]):
        df = rn32(Cs[:, None, d].astype(np.float64) - Xs[None, :, d].astype(np.float64))
        d2 = fma32(df, df, d2)
    k = kernel_value(d2, constant, bump)
    return (k.astype(np.float64) * alpha[None, :]).sum(1)


def screen_mean(Cs, Xs, alpha, constant, order="sequential", trunc=False, bump=0):
    """mu_s as prune_screen_kernel forms it; `order` / `trunc` model the matrix core's undocumented inside"""
    M, N = Cs.shape[0], Xs.shape[0]
    nc, nx = sq_norms(Cs), sq_norms(Xs)
    acc = dot_m2(Cs, Xs, order, rz32 if trunc else rn32)
    t = rn32(nc[:, None].astype(np.float64) + nx[None, :].astype(np.float64))
    s = np.maximum(np.float32(0), rn32(t.astype(np.float64) + acc.astype(np.float64)))
    k = kernel_value(s, constant, bump)
    # the epilogue: tiles of 128 training points; a lane holds columns l, l + 32, l + 64, l + 96 of a tile and sums their
    # four k * alpha in f32 (a product, then three fmas), then one f64 add per tile
    Np = -(-N // 128) * 128
    kp = np.zeros((M, Np), dtype=np.float32)
    kp[:, :N] = k
    ap = np.zeros(Np, dtype=np.float32)
    ap[:N] = rn32(alpha)
    kt, at = kp.reshape(M, Np // 128, 4, 32), np.broadcast_to(ap.reshape(1, Np // 128, 4, 32), (M, Np // 128, 4, 32))
    p = rn32(kt[:, :, 0].astype(np.float64) * at[:, :, 0].astype(np.float64))
    for b in range(1, 4):
        p = fma32(kt[:, :, b], at[:, :, b], p)
    return p.astype(np.float64).sum(axis=(1, 2))


CONFIGS = ("iso_c1", "ard100_c50", "underflow_c1", "iso_c50")


def adversarial_case(D, config, N=300, M=512, seed=0):
    """(Cs, Xs, alpha, constant): SCALED float32 inputs (what prep_candidates_kernel leaves) and an alpha of mixed signs
    with |alpha|_1 about 1e4.  Every 7th candidate equals a training point (d^2 = 0: the expansion cancels); every 11th
    lies ten times further out than the unit cube."""
    rng = np.random.RandomState(1000 * D + 17 * CONFIGS.index(config) + seed)
    X = rng.uniform(0, 1, size=(N, D))
    Xc = rng.uniform(0, 1, size=(M, D))
    Xc[::11] *= 10.0
    Xc[::7] = X[rng.randint(0, N, size=len(Xc[::7]))]
    if config == "ard100_c50":
        ls = np.sqrt(D / 6.0) * np.logspace(-1, 1, D) if D > 1 else np.array([0.1])
        constant = 50.0
    elif config == "underflow_c1":
        ls = np.full(D, 2e-2 / np.sqrt(D))       # d^2 of the order of 1e3 .. 1e6: k underflows for all but the copies
        constant = 1.0
    else:
        ls = np.full(D, np.sqrt(D / 6.0))
        constant = 50.0 if config == "iso_c50" else 1.0
    alpha = rng.normal(size=N)
    alpha *= 1e4 / np.abs(alpha).sum()
    return (Xc / ls).astype(np.float32), (X / ls).astype(np.float32), alpha, constant
