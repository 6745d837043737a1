// kg_kernels.hip -- the knowledge gradient over the resident batch (tgp_kg_set_points, tgp_sweep_kg; include/turbogp.h):
// the first acquisition that needs the posterior covariance between every candidate and a set of OTHER points, the
// discretisation set Xa (A <= 256).  All f64, whatever the handle's dtype.  In normalised units (u = x / l, c the
// constant, k0 the unit kernel, K the fitted kernel matrix):
//   once per fit and point set (launch_kg_points)
//     Ka   = c k0(Xa, X)                      (Apad, Np)   the cov path's scale / cross-kernel / mean kernels
//     mu_a = y_mean + y_std Ka alpha          (Apad)
//     W    = Linv^T (Linv Ka^T), row-wise     (Apad, Np)   launch_linv_solve: the K^-1 apply of the Thompson draw
//   per chunk of candidates (launch_kg_chunk)
//     Ks   = c k0(Xc, X)                      (rows, Np)   the cov path's cross-kernel
//     mu   = y_mean + y_std Ks alpha          (rows)       only where the sweep ran in f32 arithmetic: the cov path's mean
//                                                          kernel over the slab that is there anyway replaces the sweep's
//                                                          f32 mean (the variance needs the N^2 contraction: it stays)
//     G    = Ks W^T                           (rows, Apad) gemm_nt_glds.hpp, KN_FULL: v_mfma_f64_16x16x4 over 16-wide k-tiles
//     C    = y_std^2 (c k0(Xc, Xa) - G)                    kg_prior_kernel: pairwise.hpp's 64 x 64 tiles, in place
//     KG   per candidate from C, mu, sigma                 kg_envelope_kernel: one wave per candidate
//   per call of tgp_kg_grad, m <= 4096 query points (launch_kg_grad): the query front (x / l, c k0, c h, K^-1 k), C as above,
//     the envelope with its record (kg_envelope_kernel<true>), omega (kg_omega_kernel), the (point, dimension) reductions
//     (kg_grad_kernel)
// Order of every sum: the k-loop of G runs over ALL Np training columns in ascending 16-wide tiles whatever M, the
// chunk or the row is, and a row's position only selects which lanes hold it; the envelope walks its lines in
// ascending slope.  No atomics on floating-point data, no split of the k-range: a candidate's C row and KG are the
// same bits alone (M = 1) or as row 20 000 of a batch.
//
// The envelope (Frazier, Powell & Dayanik 2009, algorithm 1, without the sort).  Lines i = 0 .. A: a_i + b_i Z.  The line
// of the smallest slope (the largest intercept among equals) is the envelope's left end.  From an envelope line i the
// next one is the steeper line j whose intersection z_ij = (a_i - a_j) / (b_j - b_i) comes first (the steepest among
// equal z); of two lines with EQUAL slope b_j the one with the larger intercept meets i first, so the lower one is
// never chosen, and a dominated line never comes first.  KG = sum over the walk of (b_j - b_i) f(-|z_ij|),
// f(z) = phi(z) + z Phi(z) through erfcx: every term is >= 0, nothing cancels against max_i a_i.
#include <hip/hip_runtime.h>
#include <math.h>

#include "gemm_nt_glds.hpp"
#include "pairwise.hpp"
#include "query_math.hpp"
#include "tgp_internal.hpp"

namespace tgp {

#define TGP_TRY(call)                          \
    do {                                       \
        hipError_t e_ = (call);                \
        if (e_ != hipSuccess) return e_;       \
    } while (0)

constexpr int KG_MAXA = 256;       // most discretisation points
constexpr int KG_WAVES = 4;        // candidates per workgroup of the envelope kernel

// C tile (64 candidates x 64 points) in place: C = scale (c k0(Uc, Ua) - G) for rows < m and columns < A, zero elsewhere
template <int KIND>
__global__ __launch_bounds__(256) void kg_prior_kernel(const double *__restrict__ Uc, const double *__restrict__ Ua,
                                                       double *__restrict__ C, int m, int A, int Apad, int Dp,
                                                       double constant, double scale) {
    constexpr int LD = PwCfg<double>::LD, DC = PwCfg<double>::DC;
    __shared__ __attribute__((aligned(16))) double Ct[DC][LD];
    __shared__ __attribute__((aligned(16))) double Xt[DC][LD];
    const int j0 = blockIdx.x * PW_T, i0 = blockIdx.y * PW_T;
    double d2[4][4];
    pairwise_sqdist<double>(Uc, i0, m, Ua, j0, A, Dp, Ct, Xt, d2);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + 4 * ty + a;
        double *row = C + (long)i * Apad + j0 + 4 * tx;
        d4_t g = *reinterpret_cast<const d4_t *>(row);
        d4_t v;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + 4 * tx + b;
            v[b] = (i < m && j < A) ? scale * (kernel_value<double, KIND>(d2[a][b], constant) - g[b]) : 0.0;
        }
        *reinterpret_cast<d4_t *>(row) = v;
    }
}

// f(z) = phi(z) + z Phi(z) at z = -az, az >= 0: exp(-az^2 / 2) (1 / sqrt(2 pi) - az erfcx(az / sqrt 2) / 2); 0 from
// az = 40 on (exp(-800) is below the smallest double) and for a NaN
__device__ __forceinline__ double kg_f_neg(double az) {
    if (!(az < 40.0)) return 0.0;
    const double t = az * 0.70710678118654752440;
    return exp(-t * t) * fmax(0.3989422804014327 - 0.5 * az * erfcx(t), 0.0);
}

// Phi(-az), az >= 0, through erfcx as kg_f_neg: exp(-az^2 / 2) erfcx(az / sqrt 2) / 2; 0 from az = 40 on and for a NaN
__device__ __forceinline__ double kg_Phi_neg(double az) {
    if (!(az < 40.0)) return 0.0;
    const double t = az * 0.70710678118654752440;
    return 0.5 * exp(-t * t) * erfcx(t);
}
__device__ __forceinline__ double kg_phi(double z) { return 0.3989422804014327 * exp(-0.5 * z * z); }   // 0 at +-inf
// Phi(hi) - Phi(lo), lo <= hi, from the two tails on the side where they are small
__device__ __forceinline__ double kg_Phi_between(double lo, double hi) {
    if (lo >= 0.0) return kg_Phi_neg(lo) - kg_Phi_neg(hi);
    if (hi <= 0.0) return kg_Phi_neg(-hi) - kg_Phi_neg(-lo);
    return 1.0 - kg_Phi_neg(-lo) - kg_Phi_neg(hi);
}

struct KgEnvArgs {
    const double *C;               // (rows, Apad) raw latent cross-covariance of the chunk
    const double *mu, *sigma;      // the chunk's rows of the sweep's outputs
    const double *mu_a;            // (A) raw mean at the points
    double *kg;                    // the chunk's rows of the result
    int m, A, Apad;
    double sf, noise_var, obs_var; // noise y_std^2; (noise + jitter) y_std^2
    // GRAD (tgp_kg_grad): the envelope's record per point, for kg_omega_kernel / kg_grad_kernel
    double *env_e;                 // (m, KG_ENV_LD) e_k = E_k / s of the envelope's lines i < A, left to right
    int *env_idx, *env_n;          // (m, KG_ENV_LD) their indices; (m) their number
    double *coef;                  // (m, 2) c_mu = -sf y_std T, c_v = 2 y_std^2 (dKG / dv)
    double y_std;
};

// one wave per candidate: its A + 1 lines into LDS, then the walk along the upper envelope (every lane carries the sum).
// GRAD: the walk also leaves what the gradient needs (include/turbogp.h, tgp_kg_grad).  Line j_k is the maximum on
// (z_k, z_k+1); E_k = phi(z_k) - phi(z_k+1), and by the envelope theorem
//   grad KG = sum_k E_k grad b_jk + sf T grad mu,   T = [A on the envelope] P_A - [a_A > max_{i<A} a_i]
// with grad b_i = grad C_i / s - b_i grad v / (2 s^2), grad b_A = grad v / s - b_A grad v / (2 s^2), so that
//   dKG / dv = [A on the envelope] E_A / s - (sum_k E_k b_jk) / (2 s^2)      (0 where v was clamped)
// Where the candidate's own line is the strict maximum intercept T is minus the two tails outside its interval: P_A - 1
// is never formed.  The value is the instance without GRAD's, statement for statement.
template <bool GRAD>
__global__ __launch_bounds__(64 * KG_WAVES) void kg_envelope_kernel(KgEnvArgs g) {
    __shared__ double la[KG_WAVES][KG_MAXA + 1];
    __shared__ double lb[KG_WAVES][KG_MAXA + 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int r = blockIdx.x * KG_WAVES + wave;
    const int A = g.A, L = A + 1;
    bool live = r < g.m;
    double s = 1.0, v = 0.0, mux = 0.0;
    if (live) {
        const double sg = g.sigma[r];
        mux = g.mu[r];
        v = sg * sg - g.noise_var;
        if (!(v > 0.0)) v = (v != v) ? v : 0.0;       // max(., 0); a NaN stays a NaN
        const double s2 = v + g.obs_var;
        live = s2 > 0.0 && s2 <= 1.7976931348623157e308 && fabs(mux) <= 1.7976931348623157e308;
        s = live ? sqrt(s2) : 1.0;
    }
    double *a = la[wave], *b = lb[wave];
    if (live) {
        const double *crow = g.C + (long)r * g.Apad;
        for (int i = lane; i < L; i += 64) {
            a[i] = g.sf * (i < A ? g.mu_a[i] : mux);
            b[i] = (i < A ? crow[i] : v) / s;
        }
    }
    __syncthreads();                                  // (the only barrier: every wave reaches it; the walk below has none)
    if (r >= g.m) return;
    double kg = 0.0;
    // GRAD: the lines i < A recorded so far, sum_k E_k b_jk, and the candidate's own line's E_A and interval
    int nl = 0;
    double Sb = 0.0, EA = 0.0, zlo = 0.0, zhi = 0.0, zprev = -INFINITY;
    bool onA = false;
    auto record = [&](int line, double zl, double zh) {
        const double E = kg_phi(zl) - kg_phi(zh);
        Sb = fma(E, b[line], Sb);
        if (line == A) {
            onA = true; EA = E; zlo = zl; zhi = zh;
        } else {
            if (lane == 0) { g.env_e[(long)r * KG_ENV_LD + nl] = E / s; g.env_idx[(long)r * KG_ENV_LD + nl] = line; }
            ++nl;
        }
    };
    if (live) {
        // the left end: smallest slope, then largest intercept, then lowest index
        double sb = INFINITY, sa = -INFINITY;
        int si = 0x7fffffff;
        for (int i = lane; i < L; i += 64) {
            const double bi = b[i], ai = a[i];
            if (bi < sb || (bi == sb && (ai > sa || (ai == sa && i < si)))) { sb = bi; sa = ai; si = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double b2 = __shfl_xor(sb, o, 64), a2 = __shfl_xor(sa, o, 64);
            const int i2 = __shfl_xor(si, o, 64);
            if (b2 < sb || (b2 == sb && (a2 > sa || (a2 == sa && i2 < si)))) { sb = b2; sa = a2; si = i2; }
        }
        int cur = si;
        for (int step = 0; step < L && cur != 0x7fffffff; ++step) {
            const double ai = a[cur], bi = b[cur];
            double zm = INFINITY, bm = -INFINITY;
            int jm = 0x7fffffff;
            for (int j = lane; j < L; j += 64) {
                const double bj = b[j], db = bj - bi;
                if (db > 0.0) {
                    const double z = (ai - a[j]) / db;
                    if (z < zm || (z == zm && (bj > bm || (bj == bm && j < jm)))) { zm = z; bm = bj; jm = j; }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double z2 = __shfl_xor(zm, o, 64), b2 = __shfl_xor(bm, o, 64);
                const int j2 = __shfl_xor(jm, o, 64);
                if (j2 != 0x7fffffff && (jm == 0x7fffffff || z2 < zm || (z2 == zm && (b2 > bm || (b2 == bm && j2 < jm))))) { zm = z2; bm = b2; jm = j2; }
            }
            if (jm == 0x7fffffff) break;              // (uniform: every lane holds the same winner)
            kg += (bm - bi) * kg_f_neg(fabs(zm));
            if constexpr (GRAD) { record(cur, zprev, zm); zprev = zm; }
            cur = jm;
        }
        if constexpr (GRAD) {
            if (cur != 0x7fffffff) record(cur, zprev, INFINITY);      // the envelope's right end
        }
    }
    if (lane == 0) g.kg[r] = kg;
    if constexpr (GRAD) {
        double c_mu = 0.0, c_v = 0.0;
        if (live) {
            double amax = -INFINITY;                  // max_{i<A} a_i
            for (int i = lane; i < A; i += 64) amax = fmax(amax, a[i]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o, 64));
            double T;
            if (a[A] > amax)                          // STRICT: at a tie the candidate's line is not the maximum
                T = onA ? -((zlo <= 0.0 ? kg_Phi_neg(-zlo) : 1.0 - kg_Phi_neg(zlo)) + (zhi >= 0.0 ? kg_Phi_neg(zhi) : 1.0 - kg_Phi_neg(-zhi))) : -1.0;
            else
                T = onA ? kg_Phi_between(zlo, zhi) : 0.0;
            c_mu = -g.sf * g.y_std * T;
            if (v > 0.0) c_v = 2.0 * (g.y_std * g.y_std) * ((onA ? EA / s : 0.0) - Sb / (2.0 * s * s));
        }
        if (lane == 0) { g.env_n[r] = nl; g.coef[2 * r] = c_mu; g.coef[2 * r + 1] = c_v; }
    }
}

// omega[q][j] = c_mu alpha_j + c_v w_qj + y_std^2 sum_k e_k W[j_k][j] over the envelope's lines, left to right: a gather of
// the few rows of W the envelope holds (2-10 of A + 1 in practice), not a dense product.  0 from N on.  The point's first
// workgroup also leaves the prior term's weights, once for all D dimensions: env_eh[k] = e_k c h(|u_q - ua_jk|), h(0) = 0 for
// Matern-1/2 as everywhere
template <int KIND>
__global__ __launch_bounds__(256) void kg_omega_kernel(const double *__restrict__ alpha, const double *__restrict__ w,
                                                       const double *__restrict__ W, const double *__restrict__ coef,
                                                       const double *__restrict__ env_e, const int *__restrict__ env_idx,
                                                       const int *__restrict__ env_n, const double *__restrict__ uq,
                                                       const double *__restrict__ Ua, double *__restrict__ env_eh,
                                                       double *__restrict__ omega, int N, int Np, int Dp, double constant,
                                                       double y2) {
    __shared__ double se[KG_ENV_LD];
    __shared__ int si[KG_ENV_LD];
    const int q = blockIdx.y;
    const int n = env_n[q];
    for (int k = threadIdx.x; k < n; k += 256) { se[k] = env_e[(long)q * KG_ENV_LD + k]; si[k] = env_idx[(long)q * KG_ENV_LD + k]; }
    __syncthreads();
    if (blockIdx.x == 0) {
        const double *u = uq + (long)q * Dp;
        for (int k = threadIdx.x; k < n; k += 256) {
            const double *xa = Ua + (long)si[k] * Dp;
            double d2 = 0.0;
            for (int e = 0; e < Dp; ++e) {
                const double df = u[e] - xa[e];
                d2 = fma(df, df, d2);
            }
            env_eh[(long)q * KG_ENV_LD + k] = se[k] * (constant * h_weight<KIND>(d2));
        }
    }
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Np) return;
    double o = 0.0;
    if (j < N) {
        double t = 0.0;
        for (int k = 0; k < n; ++k) t = fma(se[k], W[(long)si[k] * Np + j], t);
        o = fma(coef[2 * q], alpha[j], fma(coef[2 * q + 1], w[(long)q * Np + j], y2 * t));
    }
    omega[(long)q * Np + j] = o;
}

// grad[q][d] = (sum_j omega_qj c h_qj (u_qd - xs_jd) - y_std^2 sum_k env_eh_k (u_qd - ua_jk,d)) / l_d: the training points'
// part as q_reduce_kernel sums it (a thread's stride of 256, then the tree), the prior term over the envelope's lines the
// same way
__global__ __launch_bounds__(256) void kg_grad_kernel(const double *__restrict__ Xs, const double *__restrict__ ls,
                                                      const double *__restrict__ uq, const double *__restrict__ hw,
                                                      const double *__restrict__ omega, const double *__restrict__ Ua,
                                                      const double *__restrict__ env_eh, const int *__restrict__ env_idx,
                                                      const int *__restrict__ env_n, double *__restrict__ grad, int N,
                                                      int Np, int D, int Dp, double y2) {
    __shared__ double red[2][256];
    const int q = blockIdx.y, d = blockIdx.x;
    const double ud = uq[(long)q * Dp + d];
    const double *hq = hw + (long)q * Np, *oq = omega + (long)q * Np;
    double gs = 0.0, pr = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) gs = fma(oq[j], hq[j] * (ud - Xs[(long)j * Dp + d]), gs);
    const int n = env_n[q];
    for (int k = threadIdx.x; k < n; k += 256)
        pr = fma(env_eh[(long)q * KG_ENV_LD + k], ud - Ua[(long)env_idx[(long)q * KG_ENV_LD + k] * Dp + d], pr);
    red[0][threadIdx.x] = gs; red[1][threadIdx.x] = pr;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) grad[(long)q * D + d] = (red[0][0] - y2 * red[1][0]) / ls[d];
}

// mu = y_mean + y_std ks.alpha and sigma = y_std sqrt(max(c + noise - v.v, 0)) of query point q from the front's vectors,
// for handles whose sweep is not f64 (q_reduce_kernel's sums and order)
__global__ __launch_bounds__(256) void kg_posterior_kernel(const double *__restrict__ alpha, const double *__restrict__ ks,
                                                           const double *__restrict__ v, double *__restrict__ mu,
                                                           double *__restrict__ sigma, int N, int Np, double kss,
                                                           double y_mean, double y_std) {
    __shared__ double red[2][256];
    const int q = blockIdx.x;
    const double *kq = ks + (long)q * Np, *vq = v + (long)q * Np;
    double mun = 0.0, qv = 0.0;
    for (int j = threadIdx.x; j < N; j += 256) {
        mun = fma(kq[j], alpha[j], mun);
        qv = fma(vq[j], vq[j], qv);
    }
    red[0][threadIdx.x] = mun; red[1][threadIdx.x] = qv;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double var = kss - red[1][0];
        mu[q] = y_std * red[0][0] + y_mean;
        sigma[q] = y_std * sqrt(var > 0.0 ? var : 0.0);
    }
}

int64_t kg_points_doubles(const Context &c, int64_t A, KgPoints *out) {
    auto al = [](int64_t n) { return (n + 15) & ~(int64_t)15; };
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += al(n); return o; };
    KgPoints p{};
    p.A = A; p.Apad = (A + 127) / 128 * 128;
    p.o_cnt = take(16);
    p.o_Xa = take(A * c.D);
    p.o_Ua = take(p.Apad * c.Dp);
    p.o_mu = take(p.Apad);
    p.o_W = take(p.Apad * c.Np);
    p.o_Ka = take(p.Apad * c.Np);
    p.o_Z = take(p.Apad * c.Np);
    if (out) *out = p;
    return off;
}

hipError_t launch_kg_points(Context &c, double *ws, const KgPoints &p) {
    const int A = (int)p.A, Apad = (int)p.Apad;
    const size_t slab = (size_t)Apad * (size_t)c.Np * sizeof(double);
    // launch_linv_solve writes the first A rows up to N rounded to 16: the rest of W (and of Z) is zero by this
    TGP_TRY(hipMemsetAsync(ws + p.o_W, 0, slab, c.stream));
    TGP_TRY(hipMemsetAsync(ws + p.o_Z, 0, slab, c.stream));
    TGP_TRY(launch_cov_cross(c, ws + p.o_Xa, A, Apad, ws + p.o_Ua, ws + p.o_Ka, ws + p.o_mu, reinterpret_cast<long long *>(ws + p.o_cnt)));
    return launch_linv_solve(c, ws + p.o_Ka, ws + p.o_Z, ws + p.o_W, A);
}

int64_t kg_chunk_doubles(const Context &c, int64_t rows, int64_t Apad, KgChunk *out) {
    auto al = [](int64_t n) { return (n + 15) & ~(int64_t)15; };
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += al(n); return o; };
    KgChunk k{};
    k.rows = rows; k.Apad = Apad;
    k.o_cnt = take(16);
    k.o_Us = take(rows * c.Dp);
    k.o_Ks = take(rows * c.Np);
    k.o_C = take(rows * Apad);
    k.o_mu = take(rows);
    if (out) *out = k;
    return off;
}

// the chunk's C = y_std^2 (c k0(X, Xa) - Ks W^T) for the m rows X (m, D) on the device; mu != null: their mean re-formed
// in f64 from the cross-kernel (whole 128-row tiles are written)
static hipError_t kg_cross_cov(Context &c, double *ws, const KgChunk &k, const double *pts, const KgPoints &p, const double *X,
                               int m, double *mu) {
    hipStream_t s = c.stream;
    const int mpad = (m + 127) / 128 * 128, Apad = (int)p.Apad, A = (int)p.A, Np = (int)c.Np;   // mpad <= k.rows
    double *Us = ws + k.o_Us, *Ks = ws + k.o_Ks, *C = ws + k.o_C;
    TGP_TRY(launch_cov_cross(c, X, m, mpad, Us, Ks, mu, reinterpret_cast<long long *>(ws + k.o_cnt)));
    {
        GemmNtArgs g{};
        g.A = Ks; g.lda = Np; g.B = pts + p.o_W; g.ldb = Np; g.C = C; g.ldc = Apad; g.Ct = nullptr;
        g.ntm = mpad / 128; g.ntn = Apad / 128; g.K = Np; g.alpha = 1.0; g.beta = 0.0;
        TGP_TRY((launch_gemm_nt_glds<double, KN_FULL, TM_FULL>(s, c.device, g, g.ntm * g.ntn, 1)));
    }
    auto kern = by_kind(c.kernel, [](auto K) { return kg_prior_kernel<K()>; });
    hipLaunchKernelGGL(kern, dim3(Apad / PW_T, mpad / PW_T), dim3(256), 0, s, Us, pts + p.o_Ua, C, m, A, Apad, (int)c.Dp,
                       c.constant, c.y_std * c.y_std);
    return hipGetLastError();
}

// what both envelope instances read: the chunk's C and the posterior of its m rows
static KgEnvArgs kg_env_args(const Context &c, const double *C, const double *pts, const KgPoints &p, const double *mu,
                             const double *sigma, double *kg, int m, double sf) {
    KgEnvArgs e{};
    e.C = C; e.mu = mu; e.sigma = sigma; e.mu_a = pts + p.o_mu; e.kg = kg;
    e.m = m; e.A = (int)p.A; e.Apad = (int)p.Apad;
    e.sf = sf; e.noise_var = c.noise * (c.y_std * c.y_std); e.obs_var = (c.noise + c.jitter) * (c.y_std * c.y_std);
    return e;
}

hipError_t launch_kg_chunk(Context &c, double *ws, const KgChunk &k, const double *pts, const KgPoints &p, int64_t i0, int m,
                           double sf, double *kg, bool remean) {
    TGP_TRY(kg_cross_cov(c, ws, k, pts, p, c.d_cand + i0 * c.D, m, remean ? ws + k.o_mu : nullptr));
    // (the mean kernel writes whole 128-row tiles: into the workspace, then the m live rows over the sweep's)
    if (remean) TGP_TRY(hipMemcpyAsync(c.d_mu + i0, ws + k.o_mu, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, c.stream));
    const KgEnvArgs e = kg_env_args(c, ws + k.o_C, pts, p, c.d_mu + i0, c.d_sigma + i0, kg + i0, m, sf);
    hipLaunchKernelGGL(kg_envelope_kernel<false>, dim3((m + KG_WAVES - 1) / KG_WAVES), dim3(64 * KG_WAVES), 0, c.stream, e);
    return hipGetLastError();
}

int64_t kg_grad_doubles(const Context &c, int64_t m, int64_t Apad, KgGradWs *out) {
    auto al = [](int64_t n) { return (n + 15) & ~(int64_t)15; };
    KgGradWs g{};
    int64_t off = kg_chunk_doubles(c, (m + 127) / 128 * 128, Apad, &g.k);
    auto take = [&](int64_t n) { const int64_t o = off; off += al(n); return o; };
    g.o_Xq = take(m * c.D); g.o_uq = take(m * c.Dp);
    g.o_ks = take(m * c.Np); g.o_hw = take(m * c.Np); g.o_v = take(m * c.Np); g.o_w = take(m * c.Np);
    g.o_mu = take(m); g.o_sigma = take(m); g.o_coef = take(2 * m);
    g.o_env_e = take(m * KG_ENV_LD); g.o_env_eh = take(m * KG_ENV_LD); g.o_env_idx = take(m * KG_ENV_LD / 2); g.o_env_n = take((m + 1) / 2);
    g.o_val = take(m); g.o_grad = take(m * c.D);
    if (out) *out = g;
    return off;
}

// tgp_kg_grad's own kernels: the query front as tgp_acq_grad runs it, the chunk's cross-covariance as tgp_sweep_kg forms
// it (the same kernels over the same sums: C and the value are the sweep's bits), the envelope with its record, then
// omega and the (q, d) reductions.  Every sum's order is fixed and a point meets nobody else's data: its value and
// gradient do not depend on m or its row
hipError_t launch_kg_grad(Context &c, double *ws, const KgGradWs &g, const double *pts, const KgPoints &p, int m, double sf,
                          bool own_posterior) {
    hipStream_t s = c.stream;
    const int N = (int)c.N, Np = (int)c.Np, D = (int)c.D, Dp = (int)c.Dp;
    const double y2 = c.y_std * c.y_std;
    double *uq = ws + g.o_uq, *ks = ws + g.o_ks, *hw = ws + g.o_hw, *v = ws + g.o_v, *w = ws + g.o_w;
    double *env_e = ws + g.o_env_e, *coef = ws + g.o_coef;
    int *env_idx = reinterpret_cast<int *>(ws + g.o_env_idx), *env_n = reinterpret_cast<int *>(ws + g.o_env_n);
    TGP_TRY(launch_query_front(c, ws + g.o_Xq, uq, ks, hw, v, w, m));
    if (own_posterior) {
        hipLaunchKernelGGL(kg_posterior_kernel, dim3(m), dim3(256), 0, s, c.d_alpha, ks, v, ws + g.o_mu, ws + g.o_sigma, N, Np,
                           c.constant + c.noise, c.y_mean, c.y_std);
        TGP_TRY(hipGetLastError());
    }
    TGP_TRY(kg_cross_cov(c, ws, g.k, pts, p, ws + g.o_Xq, m, nullptr));
    KgEnvArgs e = kg_env_args(c, ws + g.k.o_C, pts, p, ws + g.o_mu, ws + g.o_sigma, ws + g.o_val, m, sf);
    e.env_e = env_e; e.env_idx = env_idx; e.env_n = env_n; e.coef = coef; e.y_std = c.y_std;
    hipLaunchKernelGGL(kg_envelope_kernel<true>, dim3((m + KG_WAVES - 1) / KG_WAVES), dim3(64 * KG_WAVES), 0, s, e);
    TGP_TRY(hipGetLastError());
    double *omega = v;      // (Linv ks has served: the posterior above was its last reader)
    double *env_eh = ws + g.o_env_eh;
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return kg_omega_kernel<K()>; }), dim3(Np / 256, m), dim3(256), 0, s, c.d_alpha, w,
                       pts + p.o_W, coef, env_e, env_idx, env_n, uq, pts + p.o_Ua, env_eh, omega, N, Np, Dp, c.constant, y2);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kg_grad_kernel, dim3(D, m), dim3(256), 0, s, c.d_Xs, c.d_ls, uq, hw, omega, pts + p.o_Ua, env_eh, env_idx,
                       env_n, ws + g.o_grad, N, Np, D, Dp, y2);
    return hipGetLastError();
}

}  // namespace tgp
