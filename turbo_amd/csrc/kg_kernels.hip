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

struct KgEnvArgs {
    const double *C;               // (rows, Apad) raw latent cross-covariance of the chunk
    const double *mu, *sigma;      // the chunk's rows of the sweep's outputs
    const double *mu_a;            // (A) raw mean at the points
    double *kg;                    // the chunk's rows of the result
    int m, A, Apad;
    double sf, noise_var, obs_var; // noise y_std^2; (noise + jitter) y_std^2
};

// one wave per candidate: its A + 1 lines into LDS, then the walk along the upper envelope (every lane carries the sum)
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
            cur = jm;
        }
    }
    if (lane == 0) g.kg[r] = kg;
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

hipError_t launch_kg_chunk(Context &c, double *ws, const KgChunk &k, const double *pts, const KgPoints &p, int64_t i0, int m,
                           double sf, double *kg, bool remean) {
    hipStream_t s = c.stream;
    const int mpad = (m + 127) / 128 * 128, Apad = (int)p.Apad, A = (int)p.A, Np = (int)c.Np;   // mpad <= k.rows
    double *Us = ws + k.o_Us, *Ks = ws + k.o_Ks, *C = ws + k.o_C;
    TGP_TRY(launch_cov_cross(c, c.d_cand + i0 * c.D, m, mpad, Us, Ks, remean ? ws + k.o_mu : nullptr,
                             reinterpret_cast<long long *>(ws + k.o_cnt)));
    // (the mean kernel writes whole 128-row tiles: into the workspace, then the m live rows over the sweep's)
    if (remean) TGP_TRY(hipMemcpyAsync(c.d_mu + i0, ws + k.o_mu, (size_t)m * sizeof(double), hipMemcpyDeviceToDevice, s));
    {
        GemmNtArgs g{};
        g.A = Ks; g.lda = Np; g.B = pts + p.o_W; g.ldb = Np; g.C = C; g.ldc = Apad; g.Ct = nullptr;
        g.ntm = mpad / 128; g.ntn = Apad / 128; g.K = Np; g.alpha = 1.0; g.beta = 0.0;
        TGP_TRY((launch_gemm_nt_glds<double, KN_FULL, TM_FULL>(s, c.device, g, g.ntm * g.ntn, 1)));
    }
    {
        auto kern = by_kind(c.kernel, [](auto K) { return kg_prior_kernel<K()>; });
        hipLaunchKernelGGL(kern, dim3(Apad / PW_T, mpad / PW_T), dim3(256), 0, s, Us, pts + p.o_Ua, C, m, A, Apad, (int)c.Dp,
                           c.constant, c.y_std * c.y_std);
        TGP_TRY(hipGetLastError());
    }
    KgEnvArgs e{};
    e.C = C; e.mu = c.d_mu + i0; e.sigma = c.d_sigma + i0; e.mu_a = pts + p.o_mu; e.kg = kg + i0;
    e.m = m; e.A = A; e.Apad = Apad;
    e.sf = sf; e.noise_var = c.noise * (c.y_std * c.y_std); e.obs_var = (c.noise + c.jitter) * (c.y_std * c.y_std);
    hipLaunchKernelGGL(kg_envelope_kernel, dim3((m + KG_WAVES - 1) / KG_WAVES), dim3(64 * KG_WAVES), 0, s, e);
    return hipGetLastError();
}

}  // namespace tgp
