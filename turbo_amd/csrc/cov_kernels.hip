// cov_kernels.hip -- the JOINT posterior over m <= 4096 query points: covariance, exact samples (tgp_predict_cov,
// tgp_sample_joint; include/turbogp.h).  What scikit-learn does in predict(return_cov=True) --
// V = solve_triangular(L, K*^T); y_cov = kernel_(X) - V^T V (sklearn/gaussian_process/_gpr.py:454-462) -- and in
// sample_y -- rng.multivariate_normal(y_mean, y_cov, n_samples) (:497-535) -- with the factor the fit left resident.
// All f64, whatever the handle's dtype.  In normalised units (u = x / l, c the constant, k0 the unit kernel):
//   Ks    = c k0(Xq, X)                                 (mpad, Np)   cov_ks_kernel: pairwise.hpp's 64 x 64 tiles
//   mu    = y_mean + y_std Ks alpha                     (mpad)       cov_mu_kernel: one wave per point, fixed order
//   Vt    = Ks Linv^T  (= V^T, V = Linv Ks^T)           (mpad, NV)   gemm_nt_glds.hpp, k-range cut at B's diagonal tile
//   Sigma = c k0(Xq, Xq) + diag - Vt Vt^T               (mpad, mpad) cov_syrk_kernel: lower 128 x 128 tiles only, the
//                                                                    query points' own kernel formed in the epilogue
// and for a sample: Lc = chol(Sigma + nugget I) by 64-column panels (chol64.hpp's block factorisation, a panel solve on
// its inverse, gemm64_glds.hpp's rank-64 trailing update), then Y = mu 1^T + y_std E Lc^T as one triangular product.
//
// Order of every sum: an entry's k-loop runs over the training points in ascending 16-wide k-tiles whatever m is, and
// a tile's position only selects which lanes hold it: the bits of Sigma[i][j] depend on rows i and j alone (a pair
// computed with m = 2 or inside m = 300 is the same bits), and on nothing that varies from run to run -- no atomics on
// floating-point values, no split of the k-range.  The lower triangle is computed, the upper one is its copy.
#include <hip/hip_runtime.h>
#include <math.h>

#include "chol64.hpp"
#include "gemm64_glds.hpp"
#include "gemm_nt_glds.hpp"
#include "pairwise.hpp"
#include "philox.hpp"
#include "tgp_internal.hpp"

namespace tgp {

#define TGP_TRY(call)                          \
    do {                                       \
        hipError_t e_ = (call);                \
        if (e_ != hipSuccess) return e_;       \
    } while (0)

constexpr uint32_t COV_TAG = 0x434F564Au;   // "COVJ": the fourth counter word of the joint samples' normals
constexpr int COV_EPS_STRIDE = 4096;        // element s 4096 + j: sample s depends neither on S nor on m

// Us (mpad, Dp) = Xq / length_scale, rows from m on and columns from D on zero; the call's first kernel also clears its counters
__global__ __launch_bounds__(256) void cov_scale_kernel(const double *__restrict__ Xq, const double *__restrict__ ls,
                                                        double *__restrict__ Us, int m, int mpad, int D, int Dp,
                                                        long long *__restrict__ cnt) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) { cnt[0] = 0; cnt[1] = 0; }   // the call's counters: negative diagonal entries, the factorisation's flag
    if (e >= (long)mpad * Dp) return;
    const int i = (int)(e / Dp), d = (int)(e % Dp);
    Us[e] = (i < m && d < D) ? Xq[(long)i * D + d] / ls[d] : 0.0;
}

// Ks tile (64 query points x 64 training points); rows from m on and columns from N on are written as zeros
template <int KIND>
__global__ __launch_bounds__(256) void cov_ks_kernel(const double *__restrict__ Us, const double *__restrict__ Xs,
                                                     double *__restrict__ Ks, int m, int N, int Np, int Dp,
                                                     double constant) {
    constexpr int LD = PwCfg<double>::LD, DC = PwCfg<double>::DC;
    __shared__ __attribute__((aligned(16))) double Ct[DC][LD];
    __shared__ __attribute__((aligned(16))) double Xt[DC][LD];
    const int n0 = blockIdx.x * PW_T, i0 = blockIdx.y * PW_T;
    double d2[4][4];
    pairwise_sqdist<double>(Us, i0, m, Xs, n0, N, Dp, Ct, Xt, d2);
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + 4 * ty + a;
        d4_t v;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int n = n0 + 4 * tx + b;
            v[b] = (i < m && n < N) ? kernel_value<double, KIND>(d2[a][b], constant) : 0.0;
        }
        *reinterpret_cast<d4_t *>(Ks + (long)i * Np + n0 + 4 * tx) = v;
    }
}

// mu[i] = y_mean + y_std sum_{k < N} Ks[i][k] alpha[k]: one wave per point, lane l takes k = l, l + 64, ... in
// ascending order, then the butterfly -- the same order for a point whatever travels with it
__global__ __launch_bounds__(256) void cov_mu_kernel(const double *__restrict__ Ks, const double *__restrict__ alpha,
                                                     double *__restrict__ mu, int m, int mpad, int N, int Np,
                                                     double y_mean, double y_std) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= mpad) return;
    double s = 0.0;
    if (i < m)
        for (int k = lane; k < N; k += 64) s = fma(Ks[(long)i * Np + k], alpha[k], s);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) mu[i] = i < m ? y_mean + y_std * s : 0.0;
}

// ---- Sigma = c k0(Xq, Xq) + diag - Vt Vt^T over the lower 128 x 128 tiles ------------------------------------------
// The k-loop is gemm_nt_glds.hpp's (operands DMA'd into the swizzled LDS image, two buffers, 2 x 2 waves of 64 x 64
// fragments) with A = B = Vt.  The epilogue walks the tile's four 64 x 64 quadrants: all 256 threads form the quadrant's
// squared distances with pairwise.hpp (the arithmetic of every other kernel matrix in the library), leave the kernel
// values in an LDS tile, and the wave whose accumulators ARE that quadrant combines them.  Only elements on and below
// the diagonal are formed; each is stored twice, at (i, j) and (j, i).
struct CovSyrkArgs {
    const double *Vt;     // (mpad, NV)
    const double *Us;     // (mpad, Dp)
    double *G;            // (mpad, mpad)
    double *dvec;         // (mpad) the diagonal before `scale`, as the pivot rule of the factorisation wants it, or null
    long long *nneg;      // [0] += entries of the scaled diagonal below zero
    int m, mpad, NV, Dp;
    double constant, diag_add, scale;
    int mirror;           // 1: (j, i) = (i, j); 0: zeros above the diagonal (the matrix is about to be factored in place)
};

template <int KIND>
__global__ __launch_bounds__(256, 2) void cov_syrk_kernel(CovSyrkArgs g) {
    using MF = Mfma<double>;
    using vec_t = MF::vec_t;
    using acc_t = MF::acc_t;
    constexpr int BM = 128, BK = 16, NFM = 4, NFN = 4, NG = 4, KSTEPS = 2;
    constexpr int TILE_BYTES = BM * 128, BUF_BYTES = 2 * TILE_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 64, wn0 = (wave & 1) * 64;
    int tm, tn;
    {
        const int bx = blockIdx.x;
        int r = (int)((sqrtf(8.0f * (float)bx + 1.0f) - 1.0f) * 0.5f);
        while ((r + 1) * (r + 2) / 2 <= bx) ++r;
        while (r * (r + 1) / 2 > bx) --r;
        tm = r;
        tn = bx - r * (r + 1) / 2;
    }
    const int srow = lane >> 3, schunk = lane & 7;
    const char *asrc[4];
    const char *bsrc[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int row = (4 * p + wave) * 8 + srow;
        const int src_chunk = schunk ^ ((row >> 1) & 7);
        asrc[p] = reinterpret_cast<const char *>(g.Vt + ((long)tm * BM + row) * g.NV) + src_chunk * 16;
        bsrc[p] = reinterpret_cast<const char *>(g.Vt + ((long)tn * BM + row) * g.NV) + src_chunk * 16;
    }
    auto stage = [&](int buf, int k0) {
        const long koff = (long)k0 * 8;
        char *base = smem_raw + buf * BUF_BYTES;
#pragma unroll
        for (int p = 0; p < 4; ++p)
            __builtin_amdgcn_global_load_lds((gbl_void_t *)(asrc[p] + koff), (lds_void_t *)(base + (4 * p + wave) * 8 * 128), 16, 0, 0);
#pragma unroll
        for (int p = 0; p < 4; ++p)
            __builtin_amdgcn_global_load_lds((gbl_void_t *)(bsrc[p] + koff), (lds_void_t *)(base + TILE_BYTES + (4 * p + wave) * 8 * 128), 16, 0, 0);
    };
    acc_t acc[NFM][NFN];
#pragma unroll
    for (int i = 0; i < NFM; ++i)
#pragma unroll
        for (int j = 0; j < NFN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
    const int fidx = MF::ab_idx(lane), grp = MF::ab_kg(lane);
    const int swz = (fidx >> 1) & 7;
    const int a_row_off = (wm0 + fidx) * 128, b_row_off = TILE_BYTES + (wn0 + fidx) * 128;
    int buf = 0;
    stage(0, 0);
    __syncthreads();
    for (int k0 = 0; k0 < g.NV; k0 += BK) {
        if (k0 + BK < g.NV) stage(buf ^ 1, k0 + BK);
        const char *base = smem_raw + buf * BUF_BYTES;
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
            const int coff = ((s * NG + grp) ^ swz) * 16;
            vec_t a[NFM], b[NFN];
#pragma unroll
            for (int i = 0; i < NFM; ++i) a[i] = *reinterpret_cast<const vec_t *>(base + a_row_off + i * 16 * 128 + coff);
#pragma unroll
            for (int j = 0; j < NFN; ++j) b[j] = *reinterpret_cast<const vec_t *>(base + b_row_off + j * 16 * 128 + coff);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < NFM; ++i)
#pragma unroll
                    for (int j = 0; j < NFN; ++j) acc[i][j] = MF::mma(a[i][e], b[j][e], acc[i][j]);
        }
        __syncthreads();
        buf ^= 1;
    }

    // ---- epilogue: the LDS is free (the loop's last barrier is behind every wave's last fragment read) ----
    constexpr int LD = PwCfg<double>::LD, DC = PwCfg<double>::DC, KLD = PW_T + 1;
    double (*Ct)[LD] = reinterpret_cast<double (*)[LD]>(smem_raw);
    double (*Xt)[LD] = Ct + DC;
    double (*Kt)[KLD] = reinterpret_cast<double (*)[KLD]>(smem_raw + 2 * DC * LD * sizeof(double));
    const int tx = tid & 15, ty = tid >> 4;
    int neg = 0;
    for (int qd = 0; qd < 4; ++qd) {
        const int qi = qd >> 1, qj = qd & 1;
        const int r0 = tm * BM + qi * 64, c0 = tn * BM + qj * 64;
        if (c0 > r0) continue;                         // the upper quadrant of a diagonal tile: its mirror covers it
        double d2[4][4];
        pairwise_sqdist<double>(g.Us, r0, g.mpad, g.Us, c0, g.mpad, g.Dp, Ct, Xt, d2);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) Kt[4 * ty + a][4 * tx + b] = kernel_value<double, KIND>(d2[a][b], g.constant);
        __syncthreads();
        if (wave == qd) {
#pragma unroll
            for (int i = 0; i < NFM; ++i)
#pragma unroll
                for (int j = 0; j < NFN; ++j) {
                    const int lc = j * 16 + MF::c_col(lane);
                    const int col = c0 + lc;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int lr = i * 16 + MF::c_row(lane, r);
                        const int row = r0 + lr;
                        if (row < col) continue;
                        double out;
                        if (row < g.m) {           // (col <= row < m)
                            const double v = (Kt[lr][lc] + (row == col ? g.diag_add : 0.0)) - acc[i][j][r];
                            out = g.scale * v;
                            if (row == col) {
                                if (g.dvec) g.dvec[row] = v;
                                neg += out < 0.0 ? 1 : 0;
                            }
                        } else {                   // padding: an identity block, so a factorisation passes through it
                            out = row == col ? 1.0 : 0.0;
                            if (row == col && g.dvec) g.dvec[row] = 1.0;
                        }
                        g.G[(long)row * g.mpad + col] = out;
                        if (row != col) g.G[(long)col * g.mpad + row] = g.mirror ? out : 0.0;
                    }
                }
        }
        __syncthreads();                               // Kt, Ct, Xt are rewritten by the next quadrant
    }
    if (neg) atomicAdd(reinterpret_cast<unsigned long long *>(g.nneg), (unsigned long long)neg);
}

// ---- Cholesky of the (mpad, mpad) matrix in place, right-looking by 64-column panels -------------------------------
constexpr size_t COV_DIAG_LDS = (size_t)(3 * NB * CH_LD + NB) * sizeof(double);
constexpr size_t COV_PANEL_LDS = (size_t)(2 * NB * CH_LD) * sizeof(double);

// block (j, j): L and L^-1 by chol64.hpp's factorisation; L goes back with zeros above the diagonal, the inverse to Dinv.
// The pivot rule is the fit's with each row's OWN diagonal entry of the matrix as the scale:
// a pivot whose square is <= 8 eps dvec[i], or not finite, fails; flag = first failing row + 1.
__global__ __launch_bounds__(256) void cov_chol_diag_kernel(double *__restrict__ G, int ld, int j, const double *__restrict__ dvec,
                                                            double *__restrict__ Dinv, int *__restrict__ flag) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double (*At)[CH_LD] = reinterpret_cast<double (*)[CH_LD]>(sm);
    double (*Xt)[CH_LD] = At + NB;
    double (*Tb)[CH_LD] = Xt + NB;
    double *scratch = sm + 3 * NB * CH_LD;
    __shared__ int sfirst;
    const int tid = threadIdx.x, o = j * NB;
    double *Gd = G + (long)o * ld + o;
    if (tid == 0) sfirst = NB;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        At[r][c] = Gd[(long)r * ld + c];
        Xt[r][c] = 0.0;
    }
    __syncthreads();
    factor64_v4(At, Xt, Tb, scratch, o, flag, 0.0);
    if (tid < NB) {
        const double l = At[tid][tid];
        const bool ok = (l * l > 8.0 * 2.220446049250313e-16 * dvec[o + tid]) && (l <= 1.3407807929942596e154);
        if (!ok) atomicMin(&sfirst, tid);
    }
    __syncthreads();
    if (tid == 0 && sfirst < NB && *flag == 0) *flag = o + sfirst + 1;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        Gd[(long)r * ld + c] = c <= r ? At[r][c] : 0.0;
        Dinv[e] = Xt[r][c];
    }
}

// block (i, j), i > j: A_ij <- A_ij L_jj^-T = A_ij Dinv^T, one workgroup per block
__global__ __launch_bounds__(256) void cov_chol_panel_kernel(double *__restrict__ G, int ld, int j, const double *__restrict__ Dinv) {
    extern __shared__ __attribute__((aligned(16))) double sm[];
    double (*As)[CH_LD] = reinterpret_cast<double (*)[CH_LD]>(sm);
    double (*Bs)[CH_LD] = As + NB;
    const int tid = threadIdx.x;
    double *Ga = G + (long)(j + 1 + blockIdx.x) * NB * ld + (long)j * NB;
    for (int e = tid; e < NB * NB; e += 256) {
        const int r = e >> 6, c = e & 63;
        As[r][c] = Ga[(long)r * ld + c];
        Bs[r][c] = Dinv[e];
    }
    __syncthreads();
    d4_t acc[2][2];
    acc_zero(acc);
    tile_mma64(As, Bs, acc);
    acc_foreach(acc, [&](int r, int c, double v) { Ga[(long)r * ld + c] = v; });
}

// E (Spad, mpad) = the normals (given, or drawn: Philox element s 4096 + j under COV_TAG), zero outside (S, m);
// Y (Spad, mpad) = mu broadcast, so that the product only has to add y_std E Lc^T
__global__ __launch_bounds__(256) void cov_eps_kernel(const double *__restrict__ eps_in, double *__restrict__ E, double *__restrict__ Y,
                                                      const double *__restrict__ mu, int S, int Spad, int m, int mpad,
                                                      unsigned long long seed) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)Spad * mpad) return;
    const int s = (int)(e / mpad), j = (int)(e % mpad);
    const bool live = s < S && j < m;
    double v = 0.0;
    if (live) v = eps_in ? eps_in[(long)s * m + j] : philox_normal((unsigned long long)s * COV_EPS_STRIDE + (unsigned long long)j, 0u, COV_TAG, seed);
    E[e] = v;
    Y[e] = live ? mu[j] : 0.0;
}

// ---- launchers -----------------------------------------------------------------------------------------------------
int64_t cov_ws_doubles(const Context &c, int64_t m, int64_t S, CovWs *out) {
    const int64_t mpad = (m + 127) / 128 * 128, Spad = (S + 127) / 128 * 128;
    const int64_t NV = (c.N + 127) / 128 * 128;          // <= Np: Np is a multiple of 256
    auto al = [](int64_t n) { return (n + 15) & ~(int64_t)15; };   // 128-byte regions: the DMA'd operands need 16 bytes
    int64_t off = 0;
    auto take = [&](int64_t n) { const int64_t o = off; off += al(n); return o; };
    CovWs w{};
    w.m = m; w.mpad = mpad; w.S = S; w.Spad = Spad; w.NV = NV;
    w.o_cnt = take(16);                                  // [0] negative diagonal entries, [1] the factorisation's flag
    w.o_Xq = take(m * c.D);
    w.o_Us = take(mpad * c.Dp);
    w.o_mu = take(mpad);
    w.o_dvec = take(mpad);
    w.o_Dinv = take(NB * NB);
    w.o_G = take(mpad * mpad);
    // Ks and Vt are dead once Sigma is formed: the samples' operands take their place
    const int64_t post = al(mpad * c.Np) + al(mpad * NV);
    const int64_t samp = S > 0 ? al(S * m) + 2 * al(Spad * mpad) : 0;
    w.o_Ks = off; w.o_Vt = off + al(mpad * c.Np);
    w.o_Ein = off; w.o_E = off + al(S * m); w.o_Y = w.o_E + al(Spad * mpad);
    off += post > samp ? post : samp;
    if (out) *out = w;
    return off;
}

// the first three steps of launch_cov_posterior for rows given on the DEVICE (kg_kernels.hip: the discretisation points,
// a chunk of the resident candidates): Us = Xq / l, Ks = c k0(Xq, X), and (mu != null) the raw mean
hipError_t launch_cov_cross(Context &c, const double *Xq, int m, int mpad, double *Us, double *Ks, double *mu, long long *cnt) {
    hipStream_t s = c.stream;
    const int N = (int)c.N, Np = (int)c.Np, D = (int)c.D, Dp = (int)c.Dp;
    hipLaunchKernelGGL(cov_scale_kernel, dim3((unsigned)(((long)mpad * Dp + 255) / 256)), dim3(256), 0, s, Xq, c.d_ls, Us, m, mpad, D, Dp, cnt);
    TGP_TRY(hipGetLastError());
    auto k = by_kind(c.kernel, [](auto K) { return cov_ks_kernel<K()>; });
    hipLaunchKernelGGL(k, dim3(Np / PW_T, mpad / PW_T), dim3(256), 0, s, Us, c.d_Xs, Ks, m, N, Np, Dp, c.constant);
    TGP_TRY(hipGetLastError());
    if (!mu) return hipSuccess;
    hipLaunchKernelGGL(cov_mu_kernel, dim3(mpad / 4), dim3(256), 0, s, Ks, c.d_alpha, mu, m, mpad, N, Np, c.y_mean, c.y_std);
    return hipGetLastError();
}

hipError_t launch_cov_posterior(Context &c, double *ws, const CovWs &w, int latent, double nugget, bool for_sample) {
    hipStream_t s = c.stream;
    const int m = (int)w.m, mpad = (int)w.mpad, N = (int)c.N, Np = (int)c.Np, D = (int)c.D, Dp = (int)c.Dp, NV = (int)w.NV;
    double *Us = ws + w.o_Us, *Ks = ws + w.o_Ks, *Vt = ws + w.o_Vt, *G = ws + w.o_G, *mu = ws + w.o_mu;
    long long *cnt = reinterpret_cast<long long *>(ws + w.o_cnt);
    hipLaunchKernelGGL(cov_scale_kernel, dim3((unsigned)(((long)mpad * Dp + 255) / 256)), dim3(256), 0, s, ws + w.o_Xq, c.d_ls, Us, m, mpad, D, Dp, cnt);
    TGP_TRY(hipGetLastError());
    {
        auto k = by_kind(c.kernel, [](auto K) { return cov_ks_kernel<K()>; });
        hipLaunchKernelGGL(k, dim3(Np / PW_T, mpad / PW_T), dim3(256), 0, s, Us, c.d_Xs, Ks, m, N, Np, Dp, c.constant);
        TGP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(cov_mu_kernel, dim3(mpad / 4), dim3(256), 0, s, Ks, c.d_alpha, mu, m, mpad, N, Np, c.y_mean, c.y_std);
    TGP_TRY(hipGetLastError());
    {
        // Vt[i][n] = sum_{k <= n} Ks[i][k] Linv[n][k]: B's rows are lower triangular, the k-range of column tile tn ends
        // with its diagonal tile -- the zero blocks right of it are never fetched
        GemmNtArgs g{};
        g.A = Ks; g.lda = Np; g.B = c.d_Linv; g.ldb = Np; g.C = Vt; g.ldc = NV; g.Ct = nullptr;
        g.ntm = mpad / 128; g.ntn = NV / 128; g.K = NV; g.alpha = 1.0; g.beta = 0.0;
        TGP_TRY((launch_gemm_nt_glds<double, KN_LOWER_B, TM_FULL>(s, c.device, g, g.ntm * g.ntn, 1)));
    }
    {
        CovSyrkArgs a{};
        a.Vt = Vt; a.Us = Us; a.G = G; a.dvec = for_sample ? ws + w.o_dvec : nullptr; a.nneg = cnt;
        a.m = m; a.mpad = mpad; a.NV = NV; a.Dp = Dp;
        a.constant = c.constant; a.diag_add = (latent ? 0.0 : c.noise) + (for_sample ? nugget : 0.0);
        a.scale = for_sample ? 1.0 : c.y_std * c.y_std;
        a.mirror = for_sample ? 0 : 1;
        auto k = by_kind(c.kernel, [](auto K) { return cov_syrk_kernel<K()>; });
        constexpr size_t lds = trmm_glds_lds_bytes();
        static LdsOptIn opt_in[4];
        TGP_TRY(opt_in[c.kernel & 3].ensure(reinterpret_cast<const void *>(k), c.device, lds));
        const int nt = mpad / 128;
        hipLaunchKernelGGL(k, dim3(nt * (nt + 1) / 2), dim3(256), lds, s, a);
        TGP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

hipError_t launch_cov_sample(Context &c, double *ws, const CovWs &w, bool draw, unsigned long long seed) {
    hipStream_t s = c.stream;
    const int m = (int)w.m, mpad = (int)w.mpad, S = (int)w.S, Spad = (int)w.Spad;
    double *G = ws + w.o_G, *Dinv = ws + w.o_Dinv, *E = ws + w.o_E, *Y = ws + w.o_Y;
    int *flag = reinterpret_cast<int *>(ws + w.o_cnt + 1);
    static LdsOptIn opt_diag, opt_panel;
    TGP_TRY(opt_diag.ensure(reinterpret_cast<const void *>(cov_chol_diag_kernel), c.device, COV_DIAG_LDS));
    TGP_TRY(opt_panel.ensure(reinterpret_cast<const void *>(cov_chol_panel_kernel), c.device, COV_PANEL_LDS));
    const int nb = (m + NB - 1) / NB;                    // live 64-blocks (the rest of mpad is an identity block)
    for (int j = 0; j < nb; ++j) {
        hipLaunchKernelGGL(cov_chol_diag_kernel, dim3(1), dim3(256), COV_DIAG_LDS, s, G, mpad, j, ws + w.o_dvec, Dinv, flag);
        TGP_TRY(hipGetLastError());
        const int below = nb - 1 - j;
        if (below == 0) break;
        hipLaunchKernelGGL(cov_chol_panel_kernel, dim3(below), dim3(256), COV_PANEL_LDS, s, G, mpad, j, Dinv);
        TGP_TRY(hipGetLastError());
        GemmArgs g{};
        g.A = G + (long)(j + 1) * NB * mpad + (long)j * NB; g.lda = mpad;
        g.B = g.A; g.ldb = mpad;
        g.C = G + (long)(j + 1) * NB * mpad + (long)(j + 1) * NB; g.ldc = mpad;
        g.Ct = nullptr;
        g.ntm = g.ntn = below; g.K = NB; g.alpha = -1.0; g.beta = 1.0;
        TGP_TRY((launch_gemm64_glds<KR_FULL, TM_LOWER>(s, c.device, g, below * (below + 1) / 2, 1)));
    }
    hipLaunchKernelGGL(cov_eps_kernel, dim3((unsigned)(((long)Spad * mpad + 255) / 256)), dim3(256), 0, s,
                       draw ? (const double *)nullptr : ws + w.o_Ein, E, Y, ws + w.o_mu, S, Spad, m, mpad, seed);
    TGP_TRY(hipGetLastError());
    // Y[s][j] += y_std sum_{k <= j} E[s][k] Lc[j][k]
    GemmNtArgs g{};
    g.A = E; g.lda = mpad; g.B = G; g.ldb = mpad; g.C = Y; g.ldc = mpad; g.Ct = nullptr;
    g.ntm = Spad / 128; g.ntn = mpad / 128; g.K = mpad; g.alpha = c.y_std; g.beta = 1.0;
    TGP_TRY((launch_gemm_nt_glds<double, KN_LOWER_B, TM_FULL>(s, c.device, g, g.ntm * g.ntn, 1)));
    return hipSuccess;
}

}  // namespace tgp
