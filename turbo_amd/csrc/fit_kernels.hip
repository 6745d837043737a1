// fit_kernels.hip -- GP fit on the GPU, all float64.
//
//   kernel matrix   sklearn/gaussian_process/kernels.py RBF :1553-1560, Matern :1708-1738,
//                   Product :966, Sum :866, WhiteKernel :1402; _gpr.py:346-347 (jitter)
//   Cholesky        _gpr.py:349 (scipy.linalg.cholesky -> LAPACK dpotrf): right-looking blocked
//                   factorisation, NB = 64: LDS diagonal-block potf2 (+ its inverse), MFMA panel
//                   solve, MFMA trailing update
//   inverse factor  Linv = L^-1 by recursive doubling on MFMA (feeds the candidate sweep, which
//                   replaces solve_triangular at _gpr.py:454 by a triangular contraction)
//   alpha, LML      _gpr.py:360-364 and :584-613
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <vector>
#include <stdio.h>
#include <math.h>
#include <stdlib.h>

#include "chol64.hpp"
#include "gemm64_glds.hpp"
#include "gemm_nt_glds.hpp"
#include "mfma_gemm.hpp"
#include "pairwise.hpp"
#include <string.h>

#include "tgp_internal.hpp"

namespace tgp {

#define TGP_TRY(x)                         \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

// ------------------------------------------------------------------------------------------
// Kernel matrix: the 64x64 tiles on and below the diagonal (nothing reads the ones above it).
// Padding rows/cols (>= N) form an identity block so the padded factor is [[L,0],[0,I]].
// ------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(256) void kernel_matrix_kernel(
    const double *__restrict__ Xs, double *__restrict__ K, int N, int Np, int Dp,
    double constant, double noise, double jitter) {
    __shared__ double Ct[PwCfg<double>::DC][PwCfg<double>::LD];
    __shared__ double Xt[PwCfg<double>::DC][PwCfg<double>::LD];
    int bx = blockIdx.x;
    int tm = (int)((sqrtf(8.0f * (float)bx + 1.0f) - 1.0f) * 0.5f);
    while ((tm + 1) * (tm + 2) / 2 <= bx) ++tm;
    while (tm * (tm + 1) / 2 > bx) --tm;
    const int tn = bx - tm * (tm + 1) / 2;
    const int i0 = tm * PW_T, j0 = tn * PW_T;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;

    double d2[4][4];
    pairwise_sqdist<double>(Xs, i0, Np, Xs, j0, Np, Dp, Ct, Xt, d2);

#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + 4 * ty + a;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + 4 * tx + b;
            double v;
            if (i == j) {
                // np.fill_diagonal(K, 1); constant * K; + noise; + jitter
                v = (i < N) ? ((constant * 1.0 + noise) + jitter) : 1.0;
            } else if (i < N && j < N) {
                v = kernel_value<double, KIND>(d2[a][b], constant);
            } else {
                v = 0.0;
            }
            K[(long)i * Np + j] = v;   // tiles above the diagonal are never read: left unwritten
        }
    }
}

// Diagonal block (factor + inverse) of panel o and, in the same launch, the panel solve of every
// row block below it.  VAR selects the factorisation: 4 / 8 = variant B with that many columns
// per barrier (4 is the default), 0 = variant A (the round-1 form, kept for A/B runs).
template <int VAR>
__global__ __launch_bounds__(256) void panel_kernel(double *__restrict__ K, int Np, int o,
                                                        double *__restrict__ Dinv,
                                                        double *__restrict__ Linv,
                                                        double *__restrict__ Lstage,
                                                        double *__restrict__ scal,
                                                        int *__restrict__ flag, double tiny) {
    // one LDS arena: the factorisation's column / row buffers, later the panel solve's two
    // 64 x 66 operand tiles
    __shared__ __attribute__((aligned(16))) double panel_lds[2 * NB * (NB + 2)];
    double *logs = panel_lds + 4 * 8 * NB;
    const int tid = threadIdx.x;
    const int tc = tid >> 4, tr = tid & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // holds tc = 4*wave .. 4*wave+3
    double a[4][4], x[4][4];
    const double *src = K + (long)(o + 4 * tr) * Np + o + 4 * tc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const d2_t v0 = *reinterpret_cast<const d2_t *>(src + (long)i * Np);
        const d2_t v1 = *reinterpret_cast<const d2_t *>(src + (long)i * Np + 2);
        a[i][0] = v0[0]; a[i][1] = v0[1]; a[i][2] = v1[0]; a[i][3] = v1[1];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[i][j] = (tr == tc && i == j) ? 1.0 : 0.0;
    }
    // Workgroup 0 publishes L_kk.  The other workgroups of this launch READ A_kk from K(o, o)
    // whenever they happen to be dispatched, so L_kk must not land there before the launch is
    // over: it is parked in Lstage[k] and moved into K by workgroup 0 of the NEXT panel's launch
    // (stream order = all readers done).  The last panel runs alone (gridDim.x == 1) and writes
    // in place.
    const bool alone = gridDim.x == 1;
    // row blocks below the diagonal: fetch the A_ik tile now, so its latency hides behind the
    // factorisation (it is only needed by the panel solve at the end)
    double *Ablk = K + (long)(o + NB * blockIdx.x) * Np + o;
    d2_t apre[8];
    if (blockIdx.x > 0) {
#pragma unroll
        for (int p8 = 0; p8 < 8; ++p8) {
            const int idx = tid + 256 * p8;
            apre[p8] = *reinterpret_cast<const d2_t *>(Ablk + (long)(idx >> 5) * Np + (idx & 31) * 2);
        }
    }
    if (VAR == 3 || VAR == 38) {
        double *Ldst = nullptr;
        if (blockIdx.x == 0) Ldst = alone ? K + (long)o * Np + o : Lstage + (long)(o / NB) * NB * NB;
        if (VAR == 38) factor64_v3<8>(a, panel_lds, o, Ldst, alone ? (long)Np : (long)NB, flag, tiny);
        else factor64_v3<4>(a, panel_lds, o, Ldst, alone ? (long)Np : (long)NB, flag, tiny);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) x[i][j] = a[i][j];          // the live tile ended as the X tile
    } else if (VAR == 8) {
        factor64_steps<8>(a, x, panel_lds, o, flag, tiny);
    } else if (VAR == 4) {
        factor64_steps<4>(a, x, panel_lds, o, flag, tiny);
    } else {
        factor64_steps4(a, x, panel_lds, o, flag, tiny);
    }
    if (blockIdx.x > 0) {
        // ---- panel solve for row block blockIdx.x - 1 below the diagonal: L_ik = A_ik * X^T ----
        // (every workgroup of the launch factored the diagonal block redundantly above, so X is
        // already in this workgroup's registers; no second launch, no round trip through HBM)
        constexpr int LDP = NB + 2;
        double (*As)[LDP] = reinterpret_cast<double (*)[LDP]>(panel_lds);
        double (*Xs)[LDP] = As + NB;
        __syncthreads();   // colbuf/xbuf (aliased by panel_lds) are no longer read
#pragma unroll
        for (int p8 = 0; p8 < 8; ++p8) {
            const int idx = tid + 256 * p8;
            *reinterpret_cast<d2_t *>(&As[idx >> 5][(idx & 31) * 2]) = apre[p8];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                Xs[4 * tr + i][4 * tc + j] = ((4 * tc + j) <= (4 * tr + i)) ? x[i][j] : 0.0;
        __syncthreads();
        // 4 waves, each a 32x32 quadrant of the 64x64 block: 2x2 fragments of v_mfma_f64_16x16x4
        using MF = Mfma<double>;
        const int lane = tid & 63;
        const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
        const int fidx = MF::ab_idx(lane), fkg = MF::ab_kg(lane) * 2;
        d4_t acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
#pragma unroll
        for (int ks = 0; ks < NB; ks += 8) {
            d2_t av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const d2_t *>(&As[wm0 + 16 * i + fidx][ks + fkg]);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const d2_t *>(&Xs[wn0 + 16 * j + fidx][ks + fkg]);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = MF::mma(av[i][e], bv[j][e], acc[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Ablk[(long)(wm0 + 16 * i + MF::c_row(lane, r)) * Np + wn0 + 16 * j + MF::c_col(lane)] = acc[i][j][r];
        return;
    }
    // Workgroup 0 publishes the result: X to Dinv[k] and to the diagonal of Linv, L_kk (zeros above
    // the diagonal) to K or Lstage (see the top of the kernel).
    double *dstK = alone ? K + (long)(o + 4 * tr) * Np + o + 4 * tc
                         : Lstage + (long)(o / NB) * NB * NB + (4 * tr) * NB + 4 * tc;
    const long ldK = alone ? (long)Np : (long)NB;
    double *dstL = Linv + (long)(o + 4 * tr) * Np + o + 4 * tc;
    double *dstD = Dinv + (long)(o / NB) * NB * NB + (4 * tr) * NB + 4 * tc;
    if (o > 0) {   // the previous panel's parked L_kk
        const double *prev = Lstage + (long)(o / NB - 1) * NB * NB + (4 * tr) * NB + 4 * tc;
        double *pk = K + (long)(o - NB + 4 * tr) * Np + (o - NB) + 4 * tc;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) pk[(long)i * Np + j] = prev[i * NB + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool low = (4 * tc + j) <= (4 * tr + i);
            if (VAR != 3 && VAR != 38) dstK[(long)i * ldK + j] = low ? a[i][j] : 0.0;   // variant C stored L during the loop
            const double xv = low ? x[i][j] : 0.0;
            dstL[(long)i * Np + j] = xv;
            dstD[i * NB + j] = xv;
        }
    // sum(log(diag L)) of this block, fixed-order tree in one wave
    if (VAR == 3 || VAR == 38) {
        // variant C left 1 / L[j][j] in LDS: log L[j][j] = -log(rs[j])
        __syncthreads();
        if (tid < 64) {
            double s = -log(panel_lds[CHOL64_RS_OFF + tid]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
            if (tid == 0) scal[0] += s;
        }
        return;
    }
    if (tr == tc) logs[tr] = (log(a[0][0]) + log(a[1][1])) + (log(a[2][2]) + log(a[3][3]));
    __syncthreads();
    if (tid < 64) {
        double s = tid < 16 ? logs[tid] : 0.0;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (tid == 0) scal[0] += s;
    }
}

// Panel kernel on variant D of the diagonal-block factorisation (chol64.hpp: block in LDS, one wave
// factors + inverts 16 x 16 pivot blocks, MFMA for the rest).  Same contract as panel_kernel.
__global__ __launch_bounds__(256) void panel_d_kernel(double *__restrict__ K, int Np, int o,
                                                      double *__restrict__ Dinv,
                                                      double *__restrict__ Linv,
                                                      double *__restrict__ Lstage,
                                                      double *__restrict__ scal,
                                                      int *__restrict__ flag, double tiny) {
    __shared__ __attribute__((aligned(16))) double lds[3 * NB * CH_LD + NB + 32];
    double (*At)[CH_LD] = reinterpret_cast<double (*)[CH_LD]>(lds);
    double (*Xt)[CH_LD] = At + NB;
    double (*Tb)[CH_LD] = Xt + NB;
    double *rsbuf = lds + 3 * NB * CH_LD;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool alone = gridDim.x == 1;          // see panel_kernel: where L_kk may be written
    const d2_t z2 = {0.0, 0.0};
    const double *Akk = K + (long)o * Np + o;
#pragma unroll
    for (int p8 = 0; p8 < 8; ++p8) {
        const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
        *reinterpret_cast<d2_t *>(&At[r][c2]) = *reinterpret_cast<const d2_t *>(Akk + (long)r * Np + c2);
        *reinterpret_cast<d2_t *>(&Xt[r][c2]) = z2;
    }
    double *Ablk = K + (long)(o + NB * blockIdx.x) * Np + o;
    d2_t apre[8];
    if (blockIdx.x > 0) {   // the A_ik tile of this workgroup's row block, fetched behind the factorisation
#pragma unroll
        for (int p8 = 0; p8 < 8; ++p8) {
            const int idx = tid + 256 * p8;
            apre[p8] = *reinterpret_cast<const d2_t *>(Ablk + (long)(idx >> 5) * Np + (idx & 31) * 2);
        }
    }
    __syncthreads();
    factor64_v4(At, Xt, Tb, rsbuf, o, flag, tiny);
    if (blockIdx.x > 0) {
        // ---- panel solve: L_ik = A_ik X^T, X already sits in LDS ----
#pragma unroll
        for (int p8 = 0; p8 < 8; ++p8) {
            const int idx = tid + 256 * p8;
            *reinterpret_cast<d2_t *>(&Tb[idx >> 5][(idx & 31) * 2]) = apre[p8];
        }
        __syncthreads();
        using MF = Mfma<double>;
        const int lane = tid & 63;
        const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
        const int fidx = MF::ab_idx(lane), fkg = MF::ab_kg(lane) * 2;
        d4_t acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
#pragma unroll
        for (int ks = 0; ks < NB; ks += 8) {
            d2_t av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const d2_t *>(&Tb[wm0 + 16 * i + fidx][ks + fkg]);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const d2_t *>(&Xt[wn0 + 16 * j + fidx][ks + fkg]);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = MF::mma(av[i][e], bv[j][e], acc[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    Ablk[(long)(wm0 + 16 * i + MF::c_row(lane, r)) * Np + wn0 + 16 * j + MF::c_col(lane)] = acc[i][j][r];
        return;
    }
    // ---- workgroup 0 publishes: L_kk (zeros above the diagonal) to K or Lstage, X to Dinv and Linv ----
    double *dstK = alone ? K + (long)o * Np + o : Lstage + (long)(o / NB) * NB * NB;
    const long ldK = alone ? (long)Np : (long)NB;
    double *dstL = Linv + (long)o * Np + o;
    double *dstD = Dinv + (long)(o / NB) * NB * NB;
    const double *prev = Lstage + (long)(o / NB - 1) * NB * NB;
    double *pk = K + (long)(o - NB) * Np + (o - NB);
#pragma unroll
    for (int p8 = 0; p8 < 8; ++p8) {
        const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
        if (o > 0)   // the previous panel's parked L_kk
            *reinterpret_cast<d2_t *>(pk + (long)r * Np + c2) = *reinterpret_cast<const d2_t *>(prev + r * NB + c2);
        d2_t lv = *reinterpret_cast<const d2_t *>(&At[r][c2]);
        lv[0] = (c2 <= r) ? lv[0] : 0.0;
        lv[1] = (c2 + 1 <= r) ? lv[1] : 0.0;
        *reinterpret_cast<d2_t *>(dstK + (long)r * ldK + c2) = lv;
        const d2_t xv = *reinterpret_cast<const d2_t *>(&Xt[r][c2]);
        *reinterpret_cast<d2_t *>(dstL + (long)r * Np + c2) = xv;
        *reinterpret_cast<d2_t *>(dstD + r * NB + c2) = xv;
    }
    if (tid < 64) {   // sum(log(diag L)), fixed-order tree
        double s = log(At[tid][tid]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (tid == 0) scal[0] += s;
    }
}

// z[i] = sum_{j<=i} Linv[i][j] * v[j]   (one wave per row)
__global__ __launch_bounds__(256) void gemv_lower_rows_kernel(const double *__restrict__ Linv,
                                                              const double *__restrict__ v,
                                                              double *__restrict__ z, int Np) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= Np) return;
    double s = 0.0;
    const double *row = Linv + (long)i * Np;
    for (int jj = lane; jj <= i; jj += 64) s = fma(row[jj], v[jj], s);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) z[i] = s;
}

// partial[y][j] = sum over the y-th row slice of Linv[i][j] * z[i], i >= j
// (64 columns x GEMV_RS row slices per grid; 4 row lanes per column inside a block)
constexpr int GEMV_RS = 16;
__global__ __launch_bounds__(256) void gemv_lower_cols_kernel(const double *__restrict__ Linv,
                                                              const double *__restrict__ z,
                                                              double *__restrict__ partial, int Np) {
    __shared__ double red[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int j0 = blockIdx.x * 64, j = j0 + c;
    const int rows = Np - j0;                       // rows j0 .. Np-1 can be non-zero
    const int per = (rows + GEMV_RS - 1) / GEMV_RS;
    const int i0 = j0 + blockIdx.y * per;
    const int i1 = (i0 + per < Np) ? i0 + per : Np;
    double s = 0.0;
    for (int i = i0 + rg; i < i1; i += 4)
        if (i >= j) s = fma(Linv[(long)i * Np + j], z[i], s);
    red[rg][c] = s;
    __syncthreads();
    if (rg == 0) partial[(long)blockIdx.y * Np + j] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

// alpha[j] = sum_y partial[y][j] (fixed order);  scal[1] = yn . alpha   (single block)
__global__ __launch_bounds__(256) void alpha_finish_kernel(const double *__restrict__ partial,
                                                           const double *__restrict__ yn,
                                                           double *__restrict__ alpha,
                                                           double *__restrict__ scal, int Np,
                                                           const int *__restrict__ flag = nullptr,
                                                           double *__restrict__ res_host = nullptr) {
    __shared__ double red[256];
    double d = 0.0;
    for (int j = threadIdx.x; j < Np; j += 256) {
        double a = 0.0;
#pragma unroll
        for (int y = 0; y < GEMV_RS; ++y) a += partial[(long)y * Np + j];
        alpha[j] = a;
        d = fma(yn[j], a, d);
    }
    red[threadIdx.x] = d;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        scal[1] = red[0];
        if (res_host) {   // device-mapped host memory: the fit's scalars land there without a D2H copy
            res_host[0] = scal[0];
            res_host[1] = red[0];
            res_host[2] = (double)*flag;
        }
    }
}

// ---- the same two products taken row block by row block (the inverse behind the panel chain) ----
// z[i] = sum_{j<=i} Linv[i][j] * v[j] for the rows from row0 on (one workgroup per row, four loads in
// flight per lane) and, for an f32 sweep, the f32 copy of that row (all Np columns: the zeros right of
// the diagonal included)
__global__ __launch_bounds__(256) void rowblock_finish_kernel(const double *__restrict__ Linv,
                                                              const double *__restrict__ v,
                                                              double *__restrict__ z,
                                                              float *__restrict__ Linv32, int Np, int row0) {
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = row0 + blockIdx.x;
    const double *row = Linv + (long)i * Np;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int jj = tid;
    for (; jj + 768 <= i; jj += 1024) {
        const double a0 = row[jj], a1 = row[jj + 256], a2 = row[jj + 512], a3 = row[jj + 768];
        s0 = fma(a0, v[jj], s0);
        s1 = fma(a1, v[jj + 256], s1);
        s2 = fma(a2, v[jj + 512], s2);
        s3 = fma(a3, v[jj + 768], s3);
    }
    for (; jj <= i; jj += 256) s0 = fma(row[jj], v[jj], s0);
    double s = (s0 + s1) + (s2 + s3);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) red[tid >> 6] = s;
    if (Linv32) {
        float *o = Linv32 + (long)i * Np;
        for (int j2 = tid * 2; j2 < Np; j2 += 512) {
            const d2_t x = *reinterpret_cast<const d2_t *>(row + j2);
            float2 y;
            y.x = (float)x[0];
            y.y = (float)x[1];
            *reinterpret_cast<float2 *>(o + j2) = y;
        }
    }
    __syncthreads();
    if (tid == 0) z[i] = (red[0] + red[1]) + (red[2] + red[3]);
}

// partial[s][j] = sum over the 128-row slice s = i / 128 of Linv[i][j] * z[i], i >= j  (64 columns per
// workgroup, blockIdx.y = slice inside the row block that starts at row0); zsq[s] = sum of z[i]^2
// over the slice (yn . alpha = z . z)
constexpr int GEMV_SLICE = 128;
__global__ __launch_bounds__(256) void rowblock_cols_kernel(const double *__restrict__ Linv,
                                                            const double *__restrict__ z,
                                                            double *__restrict__ partial,
                                                            double *__restrict__ zsq, int Np, int row0) {
    __shared__ double red[4][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    const int i0 = row0 + blockIdx.y * GEMV_SLICE;
    const double *col = Linv + j;
    double s0 = 0.0, s1 = 0.0;
#pragma unroll
    for (int q = 0; q < GEMV_SLICE / 4; q += 8) {   // rows i0 + rg + 4 (q + u): eight loads in flight
        double a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = i0 + rg + 4 * (q + u);
            a[u] = (i >= j) ? col[(long)i * Np] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            s0 = fma(a[u], z[i0 + rg + 4 * (q + u)], s0);
            s1 = fma(a[u + 1], z[i0 + rg + 4 * (q + u + 1)], s1);
        }
    }
    red[rg][c] = s0 + s1;
    __syncthreads();
    if (rg == 0) partial[(long)(i0 / GEMV_SLICE) * Np + j] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    if (blockIdx.x == 0 && threadIdx.x < 64) {   // fixed-order tree over the slice's 128 rows
        const double za = z[i0 + threadIdx.x], zb = z[i0 + 64 + threadIdx.x];
        double q = fma(za, za, zb * zb);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
        if (threadIdx.x == 0) zsq[i0 / GEMV_SLICE] = q;
    }
}

// alpha[j] = sum of partial[s][j] over the slices that reach column j, s = j / 128 ... (fixed order:
// four interleaved groups of slices, then the groups); workgroup 0 also leaves scal[1] = yn . alpha
// = z . z = sum of zsq (fixed order) and the fit's scalars
__global__ __launch_bounds__(256) void alpha_finish_sliced_kernel(const double *__restrict__ partial,
                                                                  const double *__restrict__ zsq,
                                                                  double *__restrict__ alpha,
                                                                  double *__restrict__ scal, int Np,
                                                                  const int *__restrict__ flag,
                                                                  double *__restrict__ res_host) {
    __shared__ double red[4][64];
    const int ns = Np / GEMV_SLICE;
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    double a = 0.0;
    for (int y = j / GEMV_SLICE + rg; y < ns; y += 4) a += partial[(long)y * Np + j];
    red[rg][c] = a;
    __syncthreads();
    if (rg == 0) alpha[j] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        double d = 0.0;
        for (int y = threadIdx.x; y < ns; y += 64) d += zsq[y];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) d += __shfl_xor(d, off, 64);
        if (threadIdx.x == 0) {
            scal[1] = d;
            if (res_host) {
                res_host[0] = scal[0];
                res_host[1] = d;
                res_host[2] = (double)*flag;
            }
        }
    }
}

// U[blk] = Linv[blk]^T for every 128x128 diagonal block (32x32 LDS tiles)
__global__ __launch_bounds__(256) void transpose_diag128_kernel(const double *__restrict__ Linv,
                                                                double *__restrict__ U, int Np) {
    __shared__ double t[32][33];
    const int blk = blockIdx.x, tile = blockIdx.y;          // 16 tiles per block
    const int tr = tile >> 2, tc = tile & 3;
    const long base = (long)blk * 128 * ((long)Np + 1);
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;   // 32 x 8
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = y + 8 * k;
        t[r][x] = Linv[base + (long)(32 * tr + r) * Np + 32 * tc + x];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = y + 8 * k;
        U[base + (long)(32 * tc + r) * Np + 32 * tr + x] = t[x][r];
    }
}

// The 64 -> 128 level of the inverse in ONE launch (round 5; it was three: two 64 x 64 products on the generic template
// and the transpose): workgroup b takes the 128-block at row o + 128 b,
//     T = L21 X11,   Linv21 = -X22 T,   U[block] = Linv[block]^T
// with the tiles in LDS and the products on tile_mma64 (the template's k order: the same bits).  Saves two launches
// (~12 us) per fit where the inverse is not hidden behind the panel chain (Np <= 512: every evaluation of a mid-size
// hyper-parameter fit, C1).
__global__ __launch_bounds__(256) void level64_fused_kernel(const double *__restrict__ K, double *__restrict__ Linv,
                                                            double *__restrict__ U, int Np, long o) {
    __shared__ __attribute__((aligned(16))) double lds[3 * NB * CH_LD];
    typedef double (*tile_t)[CH_LD];
    tile_t A = reinterpret_cast<tile_t>(lds), B = A + NB, Tt = B + NB;
    const int tid = threadIdx.x;
    const long d = (o + (long)blockIdx.x * 2 * NB) * ((long)Np + 1);
    const double *L21 = K + d + (long)NB * Np;
    const double *X11 = Linv + d;
    const double *X22 = Linv + d + (long)NB * Np + NB;
    double *Ub = U + d;
    // A = L21 [i][k];  B[j][k] = X11[k][j] (= U11[j][k]: stored as the block's upper-left tile of U on the way)
#pragma unroll
    for (int p8 = 0; p8 < 8; ++p8) {
        const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
        *reinterpret_cast<d2_t *>(&A[r][c2]) = *reinterpret_cast<const d2_t *>(L21 + (long)r * Np + c2);
        const d2_t v = *reinterpret_cast<const d2_t *>(X11 + (long)r * Np + c2);
        B[c2][r] = v[0];
        B[c2 + 1][r] = v[1];
    }
    __syncthreads();
    d4_t acc[2][2];
    acc_zero(acc);
    tile_mma64(A, B, acc);                                   // T[i][j] = sum_k L21[i][k] X11[k][j]
#pragma unroll
    for (int p8 = 0; p8 < 8; ++p8) {                         // U11 = X11^T, and zeros below it (the transpose of Linv's zero upper-right tile)
        const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
        *reinterpret_cast<d2_t *>(Ub + (long)r * Np + c2) = *reinterpret_cast<const d2_t *>(&B[r][c2]);
        const d2_t z = {0.0, 0.0};
        *reinterpret_cast<d2_t *>(Ub + (long)(NB + r) * Np + c2) = z;
    }
    acc_foreach(acc, [&](int r, int c, double v) { Tt[c][r] = v; });   // T^T: the second product's B operand, [j][k] = T[k][j]
    __syncthreads();                                         // A's readers are done, Tt is complete
#pragma unroll
    for (int p8 = 0; p8 < 8; ++p8) {
        const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
        *reinterpret_cast<d2_t *>(&A[r][c2]) = *reinterpret_cast<const d2_t *>(X22 + (long)r * Np + c2);
    }
    __syncthreads();
    acc_zero(acc);
    tile_mma64(A, Tt, acc);                                  // (X22 T)[i][j]
    double *L21inv = Linv + d + (long)NB * Np;
    acc_foreach(acc, [&](int r, int c, double v) {
        L21inv[(long)r * Np + c] = -v;                       // Linv21
        Ub[(long)c * Np + NB + r] = -v;                      // ... and its transpose, the block's upper-right tile of U
    });
    for (int idx = tid; idx < NB * NB; idx += 256) {         // U22 = X22^T
        const int r = idx >> 6, c = idx & 63;
        Ub[(long)(NB + r) * Np + NB + c] = A[c][r];
    }
}

__global__ void f64_to_f32_kernel(const double *__restrict__ in, float *__restrict__ out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = (float)in[i];
}

hipError_t launch_f64_to_f32(Context &c, const double *in, float *out, long n) {
    if (n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<long>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(f64_to_f32_kernel, dim3(blocks), dim3(256), 0, c.stream, in, out, n);
    return hipGetLastError();
}

// ---- one-row append: K' = [[K, k], [k^T, kappa]] ------------------------------------
// k[j] = c * k0(x_new, x_j) for j < n_old, 0 beyond
template <int KIND>
__global__ __launch_bounds__(256) void kvec_kernel(const double *__restrict__ Xs, double *__restrict__ k,
                                                   int n_old, int Np, int Dp, double constant) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Np) return;
    double v = 0.0;
    if (j < n_old) {
        const double *xn = Xs + (long)n_old * Dp;
        const double *xj = Xs + (long)j * Dp;
        double d2 = 0.0;
        for (int d = 0; d < Dp; ++d) {
            const double df = xn[d] - xj[d];
            d2 = fma(df, df, d2);
        }
        v = kernel_value<double, KIND>(d2, constant);
    }
    k[j] = v;
}

// pivot of the new row: lambda^2 = kappa - l.l ; writes L row, scal[2] = 1/lambda, scal[3] = log(lambda)
__global__ __launch_bounds__(256) void append_pivot_kernel(const double *__restrict__ l,
                                                           double *__restrict__ K, double *__restrict__ scal,
                                                           int *__restrict__ flag, int n_old, int Np,
                                                           double kappa, double tiny) {
    __shared__ double red[256];
    double s = 0.0;
    for (int j = threadIdx.x; j < n_old; j += 256) s = fma(l[j], l[j], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    double piv = kappa - red[0];
    if (!(piv > tiny) || !isfinite(piv)) {
        if (threadIdx.x == 0) *flag = n_old + 1;
        piv = 1.0;
    }
    const double lam = sqrt(piv);
    double *row = K + (long)n_old * Np;
    for (int j = threadIdx.x; j < Np; j += 256) row[j] = (j < n_old) ? l[j] : (j == n_old ? lam : 0.0);
    if (threadIdx.x == 0) { scal[2] = 1.0 / lam; scal[3] = log(lam); }
}

// Linv row n_old = [-(Linv^T l) / lambda, 1 / lambda, 0...] from the column partials
__global__ __launch_bounds__(256) void append_inv_row_kernel(const double *__restrict__ partial,
                                                             const double *__restrict__ scal,
                                                             double *__restrict__ Linv,
                                                             float *__restrict__ Linv32,
                                                             const double *__restrict__ Xs,
                                                             float *__restrict__ Xs32, int n_old, int Np,
                                                             int Dp) {
    const double rl = scal[2];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < Np; j += gridDim.x * 256) {
        double v = 0.0;
        if (j < n_old) {
            double a = 0.0;
#pragma unroll
            for (int y = 0; y < GEMV_RS; ++y) a += partial[(long)y * Np + j];
            v = -a * rl;
        } else if (j == n_old) {
            v = rl;
        }
        Linv[(long)n_old * Np + j] = v;
        if (Linv32) Linv32[(long)n_old * Np + j] = (float)v;
        if (Xs32 && j < Dp) Xs32[(long)n_old * Dp + j] = (float)Xs[(long)n_old * Dp + j];
    }
}

hipError_t launch_fit_append(Context &c, int n_old) {
    hipStream_t s = c.stream;
    const int Np = (int)c.Np, Dp = (int)c.Dp;
    TGP_TRY(hipMemsetAsync(c.d_flag, 0, sizeof(int), s));
    const dim3 kg((Np + 255) / 256);
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return kvec_kernel<K()>; }), kg, dim3(256), 0, s, c.d_Xs, c.d_t1, n_old, Np, Dp, c.constant);
    TGP_TRY(hipGetLastError());
    // l = Linv k  (the new row of L), then its pivot
    hipLaunchKernelGGL(gemv_lower_rows_kernel, dim3((Np + 3) / 4), dim3(256), 0, s, c.d_Linv, c.d_t1, c.d_t2, Np);
    TGP_TRY(hipGetLastError());
    const double kappa = (c.constant * 1.0 + c.noise) + c.jitter;
    const double tiny = 8.0 * 2.220446049250313e-16 * kappa;
    hipLaunchKernelGGL(append_pivot_kernel, dim3(1), dim3(256), 0, s, c.d_t2, c.d_K, c.d_scal, c.d_flag, n_old, Np, kappa, tiny);
    TGP_TRY(hipGetLastError());
    // new row of Linv = [-(Linv^T l) / lambda, 1 / lambda]
    hipLaunchKernelGGL(gemv_lower_cols_kernel, dim3(Np / 64, GEMV_RS), dim3(256), 0, s, c.d_Linv, c.d_t2, c.d_W, Np);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(append_inv_row_kernel, dim3(16), dim3(256), 0, s, c.d_W, c.d_scal, c.d_Linv,
                       c.dtype != TGP_F64 ? c.d_Linv32 : nullptr, c.d_Xs, c.dtype != TGP_F64 ? c.d_Xs32 : nullptr,
                       n_old, Np, Dp);
    TGP_TRY(hipGetLastError());
    // alpha = Linv^T (Linv yn) with the re-normalised targets, yn . alpha
    hipLaunchKernelGGL(gemv_lower_rows_kernel, dim3((Np + 3) / 4), dim3(256), 0, s, c.d_Linv, c.d_yn, c.d_z, Np);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gemv_lower_cols_kernel, dim3(Np / 64, GEMV_RS), dim3(256), 0, s, c.d_Linv, c.d_z, c.d_W, Np);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(alpha_finish_kernel, dim3(1), dim3(256), 0, s, c.d_W, c.d_yn, c.d_alpha, c.d_scal, Np, nullptr, nullptr);
    TGP_TRY(hipGetLastError());
    return hipSuccess;
}

// ------------------------------------------------------------------------------------------
template <int BM, int BN, bool BK_MAJOR, int KR, int TMAP>
static hipError_t launch_gemm64(hipStream_t s, int device, const GemmArgs &g, int nblocks, int batch) {
    constexpr int BK = 16;
    // every NT product (both operands K-contiguous) goes to the direct-to-LDS kernel of gemm64_glds.hpp (round 4);
    // TGP_GEMM64=reg keeps the register-staged template (A/B; same k order, bit-identical results).  The two NN
    // products of the inverse's 64 -> 128 level (K = 64) stay on the template.
    // A debug build (make debug: -DTGP_DEBUG_KERNELS, libturbogp_dbg.so -- never the shipped library) adds the
    // routes tools/repeat_fit.py bisected the k-loop race with: reg-trail / glds-trail = only the trailing update on
    // the template / on the direct-to-LDS kernel; wait0 = its barriers drain every DMA; round4-war = its k-loop as it
    // was before the LDS reads were awaited in front of the barrier (one fit in ten wrong at N = 5000).
    if constexpr (BK_MAJOR && BM == 64 && BN == 64 && (KR == KR_FULL || KR == KR_LOWER_A || KR == KR_UPPER_A)) {
        bool reg = tuning().gemm64_reg;
#ifdef TGP_DEBUG_KERNELS
        static const char *sel = getenv("TGP_GEMM64") ? getenv("TGP_GEMM64") : "";
        constexpr bool trail = KR == KR_FULL && TMAP == TM_LOWER;
        reg = reg || (!strcmp(sel, "reg-trail") && trail) || (!strcmp(sel, "glds-trail") && !trail);
        if (!reg && !strcmp(sel, "wait0")) return launch_gemm64_glds<KR, TMAP, 3, 4>(s, device, g, nblocks, batch);
        if (!reg && !strcmp(sel, "round4-war")) return launch_gemm64_glds<KR, TMAP, 3, 5>(s, device, g, nblocks, batch);
#endif
        if (!reg) return launch_gemm64_glds<KR, TMAP>(s, device, g, nblocks, batch);
    }
    auto kern = mfma_gemm_kernel<double, BM, BN, BK, BK_MAJOR, KR, TMAP, EP_STORE>;
    constexpr size_t lds = gemm_lds_bytes<double, BM, BN, BK>();
    static LdsOptIn opt_in;
    TGP_TRY(opt_in.ensure(reinterpret_cast<const void *>(kern), device, lds));
    hipLaunchKernelGGL(kern, dim3(nblocks, 1, batch), dim3(256), lds, s, g);
    return hipGetLastError();
}

// Rank-64 update inside an outer block: A[i][j] -= L_ik * L_jk^T for the row blocks i below panel k
// and the ncol column blocks j right of it (j <= i; tiles above the diagonal are skipped).  One
// 64 x 64 tile per workgroup, both 64 x 64 operands fetched in one round trip, 16 MFMA k-steps.
// The generic template spends most of its ~12 us on pipeline prologue for so short a k-range.
constexpr int R64_LDP = NB + 2;
__device__ __forceinline__ void rank64_tile(double *__restrict__ K, int Np, int o, int bi, int bj,
                                            double (*As)[R64_LDP], double (*Bs)[R64_LDP]) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double *A = K + (long)(o + NB * (1 + bi)) * Np + o;
    const double *B = K + (long)(o + NB * (1 + bj)) * Np + o;
    double *C = K + (long)(o + NB * (1 + bi)) * Np + o + NB * (1 + bj);
    d2_t ra[8], rb[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int idx = tid + 256 * p;
        ra[p] = *reinterpret_cast<const d2_t *>(A + (long)(idx >> 5) * Np + (idx & 31) * 2);
        rb[p] = *reinterpret_cast<const d2_t *>(B + (long)(idx >> 5) * Np + (idx & 31) * 2);
    }
    using MF = Mfma<double>;
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    d4_t acc[2][2];   // starts as the old C tile: the MFMAs then subtract in place
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                acc[i][j][r] = C[(long)(wm0 + 16 * i + MF::c_row(lane, r)) * Np + wn0 + 16 * j + MF::c_col(lane)];
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int idx = tid + 256 * p;
        *reinterpret_cast<d2_t *>(&As[idx >> 5][(idx & 31) * 2]) = ra[p];
        *reinterpret_cast<d2_t *>(&Bs[idx >> 5][(idx & 31) * 2]) = rb[p];
    }
    __syncthreads();
    const int fidx = MF::ab_idx(lane), fkg = MF::ab_kg(lane) * 2;
#pragma unroll
    for (int ks = 0; ks < NB; ks += 8) {
        d2_t av[2], bv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const d2_t *>(&As[wm0 + 16 * i + fidx][ks + fkg]);
#pragma unroll
        for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const d2_t *>(&Bs[wn0 + 16 * j + fidx][ks + fkg]);
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = MF::mma(-av[i][e], bv[j][e], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                C[(long)(wm0 + 16 * i + MF::c_row(lane, r)) * Np + wn0 + 16 * j + MF::c_col(lane)] = acc[i][j][r];
}

__global__ __launch_bounds__(256, 2) void rank64_update_kernel(double *__restrict__ K, int Np, int o, int ncol) {
    __shared__ __attribute__((aligned(16))) double As[NB][R64_LDP];
    __shared__ __attribute__((aligned(16))) double Bs[NB][R64_LDP];
    const int bi = blockIdx.x / ncol, bj = blockIdx.x - bi * ncol;
    if (bj > bi) return;
    rank64_tile(K, Np, o, bi, bj, As, Bs);
}

// ------------------------------------------------------------------------------------------
// The panel chain with the pivot taken off the update's back (TGP_PANEL_LA, default on):
//   pivot_update_kernel(o, upd)   workgroup 0: the diagonal block at o -- with upd its pending
//                                 rank-64 update from the panel at o - NB applied in LDS first --
//                                 factored and inverted by one wave + MFMA (chol64.hpp), L_kk
//                                 written into K, X = L_kk^-1 into Dinv and Linv;
//                                 every other workgroup: one 64 x 64 tile of the rank-64 update
//                                 of the panel at o - NB (all tiles but that diagonal block)
//   panel_solve_kernel(o)         L_ik = A_ik X^T for the row blocks below, X read from Dinv
// Per panel the chain is solve (4 us) + pivot (14 us) with the update (7 us) hidden beside the
// pivot, instead of panel_d_kernel (16 us: every workgroup factoring the same block before its
// solve) followed by the update (7 us).  Same arithmetic in the same order: bit-identical results.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pivot_update_kernel(double *__restrict__ K, int Np, int o, int upd, int ncol,
                                                           double *__restrict__ Dinv, double *__restrict__ Linv,
                                                           double *__restrict__ scal, int *__restrict__ flag,
                                                           double tiny) {
    __shared__ __attribute__((aligned(16))) double lds[3 * NB * CH_LD + NB + 32];
    static_assert(CH_LD == R64_LDP, "the update tiles reuse the pivot's LDS");
    if (blockIdx.x > 0) {
        // tile t of the update with the panel at o - NB, skipping the diagonal block (workgroup 0 has it)
        const int t = blockIdx.x - 1;
        const int bi = t / ncol, bj = t - bi * ncol;
        if (bj > bi || (bi == 0 && bj == 0)) return;
        rank64_tile(K, Np, o - NB, bi, bj, reinterpret_cast<double (*)[R64_LDP]>(lds),
                    reinterpret_cast<double (*)[R64_LDP]>(lds + NB * R64_LDP));
        return;
    }
    double (*At)[CH_LD] = reinterpret_cast<double (*)[CH_LD]>(lds);
    double (*Xt)[CH_LD] = At + NB;
    double (*Tb)[CH_LD] = Xt + NB;
    double *rsbuf = lds + 3 * NB * CH_LD;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const d2_t z2 = {0.0, 0.0};
    double *Akk = K + (long)o * Np + o;
    if (upd) {
        // A_kk -= L_r L_r^T, L_r = rows o .. o+63 of the previous panel: the arithmetic of rank64_tile(0, 0)
        const double *Lr = K + (long)o * Np + (o - NB);
#pragma unroll
        for (int p8 = 0; p8 < 8; ++p8) {
            const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
            *reinterpret_cast<d2_t *>(&Tb[r][c2]) = *reinterpret_cast<const d2_t *>(Lr + (long)r * Np + c2);
            *reinterpret_cast<d2_t *>(&Xt[r][c2]) = z2;
        }
        using MF = Mfma<double>;
        const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
        d4_t acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[i][j][r] = Akk[(long)(wm0 + 16 * i + MF::c_row(lane, r)) * Np + wn0 + 16 * j + MF::c_col(lane)];
        __syncthreads();
        const int fidx = MF::ab_idx(lane), fkg = MF::ab_kg(lane) * 2;
#pragma unroll
        for (int ks = 0; ks < NB; ks += 8) {
            d2_t av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const d2_t *>(&Tb[wm0 + 16 * i + fidx][ks + fkg]);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const d2_t *>(&Tb[wn0 + 16 * j + fidx][ks + fkg]);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = MF::mma(-av[i][e], bv[j][e], acc[i][j]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    At[wm0 + 16 * i + MF::c_row(lane, r)][wn0 + 16 * j + MF::c_col(lane)] = acc[i][j][r];
    } else {
#pragma unroll
        for (int p8 = 0; p8 < 8; ++p8) {
            const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
            *reinterpret_cast<d2_t *>(&At[r][c2]) = *reinterpret_cast<const d2_t *>(Akk + (long)r * Np + c2);
            *reinterpret_cast<d2_t *>(&Xt[r][c2]) = z2;
        }
    }
    __syncthreads();
    factor64_v4(At, Xt, Tb, rsbuf, o, flag, tiny);
    // publish: L_kk (zeros above the diagonal) into K, X to Dinv and Linv
    double *dstL = Linv + (long)o * Np + o;
    double *dstD = Dinv + (long)(o / NB) * NB * NB;
#pragma unroll
    for (int p8 = 0; p8 < 8; ++p8) {
        const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
        d2_t lv = *reinterpret_cast<const d2_t *>(&At[r][c2]);
        lv[0] = (c2 <= r) ? lv[0] : 0.0;
        lv[1] = (c2 + 1 <= r) ? lv[1] : 0.0;
        *reinterpret_cast<d2_t *>(Akk + (long)r * Np + c2) = lv;
        const d2_t xv = *reinterpret_cast<const d2_t *>(&Xt[r][c2]);
        *reinterpret_cast<d2_t *>(dstL + (long)r * Np + c2) = xv;
        *reinterpret_cast<d2_t *>(dstD + r * NB + c2) = xv;
    }
    if (tid < 64) {   // sum(log(diag L)), fixed-order tree
        double s = log(At[tid][tid]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (tid == 0) scal[0] += s;
    }
}

__global__ __launch_bounds__(256, 2) void panel_solve_kernel(double *__restrict__ K, int Np, int o,
                                                          const double *__restrict__ Dinv) {
    __shared__ __attribute__((aligned(16))) double Xt[NB][CH_LD];
    __shared__ __attribute__((aligned(16))) double Tb[NB][CH_LD];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *Ablk = K + (long)(o + NB * (1 + blockIdx.x)) * Np + o;
    const double *X = Dinv + (long)(o / NB) * NB * NB;
#pragma unroll
    for (int p8 = 0; p8 < 8; ++p8) {
        const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
        *reinterpret_cast<d2_t *>(&Tb[r][c2]) = *reinterpret_cast<const d2_t *>(Ablk + (long)r * Np + c2);
        *reinterpret_cast<d2_t *>(&Xt[r][c2]) = *reinterpret_cast<const d2_t *>(X + r * NB + c2);
    }
    __syncthreads();
    using MF = Mfma<double>;
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    const int fidx = MF::ab_idx(lane), fkg = MF::ab_kg(lane) * 2;
    d4_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.0;
#pragma unroll
    for (int ks = 0; ks < NB; ks += 8) {
        d2_t av[2], bv[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const d2_t *>(&Tb[wm0 + 16 * i + fidx][ks + fkg]);
#pragma unroll
        for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const d2_t *>(&Xt[wn0 + 16 * j + fidx][ks + fkg]);
#pragma unroll
        for (int e = 0; e < 2; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = MF::mma(av[i][e], bv[j][e], acc[i][j]);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Ablk[(long)(wm0 + 16 * i + MF::c_row(lane, r)) * Np + wn0 + 16 * j + MF::c_col(lane)] = acc[i][j][r];
}

// ------------------------------------------------------------------------------------------
// ONE launch per panel (round 3, TGP_PANEL_FUSE, default on): the panel solve folded into the
// launch that carries the next pivot and the rank-64 update, so the chain per panel is one launch
// instead of two (panel_solve_kernel 6 us + pivot_update_kernel 18 us -> 19 us).
//   mode 0  (first panel of an outer block, pivot at o)   workgroup 0: the pivot alone;
//           workgroup 1 + i: copies the unsolved block A_i of the panel into Apan_out[i]
//   mode 1  (panel at o, its X = L_kk^-1 in Dinv)
//           workgroup 0: L_r = A_r X^T for the first row block below (written in place), the diagonal
//           block at o + NB minus L_r L_r^T in LDS, its factor and inverse, published;
//           workgroup 1 + t, tile (bi, bj) of the update: L_bi = A_bi X^T and L_bj = A_bj X^T solved
//           here (each tile solves its own two operands: no hand-over between workgroups), then
//           C_ij -= L_bi L_bj^T.  The tiles of column 0 (bj = 0) also write L_bi into K in place and
//           leave their updated tile -- the NEXT panel's unsolved block -- in Apan_out as well.
// Why the copy: the tiles read the unsolved A blocks of the panel while the column-0 tiles write
// the solved ones over them.  Everybody reads the panel from Apan_in (written by the previous
// launch, read-only here), so the in-place stores race with nothing.  Two slots used in turn.
// X is not staged in LDS: every wave reads the 32 rows of X its quadrant multiplies with straight
// into registers (B fragments of v_mfma_f64_16x16x4, 16 ds-free loads per lane from L2).
// Same MFMA sequences as panel_solve_kernel / rank64_tile / pivot_update_kernel: bit-identical L.
// ------------------------------------------------------------------------------------------
constexpr unsigned FUSED_STAMP_STRIDE = 2048;   // debug stamps: entries per launch
// where a wave runs: HW_ID (wave / SIMD / CU / SH / SE ids ...) in the low word, XCC_ID in the high one (debug stamps only)
__device__ __forceinline__ unsigned long long hw_where() {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);     // hwreg(HW_REG_HW_ID, 0, 32)
    const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);   // hwreg(HW_REG_XCC_ID, 0, 32)
    return ((unsigned long long)xcc << 32) | hw;
}
// debug (TGP_STAMP_FILE): which CUs a stream reaches -- many short workgroups, each leaving where it ran
__global__ void hw_probe_kernel(unsigned long long *__restrict__ out) {
    if (threadIdx.x == 0) out[blockIdx.x] = hw_where() | (1ull << 63);   // (bit 63: the slot was written)
}
__global__ __launch_bounds__(256) void fused_panel_kernel(double *__restrict__ K, int Np, int o, int mode, int ncol,
                                                          const double *__restrict__ Apan_in,
                                                          double *__restrict__ Apan_out,
                                                          double *__restrict__ Dinv, double *__restrict__ Linv,
                                                          double *__restrict__ scal, int *__restrict__ flag,
                                                          double tiny, unsigned long long *__restrict__ stamp) {
    __shared__ __attribute__((aligned(16))) double lds[3 * NB * CH_LD + NB + 32];
    // debug stamps (TGP_STAMP_FILE; null otherwise): per workgroup [start, end] in 10 ns ticks at
    // stamp[8 + 2 b], workgroup 0's phases at stamp[0..4]
    // (a launch's slot is FUSED_STAMP_STRIDE entries: workgroups past its end do not stamp)
    if (blockIdx.x >= (FUSED_STAMP_STRIDE - 8) / 2) stamp = nullptr;
    struct Stamp {
        unsigned long long *p; int b;
        __device__ ~Stamp() { if (p && threadIdx.x == 0) p[8 + 2 * b + 1] = wall_clock64(); }
    } stamp_guard{stamp, (int)blockIdx.x};
    if (stamp && threadIdx.x == 0) stamp[8 + 2 * blockIdx.x] = wall_clock64();
    if (stamp && threadIdx.x == 0 && blockIdx.x == 0) stamp[3] = hw_where();   // the pivot workgroup's CU (round 6)
    using MF = Mfma<double>;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    const int fidx = MF::ab_idx(lane), fkg = MF::ab_kg(lane) * 2;
    const double *X = Dinv + (long)(o / NB) * NB * NB;
    if (blockIdx.x > 0) {
        const int t = blockIdx.x - 1;
        if (mode == 0) {   // copy the unsolved block t of the panel at o
            const double *src = K + (long)(o + NB * (1 + t)) * Np + o;
            double *dst = Apan_out + (long)t * NB * NB;
#pragma unroll
            for (int p8 = 0; p8 < 8; ++p8) {
                const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
                *reinterpret_cast<d2_t *>(dst + r * NB + c2) = *reinterpret_cast<const d2_t *>(src + (long)r * Np + c2);
            }
            return;
        }
        const int bi = t / ncol, bj = t - bi * ncol;
        if (bj > bi || (bi == 0 && bj == 0)) return;
        double (*As)[CH_LD] = reinterpret_cast<double (*)[CH_LD]>(lds);
        double (*Bs)[CH_LD] = As + NB;
        const double *Ai = Apan_in + (long)bi * NB * NB;
        const double *Aj = Apan_in + (long)bj * NB * NB;
        double *C = K + (long)(o + NB * (1 + bi)) * Np + o + NB * (1 + bj);
        const bool diag = bi == bj;
        d2_t ra[8], rb[8], xb[2][8];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int idx = tid + 256 * p;
            ra[p] = *reinterpret_cast<const d2_t *>(Ai + (idx >> 5) * NB + (idx & 31) * 2);
            rb[p] = *reinterpret_cast<const d2_t *>(Aj + (idx >> 5) * NB + (idx & 31) * 2);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int s = 0; s < 8; ++s)
                xb[j][s] = *reinterpret_cast<const d2_t *>(X + (wn0 + 16 * j + fidx) * NB + 8 * s + fkg);
        d4_t acc[2][2];   // the old C tile: the update's MFMAs subtract in place
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[i][j][r] = C[(long)(wm0 + 16 * i + MF::c_row(lane, r)) * Np + wn0 + 16 * j + MF::c_col(lane)];
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int idx = tid + 256 * p;
            *reinterpret_cast<d2_t *>(&As[idx >> 5][(idx & 31) * 2]) = ra[p];
            *reinterpret_cast<d2_t *>(&Bs[idx >> 5][(idx & 31) * 2]) = rb[p];
        }
        __syncthreads();
        d4_t li[2][2], lj[2][2];
        acc_zero(li);
        acc_zero(lj);
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            d2_t av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                av[i] = *reinterpret_cast<const d2_t *>(&As[wm0 + 16 * i + fidx][8 * s + fkg]);
                bv[i] = *reinterpret_cast<const d2_t *>(&Bs[wm0 + 16 * i + fidx][8 * s + fkg]);
            }
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        li[i][j] = MF::mma(av[i][e], xb[j][s][e], li[i][j]);
                        if (!diag) lj[i][j] = MF::mma(bv[i][e], xb[j][s][e], lj[i][j]);
                    }
        }
        __syncthreads();   // every wave has read the unsolved tiles
        double *Lout = K + (long)(o + NB * (1 + bi)) * Np + o;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = wm0 + 16 * i + MF::c_row(lane, r), cc = wn0 + 16 * j + MF::c_col(lane);
                    As[rr][cc] = li[i][j][r];
                    if (!diag) Bs[rr][cc] = lj[i][j][r];
                    if (bj == 0) Lout[(long)rr * Np + cc] = li[i][j][r];   // L_bi in place (nobody reads K's panel in this launch)
                }
        __syncthreads();
        double (*Bu)[CH_LD] = diag ? As : Bs;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            d2_t av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const d2_t *>(&As[wm0 + 16 * i + fidx][8 * s + fkg]);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const d2_t *>(&Bu[wn0 + 16 * j + fidx][8 * s + fkg]);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = MF::mma(-av[i][e], bv[j][e], acc[i][j]);
        }
        double *Nout = Apan_out + (long)(bi - 1) * NB * NB;   // (bj == 0 implies bi >= 1 here)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = wm0 + 16 * i + MF::c_row(lane, r), cc = wn0 + 16 * j + MF::c_col(lane);
                    C[(long)rr * Np + cc] = acc[i][j][r];
                    if (bj == 0) Nout[rr * NB + cc] = acc[i][j][r];        // the next panel's unsolved block bi - 1
                }
        return;
    }
    // ---- workgroup 0: the pivot ----
    double (*At)[CH_LD] = reinterpret_cast<double (*)[CH_LD]>(lds);
    double (*Xt)[CH_LD] = At + NB;
    double (*Tb)[CH_LD] = Xt + NB;
    double *rsbuf = lds + 3 * NB * CH_LD;
    const d2_t z2 = {0.0, 0.0};
    const int op = mode ? o + NB : o;          // the block factored here
    double *Akk = K + (long)op * Np + op;
    if (mode) {
        // Both products skip what is known to be zero -- exact zeros whose products only ever add +-0 to
        // a sum, so the results stay bit-identical to the full products:
        //   solve   L_r = A_r X^T, X lower triangular: column block jb of the result needs k < 16 (jb + 1).
        //           Wave w takes row fragment w and all four column fragments: 40 MFMAs instead of 64.
        //   update  A_kk -= L_r L_r^T: only the ten 16 x 16 fragments on and below the diagonal are ever
        //           read again (the factorisation reads the diagonal blocks and what lies below them).
        //           Waves 0, 1 take three fragments, waves 2, 3 two: 48 MFMAs instead of 64.
        d2_t ra[8];
        d2_t xb0[2], xb1[4], xb2[6], xb3[8];       // B fragments of X's row blocks 0 .. 3: k-steps s < 2 (jb + 1)
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int idx = tid + 256 * p;
            ra[p] = *reinterpret_cast<const d2_t *>(Apan_in + (idx >> 5) * NB + (idx & 31) * 2);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) xb0[s] = *reinterpret_cast<const d2_t *>(X + (0 + fidx) * NB + 8 * s + fkg);
#pragma unroll
        for (int s = 0; s < 4; ++s) xb1[s] = *reinterpret_cast<const d2_t *>(X + (16 + fidx) * NB + 8 * s + fkg);
#pragma unroll
        for (int s = 0; s < 6; ++s) xb2[s] = *reinterpret_cast<const d2_t *>(X + (32 + fidx) * NB + 8 * s + fkg);
#pragma unroll
        for (int s = 0; s < 8; ++s) xb3[s] = *reinterpret_cast<const d2_t *>(X + (48 + fidx) * NB + 8 * s + fkg);
        // this wave's fragments (row block fi, column block fj) of the diagonal update
        const int nfr = wave < 2 ? 3 : 2;
        int fi[3], fj[3];
        fi[0] = wave == 0 ? 3 : (wave == 1 ? 3 : (wave == 2 ? 2 : 1));   fj[0] = wave == 0 ? 0 : (wave == 1 ? 3 : (wave == 2 ? 2 : 1));
        fi[1] = wave == 0 ? 3 : (wave == 1 ? 2 : (wave == 2 ? 1 : 0));   fj[1] = wave == 0 ? 1 : 0;
        fi[2] = wave == 0 ? 3 : 2;                                        fj[2] = wave == 0 ? 2 : 1;
        d4_t acc[3];
#pragma unroll
        for (int f = 0; f < 3; ++f)
            if (f < nfr) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    acc[f][r] = Akk[(long)(16 * fi[f] + MF::c_row(lane, r)) * Np + 16 * fj[f] + MF::c_col(lane)];
            }
#pragma unroll
        for (int p8 = 0; p8 < 8; ++p8) {
            const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
            *reinterpret_cast<d2_t *>(&Tb[r][c2]) = ra[p8];
            *reinterpret_cast<d2_t *>(&Xt[r][c2]) = z2;
        }
        __syncthreads();
        if (stamp && tid == 0) stamp[0] = wall_clock64();   // loads landed
        d4_t li[4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
#pragma unroll
            for (int r = 0; r < 4; ++r) li[jb][r] = 0.0;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const d2_t av = *reinterpret_cast<const d2_t *>(&Tb[16 * wave + fidx][8 * s + fkg]);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (s < 2) li[0] = MF::mma(av[e], xb0[s < 2 ? s : 0][e], li[0]);
                if (s < 4) li[1] = MF::mma(av[e], xb1[s < 4 ? s : 0][e], li[1]);
                if (s < 6) li[2] = MF::mma(av[e], xb2[s < 6 ? s : 0][e], li[2]);
                li[3] = MF::mma(av[e], xb3[s][e], li[3]);
            }
        }
        __syncthreads();
        double *Lout = K + (long)op * Np + o;   // row block 0 of the panel at o, in place
#pragma unroll
        for (int jb = 0; jb < 4; ++jb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = 16 * wave + MF::c_row(lane, r), cc = 16 * jb + MF::c_col(lane);
                Tb[rr][cc] = li[jb][r];
                Lout[(long)rr * Np + cc] = li[jb][r];
            }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < 3; ++f)
            if (f < nfr) {
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const d2_t av = *reinterpret_cast<const d2_t *>(&Tb[16 * fi[f] + fidx][8 * s + fkg]);
                    const d2_t bv = *reinterpret_cast<const d2_t *>(&Tb[16 * fj[f] + fidx][8 * s + fkg]);
#pragma unroll
                    for (int e = 0; e < 2; ++e) acc[f] = MF::mma(-av[e], bv[e], acc[f]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) At[16 * fi[f] + MF::c_row(lane, r)][16 * fj[f] + MF::c_col(lane)] = acc[f][r];
            }
    } else {
#pragma unroll
        for (int p8 = 0; p8 < 8; ++p8) {
            const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
            *reinterpret_cast<d2_t *>(&At[r][c2]) = *reinterpret_cast<const d2_t *>(Akk + (long)r * Np + c2);
            *reinterpret_cast<d2_t *>(&Xt[r][c2]) = z2;
        }
    }
    __syncthreads();
    if (stamp && tid == 0) stamp[1] = wall_clock64();       // the block is in LDS, updated
    factor64_v4(At, Xt, Tb, rsbuf, op, flag, tiny);
    if (stamp && tid == 0) stamp[2] = wall_clock64();       // factored and inverted
    double *dstL = Linv + (long)op * Np + op;
    double *dstD = Dinv + (long)(op / NB) * NB * NB;
#pragma unroll
    for (int p8 = 0; p8 < 8; ++p8) {
        const int idx = tid + 256 * p8, r = idx >> 5, c2 = (idx & 31) * 2;
        d2_t lv = *reinterpret_cast<const d2_t *>(&At[r][c2]);
        lv[0] = (c2 <= r) ? lv[0] : 0.0;
        lv[1] = (c2 + 1 <= r) ? lv[1] : 0.0;
        *reinterpret_cast<d2_t *>(Akk + (long)r * Np + c2) = lv;
        const d2_t xv = *reinterpret_cast<const d2_t *>(&Xt[r][c2]);
        *reinterpret_cast<d2_t *>(dstL + (long)r * Np + c2) = xv;
        *reinterpret_cast<d2_t *>(dstD + r * NB + c2) = xv;
    }
    if (tid < 64) {   // sum(log(diag L)), fixed-order tree
        double s = log(At[tid][tid]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (tid == 0) scal[0] += s;
    }
}

// 64-bit zero fill (the factor buffers exceed 4 GiB from N = 23170 on)
__global__ __launch_bounds__(256) void zero_fill_kernel(double2 *__restrict__ p, long n2) {
    const double2 z = {0.0, 0.0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n2; i += (long)gridDim.x * 256) p[i] = z;
}

}  // namespace tgp

// the streams of a device (device_streams, private_fit_begin / _end, ensure_lookahead): part of this translation unit
#include "fit_streams.hpp"

namespace tgp {

// First launch of a fit: Linv = 0, the pivot flag and the two scalars = 0, and -- when the inputs
// were staged in device-mapped host memory (src = [Xs | yn | ls]) -- their copy into HBM, so that a
// fit issues no memcpy and no memset of its own.
__global__ __launch_bounds__(256) void fit_prologue_kernel(double2 *__restrict__ linv, long n2,
                                                           const double *__restrict__ src,
                                                           double *__restrict__ Xs, long nxs,
                                                           double *__restrict__ yn, long nyn,
                                                           double *__restrict__ ls, long nls, int Dp,
                                                           int *__restrict__ flag, double *__restrict__ scal,
                                                           unsigned long long *__restrict__ stamp) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x, stride = (long)gridDim.x * 256;
    if (stamp && t == 0) *stamp = wall_clock64();      // the start tick of a polled call (doorbell.hpp)
    if (src) {
        // src holds the RAW inputs (round 5): X / length_scale (sklearn kernels.py:1556, :1711) is taken here -- the same
        // correctly rounded IEEE division the host loop did, without 131 072 of them on the host's critical path at C3
        const double *lsrc = src + nxs + nyn;
        for (long i = t; i < nxs; i += stride) {
            const int d = (int)(i % Dp);
            Xs[i] = d < (int)nls ? src[i] / lsrc[d] : 0.0;
        }
        for (long i = t; i < nyn; i += stride) yn[i] = src[nxs + i];
        for (long i = t; i < nls; i += stride) ls[i] = src[nxs + nyn + i];
    }
    if (t == 0) { *flag = 0; scal[0] = 0.0; scal[1] = 0.0; }
    const double2 z = {0.0, 0.0};
    for (long i = t; i < n2; i += stride) linv[i] = z;
}

// The last launch of a polled call that is a CHAIN of kernels (the blocked fit, its LML gradient): a kernel of its own
// behind them on the call's stream -- everything they wrote, the scalars in mapped host memory included, is out -- that
// rings the doorbell.  One 2-us launch for two event records and a stream synchronisation.
__global__ void ring_kernel(Bell bell) { bell_ring(bell, 1); }
hipError_t launch_ring(Context &c, const Bell &bell) {
    hipLaunchKernelGGL(ring_kernel, dim3(1), dim3(64), 0, c.stream, bell);
    return hipGetLastError();
}

}  // namespace tgp

// the schedule of the blocked fit (launch_fit): part of this translation unit -- the same flags, the same code object
#include "fit_blocked.hpp"
