// warp_kernels.hip -- learned input warping (Snoek, Swersky, Zemel, Adams, ICML 2014) on the device:
//
//   input_grad_kernel        d LML / d X of the resident fit, behind tgp_fit_grad's K^-1 = U U^T in d_W:
//                                d LML / d x_id = -(c / l_d) sum_{j != i} G_ij h_ij (s_id - s_jd),   s = x / l,  G = alpha alpha^T - K^-1
//   input_grad_sum_kernel    its per-(row, dimension) partials summed in a fixed order, scaled, written (N, D)
//   warp_kernel              the Kumaraswamy warp of (m, D) points, elementwise, with its derivatives (warp_math.hpp)
//   warp_chain_kernel        d LML / d log a_d = a_d sum_i (d LML / d Wx_id) (dw/da)(u_id), the same for b
//
// The input-gradient pass is lml_weights_kernel's (grad_kernels.hip) with a sum per (row, dimension) instead of per
// dimension: the lower triangle of 64 x 64 tiles, pairwise_sqdist, the weights w = G o h in registers, then passes of
// sixteen dimensions.  An off-diagonal tile (tm, tn) feeds the rows of its tile row (sum over its columns j) AND the rows
// of its tile column (sum over its rows i, with the sign of s_j - s_i): one subtraction and two FMAs per pair and
// dimension, where lml_weights_kernel has a subtraction, a product and an FMA.  Row r of tile t receives exactly one
// contribution from every tile of its tile row (tiles (t, s), s <= t: their row side) and of its tile column (tiles
// (s, t), s > t: their column side), so the partial buffer is ONE slab per column slice, partial[s][r][Dp], s < N / 64
// rounded up, each entry written exactly once and none ever added to: no atomics, and input_grad_sum_kernel adds the
// slices s = 0, 1, ... in that order whatever ran beside the kernel.  The grid is the lml_weights_kernel's: 2080 workgroups
// at N = 4096.
//
// Within a tile a pass reduces the 4 x 4 register block of a thread over the 16 threads that share its rows (lane bits
// 0-3) and over the 16 that share its columns (lane bits 4-5 and the four waves).  Both are reduce-scatters: a thread
// holds four sums, so the first two exchange steps each halve what it keeps -- 2 + 1 + 1 + 1 shuffles for the rows and
// 2 + 1 for the columns per dimension instead of 4 x 4 + 4 x 2 -- and the waves' column shares meet in LDS, added in the
// order of the waves.
#include <hip/hip_runtime.h>
#include <math.h>

#include "pair_weight.hpp"
#include "pairwise.hpp"
#include "small_grad.hpp"
#include "tgp_internal.hpp"
#include "warp_math.hpp"

namespace tgp {

#define TGP_TRY(x)                         \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

// four sums r[0..3] per lane, to be added over the lanes that differ in lane bits m1, m2 (and, rows only, 4 and 8): after
// the two halving steps the lane holds the sum over those four lanes of entry 2 * (bit m1) + (bit m2)
__device__ __forceinline__ double reduce_scatter4(const double r[4], bool o1, bool o2, int m1, int m2) {
    double k0 = o1 ? r[2] : r[0], k1 = o1 ? r[3] : r[1];
    const double s0 = o1 ? r[0] : r[2], s1 = o1 ? r[1] : r[3];
    k0 += __shfl_xor(s0, m1, 64);
    k1 += __shfl_xor(s1, m1, 64);
    double k = o2 ? k1 : k0;
    const double s = o2 ? k0 : k1;
    k += __shfl_xor(s, m2, 64);
    return k;
}

template <int KIND, class PW>
__global__ __launch_bounds__(256) void input_grad_kernel(const double *__restrict__ Xs, const PW pw,
                                                         double *__restrict__ partial, int N, int Np, int Dp) {
    constexpr int LD = PwCfg<double>::LD;
    __shared__ double Ct[PwCfg<double>::DC][LD];
    __shared__ double Xt[PwCfg<double>::DC][LD];
    __shared__ double racc[16][LD];          // [dimension of the pass][row of the tile]: the row side's sums
    __shared__ double cpart[4][16][LD];      // [wave][dimension][column of the tile]: the waves' shares of the column side
    int bx = blockIdx.x;
    int tm = (int)((sqrtf(8.0f * (float)bx + 1.0f) - 1.0f) * 0.5f);
    while ((tm + 1) * (tm + 2) / 2 <= bx) ++tm;
    while (tm * (tm + 1) / 2 > bx) --tm;
    const int tn = bx - tm * (tm + 1) / 2;
    const int i0 = tm * PW_T, j0 = tn * PW_T;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, wave = tid >> 6;
    const bool offd = tm != tn;              // (a diagonal tile holds the whole square of its rows: its row side is everything)
    double d2[4][4];
    pairwise_sqdist<double>(Xs, i0, Np, Xs, j0, Np, Dp, Ct, Xt, d2);
    double w[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const int i = i0 + 4 * ty + a;
        const double ai = (i < N) ? pw.row(i) : 0.0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = j0 + 4 * tx + b;
            w[a][b] = 0.0;
            if (i < N && j < N && i != j) {
                const int hi = i > j ? i : j, lo = i > j ? j : i;
                w[a][b] = pw.G(ai, i, j, (long)hi * Np + lo) * ls_weight<KIND>(d2[a][b]);   // (ls_weight is 0 at d2 = 0: a duplicated row)
            }
        }
    }
    const int orow = tid >> 2, oq = (tid & 3) * 4;   // the output step: this thread's row of the tile and the first of its four dimensions
    PwStage<double> sp, sq;
    for (int d0 = 0; d0 < Dp; d0 += 16) {
        sp.load(Xs, i0, Np, Dp, d0);
        sq.load(Xs, j0, Np, Dp, d0);
        __syncthreads();                     // (the last pass's reads of Ct / Xt and of racc / cpart are over)
        sp.store(Ct);
        sq.store(Xt);
        __syncthreads();
#pragma unroll 4
        for (int e = 0; e < 16; ++e) {
            double cv[4], xv[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) cv[a] = Ct[e][4 * ty + a];
#pragma unroll
            for (int b = 0; b < 4; ++b) xv[b] = Xt[e][4 * tx + b];
            double r[4] = {0.0, 0.0, 0.0, 0.0}, cc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const double df = cv[a] - xv[b];
                    r[a] = fma(w[a][b], df, r[a]);
                    cc[b] = fma(w[a][b], df, cc[b]);
                }
            double k = reduce_scatter4(r, (tx & 1) != 0, (tx & 2) != 0, 1, 2);
            k += __shfl_xor(k, 4, 64);
            k += __shfl_xor(k, 8, 64);
            if (tx < 4) racc[e][4 * ty + 2 * (tx & 1) + (tx >> 1)] = k;
            if (offd) {                      // (the same in every thread of the workgroup)
                const double kc = reduce_scatter4(cc, (ty & 1) != 0, (ty & 2) != 0, 16, 32);
                cpart[wave][e][4 * tx + 2 * (ty & 1) + ((ty >> 1) & 1)] = kc;
            }
        }
        __syncthreads();
        if (d0 + oq < Dp) {                  // (Dp is a multiple of 4: the four dimensions are inside together)
            const int gi = i0 + orow, gj = j0 + orow;
            if (gi < N) {
                double *o = partial + ((long)tn * N + gi) * Dp + d0 + oq;
#pragma unroll
                for (int q = 0; q < 4; ++q) o[q] = racc[oq + q][orow];
            }
            if (offd && gj < N) {
                double *o = partial + ((long)tm * N + gj) * Dp + d0 + oq;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    o[q] = -((cpart[0][oq + q][orow] + cpart[1][oq + q][orow]) + (cpart[2][oq + q][orow] + cpart[3][oq + q][orow]));
            }
        }
    }
}

// dX[i][d] = -(c / l_d) sum_s partial[s][i][d], s = 0, 1, ... (an exact zero sum leaves +0.0)
__global__ __launch_bounds__(256) void input_grad_sum_kernel(const double *__restrict__ partial, const double *__restrict__ ls,
                                                             double constant, int nt, int N, int D, int Dp,
                                                             double *__restrict__ dX) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)N * Dp) return;
    const long i = idx / Dp;
    const int d = (int)(idx - i * Dp);
    if (d >= D) return;
    double s = 0.0;
    for (int t = 0; t < nt; ++t) s += partial[((long)t * N + i) * Dp + d];
    const double v = -(constant / ls[d]) * s;
    dX[i * D + d] = v == 0.0 ? 0.0 : v;
}

hipError_t launch_input_grad(Context &c, double *partial, double *dX) {
    const int N = (int)c.N, Np = (int)c.Np, Dp = (int)c.Dp, D = (int)c.D;
    const int nt = (N + PW_T - 1) / PW_T;
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return input_grad_kernel<K(), LmlPairWeight>; }), dim3(nt * (nt + 1) / 2),
                       dim3(256), 0, c.stream, c.d_Xs, LmlPairWeight{c.d_alpha, c.d_W}, partial, N, Np, Dp);
    TGP_TRY(hipGetLastError());
    const long total = (long)N * Dp;
    hipLaunchKernelGGL(input_grad_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.stream, partial, c.d_ls,
                       c.constant, nt, N, D, Dp, dX);
    return hipGetLastError();
}

// par: [lo (D) | hi (D) | a (D) | b (D)].  One kernel for every caller -- tgp_warp_points, tgp_warp_candidates and
// tgp_fit_warp_grad differ in which outputs they ask for -- so an element's w has the same bits in all of them, whatever
// m and wherever the element stands.  raw: a copy of the input (the batch's raw rows), or null
__global__ __launch_bounds__(256) void warp_kernel(const double *__restrict__ src, long total, int D, const double *__restrict__ par,
                                                   double *__restrict__ raw, double *__restrict__ wout, double *__restrict__ du,
                                                   double *__restrict__ da, double *__restrict__ db) {
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < total; k += (long)gridDim.x * 256) {
        const int d = (int)(k % D);
        const double x = src[k];
        if (raw) raw[k] = x;
        const double u = warp_unit(x, par[d], par[D + d]);
        WarpDerivs v;
        wout[k] = warp_value(u, par[2 * D + d], par[3 * D + d], du != nullptr, da != nullptr, db != nullptr, v);
        if (du) du[k] = v.du;
        if (da) da[k] = v.da;
        if (db) db[k] = v.db;
    }
}

hipError_t launch_warp(Context &c, const double *src, int64_t total, int D, const double *par, double *raw, double *wout,
                       double *du, double *da, double *db) {
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 2048);   // (grid-stride beyond eight workgroups per CU)
    hipLaunchKernelGGL(warp_kernel, dim3((unsigned)blocks), dim3(256), 0, c.stream, src, (long)total, D, par, raw, wout, du, da, db);
    return hipGetLastError();
}

// out[which D + d] = shape_d sum_i dWx[i][d] dq[i][d], dq = dw/da (which = 0) or dw/db (1): workgroup (d, which), a thread
// takes rows tid, tid + 256, ... in order, then the tree over the 256 threads
__global__ __launch_bounds__(256) void warp_chain_kernel(const double *__restrict__ dWx, const double *__restrict__ dwda,
                                                         const double *__restrict__ dwdb, const double *__restrict__ par, int N,
                                                         int D, double *__restrict__ out) {
    __shared__ double red[256];
    const int d = blockIdx.x, which = blockIdx.y;
    const double *dq = which ? dwdb : dwda;
    double s = 0.0;
    for (int i = threadIdx.x; i < N; i += 256) s = fma(dWx[(long)i * D + d], dq[(long)i * D + d], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[which * D + d] = par[(2 + which) * D + d] * red[0];
}

hipError_t launch_warp_chain(Context &c, const double *dWx, const double *dwda, const double *dwdb, const double *par, double *out) {
    hipLaunchKernelGGL(warp_chain_kernel, dim3((unsigned)c.D, 2), dim3(256), 0, c.stream, dWx, dwda, dwdb, par, (int)c.N, (int)c.D, out);
    return hipGetLastError();
}

}  // namespace tgp
