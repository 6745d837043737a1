// loo_kernels.hip -- leave-one-out cross-validation of a finished fit (Linv, alpha resident) in closed form,
// Rasmussen & Williams section 5.4.2, eqs. 5.10-5.13.  In normalised units, K = c k0 + (noise + jitter) I:
//
//   kappa_i = (K^-1)_ii = sum_{k >= i} Linv[k,i]^2          (column sums of squares of the inverse factor)
//   y~_i - mu_-i = alpha_i / kappa_i,   sigma^2_-i = 1 / kappa_i                                   (5.12)
//   lpd_i = 1/2 log kappa_i - 1/2 alpha_i^2 / kappa_i - 1/2 log 2 pi,   L_LOO = sum_i lpd_i        (5.10, 5.11)
//   dL_LOO/dtheta = 1/2 sum_ab G_ab (dK/dtheta)_ab,  G = b alpha^T + alpha b^T - 2 B               (5.13, as one trace)
//     p_i = alpha_i / kappa_i,  w_i = 1/2 (1 / kappa_i + alpha_i^2 / kappa_i^2),  b = K^-1 p,  B = K^-1 diag(w) K^-1
//
// The normalisation (y_mean, y_std of all N points) and the hyper-parameters are HELD across the folds: that is
// what the closed form means.  Every sum has a fixed order (no floating-point atomics): the same bits run to run.
// Rows and columns >= N are padding and are masked by index, whatever an earlier, larger fit left there.
#include <hip/hip_runtime.h>
#include <math.h>

#include "gemm64_glds.hpp"
#include "gemm_nt_glds.hpp"
#include "mfma_gemm.hpp"
#include "nt_product.hpp"
#include "tgp_internal.hpp"

namespace tgp {

#define TGP_TRY(x)                         \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

// ---- kappa, stage 1: partial[chunk][column] = sum over the chunk's rows k (column <= k < N) of Linv[k,column]^2 ----
// Memory-bound: N^2 / 2 doubles read once.  A workgroup owns 64 columns x LOO_ROWS rows; lanes run along the columns
// (a wave reads 512 contiguous bytes of a row), the four waves take every fourth row, and their shares are added
// in a fixed order.  Tiles above the diagonal read nothing and leave zeros.  At N = 4096: 64 x 16 workgroups, 544 of
// them with rows to read.
__global__ __launch_bounds__(256) void loo_kappa_partial_kernel(const double *__restrict__ Linv, int N, int Np,
                                                                double *__restrict__ partial) {
    __shared__ double sh[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 64, col = c0 + lane;
    const int r0 = blockIdx.y * LOO_ROWS;
    int r1 = r0 + LOO_ROWS;
    r1 = r1 < N ? r1 : N;
    double acc = 0.0;
    if (r1 > c0) {                                        // (else: wholly above the diagonal)
        const int rb = r0 > c0 ? r0 : c0;                 // first row with an entry on or below the diagonal in these columns
        const double *src = Linv + (long)col;
        int k = rb + wave;
        for (; k + 12 < r1; k += 16) {                    // four rows of this wave in flight
            const double v0 = src[(long)k * Np], v1 = src[(long)(k + 4) * Np];
            const double v2 = src[(long)(k + 8) * Np], v3 = src[(long)(k + 12) * Np];
            const double m0 = k >= col ? v0 : 0.0, m1 = k + 4 >= col ? v1 : 0.0;   // (what lies above the diagonal is never multiplied)
            const double m2 = k + 8 >= col ? v2 : 0.0, m3 = k + 12 >= col ? v3 : 0.0;
            acc = fma(m0, m0, acc);
            acc = fma(m1, m1, acc);
            acc = fma(m2, m2, acc);
            acc = fma(m3, m3, acc);
        }
        for (; k < r1; k += 4) {
            const double v = src[(long)k * Np];
            const double m = k >= col ? v : 0.0;
            acc = fma(m, m, acc);
        }
    }
    sh[wave][lane] = acc;
    __syncthreads();
    if (wave == 0) partial[(long)blockIdx.y * Np + col] = col < N ? (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]) : 0.0;
}

// ---- stage 2: the chunks added in index order and the per-point results, 256 points per workgroup ----
// vec: [kappa | resid | sigma | lpd | p | sqrt(w) | b (the gradient's, not written here)], Np each; p and sqrt(w) are zero from N on (a padding row must not
// reach b or B).  blockpart[blk] = the workgroup's sum of lpd in a fixed tree, blockpart[nblk + blk] = how many of its
// kappa_i are <= 0 or not finite (nothing is clamped).
__global__ __launch_bounds__(256) void loo_points_kernel(const double *__restrict__ partial, int nchunk,
                                                         const double *__restrict__ alpha, int N, int Np,
                                                         double y_std, double *__restrict__ vec,
                                                         double *__restrict__ blockpart) {
    __shared__ double red[256];
    __shared__ int bad[256];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;                  // < Np: the grid is Np / 256 workgroups
    double kap = 0.0, res = 0.0, sig = 0.0, lp = 0.0, p = 0.0, sw = 0.0;
    int nb = 0;
    if (i < N) {
        for (int c = 0; c < nchunk; ++c) kap += partial[(long)c * Np + i];
        const double a = alpha[i];
        if (!(kap > 0.0) || !isfinite(kap)) nb = 1;
        p = a / kap;
        res = y_std * p;
        sig = y_std / sqrt(kap);
        lp = 0.5 * log(kap) - 0.5 * (a * p) - 0.5 * LOO_LOG_2PI;
        sw = sqrt(0.5 * (1.0 / kap + p * p));
    }
    vec[i] = kap;
    vec[(long)Np + i] = res;
    vec[2L * Np + i] = sig;
    vec[3L * Np + i] = lp;
    vec[4L * Np + i] = p;
    vec[5L * Np + i] = sw;
    red[tid] = lp;
    bad[tid] = nb;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[tid] += red[tid + o];
            bad[tid] += bad[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        blockpart[blockIdx.x] = red[0];
        blockpart[gridDim.x + blockIdx.x] = (double)bad[0];
    }
}

// ---- stage 3 (one workgroup): the nblk <= 256 workgroups' sums in a fixed tree: scal[0] = L_LOO, scal[1] = the bad count ----
__global__ __launch_bounds__(256) void loo_total_kernel(const double *__restrict__ blockpart, int nblk, double *__restrict__ scal) {
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    red[0][tid] = tid < nblk ? blockpart[tid] : 0.0;
    red[1][tid] = tid < nblk ? blockpart[nblk + tid] : 0.0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] += red[0][tid + o];
            red[1][tid] += red[1][tid + o];
        }
        __syncthreads();
    }
    if (tid < 2) scal[tid] = red[tid][0];
}

hipError_t launch_loo_points(Context &c, double *scal) {
    const int N = (int)c.N, Np = (int)c.Np;
    const int nchunk = (N + LOO_ROWS - 1) / LOO_ROWS, nblk = Np / 256;      // (Np <= 65536: at most 256 workgroups)
    double *vec = c.d_loov, *partial = vec + 7L * Np;   // (vec's seventh vector is the gradient's b)
    double *blockpart = partial + (long)(Np / LOO_ROWS) * Np;
    hipLaunchKernelGGL(loo_kappa_partial_kernel, dim3((N + 63) / 64, nchunk), dim3(256), 0, c.stream, c.d_Linv, N, Np, partial);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loo_points_kernel, dim3(nblk), dim3(256), 0, c.stream, partial, nchunk, c.d_alpha, N, Np, c.y_std, vec, blockpart);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loo_total_kernel, dim3(1), dim3(256), 0, c.stream, blockpart, nblk, scal);
    return hipGetLastError();
}

// ---- the gradient's chain ----
// y_i = sum_k M[i,k] x_k over k <= i (lower = 1: M = Linv) or k >= i (lower = 0: M = U = Linv^T), k < N; one wave per
// row, lanes along the row, the lanes' shares added in a fixed tree.  Rows >= N give 0.
__global__ __launch_bounds__(256) void loo_tri_gemv_kernel(const double *__restrict__ M, const double *__restrict__ x,
                                                           double *__restrict__ y, int N, int Np, int lower) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= Np) return;
    double s = 0.0;
    if (i < N) {
        const double *row = M + (long)i * Np;
        const int kb = lower ? 0 : (i & ~63), ke = lower ? i + 1 : N;
        for (int k = kb + lane; k < ke; k += 64) {
            const bool in = lower ? true : k >= i;
            const double m = in ? row[k] : 0.0;
            s = fma(m, x[k], s);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) y[i] = s;
}

// A = K^-1 diag(sqrt(w)), the full (Np, Np) matrix from the lower triangle of Kinv: A[i,j] = Kinv[max(i,j), min(i,j)] sw[j];
// rows >= N are zero (columns >= N are, because sw is).  64 x 64 tiles, the source tile transposed through LDS above the diagonal.
__global__ __launch_bounds__(256) void loo_expand_kernel(const double *__restrict__ Kinv, const double *__restrict__ sw,
                                                         double *__restrict__ A, int N, int Np) {
    __shared__ double S[64][65];
    const int ti = blockIdx.y, tj = blockIdx.x;
    const int si = ti > tj ? ti : tj, sj = ti > tj ? tj : ti;       // the source tile: on or below the diagonal
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int r = ty; r < 64; r += 4) S[r][tx] = Kinv[(long)(si * 64 + r) * Np + sj * 64 + tx];
    __syncthreads();
    const int j = tj * 64 + tx;
    const double wj = sw[j];
    for (int r = ty; r < 64; r += 4) {
        const int i = ti * 64 + r;
        double v;
        if (ti > tj) v = S[r][tx];
        else if (ti < tj) v = S[tx][r];
        else v = r >= tx ? S[r][tx] : S[tx][r];
        A[(long)i * Np + j] = (i < N && j < N) ? v * wj : 0.0;
    }
}

// behind the fit on c.stream: K^-1 into d_W (as launch_lml_grad forms it), kappa / p / w by tgp_loo's own kernels on
// d_Linv (so *loo has tgp_loo's bytes), b, A, B = A A^T over the lower tiles into d_W (K^-1 is not needed any more),
// then the pairwise pass with the LOO pair weight.  scal: [L_LOO, bad kappa count]; gout as launch_lml_grad leaves it.
hipError_t launch_loo_grad(Context &c, bool ard, double *gout, double *scal, bool timed) {
    hipStream_t s = c.stream;
    const int N = (int)c.N, Np = (int)c.Np;
    if (timed) {
        for (int i = 0; i < 4; ++i)
            TGP_TRY(c.evg[i].create(hipEventDefault));
        TGP_TRY(hipEventRecord(c.evg[0], s));
    }
    TGP_TRY(launch_kinv_product(c));
    TGP_TRY(launch_loo_points(c, scal));
    double *vec = c.d_loov;
    const double *p = vec + 4L * Np, *sw = vec + 5L * Np;
    double *b = vec + 6L * Np, *t = vec + 7L * Np;  // (the chunks' partials are spent) t = Linv p, then b = Linv^T t = K^-1 p
    hipLaunchKernelGGL(loo_tri_gemv_kernel, dim3(Np / 4), dim3(256), 0, s, c.d_Linv, p, t, N, Np, 1);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loo_tri_gemv_kernel, dim3(Np / 4), dim3(256), 0, s, c.d_U, t, b, N, Np, 0);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(loo_expand_kernel, dim3(Np / 64, Np / 64), dim3(256), 0, s, c.d_W, sw, c.d_looA, N, Np);
    TGP_TRY(hipGetLastError());
    NtProduct g;   // B = A A^T, lower tiles, into W
    g.device = c.device;
    g.A = c.d_looA; g.lda = Np;
    g.B = c.d_looA; g.ldb = Np;
    g.C = c.d_W; g.ldc = Np;
    g.rows = g.cols = Np; g.K = Np; g.alpha = 1.0; g.beta = 0.0;
    if (Np <= tuning().kinv64) {
        const int nt = Np / 64;
        TGP_TRY((g.on64<KR_FULL, TM_LOWER>(s, nt * (nt + 1) / 2, 1)));
    } else {
        const int nt = Np / 128;
        TGP_TRY((g.on128<KN_FULL, TM_LOWER>(s, nt * (nt + 1) / 2, 1)));
    }
    if (timed) TGP_TRY(hipEventRecord(c.evg[1], s));
    return launch_pair_sums(c, ard, b, gout, timed);
}

}  // namespace tgp
