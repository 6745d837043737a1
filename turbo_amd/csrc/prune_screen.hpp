// prune_screen.hpp -- the loose screen in front of the pruned sweep's bound pass (sweep_pruned.hpp, sweep_pruned).
//
// f32 handles with the RBF kernel only.  For every candidate c the screen forms
//     mu_s(c) = sum_i k_s(c, i) alpha_i,     k_s = exp2(fma(s, -log2(e) / 2, log2(constant))),
//     s = max(0, (|c|^2 + |x_i|^2) + (-2 c . x_i))
// with the dot products on v_mfma_f32_32x32x2_f32 (the training points enter LDS already multiplied by -2, which is
// exact) and an error term E(c) with |mu_s(c) - mu~(c)| <= E(c), mu~ the mean the contraction forms for the same
// candidate (direct-difference f32 distances, the same exp2 sequence, MeanAcc's f64 sum).  Nothing of it is ever reported:
// mu_s -+ E only decides which candidates go on to the tight bound pass and the exact contraction.
//
// E(c), derived in DESIGN §4 ("the screen's error term"), u = 2^-24:
//     E(c) = 1.001 |alpha|_1 (P (|c|^2 + max_i |x_i|^2) + Q)
//     P = 1.001 constant u (1.5 D + 6)
//     Q = 1.001 constant (u (0.5 (D + 3) + 1.4 |log2 constant| + 11.2) + 8 (N + 8) 2^-53) + 2^-120
// screen_error_terms() below is the ONE place the constants live; tests/prune_screen_reference.py restates them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mfma_gemm.hpp"

namespace tgp {

constexpr int SCR_T = 128;           // candidates per workgroup and training points per tile
constexpr int SCR_DC = 32;           // dimensions staged per pass
constexpr int SCR_LD = SCR_DC + 4;   // LDS row of a point: 16-byte pad, so a lane's ds_read_b128 of 4 k-values meets no conflict
constexpr int SCR_MAXD = 2048;       // the first-order constants of E hold while (D + 3) 2^-23 stays far below 1

struct ScreenTerms { double P, Q; };
inline ScreenTerms screen_error_terms(double constant, int D, int N) {
    const double u = 0x1p-24, ce = 1.001 * constant;
    ScreenTerms t;
    t.P = ce * u * (1.5 * D + 6.0);
    t.Q = ce * (u * (0.5 * (D + 3) + 1.4 * fabs(log2(constant)) + 11.2) + 8.0 * (double)(N + 8) * 0x1p-53) + 0x1p-120;
    return t;
}

// once per sweep: nx[i] = |x_i|^2 in f32 (i < Np; the padding rows are zero), scal = {ea, eb} with E(c) = ea + eb |c|^2
__global__ __launch_bounds__(1024) void screen_stats_kernel(const float *__restrict__ Xs, const double *__restrict__ alpha, int N,
                                                            int Np, int Dp, double P, double Q, float *__restrict__ nx,
                                                            double *__restrict__ scal) {
    __shared__ double sa[1024];
    __shared__ float sm[1024];
    double a1 = 0.0;
    float mx = 0.f;
    for (int i = threadIdx.x; i < Np; i += 1024) {
        float s = 0.f;
        if (i < N) {
            for (int d = 0; d < Dp; ++d) { const float x = Xs[(long)i * Dp + d]; s = fmaf(x, x, s); }
            a1 += fabs(alpha[i]);
            mx = fmaxf(mx, s);
        }
        nx[i] = s;
    }
    sa[threadIdx.x] = a1;
    sm[threadIdx.x] = mx;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sa[threadIdx.x] += sa[threadIdx.x + o];
            sm[threadIdx.x] = fmaxf(sm[threadIdx.x], sm[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double an = 1.001 * sa[0];
        scal[0] = an * (P * (double)sm[0] + Q);
        scal[1] = an * P;
    }
}

struct ScreenArgs {
    const float *Cs;          // (rows, Dp) scaled candidates, rows a multiple of 128, padding zero
    const float *Xs;          // (Np, Dp) scaled training points
    const double *alpha;      // (N,)
    const float *nx;          // (Np,) screen_stats_kernel
    const double *scal;       // {ea, eb}
    double *mupart;           // (gridDim.y, ldpart): split y's share of mu_s
    double *err;              // (rows,) E(c), written by split 0
    long ldpart;
    int N, Np, Dp;
    double constant;
};

// 16-byte vectors of a 128-point block, global -> registers -> LDS [point][k] (k contiguous: the MFMA operand order)
struct ScrStage {
    f4_t v[4];
    __device__ __forceinline__ void load(const float *__restrict__ M, long r0, int Dp, int d0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = (int)threadIdx.x + 256 * p;
            const int r = idx >> 3, dv = (idx & 7) * 4;
            v[p] = (f4_t){0.f, 0.f, 0.f, 0.f};
            if (d0 + dv < Dp) v[p] = *reinterpret_cast<const f4_t *>(M + (r0 + r) * Dp + d0 + dv);   // (Dp is a multiple of 4)
        }
    }
    __device__ __forceinline__ void store(float (*S)[SCR_LD], float scale) const {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = (int)threadIdx.x + 256 * p;
            const int r = idx >> 3, dv = (idx & 7) * 4;
            *reinterpret_cast<f4_t *>(&S[r][dv]) = v[p] * scale;
        }
    }
};

// grid = (rows / 128, splits of the training tiles); 4 waves, wave w owns candidates 32 w .. 32 w + 31 of the tile against
// all 128 training points of a tile: four 32 x 32 accumulators.  A row of C/D (a candidate) lies in one register of 32
// lanes, a column (a training point) on the lane: alpha and |x|^2 cost a lane one value per fragment, |c|^2 and the f64
// sums one per register.  Per pair the epilogue issues add, add, max, fma, v_exp_f32, fma; the four columns a lane holds of
// a row are summed in f32, then ONE f64 add per row and tile.
__global__ __launch_bounds__(256, 2) void prune_screen_kernel(ScreenArgs g) {
    __shared__ __attribute__((aligned(16))) float Ct[SCR_T][SCR_LD];
    __shared__ __attribute__((aligned(16))) float Xt[SCR_T][SCR_LD];
    __shared__ float ncs[SCR_T];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const long c0 = (long)blockIdx.x * SCR_T;
    const int Dp = g.Dp, N = g.N;
    const int njt = (N + SCR_T - 1) / SCR_T;                        // tiles that hold real points
    const int per = (njt + (int)gridDim.y - 1) / (int)gridDim.y;
    const int jt0 = blockIdx.y * per;
    const int jt1 = jt0 + per < njt ? jt0 + per : njt;
    const int nch = (Dp + SCR_DC - 1) / SCR_DC;
    const int nsteps = (jt1 > jt0 ? jt1 - jt0 : 0) * nch;
    const bool one_pass = nch == 1;

    // |c|^2, one fma chain per candidate in dimension order
    if (tid < SCR_T) {
        const float *row = g.Cs + (c0 + tid) * Dp;
        float s = 0.f;
        for (int d = 0; d < Dp; d += 4) {
            const f4_t x = *reinterpret_cast<const f4_t *>(row + d);
            s = fmaf(x[0], x[0], s); s = fmaf(x[1], x[1], s); s = fmaf(x[2], x[2], s); s = fmaf(x[3], x[3], s);
        }
        ncs[tid] = s;
        if (blockIdx.y == 0) g.err[c0 + tid] = g.scal[0] + g.scal[1] * (double)s;
    }
    ScrStage sp, sq;
    if (nsteps > 0) {
        sp.load(g.Cs, c0, Dp, 0);
        sq.load(g.Xs, (long)jt0 * SCR_T, Dp, 0);
        sp.store(Ct, 1.f);
        sq.store(Xt, -2.f);
    }
    __syncthreads();
    float nc[16];
    double sum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        nc[r] = ncs[32 * w + Mfma<float>::c_row(lane, r)];
        sum[r] = 0.0;
    }
    const float log2c = log2f((float)g.constant);
    f16_t acc[4];
    for (int st = 0; st < nsteps; ++st) {
        const int jt = jt0 + st / nch, ch = st - (st / nch) * nch;
        const int j0 = jt * SCR_T;
        const bool more = st + 1 < nsteps;
        if (more) {
            const int jn = jt0 + (st + 1) / nch, cn = (st + 1) - ((st + 1) / nch) * nch;
            if (!one_pass) sp.load(g.Cs, c0, Dp, cn * SCR_DC);
            sq.load(g.Xs, (long)jn * SCR_T, Dp, cn * SCR_DC);
        }
        float nxv[4], al[4];
        if (ch == nch - 1) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int j = j0 + 32 * b + li;
                nxv[b] = g.nx[j];
                al[b] = j < N ? (float)g.alpha[j] : 0.f;
            }
        }
        if (ch == 0) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
        }
        int dn = Dp - ch * SCR_DC;
        if (dn > SCR_DC) dn = SCR_DC;
        const int ns8 = (dn + 7) >> 3;                // (the staged block is zero beyond Dp)
        // k-values 8 s .. 8 s + 7: lane half h takes 8 s + 4 h + e for MFMA e, both operands alike
#pragma unroll 1
        for (int s8 = 0; s8 < ns8; ++s8) {
            const int k = 8 * s8 + 4 * lh;
            const f4_t a = *reinterpret_cast<const f4_t *>(&Ct[32 * w + li][k]);
            f4_t bv[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) bv[b] = *reinterpret_cast<const f4_t *>(&Xt[32 * b + li][k]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[b] = Mfma<float>::mma(a[e], bv[b][e], acc[b]);
        }
        if (ch == nch - 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float p = 0.f;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float s = fmaxf(0.f, (nc[r] + nxv[b]) + acc[b][r]);
                    const float kv = __builtin_amdgcn_exp2f(fmaf(s, -0.72134752044448170368f, log2c));
                    p = b == 0 ? kv * al[0] : fmaf(kv, al[b], p);
                }
                sum[r] += (double)p;
            }
        }
        if (more) {
            __syncthreads();
            if (!one_pass) sp.store(Ct, 1.f);
            sq.store(Xt, -2.f);
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        double s = sum[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (li == 0) g.mupart[(long)blockIdx.y * g.ldpart + c0 + 32 * w + Mfma<float>::c_row(lane, r)] = s;
    }
}

}  // namespace tgp
