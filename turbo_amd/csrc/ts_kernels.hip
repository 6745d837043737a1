// ts_kernels.hip -- Thompson sampling: S posterior sample paths of the fitted model (tgp_ts_draw), their arg-max over
// the resident candidates (tgp_ts_sweep) and their values and gradients at host points (tgp_ts_eval).
//
// The reference names a TS acquisition and the 'asyTS' batch strategy but leaves both unimplemented
// (old_library/acquisition_functions.py:20-21, bayesian_optimiser.py:102-104, :512-513).  Pathwise conditioning with
// random Fourier features (Wilson et al. 2020, "Efficiently sampling functions from Gaussian process posteriors"), in the
// fitted model's normalised units (c the constant, u = x / l, K = c k0(X, X) + (noise + jitter) I):
//
//   f_prior_s(x) = sqrt(2c / F) sum_i W[s,i] cos(omega_i . u + b_i)            F features shared by all samples
//   v_s          = K^-1 (y~ - f_prior_s(X) - eps_s) = alpha - K^-1 (f_prior_s(X) + eps_s),  eps_s ~ N(0, (noise + jitter) I)
//   f_s(x)       = f_prior_s(x) + sum_n c k0(x, X_n) v_s[n],      raw value = y_mean + y_std f_s(x)
//
// (alpha = K^-1 y~ is the fit's own, so a received factor, which carries no y~, draws too.)  The samples are of the
// latent f, not of y: their variance is the posterior variance without the WhiteKernel noise.
//
// Random numbers: Philox-4x32-10 keyed by the 64-bit seed, counter (element lo, element hi, stream, TS_TAG).  One call
// gives two 53-bit uniforms ((a >> 5) 2^26 + (b >> 6)) / 2^53 from words (0, 1) and (2, 3); a normal is ONE Box-Muller
// branch sqrt(-2 log(1 - u1)) cos(2 pi u2).  Streams and elements:
//   0  omega's normals z   element i D + d          omega_i = z_i (RBF),  z_i sqrt(2 nu / chi2_i) (Matern nu)
//   1  the chi2 normals    element 8 i + j, j < 2 nu   chi2_i = sum_j n_j^2
//   2  b                   element i                b_i = 2 pi u1 (one rounding)
//   3  W                   element s F + i
//   4  eps                 element s N + n          eps = sqrt(noise + jitter) z
// so sample s of an S-sample draw is the same whatever S is.  Everything here is f64, whatever the handle's sweep dtype.
//
// ts_pass_kernel is the one O(M (F + N) D) pass: per 64 candidates the phases Cs . Omega^T on v_mfma_f64_16x16x4 in
// chunks of 16 features, cos, and the contraction with W on the matrix cores (the phase tile's accumulator is the
// next product's B operand as it lies); then bt_pass_kernel's staged direct sums of squared differences, the kernel
// values again a B operand, against S columns of V.  Nothing M x N or M x F is written.
#include <hip/hip_runtime.h>
#include <math.h>

#include "mfma_gemm.hpp"
#include "pairwise.hpp"
#include "philox.hpp"
#include "query_math.hpp"
#include "tgp_internal.hpp"

namespace tgp {

#define TGP_TRY(x)                         \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

constexpr uint32_t TS_TAG = 0x54534D50u;   // "TSMP": the fourth counter word of every draw
constexpr double TS_TWO_PI = 6.283185307179586;

// (the uniform, the counter layout and the Box-Muller branch: philox.hpp)
__device__ __forceinline__ double ts_u53(uint32_t a, uint32_t b) { return philox_u53(a, b); }
__device__ __forceinline__ void ts_words(unsigned long long e, uint32_t stream, unsigned long long seed, uint32_t r[4]) {
    philox_words(e, stream, TS_TAG, seed, r);
}
__device__ __forceinline__ double ts_normal(unsigned long long e, uint32_t stream, unsigned long long seed) {
    return philox_normal(e, stream, TS_TAG, seed);
}

// omega (F, Dp; columns >= D zero), b (F), W (Spad, F; rows >= S zero), eps (S, N)
__global__ __launch_bounds__(256) void ts_rng_kernel(double *__restrict__ omega, double *__restrict__ b,
                                                     double *__restrict__ W, double *__restrict__ eps, int F, int D,
                                                     int Dp, int S, int Spad, int N, int nu2, double eps_sd,
                                                     unsigned long long seed) {
    const long n_om = (long)F * Dp, n_b = F, n_w = (long)Spad * F, n_e = (long)S * N;
    const long total = n_om + n_b + n_w + n_e;
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
        if (e < n_om) {
            const int i = (int)(e / Dp), d = (int)(e - (long)i * Dp);
            double v = 0.0;
            if (d < D) {
                v = ts_normal((unsigned long long)i * D + d, 0u, seed);
                if (nu2 > 0) {
                    double chi = 0.0;
                    for (int j = 0; j < nu2; ++j) {
                        const double n = ts_normal(8ull * i + j, 1u, seed);
                        chi = fma(n, n, chi);
                    }
                    v = v * sqrt((double)nu2 / chi);
                }
            }
            omega[e] = v;
        } else if (e < n_om + n_b) {
            const long i = e - n_om;
            uint32_t r[4];
            ts_words((unsigned long long)i, 2u, seed, r);
            b[i] = TS_TWO_PI * ts_u53(r[0], r[1]);
        } else if (e < n_om + n_b + n_w) {
            const long k = e - n_om - n_b;
            const long s = k / F;
            W[k] = s < S ? ts_normal((unsigned long long)k, 3u, seed) : 0.0;
        } else {
            const long k = e - n_om - n_b - n_w;
            eps[k] = eps_sd * ts_normal((unsigned long long)k, 4u, seed);
        }
    }
}

struct TsPass {
    const double *P; int rows, ld;                 // points (rows, ld = Dp), scaled; read up to the 64-row tile's end
    const double *omega, *b, *W; int F; double pscale;   // pscale = sqrt(2c / F)
    const double *Xs, *V; int N, Np, Dp; double constant;   // V (16 SG, Np); N = 0: the prior alone
    double *out; int S; double o0, o1;             // out[row * S + s] = o0 + o1 f_s(row)
};

constexpr int TS_CT = 64;   // points per workgroup

// 4 waves; point (a, r) of the tile is row 4 r + a (a < 4: the lane's four points are adjacent).  The waves split the
// feature chunks (wave w: chunks w, w + 4, ...) and each 128-point training step (wave w: points 32 w .. 32 w + 31);
// their accumulators acc[a] = f for samples s0 + (lane >> 4) + 4 t, point (a, lane & 15), are added in LDS at the end.
// One group of 16 samples per workgroup (s0 = 16 blockIdx.y): S = 64 repeats the distances four times, but the kernel
// keeps 16 accumulators a lane.  (A variant holding all four groups, 64 accumulators a lane, gave wrong sums for one
// accumulator element in tests at N <= 128 and was not pursued.)
template <int KIND>
__global__ __launch_bounds__(256) void ts_pass_kernel(TsPass p) {
    constexpr int SG = 1;
    using St = KsStage<double>;
    constexpr int DC = St::DC, LD = St::LD;
    static_assert(16 * SG * (TS_CT + 1) <= 2 * DC * LD, "the reduction reuses the staging buffers");
    __shared__ __attribute__((aligned(16))) double smem[2 * DC * LD];
    double (*Ct)[LD] = reinterpret_cast<double (*)[LD]>(smem);
    double (*Xt)[LD] = reinterpret_cast<double (*)[LD]>(smem + DC * LD);
    double (*red)[TS_CT + 1] = reinterpret_cast<double (*)[TS_CT + 1]>(smem);   // after the staging is done
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, kq = lane >> 4;
    const int c0 = blockIdx.x * TS_CT;
    const int s0 = 16 * (int)blockIdx.y;
    d4_t acc[4][SG];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int g = 0; g < SG; ++g) acc[a][g] = d4_t{0.0, 0.0, 0.0, 0.0};

    // ---- (a) the prior
    const int Dp = p.Dp;
    for (int fc = wave; fc < p.F / 16; fc += 4) {
        const int f0 = 16 * fc;
        d4_t ph[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) ph[a] = d4_t{0.0, 0.0, 0.0, 0.0};
        const double *om = p.omega + (long)(f0 + r) * Dp + kq;
#pragma unroll 1
        for (int d0 = 0; d0 < Dp; d0 += 4) {
            const double av = om[d0];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int row = c0 + 4 * r + a;
                const double bv = row < p.rows ? p.P[(long)row * p.ld + d0 + kq] : 0.0;
                ph[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, ph[a], 0, 0, 0);
            }
        }
        // ph[a][t]: phase of feature f0 + kq + 4 t at point (a, r) -- as it lies, the B operand of MFMA t below
        double bb[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) bb[t] = p.b[f0 + kq + 4 * t];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int t = 0; t < 4; ++t) ph[a][t] = p.pscale * cos(ph[a][t] + bb[t]);
#pragma unroll
        for (int g = 0; g < SG; ++g) {
            const double *wr = p.W + (long)(s0 + 16 * g + r) * p.F + f0 + kq;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const double wv = wr[4 * t];
#pragma unroll
                for (int a = 0; a < 4; ++a) acc[a][g] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv, ph[a][t], acc[a][g], 0, 0, 0);
            }
        }
    }

    // ---- (b) the update: bt_pass_kernel's staging (64 points, 128 training points, DC dimensions at a time)
    const int njt = (p.N + 127) / 128;
    const int nch = (Dp + DC - 1) / DC;
    const int nsteps = njt * nch;
    const bool one_pass = nch == 1;
    const int crows = c0 + TS_CT < p.rows ? c0 + TS_CT : p.rows;
    St sp, sq;
    double d2[4][2][4];
    if (nsteps > 0) {
        sp.load(p.P, c0, crows, Dp, 0);
        sq.load(p.Xs, 0, p.Np, Dp, 0);
        sp.store(Ct);
        sq.store(Xt);
    }
    __syncthreads();
    const int xoff = 32 * wave + 4 * kq;   // the lane's training points: xoff + 16 bb + t
    for (int st = 0; st < nsteps; ++st) {
        const int jt = st / nch, ch = st - jt * nch;
        const bool more = (st + 1) < nsteps;
        if (more) {
            const int jn = (st + 1) / nch, cn = (st + 1) - jn * nch;
            if (!one_pass) sp.load(p.P, c0, crows, Dp, cn * DC);
            sq.load(p.Xs, jn * 128, p.Np, Dp, cn * DC);
        }
        if (ch == 0) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int t = 0; t < 4; ++t) d2[a][q][t] = 0.0;
        }
        {
            int dn = Dp - ch * DC;
            if (dn > DC) dn = DC;
#pragma unroll 1
            for (int d4 = 0; d4 < dn; d4 += 4) {
#pragma unroll
                for (int dd = 0; dd < 4; ++dd) {
                    const int d = d4 + dd;
                    double cv[4], xv[2][4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) cv[a] = Ct[d][4 * r + a + St::rot(d4)];
#pragma unroll
                    for (int q = 0; q < 2; ++q)
#pragma unroll
                        for (int t = 0; t < 4; ++t) xv[q][t] = Xt[d][xoff + 16 * q + t + St::rot(d4)];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int q = 0; q < 2; ++q)
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                const double df = cv[a] - xv[q][t];
                                d2[a][q][t] = fma(df, df, d2[a][q][t]);
                            }
                }
            }
        }
        if (ch == nch - 1) {
            // kernel value of point (a, r) and training point j0 + xoff + 16 q + t: the B operand of MFMA t; V[s][that
            // point] the A operand (V is zero from N on)
            const int j0 = jt * 128;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int t = 0; t < 4; ++t) d2[a][q][t] = kernel_value<double, KIND>(d2[a][q][t], p.constant);
#pragma unroll
            for (int g = 0; g < SG; ++g)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const d4_t vv = *reinterpret_cast<const d4_t *>(p.V + (long)(s0 + 16 * g + r) * p.Np + j0 + xoff + 16 * q);
#pragma unroll
                    for (int t = 0; t < 4; ++t)
#pragma unroll
                        for (int a = 0; a < 4; ++a)
                            acc[a][g] = __builtin_amdgcn_mfma_f64_16x16x4f64(vv[t], d2[a][q][t], acc[a][g], 0, 0, 0);
                }
        }
        if (more) {
            __syncthreads();
            if (!one_pass) sp.store(Ct);
            sq.store(Xt);
            __syncthreads();
        }
    }

    // ---- the four waves' shares, added in a fixed order
    __syncthreads();
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int g = 0; g < SG; ++g)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        double &dst = red[16 * g + kq + 4 * t][4 * r + a];
                        dst = (w == 0) ? acc[a][g][t] : dst + acc[a][g][t];
                    }
        }
        __syncthreads();
    }
    const int ns = p.S - s0 < 16 ? p.S - s0 : 16;
    for (int e = tid; e < TS_CT * ns; e += 256) {
        const int c = e / ns, sl = e - c * ns;
        const int row = c0 + c;
        if (row < p.rows) p.out[(long)row * p.S + s0 + sl] = p.o0 + p.o1 * red[sl][c];
    }
}

// R[s][n] = f_prior_s(X_n) + eps_s[n] (0 from N on)
__global__ __launch_bounds__(256) void ts_resid_kernel(const double *__restrict__ priorX, const double *__restrict__ eps,
                                                       double *__restrict__ R, int S, int N, int Np) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)S * Np) return;
    const int s = (int)(e / Np), n = (int)(e - (long)s * Np);
    R[e] = n < N ? priorX[(long)n * S + s] + eps[(long)s * N + n] : 0.0;
}

// V[s][n] = alpha[n] - (K^-1 R_s)[n] (0 from N on; rows >= S stay zero)
__global__ __launch_bounds__(256) void ts_vfinish_kernel(const double *__restrict__ alpha, double *__restrict__ V, int S,
                                                         int N, int Np) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long)S * Np) return;
    const int n = (int)(e % Np);
    V[e] = n < N ? alpha[n] - V[e] : 0.0;
}

// per block of 256 candidates and sample s0 + blockIdx.y: the (sf f, lowest index) arg-max of the unmasked rows
__global__ __launch_bounds__(256) void ts_argmax_part_kernel(const double *__restrict__ f, long M, int S, int s0,
                                                             double sf, const unsigned char *__restrict__ mask,
                                                             double *__restrict__ bval, long long *__restrict__ bidx,
                                                             long nblk) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const int tid = threadIdx.x;
    const int s = s0 + (int)blockIdx.y;
    const long x = (long)blockIdx.x * 256 + tid;
    Best best;
    if (x < M && !mask[x]) best = candidate(sf * f[x * S + s], x);
    block_argmax<256>(best, sv, si);
    if (tid == 0) {
        bval[(long)blockIdx.y * nblk + blockIdx.x] = sv[0];
        bidx[(long)blockIdx.y * nblk + blockIdx.x] = si[0];
    }
}

// selection of sample s0 + blockIdx.x from the partials: index, raw value, its row gathered; distinct: masked from now on
__global__ __launch_bounds__(256) void ts_argmax_final_kernel(const double *__restrict__ bval,
                                                              const long long *__restrict__ bidx, long nblk,
                                                              const double *__restrict__ f, const double *__restrict__ cand,
                                                              long M, int S, int D, int s0, unsigned char *__restrict__ mask,
                                                              int distinct, long long *__restrict__ sel_idx,
                                                              double *__restrict__ sel_val, double *__restrict__ sel_x) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const int j = blockIdx.x, s = s0 + j;
    const double *bv = bval + (long)j * nblk;
    const long long *bx = bidx + (long)j * nblk;
    block_argmax<256>(strided_argmax<256>(bv, bx, nblk), sv, si);
    long long w = si[0];
    if (w < 0 || w >= M) w = M - 1;   // (never: S <= M with distinct leaves an unmasked row, and every one takes part)
    for (int d = threadIdx.x; d < D; d += 256) sel_x[(long)s * D + d] = cand[w * D + d];
    if (threadIdx.x == 0) {
        sel_idx[s] = w;
        sel_val[s] = f[w * S + s];
        if (distinct) mask[w] = 1;
    }
}

// one workgroup per query point: out[s] (raw f_s) and grad[s][d] (d f_s / d x_d), accumulated in LDS over chunks of 256
// features, then of 256 training points.  lds: [u (Dp) | acc (S (1 + D)) | two chunk arrays (256 each)]
struct TsEval {
    const double *Xq, *ls, *omega, *b, *W, *Xs, *V;
    int m, D, Dp, F, S, N, Np;
    double pscale, constant, y_mean, y_std;
    double *fout, *gout;   // gout nullable
};
template <int KIND>
__global__ __launch_bounds__(256) void ts_eval_kernel(TsEval p) {
    extern __shared__ double sm[];
    const int q = blockIdx.x, tid = threadIdx.x;
    const int D = p.D, Dp = p.Dp, S = p.S, per = 1 + D;
    const int nout = p.gout ? S * per : S;
    const int stride = p.gout ? per : 1;
    double *u = sm, *acc = u + Dp, *ca = acc + S * per, *cb = ca + 256;
    for (int d = tid; d < Dp; d += 256) u[d] = d < D ? p.Xq[(long)q * D + d] / p.ls[d] : 0.0;
    for (int o = tid; o < S * per; o += 256) acc[o] = 0.0;
    __syncthreads();
    for (int i0 = 0; i0 < p.F; i0 += 256) {
        const int cnt = p.F - i0 < 256 ? p.F - i0 : 256;
        if (tid < cnt) {
            const int i = i0 + tid;
            double ph = 0.0;
            const double *om = p.omega + (long)i * Dp;
            for (int d = 0; d < D; ++d) ph = fma(om[d], u[d], ph);
            double sn, cs;
            sincos(ph + p.b[i], &sn, &cs);
            ca[tid] = p.pscale * cs;
            cb[tid] = -p.pscale * sn;
        }
        __syncthreads();
        for (int o = tid; o < nout; o += 256) {
            const int s = o / stride, d = o - s * stride - 1;
            const double *wr = p.W + (long)s * p.F + i0;
            double a = 0.0;
            if (d < 0) {
                for (int k = 0; k < cnt; ++k) a = fma(wr[k], ca[k], a);
            } else {
                for (int k = 0; k < cnt; ++k) a = fma(wr[k] * cb[k], p.omega[(long)(i0 + k) * Dp + d], a);
            }
            acc[s * per + d + 1] += a;
        }
        __syncthreads();
    }
    for (int n0 = 0; n0 < p.N; n0 += 256) {
        {
            const int n = n0 + tid;
            double kv = 0.0, hv = 0.0;
            if (n < p.N) {
                const double *xn = p.Xs + (long)n * Dp;
                double d2 = 0.0;
                for (int d = 0; d < D; ++d) {
                    const double df = u[d] - xn[d];
                    d2 = fma(df, df, d2);
                }
                kv = kernel_value<double, KIND>(d2, p.constant);
                hv = p.constant * h_weight<KIND>(d2);
            }
            ca[tid] = kv;
            cb[tid] = hv;
        }
        __syncthreads();
        const int cnt = p.N - n0 < 256 ? p.N - n0 : 256;
        for (int o = tid; o < nout; o += 256) {
            const int s = o / stride, d = o - s * stride - 1;
            const double *vr = p.V + (long)s * p.Np + n0;
            double a = 0.0;
            if (d < 0) {
                for (int k = 0; k < cnt; ++k) a = fma(vr[k], ca[k], a);
            } else {
                for (int k = 0; k < cnt; ++k) a = fma(vr[k] * cb[k], p.Xs[(long)(n0 + k) * Dp + d] - u[d], a);
            }
            acc[s * per + d + 1] += a;
        }
        __syncthreads();
    }
    for (int o = tid; o < nout; o += 256) {
        const int s = o / stride, d = o - s * stride - 1;
        const double a = acc[s * per + d + 1];
        if (d < 0) p.fout[(long)q * S + s] = p.y_mean + p.y_std * a;
        else p.gout[((long)q * S + s) * D + d] = p.y_std * a / p.ls[d];
    }
}

// ---- launchers ----
int ts_spad(int64_t S) { return S <= 16 ? 16 : (S <= 32 ? 32 : 64); }

hipError_t launch_ts_pass(Context &c, const TsDraw &t, const double *P, int64_t rows, bool update, double *out,
                          double o0, double o1) {
    TsPass p{};
    p.P = P; p.rows = (int)rows; p.ld = (int)c.Dp;
    p.omega = t.omega; p.b = t.b; p.W = t.W; p.F = (int)t.F; p.pscale = sqrt(2.0 * c.constant / (double)t.F);
    p.Xs = c.d_Xs; p.V = t.V; p.N = update ? (int)c.N : 0; p.Np = (int)c.Np; p.Dp = (int)c.Dp; p.constant = c.constant;
    p.out = out; p.S = (int)t.S; p.o0 = o0; p.o1 = o1;
    const dim3 grid((unsigned)((rows + TS_CT - 1) / TS_CT), (unsigned)(ts_spad(t.S) / 16));
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return ts_pass_kernel<K()>; }), grid, dim3(256), 0, c.stream, p);
    return hipGetLastError();
}

hipError_t launch_ts_draw(Context &c, const TsDraw &t, unsigned long long seed, double *priorX, double *R, double *Z) {
    const int S = (int)t.S, Spad = ts_spad(t.S), N = (int)c.N, Np = (int)c.Np;
    const int nu2 = c.kernel == TGP_MATERN12 ? 1 : (c.kernel == TGP_MATERN32 ? 3 : (c.kernel == TGP_MATERN52 ? 5 : 0));
    const long total = t.F * c.Dp + t.F + (long)Spad * t.F + (long)S * N;
    const unsigned blocks = (unsigned)std::min<long>((total + 255) / 256, 8192);
    hipLaunchKernelGGL(ts_rng_kernel, dim3(blocks), dim3(256), 0, c.stream, t.omega, t.b, t.W, t.eps, (int)t.F, (int)c.D,
                       (int)c.Dp, S, Spad, N, nu2, sqrt(c.noise + c.jitter), seed);
    TGP_TRY(hipGetLastError());
    // the prior at the training points (the same feature code as the candidates), then R = prior + eps
    TGP_TRY(launch_ts_pass(c, t, c.d_Xs, c.N, false, priorX, 0.0, 1.0));
    const long nr = (long)S * Np;
    hipLaunchKernelGGL(ts_resid_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, c.stream, priorX, t.eps, R, S, N, Np);
    TGP_TRY(hipGetLastError());
    // V = alpha - Linv^T (Linv R)
    TGP_TRY(hipMemsetAsync(t.V, 0, (size_t)Spad * Np * sizeof(double), c.stream));
    TGP_TRY(launch_linv_solve(c, R, Z, t.V, S));
    hipLaunchKernelGGL(ts_vfinish_kernel, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, c.stream, c.d_alpha, t.V, S, N, Np);
    return hipGetLastError();
}

// the sampled maxima of max-value entropy search (tgp_mes_draw): the Thompson sweep's winners, none worse than the incumbent
__global__ void mes_take_kernel(const double *__restrict__ src, int S, double sf, double incumbent, double *__restrict__ dst) {
    const int s = threadIdx.x;
    if (s >= S) return;
    const double y = src[s];
    dst[s] = sf * incumbent > sf * y ? incumbent : y;
}

hipError_t launch_mes_take(Context &c, const double *src, int S, double sf, double incumbent, double *dst) {
    hipLaunchKernelGGL(mes_take_kernel, dim3(1), dim3(MES_MAXS), 0, c.stream, src, S, sf, incumbent, dst);
    return hipGetLastError();
}

hipError_t launch_ts_select(Context &c, const TsDraw &t, const double *f, double sf, int distinct, unsigned char *mask,
                            double *bval, long long *bidx, long long *sel_idx, double *sel_val, double *sel_x) {
    const long M = (long)c.M, nblk = (M + 255) / 256;
    const int S = (int)t.S;
    TGP_TRY(hipMemsetAsync(mask, 0, (size_t)M, c.stream));
    const int rounds = distinct ? S : 1, per = distinct ? 1 : S;
    for (int k = 0; k < rounds; ++k) {
        const int s0 = k * per;
        hipLaunchKernelGGL(ts_argmax_part_kernel, dim3((unsigned)nblk, (unsigned)per), dim3(256), 0, c.stream, f, M, S, s0,
                           sf, mask, bval, bidx, nblk);
        TGP_TRY(hipGetLastError());
        hipLaunchKernelGGL(ts_argmax_final_kernel, dim3((unsigned)per), dim3(256), 0, c.stream, bval, bidx, nblk, f,
                           c.d_cand, M, S, (int)c.D, s0, mask, distinct, sel_idx, sel_val, sel_x);
        TGP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

size_t ts_eval_lds_bytes(const Context &c, int64_t S) {
    return (size_t)(c.Dp + S * (1 + c.D) + 512) * sizeof(double);
}

hipError_t launch_ts_eval(Context &c, const TsDraw &t, const double *Xq, int m, double *fout, double *gout) {
    TsEval p{};
    p.Xq = Xq; p.ls = c.d_ls; p.omega = t.omega; p.b = t.b; p.W = t.W; p.Xs = c.d_Xs; p.V = t.V;
    p.m = m; p.D = (int)c.D; p.Dp = (int)c.Dp; p.F = (int)t.F; p.S = (int)t.S; p.N = (int)c.N; p.Np = (int)c.Np;
    p.pscale = sqrt(2.0 * c.constant / (double)t.F); p.constant = c.constant; p.y_mean = c.y_mean; p.y_std = c.y_std;
    p.fout = fout; p.gout = gout;
    const size_t sh = ts_eval_lds_bytes(c, t.S);
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return ts_eval_kernel<K()>; }), dim3((unsigned)m), dim3(256), sh, c.stream, p);
    return hipGetLastError();
}

}  // namespace tgp
