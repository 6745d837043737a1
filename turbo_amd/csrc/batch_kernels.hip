// batch_kernels.hip -- greedy selection of q candidates with Kriging Believer / Constant Liar (tgp_sweep_batch).
//
// The reference stubs batch selection out (turbo/optimiser.py:44-45, :361-396); the author's older library shipped it
// (old_library/bayesian_optimiser.py:76-103, Kriging Believer :527-566, the incumbent over real AND hypothesised costs
// :509).  With the hyper-parameters and the normalisation held, conditioning on one more (fantasised) observation z_j
// changes every candidate's posterior by a rank-1 update (normalised units; G (M x j) holds the scaled cross-covariance
// columns of the points conditioned so far, R (j x j) their block of the augmented factor):
//
//   w_j     = K^-1 k*(z_j)                                       (launch_query_front: two triangular products with Linv)
//   R[j,i]  = (S[j,i] - sum_{l<i} R[j,l] R[i,l]) / R[i,i],   R[j,j] = sqrt(S[j,j] - sum_{l<j} R[j,l]^2)
//             with S[j,i] = c k(z_j, z_i) - k*(z_i).w_j  and  S[j,j] = c + noise + jitter - k*(z_j).w_j
//   c(x)    = c k(x, z_j) - k*(x).w_j - sum_{i<j} G[x,i] R[j,i]                    (every candidate x)
//   G[x,j]  = c(x) / R[j,j],   var(x) -= G[x,j]^2 (clamped at 0, counted),   mu(x) += G[x,j] e_j
//   e_j     = (y~_j - mu~_{j-1}(z_j)) / R[j,j],   mu~_{j-1}(z_j) = k*(z_j).alpha + sum_{i<j} R[j,i] e_i   (KB: e_j = 0)
//
// bt_small_kernel forms the R row, the fantasy and e_j for one point (one workgroup); bt_pass_kernel is the one O(M N D)
// pass per point -- kstar_kernel's tiles (sweep_kernels.hip) with w_j in place of alpha and no slab written; bt_update_kernel
// applies the update (bt_rank1), evaluates the acquisition (acq_value, acq_math.hpp: every sweep's formulas) and leaves
// per-block arg-max partials that bt_argmax_kernel turns into the next selection, in device memory.  Everything here is f64, whatever the handle's
// sweep dtype.
//
// Monte Carlo (tgp_sweep_batch_mc; old_library/bayesian_optimiser.py:76-106, _max_mc_acq_suggestion :568-624): S
// simulations of the pending and selected points' outcomes, and the AVERAGE of the S acquisition functions maximised.
// With the hyper-parameters held the variance update above does not depend on the fantasised values and the mean is
// linear in them through the stored columns of G, so one conditioned point costs one bt_pass_kernel pass whatever S is:
//
//   y~[s,j]  = mu~_{s,j-1}(z_j) + R[j,j] eps[s,j],  eps[s,j] ~ N(0,1)        a draw of the OBSERVATION y (R[j,j]^2 holds
//              mu~_{s,j-1}(z_j) = k*(z_j).alpha + sum_{i<j} R[j,i] eps[s,i]    noise + jitter), so e[s,j] = eps[s,j]
//   mu~_s(x) = mu0(x) + sum_{i<=j} G[x,i] eps[s,i],   sigma~(x) shared: the update above
//   inc_s    = best(incumbent, the raw fantasies of simulation s so far) in the direction of sf        (EI / PI)
//   a(x)     = (1/S) sum_s acq(y_mean + y_std mu~_s(x), y_std sigma~(x); inc_s),   summed in the order s = 0, 1, ...
//
// The draw is JOINT: point j is drawn given simulation s's own draws of the points before it.  The old library draws
// every pending point on its own from the concrete model (:582-585), which ignores that two nearby pending points come
// out alike; with one pending point the two coincide.  eps[s,j] is a Philox-4x32-10 normal (philox.hpp) keyed by the
// seed, counter (element lo, element hi, 0, MC_TAG), element s 64 + j with j counted pending-first: simulation s does
// not depend on S, the draw for point j not on P or q.  mc_small_kernel stands in bt_small_kernel's place and
// mc_update_kernel in bt_update_kernel's, each pair on one shared body (bt_factor_row; bt_rank1 and bt_finish_block); the
// point, front, pass and arg-max kernels are shared.
#include <hip/hip_runtime.h>
#include <math.h>

#include "acq_math.hpp"
#include "pairwise.hpp"
#include "philox.hpp"
#include "tgp_internal.hpp"

namespace tgp {

#define TGP_TRY(x)                         \
    do {                                   \
        hipError_t e_ = (x);               \
        if (e_ != hipSuccess) return e_;   \
    } while (0)

constexpr int BT_CT = 64;          // candidates per tile of the pass (AR = 4)
constexpr int BT_BLOCK = 256;      // candidates per block of the update = per arg-max partial

// Cs (Mpad, Dp) = candidates / length scales, rows >= M and columns >= D zero
__global__ __launch_bounds__(256) void bt_prep_kernel(const double *__restrict__ cand, const double *__restrict__ ls,
                                                      double *__restrict__ Cs, long M, long Mpad, int D, int Dp) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= Mpad * Dp) return;
    const long r = e / Dp;
    const int d = (int)(e - r * Dp);
    Cs[e] = (r < M && d < D) ? cand[r * D + d] / ls[d] : 0.0;
}

// the state the steps update: var~ = (sigma / s_y)^2 of the first sweep, its means, no row selected
__global__ __launch_bounds__(256) void bt_init_kernel(const double *__restrict__ mu0, const double *__restrict__ sg0,
                                                      double *__restrict__ mu, double *__restrict__ var,
                                                      unsigned char *__restrict__ mask, long M, double y_std) {
    const long x = (long)blockIdx.x * 256 + threadIdx.x;
    if (x >= M) return;
    const double s = sg0[x] / y_std;
    mu[x] = mu0[x];
    var[x] = s * s;
    mask[x] = 0;
}


// selection k's candidate row -> the raw coordinates of conditioned point j.  from_rec: selection 0 is the first sweep's
// arg-max, read from its result record [value, index, clamp count]
__global__ __launch_bounds__(64) void bt_point_kernel(const double *__restrict__ rec, BtSmall s, int k,
                                                      const double *__restrict__ cand, double *__restrict__ zraw,
                                                      unsigned char *__restrict__ mask, long M, int D) {
    long long idx;
    if (rec) {
        idx = (long long)rec[1];
        if (idx < 0 || idx >= M) idx = 0;
        if (threadIdx.x == 0) {
            s.sel_idx[k] = idx;
            s.sel_val[k] = rec[0];
            mask[idx] = 1;
        }
    } else {
        idx = s.sel_idx[k];
    }
    for (int d = threadIdx.x; d < D; d += 64) zraw[d] = cand[idx * D + d];
}

__device__ __forceinline__ double bt_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// what the two small kernels share, one workgroup: S[i] = k*(z_i).w_j (i <= j), k*(z_j).alpha, the cross-kernel between
// z_j and the earlier points, then thread 0's R row j, pivot test and flag.  Returns, in thread 0 only, R[j,j] and
// m = k*(z_j).alpha + sum_{i<j} R[j,i] e[i] (e null: the first term alone) accumulated inside the row loop, i ascending;
// Rl (nullable, LDS) receives a copy of the row.  red (256), S (BT_MAXP + 1) and Rl (BT_MAXP) are the caller's LDS; the
// caller synchronises before other threads read S[BT_MAXP] or Rl
struct BtRow { double m, rjj; };
template <int KIND>
__device__ __forceinline__ BtRow bt_factor_row(const double *__restrict__ Kz, const double *__restrict__ w,
                                               const double *__restrict__ alpha, const double *__restrict__ Zs,
                                               const BtSmall &s, int j, int N, int Np, int Dp, double constant,
                                               double noise, double jitter, const double *e, double *red, double *S,
                                               double *Rl) {
    const int tid = threadIdx.x;
    for (int i = 0; i <= j; ++i) {
        const double *k = Kz + (long)i * Np;
        double a = 0.0;
        for (int n = tid; n < N; n += 256) a = fma(k[n], w[n], a);
        a = bt_block_sum(a, red);
        if (tid == 0) S[i] = a;
    }
    {
        const double *k = Kz + (long)j * Np;
        double a = 0.0;
        for (int n = tid; n < N; n += 256) a = fma(k[n], alpha[n], a);
        a = bt_block_sum(a, red);
        if (tid == 0) S[BT_MAXP] = a;   // k*(z_j).alpha
    }
    __syncthreads();
    // the cross-kernel between z_j and the earlier points (no noise term)
    if (tid < j) {
        const double *zj = Zs + (long)j * Dp, *zi = Zs + (long)tid * Dp;
        double d2 = 0.0;
        for (int d = 0; d < Dp; ++d) {
            const double df = zj[d] - zi[d];
            d2 = fma(df, df, d2);
        }
        S[tid] = kernel_value<double, KIND>(d2, constant) - S[tid];
    }
    __syncthreads();
    BtRow r{0.0, 0.0};
    if (tid == 0) {
        double *Rj = s.R + (long)j * BT_MAXP;
        double m = S[BT_MAXP];
        double piv = ((constant + noise) + jitter) - S[j];
        for (int i = 0; i < j; ++i) {
            const double *Ri = s.R + (long)i * BT_MAXP;
            double t = S[i];
            for (int l = 0; l < i; ++l) t -= Rj[l] * Ri[l];
            t /= Ri[i];
            Rj[i] = t;
            if (Rl) Rl[i] = t;
            piv -= t * t;
            if (e) m += t * e[i];
        }
        if (!(piv > 0.0) || !isfinite(piv)) {
            if (s.flag[0] == 0) s.flag[0] = j + 1;
            piv = NAN;
        }
        const double rjj = sqrt(piv);
        Rj[j] = rjj;
        if (Rl) Rl[j] = rjj;
        r = BtRow{m, rjj};
    }
    return r;
}

// one workgroup: R row j (bt_factor_row), the fantasy of point j, e_j, the incumbent
template <int KIND>
__global__ __launch_bounds__(256) void bt_small_kernel(const double *__restrict__ Kz, const double *__restrict__ w,
                                                       const double *__restrict__ alpha, const double *__restrict__ Zs,
                                                       BtSmall s, int j, int N, int Np, int Dp, double constant,
                                                       double noise, double jitter, double y_mean, double y_std,
                                                       int kb, double lie, double sf) {
    __shared__ double red[256];
    __shared__ double S[BT_MAXP + 1];
    const BtRow r = bt_factor_row<KIND>(Kz, w, alpha, Zs, s, j, N, Np, Dp, constant, noise, jitter, s.e, red, S, nullptr);
    if (threadIdx.x == 0) {
        const double f = kb ? y_std * r.m + y_mean : lie;
        s.fant[j] = f;
        s.e[j] = kb ? 0.0 : ((f - y_mean) / y_std - r.m) / r.rjj;
        const double inc = s.inc[0];
        s.inc[0] = sf > 0.0 ? (f > inc ? f : inc) : (f < inc ? f : inc);
    }
}

// part[s][x] = sum over the training points of split s of c k0(x, X_n) w_n: kstar_kernel's 128 x 128 tiles (f64, AR = 8,
// direct sums of squared differences from LDS-staged, transposed point blocks) with w in place of alpha, nothing else written
template <int KIND>
__global__ __launch_bounds__(256, 2) void bt_pass_kernel(const double *__restrict__ Cs, const double *__restrict__ Xs,
                                                         const double *__restrict__ w, double *__restrict__ part, int rows,
                                                         int N, int Np, int Dp, double constant, long ldpart) {
    using St = KsStage<double>;
    constexpr int DC = St::DC, LD = St::LD, AR = 4;   // (64 f64 accumulators do not fit: 4 x 8, as kstar_kernel in f64)
    __shared__ __attribute__((aligned(16))) double Ct[DC][LD];
    __shared__ __attribute__((aligned(16))) double Xt[DC][LD];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int c0 = blockIdx.x * BT_CT;
    const int njt = Np / 128;
    const int per = (njt + (int)gridDim.y - 1) / (int)gridDim.y;
    const int jt0 = blockIdx.y * per;
    int jt_end = jt0 + per;
    if (jt_end > njt) jt_end = njt;
    const int jt_real = (N + 127) / 128;
    const int jt_live = jt_end < jt_real ? jt_end : jt_real;
    auto crow = [&](int a) { return (a < 4 ? 0 : 60) + 4 * ty + a; };
    auto jcol = [&](int b) { return ((b >> 1) << 5) + 2 * tx + (b & 1); };
    double pm[AR];
#pragma unroll
    for (int a = 0; a < AR; ++a) pm[a] = 0.0;
    const int nch = (Dp + DC - 1) / DC;
    const int nsteps = (jt_live > jt0 ? jt_live - jt0 : 0) * nch;
    const bool one_pass = (nch == 1);
    const int crows = c0 + BT_CT < rows ? c0 + BT_CT : rows;
    St sp, sq;
    double d2[AR][8];
    if (nsteps > 0) {
        sp.load(Cs, c0, crows, Dp, 0);
        sq.load(Xs, jt0 * 128, Np, Dp, 0);
        sp.store(Ct);
        sq.store(Xt);
    }
    __syncthreads();
    for (int st = 0; st < nsteps; ++st) {
        const int jt = jt0 + st / nch, ch = st - (st / nch) * nch;
        const int j0 = jt * 128;
        const bool more = (st + 1) < nsteps;
        if (more) {
            const int jn = jt0 + (st + 1) / nch, cn = (st + 1) - ((st + 1) / nch) * nch;
            if (!one_pass) sp.load(Cs, c0, crows, Dp, cn * DC);
            sq.load(Xs, jn * 128, Np, Dp, cn * DC);
        }
        if (ch == 0) {
#pragma unroll
            for (int a = 0; a < AR; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) d2[a][b] = 0.0;
        }
        {
            int dn = Dp - ch * DC;
            if (dn > DC) dn = DC;
#pragma unroll 1
            for (int d4 = 0; d4 < dn; d4 += 4) {
#pragma unroll
                for (int dd = 0; dd < 4; ++dd) {
                    const int d = d4 + dd;
                    double cv[AR], xv[8];
#pragma unroll
                    for (int a = 0; a < AR; ++a) cv[a] = Ct[d][crow(a) + St::rot(d4)];
#pragma unroll
                    for (int b = 0; b < 8; ++b) xv[b] = Xt[d][jcol(b) + St::rot(d4)];
#pragma unroll
                    for (int a = 0; a < AR; ++a)
#pragma unroll
                        for (int b = 0; b < 8; ++b) {
                            const double df = cv[a] - xv[b];
                            d2[a][b] = fma(df, df, d2[a][b]);
                        }
                }
            }
        }
        if (ch == nch - 1) {
            double wl[8];
            const bool edge = j0 + 128 > N;
#pragma unroll
            for (int b = 0; b < 8; ++b) wl[b] = (!edge || j0 + jcol(b) < N) ? w[j0 + jcol(b)] : 0.0;
#pragma unroll
            for (int a = 0; a < AR; ++a)
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const double kv = kernel_value<double, KIND>(d2[a][b], constant);
                    pm[a] = fma(kv, wl[b], pm[a]);
                }
        }
        if (more) {
            __syncthreads();
            if (!one_pass) sp.store(Ct);
            sq.store(Xt);
            __syncthreads();
        }
    }
#pragma unroll
    for (int a = 0; a < AR; ++a) {
        double s = pm[a];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (tx == 0) part[(long)blockIdx.y * ldpart + c0 + crow(a)] = s;
    }
}

// what the two update kernels are given alike (bt_upd_base fills it)
struct BtUpdBase {
    const double *cand, *ls, *zs;     // raw candidates (M, D), length scales, scaled z_j (Dp)
    const double *part; int njs; long ldpart;
    double *G; long ldG; int j;       // column j of G at G + j ldG
    double *var; const unsigned char *mask;
    long M; int D;
    double constant, y_std;
    int acq; double sf, param;        // acq == TGP_ACQ_NONE: no selection follows this point
    double *bval; long long *bidx; unsigned long long *clamp;
    double *sigma_out;                // nullable: sigma after this point
};

// candidate x's rank-1 step for point j (R: the call's factor block): c(x), G[x,j] (stored when a later point or mean
// reads it), the variance update with its clamp (counted in *sclamp, LDS) and sigma in raw units, written where asked
struct BtRank1 { double g, var, sigma; };
template <int KIND>
__device__ __forceinline__ BtRank1 bt_rank1(const BtUpdBase &u, const double *R, long x, int store, int *sclamp) {
    double kdot = 0.0;
    for (int s = 0; s < u.njs; ++s) kdot += u.part[(long)s * u.ldpart + x];
    double d2 = 0.0;
    for (int d = 0; d < u.D; ++d) {
        const double df = u.cand[x * u.D + d] / u.ls[d] - u.zs[d];
        d2 = fma(df, df, d2);
    }
    double cx = kernel_value<double, KIND>(d2, u.constant) - kdot;
    const double *Rj = R + (long)u.j * BT_MAXP;
    for (int i = 0; i < u.j; ++i) cx -= u.G[(long)i * u.ldG + x] * Rj[i];
    const double g = cx / Rj[u.j];
    if (store) u.G[(long)u.j * u.ldG + x] = g;
    double var = u.var[x] - g * g;
    if (var < 0.0) { var = 0.0; atomicAdd(sclamp, 1); }
    u.var[x] = var;
    const double sigma = sqrt(var * (u.y_std * u.y_std));
    if (u.sigma_out) u.sigma_out[x] = sigma;
    return BtRank1{g, var, sigma};
}

// the block's arg-max partial and its clamp count (sv, si: BT_BLOCK entries of LDS each)
__device__ __forceinline__ void bt_finish_block(const BtUpdBase &u, Best best, double *sv, long long *si, const int *sclamp) {
    best = block_argmax<BT_BLOCK>(best, sv, si);
    if (threadIdx.x == 0) {
        if (u.acq != TGP_ACQ_NONE) { u.bval[blockIdx.x] = best.v; u.bidx[blockIdx.x] = best.i; }
        if (*sclamp) atomicAdd(u.clamp, (unsigned long long)*sclamp);
    }
}

struct BtUpd {
    BtUpdBase b;
    BtSmall s;
    int store;                        // column j of G is kept: a later point reads it
    double *mu;                       // the running means, raw units
    double *mu_out;                   // nullable: the means after the last point
};

template <int KIND>
__global__ __launch_bounds__(BT_BLOCK) void bt_update_kernel(BtUpd u) {
    __shared__ double sv[BT_BLOCK];
    __shared__ long long si[BT_BLOCK];
    __shared__ int sclamp;
    const int tid = threadIdx.x;
    if (tid == 0) sclamp = 0;
    __syncthreads();
    const long x = (long)blockIdx.x * BT_BLOCK + tid;
    Best best;
    if (x < u.b.M) {
        const BtRank1 r = bt_rank1<KIND>(u.b, u.s.R, x, u.store, &sclamp);
        double mu = u.mu[x];
        const double e = u.s.e[u.b.j];
        if (e != 0.0) { mu += u.b.y_std * (r.g * e); u.mu[x] = mu; }
        if (u.mu_out) u.mu_out[x] = mu;
        if (u.b.acq != TGP_ACQ_NONE && !u.b.mask[x])
            best = candidate(acq_value(u.b.acq, u.b.sf, u.s.inc[0], u.b.param, mu, r.sigma), x);
    }
    bt_finish_block(u.b, best, sv, si, &sclamp);
}

// selection k = the (value, lowest index) of the partials; the row is masked for the rest of the call
__global__ __launch_bounds__(256) void bt_argmax_kernel(const double *__restrict__ bval, const long long *__restrict__ bidx,
                                                        long nblk, BtSmall s, int k, unsigned char *__restrict__ mask,
                                                        long M) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const Best b = block_argmax<256>(strided_argmax<256>(bval, bidx, nblk), sv, si);
    if (threadIdx.x == 0) {
        long long w = b.i;
        if (w < 0 || w >= M) w = M - 1;   // (never: q <= M leaves an unmasked row, and every unmasked row takes part)
        s.sel_idx[k] = w;
        s.sel_val[k] = b.v;
        mask[w] = 1;
    }
}

// ---- Monte Carlo: S simulations of every conditioned point's outcome ----
constexpr uint32_t MC_TAG = 0x4D435349u;   // "MCSI": the fourth counter word of the fantasies' normals
constexpr int MC_SC = 16;                  // simulations whose means a thread holds at a time

// eps (64, 64) POINT-major (eps[j * 64 + s]): the Philox normal of element s 64 + j for s < S, j < J, zero elsewhere;
// inc[s] = the incumbent
__global__ __launch_bounds__(256) void mc_init_kernel(double *__restrict__ eps, double *__restrict__ inc, int S, int J,
                                                      int draw, unsigned long long seed, double incumbent) {
    const int e = blockIdx.x * 256 + threadIdx.x;   // = j * 64 + s
    if (e >= BT_MAXP * MC_MAXS) return;
    const int j = e >> 6, s = e & 63;
    if (draw) eps[e] = (s < S && j < J) ? philox_normal((unsigned long long)s * 64ull + (unsigned long long)j, 0u, MC_TAG, seed) : 0.0;
    if (j == 0) inc[s] = incumbent;
}

// one workgroup: R row j and the pivot test (bt_factor_row, the row also left in LDS); then per simulation the
// conditional mean at z_j, the fantasy (a draw of y) and the incumbent
template <int KIND>
__global__ __launch_bounds__(256) void mc_small_kernel(const double *__restrict__ Kz, const double *__restrict__ w,
                                                       const double *__restrict__ alpha, const double *__restrict__ Zs,
                                                       McSmall s, int j, int N, int Np, int Dp, double constant,
                                                       double noise, double jitter, double y_mean, double y_std,
                                                       double sf) {
    __shared__ double red[256];
    __shared__ double S[BT_MAXP + 1];
    __shared__ double Rl[BT_MAXP];
    const int tid = threadIdx.x;
    bt_factor_row<KIND>(Kz, w, alpha, Zs, s.b, j, N, Np, Dp, constant, noise, jitter, nullptr, red, S, Rl);
    __syncthreads();
    if (tid < s.S) {
        double m = S[BT_MAXP];
        for (int i = 0; i < j; ++i) m += Rl[i] * s.eps[i * MC_MAXS + tid];
        const double yn = m + Rl[j] * s.eps[j * MC_MAXS + tid];
        const double f = y_std * yn + y_mean;
        s.fant[j * MC_MAXS + tid] = f;
        const double inc = s.inc[tid];
        s.inc[tid] = sf > 0.0 ? (f > inc ? f : inc) : (f < inc ? f : inc);
    }
}

struct McUpd {
    BtUpdBase b;                      // (column j of G is always stored: the later means read it)
    McSmall s;
    const double *mu0;                // the first sweep's means, raw units: never updated
    double *acq_out;                  // nullable: this step's averaged acquisition (taken rows -inf)
};

// bt_rank1's step; then the S means from G[x, 0..j] and eps (LDS), S acquisition values (acq_value), their mean in the
// order s = 0, 1, ... and the per-block arg-max partials.  A thread per candidate: G is column-major, so its reads are
// coalesced; MC_SC means at a time stay in registers (plain f64 FMAs: at S = J = 64 the erf / exp evaluations outweigh
// the product)
template <int KIND>
__global__ __launch_bounds__(BT_BLOCK) void mc_update_kernel(McUpd u) {
    __shared__ double sv[BT_BLOCK];
    __shared__ long long si[BT_BLOCK];
    __shared__ int sclamp;
    __shared__ __attribute__((aligned(16))) double epsl[BT_MAXP * MC_MAXS];   // [i][s]
    __shared__ double incl[MC_MAXS];
    const int tid = threadIdx.x;
    const int j = u.b.j, S = u.s.S;
    if (tid == 0) sclamp = 0;
    if (u.b.acq != TGP_ACQ_NONE && u.b.acq != TGP_ACQ_SIGMA) {
        for (int e = tid; e < (j + 1) * MC_MAXS; e += BT_BLOCK) epsl[e] = u.s.eps[e];
        if (tid < MC_MAXS) incl[tid] = u.s.inc[tid];
    }
    __syncthreads();
    const long x = (long)blockIdx.x * BT_BLOCK + tid;
    Best best;
    if (x < u.b.M) {
        const BtRank1 r = bt_rank1<KIND>(u.b, u.s.b.R, x, 1, &sclamp);
        const double g = r.g, sigma = r.sigma;
        if (u.b.acq != TGP_ACQ_NONE) {
            if (!u.b.mask[x]) {
                double a;
                if (u.b.acq == TGP_ACQ_SIGMA) {
                    a = sigma;                 // the same for every simulation: no average to round
                } else {
                    const double mu0 = u.mu0[x];
                    double sum = 0.0;
                    for (int s0 = 0; s0 < S; s0 += MC_SC) {
                        double acc[MC_SC];
#pragma unroll
                        for (int t = 0; t < MC_SC; ++t) acc[t] = 0.0;
                        for (int i = 0; i <= j; ++i) {
                            const double gi = i == j ? g : u.b.G[(long)i * u.b.ldG + x];
                            const double *er = epsl + i * MC_MAXS + s0;
#pragma unroll
                            for (int t = 0; t < MC_SC; ++t) acc[t] = fma(gi, er[t], acc[t]);
                        }
#pragma unroll
                        for (int t = 0; t < MC_SC; ++t) {
                            if (s0 + t < S) {
                                const double mu = mu0 + u.b.y_std * acc[t];
                                sum += acq_value(u.b.acq, u.b.sf, incl[s0 + t], u.b.param, mu, sigma);
                            }
                        }
                    }
                    a = sum / (double)S;
                }
                best = candidate(a, x);
            }
            if (u.acq_out) u.acq_out[x] = best.v;
        }
    }
    bt_finish_block(u.b, best, sv, si, &sclamp);
}

// ---- launchers ----
int bt_pass_splits(const Context &c, int64_t M) {
    const int64_t tiles = (M + BT_CT - 1) / BT_CT;
    const int live = (int)((c.N + 127) / 128);
    int js = (int)std::max<int64_t>(1, 1024 / std::max<int64_t>(tiles, 1));   // about four workgroups per CU
    return std::min(std::min(js, live), KS_JS);
}

hipError_t launch_bt_prep(Context &c, double *Cs, int64_t Mpad) {
    const long n = (long)Mpad * c.Dp;
    hipLaunchKernelGGL(bt_prep_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c.stream, c.d_cand, c.d_ls, Cs,
                       (long)c.M, (long)Mpad, (int)c.D, (int)c.Dp);
    return hipGetLastError();
}

hipError_t launch_bt_init(Context &c, double *mu, double *var, unsigned char *mask) {
    hipLaunchKernelGGL(bt_init_kernel, dim3((unsigned)((c.M + 255) / 256)), dim3(256), 0, c.stream, c.d_mu, c.d_sigma,
                       mu, var, mask, (long)c.M, c.y_std);
    return hipGetLastError();
}

hipError_t launch_bt_point(Context &c, const double *rec, const BtSmall &s, int k, double *zraw, unsigned char *mask) {
    hipLaunchKernelGGL(bt_point_kernel, dim3(1), dim3(64), 0, c.stream, rec, s, k, c.d_cand, zraw, mask, (long)c.M,
                       (int)c.D);
    return hipGetLastError();
}

// the front of point j (its vectors into slot j of Kz / Zs) and its small side: mc_small_kernel when mc is given
hipError_t launch_bt_condition(Context &c, const BatchWs &ws, const BtSmall &s, const McSmall *mc, int j, int kb,
                               double lie, double sf) {
    TGP_TRY(launch_query_front(c, ws.Zraw + (long)j * c.D, ws.Zs + (long)j * c.Dp, ws.Kz + (long)j * c.Np, ws.hw, ws.v, ws.w));
    if (mc)
        hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return mc_small_kernel<K()>; }), dim3(1), dim3(256), 0, c.stream, ws.Kz, ws.w,
                           c.d_alpha, ws.Zs, *mc, j, (int)c.N, (int)c.Np, (int)c.Dp, c.constant, c.noise, c.jitter, c.y_mean, c.y_std, sf);
    else
        hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return bt_small_kernel<K()>; }), dim3(1), dim3(256), 0, c.stream, ws.Kz, ws.w,
                           c.d_alpha, ws.Zs, s, j, (int)c.N, (int)c.Np, (int)c.Dp, c.constant, c.noise, c.jitter, c.y_mean, c.y_std, kb, lie, sf);
    return hipGetLastError();
}

// the pass over every candidate for the point whose w is in ws.w
static hipError_t launch_bt_pass(Context &c, const BatchWs &ws) {
    const dim3 gp((unsigned)((c.M + BT_CT - 1) / BT_CT), (unsigned)ws.js);
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return bt_pass_kernel<K()>; }), gp, dim3(256), 0, c.stream, ws.Cs, c.d_Xs, ws.w,
                       ws.part, (int)c.M, (int)c.N, (int)c.Np, (int)c.Dp, c.constant, (long)ws.Mpad);
    return hipGetLastError();
}

static BtUpdBase bt_upd_base(const Context &c, const BatchWs &ws, int j, int acq, double sf, double param, double *sigma_out) {
    BtUpdBase u{};
    u.cand = c.d_cand; u.ls = c.d_ls; u.zs = ws.Zs + (long)j * c.Dp;
    u.part = ws.part; u.njs = ws.js; u.ldpart = (long)ws.Mpad;
    u.G = ws.G; u.ldG = (long)c.M; u.j = j;
    u.var = ws.bvar; u.mask = ws.mask;
    u.M = (long)c.M; u.D = (int)c.D;
    u.constant = c.constant; u.y_std = c.y_std;
    u.acq = acq; u.sf = sf; u.param = param;
    u.bval = ws.bval; u.bidx = ws.bidx; u.clamp = reinterpret_cast<unsigned long long *>(ws.clampw);
    u.sigma_out = sigma_out;
    return u;
}

// selection k from the update's partials
static hipError_t launch_bt_select(Context &c, const BatchWs &ws, const BtSmall &s, int k) {
    hipLaunchKernelGGL(bt_argmax_kernel, dim3(1), dim3(256), 0, c.stream, ws.bval, ws.bidx, (long)ws.nblk, s, k, ws.mask,
                       (long)c.M);
    return hipGetLastError();
}

// the pass for point j, its update, and (acq != NONE) selection k from the result
hipError_t launch_bt_step(Context &c, const BatchWs &ws, const BtSmall &s, int j, int store, int acq, double sf,
                          double param, double *mu_out, double *sigma_out, int k) {
    TGP_TRY(launch_bt_pass(c, ws));
    BtUpd u{};
    u.b = bt_upd_base(c, ws, j, acq, sf, param, sigma_out);
    u.s = s; u.store = store; u.mu = ws.bmu; u.mu_out = mu_out;
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return bt_update_kernel<K()>; }), dim3((unsigned)ws.nblk), dim3(BT_BLOCK), 0, c.stream, u);
    TGP_TRY(hipGetLastError());
    return acq != TGP_ACQ_NONE ? launch_bt_select(c, ws, s, k) : hipSuccess;
}

// ---- Monte Carlo launchers ----
hipError_t launch_mc_init(Context &c, const McSmall &s, int J, bool draw, unsigned long long seed, double incumbent) {
    hipLaunchKernelGGL(mc_init_kernel, dim3(BT_MAXP * MC_MAXS / 256), dim3(256), 0, c.stream, s.eps, s.inc, s.S, J,
                       draw ? 1 : 0, seed, incumbent);
    return hipGetLastError();
}

hipError_t launch_mc_step(Context &c, const BatchWs &ws, const McSmall &s, int j, int acq, double sf, double param,
                          double *acq_out, double *sigma_out, int k) {
    TGP_TRY(launch_bt_pass(c, ws));
    McUpd u{};
    u.b = bt_upd_base(c, ws, j, acq, sf, param, sigma_out);
    u.s = s; u.mu0 = ws.bmu; u.acq_out = acq_out;
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return mc_update_kernel<K()>; }), dim3((unsigned)ws.nblk), dim3(BT_BLOCK), 0, c.stream, u);
    TGP_TRY(hipGetLastError());
    return acq != TGP_ACQ_NONE ? launch_bt_select(c, ws, s.b, k) : hipSuccess;
}

}  // namespace tgp
