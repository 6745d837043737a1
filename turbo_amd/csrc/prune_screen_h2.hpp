// prune_screen_h2.hpp -- the pruned sweep's screen (prune_screen.hpp) with its dot products on the fp16 matrix
// pipe and an error term weighted by the computed kernel values.  Selected by TGP_SCREEN_ARITH=h2 (the default) for
// D >= SCRH_MIN_D; prune_screen.hpp's kernels are untouched and run for TGP_SCREEN_ARITH=f32 and for smaller D.
//
// Arithmetic.  Every operand is cut into two fp16 planes as trmm_f16x2.hpp does (split2_f16x2):
//     v s = v1 + 2^-11 v2,   s a power of two that puts the largest |v| into [2^13, 2^14),
// s = S_x for all training points (they enter as -2 x, which is exact), s = S_r for candidate r -- finer than one scale per
// tile: a far-out candidate would otherwise push its neighbours' coordinates towards fp16's subnormals, and a row of C/D
// is one register, so a scale per row costs the epilogue nothing.  The dot product is
//     hi = sum a1 b1,   mid = sum (a1 b2 + a2 b1)        (three v_mfma_f32_32x32x16_f16 per fragment and 16 k, two accumulators)
//     S (-2 c.x) = hi + 2^-11 mid   [the a2 b2 products, 2^-22 relative, are dropped],     S = S_r S_x
// and per pair the epilogue issues fma, fma, max, fma, v_exp_f32, fma:
//     t = fma(mid, 2^-11, hi);  s' = max(fma(|x|^2, S, t), -S |c|^2);  k_s = exp2(fma(s', kappa / S, L_r));  p = fma(k_s, |alpha|, p)
// with L_r = fl(log2 constant + kappa |c|^2): |c|^2 enters through the exponent's constant and the clamp, which costs no
// VALU issue and, unlike an accumulator that starts at S |c|^2, sends it through no matrix-core addition.  kappa / S is
// exact.  Both squared norms are f64 fma chains rounded to f32 once.
//
// Sign partition.  screen_h2_prep_kernel writes the screen's own copy of the training points with alpha >= 0 first, padded
// with alpha = 0 rows (zero planes) to a multiple of 128, then alpha < 0: every 128-point tile is sign-pure, there is no
// mixed tile and no slow path, at the price of at most one more tile.  p = sum k_s |alpha| then feeds one f64 sum for the
// positive tiles and one for the negative: mu_s = mu+ - mu-, W = mu+ + mu- = sum k_s |alpha|.
//
// Error term (derived in DESIGN §4, "the fp16 screen's error term"; u = 2^-24, R = |c|^2 + max |x_i|^2):
//     delta(c) = (2.01 D + 25 + 0.26 sqrt D) u R + 2^-40            bounds |s - d^2|
//     closed   = 1.001 |alpha|_1 (P_h R + Q_c),   P_h = 1.001 constant u delta-coefficient / 2
//     weighted = 1.001 (expm1(0.5001 delta) W + |alpha|_1 Q_w),     needs delta <= 1
//     E(c)     = min(closed, weighted)
// Range conditions, checked where the data are: the training points' largest coordinate finite and below 2^53, every
// |x_i|^2 finite (else no candidate is screened: E = inf); a candidate's |c|^2 + max |x_i|^2 below 2^46 (else that
// candidate's E = inf).  An infinite E makes prune_bound_kernel pass the candidate on to the tight bound pass.
// screen_h2_error_terms() is the ONE place the constants live; tests/prune_screen_h2_reference.py restates them.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "prune_screen.hpp"
#include "trmm_f16x2.hpp"

namespace tgp {

constexpr int SCRH_MIN_D = 15;       // from here on the fp16 screen's closed form is no looser than the f32 screen's: 2.01 D + 25 + 0.26 sqrt D <= 3 D + 12
constexpr int SCRH_ROW = 144;        // LDS bytes of a point: 32 k of plane 1, 32 k of plane 2, 16 bytes of pad (prune_screen.hpp's row)
constexpr int SCRH_MAXEXP = 40;      // |exponent| of a scale

struct ScreenH2Terms { double dcoef, P, Qc, Qw; };
inline ScreenH2Terms screen_h2_error_terms(double constant, int D, int N) {
    const double u = 0x1p-24, ce = 1.001 * constant, L = fabs(log2(constant));
    ScreenH2Terms t;
    t.dcoef = 2.01 * D + 25.0 + 0.26 * sqrt((double)D);
    t.P = ce * u * 0.5 * t.dcoef;
    t.Qc = screen_error_terms(constant, D, N).Q + ce * (0.7 * L * u + 0x1p-41);
    t.Qw = t.Qc + ce * u * (2.4 + 1.4 * L);
    return t;
}

// the weight's factor 1.001 expm1(0.5001 delta); +inf where delta > 1 (or is NaN): the closed form then stands alone
__host__ __device__ inline double screen_h2_weight(double dcoef, double R) {
    const double delta = dcoef * 0x1p-24 * R + 0x1p-40;
    return delta <= 1.0 ? 1.001 * expm1(0.5001 * delta) : INFINITY;
}
// E = min(closed, weighted); fmin drops a NaN weighted form (inf * 0)
__host__ __device__ inline double screen_h2_error(double closed, double wcoef, double W, double wadd) {
    return fmin(closed, wcoef * W + wadd);
}

// the power of two that puts m > 0 into [2^13, 2^14), its exponent kept within +-SCRH_MAXEXP; from the exponent bits
__host__ __device__ inline float screen_h2_scale(float m) {
    int e;
    frexpf(m, &e);
    int ex = 14 - e;
    ex = ex > SCRH_MAXEXP ? SCRH_MAXEXP : (ex < -SCRH_MAXEXP ? -SCRH_MAXEXP : ex);
    return ldexpf(1.f, ex);
}

struct ScreenH2Scal {
    double ea, eb, wadd;      // closed form = ea + eb |c|^2; the weighted form's constant 1.001 |alpha|_1 Q_w
    float nxmax, sx;          // max |x_i|^2, S_x
    int npos, nneg, ok, pad;  // points with alpha >= 0 / < 0; 0 = the training points fail the range conditions
};

struct ScreenH2PrepArgs {
    const float *Xs;          // (>= N, Dp) scaled training points
    const double *alpha;      // (N,)
    int N, Dp, nch;           // nch = 32-k chunks of a row
    long ncap;                // rows of the partitioned copy: (ceil(N / 128) + 1) 128
    double P, Qc, Qw;
    unsigned char *Xh;        // [chunk][row][plane][32 k] fp16: -2 x S_x
    float *nxp, *absa;        // (ncap,) |x|^2 and |alpha| in partition order, the padding rows zero
    ScreenH2Scal *scal;
};

// One launch per sweep, ceil(N / 256) workgroups.  Every workgroup first walks ALL points for the quantities every row
// needs -- max |x|, max |x|^2, the count of alpha >= 0 (in all and before its own rows), |alpha|_1 -- each in one fixed
// order, so all workgroups hold the same bits and no workgroup waits for another; then it writes its own 256 rows to
// their places.  No float atomics: E is the same bytes on every run.
__global__ __launch_bounds__(256) void screen_h2_prep_kernel(ScreenH2PrepArgs a) {
    __shared__ double sa[256];
    __shared__ float smx[256], smn[256];
    __shared__ int spos[256], sbef[256], sbad[256];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, base = blockIdx.x * 256;
    const int N = a.N, Dp = a.Dp;
    double a1 = 0.0;
    float mxx = 0.f, mxn = 0.f;
    int npos = 0, before = 0, bad = 0;
    // four of this thread's rows at a time: their f64 chains are independent (each in its own dimension order, as one row
    // alone would run it), so the loads and the fmas of four rows overlap; the per-thread sums then take the rows in order
    for (int i0 = tid; i0 < N; i0 += 4 * 256) {
        double s[4] = {0.0, 0.0, 0.0, 0.0}, al[4];
        float m[4] = {0.f, 0.f, 0.f, 0.f};
        const float *row[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + 256 * q;
            row[q] = a.Xs + (long)(i < N ? i : i0) * Dp;      // (a row past the end: the first one again, not used)
            al[q] = a.alpha[i < N ? i : i0];
        }
        for (int d = 0; d < Dp; d += 4) {
            f4_t x[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const f4_t *>(row[q] + d);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int q = 0; q < 4; ++q) { s[q] = fma((double)x[q][e], (double)x[q][e], s[q]); m[q] = fmaxf(m[q], fabsf(x[q][e])); }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + 256 * q;
            if (i < N) {
                if (!(s[q] < (double)INFINITY)) bad = 1;      // (an inf or a NaN coordinate)
                mxn = fmaxf(mxn, (float)s[q]);
                mxx = fmaxf(mxx, m[q]);
                a1 += fabs(al[q]);
                const int p = al[q] >= 0.0;
                npos += p;
                if (i < base) before += p;
            }
        }
    }
    sa[tid] = a1; smx[tid] = mxx; smn[tid] = mxn; spos[tid] = npos; sbef[tid] = before; sbad[tid] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            sa[tid] += sa[tid + o];
            smx[tid] = fmaxf(smx[tid], smx[tid + o]);
            smn[tid] = fmaxf(smn[tid], smn[tid + o]);
            spos[tid] += spos[tid + o];
            sbef[tid] += sbef[tid + o];
            sbad[tid] |= sbad[tid + o];
        }
        __syncthreads();
    }
    npos = spos[0];
    before = sbef[0];
    const int nneg = N - npos, np128 = (npos + 127) & ~127, nn128 = (nneg + 127) & ~127;
    const float xm2 = 2.f * smx[0];
    const float sx = xm2 > 0.f ? screen_h2_scale(xm2) : 1.f;
    const int ok = !sbad[0] && xm2 < 0x1p54f;
    if (blockIdx.x == 0 && tid == 0) {
        const double an = 1.001 * sa[0];
        ScreenH2Scal s;
        s.ea = an * (a.P * (double)smn[0] + a.Qc);
        s.eb = an * a.P;
        s.wadd = an * a.Qw;
        s.nxmax = smn[0]; s.sx = sx;
        s.npos = npos; s.nneg = nneg; s.ok = ok; s.pad = 0;
        *a.scal = s;
    }

    // this workgroup's rows: positives keep their order in [0, npos), negatives theirs from np128 on
    const int i = base + tid;
    const bool live = i < N;
    const double al = live ? a.alpha[i] : -1.0;
    const bool pos = live && al >= 0.0;
    const unsigned long long bal = __ballot(pos);
    const int lane = tid & 63, w = tid >> 6;
    if (lane == 0) wcnt[w] = __popcll(bal);
    __syncthreads();
    int pre = __popcll(bal & ((1ull << lane) - 1ull));
    for (int k = 0; k < w; ++k) pre += wcnt[k];
    auto write_row = [&](long dest, const float *row, float absal) {
        double s = 0.0;
        for (int ch = 0; ch < a.nch; ++ch) {
            unsigned h[2][16];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int d = ch * SCR_DC + 4 * q;
                f4_t x = {0.f, 0.f, 0.f, 0.f};
                if (row && d < Dp) x = *reinterpret_cast<const f4_t *>(row + d);
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fma((double)x[e], (double)x[e], s);
                split2_f16x2(-2.f * x[0], -2.f * x[1], sx, h[0][2 * q], h[1][2 * q]);
                split2_f16x2(-2.f * x[2], -2.f * x[3], sx, h[0][2 * q + 1], h[1][2 * q + 1]);
            }
            unsigned char *o = a.Xh + ((long)ch * a.ncap + dest) * 128;
#pragma unroll
            for (int pl = 0; pl < 2; ++pl)
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    *reinterpret_cast<u4_t *>(o + 64 * pl + 16 * q) = (u4_t){h[pl][4 * q], h[pl][4 * q + 1], h[pl][4 * q + 2], h[pl][4 * q + 3]};
        }
        a.nxp[dest] = (float)s;
        a.absa[dest] = absal;
    };
    if (live) write_row(pos ? before + pre : np128 + (i - before - pre), a.Xs + (long)i * Dp, (float)fabs(al));
    if (blockIdx.x == 0 && tid < 128) {      // the padding of the two blocks
        if (npos + tid < np128) write_row(npos + tid, nullptr, 0.f);
        if (nneg + tid < nn128) write_row(np128 + nneg + tid, nullptr, 0.f);
    }
}

struct ScreenH2Args {
    const float *Cs;          // (rows, Dp) scaled candidates, rows a multiple of 128, padding zero
    const unsigned char *Xh;  // screen_h2_prep_kernel's planes, nxp, absa, scal
    const float *nxp, *absa;
    const ScreenH2Scal *scal;
    double *mupart, *wpart;   // (gridDim.y, ldpart): split y's share of mu+ - mu- and of mu+ + mu-
    double *err, *wcoef;      // (rows,) the closed form and the weighted form's factor of W, written by split 0
    long ldpart, ncap;
    int Dp;
    double constant, dcoef;
};

// grid = (rows / 128, splits of the tiles); geometry and the C/D roles are prune_screen_kernel's: wave w owns candidates
// 32 w .. 32 w + 31 against the 128 points of a tile, a candidate in one register of 32 lanes, a point on the lane.
__global__ __launch_bounds__(256, 2) void prune_screen_h2_kernel(ScreenH2Args g) {
    __shared__ __attribute__((aligned(16))) unsigned char Ct[SCR_T * SCRH_ROW];
    __shared__ __attribute__((aligned(16))) unsigned char Xt[SCR_T * SCRH_ROW];
    __shared__ __attribute__((aligned(16))) f4_t rowc[SCR_T];      // per candidate: S, kappa / S, L_r, -S |c|^2
    __shared__ float srow[SCR_T];                                   // S_r
    __shared__ double mpos[SCR_T];                                  // mu+ while the negative tiles run
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const long c0 = (long)blockIdx.x * SCR_T;
    const int Dp = g.Dp;
    const ScreenH2Scal sc = *g.scal;
    const int ntp = (sc.npos + SCR_T - 1) / SCR_T;                  // positive tiles, then the negative ones
    const int njt = ntp + (sc.nneg + SCR_T - 1) / SCR_T;
    const int per = (njt + (int)gridDim.y - 1) / (int)gridDim.y;
    const int jt0 = blockIdx.y * per;
    const int jt1 = jt0 + per < njt ? jt0 + per : njt;
    const int nch = (Dp + SCR_DC - 1) / SCR_DC;
    const int nsteps = (jt1 > jt0 ? jt1 - jt0 : 0) * nch;
    const bool one_pass = nch == 1;
    constexpr float KAPPA = -0.72134752044448170368f;

    // |c|^2 (f64 chain, dimension order), the candidate's scale and its four epilogue constants
    if (tid < SCR_T) {
        const float *row = g.Cs + (c0 + tid) * Dp;
        double s = 0.0;
        float m = 0.f;
        for (int d = 0; d < Dp; d += 4) {
            const f4_t x = *reinterpret_cast<const f4_t *>(row + d);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s = fma((double)x[e], (double)x[e], s); m = fmaxf(m, fabsf(x[e])); }
        }
        const double R = s + (double)sc.nxmax;
        const bool ok = sc.ok && R < 0x1p46;                        // (false for a NaN)
        const float sr = ok ? (m > 0.f ? screen_h2_scale(m) : 1.f) : 0.f;
        const float S = sr * sc.sx;
        srow[tid] = sr;
        rowc[tid] = (f4_t){S, KAPPA / S, (float)((double)log2f((float)g.constant) + (double)KAPPA * s), -(float)((double)S * s)};
        if (blockIdx.y == 0) {
            g.err[c0 + tid] = ok ? sc.ea + sc.eb * s : (double)INFINITY;
            g.wcoef[c0 + tid] = ok ? screen_h2_weight(g.dcoef, R) : (double)INFINITY;
        }
    }
    __syncthreads();
    ScrStage sp;
    u4_t xq[4];
    auto store_c = [&]() {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = tid + 256 * p;
            const int r = idx >> 3, dv = (idx & 7) * 4;
            const float sr = srow[r];
            unsigned a0, a1, b0, b1;
            split2_f16x2(sp.v[p][0], sp.v[p][1], sr, a0, b0);
            split2_f16x2(sp.v[p][2], sp.v[p][3], sr, a1, b1);
            *reinterpret_cast<uint2 *>(Ct + r * SCRH_ROW + 2 * dv) = make_uint2(a0, a1);
            *reinterpret_cast<uint2 *>(Ct + r * SCRH_ROW + 64 + 2 * dv) = make_uint2(b0, b1);
        }
    };
    auto load_x = [&](int jt, int ch) {
        const unsigned char *src = g.Xh + ((long)ch * g.ncap + (long)jt * SCR_T) * 128;
#pragma unroll
        for (int p = 0; p < 4; ++p) xq[p] = *reinterpret_cast<const u4_t *>(src + (tid + 256 * p) * 16);
    };
    auto store_x = [&]() {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int idx = tid + 256 * p;
            *reinterpret_cast<u4_t *>(Xt + (idx >> 3) * SCRH_ROW + (idx & 7) * 16) = xq[p];
        }
    };
    if (nsteps > 0) {
        sp.load(g.Cs, c0, Dp, 0);
        load_x(jt0, 0);
        store_c();
        store_x();
    }
    __syncthreads();
    double sum[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) sum[r] = 0.0;
    auto mma = [](u4_t a, u4_t b, f16_t c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    };
    f16_t hi[4], mid[4];
    auto kstep = [&](int kb, auto first_tag) {
        constexpr bool FIRST = decltype(first_tag)::value;
        const int off = 32 * kb + 16 * lh;
        const unsigned char *ap = Ct + (32 * w + li) * SCRH_ROW + off;
        const u4_t a1 = *reinterpret_cast<const u4_t *>(ap), a2 = *reinterpret_cast<const u4_t *>(ap + 64);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const unsigned char *bp = Xt + (32 * b + li) * SCRH_ROW + off;
            const u4_t b1 = *reinterpret_cast<const u4_t *>(bp), b2 = *reinterpret_cast<const u4_t *>(bp + 64);
            if constexpr (FIRST) {
                const f16_t zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                hi[b] = mma(a1, b1, zero);
                mid[b] = mma(a1, b2, zero);
            } else {
                hi[b] = mma(a1, b1, hi[b]);
                mid[b] = mma(a1, b2, mid[b]);
            }
            mid[b] = mma(a2, b1, mid[b]);
        }
    };
    for (int st = 0; st < nsteps; ++st) {
        const int jt = jt0 + st / nch, ch = st - (st / nch) * nch;
        const int j0 = jt * SCR_T;
        const bool more = st + 1 < nsteps;
        if (more) {
            const int jn = jt0 + (st + 1) / nch, cn = (st + 1) - ((st + 1) / nch) * nch;
            load_x(jn, cn);
        }
        float nxv[4], al[4];
        if (ch == nch - 1) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                nxv[b] = g.nxp[j0 + 32 * b + li];
                al[b] = g.absa[j0 + 32 * b + li];
            }
        }
        if (ch == 0 && jt == ntp && jt > jt0) {
            // the sign boundary: the f64 sums so far are mu+; close them once and start mu-
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                double s = sum[r];
#pragma unroll
                for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
                if (li == 0) mpos[32 * w + Mfma<float>::c_row(lane, r)] = s;
                sum[r] = 0.0;
            }
        }
        int dn = Dp - ch * SCR_DC;
        if (dn > SCR_DC) dn = SCR_DC;
        const int nkb = (dn + 15) >> 4;               // 1 or 2 (the staged block is zero beyond Dp)
        // k-values 16 kb .. 16 kb + 15: lane half h takes 16 kb + 8 h + j for element j, both operands alike.  The first
        // step of a tile's first chunk hands the MFMAs a zero constant for C (the instruction's inline 0, the same
        // product as on a zeroed accumulator): no accumulator is zeroed in front of a tile.
        if (ch == 0) kstep(0, std::true_type{});
        else kstep(0, std::false_type{});
        if (nkb == 2) kstep(1, std::false_type{});
        if (ch == nch - 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const f4_t rc = rowc[32 * w + Mfma<float>::c_row(lane, r)];
                float p = 0.f;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const float t = fmaf(mid[b][r], 0x1p-11f, hi[b][r]);
                    const float s = fmaxf(fmaf(nxv[b], rc[0], t), rc[3]);
                    const float kv = __builtin_amdgcn_exp2f(fmaf(s, rc[1], rc[2]));
                    p = b == 0 ? kv * al[0] : fmaf(kv, al[b], p);
                }
                sum[r] += (double)p;
            }
        }
        if (more) {
            __syncthreads();
            if (!one_pass) {      // (D > 32: the candidate chunk is fetched here, not ahead of the MFMAs -- 16 registers the loop has no room for)
                sp.load(g.Cs, c0, Dp, ((st + 1) - ((st + 1) / nch) * nch) * SCR_DC);
                store_c();
            }
            store_x();
            __syncthreads();
        }
    }
    const bool has_pos = nsteps > 0 && jt0 < ntp, has_neg = nsteps > 0 && jt1 > ntp;
    // (the lane index read again, not kept in a register across the tile loop: the loop has none to spare)
    const int elane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        double s = sum[r];
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if ((elane & 31) == 0) {
            const int row = 32 * w + Mfma<float>::c_row(elane, r);
            const double mp = has_neg ? (has_pos ? mpos[row] : 0.0) : s, mn = has_neg ? s : 0.0;
            const long o = (long)blockIdx.y * g.ldpart + c0 + row;
            g.mupart[o] = mp - mn;
            g.wpart[o] = mp + mn;
        }
    }
}

}  // namespace tgp
