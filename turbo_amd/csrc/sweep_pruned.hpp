// sweep_pruned.hpp -- the pruned arg-max sweep: its kernels, its workspace, and the schedule as a driver over
// named steps.
//
// NOT a header of its own: sweep_kernels.hip includes it once, after SweepPlan, make_plan and the launch helpers both
// schedules share (launch_kstar, launch_trmm, fin_args, launch_argmax, ProfCursor, grid_splits, pad128), so that the pruned
// sweep stays in that translation unit -- the same compile flags, the same kernel symbols, the same code object.
#pragma once

namespace tgp {

// ---- the pruned sweep: contract only the candidates that can still win ----------------------------------
// An arg-max-only sweep (no mean, deviation or acquisition vector asked for) needs a candidate's variance only if its
// acquisition could still be the largest.  c + s^2 - q lies in [s^2, c + s^2] (q = k^T K^-1 k in [0, c]), and for a fixed
// mean EI and UCB (param >= 0) increase with sigma, PI increases or decreases with it by the sign of its argument -- so
// the mean alone bounds each candidate's acquisition from above, at the larger of its values at the interval's ends:
//   1. bound pass: kstar (XP = 4) over all M without a slab -> Ks.alpha and |Ks|.|alpha| -> prune_bound_kernel: the mean
//      moved by its rounding-error bound the way that raises the acquisition, then a relative margin on top;
//   2. lb set: the largest bound of each of prune_top groups of consecutive candidates, contracted exactly (kstar, the
//      128 x 128 contraction, finalize on the gathered rows); its best value is the bar lb;
//   3. survivors: every other candidate whose bound reaches lb (less the margin), compacted in index order and contracted
//      the same way; ONE arg-max over both sets with the batch indices, so the lowest index still wins a tie.
// A contracted candidate goes through the full sweep's arithmetic (same Ks bits, MeanAcc's one summation order, the same
// units in finalize whichever tiling ran): the winner's value and index are the full sweep's, bit for bit.  The clamp gate
// s^2 / (c + s^2) >= prune_tau * u (u: the contraction's unit roundoff; measured |q - q_f64| / c stays below 122 u,
// DESIGN §4) keeps every computed variance above 0.99 s^2: no skipped candidate could have clamped, and 0.99 s^2 is a valid
// lower end of the interval.  More than prune_frac of the batch surviving: the full schedule runs instead.
struct BoundArgs {
    const double *mupart, *abspart; long ldpart; int njs;   // the bound pass's partial sums, njs rows each
    long m;
    double err_scale;          // |the contraction's K*.alpha - this sum| <= err_scale * sum |k| |alpha| (two orders of the same products)
    const double *err;         // null (the tight pass: the line above), or (m,) the error of each mean as formed elsewhere (the
                               // screen's E(c), prune_screen.hpp); abspart is then not read ...
    const double *wcoef;       // ... unless this is given too (the fp16 screen, prune_screen_h2.hpp): abspart then holds the shares of
    const double *wadd;        // W = sum k_s |alpha|, and the error is the smaller of err and wcoef[c] * W + wadd[0]
    double y_mean, y_std;
    double sig_lo, sig_hi;     // every candidate's computed sigma lies in [sig_lo, sig_hi]
    int acq; double sf, incumbent, param, margin;
    double *ub;                // (m,) the bound; NaN -> +inf (always contracted)
};

__global__ __launch_bounds__(256) void prune_bound_kernel(BoundArgs b) {
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    if (c >= b.m) return;
    double mun = 0.0, s = 0.0;
    for (int j = 0; j < b.njs; ++j) {
        mun += b.mupart[(long)j * b.ldpart + c];
        if (!b.err || b.wcoef) s += b.abspart[(long)j * b.ldpart + c];
    }
    double e = b.err ? b.err[c] : b.err_scale * s;
    if (b.wcoef) e = screen_h2_error(e, b.wcoef[c], s, b.wadd[0]);
    const double mu = b.y_std * (b.sf > 0.0 ? mun + e : mun - e) + b.y_mean;
    // (EI / PI / UCB only reach the pruned sweep, so acq_value's other cases are never taken here)
    const double a_lo = acq_value(b.acq, b.sf, b.incumbent, b.param, mu, b.sig_lo);
    const double a_hi = acq_value(b.acq, b.sf, b.incumbent, b.param, mu, b.sig_hi);
    double a = a_lo > a_hi ? a_lo : a_hi;
    // margin against the rounding of the formulas themselves (UCB: relative to its terms, which may cancel)
    double scale = fabs(a);
    if (b.acq == TGP_ACQ_UCB) scale += fabs(mu) + fabs(b.param) * b.sig_hi;
    a += b.margin * scale;
    b.ub[c] = (isnan(a_lo) || isnan(a_hi) || isnan(a)) ? INFINITY : a;
}

// the lb set: per group of gs consecutive candidates the one with the largest bound (lowest index on ties)
__global__ __launch_bounds__(256) void prune_pick_kernel(const double *__restrict__ ub, long m, long gs,
                                                         long long *__restrict__ pick) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const long g0 = (long)blockIdx.x * gs;
    const long g1 = g0 + gs < m ? g0 + gs : m;
    Best b;   // (not strided_argmax: the values carry no index array, and a thread's own indices only ascend)
    for (long c = g0 + threadIdx.x; c < g1; c += 256) {
        const double u = ub[c];
        if (u > b.v) { b.v = u; b.i = c; }
    }
    b = block_argmax<256>(b, sv, si);
    if (threadIdx.x == 0) pick[blockIdx.x] = b.i == IDX_NONE ? g0 : b.i;   // (all bounds -inf: the group's first)
}

// The speculative round's lb set (sweep_pruned below): prune_pick_kernel's pick AND the next three bounds of each group, in
// `better`'s order (larger bound first, lower index on ties), into runner[3 g ..]; IDX_NONE where the group has no more
// members.  A thread keeps the best four of its own candidates, then four block arg-max rounds take them off the threads'
// heads.  pick[g] is prune_pick_kernel's: the largest bound at its lowest index, the group's first when every bound is -inf.
__global__ __launch_bounds__(256) void prune_pick4_kernel(const double *__restrict__ ub, long m, long gs, long long *__restrict__ pick,
                                                          long long *__restrict__ runner) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const long g0 = (long)blockIdx.x * gs;
    const long g1 = g0 + gs < m ? g0 + gs : m;
    double v[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    long long ix[4] = {IDX_NONE, IDX_NONE, IDX_NONE, IDX_NONE};
    for (long c = g0 + threadIdx.x; c < g1; c += 256) {
        const double u = ub[c];
        if (better(u, c, v[3], ix[3])) {
            v[3] = u; ix[3] = c;
#pragma unroll
            for (int k = 3; k > 0; --k)
                if (better(v[k], ix[k], v[k - 1], ix[k - 1])) {
                    const double tv = v[k]; v[k] = v[k - 1]; v[k - 1] = tv;
                    const long long ti = ix[k]; ix[k] = ix[k - 1]; ix[k - 1] = ti;
                }
        }
    }
#pragma unroll
    for (int round = 0; round < 4; ++round) {
        Best b;
        b.v = v[0]; b.i = ix[0];
        b = block_argmax<256>(b, sv, si);
        __syncthreads();   // (every thread has read the result before the next round stages its head)
        if (b.i != IDX_NONE && b.i == ix[0]) {
            v[0] = v[1]; v[1] = v[2]; v[2] = v[3]; v[3] = -INFINITY;
            ix[0] = ix[1]; ix[1] = ix[2]; ix[2] = ix[3]; ix[3] = IDX_NONE;
        }
        if (threadIdx.x == 0) {
            if (round == 0) pick[blockIdx.x] = b.i == IDX_NONE ? g0 : b.i;
            else runner[3 * (long)blockIdx.x + round - 1] = b.i;
        }
    }
}

// The extras of the speculative round: of the R runner-ups (IDX_NONE: none) the first `cap` in `better`'s order of their
// bounds, written in that order (larger bound first, lower index on ties: the runner-ups are distinct candidates, so the
// order is total and the gathered rows, and every byte behind them, are the same on every run).  One wave per runner-up:
// every workgroup stages all R (bound, index) pairs in LDS (R <= SPEC_MAXR), a wave counts the pairs in front of its own
// with ballots, and a runner-up whose rank is below `cap` is written to extras[rank] and marked in sel.  An infinite bound
// ranks first; an IDX_NONE place is in front of nothing.  words[1] = 0: the survivors' scatter counts there the survivors
// that are not among the extras; words[2] = nx, the number of extras (the smaller of cap and the real runner-ups).
constexpr int SPEC_MAXR = 3072;
__global__ __launch_bounds__(256) void prune_extras_kernel(const double *__restrict__ ub, const long long *__restrict__ runner, int R,
                                                           int cap, long long nx, long long *__restrict__ extras,
                                                           int *__restrict__ sel, long long *__restrict__ words) {
    __shared__ double sv[SPEC_MAXR];
    __shared__ long long si[SPEC_MAXR];
    for (int k = threadIdx.x; k < R; k += 256) {
        const long long i = runner[k];
        si[k] = i;
        sv[k] = i == IDX_NONE ? -INFINITY : ub[i];
    }
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) { words[1] = 0; words[2] = nx; }
    const int lane = threadIdx.x & 63;
    const int k = (int)blockIdx.x * 4 + (threadIdx.x >> 6);   // (one value per wave)
    if (k >= R) return;
    const double vk = sv[k];
    const long long ik = si[k];
    int rank = 0;
    for (int j0 = 0; j0 < R; j0 += 64) {
        const int j = j0 + lane;
        rank += __popcll(__ballot(j < R && better(sv[j], si[j], vk, ik)));
    }
    if (lane == 0) {
        const int take = ik != IDX_NONE && rank < cap;
        sel[k] = take;
        if (take) extras[rank] = ik;
    }
}

// rows idx[0..n), then idx1[0..n1), of the scaled candidates into a dense block of `rows` rows (rows >= n + n1 zero)
template <typename T>
__global__ __launch_bounds__(256) void prune_gather_kernel(const T *__restrict__ Cs, int Dp, const long long *__restrict__ idx,
                                                           long n, const long long *__restrict__ idx1, long n1, long rows,
                                                           T *__restrict__ out) {
    const long total = rows * Dp;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long r = i / Dp;
        const int d = (int)(i - r * Dp);
        out[i] = r < n ? Cs[idx[r] * Dp + d] : (r < n + n1 ? Cs[idx1[r - n] * Dp + d] : (T)0);
    }
}

struct SurvArgs {
    const double *ub; long m;
    const long long *pick; long gs;   // the lb set (already contracted: not a survivor)
    const double *lb; double margin;  // lb: the lb set's best exact value (device)
    int *bcnt; const int *boff;       // survivors per 256-candidate block / exclusive offsets
    long long *sidx;                  // survivors' batch indices, in order
    const long long *src;             // null, or ub is over a gathered set (already clear of the lb set): src[c] is row c's batch index
    const long long *runner;          // null, or the speculative round's runner-ups (three places per group of the lb set), ...
    const int *sel;                   // ... which of them are its extras, ...
    int *leftover;                    // ... and where the scatter counts the survivors that are not among the extras
};

__device__ __forceinline__ bool prune_survives(const SurvArgs &s, long c) {
    const double lb = s.lb[0];
    const double bar = isinf(lb) ? lb : lb - s.margin * fabs(lb);
    return c < s.m && s.ub[c] >= bar && (s.src || s.pick[c / s.gs] != c);
}

__global__ __launch_bounds__(256) void prune_count_kernel(SurvArgs s) {
    __shared__ int wsum[4];
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long bal = __ballot(prune_survives(s, c));
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = __popcll(bal);
    __syncthreads();
    if (threadIdx.x == 0) s.bcnt[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

__global__ __launch_bounds__(1024) void prune_scan_kernel(const int *__restrict__ bcnt, int nb, int *__restrict__ boff,
                                                          long long *__restrict__ total) {
    __shared__ int part[1024];
    const int per = (nb + 1023) / 1024;
    const int b0 = (int)threadIdx.x * per;
    const int b1 = b0 + per < nb ? b0 + per : nb;
    int s = 0;
    for (int b = b0; b < b1; ++b) s += bcnt[b];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const int v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int b = b0; b < b1; ++b) { boff[b] = run; run += bcnt[b]; }
    if (threadIdx.x == 1023) total[0] = part[1023];
}

__global__ __launch_bounds__(256) void prune_scatter_kernel(SurvArgs s) {
    __shared__ int wsum[4];
    const long c = (long)blockIdx.x * 256 + threadIdx.x;
    const bool keep = prune_survives(s, c);
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int off = s.boff[blockIdx.x];
    for (int k = 0; k < w; ++k) off += wsum[k];
    if (keep) {
        const long long gc = s.src ? s.src[c] : c;
        s.sidx[off + __popcll(bal & ((1ull << lane) - 1ull))] = gc;
        if (s.runner) {   // an extra is one of its own group's runner-ups (an integer count: the same on every run)
            const long g3 = 3 * (long)(gc / s.gs);
            bool found = false;
            for (int k = 0; k < 3; ++k) found = found || (s.runner[g3 + k] == gc && s.sel[g3 + k] != 0);
            if (!found) atomicAdd(s.leftover, 1);
        }
    }
}

// the pruned sweep's own workspace (grow-only): bounds, lb set, survivors, block counts, the gathered scaled rows; for the
// screen: E(c), the gathered set's tight bounds, the second survivor list, |x_i|^2 (misc + 8: its scalars); for the fp16
// screen also the weighted form's factors and the sign-partitioned copy of the training points (planes, |x|^2, |alpha|)
struct PruneWs {
    double *ub; long long *pick, *sidx, *misc; int *bcnt, *boff; void *cs;
    double *err, *ub1; long long *sidx1; float *nx;
    double *wcoef; unsigned char *xh; float *nxp, *absa; long ncap;
    long long *runner, *extras; int *sel;   // the speculative round: three runner-ups per group, the extras taken from them, which they are
};
static size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// sub-buffers of one allocation in the order they are taken, each on a 256-byte boundary; one that is not wanted takes no
// room (its pointer is the next one's).  Without a base only the bytes are counted.
struct Carver {
    char *base = nullptr;
    size_t off = 0;
    template <typename U>
    U *take(size_t count, bool wanted = true) {
        U *ptr = base ? reinterpret_cast<U *>(base + off) : nullptr;
        if (wanted) off += al256(count * sizeof(U));
        return ptr;
    }
};

template <typename T>
static void prune_carve(const Context &c, int64_t npick, int64_t rows_cap, bool screen, bool h2, bool spec, Carver &k, PruneWs &w) {
    const size_t M = (size_t)c.M, nb = (size_t)((c.M + 255) / 256), Mpad = (size_t)c.ws_Mpad;
    w.ncap = (long)((c.N + SCR_T - 1) / SCR_T + 1) * SCR_T;
    const size_t ncap = (size_t)w.ncap, nch = (size_t)((c.Dp + SCR_DC - 1) / SCR_DC);
    w.ub = k.take<double>(M);
    w.pick = k.take<long long>((size_t)npick);
    w.sidx = k.take<long long>(M);
    w.misc = k.take<long long>(32);   // 256 bytes: [0] a survivor count; from word 8 on the screen's scalars
    w.bcnt = k.take<int>(nb);
    w.boff = k.take<int>(nb);
    w.cs = k.take<T>((size_t)rows_cap * c.Dp);
    w.err = k.take<double>(Mpad, screen);
    w.ub1 = k.take<double>((size_t)rows_cap, screen);
    w.sidx1 = k.take<long long>(M, screen);
    w.nx = k.take<float>((size_t)c.Np, screen);
    w.wcoef = k.take<double>(Mpad, h2);
    w.xh = k.take<unsigned char>(nch * ncap * 128, h2);
    w.nxp = k.take<float>(ncap, h2);
    w.absa = k.take<float>(ncap, h2);
    w.runner = k.take<long long>(3 * (size_t)npick, spec);
    w.extras = k.take<long long>(3 * (size_t)npick, spec);
    w.sel = k.take<int>(3 * (size_t)npick, spec);
}

template <typename T>
static hipError_t prune_workspace(Context &c, int64_t npick, int64_t rows_cap, bool screen, bool h2, bool spec, PruneWs &w) {
    Carver count;
    prune_carve<T>(c, npick, rows_cap, screen, h2, spec, count, w);
    TGP_TRY(c.d_prune.reserve(count.off, [&] { return hipStreamSynchronize(c.stream); }));
    Carver k{c.d_prune};
    prune_carve<T>(c, npick, rows_cap, screen, h2, spec, k, w);
    return hipSuccess;
}

// The contraction of `rows` gathered candidates (a multiple of 128) over ntm 128-row tiles: the widest candidate tile of
// 128 / 64 / 32 that still gives CONTRACT_MIN_WGS workgroups, else the narrowest.  A launch with fewer workgroups than
// CUs lasts as long as its heaviest wave, and the narrow variants (trmm_sweep.hpp) cut that wave's share of a row tile
// from 128 x 32 to 32 x 64 / 32 x 32; they write the 128 x 128 kernel's bits, so the choice never shows in a result.
template <typename T>
static TrmmVariant contract_variant(const SweepPlan<T> &p, int64_t rows, int ntm) {
    TrmmVariant v;
    v.kern = p.early.kern; v.lds = trmm_glds_lds_bytes(); v.tile_m = 128; v.tile_n = 128; v.threads = 256;
    if ((rows / 128) * ntm >= CONTRACT_MIN_WGS) return v;
    if ((rows / 64) * ntm >= CONTRACT_MIN_WGS) {
        v.kern = trmm_sumsq_glds_narrow_kernel<T, 64>; v.lds = trmm_narrow_lds_bytes<64>(); v.tile_n = 64;
    } else {
        v.kern = trmm_sumsq_glds_narrow_kernel<T, 32>; v.lds = trmm_narrow_lds_bytes<32>(); v.tile_n = 32;
    }
    return v;
}

// n gathered rows: per launch_rows of them the cross-kernel into slot 0, then the 128-row contraction over every row
// tile with the mean inside (part / mupart rows [0, n))
template <typename T>
static hipError_t contract_rows(Context &c, const SweepPlan<T> &p, const T *cs, int64_t n, ProfCursor &cur) {
    for (int64_t off = 0; off < n; off += c.launch_rows) {
        const int64_t m = n - off < c.launch_rows ? n - off : c.launch_rows;
        const int64_t rows = pad128(m);
        // (SlabNoMean writes no row of mupart, so KS_JS does not bind its splits: every Ks entry is formed the same way
        // whatever the split count, and a small gathered set has one or two candidate tiles to fill the chip with.  A
        // set with candidate tiles enough keeps the plan's splits.)
        const int ntile = (int)c.Np / 128;
        const int njs_s = grid_splits(rows / (16 * kstar_ar(sizeof(T))), GATHER_KS_MIN_WGS, ntile, ntile);
        const int njs_g = njs_s > p.njs ? njs_s : p.njs;
        TGP_TRY(launch_kstar<T>(c, Kstar::SlabNoMean, cs + off * c.Dp, rows, njs_g, c.d_Ks[0].get(), c.d_mupart + off,
                                (long)c.Np / 16, 1.f, cur.st));
        cur.seg(1);
        TGP_TRY(launch_trmm<T>(c, p, contract_variant<T>(p, rows, p.n128), 0, off, rows, 0, p.n128, 0, true, cur.st));
        cur.seg(0, (double)m * (double)c.N * (double)c.N);
    }
    return hipSuccess;
}

// May this sweep take the pruned schedule?  NotEligible: not an arg-max-only EI / PI / UCB sweep in f32 / f64 with the mean
// inside the contraction, switched off, or too small to pay (prune_state stays -1).  GatedOff: the noise is too small for
// the clamp gate above (-2).
enum class PruneGo { NotEligible, GatedOff, Go };
template <typename T>
static PruneGo prune_eligible(const Context &c, const SweepPlan<T> &p, const SweepCall &call) {
    const int acq = call.acq;
    if (call.mu || call.sigma || call.acqv) return PruneGo::NotEligible;
    if (acq != TGP_ACQ_EI && acq != TGP_ACQ_PI && acq != TGP_ACQ_UCB) return PruneGo::NotEligible;
    if (c.dtype != TGP_F32 && c.dtype != TGP_F64) return PruneGo::NotEligible;
    if (!p.mean_in_trmm || tuning_sweep_prune_now() == 0) return PruneGo::NotEligible;
    if (!(c.M > tuning().prune_top)) return PruneGo::NotEligible;
    if (!((double)c.M * (double)c.N * (double)c.N >= tuning_prune_min_work_now())) return PruneGo::NotEligible;
    const double u = sizeof(T) == 4 ? 0x1p-24 : 0x1p-53;
    const bool gate = c.noise > 0.0 && c.noise / (c.constant + c.noise) >= tuning().prune_tau * u;
    return gate ? PruneGo::Go : PruneGo::GatedOff;
}

// what the steps of one pruned sweep share
template <typename T>
struct PruneRun {
    Context &c;
    const SweepPlan<T> &p;
    const SweepCall &call;
    PruneWs w;
    BoundArgs b;               // a bound pass's arguments; each pass sets its rows (njs, m, err, wcoef, ub)
    const T *Cs, *Xs;          // every scaled candidate; the scaled training points
    T *cs;                     // the gathered rows (w.cs)
    int64_t gs, npick, keep;   // candidates per group of the lb set; its size; the most survivors taken (-1: none)
    bool screen, h2;           // the screen runs; on the fp16 matrix pipe
    ProfCursor cur;
    int64_t nx = 0;            // the speculative round's extras (0: this sweep does not speculate)
};

// The tight bound of `rows` scaled candidates (a multiple of 16 KAR; m of them real) into ub.
// Splits of the training points over the bound pass's grid: a big batch fills the chip with its candidate tiles
// alone, and every split costs a workgroup its prologue (candidate tile staged, first barrier), 2 x 8 shuffled
// partial sums and a row of each partial array for prune_bound_kernel to read.  (Any split is covered by
// err_scale: it bounds the distance between two summation orders of the same products.)
template <typename T>
static hipError_t tight_bound(PruneRun<T> &r, const T *rowsrc, int64_t rows, int64_t m, double *ub) {
    Context &c = r.c;
    const int njs_b = grid_splits(rows / (16 * kstar_ar(sizeof(T))), BOUND_MIN_WGS, r.p.njs, r.p.njs);
    TGP_TRY(launch_kstar<T>(c, Kstar::Bound, rowsrc, rows, njs_b, c.d_part.get(), c.d_mupart, 0L, 1.f, c.stream));
    r.cur.seg(1);
    r.b.njs = njs_b; r.b.m = m; r.b.err = nullptr; r.b.wcoef = nullptr; r.b.ub = ub;
    hipLaunchKernelGGL(prune_bound_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c.stream, r.b);
    return hipGetLastError();
}

// The screen on the fp16 matrix pipe (prune_screen_h2.hpp) over all M on a grid of (xb, njs_s): one prep launch (sign
// partition, fp16 planes, the scalars of E), the screen; prune_bound_kernel then sums the splits' weights (in d_part, which
// the screened bound does not otherwise read) and takes the smaller form
static hipError_t screen_h2_bound(PruneRun<float> &r, int64_t xb, int njs_s) {
    Context &c = r.c;
    const PruneWs &w = r.w;
    const int N = (int)c.N, Dp = (int)c.Dp;
    const ScreenH2Terms et = screen_h2_error_terms(c.constant, (int)c.D, N);
    ScreenH2Scal *scal = reinterpret_cast<ScreenH2Scal *>(w.misc + 8);
    static_assert(sizeof(ScreenH2Scal) <= 256 - 64, "the scalars live behind misc's first eight words");
    ScreenH2PrepArgs a{};
    a.Xs = r.Xs; a.alpha = c.d_alpha; a.N = N; a.Dp = Dp; a.nch = (Dp + SCR_DC - 1) / SCR_DC; a.ncap = w.ncap;
    a.P = et.P; a.Qc = et.Qc; a.Qw = et.Qw;
    a.Xh = w.xh; a.nxp = w.nxp; a.absa = w.absa; a.scal = scal;
    hipLaunchKernelGGL(screen_h2_prep_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c.stream, a);
    TGP_TRY(hipGetLastError());
    r.cur.restart();
    ScreenH2Args g{};
    g.Cs = r.Cs; g.Xh = w.xh; g.nxp = w.nxp; g.absa = w.absa; g.scal = scal;
    g.mupart = c.d_mupart; g.wpart = c.d_part; g.err = w.err; g.wcoef = w.wcoef; g.ldpart = c.ws_Mpad; g.ncap = w.ncap;
    g.Dp = Dp; g.constant = c.constant; g.dcoef = et.dcoef;
    hipLaunchKernelGGL(prune_screen_h2_kernel, dim3((unsigned)xb, (unsigned)njs_s), dim3(256), 0, c.stream, g);
    TGP_TRY(hipGetLastError());
    r.cur.seg(2);
    c.prune_arith = 2;
    r.b.wcoef = w.wcoef; r.b.wadd = &scal->wadd;
    return hipSuccess;
}

// The screen in f32 (prune_screen.hpp) on the same grid: |x_i|^2 and the scalars of E, then the screen
static hipError_t screen_f32_bound(PruneRun<float> &r, int64_t xb, int njs_s) {
    Context &c = r.c;
    const PruneWs &w = r.w;
    const int N = (int)c.N, Dp = (int)c.Dp;
    const ScreenTerms et = screen_error_terms(c.constant, (int)c.D, N);
    double *scal = reinterpret_cast<double *>(w.misc + 8);
    hipLaunchKernelGGL(screen_stats_kernel, dim3(1), dim3(1024), 0, c.stream, r.Xs, c.d_alpha, N, (int)c.Np, Dp, et.P, et.Q, w.nx, scal);
    TGP_TRY(hipGetLastError());
    r.cur.restart();
    ScreenArgs g{};
    g.Cs = r.Cs; g.Xs = r.Xs; g.alpha = c.d_alpha; g.nx = w.nx; g.scal = scal;
    g.mupart = c.d_mupart; g.err = w.err; g.ldpart = c.ws_Mpad;
    g.N = N; g.Np = (int)c.Np; g.Dp = Dp; g.constant = c.constant;
    hipLaunchKernelGGL(prune_screen_kernel, dim3((unsigned)xb, (unsigned)njs_s), dim3(256), 0, c.stream, g);
    TGP_TRY(hipGetLastError());
    r.cur.seg(2);
    c.prune_arith = 1;
    r.b.wcoef = nullptr;
    return hipSuccess;
}

// 1. the bound of every candidate into w.ub: the screen's where it applies (its error the input of prune_bound_kernel), else
// the tight one
template <typename T>
static hipError_t bound_all(PruneRun<T> &r) {
    Context &c = r.c;
    if (!r.screen) return tight_bound<T>(r, r.Cs, c.ws_Mpad, c.M, r.w.ub);
    if constexpr (sizeof(T) == 4) {
        const int64_t xb = c.ws_Mpad / SCR_T;
        const int njt = ((int)c.N + SCR_T - 1) / SCR_T;
        const int njs_s = grid_splits(xb, SCREEN_MIN_WGS, r.p.njs, njt < r.p.njs ? njt : r.p.njs);
        TGP_TRY(r.h2 ? screen_h2_bound(r, xb, njs_s) : screen_f32_bound(r, xb, njs_s));
        r.b.njs = njs_s; r.b.m = c.M; r.b.err = r.w.err; r.b.ub = r.w.ub;
        hipLaunchKernelGGL(prune_bound_kernel, dim3((unsigned)((c.M + 255) / 256)), dim3(256), 0, c.stream, r.b);
        return hipGetLastError();
    }
    return hipSuccess;
}

// rows idx[0, n), then idx1[0, n1), of the scaled candidates into the dense block cs (zero rows up to a multiple of 128)
template <typename T>
static hipError_t gather_rows(PruneRun<T> &r, const long long *idx, int64_t n, const long long *idx1 = nullptr, int64_t n1 = 0) {
    const int Dp = (int)r.c.Dp;
    const long total = (long)pad128(n + n1) * Dp;
    const long blocks = (total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192;
    hipLaunchKernelGGL(prune_gather_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, r.c.stream, r.Cs, Dp, idx, (long)n, idx1,
                       (long)n1, (long)pad128(n + n1), r.cs);
    return hipGetLastError();
}

// value and block arg-max of the n contracted rows idx[0, n): their partial sums from column col0 of part / mupart on (the
// rows' place in the gathered block), their block partials from block blk0 on
template <typename T>
static hipError_t finalize_rows(PruneRun<T> &r, const long long *idx, int64_t n, int64_t blk0, int64_t col0 = 0) {
    FinArgs f = fin_args<T>(r.c, r.p, r.call);
    f.part += col0; f.mupart += col0;
    f.base_pairs = r.p.nunits;   // 128-row tiles throughout
    f.njs = 1;
    f.off = blk0 * FIN_BLOCK; f.m = n;
    f.gidx = idx;
    hipLaunchKernelGGL(finalize_kernel, dim3((unsigned)((n + FIN_BLOCK - 1) / FIN_BLOCK)), dim3(FIN_BLOCK), 0, r.c.stream, f);
    return hipGetLastError();
}

// 2. the lb set, picked from w.ub and contracted exactly; its best value is the bar (d_best); nblk: its blocks of partials
template <typename T>
static hipError_t lb_set(PruneRun<T> &r, int64_t &nblk) {
    Context &c = r.c;
    hipLaunchKernelGGL(prune_pick_kernel, dim3((unsigned)r.npick), dim3(256), 0, c.stream, r.w.ub, (long)c.M, (long)r.gs, r.w.pick);
    TGP_TRY(hipGetLastError());
    TGP_TRY(gather_rows(r, r.w.pick, r.npick));
    TGP_TRY(contract_rows<T>(c, r.p, r.cs, r.npick, r.cur));
    TGP_TRY(finalize_rows(r, r.w.pick, r.npick, 0));
    nblk = (r.npick + FIN_BLOCK - 1) / FIN_BLOCK;
    return launch_argmax(c, c.stream, (long)nblk, nullptr, nullptr, Bell{nullptr, 0, nullptr});
}

// 2 (speculating). the lb set AND the r.nx extras in ONE exact round: the picks with three runner-ups per group
// (prune_pick4_kernel), the extras chosen from the runner-ups (prune_extras_kernel), both gathered into one block -- picks
// first -- and contracted together; the picks finalized into blocks [0, nblk) as lb_set does, the extras into the nblk_x
// blocks behind them.  The bar is lb_set's: the arg-max over the PICKS' blocks alone.
template <typename T>
static hipError_t lb_set_with_extras(PruneRun<T> &r, int64_t &nblk, int64_t &nblk_x) {
    Context &c = r.c;
    const PruneWs &w = r.w;
    hipLaunchKernelGGL(prune_pick4_kernel, dim3((unsigned)r.npick), dim3(256), 0, c.stream, w.ub, (long)c.M, (long)r.gs, w.pick, w.runner);
    TGP_TRY(hipGetLastError());
    const int R = (int)(3 * r.npick);
    hipLaunchKernelGGL(prune_extras_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, c.stream, w.ub, w.runner, R, (int)r.nx,
                       (long long)r.nx, w.extras, w.sel, w.misc);
    TGP_TRY(hipGetLastError());
    TGP_TRY(gather_rows(r, w.pick, r.npick, w.extras, r.nx));
    TGP_TRY(contract_rows<T>(c, r.p, r.cs, r.npick + r.nx, r.cur));
    TGP_TRY(finalize_rows(r, w.pick, r.npick, 0));
    nblk = (r.npick + FIN_BLOCK - 1) / FIN_BLOCK;
    TGP_TRY(finalize_rows(r, w.extras, r.nx, nblk, r.npick));
    nblk_x = (r.nx + FIN_BLOCK - 1) / FIN_BLOCK;
    return launch_argmax(c, c.stream, (long)nblk, nullptr, nullptr, Bell{nullptr, 0, nullptr});
}

// 3. the candidates of ub[0, m) that reach the bar, compacted in order into out; their number comes back to the host
// (the launches behind it are sized by the count).  leftover (the speculative round): with it comes the number of them that
// are not among the extras
template <typename T>
static hipError_t survivors(PruneRun<T> &r, const double *ub, int64_t m, const long long *src, long long *out, long long &n,
                            long long *leftover = nullptr) {
    Context &c = r.c;
    const PruneWs &w = r.w;
    hipStream_t st = c.stream;
    const int64_t nb = (m + 255) / 256;
    SurvArgs s{ub, (long)m, w.pick, (long)r.gs, c.d_best, r.b.margin, w.bcnt, w.boff, out, src, nullptr, nullptr, nullptr};
    if (leftover) { s.runner = w.runner; s.sel = w.sel; s.leftover = reinterpret_cast<int *>(w.misc + 1); }
    hipLaunchKernelGGL(prune_count_kernel, dim3((unsigned)nb), dim3(256), 0, st, s);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(prune_scan_kernel, dim3(1), dim3(1024), 0, st, w.bcnt, (int)nb, w.boff, w.misc);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(prune_scatter_kernel, dim3((unsigned)nb), dim3(256), 0, st, s);
    TGP_TRY(hipGetLastError());
    if (!leftover) {
        TGP_TRY(hipMemcpyAsync(&n, w.misc, sizeof(long long), hipMemcpyDeviceToHost, st));
        return hipStreamSynchronize(st);
    }
    long long back[2] = {0, 0};   // [0] the count, [1] the leftover count (prune_extras_kernel zeroed it)
    TGP_TRY(hipMemcpyAsync(back, w.misc, sizeof back, hipMemcpyDeviceToHost, st));
    TGP_TRY(hipStreamSynchronize(st));
    n = back[0]; *leftover = back[1];
    return hipSuccess;
}

// 4. behind the screen, by the number of its survivors S0 (in w.sidx): more than `keep` -- the screen was too loose for this
// batch: the tight bound of every candidate, against the same lb; more than TGP_PRUNE_DIRECT -- the tight bound on the
// gathered S0 rows and a second filter (S1, in w.sidx1); else S0 as it is.  nsurv / sidx: the set to contract
template <typename T>
static hipError_t narrow_after_screen(PruneRun<T> &r, long long &nsurv, const long long *&sidx) {
    Context &c = r.c;
    const PruneWs &w = r.w;
    if (nsurv > r.keep) {
        r.cur.restart();
        TGP_TRY(tight_bound<T>(r, r.Cs, c.ws_Mpad, c.M, w.ub));
        TGP_TRY(survivors(r, w.ub, c.M, nullptr, w.sidx, nsurv));
    } else if (nsurv > tuning_prune_direct_now()) {
        TGP_TRY(gather_rows(r, w.sidx, nsurv));
        r.cur.restart();
        TGP_TRY(tight_bound<T>(r, r.cs, pad128(nsurv), nsurv, w.ub1));
        const long long n0 = nsurv;
        TGP_TRY(survivors(r, w.ub1, n0, w.sidx, w.sidx1, nsurv));
        sidx = w.sidx1;
    }
    r.cur.restart();
    return hipSuccess;
}

// 5. the survivors contracted like the lb set, then ONE arg-max over both sets' partials with the batch indices
template <typename T>
static hipError_t contract_survivors_and_pick(PruneRun<T> &r, const long long *sidx, int64_t nsurv, int64_t nblk_lb) {
    int64_t nblk = 0;
    if (nsurv > 0) {
        TGP_TRY(gather_rows(r, sidx, nsurv));
        TGP_TRY(contract_rows<T>(r.c, r.p, r.cs, nsurv, r.cur));
        TGP_TRY(finalize_rows(r, sidx, nsurv, nblk_lb));
        nblk = (nsurv + FIN_BLOCK - 1) / FIN_BLOCK;
    }
    return launch_argmax(r.c, r.c.stream, (long)(nblk_lb + nblk), r.call.winner, r.call.res, Bell{nullptr, 0, nullptr});
}

// what every bound pass of this sweep shares: the partial sums' home, the error scale of the tight pass, the interval of
// sigma, the acquisition and the margin
static BoundArgs bound_args(const Context &c, const SweepCall &call, double margin) {
    BoundArgs b{};
    b.mupart = c.d_mupart; b.abspart = c.d_part; b.ldpart = c.ws_Mpad;
    b.err_scale = 4.0 * (double)((int)c.N + 8) * 0x1p-53;
    b.y_mean = c.y_mean; b.y_std = c.y_std;
    b.sig_lo = sqrt((0.99 * c.noise) * (c.y_std * c.y_std));
    b.sig_hi = sqrt((c.constant + c.noise) * (c.y_std * c.y_std));
    b.acq = call.acq; b.sf = call.sf; b.incumbent = call.incumbent; b.param = call.param; b.margin = margin;
    return b;
}

// done = false: too many survivors -- the caller runs the full schedule (nothing of this call's results is left behind)
//
// With the screen (TGP_PRUNE_SCREEN, f32 + RBF; prune_screen.hpp) the order of work is
//   1. screen over all M: mu_s and E(c) with |mu_s - mu~| <= E  ->  prune_bound_kernel (the error as its input)  ->  ub0
//      (TGP_SCREEN_ARITH: on the fp16 matrix pipe with the k-weighted E of prune_screen_h2.hpp, or the f32 kernel);
//   2. the lb set picked from ub0 and contracted exactly -> lb (the code below, unchanged);
//   3. count / scan / scatter on ub0 -> the screen's survivors S0 (one host synchronisation for the count);
//   4. |S0| <= TGP_PRUNE_DIRECT: S0 is contracted as it is.  |S0| > prune_frac M: the tight bound pass over all M --
//      the schedule without a screen from its step 1 on, the lb set kept.  Between the two: the tight bound pass
//      (kstar XP = 4 + prune_bound_kernel, their arithmetic and err_scale unchanged) on the gathered S0 rows, its grid
//      splitting the training points until the chip is full, and a second filter against lb -> S1 (a second
//      synchronisation for its count);
//   5. gather, contract, finalize, ONE arg-max over the lb set and the last survivor set.
// Why the result is the full sweep's, bit for bit: a candidate's exact value a(c) is formed from the contraction's mean
// mu~(c) and a variance inside [sig_lo^2, sig_hi^2]; ub0(c) >= a(c) because mu~ lies within E(c) of mu_s(c) and
// prune_bound_kernel takes the end of that interval, and of the variance's, that raises the acquisition; the tight bound
// ub1(c) >= a(c) as before.  The winner w of the full sweep has a(w) >= a(any lb-set member) = lb, hence ub0(w) >= lb and
// ub1(w) >= lb: it is in the lb set or survives every filter, and so does every candidate that ties with it.  Every
// contracted candidate goes through the full sweep's arithmetic, the one arg-max sees batch indices, and no skipped
// candidate can clamp (the gate above): value, index and n_clamped are the full sweep's.  The screen's own values and
// its looseness never reach a result; they only move work between "skipped" and "contracted".
//
// The speculative round (TGP_PRUNE_SPEC).  Steps 2 and 5 are two exact rounds in series only because the survivors are
// named by lb, and a small round lasts as long as its heaviest workgroup's k-chain however few rows it holds: the second
// round's rows cost next to nothing as more workgroups of the first.  So the survivors are guessed: the runner-ups -- the
// second to fourth bound of each group -- ranked by bound, the first TGP_PRUNE_SPEC_CAP of them (the extras, in that
// order) gathered behind the picks and contracted in the lb set's round; the picks' blocks alone give lb, as in step 2;
// step 3 runs unchanged and also counts the survivors that are no extras.  None left over (a hit): the arg-max over the
// picks' and the extras' blocks ends the sweep.  Otherwise (a miss) steps 4 and 5 run as if the extras had never been.
// Mode 1 speculates only when the handle's previous pruned sweep ended pruned with 1 .. cap survivors of its first filter:
// a handle's first sweep, and every sweep after one without survivors, makes today's launches one for one.  The history
// and the guess choose a schedule, never a value.
// Why the result is still the full sweep's, byte for byte: (a) lb is the same value -- the same picks (prune_pick4_kernel's
// first place is prune_pick_kernel's), each contracted by the full sweep's arithmetic, and a contracted candidate's value
// does not depend on which row of which launch it sat in (contract_variant); (b) every candidate with ub >= lb - margin
// |lb| is contracted before the final arg-max -- on a hit the survivors are all extras, on a miss by steps 4 and 5; (c) an
// extra that is no survivor has a value <= ub < lb - margin |lb| <= lb and cannot win or tie (lb = -inf: every candidate
// survives; the arg-max sees batch indices, so the lowest index still wins a tie among survivors); (d) under the clamp gate
// no candidate clamps, so the extras add nothing to the counter.  last_prune() reports what the two-round schedule would.
template <typename T>
static hipError_t sweep_pruned(Context &c, const SweepPlan<T> &p, const SweepCall &call, bool front_usable, bool &done) {
    done = false;
    const Tuning &tu = tuning();
    const int64_t M = c.M;
    const int64_t top = tu.prune_top < 1 ? 1 : tu.prune_top;
    const int64_t gs = (M + top - 1) / top, npick = (M + gs - 1) / gs;
    const double frac = tuning_prune_frac_now();
    const int64_t keep = frac < 0.0 ? -1 : (frac >= 1.0 ? M : (int64_t)(frac * (double)M));   // most survivors taken
    // the speculative round (the comment above): this many extras ride in the lb set's exact round
    const int spec_mode = tuning_prune_spec_now();
    const int64_t cap = tuning_prune_spec_cap_now();
    const int64_t last = M - (npick - 1) * gs;   // members of the last group
    const int64_t nrunner = (npick - 1) * (gs - 1 < 3 ? gs - 1 : 3) + (last - 1 < 3 ? last - 1 : 3);
    const int64_t nx_max = spec_mode != 0 && cap > 0 && 3 * npick <= SPEC_MAXR ? (cap < nrunner ? cap : nrunner) : 0;
    const bool spec = nx_max > 0 && (spec_mode >= 2 || (c.prune_hist >= 1 && c.prune_hist <= cap));
    const int64_t rows_cap = pad128(npick + nx_max > keep ? npick + nx_max : keep);
    const bool screen = sizeof(T) == 4 && c.kernel == TGP_RBF && c.D <= SCR_MAXD && tuning_prune_screen_now() != 0;
    // the screen's arithmetic: fp16 planes and the weighted error where its closed form is no looser than the f32 screen's
    const bool h2 = screen && tuning_screen_arith_now() == 2 && c.D >= SCRH_MIN_D;
    PruneRun<T> r{c, p, call, PruneWs{}, BoundArgs{}, reinterpret_cast<const T *>(c.d_Cs.get()), train_points<T>(c), nullptr,
                  gs, npick, keep, screen, h2, ProfCursor{c, c.stream, -1}};
    TGP_TRY(prune_workspace<T>(c, npick, rows_cap, screen, h2, nx_max > 0, r.w));
    TGP_TRY(lds_opt_in(c, p.early.kern, p.early.lds));   // (the request the fit's early row tiles make of the same kernel)
    r.cs = reinterpret_cast<T *>(r.w.cs);
    c.prune_screen = -1;
    c.prune_arith = 0;
    c.prune_hist = -1;   // (what this sweep leaves for the next one's choice: set where it ends in state 0)
    if (!front_usable) TGP_TRY(issue_prep<T>(c, c.stream));   // (a fit's front has scaled them already)
    r.cur.restart();
    r.b = bound_args(c, call, tu.prune_margin);
    r.nx = spec ? nx_max : 0;

    TGP_TRY(bound_all(r));                                                   // 1. the bound of every candidate
    int64_t nblk_lb = 0, nblk_x = 0;
    long long nsurv = 0, leftover = 0;
    const long long *sidx = r.w.sidx;
    if (spec) {
        TGP_TRY(lb_set_with_extras(r, nblk_lb, nblk_x));                     // 2. the lb set and the extras, exactly: the bar
        TGP_TRY(survivors(r, r.w.ub, M, nullptr, r.w.sidx, nsurv, &leftover));   // 3. the survivors; how many the extras miss
    } else {
        TGP_TRY(lb_set(r, nblk_lb));                                         // 2. the lb set, exactly: the bar
        TGP_TRY(survivors(r, r.w.ub, M, nullptr, r.w.sidx, nsurv));          // 3. the survivors, in index order
    }
    c.prune_lbset = npick;
    const long long nsurv0 = nsurv;   // the first filter's survivors
    if (spec && leftover == 0 && nsurv <= r.nx && nsurv <= keep && (!screen || nsurv <= tuning_prune_direct_now())) {
        // hit: every survivor is an extra and already contracted -- ONE arg-max over the picks' and the extras' blocks
        if (screen) c.prune_screen = nsurv;
        c.prune_surv = nsurv;
        c.prune_spec = 1;
        TGP_TRY(launch_argmax(c, c.stream, (long)(nblk_lb + nblk_x), call.winner, call.res, Bell{nullptr, 0, nullptr}));
        c.prune_state = 0;
        c.prune_hist = nsurv0;
        done = true;
        return hipSuccess;
    }
    if (spec) c.prune_spec = 2;   // miss: on as if the extras had never been (their blocks are overwritten or not read)
    if (screen) {
        c.prune_screen = nsurv;
        TGP_TRY(narrow_after_screen(r, nsurv, sidx));                        // 4. the screen's survivors, narrowed
    }
    c.prune_surv = nsurv;
    if (nsurv > keep) {
        // the full schedule instead: it counts the lb set's clamps again (the counter was zero when this sweep began)
        c.prune_state = 1;
        return hipMemsetAsync(c.d_besti + 1, 0, sizeof(long long), c.stream);
    }
    TGP_TRY(contract_survivors_and_pick(r, sidx, nsurv, nblk_lb));           // 5. contract them; one arg-max over both sets
    c.prune_state = 0;
    c.prune_hist = nsurv0;
    done = true;
    return hipSuccess;
}

}  // namespace tgp
