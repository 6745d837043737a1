// fit_blocked.hpp -- the schedule of the blocked fit: launch_fit as a driver over named steps.
//
//   fit_prologue, overlap_front, kernel_matrix, prepare_chain
//   per outer block O:  panel_chain(O)  ->  inverse_behind_chain(O)  ->  trailing_update(O)
//   inverse_tail, finish_alpha, overlap_mark, dump_stamps
//
// What is decided before the first launch (outer block, panel mode per block, the switches) is FitPlan, fit_plan.hpp.
//
// NOT a header of its own: fit_kernels.hip includes it once, at its end, behind every kernel and launch_gemm64, so that
// the fit stays in that translation unit -- the same compile flags, the same kernel symbols, the same code object.
#pragma once
#include "fit_plan.hpp"
#include "nt_product.hpp"

namespace tgp {

static_assert(PLAN_NB == NB, "fit_plan.hpp plans in panels of NB columns");

// one blocked fit in flight: what every step of the schedule reads
struct FitRun {
    Context &c;
    const FitPlan plan;
    const hipStream_t s;           // the call's stream: the panel chain
    hipStream_t sbg = nullptr;     // the inverse behind the chain (the device's background stream, or the one on loan)
    hipStream_t spre = nullptr;    // the front of the next sweep (null: none issued)
    const double tiny;             // pivot threshold
    // A handle on a PRIVATE stream (the workers of a threaded hyper-parameter fit) keeps its share of the inverse on that
    // stream: the device has ONE background stream, and the workers' inverses queued on it one behind the other while
    // every worker's chain waited for its own -- three starts side by side at N = 1000 took as long as one after the
    // other (28.5 vs 28.6 ms; 19.1 with the inverses in line, N = 2048 101 -> 83).  Same launches in the same order of
    // arithmetic, so the results are those of the shared-stream path bit for bit.
    const bool bg_shared;          // (bg_lease: the background stream this fit holds on loan)
    int pre_budget128 = 0;         // 128-row tiles of the sweep's launch pair 0 this fit contracts
    unsigned long long *stamp_dev = nullptr;   // debug (TGP_STAMP_FILE): the panels' in-kernel time stamps
};

// the fit's 64 x 64 NT products go through launch_gemm64: the TGP_GEMM64=reg A/B route and the debug build's routes
template <int KR, int TMAP>
static hipError_t fit_on64(const NtProduct &p, hipStream_t st, int nblocks, int batch) {
    return launch_gemm64<64, 64, true, KR, TMAP>(st, p.device, p.args64(), nblocks, batch);
}

static hipError_t fit_prologue(FitRun &r, const double *staged_in, bool zero_linv, unsigned long long *start_stamp) {
    Context &c = r.c;
    const int Np = r.plan.Np, Dp = (int)c.Dp;
    const long NN = (long)Np * Np;
    long blocks = NN / 2 / 256;
    if (blocks > 4096) blocks = 4096;
    // Linv = 0: only when something other than zeros can sit above the diagonal or in the rows this fit
    // skips (a fresh allocation, another leading dimension, an older fit with more rows): everything on
    // and below the diagonal of the rows it does not skip is written by this fit anyway (27 us at Np = 4096,
    // 96 us at 8192 when it has to run)
    if (!zero_linv) blocks = std::min<long>(blocks, std::max<long>(1, ((long)Np * Dp + 255) / 256));
    hipLaunchKernelGGL(fit_prologue_kernel, dim3((unsigned)blocks), dim3(256), 0, r.s,
                       reinterpret_cast<double2 *>(c.d_Linv.get()), zero_linv ? NN / 2 : 0L, staged_in, c.d_Xs, (long)Np * Dp,
                       c.d_yn, (long)Np, c.d_ls, (long)c.D, Dp, c.d_flag, c.d_scal, start_stamp);
    TGP_TRY(hipGetLastError());
    // the f32 copy of Xs right away (it used to be the fit's last launch): the cross-kernel of an f32 sweep that
    // starts inside this fit reads it
    if (c.dtype != TGP_F64) {
        hipLaunchKernelGGL(f64_to_f32_kernel, dim3(64), dim3(256), 0, r.s, c.d_Xs, c.d_Xs32,
                           (long)Np * Dp);
        TGP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

// ---- the front of the next sweep, beside everything that follows (tgp_set_overlap; sweep_kernels.hip) ----
static hipError_t overlap_front(FitRun &r) {
    Context &c = r.c;
    if (c.pre.issue > 0) {
        if (!c.stream_pre) TGP_TRY(device_streams(c.device, nullptr, &c.stream_bg, &c.stream_pre));
        r.spre = c.stream_pre;   // (null: this process has no hardware queue left for a third stream -- no front)
    }
    if (r.spre) {
        TGP_TRY(hipEventRecord(c.pre.ev_in, r.s));
        TGP_TRY(hipStreamWaitEvent(r.spre, c.pre.ev_in, 0));
        TGP_TRY(presweep_front(c, r.spre));
        if (c.pre.issue >= 2 && c.pre.front) {
            // how many 128-row tiles of launch pair 0 the fit takes: a quarter of the rows unless TGP_PRE_TILES says otherwise
            const int n128 = (r.plan.N + 127) / 128;
            r.pre_budget128 = r.plan.pre_tiles >= 0 ? r.plan.pre_tiles : n128 / 4;
        }
    }
    return hipSuccess;
}

// ---- K ----
static hipError_t kernel_matrix(FitRun &r) {
    Context &c = r.c;
    const int Np = r.plan.Np;
    const int nt = Np / PW_T;
    const dim3 grid(nt * (nt + 1) / 2);
    hipLaunchKernelGGL(by_kind(c.kernel, [](auto K) { return kernel_matrix_kernel<K()>; }), grid, dim3(256), 0, r.s, c.d_Xs, c.d_K, r.plan.N, Np, (int)c.Dp, c.constant, c.noise, c.jitter);
    return hipGetLastError();
}

// the look-ahead events and the background stream of an inverse behind the chain; the debug stamps' buffer
static hipError_t prepare_chain(FitRun &r) {
    Context &c = r.c;
    const int Np = r.plan.Np;
    if (r.plan.bginv && r.bg_shared) TGP_TRY(ensure_lookahead(c, (size_t)2 * r.plan.nblk));
    r.sbg = c.bg_lease ? c.bg_lease : c.stream_bg;
    // debug: TGP_STAMP_FILE=path makes every fused panel launch leave in-kernel time stamps (10 ns
    // ticks) and the fit dump them there (tools/stamp_summary.py reads the file); Np <= 8192 only
    // (debug only.  The buffer belongs to the handle -- it goes with the fit's memory -- so fits on several handles, e.g.
    // the threaded hyper-parameter starts, stamp buffers of their own; the FILE is the last finisher's)
    if (r.plan.stamp_path && Np <= 8192) {
        TGP_TRY(c.d_stamp.reserve(2 * 128 * FUSED_STAMP_STRIDE * sizeof(unsigned long long)));
        TGP_TRY(hipMemsetAsync(c.d_stamp, 0, 2 * 128 * FUSED_STAMP_STRIDE * sizeof(unsigned long long), r.s));
        r.stamp_dev = c.d_stamp;
    }
    return hipSuccess;
}

// ---- the panels of one outer block ----
// A panel function gets the panel at column o (the kk-th of its outer block), rem = the real block rows below it and
// ncol = the panels right of it inside the block that exist (the last outer block may be partial).

// one launch per panel: see fused_panel_kernel.  Slot kk & 1 of Apan holds this panel's
// unsolved blocks; the last panel of an outer block (no update follows) is solved in place.
static hipError_t panel_fused(FitRun &r, int o, int kk, int rem, int ncol) {
    Context &c = r.c;
    const int Np = r.plan.Np;
    const long slot = (long)(Np / NB) * NB * NB;
    unsigned long long *st0 = r.stamp_dev ? r.stamp_dev + (size_t)(2 * (o / NB)) * FUSED_STAMP_STRIDE : nullptr;
    if (kk == 0) {
        hipLaunchKernelGGL(fused_panel_kernel, dim3(1 + (ncol > 0 ? rem : 0)), dim3(256), 0, r.s, c.d_K, Np, o, 0, 1,
                           c.d_Apan, c.d_Apan, c.d_Dinv, c.d_Linv, c.d_scal, c.d_flag, r.tiny, st0);
        TGP_TRY(hipGetLastError());
    }
    if (rem == 0) return hipSuccess;
    if (ncol > 0) {
        hipLaunchKernelGGL(fused_panel_kernel, dim3(1 + rem * ncol), dim3(256), 0, r.s, c.d_K, Np, o, 1, ncol,
                           c.d_Apan + (kk & 1) * slot, c.d_Apan + ((kk + 1) & 1) * slot, c.d_Dinv,
                           c.d_Linv, c.d_scal, c.d_flag, r.tiny, st0 ? st0 + FUSED_STAMP_STRIDE : nullptr);
    } else {
        hipLaunchKernelGGL(panel_solve_kernel, dim3(rem), dim3(256), 0, r.s, c.d_K, Np, o, c.d_Dinv);
    }
    return hipGetLastError();
}

// the pivot off the update's back: see pivot_update_kernel.  The first panel of an outer block
// factors its pivot alone (the trailing update before it has touched everything); every
// later pivot was factored beside the previous panel's update.
static hipError_t panel_pivot_beside(FitRun &r, int o, int kk, int rem, int ncol) {
    Context &c = r.c;
    const int Np = r.plan.Np;
    if (kk == 0) {
        hipLaunchKernelGGL(pivot_update_kernel, dim3(1), dim3(256), 0, r.s, c.d_K, Np, o, 0, 1, c.d_Dinv, c.d_Linv,
                           c.d_scal, c.d_flag, r.tiny);
        TGP_TRY(hipGetLastError());
    }
    if (rem == 0) return hipSuccess;
    hipLaunchKernelGGL(panel_solve_kernel, dim3(rem), dim3(256), 0, r.s, c.d_K, Np, o, c.d_Dinv);
    TGP_TRY(hipGetLastError());
    if (ncol > 0) {
        hipLaunchKernelGGL(pivot_update_kernel, dim3(1 + rem * ncol), dim3(256), 0, r.s, c.d_K, Np, o + NB, 1, ncol,
                           c.d_Dinv, c.d_Linv, c.d_scal, c.d_flag, r.tiny);
        TGP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

// diagonal block (factor + inverse) and, in the same launch, the panel solve of every
// row block below it; then the rank-64 update of the block's remaining columns
static hipError_t panel_plain(FitRun &r, int o, int kk, int rem, int ncol) {
    Context &c = r.c;
    const int Np = r.plan.Np, panel_var = r.plan.panel_var;
    auto pk = panel_kernel<3>;
    if (panel_var == 38) pk = panel_kernel<38>;
    else if (panel_var == 8) pk = panel_kernel<8>;
    else if (panel_var == 4) pk = panel_kernel<4>;
    else if (panel_var == 0) pk = panel_kernel<0>;
    if (panel_var == 5) pk = panel_d_kernel;
    hipLaunchKernelGGL(pk,
                       dim3(rem + 1), dim3(256), 0, r.s, c.d_K, Np, o, c.d_Dinv,
                       c.d_Linv, c.d_Dinv + (long)(Np / NB) * NB * NB, c.d_scal, c.d_flag, r.tiny);   // second half of Dinv: where a diagonal block waits
    TGP_TRY(hipGetLastError());
    if (rem == 0 || ncol <= 0) return hipSuccess;
    if (!r.plan.inner_generic) {   // A[:, o+64 : O+OB] -= L_:k * L_jk^T
        hipLaunchKernelGGL(rank64_update_kernel, dim3(rem * ncol), dim3(256), 0, r.s, c.d_K, Np, o, ncol);
        return hipGetLastError();
    }
    double *panel = c.d_K + (long)(o + NB) * Np + o;
    NtProduct p;
    p.device = c.device;
    p.A = panel; p.lda = Np;
    p.B = panel; p.ldb = Np;
    p.C = c.d_K + (long)(o + NB) * Np + (o + NB); p.ldc = Np;
    p.rows = rem * NB; p.cols = ncol * NB; p.K = NB; p.alpha = -1.0; p.beta = 1.0;
    return fit_on64<KR_FULL, TM_FULL>(p, r.s, rem * ncol, 1);
}

// the panel chain of the outer block at O, on the call's stream
static hipError_t panel_chain(FitRun &r, int O) {
    const FitPlan &pl = r.plan;
    const PanelMode mode = pl.panel_mode(O);
    const auto panel = mode == PANEL_FUSED ? panel_fused : (mode == PANEL_PIVOT_BESIDE ? panel_pivot_beside : panel_plain);
    for (int kk = 0; kk < pl.OB / NB; ++kk) {
        const int o = O + kk * NB;
        if (o >= pl.Nr) break;
        const int rem = (pl.Nr - o - NB) / NB;   // real block rows below
        int ncol = pl.OB / NB - 1 - kk;          // panels left inside this outer block
        if (ncol > rem) ncol = rem;              // ... that exist (last, partial outer block)
        TGP_TRY(panel(r, o, kk, rem, ncol));
    }
    return hipSuccess;
}

// ---- the inverse factor: [[A,0],[C,B]]^-1 = [[Ai,0],[-Bi*C*Ai,Bi]] ----
// Level 64 -> 128 on the k-major GEMM template; from 128 up the transpose U = Linv^T is kept
// alongside so both products of a merge are NT:
//     T^T   = U11 * L21^T            (U11 upper triangular: k from the tile's own row on)  -> W
//     Linv21 = -Linv22 * (T^T)^T     (Linv22 lower triangular), stored to Linv and, transposed, to U
// level64(st, o, pairs): the `pairs` 128-blocks from row o on, one batched launch per product.
static hipError_t level64(FitRun &r, hipStream_t st, long o, int pairs) {
    Context &c = r.c;
    const int Np = r.plan.Np;
    if (r.plan.level64_fused) {
        hipLaunchKernelGGL(level64_fused_kernel, dim3(pairs), dim3(256), 0, st, c.d_K, c.d_Linv, c.d_U, Np, o);
        return hipGetLastError();
    }
    const long bs64 = (long)2 * NB * ((long)Np + 1);
    const long d = o * ((long)Np + 1);
    // (these two are NN products, B k-major, on the register-staged template: the description serves them as it stands)
    NtProduct t;   // T = L21 * L11inv -> W
    t.device = c.device;
    t.A = c.d_K + d + (long)NB * Np; t.lda = Np; t.strideA = bs64;
    t.B = c.d_Linv + d; t.ldb = Np; t.strideB = bs64;
    t.C = c.d_W + d + (long)NB * Np; t.ldc = Np; t.strideC = bs64;
    t.rows = t.cols = NB; t.K = NB; t.alpha = 1.0; t.beta = 0.0;
    NtProduct u;   // Linv21 = -L22inv * T
    u.device = c.device;
    u.A = c.d_Linv + d + (long)NB * Np + NB; u.lda = Np; u.strideA = bs64;
    u.B = c.d_W + d + (long)NB * Np; u.ldb = Np; u.strideB = bs64;
    u.C = c.d_Linv + d + (long)NB * Np; u.ldc = Np; u.strideC = bs64;
    u.rows = u.cols = NB; u.K = NB; u.alpha = -1.0; u.beta = 0.0;
    TGP_TRY((launch_gemm64<64, 64, false, KR_LOWER_B, TM_FULL>(st, c.device, t.args64(), 1, pairs)));
    TGP_TRY((launch_gemm64<64, 64, false, KR_LOWER_A, TM_FULL>(st, c.device, u.args64(), 1, pairs)));
    hipLaunchKernelGGL(transpose_diag128_kernel, dim3(pairs, 16), dim3(256), 0, st, c.d_Linv + d,
                       c.d_U + d, Np);
    return hipGetLastError();
}

// Merges with a leading block up to MERGE64 (few, very unequal 128-tiles) go to the 64 x 64
// register-staged template like the small trailing updates.  Measured: fit 4.52 -> 4.13 ms
// at N = 4096, 0.54 -> 0.46 ms at N = 512; the 4096-level of N = 8192 is faster on the
// 128-tile direct-to-LDS kernel (13.39 vs 13.59 ms), hence 2048.
// leading block [o, o+a), trailing block [o+a, o+a+b); a, b multiples of 128 (64 with small = true)
static hipError_t merge_t(FitRun &r, hipStream_t st, long o, int a, int b, int nprob, long bstride, bool small) {
    Context &c = r.c;
    const long Np = r.plan.Np;
    NtProduct tt;   // T^T (a x b) -> W[o.., o+a..]
    tt.device = c.device;
    tt.A = c.d_U + o * Np + o; tt.lda = Np; tt.strideA = bstride;
    tt.B = c.d_K + (o + a) * Np + o; tt.ldb = Np; tt.strideB = bstride;
    tt.C = c.d_W + o * Np + (o + a); tt.ldc = Np; tt.strideC = bstride;
    tt.rows = a; tt.cols = b; tt.K = a; tt.alpha = 1.0; tt.beta = 0.0;
    if (small || a <= r.plan.merge64) return fit_on64<KR_UPPER_A, TM_FULL>(tt, st, (a / NB) * (b / NB), nprob);
    return tt.on128<KN_UPPER_A, TM_FULL>(st, (a / 128) * (b / 128), nprob);
}
static hipError_t merge_u(FitRun &r, hipStream_t st, long o, int a, int b, int nprob, long bstride, bool small) {
    Context &c = r.c;
    const long Np = r.plan.Np;
    NtProduct uu;   // Linv21 (b x a) and its transpose into U
    uu.device = c.device;
    uu.A = c.d_Linv + (o + a) * Np + (o + a); uu.lda = Np; uu.strideA = bstride;
    uu.B = c.d_W + o * Np + (o + a); uu.ldb = Np; uu.strideB = bstride;
    uu.C = c.d_Linv + (o + a) * Np + o; uu.ldc = Np; uu.strideC = bstride;
    uu.Ct = c.d_U + o * Np + (o + a); uu.ldct = Np; uu.strideCt = bstride;
    uu.rows = b; uu.cols = a; uu.K = b; uu.alpha = -1.0; uu.beta = 0.0;
    if (small || a <= r.plan.merge64) return fit_on64<KR_LOWER_A, TM_FULL>(uu, st, (b / NB) * (a / NB), nprob);
    return uu.on128<KN_LOWER_A, TM_FULL>(st, (b / 128) * (a / 128), nprob);
}
static hipError_t merge(FitRun &r, hipStream_t st, long o, int a, int b, int nprob, long bstride) {
    TGP_TRY(merge_t(r, st, o, a, b, nprob, bstride, false));
    return merge_u(r, st, o, a, b, nprob, bstride, false);
}

// (1) level by level over the whole matrix, after the factorisation: all complete pairs of a
// level share one batched launch; an odd segment out (Np is a multiple of 256, not necessarily
// a power of two) is merged separately when it finds a partner.
static hipError_t inverse_levels(FitRun &r, hipStream_t st) {
    const int Np = r.plan.Np;
    TGP_TRY(level64(r, st, 0, Np / (2 * NB)));
    int nfull = Np / 128;  // complete segments of size sz
    int tail = 0;          // size of the trailing odd segment (0 = none)
    for (int sz = 128; nfull + (tail ? 1 : 0) > 1; sz *= 2) {
        const int pairs = nfull / 2;
        if (pairs > 0) TGP_TRY(merge(r, st, 0, sz, sz, pairs, (long)2 * sz * ((long)Np + 1)));
        if (nfull & 1) {
            const long o = (long)(nfull - 1) * sz;
            if (tail) {   // odd full segment + tail -> new tail
                TGP_TRY(merge(r, st, o, sz, tail, 1, 0));
                tail += sz;
            } else {
                tail = sz;
            }
        }
        nfull = pairs;
    }
    return hipSuccess;
}

// (2) outer block by outer block, BEHIND the panel chain on the background stream: once the
// panels of block [O, E) are final,
//     X_bb              the block's own inverse (levels 64, 128, 256 inside the block)
//     Linv[O:E, 0:O]  = -X_bb * T[O:E, 0:O]                       (T^T sits in W above the diagonal)
//     T[E:, 0:E]     +=  L[E:, O:E] * Linv[O:E, 0:E]              (every later row block's share)
// so that after the last panel only the last block's X_bb and row block are left to do.
// `inner` = the block's own inverse X_bb (false: already there, see inverse_inner_all)
static hipError_t inverse_block(FitRun &r, hipStream_t st, long O, long E, bool inner = true) {
    Context &c = r.c;
    const int Np = r.plan.Np;
    const int len = (int)(E - O);
    if (inner) {
        TGP_TRY(level64(r, st, O, len / 128));
        for (int sz = 128; sz < len; sz *= 2)
            TGP_TRY(merge(r, st, O, sz, sz, len / (2 * sz), (long)2 * sz * ((long)Np + 1)));
    }
    if (O > 0) TGP_TRY(merge_u(r, st, 0, (int)O, len, 1, 0, true));
    if (E < Np) {
        if (O > 0) {   // rows 0:O of T^T: W[0:O, E:] += U[0:O, O:E] * L[E:, O:E]^T
            NtProduct g;
            g.device = c.device;
            g.A = c.d_U + O; g.lda = Np;
            g.B = c.d_K + E * Np + O; g.ldb = Np;
            g.C = c.d_W + E; g.ldc = Np;
            g.rows = (int)O; g.cols = (int)(Np - E); g.K = len; g.alpha = 1.0; g.beta = 1.0;
            TGP_TRY((fit_on64<KR_FULL, TM_FULL>(g, st, (int)(O / NB) * (int)((Np - E) / NB), 1)));
        }
        TGP_TRY(merge_t(r, st, O, len, (int)(Np - E), 1, 0, true));   // rows O:E, first contribution
    }
    return hipSuccess;
}

// The X_bb of EVERY outer block at once, after the factorisation: the launches of inverse_block's first part batched
// over the blocks (a pair of 64-, 128-, ... row segments never straddles an outer block: OB and the tail are powers
// of two times 128) -- the same tiles with the same operands in the same k order, i.e. the same bits, in 1 + 2 log2(OB /
// 128) launches instead of that many per block.  For a fit that cannot put its inverse behind the chain (a handle on a
// private stream): 40 -> 25 launches at Np = 2048, 80 -> 45 at 4096.
static hipError_t inverse_inner_all(FitRun &r, hipStream_t st) {
    const int Np = r.plan.Np;
    TGP_TRY(level64(r, st, 0, Np / (2 * NB)));
    for (int sz = 128; sz < r.plan.OB; sz *= 2) {
        const int pairs = Np / (2 * sz);
        if (pairs > 0) TGP_TRY(merge(r, st, 0, sz, sz, pairs, (long)2 * sz * ((long)Np + 1)));
    }
    return hipSuccess;
}

// ... and with a row block of Linv final: its rows of z = Linv yn, its share of alpha = Linv^T z,
// its f32 copy for an f32 sweep
static hipError_t finish_block(FitRun &r, hipStream_t st, long O, long E) {
    Context &c = r.c;
    const int Np = r.plan.Np;
    hipLaunchKernelGGL(rowblock_finish_kernel, dim3((unsigned)(E - O)), dim3(256), 0, st, c.d_Linv, c.d_yn,
                       c.d_z, c.dtype != TGP_F64 ? c.d_Linv32 : nullptr, Np, (int)O);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rowblock_cols_kernel, dim3((unsigned)(E / 64), (unsigned)((E - O) / GEMV_SLICE)), dim3(256), 0, st,
                       c.d_Linv, c.d_z, c.d_apart, c.d_apart + (long)(Np / GEMV_SLICE) * Np, Np, (int)O);
    return hipGetLastError();
}

// every outer block but the last: its share of the inverse goes behind the chain
static hipError_t inverse_behind_chain(FitRun &r, int O) {
    Context &c = r.c;
    const int OB = r.plan.OB;
    if (!(r.plan.bginv && O + OB < r.plan.Np)) return hipSuccess;
    // (a handle on a private stream without the background stream on loan: after the last panel, inverse_tail)
    if (!r.bg_shared) return hipSuccess;
    const int b = O / OB;
    TGP_TRY(hipEventRecord(c.ev_la[2 * b], r.s));
    TGP_TRY(hipStreamWaitEvent(r.sbg, c.ev_la[2 * b], 0));
    TGP_TRY(inverse_block(r, r.sbg, O, O + OB));
    TGP_TRY(finish_block(r, r.sbg, O, O + OB));
    TGP_TRY(hipEventRecord(c.ev_la[2 * b + 1], r.sbg));
    if (r.spre && r.pre_budget128 > c.pre.rows128) {   // rows < O + OB of Linv (and its f32 copy) are final behind that event
        TGP_TRY(hipStreamWaitEvent(r.spre, c.ev_la[2 * b + 1], 0));
        TGP_TRY(presweep_rows(c, r.spre, O + OB, r.pre_budget128));
    }
    return hipSuccess;
}

// the ONE rank-OB update of the trailing matrix behind the outer block at O
static hipError_t trailing_update(FitRun &r, int O) {
    Context &c = r.c;
    const int Np = r.plan.Np, OB = r.plan.OB;
    const int R = ((r.plan.Nr - O - OB + 127) / 128) * 128;   // real trailing rows in whole 128-tiles (<= Np - O - OB)
    if (R <= 0) return hipSuccess;
    NtProduct g;   // A[i][j] -= L[i][O:O+OB] * L[j][O:O+OB]^T, i >= j >= O+OB
    g.device = c.device;
    g.A = c.d_K + (long)(O + OB) * Np + O; g.lda = Np;
    g.B = g.A; g.ldb = Np;
    g.C = c.d_K + (long)(O + OB) * Np + (O + OB); g.ldc = Np;
    g.rows = g.cols = R; g.K = OB; g.alpha = -1.0; g.beta = 1.0;
    // Trailing matrices up to TRAIL64 rows have too few 128-tiles to fill the chip and each tile
    // then runs its whole k-range alone on a CU: use 64 x 64 tiles (4x the tiles, a quarter of
    // the critical path) on the register-staged template.  Measured: fit 4.73 -> 4.50 ms at
    // N = 4096, 14.35 -> 13.59 ms at N = 8192; from N = 20000 on the 128-tile direct-to-LDS
    // kernel wins again (448 vs 419 ms at N = 33000), hence the threshold.
    if (R <= r.plan.trail64) {
        const int nt = R / NB;
        return fit_on64<KR_FULL, TM_LOWER>(g, r.s, nt * (nt + 1) / 2, 1);
    }
    const int nt = R / 128;
    return g.on128<KN_FULL, TM_LOWER>(r.s, nt * (nt + 1) / 2, 1);
}

// what is left of the inverse behind the last panel
static hipError_t inverse_tail(FitRun &r) {
    Context &c = r.c;
    const int Np = r.plan.Np, OB = r.plan.OB, nblk = r.plan.nblk;
    if (!r.plan.bginv) return inverse_levels(r, r.s);   // all of it
    const long O = (long)(nblk - 1) * OB;
    if (r.bg_shared) {   // the last block's own inverse and row block, behind the background stream's last event
        TGP_TRY(hipStreamWaitEvent(r.s, c.ev_la[2 * (nblk - 2) + 1], 0));
        return inverse_block(r, r.s, O, Np);
    }
    // in line, on the private stream: every block's own inverse in batched launches, then block by block what
    // depends on the blocks before it -- the arithmetic of the background schedule, operation for operation
    TGP_TRY(inverse_inner_all(r, r.s));
    for (long Ob = 0; Ob < O; Ob += OB) {
        TGP_TRY(inverse_block(r, r.s, Ob, Ob + OB, false));
        TGP_TRY(finish_block(r, r.s, Ob, Ob + OB));
    }
    return inverse_block(r, r.s, O, Np, false);
}

// ---- alpha = Linv^T (Linv yn),  yn . alpha ----
static hipError_t finish_alpha(FitRun &r, double *res_host) {
    Context &c = r.c;
    const int Np = r.plan.Np;
    const hipStream_t s = r.s;
    if (r.plan.bginv) {   // sliced: every earlier row block has left its share (finish_block), the last one does now
        TGP_TRY(finish_block(r, s, (long)(r.plan.nblk - 1) * r.plan.OB, Np));
        hipLaunchKernelGGL(alpha_finish_sliced_kernel, dim3(Np / 64), dim3(256), 0, s, c.d_apart,
                           c.d_apart + (long)(Np / GEMV_SLICE) * Np, c.d_alpha, c.d_scal, Np, c.d_flag, res_host);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(gemv_lower_rows_kernel, dim3((Np + 3) / 4), dim3(256), 0, s, c.d_Linv,
                       c.d_yn, c.d_z, Np);
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(gemv_lower_cols_kernel, dim3(Np / 64, GEMV_RS), dim3(256), 0, s, c.d_Linv,
                       c.d_z, c.d_W, Np);   // W is free again after the inverse
    TGP_TRY(hipGetLastError());
    hipLaunchKernelGGL(alpha_finish_kernel, dim3(1), dim3(256), 0, s, c.d_W, c.d_yn, c.d_alpha,
                       c.d_scal, Np, c.d_flag, res_host);
    TGP_TRY(hipGetLastError());
    if (c.dtype != TGP_F64) {
        hipLaunchKernelGGL(f64_to_f32_kernel, dim3(2048), dim3(256), 0, s, c.d_Linv, c.d_Linv32, (long)Np * Np);
        TGP_TRY(hipGetLastError());
    }
    return hipSuccess;
}

// the sweep's front is complete behind this event (tgp_sweep waits for it)
static hipError_t overlap_mark(FitRun &r) {
    if (!r.spre) return hipSuccess;
    TGP_TRY(hipEventRecord(r.c.pre.ev, r.spre));
    r.c.pre.pending = true;
    return hipSuccess;
}

// debug (TGP_STAMP_FILE): the panels' stamps to the file, and the CUs each of the fit's streams reaches to <file>.cus
static hipError_t dump_stamps(FitRun &r) {
    if (!r.stamp_dev) return hipSuccess;
    const char *stamp_path = r.plan.stamp_path;
    std::vector<unsigned long long> hst(2 * 128 * FUSED_STAMP_STRIDE);
    TGP_TRY(hipStreamSynchronize(r.s));
    TGP_TRY(hipMemcpy(hst.data(), r.stamp_dev, hst.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (FILE *fh = fopen(stamp_path, "wb")) {
        fwrite(hst.data(), sizeof(unsigned long long), hst.size(), fh);
        fclose(fh);
    }
    // round 6: the CUs each of the fit's streams reaches (main | background | third), HW_PROBE_WGS workgroups each, in
    // <path>.cus -- so that tools/stamp_summary.py can say whether a panel's pivot workgroup sat on a CU the
    // background stream's GEMMs can run on
    constexpr int HW_PROBE_WGS = 16384;
    unsigned long long *pd = nullptr;
    TGP_TRY(hipMalloc((void **)&pd, 3 * HW_PROBE_WGS * sizeof(unsigned long long)));
    TGP_TRY(hipMemset(pd, 0, 3 * HW_PROBE_WGS * sizeof(unsigned long long)));
    const hipStream_t probe_on[3] = {r.s, r.sbg, r.c.stream_pre};
    for (int k = 0; k < 3; ++k) {
        if (!probe_on[k]) continue;
        hipLaunchKernelGGL(hw_probe_kernel, dim3(HW_PROBE_WGS), dim3(64), 0, probe_on[k], pd + (size_t)k * HW_PROBE_WGS);
        TGP_TRY(hipGetLastError());
        TGP_TRY(hipStreamSynchronize(probe_on[k]));
    }
    std::vector<unsigned long long> hp(3 * HW_PROBE_WGS);
    TGP_TRY(hipMemcpy(hp.data(), pd, hp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    (void)hipFree(pd);
    const std::string cus = std::string(stamp_path) + ".cus";
    if (FILE *fh = fopen(cus.c_str(), "wb")) {
        fwrite(hp.data(), sizeof(unsigned long long), hp.size(), fh);
        fclose(fh);
    }
    return hipSuccess;
}

hipError_t launch_fit(Context &c, const double *staged_in, double *res_host, bool zero_linv, unsigned long long *start_stamp) {
    FitRun r{c, plan_fit((int)c.N, (int)c.Np, tuning()), c.stream, nullptr, nullptr,
             8.0 * 2.220446049250313e-16 * ((c.constant + c.noise) + c.jitter),
             c.stream_own == nullptr || c.bg_lease != nullptr};
    TGP_TRY(fit_prologue(r, staged_in, zero_linv, start_stamp));
    TGP_TRY(overlap_front(r));
    TGP_TRY(kernel_matrix(r));
    TGP_TRY(prepare_chain(r));
    for (int O = 0; O < r.plan.Nr; O += r.plan.OB) {
        TGP_TRY(panel_chain(r, O));
        TGP_TRY(inverse_behind_chain(r, O));
        TGP_TRY(trailing_update(r, O));
    }
    TGP_TRY(inverse_tail(r));
    TGP_TRY(finish_alpha(r, res_host));
    TGP_TRY(overlap_mark(r));
    return dump_stamps(r);
}

}  // namespace tgp
