// fit_plan.hpp -- what the blocked fit decides before its first launch: the outer block, whether the inverse may run behind
// the panel chain, how each outer block's panels are launched, and the tuning switches the schedule reads (once, here).
//
// Plain C++ (no HIP): tests/fit_plan_driver.cpp builds it with g++ and prints the plan over every size.
#pragma once
#include "tuning.hpp"

namespace tgp {

constexpr int PLAN_NB = 64;   // the Cholesky panel (NB of tgp_internal.hpp; fit_blocked.hpp asserts they agree)

// how the panels of one outer block are launched
enum PanelMode { PANEL_FUSED = 0,          // one launch per panel: fused_panel_kernel
                 PANEL_PIVOT_BESIDE = 1,   // the pivot off the update's back: pivot_update_kernel
                 PANEL_PLAIN = 2 };        // diagonal block + panel solve in one launch (FitPlan::panel_var), then the update

struct FitPlan {
    int N = 0, Np = 0;
    // Rows >= N are padding: K is the identity there, so its factor is the identity too and the
    // panels, panel rows and trailing tiles that hold nothing but padding are skipped (their L
    // stays as kernel_matrix_kernel wrote it; Linv stays zero, which is all the sweep needs since
    // the cross-kernel slab is zero in those columns).
    int Nr = 0;        // real rows, rounded up to whole panels
    int OB = 0;        // outer block (multiple of 256)
    int nblk = 0;      // outer blocks of Np
    bool bginv = false;   // the inverse is eligible to run behind the panel chain (whether it does: FitRun::bg_shared)
    // ---- the switches of the schedule ----
    int panel_var = 5;   // A/B: 5 = variant D (block in LDS, MFMA), 3 / 38 = variant C with 4 / 8 columns per barrier, 4 / 8 = variant B, 0 = round-1 form
    int panel_la = 1, panel_fuse = 1, panel_fuse_tiles = 0;
    bool inner_generic = false;
    int level64_fused = 1;
    int merge64 = 0;     // MERGE64
    int trail64 = 0;     // TRAIL64
    int pre_tiles = -1;
    const char *stamp_path = nullptr;   // TGP_STAMP_FILE or null (points into the Tuning the plan was made from)

    int tail() const { return Np % OB; }   // rows of the last, partial outer block (0: none)

    // tiles of the first update of the outer block at O
    int first_update_tiles(int O) const {
        const int NB = PLAN_NB;
        const int rem0 = (Nr - O - NB) / NB;                                  // row blocks below the block's first panel
        return rem0 * (OB / NB - 1 < rem0 ? OB / NB - 1 : rem0);              // tiles of its first update
    }

    // Decided per OUTER BLOCK by the tiles of its first update.  Each fused tile is three f64 products on
    // a CU of its own (10 us against 3 for a plain update tile), so a block with hundreds of them holds
    // CUs the background stream's inverse wants: measured on one box, fit ms at N = 2048 / 4096 / 8192 with
    // the limit at 0 (never): 1.037 / 2.379 / 9.997, 128: 1.004 / 2.373 / 9.953, 256: 1.010 / 2.428 / 9.967,
    // no limit: 1.000 / 2.418 / 10.185 -- the fused launch is kept for blocks of up to 128 tiles
    // (everything up to N = 2048, the last two outer blocks beyond).  TGP_PANEL_FUSE_TILES overrides.
    // Round 4 (MFMAs in VGPR form: a fused tile is shorter): 384 -- N = 2048 0.949 -> 0.903 ms, 3072 1.506 -> 1.427,
    // 4096 / 6144 / 8192 unchanged; 512: 6144 +2 %, no limit: 8192 +3 %.
    PanelMode panel_mode(int O) const {
        if (!(panel_la && panel_var == 5)) return PANEL_PLAIN;
        return panel_fuse && first_update_tiles(O) <= panel_fuse_tiles ? PANEL_FUSED : PANEL_PIVOT_BESIDE;
    }
};

inline FitPlan plan_fit(int N, int Np, const Tuning &tu) {
    const int NB = PLAN_NB;
    FitPlan p;
    p.N = N;
    p.Np = Np;
    // ---- blocked Cholesky, two levels ----
    // Panels of NB = 64 columns (LDS factorisation + MFMA panel solve) are grouped into outer
    // blocks of OB = 512: inside an outer block a panel only updates the remaining columns of
    // that block (narrow, K = 64); the trailing matrix gets ONE rank-OB update per outer block
    // on the direct-to-LDS NT kernel (OB/16 k-tiles per tile instead of OB/64 launches of 4).
    // outer block (multiple of 256).  With the inverse behind the chain: 256 wins from Np = 1024 to
    // 3072 (1.06 vs 1.10 ms at N = 2048), 512 at N = 4096 (2.53 vs 2.59) and beyond.
    const int OB_env = tu.ob;
    // (round 3, with the fused panel launches: 512 is now equal or better from Np = 1536 on -- 2560: 1.293 vs 1.334 ms,
    // 3072: 1.617 vs 1.713 -- and 256 only wins where 512 leaves a half-empty last block: Np = 1280 0.618 vs 0.667)
    // (round 4, after the f64 kernels got faster: 1024 from Np = 6144 on -- 6144: 4.66 -> 4.48 ms, 8192: 8.87 -> 8.62 --
    // half as many trailing updates and event hops; still 512 at 4096: 2.20 vs 2.26)
    // (round 5, late: up to Np = 1024 ONE outer block -- no trailing update, the inverse level by level behind the last
    // panel.  With the one-launch panels the in-block updates cost no more than the rank-256 ones did, and the chain
    // loses its hand-overs to the background stream: fit 0.455 -> 0.417 / 0.452 -> 0.439 ms at N = 900 / 1000, an
    // evaluation of the hyper-parameter objective at N = 1000 0.562 -> 0.544 ms on the caller's handle and, on the
    // pooled workers whose inverse runs in line, 0.73 -> 0.55 alone, 0.88 -> 0.63 three side by side; Np = 768 equal)
    int OB = OB_env ? OB_env : (Np <= 1024 ? Np : (Np <= 1280 ? 256 : (Np >= 6144 ? 1024 : 512)));
    // The last, partial outer block builds its own inverse by merging halves (inverse_block): its length has to
    // be a power of two.  Np is a multiple of 256, so 256 and 512 always leave 0 or 256; 1024 can leave 768 (Np = 6912,
    // 7936, 8960: `invalid configuration argument` from a merge of zero pairs before this check) -> 512 there.
    if (const int tail = Np % OB; (tail & (tail - 1)) != 0) OB = 512;
    p.OB = OB;
    p.Nr = ((N + NB - 1) / NB) * NB;
    const int bginv_on = tu.bginv;
    // up to Np = 9216: beyond, the inverse's products want the 128-tile direct-to-LDS kernel and the whole
    // chip (N = 10000: 17.7 vs 17.2 ms, 16384: 63.0 vs 57.5, 20000: 114 vs 101 for the level-by-level path)
    const int bginv_max = tu.bginv_max;
    p.bginv = bginv_on && Np > OB && Np <= bginv_max;
    p.nblk = (Np + OB - 1) / OB;
    p.panel_var = tu.panel;
    p.panel_la = tu.panel_la;
    p.panel_fuse = tu.panel_fuse;
    p.panel_fuse_tiles = tu.panel_fuse_tiles;
    p.inner_generic = tu.inner_generic;
    p.level64_fused = tu.level64_fused;
    p.merge64 = tu.merge64;
    p.trail64 = tu.trail64;
    p.pre_tiles = tu.pre_tiles;
    p.stamp_path = tu.stamp_file.empty() ? nullptr : tu.stamp_file.c_str();
    return p;
}

}  // namespace tgp
