// tgp_internal.hpp -- state shared by the C-ABI layer and the kernel launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/turbogp.h"
#include "dev_mem.hpp"
#include "doorbell.hpp"
#include "lds_opt_in.hpp"
#include "mes_math.hpp"
#include "tuning.hpp"

namespace tgp {


constexpr int NB = 64;          // Cholesky / inverse block
constexpr int NPAD = 256;       // N is padded to a multiple of this (identity padding)
constexpr int SW_BM = 128;      // sweep tile: rows of Linv
constexpr int SW_BN = 128;      // sweep tile: candidates
constexpr int KS_JS = 8;        // most training-point splits of the cross-kernel grid (rows of mupart)
constexpr int FIN_BLOCK = 256;  // finalize block = candidates per arg-max partial
constexpr int CONTRACT_MIN_WGS = 512;   // a gathered set's contraction takes the widest candidate tile that still gives this many workgroups (two per CU)
constexpr int GATHER_KS_MIN_WGS = 256;   // ... and its cross-kernel splits the training points until its grid has one workgroup per CU (it writes no mupart row: KS_JS does not bind it)
constexpr int SCREEN_MIN_WGS = 1024;    // ... and the screen in front of it (prune_screen.hpp; 128 candidates per workgroup, two workgroups per CU)
constexpr int BOUND_MIN_WGS = 2048;     // the bound pass splits the training points only as far as its grid needs to reach this many workgroups

// THE dispatch on the covariance kind: f(std::integral_constant<int, KIND>{}) for the handle's kind, anything that is not
// one of the first three being Matern-5/2.  A launcher picks its kernel's instance with it and launches that once:
//     auto k = by_kind(c.kernel, [](auto K) { return small_fit_kernel<K()>; });
template <class F>
inline auto by_kind(int kernel, F &&f) {
    switch (kernel) {
        case TGP_RBF: return f(std::integral_constant<int, TGP_RBF>{});
        case TGP_MATERN12: return f(std::integral_constant<int, TGP_MATERN12>{});
        case TGP_MATERN32: return f(std::integral_constant<int, TGP_MATERN32>{});
        default: return f(std::integral_constant<int, TGP_MATERN52>{});
    }
}

struct ProfSeg { int a, b, kind; double flops; };   // pooled events a -> b bracket one launch; kind: 0 trmm, 1 kstar, 2 the pruned sweep's screen (counted apart: screen_ms); flops: the contraction's algorithmic flops of that launch (a launch a fit took row tiles of has fewer)

// The front of the resident batch's sweep, started INSIDE a fit (tgp_set_overlap; sweep_kernels.hip presweep_*)
struct PreSweep {
    int mode = 0;             // 0 off, 1 = candidate scaling + launch pair 0's cross-kernel, 2 = + the contraction's early row tiles
    int issue = 0;            // set by tgp_fit around launch_fit: the mode to issue for THIS fit (0: nothing)
    bool front = false;       // a fit issued the front for the batch recorded below
    int rows128 = 0;          // 128-row tiles [0, rows128) of launch pair 0 contracted inside that fit
    long gen = -1;            // fit_gen that fit leaves behind when it succeeds
    const double *cand = nullptr;
    int64_t M = 0, Mpad = 0, launch_rows = 0, chunk = 0;   // the batch and workspace geometry it was issued for
    bool pending = false;     // work on the device's third stream the main stream has not been told to wait for
    Ev ev;                    // third stream: end of the front
    Ev ev_in;                 // main stream: Xs / length scales staged
};

// A handle OWNS its Dev / Pin / Ev members (dev_mem.hpp: freed with it); raw pointers and streams are borrowed unless
// their comment says otherwise.  The fit's memory is released as a whole by `static_cast<FitMem &>(c) = FitMem{}`.
struct FitMem {
    Dev<double> d_t1, d_t2;        // (Np,) scratch vectors of the row append
    Dev<double> d_Xs;              // (Np, Dp) X / ls, rows >= N and columns >= D zero
    Dev<double> d_ls;              // (D,)
    Dev<double> d_K;               // (Np, Np) K, then L in the lower triangle
    Dev<double> d_Linv;            // (Np, Np) L^-1, zeros above the diagonal
    Dev<double> d_W;               // (Np, Np) workspace of the triangular inverse (T^T above the block diagonal)
    Dev<double> d_U;               // (Np, Np) Linv^T (upper triangular), so every merge product is NT
    Dev<double> d_Dinv;            // (2, Np/NB, NB, NB): inverses of the diagonal blocks | the diagonal blocks of L while they wait to be written into K
    Dev<double> d_Apan;            // (2, Np/NB, NB, NB): the unsolved blocks of the current panel, two slots used in turn (fused_panel_kernel)
    Dev<double> d_yn;              // (Np,) normalised y
    Dev<double> d_z;               // (Np,) Linv * yn
    Dev<double> d_alpha;           // (Np,)
    Dev<double> d_apart;           // (Np/128, Np) shares of alpha = Linv^T z, one row per 128-row slice of Linv, then (Np/128,) sums of z^2
    Dev<float> d_Xs32;             // f32 copies for the f32 sweep
    Dev<float> d_Linv32;
    Dev<unsigned short> d_Linv16;  // TGP_F32X3: Linv32 as three bf16 planes (3, Np, Np), cut before the first sweep after a fit
    long linv16_gen = -1;          // which fit (fit_gen) the planes belong to
    Dev<unsigned> d_x2scal;        // TGP_F32H2: [bits of max|Linv32|, bits of 1 / (s_a s_b)]
    int64_t cap_Np = 0, cap_D = 0; // the geometry the set above was allocated for
    bool cap_full = false;         // the buffers include what a FIT needs (K, the inverse's workspaces), not only what a sweep needs
    int64_t linv_ld = 0;           // d_Linv is zero from row / column linv_extent on for this leading dimension (0: unknown -> clear everything)
    // LML-gradient workspace (allocated on first tgp_fit_grad)
    Dev<double> d_gpart;           // (tiles, 3 + Dp) partial sums: [S_c, S_iso, S_diag, gd[0..Dp)] per 64 x 64 tile
    Dev<double> d_gout;            // [S_c, S_iso, S_diag, gd[Dp]]
    int64_t g_cap_Np = 0, g_cap_Dp = 0;   // the geometry those two were allocated for
    // input-gradient workspace (allocated on first tgp_fit_input_grad / tgp_fit_warp_grad; warp_kernels.hip)
    Dev<double> d_xgpart;          // (tiles of 64 rows, N, Dp) the column slices' shares of d LML / d X, each entry written once
    Dev<double> d_xgout;           // (N, D) d LML / d X, raw units of the fitted inputs
    // leave-one-out workspaces (allocated on first tgp_loo / tgp_fit_loo_grad)
    Dev<double> d_loov;            // the per-point vectors, the kappa kernel's partials and [L_LOO, bad count] (loo_vec_doubles + 2)
    Dev<double> d_looA;            // (Np, Np) A = K^-1 diag(sqrt(w)) of the LOO gradient
    int64_t loov_cap_Np = 0, looA_cap_Np = 0;
    Dev<double> d_qws;             // small-batch query workspace (tgp_acq_grad)
    Dev<double> d_rf;              // on-device optimiser state (tgp_acq_refine)
    Dev<unsigned long long> d_stamp;   // TGP_STAMP_FILE (debug): in-kernel time stamps of the panel chain
};

struct WsMem {                     // the sweeps' and the acquisition entries' workspaces: grow-only, each on its own
    Dev<void> d_Cs;                // (Mpad, Dp) scaled candidates, compute dtype
    Dev<void> d_Ks[2];             // (chunk, Np) cross-kernel slab, two slots
    Dev<double> d_part;            // (Np/SW_BM, Mpad) partial ||v||^2
    Dev<double> d_mupart;          // (KS_JS, Mpad) partial K*.alpha
    int64_t ws_Mpad = 0;           // leading dimension of Cs / part / mupart for this sweep
    Dev<char> d_prune;             // the pruned sweep's workspace (sweep_pruned.hpp, prune_workspace)
    Dev<double> d_topv;            // top-k workspace (tgp_sweep_topk)
    Dev<long long> d_topi;
    Dev<double> d_batch;           // tgp_predict_batch: per-model workspaces, outputs, counters
    Dev<double> d_bt;              // tgp_sweep_batch: the small state and the conditioned points' vectors
    Dev<double> d_btm;             // ... its per-candidate arrays (scaled candidates, pass partials, G, mean, variance)
    Dev<long long> d_bti;          // ... its indices, counters and the selection mask
    Dev<double> d_ts;              // tgp_ts_draw: the draw (omega, b, W, eps, V) and its workspace
    Dev<double> d_tsm;             // tgp_ts_sweep / tgp_ts_eval: per-call arrays (scaled candidates, f, partials, points)
    int64_t ts_S = 0, ts_F = 0;    // the resident draw's shape ...
    long ts_gen = -1;              // ... and the fit_gen it belongs to (-1: none)
    Dev<double> d_cov;             // tgp_predict_cov / tgp_sample_joint: the joint posterior's workspace (cov_kernels.hip), kept between calls
    Dev<double> d_mes;             // tgp_mes_set_maxima / tgp_mes_draw: MES_MAXS doubles, the first mes_S are the maxima
    int mes_S = 0;
    long mes_gen = -1;             // the fit_gen the maxima belong to (-1: none)
    Dev<double> d_int_a, d_int_mu, d_int_m2;   // tgp_sweep_integrated: (M,) sums over the samples of acq, mu, sigma^2 + mu^2
    Dev<double> d_kgp;             // tgp_kg_set_points: the stored points (kg_kernels.hip, KgPoints) and the workspace they were built in
    int kg_A = 0;
    long kg_gen = -1;              // the fit_gen the points belong to (-1: none)
    Dev<double> d_kgw;             // tgp_sweep_kg: a chunk's scaled candidates, cross-kernel slab and cross-covariance (KgChunk)
    Dev<double> d_wt_logw, d_wt_val;   // tgp_sweep_weighted: (M,) summed log weight and weighted value
    Dev<double> d_wt_smu, d_wt_ssg;    // ... and the sides' (K, M) mu / sigma rows, when asked for
    Dev<double> d_wt_q;            // tgp_weighted_grad: [Xq (m D) | val (m) | grad (m D) | mu, sigma ((K + 1) m each)] on the objective's handle
    std::vector<Ev> ev_wt;         // ... and, per side on another stream, "its sweep / its query sums are out" (no timing)
    Ev ev_wt_in;                   // tgp_weighted_grad: the query points are on the device (what a side's private stream waits for)
    // tgp_ehvi_set_front: the front of objective 1's handle -- kept until the next tgp_ehvi_set_front (no fit touches it)
    int ehvi_P = -1;               // points of the front (-1: none set)
    double ehvi_sf[2] = {1.0, 1.0};
    std::vector<double> ehvi_a, ehvi_c;   // host copy: the P + 1 breakpoints and levels, oriented coordinates
    Dev<double> d_ehvi_front;      // [a | c], TGP_EHVI_MAX_FRONT + 1 doubles each
    Dev<double> d_ehvi_val;        // tgp_sweep_ehvi: (M,) values
    Dev<double> d_ehvi_q;          // tgp_ehvi_grad: [Xq (m D) | val (m) | coef (4 m) | grad (m D) | mu, sigma (2 m each)]
    Ev ev_ehvi, ev_ehvi_in;        // g's sweep / sums are out; the query points are on the device (no timing)
    std::vector<Ev> ev_kg;         // brackets of the last tgp_sweep_kg's own kernels, a pair per chunk (the copies between them are not timed)
    double last_kg_ms = 0.0;
};

struct OutMem {                    // the sweep's optional (M,) outputs: created lazily at ONE size, released together
    Dev<double> d_mu, d_sigma, d_acq;
    int64_t out_cap = 0;           // candidates each of them holds once it exists
};

struct Context : FitMem, WsMem, OutMem {
    int device = 0;
    int dtype = TGP_F64;
    hipStream_t stream = nullptr;    // everything runs in order on this stream (the device's shared main stream: not owned) ...
    hipStream_t stream_own = nullptr; // tgp_set_private_stream: this handle's own main stream (owned), else null
    hipStream_t bg_lease = nullptr;   // the background stream this fit of a private-stream handle holds on loan (private_fit_begin), else null
    hipStream_t stream_bg = nullptr; // ... except the inverse factor's GEMMs behind the panel chain (the device's shared background stream: not owned)
    hipStream_t stream_pre = nullptr; // ... and the front of the next sweep inside a fit (the device's shared third stream: not owned)
    PreSweep pre;
    std::vector<Ev> ev_la;           // the events that order the two (no timing)
    Ev ev0, ev1;                     // brackets of the last fit / sweep (last_*_ms)
    Ev evg[4];                       // stages of the last LML gradient
    double last_grad_ms[3] = {0.0, 0.0, 0.0};  // K^-1 = U U^T | pairwise weights + traces | ARD products
    std::string err;

    // ---- fitted state (device, f64) ----
    bool fitted = false;
    int64_t N = 0, D = 0, Np = 0;
    int64_t Dp = 0;                // D rounded up to a multiple of 4: row stride of Xs / Cs
    int kernel = TGP_RBF;
    double constant = 1.0, noise = 0.0, jitter = 0.0;
    double y_mean = 0.0, y_std = 1.0, lml = 0.0;
    std::vector<double> ls;        // D entries (broadcast when isotropic)
    std::vector<double> h_X;       // host copy of the training inputs (N, D): prefix test of tgp_fit_append
    std::vector<double> h_y;       // host copy of the raw targets (N,): tgp_export_state
    int normalize_y = 1;
    double sumlog = 0.0;           // sum(log(diag L)) of the resident factor
    Dev<double> d_scal;            // [0] sum log diag, [1] yn . alpha
    Dev<int> d_flag;               // first failing pivot + 1, or 0
    bool grad_staged = false;      // the last tgp_fit_grad left its sums in the pinned result buffer (+8), not in d_gout
    bool grad_timed = true;        // ... and recorded the events its stage times are read from (false: a polled call)
    double last_loo_ms = 0.0;      // device time of the last tgp_loo's kernels
    double last_cov_ms = 0.0;      // device time of the last joint-posterior call's kernels (the H2D / D2H copies not included)
    long fit_gen = 0;              // counts the fits, appends and imports: what a draw, the maxima and the planes of Linv belong to
    float linv16_sb = 0.f;         // TGP_F32H2: the cross-kernel scale the stored 1 / (s_a s_b) was formed with
    bool imported = false;         // the resident factor was received (tgp_import_factor_dev), not computed: no training set on the host
    int64_t import_rows = 0;       // rows of Linv received so far of a factor that is arriving block by block
    int64_t fit_gen_src = -1;      // ... and the giver's fit generation they belong to

    // ---- small-problem path (N <= 128): pinned, device-mapped staging ----
    bool small = false;            // the resident fit came from small_fit_kernel
    int64_t linv_extent = 0;       // rows / columns of d_Linv from this on are zero (for the leading dimension linv_ld)
    // each the host pointer, .dev() the device's view of the same block
    Pin<double> h_pin_in{hipHostMallocMapped | hipHostMallocCoherent};    // the input staging
    Pin<double> h_pin_out{hipHostMallocMapped | hipHostMallocCoherent};   // the result staging
    Pin<double> h_pin_cand{hipHostMallocMapped};                          // candidates handed over by tgp_evaluate on that path
    Pin<uint32_t> h_mt_words{hipHostMallocDefault, false};               // tgp_set_candidates_mt19937: two pinned column buffers of the stream's words (unmapped)
    Ev ev_mt[2];                                                          // ... and "this buffer's copy has left" (no timing)
    // ---- polled completion (doorbell.hpp): coherent device-mapped [sequence number, start tick, end tick, -] ----
    Pin<unsigned long long> h_bell{hipHostMallocMapped | hipHostMallocCoherent};
    unsigned long long bell_seq = 0;   // number of the last polled call issued on this handle
    Dev<unsigned> d_ticket;            // ticket counters of the polled multi-workgroup kernels (zero between launches)
    Dev<double> d_sfg;                 // small fit + gradient in one launch: the workspaces of the two workgroups that only contribute a block pair

    // ---- candidates ----
    const double *d_cand = nullptr;   // (M, D) f64 row-major: borrowed -- the caller's, or a view of d_cand_owned / h_pin_cand
    Dev<double> d_cand_owned;
    int64_t M = 0;
    // ---- the warped batch (tgp_warp_candidates): in force while d_cand == d_wcand and M == warp_M, i.e. until any entry
    //      makes another batch resident; the raw rows are the library's own copy, so whoever owns the rows they came from
    //      may overwrite or free them ----
    Dev<double> d_wcand;              // (warp_M, D) the warped rows: the resident batch
    Dev<double> d_wraw;               // (warp_M, D) the rows as they were before the warp (tgp_warp_read_raw; the source of a re-warp)
    Dev<double> d_wpar;               // [lo | hi | a | b] (4 D) of the last tgp_warp_candidates
    int64_t warp_M = 0, warp_D = 0;
    Dev<double> d_wpts;               // tgp_warp_points / tgp_fit_warp_grad: [lo | hi | a | b | points | w | dw/du | dw/da | dw/db | 2 D sums]

    // ---- sweep workspace ----
    int64_t chunk = 0;            // candidates per GROUP of a trmm launch (the slab the caches re-serve: about 256 MiB)
    int64_t launch_rows = 0;      // candidates per trmm launch = rows of the slab (a multiple of chunk; the whole batch when it fits)
    int prune_state = -1;         // the last sweep: -1 not eligible, -2 gated off, 0 pruned, 1 fell back to every candidate
    int64_t prune_lbset = 0, prune_surv = 0;   // ... candidates in its lb set / survivors
    int64_t prune_screen = -1;    // ... survivors of its screen (prune_screen.hpp); -1: the screen did not apply (f64, Matern, TGP_PRUNE_SCREEN=0, not pruned)
    int prune_arith = 0;          // ... and the screen's arithmetic: 0 no screen, 1 f32 (prune_screen.hpp), 2 fp16 planes (prune_screen_h2.hpp)
    int prune_spec = 0;           // ... and its speculative round (sweep_pruned.hpp): 0 not tried, 1 hit, 2 miss
    int64_t prune_hist = -1;      // the handle's PREVIOUS pruned sweep: the survivors of its first filter when it ended in state 0, else -1.
                                  // Survives a refit; only ever chooses the schedule (TGP_PRUNE_SPEC=1), never a result
    double screen_ms = 0.0;       // profiling: the screen's launches since tgp_profile_reset
    Dev<double> d_bval;           // per finalize block arg-max value
    Dev<long long> d_bidx;        // per finalize block arg-max index
    double *d_winner = nullptr;   // borrowed (D + 2) record [value, global index, row] or null (tgp_set_winner_out)
    int64_t winner_offset = 0;    // global index of candidate 0 of the resident batch
    Ev ev_winner;                 // recorded on the stream behind the kernel that packs the record (tgp_winner_wait)
    bool winner_recorded = false;
    Dev<double> d_best;           // [0] value
    Dev<long long> d_besti;       // [0] index, [1] clamp count, [2] ticket counter of mid_sweep_kernel (zero between launches), [3] spare

    // ---- profiling ----
    bool profiling = false;
    std::vector<Ev> ev_pool;           // timing events, created once and reused (no create / destroy in the sweep loop)
    size_t ev_used = 0;
    std::vector<ProfSeg> segs;
    int64_t trmm_launches = 0, kstar_launches = 0;
    double trmm_ms = 0.0, kstar_ms = 0.0;
    double trmm_flops = 0.0;      // algorithmic flops (rows^2 per candidate over the rows a launch covered) of the timed contraction launches
    double last_fit_ms = 0.0, last_sweep_ms = 0.0;
    int last_sweep_f64 = -1;      // 1: the last sweep ran in f64 whatever the dtype (one-workgroup / one-launch kernels), 0: in the handle's arithmetic, -1: none yet
};

// launchers (fit_kernels.hip / sweep_kernels.hip); return hipSuccess or the first error
hipStream_t private_fit_begin(int device, bool may_borrow);   // fit_streams.hpp: a fit of a private-stream handle starts; the device's background stream if it gets it on loan, else null
void private_fit_end(int device, bool held);
hipError_t launch_fit(Context &c, const double *staged_in, double *res_host, bool zero_linv = true, unsigned long long *start_stamp = nullptr);   // start_stamp: device view of a mapped word the first kernel leaves its wall_clock64() in (a polled call)
hipError_t launch_ring(Context &c, const Bell &bell);   // a one-wave kernel behind everything queued on c.stream: rings the doorbell   // staged_in: device-mapped [Xs | yn | ls] or null (already in HBM); res_host: device-mapped [sum log, yn.alpha, flag] or null; zero_linv: false when Linv is known to be zero above the diagonal and from row Nr on
// the device's shared main / background stream (fit_streams.hpp); either pointer may be null
hipError_t device_streams(int device, hipStream_t *main, hipStream_t *bg, hipStream_t *pre = nullptr);   // main != null takes a reference
void device_streams_release(int device);
void device_stream_status(int device, int *bg_ok, int *pre_ok);   // 1 runs beside the main stream, 0 serialised (one hardware queue), -1 not probed
hipError_t launch_lml_grad(Context &c, bool ard, double *gout, bool timed = true);   // timed = false: no event records between its stages
// the two halves of launch_lml_grad, shared with the leave-one-out gradient (grad_kernels.hip): K^-1 = U U^T over the lower
// tiles into d_W; the pairwise pass over d_W (loo_b == null: K^-1 and the LML's pair weight; else B and b, the LOO weight)
hipError_t launch_kinv_product(Context &c);
hipError_t launch_pair_sums(Context &c, bool ard, const double *loo_b, double *gout, bool timed);
// learned input warping (warp_kernels.hip).  launch_input_grad: behind launch_lml_grad (K^-1 in d_W, alpha, Xs resident):
// dX (N, D) = d LML / d X through partial (tiles of 64 rows, N, Dp).  launch_warp: `total` = m D elements of src through the
// Kumaraswamy warp with par = [lo | hi | a | b] (4 D); raw (a copy of src), du, da, db nullable.  launch_warp_chain: out
// (2 D) = [d LML / d log a | d LML / d log b] from dWx = d LML / d w(X) and the warp's derivatives, all (N, D)
hipError_t launch_input_grad(Context &c, double *partial, double *dX);
hipError_t launch_warp(Context &c, const double *src, int64_t total, int D, const double *par, double *raw, double *wout,
                       double *du, double *da, double *db);
hipError_t launch_warp_chain(Context &c, const double *dWx, const double *dwda, const double *dwdb, const double *par, double *out);
// leave-one-out cross-validation (loo_kernels.hip).  c.d_loov: [kappa | resid | sigma | lpd | p | sqrt(w) | b] (Np each), then
// the (Np / LOO_ROWS, Np) partial column sums and the (2, Np / 256) sums of the points' workgroups; scal (device or
// device-mapped): [L_LOO, count of kappa_i <= 0 or not finite]
constexpr int LOO_ROWS = 256;                       // rows of Linv per chunk of the kappa kernel
constexpr double LOO_LOG_2PI = 1.8378770664093453;  // log(2 pi)
inline size_t loo_vec_doubles(int64_t Np) { return (size_t)(7 + Np / LOO_ROWS) * (size_t)Np + 2 * (size_t)(Np / 256); }
hipError_t launch_loo_points(Context &c, double *scal);
// behind a blocked fit: the gradient's sums into gout as launch_lml_grad leaves them; needs c.d_loov, c.d_looA (Np, Np)
hipError_t launch_loo_grad(Context &c, bool ard, double *gout, double *scal, bool timed = true);
hipError_t launch_f64_to_f32(Context &c, const double *in, float *out, long n);   // out[i] = (float)in[i] on c.stream (fit_kernels.hip: the cast every fit path uses)
// N <= 128, Dp <= 64, behind launch_small_fit: one workgroup per block pair (1 or 3), workgroup g leaving
// [S_c, S_iso, S_diag, gd[0..Dp)] for its pair at out + g * SMALL_GRAD_OUT_STRIDE; the caller adds them
constexpr int SMALL_GRAD_OUT_STRIDE = 72;
hipError_t launch_small_grad(Context &c, bool ard, double *out);
hipError_t launch_query(Context &c, const double *d_Xq, int m, int acq, double sf, double incumbent,
                        double param, double *d_ws, double *d_val, double *d_grad,   // d_val == nullptr: the sums only
                        const Bell &bell = Bell{nullptr, 0, nullptr});   // bell.word != null: value + gradient formed by the reduction's last workgroup, which rings it (d_Xq / d_val / d_grad may then be device-mapped host memory)
// c.d_qws as tgp_acq_grad and tgp_acq_refine use it for m points, laid out in ONE place (query_kernels.hip):
// [Xq (m D) | val (m) | grad (m D) | up to 3 doubles of padding | launch_query's workspace]
struct QueryWs {
    size_t bytes;                  // what c.d_qws has to hold
    double *Xq, *val, *grad;       // the entry's points and results
    double *ws;                    // launch_query's d_ws: 32-byte aligned for every m (its kernels load 2 and 4 doubles at once)
    double *red;                   // ... and in it, per query point, [k.alpha, v.v, gm (D), gv (D)]
};
QueryWs query_ws(const Context &c, int m);   // the pointers are into c.d_qws as it is: take them once it holds `bytes`
hipError_t launch_gen_candidates(Context &c, double *dst, int64_t M, unsigned long long seed,
                                 unsigned long long first_candidate, const double *d_lo,
                                 const double *d_hi);
hipError_t launch_gen_lhs(Context &c, double *dst, int64_t M, int64_t D, unsigned long long seed,
                          unsigned long long first_sample, unsigned long long n_total,
                          const double *d_lo, const double *d_hi);
// d_words: per column the 2 M tempered MT19937 outputs of its M draws; dst (M, D) = lo + range * u, NumPy's arithmetic (sweep_kernels.hip)
hipError_t launch_mt19937_columns(Context &c, const void *d_words, double *dst, int64_t M, const double *d_lo,
                                  const double *d_range);
hipError_t launch_fit_append(Context &c, int n_old);
// done_host != null (a polled call): the final pass also leaves [k values | k indices as doubles, -1 = none | clamp count]
// in that device-mapped host record, hands the sweep's counters back at zero and rings the bell
hipError_t launch_topk(Context &c, const double *d_vals, long M, int k, double *ws_v, long long *ws_i,
                       long *final_off, double *done_host = nullptr, const Bell &bell = Bell{nullptr, 0, nullptr});
hipError_t launch_refine_clip(Context &c, double *d_xt, const double *d_lo, const double *d_hi, int R);
hipError_t launch_refine_step(Context &c, double *d_state, double *d_xt, const double *d_val,
                              const double *d_grad, const double *d_lo, const double *d_hi, int R,
                              int it, double pgtol, double ftol, int *d_active,   // d_active: 2 ints, used in turn
                              const double *d_red = nullptr, int acq = 0, double sf = 1.0, double incumbent = 0.0,
                              double param = 0.0);   // d_red (D <= 64 only): value + gradient taken from launch_query's sums here
hipError_t launch_refine_collect(Context &c, const double *d_state, int R, double *d_x, double *d_v, double *d_info);
long refine_state_stride(int D);
long refine_hist_doubles(int D, int R);   // behind the R states in the same buffer
// N <= 128, D <= 64: the whole stage in one launch, one workgroup per restart (refine_kernels.hip);
// d_info: (3 R) status, accepted steps, evaluations.  Pointers may be device-mapped host memory.
bool small_refine_fits(const Context &c);
hipError_t launch_small_refine(Context &c, const double *d_x0, const double *d_lo, const double *d_hi, int R,
                               int acq, double sf, double incumbent, double param, int max_iter,
                               double pgtol, double ftol, double *d_x, double *d_v, double *d_info);
// N <= 128, D <= 64 (small_refine_fits): tgp_acq_grad in one launch, one workgroup per point; the pointers may be
// device-mapped host memory; bell.word != null: the last workgroup rings it (refine_kernels.hip)
hipError_t launch_small_query(Context &c, const double *d_xq, int m, int acq, double sf, double incumbent, double param,
                              double *d_val, double *d_grad, const Bell &bell);
hipError_t launch_small_fit(Context &c, const Bell &bell);   // bell.word != null: the kernel rings it when the results are out (doorbell.hpp)
// N <= 128, Dp <= 64: fit + LML gradient in ONE launch (one workgroup per block pair, each running the fit itself);
// gout_host: device-mapped host memory for the pairs' sums (as launch_small_grad leaves them); needs c.d_sfg
hipError_t launch_small_fit_grad(Context &c, bool ard, double *gout_host, const Bell &bell);
size_t small_fit_grad_ws_bytes();
// N <= 128: the hyper-parameter fit in one launch, one workgroup per start (small_kernels.hip).  theta = log(constant,
// length scale(s), noise); d_ws: S * small_hyper_workspace_doubles() doubles; d_info (3 S): status, steps, evaluations
long small_hyper_workspace_doubles(int N, int D, int Dp);
hipError_t launch_small_hyper(Context &c, int kernel, const double *d_X, const double *d_yn, const double *d_theta0,
                              const double *d_blo, const double *d_bhi, int S, int N, int D, int Dp, int n_ls,
                              int max_iter, double jitter, double *d_ws, double *d_theta, double *d_f, double *d_info,
                              bool one_wg_per_start = false);
size_t small_fit_args_bytes();
size_t small_sweep_args_bytes();
int64_t small_batch_ws_doubles(int64_t D, int64_t Dp);
// ... and for batches with models of 128 < N <= 256 (one-workgroup fit with the tiles in the model's workspace, one-launch sweep)
int64_t mid_batch_ws_doubles(int64_t D, int64_t Dp);
void fill_mid_batch_args(void *fit_args, void *sweep_args, int64_t t, const double *in_dev, double *ws_dev,
                         double *res_dev, long long *counters_dev, const double *cand_dev, double *mu_dev,
                         double *sigma_dev, int64_t N, int64_t D, int64_t Dp, int64_t M, double constant,
                         double noise, double jitter, double y_mean, double y_std);
hipError_t launch_mid_batch(Context &c, int kernel, const void *fit_args_dev, const void *sweep_args_dev, int64_t T, int64_t M);
void fill_small_batch_args(void *fit_args, void *sweep_args, int64_t t, const double *in_dev, double *ws_dev,
                           double *res_dev, long long *counters_dev, const double *cand_dev, double *mu_dev,
                           double *sigma_dev, int64_t N, int64_t D, int64_t Dp, int64_t M, double constant,
                           double noise, double jitter, double y_mean, double y_std);
hipError_t launch_small_batch(Context &c, int kernel, const void *fit_args_dev, const void *sweep_args_dev,
                              int64_t T, int64_t M, bool fit, bool sweep);
// One sweep of the resident candidates with the resident model: what the C-ABI entries ask of run_sweep (tgp_api.hip)
// and the launchers below read.  Nothing of it travels through the handle.
struct SweepCall {
    int acq = TGP_ACQ_NONE;
    double sf = 1.0, incumbent = 0.0, param = 0.0;
    double *mu = nullptr, *sigma = nullptr, *acqv = nullptr;   // (M,) optional outputs: device memory, or device-mapped host memory behind the one-workgroup / one-launch kernels
    double *res = nullptr;          // device-mapped [best value, best index, clamp count] the sweep's last kernel fills, handing the counters back at zero (no D2H copy, no memset behind it), or null
    double *winner = nullptr;       // the (D + 2) record [value, global index, row] to pack (tgp_set_winner_out), or null
    Bell bell{nullptr, 0, nullptr}; // word != null: the one-workgroup / one-launch family's last kernel rings when the record is out (the general sweep never rings)
    MesArgs mes{nullptr, 0, 0.0};   // TGP_ACQ_MES: the handle's maxima (run_sweep fills it in)
    bool may_use_front = false;     // the caller saw c.pre.front before pre_join discarded it: the front a fit issued may serve this sweep
};
// which kernel family sweeps a batch of M candidates with the resident model
enum class SweepPath {
    OneWorkgroup,   // N <= 128 off small_fit_kernel: small_sweep_kernel + the arg-max's final kernel (f64)
    OneLaunch,      // 128 < N <= 512: mid_sweep_kernel, everything in one launch (f64)
    General         // the cross-kernel / contraction / finalize schedule in the handle's arithmetic (sweep_kernels.hip)
};
// mid_sweep_cpw: candidates per workgroup of the one-launch sweep (64 up to N = 256, 32 up to N = 512 and moderate
// batches), 0 = not that family
int mid_sweep_cpw(const Context &c, int64_t M);   // M: the batch about to be swept
inline SweepPath sweep_path(const Context &c, int64_t M) {
    if (c.small && c.N <= 2 * NB) return SweepPath::OneWorkgroup;
    return mid_sweep_cpw(c, M) != 0 ? SweepPath::OneLaunch : SweepPath::General;
}
// the three families' launchers, on c.stream over c.d_cand / c.M.  One-workgroup: launch_small_sweep, then
// launch_argmax_final (record, winner, bell).  One-launch: launch_mid_sweep does all of it.  General: launch_sweep;
// front_usable: the front a fit issued belongs to the resident fit, batch and workspace geometry
hipError_t launch_small_sweep(Context &c, const SweepCall &s);
hipError_t launch_argmax_final(Context &c, const SweepCall &s);
hipError_t launch_mid_sweep(Context &c, const SweepCall &s);
hipError_t launch_sweep(Context &c, const SweepCall &s, bool front_usable);
// inside launch_fit, on the third stream (c.pre.mode > 0, candidates resident, workspace ensured): the candidate scaling and
// launch pair 0's cross-kernel (needs Xs, the length scales) / the contraction's 128-row tiles whose rows of Linv are
// final (rows < rows_final), at most budget128 of them in all
hipError_t presweep_front(Context &c, hipStream_t st);
hipError_t presweep_rows(Context &c, hipStream_t st, int rows_final, int budget128);

// Profiling marks on the sweep's stream: ONE event between consecutive launches (the end of one
// launch is the start of the next), so a chunk costs two records instead of four.  prof_mark
// returns the event's index or -1 (profiling off); prof_seg names the launch between two marks.
int prof_mark(Context &c, hipStream_t s);
void prof_seg(Context &c, int a, int b, int kind, double flops = 0.0);

// tgp_sweep_batch (batch_kernels.hip): greedy batch selection with Kriging Believer / Constant Liar, all on the device
constexpr int BT_MAXP = 64;        // P + q <= 64 conditioned points per call
struct BtSmall {                   // the small state of one call (device memory)
    double *R;                     // (64, 64) rows of the new block of the augmented factor
    double *e;                     // (64) e_j = (y~_j - mu~_{j-1}(z_j)) / R[j,j]
    double *fant;                  // (64) fantasies, raw units
    double *inc;                   // [0] incumbent after the fantasies so far
    double *sel_val;               // (64) acquisition at each selection
    long long *sel_idx;            // (64) candidate index of each selection
    int *flag;                     // first point whose pivot failed + 1, or 0
};
// one batch call's regions of d_bt / d_btm / d_bti, named once for both strategies (tgp_api.hip carves them)
struct BatchWs {
    int64_t Mpad, nblk;            // rows of the scaled candidates and of the pass partials; arg-max partials of the update
    int js;                        // training-point splits of the pass
    double *Zraw, *Zs, *Kz, *hw, *v, *w, *R, *selv;   // d_bt: the conditioned points' vectors and the small state ...
    double *fant, *inc;            // ... greedy: fant (64) right behind selv, inc [1]; Monte Carlo: fant (64, 64), inc (64)
    double *e, *eps;               // ... greedy only: e (64); Monte Carlo only: eps (64, 64)
    double *Cs, *part, *bmu, *bvar, *bval, *G, *acqd;  // d_btm (acqd: the Monte Carlo acq_out rows)
    long long *seli, *clampw, *flagw, *bidx;          // d_bti: clampw and flagw right behind seli (one copy back)
    unsigned char *mask;           // ... and the selection mask last
};
// launch_query's front for m points (rows of stride D in, Dp / Np out): uq = x / l, ks = k*(x), v = Linv ks, w = Linv^T v (query_kernels.hip)
hipError_t launch_query_front(Context &c, const double *d_xq, double *uq, double *ks, double *hw, double *v, double *w, int m = 1);
int bt_pass_splits(const Context &c, int64_t M);   // training-point splits of the pass = rows of its partials
hipError_t launch_bt_prep(Context &c, double *Cs, int64_t Mpad);
hipError_t launch_bt_init(Context &c, double *mu, double *var, unsigned char *mask);   // from c.d_mu / c.d_sigma of the first sweep
hipError_t launch_bt_point(Context &c, const double *rec, const BtSmall &s, int k, double *zraw, unsigned char *mask);
struct McSmall;
// launch_bt_condition: the front of point j and its small side (mc given: mc_small_kernel); launch_bt_step: the pass, the
// update and (acq != NONE) selection k
hipError_t launch_bt_condition(Context &c, const BatchWs &ws, const BtSmall &s, const McSmall *mc, int j, int kb,
                               double lie, double sf);
hipError_t launch_bt_step(Context &c, const BatchWs &ws, const BtSmall &s, int j, int store, int acq, double sf,
                          double param, double *mu_out, double *sigma_out, int k);
// tgp_sweep_batch_mc (batch_kernels.hip): the Monte Carlo strategy, S <= 64 simulations of every conditioned point
constexpr int MC_MAXS = 64;
struct McSmall {
    BtSmall b;                     // R, sel_val, sel_idx, flag as tgp_sweep_batch (e, fant, inc unused: null)
    double *eps;                   // (64, 64) POINT-major: eps[j * 64 + s], zero from S / J on
    double *fant;                  // (64, 64) point-major fantasies, raw units
    double *inc;                   // (64) per simulation: the incumbent after its fantasies so far
    int S;
};
// eps from the Philox stream (draw) or left as the caller copied it; inc[s] = incumbent
hipError_t launch_mc_init(Context &c, const McSmall &s, int J, bool draw, unsigned long long seed, double incumbent);
hipError_t launch_mc_step(Context &c, const BatchWs &ws, const McSmall &s, int j, int acq, double sf, double param,
                          double *acq_out, double *sigma_out, int k);

// Thompson sampling (ts_kernels.hip): S <= 64 sample paths of the fitted model, F random Fourier features
struct TsDraw {
    int64_t S, F;
    double *omega;                 // (F, Dp) in scaled coordinates, columns >= D zero
    double *b;                     // (F)
    double *W;                     // (ts_spad(S), F), rows >= S zero
    double *eps;                   // (S, N)
    double *V;                     // (ts_spad(S), Np): v_s = K^-1 (y~ - f_prior_s(X) - eps_s), zero from N on and from row S on
};
int ts_spad(int64_t S);            // rows of W / V: S rounded up to 16, 32 or 64
// z = Linv r, w = Linv^T z for m vectors (rows of stride Np, zero from N on) on the matrix-core products (query_kernels.hip)
hipError_t launch_linv_solve(Context &c, const double *r, double *z, double *w, int m);
// fill the draw; priorX (N, S), R and Z (S, Np) are its workspace
hipError_t launch_ts_draw(Context &c, const TsDraw &t, unsigned long long seed, double *priorX, double *R, double *Z);
// out[row * S + s] = o0 + o1 f_s(P[row]) for scaled points P (rows up to the 64-row tile's end readable, Dp stride);
// update = false: the prior alone
hipError_t launch_ts_pass(Context &c, const TsDraw &t, const double *P, int64_t rows, bool update, double *out, double o0,
                          double o1);
// per sample the (sf f, lowest index) arg-max over the resident candidates, from f (M, S); distinct: sample s skips the
// rows of samples < s.  bval / bidx: S * ceil(M / 256) partials; sel_x (S, D) the winners' rows
hipError_t launch_ts_select(Context &c, const TsDraw &t, const double *f, double sf, int distinct, unsigned char *mask,
                            double *bval, long long *bidx, long long *sel_idx, double *sel_val, double *sel_x);
// tgp_mes_draw: dst[s] = the better of src[s] and incumbent in the direction of sf (a NaN incumbent changes nothing)
hipError_t launch_mes_take(Context &c, const double *src, int S, double sf, double incumbent, double *dst);
size_t ts_eval_lds_bytes(const Context &c, int64_t S);

// The joint posterior over m <= 4096 query points (cov_kernels.hip): one workspace, offsets in doubles
struct CovWs {
    int64_t m, mpad, S, Spad, NV;  // mpad / Spad: m / S in whole 128-tiles; NV: N in whole 128-tiles, the columns of Vt
    int64_t o_cnt;                 // [0] (long long) negative entries of the diagonal, [1] (int) first failed pivot + 1
    int64_t o_Xq, o_Us, o_mu, o_dvec, o_Dinv, o_G;   // raw and scaled points, mu, the unfactored diagonal, a block's inverse, Sigma (mpad, mpad)
    int64_t o_Ks, o_Vt;            // (mpad, Np), (mpad, NV)
    int64_t o_Ein, o_E, o_Y;       // (S, m) normals as given; (Spad, mpad) padded normals and samples -- in Ks / Vt's place
};
int64_t cov_ws_doubles(const Context &c, int64_t m, int64_t S, CovWs *out);   // S = 0: the covariance alone
// Xq is in the workspace; leaves mu and G = y_std^2 Sigma mirrored (for_sample = false) or Sigma + nugget I with zeros
// above the diagonal and its diagonal in dvec (for_sample = true)
hipError_t launch_cov_posterior(Context &c, double *ws, const CovWs &w, int latent, double nugget, bool for_sample);
// behind launch_cov_posterior(for_sample = true): G = Lc in place, E = the normals (draw: Philox, else from o_Ein), Y = the samples
hipError_t launch_cov_sample(Context &c, double *ws, const CovWs &w, bool draw, unsigned long long seed);
hipError_t launch_ts_eval(Context &c, const TsDraw &t, const double *Xq, int m, double *fout, double *gout);

// tgp_sweep_integrated (integrate_kernels.hip): behind sample k's predict-only sweep into c.d_mu / c.d_sigma, add its
// acquisition and moments into c.d_int_* (k == 0 stores); behind the last one, the averages into s.mu / s.sigma / s.acqv
// (device memory, nullable), their arg-max, the record s.res and the winner record s.winner as a plain sweep leaves them
hipError_t launch_integrate_accumulate(Context &c, const SweepCall &s, int k);
hipError_t launch_integrate_final(Context &c, const SweepCall &s, int S);
// the same final kernel over ONE (M,) vector of values that is already the acquisition (tgp_sweep_kg: c.d_acq): its
// arg-max, the record s.res and the winner record s.winner; writes no (M,) output
hipError_t launch_argmax_of(Context &c, const SweepCall &s, const double *vals);

// tgp_sweep_weighted / tgp_weighted_grad (weight_kernels.hip), all on c.stream -- the OBJECTIVE's.
constexpr int WT_MAX_SIDES = 8;    // most side models of one call
// launch_weight_accumulate: behind side k's predict-only sweep into g.d_mu / g.d_sigma (the side's handle), logw (M,) on the
// objective's handle takes (k == 0) or adds log f_k; the side's rows go to side_mu / side_sigma (nullable) and its clamp
// count into c's counter.  launch_weight_value: behind the objective's predict-only sweep into c.d_mu / c.d_sigma, the
// unweighted acquisition into c.d_acq and the weighted value into val (K == 0: logw is written as 0)
hipError_t launch_weight_accumulate(Context &c, const Context &g, int k, int kind, double level, double *logw, double *side_mu,
                                    double *side_sigma);
hipError_t launch_weight_value(Context &c, const SweepCall &s, int K, double *logw, double *val);
// the K + 1 models' value-with-partials at m query points combined: mdl[0] the objective, mdl[1 + k] side k; red: where
// launch_query(d_val == nullptr) left that model's sums (QueryWs::red)
struct WtModel {
    const double *red, *ls; double kss, y_mean, y_std, level; int kind;
    const double *mu, *sigma;      // (m) the model's own predict-only sweep of the points where that sweep is f64 (the VALUES are then the
                                   // sweep's bits; the partials always come from the sums), else null
};
struct WtGrad {
    WtModel mdl[1 + WT_MAX_SIDES];
    int K, m, D, acq;
    double sf, incumbent, param;
    double *val, *grad;            // (m), (m, D) device memory
};
hipError_t launch_weight_grad(Context &c, const WtGrad &g);

// tgp_sweep_ehvi / tgp_ehvi_grad (ehvi_kernels.hip), all on c.stream -- objective 1's.  front: c.d_ehvi_front,
// [a_0 .. a_P | c_0 .. c_P] at a stride of TGP_EHVI_MAX_FRONT + 1, oriented coordinates.
// launch_ehvi_value: behind g's and c's predict-only sweeps into their d_mu / d_sigma, the value into val (M,); g's clamp
// count moves into c's counter
hipError_t launch_ehvi_value(Context &c, const Context &g, const double *front, int P, double sf1, double sf2, double *val);
// the two models' value-with-partials at m query points combined; the members as WtModel's
struct EhviModel {
    const double *red, *ls; double kss, y_mean, y_std;
    const double *mu, *sigma;
};
struct EhviGrad {
    EhviModel mdl[2];
    const double *front;
    int P, m, D;
    double sf[2];
    double *val, *coef, *grad;     // (m), (m, 4), (m, D) device memory
};
hipError_t launch_ehvi_grad(Context &c, const EhviGrad &g);

// the cov path's scaling, cross-kernel and mean for m rows Xq (m, D) on the device (cov_kernels.hip): Us (mpad, Dp),
// Ks (mpad, Np), mu (mpad) or null; mpad a multiple of 64; cnt: two counters the first kernel clears
hipError_t launch_cov_cross(Context &c, const double *Xq, int m, int mpad, double *Us, double *Ks, double *mu, long long *cnt);

// The knowledge gradient (kg_kernels.hip).  KgPoints: c.d_kgp for A discretisation points, offsets in doubles
struct KgPoints {
    int64_t A, Apad;               // Apad: A in whole 128-tiles
    int64_t o_cnt, o_Xa, o_Ua, o_mu, o_W;   // counters, raw (A, D) and scaled (Apad, Dp) points, mu(Xa) (Apad), W = K^-1 c k0(X, Xa) as (Apad, Np)
    int64_t o_Ka, o_Z;             // workspace: c k0(Xa, X) and Linv of it, (Apad, Np) each
};
int64_t kg_points_doubles(const Context &c, int64_t A, KgPoints *out);
hipError_t launch_kg_points(Context &c, double *ws, const KgPoints &p);   // Xa is in the workspace
// KgChunk: c.d_kgw for chunks of `rows` candidates (a multiple of 128)
struct KgChunk {
    int64_t rows, Apad;
    int64_t o_cnt, o_Us, o_Ks, o_C;   // counters, (rows, Dp), (rows, Np), (rows, Apad)
    int64_t o_mu;                  // (rows) the chunk's raw mean re-formed in f64 (handles whose sweep is not f64)
};
int64_t kg_chunk_doubles(const Context &c, int64_t rows, int64_t Apad, KgChunk *out);
// candidates [i0, i0 + m) of the resident batch: the raw latent cross-covariance into the chunk's C and the knowledge
// gradient into kg[i0 ..) from c.d_mu / c.d_sigma; remean: the mean of these rows is first re-formed in f64 from the
// chunk's cross-kernel (y_mean + y_std Ks alpha, the cov path's kernel) and replaces c.d_mu[i0 ..)
hipError_t launch_kg_chunk(Context &c, double *ws, const KgChunk &k, const double *pts, const KgPoints &p, int64_t i0, int m,
                           double sf, double *kg, bool remean);
// tgp_kg_grad: c.d_kgw for m <= 4096 query points -- the chunk's buffers (k: rows = m in whole 128-tiles) and behind them
// the query front's vectors, the envelope's record and the results
constexpr int KG_ENV_LD = 264;     // row stride of env_e / env_idx: the A + 1 <= 257 lines an envelope can hold
struct KgGradWs {
    KgChunk k;
    int64_t o_Xq, o_uq, o_ks, o_hw, o_v, o_w;   // (m, D), (m, Dp), then (m, Np) each: x, x / l, c k0, c h, Linv ks (then omega), K^-1 ks
    int64_t o_mu, o_sigma;         // (m) the posterior the lines are formed from: the predict-only sweep's, or kg_posterior_kernel's
    int64_t o_coef;                // (m, 2) c_mu, c_v: the weights of alpha and w in omega
    int64_t o_env_e, o_env_idx, o_env_n;   // (m, KG_ENV_LD) E_k / s of the envelope's lines i < A, their indices (int), (m) their number (int)
    int64_t o_env_eh;              // (m, KG_ENV_LD) the prior term's weights e_k c h(|u - ua_k|)
    int64_t o_val, o_grad;         // (m), (m, D)
};
int64_t kg_grad_doubles(const Context &c, int64_t m, int64_t Apad, KgGradWs *out);
// Xq is in the workspace.  own_posterior: mu and sigma are formed here from the front's vectors (handles whose sweep is not
// f64); else the caller has left the sweep's in o_mu / o_sigma.  Leaves val and grad in the workspace
hipError_t launch_kg_grad(Context &c, double *ws, const KgGradWs &g, const double *pts, const KgPoints &p, int m, double sf,
                          bool own_posterior);

}  // namespace tgp
