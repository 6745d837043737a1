/*
 * turbogp.h -- C-ABI of libturbogp.so: the MI355X-native GP-surrogate hot path of mbway/turbo.
 *
 * The reference has no FFI on this path: it is pure Python that calls scikit-learn / SciPy
 * (SURVEY.md section 8b).  Each entry point below therefore names the reference call site
 * (file:line under /root/reference, or sklearn/... for the third-party code it delegates to)
 * whose work it replaces.  The Python plugin classes in turbo_amd/ bind these symbols with
 * ctypes (INTEGRATION.md shows the stub a maintainer of the reference would add).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, int status return, no torch / C++ types.
 *   - All host arrays are caller-owned, row-major float64.  The library copies on entry and
 *     never keeps a caller pointer past return, except the *_dev candidate entry which borrows a
 *     DEVICE pointer until the next tgp_set_candidates* / tgp_destroy.
 *   - One handle = one GPU.  Calls on one handle must not overlap; a handle may be used from a
 *     different host thread than the one that created it (every entry calls hipSetDevice).
 *     Every call is synchronous: it returns with its results on the host.  All handles on one
 *     device share one HIP stream pair (a main stream and a CU-masked background stream the fit
 *     overlaps its inverse factor on; created with the first handle, released with the last), so
 *     calls on DIFFERENT handles of one device may be issued from different threads but do not
 *     overlap on the GPU.  The library never touches the null stream.
 *   - dtype selects the arithmetic of the candidate sweep (cross-kernel + triangular
 *     contraction).  The fit (kernel matrix, Cholesky, inverse factor, alpha) is always f64.
 */
#ifndef TURBOGP_H
#define TURBOGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tgp_handle_s *tgp_handle;

enum tgp_status {
    TGP_OK = 0,
    TGP_NOT_PD = 1,      /* kernel matrix not positive definite -> numpy.linalg.LinAlgError
                            (sklearn/gaussian_process/_gpr.py:348-358) */
    TGP_BAD_ARG = 2,     /* AssertionError / ValueError on the Python side */
    TGP_HIP_ERROR = 3,   /* RuntimeError; tgp_last_error() holds the HIP message */
    TGP_NOT_FITTED = 4,
    TGP_NO_MEMORY = 5,   /* host allocation failed -> MemoryError */
    TGP_NO_DEVICE = 6    /* tgp_create: no HIP device visible to this process */
};

/* TGP_F32X3 (opt-in): the sweep at f32 accuracy on the bf16 matrix pipe -- every f32 operand of the
 * triangular contraction split into three bf16 planes, six products accumulated in f32;
 * everything else as TGP_F32. */
/* TGP_F32H2 (opt-in): the same from two scaled fp16 planes and three products -- half the matrix
 * work and 4 bytes per element; same accuracy class. */
enum tgp_dtype { TGP_F64 = 0, TGP_F32 = 1, TGP_F32X3 = 2, TGP_F32H2 = 3 };

/* unit-amplitude stationary kernels: sklearn/gaussian_process/kernels.py RBF :1553-1565,
 * Matern nu=0.5/1.5/2.5 :1717-1724 */
enum tgp_kernel { TGP_RBF = 0, TGP_MATERN12 = 1, TGP_MATERN32 = 2, TGP_MATERN52 = 3 };

/* turbo/modules/acquisition_functions.py: UCB :147-158 (TGP_ACQ_SIGMA = its beta=inf branch),
 * PI :225-247, EI :336-358.  TGP_ACQ_NONE = predict only. */
/* TGP_ACQ_MES: max-value entropy search (Wang & Jegelka 2017), which the reference does not have: the average over the
 * handle's S maxima (tgp_mes_set_maxima / tgp_mes_draw, below) of a closed form of (mu, sigma); `incumbent` and `param`
 * are ignored.  Accepted by tgp_sweep, tgp_evaluate, tgp_sweep_topk, tgp_acq_grad and tgp_acq_lbfgsb. */
enum tgp_acq { TGP_ACQ_NONE = 0, TGP_ACQ_UCB = 1, TGP_ACQ_PI = 2, TGP_ACQ_EI = 3, TGP_ACQ_SIGMA = 4, TGP_ACQ_MES = 5 };

/* buffers readable through tgp_debug_read (parity tests only) */
enum tgp_buffer { TGP_BUF_K = 0, TGP_BUF_L = 1, TGP_BUF_LINV = 2, TGP_BUF_ALPHA = 3 };

/* ---- lifetime ------------------------------------------------------------------------- */

/* Create a context on HIP device `device` (index among visible devices); TGP_NO_DEVICE when the
 * process sees no GPU.
 * device == TGP_DEVICE_HOST: a context that never calls HIP -- the RELOAD path.  The reference pickles
 * every trial's model (turbo/recorder.py:117-155) and the plot path queries the reloaded models in
 * whatever process loaded the recorder (turbo/recorder.py:157-163, turbo/plotting/trials.py:192-195,
 * :371, :448, :574-577), which need not own an MI355X.  A host handle serves tgp_fit, tgp_fit_append
 * (as a full fit), tgp_export_state / tgp_import_state (the same blob), tgp_debug_read (L, alpha),
 * tgp_set_candidates, tgp_read_candidates, tgp_get_candidate, tgp_sweep, tgp_evaluate, tgp_predict,
 * tgp_mes_set_maxima, tgp_predict_cov, tgp_sample_joint (eps_in given), tgp_hyper_sample and the timing queries, always in float64 (csrc/host_backend.cpp: plain C++, its own arithmetic -- not
 * the HIP kernels, not the test oracle); every other entry returns TGP_BAD_ARG on it. */
#define TGP_DEVICE_HOST (-1)
int tgp_create(int device, int dtype, tgp_handle *out);
int tgp_destroy(tgp_handle h);
/* Message of the last failing call on this handle (or of tgp_create when h == NULL). */
const char *tgp_last_error(tgp_handle h);
/* "turbogp <version> gfx950" */
const char *tgp_version(void);

/* ---- fit ------------------------------------------------------------------------------- */

/* Fixed-hyper-parameter GP fit.  Replaces SciKitGPSurrogate.construct_model -> model.fit
 * (turbo/modules/surrogates.py:294-326, :318) i.e. sklearn _gpr.py:272-282 (y normalisation),
 * :346-347 (K = c*k(X,X) + noise*I, K.diag += jitter), :349 (lower Cholesky), :360-364 (alpha)
 * and :584-613 (log marginal likelihood, returned through `lml`).
 *   X   (N, D) row-major, y (N,)
 *   ls  length scale(s): n_ls == 1 (isotropic) or n_ls == D (ARD)
 * Outputs (nullable): lml, y_mean, y_std.
 * Returns TGP_NOT_PD when a pivot is <= 0 or not finite. */
int tgp_fit(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y,
            int kernel, double constant, const double *ls, int64_t n_ls,
            double noise, double jitter, int normalize_y,
            double *lml, double *y_mean, double *y_std);

/* Fit (exactly as tgp_fit) plus the gradient of the log marginal likelihood with respect to the
 * LOG hyper-parameters, `grad` = [d/dlog(constant), d/dlog(ls[0..n_ls)), d/dlog(noise)]
 * (2 + n_ls doubles; the noise entry is 0 when noise == 0).  Replaces
 * log_marginal_likelihood(theta, eval_gradient=True) (sklearn _gpr.py:537-652: K^-1 by
 * cho_solve(L, I) and 0.5*einsum("ijl,jik->kl", alpha alpha^T - K^-1, K_gradient)) that the
 * optimiser loop of GaussianProcessRegressor.fit (:296-337) evaluates per L-BFGS-B step, reached
 * from turbo/modules/surrogates.py:313-318 whenever training_iterations > 0.  The model is left
 * fitted at these hyper-parameters. */
int tgp_fit_grad(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y,
                 int kernel, double constant, const double *ls, int64_t n_ls,
                 double noise, double jitter, int normalize_y,
                 double *lml, double *y_mean, double *y_std, double *grad);

/* Leave-one-out cross-validation of the fitted model in closed form (Rasmussen & Williams, Gaussian Processes for
 * Machine Learning, section 5.4.2, eqs. 5.10-5.12): with K = c k0 + (noise + jitter) I in normalised units,
 * alpha = K^-1 y~ and kappa_i = (K^-1)_ii,
 *   mu_-i = y~_i - alpha_i / kappa_i,  sigma^2_-i = 1 / kappa_i                                           (5.12)
 *   lpd_i = -1/2 log sigma^2_-i - (y~_i - mu_-i)^2 / (2 sigma^2_-i) - 1/2 log 2 pi,  L_LOO = sum_i lpd_i  (5.10, 5.11)
 * The normalisation (y_mean, y_std of ALL N points) and the hyper-parameters are held across the folds: that is what the
 * closed form means; no model is refitted.  Outputs, all nullable:
 *   resid (N)   y_i - mu_-i in RAW units (y_std alpha_i / kappa_i); the held-out mean is y_i - resid_i.  The residual
 *               and not the mean, because a handle that received its factor (tgp_import_factor_dev) holds no y.
 *   sigma (N)   y_std / sqrt(kappa_i), RAW units: the predictive deviation of the held-out OBSERVATION.  It contains
 *               the noise AND the jitter, because K carries both; tgp_predict's sigma has the noise but no jitter.
 *   lpd (N), *loo   NORMALISED units, as `lml` is; *loo is the sum of lpd in a fixed order (the same bits run to run).
 * TGP_NOT_FITTED without a model; TGP_NOT_PD if a kappa_i is <= 0 or not finite (nothing is clamped; it cannot happen
 * after a successful fit).  Works on every fitted handle -- the one-workgroup fits, the blocked fit, a fit extended by
 * tgp_fit_append, a received factor, TGP_DEVICE_HOST handles (plain C++, csrc/host_backend.cpp) -- always in float64
 * whatever the handle's dtype, and touches neither the fit, the resident candidates, the winner record, a Thompson
 * draw nor the MES maxima. */
int tgp_loo(tgp_handle h, double *resid, double *sigma, double *lpd, double *loo);

/* Fit (as tgp_fit; arguments through y_std as tgp_fit_grad's) plus the leave-one-out score `loo` = L_LOO and ITS
 * gradient with respect to the LOG hyper-parameters (R&W eq. 5.13, taken as one trace 1/2 tr(G dK/dtheta) with
 * G = b alpha^T + alpha b^T - 2 K^-1 diag(w) K^-1, p_i = alpha_i / kappa_i, w_i = (1 / kappa_i + p_i^2) / 2,
 * b = K^-1 p): `grad` = [d/dlog(constant), d/dlog(ls[0..n_ls)), d/dlog(noise)], 2 + n_ls doubles in normalised units,
 * the noise entry exactly 0.0 when noise == 0 -- tgp_fit_grad's layout.  `lml` is the log marginal likelihood as
 * tgp_fit returns it.  The fit takes the BLOCKED route for every N (the gradient needs Linv^T and the N^2 workspaces
 * only that route guarantees), so `lml` has the bytes of tgp_fit_grad under TGP_SMALL=0; *loo is byte for byte what
 * tgp_loo returns on the handle afterwards.  The model is left fitted at these hyper-parameters.  GPU only: a host
 * handle answers TGP_BAD_ARG.  Status as tgp_fit, plus TGP_NOT_PD for a kappa_i <= 0 or not finite. */
int tgp_fit_loo_grad(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y,
                     int kernel, double constant, const double *ls, int64_t n_ls,
                     double noise, double jitter, int normalize_y,
                     double *lml, double *y_mean, double *y_std, double *loo, double *grad);

/* Fit like tgp_fit, but when the handle already holds a fit with the same kernel, hyper-parameters,
 * jitter and normalisation whose training inputs are bit-for-bit the first N-1 rows of X, extend
 * the factor by ONE row in O(N^2) (four triangular GEMVs) instead of refactorising in O(N^3):
 *   l = Linv k,  lambda = sqrt(kappa - l.l),  L' = [[L,0],[l^T,lambda]],
 *   Linv' = [[Linv,0],[-(Linv^T l)^T/lambda, 1/lambda]],  alpha' = Linv'^T Linv' yn'.
 * That is the reference's loop: the Optimiser appends exactly one trial per iteration and refits
 * from scratch (turbo/optimiser.py:93-96, :335-336 -> surrogates.py:318).  Any mismatch (or a new
 * 256-row padding block) falls back to tgp_fit.  *appended (nullable) tells which path ran. */
int tgp_fit_append(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y,
                   int kernel, double constant, const double *ls, int64_t n_ls,
                   double noise, double jitter, int normalize_y,
                   double *lml, double *y_mean, double *y_std, int *appended);

/* Persistence (turbo/recorder.py:141-147 pickles every trial's model with dill; turbo/utils.py:72-90
 * loads them back, possibly in another process).  The blob holds what DEFINES the model -- kernel,
 * hyper-parameters, X, y: (8 + D + N*D + N) * 8 bytes -- not the O(N^2) factor, which import rebuilds
 * by running tgp_fit (milliseconds), so a Recorder that keeps one model per trial stays O(N*D) per
 * trial as with the reference's sklearn objects (which hold X_train_, y_train_, L_, alpha_).
 *   export: *size receives the bytes needed; buf == NULL only queries the size.
 *   import: status of the fit it runs (TGP_NOT_PD possible); lml nullable. */
int tgp_export_state(tgp_handle h, void *buf, int64_t cap, int64_t *size);
int tgp_import_state(tgp_handle h, const void *buf, int64_t size, double *lml);

/* ---- Handing a FACTOR over instead of recomputing it (round 6) -------------------------------------------------
 * SURVEY.md 8e's alternative to the replicated fit ("fit on GPU0 + broadcast of L, alpha"); what scikit-learn keeps as
 * L_ / alpha_ (sklearn/gaussian_process/_gpr.py:349,360), reached from turbo/modules/surrogates.py:318.
 * With the candidate batch sharded over G GPUs the fit is the part that does not shrink (C3, 8 shards: 2.2 of 6.4 ms).
 * A handle can instead RECEIVE what a sweep needs -- the scaled training points, the length scales, alpha, the scalars
 * and the inverse factor Linv -- from device memory: another handle's buffers in the same process (tgp_export_factor_dev),
 * or a buffer a collective filled (an RCCL broadcast into a torch tensor).  Only float64 state travels; an f32 / f32h2 /
 * f32x3 handle cuts its own copies with the casts its own fit uses, so a receiver's sweep returns the giver's bytes.
 *
 * tgp_export_factor_dev fills `out` with the giver's shapes, hyper-parameters, scalars and DEVICE pointers INTO its own
 * buffers: valid until the giver's next fit / import / destroy, never owned by the caller.
 * tgp_import_factor_dev copies rows [row0, row0 + rows) of Linv (leading dimension Np) into the handle, on its stream.
 * The rows must arrive in order -- top down, as a Cholesky finishes them (the inverse factor's row block i is final once
 * panel i is): row0 = 0 starts a new factor (shapes, scalars, Xs, ls, alpha are taken from `f` then), every later call
 * continues it, and the call that delivers row Np - 1 completes it: the handle is fitted from then on (TGP_NOT_FITTED
 * before).  One call with rows = Np imports the whole factor.  A handle that received its factor holds no training
 * set: tgp_export_state and tgp_debug_read(L) refuse, tgp_fit_append refits; everything that evaluates the model
 * (sweeps, tgp_acq_grad, the gradient stage) works.  Host handles: TGP_BAD_ARG. */
typedef struct tgp_factor {
    int64_t N, D, Np, Dp;        /* Np = N rounded up to 256, Dp = D rounded up to 4 */
    int64_t fit_gen;             /* the giver's fit generation: the blocks of one import must all carry the same */
    int32_t kernel, normalize_y; /* tgp_kernel; as given to tgp_fit */
    int32_t small_path, reserved;/* 1: the giver's fit came from the one-workgroup kernels (N <= 128): the receiver sweeps with them too */
    double constant, noise, jitter, y_mean, y_std, lml, sumlog;
    const void *Xs;              /* (Np, Dp) f64: X / length_scale, padded rows and columns zero */
    const void *ls;              /* (D) f64 */
    const void *alpha;           /* (Np) f64 */
    const void *Linv;            /* (Np, Np) f64 row-major: L^-1, zeros above the diagonal */
} tgp_factor;
int tgp_export_factor_dev(tgp_handle h, tgp_factor *out);
int tgp_import_factor_dev(tgp_handle h, const tgp_factor *f, int64_t row0, int64_t rows);

/* Copy a fitted buffer to the host (tests): K / L / LINV are (N, N) row-major (L and LINV
 * lower-triangular with zeros above the diagonal), ALPHA is (N,). */
int tgp_debug_read(tgp_handle h, int which, double *out);

/* ---- candidates ------------------------------------------------------------------------- */

/* Upload an (M, D) float64 candidate batch; it stays resident in HBM for later sweeps.
 * Replaces the hand-over of `random_x` at turbo/modules/auxiliary_optimisers.py:60-61. */
int tgp_set_candidates(tgp_handle h, const double *Xc, int64_t M);
/* Borrow an (M, D) float64 row-major batch that already lives in this GPU's memory
 * (e.g. a torch tensor's data_ptr()).  The pointer is checked against the HIP runtime's records
 * (device memory, this GPU, at least M*D doubles left in its allocation) -> TGP_BAD_ARG. */
int tgp_set_candidates_dev(tgp_handle h, const void *Xc_dev, int64_t M);
/* Fill the resident batch with M uniform candidates drawn ON the GPU: x[d] = lo[d] + (hi[d] -
 * lo[d]) * u, u from Philox-4x32-10 keyed by `seed`; candidate i of this call is number
 * first_candidate + i of the stream, so shards of one batch on several GPUs are disjoint pieces
 * of the same stream.  Device-side counterpart of random_selector
 * (turbo/modules/naive_selectors.py:39-46; that one draws from the global NumPy RNG, so the
 * values differ by design -- opt-in). */
int tgp_gen_candidates(tgp_handle h, uint64_t seed, uint64_t first_candidate, int64_t M,
                       const double *lo, const double *hi);
/* Latin hypercube design on the GPU: samples first_sample .. first_sample + M - 1 of an
 * n_total-point design.  Sample i, dimension d:  lo_d + (hi_d - lo_d) * ((pi_d(i) + u_id) / n_total)
 * with pi_d a keyed pseudo-random permutation of the n_total strata (4-round Feistel network over
 * Philox-4x32-10, cycle-walked) and u_id uniform in [0, 1) from the Philox stream of `seed`: every
 * sample is computed on its own, so shards are rows of one design.  Device-side counterpart of
 * LHS_selector (turbo/modules/naive_selectors.py:58-83: arange + rand per stratum, then
 * np.random.permutation per column from the global NumPy RNG -- the values differ by design).
 *   tgp_gen_candidates_lhs  fills the resident candidate batch (needs a fitted model for D)
 *   tgp_lhs_design          hands an (M, D) design back to the host; needs no model (the reference
 *                           uses the selector for the pre-phase trials, before any fit) */
int tgp_gen_candidates_lhs(tgp_handle h, uint64_t seed, uint64_t first_sample, int64_t M,
                           uint64_t n_total, const double *lo, const double *hi);
int tgp_lhs_design(tgp_handle h, uint64_t seed, uint64_t first_sample, int64_t M, uint64_t n_total,
                   int64_t D, const double *lo, const double *hi, double *out);
/* Read rows first .. first + count - 1 of the resident batch back: (count, D). */
int tgp_read_candidates(tgp_handle h, int64_t first, int64_t count, double *out);
/* Read candidate row `idx` back (the argmax row: auxiliary_optimisers.py:64-65). */
int tgp_get_candidate(tgp_handle h, int64_t idx, double *out_row);

/* ---- sweep ------------------------------------------------------------------------------ */

/* Posterior mean / std and acquisition over the resident candidate batch, plus its argmax.
 * Replaces  acq(random_x)  ->  model.predict(X, return_std_dev=True)
 * (turbo/modules/acquisition_functions.py:152,230,341 -> surrogates.py:332-338 -> sklearn
 * _gpr.py:443-494) and the argsort/[0] of auxiliary_optimisers.py:63-66.
 *   acq        enum tgp_acq;  sf = +1 ('max') or -1 ('min');  incumbent = best raw y so far
 *   param      beta (UCB) or xi (PI / EI)
 *   mu, sigma, acq_out   nullable (M,) host outputs
 *   best_val, best_idx   nullable; argmax of the acquisition (of -inf if all NaN), lowest index
 *                        wins ties.  With TGP_ACQ_NONE they are left untouched.
 *   n_clamped  nullable; number of candidates whose variance was < 0 and clamped to 0
 *              (sklearn _gpr.py:479-485 warns once in that case) */
int tgp_sweep(tgp_handle h, int acq, double sf, double incumbent, double param,
              double *mu, double *sigma, double *acq_out,
              double *best_val, int64_t *best_idx, int64_t *n_clamped);

/* Sharded arg-max (the candidate batch is cut into contiguous shards, one per GPU,
 * and the per-shard winners are combined; the reference's own arg-max is the argsort/[0] of
 * turbo/modules/auxiliary_optimisers.py:63-66 over the whole batch).  Attach a DEVICE buffer of
 * D + 2 doubles on this GPU: every later single-winner sweep with an acquisition (tgp_sweep,
 * tgp_evaluate, tgp_sweep_topk; not tgp_sweep_batch) also packs
 *     [best value, (double)(global_offset + best index), candidate row (D)]
 * into it, on the device and before the call returns, so the all-gather between GPUs (RCCL) can
 * read it in place -- no D2H of the row, no host-built tensor.  global_offset = global index of
 * candidate 0 of this handle's shard.  The record is written on the library's stream; another
 * stream -- RCCL on the caller's -- is ordered behind it by tgp_winner_wait.  The buffer is borrowed (checked like
 * tgp_set_candidates_dev) until replaced, detached with rec_dev == NULL, a fit with another D,
 * or tgp_destroy. */
int tgp_set_winner_out(tgp_handle h, void *rec_dev, int64_t global_offset);
/* (round 6) Make `stream` -- a hipStream_t of the CALLER on this handle's device, passed as a plain pointer; NULL is
 * the legacy default stream -- wait for the winner record of the last sweep that packed one: the library records an
 * event on its own stream behind every kernel chain that packs the record (tgp_sweep, tgp_evaluate, tgp_sweep_topk),
 * and this call is one hipStreamWaitEvent on it.  The record is written on the library's stream and read by RCCL on
 * the caller's (turbo_amd/distributed.py); the polled sweeps return on their doorbell, without a synchronisation of the
 * library's stream, so this event is what orders the caller's stream behind the record.  Nothing has packed a record
 * into the attached buffer yet (tgp_set_winner_out starts a buffer afresh): nothing to wait for, TGP_OK.  No record
 * attached: TGP_BAD_ARG. */
int tgp_winner_wait(tgp_handle h, void *stream);

/* Acquisition value AND gradient with respect to the query point for a small batch (m <= 4096)
 * of host points Xq (m, D): val (m,), grad (m, D).  TGP_ACQ_NONE returns the posterior mean and its
 * gradient.  Serves the gradient stage of the auxiliary optimiser
 * (turbo/modules/auxiliary_optimisers.py:69-112, which differentiates 1-point acq calls by finite
 * differences); always float64, independent of the handle's sweep dtype. */
int tgp_acq_grad(tgp_handle h, const double *Xq, int64_t m, int acq, double sf, double incumbent,
                 double param, double *val, double *grad);

/* Greedy selection of q candidates for W parallel workers, conditioned on P trials still running.  The reference stubs
 * this out (turbo/optimiser.py:44-45 `#self.parallel_strategy = None#TODO`, the commented-out run_async /
 * _next_async_trial of :361-396); the author's older library documents the strategies
 * (old_library/bayesian_optimiser.py:76-103) and implements Kriging Believer at :527-566.
 * From the fitted handle and the resident candidate batch (M rows): condition on the pending points Xp (P, D) in order,
 * then select q rows one after the other.  Each new point z gets a fantasy value in raw units --
 *   TGP_BATCH_KB  the posterior mean at z given every earlier point (Kriging Believer)
 *   TGP_BATCH_CL  `lie` (Constant Liar; finite)
 * -- and conditioning is exactly what a refit on the augmented data would predict with the kernel hyper-parameters,
 * the jitter and y_mean / y_std of the real observations held (the fantasy enters as (y - y_mean) / y_std, noise and
 * jitter on the augmented diagonal, no noise in the cross-kernel).  For EI / PI the incumbent after each fantasy is
 * the best of (incumbent, fantasies so far) in the direction of sf (old_library/bayesian_optimiser.py:509); UCB and
 * TGP_ACQ_SIGMA do not use it; TGP_ACQ_NONE and TGP_ACQ_MES are TGP_BAD_ARG.  Each selection is the arg-max over the rows not yet
 * selected in this call (lowest index on ties, NaN never wins); with q = 1 and P = 0 it is tgp_sweep's best_idx /
 * best_val bit for bit.  The fit and the batch are unchanged by the call.
 *   q          1 <= q <= M, P + q <= 64 (else TGP_BAD_ARG)
 *   Xp         (P, D) pending points, NULL when P == 0
 *   idx_out, val_out   (q) candidate index and acquisition value of each selection
 *   x_out      (q, D) the selected rows (nullable);  fantasy_out (P + q) the fantasies, pending first (nullable)
 *   mu_out, sigma_out  (M) posterior after all P + q points (nullable; asking for them costs one more pass)
 *   n_clamped  (nullable) variances clamped at 0, summed over the sweep and every step
 * TGP_NOT_PD when a pivot of the augmented factor is <= 0 or not finite (a pending point duplicating a training point
 * with noise 0).  The step arithmetic is f64 whatever the handle's dtype.  GPU only: TGP_BAD_ARG
 * on host handles. */
enum tgp_batch_strategy { TGP_BATCH_KB = 0, TGP_BATCH_CL = 1 };
int tgp_sweep_batch(tgp_handle h, int64_t q, int strategy, double lie, const double *Xp, int64_t P, int acq, double sf,
                    double incumbent, double param, int64_t *idx_out, double *val_out, double *x_out,
                    double *fantasy_out, double *mu_out, double *sigma_out, int64_t *n_clamped);

/* The Monte Carlo parallel strategy of the author's older library (old_library/bayesian_optimiser.py:76-106,
 * _max_mc_acq_suggestion :568-624): S simulations of the outcomes of the P pending and the selected points, and the
 * AVERAGE of the S acquisition functions maximised.  Arguments and rules as tgp_sweep_batch without strategy / lie.  In
 * normalised units, with R the new block of the augmented factor and G the scaled cross-covariance columns of
 * tgp_sweep_batch (hyper-parameters, jitter, y_mean / y_std held):
 *   y~[s,j]  = mu~_{s,j-1}(z_j) + R[j,j] eps[s,j],  eps[s,j] ~ N(0,1)   a draw of the OBSERVATION y at z_j given simulation
 *                                                                      s's own earlier draws (noise + jitter in R[j,j]^2)
 *   mu~_s(x) = mu0(x) + sum_{i<=j} G[x,i] eps[s,i];   sigma~(x) is tgp_sweep_batch's and shared by the simulations
 *   inc_s    = best(incumbent, raw fantasies of simulation s so far) in the direction of sf      (EI / PI only)
 *   a(x)     = (1/S) sum_s acq(y_mean + y_std mu~_s(x), y_std sigma~(x); inc_s), summed in the order s = 0, 1, ...
 * which is what S literal refits on the augmented data give.  The draw is JOINT (sequential conditioning); the old
 * library draws each pending point on its own (:582-585), which ignores that two nearby pending points come out alike --
 * with one pending point the two coincide.  TGP_ACQ_SIGMA does not depend on the simulations: a(x) = sigma~(x).
 *   S          1 <= S <= 64 simulations
 *   eps_in     NULL: eps[s,j] is a Philox-4x32-10 normal keyed by `seed`, counter (element lo, element hi, 0, tag),
 *              element s 64 + j with j counted pending-first, the 53-bit uniforms and the Box-Muller branch of the
 *              Thompson draw (csrc/philox.hpp) -- simulation s does not depend on S, the draw for point j not on P or q.
 *              Else (S, P + q) finite standard normals used as they are (quasi-random or common random numbers)
 *   idx_out, val_out   (q) candidate index and AVERAGED acquisition of each selection (lowest index on ties, NaN never
 *              wins, taken rows masked); with P = 0 the first selection is tgp_sweep's launch path, so q = 1, P = 0
 *              returns tgp_sweep's best_idx / best_val bit for bit
 *   x_out      (q, D) the selected rows;  fantasy_out (S, P + q) the fantasies, raw units;  eps_out (S, P + q) the
 *              normals used;  acq_out (q, M) every step's averaged acquisition with the rows already taken (and NaN)
 *              at -inf -- row 0 with P = 0 holds the values of tgp_sweep's acq_out, so in the handle's arithmetic
 *              (f32 on an f32 handle; every other row is f64);  sigma_out (M) after all P + q points (costs one more
 *              pass).  All nullable
 *   n_clamped  (nullable) variances clamped at 0, summed over the sweep and every step, once per (candidate, point)
 * TGP_ACQ_MES is TGP_BAD_ARG here too.
 * TGP_NOT_PD as tgp_sweep_batch (the pivot does not depend on the simulation).  f64 whatever the handle's dtype.  The
 * fit, the candidates, the winner record, a Thompson draw and later sweeps are untouched.  GPU only: TGP_BAD_ARG on host
 * handles. */
int tgp_sweep_batch_mc(tgp_handle h, int64_t q, int64_t S, uint64_t seed, const double *eps_in, const double *Xp, int64_t P,
                       int acq, double sf, double incumbent, double param, int64_t *idx_out, double *val_out,
                       double *x_out, double *fantasy_out, double *eps_out, double *acq_out, double *sigma_out,
                       int64_t *n_clamped);

/* Thompson sampling: the acquisition the author's older library names but leaves unimplemented
 * (old_library/acquisition_functions.py:20-21, bayesian_optimiser.py:137-138, :263-264) and its 'asyTS' batch
 * strategy (:102-104).  tgp_ts_draw draws S sample paths of the fitted model by pathwise conditioning with F random
 * Fourier features (Wilson et al. 2020), in normalised units (u = x / l, c the constant):
 *   f_prior_s(x) = sqrt(2c/F) sum_i W[s,i] cos(omega_i . u + b_i)   (omega, b shared by the samples)
 *   f_s(x)       = f_prior_s(x) + sum_n c k0(x, X_n) v_s[n],  v_s = K^-1 (y~ - f_prior_s(X) - eps_s)
 *   raw value    = y_mean + y_std f_s(x)
 * omega_i ~ N(0, I) for RBF and z sqrt(2 nu / chi2_{2 nu}) for Matern nu; b_i ~ U[0, 2 pi); W, eps standard normal,
 * eps scaled by sqrt(noise + jitter).  The samples are of the LATENT function: their variance is the posterior
 * variance without the WhiteKernel noise, and their mean is the posterior mean exactly whatever F is.  Random numbers
 * are Philox-4x32-10 keyed by the seed, counter (element lo, element hi, stream, tag); W is indexed s F + i and eps
 * s N + n, so sample s does not depend on S (the layout: csrc/ts_kernels.hip).  All arithmetic is f64 whatever the
 * handle's dtype.  A draw belongs to one fit: after any later fit, append or factor import the three other entries
 * return TGP_BAD_ARG until the next draw (as they do before the first).  The fit, the candidates, the winner record
 * and tgp_sweep / tgp_sweep_batch are not touched.  GPU only: TGP_BAD_ARG on host handles.
 *   tgp_ts_draw   1 <= S <= 64, F a multiple of 64 in [64, 16384]; stored in the handle until the next draw
 *   tgp_ts_sweep  over the resident candidates: per sample the arg-max of sf * raw value (sf = +1 or -1; lowest index
 *                 on ties, NaN never wins); distinct != 0: sample s takes the best row not taken by samples < s (needs
 *                 S <= M).  idx_out, val_out (S): index and RAW sampled value; x_out (S, D) the rows and f_out (M, S)
 *                 every raw value: nullable
 *   tgp_ts_eval   the paths at m <= 4096 host points Xq (m, D): f_out (m, S) raw values, grad_out (m, S, D) d f / d x
 *                 (nullable)
 *   tgp_ts_read   the draw itself: omega (F, D) in scaled coordinates, b (F), W (S, F), eps (S, N); each nullable */
int tgp_ts_draw(tgp_handle h, uint64_t seed, int64_t S, int64_t F);
int tgp_ts_sweep(tgp_handle h, double sf, int distinct, int64_t *idx_out, double *val_out, double *x_out, double *f_out);
int tgp_ts_eval(tgp_handle h, const double *Xq, int64_t m, double *f_out, double *grad_out);
int tgp_ts_read(tgp_handle h, double *omega, double *b, double *W, double *eps);

/* Max-value entropy search (TGP_ACQ_MES).  With y*_s, s = 0 .. S-1, samples of the optimum's RAW value (maxima for
 * sf = +1, minima for sf = -1) and mu, sigma tgp_sweep's raw posterior mean and deviation at a candidate:
 *   sigma_f^2 = max(sigma^2 - noise y_std^2, 0)     the latent deviation: sigma includes the WhiteKernel noise, the y*
 *                                                   are maxima of the LATENT function (the Thompson section above)
 *   gamma_s   = sf (y*_s - mu) / sigma_f
 *   h(gamma)  = gamma phi(gamma) / (2 Phi(gamma)) - log Phi(gamma)
 *   a         = (1/S) sum_s h(gamma_s), summed in the order s = 0, 1, ...;  a = 0 where sigma_f == 0
 * always in float64, through the scaled complementary error function: finite for every finite input.
 *   tgp_mes_set_maxima  stores 1 <= S <= 64 finite raw values in the handle (host handles too).  Like a Thompson draw
 *                       they belong to ONE fit: any later fit, append, factor import or state import drops them, and
 *                       TGP_ACQ_MES without maxima is TGP_BAD_ARG.
 *   tgp_mes_draw        GPU only: tgp_ts_draw(seed, S, F), then the non-distinct tgp_ts_sweep(sf) over the resident
 *                       candidates; each sampled maximum is moved to `incumbent` where the incumbent is better in the
 *                       direction of sf (a NaN incumbent skips that), and the result becomes the handle's maxima on
 *                       the device.  ystar_out (S) is nullable.  The Thompson draw it made STAYS in the handle,
 *                       replacing an earlier one (tgp_ts_sweep / tgp_ts_eval / tgp_ts_read then see this draw).
 * An arg-max-only TGP_ACQ_MES sweep always takes the unpruned schedule (tgp_last_timings slot 12 stays -1): the pruned
 * sweep's bounds are proved for EI / PI / UCB only.  The winner record is packed as for the others. */
int tgp_mes_set_maxima(tgp_handle h, const double *ystar, int64_t S);
int tgp_mes_draw(tgp_handle h, uint64_t seed, int64_t S, int64_t F, double sf, double incumbent, double *ystar_out);

/* The JOINT posterior over m <= 4096 host points Xq (m, D): what the model the reference wraps answers with
 * predict(return_cov=True) -- sklearn _gpr.py:454-469: V = solve_triangular(L, K*^T), y_cov = kernel_(X) - V^T V, times
 * y_train_std^2 -- and what its sample_y draws from (:498-535, rng.multivariate_normal(y_mean, y_cov, n_samples)); the
 * reference's SciKitGPSurrogate.ModelInstance.predict (turbo/modules/surrogates.py:332-338) keeps the diagonal only, and its
 * roadmap asks the Surrogate for "sampling methods" (docs/source/refactor.md:54-62).  In normalised units (u = x / l, c the
 * constant, k0 the unit kernel):
 *   Ks = c k0(Xq, X) (m, N);  V = Linv Ks^T (N, m);  Sigma = c k0(Xq, Xq) + [latent ? 0 : noise] I - V^T V (m, m)
 *   mu = y_mean + y_std Ks alpha;  raw covariance = y_std^2 Sigma
 * The noise goes on the diagonal only, duplicated query rows included (sklearn's WhiteKernel(X)); the jitter is not in Sigma
 * (kernel_(X) does not carry sklearn's alpha).  latent = 0: the diagonal is tgp_predict's sigma^2 before its clamp;
 * latent = 1: the latent function's covariance, the quantity the Thompson and MES sections above define.  Always float64.
 * tgp_predict_cov
 *   mu_out (m) nullable; cov_out (m, m) row-major, raw units, symmetric BIT FOR BIT (the lower triangle is computed, the
 *   upper one is its copy), the same bits from run to run, and an entry depends on its own two points only: pair (i, j)
 *   has the same bits whatever other points travel with it.  Negative diagonal entries are NOT clamped (sklearn does not
 *   clamp y_cov); n_negative_diag (nullable) counts them.
 * tgp_sample_joint: S exact joint samples,  y_out[s, j] = mu[j] + y_std (Lc eps[s, :])[j],  y_out (S, m)
 *   Lc         the lower Cholesky factor of Sigma + nugget I (nugget >= 0 and finite), under the fit's pivot rule with the
 *              row's own diagonal entry as the scale: TGP_NOT_PD when a pivot's square is <= 8 eps (that diagonal entry of
 *              Sigma + nugget I) or not finite -- exactly duplicated query rows with latent = 1 and nugget = 0 are
 *              therefore TGP_NOT_PD (sklearn's multivariate_normal falls back to an SVD there; here the nugget is explicit)
 *   1 <= S <= 4096
 *   eps_in     NULL: eps[s, j] is a Philox-4x32-10 normal keyed by `seed`, counter (element lo, element hi, 0, tag "COVJ"),
 *              element s 4096 + j, the 53-bit uniforms and the Box-Muller branch of the Thompson draw (csrc/philox.hpp):
 *              sample s depends neither on S nor on m.  Else (S, m) finite standard normals used as they are (quasi-random
 *              or common random numbers)
 *   eps_out (S, m) the normals used, mu_out (m): nullable
 * Both: TGP_NOT_FITTED without a model; TGP_BAD_ARG for m or S out of range or non-finite input.  They work on every fitted
 * GPU handle (all size classes, a factor received with tgp_import_factor_dev included) and touch neither the fit, the
 * resident candidates, the winner record, a Thompson draw nor the MES maxima.  Host handles serve both in plain C++
 * (csrc/host_backend.cpp: the Recorder's reload path, turbo/recorder.py:157-163 -- posterior sample paths plotted where no
 * GPU is visible); tgp_sample_joint needs eps_in there (the Philox draw is device code): NULL is TGP_BAD_ARG. */
int tgp_predict_cov(tgp_handle h, const double *Xq, int64_t m, int latent,
                    double *mu_out, double *cov_out, int64_t *n_negative_diag);
int tgp_sample_joint(tgp_handle h, const double *Xq, int64_t m, int64_t S, int latent, double nugget,
                     uint64_t seed, const double *eps_in, double *y_out, double *eps_out, double *mu_out);

/* The sweep of tgp_sweep, returning the k <= 64 BEST candidates instead of the single best:
 * vals[0..k) descending, idxs[0..k) their indices (lowest index first among equal values, NaN
 * last, -1 when the batch holds fewer than k candidates).  This is
 * `best_ids = np.argsort(random_y)[:start_from_best]` of the reference's gradient stage
 * (turbo/modules/auxiliary_optimisers.py:63-66, :77-79) without the (M,) acquisition vector leaving
 * the GPU. */
int tgp_sweep_topk(tgp_handle h, int acq, double sf, double incumbent, double param, int64_t k,
                   double *vals, int64_t *idxs, int64_t *n_clamped);

/* The hyper-parameter fit inside the library: S <= 64 starts theta0 (S, P), theta = log(constant, length
 * scale(s), noise) with P = 2 + n_ls (n_ls = 1 or D), are each optimised to a local maximum of the log
 * marginal likelihood inside [log_lo, log_hi].  What GaussianProcessRegressor.fit does with
 * optimizer='fmin_l_bfgs_b' and n_restarts_optimizer = S - 1 (sklearn _gpr.py:296-337, :654-670, reached
 * from turbo/modules/surrogates.py:313-318), the restarts side by side.
 *
 * tgp_fit_lbfgsb: every start is walked by L-BFGS-B itself (csrc/host_lbfgsb.hpp: the algorithm behind
 *   scipy.optimize.minimize(method='L-BFGS-B') restated -- generalised Cauchy point, subspace minimisation,
 *   More-Thuente line search, 10 pairs, SciPy's defaults pgtol 1e-5 and factr 1e7): the iterates, the number
 *   of evaluations and the optimum are the ones scikit-learn's fit arrives at on the same objective (to the
 *   rounding of the objective).  A host thread and a worker handle (tgp_workers_acquire) per start drive
 *   tgp_fit_grad from inside the library -- no interpreter between two evaluations.  With more than one start
 *   the caller's handle is not touched at all; with a single start (or one thread) it runs the evaluations
 *   itself and is left holding the LAST evaluation of the LAST start -- not a model to use.
 * tgp_fit_optimise: the library's choice of optimiser.
 *   N <= 128, D <= 64:  ONE launch, a workgroup per start (kernel matrix, Cholesky, inverse factor, alpha,
 *       LML, its gradient and one step of a projected L-BFGS per iteration, with L-BFGS-B's stopping rules):
 *       no host round trip per evaluation -- other iterates than SciPy's, the same or a better optimum.  The
 *       handle's fitted model is left untouched.
 *   larger problems:    tgp_fit_lbfgsb.
 * An entry with log_lo == log_hi is a FIXED hyper-parameter: tgp_fit_lbfgsb leaves it out of the optimiser's vector
 * (as scikit-learn leaves a "fixed" hyper-parameter out of theta; theta0's value there is replaced by the bound), the
 * one-launch path treats it as a coordinate that cannot move.  The noise entry may be fixed at -INFINITY: a kernel
 * without a noise term (noise = 0; such a call always takes the tgp_fit_lbfgsb route).
 * Either way the caller picks the best start and fits it with tgp_fit.
 *   max_iter: accepted iterations per start (SciPy's maxiter); line-search trials do not count against it
 *       (they have SciPy's maxfun = 15000 of their own).
 *   theta_out (S, P), f_out (S) = -LML at theta_out
 *   status_out (S, nullable): 1 converged, 0 stopped by max_iter (SciPy's status 1), 2 no acceptable step
 *       from the last iterate (SciPy's status 2, ABNORMAL_TERMINATION_IN_LNSRCH; theta_out is that iterate)
 *   evaluations (nullable): LML + gradient evaluations over all starts */
int tgp_fit_lbfgsb(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                   const double *theta0, int64_t S, int64_t n_ls, const double *log_lo, const double *log_hi,
                   double jitter, int normalize_y, int64_t max_iter, double *theta_out, double *f_out,
                   int64_t *status_out, int64_t *evaluations);
int tgp_fit_optimise(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                     const double *theta0, int64_t S, int64_t n_ls, const double *log_lo, const double *log_hi,
                     double jitter, int normalize_y, int64_t max_iter, double *theta_out, double *f_out,
                     int64_t *status_out, int64_t *evaluations);

/* MARGINALISED hyper-parameters: the second of the two ways the author's older library names for them
 * (old_library/bayesian_optimiser.py:53-75 -- 'optimise' fits a point estimate, 'marginalise' draws MCMC samples of the
 * hyper-parameters and averages the acquisition over them, the integrated acquisition of Snoek et al. 2012 -- with the
 * arguments left #TODO at :153-165).  tgp_fit_optimise / tgp_fit_lbfgsb above are the first; these two are the second.
 *
 * tgp_hyper_sample: S samples of theta = log(constant, length scale(s), noise) (layout, units and P = 2 + n_ls of
 *   tgp_fit_lbfgsb) from the density exp(LML(theta)) on the box [log_lo, log_hi] -- a uniform prior in log space over the
 *   bounds the optimiser uses.  An entry with log_lo == log_hi is fixed at the bound and not sampled; the noise entry may
 *   be fixed at -INFINITY.  theta0's free entries must lie inside the box.  The chain is coordinate-wise slice sampling
 *   with stepping-out and shrinkage (Neal 2003, figs. 3 and 5; csrc/host_slice.hpp): one sweep is one pass over the free
 *   coordinates in index order; per coordinate the initial interval has width[p] (NULL: 1.0 each) and is placed at random
 *   around the current value, each side steps out at most 8 times (the left side first) while LML(end) exceeds the slice
 *   level, an end that leaves the box is clipped to the bound, and proposals are drawn from the interval, which shrinks
 *   towards the current value, until one exceeds the level.  `burn` sweeps are discarded; sample k is the state after
 *   sweep burn + (k + 1) thin, thin >= 1, 1 <= S <= 64.
 *   Every evaluation is this handle's own tgp_fit taken for its LML -- whichever fit path N selects, the host backend on
 *   a TGP_DEVICE_HOST handle (and in libturbogp_host.so) -- from inside the library: no interpreter between two
 *   evaluations.  TGP_NOT_PD at a proposal counts as LML = -inf: the proposal is rejected and counted in *not_pd;
 *   TGP_NOT_PD at theta0 is returned.  The handle is left fitted at the LAST evaluation -- not a model to use.
 *   Randomness is counter-based, so the walk is a pure function of the arguments: the j-th uniform of the call
 *   (j = 0, 1, ...) is the 53-bit uniform (csrc/philox.hpp philox_u53) of words 0 and 1 of
 *   Philox-4x32-10(counter (j lo, j hi, tag "SLIC" = 0x534C4943, 0), key (seed lo, seed hi)).  Consumption order, per
 *   coordinate update: one uniform u for the slice level (LML(current) + log u), one for the interval's position
 *   (left end = current - width[p] v), then one per shrinkage proposal (left + t (right - left)); stepping out draws none.
 *   theta_out (S, P), lml_out (S) the LML at each sample; evaluations (nullable): tgp_fit calls made, theta0's and the
 *   non-PD ones included; not_pd (nullable).
 *
 * tgp_sweep_integrated: the acquisition averaged over S hyper-parameter samples thetas (S, P) (log units, as above) over
 *   the RESIDENT candidates, and the moments of the equal-weight mixture of the S posteriors.  For k = 0 .. S-1 in order:
 *   tgp_fit at theta_k, the unpruned predict-only sweep in the handle's dtype (the pruned sweep's bounds belong to a single
 *   model's arg-max), and -- in float64 whatever the dtype -- the sums of acq(mu_k, sigma_k), mu_k and sigma_k^2 + mu_k^2
 *   per candidate (csrc/integrate_kernels.hip).  Then
 *     acq_out = sum_k acq_k / S;   mu = sum_k mu_k / S;   sigma = sqrt(max(0, sum_k (sigma_k^2 + mu_k^2) / S - mu^2))
 *   and best_val / best_idx the arg-max of acq_out under the library-wide rule (lowest index on ties, NaN never wins; left
 *   untouched with TGP_ACQ_NONE = moments only).  What replaces S x (acq(random_x) + the argsort of
 *   turbo/modules/auxiliary_optimisers.py:59-66) and a NumPy mean in a caller's loop.
 *   acq: TGP_ACQ_UCB / PI / EI / SIGMA / NONE; TGP_ACQ_MES is TGP_BAD_ARG (its maxima belong to one fit).  `incumbent` is
 *   in raw y units and the same for every sample.  n_clamped is the sum over the samples.  A winner record attached with
 *   tgp_set_winner_out is packed as by tgp_sweep (and tgp_winner_wait orders another stream behind it).  The candidates
 *   must be resident for this D (TGP_BAD_ARG otherwise).  TGP_NOT_PD at a sample fails the call with that status and
 *   names k in tgp_last_error.  The handle ends fitted at theta_{S-1}.  GPU only: TGP_BAD_ARG on host handles. */
int tgp_hyper_sample(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                     const double *theta0, int64_t n_ls, const double *log_lo, const double *log_hi,
                     double jitter, int normalize_y, int64_t S, int64_t burn, int64_t thin,
                     const double *width, uint64_t seed, double *theta_out, double *lml_out,
                     int64_t *evaluations, int64_t *not_pd);
int tgp_sweep_integrated(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                         const double *thetas, int64_t S, int64_t n_ls, double jitter, int normalize_y,
                         int acq, double sf, double incumbent, double param,
                         double *mu, double *sigma, double *acq_out,
                         double *best_val, int64_t *best_idx, int64_t *n_clamped);

/* The knowledge gradient (Frazier, Powell & Dayanik 2009) over the RESIDENT candidates, against a discretisation set
 * Xa (A, D), 1 <= A <= 256: the one acquisition here that needs the posterior covariance between every candidate and
 * other points.  With the fitted model in normalised units (c the constant, u = x / l, K = c k0(X, X) + (noise + jitter) I):
 *   mu(.)     raw posterior mean, y_mean + y_std c k0(., X) alpha
 *   C(a, x)   raw LATENT posterior covariance, y_std^2 (c k0(a, x) - c k0(a, X) K^-1 c k0(X, x))
 *   v(x)      raw latent variance, max(sigma(x)^2 - noise y_std^2, 0), sigma the sweep's own (TGP_ACQ_MES's sigma_f^2)
 *   s(x)^2    v(x) + (noise + jitter) y_std^2: the deviation of the OBSERVATION a refit would condition on
 *   lines     i < A: a_i = sf mu(Xa_i), b_i = C(Xa_i, x) / s(x);   i = A (x itself): a_A = sf mu(x), b_A = v(x) / s(x)
 *   KG(x)     E_Z[max_i (a_i + b_i Z)] - max_i a_i, Z ~ N(0, 1): raw units, >= 0; 0 where s(x)^2 <= 0 or not finite
 * -- what a literal refit on (X + {x}, y + {mu(x) + s(x) Z}) predicts at Xa and x, with the hyper-parameters, the jitter,
 * y_mean and y_std held (tgp_sweep_batch's conditioning rule).  KG(x) is evaluated in the cancellation-free form: over the
 * upper envelope's consecutive lines KG = sum (b_next - b_i) f(-|c_i|), c_i = (a_i - a_next) / (b_next - b_i),
 * f(z) = phi(z) + z Phi(z) through the scaled complementary error function TGP_ACQ_MES uses; of lines with equal slope only
 * the one with the largest intercept counts.  Finite for every finite input; may underflow to exactly 0.
 *   tgp_kg_set_points  stores in the handle, on the device and always in float64: the scaled points, mu(Xa) (mu_out (A),
 *                      nullable) and W = K^-1 c k0(X, Xa) as (Apad, Np) rows, Apad = A in whole 128s.  Like the MES maxima
 *                      the points belong to ONE fit: any later fit, append, factor import or state import drops them.
 *                      Non-finite Xa or A outside [1, 256]: TGP_BAD_ARG; no model: TGP_NOT_FITTED.  Duplicates are legal.
 *                      Device memory kept: 3 Apad Np + Apad (Dp + 1) + A D doubles.
 *   tgp_sweep_kg       (1) the unpruned predict-only sweep in the handle's arithmetic (its clamp count is n_clamped);
 *                      where that arithmetic is not float64 the MEAN is re-formed in float64 from step (2)'s cross-kernel
 *                      (y_mean + y_std Ks alpha, one wave a candidate, fixed order) and is what the lines and `mu` hold;
 *                      sigma, and with it v(x), stays the sweep's own;
 *                      (2) per chunk of candidates C = y_std^2 (c k0(Xc, Xa) - Ks W^T) in float64 on v_mfma_f64_16x16x4,
 *                      the sum over the training points in ascending 16-wide tiles whatever M, the chunk or the row;
 *                      (3) per candidate the A + 1 lines and KG(x), one wave a candidate, lines taken in ascending slope;
 *                      (4) the library-wide arg-max (lowest index on ties, NaN never wins), the winner record
 *                      (tgp_set_winner_out / tgp_winner_wait) and the completion of tgp_sweep.
 *                      kg_out (M), mu (M), sigma (M), cov_out (M, A) = C(Xa_j, x_i) raw and latent; all outputs nullable.
 *                      Without points for the resident fit, without candidates, or sf not +-1: TGP_BAD_ARG.
 * Properties: float64 from step (2) on, whatever the handle's dtype; the same bits from run to run; on float64 handles a
 * candidate's kg_out and cov_out bits depend neither on M, nor on its row index, nor on the chunk it falls in (no atomics on
 * floating-point data, no split of a sum).  The call leaves the fit, the candidates, a Thompson draw, the MES maxima and
 * later tgp_sweep results untouched.  Every fitted GPU handle is served: the one-workgroup fits, 128 < N <= 256, the
 * blocked fit, an appended fit, a received factor.  GPU only: TGP_BAD_ARG on host handles for both entries.  The chunk's
 * workspace (rows (Np + Dp + Apad + 1) doubles, rows <= 16384 candidates or TGP_CHUNK) is grown on first use and released with
 * the handle.  tgp_last_timings slot [20] holds the device time of the call's own kernels. */
int tgp_kg_set_points(tgp_handle h, const double *Xa, int64_t A, double *mu_out);
int tgp_sweep_kg(tgp_handle h, double sf, double *kg_out, double *mu, double *sigma, double *cov_out,
                 double *best_val, int64_t *best_idx, int64_t *n_clamped);

/* The knowledge gradient AND its gradient w.r.t. the query point at m <= 4096 points Xq (m, D), in closed form and in
 * float64 whatever the handle's dtype: val (m) is tgp_sweep_kg's kg_out for the same point (same lines, same envelope
 * order: ascending slope, of equal slopes the largest intercept), grad (m, D) its derivative.  Notation as above.  Let the
 * upper envelope, left to right, be the lines j_0 .. j_n-1 with breakpoints -inf = z_0 < z_1 < .. < z_n = +inf, line j_k the
 * maximum on (z_k, z_k+1), P_k = Phi(z_k+1) - Phi(z_k), E_k = phi(z_k) - phi(z_k+1).  By the envelope theorem the
 * breakpoints' own derivatives cancel, and a line leaving the envelope takes P_k, E_k -> 0 with it (KG is C1 there):
 *   grad KG(x) = sum_k E_k grad b_jk(x) + sf grad mu(x) ([A on the envelope] P_A - [a_A > max_{i<A} a_i])
 *   grad b_i = grad C(Xa_i, x) / s - C(Xa_i, x) grad s / s^2 (i < A),  grad b_A = grad v / s - v grad s / s^2,  grad s = grad v / (2 s)
 *   grad_d C(Xa_i, x) = y_std^2 (d_d c k0(x, Xa_i) - sum_j d_d c k0(x, X_j) W_ji),  d_d c k0(x, X_j) = -c h(r_j) (u_d - xs_jd) / l_d
 * (h as in the LML gradient and tgp_acq_grad; grad mu and grad v are tgp_acq_grad's).  With e_i = E_k / s for i = j_k < A the
 * training points' part is ONE reduction per (point, dimension), sum_j omega_j c h_j (u_d - xs_jd) / l_d, against
 *   omega = c_mu alpha + c_v K^-1 k(x) + y_std^2 sum_k e_jk W_jk
 * -- the sum a gather of the few rows of W the envelope holds, not a dense product -- plus the prior term
 * y_std^2 sum_k e_jk d_d c k0(x, Xa_jk) over the same lines.  Conventions:
 *   the only kink lies where a_A crosses max_{i<A} a_i; the indicator is a STRICT >: at a tie the derivative is the one-sided
 *     one of "the candidate's line is not the maximum".  Where it is the maximum, P_A - 1 is never formed: the term is
 *     -(Phi(z_lo) + Phi(-z_hi)), the two tails outside the line's interval, through the scaled complementary error function;
 *   dead points (s^2 <= 0 or not finite, a non-finite mean): value 0 and gradient 0, as tgp_sweep_kg's value;
 *   a clamped latent variance: grad v = 0 and b_A = 0;
 *   h(0) = 0 for Matern-1/2 as everywhere: a query ON a discretisation or training point takes part with a zero kernel
 *     derivative (for the other kernels h(0) (u - xs) is zero anyway).
 * The posterior the lines are formed from is the predict-only sweep's of these m points wherever that sweep runs in
 * float64 -- every float64 handle, and the one-workgroup / one-launch sizes of the others -- so that val is tgp_sweep_kg's
 * kg_out bit for bit; elsewhere mu and sigma are formed in float64 from the query vectors (never the float32 sweep's).
 * Kernels: the query front of tgp_acq_grad (x / l, c k0, c h, K^-1 k on the matrix cores), the cross-covariance of
 * tgp_sweep_kg's step (2), the envelope walk with its record, omega, the (point, dimension) reductions.  No atomics on
 * floating-point data, no split sums, every order fixed: a point's value and gradient bits depend neither on m, nor on its
 * row, nor on what travels with it, and are the same from run to run.
 *   Needs a fitted GPU handle with points set for the resident fit (else TGP_BAD_ARG; no model: TGP_NOT_FITTED; a host
 *   handle: TGP_BAD_ARG); sf not +-1, m outside [1, 4096] or a non-finite Xq: TGP_BAD_ARG.  Leaves the fit, the resident
 *   candidates, the winner record, a Thompson draw, the MES maxima and later tgp_sweep / tgp_sweep_kg results untouched.
 *   Serves every fitted GPU handle tgp_sweep_kg serves.  tgp_last_timings slot [20]: the device time of its own kernels
 *   (the predict-only sweep in front of them and the copies left out).
 * tgp_kg_lbfgsb is tgp_acq_lbfgsb with KG as the objective: the same L-BFGS-B walks in lock-step, one batched tgp_kg_grad
 * per round; arguments, outputs and checks as tgp_acq_lbfgsb's, without the acquisition's. */
int tgp_kg_grad(tgp_handle h, const double *Xq, int64_t m, double sf, double *val, double *grad);
int tgp_kg_lbfgsb(tgp_handle h, const double *X0, int64_t R, const double *lo, const double *hi, double sf,
                  int64_t max_iter, double *x_out, double *val_out, int64_t *status_out, int64_t *evaluations);

/* ---- learned input warping (Snoek, Swersky, Zemel, Adams, ICML 2014) -----------------------------------------------
 * Every input dimension goes through a monotone map of the unit interval, the Kumaraswamy CDF, whose two shape parameters
 * are learned with the kernel's hyper-parameters from the same marginal likelihood: a warped model is an ordinary fit on
 * w(X), its sweep an ordinary sweep over w(Xc).  Per dimension d, with the box [lo_d, hi_d] and shapes a_d, b_d > 0:
 *   u = clip((x - lo) / (hi - lo), 0, 1),   w = 1 - (1 - u^a)^b,   evaluated as -expm1(b log(1 - u^a)) with
 *   log(1 - u^a) = log1p(-exp(a log u)) up to u^a = 1/2 and log(-expm1(a log u)) above (csrc/warp_math.hpp: one header
 *   for the device kernels and the host backend).  u = 0 gives 0 and u = 1 gives 1 exactly; a == 1 and b == 1 give w = u
 *   exactly, a plain rescale to the unit cube.
 *   dw/du = a b u^(a-1) (1-u^a)^(b-1),   dw/da = b (1-u^a)^(b-1) u^a log u,   dw/db = -(1-u^a)^b log(1-u^a);
 *   dw/da and dw/db are 0 at both endpoints (their limit); dw/du at u = 0 with a < 1 and at u = 1 with b < 1 is +inf and
 *   is returned as such.   Inverse: u = (1 - (1 - w)^(1/b))^(1/a).
 * All of it is float64 whatever the handle's dtype.
 *
 * tgp_fit_input_grad is tgp_fit_grad (same arguments, same `grad`) plus dX (N, D) = d LML / d X in RAW X units:
 *   d LML / d x_id = -(c / l_d) sum_{j != i} G_ij h_ij (s_id - s_jd),   s = x / l,  G = alpha alpha^T - K^-1,
 *   h the length-scale weight of tgp_fit_grad (dK_ij / dlog l_d = c h_ij (s_id - s_jd)^2); a pair with d2 = 0 (the diagonal,
 *   a duplicated training row) contributes nothing, under Matern-1/2 too.  So sum_i dX[i][d] = 0 and
 *   sum_i x_id dX[i][d] = -d LML / d log l_d.  It is what any parametric input transform differentiates through.
 *   The fit takes the BLOCKED route for every N, as tgp_fit_loo_grad does and for its reason (the pass reads K^-1 from the
 *   workspace only that route's gradient fills): `lml` and `grad` are byte for byte tgp_fit_grad's under TGP_SMALL=0.  One
 *   pass over the lower triangle of 64 x 64 tiles; nothing N x N is written, no atomics, every sum in a fixed order: the
 *   same bits from run to run.  dX may be NULL: the call is then tgp_fit_grad on that route.  N = 1 gives zeros.  GPU only:
 *   a host handle answers TGP_BAD_ARG.  The model is left fitted.  Status as tgp_fit_grad.
 *   Memory: the pass keeps ceil(N / 64) N Dp doubles of partial sums (Dp = D rounded up to 4) in a workspace of the handle's
 *   that only grows, like the fit's: 64 MiB at N = 4096, D = 32; 1 GiB at N = 16384, D = 32; 16 GiB at N = 65536, D = 32 --
 *   an allocation that fails answers TGP_HIP_ERROR with the fit intact.
 *
 * tgp_warp_points: w_out (m, D) = w(X) for host points X (m, D) and, where the pointers are non-NULL, dw_du, dw_da, dw_db
 *   (m, D each; dw/dx = dw_du / (hi - lo)).  A GPU handle runs the device kernel, a TGP_DEVICE_HOST handle (and
 *   libturbogp_host.so) the same header on the host.  Needs no fitted model.  m < 1, D outside [1, 4096], a box without
 *   hi > lo (finite), an a or b that is not finite and > 0, a NULL X / w_out / lo / hi / a / b: TGP_BAD_ARG.
 * tgp_warp_inverse: x_out (m, D) = lo + u(W) (hi - lo), the closed-form inverse, W clipped to [0, 1]; host arithmetic on
 *   every handle (m is the gradient stage's few results).  Arguments checked as tgp_warp_points'.
 *
 * tgp_warp_candidates warps the RESIDENT batch, however it got there (uploaded, a borrowed device pointer, generated, LHS,
 *   the MT19937 stream), on the device: the result goes into a library-owned buffer that BECOMES the resident batch, so
 *   from the next call on every entry that reads the resident batch -- the sweeps, tgp_sweep_topk, the batch entries,
 *   tgp_read_candidates, tgp_get_candidate, the winner record's row -- sees the warped rows exactly as if the caller had
 *   handed them to tgp_set_candidates_dev.  A borrowed buffer is never written to.  The raw rows are kept as a copy of the
 *   library's own and stay readable through tgp_warp_read_raw(first, count, out) until the next call that makes another
 *   batch resident (tgp_set_candidates*, tgp_gen_candidates*, tgp_set_candidates_mt19937, tgp_evaluate, a fit with
 *   another D), which drops both; tgp_warp_read_raw then answers TGP_BAD_ARG.  A second tgp_warp_candidates without a
 *   new batch warps the RAW rows again with the new parameters (a hyper-parameter fit changes a and b between trials
 *   while a prefetched batch may stay).  A row's bits depend neither on M nor on the row's position, and equal what
 *   tgp_warp_points gives for that row on the same handle (one kernel serves both).  D is the resident model's.  GPU
 *   only; no resident batch or a bad box or shape: TGP_BAD_ARG.
 *   Memory: the warped rows and the raw copy are 2 M D doubles of the handle's own, grow-only and kept for the next batch
 *   after the warp is dropped (as the owned candidate buffer is); tgp_destroy releases them.
 *
 * tgp_fit_warp_grad warps X (N, D) on the device, fits on w(X) as tgp_fit_input_grad does, and returns `grad` with
 *   2 + n_ls + 2 D entries: tgp_fit_grad's layout, then d LML / d log a_0..D-1, then d LML / d log b_0..D-1, by the chain rule
 *   d LML / d log a_d = a_d sum_i (d LML / d w(X)_id) (dw/da)(u_id), i = 0, 1, ... per thread and a fixed tree (one small
 *   kernel).  The length scales are in WARPED units.  `lml` and the first 2 + n_ls entries are byte for byte what
 *   tgp_fit_input_grad returns when handed tgp_warp_points' own output as X: the composite is the composition of its parts.
 *   The handle is left fitted on w(X), ready to sweep a warped batch.  GPU only.
 *
 * tgp_fit_warp_lbfgsb is tgp_fit_lbfgsb over theta' = [log constant, log ls.., log noise, log a_0.., log b_0..], P' =
 *   2 + n_ls + 2 D entries per start (theta0 (S, P'), log_lo / log_hi (P'), theta_out (S, P')): the same L-BFGS-B walk, free
 *   mask (log_lo == log_hi fixes an entry), worker handles, thread rule and TGP_NOT_PD rule, every evaluation a
 *   tgp_fit_warp_grad in the box lo / hi (D each).  prior_sigma > 0 adds sum over the FREE warp entries of
 *   theta^2 / (2 prior_sigma^2) to the minimised objective and its gradient -- a log-normal prior centred on the identity
 *   warp; 0: none.  f_out (S) is the MINIMISED OBJECTIVE at theta_out, -LML plus that penalty, not -LML alone.  The
 *   caller's handle is left as the last evaluation that ran on it left it (with several starts: untouched) -- fit at
 *   the chosen theta afterwards. */
int tgp_fit_input_grad(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y,
                       int kernel, double constant, const double *ls, int64_t n_ls,
                       double noise, double jitter, int normalize_y,
                       double *lml, double *y_mean, double *y_std, double *grad, double *dX);
int tgp_warp_points(tgp_handle h, const double *X, int64_t m, int64_t D, const double *lo, const double *hi,
                    const double *a, const double *b, double *w_out, double *dw_du, double *dw_da, double *dw_db);
int tgp_warp_inverse(tgp_handle h, const double *W, int64_t m, int64_t D, const double *lo, const double *hi,
                     const double *a, const double *b, double *x_out);
int tgp_warp_candidates(tgp_handle h, const double *lo, const double *hi, const double *a, const double *b);
int tgp_warp_read_raw(tgp_handle h, int64_t first, int64_t count, double *out);
int tgp_fit_warp_grad(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y,
                      int kernel, double constant, const double *ls, int64_t n_ls,
                      double noise, double jitter, int normalize_y,
                      const double *lo, const double *hi, const double *a, const double *b,
                      double *lml, double *y_mean, double *y_std, double *grad);
int tgp_fit_warp_lbfgsb(tgp_handle h, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                        const double *lo, const double *hi, const double *theta0, int64_t S, int64_t n_ls,
                        const double *log_lo, const double *log_hi, double prior_sigma, double jitter,
                        int normalize_y, int64_t max_iter, double *theta_out, double *f_out,
                        int64_t *status_out, int64_t *evaluations);

/* ---- constrained and cost-aware acquisition ----------------------------------------------------------------------
 * Scoring a candidate under SEVERAL models at once: the objective's EI / PI multiplied by the probability that every
 * constraint model is satisfied (Gardner et al. 2014; Gelbart, Snoek & Adams 2014) and divided by a predicted cost ("EI per
 * second", Snoek, Larochelle & Adams 2012, section 3.2: a GP on the LOG of the cost).  The reference has neither; its
 * objective may return (cost, eval_info) and every listener receives evaluation_finished(trial_num, y, eval_info)
 * (turbo/optimiser.py:243-256), which is where the plugin turbo_amd.Constrained collects the side values from.
 * `h` is the objective's fitted GPU handle with a resident batch of M rows; sides[0..K), 0 <= K <= 8, each name another
 * fitted GPU handle `g` on the same device with the same D (any dtype, kernel, N, training inputs and fit path; `h` itself
 * and a handle named twice are TGP_BAD_ARG).  With mu_k, sigma_k what g_k's own unpruned predict-only sweep reports for a
 * row, in raw units, and everything below in float64 whatever the dtypes:
 *   TGP_SIDE_GE    log f_k = log Phi(z_k), z_k = (mu_k - level) / sigma_k         the side's value should be >= level
 *   TGP_SIDE_LE    the same with z_k = (level - mu_k) / sigma_k
 *                  sigma_k == 0: a step function, log f_k = 0 where the inequality holds (equality included), else -inf
 *   TGP_SIDE_COST  log f_k = -mu_k: the side models the log of a cost; level must be 0
 *   logw   = sum_k log f_k, summed in the order k = 0, 1, ...
 *   a      = the objective's unweighted acquisition (acq_out)
 *   value  = a exp(logw) for TGP_ACQ_EI / TGP_ACQ_PI, exactly 0 where a == 0 or logw == -inf;
 *            logw itself for TGP_ACQ_NONE: the pure feasibility search of Gelbart et al. before any feasible observation
 *            exists, kept in logs so that the order survives underflow.  UCB, SIGMA and MES are TGP_BAD_ARG: a weight on a
 *            signed or entropy-valued acquisition has no meaning here.
 * log Phi goes through the scaled complementary error function (csrc/weight_math.hpp, the route of TGP_ACQ_MES): finite for
 * every finite z whose square is finite, so a 1e-400 feasibility still orders the candidates.  A NaN in any mu or sigma
 * makes the row's value NaN, and such a row never wins.
 * tgp_sweep_weighted
 *   makes every g_k's resident batch a device-to-device COPY of h's M x D rows, owned by g_k (nothing is borrowed across
 *   handles; a buffer g_k had borrowed with tgp_set_candidates_dev is released, never written): afterwards g_k behaves
 *   exactly as after tgp_set_candidates with those rows.  h's fit, batch, Thompson draw, MES maxima and KG points are
 *   untouched.  A batch on h that was warped with tgp_warp_candidates is TGP_BAD_ARG (each model would need its own warp).
 *   The call enqueues the K side sweeps, the accumulation behind each, the objective's sweep -- the unpruned one: the pruned
 *   sweep's bounds belong to the unweighted arg-max, as for tgp_sweep_integrated -- and the final step, and waits once, at
 *   the end; handles on private streams (tgp_set_private_stream) are ordered with events.
 *   mu, sigma, acq_out, logw_out, value_out (M) and side_mu, side_sigma (K, M): nullable host outputs; mu / sigma /
 *   side_mu / side_sigma are the bits of the same handles' own predict-only tgp_sweep of the same rows.
 *   best_val, best_idx: the arg-max of value under the library-wide rule (lowest index on ties, NaN never wins), for
 *   TGP_ACQ_NONE too; the winner record (tgp_set_winner_out / tgp_winner_wait) is packed as by tgp_sweep.  n_clamped is
 *   the sum over the K + 1 sweeps.
 * tgp_weighted_grad
 *   value (val, as defined above) and its gradient (grad (m, D)) at m <= 4096 host points Xq, formed from every handle's
 *   value-with-partials -- mu, sigma and their gradients from the query kernels behind tgp_acq_grad; where a handle's
 *   sweep of the points runs in f64 (every f64 handle, the one-workgroup and one-launch kernels of any handle) the VALUES
 *   mu and sigma are that sweep's own bits, so val is what tgp_sweep_weighted returns for the same rows, as tgp_kg_grad
 *   does for tgp_sweep_kg -- without a division by a quantity that can underflow:
 *     EI / PI:  grad = (prod f) grad a + a sum_k (prod_{j != k} f_j) grad f_k,   NONE:  sum_k (phi / Phi)(z_k) grad z_k
 *   summed in the order k = 0, 1, ...; a step-function side contributes no gradient.  A point's bits depend neither on m
 *   nor on its row.  The resident batches are not touched.
 * tgp_weighted_lbfgsb
 *   tgp_acq_lbfgsb (below) with that evaluation: its arguments with (sides, K) after h, its contract, statuses and limits.
 * Status: TGP_NOT_FITTED for an unfitted handle; TGP_BAD_ARG for a host handle, another device, another D, a duplicate
 * side or g == h, K outside [0, 8], an unknown kind, a non-finite level, a cost side with level != 0, sf not +-1, no
 * candidates on h; tgp_last_error names the side's index.
 * Out of scope: pruning the objective's sweep under weights, batch selection (the tgp_sweep_batch entries) under weights,
 * the sharded multi-GPU route, warped or marginalised sides, band constraints on one model, a host backend. */
enum tgp_side_kind { TGP_SIDE_GE = 0, TGP_SIDE_LE = 1, TGP_SIDE_COST = 2 };
typedef struct tgp_side { tgp_handle g; int32_t kind; int32_t reserved; double level; } tgp_side;
int tgp_sweep_weighted(tgp_handle h, const tgp_side *sides, int64_t K, int acq, double sf, double incumbent, double param,
                       double *mu, double *sigma, double *acq_out, double *logw_out, double *value_out,
                       double *side_mu, double *side_sigma, double *best_val, int64_t *best_idx, int64_t *n_clamped);
int tgp_weighted_grad(tgp_handle h, const tgp_side *sides, int64_t K, const double *Xq, int64_t m, int acq, double sf,
                      double incumbent, double param, double *val, double *grad);
int tgp_weighted_lbfgsb(tgp_handle h, const tgp_side *sides, int64_t K, const double *X0, int64_t R, const double *lo,
                        const double *hi, int acq, double sf, double incumbent, double param, int64_t max_iter,
                        double *x_out, double *val_out, int64_t *status_out, int64_t *evaluations);

/* ---- two-objective expected hypervolume improvement (EHVI) --------------------------------------------------------
 * Two competing objectives and a Pareto front: the expected growth of the area the front dominates over a reference
 * point, under two INDEPENDENT GPs -- an exact closed form, a sum over the P + 1 strips of the front (Emmerich, Giannakoglou
 * & Naujoks 2006; the strip form of Emmerich, Yang, Deutz, Wang & Fonseca 2016).  The reference has no second objective; the
 * plugin turbo_amd.EHVI collects it from eval_info as turbo_amd.Constrained collects its side values.
 * `h` is objective 1's fitted GPU handle with a resident batch of M rows, `g` objective 2's, on the same device with the
 * same D (any dtype, kernel, N, training inputs and fit path).  Each has a direction sf_j in {+1, -1}, +1 = maximise as
 * everywhere in the library.  Everything below is float64 whatever the dtypes.  In the oriented coordinates u_j = sf_j y_j:
 *   r = (sf_1 ref_1, sf_2 ref_2) is the reference point; the front is the set of non-dominated observed pairs with
 *   u_1 > r_1 and u_2 > r_2, sorted by u_1 ascending (u_2 is then strictly descending): (u_1^(i), u_2^(i)), i = 1 .. P,
 *   0 <= P <= 256.  Breakpoints a_0 = r_1, a_i = u_1^(i), a_{P+1} = +inf; levels c_i = u_2^(i+1) for i < P, c_P = r_2.
 * With (mu_j, sigma_j) the raw-unit posterior the handle's own unpruned predict-only sweep reports for the row, m_j = sf_j mu_j:
 *   e_j(t) = sigma_j H((m_j - t) / sigma_j),  H(z) = phi(z) + z Phi(z);   sigma_j == 0: max(m_j - t, 0);   e_j(+inf) = 0
 *   EHVI   = sum_{i = 0 .. P} max(e_1(a_i) - e_1(a_{i+1}), 0) e_2(c_i),   summed in the order i = 0, 1, ...
 * the expectation of sum_i (min(V_1, a_{i+1}) - a_i)_+ (V_2 - c_i)_+, the improvement of the dominated area.  P = 0: the
 * product e_1(r_1) e_2(r_2) of the two plain EIs at incumbent ref_j, xi = 0.  The partials, z_j(t) = (m_j - t) / sigma_j:
 *   d/dm_1 = sum_i [Phi(z_1(a_i)) - Phi(z_1(a_{i+1}))] e_2(c_i)     d/dsigma_1 = sum_i [phi(z_1(a_i)) - phi(z_1(a_{i+1}))] e_2(c_i)
 *   d/dm_2 = sum_i [e_1(a_i) - e_1(a_{i+1})] Phi(z_2(c_i))          d/dsigma_2 = sum_i [e_1(a_i) - e_1(a_{i+1})] phi(z_2(c_i))
 * every term at t = +inf being 0.  H(z) for z <= 0 goes through the scaled complementary error function
 * (csrc/ehvi_math.hpp, the route of TGP_ACQ_MES and of the weighted entries), never as phi + z ndtr(z) with the two tails
 * formed separately.  H leaves the double range near z = -38.4: such a candidate's value is exactly 0 (there is no log
 * form).  A NaN in any mu or sigma makes the row's value NaN, and such a row never wins.
 * tgp_ehvi_set_front
 *   Y (n, 2) raw observed pairs, n >= 0 (Y may be NULL when n == 0); ref: 2 finite raw values.  Every pair that does not
 *   strictly beat ref in both oriented coordinates is dropped, duplicates merge, the non-dominated rest is kept (weak
 *   dominance removes a point; equal u_1 keeps the larger u_2) and sorted (csrc/host_front.hpp, O(n log n)).  The front
 *   is stored on h -- host copy and device breakpoints, with sf and r -- and survives refits, batches and every other
 *   call until the next tgp_ehvi_set_front or tgp_destroy; it needs no fitted model.  Nullable outputs: P_out; front_out,
 *   room for 2 TGP_EHVI_MAX_FRONT doubles, raw units, sorted order; hv_out, the front's dominated area over ref.
 *   TGP_BAD_ARG for a non-finite Y or ref, an sf other than +-1, P > 256: the previous front is untouched.
 * tgp_sweep_ehvi
 *   makes g's resident batch a device-to-device COPY of h's M x D rows, owned by g (nothing is borrowed across handles; a
 *   buffer g had borrowed with tgp_set_candidates_dev is released, never written): afterwards g behaves exactly as after
 *   tgp_set_candidates with those rows.  h's fit, batch, Thompson draw, MES maxima and KG points are untouched.  A batch
 *   on h that was warped with tgp_warp_candidates is TGP_BAD_ARG (each model would need its own warp).  The call enqueues
 *   g's unpruned predict-only sweep on g's stream, orders that stream in front of h's (an event, where g has a private
 *   stream), h's unpruned predict-only sweep, the value kernel and the final step, and waits once, at the end.
 *   mu, sigma, mu2, sigma2, ehvi_out (M): nullable host outputs; mu / sigma / mu2 / sigma2 are the bits of the handles'
 *   own predict-only tgp_sweep of the same rows.  best_val, best_idx: the arg-max of the value under the library-wide
 *   rule (lowest index on ties, NaN never wins); the winner record (tgp_set_winner_out / tgp_winner_wait) is packed as by
 *   tgp_sweep.  n_clamped is the sum of both sweeps.
 * tgp_ehvi_grad
 *   the value and its gradient (grad (m, D)) at m <= 4096 host points Xq, formed from both handles' value-with-partials --
 *   mu, sigma and their gradients from the query kernels behind tgp_acq_grad, each on its own stream and workspace; where
 *   a handle's sweep of the points runs in f64 (every f64 handle, the one-workgroup and one-launch kernels of any handle)
 *   the VALUES mu and sigma are that sweep's own bits, so on such handles val is tgp_sweep_ehvi's ehvi_out for the same
 *   rows, bit for bit:   grad = sf_1 C_m1 grad mu_1 + C_s1 grad sigma_1 + sf_2 C_m2 grad mu_2 + C_s2 grad sigma_2
 *   with the four coefficients the strip sums above.  A model with sigma_j == 0 at the point contributes no sigma term; a
 *   NaN value gives a NaN gradient.  A point's bits depend neither on m nor on its row.  The resident batches are not touched.
 * tgp_ehvi_lbfgsb
 *   tgp_acq_lbfgsb (below) with that evaluation: its contract, statuses and limits (no acq, sf, incumbent, param).
 * Status: TGP_NOT_FITTED for an unfitted handle; TGP_BAD_ARG for no front set on h, g == h, a host handle, another device,
 * another D, a warped batch on h, no candidates.  GPU only: the host-only library does not export these entries.
 * Out of scope: more than two objectives, correlated objectives, a log form below the underflow, pruning either sweep,
 * batch selection under EHVI, the sharded multi-GPU route, warped or marginalised models. */
#define TGP_EHVI_MAX_FRONT 256
int tgp_ehvi_set_front(tgp_handle h, const double *Y, int64_t n, double sf1, double sf2, const double *ref,
                       int64_t *P_out, double *front_out, double *hv_out);
int tgp_sweep_ehvi(tgp_handle h, tgp_handle g, double *mu, double *sigma, double *mu2, double *sigma2,
                   double *ehvi_out, double *best_val, int64_t *best_idx, int64_t *n_clamped);
int tgp_ehvi_grad(tgp_handle h, tgp_handle g, const double *Xq, int64_t m, double *val, double *grad);
int tgp_ehvi_lbfgsb(tgp_handle h, tgp_handle g, const double *X0, int64_t R, const double *lo, const double *hi,
                    int64_t max_iter, double *x_out, double *val_out, int64_t *status_out, int64_t *evaluations);

/* The gradient stage itself on the device: R <= 4096 restarts X0 (R, D) are refined together by a
 * projected L-BFGS (memory 8; a line search that asks for sufficient decrease 1e-4 and the curvature
 * condition 0.9 as L-BFGS-B's does, lengthening a step whose slope is still steep; bounds lo / hi
 * per dimension; stopping rules of SciPy's L-BFGS-B defaults: projected gradient <= 1e-5 or
 * relative reduction <= 2.2e-9) that MAXIMISES the acquisition.  N <= 128 and D <= 64: ONE launch,
 * a workgroup per restart runs its whole optimisation with the model in LDS.  Larger models:
 * every iteration is one batched closed-form value + gradient evaluation (the kernels of
 * tgp_acq_grad) and one optimiser step for all restarts in lock-step, all resident on the GPU.
 * Replaces the loop of scipy.optimize.minimize(method='L-BFGS-B') runs over finite-difference
 * gradients at turbo/modules/auxiliary_optimisers.py:80-99.
 *   x_out (R, D), val_out (R): refined points and their acquisition values (TGP_ACQ_MES: TGP_BAD_ARG, use tgp_acq_lbfgsb)
 *   status_out (R, nullable): 1 converged, 2 no progress from the start point, 0 stopped by max_iter
 *   iterations (nullable): value + gradient evaluations made (by the slowest restart) */
int tgp_acq_refine(tgp_handle h, const double *X0, int64_t R, const double *lo, const double *hi,
                   int acq, double sf, double incumbent, double param, int64_t max_iter,
                   double *x_out, double *val_out, int64_t *status_out, int64_t *iterations);

/* The gradient stage as the reference runs it, inside the library: every restart X0 (R, D), R <= 4096, walked by
 * L-BFGS-B itself (csrc/host_lbfgsb.hpp, SciPy's algorithm and defaults: the optimiser behind
 * scipy.optimize.minimize(method='L-BFGS-B', options=dict(maxiter=15000)) at
 * turbo/modules/auxiliary_optimisers.py:80-99) on the negated acquisition with its closed-form gradient, the
 * restarts in lock-step: one batched value + gradient evaluation (the kernels of tgp_acq_grad) per round serves every
 * restart still running.  Each restart walks what it would walk alone -- a point's value does not depend on the batch
 * it is evaluated in.  Where tgp_acq_refine runs an optimiser of its own on the device (other iterates, one launch for
 * small models), this one reproduces SciPy's walk with no interpreter between two rounds.
 *   max_iter: accepted iterations per restart (SciPy's maxiter)
 *   x_out (R, D), val_out (R): the end points and their acquisition values
 *   status_out (R, nullable): 1 converged (SciPy's success), 0 stopped by max_iter, 2 no acceptable step
 *   evaluations (nullable): value + gradient evaluations over all restarts */
int tgp_acq_lbfgsb(tgp_handle h, const double *X0, int64_t R, const double *lo, const double *hi,
                   int acq, double sf, double incumbent, double param, int64_t max_iter,
                   double *x_out, double *val_out, int64_t *status_out, int64_t *evaluations);

/* One call = tgp_set_candidates + tgp_sweep: what ONE call of the reference's acquisition
 * instance does, acq(X) -> model.predict(X, return_std_dev=True) -> formula
 * (turbo/modules/acquisition_functions.py:152,230,341; surrogates.py:332-338), and what the plot
 * path repeats per stored model on 200 .. 10^4 points (turbo/plotting/trials.py:371,448,574-577).
 * Arguments as tgp_sweep; the batch stays resident afterwards.  For a model of N <= 256 and a batch
 * of up to 8 MB the candidates and results travel through pinned host memory the GPU reads and
 * writes directly: one or two kernel launches (128 < N <= 256: one), one synchronisation, no memcpy. */
int tgp_evaluate(tgp_handle h, const double *Xc, int64_t M, int acq, double sf, double incumbent,
                 double param, double *mu, double *sigma, double *acq_out, double *best_val,
                 int64_t *best_idx, int64_t *n_clamped);

/* Many stored models, one batch of points: what the plot path does when it walks the recorder's
 * trials and predicts the same grid with every trial's model (turbo/plotting/trials.py:371,448,
 * 574-577; turbo/plotting/surrogates.py:23-24,61-65).  Each of the T models is given by what
 * defines it -- X_t (N_t, D), y_t, hyper-parameters -- with N_t <= 256; all share the kernel kind,
 * D and normalize_y.  The T fits run as ONE launch of T workgroups, the T sweeps as one launch
 * (a batch whose largest model has more than 128 points runs every model of it on the kernels of
 * 128 < N <= 256: group the models by size for the faster small-problem kernels); the handle's
 * resident model, if any, is not touched.
 *   ls (T, D) row-major (broadcast an isotropic length scale); mu, sigma (T, M) row-major
 *   (sigma, lml nullable); n_clamped: total over the batch.
 * TGP_NOT_PD names the failing model in tgp_last_error. */
int tgp_predict_batch(tgp_handle h, int64_t T, const int64_t *Ns, int64_t D, const double *const *Xs,
                      const double *const *ys, int kernel, const double *constants, const double *ls,
                      const double *noises, const double *jitters, int normalize_y, const double *Xc,
                      int64_t M, double *mu, double *sigma, double *lml, int64_t *n_clamped);

/* Convenience = tgp_evaluate(TGP_ACQ_NONE): ModelInstance.predict
 * (turbo/modules/surrogates.py:332-338). */
int tgp_predict(tgp_handle h, const double *Xc, int64_t M, double *mu, double *sigma);

/* ---- one process, several GPUs ------------------------------------------------------------ */

/* The sharded candidate sweep of one node behind the C-ABI (across processes the
 * Python side does the same with torch.distributed / RCCL).  A tgp_multi owns one tgp_handle per
 * listed device and drives each from its own host thread:
 *   tgp_multi_fit             tgp_fit replicated on every device (identical inputs -> identical
 *                             factor, checked; no exchange)
 *   tgp_multi_set_candidates  contiguous shards of ceil(M / n) rows of the (M, D) host batch
 *   tgp_multi_gen_candidates  every device draws its rows of the one Philox stream (tgp_gen_candidates)
 *   tgp_multi_sweep           tgp_sweep on every shard at once; the winners are reduced with the
 *                             library-wide rule (largest value, lowest GLOBAL index, NaN never wins):
 *                             best_val, best_idx (global), best_row (D, nullable), acq_out (M, nullable).
 *                             = the argsort()[0] of turbo/modules/auxiliary_optimisers.py:63-66 over
 *                             the whole batch.
 * Errors as for the single-device calls; tgp_multi_last_error names the device.  The same device
 * may be listed more than once (each entry gets its own context and stream). */
typedef struct tgp_multi_s *tgp_multi;
int tgp_multi_create(int n, const int *device_ids, int dtype, tgp_multi *out);
int tgp_multi_destroy(tgp_multi m);
const char *tgp_multi_last_error(tgp_multi m);
int tgp_multi_size(tgp_multi m);
int tgp_multi_handle(tgp_multi m, int i, tgp_handle *out);
int tgp_multi_fit(tgp_multi m, const double *X, int64_t N, int64_t D, const double *y, int kernel,
                  double constant, const double *ls, int64_t n_ls, double noise, double jitter,
                  int normalize_y, double *lml, double *y_mean, double *y_std);
int tgp_multi_set_candidates(tgp_multi m, const double *Xc, int64_t M);
int tgp_multi_gen_candidates(tgp_multi m, uint64_t seed, int64_t M, const double *lo, const double *hi);
int tgp_multi_sweep(tgp_multi m, int acq, double sf, double incumbent, double param, double *best_val,
                    int64_t *best_idx, double *best_row, double *acq_out);

/* Handles of one device share one stream (see the conventions above).  A handle switched to a
 * private stream (on != 0) submits to a stream of its own instead, so calls made on several such
 * handles from several host threads overlap on the GPU -- what HipGPSurrogate uses to run the
 * restarts of the hyper-parameter fit (sklearn _gpr.py:326-337) side by side above N = 128, where a
 * single evaluation leaves most of the chip idle.  Synchronises the handle's current stream. */
int tgp_set_private_stream(tgp_handle h, int on);

/* The device's pool of WORKER handles (round 5): handles on private streams that run the concurrent starts of a
 * hyper-parameter fit above the one-launch sizes (sklearn _gpr.py:326-337, n_restarts_optimizer; reached from
 * turbo/modules/surrogates.py:313-318) -- in the library's own threads (tgp_fit_optimise) or in the host's
 * (HipGPSurrogate drives tgp_fit_grad on them with SciPy).  ONE pool per device whatever the number of handles and
 * factories in the process, at most four workers: the HIP runtime deals a process's streams onto a fixed number of
 * hardware queues and two streams on one queue run one after the other (a second factory with workers of its own
 * doubled the time of a hyper-parameter fit in round 4).
 *   tgp_workers_acquire   out[0..n) = n worker handles (1 <= n <= 4) of h's device, created on demand; the pool is
 *                         LOCKED for the calling thread until tgp_workers_release (one hyper-parameter fit at a time per
 *                         device; a second caller blocks).  The workers accept every call a handle accepts except
 *                         tgp_destroy and tgp_workers_*; they belong to the library and live until the last handle
 *                         made by tgp_create on that device is destroyed.
 *   tgp_workers_release   unlocks the pool; must be called by the thread that acquired it (TGP_BAD_ARG otherwise; a
 *                         second acquire by the thread that holds the pool is refused the same way instead of deadlocking). */
int tgp_workers_acquire(tgp_handle h, int n, tgp_handle *out);
int tgp_workers_release(tgp_handle h);

/* Fit and sweep overlapped (round 5).  The reference runs them back to back -- turbo/optimiser.py:336-340:
 * construct_model, then the acquisition's maximisation over ONE vectorised batch
 * (turbo/modules/auxiliary_optimisers.py:59-66) -- and so does this library, call by call.  But the batch does not
 * depend on the model: when the candidates of the NEXT sweep are already resident (tgp_set_candidates[_dev],
 * tgp_gen_candidates[_lhs]) at the time tgp_fit / tgp_fit_grad is called, the front of that sweep can run INSIDE
 * the fit, beside its latency-bound panel chain, on the device's third stream:
 *   mode 1   the candidates' scaling by the new length scales and the first launch pair's cross-kernel
 *            (needs nothing of the fit but X / length_scale);
 *   mode 2   ... and the contraction of that pair over the row tiles whose rows of L^-1 are already final.
 *   mode 0   (default) nothing: fit and sweep strictly one after the other.
 * tgp_sweep then skips what is done; any call that changes the candidates, the fit or the sweep workspace in between
 * simply discards the front.  Same kernels, same arithmetic and the same order of every sum either way: results are
 * bit-identical to mode 0.  Applies to the general sweep of f64 / f32 handles (N > 256) on the shared streams; a no-op
 * elsewhere.  The environment's TGP_OVERLAP caps the mode for A/B runs.
 * A batch borrowed with tgp_set_candidates_dev is READ during the next tgp_fit once a mode is armed: it has to stay
 * valid (and unchanged) from the arming until the sweep that consumes it, not only during tgp_sweep. */
int tgp_set_overlap(tgp_handle h, int mode);

/* (round 6) What the device's shared streams probed as when they were created (the first tgp_create on the device):
 * out3[0] = 1 when the BACKGROUND stream really runs beside the main one (the inverse factor behind the Cholesky's
 * panel chain), 0 when the runtime put both on one hardware queue -- they then run one after the other and every
 * large fit takes about twice as long --, -1 not probed (TGP_BG_PROBE=0); out3[1] likewise for the THIRD stream
 * (tgp_set_overlap; 0: there is none and the overlap is a no-op); out3[2] = GPU_MAX_HW_QUEUES of the process
 * environment (0: unset).  The HIP runtime deals streams onto 4 hardware queues unless that variable said otherwise
 * BEFORE its first call in the process; turbo_amd/_lib.py sets 8 at import and warns, from this entry, when another
 * library (torch) initialised the runtime first and the probes came back serialised. */
int tgp_stream_status(tgp_handle h, int *out3);
/* Every environment switch (TGP_*) of the library with the value in force in this process, one
 * "NAME=value<TAB># what it selects" line each (csrc/tuning.hpp: the ONE table they are all read from).  Writes at
 * most cap bytes including the terminating 0; returns the size needed (or -1). */
int64_t tgp_tuning(char *buf, int64_t cap);

/* ---- the reference's HOST candidate draw, outside the interpreter ------------------------------ */

/* The batch of the reference's random_selector (turbo/modules/naive_selectors.py:39-46: one
 * np.random.uniform(pmin, pmax, size=(M, 1)) per parameter from NumPy's GLOBAL legacy RNG, hstacked), bit for bit:
 * key624 / pos are MT19937's state words and position as np.random.get_state() returns them; on return they are
 * where NumPy's own D calls would have left them (np.random.set_state) and out (M, D) row-major holds the batch,
 * column c = lo[c] + (hi[c] - lo[c]) * u with u the stream's next M doubles.  Plain host code (no handle, no GPU,
 * in the host-only library too): NumPy spends 66 ms on C3's 262 144 x 32 draw -- twice the GPU step it feeds --
 * this 10-20.  turbo_amd/naive_selectors.py random_selector calls it for large batches. */
int tgp_mt19937_uniform_columns(uint32_t *key624, int32_t *pos, int64_t M, int64_t D, const double *lo,
                                const double *hi, double *out);

/* The same draw made RESIDENT (GPU handles): the stream's words are generated on the host -- the one part that cannot
 * run in parallel -- and copied a column at a time while the next is generated; the GPU forms the doubles and the
 * (rows, D) layout in NumPy's arithmetic.  The resident batch is rows [first_row, first_row + rows) of the M_total-row
 * batch NumPy would have drawn -- a rank's shard of ONE batch: every rank with the same RNG state gets its
 * own rows of the same batch, and key624 / pos end behind the WHOLE batch on all of them (the other rows' words are
 * passed over).  tgp_read_candidates returns those doubles bit for bit; on any failure key624 / pos are untouched.
 * D is the fitted model's.  C3's batch: 2.2 ms instead of 46-66 ms of NumPy + the upload. */
int tgp_set_candidates_mt19937(tgp_handle h, uint32_t *key624, int32_t *pos, int64_t M_total, int64_t first_row,
                               int64_t rows, const double *lo, const double *hi);

/* ---- measurement ------------------------------------------------------------------------ */

/* Turn per-kernel HIP-event timing on/off (on the library's own stream). */
int tgp_profile_enable(tgp_handle h, int on);
/* Totals since the last tgp_profile_reset: launches and milliseconds of the dominant sweep
 * kernel (trmm_sumsq), of the cross-kernel build, and of the whole last fit / sweep. */
int tgp_profile_read(tgp_handle h, int64_t *trmm_launches, double *trmm_ms,
                     int64_t *kstar_launches, double *kstar_ms,
                     double *last_fit_ms, double *last_sweep_ms);
int tgp_profile_reset(tgp_handle h);
/* Device times (ms, hipEvents on the library's stream) of the last calls, first n of:
 * [fit, sweep, LML gradient: K^-1 = U U^T, LML gradient: pairwise weights and traces,
 *  LML gradient: ARD products, (not a time) the algorithmic flops of the contraction launches timed since
 *  tgp_profile_reset: rows^2 per candidate over the rows each launch covered -- the numerator that goes with
 *  tgp_profile_read's trmm_ms when a fit took row tiles of a launch (tgp_set_overlap),
 *  (not a time, round 6) 1 when the last sweep ran in float64 whatever the handle's dtype -- the one-workgroup
 *  kernels for N <= 128 and the one-launch sweep above them only exist in f64 --, 0 when it ran in the handle's
 *  arithmetic, -1 before the first sweep: what CandidateSweep asks before it re-forms the winner's value in f64].
 * The short polled calls (small fit, fit + gradient; doorbell.hpp) report the kernels' own wall_clock64() span;
 * slots [7..11] (a debugging aid) hold that kernel's phase stamps in microseconds from its start: inputs staged,
 * first kernel-matrix tile in LDS, first block factored, fit done, call done (0 when the last fit was not polled).
 * Slots [12..14] (not times): what the last tgp_sweep did about pruning -- -1 not eligible, -2 gated off by the
 * noise, 0 the pruned schedule ran, 1 it fell back to every candidate -- and the candidates of its lb set and its
 * survivors (TGP_SWEEP_PRUNE).
 * Slot [15]: device time (ms) of the kernels of the last tgp_predict_cov / tgp_sample_joint, the copies of its inputs and
 * outputs left out (0 on host handles).
 * Slot [16] (not a time): the candidates that survived the screen in front of the pruned sweep's bound pass (f32 RBF
 * handles, TGP_PRUNE_SCREEN; `survivors` of slot 14 are those that went on to the exact contraction), -1 when the screen
 * did not apply.  Slot [17]: profiled time (ms) of the screen's launches since tgp_profile_reset, kept apart from
 * tgp_profile_read's cross-kernel and contraction times.  Slot [18] (not a time): that screen's arithmetic, 0 none,
 * 1 the f32 matrix pipe, 2 fp16 planes with the k-weighted error (TGP_SCREEN_ARITH).
 * Slot [19]: device time (ms) of the kernels of the last tgp_loo, the copies back left out (0 on host handles).  After
 * tgp_fit_loo_grad slot [2] holds everything up to B = A A^T (K^-1, kappa, b, A, B), slots [3] and [4] as for tgp_fit_grad.
 * Slot [20]: device time (ms) of the last tgp_sweep_kg's own kernels -- cross-covariance and envelope, chunk by chunk; the
 * predict-only sweep in front of them and the copies left out (0 on host handles); after tgp_kg_grad, that call's own
 * kernels likewise.
 * Slot [21] (not a time): the speculative round of the last tgp_sweep's pruned schedule (TGP_PRUNE_SPEC; DESIGN.md section
 * 4) -- 0 not tried, 1 hit: the runner-ups contracted beside the lb set covered every survivor, so the sweep made one exact
 * round; 2 miss: the survivors' round ran as well.  Slots [12..14] and [16] read the same either way. */
int tgp_last_timings(tgp_handle h, double *out, int64_t n);
/* Candidates per trmm launch (chunk) and padded N used by the sweep, for the roofline maths. */
int tgp_sweep_geometry(tgp_handle h, int64_t *chunk, int64_t *n_padded);

#ifdef __cplusplus
}
#endif
#endif /* TURBOGP_H */
