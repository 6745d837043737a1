// api_warp.hpp -- learned input warping in the C-ABI (include/turbogp.h, "learned input warping"), as named steps:
//
//   tgp_fit_input_grad    fit_input_grad:  fit_impl on the blocked route with the LML gradient behind it (tgp_fit_grad under
//                                          TGP_SMALL=0, to the byte), then input_grad_pass over the K^-1 it left in W
//   tgp_warp_points       check_warp_box -> the host backend's loop | warp_points_device
//   tgp_warp_inverse      the host backend's loop on every handle
//   tgp_warp_candidates   check_warp_box -> warp_resident:  the resident rows (or, while a warp is in force, their raw copy)
//                                          through warp_kernel into the library's buffer, which becomes the resident batch
//   tgp_warp_read_raw     the raw copy's rows
//   tgp_fit_warp_grad     warp_training_set -> fit_input_grad on w(X) -> warp_chain:  the composition of the entries above
//   tgp_fit_warp_lbfgsb   check_optimise_args + the warp's own -> warp_optimise_streams:  run_start's sibling warp_run_start
//                                          over tgp_fit_warp_grad, with the LbfgsbWalk, FreeMask, worker handles and thread rule
//                                          of tgp_fit_lbfgsb
//
// NOT a header of its own: tgp_api.hip includes it once behind api_optimise.hpp -- the same translation unit.
#pragma once

struct WarpBox { int64_t D; const double *lo, *hi, *a, *b; };

// Copies queued on c.stream from host memory that dies with the call (the box's vector, w(X)'s vector, the caller's
// arrays): declared BEHIND those vectors and armed when the first copy is queued, it drains the stream on every way out
// that has not drained it itself, so nothing queued ever outlives what it reads or writes
struct StreamDrain {
    Context &c;
    bool armed = false;
    ~StreamDrain() { if (armed) (void)hipStreamSynchronize(c.stream); }
};

static int check_warp_box(Context &c, const char *fn, const WarpBox &w) {
    bool ok = w.lo && w.hi && w.a && w.b && w.D >= 1 && w.D <= 4096;
    for (int64_t d = 0; ok && d < w.D; ++d) ok = warp_params_ok(w.lo[d], w.hi[d], w.a[d], w.b[d]);
    return ok ? TGP_OK : fail(c, TGP_BAD_ARG, std::string(fn) + ": need lo, hi, a, b with 1 <= D <= 4096, hi > lo (finite) and finite a, b > 0");
}

// [lo | hi | a | b] on the device, queued on c.stream (host: at least 4 D doubles that live until the stream is drained)
static int warp_box_to_device(Context &c, const WarpBox &w, double *host, double *dev) {
    const size_t D = (size_t)w.D;
    memcpy(host, w.lo, D * sizeof(double));
    memcpy(host + D, w.hi, D * sizeof(double));
    memcpy(host + 2 * D, w.a, D * sizeof(double));
    memcpy(host + 3 * D, w.b, D * sizeof(double));
    API_HIP(hipMemcpyAsync(dev, host, 4 * D * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D warp box");
    return TGP_OK;
}

// ---- the LML's gradient in the training inputs ----------------------------------------------------------------------
// behind a blocked fit with the LML gradient (K^-1 = U U^T is in d_W): dX (N, D) into c.d_xgout, queued on c.stream
static int input_grad_pass(Context &c) {
    const size_t nt = (size_t)((c.N + PW_T - 1) / PW_T);
    API_MEM(grow(c, c.d_xgpart, nt * (size_t)c.N * (size_t)c.Dp * sizeof(double), "hipMalloc input-gradient partials"));
    API_MEM(grow(c, c.d_xgout, (size_t)c.N * (size_t)c.D * sizeof(double), "hipMalloc input gradient"));
    const hipError_t le = launch_input_grad(c, c.d_xgpart, c.d_xgout);
    return le == hipSuccess ? TGP_OK : hip_fail(c, le, "launch_input_grad");
}

// tgp_fit_grad on the blocked route for every N, and d LML / d X behind it: into dX (host, nullable) and, where dX is given or
// keep_on_device, left in c.d_xgout
static int fit_input_grad(tgp_handle h, const FitArgs &a, const FitOut &out, double *grad, double *dX, bool keep_on_device) {
    Context &c = h->c;
    const bool ard = a.n_ls > 1;
    // the blocked route for every N: the pass needs K^-1 in W, which only that route's gradient leaves
    const int rc = fit_impl(h, a, out, false, ard ? 2 : 1);
    if (rc != TGP_OK) return rc;
    const int nout = ard ? 3 + (int)c.Dp : 3;
    std::vector<double> sums((size_t)(3 + c.Dp), 0.0);
    if (c.grad_staged) {
        memcpy(sums.data(), c.h_pin_out + 8, (size_t)nout * sizeof(double));
    } else {
        API_HIP(hipSetDevice(c.device), "hipSetDevice");
        API_HIP(hipMemcpy(sums.data(), c.d_gout, (size_t)nout * sizeof(double), hipMemcpyDeviceToHost), "D2H grad");
    }
    for (int i = 0; i < 3; ++i) {
        float gms = 0.f;
        if (c.grad_timed) (void)hipEventElapsedTime(&gms, c.evg[i], c.evg[i + 1]);
        c.last_grad_ms[i] = gms;
    }
    lml_grad_from_sums(a, sums.data(), grad);
    if (!dX && !keep_on_device) return TGP_OK;
    API_MEM(input_grad_pass(c));
    StreamDrain drain{c};
    drain.armed = true;
    if (dX) API_HIP(hipMemcpyAsync(dX, c.d_xgout, (size_t)(a.N * a.D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H input gradient");
    API_HIP(hipStreamSynchronize(c.stream), "input gradient sync");
    drain.armed = false;
    return TGP_OK;
}

// ---- the warp at host points ------------------------------------------------------------------------------------------
// c.d_wpts for m points of D dimensions, in doubles
struct WarpPointsWs {
    Packed all;
    size_t par, x, w, du, da, db, sums;
    WarpPointsWs(int64_t m, int64_t D) {
        const size_t n = (size_t)(m * D);
        par = all.take((size_t)(4 * D)); x = all.take(n); w = all.take(n); du = all.take(n); da = all.take(n); db = all.take(n);
        sums = all.take((size_t)(2 * D));
    }
};

static int warp_points_device(Context &c, const double *X, int64_t m, const WarpBox &w, double *w_out, double *dw_du, double *dw_da,
                              double *dw_db) {
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const WarpPointsWs ws(m, w.D);
    API_MEM(grow(c, c.d_wpts, ws.all.bytes(), "hipMalloc warp workspace"));
    double *d = c.d_wpts;
    std::vector<double> par((size_t)(4 * w.D));
    StreamDrain drain{c};
    drain.armed = true;
    API_MEM(warp_box_to_device(c, w, par.data(), d + ws.par));
    const size_t nb = (size_t)(m * w.D) * sizeof(double);
    API_HIP(hipMemcpyAsync(d + ws.x, X, nb, hipMemcpyHostToDevice, c.stream), "H2D points");
    const hipError_t le = launch_warp(c, d + ws.x, m * w.D, (int)w.D, d + ws.par, nullptr, d + ws.w, dw_du ? d + ws.du : nullptr,
                                      dw_da ? d + ws.da : nullptr, dw_db ? d + ws.db : nullptr);
    if (le != hipSuccess) return hip_fail(c, le, "launch_warp");
    API_HIP(hipMemcpyAsync(w_out, d + ws.w, nb, hipMemcpyDeviceToHost, c.stream), "D2H w");
    if (dw_du) API_HIP(hipMemcpyAsync(dw_du, d + ws.du, nb, hipMemcpyDeviceToHost, c.stream), "D2H dw/du");
    if (dw_da) API_HIP(hipMemcpyAsync(dw_da, d + ws.da, nb, hipMemcpyDeviceToHost, c.stream), "D2H dw/da");
    if (dw_db) API_HIP(hipMemcpyAsync(dw_db, d + ws.db, nb, hipMemcpyDeviceToHost, c.stream), "D2H dw/db");
    API_HIP(hipStreamSynchronize(c.stream), "warp sync");
    drain.armed = false;
    return TGP_OK;
}

// ---- the warp of the resident batch -----------------------------------------------------------------------------------
static bool warp_in_force(const Context &c) {
    return c.d_cand != nullptr && c.d_cand == c.d_wcand.get() && c.M == c.warp_M && c.D == c.warp_D && c.M > 0;
}

static int warp_resident(Context &c, const WarpBox &w) {
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const bool again = warp_in_force(c);      // re-warp: from the raw copy, which stays as it is
    const int64_t M = c.M, D = c.D;
    const size_t nb = (size_t)(M * D) * sizeof(double);
    const double *src = again ? c.d_wraw.get() : c.d_cand;
    if (!again) {
        // (c.d_cand is not one of these two: growing them cannot free the rows about to be read)
        API_MEM(grow(c, c.d_wraw, nb, "hipMalloc raw candidates"));
        API_MEM(grow(c, c.d_wcand, nb, "hipMalloc warped candidates"));
    }
    API_MEM(grow(c, c.d_wpar, (size_t)(4 * D) * sizeof(double), "hipMalloc warp box"));
    std::vector<double> par((size_t)(4 * D));
    StreamDrain drain{c};
    drain.armed = true;
    API_MEM(warp_box_to_device(c, w, par.data(), c.d_wpar));
    const hipError_t le = launch_warp(c, src, M * D, (int)D, c.d_wpar, again ? nullptr : c.d_wraw.get(), c.d_wcand, nullptr, nullptr, nullptr);
    if (le != hipSuccess) return hip_fail(c, le, "launch_warp");
    API_HIP(hipStreamSynchronize(c.stream), "warp sync");
    drain.armed = false;
    c.d_cand = c.d_wcand;
    c.warp_M = M; c.warp_D = D;
    return TGP_OK;
}

// ---- fit on w(X) with the gradient in log a, log b --------------------------------------------------------------------
static int fit_warp_grad(tgp_handle h, const FitArgs &a, const WarpBox &w, const FitOut &out, double *grad) {
    Context &c = h->c;
    c.fitted = false;
    API_MEM(check_fit_args(c, a));
    API_MEM(check_warp_box(c, "tgp_fit_warp_grad", w));
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    // warp_training_set: X through the warp on the device; w(X) comes back for the fit's staging (N D doubles), the
    // derivatives in a and b stay
    const WarpPointsWs ws(a.N, a.D);
    API_MEM(grow(c, c.d_wpts, ws.all.bytes(), "hipMalloc warp workspace"));
    double *d = c.d_wpts;
    const size_t nb = (size_t)(a.N * a.D) * sizeof(double);
    std::vector<double> par((size_t)(4 * a.D)), Wx((size_t)(a.N * a.D));
    StreamDrain drain{c};
    drain.armed = true;
    API_MEM(warp_box_to_device(c, w, par.data(), d + ws.par));
    API_HIP(hipMemcpyAsync(d + ws.x, a.X, nb, hipMemcpyHostToDevice, c.stream), "H2D X");
    hipError_t le = launch_warp(c, d + ws.x, a.N * a.D, (int)a.D, d + ws.par, nullptr, d + ws.w, nullptr, d + ws.da, d + ws.db);
    if (le != hipSuccess) return hip_fail(c, le, "launch_warp");
    API_HIP(hipMemcpyAsync(Wx.data(), d + ws.w, nb, hipMemcpyDeviceToHost, c.stream), "D2H w(X)");
    API_HIP(hipStreamSynchronize(c.stream), "warp sync");
    FitArgs aw = a;
    aw.X = Wx.data();
    const int rc = fit_input_grad(h, aw, out, grad, nullptr, true);
    if (rc != TGP_OK) return rc;
    // warp_chain: [d/d log a | d/d log b] behind the model's own entries
    le = launch_warp_chain(c, c.d_xgout, d + ws.da, d + ws.db, d + ws.par, d + ws.sums);
    if (le != hipSuccess) return hip_fail(c, le, "launch_warp_chain");
    API_HIP(hipMemcpyAsync(grad + 2 + a.n_ls, d + ws.sums, (size_t)(2 * a.D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H warp gradient");
    API_HIP(hipStreamSynchronize(c.stream), "warp gradient sync");
    drain.armed = false;
    return TGP_OK;
}

// ---- the hyper-parameter fit over theta' = [log constant, log ls..., log noise, log a..., log b...] --------------------
struct WarpOptArgs { const double *lo, *hi; double prior_sigma; };

// HyperRun over the longer vector: what the starts of one call share
struct WarpRun {
    const HyperOptArgs &a;
    const HyperOptOut &out;
    const WarpOptArgs &w;
    const int P;                           // 2 + n_ls + 2 D
    const FreeMask mask;
    std::vector<int> status, rcs;
    std::vector<int64_t> evals;
    std::vector<std::string> errs;
    WarpRun(const HyperOptArgs &a_, const HyperOptOut &out_, const WarpOptArgs &w_, int T)
        : a(a_), out(out_), w(w_), P((int)(2 + a_.n_ls + 2 * a_.D)), mask(a_.log_lo, a_.log_hi, P), status((size_t)a_.S, 0),
          rcs((size_t)T, TGP_OK), evals((size_t)a_.S, 0), errs((size_t)T) {}
};

// run_start's sibling: start s on handle hw, its walk over tgp_fit_warp_grad; the minimised objective is -LML plus, with
// prior_sigma > 0, sum over the FREE warp entries of theta^2 / (2 prior_sigma^2)
static int warp_run_start(WarpRun &run, int64_t s, tgp_handle hw) {
    const HyperOptArgs &a = run.a;
    const WarpOptArgs &wa = run.w;
    const FreeMask &mask = run.mask;
    const int P0 = (int)(2 + a.n_ls), D = (int)a.D, P = run.P, Pf = mask.Pf;
    std::vector<double> ls((size_t)a.n_ls), grad((size_t)P), th((size_t)P), xt((size_t)Pf), gt((size_t)Pf), wa_((size_t)D), wb_((size_t)D);
    for (int k = 0; k < P; ++k) th[(size_t)k] = HostLbfgsb::clip(a.theta0[s * P + k], a.log_lo[k], a.log_hi[k]);
    mask.gather(th.data(), xt.data());
    LbfgsbWalk walk(xt.data(), mask.lo_f.data(), mask.hi_f.data(), Pf, a.max_iter);
    const double ip = wa.prior_sigma > 0.0 ? 1.0 / (wa.prior_sigma * wa.prior_sigma) : 0.0;
    while (walk.wants_eval()) {
        mask.scatter(walk.xt.data(), th.data());
        double constant, noise, lml = 0.0, phit;
        slice_unpack(th.data(), a.n_ls, constant, ls.data(), noise);
        for (int d = 0; d < D; ++d) { wa_[(size_t)d] = exp(th[(size_t)(P0 + d)]); wb_[(size_t)d] = exp(th[(size_t)(P0 + D + d)]); }
        const int rc = fit_warp_grad(hw, FitArgs{a.X, a.N, a.D, a.y, a.kernel, constant, ls.data(), a.n_ls, noise, a.jitter, a.normalize_y},
                                     WarpBox{a.D, wa.lo, wa.hi, wa_.data(), wb_.data()}, FitOut{&lml, nullptr, nullptr}, grad.data());
        if (rc == TGP_NOT_PD) {            // -inf likelihood, zero gradient (_gpr.py:586-589)
            phit = INFINITY;
            std::fill(gt.begin(), gt.end(), 0.0);
        } else if (rc != TGP_OK) {
            return rc;
        } else {
            phit = -lml;
            mask.gather(grad.data(), gt.data(), -1.0);
            for (int k = 0; k < Pf; ++k) {   // the log-normal prior centred on the identity warp, free warp entries only
                const int p = mask.fr[(size_t)k];
                if (p < P0) continue;
                phit += 0.5 * ip * th[(size_t)p] * th[(size_t)p];
                gt[(size_t)k] += ip * th[(size_t)p];
            }
        }
        if (Pf == 0) {                     // nothing is free: the one evaluation is the answer
            ++walk.evals;
            walk.opt.phi = phit;
            walk.opt.status = 1;
            break;
        }
        walk.tell(phit, gt);
    }
    run.status[(size_t)s] = walk.opt.status;
    run.evals[(size_t)s] = walk.evals;
    mask.scatter(walk.opt.x.data(), th.data());
    for (int k = 0; k < P; ++k) run.out.theta[s * P + k] = th[(size_t)k];
    run.out.f[s] = walk.opt.phi;
    return TGP_OK;
}

static void warp_run_share(WarpRun &run, int t, int T, tgp_handle hw) {
    try {
        for (int64_t s = t; s < run.a.S; s += T)
            if (const int rc = warp_run_start(run, s, hw); rc != TGP_OK) {
                run.rcs[(size_t)t] = rc;
                run.errs[(size_t)t] = tgp_last_error(hw);
                return;
            }
    } catch (const std::bad_alloc &) {    // (no exception leaves a worker thread: that would be std::terminate)
        run.rcs[(size_t)t] = TGP_NO_MEMORY;
        run.errs[(size_t)t] = "out of host memory";
    } catch (...) {
        run.rcs[(size_t)t] = TGP_HIP_ERROR;
        run.errs[(size_t)t] = "unexpected exception in a start's thread";
    }
}

// fit_optimise_streams's sibling: the same thread rule, the same worker handles, every start on its own handle
static int warp_optimise_streams(tgp_handle h, const HyperOptArgs &a, const WarpOptArgs &wa, const HyperOptOut &out) {
    Context &c = h->c;
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int T = hyper_thread_count(a.N, a.S);
    Borrowed borrowed{h};
    if (const int rc = borrowed.acquire(T); rc != TGP_OK) return rc;
    WarpRun run(a, out, wa, T);
    (void)run_on_start_threads(T, [&](int t) { warp_run_share(run, t, T, T == 1 ? h : borrowed.workers[(size_t)t]); });
    for (int t = 0; t < T; ++t)
        if (run.rcs[(size_t)t] != TGP_OK) return fail(c, run.rcs[(size_t)t], "tgp_fit_warp_lbfgsb: " + run.errs[(size_t)t]);
    int64_t ev = 0;
    for (int64_t s = 0; s < a.S; ++s) {
        if (out.status) out.status[s] = run.status[(size_t)s];
        ev += run.evals[(size_t)s];
    }
    if (out.evaluations) *out.evaluations = ev;
    return TGP_OK;
}
