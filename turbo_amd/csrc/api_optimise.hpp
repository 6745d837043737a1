// api_optimise.hpp -- the optimiser entries of the C-ABI, as named steps over their argument records:
//
//   tgp_acq_refine    check_refine_args -> acq_refine:  refine_small | refine_general (refine_iterate)
//   tgp_acq_lbfgsb    check_refine_args -> acq_lbfgsb_lockstep:  R walks, one batched tgp_acq_grad per round
//   tgp_kg_lbfgsb     check_refine_args -> acq_lbfgsb_lockstep:  the same walks, one batched tgp_kg_grad per round
//   tgp_fit_lbfgsb    check_optimise_args -> fit_optimise_streams:  hyper_thread_count, Borrowed, HyperRun, run_start
//   tgp_fit_optimise  check_optimise_args -> hyper_one_launch | fit_optimise_streams
//
// The walk itself (the reverse-communication loop, its cache rule and its stop rule) is LbfgsbWalk, host_lbfgsb.hpp; the
// entries stay in tgp_api.hip: the null check, HOST_NA, the records, the check and one call.
//
// NOT a header of its own: tgp_api.hip includes it once, where these functions stood, behind the helpers they use
// (fail, grow, ensure_pinned, call_begin / call_finish, fit_grad_entry, acq_check_args) -- the same translation unit.
#pragma once

// Blocks of doubles laid end to end in one buffer, in the order they are taken: each block's offset is written once and
// serves the host pointer, the device pointer and the size alike.  (Not sweep_pruned.hpp's Carver, which rounds every
// block up to 256 bytes: these layouts are packed, the kernels behind them were handed consecutive blocks from the start,
// and the sizes asked of ensure_pinned / grow stay what they were.)
struct Packed {
    size_t n = 0;
    size_t take(size_t count) { const size_t at = n; n += count; return at; }
    size_t bytes() const { return n * sizeof(double); }
};

// ---- the gradient stage: tgp_acq_refine, tgp_acq_lbfgsb -------------------------------------------------------------
struct RefineArgs {
    const double *X0; int64_t R; const double *lo, *hi;
    int acq; double sf, incumbent, param; int64_t max_iter;
};
struct RefineOut { double *x, *val; int64_t *status, *evaluations; };

// in the order they report: a fitted model, the entry's own text, the acquisition (up to acq_max), max_iter, the box
static int check_refine_args(Context &c, const char *fn, const RefineArgs &a, const RefineOut &out, int acq_max) {
    const char *own = (!a.X0 || !a.lo || !a.hi || !out.x || !out.val || a.R < 1 || a.R > 4096) ? "need X0, lo, hi, x_out, val_out and 1 <= R <= 4096" : nullptr;
    if (int arc = acq_check_args(c, fn, own, a.acq, acq_max, a.sf); arc != TGP_OK) return arc;
    if (a.max_iter < 1) return fail(c, TGP_BAD_ARG, std::string(fn) + ": max_iter >= 1");
    return box_check(c, fn, a.lo, a.hi);
}

// small problems: one launch, one workgroup per restart running its whole optimisation; starts and
// bounds are read from, results written to, device-mapped host memory (no memcpy)
struct RefineSmallIO {      // in: X0 | lo | hi      out: 8 (the call's record) | x | v | info (3 per restart)
    Packed in, out;
    size_t X0, lo, hi, x, v, info;
    RefineSmallIO(int64_t R, int64_t D) {
        X0 = in.take((size_t)(R * D)); lo = in.take((size_t)D); hi = in.take((size_t)D);
        out.take(8); x = out.take((size_t)(R * D)); v = out.take((size_t)R); info = out.take((size_t)(3 * R));
    }
};
static int refine_small(Context &c, const RefineArgs &a, const RefineOut &out) {
    const int64_t R = a.R, D = c.D;
    const RefineSmallIO io(R, D);
    int prc = ensure_pinned(c, io.in.bytes(), io.out.bytes());
    if (prc != TGP_OK) return prc;
    double *h_in = c.h_pin_in, *d_in = c.h_pin_in.dev(), *h_out = c.h_pin_out, *d_out = c.h_pin_out.dev();
    memcpy(h_in + io.X0, a.X0, (size_t)(R * D) * sizeof(double));
    memcpy(h_in + io.lo, a.lo, (size_t)D * sizeof(double));
    memcpy(h_in + io.hi, a.hi, (size_t)D * sizeof(double));
    CallClock clk;
    if ((prc = call_begin(c, clk)) != TGP_OK) return prc;
    hipError_t le = launch_small_refine(c, d_in + io.X0, d_in + io.lo, d_in + io.hi, (int)R, a.acq, a.sf, a.incumbent, a.param,
                                        (int)std::min<int64_t>(a.max_iter, 1 << 30), LBFGSB_PGTOL, LBFGSB_FTOL, d_out + io.x,
                                        d_out + io.v, d_out + io.info);
    if (le != hipSuccess) return hip_fail(c, le, "launch_small_refine");
    if ((prc = call_finish(c, clk, c.last_sweep_ms, "refine sync")) != TGP_OK) return prc;
    const double *h_info = h_out + io.info;
    memcpy(out.x, h_out + io.x, (size_t)(R * D) * sizeof(double));
    memcpy(out.val, h_out + io.v, (size_t)R * sizeof(double));
    int64_t ev = 0;
    for (int64_t r = 0; r < R; ++r) {
        if (out.status) out.status[r] = (int64_t)h_info[3 * r];
        ev = std::max<int64_t>(ev, (int64_t)h_info[3 * r + 2]);
    }
    if (out.evaluations) *out.evaluations = ev;      // evaluations of the slowest restart (what the lock-step path counts)
    return TGP_OK;
}

// optimiser state in c.d_rf: [state (R stride) | history of the eight-wave teams (D > 1024) | lo (D) | hi (D) | x_out (R D) |
//                             v_out (R) | info (2 R) | active (int)]
struct RefineGeneralWs {
    Packed all;
    size_t state, hist, lo, hi, x, v, info, active;
    RefineGeneralWs(int64_t R, int64_t D) {
        state = all.take((size_t)(R * refine_state_stride((int)D))); hist = all.take((size_t)refine_hist_doubles((int)D, (int)R));
        lo = all.take((size_t)D); hi = all.take((size_t)D); x = all.take((size_t)(R * D)); v = all.take((size_t)R);
        info = all.take((size_t)(2 * R)); active = all.take(2);
    }
};

// every iteration: one batched value + gradient evaluation of all R trial points (the closed-form
// kernels of tgp_acq_grad), then one optimiser step for all restarts.  The host only looks at
// the count of unfinished restarts, every 4th iteration.  it: the iterations run.
static int refine_iterate(Context &c, const RefineArgs &a, const QueryWs &q, const RefineGeneralWs &ws, int64_t &it) {
    double *d_rf = c.d_rf;
    int *d_active = reinterpret_cast<int *>(d_rf + ws.active);
    int active = (int)a.R;
    for (it = 0; it <= a.max_iter; ++it) {
        // (the wave step turns the evaluation's sums into value + gradient itself, one launch fewer)
        hipError_t le = launch_query(c, q.Xq, (int)a.R, a.acq, a.sf, a.incumbent, a.param, q.ws, nullptr, q.grad);
        if (le != hipSuccess) return hip_fail(c, le, "launch_query");
        le = launch_refine_step(c, d_rf + ws.state, q.Xq, q.val, q.grad, d_rf + ws.lo, d_rf + ws.hi, (int)a.R, (int)it, LBFGSB_PGTOL,
                                LBFGSB_FTOL, d_active, q.red, a.acq, a.sf, a.incumbent, a.param);
        if (le != hipSuccess) return hip_fail(c, le, "launch_refine_step");
        if ((it & 3) == 3 || it == a.max_iter) {
            API_HIP(hipMemcpyAsync(&active, d_active + (it & 1), sizeof(int), hipMemcpyDeviceToHost, c.stream), "D2H active");
            API_HIP(hipStreamSynchronize(c.stream), "refine sync");
            if (active == 0) { ++it; break; }
        }
    }
    return TGP_OK;
}

static int refine_general(Context &c, const RefineArgs &a, const RefineOut &out) {
    const int64_t R = a.R, D = c.D;
    API_MEM(grow(c, c.d_qws, query_ws(c, (int)R).bytes, "hipMalloc query workspace"));   // as tgp_acq_grad
    const RefineGeneralWs ws(R, D);
    int rc = grow(c, c.d_rf, ws.all.bytes(), "hipMalloc refine state");
    if (rc != TGP_OK) return rc;
    const QueryWs q = query_ws(c, (int)R);
    double *d_rf = c.d_rf;
    CallClock clk;
    if ((rc = call_begin(c, clk)) != TGP_OK) return rc;
    API_HIP(hipMemcpyAsync(q.Xq, a.X0, (size_t)(R * D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D X0");
    API_HIP(hipMemcpyAsync(d_rf + ws.lo, a.lo, (size_t)D * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D lo");
    API_HIP(hipMemcpyAsync(d_rf + ws.hi, a.hi, (size_t)D * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D hi");
    hipError_t le = launch_refine_clip(c, q.Xq, d_rf + ws.lo, d_rf + ws.hi, (int)R);
    if (le != hipSuccess) return hip_fail(c, le, "launch_refine_clip");
    int64_t it = 0;
    if ((rc = refine_iterate(c, a, q, ws, it)) != TGP_OK) return rc;
    le = launch_refine_collect(c, d_rf + ws.state, (int)R, d_rf + ws.x, d_rf + ws.v, d_rf + ws.info);
    if (le != hipSuccess) return hip_fail(c, le, "launch_refine_collect");
    std::vector<double> info((size_t)(2 * R));
    API_HIP(hipMemcpyAsync(out.x, d_rf + ws.x, (size_t)(R * D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H x");
    API_HIP(hipMemcpyAsync(out.val, d_rf + ws.v, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H values");
    API_HIP(hipMemcpyAsync(info.data(), d_rf + ws.info, (size_t)(2 * R) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H info");
    if ((rc = call_finish(c, clk, c.last_sweep_ms, "refine sync")) != TGP_OK) return rc;
    if (out.status)
        for (int64_t r = 0; r < R; ++r) out.status[r] = (int64_t)info[(size_t)(2 * r)];
    if (out.evaluations) *out.evaluations = it;
    return TGP_OK;
}

static int acq_refine(Context &c, const RefineArgs &a, const RefineOut &out) {
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    return small_refine_fits(c) && small_path_enabled() ? refine_small(c, a, out) : refine_general(c, a, out);
}

// The gradient stage as the reference runs it -- scipy.optimize.minimize(method='L-BFGS-B', default limits) on the
// negated acquisition from every start (turbo/modules/auxiliary_optimisers.py:80-99) -- inside the library: one
// host_lbfgsb.hpp optimiser per restart, all of them in LOCK-STEP on the calling thread (reverse communication needs no
// threads): every round gathers the trial points of the restarts still running, ONE batched closed-form value +
// gradient evaluation serves them all (tgp_acq_grad: a point's value does not depend on the batch it travels in), and
// every optimiser takes its step.  What turbo_amd/auxiliary_optimisers.py did with a Python thread and a SciPy
// optimiser per restart meeting at a rendezvous; same walk per restart, no interpreter between two rounds.
// (No hipSetDevice, no pre_join here: every tgp_acq_grad makes its own.)
// eval(Xq, m, val, grad): the round's batched evaluation -- tgp_acq_grad, or tgp_kg_grad for the knowledge gradient.
template <class Eval>
static int acq_lbfgsb_lockstep(tgp_handle h, const RefineArgs &a, const RefineOut &out, Eval &&eval) {
    const int D = (int)h->c.D;
    const int64_t R = a.R;
    std::vector<LbfgsbWalk> walks;
    walks.reserve((size_t)R);
    for (int64_t r = 0; r < R; ++r) walks.emplace_back(a.X0 + r * D, a.lo, a.hi, D, a.max_iter);
    std::vector<double> Xq((size_t)R * D), val((size_t)R), grad((size_t)R * D), gt((size_t)D);
    std::vector<int64_t> who((size_t)R);
    int64_t ev = 0;
    for (;;) {
        // restarts whose next point is the one they evaluated last (a search giving up on "no further progress") are
        // answered from that evaluation, as SciPy answers them from its cache; the others go into this round's batch
        int64_t m = 0;
        for (int64_t r = 0; r < R; ++r) {
            if (!walks[(size_t)r].wants_eval()) continue;
            memcpy(&Xq[(size_t)(m * D)], walks[(size_t)r].xt.data(), (size_t)D * sizeof(double));
            who[(size_t)m++] = r;
        }
        if (m == 0) break;
        const int rc = eval(Xq.data(), m, val.data(), grad.data());
        if (rc != TGP_OK) return rc;
        ev += m;
        for (int64_t i = 0; i < m; ++i) {
            for (int d = 0; d < D; ++d) gt[(size_t)d] = -grad[(size_t)(i * D + d)];     // maximise = minimise the negation
            walks[(size_t)who[(size_t)i]].tell(-val[(size_t)i], gt);
        }
    }
    for (int64_t r = 0; r < R; ++r) {
        const HostLbfgsb &o = walks[(size_t)r].opt;
        for (int d = 0; d < D; ++d) out.x[r * D + d] = o.x[(size_t)d];
        out.val[r] = -o.phi;
        if (out.status) out.status[r] = o.status;
    }
    if (out.evaluations) *out.evaluations = ev;
    return TGP_OK;
}

// ---- the hyper-parameter fit: tgp_fit_lbfgsb, tgp_fit_optimise ------------------------------------------------------
struct HyperOptArgs {
    const double *X; int64_t N, D; const double *y; int kernel;
    const double *theta0; int64_t S, n_ls; const double *log_lo, *log_hi;
    double jitter; int normalize_y; int64_t max_iter;
};
struct HyperOptOut { double *theta, *f; int64_t *status, *evaluations; };

static int check_optimise_args(Context &c, const char *fn, const HyperOptArgs &a, const HyperOptOut &out) {
    const std::string name(fn);
    if (!a.X || !a.y || !a.theta0 || !a.log_lo || !a.log_hi || !out.theta || !out.f)
        return fail(c, TGP_BAD_ARG, name + ": need X, y, theta0, log_lo, log_hi, theta_out, f_out");
    if (a.kernel < 0 || a.kernel > 3) return fail(c, TGP_BAD_ARG, name + ": unknown kernel");
    if (a.N < 1 || a.D < 1 || a.D > 4096 || (a.n_ls != 1 && a.n_ls != a.D) || a.S < 1 || a.S > 64 || a.max_iter < 1)
        return fail(c, TGP_BAD_ARG, name + ": needs N >= 1, 1 <= D <= 4096, n_ls 1 or D, 1 <= S <= 64, max_iter >= 1");
    for (int64_t i = 0; i < 2 + a.n_ls; ++i) {
        // (the noise entry fixed at log 0: a kernel without a noise term)
        if (i == 1 + a.n_ls && a.log_lo[i] == -INFINITY && a.log_hi[i] == -INFINITY) continue;
        if (!(a.log_lo[i] <= a.log_hi[i]) || !isfinite(a.log_lo[i]) || !isfinite(a.log_hi[i]))
            return fail(c, TGP_BAD_ARG, name + ": bounds must be finite with lo <= hi (the noise entry may be fixed at -inf: no noise term)");
    }
    return TGP_OK;
}

// how many starts run side by side: a rule of N, S and the TGP_HYPER_THREADS switch
static int hyper_thread_count(int64_t N, int64_t S) {
    // measured through the plugin path (tools/bench_latency.py): one evaluation is a serial chain of ~35 launches that
    // leaves the chip idle up to N ~ 1000; beyond, two chains already share the CUs
    const int threads_env = tuning().hyper_threads;
    // (round 4, late, with the workers' inverses in line and every start on a worker: three starts at N = 700 / 1000 / 1500
    // take 18.6 / 27.1 / 36.8 ms on three threads against 32 / 42 / 53 on one; at 2048 the chains fill the chip: 120 vs 117)
    // (round 5, late, re-measured with L-BFGS-B in the library and the one-outer-block fits: three starts side by side
    // now pay well beyond 1536 -- N = 2048 55.8 -> 42.2 ms, 3000 110 -> 82, 4096 240 -> 206, 6144 482 -> 440, 8192 984 ->
    // 911 -- two threads never do (2 + 1); the limit is the workers' workspaces, 4 N^2 doubles each: 2 GiB at 8192)
    const int T = threads_env > 0 ? threads_env : (N <= 1536 ? 4 : (N <= 8192 ? 3 : 1));
    return (int)std::min<int64_t>(T, S);
}

// With more than one thread EVERY start runs on a worker handle (a private stream each) and the caller's handle sits
// out: on its shared main stream it ended up serialised with one of the workers in the first factory of a fresh
// process (an evaluation 0.35 -> 0.83 ms on both; N = 500, three starts: 23-27 ms instead of 11.6; tools/diag_streams.py
// shows the pairing).  No probe saw it -- one launch on each stream, chains of memory-dependent launches from one
// thread, launch + wait cycles from two threads all ran side by side -- so re-creating streams until a probe passes
// is no cure; the workers do not show it among themselves.
struct Borrowed {   // the pool is this call's from here to the return
    tgp_handle h; bool held = false;
    std::vector<tgp_handle> workers;
    int acquire(int T) {
        workers.assign((size_t)T, nullptr);
        if (T <= 1) return TGP_OK;
        const int rc = tgp_workers_acquire(h, T, workers.data());
        held = rc == TGP_OK;
        return rc;
    }
    ~Borrowed() { if (held) (void)tgp_workers_release(h); }
};

// what the starts of one call share: the arguments, the free entries, and what each start (status, evals) and each
// thread (rcs, errs) leaves behind
struct HyperRun {
    const HyperOptArgs &a;
    const HyperOptOut &out;
    const FreeMask mask;
    std::vector<int> status, rcs;
    std::vector<int64_t> evals;
    std::vector<std::string> errs;
    HyperRun(const HyperOptArgs &a_, const HyperOptOut &out_, int T)
        : a(a_), out(out_), mask(a_.log_lo, a_.log_hi, (int)(2 + a_.n_ls)), status((size_t)a_.S, 0), rcs((size_t)T, TGP_OK),
          evals((size_t)a_.S, 0), errs((size_t)T) {}
};

// start s on handle hw: its walk over tgp_fit_grad (fit + LML gradient on the GPU); an evaluation's failure comes back
static int run_start(HyperRun &run, int64_t s, tgp_handle hw) {
    const HyperOptArgs &a = run.a;
    const FreeMask &mask = run.mask;
    const int P = (int)(2 + a.n_ls), Pf = mask.Pf;
    std::vector<double> ls((size_t)a.n_ls), grad((size_t)P), th((size_t)P), xt((size_t)Pf), gt((size_t)Pf);
    // th = the full vector log(constant, length scale(s), noise); the optimiser sees its free entries only
    for (int k = 0; k < P; ++k) th[(size_t)k] = HostLbfgsb::clip(a.theta0[s * P + k], a.log_lo[k], a.log_hi[k]);
    mask.gather(th.data(), xt.data());
    LbfgsbWalk walk(xt.data(), mask.lo_f.data(), mask.hi_f.data(), Pf, a.max_iter);
    while (walk.wants_eval()) {
        mask.scatter(walk.xt.data(), th.data());
        double constant, noise, lml = 0.0, phit;
        slice_unpack(th.data(), a.n_ls, constant, ls.data(), noise);
        const int rc = fit_grad_entry(hw, FitArgs{a.X, a.N, a.D, a.y, a.kernel, constant, ls.data(), a.n_ls, noise, a.jitter, a.normalize_y},
                                      FitOut{&lml, nullptr, nullptr}, grad.data());
        if (rc == TGP_NOT_PD) {            // -inf likelihood, zero gradient (_gpr.py:586-589)
            phit = INFINITY;
            std::fill(gt.begin(), gt.end(), 0.0);
        } else if (rc != TGP_OK) {
            return rc;
        } else {
            phit = -lml;
            mask.gather(grad.data(), gt.data(), -1.0);
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

// thread t's share: starts t, t + T, ... one after the other on handle hw
static void run_share(HyperRun &run, int t, int T, tgp_handle hw) {
    try {
        for (int64_t s = t; s < run.a.S; s += T)
            if (const int rc = run_start(run, s, hw); rc != TGP_OK) {
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

// tgp_fit_optimise above the one-launch sizes: every start is a host_lbfgsb.hpp optimiser (SciPy's L-BFGS-B restated:
// the iterates scikit-learn's fit walks) driving tgp_fit_grad
// (fit + LML gradient on the GPU); the starts run side by side, a C++ thread and a handle on a stream of its own
// each (start j of a thread's share after the other: thread t takes starts t, t + T, ...), with no interpreter
// between two evaluations.  Every start walks the iterates it walks alone -- its own optimiser state, its own
// handle -- so the result does not depend on the number of threads.
static int fit_optimise_streams(tgp_handle h, const HyperOptArgs &a, const HyperOptOut &out) {
    Context &c = h->c;
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int T = hyper_thread_count(a.N, a.S);
    Borrowed borrowed{h};
    if (const int rc = borrowed.acquire(T); rc != TGP_OK) return rc;
    HyperRun run(a, out, T);
    // (the library's parked start threads; shares no thread could be had for run on this one)
    (void)run_on_start_threads(T, [&](int t) { run_share(run, t, T, T == 1 ? h : borrowed.workers[(size_t)t]); });
    for (int t = 0; t < T; ++t)
        if (run.rcs[(size_t)t] != TGP_OK) return fail(c, run.rcs[(size_t)t], "tgp_fit_optimise: " + run.errs[(size_t)t]);
    int64_t ev = 0;
    for (int64_t s = 0; s < a.S; ++s) {
        if (out.status) out.status[s] = run.status[(size_t)s];
        ev += run.evals[(size_t)s];
    }
    if (out.evaluations) *out.evaluations = ev;
    return TGP_OK;
}

static int fit_lbfgsb(tgp_handle h, const HyperOptArgs &a, const HyperOptOut &out) {
    Context &c = h->c;
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    return fit_optimise_streams(h, a, out);
}

// N <= 128: every start's whole optimisation in ONE launch (small_kernels.hip); inputs through device-mapped host memory
// (each start copies X and the targets once), results the same way
struct HyperSmallIO {       // in: X | yn | theta0 | lo | hi      out: 8 (the call's record) | theta | f | info (3 per start)
    Packed in, out;
    size_t X, yn, theta0, lo, hi, theta, f, info;
    HyperSmallIO(int64_t N, int64_t D, int64_t S, int64_t P) {
        X = in.take((size_t)(N * D)); yn = in.take((size_t)N); theta0 = in.take((size_t)(S * P)); lo = in.take((size_t)P); hi = in.take((size_t)P);
        out.take(8); theta = out.take((size_t)(S * P)); f = out.take((size_t)S); info = out.take((size_t)(3 * S));
    }
};
static int hyper_one_launch(Context &c, const HyperOptArgs &a, const HyperOptOut &out) {
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t N = a.N, D = a.D, S = a.S, Dp = ((D + 3) / 4) * 4, P = 2 + a.n_ls;
    double mean = 0.0, sd = 1.0;
    std::vector<double> yn((size_t)N, 0.0);
    normalise_targets(a.y, N, a.normalize_y, yn, mean, sd);
    const HyperSmallIO io(N, D, S, P);
    int rc = ensure_pinned(c, io.in.bytes(), io.out.bytes());
    if (rc != TGP_OK) return rc;
    double *h_in = c.h_pin_in;
    memcpy(h_in + io.X, a.X, (size_t)(N * D) * sizeof(double));
    memcpy(h_in + io.yn, yn.data(), (size_t)N * sizeof(double));
    memcpy(h_in + io.theta0, a.theta0, (size_t)(S * P) * sizeof(double));
    memcpy(h_in + io.lo, a.log_lo, (size_t)P * sizeof(double));
    memcpy(h_in + io.hi, a.log_hi, (size_t)P * sizeof(double));
    const size_t ws_need = (size_t)S * (size_t)small_hyper_workspace_doubles((int)N, (int)D, (int)Dp) * sizeof(double);
    rc = grow(c, c.d_rf, ws_need, "hipMalloc hyper workspace");
    if (rc != TGP_OK) return rc;
    const double *d_in = c.h_pin_in.dev(), *h_out = c.h_pin_out, *h_info = h_out + io.info;
    double *d_out = c.h_pin_out.dev();
    bool timed_out = false;
    // A start whose three workgroups never met (status 3: the barrier's time budget ran out, e.g. CUs taken
    // away by HSA_CU_MASK or by another process on the card) invalidates the launch: nothing of it reaches
    // the caller, and the fit runs once more with one workgroup per start -- no barrier, no way to wait.
    for (int attempt = 0; attempt < 2; ++attempt) {
        CallClock clk;
        if ((rc = call_begin(c, clk)) != TGP_OK) return rc;
        hipError_t le = launch_small_hyper(c, a.kernel, d_in + io.X, d_in + io.yn, d_in + io.theta0, d_in + io.lo, d_in + io.hi, (int)S,
                                           (int)N, (int)D, (int)Dp, (int)a.n_ls, (int)std::min<int64_t>(a.max_iter, 1 << 30), a.jitter,
                                           c.d_rf, d_out + io.theta, d_out + io.f, d_out + io.info, attempt > 0);
        if (le != hipSuccess) return hip_fail(c, le, "launch_small_hyper");
        if ((rc = call_finish(c, clk, c.last_fit_ms, "hyper sync")) != TGP_OK) return rc;
        timed_out = false;
        for (int64_t s = 0; s < S; ++s) timed_out = timed_out || (int64_t)h_info[3 * s] == 3;
        if (!timed_out) break;
    }
    if (timed_out) return fail(c, TGP_HIP_ERROR, "tgp_fit_optimise: the barrier between a start's workgroups timed out, and so did the relaunch with one workgroup per start");
    memcpy(out.theta, h_out + io.theta, (size_t)(S * P) * sizeof(double));
    memcpy(out.f, h_out + io.f, (size_t)S * sizeof(double));
    int64_t ev = 0;
    for (int64_t s = 0; s < S; ++s) {
        if (out.status) out.status[s] = (int64_t)h_info[3 * s];
        ev += (int64_t)h_info[3 * s + 2];
    }
    if (out.evaluations) *out.evaluations = ev;
    return TGP_OK;
}

// one launch where the kernel takes the problem (and the switch allows it, and there is a noise term); else the streams
// path -- routed before any hipSetDevice of this entry's own
static int fit_optimise(tgp_handle h, const HyperOptArgs &a, const HyperOptOut &out) {
    const int64_t Dp = ((a.D + 3) / 4) * 4, P = 2 + a.n_ls;
    if (a.N > 2 * NB || Dp > 64 || P > 64 || !small_path_enabled() || a.log_lo[P - 1] == -INFINITY) return fit_optimise_streams(h, a, out);
    return hyper_one_launch(h->c, a, out);
}
