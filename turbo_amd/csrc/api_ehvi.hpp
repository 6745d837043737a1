// api_ehvi.hpp -- two-objective expected hypervolume improvement in the C-ABI (include/turbogp.h), as named steps:
//
//   tgp_ehvi_set_front  ehvi_set_front:  host_front.hpp's builder, then the breakpoints to the device and onto the handle
//   tgp_sweep_ehvi      ehvi_check -> ehvi_sweep:  tgp_sweep_weighted's schedule with K = 1 -- g's copy of the rows, g's
//                                                  sweep, weighted_join, h's sweep, ehvi_value_kernel, the shared arg-max
//   tgp_ehvi_grad       ehvi_check -> ehvi_grad:   both handles' launch_query sums (and their own sweeps' bits where
//                                                  those are f64), ehvi_coef_kernel, ehvi_grad_kernel
//   tgp_ehvi_lbfgsb     check_refine_args -> ehvi_check -> acq_lbfgsb_lockstep over ehvi_grad
//
// NOT a header of its own: tgp_api.hip includes it once behind the weighted entries, whose helpers it uses
// (weighted_join, weighted_sweep_is_f64, kg_grad_sweep_posterior) -- the same translation unit.
#pragma once

#include "host_front.hpp"

constexpr int64_t EHVI_STRIPS = TGP_EHVI_MAX_FRONT + 1;

static int ehvi_set_front(tgp_handle h, const double *Y, int64_t n, double sf1, double sf2, const double *ref, int64_t *P_out,
                          double *front_out, double *hv_out) {
    Context &c = h->c;
    tgp_front::Front f;
    switch (tgp_front::build_front(Y, n, sf1, sf2, ref, TGP_EHVI_MAX_FRONT, f)) {
        case tgp_front::FRONT_OK: break;
        case tgp_front::FRONT_BAD_SF: return fail(c, TGP_BAD_ARG, "tgp_ehvi_set_front: sf1 and sf2 must be +1 or -1");
        case tgp_front::FRONT_BAD_REF: return fail(c, TGP_BAD_ARG, "tgp_ehvi_set_front: ref must be 2 finite values");
        case tgp_front::FRONT_BAD_Y: return fail(c, TGP_BAD_ARG, "tgp_ehvi_set_front: need n >= 0 and finite Y (n, 2)");
        case tgp_front::FRONT_TOO_LARGE: return fail(c, TGP_BAD_ARG, "tgp_ehvi_set_front: the front has more than 256 points");
    }
    std::vector<double> a, lv, both((size_t)(2 * EHVI_STRIPS), 0.0);
    tgp_front::front_strips(f, a, lv);
    std::copy(a.begin(), a.end(), both.begin());
    std::copy(lv.begin(), lv.end(), both.begin() + EHVI_STRIPS);
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    // (every argument is checked by now; a HIP failure below leaves the handle without a front, not with half of one)
    API_MEM(grow(c, c.d_ehvi_front, both.size() * sizeof(double), "hipMalloc front"));
    c.ehvi_P = -1;
    API_HIP(hipMemcpyAsync(c.d_ehvi_front.get(), both.data(), both.size() * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D front");
    API_HIP(hipStreamSynchronize(c.stream), "front sync");
    c.ehvi_P = (int)f.size();
    c.ehvi_sf[0] = sf1; c.ehvi_sf[1] = sf2;
    c.ehvi_a = std::move(a);
    c.ehvi_c = std::move(lv);
    if (P_out) *P_out = f.size();
    if (front_out)
        for (int64_t i = 0; i < f.size(); ++i) {
            front_out[2 * i] = sf1 * f.u[(size_t)i].first;
            front_out[2 * i + 1] = sf2 * f.u[(size_t)i].second;
        }
    if (hv_out) *hv_out = f.hv;
    return TGP_OK;
}

// the checks the three entries share, in the order they report
static int ehvi_check(tgp_handle h, tgp_handle g, const char *fn) {
    Context &c = h->c;
    const std::string f = std::string(fn) + ": ";
    if (!g) return fail(c, TGP_BAD_ARG, f + "the second objective's handle is NULL");
    if (g->host) return fail(c, TGP_BAD_ARG, f + "a TGP_DEVICE_HOST handle cannot be the second objective");
    if (g == h) return fail(c, TGP_BAD_ARG, f + "the two objectives need two handles");
    if (!c.fitted) return fail(c, TGP_NOT_FITTED, f + "no fitted model");
    if (!g->c.fitted) return fail(c, TGP_NOT_FITTED, f + "the second objective: no fitted model");
    if (g->c.device != c.device) return fail(c, TGP_BAD_ARG, f + "the second objective's handle is on another device");
    if (g->c.D != c.D) return fail(c, TGP_BAD_ARG, f + "the second objective's D differs from the first's");
    if (c.ehvi_P < 0) return fail(c, TGP_BAD_ARG, f + "no front set (tgp_ehvi_set_front)");
    return TGP_OK;
}

static int ehvi_sweep(tgp_handle h, tgp_handle gh, double *mu, double *sigma, double *mu2, double *sigma2, double *ehvi_out,
                      double *best_val, int64_t *best_idx, int64_t *n_clamped) {
    Context &c = h->c, &g = gh->c;
    if (!c.d_cand || c.M < 1) return fail(c, TGP_BAD_ARG, "tgp_sweep_ehvi: no candidates set");
    if (warp_in_force(c))
        return fail(c, TGP_BAD_ARG, "tgp_sweep_ehvi: the resident batch is a warped one (tgp_warp_candidates): each model would need its own warp");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t M = c.M, D = c.D;
    const size_t mb = (size_t)M * sizeof(double);
    int rc = ensure_outputs(c, true, true, false);
    if (rc != TGP_OK) return rc;
    API_MEM(grow(c, c.d_ehvi_val, mb, "hipMalloc ehvi value"));
    // a failure between the first sweep and the final kernel leaves clamp counts in the counters of the handles swept so
    // far: they are handed back at zero, as every sweep does
    bool g_swept = false;
    auto bail = [&](int code) {
        if (g_swept) {
            (void)hipMemsetAsync(g.d_besti + 1, 0, sizeof(long long), g.stream);
            (void)hipStreamSynchronize(g.stream);
        }
        (void)hipMemsetAsync(c.d_besti + 1, 0, sizeof(long long), c.stream);
        (void)hipStreamSynchronize(c.stream);
        (void)hipGetLastError();
        return code;
    };
    auto g_fail = [&](int code) {
        const std::string why = g.err;
        return bail(fail(c, code, "tgp_sweep_ehvi: the second objective: " + why));
    };
    // g's batch becomes its OWN device-to-device copy of h's rows -- what tgp_set_candidates with those rows leaves: a
    // front of a sweep is dropped, a borrowed buffer is released (never written), a warped batch is gone
    if (const hipError_t e = pre_join(g); e != hipSuccess) { (void)hip_fail(g, e, "hipStreamWaitEvent"); return g_fail(TGP_HIP_ERROR); }
    if ((rc = grow_candidates(g, M * D)) != TGP_OK) return g_fail(rc);
    if (const hipError_t e = hipMemcpyAsync(g.d_cand_owned, c.d_cand, (size_t)(M * D) * sizeof(double), hipMemcpyDeviceToDevice, g.stream);
        e != hipSuccess) { (void)hip_fail(g, e, "D2D candidates"); return g_fail(TGP_HIP_ERROR); }
    g.d_cand = g.d_cand_owned;
    g.M = M;
    if ((rc = ensure_outputs(g, true, true, false)) != TGP_OK) return g_fail(rc);
    {   // its unpruned predict-only sweep, in its own arithmetic and on its own stream: no record, no winner, no bell
        SweepCall s;
        s.mu = g.d_mu; s.sigma = g.d_sigma;
        CallClock clk;
        g_swept = true;
        if ((rc = run_sweep(g, s, clk)) != TGP_OK) return g_fail(rc);
    }
    if ((rc = weighted_join(c, g, c.ev_ehvi)) != TGP_OK) return bail(rc);
    {   // h's unpruned predict-only sweep (the pruned sweep's bounds belong to the single-objective arg-max)
        SweepCall s;
        s.mu = c.d_mu; s.sigma = c.d_sigma;
        CallClock clk;
        if ((rc = run_sweep(c, s, clk)) != TGP_OK) return bail(rc);
    }
    if (const hipError_t le = launch_ehvi_value(c, g, c.d_ehvi_front, c.ehvi_P, c.ehvi_sf[0], c.ehvi_sf[1], c.d_ehvi_val); le != hipSuccess)
        return bail(hip_fail(c, le, "launch_ehvi_value"));
    SweepCall fin;
    fin.acq = TGP_ACQ_EI;                 // (any acquisition: the final kernel only asks whether there is one)
    fin.winner = c.d_winner;
    const bool zc = tuning().sweep_zc != 0;
    if (zc && (rc = ensure_pinned(c, 0, 8 * sizeof(double))) != TGP_OK) return bail(rc);
    fin.res = zc ? c.h_pin_out.dev() : nullptr;
    if (const hipError_t le = launch_argmax_of(c, fin, c.d_ehvi_val); le != hipSuccess) return bail(hip_fail(c, le, "launch_argmax_of"));
    if ((rc = winner_mark(c, fin)) != TGP_OK) return rc;
    SweepRecord rec;
    if ((rc = sweep_queue_return(c, zc, fin.acq, rec, nullptr, mu, sigma, nullptr)) != TGP_OK) return rc;
    if (mu2) API_HIP(hipMemcpyAsync(mu2, g.d_mu, mb, hipMemcpyDeviceToHost, c.stream), "D2H mu2");
    if (sigma2) API_HIP(hipMemcpyAsync(sigma2, g.d_sigma, mb, hipMemcpyDeviceToHost, c.stream), "D2H sigma2");
    if (ehvi_out) API_HIP(hipMemcpyAsync(ehvi_out, c.d_ehvi_val, mb, hipMemcpyDeviceToHost, c.stream), "D2H ehvi");
    API_HIP(hipStreamSynchronize(c.stream), "ehvi sweep sync");     // the one wait: g's stream is ordered in front of it
    sweep_read_record(c, zc, fin.acq, rec, best_val, best_idx, n_clamped);
    return TGP_OK;
}

static int ehvi_grad(tgp_handle h, tgp_handle gh, const double *Xq, int64_t m, double *val, double *grad) {
    Context &c = h->c, &g = gh->c;
    if (!Xq || !val || !grad || m < 1 || m > 4096) return fail(c, TGP_BAD_ARG, "tgp_ehvi_grad: need Xq, val, grad and 1 <= m <= 4096");
    API_HIP(hipSetDevice(c.device), "hipSetDevice");
    API_HIP(pre_join(c), "hipStreamWaitEvent");
    const int64_t D = c.D;
    API_MEM(grow(c, c.d_ehvi_q, (size_t)(2 * m * D + 9 * m) * sizeof(double), "hipMalloc ehvi query"));
    API_MEM(grow(c, c.d_qws, query_ws(c, (int)m).bytes, "hipMalloc query workspace"));
    double *d_Xq = c.d_ehvi_q, *d_val = d_Xq + m * D, *d_coef = d_val + m, *d_grad = d_coef + 4 * m, *d_mu = d_grad + m * D, *d_sg = d_mu + 2 * m;
    API_HIP(hipMemcpyAsync(d_Xq, Xq, (size_t)(m * D) * sizeof(double), hipMemcpyHostToDevice, c.stream), "H2D Xq");
    EhviGrad w{};
    w.front = c.d_ehvi_front; w.P = c.ehvi_P; w.m = (int)m; w.D = (int)D;
    w.sf[0] = c.ehvi_sf[0]; w.sf[1] = c.ehvi_sf[1];
    w.val = d_val; w.coef = d_coef; w.grad = d_grad;
    // each model's sums [k.alpha, v.v, gm, gv] per point from the query kernels behind tgp_acq_grad, on its handle's stream
    // and in its handle's workspace; the combination reads both on h's
    {
        const QueryWs q = query_ws(c, (int)m);
        const hipError_t le = launch_query(c, d_Xq, (int)m, TGP_ACQ_NONE, 1.0, 0.0, 0.0, q.ws, nullptr, nullptr);
        if (le != hipSuccess) return hip_fail(c, le, "launch_query");
        const bool own = weighted_sweep_is_f64(c, m);
        if (own)
            if (int rc = kg_grad_sweep_posterior(c, d_Xq, m, d_mu, d_sg); rc != TGP_OK) return rc;
        w.mdl[0] = EhviModel{q.red, c.d_ls, c.constant + c.noise, c.y_mean, c.y_std, own ? d_mu : nullptr, own ? d_sg : nullptr};
    }
    auto g_fail = [&](int code) {
        const std::string why = g.err;
        (void)hipStreamSynchronize(c.stream);
        (void)hipStreamSynchronize(g.stream);
        (void)hipGetLastError();
        return fail(c, code, "tgp_ehvi_grad: the second objective: " + why);
    };
    if (const hipError_t e = pre_join(g); e != hipSuccess) { (void)hip_fail(g, e, "hipStreamWaitEvent"); return g_fail(TGP_HIP_ERROR); }
    if (const int rc = grow(g, g.d_qws, query_ws(g, (int)m).bytes, "hipMalloc query workspace"); rc != TGP_OK) return g_fail(rc);
    if (g.stream != c.stream) {          // the points are on the device before a private stream reads them
        API_HIP(c.ev_ehvi_in.create(hipEventDisableTiming), "hipEventCreate");
        API_HIP(hipEventRecord(c.ev_ehvi_in, c.stream), "hipEventRecord");
        API_HIP(hipStreamWaitEvent(g.stream, c.ev_ehvi_in, 0), "hipStreamWaitEvent");
    }
    {
        const QueryWs q = query_ws(g, (int)m);
        const hipError_t le = launch_query(g, d_Xq, (int)m, TGP_ACQ_NONE, 1.0, 0.0, 0.0, q.ws, nullptr, nullptr);
        if (le != hipSuccess) { (void)hip_fail(g, le, "launch_query"); return g_fail(TGP_HIP_ERROR); }
        const bool own = weighted_sweep_is_f64(g, m);
        if (own)
            if (const int rc = kg_grad_sweep_posterior(g, d_Xq, m, d_mu + m, d_sg + m); rc != TGP_OK) return g_fail(rc);
        if (const int rc = weighted_join(c, g, c.ev_ehvi); rc != TGP_OK) return rc;
        w.mdl[1] = EhviModel{q.red, g.d_ls, g.constant + g.noise, g.y_mean, g.y_std, own ? d_mu + m : nullptr, own ? d_sg + m : nullptr};
    }
    if (const hipError_t le = launch_ehvi_grad(c, w); le != hipSuccess) return hip_fail(c, le, "launch_ehvi_grad");
    API_HIP(hipMemcpyAsync(val, d_val, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H val");
    API_HIP(hipMemcpyAsync(grad, d_grad, (size_t)(m * D) * sizeof(double), hipMemcpyDeviceToHost, c.stream), "D2H grad");
    API_HIP(hipStreamSynchronize(c.stream), "ehvi grad sync");
    return TGP_OK;
}
