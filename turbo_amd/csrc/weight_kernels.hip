// weight_kernels.hip -- constrained and cost-aware acquisition (tgp_sweep_weighted, tgp_weighted_grad): the objective's
// acquisition weighted by the K <= 8 side models' probability of feasibility (Gardner et al. 2014; Gelbart, Snoek & Adams
// 2014) and predicted cost (Snoek, Larochelle & Adams 2012, section 3.2).  The per-model work is the existing
// predict-only sweep and the query kernels (tgp_api.hip); what is new is per candidate and memory-bound: behind side k's
// sweep, which has left mu_k, sigma_k in ITS handle's d_mu / d_sigma,
//     weight_accumulate_kernel   logw += log f_k(mu_k, sigma_k)                  (stored at k = 0)
// and behind the objective's sweep
//     weight_value_kernel        a = acq(mu, sigma),  value = a exp(logw)  (or logw itself for TGP_ACQ_NONE)
// in float64 whatever the dtypes, summed in the order k = 0, 1, ...; launch_argmax_of (integrate_kernels.hip) then takes
// the arg-max and packs the records.  weight_grad_kernel combines the K + 1 models' value-with-partials at m query points.
// log Phi, the step function and the value come from weight_math.hpp.  No atomics: every element has one writer.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "acq_math.hpp"
#include "query_math.hpp"
#include "tgp_internal.hpp"
#include "weight_math.hpp"

namespace tgp {

constexpr int WT_BLOCK = 256;

// grid-stride over the M candidates; thread 0 of workgroup 0 also moves the side's clamp count into the objective's
// counter and hands the side's back at zero (one writer, ordered by the stream)
__global__ __launch_bounds__(WT_BLOCK) void weight_accumulate_kernel(const double *__restrict__ mu, const double *__restrict__ sigma,
                                                                     long M, int kind, double level, int first,
                                                                     double *__restrict__ logw, double *__restrict__ side_mu,
                                                                     double *__restrict__ side_sigma, long long *side_cnt,
                                                                     long long *obj_cnt) {
    const long stride = (long)gridDim.x * WT_BLOCK;
    for (long i = (long)blockIdx.x * WT_BLOCK + threadIdx.x; i < M; i += stride) {
        const double m = mu[i], s = sigma[i];
        const double lf = side_logf(kind, level, m, s);
        logw[i] = first ? lf : logw[i] + lf;
        if (side_mu) side_mu[i] = m;
        if (side_sigma) side_sigma[i] = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        obj_cnt[1] += side_cnt[1];
        side_cnt[1] = 0;
    }
}

// K == 0 (have_w == 0): logw is written as 0 here
__global__ __launch_bounds__(WT_BLOCK) void weight_value_kernel(const double *__restrict__ mu, const double *__restrict__ sigma, long M,
                                                                int acq, double sf, double incumbent, double param, int have_w,
                                                                double *__restrict__ logw, double *__restrict__ acqv,
                                                                double *__restrict__ val) {
    const long stride = (long)gridDim.x * WT_BLOCK;
    for (long i = (long)blockIdx.x * WT_BLOCK + threadIdx.x; i < M; i += stride) {
        const double m = mu[i], s = sigma[i];
        const double a = acq_value(acq, sf, incumbent, param, m, s);
        double lw = 0.0;
        if (have_w) lw = logw[i];
        else logw[i] = 0.0;
        acqv[i] = a;
        val[i] = weighted_value(acq, a, lw, m, s);
    }
}

// one model's posterior and its partials in dimension d at a query point, from launch_query's sums
// r = [k.alpha, v.v, gm[0..D), gv[0..D)] -- q_finalize_point's arithmetic
struct WtPost { double mu, sigma, dmu, dsig; };
__device__ __forceinline__ WtPost wt_posterior(const WtModel &w, const double *r, int D, int d, int q) {
    WtPost p;
    p.mu = w.y_std * r[0] + w.y_mean;
    double var = w.kss - r[1];
    const bool pos = var > 0.0;
    if (!pos) var = 0.0;
    const double sn = sqrt(var);
    p.sigma = w.y_std * sn;
    if (w.mu) { p.mu = w.mu[q]; p.sigma = w.sigma[q]; }       // the sweep's own bits: val is then tgp_sweep_weighted's value for the point
    p.dmu = -w.y_std * r[2 + d] / w.ls[d];
    const double dvar = 2.0 * r[2 + D + d] / w.ls[d];
    p.dsig = pos && sn > 0.0 && p.sigma != 0.0 ? w.y_std * dvar / (2.0 * sn) : 0.0;
    return p;
}

// one thread per (point, dimension); the thread of dimension 0 also writes the value.  Every thread forms its point's
// scalars itself (K <= 8 erfcx), so a point's bits depend neither on m nor on its row.
//   EI / PI:  grad = (prod f) grad a + a sum_k (prod_{j != k} f_j) grad f_k      (no division by a feasibility)
//   NONE:     grad = sum_k (phi / Phi)(z_k) grad z_k   (cost: -grad mu_k)
// summed in the order k = 0, 1, ...; a step-function side (sigma_k == 0) contributes no gradient
__global__ __launch_bounds__(WT_BLOCK) void weight_grad_kernel(WtGrad g) {
    const long e = (long)blockIdx.x * WT_BLOCK + threadIdx.x;
    const int D = g.D;
    if (e >= (long)g.m * D) return;
    const int q = (int)(e / D), d = (int)(e - (long)q * D);
    const long ro = (long)q * (2 + 2 * D);
    const WtPost o = wt_posterior(g.mdl[0], g.mdl[0].red + ro, D, d, q);
    double lf[WT_MAX_SIDES], dlf[WT_MAX_SIDES], dfl[WT_MAX_SIDES], df[WT_MAX_SIDES];   // log f_k; d log f_k; grad f_k = exp(dfl_k) df_k
    double logw = 0.0;
    // (fixed trip counts, fully unrolled: the per-side arrays stay in registers)
#pragma unroll
    for (int k = 0; k < WT_MAX_SIDES; ++k) {
        lf[k] = 0.0; dlf[k] = 0.0; dfl[k] = -INFINITY; df[k] = 0.0;
        if (k >= g.K) continue;
        const WtModel &w = g.mdl[1 + k];
        const WtPost p = wt_posterior(w, w.red + ro, D, d, q);
        lf[k] = side_logf(w.kind, w.level, p.mu, p.sigma);
        if (w.kind == TGP_SIDE_COST) {
            dlf[k] = -p.dmu; dfl[k] = lf[k]; df[k] = -p.dmu;
        } else if (p.sigma != 0.0 && !isnan(lf[k])) {
            const double z = side_z(w.kind, w.level, p.mu, p.sigma);
            double ratio;
            (void)log_ndtr(z, ratio);
            const double dz = ((w.kind == TGP_SIDE_GE ? p.dmu : -p.dmu) - z * p.dsig) / p.sigma;
            dlf[k] = ratio * dz;
            dfl[k] = -0.5 * z * z;                   // grad f_k = phi(z_k) grad z_k
            df[k] = 0.3989422804014327 * dz;
        }
        logw = k == 0 ? lf[k] : logw + lf[k];
    }
    double val, gr;
    if (g.acq == TGP_ACQ_NONE) {
        val = weighted_value(g.acq, 0.0, logw, o.mu, o.sigma);
        gr = 0.0;
#pragma unroll
        for (int k = 0; k < WT_MAX_SIDES; ++k)
            if (k < g.K) gr += dlf[k];
    } else {
        const AcqCoef ac = acq_coef(g.acq, o.mu, o.sigma, g.sf, g.incumbent, g.param);
        val = weighted_value(g.acq, ac.a, logw, o.mu, o.sigma);
        gr = exp(logw) * (ac.cm * o.dmu + ac.cs * o.dsig);
#pragma unroll
        for (int k = 0; k < WT_MAX_SIDES; ++k) {
            if (k >= g.K || df[k] == 0.0 || ac.a == 0.0) continue;   // (a step function, a flat direction, no acquisition: no term)
            double rest = dfl[k];                    // log of what multiplies df_k: the others' log f_j (0 beyond K) and the side's own scale
#pragma unroll
            for (int j = 0; j < WT_MAX_SIDES; ++j)
                if (j != k) rest += lf[j];
            gr += ac.a * exp(rest) * df[k];
        }
    }
    if (isnan(val)) gr = NAN;
    g.grad[e] = gr;
    if (d == 0) g.val[q] = val;
}

static unsigned wt_grid(long M) { return (unsigned)std::min<long>((M + WT_BLOCK - 1) / WT_BLOCK, 4096); }

hipError_t launch_weight_accumulate(Context &c, const Context &g, int k, int kind, double level, double *logw, double *side_mu,
                                    double *side_sigma) {
    const long M = (long)c.M;
    hipLaunchKernelGGL(weight_accumulate_kernel, dim3(wt_grid(M)), dim3(WT_BLOCK), 0, c.stream, g.d_mu.get(), g.d_sigma.get(), M, kind,
                       level, k == 0 ? 1 : 0, logw, side_mu, side_sigma, g.d_besti.get(), c.d_besti.get());
    return hipGetLastError();
}

hipError_t launch_weight_value(Context &c, const SweepCall &s, int K, double *logw, double *val) {
    const long M = (long)c.M;
    hipLaunchKernelGGL(weight_value_kernel, dim3(wt_grid(M)), dim3(WT_BLOCK), 0, c.stream, c.d_mu.get(), c.d_sigma.get(), M, s.acq, s.sf,
                       s.incumbent, s.param, K > 0 ? 1 : 0, logw, c.d_acq.get(), val);
    return hipGetLastError();
}

hipError_t launch_weight_grad(Context &c, const WtGrad &g) {
    const long total = (long)g.m * g.D;
    hipLaunchKernelGGL(weight_grad_kernel, dim3((unsigned)((total + WT_BLOCK - 1) / WT_BLOCK)), dim3(WT_BLOCK), 0, c.stream, g);
    return hipGetLastError();
}

}  // namespace tgp
