// integrate_kernels.hip -- the integrated acquisition of tgp_sweep_integrated (Snoek et al. 2012): the acquisition
// averaged over S samples theta_k of the hyper-parameters, and the moments of the equal-weight mixture of the S
// posteriors.  The per-sample work is the existing fit and predict-only sweep (tgp_api.hip); what is new is per candidate
// and memory-bound: after sample k's sweep has left mu_k, sigma_k in c.d_mu / c.d_sigma,
//     integrate_accumulate_kernel   A += acq(mu_k, sigma_k),  M1 += mu_k,  M2 += sigma_k^2 + mu_k^2    (stored at k = 0)
// and after the last sample
//     integrate_final_kernel        a = A / S,  mu = M1 / S,  sigma = sqrt(max(0, M2 / S - mu^2)),  arg-max of a
// in float64 whatever the handle's dtype, summed in the order k = 0, 1, ... so the average is the one a caller forms
// from S plain sweeps.  The acquisition and the "(larger value, then lower index)" arg-max come from acq_math.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "acq_math.hpp"
#include "tgp_internal.hpp"

namespace tgp {

constexpr int INT_BLOCK = 256;

// grid-stride over the M candidates
__global__ __launch_bounds__(INT_BLOCK) void integrate_accumulate_kernel(const double *__restrict__ mu,
                                                                         const double *__restrict__ sigma, long M, int acq,
                                                                         double sf, double incumbent, double param, int first,
                                                                         double *__restrict__ sum_a, double *__restrict__ sum_mu,
                                                                         double *__restrict__ sum_m2) {
    const long stride = (long)gridDim.x * INT_BLOCK;
    for (long i = (long)blockIdx.x * INT_BLOCK + threadIdx.x; i < M; i += stride) {
        const double m = mu[i], s = sigma[i];
        const double a = acq_value(acq, sf, incumbent, param, m, s);
        const double m2 = s * s + m * m;
        if (first) {
            sum_a[i] = a; sum_mu[i] = m; sum_m2[i] = m2;
        } else {
            sum_a[i] += a; sum_mu[i] += m; sum_m2[i] += m2;
        }
    }
}

struct IntFinal {
    const double *sum_a, *sum_mu, *sum_m2;
    long M; int S; int acq;
    double *mu, *sigma, *acqv;       // nullable (M,) outputs
    double *bval; long long *bidx;   // one arg-max partial per workgroup of phase 0
    long nblk;                       // phase 1: partials to reduce (0 without an acquisition)
    double *best; long long *besti;  // [0] value / [0] index, [1] the clamp count of the S sweeps
    double *winner; const double *cand; int D; long long global_offset;   // the (D + 2) record, or null
    double *res_host;                // device-mapped [best value, best index, clamp count], or null
};

// phase 0 (one workgroup per INT_BLOCK candidates): the averages, the outputs and the workgroup's arg-max partial;
// phase 1 (one workgroup, the next launch): the partials' arg-max, the result record and the winner record, as
// argmax_final_kernel leaves them behind a plain sweep
__global__ __launch_bounds__(INT_BLOCK) void integrate_final_kernel(IntFinal f, int phase) {
    __shared__ double sv[INT_BLOCK];
    __shared__ long long si[INT_BLOCK];
    const int tid = threadIdx.x;
    if (phase == 0) {
        const long i = (long)blockIdx.x * INT_BLOCK + tid;
        Best best;
        if (i < f.M) {
            const double n = (double)f.S;
            const double a = f.sum_a[i] / n;
            const double mu = f.sum_mu[i] / n;
            double var = f.sum_m2[i] / n - mu * mu;
            if (var < 0.0) var = 0.0;            // (a NaN stays a NaN)
            if (f.mu) f.mu[i] = mu;
            if (f.sigma) f.sigma[i] = sqrt(var);
            if (f.acqv) f.acqv[i] = a;
            if (f.acq != TGP_ACQ_NONE) best = candidate(a, i);
        }
        if (f.acq == TGP_ACQ_NONE) return;       // (uniform: nobody reaches the barrier below)
        best = block_argmax<INT_BLOCK>(best, sv, si);
        if (tid == 0) { f.bval[blockIdx.x] = best.v; f.bidx[blockIdx.x] = best.i; }
        return;
    }
    const Best all = block_argmax<INT_BLOCK>(strided_argmax<INT_BLOCK>(f.bval, f.bidx, f.nblk), sv, si);
    if (tid == 0) {
        if (f.nblk > 0) { f.best[0] = all.v; f.besti[0] = all.i; }
        if (f.res_host) {
            f.res_host[0] = all.v;
            f.res_host[1] = (double)((all.i >= f.M) ? 0 : all.i);
            f.res_host[2] = (double)f.besti[1];
            f.besti[1] = 0;                      // the clamp counter is handed back at zero
        }
    }
    if (f.winner && f.nblk > 0) {
        const long long wi = (all.i >= f.M) ? 0 : all.i;      // all-NaN batch: index 0, as tgp_sweep reports
        if (tid == 0) { f.winner[0] = all.v; f.winner[1] = (double)(f.global_offset + wi); }
        for (int d = tid; d < f.D; d += INT_BLOCK) f.winner[2 + d] = f.cand[wi * f.D + d];
    }
}

hipError_t launch_integrate_accumulate(Context &c, const SweepCall &s, int k) {
    const long M = (long)c.M;
    const unsigned grid = (unsigned)std::min<long>((M + INT_BLOCK - 1) / INT_BLOCK, 4096);
    hipLaunchKernelGGL(integrate_accumulate_kernel, dim3(grid), dim3(INT_BLOCK), 0, c.stream, c.d_mu.get(), c.d_sigma.get(), M,
                       s.acq, s.sf, s.incumbent, s.param, k == 0 ? 1 : 0, c.d_int_a.get(), c.d_int_mu.get(), c.d_int_m2.get());
    return hipGetLastError();
}

static hipError_t launch_final(Context &c, const SweepCall &s, IntFinal f);

// s.mu / s.sigma / s.acqv: where the averaged outputs go (device memory, nullable); s.res, s.winner as for a plain sweep
hipError_t launch_integrate_final(Context &c, const SweepCall &s, int S) {
    IntFinal f{};
    f.sum_a = c.d_int_a; f.sum_mu = c.d_int_mu; f.sum_m2 = c.d_int_m2;
    f.S = S;
    f.mu = s.mu; f.sigma = s.sigma; f.acqv = s.acqv;
    return launch_final(c, s, f);
}

// one "sample" whose sums are the values themselves (a / 1 is exact) and no (M,) output: the arg-max and the records alone
hipError_t launch_argmax_of(Context &c, const SweepCall &s, const double *vals) {
    IntFinal f{};
    f.sum_a = f.sum_mu = f.sum_m2 = vals;
    f.S = 1;
    return launch_final(c, s, f);
}

static hipError_t launch_final(Context &c, const SweepCall &s, IntFinal f) {
    f.M = (long)c.M; f.acq = s.acq;
    f.bval = c.d_bval; f.bidx = c.d_bidx;
    const long nblk = (f.M + INT_BLOCK - 1) / INT_BLOCK;
    f.nblk = s.acq != TGP_ACQ_NONE ? nblk : 0;
    f.best = c.d_best; f.besti = c.d_besti;
    f.winner = s.acq != TGP_ACQ_NONE ? s.winner : nullptr;
    f.cand = c.d_cand; f.D = (int)c.D; f.global_offset = (long long)c.winner_offset;
    f.res_host = s.res;
    hipLaunchKernelGGL(integrate_final_kernel, dim3((unsigned)nblk), dim3(INT_BLOCK), 0, c.stream, f, 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(integrate_final_kernel, dim3(1), dim3(INT_BLOCK), 0, c.stream, f, 1);
    return hipGetLastError();
}

}  // namespace tgp
