// ehvi_kernels.hip -- two-objective expected hypervolume improvement (tgp_sweep_ehvi, tgp_ehvi_grad; include/turbogp.h):
// the exact closed form for two independent GPs, a sum over the P + 1 strips of the Pareto front (P <= 256).  The per-model
// work is the existing predict-only sweep and the query kernels (tgp_api.hip); what is new is per candidate and
// compute-bound: behind both sweeps, which have left (mu_1, sigma_1) in h's and (mu_2, sigma_2) in g's d_mu / d_sigma,
//     ehvi_value_kernel   value = sum_i max(e_1(a_i) - e_1(a_{i+1}), 0) e_2(c_i)           2 (P + 1) evaluations of H
// in float64 whatever the dtypes, summed in the order i = 0, 1, ...; launch_argmax_of (integrate_kernels.hip) then takes
// the arg-max and packs the records.  For the gradient at m query points
//     ehvi_coef_kernel    per point: the value and the four partials in (m_1, sigma_1, m_2, sigma_2), one pass over the strips
//     ehvi_grad_kernel    per (point, dimension): sf_1 C_m1 dmu_1 + C_s1 dsigma_1 + sf_2 C_m2 dmu_2 + C_s2 dsigma_2
// (two launches: the D-fold recomputation of up to 257 strips is what the split avoids).  The closed form is
// ehvi_math.hpp's in both.  The 2 (P + 1) breakpoints are staged in LDS once per workgroup; the strip index is uniform
// across a wave, so every read of them is a broadcast.  No atomics: every element has one writer.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ehvi_math.hpp"
#include "tgp_internal.hpp"

namespace tgp {

constexpr int EH_BLOCK = 256;        // value kernel: 4 waves; the strips' arithmetic is f64 VALU, nothing to tile
constexpr int EH_QBLOCK = 64;        // coefficient kernel: one wave, so that 4096 points still spread over 64 workgroups
constexpr int EH_GRID_CAP = 768;     // value kernel: what is resident at once -- 130 VGPRs, 3 waves per SIMD, 3 workgroups on each of 256 CUs
                                     // (asking for 4 waves per SIMD made the compiler spill: profiles/ehvi_resources.txt) -- then the grid-stride loop
constexpr int EH_STRIPS = EHVI_MAX_FRONT + 1;

// front: [a_0 .. a_P | pad to EH_STRIPS | c_0 .. c_P | pad]; into LDS sa, sc (EH_STRIPS each)
template <int BLOCK>
__device__ __forceinline__ void ehvi_stage_front(const double *__restrict__ front, int P, double *sa, double *sc) {
    for (int i = threadIdx.x; i <= P; i += BLOCK) {
        sa[i] = front[i];
        sc[i] = front[EH_STRIPS + i];
    }
    __syncthreads();
}

// grid-stride over the M candidates; thread 0 of workgroup 0 also moves g's clamp count into h's counter and hands g's
// back at zero (one writer, ordered by the stream)
__global__ __launch_bounds__(EH_BLOCK) void ehvi_value_kernel(const double *__restrict__ mu1, const double *__restrict__ sg1,
                                                              const double *__restrict__ mu2, const double *__restrict__ sg2, long M,
                                                              const double *__restrict__ front, int P, double sf1, double sf2,
                                                              double *__restrict__ val, long long *g_cnt, long long *h_cnt) {
    __shared__ double sa[EH_STRIPS], sc[EH_STRIPS];
    ehvi_stage_front<EH_BLOCK>(front, P, sa, sc);
    const long stride = (long)gridDim.x * EH_BLOCK;
    for (long i = (long)blockIdx.x * EH_BLOCK + threadIdx.x; i < M; i += stride)
        val[i] = ehvi_point<false>(sa, sc, P, sf1 * mu1[i], sg1[i], sf2 * mu2[i], sg2[i]).val;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        h_cnt[1] += g_cnt[1];
        g_cnt[1] = 0;
    }
}

// one model's raw posterior at query point q from launch_query's sums r = [k.alpha, v.v, gm[0..D), gv[0..D)] --
// q_finalize_point's arithmetic -- or the model's own sweep's bits where the entry supplied them
__device__ __forceinline__ void eh_posterior(const EhviModel &w, const double *r, int q, double &mu, double &sigma, bool &pos, double &sn) {
    mu = w.y_std * r[0] + w.y_mean;
    double var = w.kss - r[1];
    pos = var > 0.0;
    if (!pos) var = 0.0;
    sn = sqrt(var);
    sigma = w.y_std * sn;
    if (w.mu) { mu = w.mu[q]; sigma = w.sigma[q]; }
}

// one thread per point: val[q] and coef[4 q ..] = [C_m1, C_s1, C_m2, C_s2]
__global__ __launch_bounds__(EH_QBLOCK) void ehvi_coef_kernel(EhviGrad g) {
    __shared__ double sa[EH_STRIPS], sc[EH_STRIPS];
    ehvi_stage_front<EH_QBLOCK>(g.front, g.P, sa, sc);
    const int q = blockIdx.x * EH_QBLOCK + threadIdx.x;
    if (q >= g.m) return;
    const long ro = (long)q * (2 + 2 * g.D);
    double m1, s1, m2, s2, sn;
    bool pos;
    eh_posterior(g.mdl[0], g.mdl[0].red + ro, q, m1, s1, pos, sn);
    eh_posterior(g.mdl[1], g.mdl[1].red + ro, q, m2, s2, pos, sn);
    const EhviPoint p = ehvi_point<true>(sa, sc, g.P, g.sf[0] * m1, s1, g.sf[1] * m2, s2);
    g.val[q] = p.val;
    double *c = g.coef + 4 * (long)q;
    c[0] = p.cm1; c[1] = p.cs1; c[2] = p.cm2; c[3] = p.cs2;
}

// one thread per (point, dimension), in the order of the header's sum; a model with sigma == 0 at the point contributes no
// sigma term; a NaN value gives a NaN gradient
__global__ __launch_bounds__(EH_BLOCK) void ehvi_grad_kernel(EhviGrad g) {
    const long e = (long)blockIdx.x * EH_BLOCK + threadIdx.x;
    const int D = g.D;
    if (e >= (long)g.m * D) return;
    const int q = (int)(e / D), d = (int)(e - (long)q * D);
    const long ro = (long)q * (2 + 2 * D);
    const double *c = g.coef + 4 * (long)q;
    double gr = 0.0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const EhviModel &w = g.mdl[j];
        const double *r = w.red + ro;
        double mu, sigma, sn;
        bool pos;
        eh_posterior(w, r, q, mu, sigma, pos, sn);
        const double dmu = -w.y_std * r[2 + d] / w.ls[d];
        const double dvar = 2.0 * r[2 + D + d] / w.ls[d];
        const double dsig = pos && sn > 0.0 && sigma != 0.0 ? w.y_std * dvar / (2.0 * sn) : 0.0;
        gr += g.sf[j] * c[2 * j] * dmu;
        if (dsig != 0.0) gr += c[2 * j + 1] * dsig;
    }
    if (isnan(g.val[q])) gr = NAN;
    g.grad[e] = gr;
}

hipError_t launch_ehvi_value(Context &c, const Context &g, const double *front, int P, double sf1, double sf2, double *val) {
    const long M = (long)c.M;
    const unsigned grid = (unsigned)std::min<long>((M + EH_BLOCK - 1) / EH_BLOCK, EH_GRID_CAP);
    hipLaunchKernelGGL(ehvi_value_kernel, dim3(grid), dim3(EH_BLOCK), 0, c.stream, c.d_mu.get(), c.d_sigma.get(), g.d_mu.get(),
                       g.d_sigma.get(), M, front, P, sf1, sf2, val, g.d_besti.get(), c.d_besti.get());
    return hipGetLastError();
}

hipError_t launch_ehvi_grad(Context &c, const EhviGrad &g) {
    hipLaunchKernelGGL(ehvi_coef_kernel, dim3((unsigned)((g.m + EH_QBLOCK - 1) / EH_QBLOCK)), dim3(EH_QBLOCK), 0, c.stream, g);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    const long total = (long)g.m * g.D;
    hipLaunchKernelGGL(ehvi_grad_kernel, dim3((unsigned)((total + EH_BLOCK - 1) / EH_BLOCK)), dim3(EH_BLOCK), 0, c.stream, g);
    return hipGetLastError();
}

}  // namespace tgp
