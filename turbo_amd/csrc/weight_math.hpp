// weight_math.hpp -- the ONE place that holds the feasibility / cost weight of tgp_sweep_weighted and tgp_weighted_grad
// (include/turbogp.h): log Phi and phi / Phi through the scaled complementary error function, a side's log f_k as a
// function of its (mu_k, sigma_k), and the value formed from the acquisition and the summed log weight.  The sweep
// epilogue (weight_accumulate_kernel, weight_value_kernel) and the gradient's combination (weight_grad_kernel) take them
// from here, so the two cannot drift apart.
//
// With x = |z| / sqrt 2 and e = erfcx(x) in (0, 1] -- mes_math.hpp's route:
//   z <= 0:  Phi = e exp(-x^2) / 2, so  log Phi = log(e / 2) - x^2  and  phi / Phi = sqrt(2 / pi) / e   (no underflow anywhere)
//   z >  0:  q = e exp(-x^2) / 2 = 1 - Phi, so  log Phi = log1p(-q)  and  phi / Phi = exp(-x^2) / (sqrt(2 pi) (1 - q))
// finite for every finite z whose square is finite; never log(ndtr(z)).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/turbogp.h"

namespace tgp {

// log Phi(z); ratio = phi(z) / Phi(z)
__device__ __forceinline__ double log_ndtr(double z, double &ratio) {
    const double x = fabs(z) * 0.70710678118654752440;
    const double e = erfcx(x);
    if (z <= 0.0) {
        ratio = 0.79788456080286536 / e;
        return log(0.5 * e) - x * x;
    }
    const double ez = exp(-x * x);
    const double q = 0.5 * e * ez;
    ratio = 0.3989422804014327 * ez / (1.0 - q);
    return log1p(-q);
}

// a side's standardised distance to its level (GE / LE, sigma != 0)
__device__ __forceinline__ double side_z(int kind, double level, double mu, double sigma) {
    return (kind == TGP_SIDE_GE ? mu - level : level - mu) / sigma;
}

// log f_k from the side's raw posterior: log Phi(z_k) for a constraint (a step function at sigma_k == 0, equality
// holding), -mu_k for a cost; a NaN in mu_k or sigma_k gives NaN
__device__ __forceinline__ double side_logf(int kind, double level, double mu, double sigma) {
    if (isnan(mu) || isnan(sigma)) return NAN;
    if (kind == TGP_SIDE_COST) return -mu;
    if (sigma == 0.0) {
        const bool holds = kind == TGP_SIDE_GE ? mu >= level : mu <= level;
        return holds ? 0.0 : -INFINITY;
    }
    double r;
    return log_ndtr(side_z(kind, level, mu, sigma), r);
}

// the weighted value: a exp(logw) for EI / PI -- exactly 0 where a == 0 or logw == -inf -- and logw itself for
// TGP_ACQ_NONE (the pure feasibility search, kept in logs); NaN where the objective's or any side's posterior is NaN
__device__ __forceinline__ double weighted_value(int acq, double a, double logw, double mu, double sigma) {
    if (isnan(mu) || isnan(sigma) || isnan(logw) || isnan(a)) return NAN;
    if (acq == TGP_ACQ_NONE) return logw;
    if (a == 0.0 || logw == -INFINITY) return 0.0;
    return a * exp(logw);
}

}  // namespace tgp
