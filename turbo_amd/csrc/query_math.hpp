// query_math.hpp -- the closed forms shared by the batched query kernels (query_kernels.hip) and the
// one-launch optimiser for small problems (refine_kernels.hip): the kernel's radial derivative
// weight and the acquisition as a function of (mu, sigma) with its two partials (its value: acq_math.hpp's formulas).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "acq_math.hpp"
#include "pairwise.hpp"
#include "tgp_internal.hpp"

namespace tgp {

// h(r) with dk/dx_d = -c h(r) (u_d - xs_d) / l_d   (as in the LML gradient)
template <int KIND>
__device__ __forceinline__ double h_weight(double d2) {
    if (KIND == TGP_RBF) {
        return exp(-0.5 * d2);
    } else if (KIND == TGP_MATERN12) {
        const double r = sqrt(d2);
        return r > 0.0 ? exp(-r) / r : 0.0;
    } else if (KIND == TGP_MATERN32) {
        return 3.0 * exp(-sqrt(3.0 * d2));
    } else {
        const double t = sqrt(5.0 * d2);
        return 5.0 / 3.0 * (t + 1.0) * exp(-t);
    }
}

// acq = f(mu, sigma) and its partials: d acq = cm dmu + cs dsigma
// (turbo/modules/acquisition_functions.py:147-158 UCB, :225-247 PI, :336-358 EI)
struct AcqCoef { double a, cm, cs; };
__device__ __forceinline__ AcqCoef acq_coef(int acq, double mu, double sigma, double sf, double incumbent, double param) {
    AcqCoef r{0.0, 0.0, 0.0};
    if (acq == TGP_ACQ_NONE) {
        r.a = mu; r.cm = 1.0;
    } else if (acq == TGP_ACQ_UCB) {
        r.a = ucb_value(sf, param, mu, sigma); r.cm = sf; r.cs = param;
    } else if (acq == TGP_ACQ_SIGMA) {
        r.a = sigma; r.cs = 1.0;
    } else if (sigma != 0.0) {
        const double diff = acq_diff(sf, incumbent, param, mu);
        const double Z = diff / sigma;
        const double pdf = norm_pdf(Z);
        const double cdf = ndtr(Z);
        if (acq == TGP_ACQ_PI) {
            r.a = cdf; r.cm = pdf * sf / sigma; r.cs = -pdf * Z / sigma;
        } else {
            r.a = ei_value(diff, sigma, cdf, pdf); r.cm = sf * cdf; r.cs = pdf;
        }
    }
    return r;
}

// max-value entropy search (mes_math.hpp): the value and its partials from the handle's S maxima, read from device memory
// at one address for every lane (a query batch is a few points: nothing to stage)
__device__ __forceinline__ AcqCoef mes_coef(const MesArgs &m, double mu, double sigma, double sf) {
    AcqCoef r{0.0, 0.0, 0.0};
    r.a = mes_acq<true>(m.ystar, m.S, m.noise_var, sf, mu, sigma, r.cm, r.cs);
    return r;
}

}  // namespace tgp
