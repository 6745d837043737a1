// ehvi_math.hpp -- the ONE place that holds the closed form of the two-objective expected hypervolume improvement
// (include/turbogp.h): H(z) = phi(z) + z Phi(z), e_j(t) = sigma_j H((m_j - t) / sigma_j), the strip term and the four
// coefficient terms.  The sweep epilogue (ehvi_value_kernel) and the gradient's coefficients (ehvi_coef_kernel) are both
// ehvi_point<GRAD> below, so a point's value is the same bits in both.
//
// With x = |z| / sqrt 2 and ex = erfcx(x) in (0, 1] -- mes_math.hpp's and weight_math.hpp's route:
//   z <= 0:  phi = exp(-x^2) / sqrt(2 pi),  Phi = ex exp(-x^2) / 2,  H = exp(-x^2) (1 / sqrt(2 pi) - x ex / sqrt 2)
//            one exponential scales the whole bracket: the two halves of H are never formed as separate tails.  The bracket
//            loses z^2 ulps to cancellation -- H's own condition number in z -- and exp(-x^2) leaves the double range near
//            z = -38.4: the value is then exactly 0 (there is no log form).
//   z >  0:  e = d Phi + sigma phi with d = m - t: acq_math.hpp's ei_value, the bits of TGP_ACQ_EI at incumbent t, xi = 0.
// sigma == 0: e = max(m - t, 0), Phi a step function (0 at d <= 0), phi = 0.  t = +inf: every term 0.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "acq_math.hpp"

namespace tgp {

constexpr int EHVI_MAX_FRONT = TGP_EHVI_MAX_FRONT;

// e(t), Phi(z(t)), phi(z(t)) of one model at one breakpoint
struct EhviE { double e, cdf, pdf; };

template <bool GRAD>
__device__ __forceinline__ EhviE ehvi_e(double m, double sigma, double t) {
    EhviE r;
    const double d = m - t;
    if (sigma == 0.0) {
        r.e = d > 0.0 ? d : 0.0;
        r.cdf = d > 0.0 ? 1.0 : 0.0;
        r.pdf = 0.0;
        return r;
    }
    const double z = d / sigma;
    if (z > 0.0) {
        r.cdf = ndtr(z);
        r.pdf = norm_pdf(z);
        r.e = ei_value(d, sigma, r.cdf, r.pdf);
        return r;
    }
    const double x = -z * 0.70710678118654752440;
    const double ex = erfcx(x);
    const double g = exp(-(x * x));
    r.e = sigma * (g * fma(-0.70710678118654752440 * x, ex, 0.3989422804014327));
    if (GRAD) {
        r.cdf = 0.5 * ex * g;
        r.pdf = 0.3989422804014327 * g;
    } else {
        r.cdf = 0.0;
        r.pdf = 0.0;
    }
    return r;
}

struct EhviPoint { double val, cm1, cs1, cm2, cs2; };

// the value and (GRAD) its partials in (m_1, sigma_1, m_2, sigma_2) at one point: the P + 1 strips in the order
// i = 0, 1, ...; a (P + 1) breakpoints and c (P + 1) levels are read at wave-uniform addresses (LDS: a broadcast).
// e_1(a_{i+1}) of strip i is e_1(a_i) of strip i + 1: two evaluations per strip.  A NaN in any input: NaN throughout.
template <bool GRAD>
__device__ __forceinline__ EhviPoint ehvi_point(const double *a, const double *c, int P, double m1, double s1, double m2, double s2) {
    EhviPoint o{0.0, 0.0, 0.0, 0.0, 0.0};
    if (isnan(m1) || isnan(s1) || isnan(m2) || isnan(s2)) {
        o.val = NAN;
        if (GRAD) { o.cm1 = NAN; o.cs1 = NAN; o.cm2 = NAN; o.cs2 = NAN; }
        return o;
    }
    EhviE lo = ehvi_e<GRAD>(m1, s1, a[0]);
    for (int i = 0; i <= P; ++i) {
        EhviE hi{0.0, 0.0, 0.0};                       // t = +inf
        if (i < P) hi = ehvi_e<GRAD>(m1, s1, a[i + 1]);
        const EhviE w = ehvi_e<GRAD>(m2, s2, c[i]);
        const double de = lo.e - hi.e;
        o.val = fma(de > 0.0 ? de : 0.0, w.e, o.val);
        if (GRAD) {
            o.cm1 = fma(lo.cdf - hi.cdf, w.e, o.cm1);
            o.cs1 = fma(lo.pdf - hi.pdf, w.e, o.cs1);
            o.cm2 = fma(de, w.cdf, o.cm2);
            o.cs2 = fma(de, w.pdf, o.cs2);
        }
        lo = hi;
    }
    return o;
}

}  // namespace tgp
