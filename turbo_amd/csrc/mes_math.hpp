// mes_math.hpp -- max-value entropy search (Wang & Jegelka 2017): the ONE place that holds h, dh/dgamma and the S-term
// average, shared by every sweep epilogue (finalize_kernel, small_sweep_kernel, mid_sweep_kernel) and by the query
// kernels' value + gradient, so the paths cannot drift apart ("Max-value entropy search").
//
//   sigma_f^2 = max(sigma^2 - noise y_std^2, 0)      the maxima y*_s are of the LATENT function
//   gamma_s   = sf (y*_s - mu) / sigma_f
//   h(gamma)  = gamma phi / (2 Phi) - log Phi          = H[N(0,1)] - H[N(0,1) truncated above at gamma] >= 0
//   a         = (1/S) sum_s h(gamma_s), s = 0, 1, ...;  a = 0 where sigma_f == 0
//   dh/dgamma = -(r/2)(1 + gamma^2 + gamma r),  r = phi / Phi          (gamma >= -10; below, see the last case)
//
// Always f64.  With z = |gamma| / sqrt 2 and e = erfcx(z) in (0, 1] -- one evaluation, never an overflow:
//   gamma <= 0:  Phi = e exp(-z^2) / 2, so  log Phi = log(e / 2) - z^2  and  r = sqrt(2/pi) / e  (no underflow anywhere)
//   gamma >  0:  q = e exp(-z^2) / 2 = 1 - Phi, so  log Phi = log1p(-q)  and  r = exp(-z^2) / (sqrt(2 pi) (1 - q))
//   gamma < -50: the two halves of h are each gamma^2 / 2 and cancel; the expansion of Mills' ratio in t = 1 / gamma^2 gives
//                h = log(-gamma) + (log(2 pi) - 1) / 2 + 2 t - 15/2 t^2 + 148/3 t^3
//                (next term ~ 4e2 t^4: 2.6e-12 of h just below the seam, measured against an 80-bit reference)
//   gamma < -10, the slope only (MES_DH_SEAM): 1 + gamma^2 + gamma r loses gamma^4 ulps (measured 8.9e-10 of dh at
//                gamma = -49.4).  With x = -gamma and Laplace's continued fraction T_k = x + k / T_(k+1):  r = T_1  and
//                1 + gamma^2 + gamma r = 2 / (T_2 T_3),  so  dh = -T_1 / (T_2 T_3),  every term positive.  Evaluated
//                backwards from T_17 = x (MES_DH_DEPTH = 16 levels; mes_dh_tail): the truncation is 1.4e-17 of dh at
//                x = 10 (1.9e-16 at x = 9: why the seam is not closer to 0) and falls with x, so dh is at rounding level
//                down to -DBL_MAX.
//                h keeps the erfcx route on [-50, -10) and its series below: mes_h<false> and mes_h<true> return the
//                same bits, and no sweep's output depends on the slope's form.
// so value and slope are finite for every finite gamma (dh = 0 where r has underflowed to 0).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace tgp {

constexpr int MES_MAXS = 64;       // most maxima a handle holds (tgp_mes_set_maxima)
constexpr double MES_DH_SEAM = -10.0;   // below it dh/dgamma comes from the continued fraction
constexpr int MES_DH_DEPTH = 16;

struct MesArgs {
    const double *ystar;           // (S) raw values of the sampled optimum, device memory
    int S;
    double noise_var;              // noise * y_std^2: what sigma^2 holds beyond the latent variance
};

// dh/dgamma for gamma < MES_DH_SEAM.  The fraction is evaluated without a division per level: with T_k = x a_k / a_(k+1)
// and t = 1 / x^2 the levels are  a_k = a_(k+1) + k t a_(k+2)  from a_17 = 1, a_16 = 1 + 16 t  (T_17 = x), every term
// positive and O(1), and  dh = -T_1 / (T_2 T_3) = -a_1 a_4 / (x a_2^2):  sixteen dependent FMAs and two divisions.  (One
// division per level, in one thread per query point, cost 0.9 us per maximum: a call with 64 maxima below the seam took
// 0.11 ms where the cancelling form took 0.05; this form takes 0.06.)  Within 5e-16 of the 80-bit value from -10 to
// -1e300; t underflows to 0 beyond 1e154 and leaves -1 / x.  Below -50 t is the series' own (1 / gamma)^2.
__device__ __forceinline__ double mes_dh_tail(double x, double t) {
    double hi = 1.0, lo = fma((double)MES_DH_DEPTH, t, 1.0);      // a_(k+2), a_(k+1)
    double a4 = 0.0;
#pragma unroll
    for (int k = MES_DH_DEPTH - 1; k >= 2; --k) {
        const double a = fma((double)k * t, hi, lo);
        hi = lo;
        lo = a;
        if (k == 4) a4 = a;
    }
    const double a1 = fma(t, hi, lo);                             // lo = a_2, hi = a_3
    return -(a1 * a4) / (x * lo * lo);
}

// (the seam of dh is tested inside the gamma <= 0 case: a positive gamma meets no branch it did not meet before)
template <bool GRAD>
__device__ __forceinline__ double mes_h(double g, double &dh) {
    if (g < -50.0) {
        const double ig = 1.0 / g, t = ig * ig;
        if (GRAD) dh = mes_dh_tail(-g, t);
        return log(-g) + 0.41893853320467274 + t * (2.0 + t * (-7.5 + t * (148.0 / 3.0)));
    }
    const double z = fabs(g) * 0.70710678118654752440;
    const double e = erfcx(z);
    double r, lp;
    if (g <= 0.0) {
        r = 0.79788456080286536 / e;
        lp = log(0.5 * e) - z * z;
        if (GRAD) dh = g < MES_DH_SEAM ? mes_dh_tail(-g, 1.0 / (g * g)) : -0.5 * r * (1.0 + g * g + g * r);
    } else {
        const double ez = exp(-z * z);
        const double q = 0.5 * e * ez;
        r = 0.3989422804014327 * ez / (1.0 - q);
        lp = log1p(-q);
        if (GRAD) dh = r == 0.0 ? 0.0 : -0.5 * r * (1.0 + g * g + g * r);
    }
    return 0.5 * g * r - lp;
}

// The acquisition at one candidate from S maxima ys (LDS in the sweeps: every lane reads the same address, a broadcast).
// GRAD: also cm = da / dmu and cs = da / dsigma (through sigma_f: d sigma_f / d sigma = sigma / sigma_f).
template <bool GRAD>
__device__ __forceinline__ double mes_acq(const double *ys, int S, double noise_var, double sf, double mu, double sigma,
                                          double &cm, double &cs) {
    if (GRAD) { cm = 0.0; cs = 0.0; }
    const double v = sigma * sigma - noise_var;
    if (!(v > 0.0)) return 0.0;
    const double sl = sqrt(v);
    double sum = 0.0, sdh = 0.0, sgdh = 0.0;
    for (int s = 0; s < S; ++s) {
        const double g = sf * (ys[s] - mu) / sl;
        double dh = 0.0;
        sum += mes_h<GRAD>(g, dh);
        if (GRAD) { sdh += dh; sgdh = fma(g, dh, sgdh); }
    }
    if (GRAD) {
        cm = -sf * sdh / (sl * (double)S);
        cs = -sgdh * sigma / (v * (double)S);
    }
    return sum / (double)S;
}

}  // namespace tgp
