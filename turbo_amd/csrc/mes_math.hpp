// mes_math.hpp -- max-value entropy search (Wang & Jegelka 2017): the ONE place that holds h, dh/dgamma and the S-term
// average, shared by every sweep epilogue (finalize_kernel, small_sweep_kernel, mid_sweep_kernel) and by the query
// kernels' value + gradient, so the paths cannot drift apart ("Max-value entropy search").
//
//   sigma_f^2 = max(sigma^2 - noise y_std^2, 0)      the maxima y*_s are of the LATENT function
//   gamma_s   = sf (y*_s - mu) / sigma_f
//   h(gamma)  = gamma phi / (2 Phi) - log Phi          = H[N(0,1)] - H[N(0,1) truncated above at gamma] >= 0
//   a         = (1/S) sum_s h(gamma_s), s = 0, 1, ...;  a = 0 where sigma_f == 0
//   dh/dgamma = -(r/2)(1 + gamma^2 + gamma r),  r = phi / Phi
//
// Always f64.  With z = |gamma| / sqrt 2 and e = erfcx(z) in (0, 1] -- one evaluation, never an overflow:
//   gamma <= 0:  Phi = e exp(-z^2) / 2, so  log Phi = log(e / 2) - z^2  and  r = sqrt(2/pi) / e  (no underflow anywhere)
//   gamma >  0:  q = e exp(-z^2) / 2 = 1 - Phi, so  log Phi = log1p(-q)  and  r = exp(-z^2) / (sqrt(2 pi) (1 - q))
//   gamma < -50: the two halves of h are each gamma^2 / 2 and cancel, and 1 + gamma^2 + gamma r loses gamma^4 ulps; the
//                expansion of Mills' ratio in t = 1 / gamma^2 gives
//                h = log(-gamma) + (log(2 pi) - 1) / 2 + 2 t - 15/2 t^2 + 148/3 t^3,  dh = (1 - 4 t + 30 t^2 - 296 t^3) / gamma
//                (next terms ~ 4e2 t^4: below 1e-10 there, where the erfcx route has lost as much)
// so value and slope are finite for every finite gamma (dh = 0 where r has underflowed to 0).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace tgp {

constexpr int MES_MAXS = 64;       // most maxima a handle holds (tgp_mes_set_maxima)

struct MesArgs {
    const double *ystar;           // (S) raw values of the sampled optimum, device memory
    int S;
    double noise_var;              // noise * y_std^2: what sigma^2 holds beyond the latent variance
};

template <bool GRAD>
__device__ __forceinline__ double mes_h(double g, double &dh) {
    if (g < -50.0) {
        const double ig = 1.0 / g, t = ig * ig;
        if (GRAD) dh = ig * (1.0 + t * (-4.0 + t * (30.0 - 296.0 * t)));
        return log(-g) + 0.41893853320467274 + t * (2.0 + t * (-7.5 + t * (148.0 / 3.0)));
    }
    const double z = fabs(g) * 0.70710678118654752440;
    const double e = erfcx(z);
    double r, lp;
    if (g <= 0.0) {
        r = 0.79788456080286536 / e;
        lp = log(0.5 * e) - z * z;
    } else {
        const double ez = exp(-z * z);
        const double q = 0.5 * e * ez;
        r = 0.3989422804014327 * ez / (1.0 - q);
        lp = log1p(-q);
    }
    if (GRAD) dh = r == 0.0 ? 0.0 : -0.5 * r * (1.0 + g * g + g * r);
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
