// warp_math.hpp -- the Kumaraswamy input warp (Snoek, Swersky, Zemel, Adams, ICML 2014): the ONE place that holds the warp,
// its three derivatives and its inverse, shared by the device kernels (warp_kernels.hip) and the host backend
// (host_backend.cpp: plain g++, no HIP header), so the two cannot drift apart ("Learned input warping").
//
//   u  = clip((x - lo) / (hi - lo), 0, 1)                 per dimension, box [lo, hi], shapes a, b > 0
//   w  = 1 - (1 - u^a)^b                                  the Kumaraswamy CDF: monotone, w(0) = 0, w(1) = 1
//
// Always f64, everything through logarithms so that neither end of the interval cancels.  With
//   lu = log u,   x = a lu = log u^a,   t = log(1 - u^a) = log1mexp(x):
//   w      = -expm1(b t)
//   dw/du  = a b u^(a-1) (1 - u^a)^(b-1)   = a b exp((a - 1) lu + (b - 1) t)
//   dw/da  = b (1 - u^a)^(b-1) u^a log u   = b lu exp((b - 1) t + x)
//   dw/db  = -(1 - u^a)^b log(1 - u^a)     = -t exp(b t)
// log1mexp(x) = log(1 - e^x), x <= 0, is log1p(-exp(x)) up to x = -log 2 and log(-expm1(x)) above: the first form alone
// rounds 1 - u^a to a multiple of 2^-53 and loses every digit of t at u = 1 - 2^-53.
// Endpoints: u = 0 gives w = 0 and u = 1 gives w = 1 EXACTLY (log 0 = -inf, exp(-inf) = 0, log1p(-0) = -0, expm1(-0) = -0;
// log 1 = 0, expm1(0) = 0, log 0 = -inf, expm1(-inf) = -1).  dw/da and dw/db are 0 at both endpoints, their limit where the
// closed form is 0 * inf.  dw/du at u = 0 is 0 (a > 1), b (a = 1) or +inf (a < 1), at u = 1 it is 0 (b > 1), a (b = 1) or
// +inf (b < 1): returned as such -- nothing on the optimisation path uses it (the gradient stage runs in warped
// coordinates).  a == 1 and b == 1 exactly: w = u exactly, the identity warp is a plain rescale to the unit cube.
//
//   inverse:  u = (1 - (1 - w)^(1/b))^(1/a) = exp(log1mexp(log1p(-w) / b) / a),   x = lo + u (hi - lo)
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define TGP_WARP_HD __host__ __device__ __forceinline__
#else
#define TGP_WARP_HD inline
#endif

namespace tgp {

// log(1 - e^x) for x <= 0 (x = -0: -inf; x = -inf: -0)
TGP_WARP_HD double warp_log1mexp(double x) {
    return x > -0.6931471805599453 ? log(-expm1(x)) : log1p(-exp(x));
}

TGP_WARP_HD double warp_unit(double x, double lo, double hi) {
    const double u = (x - lo) / (hi - lo);
    return fmin(fmax(u, 0.0), 1.0);
}

// w(u) for u in [0, 1]; d.du, d.da, d.db receive dw/du, dw/da, dw/db where the flag asks for them (else 0)
struct WarpDerivs { double du, da, db; };
TGP_WARP_HD double warp_value(double u, double a, double b, bool want_du, bool want_da, bool want_db, WarpDerivs &d) {
    const double lu = log(u);                    // -inf at 0
    const double x = a * lu;
    const double t = warp_log1mexp(x);           // -0 at u = 0, -inf at u = 1
    const bool inner = u > 0.0 && u < 1.0;
    d.du = d.da = d.db = 0.0;
    if (want_du) {
        const double ea = a == 1.0 ? 0.0 : (a - 1.0) * lu;      // (0 * inf at the wall is the factor 1)
        const double eb = b == 1.0 ? 0.0 : (b - 1.0) * t;
        d.du = a * b * exp(ea + eb);
    }
    if (want_da && inner) d.da = b * lu * exp((b == 1.0 ? 0.0 : (b - 1.0) * t) + x);
    if (want_db && inner) d.db = -t * exp(b * t);
    if (a == 1.0 && b == 1.0) return u;
    const double w = -expm1(b * t);
    return w == 0.0 ? 0.0 : w;                   // (+0.0 at u = 0 whatever sign the library's expm1 gives its zero)
}

// u(w) for w in [0, 1] (clipped)
TGP_WARP_HD double warp_inverse_unit(double w, double a, double b) {
    w = fmin(fmax(w, 0.0), 1.0);
    if (a == 1.0 && b == 1.0) return w;
    const double y = log1p(-w) / b;              // log (1 - w)^(1/b): -0 at w = 0, -inf at w = 1
    return exp(warp_log1mexp(y) / a);
}

// hi > lo, both finite with a finite range; a, b finite and > 0
TGP_WARP_HD bool warp_params_ok(double lo, double hi, double a, double b) {
    return hi > lo && isfinite(hi - lo) && isfinite(lo) && a > 0.0 && b > 0.0 && isfinite(a) && isfinite(b);
}

}  // namespace tgp
