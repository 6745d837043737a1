// acq_math.hpp -- the one device home of the acquisition closed forms and of the "(larger value, then lower index)"
// arg-max: every sweep epilogue (sweep_kernels.hip, small_kernels.hip, batch_kernels.hip, ts_kernels.hip) and the query
// kernels' value-with-partials (query_math.hpp) take them from here, so the copies cannot drift.  The host twin is
// host_backend.cpp (plain g++, -ffp-contract=off, no HIP header): it keeps its own ndtr and its own EI / PI / UCB lines.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/turbogp.h"

namespace tgp {

// scipy.special.ndtr (cephes ndtr.c) behind scipy.stats.norm.cdf (scipy/stats/_continuous_distns.py:368-369)
__device__ __forceinline__ double ndtr(double a) {
    constexpr double RSQRT2 = 0.70710678118654752440;
    const double x = a * RSQRT2;
    const double z = fabs(x);
    double y;
    if (z < RSQRT2) {
        y = 0.5 + 0.5 * erf(x);
    } else {
        y = 0.5 * erfc(z);
        if (x > 0) y = 1.0 - y;
    }
    return y;
}

// the pieces of EI / PI / UCB (turbo/modules/acquisition_functions.py:147-158 UCB, :225-247 PI, :336-358 EI): acq_value
// below and acq_coef (query_math.hpp, which also needs the partials) are both made of these and of nothing else
__device__ __forceinline__ double ucb_value(double sf, double param, double mu, double sigma) { return sf * mu + param * sigma; }
__device__ __forceinline__ double acq_diff(double sf, double incumbent, double param, double mu) { return sf * (mu - incumbent) - param; }
__device__ __forceinline__ double norm_pdf(double Z) { return exp(-(Z * Z) / 2.0) / 2.5066282746310002; }
__device__ __forceinline__ double ei_value(double diff, double sigma, double cdf, double pdf) { return diff * cdf + sigma * pdf; }

// the acquisition at (mu, sigma), raw units: 0 for TGP_ACQ_NONE (and for TGP_ACQ_MES, whose instances override it with
// mes_acq), 0 for PI / EI at sigma == 0
__device__ __forceinline__ double acq_value(int acq, double sf, double incumbent, double param, double mu, double sigma) {
    double a = 0.0;
    if (acq == TGP_ACQ_UCB) {
        a = ucb_value(sf, param, mu, sigma);
    } else if (acq == TGP_ACQ_SIGMA) {
        a = sigma;
    } else if (acq == TGP_ACQ_PI || acq == TGP_ACQ_EI) {
        if (sigma != 0.0) {
            const double diff = acq_diff(sf, incumbent, param, mu);
            const double Z = diff / sigma;
            if (acq == TGP_ACQ_PI) {
                a = ndtr(Z);
            } else {
                const double pdf = norm_pdf(Z);
                a = ei_value(diff, sigma, ndtr(Z), pdf);
            }
        }
    }
    return a;
}

// ---- arg-max: the larger value wins, the lower index among equal values ----
constexpr long long IDX_NONE = 0x7fffffffffffffffLL;
struct Best {
    double v = -INFINITY;          // the empty value: loses to everything, every index beats it
    long long i = IDX_NONE;
};

__device__ __forceinline__ bool better(double v2, long long i2, double v, long long i) {
    return v2 > v || (v2 == v && i2 < i);
}
__device__ __forceinline__ void take_better(Best &b, double v2, long long i2) {
    if (better(v2, i2, b.v, b.i)) { b.v = v2; b.i = i2; }
}

// a candidate's entry: a NaN value never wins, but its index still takes part (an all-NaN batch reports its lowest index)
__device__ __forceinline__ Best candidate(double a, long long index) {
    Best b;
    if (!isnan(a)) b.v = a;
    b.i = index;
    return b;
}

// over the 64 lanes of a wave; every lane ends with the result
__device__ __forceinline__ Best wave_argmax(Best b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double v2 = __shfl_xor(b.v, o, 64);
        const long long i2 = __shfl_xor(b.i, o, 64);
        take_better(b, v2, i2);
    }
    return b;
}
__device__ __forceinline__ int wave_sum(int n) {   // (the clamp count that rides along with wave_argmax)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    return n;
}

// over a workgroup of BLOCK threads through the caller's LDS (BLOCK entries each); every thread ends with the result
template <int BLOCK>
__device__ __forceinline__ Best block_argmax(Best b, double *sv, long long *si) {
    const int tid = threadIdx.x;
    sv[tid] = b.v;
    si[tid] = b.i;
    __syncthreads();
    for (int o = BLOCK / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double v2 = sv[tid + o];
            const long long i2 = si[tid + o];
            if (better(v2, i2, sv[tid], si[tid])) { sv[tid] = v2; si[tid] = i2; }
        }
        __syncthreads();
    }
    b.v = sv[0];
    b.i = si[0];
    return b;
}

// this thread's share of nblk per-block partials, BLOCK apart
template <int BLOCK>
__device__ __forceinline__ Best strided_argmax(const double *__restrict__ bval, const long long *__restrict__ bidx, long nblk) {
    Best b;
    for (long k = threadIdx.x; k < nblk; k += BLOCK) take_better(b, bval[k], bidx[k]);
    return b;
}

}  // namespace tgp
