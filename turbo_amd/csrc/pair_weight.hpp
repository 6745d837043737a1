// pair_weight.hpp -- the pair weight G_ij of the traces 1/2 tr(G dK) as a compile-time policy: everything behind it
// (distances, ls_weight, the ARD passes, the sums) is one spelling for every G.  grad_kernels.hip: the LML's and the
// leave-one-out score's gradients in the hyper-parameters; warp_kernels.hip: the LML's gradient in the training inputs.
#pragma once
#include <hip/hip_runtime.h>

namespace tgp {

struct LmlPairWeight {      // G = alpha alpha^T - K^-1: the log marginal likelihood
    const double *__restrict__ alpha;
    const double *__restrict__ Kinv;      // lower triangle read
    __device__ double row(int i) const { return alpha[i]; }
    __device__ double G(double ai, int, int j, long lower) const { return ai * alpha[j] - Kinv[lower]; }
};
struct LooPairWeight {      // G = b alpha^T + alpha b^T - 2 B: the leave-one-out score (loo_kernels.hip)
    const double *__restrict__ alpha;
    const double *__restrict__ b;
    const double *__restrict__ B;         // lower triangle read
    __device__ double row(int i) const { return alpha[i]; }
    __device__ double G(double ai, int i, int j, long lower) const { return (b[i] * alpha[j] + ai * b[j]) - 2.0 * B[lower]; }
};

}  // namespace tgp
