// nt_product.hpp -- ONE host-side description of an f64 product C = alpha * A * B^T (+ beta * C) with both operands
// K-contiguous, for the two kernels that compute it: the 64 x 64 tiles of gemm64_glds.hpp (GemmArgs) and the 128 x 128
// tiles of gemm_nt_glds.hpp (GemmNtArgs).  The callers choose between the two by size (TGP_TRAIL64, TGP_MERGE64,
// TGP_KINV64); the operands, leading dimensions, strides and scalars are the same nine values either way.
// The device structs and the kernels are untouched: this only fills them.
#pragma once
#include "gemm64_glds.hpp"
#include "gemm_nt_glds.hpp"

namespace tgp {

struct NtProduct {
    int device = 0;
    const double *A = nullptr; long lda = 0, strideA = 0;   // (rows, K) row-major
    const double *B = nullptr; long ldb = 0, strideB = 0;   // (cols, K) row-major
    double *C = nullptr; long ldc = 0, strideC = 0;         // (rows, cols) row-major
    double *Ct = nullptr; long ldct = 0, strideCt = 0;      // optional: C^T as well, (cols, rows) row-major
    int rows = 0, cols = 0;   // multiples of the tile the product is launched on
    int K = 0;
    double alpha = 1.0, beta = 0.0;   // beta is 0 or 1

    GemmArgs args64() const {
        GemmArgs g{};
        g.A = A; g.lda = lda; g.strideA = strideA;
        g.B = B; g.ldb = ldb; g.strideB = strideB;
        g.C = C; g.ldc = ldc; g.strideC = strideC;
        g.Ct = Ct; g.ldct = ldct; g.strideCt = strideCt;
        g.ntm = rows / 64; g.ntn = cols / 64; g.K = K; g.alpha = alpha; g.beta = beta;
        return g;
    }
    GemmNtArgs args128() const {
        GemmNtArgs g{};
        g.A = A; g.lda = lda; g.strideA = strideA;
        g.B = B; g.ldb = ldb; g.strideB = strideB;
        g.C = C; g.ldc = ldc; g.strideC = strideC;
        g.Ct = Ct; g.ldct = ldct; g.strideCt = strideCt;
        g.ntm = rows / 128; g.ntn = cols / 128; g.K = K; g.alpha = alpha; g.beta = beta;
        return g;
    }
    // nblocks tiles (what TMAP makes of the grid: all of it, or its lower triangle) of `batch` problems
    template <int KR, int TMAP>
    hipError_t on64(hipStream_t st, int nblocks, int batch) const {
        return launch_gemm64_glds<KR, TMAP>(st, device, args64(), nblocks, batch);
    }
    template <int KN, int TMAP>
    hipError_t on128(hipStream_t st, int nblocks, int batch) const {
        return launch_gemm_nt_glds<double, KN, TMAP>(st, device, args128(), nblocks, batch);
    }
};

}  // namespace tgp
