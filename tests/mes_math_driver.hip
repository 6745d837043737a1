// Max-value entropy search's arithmetic alone (turbo_amd/csrc/mes_math.hpp), row by row, in one launch.
// Built and run by tests/test_gpu_mes_edges.py:   mes_math_driver <in> <out>
//   in : int64 R; then R rows of 70 doubles: g, mu, sigma, noise_var, sf, S, ystar[64]
//   out: R rows of 7 doubles: mes_h<false>(g); mes_h<true>(g) and its dh; mes_acq<false>; mes_acq<true> and its cm, cs
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../turbo_amd/csrc/mes_math.hpp"

#define CK(x)                                                                       \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
            exit(2);                                                                \
        }                                                                           \
    } while (0)

constexpr int ROW_IN = 6 + tgp::MES_MAXS, ROW_OUT = 7;

__global__ void mes_rows_kernel(const double *in, long R, double *out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R) return;
    const double *r = in + i * ROW_IN;
    double *o = out + i * ROW_OUT;
    const double g = r[0], mu = r[1], sigma = r[2], noise_var = r[3], sf = r[4];
    int S = (int)r[5];
    S = S < 1 ? 1 : S > tgp::MES_MAXS ? tgp::MES_MAXS : S;
    double dh0 = 0.0, dh1 = 0.0, cm0 = 0.0, cs0 = 0.0, cm = 0.0, cs = 0.0;
    o[0] = tgp::mes_h<false>(g, dh0);
    o[1] = tgp::mes_h<true>(g, dh1);
    o[2] = dh1;
    o[3] = tgp::mes_acq<false>(r + 6, S, noise_var, sf, mu, sigma, cm0, cs0);
    o[4] = tgp::mes_acq<true>(r + 6, S, noise_var, sf, mu, sigma, cm, cs);
    o[5] = cm;
    o[6] = cs;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: mes_math_driver <in> <out>\n");
        return 1;
    }
    FILE *f = fopen(argv[1], "rb");
    int64_t R = 0;
    if (!f || fread(&R, sizeof R, 1, f) != 1 || R < 1 || R > (1 << 20)) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    std::vector<double> in((size_t)R * ROW_IN), out((size_t)R * ROW_OUT);
    if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) {
        fprintf(stderr, "%s is short\n", argv[1]);
        return 1;
    }
    fclose(f);
    double *d_in = nullptr, *d_out = nullptr;
    CK(hipMalloc(&d_in, in.size() * sizeof(double)));
    CK(hipMalloc(&d_out, out.size() * sizeof(double)));
    CK(hipMemcpy(d_in, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
    CK(hipMemset(d_out, 0xff, out.size() * sizeof(double)));          // NaNs: a row that was not written shows
    hipLaunchKernelGGL(mes_rows_kernel, dim3((unsigned)((R + 255) / 256)), dim3(256), 0, 0, d_in, (long)R, d_out);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) {
        fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    fclose(f);
    CK(hipFree(d_in));
    CK(hipFree(d_out));
    printf("mes-math-driver ok %ld rows\n", (long)R);
    return 0;
}
