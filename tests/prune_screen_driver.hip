// The pruned sweep's screen (turbo_amd/csrc/prune_screen.hpp) candidate by candidate: mu_s, E and the exact path's mean.
// Built and run by tests/test_gpu_prune_screen.py:   prune_screen_driver <splits> <in> <out> [<in> <out> ...]
//   in : int32 N, M, Dp, D; double constant; float Xs[N][Dp]; float Cs[M][Dp]; double alpha[N]   (M a multiple of 128)
//   out: double mu_s[M]; double E[M]; double mu_exact[M]
// The exact path is restated here as one thread per candidate: the direct difference summed in dimension order with fmaf,
// the same exp2 sequence, an f64 fma per training point (kstar_kernel's / MeanAcc's arithmetic up to the order of the f64 sum).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../turbo_amd/csrc/prune_screen.hpp"

#define CK(x)                                                                       \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
            exit(2);                                                                \
        }                                                                           \
    } while (0)

__global__ void exact_mean_kernel(const float *Cs, const float *Xs, const double *alpha, int M, int N, int Dp, double constant,
                                  double *mu) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= M) return;
    const float log2c = log2f((float)constant);
    double s = 0.0;
    for (int i = 0; i < N; ++i) {
        float d2 = 0.f;
        for (int d = 0; d < Dp; ++d) {
            const float df = Cs[(long)c * Dp + d] - Xs[(long)i * Dp + d];
            d2 = fmaf(df, df, d2);
        }
        const float k = __builtin_amdgcn_exp2f(fmaf(d2, -0.72134752044448170368f, log2c));
        s = fma((double)k, alpha[i], s);
    }
    mu[c] = s;
}

static int run(int splits, const char *in, const char *out) {
    FILE *f = fopen(in, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", in); return 2; }
    int32_t h[4]; double constant;
    if (fread(h, 4, 4, f) != 4 || fread(&constant, 8, 1, f) != 1) return 2;
    const int N = h[0], M = h[1], Dp = h[2], D = h[3];
    if (N < 1 || N > 65536 || M < 128 || M % 128 || M > 65536 || Dp < 4 || Dp % 4 || Dp > 4096 || D < 1 || D > Dp || splits < 1 ||
        splits > 8) { fprintf(stderr, "bad header\n"); return 2; }
    const int Np = ((N + 255) / 256) * 256;
    std::vector<float> Xs((size_t)Np * Dp, 0.f), Cs((size_t)M * Dp);
    std::vector<double> alpha(Np, 0.0);
    if (fread(Xs.data(), 4, (size_t)N * Dp, f) != (size_t)N * Dp || fread(Cs.data(), 4, Cs.size(), f) != Cs.size() ||
        fread(alpha.data(), 8, N, f) != (size_t)N) return 2;
    fclose(f);
    float *dX, *dC, *dnx; double *dal, *dscal, *dmu, *derr, *dex;
    CK(hipMalloc((void **)&dX, Xs.size() * 4));
    CK(hipMalloc((void **)&dC, Cs.size() * 4));
    CK(hipMalloc((void **)&dnx, (size_t)Np * 4));
    CK(hipMalloc((void **)&dal, (size_t)Np * 8));
    CK(hipMalloc((void **)&dscal, 16));
    CK(hipMalloc((void **)&dmu, (size_t)splits * M * 8));
    CK(hipMalloc((void **)&derr, (size_t)M * 8));
    CK(hipMalloc((void **)&dex, (size_t)M * 8));
    CK(hipMemcpy(dX, Xs.data(), Xs.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, Cs.data(), Cs.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dal, alpha.data(), (size_t)Np * 8, hipMemcpyHostToDevice));
    CK(hipMemset(dmu, 0xff, (size_t)splits * M * 8));
    CK(hipMemset(derr, 0xff, (size_t)M * 8));
    const tgp::ScreenTerms et = tgp::screen_error_terms(constant, D, N);
    hipLaunchKernelGGL(tgp::screen_stats_kernel, dim3(1), dim3(1024), 0, 0, dX, dal, N, Np, Dp, et.P, et.Q, dnx, dscal);
    CK(hipGetLastError());
    tgp::ScreenArgs g{};
    g.Cs = dC; g.Xs = dX; g.alpha = dal; g.nx = dnx; g.scal = dscal; g.mupart = dmu; g.err = derr; g.ldpart = M;
    g.N = N; g.Np = Np; g.Dp = Dp; g.constant = constant;
    hipLaunchKernelGGL(tgp::prune_screen_kernel, dim3(M / 128, splits), dim3(256), 0, 0, g);
    CK(hipGetLastError());
    hipLaunchKernelGGL(exact_mean_kernel, dim3((M + 63) / 64), dim3(64), 0, 0, dC, dX, dal, M, N, Dp, constant, dex);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<double> part((size_t)splits * M), mu(M, 0.0), err(M), ex(M);
    CK(hipMemcpy(part.data(), dmu, part.size() * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(err.data(), derr, (size_t)M * 8, hipMemcpyDeviceToHost));
    CK(hipMemcpy(ex.data(), dex, (size_t)M * 8, hipMemcpyDeviceToHost));
    for (int y = 0; y < splits; ++y)
        for (int c = 0; c < M; ++c) mu[c] += part[(size_t)y * M + c];
    f = fopen(out, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", out); return 2; }
    fwrite(mu.data(), 8, M, f); fwrite(err.data(), 8, M, f); fwrite(ex.data(), 8, M, f);
    fclose(f);
    CK(hipFree(dX)); CK(hipFree(dC)); CK(hipFree(dnx)); CK(hipFree(dal)); CK(hipFree(dscal)); CK(hipFree(dmu)); CK(hipFree(derr));
    CK(hipFree(dex));
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 2) % 2 != 0) { fprintf(stderr, "usage: %s splits in out [in out ...]\n", argv[0]); return 2; }
    const int splits = atoi(argv[1]);
    for (int a = 2; a + 1 < argc; a += 2) {
        const int r = run(splits, argv[a], argv[a + 1]);
        if (r) return r;
    }
    return 0;
}
