// The pruned sweep's fp16 screen (turbo_amd/csrc/prune_screen_h2.hpp) candidate by candidate: prep + screen run TWICE
// (the second run's bytes must be the first's), the error as prune_bound_kernel forms it, and the exact path's mean.
// Built and run by tests/test_gpu_prune_screen_h2.py:   prune_screen_h2_driver <splits> <in> <out> [<in> <out> ...]
//   in : int32 N, M, Dp, D; double constant; float Xs[N][Dp]; float Cs[M][Dp]; double alpha[N]   (M a multiple of 128)
//   out: double run1[4][M], run2[4][M] (mu_s, W, E, closed form); double mu_exact[M]
// The exact path is restated as in prune_screen_driver.hip: the direct difference summed in dimension order with fmaf, the
// same exp2 sequence, an f64 fma per training point.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../turbo_amd/csrc/prune_screen_h2.hpp"

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
    std::vector<float> Xs((size_t)N * Dp), Cs((size_t)M * Dp);
    std::vector<double> alpha(N);
    if (fread(Xs.data(), 4, Xs.size(), f) != Xs.size() || fread(Cs.data(), 4, Cs.size(), f) != Cs.size() ||
        fread(alpha.data(), 8, N, f) != (size_t)N) return 2;
    fclose(f);
    const long ncap = (long)((N + 127) / 128 + 1) * 128;
    const int nch = (Dp + tgp::SCR_DC - 1) / tgp::SCR_DC;
    const size_t xh_bytes = (size_t)nch * ncap * 128;
    float *dX, *dC, *dnxp, *dabsa; double *dal, *dmu, *dw, *derr, *dwc, *dex; unsigned char *dxh; tgp::ScreenH2Scal *dscal;
    CK(hipMalloc((void **)&dX, Xs.size() * 4));
    CK(hipMalloc((void **)&dC, Cs.size() * 4));
    CK(hipMalloc((void **)&dxh, xh_bytes));
    CK(hipMalloc((void **)&dnxp, (size_t)ncap * 4));
    CK(hipMalloc((void **)&dabsa, (size_t)ncap * 4));
    CK(hipMalloc((void **)&dal, (size_t)N * 8));
    CK(hipMalloc((void **)&dscal, sizeof(tgp::ScreenH2Scal)));
    CK(hipMalloc((void **)&dmu, (size_t)splits * M * 8));
    CK(hipMalloc((void **)&dw, (size_t)splits * M * 8));
    CK(hipMalloc((void **)&derr, (size_t)M * 8));
    CK(hipMalloc((void **)&dwc, (size_t)M * 8));
    CK(hipMalloc((void **)&dex, (size_t)M * 8));
    CK(hipMemcpy(dX, Xs.data(), Xs.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dC, Cs.data(), Cs.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dal, alpha.data(), (size_t)N * 8, hipMemcpyHostToDevice));
    const tgp::ScreenH2Terms et = tgp::screen_h2_error_terms(constant, D, N);
    std::vector<double> res((size_t)9 * M);
    for (int rep = 0; rep < 2; ++rep) {
        // every output poisoned (all-ones bytes are NaNs in fp16, f32 and f64): a row the prep left out shows
        CK(hipMemset(dxh, 0xff, xh_bytes));
        CK(hipMemset(dnxp, 0xff, (size_t)ncap * 4));
        CK(hipMemset(dabsa, 0xff, (size_t)ncap * 4));
        CK(hipMemset(dscal, 0xff, sizeof(tgp::ScreenH2Scal)));
        CK(hipMemset(dmu, 0xff, (size_t)splits * M * 8));
        CK(hipMemset(dw, 0xff, (size_t)splits * M * 8));
        CK(hipMemset(derr, 0xff, (size_t)M * 8));
        CK(hipMemset(dwc, 0xff, (size_t)M * 8));
        tgp::ScreenH2PrepArgs a{};
        a.Xs = dX; a.alpha = dal; a.N = N; a.Dp = Dp; a.nch = nch; a.ncap = ncap; a.P = et.P; a.Qc = et.Qc; a.Qw = et.Qw;
        a.Xh = dxh; a.nxp = dnxp; a.absa = dabsa; a.scal = dscal;
        hipLaunchKernelGGL(tgp::screen_h2_prep_kernel, dim3((N + 255) / 256), dim3(256), 0, 0, a);
        CK(hipGetLastError());
        tgp::ScreenH2Args g{};
        g.Cs = dC; g.Xh = dxh; g.nxp = dnxp; g.absa = dabsa; g.scal = dscal; g.mupart = dmu; g.wpart = dw; g.err = derr; g.wcoef = dwc;
        g.ldpart = M; g.ncap = ncap; g.Dp = Dp; g.constant = constant; g.dcoef = et.dcoef;
        hipLaunchKernelGGL(tgp::prune_screen_h2_kernel, dim3(M / 128, splits), dim3(256), 0, 0, g);
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        std::vector<double> pm((size_t)splits * M), pw((size_t)splits * M), err(M), wc(M);
        tgp::ScreenH2Scal sc;
        CK(hipMemcpy(pm.data(), dmu, pm.size() * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(pw.data(), dw, pw.size() * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(err.data(), derr, (size_t)M * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(wc.data(), dwc, (size_t)M * 8, hipMemcpyDeviceToHost));
        CK(hipMemcpy(&sc, dscal, sizeof sc, hipMemcpyDeviceToHost));
        double *o = res.data() + (size_t)rep * 4 * M;
        for (int c = 0; c < M; ++c) {
            double mu = 0.0, w = 0.0;      // (prune_bound_kernel's order: split after split)
            for (int y = 0; y < splits; ++y) { mu += pm[(size_t)y * M + c]; w += pw[(size_t)y * M + c]; }
            o[c] = mu; o[M + c] = w; o[2 * M + c] = tgp::screen_h2_error(err[c], wc[c], w, sc.wadd); o[3 * M + c] = err[c];
        }
    }
    hipLaunchKernelGGL(exact_mean_kernel, dim3((M + 63) / 64), dim3(64), 0, 0, dC, dX, dal, M, N, Dp, constant, dex);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(res.data() + (size_t)8 * M, dex, (size_t)M * 8, hipMemcpyDeviceToHost));
    f = fopen(out, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", out); return 2; }
    fwrite(res.data(), 8, res.size(), f);
    fclose(f);
    CK(hipFree(dX)); CK(hipFree(dC)); CK(hipFree(dxh)); CK(hipFree(dnxp)); CK(hipFree(dabsa)); CK(hipFree(dal)); CK(hipFree(dscal));
    CK(hipFree(dmu)); CK(hipFree(dw)); CK(hipFree(derr)); CK(hipFree(dwc)); CK(hipFree(dex));
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
