// The narrow contraction of a gathered candidate set (trmm_sumsq_glds_narrow_kernel, 128 rows x 32 / 64 candidates)
// against the 128 x 128 kernel on the same operands: `part` and the mean compared byte for byte.
// Built and run by tests/test_gpu_prune_tail.py:   prune_tail_driver f32|f64 N rows [N rows ...]
// One line per case: "<dtype> N=<N> rows=<rows> bn=<32|64> part_diff=<count> mu_diff=<count>"; exit status 1 on any difference.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../turbo_amd/csrc/trmm_sweep.hpp"

#define CK(x)                                                                       \
    do {                                                                            \
        hipError_t e_ = (x);                                                        \
        if (e_ != hipSuccess) {                                                     \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
            exit(2);                                                                \
        }                                                                           \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uni() {   // xorshift64*, (0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0);
}

template <typename T>
static int run_case(const char *name, int N, int rows) {
    const int Np = ((N + 255) / 256) * 256, n128 = (N + 127) / 128, K = n128 * 128;
    const int rpad = ((rows + 127) / 128) * 128;
    // Linv: lower triangle of the real rows, exact zeros elsewhere; the slab: real rows x real columns, zero padding
    std::vector<T> A((size_t)Np * Np, (T)0), B((size_t)rpad * Np, (T)0);
    std::vector<double> alpha(Np, 0.0);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j <= i; ++j) A[(size_t)i * Np + j] = (T)((uni() - 0.5) * (i == j ? 4.0 : 0.25));
    for (int r = 0; r < rows; ++r)
        for (int j = 0; j < N; ++j) B[(size_t)r * Np + j] = (T)uni();
    for (int j = 0; j < N; ++j) alpha[j] = (uni() - 0.5) * 100.0;
    T *dA, *dB; double *dal, *dpart[3], *dmu[3];
    CK(hipMalloc((void **)&dA, A.size() * sizeof(T)));
    CK(hipMalloc((void **)&dB, B.size() * sizeof(T)));
    CK(hipMalloc((void **)&dal, Np * sizeof(double)));
    CK(hipMemcpy(dA, A.data(), A.size() * sizeof(T), hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), B.size() * sizeof(T), hipMemcpyHostToDevice));
    CK(hipMemcpy(dal, alpha.data(), Np * sizeof(double), hipMemcpyHostToDevice));
    const size_t pbytes = (size_t)n128 * rpad * sizeof(double), mbytes = (size_t)rpad * sizeof(double);
    for (int v = 0; v < 3; ++v) {
        CK(hipMalloc((void **)&dpart[v], pbytes));
        CK(hipMalloc((void **)&dmu[v], mbytes));
        CK(hipMemset(dpart[v], 0xff, pbytes));
        CK(hipMemset(dmu[v], 0xff, mbytes));
    }
    void (*kern[3])(tgp::GemmArgs) = {tgp::trmm_sumsq_glds_kernel<T>, tgp::trmm_sumsq_glds_narrow_kernel<T, 32>,
                                      tgp::trmm_sumsq_glds_narrow_kernel<T, 64>};
    const size_t lds[3] = {tgp::trmm_glds_lds_bytes(), tgp::trmm_narrow_lds_bytes<32>(), tgp::trmm_narrow_lds_bytes<64>()};
    const int bn[3] = {128, 32, 64};
    for (int v = 0; v < 3; ++v) {
        tgp::GemmArgs g{};
        g.A = dA; g.lda = Np; g.B = dB; g.ldb = Np;
        g.part = dpart[v]; g.ldpart = rpad; g.prm = 1;
        g.tm0 = 0; g.ntm = n128; g.ntn = rpad / bn[v]; g.ntn_group = 0;
        g.K = K; g.mu_alpha = dal; g.mu = dmu[v];
        CK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern[v]), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds[v]));
        hipLaunchKernelGGL(kern[v], dim3((unsigned)(g.ntm * g.ntn)), dim3(256), lds[v], 0, g);
        CK(hipGetLastError());
    }
    CK(hipDeviceSynchronize());
    std::vector<double> part[3], mu[3];
    for (int v = 0; v < 3; ++v) {
        part[v].resize((size_t)n128 * rpad); mu[v].resize(rpad);
        CK(hipMemcpy(part[v].data(), dpart[v], pbytes, hipMemcpyDeviceToHost));
        CK(hipMemcpy(mu[v].data(), dmu[v], mbytes, hipMemcpyDeviceToHost));
    }
    int bad = 0;
    // (a reference that is all zeros or still the 0xff fill would compare equal to anything equally broken: count it)
    double ref_sum = 0.0;
    for (int r = 0; r < rows; ++r) ref_sum += part[0][r] + (mu[0][r] != 0.0 ? 1.0 : 0.0);
    const bool ref_ok = ref_sum == ref_sum && ref_sum > 0.0;
    for (int v = 1; v < 3; ++v) {
        long pd = 0, md = 0;
        for (size_t i = 0; i < part[0].size(); ++i) pd += memcmp(&part[0][i], &part[v][i], 8) != 0;
        for (int i = 0; i < rpad; ++i) md += memcmp(&mu[0][i], &mu[v][i], 8) != 0;
        printf("%s N=%d rows=%d bn=%d part_diff=%ld mu_diff=%ld ref_ok=%d\n", name, N, rows, bn[v], pd, md, (int)ref_ok);
        bad += (pd != 0) + (md != 0) + !ref_ok;
    }
    for (int v = 0; v < 3; ++v) { CK(hipFree(dpart[v])); CK(hipFree(dmu[v])); }
    CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dal));
    return bad;
}

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 2) % 2 != 0) { fprintf(stderr, "usage: %s f32|f64 N rows [N rows ...]\n", argv[0]); return 2; }
    const bool f64 = strcmp(argv[1], "f64") == 0;
    int bad = 0;
    for (int a = 2; a + 1 < argc; a += 2) {
        const int N = atoi(argv[a]), rows = atoi(argv[a + 1]);
        if (N < 1 || N > 16384 || rows < 1 || rows > 65536) { fprintf(stderr, "bad case %d %d\n", N, rows); return 2; }
        bad += f64 ? run_case<double>("f64", N, rows) : run_case<float>("f32", N, rows);
    }
    return bad ? 1 : 0;
}
