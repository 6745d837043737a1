// philox.hpp -- Philox-4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), shared by
// the candidate generators (sweep_kernels.hip), the Thompson-sampling draw (ts_kernels.hip) and the Monte Carlo batch
// strategy's fantasies (batch_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tgp {

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        const uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// a 53-bit uniform in [0, 1) from two words: ((a >> 5) 2^26 + (b >> 6)) / 2^53
__device__ __forceinline__ double philox_u53(uint32_t a, uint32_t b) {
    return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}
// element e of stream `stream` under `tag`: counter (e lo, e hi, stream, tag), key = the 64-bit seed
__device__ __forceinline__ void philox_words(unsigned long long e, uint32_t stream, uint32_t tag, unsigned long long seed,
                                             uint32_t r[4]) {
    philox4x32_10((uint32_t)e, (uint32_t)(e >> 32), stream, tag, (uint32_t)seed, (uint32_t)(seed >> 32), r);
}
// a standard normal per element: ONE Box-Muller branch sqrt(-2 log(1 - u1)) cos(2 pi u2), u1 from words (0, 1), u2 from (2, 3)
__device__ __forceinline__ double philox_normal(unsigned long long e, uint32_t stream, uint32_t tag, unsigned long long seed) {
    uint32_t r[4];
    philox_words(e, stream, tag, seed, r);
    const double u1 = philox_u53(r[0], r[1]), u2 = philox_u53(r[2], r[3]);
    const double t = -2.0 * log(1.0 - u1);
    const double a = 6.283185307179586 * u2;
    return sqrt(t) * cos(a);
}

}  // namespace tgp
