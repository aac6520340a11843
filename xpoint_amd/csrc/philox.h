// The counter-based generator of the augmentation noise (augment.hip) and of the training dropout (train_regnet.hip), written once: a draw is a pure
// function of (seed, sample id, stream, counter), so a sample's random numbers never depend on its batch neighbours or on the launch geometry.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

// Philox4x32-10 (Salmon et al., SC'11).  counter = (pixel index, 0, 0, seed >> 32), key = (seed & 0xffffffff, sample id * 8 + primitive).
struct AugU4 { uint32_t x, y, z, w; };
__device__ __forceinline__ AugU4 aug_philox(uint64_t seed, uint32_t sample, uint32_t primitive, uint32_t pixel) {
    uint32_t c0 = pixel, c1 = 0u, c2 = 0u, c3 = (uint32_t)(seed >> 32);
    uint32_t k0 = (uint32_t)seed, k1 = sample * 8u + primitive;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return AugU4{c0, c1, c2, c3};
}
__device__ __forceinline__ float aug_uniform(uint32_t v) { return (float)(v >> 8) * 5.9604644775390625e-08f; }      // (x >> 8) * 2^-24, exact
