// fd_keyed_noise.h -- the counter-based normal stream keyed per slice (fd_sched.hip's step noise, fd_train_step.hip's q_sample
// noise): Philox4x32-10 keyed by the slice's 64-bit seed, counter = (pixel / 4, t, domain tag, 0), Box-Muller on the four 32-bit
// outputs.  oracle/keyed_noise.py restates it in numpy.  Anonymous namespace: each file that includes this header gets its own copy.
#pragma once
#include "fd_common.h"

namespace {

struct u32q { uint32_t x, y, z, w; };

__device__ __forceinline__ u32q philox4x32_10(u32q c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = u32q{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// four standard normals of (seed, t, group g of four consecutive pixels)
__device__ __forceinline__ void keyed_normal4(uint64_t seed, uint32_t t, uint32_t g, float z[4]) {
    const u32q r = philox4x32_10(u32q{g, t, 0x46444e5au, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    // 23-bit uniforms (k + 0.5) * 2^-23, k < 2^23: k + 0.5 has 24 significant bits, so every value is exactly
    // representable, strictly inside (0, 1) and the grid is uniform over the whole range
    const float u0 = ((float)(r.x >> 9) + 0.5f) * (1.f / 8388608.f), u1 = ((float)(r.y >> 9) + 0.5f) * (1.f / 8388608.f);
    const float u2 = ((float)(r.z >> 9) + 0.5f) * (1.f / 8388608.f), u3 = ((float)(r.w >> 9) + 0.5f) * (1.f / 8388608.f);
    const float ra = sqrtf(-2.f * logf(u0)), rb = sqrtf(-2.f * logf(u2));
    float s0, c0, s1, c1;
    sincospif(2.f * u1, &s0, &c0);
    sincospif(2.f * u3, &s1, &c1);
    z[0] = ra * c0; z[1] = ra * s0; z[2] = rb * c1; z[3] = rb * s1;
}

}  // namespace
