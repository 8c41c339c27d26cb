// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) and the uniform / normal mappings built on it, shared
// by the Bayesian GAN's generator (gm_bgan.hip) and the denoising VAE's input corruption (gm_dvae.h).
//
// Each output word x becomes u = (2 (x >> 9) + 1) 2^-24, exact in fp32 and strictly inside (0, 1); Box-Muller turns
// words (0, 1) and (2, 3) into (r cos, r sin) with r = sqrt(-2 ln u_a), phi = 2 pi u_b.  sincospif(2 u_b) takes its
// argument in half-turns, so no range reduction is needed and the result stays within a couple of ulp of the fp64 value.
#pragma once
#include "gm_common.h"

static constexpr uint32_t PH_M0 = 0xD2511F53u, PH_M1 = 0xCD9E8D57u;
static constexpr uint32_t PH_W0 = 0x9E3779B9u, PH_W1 = 0xBB67AE85u;

static __device__ __forceinline__ uint4 philox10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = PH_M0 * c.x, hi0 = __umulhi(PH_M0, c.x);
        const uint32_t lo1 = PH_M1 * c.z, hi1 = __umulhi(PH_M1, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += PH_W0;
        k1 += PH_W1;
    }
    return c;
}

static __device__ __forceinline__ float ph_unit(uint32_t x) {
    return (float)(2u * (x >> 9) + 1u) * 5.9604644775390625e-08f;     // 2^-24
}

static __device__ __forceinline__ void ph_box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
    const float r = sqrtf(-2.f * logf(ph_unit(a)));
    float s, c;
    sincospif(2.f * ph_unit(b), &s, &c);
    n0 = r * c;
    n1 = r * s;
}

// The four normals of group q (elements 4q .. 4q + 3) of draw (stream, t).
static __device__ __forceinline__ float4 ph_normal4(uint64_t seed, uint32_t stream, uint32_t t, uint32_t q) {
    const uint4 x = philox10(make_uint4(q, t, stream, 0u), (uint32_t)seed, (uint32_t)(seed >> 32));
    float4 o;
    ph_box_muller(x.x, x.y, o.x, o.y);
    ph_box_muller(x.z, x.w, o.z, o.w);
    return o;
}
