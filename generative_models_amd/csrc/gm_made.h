// The masked autoregressive model's sampling rule (made.py; gm_hip.h), shared by gm_made_sample and gm_made_uniform.
//
// The uniform of pixel d of sample row r: ph_unit of word d & 3 of Philox4x32-10 at counter (d >> 2, 0, r, GM_MADE_TAG_S)
// under key (seed mod 2^32, seed >> 32).  The pixel is lit iff u < 1 / (1 + expf(-a)), compared in fp32.  Both are
// indexed by (row, pixel) alone: no work mapping can change a bit.
#pragma once
#include "gm_philox.h"

static __device__ __forceinline__ float made_unit(uint64_t seed, uint32_t d, uint32_t r) {
    const uint4 w = philox10(make_uint4(d >> 2, 0u, r, GM_MADE_TAG_S), (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t j = d & 3u;
    return ph_unit(j == 0u ? w.x : j == 1u ? w.y : j == 2u ? w.z : w.w);
}

// The conditional of a logit; pinned so that every kernel that decides a pixel rounds alike.
static __device__ __forceinline__ float made_prob(float a) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-a));
}
