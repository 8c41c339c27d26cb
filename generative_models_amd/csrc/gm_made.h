// The masked autoregressive model's sampling rule (made.py; gm_hip.h), shared by gm_made_sample and gm_made_uniform.
//
// The uniform of pixel d of sample row r: ph_uniform(seed, d, 0, r, GM_MADE_TAG_S) (gm_philox.h), word d & 3 of the block
// at counter (d >> 2, 0, r, GM_MADE_TAG_S).  The pixel is lit iff u < 1 / (1 + expf(-a)), compared in fp32.  Both are
// indexed by (row, pixel) alone: no work mapping can change a bit.
#pragma once
#include "gm_philox.h"

// The conditional of a logit; pinned so that every kernel that decides a pixel rounds alike.
static __device__ __forceinline__ float made_prob(float a) {
#pragma clang fp contract(off)
    return 1.0f / (1.0f + expf(-a));
}
