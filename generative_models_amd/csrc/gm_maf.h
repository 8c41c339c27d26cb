// The masked autoregressive flow's arithmetic (maf.py holds the contract; gm_hip.h), shared by every
// kernel of gm_maf.hip so that the forward, the backward and the one-launch inverse form s, u and y with the same bits.
//
// One layer maps y to u = (y - m) exp(-s) with s = s_cap tanh(a) (nvp_s of gm_nvp.h: the one place that forms it), [m | a]
// the masked MLP's output; the inverse is y = u exp(s) + m, the product rounded before the add.
#pragma once
#include "gm_nvp.h"

// u = (y - m) exp(-s).
static __device__ __forceinline__ float maf_fwd(float y, float s, float m) { return nvp_inv(y, s, m); }

// y = u exp(s) + m, the product rounded before the add.
static __device__ __forceinline__ float maf_inv(float u, float s, float m) { return nvp_fwd(u, s, m); }

// One element of the layer's backward.  g = dL/du, c the log-determinant's cotangent (logdet -= s):
//   dm = -g exp(-s),  da = (-(g u) - c) s_cap (1 - tanh^2(a)),  dy = g exp(-s).
static __device__ __forceinline__ void maf_bwd_elem(float a, float u, float g, float c, float cap, float& dm, float& da,
                                                    float& dy) {
#pragma clang fp contract(off)
    const NvpS s = nvp_s(a, cap);
    const float ge = g * expf(-s.s);
    dy = ge;
    dm = -ge;
    // 1 - tanh^2(a) as 4 e / (1 + e)^2, e = exp(-2 |a|): nothing cancels where the tanh saturates
    const float e = expf(-2.f * fabsf(a)), ope = 1.f + e;
    da = ((-(g * u) - c) * cap) * ((4.f * e) / (ope * ope));
}
