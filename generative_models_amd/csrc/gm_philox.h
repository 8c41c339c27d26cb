// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) and the one home of the device noise rule (DESIGN.md
// section 27): the step clock, the uniform / normal mappings and the sample-noise block.  Shared by every kernel that
// draws on the device: gm_bgan.hip, gm_dvae.h, gm_ddpm.h, gm_iwae.hip, gm_flow.hip, gm_iaf.hip, gm_tc.hip, gm_cat.hip, gm_nvp.hip, gm_made.h,
// gm_rbm.h.
//
// A stream is the counter (q, step, row, tag) under key (seed mod 2^32, seed >> 32): q the block of four elements
// 4q .. 4q + 3, step the clock below, row the sample's position, tag the model's constant.  The Bayesian GAN alone keeps
// its older order (q, t, stream, 0).
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

// The step clock: a captured graph reads ctr (advanced on the device) + base, an eager launch passes its step in add.
struct PhClock { const int64_t* ctr; const int64_t* base; int64_t add; };

static __device__ __forceinline__ uint32_t ph_step(const PhClock& k) {
    return (uint32_t)((k.ctr ? *k.ctr : 0) + (k.base ? *k.base : 0) + k.add);
}

// The four words of block (q, step, row, tag) under `seed`, and word j of a block.  Macros, not functions: the compiler
// canonicalises a helper's body before it inlines it, and these two then come out scheduled differently in some of the
// kernels; spelled in the caller's body, every kernel keeps the code it had when each wrote them out.
#define PH_BLOCK(seed, q, step, row, tag) \
    philox10(make_uint4((q), (step), (row), (tag)), (uint32_t)(seed), (uint32_t)((seed) >> 32))
#define PH_WORD(w, j) ((j) == 0u ? (w).x : (j) == 1u ? (w).y : (j) == 2u ? (w).z : (w).w)

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

// Lane i of a float4.
static __device__ __forceinline__ float ph_lane(const float4& v, int i) {
    return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w;
}

// The four normals / the four uniforms of a block's words.
static __device__ __forceinline__ float4 ph_normals_of(const uint4& w) {
    float4 o;
    ph_box_muller(w.x, w.y, o.x, o.y);
    ph_box_muller(w.z, w.w, o.z, o.w);
    return o;
}
static __device__ __forceinline__ float4 ph_units_of(const uint4& w) {
    return make_float4(ph_unit(w.x), ph_unit(w.y), ph_unit(w.z), ph_unit(w.w));
}

// The normals of elements 4q .. 4q + 3 of (step, row, tag).
static __device__ __forceinline__ float4 ph_normals(uint64_t seed, uint32_t q, uint32_t step, uint32_t row,
                                                    uint32_t tag) {
    return ph_normals_of(PH_BLOCK(seed, q, step, row, tag));
}

// The uniform of element e of (step, row, tag): word e & 3 of block e >> 2.
static __device__ __forceinline__ float ph_uniform(uint64_t seed, uint32_t e, uint32_t step, uint32_t row,
                                                   uint32_t tag) {
    const uint4 w = PH_BLOCK(seed, e >> 2, step, row, tag);
    const uint32_t j = e & 3u;
    return ph_unit(PH_WORD(w, j));
}

// The Bayesian GAN's order: the four normals of group q of draw (stream, t).
static __device__ __forceinline__ float4 ph_normal4(uint64_t seed, uint32_t stream, uint32_t t, uint32_t q) {
    return ph_normals(seed, q, t, stream, 0u);
}

// The sample-noise block of the IWAE, the flow VAE and the categorical VAE (the device form of a gm_iwae_noise): k
// samples per image, the noise row of sample j of image b is b kt + j0 + j, counter word 0 is q0 + the call's quad.
struct PhNoise {
    uint64_t seed; uint32_t tag;
    PhClock clk;
    int64_t kt, j0;
    uint32_t q0;
};

static __device__ __forceinline__ uint4 ph_noise_block(const PhNoise& n, uint32_t step, uint32_t row, uint32_t q) {
    return PH_BLOCK(n.seed, n.q0 + q, step, row, n.tag);
}

// The normals of latents 4q .. 4q + 3 of noise row `row`.
static __device__ __forceinline__ void ph_noise_eps4(const PhNoise& n, uint32_t step, uint32_t row, uint32_t q,
                                                     float (&e)[4]) {
    const float4 v = ph_normals_of(ph_noise_block(n, step, row, q));
    e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
}

// Host: the device form of a gm_iwae_noise for B images of k samples (the caller has checked B and k against its own
// limits), or GM_EINVAL.
static inline int ph_noise_fill(const gm_iwae_noise* a, int B, int k, PhNoise* n) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->j0 >= 0 && a->k_total >= a->j0 + k && a->q0 >= 0 && a->q0 < (1ll << 31));
    GM_CHECK_ARG(a->k_total < (1ll << 32) / B);              // the noise row is a 32-bit counter word
    n->seed = a->seed; n->tag = a->tag;
    n->clk = PhClock{a->step_ctr, a->step_base, a->step_add};
    n->kt = a->k_total; n->j0 = a->j0; n->q0 = (uint32_t)a->q0;
    return 0;
}
