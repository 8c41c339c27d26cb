// The restricted Boltzmann machine's noise rule and pinned arithmetic (rbm.py; gm_hip.h), shared by every kernel of
// gm_rbm.hip.
//
// The uniform of unit e of chain row r at step t under tag T: ph_uniform(seed, e, t, r, T) (gm_philox.h), word e & 3 of
// the block at counter (e >> 2, t, r, T).  T = GM_RBM_TAG_D: the binarisation of the input rows (t = the
// batch step);  GM_RBM_TAG_H / GM_RBM_TAG_V: the hidden / visible draws (t = the Gibbs step).  A unit is lit iff
// u < made_prob(a), compared in fp32 (gm_made.h's pinned sigmoid).  Indexed by (seed, t, r, e) alone: no work mapping can
// change a bit.
#pragma once
#include "gm_made.h"

// softplus, pinned: max(a, 0) + log1pf(expf(-|a|)).
static __device__ __forceinline__ float rbm_sp(float a) {
#pragma clang fp contract(off)
    return fmaxf(a, 0.f) + log1pf(expf(-fabsf(a)));
}

// The tempered visible logit beta pre_v + (1 - beta) b_A: two rounded products and an add.
static __device__ __forceinline__ float rbm_temper_v(float beta, float pre, float bA) {
#pragma clang fp contract(off)
    const float x = beta * pre;
    const float om = 1.f - beta;
    const float y = om * bA;
    return x + y;
}

// One lane's share of a tempered step's log-weight increment: dbeta * bv + sps, the product rounded before the add.
static __device__ __forceinline__ float rbm_logw_lane(float dbeta, float bv, float sps) {
#pragma clang fp contract(off)
    const float x = dbeta * bv;
    return x + sps;
}

// sp(bc pre) - sp(bp pre), every operation rounded.
static __device__ __forceinline__ float rbm_sp_diff(float bc, float bp, float pre) {
#pragma clang fp contract(off)
    const float x = bc * pre;
    const float y = bp * pre;
    return rbm_sp(x) - rbm_sp(y);
}
