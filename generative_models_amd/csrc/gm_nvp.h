// The RealNVP coupling flow's arithmetic (realnvp.py holds the contract; gm_hip.h), shared by every kernel of gm_nvp.hip
// so that the forward, the backward and the inverse form s, the split and the noise with the same bits.
//
// Split: pixel e of an image of D pixels is an entry of half A or of half B (Da = ceil(D / 2)): GM_NVP_CHECKER A = the
// even pixels, GM_NVP_HALF A = the first Da.  Noise: the uniform of pixel e is ph_unit of word e & 3 of the row's Philox
// block e >> 2; the sampler's normal of pixel e is the Box-Muller value of that word under ph_normals' pairing.  Both are
// indexed by (row, pixel) alone: no work mapping can change a bit.
#pragma once
#include "gm_philox.h"

struct NvpS { float th, s; };

// s = s_cap tanh(a): the ONE place that forms it.
static __device__ __forceinline__ NvpS nvp_s(float a, float cap) {
#pragma clang fp contract(off)
    NvpS r;
    r.th = tanhf(a);
    r.s = cap * r.th;
    return r;
}

// y = x exp(s) + t, the product rounded before the add.
static __device__ __forceinline__ float nvp_fwd(float x, float s, float t) {
#pragma clang fp contract(off)
    const float p = x * expf(s);
    return p + t;
}

// x = (y - t) exp(-s).
static __device__ __forceinline__ float nvp_inv(float y, float s, float t) {
#pragma clang fp contract(off)
    const float d = y - t;
    return d * expf(-s);
}

struct NvpPre { float alpha, om2a, log_om2a, lv; };

// Dequantise + logit of one pixel: y and the element's log-determinant.  vc = 1 - v is formed from 1 - u (exact in fp32)
// and levels - 1 - q, not by subtraction: both logs stay finite at alpha = 0 for every word.
static __device__ __forceinline__ float nvp_pre_elem(float x, float u, const NvpPre& p, float& y) {
#pragma clang fp contract(off)
    const float top = p.lv - 1.f;
    const float q = fminf(fmaxf(floorf(x * top + 0.5f), 0.f), top);
    const float v = (q + u) / p.lv;
    const float vc = ((top - q) + (1.f - u)) / p.lv;
    const float w = p.alpha + p.om2a * v;
    const float wc = p.alpha + p.om2a * vc;
    const float lw = logf(w), lwc = logf(wc);
    y = lw - lwc;
    return (p.log_om2a - lw) - lwc;
}

// x = clamp((sigmoid(y) - alpha) / (1 - 2 alpha), 0, 1).
static __device__ __forceinline__ float nvp_post_elem(float y, float alpha, float om2a) {
#pragma clang fp contract(off)
    const float sg = 1.0f / (1.0f + expf(-y));
    return fminf(fmaxf((sg - alpha) / om2a, 0.f), 1.f);
}

static __device__ __forceinline__ float nvp_get(const float4& v, int j) {
    return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w;
}
static __device__ __forceinline__ void nvp_set(float4& v, int j, float f) {
    if (j == 0) v.x = f; else if (j == 1) v.y = f; else if (j == 2) v.z = f; else v.w = f;
}

// Quad q (elements 4q .. 4q + 3) of a row of n floats: one 16-byte access when vec, element by element (zeros past the
// end, nothing stored there) otherwise.
static __device__ __forceinline__ float4 nvp_load4(const float* row, int q, int n, int vec) {
    if (vec) return reinterpret_cast<const float4*>(row)[q];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * q + j < n) nvp_set(v, j, row[4 * q + j]);
    return v;
}
static __device__ __forceinline__ void nvp_store4(float* row, int q, int n, int vec, const float4& v) {
    if (vec) { reinterpret_cast<float4*>(row)[q] = v; return; }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * q + j < n) row[4 * q + j] = nvp_get(v, j);
}

// Quad q of the unsplit image <-> the two halves.  vec (the host grants it): CHECKER needs D % 4 == 0 and 8-byte aligned
// halves (a quad is one float2 of each half); HALF needs Da % 4 == 0 too and 16-byte aligned halves (a quad lies in one).
static __device__ __forceinline__ float4 nvp_split_load(const float* a, const float* b, int q, int D, int Da, int mask,
                                                        int vec) {
    if (vec && mask == GM_NVP_CHECKER) {
        const float2 va = reinterpret_cast<const float2*>(a)[q], vb = reinterpret_cast<const float2*>(b)[q];
        return make_float4(va.x, vb.x, va.y, vb.y);
    }
    if (vec) return 4 * q < Da ? reinterpret_cast<const float4*>(a)[q] : reinterpret_cast<const float4*>(b)[q - (Da >> 2)];
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = 4 * q + j;
        if (e >= D) continue;
        const bool inb = mask == GM_NVP_CHECKER ? (e & 1) : (e >= Da);
        const int i = mask == GM_NVP_CHECKER ? (e >> 1) : (inb ? e - Da : e);
        nvp_set(v, j, inb ? b[i] : a[i]);
    }
    return v;
}
static __device__ __forceinline__ void nvp_split_store(float* a, float* b, int q, int D, int Da, int mask, int vec,
                                                       const float4& v) {
    if (vec && mask == GM_NVP_CHECKER) {
        reinterpret_cast<float2*>(a)[q] = make_float2(v.x, v.z);
        reinterpret_cast<float2*>(b)[q] = make_float2(v.y, v.w);
        return;
    }
    if (vec) {
        if (4 * q < Da) reinterpret_cast<float4*>(a)[q] = v;
        else reinterpret_cast<float4*>(b)[q - (Da >> 2)] = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = 4 * q + j;
        if (e >= D) continue;
        const bool inb = mask == GM_NVP_CHECKER ? (e & 1) : (e >= Da);
        const int i = mask == GM_NVP_CHECKER ? (e >> 1) : (inb ? e - Da : e);
        (inb ? b : a)[i] = nvp_get(v, j);
    }
}

// A row's sum from its 256 threads' partials: the wave butterfly, then the four waves in order; valid in thread 0.
static __device__ __forceinline__ float nvp_row_sum(float acc, float* sh) {
    acc = gm_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}
