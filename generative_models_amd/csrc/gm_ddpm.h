// Denoising diffusion (ddpm.py holds the contract): the one definition of the noise rule, the
// forward (q-sample) step and the reverse (sampler) step, shared by every kernel of gm_ddpm.hip.
//
// The rule.  Philox4x32-10 with key (seed mod 2^32, seed >> 32):
//   timestep of batch row `row` at batch `step`: word 0 of counter (0, step, row, tag_t), t = mulhi(word, T);
//   noise of pixels 4q .. 4q + 3 of that row: ph_normals at counter (q, step, row, tag_e);
//   x0 = fmaf(2, x, -1);   x_t = fmaf(s1[t], n, sa[t] * x0)   (the product rounded, then one fused multiply-add);
//   sampler: z of pixels 4q .. 4q + 3 of sample row `row` at sampler step s: counter (q, s, row, GM_DDPM_TAG_S).
// One 256-thread workgroup per row, thread i the quads i, i + 256, ...: a 784-pixel row is one quad per thread on 196
// threads (the DVAE's one-wave-per-row gaussian gather, 196 Philox and Box-Muller calls over 64 lanes, was ALU-bound).
#pragma once
#include "gm_gather.h"
#include "gm_philox.h"

struct DdpmNoiseP {
    uint64_t seed; uint32_t tag_t, tag_e;
    PhClock clk;
    int64_t row0;                                            // batch position of the first row
};
struct DdpmTabP { const float* sa; const float* s1; const float* temb; int T, E; };
struct DdpmOutP { float* xin; int64_t ldin; float* eps; int64_t lde; int32_t* t; int vec_tail; };

static __device__ __forceinline__ uint32_t ddpm_timestep(const DdpmNoiseP& n, uint32_t step, uint32_t row, uint32_t T) {
    return __umulhi(PH_BLOCK(n.seed, 0u, step, row, n.tag_t).x, T);
}

// x_t of one pixel: the image pixel x in [0, 1], its normal n.
static __device__ __forceinline__ float ddpm_noised(float sa, float s1, float x, float n) {
#pragma clang fp contract(off)
    const float x0 = __builtin_fmaf(2.f, x, -1.f);
    const float p = sa * x0;
    return __builtin_fmaf(s1, n, p);
}

// One sampler step of one pixel (Song et al., arXiv 2010.02502 eq. 12): every rounding pinned.
static __device__ __forceinline__ float ddpm_reverse1(float xt, float e, float z, float s1, float sa, float sap,
                                                      float dir, float sig, int clip) {
#pragma clang fp contract(off)
    float x0 = __builtin_fmaf(-s1, e, xt) / sa;
    if (clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    const float ep = __builtin_fmaf(-sa, x0, xt) / s1;
    float m = sap * x0;
    m = __builtin_fmaf(dir, ep, m);
    return __builtin_fmaf(sig, z, m);
}

// Where a row's clean pixels come from: fp32 (src) or one bit per pixel (w).
struct DdpmRow {
    const float* src; const uint32_t* w;
    __device__ __forceinline__ float4 quad(int q) const {
        return w ? gather_bits4(w, q) : reinterpret_cast<const float4*>(src)[q];
    }
    __device__ __forceinline__ float elem(int i) const {
        return w ? gather_bit(w, i) : src[i];
    }
};

// temb[t] into the tail of a network-input row (xin + I).
static __device__ __forceinline__ void ddpm_tail(float* tail, const float* te, int E, int vec_tail) {
    if (vec_tail) {
        for (int j = threadIdx.x; j < (E >> 2); j += blockDim.x)
            reinterpret_cast<float4*>(tail)[j] = reinterpret_cast<const float4*>(te)[j];
    } else {
        for (int j = threadIdx.x; j < E; j += blockDim.x) tail[j] = te[j];
    }
}

// Batch row b (this workgroup's): t, [x_t | temb[t]] -> o.xin, the noise -> o.eps, the clean pixels -> clean (or null).
static __device__ __forceinline__ void ddpm_qsample_row(const DdpmNoiseP& n, const DdpmTabP& s, const DdpmOutP& o,
                                                        int64_t b, int I, int vec, float* clean, const DdpmRow& rs) {
    const uint32_t step = ph_step(n.clk), row = (uint32_t)(n.row0 + b);
    uint32_t t = 0;
    if ((threadIdx.x & 63) == 0) t = ddpm_timestep(n, step, row, (uint32_t)s.T);
    t = (uint32_t)__shfl((int)t, 0, 64);
    const float sa = s.sa[t], s1 = s.s1[t];
    float* xin = o.xin + b * o.ldin;
    float* ep = o.eps + b * o.lde;
    if (vec) {                             // I % 4 == 0, every row 16-byte aligned
        for (int q = threadIdx.x; q < (I >> 2); q += blockDim.x) {
            const float4 v = rs.quad(q);
            const float4 z = ph_normals(n.seed, (uint32_t)q, step, row, n.tag_e);
            if (clean) reinterpret_cast<float4*>(clean)[q] = v;
            reinterpret_cast<float4*>(xin)[q] = make_float4(ddpm_noised(sa, s1, v.x, z.x), ddpm_noised(sa, s1, v.y, z.y),
                                                            ddpm_noised(sa, s1, v.z, z.z), ddpm_noised(sa, s1, v.w, z.w));
            reinterpret_cast<float4*>(ep)[q] = z;
        }
    } else {
        for (int q = threadIdx.x; 4 * q < I; q += blockDim.x) {
            const float4 z = ph_normals(n.seed, (uint32_t)q, step, row, n.tag_e);
            const int cnt = min(4, I - 4 * q);
            for (int j = 0; j < cnt; ++j) {
                const int i = 4 * q + j;
                const float x = rs.elem(i), zj = ph_lane(z, j);
                if (clean) clean[i] = x;
                xin[i] = ddpm_noised(sa, s1, x, zj);
                ep[i] = zj;
            }
        }
    }
    ddpm_tail(xin + I, s.temb + (int64_t)t * s.E, s.E, o.vec_tail);
    if (threadIdx.x == 0 && o.t) o.t[b] = (int32_t)t;
}
