// Denoising VAE (dvae.py): the input corruption x~ ~ p(x~ | x) on the device, and the batch gather
// that writes the clean rows (as gm_gather_rows does) and their corrupted copy in the same pass.  Shared by gm_dvae.hip
// (gm_dvae_corrupt, the standalone corrupting gathers) and gm_gemm.hip (the corrupting gather riding in a forward GEMM).
//
// The rule.  Philox4x32-10 with key (seed mod 2^32, seed >> 32) and counter (e >> 2, step, row, 0x44564145) gives word
// e & 3 of the call to pixel e of row `row` (the row's position in the whole batch) at training batch `step`:
//   salt-and-pepper, T = floor(p 2^31) (host, 64-bit): u < T -> 0; else u - T < T -> 1; else x;
//   gaussian, sigma: fmaf(sigma, n, x) with n the Box-Muller normal of that word (ph_normals_of);
//   none (level 0): x, bit for bit.
#pragma once
#include "gm_gather.h"
#include "gm_philox.h"

#define GM_DVAE_CTR_TAG 0x44564145u       // "DVAE": the fourth counter word

struct CorruptP {
    uint64_t seed;
    PhClock clk;
    int kind; uint32_t thresh; float sigma;
    int64_t row0;                                            // batch position of the first row
    float* out_c; int64_t ld_c;                              // the corrupted rows (the gathers)
};

static __device__ __forceinline__ float sp_pixel(uint32_t u, uint32_t T, float x) {
    return u < T ? 0.f : (u - T < T ? 1.f : x);
}

// Pixels 4q .. 4q + 3 of row `row` (x: their clean values).
static __device__ __forceinline__ float4 corrupt4(const CorruptP& c, uint32_t step, uint32_t row, uint32_t q, float4 x) {
    if (c.kind == GM_NOISE_NONE) return x;
    const uint4 u = PH_BLOCK(c.seed, q, step, row, GM_DVAE_CTR_TAG);
    if (c.kind == GM_NOISE_SALT_PEPPER)
        return make_float4(sp_pixel(u.x, c.thresh, x.x), sp_pixel(u.y, c.thresh, x.y), sp_pixel(u.z, c.thresh, x.z),
                           sp_pixel(u.w, c.thresh, x.w));
    const float4 n = ph_normals_of(u);
    return make_float4(fmaf(c.sigma, n.x, x.x), fmaf(c.sigma, n.y, x.y), fmaf(c.sigma, n.z, x.z),
                       fmaf(c.sigma, n.w, x.w));
}

// gather_body (gm_gather.h) that also writes the corrupted copy of every row to c.out_c: one row per wave, lane l takes
// the pixel quads q = l, l + 64, ... (one Philox call per quad).  Not for the packed-words form (out_bits).
static __device__ __forceinline__ void gather_corrupt_body(const GatherP& p, const CorruptP& c, int bid) {
    const int64_t* ix = p.idx + gm_slot_offset(p.idx_slot);
    const int wpb = blockDim.x >> 6;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = bid * wpb + wave;
    if (b >= p.B) return;
    int64_t r = ix[b];
    if (r < 0 || r >= p.n_rows) r = 0;     // never fault on a corrupt index; parity tests catch it
    float* dst = p.out + (int64_t)b * p.ld_out;
    float* dsc = c.out_c + (int64_t)b * c.ld_c;
    const uint32_t step = ph_step(c.clk), row = (uint32_t)(c.row0 + b);
    const uint32_t* w = p.bits ? p.bits + r * (int64_t)p.wpr : nullptr;
    const float* src = p.bits ? nullptr : p.data + r * (int64_t)p.row_elems;
    if (p.vec) {                           // row_elems % 4 == 0, 16-byte aligned rows (X and Xc)
        for (int q = lane; q < (p.row_elems >> 2); q += 64) {
            const float4 v = w ? gather_bits4(w, q) : reinterpret_cast<const float4*>(src)[q];
            reinterpret_cast<float4*>(dst)[q] = v;
            reinterpret_cast<float4*>(dsc)[q] = corrupt4(c, step, row, (uint32_t)q, v);
        }
        return;
    }
    for (int q = lane; 4 * q < p.row_elems; q += 64) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const int n = min(4, p.row_elems - 4 * q);
        for (int j = 0; j < n; ++j) {
            const int i = 4 * q + j;
            const float x = w ? gather_bit(w, i) : src[i];
            if (j == 0) v.x = x; else if (j == 1) v.y = x; else if (j == 2) v.z = x; else v.w = x;
        }
        const float4 o = corrupt4(c, step, row, (uint32_t)q, v);
        for (int j = 0; j < n; ++j) {
            dst[4 * q + j] = ph_lane(v, j);
            dsc[4 * q + j] = ph_lane(o, j);
        }
    }
}

static __global__ __launch_bounds__(256) void gather_rows_corrupt_kernel(GatherP p, CorruptP c) {
    gather_corrupt_body(p, c, blockIdx.x);
}

// Host: the device form of a gm_corrupt_args (kind, level, seed, step), or GM_EINVAL.
static inline int gm_corrupt_fill(const gm_corrupt_args* a, CorruptP* c) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->kind == GM_NOISE_NONE || a->kind == GM_NOISE_SALT_PEPPER || a->kind == GM_NOISE_GAUSSIAN);
    GM_CHECK_ARG(__builtin_isfinite(a->level) && a->level >= 0.0 && __builtin_isfinite((float)a->level));
    GM_CHECK_ARG(a->kind != GM_NOISE_SALT_PEPPER || a->level <= 1.0);
    GM_CHECK_ARG(a->row0 >= 0);
    c->seed = a->seed;
    c->clk = PhClock{a->step_ctr, a->step_base, a->step_add};
    c->kind = a->level == 0.0 ? GM_NOISE_NONE : a->kind;
    const int64_t T = (int64_t)(a->level * 2147483648.0);                                 // floor(p 2^31), p in [0, 1]
    c->thresh = a->kind == GM_NOISE_SALT_PEPPER ? (uint32_t)T : 0u;
    c->sigma = a->kind == GM_NOISE_GAUSSIAN ? (float)a->level : 0.f;
    c->row0 = a->row0;
    c->out_c = nullptr; c->ld_c = 0;
    return 0;
}

// Host: a corrupting gather's two parameter blocks (the clean rows to `out`, the corrupted ones to `out_c`, both ld_out
// floats apart); gm_gather_fill / gm_gather_fill_bits has filled g.
static inline int gm_gather_corrupt_fill(const gm_corrupt_args* a, float* out_c, GatherP* g, CorruptP* c) {
    const int rc = gm_corrupt_fill(a, c);
    if (rc) return rc;
    GM_CHECK_ARG(out_c && out_c != g->out && !g->out_bits);
    GM_CHECK_ARG((const float*)out_c != g->data && (const void*)out_c != (const void*)g->bits);
    c->out_c = out_c; c->ld_c = g->ld_out;
    g->vec = g->vec && ((reinterpret_cast<uintptr_t>(out_c) & 15) == 0);
    return 0;
}
