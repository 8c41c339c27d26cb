// Flow matching (flowmatch.py holds the contract): the one definition of the path, the noise rule
// and the solver's stage rule, shared by every kernel of gm_fm.hip.
//
// The rule.  Philox4x32-10 with key (seed mod 2^32, seed >> 32), batch row `row` at batch `step`:
//   dequantisation uniform of pixel e: ph_unit of word e & 3 of counter (e >> 2, step, row, tag_d) -- RealNVP's indexing;
//   y1 and the element's log-determinant: nvp_pre_elem (gm_nvp.h), so y1 and logdet_pre are gm_nvp_pre's bits;
//   grid index: j = mulhi(word 0 of counter (0, step, row, tag_t), T + 1), t_j = j / T;
//   y0 of pixels 4q .. 4q + 3: ph_normals at counter (q, step, row, tag_n);
//   y_t = fmaf(tt[j], y1, tc[j] * y0) (the product rounded, then one fused multiply-add);  u = y1 - y0.
// One 256-thread workgroup per row, thread i the quads i, i + 256, ... (ddpm_qsample_row's mapping).
#pragma once
#include "gm_ddpm.h"
#include "gm_nvp.h"

struct FmNoiseP {
    uint64_t seed; uint32_t tag_d, tag_t, tag_n;
    PhClock clk;
    int64_t row0;                                            // batch position of the first row
};
struct FmTabP { const float* tt; const float* tc; const float* temb; int T, E; };
struct FmOutP {
    float* xin; int64_t ldin; float* u; int64_t ldu; float* logdet; int32_t* j;
    float* y1; int64_t ldy1; float* y0; int64_t ldy0;
    NvpPre c; int vec_tail;
};

// y_t of one element on the straight path from y0 (t = 0) to y1 (t = 1): tt = 0, tc = 1 returns y0 and tt = 1, tc = 0
// returns y1 exactly.
static __device__ __forceinline__ float fm_path(float tt, float tc, float y1, float y0) {
#pragma clang fp contract(off)
    const float p = tc * y0;
    return __builtin_fmaf(tt, y1, p);
}

static __device__ __forceinline__ float fm_target(float y1, float y0) {
#pragma clang fp contract(off)
    return y1 - y0;
}

// One solver stage of one element: k the field at this evaluation, (base, acc) the step's state.  Returns the next
// evaluation's y.
static __device__ __forceinline__ float fm_stage1(float k, float& base, float& acc, float ha, float hb, bool first,
                                                  bool last) {
#pragma clang fp contract(off)
    const float p = hb * k;
    acc = first ? p : __builtin_fmaf(hb, k, acc);
    if (last) {
        base = base + acc;
        return base;
    }
    return __builtin_fmaf(ha, k, base);
}

// Batch row b (this workgroup's): j, [y_t | temb[j]] -> o.xin, the target -> o.u, the preprocessing log-determinant ->
// o.logdet, the clean pixels -> clean (or null).  sh: four floats of LDS.  Every thread of the workgroup calls it.
static __device__ __forceinline__ void fm_qsample_row(const FmNoiseP& n, const FmTabP& s, const FmOutP& o, int64_t b,
                                                      int I, int vec, float* clean, const DdpmRow& rs, float* sh) {
    const uint32_t step = ph_step(n.clk), row = (uint32_t)(n.row0 + b);
    uint32_t j = 0;
    if ((threadIdx.x & 63) == 0) j = __umulhi(PH_BLOCK(n.seed, 0u, step, row, n.tag_t).x, (uint32_t)s.T + 1u);
    j = (uint32_t)__shfl((int)j, 0, 64);
    const float tt = s.tt[j], tc = s.tc[j];
    float* xin = o.xin + b * o.ldin;
    float* up = o.u + b * o.ldu;
    float* y1p = o.y1 ? o.y1 + b * o.ldy1 : nullptr;
    float* y0p = o.y0 ? o.y0 + b * o.ldy0 : nullptr;
    float acc = 0.f;
    if (vec) {                             // I % 4 == 0, every row 16-byte aligned
        for (int q = threadIdx.x; q < (I >> 2); q += blockDim.x) {
            const float4 v = rs.quad(q);
            const float4 uv = ph_units_of(PH_BLOCK(n.seed, (uint32_t)q, step, row, n.tag_d));
            const float4 z = ph_normals(n.seed, (uint32_t)q, step, row, n.tag_n);
            float4 y;
            const float l0 = nvp_pre_elem(v.x, uv.x, o.c, y.x), l1 = nvp_pre_elem(v.y, uv.y, o.c, y.y);
            const float l2 = nvp_pre_elem(v.z, uv.z, o.c, y.z), l3 = nvp_pre_elem(v.w, uv.w, o.c, y.w);
            acc += l0;
            acc += l1;
            acc += l2;
            acc += l3;
            if (clean) reinterpret_cast<float4*>(clean)[q] = v;
            reinterpret_cast<float4*>(xin)[q] = make_float4(fm_path(tt, tc, y.x, z.x), fm_path(tt, tc, y.y, z.y),
                                                            fm_path(tt, tc, y.z, z.z), fm_path(tt, tc, y.w, z.w));
            reinterpret_cast<float4*>(up)[q] = make_float4(fm_target(y.x, z.x), fm_target(y.y, z.y), fm_target(y.z, z.z),
                                                           fm_target(y.w, z.w));
            if (y1p) reinterpret_cast<float4*>(y1p)[q] = y;
            if (y0p) reinterpret_cast<float4*>(y0p)[q] = z;
        }
    } else {
        for (int q = threadIdx.x; 4 * q < I; q += blockDim.x) {
            const float4 uv = ph_units_of(PH_BLOCK(n.seed, (uint32_t)q, step, row, n.tag_d));
            const float4 z = ph_normals(n.seed, (uint32_t)q, step, row, n.tag_n);
            const int cnt = min(4, I - 4 * q);
            for (int e = 0; e < cnt; ++e) {
                const int i = 4 * q + e;
                const float x = rs.elem(i), ze = ph_lane(z, e);
                float y;
                acc += nvp_pre_elem(x, ph_lane(uv, e), o.c, y);
                if (clean) clean[i] = x;
                xin[i] = fm_path(tt, tc, y, ze);
                up[i] = fm_target(y, ze);
                if (y1p) y1p[i] = y;
                if (y0p) y0p[i] = ze;
            }
        }
    }
    ddpm_tail(xin + I, s.temb + (int64_t)j * s.E, s.E, o.vec_tail);
    const float tot = nvp_row_sum(acc, sh);                  // gm_nvp_pre's order: the thread's quads, the wave, the waves
    if (threadIdx.x == 0) {
        o.logdet[b] = tot;
        if (o.j) o.j[b] = (int32_t)j;
    }
}
