// gm_pdw.hip -- Primal-Dual Wasserstein GAN (pdwgan.py; Gemici, Akata, Welling, arXiv 1805.09575): the two row
// kernels that make the WGAN-GP chain a PD-WGAN one.
//   gm_pdw_couple  the primal coupling of an image with its own reconstruction: n_b = ||x_b - x~_b||, the row's share
//                  of the encoder loss, d L_E / d (pre-sigmoid x~), the interpolate x^ = t x + (1 - t) x~ and a copy
//                  of x, both written into the critic's stacked input -- one pass over the row pair;
//   gm_pdw_dir     pen_b = ||g_b - d_b||^2 and gamma_b = (2 lambda / b)(g_b - d_b), d_b = (x_b - x~_b) / n_b: the
//                  counterpart of gm_gp_norm (K11) with the target a unit VECTOR instead of a unit norm.
// One wave per row and per workgroup (as K11: B short latency chains spread over the CUs), wave64 shuffle reductions
// in a fixed order, no atomics, no LDS, no scratch.  VEC4 (I % 4 == 0, I <= 1024, 16-byte aligned rows): the rows
// stay in registers between the norm and the outputs.
#include "gm_common.h"

struct PdwCoupleP {
    const float* x; int64_t ldx;
    const float* xr; int64_t ldr;
    const float* t; gm_slot t_slot;
    float* n; float* share;
    float* dA; int64_t ldd;
    float* xhat; int64_t ldh;
    float* xcopy; int64_t ldc;
    float inv_b; int B, I;
};

__device__ __forceinline__ void pdw_couple_elem(const PdwCoupleP& p, float xv, float rv, float rn, float ev, int has_t,
                                                float& da, float& xh) {
    // d L_E / d x~ = -d / b with d = (x - x~) / n; times sigmoid'(a) = x~ (1 - x~) of the decoder's output layer
    da = -(((xv - rv) * rn) * p.inv_b) * (rv * (1.f - rv));
    xh = has_t ? gm_interp_unfused(ev, xv, rv) : 0.f;
}

template <bool VEC4>
__global__ __launch_bounds__(64) void pdw_couple_kernel(PdwCoupleP p) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const float* xrow = p.x + (int64_t)b * p.ldx;
    const float* rrow = p.xr + (int64_t)b * p.ldr;
    const int has_t = p.t != nullptr;
    const float ev = has_t ? (p.t + gm_slot_offset(p.t_slot))[b] : 0.f;
    float ss = 0.f;
    float4 xv[4], rv[4];
    if (VEC4) {
        const int n4 = p.I >> 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i4 = min(lane + 64 * j, n4 - 1);                   // clamped: branch-free loads
            xv[j] = reinterpret_cast<const float4*>(xrow)[i4];
            rv[j] = reinterpret_cast<const float4*>(rrow)[i4];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lane + 64 * j < n4) {
                const float a = xv[j].x - rv[j].x, c = xv[j].y - rv[j].y, e = xv[j].z - rv[j].z, f = xv[j].w - rv[j].w;
                ss += (a * a + c * c) + (e * e + f * f);
            }
    } else {
        for (int i = lane; i < p.I; i += 64) { const float a = xrow[i] - rrow[i]; ss += a * a; }
    }
    ss = gm_wave_sum(ss);
    const float n = sqrtf(ss);
    const float rn = (n > 0.f) ? 1.f / n : 0.f;                          // d = 0 where the reconstruction is exact
    if (lane == 0) {
        if (p.n) p.n[b] = n;
        p.share[b] = n * p.inv_b;
    }
    float* da = p.dA ? p.dA + (int64_t)b * p.ldd : nullptr;
    float* xh = p.xhat ? p.xhat + (int64_t)b * p.ldh : nullptr;
    float* xc = p.xcopy ? p.xcopy + (int64_t)b * p.ldc : nullptr;
    if (VEC4) {
        const int n4 = p.I >> 2;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i4 = lane + 64 * j;
            if (i4 < n4) {
                float4 d, h;
                pdw_couple_elem(p, xv[j].x, rv[j].x, rn, ev, has_t, d.x, h.x);
                pdw_couple_elem(p, xv[j].y, rv[j].y, rn, ev, has_t, d.y, h.y);
                pdw_couple_elem(p, xv[j].z, rv[j].z, rn, ev, has_t, d.z, h.z);
                pdw_couple_elem(p, xv[j].w, rv[j].w, rn, ev, has_t, d.w, h.w);
                if (da) reinterpret_cast<float4*>(da)[i4] = d;
                if (xh) reinterpret_cast<float4*>(xh)[i4] = h;
                if (xc) reinterpret_cast<float4*>(xc)[i4] = xv[j];
            }
        }
    } else {
        for (int i = lane; i < p.I; i += 64) {
            float d, h;
            pdw_couple_elem(p, xrow[i], rrow[i], rn, ev, has_t, d, h);
            if (da) da[i] = d;
            if (xh) xh[i] = h;
            if (xc) xc[i] = xrow[i];
        }
    }
}

static bool pdw_al16(const void* q, int64_t ld) {
    return q == nullptr || ((reinterpret_cast<uintptr_t>(q) & 15) == 0 && ld % 4 == 0);
}

extern "C" int gm_pdw_couple(void* stream, const float* x, int64_t ldx, const float* xr, int64_t ldr, const float* t,
                             gm_slot t_slot, float* n, float* share, float* dA, int64_t ldd, float* xhat, int64_t ldh,
                             float* xcopy, int64_t ldc, float inv_b, int B, int I) {
    GM_CHECK_ARG(x && xr && share && B > 0 && I > 0 && ldx >= I && ldr >= I);
    GM_CHECK_ARG((!dA || ldd >= I) && (!xhat || (t && ldh >= I)) && (!xcopy || ldc >= I));
    PdwCoupleP p{x, ldx, xr, ldr, xhat ? t : nullptr, t_slot, n, share, dA, ldd, xhat, ldh, xcopy, ldc, inv_b, B, I};
    const bool vec4 = (I % 4 == 0) && I <= 1024 && pdw_al16(x, ldx) && pdw_al16(xr, ldr) && pdw_al16(dA, ldd) &&
                      pdw_al16(xhat, ldh) && pdw_al16(xcopy, ldc);
    if (vec4) hipLaunchKernelGGL(pdw_couple_kernel<true>, dim3(B), dim3(64), 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(pdw_couple_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

// pen[b] = ||g_b - d_b||^2 ; gamma_b = lambda * inv_b * 2 (g_b - d_b), d_b = (x_b - x~_b) / n_b (0 where n_b == 0).
template <bool VEC4>
__global__ __launch_bounds__(64) void pdw_dir_kernel(const float* __restrict__ g, int64_t ldg,
                                                    const float* __restrict__ x, int64_t ldx,
                                                    const float* __restrict__ xr, int64_t ldr,
                                                    const float* __restrict__ nrm, float* __restrict__ gam,
                                                    int64_t ldm, float* __restrict__ pen, float lambda, float inv_b,
                                                    int B, int I) {
    const int lane = threadIdx.x, b = blockIdx.x;
    const float* grow = g + (int64_t)b * ldg;
    const float* xrow = x + (int64_t)b * ldx;
    const float* rrow = xr + (int64_t)b * ldr;
    float* o = gam + (int64_t)b * ldm;
    const float n = nrm[b];
    const float rn = (n > 0.f) ? 1.f / n : 0.f;
    const float coef = lambda * (inv_b * 2.f);
    float ss = 0.f;
    if (VEC4) {
        const int n4 = I >> 2;
        float4 e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i4 = min(lane + 64 * j, n4 - 1);
            const float4 gv = reinterpret_cast<const float4*>(grow)[i4];
            const float4 xv = reinterpret_cast<const float4*>(xrow)[i4];
            const float4 rv = reinterpret_cast<const float4*>(rrow)[i4];
            e[j] = make_float4(gv.x - (xv.x - rv.x) * rn, gv.y - (xv.y - rv.y) * rn, gv.z - (xv.z - rv.z) * rn,
                               gv.w - (xv.w - rv.w) * rn);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lane + 64 * j < n4) {
                ss += (e[j].x * e[j].x + e[j].y * e[j].y) + (e[j].z * e[j].z + e[j].w * e[j].w);
                reinterpret_cast<float4*>(o)[lane + 64 * j] =
                    make_float4(e[j].x * coef, e[j].y * coef, e[j].z * coef, e[j].w * coef);
            }
    } else {
        for (int i = lane; i < I; i += 64) {
            const float e = grow[i] - (xrow[i] - rrow[i]) * rn;
            ss += e * e;
            o[i] = e * coef;
        }
    }
    ss = gm_wave_sum(ss);
    if (lane == 0) pen[b] = ss;
}

extern "C" int gm_pdw_dir(void* stream, const float* g, int64_t ldg, const float* x, int64_t ldx, const float* xr,
                          int64_t ldr, const float* n, float* gamma, int64_t ldm, float* pen, float lambda,
                          float inv_b, int B, int I) {
    GM_CHECK_ARG(g && x && xr && n && gamma && pen && B > 0 && I > 0 && ldg >= I && ldx >= I && ldr >= I && ldm >= I);
    const bool vec4 = (I % 4 == 0) && I <= 1024 && pdw_al16(g, ldg) && pdw_al16(x, ldx) && pdw_al16(xr, ldr) &&
                      pdw_al16(gamma, ldm);
    if (vec4) hipLaunchKernelGGL(pdw_dir_kernel<true>, dim3(B), dim3(64), 0, (hipStream_t)stream, g, ldg, x, ldx, xr,
                                 ldr, n, gamma, ldm, pen, lambda, inv_b, B, I);
    else hipLaunchKernelGGL(pdw_dir_kernel<false>, dim3(B), dim3(64), 0, (hipStream_t)stream, g, ldg, x, ldx, xr, ldr,
                            n, gamma, ldm, pen, lambda, inv_b, B, I);
    GM_LAUNCH_RET();
}
