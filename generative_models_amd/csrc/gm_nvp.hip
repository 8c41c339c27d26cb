// RealNVP coupling flow (realnvp.py holds the contract; gm_hip.h; the arithmetic in gm_nvp.h).
//
// Everything between the conditioners' GEMMs, as row kernels: one 256-thread workgroup per row, thread i the quads
// i, i + 256, ... of the row in order (a quad = four consecutive elements; of the unsplit image in nvp_pre / nvp_post, so a
// thread owns exactly one Philox block per quad), a thread's partial sum in that order, then the wave butterfly, then the
// four waves in order.  Each kernel has two paths with the same order of operations and so the same bits: 16-byte (8-byte
// on the halves of a checkerboard split) accesses where the host finds the rows aligned and their width a multiple of 4,
// element by element otherwise.
//   nvp_pre_kernel        dequantise + logit + split, the row's preprocessing log-determinant; NOISE mode: u alone
//   nvp_couple_kernel     y_t = x_t exp(s) + t and logdet += sum s (read-add-write by the row's thread 0); or the inverse
//   nvp_loss_kernel       the row's negative log-likelihood and dz = z / b
//   nvp_couple_bwd_kernel dST and dx_t from the cotangent's one or two addends
//   nvp_post_kernel       halves -> image (sigmoid, un-alpha, clamp); PRIOR mode: the sampler's normals -> halves
// No floating-point atomics, no scratch: the same bits on every run, graph or eager.
#include "gm_nvp.h"

namespace {

struct PreP {
    const float* x; int64_t ldx; float* ya; int64_t lda; float* yb; int64_t ldb; float* logdet; float* u; int64_t ldu;
    uint64_t seed; PhClock clk; int64_t row0; uint32_t tag;
    NvpPre c; int mask, mode, D, Da, vec_x, vec_h;
};

__global__ __launch_bounds__(256) void nvp_pre_kernel(PreP p) {
    __shared__ float sh[4];
    const int64_t r = blockIdx.x;
    const uint32_t step = ph_step(p.clk), row = (uint32_t)(p.row0 + r);
    const int nq = (p.D + 3) >> 2;
    if (p.mode == GM_NVP_NOISE) {
        float* u = p.u + r * p.ldu;
        for (int q = threadIdx.x; q < nq; q += 256)
            nvp_store4(u, q, p.D, p.vec_x, ph_units_of(PH_BLOCK(p.seed, (uint32_t)q, step, row, p.tag)));
        return;
    }
    const float* x = p.x + r * p.ldx;
    float* ya = p.ya + r * p.lda;
    float* yb = p.yb + r * p.ldb;
    float acc = 0.f;
    for (int q = threadIdx.x; q < nq; q += 256) {
        const float4 xv = nvp_load4(x, q, p.D, p.vec_x);
        const float4 uv = ph_units_of(PH_BLOCK(p.seed, (uint32_t)q, step, row, p.tag));
        float4 y;
        const float l0 = nvp_pre_elem(xv.x, uv.x, p.c, y.x), l1 = nvp_pre_elem(xv.y, uv.y, p.c, y.y);
        const float l2 = nvp_pre_elem(xv.z, uv.z, p.c, y.z), l3 = nvp_pre_elem(xv.w, uv.w, p.c, y.w);
        const int n = p.D - 4 * q;                               // elements of this quad inside the row
        acc += l0;
        if (n > 1) acc += l1;
        if (n > 2) acc += l2;
        if (n > 3) acc += l3;
        nvp_split_store(ya, yb, q, p.D, p.Da, p.mask, p.vec_h, y);
    }
    const float tot = nvp_row_sum(acc, sh);
    if (threadIdx.x == 0) p.logdet[r] = tot;
}

struct CoupleP {
    const float* st; int64_t ldst; const float* in; int64_t ldin; float* out; int64_t ldout; float* logdet;
    float cap; int inverse, Dt, vec;
};

__global__ __launch_bounds__(256) void nvp_couple_kernel(CoupleP p) {
    __shared__ float sh[4];
    const int64_t r = blockIdx.x;
    const float* ss = p.st + r * p.ldst;
    const float* ts = ss + p.Dt;
    const float* in = p.in + r * p.ldin;
    float* out = p.out + r * p.ldout;
    const int nq = (p.Dt + 3) >> 2;
    float acc = 0.f;
    for (int q = threadIdx.x; q < nq; q += 256) {
        const float4 a = nvp_load4(ss, q, p.Dt, p.vec), t = nvp_load4(ts, q, p.Dt, p.vec), v = nvp_load4(in, q, p.Dt, p.vec);
        const float s0 = nvp_s(a.x, p.cap).s, s1 = nvp_s(a.y, p.cap).s, s2 = nvp_s(a.z, p.cap).s, s3 = nvp_s(a.w, p.cap).s;
        float4 o;
        if (p.inverse) {
            o = make_float4(nvp_inv(v.x, s0, t.x), nvp_inv(v.y, s1, t.y), nvp_inv(v.z, s2, t.z), nvp_inv(v.w, s3, t.w));
        } else {
            o = make_float4(nvp_fwd(v.x, s0, t.x), nvp_fwd(v.y, s1, t.y), nvp_fwd(v.z, s2, t.z), nvp_fwd(v.w, s3, t.w));
            acc += s0;                                           // (the zero fill past the row's end gives s = 0)
            acc += s1;
            acc += s2;
            acc += s3;
        }
        nvp_store4(out, q, p.Dt, p.vec, o);
    }
    if (p.inverse) return;                                       // uniform: the whole grid
    const float tot = nvp_row_sum(acc, sh);
    if (threadIdx.x == 0) p.logdet[r] = p.logdet[r] + tot;
}

struct LossP {
    const float* za; int64_t ldza; const float* zb; int64_t ldzb; const float* logdet; float* part;
    float* dza; int64_t lddza; float* dzb; int64_t lddzb; float cst, scale; int Da, Db, vec_a, vec_b;
};

__device__ __forceinline__ float nvp_loss_half(const float* z, float* dz, int n, int vec, float scale) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int q = threadIdx.x; q < ((n + 3) >> 2); q += 256) {
        const float4 v = nvp_load4(z, q, n, vec);
        acc += v.x * v.x;
        acc += v.y * v.y;
        acc += v.z * v.z;
        acc += v.w * v.w;
        if (dz) nvp_store4(dz, q, n, vec, make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale));
    }
    return acc;
}

__global__ __launch_bounds__(256) void nvp_loss_kernel(LossP p) {
#pragma clang fp contract(off)
    __shared__ float sh[4];
    const int64_t r = blockIdx.x;
    float acc = nvp_loss_half(p.za + r * p.ldza, p.dza ? p.dza + r * p.lddza : nullptr, p.Da, p.vec_a, p.scale);
    acc += nvp_loss_half(p.zb + r * p.ldzb, p.dzb ? p.dzb + r * p.lddzb : nullptr, p.Db, p.vec_b, p.scale);
    const float tot = nvp_row_sum(acc, sh);
    if (threadIdx.x == 0) p.part[r] = (0.5f * tot - p.logdet[r]) + p.cst;
}

struct BwdP {
    const float* st; int64_t ldst; const float* x; int64_t ldx; const float* g0; int64_t ldg0; const float* g1;
    int64_t ldg1; float* dst; int64_t lddst; float* dx; int64_t lddx; float c, cap; int Dt, vec;
};

__device__ __forceinline__ void nvp_bwd_elem(float a, float x, float g, float c, float cap, float& ds, float& dx) {
#pragma clang fp contract(off)
    const NvpS s = nvp_s(a, cap);
    const float ge = g * expf(s.s);
    dx = ge;
    // 1 - tanh^2(a) as 4 e / (1 + e)^2, e = exp(-2 |a|): nothing cancels where the tanh saturates
    const float e = expf(-2.f * fabsf(a)), ope = 1.f + e;
    ds = ((ge * x + c) * cap) * ((4.f * e) / (ope * ope));
}

__global__ __launch_bounds__(256) void nvp_couple_bwd_kernel(BwdP p) {
    const int64_t r = blockIdx.x;
    const float* ss = p.st + r * p.ldst;
    const float* x = p.x + r * p.ldx;
    const float* g0 = p.g0 + r * p.ldg0;
    const float* g1 = p.g1 ? p.g1 + r * p.ldg1 : nullptr;
    float* ds = p.dst + r * p.lddst;
    float* dt = ds + p.Dt;
    float* dx = p.dx ? p.dx + r * p.lddx : nullptr;
    for (int q = threadIdx.x; q < ((p.Dt + 3) >> 2); q += 256) {
        const float4 a = nvp_load4(ss, q, p.Dt, p.vec), xv = nvp_load4(x, q, p.Dt, p.vec);
        float4 g = nvp_load4(g0, q, p.Dt, p.vec);
        if (g1) {
            const float4 h = nvp_load4(g1, q, p.Dt, p.vec);
            g = make_float4(g.x + h.x, g.y + h.y, g.z + h.z, g.w + h.w);
        }
        float4 o, d;
        nvp_bwd_elem(a.x, xv.x, g.x, p.c, p.cap, o.x, d.x);
        nvp_bwd_elem(a.y, xv.y, g.y, p.c, p.cap, o.y, d.y);
        nvp_bwd_elem(a.z, xv.z, g.z, p.c, p.cap, o.z, d.z);
        nvp_bwd_elem(a.w, xv.w, g.w, p.c, p.cap, o.w, d.w);
        nvp_store4(ds, q, p.Dt, p.vec, o);
        nvp_store4(dt, q, p.Dt, p.vec, g);
        if (dx) nvp_store4(dx, q, p.Dt, p.vec, d);
    }
}

struct PostP {
    float* ya; int64_t lda; float* yb; int64_t ldb; float* x; int64_t ldx; uint64_t seed; int64_t row0;
    float alpha, om2a, temp; int mask, mode, D, Da, vec_x, vec_h;
};

__global__ __launch_bounds__(256) void nvp_post_kernel(PostP p) {
    const int64_t r = blockIdx.x;
    float* ya = p.ya + r * p.lda;
    float* yb = p.yb + r * p.ldb;
    const int nq = (p.D + 3) >> 2;
    if (p.mode == GM_NVP_PRIOR) {
        // PH_BLOCK with the key split once, ahead of the loop
        const uint32_t row = (uint32_t)(p.row0 + r), k0 = (uint32_t)p.seed, k1 = (uint32_t)(p.seed >> 32);
        for (int q = threadIdx.x; q < nq; q += 256) {
            float4 z = ph_normals_of(philox10(make_uint4((uint32_t)q, 0u, row, GM_NVP_TAG_S), k0, k1));
            z = make_float4(z.x * p.temp, z.y * p.temp, z.z * p.temp, z.w * p.temp);
            nvp_split_store(ya, yb, q, p.D, p.Da, p.mask, p.vec_h, z);
        }
        return;
    }
    float* x = p.x + r * p.ldx;
    for (int q = threadIdx.x; q < nq; q += 256) {
        const float4 y = nvp_split_load(ya, yb, q, p.D, p.Da, p.mask, p.vec_h);
        nvp_store4(x, q, p.D, p.vec_x, make_float4(nvp_post_elem(y.x, p.alpha, p.om2a), nvp_post_elem(y.y, p.alpha, p.om2a),
                                                    nvp_post_elem(y.z, p.alpha, p.om2a), nvp_post_elem(y.w, p.alpha, p.om2a)));
    }
}

inline bool al(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) == 0; }

// A dense row array of width n by 16-byte accesses.
inline int vec4(const void* p, int64_t ld, int n) { return (n % 4 == 0 && ld % 4 == 0 && al(p, 16)) ? 1 : 0; }

// Both halves of a D-pixel image by vector accesses (gm_nvp.h nvp_split_load / nvp_split_store).
inline int vec_halves(const void* a, int64_t lda, const void* b, int64_t ldb, int D, int mask) {
    if (D % 4 != 0) return 0;
    if (mask == GM_NVP_CHECKER) return (lda % 2 == 0 && ldb % 2 == 0 && al(a, 8) && al(b, 8)) ? 1 : 0;
    return (D % 8 == 0 && lda % 4 == 0 && ldb % 4 == 0 && al(a, 16) && al(b, 16)) ? 1 : 0;
}

inline bool rows_ok(int B) { return B >= 1; }
inline bool d_ok(int D) { return D >= GM_NVP_MIN_D && D <= GM_NVP_MAX_D; }
inline bool dt_ok(int Dt) { return Dt >= 1 && Dt <= (GM_NVP_MAX_D + 1) / 2; }
inline bool mask_ok(int m) { return m == GM_NVP_CHECKER || m == GM_NVP_HALF; }
inline bool alpha_ok(float a) { return a >= 0.f && a < 0.5f; }            // false for a NaN
inline bool cap_ok(float c) { return c > 0.f && c <= (float)GM_NVP_MAX_S_CAP; }

}  // namespace

extern "C" int gm_nvp_pre(void* stream, const gm_nvp_pre_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(rows_ok(a->B) && d_ok(a->D));
    GM_CHECK_ARG(a->mode == GM_NVP_PRE || a->mode == GM_NVP_NOISE);
    GM_CHECK_ARG(a->row0 >= 0 && a->row0 + (int64_t)a->B <= (1ll << 32));
    const int Da = (a->D + 1) / 2, Db = a->D / 2;
    PreP p{};
    p.seed = a->seed; p.clk = PhClock{a->step_ctr, a->step_base, a->step_add}; p.row0 = a->row0; p.tag = a->tag;
    p.mode = a->mode; p.D = a->D; p.Da = Da;
    if (a->mode == GM_NVP_NOISE) {
        GM_CHECK_ARG(a->u && a->ldu >= a->D);
        p.u = a->u; p.ldu = a->ldu; p.vec_x = vec4(a->u, a->ldu, a->D);
    } else {
        GM_CHECK_ARG(a->x && a->ya && a->yb && a->logdet && a->ldx >= a->D && a->lda >= Da && a->ldb >= Db);
        GM_CHECK_ARG(mask_ok(a->mask) && alpha_ok(a->alpha) && a->levels >= 2 && a->levels <= GM_NVP_MAX_LEVELS);
        GM_CHECK_ARG((const float*)a->ya != a->x && (const float*)a->yb != a->x && a->ya != a->yb &&
                     (const float*)a->logdet != a->x && a->logdet != a->ya && a->logdet != a->yb);
        p.x = a->x; p.ldx = a->ldx; p.ya = a->ya; p.lda = a->lda; p.yb = a->yb; p.ldb = a->ldb; p.logdet = a->logdet;
        p.mask = a->mask;
        p.c.alpha = a->alpha; p.c.om2a = 1.f - 2.f * a->alpha; p.c.log_om2a = logf(p.c.om2a); p.c.lv = (float)a->levels;
        p.vec_x = vec4(a->x, a->ldx, a->D);
        p.vec_h = vec_halves(a->ya, a->lda, a->yb, a->ldb, a->D, a->mask);
    }
    hipLaunchKernelGGL(nvp_pre_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_nvp_couple(void* stream, const gm_nvp_couple_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(rows_ok(a->B) && dt_ok(a->Dt) && cap_ok(a->s_cap));
    GM_CHECK_ARG(a->st && a->inp && a->out && a->ldst >= 2 * (int64_t)a->Dt && a->ldin >= a->Dt && a->ldout >= a->Dt);
    GM_CHECK_ARG((const float*)a->out != a->st && (const float*)a->out != a->inp);
    GM_CHECK_ARG(a->inverse == 0 || a->inverse == 1);
    GM_CHECK_ARG(a->inverse || (a->logdet && a->logdet != a->out && (const float*)a->logdet != a->st &&
                                (const float*)a->logdet != a->inp));
    CoupleP p{a->st, a->ldst, a->inp, a->ldin, a->out, a->ldout, a->logdet, a->s_cap, a->inverse, a->Dt, 0};
    p.vec = vec4(a->st, a->ldst, a->Dt) & vec4(a->inp, a->ldin, a->Dt) & vec4(a->out, a->ldout, a->Dt);
    hipLaunchKernelGGL(nvp_couple_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_nvp_loss(void* stream, const gm_nvp_loss_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(rows_ok(a->B) && dt_ok(a->Da) && dt_ok(a->Db) && (a->Da == a->Db || a->Da == a->Db + 1));
    GM_CHECK_ARG(a->za && a->zb && a->logdet && a->part && a->ldza >= a->Da && a->ldzb >= a->Db);
    GM_CHECK_ARG((const float*)a->part != a->za && (const float*)a->part != a->zb && (const float*)a->part != a->logdet);
    GM_CHECK_ARG((a->dza != nullptr) == (a->dzb != nullptr));
    GM_CHECK_ARG(__builtin_isfinite(a->cst) && __builtin_isfinite(a->scale) && a->scale >= 0.f);
    if (a->dza) {
        GM_CHECK_ARG(a->lddza >= a->Da && a->lddzb >= a->Db && a->dza != a->dzb && a->dza != a->part && a->dzb != a->part);
        GM_CHECK_ARG((const float*)a->dza != a->za && (const float*)a->dza != a->zb && (const float*)a->dzb != a->za &&
                     (const float*)a->dzb != a->zb && (const float*)a->dza != a->logdet &&
                     (const float*)a->dzb != a->logdet);
    }
    LossP p{a->za, a->ldza, a->zb, a->ldzb, a->logdet, a->part, a->dza, a->lddza, a->dzb, a->lddzb, a->cst, a->scale,
            a->Da, a->Db, 0, 0};
    p.vec_a = vec4(a->za, a->ldza, a->Da) & (a->dza ? vec4(a->dza, a->lddza, a->Da) : 1);
    p.vec_b = vec4(a->zb, a->ldzb, a->Db) & (a->dzb ? vec4(a->dzb, a->lddzb, a->Db) : 1);
    hipLaunchKernelGGL(nvp_loss_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_nvp_couple_bwd(void* stream, const gm_nvp_couple_bwd_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(rows_ok(a->B) && dt_ok(a->Dt) && cap_ok(a->s_cap) && __builtin_isfinite(a->c));
    GM_CHECK_ARG(a->st && a->x && a->g0 && a->dst && a->ldst >= 2 * (int64_t)a->Dt && a->ldx >= a->Dt &&
                 a->ldg0 >= a->Dt && a->lddst >= 2 * (int64_t)a->Dt);
    GM_CHECK_ARG(!a->g1 || a->ldg1 >= a->Dt);
    GM_CHECK_ARG(!a->dx || (a->lddx >= a->Dt && a->dx != a->dst));
    for (const float* in : {a->st, a->x, a->g0, a->g1})
        GM_CHECK_ARG(!in || ((const float*)a->dst != in && (const float*)a->dx != in));
    BwdP p{a->st, a->ldst, a->x, a->ldx, a->g0, a->ldg0, a->g1, a->ldg1, a->dst, a->lddst, a->dx, a->lddx, a->c, a->s_cap,
           a->Dt, 0};
    p.vec = vec4(a->st, a->ldst, a->Dt) & vec4(a->x, a->ldx, a->Dt) & vec4(a->g0, a->ldg0, a->Dt) &
            vec4(a->dst, a->lddst, a->Dt) & (a->g1 ? vec4(a->g1, a->ldg1, a->Dt) : 1) &
            (a->dx ? vec4(a->dx, a->lddx, a->Dt) : 1);
    hipLaunchKernelGGL(nvp_couple_bwd_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_nvp_post(void* stream, const gm_nvp_post_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(rows_ok(a->B) && d_ok(a->D) && mask_ok(a->mask));
    GM_CHECK_ARG(a->mode == GM_NVP_POST || a->mode == GM_NVP_PRIOR);
    const int Da = (a->D + 1) / 2, Db = a->D / 2;
    GM_CHECK_ARG(a->ya && a->yb && a->ya != a->yb && a->lda >= Da && a->ldb >= Db);
    PostP p{};
    p.ya = a->ya; p.lda = a->lda; p.yb = a->yb; p.ldb = a->ldb; p.mask = a->mask; p.mode = a->mode; p.D = a->D; p.Da = Da;
    p.vec_h = vec_halves(a->ya, a->lda, a->yb, a->ldb, a->D, a->mask);
    if (a->mode == GM_NVP_PRIOR) {
        GM_CHECK_ARG(a->row0 >= 0 && a->row0 + (int64_t)a->B <= (1ll << 32));
        GM_CHECK_ARG(__builtin_isfinite(a->temperature) && a->temperature >= 0.f);
        p.seed = a->seed; p.row0 = a->row0; p.temp = a->temperature;
    } else {
        GM_CHECK_ARG(a->x && a->ldx >= a->D && a->x != a->ya && a->x != a->yb && alpha_ok(a->alpha));
        p.x = a->x; p.ldx = a->ldx; p.alpha = a->alpha; p.om2a = 1.f - 2.f * a->alpha;
        p.vec_x = vec4(a->x, a->ldx, a->D);
    }
    hipLaunchKernelGGL(nvp_post_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
