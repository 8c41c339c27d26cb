// Masked autoregressive flow, MAF (maf.py holds the contract; gm_hip.h; the arithmetic in gm_maf.h).
//
// maf_couple_kernel / maf_couple_bwd_kernel: what lies between a layer's GEMMs, as row kernels on gm_nvp.hip's mapping: one
//   256-thread workgroup per row, thread i the quads i, i + 256, ... of the row in order, a thread's partial sum in that
//   order, then the wave butterfly, then the four waves in order.  Two paths with the same order of operations and so the
//   same bits: 16-byte accesses where the host finds every row aligned and D a multiple of 4, element by element otherwise.
// maf_mask_kernel: zeroes W and Adam's two moments at the masked entries of linear.weight and of both halves of out.weight,
//   the masks from the degree vectors; it reads no weight and writes masked entries only.
// maf_invert_kernel: one layer's inverse in one launch, on made_sample_kernel's mapping.  One wave per row, four rows per
//   workgroup, no LDS, no barrier.  A lane keeps the pre-activations h_j of j = 64 i + lane in NJ = ceil(H / 64) registers
//   (compile-time indices: no scratch).  Positions go in order of degree, 64 at a time: each lane first fetches everything
//   position c0 + lane needs that does not depend on the chain -- the pixel index, its u, its two output biases -- then the
//   64 steps run with wave-uniform lane reads.  A step: the shift and the log-scale pre-activation (two lane-local sums in
//   ascending j, two interleaved wave butterflies, the biases), s, y = u exp(s) + m, h += y W1T[d, :].  The three weight
//   rows of the next position are loaded before the current one is reduced.  The position t has degree t + 1, so the masks
//   are (m_h <= t) and (m_h > t); masked weights are not loaded.
// No floating-point atomics, fixed reduction orders: the same bits on every run, whatever n and the grid.
#include "gm_maf.h"

namespace {

struct CoupleP {
    const float* y; int64_t ldy; const float* ma; int64_t ldma; float* u; int64_t ldu; float* logdet;
    float cap; int D, vec;
};

__global__ __launch_bounds__(256) void maf_couple_kernel(CoupleP p) {
    __shared__ float sh[4];
    const int64_t r = blockIdx.x;
    const float* ms = p.ma + r * p.ldma;
    const float* as = ms + p.D;
    const float* y = p.y + r * p.ldy;
    float* u = p.u + r * p.ldu;
    const int nq = (p.D + 3) >> 2;
    float acc = 0.f;
    for (int q = threadIdx.x; q < nq; q += 256) {
        const float4 m = nvp_load4(ms, q, p.D, p.vec), a = nvp_load4(as, q, p.D, p.vec), v = nvp_load4(y, q, p.D, p.vec);
        const float s0 = nvp_s(a.x, p.cap).s, s1 = nvp_s(a.y, p.cap).s, s2 = nvp_s(a.z, p.cap).s, s3 = nvp_s(a.w, p.cap).s;
        nvp_store4(u, q, p.D, p.vec,
                   make_float4(maf_fwd(v.x, s0, m.x), maf_fwd(v.y, s1, m.y), maf_fwd(v.z, s2, m.z), maf_fwd(v.w, s3, m.w)));
        acc += s0;                                               // (the zero fill past the row's end gives s = 0)
        acc += s1;
        acc += s2;
        acc += s3;
    }
    const float tot = nvp_row_sum(acc, sh);
    if (threadIdx.x == 0) p.logdet[r] = p.logdet[r] - tot;
}

struct BwdP {
    const float* ma; int64_t ldma; const float* u; int64_t ldu; const float* g; int64_t ldg;
    float* dout; int64_t lddout; float* dy; int64_t lddy; float c, cap; int D, vec;
};

__global__ __launch_bounds__(256) void maf_couple_bwd_kernel(BwdP p) {
    const int64_t r = blockIdx.x;
    const float* as = p.ma + r * p.ldma + p.D;
    const float* u = p.u + r * p.ldu;
    const float* g = p.g + r * p.ldg;
    float* dm = p.dout + r * p.lddout;
    float* da = dm + p.D;
    float* dy = p.dy ? p.dy + r * p.lddy : nullptr;
    for (int q = threadIdx.x; q < ((p.D + 3) >> 2); q += 256) {
        const float4 a = nvp_load4(as, q, p.D, p.vec), uv = nvp_load4(u, q, p.D, p.vec), gv = nvp_load4(g, q, p.D, p.vec);
        float4 om, oa, oy;
        maf_bwd_elem(a.x, uv.x, gv.x, p.c, p.cap, om.x, oa.x, oy.x);
        maf_bwd_elem(a.y, uv.y, gv.y, p.c, p.cap, om.y, oa.y, oy.y);
        maf_bwd_elem(a.z, uv.z, gv.z, p.c, p.cap, om.z, oa.z, oy.z);
        maf_bwd_elem(a.w, uv.w, gv.w, p.c, p.cap, om.w, oa.w, oy.w);
        nvp_store4(dm, q, p.D, p.vec, om);
        nvp_store4(da, q, p.D, p.vec, oa);
        if (dy) nvp_store4(dy, q, p.D, p.vec, oy);
    }
}

struct MaskP {
    float* W1; float* m1; float* v1; float* W2; float* m2; float* v2;
    const int* m_in; const int* m_h; int D, H;
};

__global__ __launch_bounds__(256) void maf_mask_kernel(MaskP p) {
    const int n = p.D * p.H;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    if (p.m_h[t / p.D] < p.m_in[t % p.D]) {            // linear.weight [H, D]: keeps (j, i) iff m_h[j] >= m_in[i]
        p.W1[t] = 0.f;
        if (p.m1) { p.m1[t] = 0.f; p.v1[t] = 0.f; }
    }
    if (p.m_in[t / p.H] <= p.m_h[t % p.H]) {           // out.weight [2 D, H]: rows d and D + d keep (d, j) iff m_in[d] > m_h[j]
        p.W2[t] = 0.f;
        p.W2[t + n] = 0.f;
        if (p.m2) { p.m2[t] = 0.f; p.v2[t] = 0.f; p.m2[t + n] = 0.f; p.v2[t + n] = 0.f; }
    }
}

struct InvP {
    const float* u; int64_t ldu; float* y; int64_t ldy; float* s; int64_t lds;
    const float* W2; const float* b2; const float* W1T; const float* b1;
    const int* m_h; const int* inv_order;
    float cap; int64_t n; int D, H;
};

constexpr int MAF_NO_UNIT = 0x7fffffff;                // degree of the lanes past H: in neither mask

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// Two wave sums, their butterflies interleaved step by step (each in gm_wave_sum's order).
__device__ __forceinline__ void wave_sum2(float& a, float& b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ta = __shfl_xor(a, o, 64), tb = __shfl_xor(b, o, 64);
        a += ta;
        b += tb;
    }
}

// The three weight rows of pixel d at position t (degree t + 1): both halves of out.weight where m_h <= t, W1T's where
// m_h > t.
template <int NJ>
__device__ __forceinline__ void maf_rows(const InvP& q, const int (&mh)[NJ], int lane, int d, int t, float (&wm)[NJ],
                                         float (&wa)[NJ], float (&w1)[NJ]) {
    const float* rm = q.W2 + (int64_t)d * q.H + lane;
    const float* ra = q.W2 + ((int64_t)d + q.D) * q.H + lane;
    const float* r1 = q.W1T + (int64_t)d * q.H + lane;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const bool lo = mh[j] <= t;
        wm[j] = lo ? rm[j * 64] : 0.f;
        wa[j] = lo ? ra[j * 64] : 0.f;
        w1[j] = (!lo && mh[j] != MAF_NO_UNIT) ? r1[j * 64] : 0.f;
    }
}

template <int NJ>
__global__ __launch_bounds__(256) void maf_invert_kernel(InvP q) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= q.n) return;                              // a whole wave: the kernel has no barrier
    float h[NJ];
    int mh[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = j * 64 + lane;
        h[j] = k < q.H ? q.b1[k] : 0.f;
        mh[j] = k < q.H ? q.m_h[k] : MAF_NO_UNIT;
    }
    for (int c0 = 0; c0 < q.D; c0 += 64) {
        const int tl = c0 + lane;
        int dl = 0;
        float ul = 0.f, bml = 0.f, bal = 0.f;
        if (tl < q.D) {
            dl = min(max(q.inv_order[tl], 0), q.D - 1);   // never read outside a row, whatever the table holds
            ul = q.u[r * q.ldu + dl];
            bml = q.b2[dl];
            bal = q.b2[q.D + dl];
        }
        float yl = 0.f, sl = 0.f;
        const int cnt = min(64, q.D - c0);
        float wmc[NJ], wac[NJ], w1c[NJ];
        maf_rows<NJ>(q, mh, lane, lane_i(dl, 0), c0, wmc, wac, w1c);
        for (int st = 0; st < cnt; ++st) {
            float wmn[NJ], wan[NJ], w1n[NJ];
            const int sn = min(st + 1, cnt - 1);       // (the chunk's last step reloads its own rows: unused)
            maf_rows<NJ>(q, mh, lane, lane_i(dl, sn), c0 + sn, wmn, wan, w1n);
            float am = 0.f, aa = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const float a = fmaxf(h[j], 0.f);
                am = fmaf(wmc[j], a, am);
                aa = fmaf(wac[j], a, aa);
            }
            wave_sum2(am, aa);
            const float mv = am + lane_f(bml, st);
            const float sv = nvp_s(aa + lane_f(bal, st), q.cap).s;
            const float yv = maf_inv(lane_f(ul, st), sv, mv);
#pragma unroll
            for (int j = 0; j < NJ; ++j) h[j] = fmaf(yv, w1c[j], h[j]);   // unconditional: y is real
            if (lane == st) { yl = yv; sl = sv; }
#pragma unroll
            for (int j = 0; j < NJ; ++j) { wmc[j] = wmn[j]; wac[j] = wan[j]; w1c[j] = w1n[j]; }
        }
        if (tl < q.D) {
            q.y[r * q.ldy + dl] = yl;
            if (q.s) q.s[r * q.lds + dl] = sl;
        }
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// A row array of width D by 16-byte accesses.
inline int vec4(const void* p, int64_t ld, int D) { return (D % 4 == 0 && ld % 4 == 0 && al16(p)) ? 1 : 0; }

inline bool shape_ok(int D, int H) { return D >= GM_MAF_MIN_D && D <= GM_MAF_MAX_D && H >= 1 && H <= GM_MAF_MAX_H; }
inline bool d_ok(int D) { return D >= GM_MAF_MIN_D && D <= GM_MAF_MAX_D; }
inline bool cap_ok(float c) { return c > 0.f && c <= (float)GM_NVP_MAX_S_CAP; }   // false for a NaN

template <int NJ>
void invert_launch(hipStream_t st, const InvP& p) {
    hipLaunchKernelGGL(maf_invert_kernel<NJ>, dim3((unsigned)((p.n + 3) / 4)), dim3(256), 0, st, p);
}

}  // namespace

extern "C" int gm_maf_couple(void* stream, const gm_maf_couple_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->B >= 1 && d_ok(a->D) && cap_ok(a->s_cap));
    GM_CHECK_ARG(a->y && a->ma && a->u && a->logdet && a->ldy >= a->D && a->ldma >= 2 * (int64_t)a->D && a->ldu >= a->D);
    GM_CHECK_ARG((const float*)a->u != a->y && (const float*)a->u != a->ma && a->logdet != a->u &&
                 (const float*)a->logdet != a->y && (const float*)a->logdet != a->ma);
    CoupleP p{a->y, a->ldy, a->ma, a->ldma, a->u, a->ldu, a->logdet, a->s_cap, a->D, 0};
    p.vec = vec4(a->y, a->ldy, a->D) & vec4(a->ma, a->ldma, a->D) & vec4(a->u, a->ldu, a->D);
    hipLaunchKernelGGL(maf_couple_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_maf_couple_bwd(void* stream, const gm_maf_couple_bwd_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->B >= 1 && d_ok(a->D) && cap_ok(a->s_cap) && __builtin_isfinite(a->c));
    GM_CHECK_ARG(a->ma && a->u && a->g && a->dout && a->ldma >= 2 * (int64_t)a->D && a->ldu >= a->D && a->ldg >= a->D &&
                 a->lddout >= 2 * (int64_t)a->D);
    GM_CHECK_ARG(!a->dy || (a->lddy >= a->D && a->dy != a->dout));
    for (const float* in : {a->ma, a->u, a->g})
        GM_CHECK_ARG((const float*)a->dout != in && (const float*)a->dy != in);
    BwdP p{a->ma, a->ldma, a->u, a->ldu, a->g, a->ldg, a->dout, a->lddout, a->dy, a->lddy, a->c, a->s_cap, a->D, 0};
    p.vec = vec4(a->ma, a->ldma, a->D) & vec4(a->u, a->ldu, a->D) & vec4(a->g, a->ldg, a->D) &
            vec4(a->dout, a->lddout, a->D) & (a->dy ? vec4(a->dy, a->lddy, a->D) : 1);
    hipLaunchKernelGGL(maf_couple_bwd_kernel, dim3((unsigned)a->B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_maf_mask(void* stream, const gm_maf_mask_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->W1 && a->W2 && a->m_in && a->m_h && shape_ok(a->D, a->H) && a->W1 != a->W2);
    GM_CHECK_ARG((a->m1 != nullptr) == (a->v1 != nullptr) && (a->m2 != nullptr) == (a->v2 != nullptr));
    MaskP p{a->W1, a->m1, a->v1, a->W2, a->m2, a->v2, a->m_in, a->m_h, a->D, a->H};
    hipLaunchKernelGGL(maf_mask_kernel, dim3((unsigned)((a->D * a->H + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_maf_invert(void* stream, const gm_maf_invert_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->u && a->y && a->W2 && a->b2 && a->W1T && a->b1 && a->m_h && a->inv_order && shape_ok(a->D, a->H));
    GM_CHECK_ARG(a->n >= 1 && a->n <= (1ll << 32) && a->ldu >= a->D && a->ldy >= a->D && cap_ok(a->s_cap));
    GM_CHECK_ARG((const float*)a->y != a->u);
    GM_CHECK_ARG(!a->s || (a->lds >= a->D && a->s != a->y && (const float*)a->s != a->u));
    InvP p{a->u, a->ldu, a->y, a->ldy, a->s, a->lds, a->W2, a->b2, a->W1T, a->b1, a->m_h, a->inv_order, a->s_cap, a->n,
           a->D, a->H};
    hipStream_t st = (hipStream_t)stream;
    switch ((a->H + 63) / 64) {
    case 1: invert_launch<1>(st, p); break;
    case 2: invert_launch<2>(st, p); break;
    case 3: invert_launch<3>(st, p); break;
    case 4: invert_launch<4>(st, p); break;
    case 5: invert_launch<5>(st, p); break;
    case 6: invert_launch<6>(st, p); break;
    case 7: invert_launch<7>(st, p); break;
    case 8: invert_launch<8>(st, p); break;
    case 9: invert_launch<9>(st, p); break;
    case 10: invert_launch<10>(st, p); break;
    case 11: invert_launch<11>(st, p); break;
    case 12: invert_launch<12>(st, p); break;
    case 13: invert_launch<13>(st, p); break;
    case 14: invert_launch<14>(st, p); break;
    case 15: invert_launch<15>(st, p); break;
    default: invert_launch<16>(st, p); break;
    }
    GM_LAUNCH_RET();
}
