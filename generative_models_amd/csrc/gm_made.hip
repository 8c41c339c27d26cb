// Masked autoregressive model, MADE (made.py; gm_hip.h; the sampling rule in gm_made.h).
//
// gm_made_bce: the Bernoulli-logit loss of one batch, one 256-thread workgroup per row: the row's sum of softplus(a) -
//   x a (per thread over its quads in order, the wave butterfly, the four waves in order) and, when asked, dA =
//   (sigmoid(a) - x) scale.  16-byte accesses where the rows allow them, element by element otherwise.
// gm_made_mask: zeroes W and Adam's two moments at the masked entries of both layers, the masks from the degree vectors;
//   it reads no weight and writes masked entries only.
// gm_made_sample: the ancestral sampler in one launch.  One wave per row, four rows per workgroup, no LDS, no barrier.
//   A lane keeps the pre-activations h_k of k = 64 j + lane in NJ = ceil(H / 64) registers (compile-time indices: no
//   scratch).  Pixels go in order of degree, 64 positions at a time: each lane first fetches everything position
//   c0 + lane needs that does not depend on the chain -- the pixel index, its uniform, its output bias, its given value
//   -- then the 64 steps run with wave-uniform lane reads.  A step: the logit (lane-local sum in ascending k, the wave
//   butterfly, the bias), the decision, h += x W1T[d, :].  Both weight rows of the next position are loaded before the
//   current one is reduced.  The position t has degree t + 1, so the masks are (m_h <= t) and (m_h > t).
// gm_made_uniform: the rule's uniforms as a matrix, for the sampler that runs through I forward passes.
// No floating-point atomics, fixed reduction orders: the same bits on every run, whatever n and the grid.
#include "gm_made.h"

namespace {

struct BceP {
    const float* a; int64_t lda; const float* x; int64_t ldx;
    float* dA; int64_t ldd; float* part; float scale; int I, vec;
};

__device__ __forceinline__ float bce_term(float a, float x, float scale, float& g) {
    g = (made_prob(a) - x) * scale;
    return (fmaxf(a, 0.f) + log1pf(expf(-fabsf(a)))) - x * a;
}

__global__ __launch_bounds__(256) void made_bce_kernel(BceP p) {
    __shared__ float sh[4];
    const int64_t b = blockIdx.x;
    const float* a = p.a + b * p.lda;
    const float* x = p.x + b * p.ldx;
    float* dA = p.dA ? p.dA + b * p.ldd : nullptr;
    float acc = 0.f;
    if (p.vec) {
        for (int q = threadIdx.x; q < (p.I >> 2); q += 256) {
            const float4 av = reinterpret_cast<const float4*>(a)[q], xv = reinterpret_cast<const float4*>(x)[q];
            float4 g;
            acc += bce_term(av.x, xv.x, p.scale, g.x);
            acc += bce_term(av.y, xv.y, p.scale, g.y);
            acc += bce_term(av.z, xv.z, p.scale, g.z);
            acc += bce_term(av.w, xv.w, p.scale, g.w);
            if (dA) reinterpret_cast<float4*>(dA)[q] = g;
        }
    } else {
        for (int i = threadIdx.x; i < p.I; i += 256) {
            float g;
            acc += bce_term(a[i], x[i], p.scale, g);
            if (dA) dA[i] = g;
        }
    }
    acc = gm_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) p.part[b] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

struct MaskP {
    float* W1; float* m1; float* v1; float* W2; float* m2; float* v2;
    const int* m_in; const int* m_h; int I, H;
};

__global__ __launch_bounds__(256) void made_mask_kernel(MaskP p) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= p.I * p.H) return;
    if (p.m_h[t / p.I] < p.m_in[t % p.I]) {            // linear.weight [H, I]: M1[k, i] = (m_h[k] >= m_in[i])
        p.W1[t] = 0.f;
        if (p.m1) { p.m1[t] = 0.f; p.v1[t] = 0.f; }
    }
    if (p.m_in[t / p.H] <= p.m_h[t % p.H]) {           // out.weight [I, H]: M2[d, k] = (m_in[d] > m_h[k])
        p.W2[t] = 0.f;
        if (p.m2) { p.m2[t] = 0.f; p.v2[t] = 0.f; }
    }
}

struct SampP {
    const float* W2; const float* b2; const float* W1T; const float* b1;
    const int* m_h; const int* inv_order;
    float* x; int64_t ldx; float* p; int64_t ldp; const float* given; int64_t ldg;
    uint64_t seed; int64_t n; int I, H, n_known;
};

constexpr int MADE_NO_UNIT = 0x7fffffff;               // degree of the lanes past H: in neither mask

__device__ __forceinline__ int lane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ float lane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// The two weight rows of pixel d at position t (degree t + 1): out.weight's where m_h <= t, W1T's where m_h > t.
template <int NJ>
__device__ __forceinline__ void made_rows(const SampP& q, const int (&mh)[NJ], int lane, int d, int t, float (&w2)[NJ],
                                          float (&w1)[NJ]) {
    const float* r2 = q.W2 + (int64_t)d * q.H + lane;
    const float* r1 = q.W1T + (int64_t)d * q.H + lane;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        w2[j] = mh[j] <= t ? r2[j * 64] : 0.f;
        w1[j] = (mh[j] > t && mh[j] != MADE_NO_UNIT) ? r1[j * 64] : 0.f;
    }
}

template <int NJ>
__global__ __launch_bounds__(256) void made_sample_kernel(SampP q) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= q.n) return;                              // a whole wave: the kernel has no barrier
    float h[NJ];
    int mh[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int k = j * 64 + lane;
        h[j] = k < q.H ? q.b1[k] : 0.f;
        mh[j] = k < q.H ? q.m_h[k] : MADE_NO_UNIT;
    }
    for (int c0 = 0; c0 < q.I; c0 += 64) {
        const int tl = c0 + lane;
        int dl = 0;
        float ul = 0.f, bl = 0.f, gl = 0.f;
        if (tl < q.I) {
            dl = min(max(q.inv_order[tl], 0), q.I - 1);   // never read outside a row, whatever the table holds
            ul = ph_uniform(q.seed, (uint32_t)dl, 0u, (uint32_t)r, GM_MADE_TAG_S);
            bl = q.b2[dl];
            if (tl < q.n_known) gl = q.given[r * q.ldg + dl];
        }
        float xl = 0.f, pl = 0.f;
        const int cnt = min(64, q.I - c0);
        float w2c[NJ], w1c[NJ];
        made_rows<NJ>(q, mh, lane, lane_i(dl, 0), c0, w2c, w1c);
        for (int s = 0; s < cnt; ++s) {
            const int t = c0 + s;
            float w2n[NJ], w1n[NJ];
            const int sn = min(s + 1, cnt - 1);        // (the chunk's last step reloads its own rows: unused)
            made_rows<NJ>(q, mh, lane, lane_i(dl, sn), c0 + sn, w2n, w1n);
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc = fmaf(w2c[j], fmaxf(h[j], 0.f), acc);
            const float a = gm_wave_sum(acc) + lane_f(bl, s);
            const float pv = made_prob(a);
            const float xv = t < q.n_known ? lane_f(gl, s) : (lane_f(ul, s) < pv ? 1.f : 0.f);
            if (xv != 0.f) {
#pragma unroll
                for (int j = 0; j < NJ; ++j) h[j] = fmaf(xv, w1c[j], h[j]);
            }
            if (lane == s) { xl = xv; pl = pv; }
#pragma unroll
            for (int j = 0; j < NJ; ++j) { w2c[j] = w2n[j]; w1c[j] = w1n[j]; }
        }
        if (tl < q.I) {
            q.x[r * q.ldx + dl] = xl;
            if (q.p) q.p[r * q.ldp + dl] = pl;
        }
    }
}

struct UniP { float* u; int64_t ldu; uint64_t seed; int64_t row0; int I; };

__global__ __launch_bounds__(256) void made_uniform_kernel(UniP p) {
    const int64_t b = blockIdx.x;
    for (int d = threadIdx.x; d < p.I; d += 256)
        p.u[b * p.ldu + d] = ph_uniform(p.seed, (uint32_t)d, 0u, (uint32_t)(p.row0 + b), GM_MADE_TAG_S);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool shape_ok(int I, int H) {
    return I >= GM_MADE_MIN_I && I <= GM_MADE_MAX_I && H >= 1 && H <= GM_MADE_MAX_H;
}

template <int NJ>
void sample_launch(hipStream_t st, const SampP& p) {
    hipLaunchKernelGGL(made_sample_kernel<NJ>, dim3((unsigned)((p.n + 3) / 4)), dim3(256), 0, st, p);
}

}  // namespace

extern "C" int gm_made_bce(void* stream, const float* logits, int64_t lda, const float* x, int64_t ldx, float* dA,
                           int64_t ldd, float* part, float scale, int B, int I) {
    GM_CHECK_ARG(logits && x && part && B >= 1 && I >= 1 && I <= GM_MADE_MAX_I && lda >= I && ldx >= I);
    GM_CHECK_ARG(!dA || (ldd >= I && (const float*)dA != x));
    GM_CHECK_ARG(__builtin_isfinite(scale) && scale >= 0.f);
    const int vec = (I % 4 == 0 && lda % 4 == 0 && ldx % 4 == 0 && al16(logits) && al16(x) &&
                     (!dA || (ldd % 4 == 0 && al16(dA)))) ? 1 : 0;
    BceP p{logits, lda, x, ldx, dA, ldd, part, scale, I, vec};
    hipLaunchKernelGGL(made_bce_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_made_mask(void* stream, const gm_made_mask_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->W1 && a->W2 && a->m_in && a->m_h && shape_ok(a->I, a->H) && a->W1 != a->W2);
    GM_CHECK_ARG((a->m1 != nullptr) == (a->v1 != nullptr) && (a->m2 != nullptr) == (a->v2 != nullptr));
    MaskP p{a->W1, a->m1, a->v1, a->W2, a->m2, a->v2, a->m_in, a->m_h, a->I, a->H};
    hipLaunchKernelGGL(made_mask_kernel, dim3((unsigned)((a->I * a->H + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_made_sample(void* stream, const gm_made_sample_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->W2 && a->b2 && a->W1T && a->b1 && a->m_h && a->inv_order && a->x && shape_ok(a->I, a->H));
    GM_CHECK_ARG(a->n >= 1 && a->n <= (1ll << 32) && a->ldx >= a->I && (!a->p || (a->ldp >= a->I && a->p != a->x)));
    GM_CHECK_ARG(a->n_known >= 0 && a->n_known <= a->I);
    GM_CHECK_ARG(a->n_known == 0 || (a->given && a->ldg >= a->I && a->given != (const float*)a->x &&
                                     a->given != (const float*)a->p));
    SampP p{a->W2, a->b2, a->W1T, a->b1, a->m_h, a->inv_order, a->x, a->ldx, a->p, a->ldp, a->given, a->ldg,
            a->seed, a->n, a->I, a->H, a->n_known};
    hipStream_t st = (hipStream_t)stream;
    switch ((a->H + 63) / 64) {
    case 1: sample_launch<1>(st, p); break;
    case 2: sample_launch<2>(st, p); break;
    case 3: sample_launch<3>(st, p); break;
    case 4: sample_launch<4>(st, p); break;
    case 5: sample_launch<5>(st, p); break;
    case 6: sample_launch<6>(st, p); break;
    case 7: sample_launch<7>(st, p); break;
    case 8: sample_launch<8>(st, p); break;
    case 9: sample_launch<9>(st, p); break;
    case 10: sample_launch<10>(st, p); break;
    case 11: sample_launch<11>(st, p); break;
    case 12: sample_launch<12>(st, p); break;
    case 13: sample_launch<13>(st, p); break;
    case 14: sample_launch<14>(st, p); break;
    case 15: sample_launch<15>(st, p); break;
    default: sample_launch<16>(st, p); break;
    }
    GM_LAUNCH_RET();
}

extern "C" int gm_made_uniform(void* stream, float* u, int64_t ldu, uint64_t seed, int64_t row0, int64_t rows, int I) {
    GM_CHECK_ARG(u && I >= 1 && I <= GM_MADE_MAX_I && ldu >= I && rows >= 1 && rows < (1ll << 31) && row0 >= 0 &&
                 row0 + rows <= (1ll << 32));
    UniP p{u, ldu, seed, row0, I};
    hipLaunchKernelGGL(made_uniform_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
