// Vector quantisation of the VQ-VAE (vqvae.py holds the contract; gm_hip.h).  N variables of D
// floats per row against a codebook E [K, D].
//
// gm_vq_quantise: one wave per row, four rows per workgroup pass, the codebook in LDS (filled once per workgroup; the
//   workgroup then walks its rows).  A wave's 64 lanes are Gv variable slots x Gk shares of the K codes (Gv = the power of
//   two >= N, at most 64; Gk = 64 / Gv): a lane holds its variable's D floats in registers and walks the codes k = q, q +
//   Gk, ... ascending, every distance the direct sum_d (z_d - E_kd)^2 over d ascending (pinned fused multiply-adds), the
//   strict `<` keeping the lowest index; the Gk shares meet in a butterfly that prefers the smaller distance and, at equal
//   distances, the lower index.  No distance comparing less (NaN) leaves the sentinel K, which becomes code 0: an index
//   >= K is never written or read.  qerr is the direct distance to the winner, summed over a lane's variables ascending
//   and over the wave by a fixed butterfly: a row's outputs do not depend on where the row lands.
// gm_vq_reduce: one thread per element; nothing crosses lanes.
// gm_vq_step: one 256-thread workgroup per code.  Wave w scans quarter w of the B N codes 64 at a time (four loads in
//   flight), a ballot names the matches, and lane d < D adds z_e[pair, d] for the matching pairs in ascending order (four
//   independent loads ahead of four ordered adds).  The four waves' sums are combined ((0 + 1) + 2) + 3 through LDS; then
//   the gradient 2 (n_k E_k - s_k) and gm_adam's step.  The order depends on (B, N) alone.
// No floating-point atomics anywhere; the same bits on every run, graph or eager.
#include "gm_common.h"

namespace {

struct VqP {
    const float* ze; int64_t ldz;
    const float* E; int64_t lde;
    int32_t* codes; int64_t ldc;
    float* zq; int64_t ldq;
    float* qerr; float* lp;
    const float* dz; int64_t lddz;
    const float* wn;
    float* dml; int64_t lddml;
    float beta;
    int B, N, D, K, kshift;
};

// sum_d (z_d - e_d)^2 over d ascending, DV4 groups of four of which the first D / 4 are live.
template <int DV4>
__device__ __forceinline__ float vq_dist(const float (&z)[4 * DV4], const float* e, int D) {
#pragma clang fp contract(off)
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < DV4; ++i) {
        if (4 * i < D) {
            const float4 v = reinterpret_cast<const float4*>(e)[i];
            const float d0 = z[4 * i] - v.x, d1 = z[4 * i + 1] - v.y, d2 = z[4 * i + 2] - v.z, d3 = z[4 * i + 3] - v.w;
            acc = __builtin_fmaf(d0, d0, acc);
            acc = __builtin_fmaf(d1, d1, acc);
            acc = __builtin_fmaf(d2, d2, acc);
            acc = __builtin_fmaf(d3, d3, acc);
        }
    }
    return acc;
}

// EXACT: D = 4 DV4 at compile time (4, 8, 16, 32, 64); otherwise D <= 4 DV4 is read from the arguments and the groups of
// four past it are skipped.
template <int DV4, bool EXACT>
__global__ __launch_bounds__(256) void vq_quantise_kernel(VqP p) {
    extern __shared__ __attribute__((aligned(16))) char vq_smem[];
    float* sE = reinterpret_cast<float*>(vq_smem);               // [K, D], rows D floats apart (D % 4 == 0)
    const int tid = threadIdx.x, D = EXACT ? 4 * DV4 : p.D, K = p.K, N = p.N;
    for (int i = tid; i < K * D; i += 256) {
        const int k = i / D, d = i - k * D;
        sE[i] = p.E[(int64_t)k * p.lde + d];
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int Gk = 1 << p.kshift, Gv = 64 >> p.kshift;
    const int qk = lane & (Gk - 1), vs = lane >> p.kshift;
    for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < p.B; r0 += (int64_t)gridDim.x * 4) {
        const int64_t r = r0 + wave;
        const bool on = r < p.B;
        const int64_t rr = on ? r : (int64_t)p.B - 1;            // waves past the end redo the last row and store nothing
        const float* zrow = p.ze + rr * p.ldz;
        float acc = 0.f;
        for (int v0 = 0; v0 < N; v0 += Gv) {                     // the same trip count in every lane: shuffles below
            const int v = v0 + vs;
            const bool live = v < N;
            const float* zp = zrow + (int64_t)min(v, N - 1) * D;
            float z[4 * DV4];
#pragma unroll
            for (int i = 0; i < 4 * DV4; ++i) z[i] = i < D ? zp[i] : 0.f;
            float best = INFINITY;
            int bi = K;                                          // the sentinel: nothing compared less yet
            for (int k = qk; k < K; k += Gk) {
                const float d = vq_dist<DV4>(z, sE + k * D, D);
                if (d < best) {
                    best = d;
                    bi = k;
                }
            }
            for (int o = Gk >> 1; o > 0; o >>= 1) {              // the variable's Gk adjacent lanes
                const float od = __shfl_xor(best, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (od < best || (od == best && oi < bi)) {
                    best = od;
                    bi = oi;
                }
            }
            const int code = bi < K ? bi : 0;
            const float* ec = sE + code * D;
            const float e = vq_dist<DV4>(z, ec, D);              // the direct differences against the winner
            if (live && qk == 0) acc += e;
            if (on && live) {
                float* qo = p.zq + r * p.ldq + (int64_t)v * D;
                for (int d = qk; d < D; d += Gk) qo[d] = ec[d];
                if (qk == 0) p.codes[r * p.ldc + v] = code;
            }
        }
        acc = gm_wave_sum(acc);
        if (on && lane == 0) {
#pragma clang fp contract(off)
            p.qerr[r] = acc;
            p.lp[r] = -((1.f + p.beta) * acc);
        }
    }
}

__global__ __launch_bounds__(256) void vq_reduce_kernel(VqP p) {
#pragma clang fp contract(off)
    const int W = p.N * p.D;
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= (int64_t)p.B * W) return;
    const int64_t b = gi / W;
    const int e = (int)(gi - b * W), n = e / p.D, d = e - n * p.D;
    const int c = min(max(p.codes[b * p.ldc + n], 0), p.K - 1);
    const float t = p.ze[b * p.ldz + e] - p.E[(int64_t)c * p.lde + d];
    const float u = ((2.f * p.beta) * p.wn[b]) * t;
    p.dml[b * p.lddml + e] = p.dz[b * p.lddz + e] + u;
}

struct VqStepP {
    const float* ze; int64_t ldz;
    const int32_t* codes; int64_t ldc;
    float* E; float* m; float* v; float* grad;
    int32_t* nk; int32_t* usage;
    const float* sched; gm_slot slot;
    float omb1, b2, omb2, eps, wd;
    int B, N, D, K;
};

__global__ __launch_bounds__(256) void vq_step_kernel(VqStepP p) {
    __shared__ float sS[4][64];
    __shared__ int sN[4];
    const int k = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned N = (unsigned)p.N, P = (unsigned)p.B * N;     // B N < 2^31 (checked on the host)
    const unsigned Q = ((P + 255u) / 256u) * 64u;                // a wave's share: a multiple of 64
    const unsigned lo = min((unsigned)wave * Q, P), hi = min(lo + Q, P);
    const bool dense = p.ldc == (int64_t)N;
    float s = 0.f;
    int n = 0;
    for (unsigned base = lo; base < hi; base += 256u) {
        int c[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned q = base + 64u * u + lane;
            c[u] = -1;
            if (q < hi) {
                const unsigned b = q / N;
                c[u] = dense ? p.codes[q] : p.codes[(int64_t)b * p.ldc + (q - b * N)];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            unsigned long long mask = __ballot(c[u] == k);
            n += __popcll(mask);
            while (mask) {                                       // the wave's matches, ascending, four loads ahead
                float x[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    x[j] = 0.f;                                  // s + 0 = s: a short group changes nothing
                    if (mask) {
                        const unsigned q = base + 64u * u + (unsigned)__builtin_ctzll(mask);
                        mask &= mask - 1;
                        const unsigned b = q / N;
                        if (lane < p.D) x[j] = p.ze[(int64_t)b * p.ldz + (int64_t)(q - b * N) * p.D + lane];
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) s += x[j];
            }
        }
    }
    sS[wave][lane] = s;
    if (lane == 0) sN[wave] = n;
    __syncthreads();
    if (wave != 0) return;
    const int nt = sN[0] + sN[1] + sN[2] + sN[3];
    if (lane < p.D) {
#pragma clang fp contract(off)
        const float st = ((sS[0][lane] + sS[1][lane]) + sS[2][lane]) + sS[3][lane];
        const int o = k * p.D + lane;
        const float t = (float)nt * p.E[o];
        const float g = 2.f * (t - st);
        if (p.grad) p.grad[o] = g;
        if (p.sched) {
            const int64_t si = gm_slot_index(p.slot);
            adam_update(p.E[o], g, p.m[o], p.v[o], p.sched[2 * si], p.sched[2 * si + 1], p.omb1, p.b2, p.omb2, p.eps,
                        p.wd, 0.f);
        }
    }
    if (lane == 0) {
        if (p.nk) p.nk[k] = nt;
        if (p.usage) p.usage[k] += nt;
    }
}

inline int vq_shape_ok(int B, int N, int D, int K) {
    GM_CHECK_ARG(B >= 1 && N >= 1 && D >= GM_VQ_MIN_D && D <= GM_VQ_MAX_D && D % 4 == 0);
    GM_CHECK_ARG((int64_t)N * D <= GM_VQ_MAX_ND && K >= GM_VQ_MIN_K && K <= GM_VQ_MAX_K &&
                 (int64_t)K * D <= GM_VQ_MAX_KD);
    GM_CHECK_ARG((int64_t)B * N < (1ll << 31));
    return 0;
}

inline int vq_fill(const gm_vq_args* a, VqP* p) {
    GM_CHECK_ARG(a != nullptr);
    int rc = vq_shape_ok(a->B, a->N, a->D, a->K);
    if (rc) return rc;
    const int W = a->N * a->D;
    GM_CHECK_ARG(a->ze && a->E && a->codes && a->ldz >= W && a->lde >= a->D && a->ldc >= a->N);
    GM_CHECK_ARG(a->beta >= 0.f && a->beta < INFINITY);
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(a->ze) & 3) == 0 && (reinterpret_cast<uintptr_t>(a->E) & 3) == 0);
    p->ze = a->ze; p->ldz = a->ldz; p->E = a->E; p->lde = a->lde; p->codes = a->codes; p->ldc = a->ldc;
    p->beta = a->beta; p->B = a->B; p->N = a->N; p->D = a->D; p->K = a->K;
    return 0;
}

}  // namespace

extern "C" int gm_vq_quantise(void* stream, const gm_vq_args* a) {
    VqP p{};
    int rc = vq_fill(a, &p);
    if (rc) return rc;
    GM_CHECK_ARG(a->zq && a->qerr && a->lp && a->ldq >= a->N * a->D);
    const void* in[] = {a->ze, a->E};
    const void* out[] = {a->zq, a->qerr, a->lp, a->codes};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 2; ++j) GM_CHECK_ARG(out[i] != in[j]);
        for (int j = i + 1; j < 4; ++j) GM_CHECK_ARG(out[i] != out[j]);
    }
    p.zq = a->zq; p.ldq = a->ldq; p.qerr = a->qerr; p.lp = a->lp;
    int gv = 1;
    while (gv < a->N && gv < 64) gv <<= 1;
    p.kshift = 0;
    while ((gv << p.kshift) < 64) ++p.kshift;
    const int64_t blocks = ((int64_t)a->B + 3) / 4;
    const unsigned grid = (unsigned)(blocks < 1024 ? blocks : 1024);
    const size_t lds = (size_t)a->K * a->D * sizeof(float);
#define VQ_LAUNCH(DV4, EXACT) \
    hipLaunchKernelGGL((vq_quantise_kernel<DV4, EXACT>), dim3(grid), dim3(256), lds, (hipStream_t)stream, p)
    switch (a->D) {
    case 4: VQ_LAUNCH(1, true); break;
    case 8: VQ_LAUNCH(2, true); break;
    case 16: VQ_LAUNCH(4, true); break;
    case 32: VQ_LAUNCH(8, true); break;
    case 64: VQ_LAUNCH(16, true); break;
    default:
        if (a->D < 16)
            VQ_LAUNCH(4, false);
        else
            VQ_LAUNCH(16, false);
    }
#undef VQ_LAUNCH
    GM_LAUNCH_RET();
}

extern "C" int gm_vq_reduce(void* stream, const gm_vq_args* a) {
    VqP p{};
    int rc = vq_fill(a, &p);
    if (rc) return rc;
    const int W = a->N * a->D;
    GM_CHECK_ARG(a->dzdec && a->wn && a->dml && a->lddz >= W && a->lddml >= W);
    const void* in[] = {a->ze, a->E, a->codes, a->wn};
    for (int j = 0; j < 4; ++j) GM_CHECK_ARG((const void*)a->dml != in[j]);
    p.dz = a->dzdec; p.lddz = a->lddz; p.wn = a->wn; p.dml = a->dml; p.lddml = a->lddml;
    const int64_t blocks = ((int64_t)a->B * W + 255) / 256;
    GM_CHECK_ARG(blocks < (1ll << 31));
    hipLaunchKernelGGL(vq_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_vq_step(void* stream, const gm_vq_step_args* a) {
    GM_CHECK_ARG(a != nullptr);
    int rc = vq_shape_ok(a->B, a->N, a->D, a->K);
    if (rc) return rc;
    GM_CHECK_ARG(a->ze && a->codes && a->E && a->ldz >= a->N * a->D && a->ldc >= a->N);
    GM_CHECK_ARG(!a->sched || (a->m && a->v));
    GM_CHECK_ARG(a->sched || a->grad || a->nk || a->usage);      // something to write
    const void* ptr[] = {a->ze, a->codes, a->E, a->m, a->v, a->grad, a->nk, a->usage, a->sched};
    for (int i = 0; i < 9; ++i)
        for (int j = i + 1; j < 9; ++j) GM_CHECK_ARG(!ptr[i] || ptr[i] != ptr[j]);
    VqStepP p{a->ze, a->ldz, a->codes, a->ldc, a->E, a->m, a->v, a->grad, a->nk, a->usage, a->sched, a->sched_slot,
              (float)(1.0 - a->beta1), (float)a->beta2, (float)(1.0 - a->beta2), (float)a->eps, (float)a->weight_decay,
              a->B, a->N, a->D, a->K};
    hipLaunchKernelGGL(vq_step_kernel, dim3((unsigned)a->K), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
