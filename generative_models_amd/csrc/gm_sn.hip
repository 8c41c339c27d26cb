// Spectrally normalised hinge critic (sngan.py; gm_hip.h): one power-iteration step on W [H, I] in front of every
// critic forward, the hinge head on the normalised w2, and the projections that carry d loss / d Wbar and d loss / d
// w2bar back to the raw weights.  None of it is a GEMM: the hidden layer's products stay gm_gemm.hip's, with Wbar in W's
// place.
//
// gm_sn_power_iter = three launches.
//   wtu:  t = W^T u.  A workgroup owns 16 columns; thread (g, c) walks rows g, g + 16, ... of column c (a wave reads four
//         64-byte row segments per step), the 16 row groups are added in order through LDS.
//   wv:   W v = W t / max(||t||, 1e-12).  t sits in LDS; every workgroup re-derives ||t|| from it; a wave per row.
//   wbar: every workgroup re-derives ||W v||, u' = W v / max(||W v||, 1e-12) and sigma = u' . W v from the H-vector and
//         writes its 8 rows of Wbar = W / sigma; workgroup 0 also writes u (update_u), v, w2bar and the four stats.
// gm_sn_head_fwd = one launch (gm_acgan_heads_fwd's layout: a wave per 2 rows, float4 lanes); the loss slot by the last
//   workgroup to arrive (gm_fused.hip's head_finalize protocol).
// gm_sn_head_bwd = the rows kernel (+ in critic mode a one-workgroup combine: partials in workgroup order, then the
//   projection onto w2's tangent space).
// gm_sn_grad = partials of c = <G, Wbar> per 8 rows, then gW = (G - c u v^T) / sigma.
// Every sum is accumulated in fp64 in a fixed order and rounded once; no floating-point atomics.
#include <math.h>
#include "gm_common.h"

namespace {

constexpr int SN_ROWS = 8;           // rows of W / of the batch per workgroup
constexpr int SN_HDR = 4;            // head workspace header (floats): the forward's arrival counter
constexpr double SN_EPS = 1e-12;

__host__ __device__ inline int64_t sn_align4(int64_t n) { return (n + 3) & ~int64_t(3); }
inline int sn_blocks(int rows) { return (rows + SN_ROWS - 1) / SN_ROWS; }
inline bool sn_w_ok(int H, int I) {
    return H >= 4 && H <= GM_SN_MAX_H && H % 4 == 0 && I >= 1 && I <= GM_SN_MAX_I;
}
inline bool sn_head_ok(int rows, int Hd) {
    return rows >= 1 && rows < (1 << 28) && Hd >= 4 && Hd <= GM_SN_MAX_H && Hd % 4 == 0;
}
inline bool sn_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The sum of one value per thread over the 256-thread workgroup, in a fixed order, on every thread.
__device__ __forceinline__ double sn_block_sum(double v, double* sh) {
    v = gm_wave_sum_d(v);
    __syncthreads();                                    // (sh may still be read from the call before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// ||x|| of x[0 .. n) by the whole workgroup: the same bits in every workgroup and every kernel that asks.
__device__ __forceinline__ double sn_block_norm(const float* x, int n, double* sh) {
    double ss = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) ss = fma((double)x[i], (double)x[i], ss);
    return sqrt(sn_block_sum(ss, sh));
}

struct PowerP {
    const float* W; int H, I;
    float* u; float* v; float* Wbar; const float* w2; float* w2bar; float* stats;
    int update_u;
    float* t; float* r;               // workspace: W^T u [I], W v [H]
};

__global__ __launch_bounds__(256) void sn_wtu_kernel(PowerP p) {
    __shared__ float su[GM_SN_MAX_H];
    __shared__ double part[16][16];
    const int t = threadIdx.x, c = t & 15, g = t >> 4;
    for (int i = t; i < p.H; i += 256) su[i] = p.u[i];
    __syncthreads();
    const int col = blockIdx.x * 16 + c;
    double acc = 0.0;
    if (col < p.I) {
#pragma unroll 4
        for (int r = g; r < p.H; r += 16) acc = fma((double)p.W[(int64_t)r * p.I + col], (double)su[r], acc);
    }
    part[g][c] = acc;
    __syncthreads();
    if (t < 16 && col < p.I) {                          // (c == t here) the row groups in ascending order
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) s += part[k][t];
        p.t[col] = (float)s;
    }
}

__global__ __launch_bounds__(256) void sn_wv_kernel(PowerP p) {
    __shared__ float st[GM_SN_MAX_I];
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, I = p.I;
    for (int i = threadIdx.x; i < I; i += 256) st[i] = p.t[i];
    __syncthreads();
    const double nt = fmax(sn_block_norm(st, I, red), SN_EPS);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int row = blockIdx.x * SN_ROWS + wave * 2 + k;
        if (row >= p.H) break;                          // (wave-uniform)
        const float* w = p.W + (int64_t)row * I;
        double acc = 0.0;
#pragma unroll 4
        for (int i = lane; i < I; i += 64) acc = fma((double)w[i], (double)st[i], acc);
        acc = gm_wave_sum_d(acc);
        if (lane == 0) p.r[row] = (float)(acc / nt);
    }
}

__global__ __launch_bounds__(256) void sn_wbar_kernel(PowerP p) {
    __shared__ float sr[GM_SN_MAX_H];
    __shared__ float su[GM_SN_MAX_H];
    __shared__ double red[4];
    const int t = threadIdx.x, H = p.H, I = p.I;
    for (int i = t; i < H; i += 256) sr[i] = p.r[i];
    __syncthreads();
    const double nr = fmax(sn_block_norm(sr, H, red), SN_EPS);
    double sd = 0.0;
    for (int i = t; i < H; i += 256) {
        const float ui = p.update_u ? (float)((double)sr[i] / nr) : p.u[i];
        su[i] = ui;
        sd = fma((double)ui, (double)sr[i], sd);
    }
    const float sigma = (float)sn_block_sum(sd, red);
    const int r0 = blockIdx.x * SN_ROWS;
    const int nrow = min(SN_ROWS, H - r0);
    const int64_t base = (int64_t)r0 * I;
    for (int e = t; e < nrow * I; e += 256) p.Wbar[base + e] = p.W[base + e] / sigma;
    if (blockIdx.x != 0) return;
    // workgroup 0: the vectors and scalars the rest of the step reads
    const double ntr = sn_block_norm(p.t, I, red);       // (sn_wv_kernel's value: the same sum in the same order)
    const double nt = fmax(ntr, SN_EPS);
    for (int j = t; j < I; j += 256) p.v[j] = (float)((double)p.t[j] / nt);
    const double nw2 = sn_block_norm(p.w2, H, red);
    for (int i = t; i < H; i += 256) {
        p.w2bar[i] = (float)((double)p.w2[i] / nw2);
        if (p.update_u) p.u[i] = su[i];                  // in place: u was last read by sn_wtu_kernel
    }
    if (t == 0) {
        p.stats[GM_SN_STAT_SIGMA] = sigma;
        p.stats[GM_SN_STAT_NW2] = (float)nw2;
        p.stats[GM_SN_STAT_NT] = (float)ntr;
        p.stats[GM_SN_STAT_NR] = (float)nr;
    }
}

// ---- the hinge head ------------------------------------------------------------------------------------------------
struct HeadFwdP {
    const float* H; int64_t ldh;
    int rows, B, Hd, gen_mode;
    const float* w2bar; const float* b2;
    float* s; float* ds;
    float* loss_out; gm_slot loss_slot;
    float inv_b;
    unsigned int* done;
    float* rowterm;                   // [rows]
};

__device__ void sn_finalize(const HeadFwdP& p) {
    __shared__ int is_last;
    __shared__ double red[4];
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int prev = __hip_atomic_fetch_add(p.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (prev == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    double sl = 0.0;
    for (int m = threadIdx.x; m < p.rows; m += 256)
        sl += (double)__hip_atomic_load(p.rowterm + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sl = gm_wave_sum_d(sl);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double tot = ((red[0] + red[1]) + red[2]) + red[3];
        p.loss_out[gm_slot_index(p.loss_slot)] = (float)(tot * (double)p.inv_b);
        __hip_atomic_store(p.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void sn_head_fwd_kernel(HeadFwdP p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Hd = p.Hd;
    const float b2 = p.b2[0];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int m = blockIdx.x * SN_ROWS + wave * 2 + k;
        if (m >= p.rows) break;                         // (wave-uniform)
        const float* h = p.H + (int64_t)m * p.ldh;
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * lane + 256 * j;
            if (col < Hd) {
                const float4 hv = *(const float4*)(h + col);
                const float4 wv = *(const float4*)(p.w2bar + col);
                acc = fma((double)wv.x, (double)hv.x, acc);
                acc = fma((double)wv.y, (double)hv.y, acc);
                acc = fma((double)wv.z, (double)hv.z, acc);
                acc = fma((double)wv.w, (double)hv.w, acc);
            }
        }
        acc = gm_wave_sum_d(acc);
        if (lane == 0) {
            const float s = (float)acc + b2;
            float term, d;
            if (p.gen_mode) { term = -s; d = -p.inv_b; }
            else if (m < p.B) { const float a = 1.f - s; term = fmaxf(a, 0.f); d = a > 0.f ? -p.inv_b : 0.f; }
            else { const float a = 1.f + s; term = fmaxf(a, 0.f); d = a > 0.f ? p.inv_b : 0.f; }
            p.s[m] = s;
            p.ds[m] = d;
            p.rowterm[m] = term;
        }
    }
    if (p.loss_out) sn_finalize(p);                     // (kernel-argument uniform)
}

struct HeadBwdP {
    const float* H; int64_t ldh;
    int rows, Hd, grads, nblk;
    const float* w2bar; const float* ds;
    float* dPre; int64_t ldp;
    float* part; int64_t P4;          // [nblk][P4]: g[0 .. Hd), gb2 at Hd
    const float* stats; float* gw2; float* gb2;
};

__global__ __launch_bounds__(256) void sn_head_bwd_kernel(HeadBwdP p) {
    __shared__ float sds[SN_ROWS];
    const int t = threadIdx.x, Hd = p.Hd;
    const int m0 = blockIdx.x * SN_ROWS;
    if (t < SN_ROWS) sds[t] = (m0 + t < p.rows) ? p.ds[m0 + t] : 0.f;
    __syncthreads();
    float* part = p.part + (int64_t)blockIdx.x * p.P4;
    for (int n = t; n < Hd; n += 256) {
        const float wn = p.w2bar[n];
        float g = 0.f;
#pragma unroll
        for (int r = 0; r < SN_ROWS; ++r) {
            if (m0 + r < p.rows) {
                const float hv = p.H[(int64_t)(m0 + r) * p.ldh + n];
                g = fmaf(sds[r], hv, g);
                p.dPre[(int64_t)(m0 + r) * p.ldp + n] = hv > 0.f ? sds[r] * wn : 0.f;
            }
        }
        if (p.grads) part[n] = g;
    }
    if (p.grads && t == 0) {
        float s = 0.f;
        for (int r = 0; r < SN_ROWS; ++r) s += sds[r];
        part[Hd] = s;
    }
}

// One workgroup: thread t owns columns t + 256 j of w2.
__global__ __launch_bounds__(256) void sn_head_combine_kernel(HeadBwdP p) {
    __shared__ double red[4];
    const int t = threadIdx.x, Hd = p.Hd;
    double g[GM_SN_MAX_H / 256];
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < GM_SN_MAX_H / 256; ++j) {
        const int n = t + 256 * j;
        g[j] = 0.0;
        if (n < Hd) {
            for (int w = 0; w < p.nblk; ++w) g[j] += (double)p.part[(int64_t)w * p.P4 + n];
            dot = fma(g[j], (double)p.w2bar[n], dot);
        }
    }
    dot = sn_block_sum(dot, red);
    const double nw2 = (double)p.stats[GM_SN_STAT_NW2];
#pragma unroll
    for (int j = 0; j < GM_SN_MAX_H / 256; ++j) {
        const int n = t + 256 * j;
        if (n < Hd) p.gw2[n] = (float)((g[j] - dot * (double)p.w2bar[n]) / nw2);
    }
    if (t == 0) {
        double gb = 0.0;
        for (int w = 0; w < p.nblk; ++w) gb += (double)p.part[(int64_t)w * p.P4 + Hd];
        p.gb2[0] = (float)gb;
    }
}

// ---- the weight gradient's projection -------------------------------------------------------------------------------
struct GradP {
    const float* G; const float* Wbar; int H, I, nblk;
    const float* u; const float* v; const float* stats;
    float* gW; double* part;          // [nblk]
};

__global__ __launch_bounds__(256) void sn_grad_dot_kernel(GradP p) {
    __shared__ double red[4];
    const int r0 = blockIdx.x * SN_ROWS;
    const int nrow = min(SN_ROWS, p.H - r0);
    const int64_t base = (int64_t)r0 * p.I;
    double acc = 0.0;
#pragma unroll 4
    for (int e = threadIdx.x; e < nrow * p.I; e += 256) acc = fma((double)p.G[base + e], (double)p.Wbar[base + e], acc);
    acc = sn_block_sum(acc, red);
    if (threadIdx.x == 0) p.part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void sn_grad_apply_kernel(GradP p) {
    double c = 0.0;
    for (int w = 0; w < p.nblk; ++w) c += p.part[w];    // every thread of every workgroup: the same order
    const double sigma = (double)p.stats[GM_SN_STAT_SIGMA];
    const int r0 = blockIdx.x * SN_ROWS;
    const int nrow = min(SN_ROWS, p.H - r0);
    for (int r = 0; r < nrow; ++r) {
        const double cu = c * (double)p.u[r0 + r];
        const int64_t base = (int64_t)(r0 + r) * p.I;
        for (int j = threadIdx.x; j < p.I; j += 256)
            p.gW[base + j] = (float)(((double)p.G[base + j] - cu * (double)p.v[j]) / sigma);
    }
}

int sn_head_check(const gm_sn_head_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(sn_head_ok(a->rows, a->Hd));
    GM_CHECK_ARG(a->B >= 1 && (a->gen_mode ? a->rows == a->B : a->rows == 2 * a->B));
    GM_CHECK_ARG(a->H && a->ldh >= a->Hd && a->ldh % 4 == 0 && sn_aligned16(a->H));
    GM_CHECK_ARG(a->w2bar && sn_aligned16(a->w2bar) && a->ds);
    GM_CHECK_ARG(a->ws && sn_aligned16(a->ws) && a->ws_bytes >= gm_sn_head_workspace_bytes(a->rows, a->Hd));
    return 0;
}

}  // namespace

extern "C" int64_t gm_sn_power_workspace_bytes(int H, int I) {
    if (!sn_w_ok(H, I)) return -1;
    return 4 * (sn_align4(I) + sn_align4(H));
}

extern "C" int gm_sn_power_iter(void* stream, const gm_sn_power_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(sn_w_ok(a->H, a->I));
    GM_CHECK_ARG(a->W && a->u && a->v && a->Wbar && a->w2 && a->w2bar && a->stats);
    GM_CHECK_ARG((const float*)a->Wbar != a->W && (const float*)a->w2bar != a->w2);
    GM_CHECK_ARG(a->ws && sn_aligned16(a->ws) && a->ws_bytes >= gm_sn_power_workspace_bytes(a->H, a->I));
    PowerP p{a->W, a->H, a->I, a->u, a->v, a->Wbar, a->w2, a->w2bar, a->stats, a->update_u ? 1 : 0,
             a->ws, a->ws + sn_align4(a->I)};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sn_wtu_kernel, dim3((a->I + 15) / 16), dim3(256), 0, s, p);
    hipLaunchKernelGGL(sn_wv_kernel, dim3(sn_blocks(a->H)), dim3(256), 0, s, p);
    hipLaunchKernelGGL(sn_wbar_kernel, dim3(sn_blocks(a->H)), dim3(256), 0, s, p);
    GM_LAUNCH_RET();
}

extern "C" int64_t gm_sn_head_workspace_bytes(int rows, int Hd) {
    if (!sn_head_ok(rows, Hd)) return -1;
    return 4 * (SN_HDR + sn_align4(rows) + (int64_t)sn_blocks(rows) * sn_align4(Hd + 1));
}

extern "C" int gm_sn_head_fwd(void* stream, const gm_sn_head_args* a) {
    const int rc = sn_head_check(a);
    if (rc) return rc;
    GM_CHECK_ARG(a->b2 && a->s);
    HeadFwdP p{a->H, a->ldh, a->rows, a->B, a->Hd, a->gen_mode ? 1 : 0, a->w2bar, a->b2, a->s, a->ds,
               a->loss_out, a->loss_slot, 1.f / (float)a->B, (unsigned int*)a->ws, a->ws + SN_HDR};
    hipLaunchKernelGGL(sn_head_fwd_kernel, dim3(sn_blocks(a->rows)), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_sn_head_bwd(void* stream, const gm_sn_head_args* a) {
    const int rc = sn_head_check(a);
    if (rc) return rc;
    GM_CHECK_ARG(a->dPre && a->ldp >= a->Hd && (const float*)a->dPre != a->H);
    const bool grads = a->gw2 || a->gb2;
    if (a->gen_mode) GM_CHECK_ARG(!grads);              // the critic is frozen in the generator step
    else GM_CHECK_ARG(a->gw2 && a->gb2 && a->stats);
    HeadBwdP p{a->H, a->ldh, a->rows, a->Hd, grads ? 1 : 0, sn_blocks(a->rows), a->w2bar, a->ds, a->dPre, a->ldp,
               a->ws + SN_HDR + sn_align4(a->rows), sn_align4(a->Hd + 1), a->stats, a->gw2, a->gb2};
    hipLaunchKernelGGL(sn_head_bwd_kernel, dim3(p.nblk), dim3(256), 0, (hipStream_t)stream, p);
    if (grads) hipLaunchKernelGGL(sn_head_combine_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int64_t gm_sn_grad_workspace_bytes(int H) {
    if (!sn_w_ok(H, 1)) return -1;
    return 8 * sn_align4(sn_blocks(H));
}

extern "C" int gm_sn_grad(void* stream, const gm_sn_grad_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(sn_w_ok(a->H, a->I));
    GM_CHECK_ARG(a->G && a->Wbar && a->u && a->v && a->stats && a->gW);
    GM_CHECK_ARG((const float*)a->gW != a->Wbar);
    GM_CHECK_ARG(a->ws && sn_aligned16(a->ws) && a->ws_bytes >= gm_sn_grad_workspace_bytes(a->H));
    GradP p{a->G, a->Wbar, a->H, a->I, sn_blocks(a->H), a->u, a->v, a->stats, a->gW, (double*)a->ws};
    hipLaunchKernelGGL(sn_grad_dot_kernel, dim3(p.nblk), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(sn_grad_apply_kernel, dim3(p.nblk), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
