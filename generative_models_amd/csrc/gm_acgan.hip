// Auxiliary-classifier GAN's two critic heads (acgan.py; gm_hip.h): on the shared hidden rows H [rows, Hd] the source
// head sigmoid(w2 . h + b2) with ns_gan.py's loss and the C-way class head Wc h + bc with a softmax cross-entropy
// against the batch's labels, both from ONE read of H per direction.
//
// gm_acgan_heads_fwd = one launch.  One wave per 2 rows, 4 waves per workgroup.  A lane holds its rows' columns
//   4 lane + 256 j as float4s; w2 and each class row of Wc are loaded once per wave and used for both rows; every dot
//   product is a wave sum (a fixed butterfly), lane c keeps class logit c.  Per row: s, the NS term and d loss / d
//   logit with gm_gan_loss's NS targets (the +1e-8 included); the class logits' maximum, a max-subtracted
//   log-softmax, the cross-entropy term, dq = class_weight (softmax - onehot) / B, and whether the first maximal
//   logit is the label.  Three numbers per row go to a workspace; the last workgroup to finish (an integer arrival
//   counter) adds ALL rows' terms in fp64 in a fixed order and writes the loss slots -- whichever workgroup it is.
// gm_acgan_heads_bwd = one launch in generator mode, two in critic mode.
//   rows:    one workgroup per 8 rows, thread t owns hidden columns t + 256 j.  dPre1[m, n] = (da2[m] w2[n] +
//            sum_c dq[m, c] Wc[c, n]) . [H[m, n] > 0], classes in ascending order; in critic mode the thread also adds
//            its columns' gw2 / gWc over the block's rows in ascending order and the workgroup writes them (and gb2 /
//            gbc) as its partial, a [nblk][P] workspace with P = (C + 1)(Hd + 1).
//   combine: (critic mode) one thread per element of w2, Wc, b2, bc adds the nblk partials in workgroup order, writes
//            the gradient and steps Adam with the iteration's schedule row, as gm_label_grad_adam does for E.
//   No floating-point atomics: the same bits on every run, in a graph or not.
#include <math.h>
#include "gm_common.h"

namespace {

constexpr int AC_MAXH = 1024;
constexpr int AC_MAXC = 32;
constexpr int AC_FROWS = 8;          // forward: rows per workgroup (2 per wave)
constexpr int AC_BROWS = 8;          // backward: rows per workgroup
constexpr int AC_HDR = 4;            // workspace header (floats): the forward's arrival counter

__host__ __device__ inline int64_t ac_align4(int64_t n) { return (n + 3) & ~int64_t(3); }
inline int64_t ac_params(int Hd, int C) { return (int64_t)(C + 1) * (Hd + 1); }
inline int ac_fblocks(int rows) { return (rows + AC_FROWS - 1) / AC_FROWS; }
inline int ac_bblocks(int rows) { return (rows + AC_BROWS - 1) / AC_BROWS; }
inline bool ac_shape_ok(int rows, int Hd, int C) {
    return rows >= 1 && rows < (1 << 28) && Hd >= 4 && Hd <= AC_MAXH && Hd % 4 == 0 && C >= 1 && C <= AC_MAXC;
}
inline bool ac_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

struct HeadsP {
    gm_acgan_heads_args a;
    float inv_b;
    int nblk;                 // backward workgroups = partials
    int64_t P, P4;
    unsigned int* done;
    float* rowterm;           // [rows][3]: NS term, CE term, 1 if a real row is classified correctly
    float* part;              // [nblk][P4]
    float omb1, b2, omb2, eps;
};

// What the backward's rows kernel reads (a block of its own: the whole descriptor does not fit the scalar registers).
struct BwdP {
    const float* H; int64_t ldh;
    int rows, Hd, C, grads;
    const float* w2; const float* Wc; const float* da2; const float* dq; int64_t lddq;
    float* dPre; int64_t ldp;
    float* part; int64_t P4;
};

__device__ __forceinline__ float ac_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float ac_dot4(const float4& w, const float4& h, float acc) {
    acc = fmaf(w.x, h.x, acc);
    acc = fmaf(w.y, h.y, acc);
    acc = fmaf(w.z, h.z, acc);
    return fmaf(w.w, h.w, acc);
}

// The iteration's loss values by the last workgroup to arrive (gm_fused.hip's head_finalize protocol).
__device__ void ac_finalize(const HeadsP& p) {
    __shared__ int is_last;
    __shared__ double red[4][4];
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int prev = __hip_atomic_fetch_add(p.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (prev == gridDim.x - 1) ? 1 : 0;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    const gm_acgan_heads_args& a = p.a;
    double ns = 0.0, ce = 0.0, cer = 0.0, ok = 0.0;
    for (int m = threadIdx.x; m < a.rows; m += 256) {
        const double l = (double)__hip_atomic_load(p.rowterm + 3 * (int64_t)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double c = (double)__hip_atomic_load(p.rowterm + 3 * (int64_t)m + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double k = (double)__hip_atomic_load(p.rowterm + 3 * (int64_t)m + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ns += l; ce += c;
        if (m < a.B) { cer += c; ok += k; }
    }
    ns = gm_wave_sum_d(ns); ce = gm_wave_sum_d(ce); cer = gm_wave_sum_d(cer); ok = gm_wave_sum_d(ok);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red[0][w] = ns; red[1][w] = ce; red[2][w] = cer; red[3][w] = ok;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) t[q] = ((red[q][0] + red[q][1]) + red[q][2]) + red[q][3];
        const double ib = (double)p.inv_b;
        a.loss_out[gm_slot_index(a.loss_slot)] = (float)((t[0] + (double)a.class_weight * t[1]) * ib);
        if (a.ce_out) a.ce_out[gm_slot_index(a.ce_slot)] = (float)(t[2] * ib);
        if (a.acc_out) a.acc_out[gm_slot_index(a.acc_slot)] = (float)t[3];
        __hip_atomic_store(p.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(256) void acgan_heads_fwd_kernel(HeadsP p) {
    const gm_acgan_heads_args& a = p.a;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Hd = a.Hd, C = a.C, rows = a.rows;
    const int m0 = blockIdx.x * AC_FROWS + wave * 2;
    float4 h[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * lane + 256 * j;
            h[r][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m0 + r < rows && col < Hd) h[r][j] = *(const float4*)(a.H + (int64_t)(m0 + r) * a.ldh + col);
        }
    float src[2], z[2] = {0.f, 0.f};
    {
        float acc[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * lane + 256 * j;
            if (col < Hd) {
                const float4 w = *(const float4*)(a.w2 + col);
                acc[0] = ac_dot4(w, h[0][j], acc[0]);
                acc[1] = ac_dot4(w, h[1][j], acc[1]);
            }
        }
        src[0] = gm_wave_sum(acc[0]);
        src[1] = gm_wave_sum(acc[1]);
    }
    for (int c = 0; c < C; ++c) {                       // lane c keeps class logit c of both rows
        const float* wr = a.Wc + (int64_t)c * Hd;
        float acc[2] = {0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int col = 4 * lane + 256 * j;
            if (col < Hd) {
                const float4 w = *(const float4*)(wr + col);
                acc[0] = ac_dot4(w, h[0][j], acc[0]);
                acc[1] = ac_dot4(w, h[1][j], acc[1]);
            }
        }
        const float v0 = gm_wave_sum(acc[0]), v1 = gm_wave_sum(acc[1]);
        if (lane == c) { z[0] = v0; z[1] = v1; }
    }
    const float bcl = lane < C ? a.bc[lane] : 0.f;
    const float b2 = a.b2[0];
    const bool gen = a.gen_mode != 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int m = m0 + r;
        if (m >= rows) break;                           // (wave-uniform)
        const bool real = !gen && m < a.B;
        const int y = gm_row_label(a.lab, m < a.B ? m : m - a.B, C);    // fake row B + i: the class of row i
        const float zz = lane < C ? z[r] + bcl : -INFINITY;
        const float mx = ac_wave_max(zz);
        const float e = lane < C ? expf(zz - mx) : 0.f;
        const float se = gm_wave_sum(e);
        const float zy = __shfl(zz, y, 64);
        const float ce = logf(se) - (zy - mx);
        if (lane < C) a.dq[(int64_t)m * a.lddq + lane] = (a.class_weight * p.inv_b) * (e / se - (lane == y ? 1.f : 0.f));
        const unsigned long long top = __ballot(lane < C && zz == mx);
        const int pred = __builtin_ctzll(top);          // torch.argmax: the first maximal logit
        if (lane == 0) {
            const float s = gm_sigmoid(src[r] + b2);
            float lx, lg, dx, dg;
            sample_terms(GM_LOSS_NS, !gen, s, s, p.inv_b, nullptr, lx, lg, dx, dg);
            a.da2[m] = act_grad(real ? dx : dg, s, GM_ACT_SIGMOID);
            float* rt = p.rowterm + 3 * (int64_t)m;
            rt[0] = real ? lx : lg;
            rt[1] = ce;
            rt[2] = (real && pred == y) ? 1.f : 0.f;
        }
    }
    if (a.loss_out) ac_finalize(p);                     // (kernel-argument uniform)
}

__global__ __launch_bounds__(256) void acgan_heads_bwd_kernel(BwdP a) {
    __shared__ float sda[AC_BROWS];
    __shared__ float sdq[AC_BROWS][AC_MAXC];
    const int t = threadIdx.x, Hd = a.Hd, C = a.C, rows = a.rows;
    const int m0 = blockIdx.x * AC_BROWS;
    if (t < AC_BROWS) sda[t] = (m0 + t < rows) ? a.da2[m0 + t] : 0.f;
    {
        const int r = t >> 5, c = t & 31;               // 8 x 32 = one element per thread
        sdq[r][c] = (m0 + r < rows && c < C) ? a.dq[(int64_t)(m0 + r) * a.lddq + c] : 0.f;
    }
    __syncthreads();
    const bool grads = a.grads != 0;                    // generator step: the critic is frozen
    float* part = a.part + (int64_t)blockIdx.x * a.P4;
#pragma unroll 1
    for (int n = t; n < Hd; n += 256) {
        const float w2n = a.w2[n];
        float hv[AC_BROWS], v[AC_BROWS];
        float gw = 0.f;
#pragma unroll
        for (int r = 0; r < AC_BROWS; ++r) {
            hv[r] = m0 + r < rows ? a.H[(int64_t)(m0 + r) * a.ldh + n] : 0.f;
            v[r] = sda[r] * w2n;
            gw = fmaf(sda[r], hv[r], gw);
        }
        if (grads) part[n] = gw;
#pragma unroll 1
        for (int c = 0; c < C; ++c) {                   // classes in ascending order
            const float wcn = a.Wc[(int64_t)c * Hd + n];
            float gc = 0.f;
#pragma unroll
            for (int r = 0; r < AC_BROWS; ++r) {
                const float d = sdq[r][c];
                v[r] = fmaf(d, wcn, v[r]);
                gc = fmaf(d, hv[r], gc);
            }
            if (grads) part[(int64_t)Hd + (int64_t)c * Hd + n] = gc;
        }
#pragma unroll
        for (int r = 0; r < AC_BROWS; ++r)
            if (m0 + r < rows) a.dPre[(int64_t)(m0 + r) * a.ldp + n] = hv[r] > 0.f ? v[r] : 0.f;
    }
    if (grads && t <= C) {                              // gb2 (t == 0) and gbc[t - 1]
        float s = 0.f;
        for (int r = 0; r < AC_BROWS; ++r) s += t == 0 ? sda[r] : sdq[r][t - 1];
        part[(int64_t)(C + 1) * Hd + t] = s;
    }
}

__global__ __launch_bounds__(256) void acgan_heads_combine_kernel(HeadsP p) {
    const gm_acgan_heads_args& a = p.a;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= p.P) return;
    float g = 0.f;
    for (int w = 0; w < p.nblk; ++w) g += p.part[(int64_t)w * p.P4 + j];
    const int64_t nW = (int64_t)(a.C + 1) * a.Hd;
    float *P, *G, *Mm, *V;
    int64_t o;
    if (j < a.Hd) { P = a.w2; G = a.gw2; Mm = a.mw2; V = a.vw2; o = j; }
    else if (j < nW) { P = a.Wc; G = a.gWc; Mm = a.mWc; V = a.vWc; o = j - a.Hd; }
    else if (j == nW) { P = a.b2; G = a.gb2; Mm = a.mb2; V = a.vb2; o = 0; }
    else { P = a.bc; G = a.gbc; Mm = a.mbc; V = a.vbc; o = j - nW - 1; }
    if (G) G[o] = g;
    if (a.sched) {
        const int64_t si = gm_slot_index(a.sched_slot);
        const float step_size = a.sched[2 * si], bc2_sqrt = a.sched[2 * si + 1];
        float pp = P[o], mm = Mm[o], vv = V[o];
        adam_update(pp, g, mm, vv, step_size, bc2_sqrt, p.omb1, p.b2, p.omb2, p.eps, 0.f, 0.f);
        P[o] = pp; Mm[o] = mm; V[o] = vv;
    }
}

int ac_common_check(const gm_acgan_heads_args* a, HeadsP* p) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(ac_shape_ok(a->rows, a->Hd, a->C));
    GM_CHECK_ARG(a->B >= 1 && (a->gen_mode ? a->rows == a->B : a->rows == 2 * a->B));
    GM_CHECK_ARG(a->H && a->ldh >= a->Hd && a->ldh % 4 == 0 && ac_aligned16(a->H));
    GM_CHECK_ARG(a->w2 && a->b2 && a->Wc && a->bc && ac_aligned16(a->w2) && ac_aligned16(a->Wc));
    GM_CHECK_ARG(a->da2 && a->dq && a->lddq >= a->C);
    GM_CHECK_ARG(a->ws && ac_aligned16(a->ws) && a->ws_bytes >= gm_acgan_heads_workspace_bytes(a->rows, a->Hd, a->C));
    p->a = *a;
    p->inv_b = 1.f / (float)a->B;
    p->nblk = ac_bblocks(a->rows);
    p->P = ac_params(a->Hd, a->C);
    p->P4 = ac_align4(p->P);
    p->done = (unsigned int*)a->ws;
    p->rowterm = a->ws + AC_HDR;
    p->part = p->rowterm + ac_align4(3 * (int64_t)a->rows);
    p->omb1 = (float)(1.0 - a->beta1); p->b2 = (float)a->beta2; p->omb2 = (float)(1.0 - a->beta2);
    p->eps = (float)a->eps;
    return 0;
}

}  // namespace

extern "C" int64_t gm_acgan_heads_workspace_bytes(int rows, int Hd, int C) {
    if (!ac_shape_ok(rows, Hd, C)) return -1;
    return (int64_t)4 * (AC_HDR + ac_align4(3 * (int64_t)rows) + (int64_t)ac_bblocks(rows) * ac_align4(ac_params(Hd, C)));
}

extern "C" int gm_acgan_heads_fwd(void* stream, const gm_acgan_heads_args* a) {
    HeadsP p{};
    const int rc = ac_common_check(a, &p);
    if (rc) return rc;
    GM_CHECK_ARG(a->lab.labels);
    GM_CHECK_ARG(a->loss_out || (!a->ce_out && !a->acc_out));
    hipLaunchKernelGGL(acgan_heads_fwd_kernel, dim3(ac_fblocks(a->rows)), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_acgan_heads_bwd(void* stream, const gm_acgan_heads_args* a) {
    HeadsP p{};
    const int rc = ac_common_check(a, &p);
    if (rc) return rc;
    GM_CHECK_ARG(a->dPre && a->ldp >= a->Hd && (const float*)a->dPre != a->H);
    const bool grads = a->gw2 || a->gb2 || a->gWc || a->gbc;
    if (a->gen_mode) {
        GM_CHECK_ARG(!grads && !a->sched);              // the critic is frozen in the generator step
    } else {
        GM_CHECK_ARG(!grads || (a->gw2 && a->gb2 && a->gWc && a->gbc));
        GM_CHECK_ARG(grads || a->sched);
        GM_CHECK_ARG(!a->sched || (a->mw2 && a->vw2 && a->mb2 && a->vb2 && a->mWc && a->vWc && a->mbc && a->vbc));
    }
    BwdP b{a->H, a->ldh, a->rows, a->Hd, a->C, a->gen_mode ? 0 : 1, a->w2, a->Wc, a->da2, a->dq, a->lddq,
           a->dPre, a->ldp, p.part, p.P4};
    hipLaunchKernelGGL(acgan_heads_bwd_kernel, dim3(p.nblk), dim3(256), 0, (hipStream_t)stream, b);
    if (!a->gen_mode)
        hipLaunchKernelGGL(acgan_heads_combine_kernel, dim3((unsigned)((p.P + 255) / 256)), dim3(256), 0,
                           (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
