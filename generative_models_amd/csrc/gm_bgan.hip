// Bayesian GAN (bgan.py; gm_hip.h): the device-side counter-based generator, the SGHMC update and the critic
// ensemble's head.
//
// Philox4x32-10 (gm_philox.h): key = (seed mod 2^32, seed >> 32), counter = (e >> 2, t, stream, 0) for element e of the
// draw (stream, step t); normals by ph_normal4's Box-Muller mapping.
//
// gm_sghmc_step: one thread per four elements of one tensor (one Philox call -> the four normals of that group); the
//   segment table rides in the kernel arguments, the step t and the learning rate are read from device memory.
//   v <- (1 - a) v - lr (g + theta prior) + sqrt(noise lr) xi ; theta <- theta + v.  No atomics, no reductions.
//
// gm_bgan_head = two launches over h [R, Jd H] (the stacked critics' hidden rows):
//   rows:    workgroup (16-row block, critic k).  Each thread holds four hidden columns of the 16 rows in registers,
//            its share of every row's logit w2_k . h, added wave by wave in wave order; 16 threads form s, the loss
//            term and d loss / d logit; then dH = dlogit w2_k [h > 0] goes back over h in place and the block's gw2
//            partial (rows in ascending order) goes to the workspace, with the per-row terms and dlogits.
//   combine: one thread per gw2 element adds the block partials in block order; one workgroup per gb2 / loss output
//            adds its row values in fp64, strided then wave then the four waves in order.
//   The same bits on every run, in a graph or not.
#include "gm_common.h"
#include "gm_philox.h"

namespace {

__global__ __launch_bounds__(256) void philox_raw_kernel(const uint32_t* __restrict__ ctr,
                                                         const uint32_t* __restrict__ key, uint32_t* __restrict__ out,
                                                         int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint4 c = make_uint4(ctr[4 * i], ctr[4 * i + 1], ctr[4 * i + 2], ctr[4 * i + 3]);
    const uint4 x = philox10(c, key[2 * i], key[2 * i + 1]);
    out[4 * i] = x.x;
    out[4 * i + 1] = x.y;
    out[4 * i + 2] = x.z;
    out[4 * i + 3] = x.w;
}

struct NormalP {
    uint64_t seed;
    uint32_t stream0, stream_stride;
    const int64_t* step; int64_t step_add;
    float* out; int64_t n, groups;       // groups per stream = ceil(n / 4)
    int nstreams;
};

__global__ __launch_bounds__(256) void philox_normal_kernel(NormalP p) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= p.groups * p.nstreams) return;
    const int64_t j = gi / p.groups, q = gi - j * p.groups;
    const uint32_t t = (uint32_t)((p.step ? *p.step : 0) + p.step_add);
    const float4 v = ph_normal4(p.seed, p.stream0 + (uint32_t)j * p.stream_stride, t, (uint32_t)q);
    float* o = p.out + j * p.n;
    const int64_t e0 = 4 * q;
    if (e0 + 4 <= p.n && (((uintptr_t)(o + e0)) & 15) == 0) {
        *reinterpret_cast<float4*>(o + e0) = v;
    } else {
        for (int i = 0; i < 4 && e0 + i < p.n; ++i) o[e0 + i] = ph_lane(v, i);
    }
}

struct SghmcP {
    float* theta; const float* grad; float* mom;
    const int64_t* step; int64_t step_add;
    const float* lr;
    float friction, prior, noise;
    uint64_t seed;
    int nseg;
    int64_t off[GM_SGHMC_MAX_SEGS], numel[GM_SGHMC_MAX_SEGS];
    uint32_t stream[GM_SGHMC_MAX_SEGS];
    int64_t gstart[GM_SGHMC_MAX_SEGS + 1];     // first group of each segment; gstart[nseg] = total groups
};

__device__ __forceinline__ void sghmc_elem(float& th, float g, float& v, float xi, float keep, float lr, float prior,
                                           float sd) {
    const float ge = fmaf(th, prior, g);
    float vv = fmaf(keep, v, -lr * ge);
    vv = fmaf(sd, xi, vv);
    v = vv;
    th = th + vv;
}

__global__ __launch_bounds__(256) void sghmc_kernel(SghmcP p) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= p.gstart[p.nseg]) return;
    int lo = 0, hi = p.nseg - 1;                 // the segment holding group gi
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (p.gstart[mid] <= gi) lo = mid; else hi = mid - 1;
    }
    const int s = lo;
    const int64_t q = gi - p.gstart[s], e0 = 4 * q, n = p.numel[s], base = p.off[s] + e0;
    const uint32_t t = (uint32_t)((p.step ? *p.step : 0) + p.step_add);
    const float lr = *p.lr;
    const float sd = sqrtf(p.noise * lr), keep = 1.f - p.friction;
    const float4 xi = ph_normal4(p.seed, p.stream[s], t, (uint32_t)q);
    if (e0 + 4 <= n && (base & 3) == 0) {
        float4 th = *reinterpret_cast<const float4*>(p.theta + base);
        const float4 g = *reinterpret_cast<const float4*>(p.grad + base);
        float4 v = *reinterpret_cast<const float4*>(p.mom + base);
        sghmc_elem(th.x, g.x, v.x, xi.x, keep, lr, p.prior, sd);
        sghmc_elem(th.y, g.y, v.y, xi.y, keep, lr, p.prior, sd);
        sghmc_elem(th.z, g.z, v.z, xi.z, keep, lr, p.prior, sd);
        sghmc_elem(th.w, g.w, v.w, xi.w, keep, lr, p.prior, sd);
        *reinterpret_cast<float4*>(p.theta + base) = th;
        *reinterpret_cast<float4*>(p.mom + base) = v;
    } else {
        for (int i = 0; i < 4 && e0 + i < n; ++i) {
            float th = p.theta[base + i], v = p.mom[base + i];
            sghmc_elem(th, p.grad[base + i], v, ph_lane(xi, i), keep, lr, p.prior, sd);
            p.theta[base + i] = th;
            p.mom[base + i] = v;
        }
    }
}

// ---- the critic ensemble's head ----------------------------------------------------------------------------------
constexpr int BH_ROWS = 16;
constexpr int BH_COLS = 4;                   // hidden columns per thread: H <= 1024
constexpr int BH_MAXH = 256 * BH_COLS;

struct HeadP {
    gm_bgan_head_args a;
    int R, nblk;
    float* part;                             // [nblk][Jd H]
    float* rterm;                            // [Jd][R]
    float* rdl;                              // [Jd][R]
};

inline int bh_rows(int mode, int B, int Jg) { return mode == 0 ? (1 + Jg) * B : Jg * B; }
inline int bh_blocks(int R) { return (R + BH_ROWS - 1) / BH_ROWS; }

__global__ __launch_bounds__(256) void bgan_head_rows_kernel(HeadP p) {
    __shared__ float red[4][BH_ROWS];
    __shared__ float sdl[BH_ROWS];
    const gm_bgan_head_args& a = p.a;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int k = blockIdx.y, H = a.H, i0 = blockIdx.x * BH_ROWS;
    float* hk = a.h + (int64_t)k * H;
    const float* w2 = a.w2 + (int64_t)k * H;
    float hv[BH_ROWS][BH_COLS];
    float lp[BH_ROWS];
#pragma unroll
    for (int r = 0; r < BH_ROWS; ++r) lp[r] = 0.f;
#pragma unroll
    for (int c = 0; c < BH_COLS; ++c) {
        const int n = t + 256 * c;
        const float ww = n < H ? w2[n] : 0.f;
#pragma unroll
        for (int r = 0; r < BH_ROWS; ++r) {
            const int i = i0 + r;
            hv[r][c] = (n < H && i < p.R) ? hk[(int64_t)i * a.ldh + n] : 0.f;
            lp[r] = fmaf(ww, hv[r][c], lp[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < BH_ROWS; ++r) {
        const float v = gm_wave_sum(lp[r]);
        if (lane == 0) red[w][r] = v;
    }
    __syncthreads();
    if (t < BH_ROWS) {
        const int i = i0 + t;
        float dl = 0.f;
        if (i < p.R) {
            const float logit = (((red[0][t] + red[1][t]) + red[2][t]) + red[3][t]) + a.b2[k];
            const float s = gm_sigmoid(logit), ds = s * (1.f - s);
            const float ib = 1.f / (float)a.B;
            float term;
            if (a.mode == 0 && i < a.B) {            // -(1/b) log(D_k(x_i) + eps)
                const float u = s + EPS;
                term = -logf(u) * ib;
                dl = -ib * ds / u;
            } else if (a.mode == 0) {                // -(1/b)(1/Jg) log(1 - D_k(G_j(z_j,i)) + eps)
                const float wf = ib / (float)a.Jg, u = (1.f - s) + EPS;
                term = -logf(u) * wf;
                dl = wf * ds / u;
            } else {                                 // -(1/b)(1/Jd) log(D_k(G_j(z_j,i)) + eps)
                const float wg = ib / (float)a.Jd, u = s + EPS;
                term = -logf(u) * wg;
                dl = -wg * ds / u;
            }
            p.rterm[(int64_t)k * p.R + i] = term;
            p.rdl[(int64_t)k * p.R + i] = dl;
        }
        sdl[t] = dl;
    }
    __syncthreads();
    float* part = p.part + (int64_t)blockIdx.x * a.Jd * H + (int64_t)k * H;
#pragma unroll
    for (int c = 0; c < BH_COLS; ++c) {
        const int n = t + 256 * c;
        if (n >= H) break;
        const float ww = w2[n];
        float gw = 0.f;
#pragma unroll
        for (int r = 0; r < BH_ROWS; ++r) {
            gw = fmaf(sdl[r], hv[r][c], gw);
            const int i = i0 + r;
            if (i < p.R) hk[(int64_t)i * a.ldh + n] = hv[r][c] > 0.f ? sdl[r] * ww : 0.f;
        }
        part[n] = gw;
    }
}

// Sum of the n floats p[0], p[stride], ... by one 256-thread workgroup in a fixed order (fp64); valid in thread 0.
__device__ __forceinline__ double bh_block_sum(const float* __restrict__ p, int n, double* sh) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) acc += (double)p[i];
    acc = gm_wave_sum_d(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void bgan_head_combine_kernel(HeadP p, int nw) {
    __shared__ double sh[4];
    const gm_bgan_head_args& a = p.a;
    const int JH = a.Jd * a.H;
    if ((int)blockIdx.x < nw) {                  // gw2[k, n]: the block partials in block order
        const int e = blockIdx.x * 256 + threadIdx.x;
        if (e >= JH) return;
        float s = 0.f;
        for (int b = 0; b < p.nblk; ++b) s += p.part[(int64_t)b * JH + e];
        a.gw2[e] = s;
        return;
    }
    const int o = blockIdx.x - nw;
    float* loss = a.loss_out ? a.loss_out + gm_slot_offset(a.loss_slot) : nullptr;
    if (a.mode == 0) {
        if (o < a.Jd) {                          // gb2[k]
            const double s = bh_block_sum(p.rdl + (int64_t)o * p.R, p.R, sh);
            if (threadIdx.x == 0 && a.gb2) a.gb2[o] = (float)s;
        } else {                                 // L_D^k
            const int k = o - a.Jd;
            const double s = bh_block_sum(p.rterm + (int64_t)k * p.R, p.R, sh);
            if (threadIdx.x == 0 && loss) loss[k] = (float)s;
        }
        return;
    }
    // G mode: L_G^j = sum over critics (in order) of generator j's B rows
    double tot = 0.0;
    for (int k = 0; k < a.Jd; ++k) {
        tot += bh_block_sum(p.rterm + (int64_t)k * p.R + (int64_t)o * a.B, a.B, sh);
        __syncthreads();
    }
    if (threadIdx.x == 0 && loss) loss[o] = (float)tot;
}

bool head_shape_ok(int mode, int B, int Jg, int Jd, int H) {
    return (mode == 0 || mode == 1) && B > 0 && Jg >= 1 && Jg <= GM_BGAN_MAX_J && Jd >= 1 && Jd <= GM_BGAN_MAX_J &&
           H > 0 && H <= BH_MAXH && H % 4 == 0 && (int64_t)(1 + Jg) * B < (1 << 24);
}

}  // namespace

extern "C" int gm_philox_raw(void* stream, const uint32_t* ctr, const uint32_t* key, uint32_t* out, int64_t n) {
    GM_CHECK_ARG(ctr && key && out && n > 0 && n < (1ll << 31));
    hipLaunchKernelGGL(philox_raw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ctr,
                       key, out, n);
    GM_LAUNCH_RET();
}

extern "C" int gm_philox_normal(void* stream, uint64_t seed, uint32_t stream0, uint32_t stream_stride, int nstreams,
                                const int64_t* step, int64_t step_add, float* out, int64_t n) {
    GM_CHECK_ARG(out && n > 0 && n < (1ll << 33) && nstreams >= 1 && nstreams <= 4096);
    NormalP p{seed, stream0, stream_stride, step, step_add, out, n, (n + 3) / 4, nstreams};
    const int64_t total = p.groups * nstreams;
    GM_CHECK_ARG(total < (1ll << 31) * 256);
    hipLaunchKernelGGL(philox_normal_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_sghmc_step(void* stream, const gm_sghmc_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->theta && a->grad && a->mom && a->lr && a->segs && a->n_flat > 0);
    GM_CHECK_ARG(a->nseg >= 1 && a->nseg <= GM_SGHMC_MAX_SEGS);
    GM_CHECK_ARG(a->friction >= 0.f && a->friction <= 1.f && a->noise >= 0.f && a->prior >= 0.f);
    GM_CHECK_ARG(a->theta != a->mom && (const float*)a->theta != a->grad && (const float*)a->mom != a->grad);
    SghmcP p{};
    p.theta = a->theta; p.grad = a->grad; p.mom = a->mom;
    p.step = a->step; p.step_add = a->step_add; p.lr = a->lr;
    p.friction = a->friction; p.prior = a->prior; p.noise = a->noise; p.seed = a->seed;
    p.nseg = a->nseg;
    int64_t g = 0;
    for (int s = 0; s < a->nseg; ++s) {
        const gm_sghmc_seg& sg = a->segs[s];
        GM_CHECK_ARG(sg.offset >= 0 && sg.numel > 0 && sg.offset + sg.numel <= a->n_flat);
        for (int r = 0; r < s; ++r) {           // disjoint segments: every element is written by one thread
            const gm_sghmc_seg& o = a->segs[r];
            GM_CHECK_ARG(sg.offset + sg.numel <= o.offset || o.offset + o.numel <= sg.offset);
        }
        GM_CHECK_ARG(sg.numel < (1ll << 34));
        p.off[s] = sg.offset; p.numel[s] = sg.numel; p.stream[s] = sg.stream;
        p.gstart[s] = g;
        g += (sg.numel + 3) / 4;
    }
    p.gstart[a->nseg] = g;
    GM_CHECK_ARG(g < (1ll << 31) * 256);
    hipLaunchKernelGGL(sghmc_kernel, dim3((unsigned)((g + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int64_t gm_bgan_head_workspace_bytes(int mode, int B, int Jg, int Jd, int H) {
    if (!head_shape_ok(mode, B, Jg, Jd, H)) return -1;
    const int64_t R = bh_rows(mode, B, Jg);
    return 4 * ((int64_t)bh_blocks((int)R) * Jd * H + 2 * (int64_t)Jd * R);
}

extern "C" int gm_bgan_head(void* stream, const gm_bgan_head_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(head_shape_ok(a->mode, a->B, a->Jg, a->Jd, a->H));
    GM_CHECK_ARG(a->h && a->ldh >= (int64_t)a->Jd * a->H && a->w2 && a->b2 && a->ws);
    GM_CHECK_ARG(a->ws_bytes >= gm_bgan_head_workspace_bytes(a->mode, a->B, a->Jg, a->Jd, a->H));
    GM_CHECK_ARG(a->mode == 1 || a->gw2);
    HeadP p{};
    p.a = *a;
    p.R = bh_rows(a->mode, a->B, a->Jg);
    p.nblk = bh_blocks(p.R);
    p.part = a->ws;
    p.rterm = p.part + (int64_t)p.nblk * a->Jd * a->H;
    p.rdl = p.rterm + (int64_t)a->Jd * p.R;
    hipLaunchKernelGGL(bgan_head_rows_kernel, dim3(p.nblk, a->Jd), dim3(256), 0, (hipStream_t)stream, p);
    const int nw = a->mode == 0 ? (a->Jd * a->H + 255) / 256 : 0;
    const int nred = a->mode == 0 ? 2 * a->Jd : a->Jg;
    hipLaunchKernelGGL(bgan_head_combine_kernel, dim3(nw + nred), dim3(256), 0, (hipStream_t)stream, p, nw);
    GM_LAUNCH_RET();
}
