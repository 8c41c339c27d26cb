// Planar-flow posterior of the normalizing-flow VAE (nfvae.py holds the contract; gm_hip.h).  The
// IWAE's two row kernels with a chain of K planar layers between z_0 and the decoder, and the flow's own optimiser step.
// Rows are image-major (sample j of image b is row b k + j); the noise block and the counter layout are gm_philox.h's PhNoise.
//
// Layer constants (every kernel, once per workgroup, into LDS): 8 lanes per layer, lane q the latents 4q .. 4q + 3;
//   s0 = w.u, u_hat = u + (m(s0) - s0) w / (|w|^2 + 1e-12) with m(x) = -1 + softplus(x), s = w.u_hat.
// gm_flow_sample: 8 lanes per sample row (gm_iwae_sample's mapping), z in registers through the K layers, every dot
//   product by the fixed 8-lane butterfly; writes z_K and lp = 1/2 |eps|^2 + 1/2 sum lv + sum_k logdet_k - 1/2 |z_K|^2.
// gm_flow_reduce: one wave per 8 images, 8 lanes per image, the image's samples j ascending (so d loss / d [mu | lv] is
//   summed in gm_iwae_reduce's order whatever workgroup the image lands in).  Per sample the chain is run forward (t_k =
//   tanh(a_k) kept in the lane's own LDS column), then walked back: z_{k-1} = z_k - u_hat_k t_k, and the closed-form
//   gradients.  The parameter gradients of a layer are summed over the wave's 8 images by a fixed butterfly and over j
//   in LDS; one partial block [K, 68] per workgroup: [d u_hat (32) | d w through a (32) | d b | d s | 0 0].
// gm_flow_step: one workgroup, 8 lanes per layer: the partial blocks summed in ascending order, the u_hat gradient
//   mapped through the constraint onto u and w, Adam (adam_update, the arithmetic of every other step of the project).
// No atomics, fixed reduction orders, no scratch: the same bits on every run, graph or eager.
#include "gm_philox.h"

namespace {

constexpr int FL_K = GM_FLOW_MAX_K, FL_Z = GM_IWAE_MAX_Z, FL_FS = GM_FLOW_PART_STRIDE;
static_assert(FL_K == 32 && FL_Z == 32 && FL_FS >= 2 * FL_Z + 2 && FL_FS % 4 == 0, "the lane mappings assume 32 x 32");

struct FlowW { const float* u; const float* w; const float* b; int K; };

struct FlowLds {                                                 // the layers' constants, columns >= Z zero
    float w[FL_K][FL_Z];
    float uh[FL_K][FL_Z];
    float b[FL_K];
    float s[FL_K];
};

// Sum over the 8 lanes of a row / layer group: the same bits in each of them.
__device__ __forceinline__ float fl_sum8(float v) {
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

__device__ __forceinline__ float fl_dot4(const float (&a)[4], const float (&b)[4]) {
    return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])));
}

__device__ __forceinline__ float fl_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// u_hat, s0, the constraint's coefficient c = (m(s0) - s0) / n2 and n2 = |w|^2 + 1e-12 of one layer from the group's
// quads of u and w (zero beyond Z).
__device__ __forceinline__ void fl_constrain(const float (&u)[4], const float (&w)[4], float (&uh)[4], float& s0,
                                             float& coef, float& n2) {
#pragma clang fp contract(off)
    s0 = fl_sum8(fl_dot4(w, u));
    n2 = fl_sum8(fl_dot4(w, w)) + 1e-12f;
    coef = ((-1.f + fl_softplus(s0)) - s0) / n2;
#pragma unroll
    for (int i = 0; i < 4; ++i) uh[i] = fmaf(coef, w[i], u[i]);
}

// Every thread of the workgroup (a multiple of 64 threads) calls this; a barrier follows at the caller.
__device__ __forceinline__ void fl_constants(const FlowW& f, int Z, FlowLds& L) {
    const int g = threadIdx.x >> 3, q = threadIdx.x & 7, G = blockDim.x >> 3;
    for (int k0 = 0; k0 < f.K; k0 += G) {                        // uniform trip count: the butterflies see whole waves
        const int k = k0 + g, kk = min(k, f.K - 1);
        float u[4], w[4], uh[4], s0, coef, n2;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * q + i;
            u[i] = c < Z ? f.u[kk * Z + c] : 0.f;
            w[i] = c < Z ? f.w[kk * Z + c] : 0.f;
        }
        fl_constrain(u, w, uh, s0, coef, n2);
        const float s = fl_sum8(fl_dot4(w, uh));
        if (k < f.K) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                L.w[k][4 * q + i] = w[i];
                L.uh[k][4 * q + i] = uh[i];
            }
            if (q == 0) {
                L.b[k] = f.b[k];
                L.s[k] = s;
            }
        }
    }
}

// One planar layer on the row's z (lane q: latents 4q .. 4q + 3): z += u_hat t; returns log D, t = tanh(w.z + b).
__device__ __forceinline__ float fl_layer(const FlowLds& L, int k, int q, float (&z)[4], float& t) {
#pragma clang fp contract(off)
    float w[4], uh[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = L.w[k][4 * q + i];
        uh[i] = L.uh[k][4 * q + i];
    }
    const float a = fl_sum8(fl_dot4(w, z)) + L.b[k];
    t = tanhf(a);
    const float D = fmaf(fmaf(-t, t, 1.f), L.s[k], 1.f);
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = fmaf(uh[i], t, z[i]);
    return logf(D);
}

struct SampleP {
    const float* ml; int64_t ldml;
    float* z; int64_t ldz;
    float* lp;
    int64_t rows; int k, Z;
};

__global__ __launch_bounds__(256) void flow_sample_kernel(SampleP p, FlowW f, PhNoise n) {
    __shared__ FlowLds L;
    fl_constants(f, p.Z, L);
    __syncthreads();
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = gi >> 3, rr = min(r, p.rows - 1);          // rows past the end redo the last one and store nothing
    const int q = (int)(gi & 7);
    const int64_t b = rr / p.k;
    const int j = (int)(rr - b * p.k);
    float e[4], z[4];
    ph_noise_eps4(n, ph_step(n.clk), (uint32_t)(b * n.kt + n.j0 + j), (uint32_t)q, e);
    const float* ml = p.ml + b * p.ldml;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * q + i;
        z[i] = 0.f;
        if (c < p.Z) {
            const float lv = ml[p.Z + c];
            z[i] = gm_reparam_z(ml[c], e[i], lv);
            acc += 0.5f * (e[i] * e[i] + lv);
        }
    }
    float ld = 0.f, t;
    for (int k = 0; k < f.K; ++k) ld += fl_layer(L, k, q, z, t);
    acc -= 0.5f * fl_dot4(z, z);
    acc = fl_sum8(acc) + ld;
    if (r < p.rows) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (4 * q + i < p.Z) p.z[r * p.ldz + 4 * q + i] = z[i];
        if (q == 0) p.lp[r] = acc;
    }
}

struct ReduceP {
    const float* ml; int64_t ldml;
    const float* wn;
    const float* dzdec; int64_t lddz;
    float* dml; int64_t lddml;
    float* part;
    int64_t B; int k, Z;
};

// Sum over the wave's 8 groups (lanes q, q + 8, ..., q + 56): fixed butterfly, the total in every lane.
__device__ __forceinline__ float fl_sum_groups(float v) {
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

__global__ __launch_bounds__(64) void flow_reduce_kernel(ReduceP p, FlowW f, PhNoise n) {
    __shared__ FlowLds L;
    __shared__ float tl[FL_K][64];                               // t_k of the lane's current sample (its own column)
    __shared__ float acc[FL_K][FL_FS];                           // the workgroup's partial block
    fl_constants(f, p.Z, L);
    for (int i = threadIdx.x; i < FL_K * FL_FS; i += 64) (&acc[0][0])[i] = 0.f;
    __syncthreads();
    const int tid = threadIdx.x, q = tid & 7, Z = p.Z;
    const int64_t b = (int64_t)blockIdx.x * 8 + (tid >> 3), bb = min(b, p.B - 1);
    const bool on = b < p.B;                                     // images past the end: weight 0, nothing stored
    const float* ml = p.ml + bb * p.ldml;
    float mu[4], lv[4], sd[4], amu[4], alv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = min(4 * q + i, Z - 1);
        mu[i] = ml[c];
        lv[i] = ml[Z + c];
        sd[i] = expf(lv[i] / 2.f);
        amu[i] = alv[i] = 0.f;
    }
    const uint32_t step = ph_step(n.clk);
    for (int j = 0; j < p.k; ++j) {
        const int64_t r = bb * p.k + j;
        float e[4], z[4], g[4];
        ph_noise_eps4(n, step, (uint32_t)(bb * n.kt + n.j0 + j), (uint32_t)q, e);
#pragma unroll
        for (int i = 0; i < 4; ++i) z[i] = 4 * q + i < Z ? gm_reparam_z(mu[i], e[i], lv[i]) : 0.f;
        for (int k = 0; k < f.K; ++k) {
            float t;
            fl_layer(L, k, q, z, t);
            tl[k][tid] = t;
        }
        const float wn = on ? p.wn[r] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            g[i] = (on && 4 * q + i < Z) ? fmaf(wn, z[i], p.dzdec[r * p.lddz + 4 * q + i]) : 0.f;
        for (int k = f.K - 1; k >= 0; --k) {
            const float t = tl[k][tid], s = L.s[k];
            float w[4], uh[4], cu[4], cw[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w[i] = L.w[k][4 * q + i];
                uh[i] = L.uh[k][4 * q + i];
            }
            const float omt = fmaf(-t, t, 1.f), D = fmaf(omt, s, 1.f);
            // d loss / d logdet_k = -wn: through D = 1 + (1 - t^2) s onto t and s
            const float dt = fl_sum8(fl_dot4(g, uh)) + wn * ((2.f * t * s) / D);
            const float da = dt * omt, ds = -(wn * omt) / D;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                z[i] = fmaf(-uh[i], t, z[i]);                    // the layer's input z_{k-1}
                cu[i] = fl_sum_groups(g[i] * t);
                cw[i] = fl_sum_groups(da * z[i]);
                g[i] = fmaf(da, w[i], g[i]);
            }
            const float cb = fl_sum_groups(da), cs = fl_sum_groups(ds);
            if (tid < 8) {                                       // group 0 owns the block: j ascending, k descending
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[k][4 * q + i] += cu[i];
                    acc[k][FL_Z + 4 * q + i] += cw[i];
                }
                if (tid == 0) {
                    acc[k][2 * FL_Z] += cb;
                    acc[k][2 * FL_Z + 1] += cs;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            amu[i] += g[i];
            alv[i] = fmaf(g[i] * e[i], sd[i], alv[i]);
        }
    }
    if (on) {
        float* o = p.dml + b * p.lddml;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * q + i;
            if (c < Z) {
                o[c] = amu[i];
                o[Z + c] = 0.5f * alv[i] - 0.5f;
            }
        }
    }
    __syncthreads();
    float* po = p.part + (int64_t)blockIdx.x * f.K * FL_FS;
    for (int i = tid; i < f.K * FL_FS; i += 64) po[i] = (&acc[0][0])[i];
}

struct StepP {
    const float* part; int nparts;
    float* u; float* w; float* b;
    float* gu; float* gw; float* gb;
    float* mu; float* vu; float* mw; float* vw; float* mb; float* vb;
    const float* sched; gm_slot slot;
    float omb1, b2, omb2, eps, wd;
    int K, Z;
};

__global__ __launch_bounds__(256) void flow_step_kernel(StepP p) {
    const int g = threadIdx.x >> 3, q = threadIdx.x & 7, K = p.K, Z = p.Z;
    const int k = min(g, K - 1);                                 // groups past K redo the last layer and store nothing
    float u[4], w[4], uh[4], s0, coef, n2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * q + i;
        u[i] = c < Z ? p.u[k * Z + c] : 0.f;
        w[i] = c < Z ? p.w[k * Z + c] : 0.f;
    }
    fl_constrain(u, w, uh, s0, coef, n2);
    float Gu[4] = {0.f, 0.f, 0.f, 0.f}, Gw[4] = {0.f, 0.f, 0.f, 0.f}, Gb = 0.f, Gs = 0.f;
#pragma unroll 4
    for (int i = 0; i < p.nparts; ++i) {                         // ascending: the sum does not depend on the grid
        const float* a = p.part + ((int64_t)i * K + k) * FL_FS;
        const float4 x = reinterpret_cast<const float4*>(a)[q], y = reinterpret_cast<const float4*>(a + FL_Z)[q];
        Gu[0] += x.x; Gu[1] += x.y; Gu[2] += x.z; Gu[3] += x.w;
        Gw[0] += y.x; Gw[1] += y.y; Gw[2] += y.z; Gw[3] += y.w;
        Gb += a[2 * FL_Z];
        Gs += a[2 * FL_Z + 1];
    }
    float G[4], du[4], dw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) G[i] = fmaf(Gs, w[i], Gu[i]);    // d loss / d u_hat, s = w.u_hat included
    // u_hat = u + c(s0, n2) w:  dc / ds0 = (sigmoid(s0) - 1) / n2,  dc / dn2 = -c / n2,  ds0 = u dw + w du,  dn2 = 2 w dw
    const float Gdw = fl_sum8(fl_dot4(G, w));
    const float c_s = Gdw * ((gm_sigmoid(s0) - 1.f) / n2), c_n = Gdw * (-coef / n2);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        du[i] = fmaf(c_s, w[i], G[i]);
        dw[i] = fmaf(Gs, uh[i], Gw[i]) + fmaf(coef, G[i], fmaf(c_s, u[i], (2.f * c_n) * w[i]));
    }
    if (g >= K) return;
    const int64_t si = gm_slot_index(p.slot);
    const float step_size = p.sched[2 * si], bc2_sqrt = p.sched[2 * si + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = 4 * q + i;
        if (c < Z) {
            const int o = k * Z + c;
            if (p.gu) {
                p.gu[o] = du[i];
                p.gw[o] = dw[i];
            }
            adam_update(p.u[o], du[i], p.mu[o], p.vu[o], step_size, bc2_sqrt, p.omb1, p.b2, p.omb2, p.eps, p.wd, 0.f);
            adam_update(p.w[o], dw[i], p.mw[o], p.vw[o], step_size, bc2_sqrt, p.omb1, p.b2, p.omb2, p.eps, p.wd, 0.f);
        }
    }
    if (q == 0) {
        if (p.gb) p.gb[k] = Gb;
        adam_update(p.b[k], Gb, p.mb[k], p.vb[k], step_size, bc2_sqrt, p.omb1, p.b2, p.omb2, p.eps, p.wd, 0.f);
    }
}

inline int fl_params_fill(const gm_flow_params* a, FlowW* f) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->u && a->w && a->b && a->K >= 1 && a->K <= GM_FLOW_MAX_K);
    GM_CHECK_ARG(a->u != a->w && a->u != a->b && a->w != a->b);
    f->u = a->u; f->w = a->w; f->b = a->b; f->K = a->K;
    return 0;
}

}  // namespace

#define FL_CHECK_SHAPE(B, k, Z) \
    GM_CHECK_ARG((B) >= 1 && (k) >= 1 && (k) <= GM_IWAE_MAX_K && (Z) >= 1 && (Z) <= GM_IWAE_MAX_Z)

extern "C" int gm_flow_sample(void* stream, const gm_iwae_noise* a, const gm_flow_params* fp, const float* ml,
                              int64_t ldml, float* z, int64_t ldz, float* lp, int B, int k, int Z) {
    FL_CHECK_SHAPE(B, k, Z);
    GM_CHECK_ARG(ml && z && lp && ldml >= 2 * Z && ldz >= Z);
    GM_CHECK_ARG((const float*)z != ml && (const float*)lp != ml && lp != z);
    PhNoise n{};
    FlowW f{};
    int rc = ph_noise_fill(a, B, k, &n);
    if (rc) return rc;
    rc = fl_params_fill(fp, &f);
    if (rc) return rc;
    GM_CHECK_ARG(f.u != z && f.w != z && f.b != z && f.u != lp && f.w != lp && f.b != lp);
    SampleP p{ml, ldml, z, ldz, lp, (int64_t)B * k, k, Z};
    const int64_t blocks = (p.rows * 8 + 255) / 256;
    GM_CHECK_ARG(blocks < (1ll << 31));
    hipLaunchKernelGGL(flow_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, f, n);
    GM_LAUNCH_RET();
}

extern "C" int gm_flow_reduce(void* stream, const gm_iwae_noise* a, const gm_flow_params* fp, const float* ml,
                              int64_t ldml, const float* wn, const float* dzdec, int64_t lddz, float* dml,
                              int64_t lddml, float* part, int B, int k, int Z) {
    FL_CHECK_SHAPE(B, k, Z);
    GM_CHECK_ARG(ml && wn && dzdec && dml && part && ldml >= 2 * Z && lddz >= Z && lddml >= 2 * Z);
    GM_CHECK_ARG((const float*)dml != ml && (const float*)dml != dzdec && (const float*)dml != wn);
    GM_CHECK_ARG((const float*)part != ml && (const float*)part != dzdec && (const float*)part != wn && part != dml);
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(part) & 15) == 0);
    PhNoise n{};
    FlowW f{};
    int rc = ph_noise_fill(a, B, k, &n);
    if (rc) return rc;
    rc = fl_params_fill(fp, &f);
    if (rc) return rc;
    GM_CHECK_ARG(f.u != dml && f.w != dml && f.b != dml && f.u != part && f.w != part && f.b != part);
    ReduceP p{ml, ldml, wn, dzdec, lddz, dml, lddml, part, (int64_t)B, k, Z};
    hipLaunchKernelGGL(flow_reduce_kernel, dim3((unsigned)((B + 7) / 8)), dim3(64), 0, (hipStream_t)stream, p, f, n);
    GM_LAUNCH_RET();
}

extern "C" int gm_flow_step(void* stream, const gm_flow_step_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->K >= 1 && a->K <= GM_FLOW_MAX_K && a->Z >= 1 && a->Z <= GM_IWAE_MAX_Z && a->nparts >= 1);
    GM_CHECK_ARG(a->part && a->u && a->w && a->b && a->mu && a->vu && a->mw && a->vw && a->mb && a->vb && a->sched);
    GM_CHECK_ARG((a->gu && a->gw && a->gb) || (!a->gu && !a->gw && !a->gb));
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(a->part) & 15) == 0);
    const float* ptr[] = {a->part, a->u, a->w, a->b, a->gu, a->gw, a->gb, a->mu, a->vu, a->mw, a->vw, a->mb, a->vb};
    for (int i = 0; i < 13; ++i)
        for (int j = i + 1; j < 13; ++j) GM_CHECK_ARG(!ptr[i] || ptr[i] != ptr[j]);
    StepP p{a->part, a->nparts, a->u, a->w, a->b, a->gu, a->gw, a->gb, a->mu, a->vu, a->mw, a->vw, a->mb, a->vb,
            a->sched, a->sched_slot,
            (float)(1.0 - a->beta1), (float)a->beta2, (float)(1.0 - a->beta2), (float)a->eps, (float)a->weight_decay,
            a->K, a->Z};
    hipLaunchKernelGGL(flow_step_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
