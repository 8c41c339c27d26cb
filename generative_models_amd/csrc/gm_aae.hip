// Adversarial autoencoder's regularization phase (aae.py; gm_hip.h): the latent critic D: z (Z) -> H (relu) -> 1
// (sigmoid) on 2B rows with its own Adam step, and the generator phase's narrow backward into the encoder.
//
// gm_aae_critic_step = two launches.
//   rows:    one workgroup per 16 of the 2B rows (the B prior rows first, then the B encoder rows).  Each thread owns
//            hidden columns t and t + 256: h = relu(W1 z + b1) over the block's rows into LDS, its share of every row's
//            logit w2.h; the logits are added wave by wave in wave order, s = sigmoid(logit + b2), the row's loss term
//            and d loss / d logit as ns_gan.py's discriminator loss with the 1e-8 terms.  The thread then adds its
//            columns' dW1 / db1 / dw2 over the block's rows in ascending order and the workgroup writes them as its
//            partial (db2: thread 0) -- a [nblk][P] workspace, P = H Z + 2 H + 1, plus the 2B per-row loss terms.
//   combine: one thread per parameter element adds the nblk partials in workgroup order, writes the gradient and
//            steps Adam (torch's update, weight decay folded into the gradient) with the schedule row of the batch;
//            workgroup 0 also adds the 2B loss terms in fp64 (fixed order) and writes the mean.
//   No atomics anywhere: the same bits on every run, in a graph or not.  Two launches rather than one with a
//   last-arrival combine: the combine reads every partial once whichever way, and the second launch keeps the
//   rows kernel free of the cross-workgroup release/acquire protocol.
//
// gm_aae_gen_mid = one launch, one workgroup per 16 rows: D (already stepped) on the encoder's z rows, s, the row's
//   term -log(s + 1e-8), dlogit = d(-mean log(s + 1e-8)) / d logit, dh = dlogit w2 . [h > 0] (LDS),
//   dz = dh W1 (Z wide, four accumulators over the hidden columns added in a fixed order), and
//   dHe = (dz Wz) . [He > 0] (H wide) -- the inputs of the encoder's paired weight-gradient launch that follows.
#include "gm_common.h"

namespace {

constexpr int AAE_ROWS = 16;
constexpr int AAE_MAXH = 512;
constexpr int AAE_MAXZ = 32;

__host__ __device__ inline int64_t aae_align4(int64_t n) { return (n + 3) & ~int64_t(3); }
__host__ __device__ inline int64_t aae_params(int Z, int H) { return (int64_t)H * Z + 2 * (int64_t)H + 1; }
inline int aae_blocks(int rows) { return (rows + AAE_ROWS - 1) / AAE_ROWS; }

// h = relu(W1 z + b1) of the block's rows into sh (columns t, t + 256), and every row's logit share of this thread.
__device__ __forceinline__ void aae_hidden(const float* __restrict__ W1, const float* __restrict__ b1,
                                           const float* __restrict__ w2, const float (*sz)[AAE_MAXZ + 1],
                                           float (*sh)[AAE_MAXH], float* lp, int Z, int H) {
#pragma unroll
    for (int r = 0; r < AAE_ROWS; ++r) lp[r] = 0.f;
    for (int c = 0; c < 2; ++c) {
        const int n = threadIdx.x + 256 * c;
        if (n >= H) break;
        float w[AAE_MAXZ];
#pragma unroll
        for (int k = 0; k < AAE_MAXZ; ++k) w[k] = k < Z ? W1[(int64_t)n * Z + k] : 0.f;
        const float bb = b1[n], ww = w2[n];
#pragma unroll
        for (int r = 0; r < AAE_ROWS; ++r) {
            float a = 0.f;
#pragma unroll
            for (int k = 0; k < AAE_MAXZ; ++k)
                if (k < Z) a = fmaf(w[k], sz[r][k], a);
            const float hv = fmaxf(a + bb, 0.f);
            sh[r][n] = hv;
            lp[r] = fmaf(ww, hv, lp[r]);
        }
    }
}

// The block's logits: per-row wave sums, the four waves added in order (red: [4][AAE_ROWS] of LDS).  After the
// barrier red[0][r] holds row r's logit without b2.
__device__ __forceinline__ void aae_logits(float* lp, float (*red)[AAE_ROWS]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < AAE_ROWS; ++r) {
        const float v = gm_wave_sum(lp[r]);
        if (lane == 0) red[w][r] = v;
    }
    __syncthreads();
    if (threadIdx.x < AAE_ROWS) {
        const int r = threadIdx.x;
        red[0][r] = ((red[0][r] + red[1][r]) + red[2][r]) + red[3][r];
    }
    __syncthreads();
}

__device__ __forceinline__ void aae_load_rows(float (*sz)[AAE_MAXZ + 1], const float* __restrict__ zr,
                                              const float* __restrict__ zf, int64_t ldf, int i0, int nreal,
                                              int ntot, int Z) {
    for (int o = threadIdx.x; o < AAE_ROWS * Z; o += 256) {
        const int r = o / Z, k = o - r * Z, i = i0 + r;
        float v = 0.f;
        if (i < ntot) v = i < nreal ? zr[(int64_t)i * Z + k] : zf[(int64_t)(i - nreal) * ldf + k];
        sz[r][k] = v;
    }
}

struct CriticP {
    gm_aae_critic_args a;
    int nblk;
    int64_t P, P4;
};

__global__ __launch_bounds__(256) void aae_critic_rows_kernel(CriticP p) {
    __shared__ float sz[AAE_ROWS][AAE_MAXZ + 1];
    __shared__ float sh[AAE_ROWS][AAE_MAXH];
    __shared__ float red[4][AAE_ROWS];
    __shared__ float sdl[AAE_ROWS];
    const gm_aae_critic_args& a = p.a;
    const int Z = a.Z, H = a.H, B = a.B, t = threadIdx.x;
    const int i0 = blockIdx.x * AAE_ROWS;
    aae_load_rows(sz, a.z_real + gm_slot_offset(a.real_slot), a.z_fake, a.ld_fake, i0, B, 2 * B, Z);
    __syncthreads();
    float lp[AAE_ROWS];
    aae_hidden(a.W1, a.b1, a.w2, sz, sh, lp, Z, H);
    aae_logits(lp, red);
    float* rowloss = a.ws + p.nblk * p.P4;
    if (t < AAE_ROWS) {
        const int i = i0 + t;
        float dl = 0.f;
        if (i < 2 * B) {
            const float s = gm_sigmoid(red[0][t] + a.b2[0]);
            const float ib = 1.f / (float)B;
            float l;
            if (i < B) {                           // log(D(z_real) + 1e-8)
                const float u = s + EPS;
                l = -logf(u);
                dl = (-ib) / u;
            } else {                               // log(1 - D(z_fake) + 1e-8)
                const float u = (1.f - s) + EPS;
                l = -logf(u);
                dl = ib / u;
            }
            dl = (dl * (1.f - s)) * s;             // SigmoidBackward
            rowloss[i] = l;
        }
        sdl[t] = dl;
    }
    __syncthreads();
    float* part = a.ws + (int64_t)blockIdx.x * p.P4;
    const int64_t HZ = (int64_t)H * Z;
    for (int c = 0; c < 2; ++c) {
        const int n = t + 256 * c;
        if (n >= H) break;
        const float ww = a.w2[n];
        float acc[AAE_MAXZ];
#pragma unroll
        for (int k = 0; k < AAE_MAXZ; ++k) acc[k] = 0.f;
        float gb = 0.f, gw = 0.f;
#pragma unroll
        for (int r = 0; r < AAE_ROWS; ++r) {
            const float hv = sh[r][n], dl = sdl[r];
            const float dA = hv > 0.f ? dl * ww : 0.f;
            gb += dA;
            gw = fmaf(dl, hv, gw);
#pragma unroll
            for (int k = 0; k < AAE_MAXZ; ++k)
                if (k < Z) acc[k] = fmaf(dA, sz[r][k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < AAE_MAXZ; ++k)
            if (k < Z) part[(int64_t)n * Z + k] = acc[k];
        part[HZ + n] = gb;
        part[HZ + H + n] = gw;
    }
    if (t == 0) {
        float g = 0.f;
        for (int r = 0; r < AAE_ROWS; ++r) g += sdl[r];
        part[HZ + 2 * H] = g;
    }
}

__global__ __launch_bounds__(256) void aae_critic_combine_kernel(CriticP p) {
    __shared__ double sl[4];
    const gm_aae_critic_args& a = p.a;
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t HZ = (int64_t)a.H * a.Z;
    if (j < p.P) {
        float g = 0.f;
        for (int w = 0; w < p.nblk; ++w) g += a.ws[(int64_t)w * p.P4 + j];
        float *P, *G, *Mm, *V;
        int64_t o;
        if (j < HZ) { P = a.W1; G = a.gW1; Mm = a.mW1; V = a.vW1; o = j; }
        else if (j < HZ + a.H) { P = a.b1; G = a.gb1; Mm = a.mb1; V = a.vb1; o = j - HZ; }
        else if (j < HZ + 2 * a.H) { P = a.w2; G = a.gw2; Mm = a.mw2; V = a.vw2; o = j - HZ - a.H; }
        else { P = a.b2; G = a.gb2; Mm = a.mb2; V = a.vb2; o = 0; }
        if (G) G[o] = g;
        if (a.sched) {
            const int64_t si = gm_slot_index(a.sched_slot);
            const float step_size = a.sched[2 * si], bc2_sqrt = a.sched[2 * si + 1];
            float pp = P[o], mm = Mm[o], vv = V[o];
            adam_update(pp, g, mm, vv, step_size, bc2_sqrt, (float)(1.0 - a.beta1), (float)a.beta2,
                        (float)(1.0 - a.beta2), (float)a.eps, (float)a.weight_decay, 0.f);
            P[o] = pp; Mm[o] = mm; V[o] = vv;
        }
    }
    if (blockIdx.x != 0 || !a.loss_out) return;     // (block-uniform)
    const float* rowloss = a.ws + p.nblk * p.P4;
    double s = 0.0;
    for (int i = threadIdx.x; i < 2 * a.B; i += 256) s += (double)rowloss[i];
    s = gm_wave_sum_d(s);
    if ((threadIdx.x & 63) == 0) sl[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        a.loss_out[gm_slot_index(a.loss_slot)] = (float)((((sl[0] + sl[1]) + sl[2]) + sl[3]) / (double)a.B);
}

__global__ __launch_bounds__(256) void aae_gen_mid_kernel(gm_aae_gen_args a) {
    __shared__ float sz[AAE_ROWS][AAE_MAXZ + 1];
    __shared__ float sh[AAE_ROWS][AAE_MAXH];
    __shared__ float red[4][AAE_ROWS];
    __shared__ float sdl[AAE_ROWS];
    __shared__ float sdz[AAE_ROWS][AAE_MAXZ + 1];
    const int Z = a.Z, H = a.H, B = a.B, t = threadIdx.x;
    const int m0 = blockIdx.x * AAE_ROWS;
    aae_load_rows(sz, a.z, a.z, a.ldz, m0, 0, B, Z);
    __syncthreads();
    float lp[AAE_ROWS];
    aae_hidden(a.W1, a.b1, a.w2, sz, sh, lp, Z, H);
    aae_logits(lp, red);
    if (t < AAE_ROWS) {
        const int m = m0 + t;
        float dl = 0.f;
        if (m < B) {                               // -mean(log(D(encoder(x)) + 1e-8))
            const float s = gm_sigmoid(red[0][t] + a.b2[0]);
            const float u = s + EPS;
            a.loss_part[m] = -logf(u);
            dl = (-(1.f / (float)B)) / u;
            dl = (dl * (1.f - s)) * s;
        }
        sdl[t] = dl;
    }
    __syncthreads();
    for (int c = 0; c < 2; ++c) {                  // dh = dlogit w2 . [h > 0], in place (each thread its columns)
        const int n = t + 256 * c;
        if (n >= H) break;
        const float ww = a.w2[n];
#pragma unroll
        for (int r = 0; r < AAE_ROWS; ++r) sh[r][n] = sh[r][n] > 0.f ? sdl[r] * ww : 0.f;
    }
    __syncthreads();
    // dz = dh W1: one (row, k) per thread and pass, hidden columns in four interleaved accumulators
    for (int o = t; o < AAE_ROWS * Z; o += 256) {
        const int r = o / Z, k = o - r * Z;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        int n = 0;
        for (; n + 4 <= H; n += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = fmaf(sh[r][n + u], a.W1[(int64_t)(n + u) * Z + k], acc[u]);
        }
        for (int u = 0; n < H; ++n, ++u) acc[u] = fmaf(sh[r][n], a.W1[(int64_t)n * Z + k], acc[u]);
        const float v = (acc[0] + acc[1]) + (acc[2] + acc[3]);
        sdz[r][k] = v;
        if (m0 + r < B) a.dz[(int64_t)(m0 + r) * a.lddz + k] = v;
    }
    __syncthreads();
    // dHe = (dz Wz) . [He > 0]
    for (int c = 0; c < 2; ++c) {
        const int n = t + 256 * c;
        if (n >= H) break;
        float wz[AAE_MAXZ];
#pragma unroll
        for (int k = 0; k < AAE_MAXZ; ++k) wz[k] = k < Z ? a.Wz[(int64_t)k * H + n] : 0.f;
        for (int r = 0; r < AAE_ROWS; ++r) {
            const int m = m0 + r;
            if (m >= B) break;
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < AAE_MAXZ; ++k)
                if (k < Z) v = fmaf(sdz[r][k], wz[k], v);
            a.dHe[(int64_t)m * a.lddhe + n] = a.He[(int64_t)m * a.ldhe + n] > 0.f ? v : 0.f;
        }
    }
}

bool aae_shape_ok(int B, int Z, int H) {
    return B > 0 && Z > 0 && Z <= AAE_MAXZ && Z % 4 == 0 && H > 0 && H <= AAE_MAXH;
}

}  // namespace

extern "C" int64_t gm_aae_critic_workspace_bytes(int B, int Z, int H) {
    if (!aae_shape_ok(B, Z, H)) return -1;
    return (int64_t)4 * ((int64_t)aae_blocks(2 * B) * aae_align4(aae_params(Z, H)) + aae_align4(2 * (int64_t)B));
}

extern "C" int gm_aae_critic_step(void* stream, const gm_aae_critic_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(aae_shape_ok(a->B, a->Z, a->H) && (int64_t)a->B * 2 < (1ll << 30));
    GM_CHECK_ARG(a->z_real && a->z_fake && a->ld_fake >= a->Z && a->W1 && a->b1 && a->w2 && a->b2 && a->ws);
    GM_CHECK_ARG(a->ws_bytes >= gm_aae_critic_workspace_bytes(a->B, a->Z, a->H));
    const bool grads = a->gW1 || a->gb1 || a->gw2 || a->gb2;
    GM_CHECK_ARG(!grads || (a->gW1 && a->gb1 && a->gw2 && a->gb2));
    GM_CHECK_ARG(grads || a->sched);
    GM_CHECK_ARG(!a->sched || (a->mW1 && a->vW1 && a->mb1 && a->vb1 && a->mw2 && a->vw2 && a->mb2 && a->vb2));
    CriticP p{};
    p.a = *a;
    p.nblk = aae_blocks(2 * a->B);
    p.P = aae_params(a->Z, a->H);
    p.P4 = aae_align4(p.P);
    hipLaunchKernelGGL(aae_critic_rows_kernel, dim3(p.nblk), dim3(256), 0, (hipStream_t)stream, p);
    hipLaunchKernelGGL(aae_critic_combine_kernel, dim3((unsigned)((p.P + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_aae_gen_mid(void* stream, const gm_aae_gen_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(aae_shape_ok(a->B, a->Z, a->H));
    GM_CHECK_ARG(a->z && a->ldz >= a->Z && a->He && a->ldhe >= a->H && a->W1 && a->b1 && a->w2 && a->b2 && a->Wz);
    GM_CHECK_ARG(a->dz && a->lddz >= a->Z && a->dHe && a->lddhe >= a->H && a->loss_part);
    GM_CHECK_ARG((const float*)a->dHe != a->He && (const float*)a->dz != a->z);
    hipLaunchKernelGGL(aae_gen_mid_kernel, dim3(aae_blocks(a->B)), dim3(256), 0, (hipStream_t)stream, *a);
    GM_LAUNCH_RET();
}
