// Importance-weighted autoencoder (iwae.py holds the contract; gm_hip.h).  k samples per image,
// rows image-major (sample j of image b is row b k + j).
//
// gm_iwae_sample: 8 lanes per sample row, lane q takes latents 4q .. 4q + 3 (one Philox call); z and the row's
//   lp = 1/2 sum_c (eps^2 - z^2 + lv), summed over the 8 lanes by a fixed butterfly.
// gm_iwae_weights: one 256-thread workgroup per image.  Pass 1: wave w takes the image's rows j = w, w + 4, ...; lane l
//   the elements l, l + 64, ... of (x - xr_j)^2 (quads where the rows allow 16-byte loads), then the wave butterfly.
//   The squares are summed and log w is kept in fp64: at log w ~ -150 one fp32 rounding of it (7.6e-6) would already be a
//   relative error of that size in every weight; the fp64 adds are 784 k per image, noise beside the loads.
//   Wave 0 then takes the softmax over the k values of log w with the maximum subtracted (typical log w is below -100:
//   the unshifted exp is 0 in fp32).  Pass 2 (training): all threads write dA = wn_j * d sq_j / d (pre-sigmoid) over
//   the flattened k x I block.  The rows stay in LDS between the passes while k I floats fit in 64 KB (the default
//   dynamic allocation; several workgroups still share a CU), else pass 2 reads them again (they are L2 hits).
// gm_iwae_reduce: one thread per (image, latent quad); j ascending; eps and z rebuilt from the counter and [mu | lv].
// No atomics, fixed reduction order: the same bits on every run, graph or eager.
#include "gm_philox.h"

namespace {

struct SampleP {
    const float* ml; int64_t ldml;
    float* z; int64_t ldz;
    float* lp;
    int64_t rows; int k, Z, nq;
};

__global__ __launch_bounds__(256) void iwae_sample_kernel(SampleP p, PhNoise n) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = gi >> 3;
    const int q = (int)(gi & 7);
    float acc = 0.f;
    if (r < p.rows && q < p.nq) {
        const int64_t b = r / p.k;
        const int j = (int)(r - b * p.k);
        float e[4];
        ph_noise_eps4(n, ph_step(n.clk), (uint32_t)(b * n.kt + n.j0 + j), (uint32_t)q, e);
        const float* ml = p.ml + b * p.ldml;
        float* zo = p.z + r * p.ldz;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * q + i;
            if (c < p.Z) {
                const float lv = ml[p.Z + c];
                const float z = gm_reparam_z(ml[c], e[i], lv);
                zo[c] = z;
                acc += 0.5f * (e[i] * e[i] - z * z + lv);
            }
        }
    }
    // the 8 lanes of a row (whole groups are inside or outside the array, so every lane of the wave arrives here)
    acc += __shfl_xor(acc, 4, 64);
    acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 1, 64);
    if (r < p.rows && q == 0) p.lp[r] = acc;
}

struct WeightsP {
    const float* x; int64_t ldx;
    const float* xr; int64_t ldr;
    const float* lp;
    float* negL; float* ess; float* wn;
    float* dA; int64_t lda;
    float* ms;
    int k, I, vec;
};

constexpr int IW_HEAD = 192;          // floats of LDS in front of the rows: log w [64] (fp64), wn [64]

template <bool LDS>
__global__ __launch_bounds__(256) void iwae_weights_kernel(WeightsP p) {
    extern __shared__ __attribute__((aligned(16))) float iw_sm[];
    double* lw = reinterpret_cast<double*>(iw_sm);
    float* wnS = iw_sm + 128;
    float* rows = iw_sm + IW_HEAD;
    const int64_t b = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = p.k, I = p.I;
    const float* x = p.x + b * p.ldx;
    const float* xr = p.xr + b * k * p.ldr;
    for (int j = wave; j < k; j += 4) {
        const float* r = xr + (int64_t)j * p.ldr;
        double acc = 0.0;
        if (p.vec) {
            const int nq = I >> 2;
            for (int q = lane; q < nq; q += 64) {
                const float4 a = reinterpret_cast<const float4*>(x)[q];
                const float4 v = reinterpret_cast<const float4*>(r)[q];
                if (LDS) reinterpret_cast<float4*>(rows)[j * nq + q] = v;
                const double d0 = a.x - v.x, d1 = a.y - v.y, d2 = a.z - v.z, d3 = a.w - v.w;
                acc = fma(d0, d0, acc);
                acc = fma(d1, d1, acc);
                acc = fma(d2, d2, acc);
                acc = fma(d3, d3, acc);
            }
        } else {
            for (int i = lane; i < I; i += 64) {
                const float v = r[i];
                if (LDS) rows[j * I + i] = v;
                const double d = x[i] - v;
                acc = fma(d, d, acc);
            }
        }
        acc = gm_wave_sum_d(acc);
        if (lane == 0) lw[j] = (double)p.lp[b * k + j] - acc;
    }
    __syncthreads();
    if (wave == 0) {
        const double v = lane < k ? lw[lane] : -(double)INFINITY;
        double m = v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
        const float e = lane < k ? expf((float)(v - m)) : 0.f;
        const float s = gm_wave_sum(e), s2 = gm_wave_sum(e * e);
        const float w = e / s;
        if (lane < k) {
            wnS[lane] = w;
            p.wn[b * k + lane] = w;
        }
        if (lane == 0) {
            p.negL[b] = (float)-(m + log((double)s) - log((double)k));
            p.ess[b] = (s * s) / s2;
            if (p.ms) {
                p.ms[2 * b] = (float)m;
                p.ms[2 * b + 1] = s;
            }
        }
    }
    if (!p.dA) return;
    __syncthreads();
    float* dA = p.dA + b * k * p.lda;
    if (p.vec) {
        const int nq = I >> 2;
        for (int idx = threadIdx.x; idx < k * nq; idx += 256) {
            const int j = idx / nq, q = idx - j * nq;
            const float4 a = reinterpret_cast<const float4*>(x)[q];
            const float4 v = LDS ? reinterpret_cast<const float4*>(rows)[idx]
                                 : reinterpret_cast<const float4*>(xr + (int64_t)j * p.ldr)[q];
            const float w = wnS[j];
            float4 o;
            o.x = w * (((-2.f * (a.x - v.x)) * (1.f - v.x)) * v.x);
            o.y = w * (((-2.f * (a.y - v.y)) * (1.f - v.y)) * v.y);
            o.z = w * (((-2.f * (a.z - v.z)) * (1.f - v.z)) * v.z);
            o.w = w * (((-2.f * (a.w - v.w)) * (1.f - v.w)) * v.w);
            reinterpret_cast<float4*>(dA + (int64_t)j * p.lda)[q] = o;
        }
    } else {
        for (int idx = threadIdx.x; idx < k * I; idx += 256) {
            const int j = idx / I, i = idx - j * I;
            const float v = LDS ? rows[idx] : xr[(int64_t)j * p.ldr + i];
            dA[(int64_t)j * p.lda + i] = wnS[j] * (((-2.f * (x[i] - v)) * (1.f - v)) * v);
        }
    }
}

struct ReduceP {
    const float* ml; int64_t ldml;
    const float* wn;
    const float* dzdec; int64_t lddz;
    float* dml; int64_t lddml;
    float* dZ; int64_t lddZ;
    int64_t B; int k, Z, nq;
};

__global__ __launch_bounds__(256) void iwae_reduce_kernel(ReduceP p, PhNoise n) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= p.B * p.nq) return;
    const int64_t b = gi / p.nq;
    const int q = (int)(gi - b * p.nq);
    const int Z = p.Z;
    const float* ml = p.ml + b * p.ldml;
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
        const int64_t r = b * p.k + j;
        float e[4];
        ph_noise_eps4(n, step, (uint32_t)(b * n.kt + n.j0 + j), (uint32_t)q, e);
        const float w = p.wn[r];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * q + i;
            if (c < Z) {
                const float dz = fmaf(w, gm_reparam_z(mu[i], e[i], lv[i]), p.dzdec[r * p.lddz + c]);
                if (p.dZ) p.dZ[r * p.lddZ + c] = dz;
                amu[i] += dz;
                alv[i] = fmaf(dz * e[i], sd[i], alv[i]);
            }
        }
    }
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

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

#define IW_CHECK_SHAPE(B, k, Z) \
    GM_CHECK_ARG((B) >= 1 && (k) >= 1 && (k) <= GM_IWAE_MAX_K && (Z) >= 1 && (Z) <= GM_IWAE_MAX_Z)

extern "C" int gm_iwae_sample(void* stream, const gm_iwae_noise* a, const float* ml, int64_t ldml, float* z,
                              int64_t ldz, float* lp, int B, int k, int Z) {
    IW_CHECK_SHAPE(B, k, Z);
    GM_CHECK_ARG(ml && z && lp && ldml >= 2 * Z && ldz >= Z);
    PhNoise n{};
    const int rc = ph_noise_fill(a, B, k, &n);
    if (rc) return rc;
    SampleP p{ml, ldml, z, ldz, lp, (int64_t)B * k, k, Z, (Z + 3) / 4};
    const int64_t blocks = (p.rows * 8 + 255) / 256;
    GM_CHECK_ARG(blocks < (1ll << 31));
    hipLaunchKernelGGL(iwae_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, n);
    GM_LAUNCH_RET();
}

extern "C" int gm_iwae_weights(void* stream, const float* x, int64_t ldx, const float* xr, int64_t ldr,
                               const float* lp, float* negL, float* ess, float* wn, float* dA, int64_t lda, float* ms,
                               int B, int k, int I) {
    IW_CHECK_SHAPE(B, k, 1);
    GM_CHECK_ARG(x && xr && lp && negL && ess && wn && I >= 1 && I <= (1 << 24) && ldx >= I && ldr >= I);
    GM_CHECK_ARG(!dA || (lda >= I && (const float*)dA != x && (const float*)dA != xr));
    const int vec = (I % 4 == 0 && ldx % 4 == 0 && ldr % 4 == 0 && al16(x) && al16(xr) &&
                     (!dA || (lda % 4 == 0 && al16(dA)))) ? 1 : 0;
    WeightsP p{x, ldx, xr, ldr, lp, negL, ess, wn, dA, lda, ms, k, I, vec};
    const size_t head = IW_HEAD * sizeof(float), full = head + (size_t)k * I * sizeof(float);
    if (dA && full <= 65536)
        hipLaunchKernelGGL(iwae_weights_kernel<true>, dim3((unsigned)B), dim3(256), full, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(iwae_weights_kernel<false>, dim3((unsigned)B), dim3(256), head, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_iwae_reduce(void* stream, const gm_iwae_noise* a, const float* ml, int64_t ldml, const float* wn,
                              const float* dzdec, int64_t lddz, float* dml, int64_t lddml, float* dZ, int64_t lddZ,
                              int B, int k, int Z) {
    IW_CHECK_SHAPE(B, k, Z);
    GM_CHECK_ARG(ml && wn && dzdec && dml && ldml >= 2 * Z && lddz >= Z && lddml >= 2 * Z);
    GM_CHECK_ARG(!dZ || (lddZ >= Z && (const float*)dZ != dzdec));
    PhNoise n{};
    const int rc = ph_noise_fill(a, B, k, &n);
    if (rc) return rc;
    ReduceP p{ml, ldml, wn, dzdec, lddz, dml, lddml, dZ, lddZ, (int64_t)B, k, Z, (Z + 3) / 4};
    const int64_t blocks = (p.B * p.nq + 255) / 256;
    hipLaunchKernelGGL(iwae_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, n);
    GM_LAUNCH_RET();
}
