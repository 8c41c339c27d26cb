// beta-TCVAE (tcvae.py holds the contract; gm_hip.h): the minibatch-weighted-sampling estimate of
// log q(z) and log prod_d q(z_d) over every pair (sample i, posterior j) of a batch, forward and backward, without a
// [B, B] or [B, B, Z] array.  With l'(i, j, d) = -1/2 (lv_jd + (z_id - mu_jd)^2 exp(-lv_jd)) (log N without its
// -1/2 log 2 pi, which cancels out of all three terms):
//   J_i = logsumexp_j sum_d l'(i, j, d)  (lse_joint)        D_id = logsumexp_j l'(i, j, d)  (lse_dim)
//
// Both kernels: 1024 threads, workgroup g owns rows 2 g and 2 g + 1, eight waves per row.  A tile of 64 partner rows is
// staged in LDS by the whole workgroup (exp(-lv) is formed there, once per partner and workgroup, never per pair); each of
// a row's waves takes an eighth of the tile, lane (d, h) = (lane & 31, lane >> 5) latent d of two partners per step.
// sum_d is a reduction over a half wave (tc_sum32); the sums over j are per-lane running values in ascending j, joined
// at the end by fixed butterflies and, across the row's waves, through LDS in ascending order: the same bits on every
// run, graph or eager.  Rows past B stage as -inf (their exponentials are exact zeros), latents past Z as exact zeros of
// sum_d.  The kernels are latency-bound (DESIGN.md section 33 has the measurements behind the mapping).
//
// gm_tc_sample: one pass over the partners with a running logsumexp (m, s) <- exp(l): one exponential per element,
//   exp(-|l - m|), the maximum always subtracted.  The joint sums of a tile's 32 steps are parked one per lane and join
//   the running value once per tile, so the joint costs one exponential per pair, not 32.
// gm_tc_reduce: row r as sample (dz_r over the partners) and as posterior (dmu_r, dlv_r over the samples, z read from
//   Zs) in the same pass, then the reparameterisation with eps rebuilt from the counter.
// No atomics, no scratch.
#include "gm_philox.h"

namespace {

constexpr int TC_TILE = 64;                 // rows staged per tile
constexpr int TC_ROWS = 2;                  // owner rows per workgroup
constexpr int TC_WPR = 8;                   // waves per owner row: wave w is share w % 8 of row w / 8
constexpr int TC_THREADS = 64 * TC_ROWS * TC_WPR;
constexpr int TC_STEPS = TC_TILE / 2 / TC_WPR;      // steps of a wave per tile (two partners per step)
constexpr int TC_ZP = 32;                   // lanes per row of a tile (GM_IWAE_MAX_Z)
constexpr int TC_TILE_N = TC_TILE * TC_ZP;
constexpr float TC_LOW = -3.0e38f;          // a running maximum before its first term (finite: LOW - LOW is 0, not NaN)

static_assert(TC_ZP == GM_IWAE_MAX_Z, "a latent per lane of a half wave");

// The sum over a half wave (32 lanes), the same bits in every lane.  It sits in the dependent chain of every step of
// both kernels: four DPP adds inside a row of 16 (lane ^ 1, lane ^ 2, mirrored halves of 8, mirrored row) and one
// swizzle across the two rows; five ds_bpermute round trips in its place cost 22 % (sample) and 31 % (reduce) more (one wave per row).
// Every lane of the wave is active wherever this is called (the callers' branches are wave-uniform).
template <int CTRL>
__device__ __forceinline__ float tc_dpp(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

__device__ __forceinline__ float tc_sum32(float v) {
    v += tc_dpp<0xB1>(v);                                   // quad_perm [1, 0, 3, 2]
    v += tc_dpp<0x4E>(v);                                   // quad_perm [2, 3, 0, 1]
    v += tc_dpp<0x141>(v);                                  // row_half_mirror
    v += tc_dpp<0x140>(v);                                  // row_mirror
    v += __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401F));   // lane ^ 16 inside 32 lanes
    return v;
}

// l'(i, j, d) from z_id - mu_jd, exp(-lv_jd) and -lv_jd / 2.  One body for every site: gm_tc_reduce meets the pair
// (r, r) in both of its roles, and only equal bits there let its two contributions to d mu_r cancel as they do in exact
// arithmetic (with different roundings of the same l the error of a_rr, times (z - mu) / sigma^2, stays in dml).
__device__ __forceinline__ float tc_l(float dz, float iv, float hl) {
#pragma clang fp contract(off)
    const float q = (dz * dz) * iv;
    return hl - 0.5f * q;
}

// (m, s) <- (m, s) + exp(l), s relative to the running maximum m
__device__ __forceinline__ void tc_lse_add(float& m, float& s, float l) {
    const float e = expf(-fabsf(l - m));
    const bool up = l > m;
    s = up ? fmaf(s, e, 1.f) : s + e;
    m = up ? l : m;
}

// (m, s) <- (m, s) + (m2, s2); both lanes of an exchange get the same bits
__device__ __forceinline__ void tc_lse_merge(float& m, float& s, float m2, float s2) {
#pragma clang fp contract(off)
    const float M = fmaxf(m, m2);
    const float a = s * expf(m - M);
    const float b = s2 * expf(m2 - M);
    s = a + b;
    m = M;
}

struct TcSampleP {
    const float* ml; int64_t ldml;
    float* z; int64_t ldz;
    float* lp; float* lsej; float* lsed; int64_t ldd; float* tc; float* terms;
    float alpha, beta, gamma, lognm;
    int B, Z;
};

__global__ __launch_bounds__(TC_THREADS) void tc_sample_kernel(TcSampleP p, PhNoise n) {
    __shared__ float smu[TC_TILE_N], shl[TC_TILE_N], siv[TC_TILE_N];
    __shared__ float xmd[TC_ROWS][TC_WPR][TC_ZP], xsd[TC_ROWS][TC_WPR][TC_ZP], xmj[TC_ROWS][TC_WPR], xsj[TC_ROWS][TC_WPR];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, d = lane & 31, h = lane >> 5;
    const int row = wave / TC_WPR, sub = wave % TC_WPR;
    const int Z = p.Z, B = p.B;
    const int i = blockIdx.x * TC_ROWS + row;
    const bool own = i < B, live = own && d < Z;
    float zi = 0.f, ei = 0.f, lvi = 0.f;
    if (live) {
        float e[4];
        ph_noise_eps4(n, ph_step(n.clk), (uint32_t)((int64_t)i * n.kt + n.j0), (uint32_t)(d >> 2), e);
        const int c = d & 3;
        ei = c == 0 ? e[0] : c == 1 ? e[1] : c == 2 ? e[2] : e[3];
        const float* ml = p.ml + (int64_t)i * p.ldml;
        lvi = ml[Z + d];
        zi = gm_reparam_z(ml[d], ei, lvi);
        if (h == 0 && sub == 0) p.z[(int64_t)i * p.ldz + d] = zi;
    }
    float md = TC_LOW, sd = 0.f, mj = TC_LOW, sj = 0.f;
    for (int j0 = 0; j0 < B; j0 += TC_TILE) {
        __syncthreads();                                     // the previous tile has been read
        for (int idx = threadIdx.x; idx < TC_TILE_N; idx += TC_THREADS) {
            const int j = j0 + (idx >> 5), c = idx & 31;
            float mu = 0.f, hl = 0.f, iv = 0.f;
            if (c < Z) {
                if (j < B) {
                    const float* r = p.ml + (int64_t)j * p.ldml;
                    const float lv = r[Z + c];
                    mu = r[c];
                    hl = -0.5f * lv;
                    iv = expf(-lv);
                } else {
                    hl = -INFINITY;
                }
            }
            smu[idx] = mu; shl[idx] = hl; siv[idx] = iv;
        }
        __syncthreads();
        if (!own) continue;                                  // wave-uniform; the barriers stay outside
        float keep = -INFINITY;                              // lane (d, h), d < TC_STEPS, parks the joint sum of step d
#pragma unroll 4
        for (int s = 0; s < TC_STEPS; ++s) {
            const int t = (2 * (sub * TC_STEPS + s) + h) * TC_ZP + d;
            const float dz = zi - smu[t];
            const float l = tc_l(dz, siv[t], shl[t]);
            tc_lse_add(md, sd, l);
            const float S = tc_sum32(l);
            keep = s == d ? S : keep;
        }
        tc_lse_add(mj, sj, keep);
    }
    // a wave's share: its two halves, then its lanes; the row's shares meet in LDS and join in ascending order
    tc_lse_merge(md, sd, __shfl_xor(md, 32, 64), __shfl_xor(sd, 32, 64));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tc_lse_merge(mj, sj, __shfl_xor(mj, o, 64), __shfl_xor(sj, o, 64));
    if (h == 0) {
        xmd[row][sub][d] = md;
        xsd[row][sub][d] = sd;
    }
    if (lane == 0) {
        xmj[row][sub] = mj;
        xsj[row][sub] = sj;
    }
    __syncthreads();
    if (!own || sub != 0) return;
#pragma unroll
    for (int w = 1; w < TC_WPR; ++w) {
        tc_lse_merge(md, sd, xmd[row][w][d], xsd[row][w][d]);
        tc_lse_merge(mj, sj, xmj[row][w], xsj[row][w]);
    }
    const float D = md + logf(sd);
    const float J = mj + logf(sj);
    const float qx = tc_sum32(live ? -0.5f * (lvi + ei * ei) : 0.f);      // log q(z_i | x_i) + Z/2 log 2 pi
    const float pz = tc_sum32(live ? -0.5f * zi * zi : 0.f);             // log p(z_i) + Z/2 log 2 pi
    const float Ds = tc_sum32(d < Z ? D : 0.f);
    if (live && h == 0) p.lsed[(int64_t)i * p.ldd + d] = D;
    if (lane == 0) {
        const float L = p.lognm;
        const float mi = (qx - J) + L;
        const float tc = (J - Ds) + (float)(Z - 1) * L;
        const float dw = (Ds - (float)Z * L) - pz;
        p.lsej[i] = J;
        p.tc[i] = tc;
        // the three terms' shares of L joined first: alpha + (Z - 1) beta - Z gamma is small (0 at Z = 1 with alpha =
        // gamma) where each share is not, and lp keeps the digits the shares would cost it
        const float cL = (p.alpha + (float)(Z - 1) * p.beta) - (float)Z * p.gamma;
        p.lp[i] = -(((p.alpha * (qx - J) + p.beta * (J - Ds)) + p.gamma * (Ds - pz)) + cL * L);
        if (p.terms) {
            p.terms[3 * (int64_t)i] = mi;
            p.terms[3 * (int64_t)i + 1] = tc;
            p.terms[3 * (int64_t)i + 2] = dw;
        }
    }
}

struct TcReduceP {
    const float* ml; int64_t ldml;
    const float* z; int64_t ldz;
    const float* lsej; const float* lsed; int64_t ldd;
    const float* wn;
    const float* dzdec; int64_t lddz;
    float* dml; int64_t lddml;
    float alpha, beta, gamma;
    int B, Z;
};

__global__ __launch_bounds__(TC_THREADS) void tc_reduce_kernel(TcReduceP p, PhNoise n) {
    __shared__ float smu[TC_TILE_N], shl[TC_TILE_N], siv[TC_TILE_N], sz[TC_TILE_N], sD[TC_TILE_N];
    __shared__ float sJ[TC_TILE], sw[TC_TILE];
    __shared__ float xaz[TC_ROWS][TC_WPR][TC_ZP], xamu[TC_ROWS][TC_WPR][TC_ZP], xalv[TC_ROWS][TC_WPR][TC_ZP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, d = lane & 31, h = lane >> 5;
    const int row = wave / TC_WPR, sub = wave % TC_WPR;
    const int Z = p.Z, B = p.B;
    const int r = blockIdx.x * TC_ROWS + row;
    const bool own = r < B, live = own && d < Z;
    // the owner's row in both roles; a latent past Z adds an exact 0 to sum_d and has coefficient 0
    float zr = 0.f, mur = 0.f, lvr = 0.f, hlr = 0.f, ivr = 0.f, Dr = INFINITY, Jr = 0.f, wr = 0.f;
    if (own) {
        Jr = p.lsej[r];
        wr = p.wn[r];
    }
    if (live) {
        const float* ml = p.ml + (int64_t)r * p.ldml;
        mur = ml[d];
        lvr = ml[Z + d];
        hlr = -0.5f * lvr;
        ivr = expf(-lvr);
        zr = p.z[(int64_t)r * p.ldz + d];
        Dr = p.lsed[(int64_t)r * p.ldd + d];
    }
    const float ca = p.beta - p.alpha, cc = p.gamma - p.beta;
    float az = 0.f, amu = 0.f, alv = 0.f;
    for (int j0 = 0; j0 < B; j0 += TC_TILE) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < TC_TILE_N; idx += TC_THREADS) {
            const int j = j0 + (idx >> 5), c = idx & 31;
            float mu = 0.f, hl = 0.f, iv = 0.f, zz = 0.f, DD = INFINITY;
            if (c < Z) {
                if (j < B) {
                    const float* q = p.ml + (int64_t)j * p.ldml;
                    const float lv = q[Z + c];
                    mu = q[c];
                    hl = -0.5f * lv;
                    iv = expf(-lv);
                    zz = p.z[(int64_t)j * p.ldz + c];
                    DD = p.lsed[(int64_t)j * p.ldd + c];
                } else {
                    hl = -INFINITY;
                }
            }
            smu[idx] = mu; shl[idx] = hl; siv[idx] = iv; sz[idx] = zz; sD[idx] = DD;
        }
        if (threadIdx.x < TC_TILE) {
            const int j = j0 + (int)threadIdx.x;
            sJ[threadIdx.x] = j < B ? p.lsej[j] : INFINITY;
            sw[threadIdx.x] = j < B ? p.wn[j] : 0.f;
        }
        __syncthreads();
        if (!own) continue;
#pragma unroll 2
        for (int s = 0; s < TC_STEPS; ++s) {
            const int t = 2 * (sub * TC_STEPS + s) + h, o = t * TC_ZP + d;
            // row r as the sample, row j0 + t as the posterior
            const float dA = zr - smu[o], ivA = siv[o];
            const float lA = tc_l(dA, ivA, shl[o]);
            const float SA = tc_sum32(lA);
            const float wA = wr * (ca * expf(SA - Jr) + cc * expf(lA - Dr));
            az = fmaf(wA, -(dA * ivA), az);
            // row j0 + t as the sample, row r as the posterior
            const float dB = sz[o] - mur;
            const float qB = (dB * dB) * ivr;
            const float lB = tc_l(dB, ivr, hlr);
            const float SB = tc_sum32(lB);
            const float wB = sw[t] * (ca * expf(SB - sJ[t]) + cc * expf(lB - sD[o]));
            amu = fmaf(wB, dB * ivr, amu);
            alv = fmaf(wB, 0.5f * (qB - 1.f), alv);
        }
    }
    // a wave's share: its two halves; the row's shares meet in LDS and are added in ascending order
    az += __shfl_xor(az, 32, 64);
    amu += __shfl_xor(amu, 32, 64);
    alv += __shfl_xor(alv, 32, 64);
    if (h == 0) {
        xaz[row][sub][d] = az;
        xamu[row][sub][d] = amu;
        xalv[row][sub][d] = alv;
    }
    __syncthreads();
    if (live && h == 0 && sub == 0) {
#pragma unroll
        for (int w = 1; w < TC_WPR; ++w) {
            az += xaz[row][w][d];
            amu += xamu[row][w][d];
            alv += xalv[row][w][d];
        }
        float e[4];
        ph_noise_eps4(n, ph_step(n.clk), (uint32_t)((int64_t)r * n.kt + n.j0), (uint32_t)(d >> 2), e);
        const int c = d & 3;
        const float er = c == 0 ? e[0] : c == 1 ? e[1] : c == 2 ? e[2] : e[3];
        // d (-lp_r) / d z_r = the pair terms + gamma z_r (the prior); the alpha term's own derivatives cancel through
        // the reparameterisation except for -alpha / 2 on lv
        const float dz = fmaf(wr * p.gamma, zr, az) + p.dzdec[(int64_t)r * p.lddz + d];
        float* o = p.dml + (int64_t)r * p.lddml;
        o[d] = amu + dz;
        o[Z + d] = fmaf(0.5f * (dz * er), expf(lvr / 2.f), alv) - 0.5f * p.alpha * wr;
    }
}

inline bool tc_coef_ok(float a, float b, float g) {
    return a >= 0.f && b >= 0.f && g >= 0.f && a <= 3.0e38f && b <= 3.0e38f && g <= 3.0e38f;   // (NaN fails >=)
}

}  // namespace

#define TC_CHECK_SHAPE(B, k, Z) GM_CHECK_ARG((B) >= 1 && (k) == 1 && (Z) >= 1 && (Z) <= GM_IWAE_MAX_Z)

extern "C" int gm_tc_sample(void* stream, const gm_iwae_noise* a, const float* ml, int64_t ldml, float* z, int64_t ldz,
                            float* lp, float* lse_joint, float* lse_dim, int64_t ldd, float* tc, float* terms,
                            float alpha, float beta, float gamma, float log_nm, int B, int k, int Z) {
    TC_CHECK_SHAPE(B, k, Z);
    GM_CHECK_ARG(ml && z && lp && lse_joint && lse_dim && tc && ldml >= 2 * Z && ldz >= Z && ldd >= Z);
    GM_CHECK_ARG(tc_coef_ok(alpha, beta, gamma) && log_nm == log_nm);
    // every output is an array of its own, and none is the input
    const void* outs[7] = {z, lp, lse_joint, lse_dim, tc, terms, ml};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j) GM_CHECK_ARG(!outs[i] || outs[i] != outs[j]);
    PhNoise n{};
    const int rc = ph_noise_fill(a, B, 1, &n);
    if (rc) return rc;
    TcSampleP p{ml, ldml, z, ldz, lp, lse_joint, lse_dim, ldd, tc, terms, alpha, beta, gamma, log_nm, B, Z};
    const unsigned blocks = (unsigned)((B + TC_ROWS - 1) / TC_ROWS);
    hipLaunchKernelGGL(tc_sample_kernel, dim3(blocks), dim3(TC_THREADS), 0, (hipStream_t)stream, p, n);
    GM_LAUNCH_RET();
}

extern "C" int gm_tc_reduce(void* stream, const gm_iwae_noise* a, const float* ml, int64_t ldml, const float* z,
                            int64_t ldz, const float* lse_joint, const float* lse_dim, int64_t ldd, const float* wn,
                            const float* dzdec, int64_t lddz, float* dml, int64_t lddml, float alpha, float beta,
                            float gamma, int B, int k, int Z) {
    TC_CHECK_SHAPE(B, k, Z);
    GM_CHECK_ARG(ml && z && lse_joint && lse_dim && wn && dzdec && dml);
    GM_CHECK_ARG(ldml >= 2 * Z && ldz >= Z && ldd >= Z && lddz >= Z && lddml >= 2 * Z);
    GM_CHECK_ARG(tc_coef_ok(alpha, beta, gamma));
    const void* ins[6] = {ml, z, lse_joint, lse_dim, wn, dzdec};
    for (int i = 0; i < 6; ++i) GM_CHECK_ARG(ins[i] != (const void*)dml);      // other rows' inputs are read late
    PhNoise n{};
    const int rc = ph_noise_fill(a, B, 1, &n);
    if (rc) return rc;
    TcReduceP p{ml, ldml, z, ldz, lse_joint, lse_dim, ldd, wn, dzdec, lddz, dml, lddml, alpha, beta, gamma, B, Z};
    const unsigned blocks = (unsigned)((B + TC_ROWS - 1) / TC_ROWS);
    hipLaunchKernelGGL(tc_reduce_kernel, dim3(blocks), dim3(TC_THREADS), 0, (hipStream_t)stream, p, n);
    GM_LAUNCH_RET();
}
