// Sliced Wasserstein distance (swg.py holds the contract): for each of P unit directions the
// projections a [N] of the generated rows and b [M] of the data rows are sorted and matched by rank,
//   W_p = (1 / (N M)) sum_ij w_ij (a_(i) - b_(j))^2,   w_ij = max(0, min((i+1) M, (j+1) N) - max(i M, j N)),
// the squared 2-Wasserstein distance of the two empirical measures on the line (w_ii = N when N = M).
//
//   sw_directions_kernel  one workgroup per direction: the row's Philox normals (gm_philox.h) through LDS, their squares
//                         summed in fp64 in a fixed order, the row scaled to unit 2-norm (a zero row stays zero);
//   sw_sort_kernel        one workgroup per projection: both columns in LDS, padded to a power of two with elements that
//                         compare above every real one, sorted by a bitonic compare-exchange network on (value, row)
//                         pairs (PAIRS: the order is numpy's stable argsort, unique; else values only), then one lane
//                         per sorted generated element walks the data elements its mass overlaps: the squares into
//                         ws[p] = W_p N M and, with PAIRS, (2 / (P N M)) sum_j w_ij (a_(i) - b_(j)) into Ct at the row's
//                         original position;
//   sw_finalize_kernel    the P column sums closed in fp64.
// Differences are fp32, their squares and every sum fp64.  Sums are closed the same way everywhere: groups of 64
// consecutive terms by the wave butterfly, the groups in ascending order by one thread -- an order that does not depend
// on how many waves ran.  The network is data-oblivious: whatever the values (a NaN included), every real row index ends
// below position N, because a real element goes before a padding one in every comparison.  No atomics, one writer per
// element.
#include "gm_common.h"
#include "gm_philox.h"
#include <math.h>

namespace {

constexpr int SW_DIR_THREADS = 256;
constexpr int SW_MAX_THREADS = 1024;
constexpr int SW_GROUP = 64;                         // terms per butterfly group of a fixed-order sum

// The sum of one term per (group, lane) over ngroups groups of 64: every wave takes whole groups, lane 0 leaves the
// group's butterfly sum in gs[group]; after the barrier thread 0 adds the groups in ascending order.
template <class F>
static __device__ __forceinline__ double sw_group_sum(int ngroups, double* gs, F term) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int g = wave; g < ngroups; g += nw) {
        const double v = gm_wave_sum_d(term(g * SW_GROUP + lane));
        if (lane == 0) gs[g] = v;
    }
    __syncthreads();
    double tot = 0.0;
    if (threadIdx.x == 0)
        for (int g = 0; g < ngroups; ++g) tot += gs[g];
    return tot;
}

__global__ __launch_bounds__(SW_DIR_THREADS) void sw_directions_kernel(PhNoise n, float* __restrict__ Theta, int64_t ldt,
                                                                       int I) {
    extern __shared__ __attribute__((aligned(16))) char sw_dir_smem[];
    const int p = blockIdx.x, nq = (I + 3) >> 2, ng = (I + SW_GROUP - 1) / SW_GROUP;
    float* v = reinterpret_cast<float*>(sw_dir_smem);                // [4 nq] normals, stored four at a time
    double* gs = reinterpret_cast<double*>(v + 4 * nq);              // [ng] group sums, then the scale
    const uint32_t step = ph_step(n.clk), row = (uint32_t)((int64_t)p * n.kt + n.j0);
    for (int q = threadIdx.x; q < nq; q += SW_DIR_THREADS) {
        const float4 z = ph_normals_of(ph_noise_block(n, step, row, (uint32_t)q));
        *reinterpret_cast<float4*>(v + 4 * q) = z;
    }
    __syncthreads();
    const double s = sw_group_sum(ng, gs, [&](int e) { return e < I ? (double)v[e] * (double)v[e] : 0.0; });
    if (threadIdx.x == 0) gs[ng] = s > 0.0 ? 1.0 / sqrt(s) : 0.0;
    __syncthreads();
    const float inv = (float)gs[ng];
    for (int e = threadIdx.x; e < I; e += SW_DIR_THREADS) Theta[(int64_t)p * ldt + e] = v[e] * inv;
}

// x strictly before y in the (value, row) order.  Padding is (+inf, position >= N): a real element, whatever its value,
// is before it (a finite value is below, an infinity or a NaN ties and has the smaller index).
static __device__ __forceinline__ bool sw_before(float vx, int ix, float vy, int iy) {
    return vx < vy || (!(vy < vx) && ix < iy);
}

template <bool PAIRS>
__global__ __launch_bounds__(SW_MAX_THREADS) void sw_sort_kernel(const float* __restrict__ Pr, int64_t ldp, int N, int M,
                                                                 int La, int Lb, float* __restrict__ Ct, int64_t ldc,
                                                                 double scale, double* __restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) char sw_smem[];
    const int ng = (N + SW_GROUP - 1) / SW_GROUP;
    double* gs = reinterpret_cast<double*>(sw_smem);                 // [ng] group sums
    float* va = reinterpret_cast<float*>(gs + ng);                   // [La] then [Lb] values
    float* vb = va + La;
    int* ia = reinterpret_cast<int*>(vb + Lb);                       // PAIRS: [La] then [Lb] original rows
    int* ib = ia + La;
    const int tid = threadIdx.x, T = blockDim.x, p = blockIdx.x;
    const float* row = Pr + (int64_t)p * ldp;
    const float inf = __builtin_huge_valf();
    for (int i = tid; i < La; i += T) {
        va[i] = i < N ? row[i] : inf;
        if (PAIRS) ia[i] = i;
    }
    for (int j = tid; j < Lb; j += T) {
        vb[j] = j < M ? row[N + j] : inf;
        if (PAIRS) ib[j] = j;
    }
    __syncthreads();

    // the bitonic network over both columns at once: pair t < La / 2 belongs to a, the others to b; a column takes part
    // in the merges up to its own length
    const int ha = La >> 1, hb = Lb >> 1, Lmax = La > Lb ? La : Lb;
    for (int k = 2; k <= Lmax; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < ha + hb; t += T) {
                const bool isa = t < ha;
                if (k > (isa ? La : Lb)) continue;
                const int u = isa ? t : t - ha;
                const int lo = 2 * u - (u & (j - 1)), hi = lo + j;
                float* v = isa ? va : vb;
                const float x = v[lo], y = v[hi];
                const bool up = (lo & k) == 0;
                bool swap;
                if (PAIRS) {
                    int* ix = isa ? ia : ib;
                    const int xi = ix[lo], yi = ix[hi];
                    swap = up ? sw_before(y, yi, x, xi) : sw_before(x, xi, y, yi);
                    if (swap) { ix[lo] = yi; ix[hi] = xi; }
                } else {
                    swap = up ? y < x : x < y;
                }
                if (swap) { v[lo] = y; v[hi] = x; }
            }
            __syncthreads();
        }
    }

    // sorted position i of a holds the mass [i M, (i + 1) M) of N M; position j of b the mass [j N, (j + 1) N)
    const double tot = sw_group_sum(ng, gs, [&](int i) {
        if (i >= N) return 0.0;
        const int64_t m0 = (int64_t)i * M, m1 = m0 + M;
        const int j0 = (int)(m0 / N), j1 = (int)((m1 - 1) / N);
        const float a = va[i];
        double s2 = 0.0, s1 = 0.0;
        for (int j = j0; j <= j1; ++j) {
            const int64_t n0 = (int64_t)j * N, n1 = n0 + N;
            const double w = (double)((m1 < n1 ? m1 : n1) - (m0 > n0 ? m0 : n0));
            const double d = (double)(a - vb[j]);
            s2 += w * (d * d);
            s1 += w * d;
        }
        if (PAIRS) {
            const int r = ia[i];
            if (r < N) Ct[(int64_t)p * ldc + r] = (float)(scale * s1);
        }
        return s2;
    });
    if (tid == 0) ws[p] = tot;
}

__global__ __launch_bounds__(256) void sw_finalize_kernel(const double* __restrict__ ws, int P, double inv,
                                                          double* __restrict__ stats, float* __restrict__ loss_out) {
    __shared__ double gs[GM_SW_MAX_P / SW_GROUP];
    const double tot = sw_group_sum((P + SW_GROUP - 1) / SW_GROUP, gs, [&](int p) { return p < P ? ws[p] : 0.0; });
    if (threadIdx.x == 0) {
        const double swd2 = tot * inv;
        stats[0] = swd2;
        stats[1] = sqrt(swd2);
        if (loss_out) *loss_out = (float)swd2;
    }
}

int sw_pow2(int n) {
    int L = 1;
    while (L < n) L <<= 1;
    return L;
}

}  // namespace

extern "C" int64_t gm_sw_workspace_bytes(int P) {
    GM_CHECK_ARG(P >= 1 && P <= GM_SW_MAX_P);
    return 8 * (int64_t)P;
}

extern "C" int gm_sw_directions(void* stream, const gm_iwae_noise* n, float* Theta, int64_t ldt, int P, int I) {
    GM_CHECK_ARG(Theta != nullptr);
    GM_CHECK_ARG(P >= 1 && P <= GM_SW_MAX_P && I >= 1 && I <= GM_MMD_MAX_I && ldt >= I);
    // one noise row per direction, the first one j0 (the metric's block offset): k_total is 1
    GM_CHECK_ARG(n != nullptr);
    GM_CHECK_ARG(n->k_total == 1 && n->j0 >= 0 && n->j0 + (int64_t)P <= (1ll << 32) && n->q0 >= 0 && n->q0 < (1ll << 31));
    const PhNoise pn{n->seed, n->tag, PhClock{n->step_ctr, n->step_base, n->step_add}, 1, n->j0, (uint32_t)n->q0};
    const size_t lds = 8 * (size_t)((I + SW_GROUP - 1) / SW_GROUP + 1) + 16 * (size_t)((I + 3) / 4);
    hipLaunchKernelGGL(sw_directions_kernel, dim3((unsigned)P), dim3(SW_DIR_THREADS), lds, (hipStream_t)stream, pn, Theta,
                       ldt, I);
    GM_LAUNCH_RET();
}

extern "C" int gm_sw_sort(void* stream, const float* Pr, int64_t ldp, int P, int N, int M, float* Ct, int64_t ldc,
                          void* ws, int64_t ws_bytes) {
    GM_CHECK_ARG(Pr && ws);
    GM_CHECK_ARG(P >= 1 && P <= GM_SW_MAX_P);
    const int lim = Ct ? GM_SW_MAX_B : GM_SW_MAX_ROWS;
    GM_CHECK_ARG(N >= 1 && N <= lim && M >= 1 && M <= lim);
    GM_CHECK_ARG(ldp >= (int64_t)N + M);
    GM_CHECK_ARG(Ct == nullptr || ldc >= N);
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0);
    GM_CHECK_ARG(ws_bytes >= 8 * (int64_t)P);
    const int La = sw_pow2(N), Lb = sw_pow2(M);
    int threads = (La + Lb) / 2;
    threads = threads < 64 ? 64 : threads > SW_MAX_THREADS ? SW_MAX_THREADS : (threads + 63) / 64 * 64;
    const size_t lds = 8 * (size_t)((N + SW_GROUP - 1) / SW_GROUP) + (Ct ? 8 : 4) * (size_t)(La + Lb);
    const double scale = 2.0 / ((double)P * (double)N * (double)M);
    if (Ct)
        hipLaunchKernelGGL(sw_sort_kernel<true>, dim3((unsigned)P), dim3((unsigned)threads), lds, (hipStream_t)stream, Pr,
                           ldp, N, M, La, Lb, Ct, ldc, scale, static_cast<double*>(ws));
    else
        hipLaunchKernelGGL(sw_sort_kernel<false>, dim3((unsigned)P), dim3((unsigned)threads), lds, (hipStream_t)stream, Pr,
                           ldp, N, M, La, Lb, Ct, ldc, scale, static_cast<double*>(ws));
    GM_LAUNCH_RET();
}

extern "C" int gm_sw_finalize(void* stream, int P, int N, int M, const void* ws, int64_t ws_bytes, double* stats,
                              float* loss_out) {
    GM_CHECK_ARG(ws && stats);
    GM_CHECK_ARG(P >= 1 && P <= GM_SW_MAX_P && N >= 1 && N <= GM_SW_MAX_ROWS && M >= 1 && M <= GM_SW_MAX_ROWS);
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 7) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7) == 0);
    GM_CHECK_ARG(ws_bytes >= 8 * (int64_t)P);
    hipLaunchKernelGGL(sw_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, static_cast<const double*>(ws), P,
                       1.0 / ((double)P * (double)N * (double)M), stats, loss_out);
    GM_LAUNCH_RET();
}
