// Gaussian Parzen-window log-likelihood of query rows under a set of sample rows (the MNIST metric of
// arXiv 1406.2661, table 1): for every bandwidth sigma and query x,
//     ll(x) = logsumexp_i(-|x - s_i|^2 / (2 sigma^2)) - log N - d log(sigma sqrt(2 pi)).
//
// Three launches:
//   parzen_norms_kernel     |row|^2 of every query and sample row (fp64 sum, rounded once);
//   parzen_lse_kernel       one workgroup per (256 queries, 128-sample chunk): -|x - s|^2 / 2 as an FP32-input MFMA
//                           dot product whose accumulator starts at -(|x|^2 + |s|^2) / 2, then an online base-2
//                           log-sum-exp per (query, sigma) kept in registers; the distance matrix is never written.
//                           The chunk's (max, scaled sum) goes to the workspace;
//   parzen_finalize_kernel  combines the chunks of one (sigma, query) in chunk order, in fp64.
// Every query's value is a function of that query's row and the samples only (its column of the MFMA tile, its own
// lanes' running sums, fixed chunk boundaries), so it is bitwise the same whichever other queries share the call.
#include "gm_common.h"
#include <float.h>
#include <math.h>

namespace {

constexpr int PZ_THREADS = 256;                      // 4 waves
constexpr int PZ_QB = 256;                           // queries per workgroup: 64 per wave, 2 MFMA column tiles
constexpr int PZ_ST = 64;                            // samples per tile: 2 MFMA row tiles, shared by the 4 waves
constexpr int PZ_KT = 16;                            // k per LDS stage
constexpr int PZ_LD = PZ_KT + 4;                     // LDS row pitch (floats): 16-byte aligned, b128 reads spread banks
constexpr int PZ_CHUNK = GM_PARZEN_CHUNK;            // samples per workgroup (a multiple of PZ_ST)
constexpr int PZ_SMAX = GM_PARZEN_MAX_SIGMAS;
constexpr int PZ_ROWS = PZ_ST + PZ_QB;               // LDS rows: samples first, then queries
constexpr int PZ_LOADS = PZ_ROWS * PZ_KT / PZ_THREADS;
static_assert(PZ_CHUNK % PZ_ST == 0, "chunks hold whole sample tiles");
static_assert(PZ_LOADS * PZ_THREADS == PZ_ROWS * PZ_KT && PZ_ST % (PZ_THREADS / PZ_KT) == 0, "loader layout");

constexpr double PZ_LOG2E = 1.4426950408889634;
constexpr double PZ_LN2 = 0.6931471805599453;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// One wave per row: fp64 sum of squares in a fixed order, rounded once.
__global__ __launch_bounds__(256) void parzen_norms_kernel(const float* __restrict__ q, int64_t ldq, int nq,
                                                           const float* __restrict__ s, int64_t lds, int ns, int d,
                                                           float* __restrict__ qn, float* __restrict__ sn) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= nq + ns) return;                      // whole waves
    const float* p = row < nq ? q + (int64_t)row * ldq : s + (int64_t)(row - nq) * lds;
    double acc = 0.0;
    for (int k = lane; k < d; k += 64) {
        const double v = p[k];
        acc += v * v;
    }
    acc = gm_wave_sum_d(acc);
    if (lane == 0) {
        if (row < nq) qn[row] = (float)acc;
        else sn[row - nq] = (float)acc;
    }
}

// v_mfma_f32_32x32x2_f32: lane l feeds A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31]; D[i][j] sits in lane
// j + 32 * ((i >> 2) & 1), register (i & 3) + 4 * (i >> 3).  Samples are A's rows, queries B's columns, so a lane owns
// one query per column tile and 16 of a row tile's 32 samples; the two lane halves merge once, at the chunk's end.
// Inside a stage a lane reads 4 consecutive k with one ds_read_b128: MFMA j of k-group g sums k = 8g + j and
// 8g + 4 + j (the same permutation on both operands, so the dot product is complete).
__global__ __launch_bounds__(PZ_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void parzen_lse_kernel(
        const float* __restrict__ q, int64_t ldq, int nq, const float* __restrict__ s, int64_t lds, int ns, int d,
        const float* __restrict__ sigmas, int nsig, const float* __restrict__ qn, const float* __restrict__ sn,
        float2* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sh[PZ_ROWS * PZ_LD];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * PZ_QB, chunk = blockIdx.y, c0 = chunk * PZ_CHUNK;
    const int ntiles = (min(c0 + PZ_CHUNK, ns) - c0 + PZ_ST - 1) / PZ_ST;
    const int nk = (d + PZ_KT - 1) / PZ_KT, nstages = ntiles * nk;

    // exponent scale per bandwidth: -|x - s|^2 / (2 sigma^2) in log2 units = acc * log2(e) / sigma^2
    float c[PZ_SMAX];
#pragma unroll
    for (int k = 0; k < PZ_SMAX; ++k)
        c[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(        // uniform: kept in SGPRs
            k < nsig ? (float)(PZ_LOG2E / ((double)sigmas[k] * (double)sigmas[k])) : 0.0f)));
    // running state per column tile: the largest acc seen (c > 0, so max(acc * c) = c * max(acc) serves every sigma)
    // and per sigma the sum of exp2(acc * c - M * c)
    float M[2] = {-FLT_MAX, -FLT_MAX}, z[2][PZ_SMAX];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int k = 0; k < PZ_SMAX; ++k) z[b][k] = 0.0f;
    int myq[2];
    float qnorm[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        myq[b] = q0 + w * 64 + b * 32 + r;
        qnorm[b] = myq[b] < nq ? qn[myq[b]] : 0.0f;
    }

    // global -> registers (one stage ahead) -> LDS.  Addresses are clamped into the operands, values outside are 0.
    const int lk = tid & (PZ_KT - 1), lr = tid / PZ_KT;
    float pf[PZ_LOADS];
    auto load_stage = [&](int st) {
        const int t = st / nk, k = (st - t * nk) * PZ_KT + lk;
        const bool kin = k < d;
        const int kc = min(k, d - 1);
#pragma unroll
        for (int i = 0; i < PZ_LOADS; ++i) {
            const int row = lr + (PZ_THREADS / PZ_KT) * i;
            float v;
            if (row < PZ_ST) {
                const int sr = c0 + t * PZ_ST + row;
                v = s[(int64_t)min(sr, ns - 1) * lds + kc];
                if (!(kin && sr < ns)) v = 0.0f;
            } else {
                const int qr = q0 + row - PZ_ST;
                v = q[(int64_t)min(qr, nq - 1) * ldq + kc];
                if (!(kin && qr < nq)) v = 0.0f;
            }
            pf[i] = v;
        }
    };

    f32x16 acc[2][2];
    load_stage(0);
    for (int st = 0; st < nstages; ++st) {
        const int t = st / nk, kt = st - t * nk;
        const int rowbase = c0 + t * PZ_ST + 4 * h;  // sample of register 0 of row tile 0 in this lane
        if (kt == 0) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int row = rowbase + a * 32 + (g & 3) + 8 * (g >> 2);
                    const float snorm = row < ns ? sn[row] : 0.0f;
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b][g] = -0.5f * (qnorm[b] + snorm);
                }
        }
        __syncthreads();                             // the previous stage's LDS reads are done
#pragma unroll
        for (int i = 0; i < PZ_LOADS; ++i) sh[(lr + (PZ_THREADS / PZ_KT) * i) * PZ_LD + lk] = pf[i];
        __syncthreads();
        if (st + 1 < nstages) load_stage(st + 1);
#pragma unroll
        for (int g = 0; g < PZ_KT / 8; ++g) {
            f32x4 A[2], B[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) A[a] = *reinterpret_cast<const f32x4*>(&sh[(a * 32 + r) * PZ_LD + 8 * g + 4 * h]);
#pragma unroll
            for (int b = 0; b < 2; ++b)
                B[b] = *reinterpret_cast<const f32x4*>(&sh[(PZ_ST + w * 64 + b * 32 + r) * PZ_LD + 8 * g + 4 * h]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[a][j], B[b][j], acc[a][b], 0, 0, 0);
        }
        if (kt == nk - 1) {
            // online log-sum-exp over this tile's 32 samples of each of the lane's two queries
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float mx = -INFINITY;
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        const int row = rowbase + a * 32 + (g & 3) + 8 * (g >> 2);
                        if (row >= ns) acc[a][b][g] = -INFINITY;
                        mx = fmaxf(mx, acc[a][b][g]);
                    }
                if (mx > -INFINITY) {                // this lane has a sample in the tile
                    const float Mn = fmaxf(M[b], mx);
#pragma unroll
                    for (int k = 0; k < PZ_SMAX; ++k) {
                        if (k < nsig) {
                            const float mn = Mn * c[k];
                            float zz = z[b][k] * __builtin_amdgcn_exp2f((M[b] - Mn) * c[k]);
#pragma unroll
                            for (int a = 0; a < 2; ++a)
#pragma unroll
                                for (int g = 0; g < 16; ++g) zz += __builtin_amdgcn_exp2f(fmaf(acc[a][b][g], c[k], -mn));
                            z[b][k] = zz;
                        }
                    }
                    M[b] = Mn;
                }
            }
        }
    }

    // the two lane halves hold disjoint samples of the same query: merge, lower half writes the chunk's partial
    // (the lower half always holds the chunk's first sample, so mm is finite)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const float Mo = __shfl_xor(M[b], 32, 64), mm = fmaxf(M[b], Mo);
#pragma unroll
        for (int k = 0; k < PZ_SMAX; ++k) {
            if (k < nsig) {
                const float zo = __shfl_xor(z[b][k], 32, 64);
                if (h == 0 && myq[b] < nq) {
                    const float zz = z[b][k] * __builtin_amdgcn_exp2f((M[b] - mm) * c[k]) +
                                     zo * __builtin_amdgcn_exp2f((Mo - mm) * c[k]);
                    part[((int64_t)chunk * nsig + k) * nq + myq[b]] = make_float2(mm * c[k], zz);
                }
            }
        }
    }
}

// One thread per (query, sigma): the chunks' partials in chunk order, fp64.
__global__ __launch_bounds__(256) void parzen_finalize_kernel(const float2* __restrict__ part, int nchunks, int nq,
                                                              int nsig, const float* __restrict__ sigmas,
                                                              double log_n, double d, float* __restrict__ out,
                                                              int64_t ldo) {
    const int qi = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (qi >= nq) return;
    const float2* p = part + (int64_t)k * nq + qi;
    const int64_t stride = (int64_t)nsig * nq;
    float mx = -FLT_MAX;
    for (int ch = 0; ch < nchunks; ++ch) mx = fmaxf(mx, p[ch * stride].x);
    double zs = 0.0;
    for (int ch = 0; ch < nchunks; ++ch) {
        const float2 v = p[ch * stride];
        zs += (double)v.y * exp2((double)v.x - (double)mx);
    }
    const double sg = sigmas[k];
    const double ll = PZ_LN2 * ((double)mx + log2(zs)) - log_n - d * log(sg * 2.5066282746310002);
    out[(int64_t)k * ldo + qi] = (float)ll;
}

int64_t parzen_chunks(int ns) { return ((int64_t)ns + PZ_CHUNK - 1) / PZ_CHUNK; }

}  // namespace

extern "C" int64_t gm_parzen_workspace_bytes(int nq, int ns, int n_sigma) {
    GM_CHECK_ARG(nq >= 1 && ns >= 1 && n_sigma >= 1 && n_sigma <= GM_PARZEN_MAX_SIGMAS);
    return 8 * (int64_t)n_sigma * nq * parzen_chunks(ns) + 4 * ((int64_t)nq + ns);
}

extern "C" int gm_parzen_ll(void* stream, const float* q, int64_t ldq, int nq, const float* s, int64_t lds, int ns,
                            int d, const float* sigmas, int n_sigma, void* workspace, int64_t ws_bytes, float* out,
                            int64_t ldo) {
    GM_CHECK_ARG(q && s && sigmas && workspace && out);
    GM_CHECK_ARG(nq >= 1 && ns >= 1 && d >= 1);
    GM_CHECK_ARG(n_sigma >= 1 && n_sigma <= GM_PARZEN_MAX_SIGMAS);
    GM_CHECK_ARG(ldq >= d && lds >= d && ldo >= nq);
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
    const int64_t nchunks = parzen_chunks(ns), nqb = ((int64_t)nq + PZ_QB - 1) / PZ_QB;
    GM_CHECK_ARG(nchunks <= 65535 && nqb <= 65535);
    const int64_t need = gm_parzen_workspace_bytes(nq, ns, n_sigma);
    GM_CHECK_ARG(ws_bytes >= need);
    hipStream_t st = (hipStream_t)stream;
    float2* part = static_cast<float2*>(workspace);
    float* qn = reinterpret_cast<float*>(part + (int64_t)n_sigma * nq * nchunks);
    float* sn = qn + nq;
    hipLaunchKernelGGL(parzen_norms_kernel, dim3((unsigned)(((int64_t)nq + ns + 3) / 4)), dim3(256), 0, st, q, ldq,
                       nq, s, lds, ns, d, qn, sn);
    hipLaunchKernelGGL(parzen_lse_kernel, dim3((unsigned)nqb, (unsigned)nchunks), dim3(PZ_THREADS), 0, st, q, ldq,
                       nq, s, lds, ns, d, sigmas, n_sigma, qn, sn, part);
    hipLaunchKernelGGL(parzen_finalize_kernel, dim3((unsigned)((nq + 255) / 256), (unsigned)n_sigma), dim3(256), 0,
                       st, part, (int)nchunks, nq, n_sigma, sigmas, log((double)ns), (double)d, out, ldo);
    GM_LAUNCH_RET();
}
