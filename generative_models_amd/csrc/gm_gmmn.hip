// Generative moment matching network (gmmn.py holds the contract): the kernel maximum mean
// discrepancy between generated rows X [N, I] and data rows Y [M, I] under k(a, b) = sum_s exp(-|a - b|^2 / (2 sigma_s^2)),
// with its gradient with respect to X.  R = [X; Y] is the stacked row set, T = N + M.
//
//   gmmn_prior_kernel    z = fmaf(2, u, -1), u the uniform of the row's Philox words (gm_philox.h);
//   mmd_norms_kernel     the rows less mu = x_1 (-> Rc) and their |row|^2, by the pairs kernel's own MFMA sequence on the
//                        row against itself;
//   mmd_pairs_kernel     one workgroup per (256 rows i of R, 128-partner chunk j of R): a.b as an FP32-input MFMA dot
//                        product (parzen_lse_kernel's tile and LDS staging), then per pair d^2 = |a|^2 + |b|^2 - 2 a.b
//                        (clamped at 0; exactly 0 where i = j and for any two equal rows), the S kernel values and
//                        w = sum_s exp(.) / sigma_s^2.  Pairs (i < N, j < N) are the xx block, (i < N, j >= N) xy,
//                        (i >= N, j >= N) yy; (i >= N, j < N) is xy again and skipped.  A complete tile goes through LDS so
//                        that one thread owns one row i and sums its pairs in fp64: the workgroup
//                        leaves five block sums (xx and yy without their diagonals, xy, the two diagonals) and, with
//                        grad, its chunk's share of r_i = sum_j C[i, j] and C's tile itself;
//   mmd_finalize_kernel  workgroup 0 adds the block sums in workgroup order (fp64) and writes mmd2, the loss, 1 / (2 loss)
//                        and the sums; the others add each row's chunk shares of r in chunk order;
//   mmd_grad_kernel      dA = inv (r_i (x - mu) - P) [x (1 - x)], P = C (R - mu) from the GEMM kernels, inv read on the
//                        device.  mu is the first generated row: r_i x_i - (C R)_i is the same number about any origin,
//                        and about a generated row the products that cancel in it are small when the generator has
//                        collapsed (and vanish when every row is equal).
// No atomics, one writer per element, fixed orders: two runs agree bit for bit.
#include "gm_common.h"
#include "gm_philox.h"
#include <math.h>

namespace {

constexpr int MM_THREADS = 256;                      // 4 waves
constexpr int MM_QB = 256;                           // rows i per workgroup: 64 per wave, 2 MFMA column tiles
constexpr int MM_ST = 64;                            // partners j per tile: 2 MFMA row tiles, shared by the 4 waves
constexpr int MM_KT = 16;                            // k per LDS stage
constexpr int MM_LD = MM_KT + 4;                     // LDS row pitch (floats): 16-byte aligned, b128 reads spread banks
constexpr int MM_CHUNK = GM_MMD_CHUNK;               // partners per workgroup (a multiple of MM_ST)
constexpr int MM_SMAX = GM_MMD_MAX_SIGMAS;
constexpr int MM_ROWS = MM_ST + MM_QB;               // LDS rows: partners first, then the workgroup's rows
constexpr int MM_LOADS = MM_ROWS * MM_KT / MM_THREADS;
constexpr int MM_DLD = MM_ST + 4;                    // row pitch of a complete tile in LDS (floats): 16-byte aligned
constexpr int MM_NSUM = 5;                           // xx off-diagonal, xy, yy off-diagonal, xx diagonal, yy diagonal
static_assert(MM_CHUNK % MM_ST == 0, "chunks hold whole partner tiles");
static_assert(MM_LOADS * MM_THREADS == MM_ROWS * MM_KT && MM_ST % (MM_THREADS / MM_KT) == 0, "loader layout");
static_assert(MM_QB * MM_DLD >= MM_ROWS * MM_LD && MM_QB == MM_THREADS, "one LDS buffer, one thread per row of a tile");

constexpr double MM_LOG2E = 1.4426950408889634;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Row t of R = [X; Y] starts (t < N ? 0 : dy) + t * (t < N ? ldx4 : ldy4) bytes past X: two selects of uniform values,
// no branch.  dy = (Y - X) in bytes - N ldy4.
struct MmRows { const char* X; int64_t ldx4; int N; int64_t ldy4; int64_t dy; int M; };

static __device__ __forceinline__ const float* mm_row(const MmRows& R, int t) {
    const bool x = t < R.N;
    return reinterpret_cast<const float*>(R.X + ((int64_t)t * (x ? R.ldx4 : R.ldy4) + (x ? (int64_t)0 : R.dy)));
}

// One thread per (row, quad of latents).
__global__ __launch_bounds__(256) void gmmn_prior_kernel(PhNoise n, float* __restrict__ z, int64_t ldz, int B, int Z) {
    const int nq = (Z + 3) >> 2;
    const int64_t id = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (int64_t)B * nq) return;
    const int b = (int)(id / nq), q = (int)(id - (int64_t)b * nq);
    const float4 u = ph_units_of(ph_noise_block(n, ph_step(n.clk), (uint32_t)((int64_t)b * n.kt + n.j0), (uint32_t)q));
    float* o = z + (int64_t)b * ldz + 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * q + j < Z) o[j] = fmaf(2.f, ph_lane(u, j), -1.f);
}

// |row|^2 of every row of R as the pairs kernel forms a dot product: one wave per 32 rows runs that kernel's MFMA
// sequence (stages of 16 k, MFMA j of k-group g on k = 8g + j and 8g + 4 + j, zeros past the row length) on the rows
// against themselves and keeps the tile's diagonal.  |a|^2, |b|^2 and a.b of two equal rows are then the same fp32 number,
// so their d^2 is exactly 0 in the xy block too.  The rows are taken less mu, the first generated row (distances do not
// change; the dot products and norms are smaller, so their fp32 sums lose less, and next to nothing once the generator
// has collapsed onto mu), and every element, passing through one lane here, is left in Rc [T, d]: what the pairs kernel
// and the product C (R - mu) read.  rn holds mmd_tpad(T) floats, zero past T: the pairs kernel reads the
// norm of any row of its tiles without a bound.
__global__ __launch_bounds__(256) void mmd_norms_kernel(MmRows R, int d, float* __restrict__ rn, int tpad,
                                                        float* __restrict__ Rc) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 32, row = row0 + r, T = R.N + R.M;
    if (row0 >= tpad) return;                        // whole waves
    const float* p = mm_row(R, min(row, T - 1));
    const float* mu = mm_row(R, 0);
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    for (int k0 = 0; k0 < d; k0 += MM_KT) {
        float v[MM_KT / 2];
#pragma unroll
        for (int g = 0; g < MM_KT / 8; ++g)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 8 * g + 4 * h + j;
                const float x = p[min(k, d - 1)];
                const float c = k < d ? x - mu[min(k, d - 1)] : 0.0f;
                v[4 * g + j] = c;
                if (k < d && row < T) Rc[(int64_t)row * d + k] = c;
            }
#pragma unroll
        for (int i = 0; i < MM_KT / 2; ++i) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[i], v[i], acc, 0, 0, 0);
    }
    // D[i][i] sits in lane i + 32 * ((i >> 2) & 1), register (i & 3) + 4 * (i >> 3)
    const int reg = (r & 3) + 4 * (r >> 3);
    float n = 0.0f;
#pragma unroll
    for (int g = 0; g < 16; ++g) n = g == reg ? acc[g] : n;
    if (h == ((r >> 2) & 1) && row < tpad) rn[row] = row < T ? n : 0.0f;
}

// v_mfma_f32_32x32x2_f32: lane l feeds A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31]; D[i][j] sits in lane
// j + 32 * ((i >> 2) & 1), register (i & 3) + 4 * (i >> 3).  Partners are A's rows, the workgroup's rows B's columns, so a
// lane holds one row i per column tile and 16 of a row tile's 32 partners, four consecutive ones per register quad (one
// 16-byte LDS store when the tile is complete).  Inside a stage a lane reads 4 consecutive k with one ds_read_b128: MFMA
// j of k-group g sums k = 8g + j and 8g + 4 + j (the same permutation on both operands: the dot product is complete).
__global__ __launch_bounds__(MM_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void mmd_pairs_kernel(
        const float* __restrict__ Rc, int N, int M, int d, const float* __restrict__ sigmas, int nsig,
        const float* __restrict__ rn, float cxx, float cxy,
        float* __restrict__ C, int64_t ldc, int cvec, double* __restrict__ rpart, double* __restrict__ bsum) {
    __shared__ __attribute__((aligned(16))) float sh[MM_QB * MM_DLD];     // the staging rows, then a tile's distances
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, r = lane & 31, h = lane >> 5;
    const int T = N + M;
    const int q0 = blockIdx.x * MM_QB, chunk = blockIdx.y, c0 = chunk * MM_CHUNK;
    const int64_t wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int cend = min(c0 + MM_CHUNK, T);
    if (q0 >= N && cend <= N) {                      // data rows against generated partners: the xy block again
        if (tid < MM_NSUM) bsum[wg * MM_NSUM + tid] = 0.0;
        return;
    }
    const int ntiles = (cend - c0 + MM_ST - 1) / MM_ST;
    const int nk = (d + MM_KT - 1) / MM_KT, nstages = ntiles * nk;
    const bool grad = C != nullptr;

    // per bandwidth: the exponent's scale in log2 units, log2(e) / (2 sigma^2), as two floats (its rounding to one would
    // tilt every kernel value of the bandwidth the same way, and r_i is a difference of their sums), and 1 / sigma^2
    // (read back as broadcasts; the stage loop's first barrier orders the writes)
    __shared__ float4 stab[MM_SMAX];
    if (tid < MM_SMAX) {
        const double s2 = tid < nsig ? (double)sigmas[tid] * (double)sigmas[tid] : 1.0;
        const double c = MM_LOG2E / (2.0 * s2);
        const float chi = (float)c;
        stab[tid] = tid < nsig ? make_float4(chi, (float)(c - (double)chi), (float)(1.0 / s2), 0.f)
                               : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int qi = q0 + tid;                         // the row this thread owns once a tile is complete
    const bool qx = qi < N, qin = qi < T;
    const float qnorm = rn[qi];
    double aX = 0.0, aY = 0.0, aD = 0.0, aR = 0.0;  // the row's sums over this chunk

    // global -> registers (one stage ahead) -> LDS.  Addresses are clamped into the operands.  Past the row length the
    // partner side is zeroed (the product vanishes whatever the other side repeats); a row past T repeats row T - 1 and
    // its pairs are dropped below.
    const int lk = tid & (MM_KT - 1), lr = tid / MM_KT;
    float pf[MM_LOADS];
    auto load_stage = [&](int st) {
        const int t = st / nk, k = (st - t * nk) * MM_KT + lk;
        const bool kin = k < d;
        const int kc = min(k, d - 1);
#pragma unroll
        for (int i = 0; i < MM_LOADS; ++i) {
            const int row = lr + (MM_THREADS / MM_KT) * i;
            const int rr = row < MM_ST ? c0 + t * MM_ST + row : q0 + row - MM_ST;
            float v = Rc[(int64_t)min(rr, T - 1) * d + kc];
            if (row < MM_ST && !kin) v = 0.0f;
            pf[i] = v;
        }
    };

    f32x16 acc[2][2];
    load_stage(0);
    for (int st = 0; st < nstages; ++st) {
        const int t = st / nk, kt = st - t * nk;
        if (kt == 0) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int g = 0; g < 16; ++g) acc[a][b][g] = 0.0f;
        }
        __syncthreads();                             // the previous stage's LDS reads are done
#pragma unroll
        for (int i = 0; i < MM_LOADS; ++i) sh[(lr + (MM_THREADS / MM_KT) * i) * MM_LD + lk] = pf[i];
        __syncthreads();
        if (st + 1 < nstages) load_stage(st + 1);
#pragma unroll
        for (int g = 0; g < MM_KT / 8; ++g) {
            f32x4 A[2], B[2];
#pragma unroll
            for (int a = 0; a < 2; ++a) A[a] = *reinterpret_cast<const f32x4*>(&sh[(a * 32 + r) * MM_LD + 8 * g + 4 * h]);
#pragma unroll
            for (int b = 0; b < 2; ++b)
                B[b] = *reinterpret_cast<const f32x4*>(&sh[(MM_ST + w * 64 + b * 32 + r) * MM_LD + 8 * g + 4 * h]);
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[a][j], B[b][j], acc[a][b], 0, 0, 0);
        }
        if (kt == nk - 1) {
            // the tile's dot products go through LDS (over the staging buffer), so that thread `tid` owns row q0 + tid
            // against the tile's 64 partners: one runtime loop, a row's sums in one thread, C in 16-byte pieces
            __syncthreads();                         // the stage's LDS reads are done
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b)
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        *reinterpret_cast<f32x4*>(&sh[(w * 64 + b * 32 + r) * MM_DLD + a * 32 + 8 * gq + 4 * h]) =
                            f32x4{acc[a][b][4 * gq], acc[a][b][4 * gq + 1], acc[a][b][4 * gq + 2], acc[a][b][4 * gq + 3]};
            __syncthreads();
            const int tile0 = c0 + t * MM_ST;
            if (!(q0 >= N && tile0 + MM_ST <= N)) {  // data rows against generated partners: nothing to take
#pragma unroll 1
                for (int jq = 0; jq < MM_ST / 4; ++jq) {
                    const int j0 = tile0 + 4 * jq;
                    const f32x4 a4 = *reinterpret_cast<const f32x4*>(&sh[tid * MM_DLD + 4 * jq]);
                    float d2[4], kv[4] = {0.f, 0.f, 0.f, 0.f}, wv[4] = {0.f, 0.f, 0.f, 0.f}, cv[4];
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi) {
                        d2[gi] = fmaxf(fmaf(-2.f, a4[gi], qnorm + rn[j0 + gi]), 0.f);
                        if (qi == j0 + gi) d2[gi] = 0.f;         // a row against itself
                    }
#pragma unroll 1
                    for (int k = 0; k < nsig; ++k) {
                        const float4 sc = stab[k];
#pragma unroll
                        for (int gi = 0; gi < 4; ++gi) {
                            const float e = __builtin_amdgcn_exp2f(-fmaf(d2[gi], sc.x, d2[gi] * sc.y));
                            kv[gi] += e;
                            wv[gi] = fmaf(e, sc.z, wv[gi]);
                        }
                    }
#pragma unroll
                    for (int gi = 0; gi < 4; ++gi) {
                        const int j = j0 + gi;
                        const bool px = j < N, ok = qin && j < T && (qx || !px), dg = qi == j;
                        aD += (double)((ok && dg) ? kv[gi] : 0.f);
                        aX += (double)((ok && !dg && px) ? kv[gi] : 0.f);
                        aY += (double)((ok && !dg && !px) ? kv[gi] : 0.f);
                        cv[gi] = (px ? cxx : cxy) * wv[gi];
                        aR += (double)((qx && j < T) ? cv[gi] : 0.f);
                    }
                    if (grad && qx) {
                        float* o = C + (int64_t)qi * ldc + j0;
                        if (cvec && j0 + 3 < T) {
                            *reinterpret_cast<f32x4*>(o) = f32x4{cv[0], cv[1], cv[2], cv[3]};
                        } else {
#pragma unroll
                            for (int gi = 0; gi < 4; ++gi)
                                if (j0 + gi < T) o[gi] = cv[gi];
                        }
                    }
                }
            }
        }
    }

    // thread `tid` holds row q0 + tid's share of r over this chunk
    if (grad && qx) rpart[(int64_t)chunk * N + qi] = aR;
    double s[MM_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (qx) { s[0] = aX; s[1] = aY; s[3] = aD; }
    else    { s[2] = aY; s[4] = aD; }
    __syncthreads();                                 // the last tile's LDS reads are done
    double* shd = reinterpret_cast<double*>(sh);
#pragma unroll
    for (int c = 0; c < MM_NSUM; ++c) {
        const double v = gm_wave_sum_d(s[c]);
        if (lane == 0) shd[w * MM_NSUM + c] = v;
    }
    __syncthreads();
    if (tid < MM_NSUM) bsum[wg * MM_NSUM + tid] = ((shd[tid] + shd[MM_NSUM + tid]) + shd[2 * MM_NSUM + tid]) + shd[3 * MM_NSUM + tid];
}

// Workgroup 0: the block sums in workgroup order (a thread's share, then the wave butterfly, then the waves in order),
// fp64, and the scalars.  Workgroups 1 ..: one thread per generated row, its chunk shares of r in chunk order.
__global__ __launch_bounds__(256) void mmd_finalize_kernel(const double* __restrict__ bsum, int64_t nwg,
                                                           const double* __restrict__ rpart, int nchunks, int N, int M,
                                                           int nsig, int sqrt_loss, double* __restrict__ stats,
                                                           float* __restrict__ rvec, float* __restrict__ loss_out) {
    __shared__ double sh[4 * MM_NSUM];
    const int tid = threadIdx.x;
    if (blockIdx.x > 0) {
        const int i = (blockIdx.x - 1) * 256 + tid;
        if (i >= N) return;
        double acc = 0.0;
        for (int ch = 0; ch < nchunks; ++ch) acc += rpart[(int64_t)ch * N + i];
        rvec[i] = (float)acc;
        return;
    }
    double s[MM_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t g = tid; g < nwg; g += 256)
#pragma unroll
        for (int c = 0; c < MM_NSUM; ++c) s[c] += bsum[g * MM_NSUM + c];
#pragma unroll
    for (int c = 0; c < MM_NSUM; ++c) {
        const double v = gm_wave_sum_d(s[c]);
        if ((tid & 63) == 0) sh[(tid >> 6) * MM_NSUM + c] = v;
    }
    __syncthreads();
    if (tid == 0) {
        double t[MM_NSUM];
        for (int c = 0; c < MM_NSUM; ++c) t[c] = ((sh[c] + sh[MM_NSUM + c]) + sh[2 * MM_NSUM + c]) + sh[3 * MM_NSUM + c];
        const double n = (double)N, m = (double)M;
        const double sxx = t[0] + t[3], sxy = t[1], syy = t[2] + t[4];
        const double mmd2 = sxx / (n * n) - 2.0 * sxy / (n * m) + syy / (m * m);
        const double loss = sqrt_loss ? sqrt(fmax(mmd2 + 1e-8, 0.0)) : mmd2;
        stats[0] = mmd2;
        stats[1] = loss;
        stats[2] = sqrt_loss ? (loss > 0.0 ? 1.0 / (2.0 * loss) : 0.0) : 1.0;
        stats[3] = sxx; stats[4] = sxy; stats[5] = syy;
        stats[6] = t[0]; stats[7] = t[2];            // xx and yy without their diagonals: the unbiased statistic's sums
        stats[8] = t[3]; stats[9] = t[4];            // the diagonals: N S and M S exactly
        if (loss_out) *loss_out = (float)loss;
    }
}

// One thread per element of dA.
__global__ __launch_bounds__(256) void mmd_grad_kernel(const float* __restrict__ X, int64_t ldx,
                                                       const float* __restrict__ mu, const float* __restrict__ P,
                                                       int64_t ldp,
                                                       const float* __restrict__ rvec, const double* __restrict__ stats,
                                                       float gscale, int sigmoid, float* __restrict__ dA, int64_t lda,
                                                       int I) {
    const int i = blockIdx.y, e = blockIdx.x * 256 + threadIdx.x;
    if (e >= I) return;
    const float inv = (float)stats[2] * gscale, x = X[(int64_t)i * ldx + e];
    float g = inv * fmaf(rvec[i], mu ? x - mu[e] : x, -P[(int64_t)i * ldp + e]);
    if (sigmoid) g *= x * (1.f - x);
    dA[(int64_t)i * lda + e] = g;
}

int64_t mmd_chunks(int64_t T) { return (T + MM_CHUNK - 1) / MM_CHUNK; }
int64_t mmd_qblocks(int64_t T) { return (T + MM_QB - 1) / MM_QB; }
int64_t mmd_tpad(int64_t T) { return (T / MM_QB + 1) * MM_QB; }     // > T, and past every tile of the grid

}  // namespace

extern "C" int64_t gm_mmd_workspace_bytes(int N, int M, int grad) {
    GM_CHECK_ARG(N >= 1 && M >= 1 && (int64_t)N + M < (1ll << 31));
    const int64_t T = (int64_t)N + M;
    return 8 * MM_NSUM * mmd_qblocks(T) * mmd_chunks(T) + (grad ? 8 * mmd_chunks(T) * N : 0) + 4 * mmd_tpad(T);
}

extern "C" int gm_gmmn_prior(void* stream, const gm_iwae_noise* n, float* z, int64_t ldz, int B, int Z) {
    GM_CHECK_ARG(z != nullptr);
    GM_CHECK_ARG(B >= 1 && Z >= 1 && Z <= GM_GMMN_MAX_Z && ldz >= Z);
    // one noise row per batch row, the first one j0 (sample()'s row offset): k_total is 1
    GM_CHECK_ARG(n != nullptr);
    GM_CHECK_ARG(n->k_total == 1 && n->j0 >= 0 && n->j0 + (int64_t)B <= (1ll << 32) && n->q0 >= 0 && n->q0 < (1ll << 31));
    const PhNoise pn{n->seed, n->tag, PhClock{n->step_ctr, n->step_base, n->step_add}, 1, n->j0, (uint32_t)n->q0};
    const int64_t total = (int64_t)B * ((Z + 3) / 4);
    hipLaunchKernelGGL(gmmn_prior_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pn, z,
                       ldz, B, Z);
    GM_LAUNCH_RET();
}

extern "C" int gm_mmd_pairs(void* stream, const float* X, int64_t ldx, int N, const float* Y, int64_t ldy, int M, int I,
                            const float* sigmas, int n_sigma, float* C, int64_t ldc, float* Rc, void* workspace,
                            int64_t ws_bytes) {
    GM_CHECK_ARG(X && Y && sigmas && workspace && Rc);
    GM_CHECK_ARG(N >= 1 && M >= 1 && I >= 1 && I <= GM_MMD_MAX_I && (int64_t)N + M < (1ll << 31));
    GM_CHECK_ARG(n_sigma >= 1 && n_sigma <= GM_MMD_MAX_SIGMAS);
    GM_CHECK_ARG(ldx >= I && ldy >= I);
    GM_CHECK_ARG(C == nullptr || ldc >= (int64_t)N + M);
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0);
    const int64_t T = (int64_t)N + M, nchunks = mmd_chunks(T), nqb = mmd_qblocks(T);
    GM_CHECK_ARG(nchunks <= 65535);
    GM_CHECK_ARG(ws_bytes >= gm_mmd_workspace_bytes(N, M, C != nullptr));
    hipStream_t st = (hipStream_t)stream;
    double* bsum = static_cast<double*>(workspace);
    double* rpart = bsum + MM_NSUM * nqb * nchunks;
    float* rn = reinterpret_cast<float*>(rpart + (C ? nchunks * N : 0));
    const MmRows R{reinterpret_cast<const char*>(X), 4 * ldx, N, 4 * ldy,
                   (int64_t)(reinterpret_cast<intptr_t>(Y) - reinterpret_cast<intptr_t>(X)) - 4 * ldy * N, M};
    const double n = (double)N, m = (double)M;
    const int cvec = C && (ldc & 3) == 0 && (reinterpret_cast<uintptr_t>(C) & 15) == 0;
    hipLaunchKernelGGL(mmd_norms_kernel, dim3((unsigned)(mmd_tpad(T) / 128)), dim3(256), 0, st, R, I, rn, (int)mmd_tpad(T), Rc);
    hipLaunchKernelGGL(mmd_pairs_kernel, dim3((unsigned)nqb, (unsigned)nchunks), dim3(MM_THREADS), 0, st, Rc, N, M, I, sigmas,
                       n_sigma, rn, (float)(-2.0 / (n * n)), (float)(2.0 / (n * m)), C, ldc, cvec, C ? rpart : nullptr,
                       bsum);
    GM_LAUNCH_RET();
}

extern "C" int gm_mmd_finalize(void* stream, int N, int M, int n_sigma, int sqrt_loss, int grad, const void* workspace,
                               int64_t ws_bytes, double* stats, float* r, float* loss_out) {
    GM_CHECK_ARG(workspace && stats);
    GM_CHECK_ARG(N >= 1 && M >= 1 && (int64_t)N + M < (1ll << 31));
    GM_CHECK_ARG(n_sigma >= 1 && n_sigma <= GM_MMD_MAX_SIGMAS);
    GM_CHECK_ARG(!grad || r != nullptr);
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(stats) & 7) == 0);
    GM_CHECK_ARG(ws_bytes >= gm_mmd_workspace_bytes(N, M, grad));
    const int64_t T = (int64_t)N + M, nchunks = mmd_chunks(T), nwg = mmd_qblocks(T) * nchunks;
    const double* bsum = static_cast<const double*>(workspace);
    const double* rpart = bsum + MM_NSUM * nwg;
    const unsigned blocks = 1u + (grad ? (unsigned)((N + 255) / 256) : 0u);
    hipLaunchKernelGGL(mmd_finalize_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, bsum, nwg, rpart,
                       (int)nchunks, N, M, n_sigma, sqrt_loss ? 1 : 0, stats, r, loss_out);
    GM_LAUNCH_RET();
}

extern "C" int gm_mmd_grad(void* stream, const float* X, int64_t ldx, const float* mu, const float* P, int64_t ldp,
                           const float* r, const double* stats, float gscale, int sigmoid, float* dA, int64_t lda, int N,
                           int I) {
    GM_CHECK_ARG(X && P && r && stats && dA);
    GM_CHECK_ARG(N >= 1 && N <= 65535 && I >= 1 && I <= GM_MMD_MAX_I);
    GM_CHECK_ARG(ldx >= I && ldp >= I && lda >= I);
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(stats) & 7) == 0);
    hipLaunchKernelGGL(mmd_grad_kernel, dim3((unsigned)((I + 255) / 256), (unsigned)N), dim3(256), 0, (hipStream_t)stream,
                       X, ldx, mu, P, ldp, r, stats, gscale, sigmoid ? 1 : 0, dA, lda, I);
    GM_LAUNCH_RET();
}
