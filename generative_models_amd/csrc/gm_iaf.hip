// Inverse-autoregressive-flow posterior of the IAF-VAE (iafvae.py holds the contract; gm_hip.h).
// The IWAE's two row kernels with a chain of K masked two-layer conditioners between z_0 and the decoder, and the flow's
// own optimiser step.  Rows are image-major (sample j of image b is row b k + j); the noise block and the counter layout
// are gm_philox.h's PhNoise.
//
// Mapping (both row kernels): 64 sample rows per workgroup, ONE LANE PER ROW in each of its four waves, which share the
// rows: every loop over hidden units, latents or output rows is dealt out to the waves in quads (a phase's outputs are
// disjoint between waves; barriers separate the phases).  A row's vectors (z, h, a, ...) live in the lane's own column of
// LDS arrays [index][IAF_LD] (IAF_LD = 65: a lane's reads are conflict-free, and so are the parameter sums, whose lanes
// walk the rows of DIFFERENT indices); a layer's weights are staged into LDS once per workgroup and read at identical
// addresses by every lane (broadcast, 16 bytes at a time: W1 and U rows are padded to a multiple of four).  Every matvec
// is a per-lane loop in a fixed order with four register accumulators, so a row's bits depend on nothing but the row: no
// cross-lane reduction anywhere in the chain.
// gm_iaf_sample: z through the K layers in the lane's column; writes z_K and lp.
// gm_iaf_reduce: a workgroup owns max(1, 64 / k) whole images.  eps and the chain are rebuilt with the K layer inputs kept
//   in LDS, the chain is walked back with the closed forms of the contract, and per layer the workgroup's da / dm / ds and
//   the layer's inputs meet in LDS, where each of the five parameter gradients is formed as a sum over the rows in
//   ascending order: one partial block [K, GM_IAF_PART_STRIDE(Z, F, C)] per workgroup.  dml of an image is the sum over
//   its own samples j ascending, wherever the image lands.
// gm_iaf_step: one thread per parameter entry: the partial blocks summed in ascending order, masked entries skipped (they
//   and their moments stay 0.0), adam_update (the arithmetic of every other step of the project).
// No atomics, fixed reduction orders, no scratch: the same bits on every run, graph or eager.
#include "gm_philox.h"

namespace {

constexpr int IAF_Z = GM_IAF_MAX_Z, IAF_K = GM_IAF_MAX_K, IAF_F = GM_IAF_MAX_F, IAF_C = GM_IAF_MAX_C;
constexpr int IAF_ROWS = GM_IAF_PART_ROWS, IAF_LD = IAF_ROWS + 1;
constexpr int IAF_WAVES = 4, IAF_THREADS = IAF_WAVES * IAF_ROWS;  // the waves share the rows, a slice of every loop each
constexpr int IAF_WA = IAF_F * IAF_Z + IAF_F * IAF_C + IAF_F;     // floats of a staged [W1 | U | b1]
constexpr int IAF_WB = 2 * IAF_Z * IAF_F + 2 * IAF_Z;             // floats of a staged [W2 | b2]
static_assert(IAF_ROWS == 64 && IAF_Z % 4 == 0 && IAF_C % 4 == 0 && IAF_F % 4 == 0, "one wave of rows, 16-byte rows");

struct IafW { const float* W1; const float* U; const float* b1; const float* W2; const float* b2; int K, F, C; };
struct IafDims { int Z, ZP, F, C, CP; };

typedef float IafCol[IAF_LD];

// for (i = thread; i < n; i += 256) with a trip count that is the same in every lane: the compiler otherwise keeps each
// such loop's per-lane entry mask in scalar registers across the layer loop and runs out of them.
#define IAF_LANES(i, n)                                                                                       \
    _Pragma("unroll 1") for (int i##_0 = 0, i = threadIdx.x; i##_0 < (n); i##_0 += IAF_THREADS, i += IAF_THREADS) \
        if (i < (n))

__device__ __forceinline__ float iaf_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float iaf_elu(float x) { return x > 0.f ? x : expm1f(x); }

__device__ __forceinline__ float iaf_dot4(const float4& w, const float (&x)[4], float acc) {
    return fmaf(w.w, x[3], fmaf(w.z, x[2], fmaf(w.y, x[1], fmaf(w.x, x[0], acc))));
}

// Rows [F, W] of a weight (W <= 32 columns) into rows padded to WP = 4 ceil(W / 4) floats, zeros in the padding: 8 threads
// per row, a quad of columns per thread, 32 rows per trip (no division, and the trips' loads are independent).
__device__ __forceinline__ void iaf_stage_rows(const float* __restrict__ src, int F, int W, int WP, float* dst, int ln) {
    const int jl = ln >> 3, c0 = 4 * (ln & 7);
#pragma unroll 2
    for (int j0 = 0; j0 < F; j0 += IAF_THREADS / 8) {
        const int j = j0 + jl;
        if (j < F && c0 < WP) {
            const float* r = src + j * W + c0;
            float4 v;
            v.x = r[0];                                          // c0 < WP means c0 < W: the quad's first column exists
            v.y = c0 + 1 < W ? r[1] : 0.f;
            v.z = c0 + 2 < W ? r[2] : 0.f;
            v.w = c0 + 3 < W ? r[3] : 0.f;
            *reinterpret_cast<float4*>(dst + j * WP + c0) = v;
        }
    }
}

// The lane index behind a compiler barrier: a bound test on it inside a layer loop is then formed where it is used.
// Left visible, every such test is hoisted out of the layer loop as a 64-bit mask, and together they overflow the scalar
// registers.
__device__ __forceinline__ int iaf_lane(int lane) {
    asm volatile("" : "+v"(lane));
    return lane;
}

// The sizes behind the same kind of barrier, for the same reason: what a layer pass derives from them (strides, trip
// counts, LDS offsets) is then formed inside the pass and dies with it.
__device__ __forceinline__ IafDims iaf_dims(IafDims d) {
    asm volatile("" : "+s"(d.Z), "+s"(d.ZP), "+s"(d.F), "+s"(d.C), "+s"(d.CP));
    return d;
}

// Layer l's [W1 (rows padded to ZP) | U (rows padded to CP) | b1] into wA; every thread of the wave calls it (ln: its
// iaf_lane of its thread index).
__device__ __forceinline__ void iaf_stage_a(const IafW& f, int l, const IafDims& d, float* wA, int ln) {
    iaf_stage_rows(f.W1 + (int64_t)l * d.F * d.Z, d.F, d.Z, d.ZP, wA, ln);
    float* Us = wA + d.F * d.ZP;
    if (d.C > 0) iaf_stage_rows(f.U + (int64_t)l * d.F * d.C, d.F, d.C, d.CP, Us, ln);
    if (ln < d.F) Us[d.F * d.CP + ln] = f.b1[l * d.F + ln];
}

// Layer l's [W2 [2Z, F] | b2 [2Z]] into wB (F % 4 == 0 and the host has checked W2's alignment: 16 bytes at a time).
__device__ __forceinline__ void iaf_stage_b(const IafW& f, int l, const IafDims& d, float* wB, int ln) {
    const int n = 2 * d.Z * d.F;
    const float4* W2 = reinterpret_cast<const float4*>(f.W2 + (int64_t)l * n);
#pragma unroll 4
    for (int i0 = 0; i0 < n / 4; i0 += IAF_THREADS) {
        const int i = i0 + ln;
        if (i < n / 4) reinterpret_cast<float4*>(wB)[i] = W2[i];
    }
    if (ln < 2 * d.Z) wB[n + ln] = f.b2[l * 2 * d.Z + ln];
}

// a = elu(W1 z + U h + b1) of the lane's row (wave wv's share of the hidden units): zs rows >= Z and hs rows >= C of the
// padded widths hold 0.
__device__ __forceinline__ void iaf_hidden(const float* wA, const IafDims& d, const IafCol* zs, const IafCol* hs,
                                           IafCol* as, int lane, int wv) {
    const float* Us = wA + d.F * d.ZP;
    const float* b1s = Us + d.F * d.CP;
#pragma unroll 1
    for (int j0 = 4 * wv; j0 < d.F; j0 += 4 * IAF_WAVES) {       // wave wv: every fourth quad of hidden units
        float acc[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[t] = b1s[j0 + t];
#pragma unroll 1
        for (int i0 = 0; i0 < d.ZP; i0 += 4) {
            const float x[4] = {zs[i0][lane], zs[i0 + 1][lane], zs[i0 + 2][lane], zs[i0 + 3][lane]};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = iaf_dot4(*reinterpret_cast<const float4*>(wA + (j0 + t) * d.ZP + i0), x, acc[t]);
        }
#pragma unroll 1
        for (int c0 = 0; c0 < d.CP; c0 += 4) {
            const float x[4] = {hs[c0][lane], hs[c0 + 1][lane], hs[c0 + 2][lane], hs[c0 + 3][lane]};
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = iaf_dot4(*reinterpret_cast<const float4*>(Us + (j0 + t) * d.CP + c0), x, acc[t]);
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) as[j0 + t][lane] = iaf_elu(acc[t]);
    }
}

// m and s of latents d0 .. d0 + 3 (those >= Z redo latent Z - 1) from the lane's a.
__device__ __forceinline__ void iaf_ms4(const float* wB, const IafDims& d, const IafCol* as, int lane, int d0,
                                        float (&m)[4], float (&s)[4]) {
    const float* b2s = wB + 2 * d.Z * d.F;
    int dd[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        dd[t] = min(d0 + t, d.Z - 1);
        m[t] = b2s[dd[t]];
        s[t] = b2s[d.Z + dd[t]];
    }
#pragma unroll 1
    for (int j0 = 0; j0 < d.F; j0 += 4) {
        const float x[4] = {as[j0][lane], as[j0 + 1][lane], as[j0 + 2][lane], as[j0 + 3][lane]};
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            m[t] = iaf_dot4(*reinterpret_cast<const float4*>(wB + dd[t] * d.F + j0), x, m[t]);
            s[t] = iaf_dot4(*reinterpret_cast<const float4*>(wB + (d.Z + dd[t]) * d.F + j0), x, s[t]);
        }
    }
}

// z <- g z + (1 - g) m with g = sigmoid(s): the one place the layer's output is formed.
__device__ __forceinline__ float iaf_gate(float z, float m, float g) {
#pragma clang fp contract(off)
    const float t = (1.f - g) * m;
    return fmaf(g, z, t);
}

// z_0 of the lane's row into zs (rows Z .. ZP - 1 zero) and h into hs (rows C .. CP - 1 zero); ee = |eps|^2, slv = sum lv.
__device__ __forceinline__ void iaf_start(const PhNoise& n, uint32_t nrow, const float* ml, const IafDims& d, IafCol* zs,
                                          IafCol* hs, int lane, float& ee, float& slv, uint32_t& step) {
#pragma clang fp contract(off)
    step = ph_step(n.clk);
    ee = slv = 0.f;
#pragma unroll 1
    for (int q = 0; q < d.ZP / 4; ++q) {
        float e[4];
        ph_noise_eps4(n, step, nrow, (uint32_t)q, e);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = 4 * q + i;
            float z = 0.f;
            if (c < d.Z) {
                const float lv = ml[d.Z + c];
                z = gm_reparam_z(ml[c], e[i], lv);
                ee += e[i] * e[i];
                slv += lv;
            }
            zs[c][lane] = z;
        }
    }
#pragma unroll 1
    for (int c = 0; c < d.CP; ++c) hs[c][lane] = c < d.C ? ml[2 * d.Z + c] : 0.f;
}

struct SampleP {
    const float* ml; int64_t ldml;
    float* z; int64_t ldz;
    float* lp;
    int64_t rows; int k;
};

__global__ __launch_bounds__(IAF_THREADS) void iaf_sample_kernel(SampleP p, IafW f, IafDims d0_, PhNoise n) {
    __shared__ __attribute__((aligned(16))) float wS[IAF_WA > IAF_WB ? IAF_WA : IAF_WB];
    __shared__ IafCol zs[IAF_Z], hs[IAF_C], as[IAF_F], lds[IAF_WAVES];
    const int lane = threadIdx.x & (IAF_ROWS - 1), wv = threadIdx.x >> 6;
    const int64_t r = (int64_t)blockIdx.x * IAF_ROWS + lane, rr = min(r, p.rows - 1);   // rows past the end redo the last
    const int64_t b = rr / p.k;
    const int j = (int)(rr - b * p.k);
    float ee = 0.f, slv = 0.f, ld = 0.f;
    uint32_t step;
    if (wv == 0)                                                 // one wave draws: a row's eps is drawn once
        iaf_start(n, (uint32_t)(b * n.kt + n.j0 + j), p.ml + b * p.ldml, d0_, zs, hs, lane, ee, slv, step);
#pragma unroll 1
    for (int l = 0; l < f.K; ++l) {
        const IafDims d = iaf_dims(d0_);
        __syncthreads();                                         // z of the layer before (or z_0) is whole; wS is free
        iaf_stage_a(f, l, d, wS, iaf_lane(threadIdx.x));
        __syncthreads();
        iaf_hidden(wS, d, zs, hs, as, lane, wv);
        __syncthreads();
        iaf_stage_b(f, l, d, wS, iaf_lane(threadIdx.x));
        __syncthreads();
#pragma unroll 1
        for (int d0 = 4 * wv; d0 < d.Z; d0 += 4 * IAF_WAVES) {   // wave wv: every fourth quad of latents
            float m[4], s[4];
            iaf_ms4(wS, d, as, lane, d0, m, s);
#pragma unroll
            for (int t = 0; t < 4; ++t)
                if (d0 + t < d.Z) {
                    ld -= iaf_softplus(-s[t]);
                    zs[d0 + t][lane] = iaf_gate(zs[d0 + t][lane], m[t], gm_sigmoid(s[t]));
                }
        }
    }
    lds[wv][lane] = ld;                                          // the waves' shares of the log-determinant
    __syncthreads();
    if (wv == 0) {
#pragma clang fp contract(off)
        float zz = 0.f;
#pragma unroll 1
        for (int c = 0; c < d0_.Z; ++c) {
            const float z = zs[c][lane];
            zz += z * z;
        }
        ld = ((lds[0][lane] + lds[1][lane]) + lds[2][lane]) + lds[3][lane];
        if (r < p.rows) {
#pragma unroll 1
            for (int c = 0; c < d0_.Z; ++c) p.z[r * p.ldz + c] = zs[c][lane];
            p.lp[r] = ((0.5f * ee + 0.5f * slv) + ld) - 0.5f * zz;
        }
    }
}

struct ReduceP {                                                 // (the strides as 32-bit words: the host has checked them)
    const float* ml; const float* wn; const float* dzdec;
    float* dml; float* part;
    int ldml, lddz, lddml, B, k, ipw;
};

// sum over the workgroup's rows, ascending, of x[r] y[r] (y == nullptr: of x[r]).
__device__ __forceinline__ float iaf_rows_dot(const float* x, const float* y) {
    float acc = 0.f;
    if (y) {
#pragma unroll 8
        for (int r = 0; r < IAF_ROWS; ++r) acc = fmaf(x[r], y[r], acc);
    } else {
#pragma unroll 8
        for (int r = 0; r < IAF_ROWS; ++r) acc += x[r];
    }
    return acc;
}

__global__ __launch_bounds__(IAF_THREADS) void iaf_reduce_kernel(ReduceP p, IafW f, IafDims d0_, PhNoise n) {
    __shared__ __attribute__((aligned(16))) float wA[IAF_WA];
    __shared__ __attribute__((aligned(16))) float wB[IAF_WB];
    __shared__ IafCol tr[IAF_K * IAF_Z];                         // layer l's input z_l at rows l ZP .. l ZP + ZP - 1
    __shared__ IafCol hs[IAF_C], as[IAF_F], dms[IAF_Z], dss[IAF_Z], gzs[IAF_Z], dhs[IAF_C];
    const int lane = threadIdx.x & (IAF_ROWS - 1), wv = threadIdx.x >> 6, k = p.k;
    const int img = lane / k, j = lane - img * k;
    const int b = (int)blockIdx.x * p.ipw + img;
    const bool on = img < p.ipw && b < p.B;                      // lanes without a row: weight 0, nothing stored
    const int bb = on ? b : (int)blockIdx.x * p.ipw;             // (the workgroup's first image always exists)
    const int jj = on ? j : 0;
    const int64_t r = (int64_t)bb * k + jj;
    const uint32_t nrow = (uint32_t)((int64_t)bb * n.kt + n.j0 + jj);
    const float* ml = p.ml + (int64_t)bb * p.ldml;
    uint32_t step = 0;
    if (wv == 0) {                                               // one wave draws: a row's eps is drawn once
        float ee, slv;
        iaf_start(n, nrow, ml, d0_, tr, hs, lane, ee, slv, step);
#pragma unroll 1
        for (int c = 0; c < d0_.CP; ++c) dhs[c][lane] = 0.f;
    }
    const float wn = on ? p.wn[r] : 0.f;
    float* part = p.part + (int64_t)blockIdx.x * f.K * GM_IAF_PART_STRIDE(d0_.Z, d0_.F, d0_.C);
    // 2 K passes over one body (staging, a, m and s are the same code forward and back): passes 0 .. K-1 go forward, z_{l+1}
    // into the next layer's rows of tr, the last layer's output becoming g_K = wn z_K + dzdec; passes K .. 2K-1 walk back
#pragma unroll 1
    for (int it = 0; it < 2 * f.K; ++it) {
        const IafDims d = iaf_dims(d0_);
        const int Z = d.Z, F = d.F, C = d.C;
        const bool fwd = it < f.K;
        const int l = fwd ? it : 2 * f.K - 1 - it;
        IafCol* zin = tr + l * d.ZP;
        __syncthreads();                                         // the pass before is done with wA, wB and as
        const int tn = iaf_lane(threadIdx.x), ln = tn & (IAF_ROWS - 1);
        iaf_stage_a(f, l, d, wA, tn);
        iaf_stage_b(f, l, d, wB, tn);
        __syncthreads();
        iaf_hidden(wA, d, zin, hs, as, lane, wv);
        __syncthreads();                                         // a is whole: every wave reads all of it
#pragma unroll 1
        for (int d0 = 4 * wv; d0 < d.ZP; d0 += 4 * IAF_WAVES) {  // wave wv: every fourth quad of latents
            float m[4], s[4];
            iaf_ms4(wB, d, as, lane, d0, m, s);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int c = d0 + t;
                const float g = gm_sigmoid(s[t]), zi = zin[c][lane];
                if (fwd) {
                    const float zo = c < Z ? iaf_gate(zi, m[t], g) : 0.f;
                    if (l + 1 < f.K) zin[d.ZP + c][lane] = zo;
                    else gzs[c][lane] = (on && c < Z) ? fmaf(wn, zo, p.dzdec[r * (int64_t)p.lddz + c]) : 0.f;
                } else {
                    float dm = 0.f, ds = 0.f, gz = 0.f;
                    if (c < Z) {
#pragma clang fp contract(off)
                        const float omg = 1.f - g, go = gzs[c][lane];
                        dm = go * omg;
                        ds = (go * (zi - m[t])) * (g * omg) - wn * omg;
                        gz = go * g;
                    }
                    dms[c][lane] = dm;
                    dss[c][lane] = ds;
                    gzs[c][lane] = gz;
                }
            }
        }
        if (fwd) continue;
        float* pW1 = part + (int64_t)l * GM_IAF_PART_STRIDE(Z, F, C);      // [d W1 | d U | d b1 | d W2 | d b2]
        const int oU = F * Z, ob1 = oU + F * C, oW2 = ob1 + F, ob2 = oW2 + 2 * Z * F;
        __syncthreads();
        // d W2 [2Z, F] and d b2 [2Z]: sums over the rows of (dm | ds) a
#pragma unroll 1
        for (int d2 = wv; d2 < 2 * Z; d2 += IAF_WAVES)           // a row of d W2 per wave and trip, lanes over its columns
            if (ln < F) pW1[oW2 + d2 * F + ln] = iaf_rows_dot(d2 < Z ? dms[d2] : dss[d2 - Z], as[ln]);
        if (tn < 2 * Z) pW1[ob2 + tn] = iaf_rows_dot(tn < Z ? dms[tn] : dss[tn - Z], nullptr);
        __syncthreads();
        // da = elu'(a) (W2m^T dm + W2s^T ds) over a, in place (elu' = 1 where a > 0, a + 1 elsewhere)
#pragma unroll 1
        for (int j0 = 4 * wv; j0 < F; j0 += 4 * IAF_WAVES) {
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
            for (int c = 0; c < Z; ++c) {
                const float dm = dms[c][lane], ds = dss[c][lane];
                const float4 wm = *reinterpret_cast<const float4*>(wB + c * F + j0);
                const float4 ws = *reinterpret_cast<const float4*>(wB + (Z + c) * F + j0);
                acc[0] = fmaf(ws.x, ds, fmaf(wm.x, dm, acc[0]));
                acc[1] = fmaf(ws.y, ds, fmaf(wm.y, dm, acc[1]));
                acc[2] = fmaf(ws.z, ds, fmaf(wm.z, dm, acc[2]));
                acc[3] = fmaf(ws.w, ds, fmaf(wm.w, dm, acc[3]));
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float a = as[j0 + t][lane];
                as[j0 + t][lane] = a > 0.f ? acc[t] : (a + 1.f) * acc[t];
            }
        }
        __syncthreads();
        // d W1 [F, Z], d U [F, C], d b1 [F]: sums over the rows of da (z_l | h | 1)
        {
            const int jl = ln >> 5, c = ln & 31;                 // two rows of d W1 / d U per wave and trip
#pragma unroll 1
            for (int j0 = 2 * wv; j0 < F; j0 += 2 * IAF_WAVES) {
                if (c < Z) pW1[(j0 + jl) * Z + c] = iaf_rows_dot(as[j0 + jl], zin[c]);
                if (c < C) pW1[oU + (j0 + jl) * C + c] = iaf_rows_dot(as[j0 + jl], hs[c]);
            }
            if (tn < F) pW1[ob1 + tn] = iaf_rows_dot(as[tn], nullptr);
        }
        // gz = gz' g + W1^T da,  dh += U^T da  (the lane's own columns)
        const float* Us = wA + F * d.ZP;
#pragma unroll 1
        for (int i0 = 4 * wv; i0 < d.ZP; i0 += 4 * IAF_WAVES) {
            float acc[4] = {gzs[i0][lane], gzs[i0 + 1][lane], gzs[i0 + 2][lane], gzs[i0 + 3][lane]};
#pragma unroll 1
            for (int jx = 0; jx < F; ++jx) {
                const float da = as[jx][lane];
                const float4 w = *reinterpret_cast<const float4*>(wA + jx * d.ZP + i0);
                acc[0] = fmaf(w.x, da, acc[0]); acc[1] = fmaf(w.y, da, acc[1]);
                acc[2] = fmaf(w.z, da, acc[2]); acc[3] = fmaf(w.w, da, acc[3]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) gzs[i0 + t][lane] = acc[t];
        }
#pragma unroll 1
        for (int c0 = 4 * wv; c0 < d.CP; c0 += 4 * IAF_WAVES) {
            float acc[4] = {dhs[c0][lane], dhs[c0 + 1][lane], dhs[c0 + 2][lane], dhs[c0 + 3][lane]};
#pragma unroll 1
            for (int jx = 0; jx < F; ++jx) {
                const float da = as[jx][lane];
                const float4 w = *reinterpret_cast<const float4*>(Us + jx * d.CP + c0);
                acc[0] = fmaf(w.x, da, acc[0]); acc[1] = fmaf(w.y, da, acc[1]);
                acc[2] = fmaf(w.z, da, acc[2]); acc[3] = fmaf(w.w, da, acc[3]);
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) dhs[c0 + t][lane] = acc[t];
        }
    }
    // g_0 e into dms (eps rebuilt once more), then per image and column the sum over its samples j ascending
    const IafDims de = iaf_dims(d0_);
    __syncthreads();                                             // g_0 is whole
    if (wv == 0) {
#pragma unroll 1
        for (int q = 0; q < de.ZP / 4; ++q) {
            float e[4];
            ph_noise_eps4(n, step, nrow, (uint32_t)q, e);
#pragma unroll
            for (int i = 0; i < 4; ++i) dms[4 * q + i][lane] = gzs[4 * q + i][lane] * e[i];
        }
    }
    __syncthreads();
    const int Z = de.Z, C = de.C, W = 2 * Z + C;
    IAF_LANES(o, p.ipw * W) {
        const int im = o / W, col = o - im * W;
        const int bo = (int)blockIdx.x * p.ipw + im;
        if (bo >= p.B) continue;
        const int l0 = im * k;
        float acc = 0.f;
        if (col < Z) {
#pragma unroll 1
            for (int s = 0; s < k; ++s) acc += gzs[col][l0 + s];
        } else if (col < 2 * Z) {
            const float sd = expf(p.ml[(int64_t)bo * p.ldml + col] / 2.f);
#pragma unroll 1
            for (int s = 0; s < k; ++s) acc = fmaf(dms[col - Z][l0 + s], sd, acc);
            acc = 0.5f * acc - 0.5f;
        } else {
#pragma unroll 1
            for (int s = 0; s < k; ++s) acc += dhs[col - 2 * Z][l0 + s];
        }
        p.dml[(int64_t)bo * p.lddml + col] = acc;
    }
}

struct StepP {
    const float* part; int nparts;
    float* p[5]; float* g[5]; float* m[5]; float* v[5];          // W1, U, b1, W2, b2
    const int32_t* m_in;
    const float* sched; gm_slot slot;
    float omb1, b2, omb2, eps, wd;
    int K, Z, F, C;
};

__global__ __launch_bounds__(256) void iaf_step_kernel(StepP p) {
    const int Z = p.Z, F = p.F, C = p.C, LS = GM_IAF_PART_STRIDE(Z, F, C);
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.K * LS) return;
    const int l = idx / LS;
    int o = idx - l * LS, t = 0, per = F * Z;                    // t: the tensor, o: the entry within layer l of it
    bool keep = true;
    const int32_t* m_in = p.m_in + l * Z;
    if (o < F * Z) {                                             // W1 (j, i): kept iff m_h[j] >= m_in[i]
        const int jx = o / Z, i = o - jx * Z;
        keep = 1 + (jx * (Z - 1)) / F >= m_in[i];
    } else if ((o -= F * Z) < F * C) {
        t = 1; per = F * C;
    } else if ((o -= F * C) < F) {
        t = 2; per = F;
    } else if ((o -= F) < 2 * Z * F) {                           // W2 (d, j), both halves: kept iff m_in[d] > m_h[j]
        t = 3; per = 2 * Z * F;
        const int d2 = o / F, jx = o - d2 * F;
        keep = m_in[d2 < Z ? d2 : d2 - Z] > 1 + (jx * (Z - 1)) / F;
    } else {
        o -= 2 * Z * F;
        t = 4; per = 2 * Z;
    }
    float G = 0.f;
#pragma unroll 4
    for (int i = 0; i < p.nparts; ++i) G += p.part[(int64_t)i * p.K * LS + idx];   // ascending: whatever the grid was
    const int64_t e = (int64_t)l * per + o;
    if (!keep) {                                                 // a masked entry: it and its moments stay 0.0
        if (p.g[t]) p.g[t][e] = 0.f;
        return;
    }
    if (p.g[t]) p.g[t][e] = G;
    const int64_t si = gm_slot_index(p.slot);
    adam_update(p.p[t][e], G, p.m[t][e], p.v[t][e], p.sched[2 * si], p.sched[2 * si + 1], p.omb1, p.b2, p.omb2, p.eps,
                p.wd, 0.f);
}

inline int iaf_params_fill(const gm_iaf_params* a, int Z, IafW* f, IafDims* d) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(Z >= GM_IAF_MIN_Z && Z <= GM_IAF_MAX_Z && a->K >= 1 && a->K <= GM_IAF_MAX_K);
    GM_CHECK_ARG(a->F >= GM_IAF_MIN_F && a->F <= GM_IAF_MAX_F && a->F % 4 == 0 && a->C >= 0 && a->C <= GM_IAF_MAX_C);
    GM_CHECK_ARG(a->W1 && a->b1 && a->W2 && a->b2 && (a->C == 0 || a->U));
    GM_CHECK_ARG((reinterpret_cast<uintptr_t>(a->W2) & 15) == 0);     // W2 is staged 16 bytes at a time
    const float* ptr[] = {a->W1, a->C ? a->U : nullptr, a->b1, a->W2, a->b2};
    for (int i = 0; i < 5; ++i)
        for (int j = i + 1; j < 5; ++j) GM_CHECK_ARG(!ptr[i] || ptr[i] != ptr[j]);
    f->W1 = a->W1; f->U = a->C ? a->U : nullptr; f->b1 = a->b1; f->W2 = a->W2; f->b2 = a->b2;
    f->K = a->K; f->F = a->F; f->C = a->C;
    d->Z = Z; d->ZP = (Z + 3) & ~3; d->F = a->F; d->C = a->C; d->CP = (a->C + 3) & ~3;
    return 0;
}

inline bool iaf_is_param(const IafW& f, const void* q) {
    return q == f.W1 || (f.U && q == f.U) || q == f.b1 || q == f.W2 || q == f.b2;
}

}  // namespace

#define IAF_CHECK_SHAPE(B, k) GM_CHECK_ARG((B) >= 1 && (k) >= 1 && (k) <= GM_IWAE_MAX_K)

extern "C" int gm_iaf_sample(void* stream, const gm_iwae_noise* a, const gm_iaf_params* fp, const float* ml,
                             int64_t ldml, float* z, int64_t ldz, float* lp, int B, int k, int Z) {
    IAF_CHECK_SHAPE(B, k);
    PhNoise n{};
    IafW f{};
    IafDims d{};
    int rc = iaf_params_fill(fp, Z, &f, &d);
    if (rc) return rc;
    GM_CHECK_ARG(ml && z && lp && ldml >= 2 * Z + f.C && ldz >= Z);
    GM_CHECK_ARG((const float*)z != ml && (const float*)lp != ml && lp != z);
    rc = ph_noise_fill(a, B, k, &n);
    if (rc) return rc;
    GM_CHECK_ARG(!iaf_is_param(f, z) && !iaf_is_param(f, lp) && !iaf_is_param(f, ml));
    SampleP p{ml, ldml, z, ldz, lp, (int64_t)B * k, k};
    const int64_t blocks = (p.rows + IAF_ROWS - 1) / IAF_ROWS;
    GM_CHECK_ARG(blocks < (1ll << 31));
    hipLaunchKernelGGL(iaf_sample_kernel, dim3((unsigned)blocks), dim3(IAF_THREADS), 0, (hipStream_t)stream, p, f, d, n);
    GM_LAUNCH_RET();
}

extern "C" int gm_iaf_reduce(void* stream, const gm_iwae_noise* a, const gm_iaf_params* fp, const float* ml,
                             int64_t ldml, const float* wn, const float* dzdec, int64_t lddz, float* dml,
                             int64_t lddml, float* part, int B, int k, int Z) {
    IAF_CHECK_SHAPE(B, k);
    PhNoise n{};
    IafW f{};
    IafDims d{};
    int rc = iaf_params_fill(fp, Z, &f, &d);
    if (rc) return rc;
    GM_CHECK_ARG(ml && wn && dzdec && dml && part && ldml >= 2 * Z + f.C && lddz >= Z && lddml >= 2 * Z + f.C);
    GM_CHECK_ARG((const float*)dml != ml && (const float*)dml != dzdec && (const float*)dml != wn);
    GM_CHECK_ARG((const float*)part != ml && (const float*)part != dzdec && (const float*)part != wn && part != dml);
    rc = ph_noise_fill(a, B, k, &n);
    if (rc) return rc;
    GM_CHECK_ARG(!iaf_is_param(f, dml) && !iaf_is_param(f, part) && !iaf_is_param(f, ml) && !iaf_is_param(f, wn) &&
                 !iaf_is_param(f, dzdec));
    const int ipw = GM_IAF_PART_ROWS / k > 1 ? GM_IAF_PART_ROWS / k : 1;
    GM_CHECK_ARG(ldml < (1ll << 31) && lddz < (1ll << 31) && lddml < (1ll << 31));
    ReduceP p{ml, wn, dzdec, dml, part, (int)ldml, (int)lddz, (int)lddml, B, k, ipw};
    hipLaunchKernelGGL(iaf_reduce_kernel, dim3((unsigned)GM_IAF_PARTS(B, k)), dim3(IAF_THREADS), 0, (hipStream_t)stream, p,
                       f, d, n);
    GM_LAUNCH_RET();
}

extern "C" int gm_iaf_step(void* stream, const gm_iaf_step_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->K >= 1 && a->K <= GM_IAF_MAX_K && a->Z >= GM_IAF_MIN_Z && a->Z <= GM_IAF_MAX_Z && a->nparts >= 1);
    GM_CHECK_ARG(a->F >= GM_IAF_MIN_F && a->F <= GM_IAF_MAX_F && a->F % 4 == 0 && a->C >= 0 && a->C <= GM_IAF_MAX_C);
    GM_CHECK_ARG(a->part && a->m_in && a->sched);
    const bool grads = a->g[0] != nullptr;
    const void* ptr[22];
    int np = 0;
    ptr[np++] = a->part; ptr[np++] = a->m_in;
    for (int t = 0; t < 5; ++t) {
        if (t == 1 && a->C == 0) continue;                       // no U: its four pointers are ignored
        GM_CHECK_ARG(a->p[t] && a->m[t] && a->v[t] && (a->g[t] != nullptr) == grads);
        ptr[np++] = a->p[t]; ptr[np++] = a->m[t]; ptr[np++] = a->v[t];
        if (grads) ptr[np++] = a->g[t];
    }
    for (int i = 0; i < np; ++i)
        for (int j = i + 1; j < np; ++j) GM_CHECK_ARG(ptr[i] != ptr[j]);
    StepP p{};
    p.part = a->part; p.nparts = a->nparts;
    for (int t = 0; t < 5; ++t) {
        const bool has = !(t == 1 && a->C == 0);
        p.p[t] = has ? a->p[t] : nullptr; p.g[t] = has ? a->g[t] : nullptr;
        p.m[t] = has ? a->m[t] : nullptr; p.v[t] = has ? a->v[t] : nullptr;
    }
    p.m_in = a->m_in; p.sched = a->sched; p.slot = a->sched_slot;
    p.omb1 = (float)(1.0 - a->beta1); p.b2 = (float)a->beta2; p.omb2 = (float)(1.0 - a->beta2);
    p.eps = (float)a->eps; p.wd = (float)a->weight_decay;
    p.K = a->K; p.Z = a->Z; p.F = a->F; p.C = a->C;
    const int total = a->K * GM_IAF_PART_STRIDE(a->Z, a->F, a->C);
    hipLaunchKernelGGL(iaf_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
