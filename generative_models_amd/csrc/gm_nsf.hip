// Neural spline flow (Durkan, Bortoli, Murray & Papamakarios, arXiv 1906.04032; nsf.py holds the contract; gm_hip.h;
// DESIGN.md section 37; the arithmetic in gm_nsf.h).
//
// The row work of a rational-quadratic coupling, between the conditioner's GEMMs: one 256-thread workgroup per row,
// thread i the pixels i, i + 256, ... of the transformed half one at a time.  ST is parameter-major (column p Dt + j is
// parameter p of pixel j), so each of a pixel's P = 3 bins - 1 dword loads is consecutive across the wave; there is no
// vector arm and any leading dimension >= P Dt is legal.  bins is a template parameter (4, 8, 16): everything a pixel
// needs stays in registers.
//   nsf_couple_kernel      y_t and logdet += the row's sum of log dy/dx (nvp_row_sum: thread partials in pixel order, the
//                          wave butterfly, the four waves in order; read-add-write by thread 0); or the inverse, which
//                          skips the sum and its barrier
//   nsf_couple_bwd_kernel  dST (every column, zeros in the tails) and dx_t from the cotangent's one or two addends
// No atomics, no scratch: the same bits on every run, graph or eager.
#include "gm_nvp.h"
#include "gm_nsf.h"

namespace {

// Pixel j's P parameters: column q Dt + j of the row, the offset advanced by a running add (one register, where P
// multiples of Dt would each hold a scalar one).
template <int P> __device__ __forceinline__ void nsf_load(const float* st, int j, int Dt, float* th) {
    int o = j;
#pragma unroll
    for (int q = 0; q < P; ++q, o += Dt) th[q] = st[o];
}

struct CoupleP {
    const float* st; int64_t ldst; const float* in; int64_t ldin; float* out; int64_t ldout; float* logdet;
    float bound; int inverse, Dt;
};

template <int BINS> __global__ __launch_bounds__(256) void nsf_couple_kernel(CoupleP p) {
    __shared__ float sh[4];
    constexpr int P = 3 * BINS - 1;
    const int64_t r = blockIdx.x;
    const float* st = p.st + r * p.ldst;
    const float* in = p.in + r * p.ldin;
    float* out = p.out + r * p.ldout;
    float acc = 0.f;
    for (int j = threadIdx.x; j < p.Dt; j += 256) {
        const float v = in[j];
        float o = v;
        if (v > -p.bound && v < p.bound) {                       // the tails are the identity: no parameter is read
            float th[P];
            nsf_load<P>(st, j, p.Dt, th);
            NsfKnots<BINS> K;
            nsf_knots<BINS>(th, p.bound, K);
            const NsfBin b = nsf_bin<BINS>(K, p.bound, v, p.inverse != 0);
            if (p.inverse) {
                o = nsf_inverse(b, v);
            } else {
                const NsfPoint pt = nsf_point_of_x(b, v);
                o = nsf_value(b, pt);
                acc += nsf_logderiv(pt);
            }
        }
        out[j] = o;
    }
    if (p.inverse) return;                                       // uniform: the whole grid
    const float tot = nvp_row_sum(acc, sh);
    if (threadIdx.x == 0) p.logdet[r] = p.logdet[r] + tot;
}

struct BwdP {
    const float* st; int64_t ldst; const float* x; int64_t ldx; const float* g0; int64_t ldg0; const float* g1;
    int64_t ldg1; float* dst; int64_t lddst; float* dx; int64_t lddx; float c, bound; int Dt;
};

template <int BINS> __global__ __launch_bounds__(256) void nsf_couple_bwd_kernel(BwdP p) {
    constexpr int P = 3 * BINS - 1;
    const int64_t r = blockIdx.x;
    const float* st = p.st + r * p.ldst;
    const float* x = p.x + r * p.ldx;
    const float* g0 = p.g0 + r * p.ldg0;
    const float* g1 = p.g1 ? p.g1 + r * p.ldg1 : nullptr;
    float* dst = p.dst + r * p.lddst;
    float* dx = p.dx ? p.dx + r * p.lddx : nullptr;
    for (int j = threadIdx.x; j < p.Dt; j += 256) {
        const float v = x[j];
        float g = g0[j];
        if (g1) g = g + g1[j];
        float d = g;
        float dth[P];
#pragma unroll
        for (int q = 0; q < P; ++q) dth[q] = 0.f;
        if (v > -p.bound && v < p.bound) {
            float th[P];
            nsf_load<P>(st, j, p.Dt, th);
            NsfKnots<BINS> K;
            nsf_knots<BINS>(th, p.bound, K);
            const NsfBin b = nsf_bin<BINS>(K, p.bound, v, false);
            d = nsf_backward<BINS>(th, K, b, p.bound, v, g, p.c, dth);
        }
        int o = j;
#pragma unroll
        for (int q = 0; q < P; ++q, o += p.Dt) dst[o] = dth[q];  // the GEMM behind reads every column
        if (dx) dx[j] = d;
    }
}

inline bool rows_ok(int B) { return B >= 1; }
inline bool dt_ok(int Dt) { return Dt >= 1 && Dt <= (GM_NVP_MAX_D + 1) / 2; }
inline bool bins_ok(int n) { return n == GM_NSF_MIN_BINS || n == 8 || n == GM_NSF_MAX_BINS; }
inline bool bound_ok(float b) { return b > 0.f && b <= (float)GM_NSF_MAX_TAIL; }      // false for a NaN

}  // namespace

extern "C" int gm_nsf_couple(void* stream, const gm_nsf_couple_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(rows_ok(a->B) && dt_ok(a->Dt) && bins_ok(a->bins) && bound_ok(a->tail_bound));
    const int64_t width = (int64_t)(3 * a->bins - 1) * a->Dt;
    GM_CHECK_ARG(a->st && a->inp && a->out && a->ldst >= width && a->ldin >= a->Dt && a->ldout >= a->Dt);
    GM_CHECK_ARG((const float*)a->out != a->st && (const float*)a->out != a->inp);
    GM_CHECK_ARG(a->inverse == 0 || a->inverse == 1);
    GM_CHECK_ARG(a->inverse || (a->logdet && a->logdet != a->out && (const float*)a->logdet != a->st &&
                                (const float*)a->logdet != a->inp));
    const CoupleP p{a->st, a->ldst, a->inp, a->ldin, a->out, a->ldout, a->logdet, a->tail_bound, a->inverse, a->Dt};
    const dim3 grid((unsigned)a->B), block(256);
    if (a->bins == 4) hipLaunchKernelGGL(nsf_couple_kernel<4>, grid, block, 0, (hipStream_t)stream, p);
    else if (a->bins == 8) hipLaunchKernelGGL(nsf_couple_kernel<8>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(nsf_couple_kernel<16>, grid, block, 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_nsf_couple_bwd(void* stream, const gm_nsf_couple_bwd_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(rows_ok(a->B) && dt_ok(a->Dt) && bins_ok(a->bins) && bound_ok(a->tail_bound) &&
                 __builtin_isfinite(a->c));
    const int64_t width = (int64_t)(3 * a->bins - 1) * a->Dt;
    GM_CHECK_ARG(a->st && a->x && a->g0 && a->dst && a->ldst >= width && a->ldx >= a->Dt && a->ldg0 >= a->Dt &&
                 a->lddst >= width);
    GM_CHECK_ARG(!a->g1 || a->ldg1 >= a->Dt);
    GM_CHECK_ARG(!a->dx || (a->lddx >= a->Dt && a->dx != a->dst));
    for (const float* in : {a->st, a->x, a->g0, a->g1})
        GM_CHECK_ARG(!in || ((const float*)a->dst != in && (const float*)a->dx != in));
    const BwdP p{a->st, a->ldst, a->x, a->ldx, a->g0, a->ldg0, a->g1, a->ldg1, a->dst, a->lddst, a->dx, a->lddx, a->c,
                 a->tail_bound, a->Dt};
    const dim3 grid((unsigned)a->B), block(256);
    if (a->bins == 4) hipLaunchKernelGGL(nsf_couple_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, p);
    else if (a->bins == 8) hipLaunchKernelGGL(nsf_couple_bwd_kernel<8>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(nsf_couple_bwd_kernel<16>, grid, block, 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
