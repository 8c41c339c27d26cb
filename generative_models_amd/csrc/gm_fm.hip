// Flow matching (flowmatch.py holds the contract; gm_hip.h; the rule in gm_fm.h).
//
// gm_fm_qsample, gm_gather_rows[_bits]_fm_qsample: per row the grid index j, [y_t | temb[j]] (the field's input row),
//   the target u = y1 - y0, the preprocessing log-determinant and -- the gathering forms -- the clean row exactly as
//   gm_gather_rows[_bits] writes it.  One 256-thread workgroup per row; 16-byte accesses where the rows allow them,
//   element by element otherwise, the same order of operations on both paths.
// gm_fm_div: the exact divergence of the field, div[b] = m2[b]^T Q m1[b], on v_mfma_f32_32x32x2_f32.  A wave owns 32
//   rows b (the MFMA's columns) and 32 indices i (its rows) and runs over all j: Q's rows are the A operand, the 0 / 1
//   pattern [H1 > 0] -- formed in registers from the H1 loads -- the B operand, so that a lane ends up with one row b
//   and 16 of the 32 i.  The epilogue keeps the products whose H2[b, i] is lit, adds them in register order, adds the
//   lane's partner (the other 16 i) and writes ONE partial per (tile, row).  Neither a mask nor the [B, H] product is
//   stored.  The tiles' partials are added in tile order by fm_div_finish_kernel or by the stage kernel: the order
//   depends on H alone, never on B or on the launch.  No LDS, no barrier, no atomics.
// gm_fm_stage: one solver stage in place (the rule in gm_fm.h), its coefficients row s of a device table, s a gm_slot
//   over a device counter, so that a captured graph of G evaluations replays n_eval / G times; the last workgroup to
//   arrive advances the counter (gm_ddpm_reverse's scheme).
#include "gm_fm.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct QsP { const float* x; int64_t ldx; int I, vec; };

__global__ __launch_bounds__(256) void fm_qsample_kernel(QsP p, FmNoiseP n, FmTabP s, FmOutP o) {
    __shared__ float sh[4];
    const int64_t b = blockIdx.x;
    fm_qsample_row(n, s, o, b, p.I, p.vec, nullptr, DdpmRow{p.x + b * p.ldx, nullptr}, sh);
}

__global__ __launch_bounds__(256) void fm_gather_qsample_kernel(GatherP g, FmNoiseP n, FmTabP s, FmOutP o) {
    __shared__ float sh[4];
    const int64_t b = blockIdx.x;
    int64_t r = (g.idx + gm_slot_offset(g.idx_slot))[b];
    if (r < 0 || r >= g.n_rows) r = 0;     // never fault on a corrupt index; parity tests catch it
    const DdpmRow rs{g.bits ? nullptr : g.data + r * (int64_t)g.row_elems, g.bits ? g.bits + r * (int64_t)g.wpr : nullptr};
    fm_qsample_row(n, s, o, b, g.row_elems, g.vec, g.out + b * g.ld_out, rs, sh);
}

// ---- the divergence ---------------------------------------------------------------------------------------------------
struct DivP {
    const float* H1; int64_t ld1; const float* H2; int64_t ld2; const float* Q; int64_t ldq; float* part;
    int B, H, vec1, vecq;
};

// Elements k .. k + 3 of a row of n floats, zeros past the end: one 16-byte load when vec (n % 4 == 0, aligned rows).
static __device__ __forceinline__ float4 fm_load4(const float* row, int k, int n, int vec) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (vec) {
        if (k < n) v = *reinterpret_cast<const float4*>(row + k);
        return v;
    }
    if (k < n) v.x = row[k];
    if (k + 1 < n) v.y = row[k + 1];
    if (k + 2 < n) v.z = row[k + 2];
    if (k + 3 < n) v.w = row[k + 3];
    return v;
}

// v_mfma_f32_32x32x2_f32: lane l feeds A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31]; D[i][j] sits in lane
// j + 32 * ((i >> 2) & 1), register (i & 3) + 4 * (i >> 3).  A lane reads 4 consecutive k of its row with one load: MFMA
// e of k-group g sums k = 8g + e and 8g + 4 + e (the same permutation on both operands: the sum over k is complete).
__global__ __launch_bounds__(256) void fm_div_kernel(DivP p) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int tile = blockIdx.y * 4 + w, i0 = tile * 32;
    if (i0 >= p.H) return;                 // the whole wave; the kernel has no barrier
    const int b0 = blockIdx.x * 32;
    const int bj = min(b0 + r, p.B - 1);   // rows past B repeat row B - 1 and are not written
    const bool qin = i0 + r < p.H;
    const float* q = p.Q + (int64_t)min(i0 + r, p.H - 1) * p.ldq;
    const float* h1 = p.H1 + (int64_t)bj * p.ld1;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.0f;
    const int nk = (p.H + 7) >> 3;
    float4 a = fm_load4(q, 4 * h, p.H, p.vecq), hv = fm_load4(h1, 4 * h, p.H, p.vec1);
    for (int g = 0; g < nk; ++g) {
        float4 an = make_float4(0.f, 0.f, 0.f, 0.f), hn = an;
        if (g + 1 < nk) {                  // the next group's loads fly while this group's MFMAs issue
            an = fm_load4(q, 8 * (g + 1) + 4 * h, p.H, p.vecq);
            hn = fm_load4(h1, 8 * (g + 1) + 4 * h, p.H, p.vec1);
        }
        if (!qin) a = make_float4(0.f, 0.f, 0.f, 0.f);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, hv.x > 0.f ? 1.f : 0.f, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, hv.y > 0.f ? 1.f : 0.f, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, hv.z > 0.f ? 1.f : 0.f, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, hv.w > 0.f ? 1.f : 0.f, acc, 0, 0, 0);
        a = an;
        hv = hn;
    }
    // this lane: row b0 + r against i = i0 + (g & 3) + 4 h + 8 (g >> 2), g = 0 .. 15
    const float* h2 = p.H2 + (int64_t)bj * p.ld2;
    float s = 0.f;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int i = i0 + (g & 3) + 4 * h + 8 * (g >> 2);
        const bool lit = i < p.H && h2[min(i, p.H - 1)] > 0.f;
        s += lit ? acc[g] : 0.f;
    }
    s += __shfl_xor(s, 32, 64);
    if (h == 0 && b0 + r < p.B) p.part[(int64_t)tile * p.B + b0 + r] = s;
}

__global__ __launch_bounds__(256) void fm_div_finish_kernel(const float* part, float* div, int B, int tiles) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    float s = part[b];
    for (int t = 1; t < tiles; ++t) s += part[(int64_t)t * B + b];
    div[b] = s;
}

// ---- one solver stage ---------------------------------------------------------------------------------------------------
struct StageP {
    const float* k; int64_t ldk; float* base; int64_t ldb; float* acc; int64_t lda; float* xin; int64_t ldin;
    float* L; const float* div; int64_t div_stride; int div_parts;
    const float* tab; gm_slot slot; const float* temb; float* traj; int64_t traj_stride;
    int64_t* tick; unsigned int* done;
    int I, E, T, S, stages, vec, vec_tail;
};

__global__ __launch_bounds__(256) void fm_stage_kernel(StageP p) {
    const int64_t b = blockIdx.x;
    const int64_t si = gm_slot_index(p.slot);
    const int s = (int)(si < 0 ? 0 : si >= p.S ? p.S - 1 : si);          // never read outside the table
    const float* c = p.tab + (int64_t)s * 8;
    const float ha = c[0], hb = c[1];
    const bool first = c[2] != 0.f, last = c[3] != 0.f;
    const int jn = (int)c[4];
    const float* k = p.k + b * p.ldk;
    float* base = p.base + b * p.ldb;
    float* acc = p.acc + b * p.lda;
    float* x = p.xin + b * p.ldin;
    float* tr = (p.traj && last) ? p.traj + ((int64_t)(s / p.stages) + 1) * p.traj_stride + b * (int64_t)p.I : nullptr;
    if (p.vec) {
        for (int q = threadIdx.x; q < (p.I >> 2); q += 256) {
            const float4 kv = reinterpret_cast<const float4*>(k)[q];
            float4 bv = reinterpret_cast<const float4*>(base)[q];
            float4 av = first ? make_float4(0.f, 0.f, 0.f, 0.f) : reinterpret_cast<const float4*>(acc)[q];
            const float4 y = make_float4(fm_stage1(kv.x, bv.x, av.x, ha, hb, first, last),
                                         fm_stage1(kv.y, bv.y, av.y, ha, hb, first, last),
                                         fm_stage1(kv.z, bv.z, av.z, ha, hb, first, last),
                                         fm_stage1(kv.w, bv.w, av.w, ha, hb, first, last));
            reinterpret_cast<float4*>(acc)[q] = av;
            if (last) reinterpret_cast<float4*>(base)[q] = bv;
            reinterpret_cast<float4*>(x)[q] = y;
            if (tr) reinterpret_cast<float4*>(tr)[q] = y;
        }
    } else {
        for (int i = threadIdx.x; i < p.I; i += 256) {
            float bv = base[i], av = first ? 0.f : acc[i];
            const float y = fm_stage1(k[i], bv, av, ha, hb, first, last);
            acc[i] = av;
            if (last) base[i] = bv;
            x[i] = y;
            if (tr) tr[i] = y;
        }
    }
    if (p.div && threadIdx.x == 0) {       // the row's log-determinant pair: the same rule on the divergence
        float d = p.div[b];
        for (int t = 1; t < p.div_parts; ++t) d += p.div[(int64_t)t * p.div_stride + b];
        float lb = p.L[2 * b], la = first ? 0.f : p.L[2 * b + 1];
        fm_stage1(d, lb, la, ha, hb, first, last);
        p.L[2 * b + 1] = la;
        if (last) p.L[2 * b] = lb;
    }
    if (jn >= 0) ddpm_tail(x + p.I, p.temb + (int64_t)min(jn, p.T) * p.E, p.E, p.vec_tail);
    if (!p.done) return;
    __syncthreads();                       // every thread's slot read is behind it
    if (threadIdx.x == 0) {
        const unsigned int arrived = __hip_atomic_fetch_add(p.done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (arrived == gridDim.x - 1) {
            __hip_atomic_store(p.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (p.tick) *p.tick += 1;
        }
    }
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool shape_ok(int I, int E, int T) {
    return I >= 1 && I <= GM_DDPM_MAX_I && E >= GM_DDPM_MIN_E && E <= GM_DDPM_MAX_E && E % 4 == 0 && T >= 2 &&
           T <= GM_DDPM_MAX_T;
}

// Host: the device forms of the three argument blocks of a path sample over B rows of I pixels, or GM_EINVAL.
// *vec: whether every output row allows 16-byte accesses (the caller ands in its own source rows).
inline int qs_fill(const gm_fm_noise* a, const gm_fm_tables* s, const gm_fm_out* o, int64_t B, int I, FmNoiseP* n,
                   FmTabP* t, FmOutP* out, int* vec) {
    GM_CHECK_ARG(a != nullptr && s != nullptr && o != nullptr);
    GM_CHECK_ARG(s->tt && s->tc && s->temb && shape_ok(I, s->E, s->T));
    GM_CHECK_ARG(o->xin && o->u && o->logdet && o->ldin >= (int64_t)I + s->E && o->ldu >= I && o->xin != o->u);
    GM_CHECK_ARG(!o->y1 || (o->ldy1 >= I && o->y1 != o->xin && o->y1 != o->u));
    GM_CHECK_ARG(!o->y0 || (o->ldy0 >= I && o->y0 != o->xin && o->y0 != o->u && o->y0 != o->y1));
    GM_CHECK_ARG(o->logdet != o->xin && o->logdet != o->u && (void*)o->j != (void*)o->logdet);
    GM_CHECK_ARG(o->alpha >= 0.f && o->alpha < 0.5f && o->levels >= 2 && o->levels <= GM_NVP_MAX_LEVELS);
    GM_CHECK_ARG(a->row0 >= 0 && B >= 1 && B < (1ll << 31) && a->row0 + B <= (1ll << 32));
    *n = FmNoiseP{a->seed, a->tag_d, a->tag_t, a->tag_n, PhClock{a->step_ctr, a->step_base, a->step_add}, a->row0};
    *t = FmTabP{s->tt, s->tc, s->temb, s->T, s->E};
    const bool rows4 = I % 4 == 0 && o->ldin % 4 == 0 && al16(o->xin);
    NvpPre c;
    c.alpha = o->alpha; c.om2a = 1.f - 2.f * o->alpha; c.log_om2a = logf(c.om2a); c.lv = (float)o->levels;
    *out = FmOutP{o->xin, o->ldin, o->u, o->ldu, o->logdet, o->j, o->y1, o->ldy1, o->y0, o->ldy0, c,
                  (rows4 && al16(s->temb)) ? 1 : 0};
    *vec = (rows4 && o->ldu % 4 == 0 && al16(o->u) && (!o->y1 || (o->ldy1 % 4 == 0 && al16(o->y1))) &&
            (!o->y0 || (o->ldy0 % 4 == 0 && al16(o->y0)))) ? 1 : 0;
    return 0;
}

int gather_qsample(void* stream, const gm_fm_noise* a, const gm_fm_tables* s, const gm_fm_out* o, GatherP& g) {
    FmNoiseP n{}; FmTabP t{}; FmOutP out{};
    int vec = 0;
    const int rc = qs_fill(a, s, o, g.B, g.row_elems, &n, &t, &out, &vec);
    if (rc) return rc;
    for (const float* w : {(const float*)o->xin, (const float*)o->u, (const float*)o->logdet, (const float*)o->y1,
                           (const float*)o->y0})
        GM_CHECK_ARG(!w || (w != g.out && w != g.data));
    g.vec = g.vec && vec;
    hipLaunchKernelGGL(fm_gather_qsample_kernel, dim3((unsigned)g.B), dim3(256), 0, (hipStream_t)stream, g, n, t, out);
    GM_LAUNCH_RET();
}

}  // namespace

extern "C" int gm_fm_qsample(void* stream, const gm_fm_noise* a, const gm_fm_tables* s, const gm_fm_out* o,
                             const float* x, int64_t ldx, int64_t rows, int I) {
    FmNoiseP n{}; FmTabP t{}; FmOutP out{};
    int vec = 0;
    const int rc = qs_fill(a, s, o, rows, I, &n, &t, &out, &vec);
    if (rc) return rc;
    GM_CHECK_ARG(x && ldx >= I);
    for (const float* w : {(const float*)o->xin, (const float*)o->u, (const float*)o->logdet, (const float*)o->y1,
                           (const float*)o->y0})
        GM_CHECK_ARG(w != x);
    QsP p{x, ldx, I, (vec && ldx % 4 == 0 && al16(x)) ? 1 : 0};
    hipLaunchKernelGGL(fm_qsample_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p, n, t, out);
    GM_LAUNCH_RET();
}

extern "C" int gm_gather_rows_fm_qsample(void* stream, const gm_fm_noise* a, const gm_fm_tables* s, const gm_fm_out* o,
                                         const float* data, int64_t n_rows, const int64_t* idx, gm_slot idx_slot,
                                         float* out, int64_t ld_out, int B, int row_elems) {
    GatherP g{};
    const int rc = gm_gather_fill(data, n_rows, idx, idx_slot, out, ld_out, B, row_elems, &g);
    if (rc) return rc;
    return gather_qsample(stream, a, s, o, g);
}

extern "C" int gm_gather_rows_bits_fm_qsample(void* stream, const gm_fm_noise* a, const gm_fm_tables* s,
                                              const gm_fm_out* o, const uint32_t* bits, int words_per_row,
                                              int64_t n_rows, const int64_t* idx, gm_slot idx_slot, float* out,
                                              int64_t ld_out, int B, int row_elems) {
    GatherP g{};
    const int rc = gm_gather_fill_bits(bits, words_per_row, n_rows, idx, idx_slot, out, ld_out, B, row_elems, &g);
    if (rc) return rc;
    return gather_qsample(stream, a, s, o, g);
}

extern "C" int gm_fm_div(void* stream, const gm_fm_div_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->H1 && a->H2 && a->Q && a->part && a->B >= 1 && a->B <= (1 << 30) && a->H >= 1 && a->H <= GM_FM_MAX_H);
    GM_CHECK_ARG(a->ld1 >= a->H && a->ld2 >= a->H && a->ldq >= a->H);
    const int tiles = (a->H + 31) / 32;
    GM_CHECK_ARG(a->part_floats >= (int64_t)tiles * a->B);
    for (const float* in : {a->H1, a->H2, a->Q})
        GM_CHECK_ARG((const float*)a->part != in && (const float*)a->div != in);
    GM_CHECK_ARG(a->div != a->part);
    DivP p{a->H1, a->ld1, a->H2, a->ld2, a->Q, a->ldq, a->part, a->B, a->H,
           (a->H % 4 == 0 && a->ld1 % 4 == 0 && al16(a->H1)) ? 1 : 0,
           (a->H % 4 == 0 && a->ldq % 4 == 0 && al16(a->Q)) ? 1 : 0};
    const dim3 grid((unsigned)(((int64_t)a->B + 31) / 32), (unsigned)((tiles + 3) / 4));
    hipLaunchKernelGGL(fm_div_kernel, grid, dim3(256), 0, (hipStream_t)stream, p);
    if (a->div)
        hipLaunchKernelGGL(fm_div_finish_kernel, dim3((unsigned)(((int64_t)a->B + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           (const float*)a->part, a->div, a->B, tiles);
    GM_LAUNCH_RET();
}

extern "C" int gm_fm_stage(void* stream, const gm_fm_stage_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->k && a->base && a->acc && a->xin && a->tab && a->temb && shape_ok(a->I, a->E, a->T));
    GM_CHECK_ARG(a->rows >= 1 && a->S >= 1 && a->stages >= 1 && a->stages <= 4 && a->S % a->stages == 0);
    GM_CHECK_ARG(a->ldk >= a->I && a->ldb >= a->I && a->lda >= a->I && a->ldin >= (int64_t)a->I + a->E);
    GM_CHECK_ARG(a->slot.stride == 8);
    GM_CHECK_ARG((const float*)a->xin != a->k && (const float*)a->base != a->k && (const float*)a->acc != a->k &&
                 a->base != a->acc && a->base != a->xin && a->acc != a->xin);
    GM_CHECK_ARG(!a->div || (a->L && a->div_parts >= 1 && a->div_parts <= GM_FM_MAX_H / 32 &&
                             (a->div_parts == 1 || a->div_stride >= a->rows) && (const float*)a->L != a->div));
    GM_CHECK_ARG(!a->traj || (a->traj_stride >= (int64_t)a->rows * a->I && a->traj != a->xin && a->traj != a->base &&
                              a->traj != a->acc));
    GM_CHECK_ARG(!a->tick || a->done);
    const bool rows4 = a->I % 4 == 0 && a->ldin % 4 == 0 && al16(a->xin);
    const bool v = rows4 && a->ldk % 4 == 0 && al16(a->k) && a->ldb % 4 == 0 && al16(a->base) && a->lda % 4 == 0 &&
                   al16(a->acc) && (!a->traj || (al16(a->traj) && a->traj_stride % 4 == 0));
    StageP p{a->k, a->ldk, a->base, a->ldb, a->acc, a->lda, a->xin, a->ldin, a->L, a->div, a->div_stride,
             a->div ? a->div_parts : 0, a->tab, a->slot, a->temb, a->traj, a->traj_stride, a->tick, a->done,
             a->I, a->E, a->T, a->S, a->stages, v ? 1 : 0, (rows4 && al16(a->temb)) ? 1 : 0};
    p.slot.stride = 1;                     // the kernel takes the row index and scales it itself
    hipLaunchKernelGGL(fm_stage_kernel, dim3((unsigned)a->rows), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
