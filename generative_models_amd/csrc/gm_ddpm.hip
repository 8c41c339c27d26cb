// Denoising diffusion (ddpm.py; gm_hip.h; the rule in gm_ddpm.h).  Every kernel: one 256-thread workgroup per row.
//
// gm_ddpm_qsample, gm_gather_rows[_bits]_qsample: per row the timestep t, [x_t | temb[t]] (the denoiser's input row), the
//   noise eps and -- the gathering forms -- the clean row exactly as gm_gather_rows[_bits] writes it.  16-byte accesses
//   where the rows allow them, element by element otherwise.
// gm_ddpm_loss: dA = (2 scale) (out - eps) and the row's sum of (out - eps)^2: per thread over its quads in order, the
//   wave butterfly, the four waves in order.
// gm_ddpm_reverse: one sampler step in place on the input rows, its coefficients row s of a device table, s a gm_slot
//   over a device counter, so that a captured graph of G steps replays S / G times; temb[t_next] into the rows' tails;
//   the last workgroup to arrive advances the counter.  gm_ddpm_prior: x_T and temb[t_first].
// No floating-point atomics, fixed reduction orders: the same bits on every run, graph or eager.
#include "gm_ddpm.h"

namespace {

struct QsP { const float* x; int64_t ldx; int I, vec; };

__global__ __launch_bounds__(256) void ddpm_qsample_kernel(QsP p, DdpmNoiseP n, DdpmTabP s, DdpmOutP o) {
    const int64_t b = blockIdx.x;
    ddpm_qsample_row(n, s, o, b, p.I, p.vec, nullptr, DdpmRow{p.x + b * p.ldx, nullptr});
}

__global__ __launch_bounds__(256) void ddpm_gather_qsample_kernel(GatherP g, DdpmNoiseP n, DdpmTabP s, DdpmOutP o) {
    const int64_t b = blockIdx.x;
    int64_t r = (g.idx + gm_slot_offset(g.idx_slot))[b];
    if (r < 0 || r >= g.n_rows) r = 0;     // never fault on a corrupt index; parity tests catch it
    const DdpmRow rs{g.bits ? nullptr : g.data + r * (int64_t)g.row_elems, g.bits ? g.bits + r * (int64_t)g.wpr : nullptr};
    ddpm_qsample_row(n, s, o, b, g.row_elems, g.vec, g.out + b * g.ld_out, rs);
}

struct LossP {
    const float* out; int64_t ldo; const float* eps; int64_t lde;
    float* dA; int64_t lda; float* part; float scale2; int I, vec;
};

__global__ __launch_bounds__(256) void ddpm_loss_kernel(LossP p) {
    __shared__ float sh[4];
    const int64_t b = blockIdx.x;
    const float* o = p.out + b * p.ldo;
    const float* e = p.eps + b * p.lde;
    float* dA = p.dA ? p.dA + b * p.lda : nullptr;
    float acc = 0.f;
    if (p.vec) {
        for (int q = threadIdx.x; q < (p.I >> 2); q += 256) {
            const float4 a = reinterpret_cast<const float4*>(o)[q], c = reinterpret_cast<const float4*>(e)[q];
            const float d0 = a.x - c.x, d1 = a.y - c.y, d2 = a.z - c.z, d3 = a.w - c.w;
            if (dA) reinterpret_cast<float4*>(dA)[q] = make_float4(p.scale2 * d0, p.scale2 * d1, p.scale2 * d2, p.scale2 * d3);
            acc = fmaf(d0, d0, acc);
            acc = fmaf(d1, d1, acc);
            acc = fmaf(d2, d2, acc);
            acc = fmaf(d3, d3, acc);
        }
    } else {
        for (int i = threadIdx.x; i < p.I; i += 256) {
            const float d = o[i] - e[i];
            if (dA) dA[i] = p.scale2 * d;
            acc = fmaf(d, d, acc);
        }
    }
    acc = gm_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) p.part[b] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

struct RevP {
    float* xin; int64_t ldin; const float* eps; int64_t lde;
    const float* coef; gm_slot slot; const float* temb;
    float* traj; int64_t traj_stride;
    uint64_t seed; int64_t* tick; unsigned int* done;
    int I, E, T, S, clip, vec, vec_tail;
};

__global__ __launch_bounds__(256) void ddpm_reverse_kernel(RevP p) {
    const int64_t b = blockIdx.x;
    const int64_t si = gm_slot_index(p.slot);
    const int s = (int)(si < 0 ? 0 : si >= p.S ? p.S - 1 : si);          // never read outside the table
    const float* c = p.coef + (int64_t)s * 8;
    const float s1 = c[0], sa = c[1], sap = c[2], dir = c[3], sig = c[4];
    const int tn = (int)c[5];
    float* x = p.xin + b * p.ldin;
    const float* e = p.eps + b * p.lde;
    float* tr = p.traj ? p.traj + ((int64_t)s + 1) * p.traj_stride + b * (int64_t)p.I : nullptr;
    const bool noisy = sig != 0.f;         // eta = 0 and the last step draw nothing: no bit depends on the seed
    if (p.vec) {
        for (int q = threadIdx.x; q < (p.I >> 2); q += 256) {
            const float4 xt = reinterpret_cast<const float4*>(x)[q], ev = reinterpret_cast<const float4*>(e)[q];
            const float4 z = noisy ? ph_normals(p.seed, (uint32_t)q, (uint32_t)s, (uint32_t)b, GM_DDPM_TAG_S)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 y = make_float4(ddpm_reverse1(xt.x, ev.x, z.x, s1, sa, sap, dir, sig, p.clip),
                                         ddpm_reverse1(xt.y, ev.y, z.y, s1, sa, sap, dir, sig, p.clip),
                                         ddpm_reverse1(xt.z, ev.z, z.z, s1, sa, sap, dir, sig, p.clip),
                                         ddpm_reverse1(xt.w, ev.w, z.w, s1, sa, sap, dir, sig, p.clip));
            reinterpret_cast<float4*>(x)[q] = y;
            if (tr) reinterpret_cast<float4*>(tr)[q] = y;
        }
    } else {
        for (int q = threadIdx.x; 4 * q < p.I; q += 256) {
            const float4 z = noisy ? ph_normals(p.seed, (uint32_t)q, (uint32_t)s, (uint32_t)b, GM_DDPM_TAG_S)
                                   : make_float4(0.f, 0.f, 0.f, 0.f);
            const int cnt = min(4, p.I - 4 * q);
            for (int j = 0; j < cnt; ++j) {
                const int i = 4 * q + j;
                const float y = ddpm_reverse1(x[i], e[i], ph_lane(z, j), s1, sa, sap, dir, sig, p.clip);
                x[i] = y;
                if (tr) tr[i] = y;
            }
        }
    }
    if (tn >= 0) ddpm_tail(x + p.I, p.temb + (int64_t)min(tn, p.T - 1) * p.E, p.E, p.vec_tail);
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

struct PriorP {
    float* xin; int64_t ldin; const float* te; float* traj; uint64_t seed; uint32_t step; int I, E, vec, vec_tail;
};

__global__ __launch_bounds__(256) void ddpm_prior_kernel(PriorP p) {
    const int64_t b = blockIdx.x;
    float* x = p.xin + b * p.ldin;
    float* tr = p.traj ? p.traj + b * (int64_t)p.I : nullptr;
    for (int q = threadIdx.x; 4 * q < p.I; q += 256) {
        const float4 z = ph_normals(p.seed, (uint32_t)q, p.step, (uint32_t)b, GM_DDPM_TAG_S);
        if (p.vec) {
            reinterpret_cast<float4*>(x)[q] = z;
            if (tr) reinterpret_cast<float4*>(tr)[q] = z;
        } else {
            const int cnt = min(4, p.I - 4 * q);
            for (int j = 0; j < cnt; ++j) {
                x[4 * q + j] = ph_lane(z, j);
                if (tr) tr[4 * q + j] = ph_lane(z, j);
            }
        }
    }
    ddpm_tail(x + p.I, p.te, p.E, p.vec_tail);
}

inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline bool shape_ok(int I, int E, int T) {
    return I >= 1 && I <= GM_DDPM_MAX_I && E >= GM_DDPM_MIN_E && E <= GM_DDPM_MAX_E && E % 4 == 0 && T >= 2 &&
           T <= GM_DDPM_MAX_T;
}

// Host: the device forms of the three argument blocks of a q-sample over B rows of I pixels, or GM_EINVAL.
// *vec: whether the noise / input rows allow 16-byte accesses (the caller ands in its own source rows).
inline int qs_fill(const gm_ddpm_noise* a, const gm_ddpm_tables* s, const gm_ddpm_out* o, int64_t B, int I,
                   DdpmNoiseP* n, DdpmTabP* t, DdpmOutP* out, int* vec) {
    GM_CHECK_ARG(a != nullptr && s != nullptr && o != nullptr);
    GM_CHECK_ARG(s->sa && s->s1 && s->temb && shape_ok(I, s->E, s->T));
    GM_CHECK_ARG(o->xin && o->eps && o->ldin >= (int64_t)I + s->E && o->lde >= I && (const float*)o->xin != o->eps);
    GM_CHECK_ARG(a->row0 >= 0 && B >= 1 && B < (1ll << 31) && a->row0 + B <= (1ll << 32));
    *n = DdpmNoiseP{a->seed, a->tag_t, a->tag_e, PhClock{a->step_ctr, a->step_base, a->step_add}, a->row0};
    *t = DdpmTabP{s->sa, s->s1, s->temb, s->T, s->E};
    const bool rows4 = I % 4 == 0 && o->ldin % 4 == 0 && al16(o->xin);
    *out = DdpmOutP{o->xin, o->ldin, o->eps, o->lde, o->t, (rows4 && al16(s->temb)) ? 1 : 0};
    *vec = (rows4 && o->lde % 4 == 0 && al16(o->eps)) ? 1 : 0;
    return 0;
}

int gather_qsample(void* stream, const gm_ddpm_noise* a, const gm_ddpm_tables* s, const gm_ddpm_out* o, GatherP& g) {
    DdpmNoiseP n{}; DdpmTabP t{}; DdpmOutP out{};
    int vec = 0;
    const int rc = qs_fill(a, s, o, g.B, g.row_elems, &n, &t, &out, &vec);
    if (rc) return rc;
    GM_CHECK_ARG(g.out != o->xin && g.out != o->eps && (const float*)o->xin != g.data && (const float*)o->eps != g.data);
    g.vec = g.vec && vec;
    hipLaunchKernelGGL(ddpm_gather_qsample_kernel, dim3((unsigned)g.B), dim3(256), 0, (hipStream_t)stream, g, n, t, out);
    GM_LAUNCH_RET();
}

}  // namespace

extern "C" int gm_ddpm_qsample(void* stream, const gm_ddpm_noise* a, const gm_ddpm_tables* s, const gm_ddpm_out* o,
                               const float* x, int64_t ldx, int64_t rows, int I) {
    DdpmNoiseP n{}; DdpmTabP t{}; DdpmOutP out{};
    int vec = 0;
    const int rc = qs_fill(a, s, o, rows, I, &n, &t, &out, &vec);
    if (rc) return rc;
    GM_CHECK_ARG(x && ldx >= I && x != (const float*)o->xin && x != (const float*)o->eps);
    QsP p{x, ldx, I, (vec && ldx % 4 == 0 && al16(x)) ? 1 : 0};
    hipLaunchKernelGGL(ddpm_qsample_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p, n, t, out);
    GM_LAUNCH_RET();
}

extern "C" int gm_gather_rows_qsample(void* stream, const gm_ddpm_noise* a, const gm_ddpm_tables* s,
                                      const gm_ddpm_out* o, const float* data, int64_t n_rows, const int64_t* idx,
                                      gm_slot idx_slot, float* out, int64_t ld_out, int B, int row_elems) {
    GatherP g{};
    const int rc = gm_gather_fill(data, n_rows, idx, idx_slot, out, ld_out, B, row_elems, &g);
    if (rc) return rc;
    return gather_qsample(stream, a, s, o, g);
}

extern "C" int gm_gather_rows_bits_qsample(void* stream, const gm_ddpm_noise* a, const gm_ddpm_tables* s,
                                           const gm_ddpm_out* o, const uint32_t* bits, int words_per_row,
                                           int64_t n_rows, const int64_t* idx, gm_slot idx_slot, float* out,
                                           int64_t ld_out, int B, int row_elems) {
    GatherP g{};
    const int rc = gm_gather_fill_bits(bits, words_per_row, n_rows, idx, idx_slot, out, ld_out, B, row_elems, &g);
    if (rc) return rc;
    return gather_qsample(stream, a, s, o, g);
}

extern "C" int gm_ddpm_loss(void* stream, const float* out, int64_t ldo, const float* eps, int64_t lde, float* dA,
                            int64_t lda, float* part, float scale, int B, int I) {
    GM_CHECK_ARG(out && eps && part && B >= 1 && I >= 1 && I <= GM_DDPM_MAX_I && ldo >= I && lde >= I);
    GM_CHECK_ARG(!dA || (lda >= I && (const float*)dA != eps));
    GM_CHECK_ARG(__builtin_isfinite(scale) && scale >= 0.f);
    const int vec = (I % 4 == 0 && ldo % 4 == 0 && lde % 4 == 0 && al16(out) && al16(eps) &&
                     (!dA || (lda % 4 == 0 && al16(dA)))) ? 1 : 0;
    LossP p{out, ldo, eps, lde, dA, lda, part, 2.f * scale, I, vec};
    hipLaunchKernelGGL(ddpm_loss_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_ddpm_reverse(void* stream, const gm_ddpm_reverse_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->xin && a->eps && a->coef && a->temb && shape_ok(a->I, a->E, a->T));
    GM_CHECK_ARG(a->rows >= 1 && a->S >= 1 && a->S <= a->T && a->ldin >= (int64_t)a->I + a->E && a->lde >= a->I);
    GM_CHECK_ARG((const float*)a->xin != a->eps && a->slot.stride == 8);
    GM_CHECK_ARG(!a->traj || (a->traj_stride >= (int64_t)a->rows * a->I && a->traj != a->xin));
    GM_CHECK_ARG(!a->tick || a->done);
    const bool rows4 = a->I % 4 == 0 && a->ldin % 4 == 0 && al16(a->xin);
    RevP p{a->xin, a->ldin, a->eps, a->lde, a->coef, a->slot, a->temb, a->traj, a->traj_stride, a->seed, a->tick, a->done,
           a->I, a->E, a->T, a->S, a->clip ? 1 : 0,
           (rows4 && a->lde % 4 == 0 && al16(a->eps) && (!a->traj || (al16(a->traj) && a->traj_stride % 4 == 0))) ? 1 : 0,
           (rows4 && al16(a->temb)) ? 1 : 0};
    p.slot.stride = 1;                     // the kernel takes the row index and scales it itself
    hipLaunchKernelGGL(ddpm_reverse_kernel, dim3((unsigned)a->rows), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_ddpm_prior(void* stream, float* xin, int64_t ldin, const float* temb, uint64_t seed, int64_t step,
                             int t, float* traj, int rows, int I, int E, int T) {
    GM_CHECK_ARG(xin && temb && shape_ok(I, E, T) && rows >= 1 && ldin >= (int64_t)I + E && t >= 0 && t < T);
    GM_CHECK_ARG(step >= 0 && traj != xin);
    const bool rows4 = I % 4 == 0 && ldin % 4 == 0 && al16(xin);
    PriorP p{xin, ldin, temb + (int64_t)t * E, traj, seed, (uint32_t)step, I, E, (rows4 && (!traj || al16(traj))) ? 1 : 0,
             (rows4 && al16(temb)) ? 1 : 0};
    hipLaunchKernelGGL(ddpm_prior_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
