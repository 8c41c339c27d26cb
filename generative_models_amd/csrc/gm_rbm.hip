// Binary restricted Boltzmann machine (rbm.py; gm_hip.h; the noise rule and the pinned arithmetic in gm_rbm.h).
//
// gm_rbm_chain: a whole Gibbs chain in one launch.  One wave per chain, four chains per workgroup, no LDS, no barrier.
//   A wave holds v and h as ballot words in scalar registers (NW = ceil(max(I, H) / 64) words each, compile-time
//   indices) and the pre-activations of the layer being formed in NW vector registers, unit 64 j + lane in register j.
//   Both layers are binary, so a pre-activation is the bias plus the weight rows of the lit units: the wave walks the
//   set bits of each ballot word in ascending order and adds the selected row of WT (hidden) or W (visible) with
//   coalesced loads, four or eight rows in flight -- one fp32 accumulator per unit, no multiply, no reassociation.  The walk is
//   ONE loop over all words (the current word picked by wave-uniform selects), so the kernel stays small.
//   With the tempering block the step also adds its annealed-importance-sampling term to the chain's log-weight.
// gm_rbm_grad: from pre [2B, H] of the stacked V = [v0; vk], dA = [-p0; +pk] inv_b and the signed free energies.
// gm_rbm_vbias: the visible bias' gradient inv_b sum_r (vk - v0), rows in order, and its Adam step (gm_adam's arithmetic).
// gm_rbm_transpose: WT = W^T through a 32 x 33 LDS tile, words copied bit for bit.
// gm_rbm_uniform: the rule's uniforms as a matrix, for the general path and the tests.
// No floating-point atomics, fixed reduction orders: the same bits on every run, whatever n and the grid.
#include "gm_rbm.h"

namespace {

struct ChainP {
    const float* W; const float* WT; const float* c; const float* b;
    const float* x; int64_t ldx;
    float* v0; int64_t ldv0; float* v; int64_t ldv; float* p; int64_t ldp; float* a; int64_t lda;
    uint64_t seed; int64_t row0;
    const int64_t* ctr; const int64_t* base; int64_t d_add, g_mul, g_add;
    const float* betas; const float* bA; double* logw;
    int64_t n; int I, H, steps;
};

// Word w of a ballot array by wave-uniform selects: the index into the register array stays a compile-time one.
template <int NW>
__device__ __forceinline__ uint64_t rbm_word(const uint64_t (&bits)[NW], int w) {
    uint64_t r = 0;
#pragma unroll
    for (int j = 0; j < NW; ++j)
        if (j == w) r = bits[j];
    return r;
}

// pre[j] += M[i, 64 j + lane] for every set bit i of `bits` (units below nsel), in ascending i; M's rows are `width`
// floats.  One loop over the set bits of all words, so its body exists once: up to R rows (of one word) are loaded
// before the first is added -- the chain is bound by the latency of these dependent round trips, so R is as large as
// the 64 loads a wave may have in flight allow; an absent row of a word's last group is loaded again from the group's
// first (a valid address) and not added.
template <int NW, int R>
__device__ __forceinline__ void rbm_accum(float (&pre)[NW], const uint64_t (&bits)[NW], const float* __restrict__ M,
                                          int nsel, int width, int lane) {
    const int nw = (nsel + 63) >> 6;
    int w = 0;
    uint64_t m = bits[0];
    for (;;) {
        while (m == 0 && ++w < nw) m = rbm_word<NW>(bits, w);
        if (m == 0) break;
        const int base = w * 64;
        bool has[R];
        const float* row[R];
        const int i0 = base + __builtin_ctzll(m);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            has[r] = m != 0;
            const int i = has[r] ? base + __builtin_ctzll(m) : i0;
            m &= m - 1;
            row[r] = M + (int64_t)i * width + lane;
        }
        float a[R][NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) {
#pragma unroll
            for (int r = 0; r < R; ++r) a[r][j] = 0.f;
            if (j * 64 < width && j * 64 + lane < width) {
#pragma unroll
                for (int r = 0; r < R; ++r) a[r][j] = row[r][j * 64];
            }
        }
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            if (j * 64 >= width) continue;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (has[r]) pre[j] += a[r][j];
        }
    }
}

// The rows in flight: 8 while a row is at most 7 words (56 loads), else 4 (at most 64 with 16 words).
template <int NW>
__device__ __forceinline__ void rbm_accum_any(float (&pre)[NW], const uint64_t (&bits)[NW], const float* __restrict__ M,
                                              int nsel, int width, int lane) {
    if constexpr (NW <= 7) {
        rbm_accum<NW, 8>(pre, bits, M, nsel, width, lane);
    } else if constexpr (NW <= 13) {
        if (width <= 448) rbm_accum<NW, 8>(pre, bits, M, nsel, width, lane);
        else rbm_accum<NW, 4>(pre, bits, M, nsel, width, lane);
    } else {
        rbm_accum<NW, 4>(pre, bits, M, nsel, width, lane);
    }
}

template <int NW>
__global__ __launch_bounds__(256) void rbm_chain_kernel(ChainP q) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= q.n) return;                              // a whole wave: the kernel has no barrier
    const uint32_t row = (uint32_t)(q.row0 + r);
    const int64_t cnt = (q.ctr ? *q.ctr : 0) + (q.base ? *q.base : 0);
    const uint32_t dstep = (uint32_t)(cnt + q.d_add);
    const int64_t g0 = cnt * q.g_mul + q.g_add;
    const int I = q.I, H = q.H;
    uint64_t vb[NW], hb[NW];
    float pre[NW];
    // the binarisation v0 = (u < x)
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int i = w * 64 + lane;
        bool lit = false;
        if (i < I) {
            lit = ph_uniform(q.seed, (uint32_t)i, dstep, row, GM_RBM_TAG_D) < q.x[r * q.ldx + i];
            if (q.v0) q.v0[r * q.ldv0 + i] = lit ? 1.f : 0.f;
        }
        vb[w] = __ballot(lit);
        hb[w] = 0;
    }
    double lw = 0.0;
    for (int s = 0; s < q.steps; ++s) {
        const uint32_t t = (uint32_t)(g0 + s);
        const bool last = s + 1 == q.steps;
        float bc = 1.f, bp = 1.f;
        if (q.betas) { bp = q.betas[s]; bc = q.betas[s + 1]; }
        // pre_h = c + the WT rows of the lit pixels
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int k = j * 64 + lane;
            pre[j] = k < H ? q.c[k] : 0.f;
        }
        rbm_accum_any<NW>(pre, vb, q.WT, I, H, lane);
        if (q.betas) {
            // log w += (bc - bp) (b - b_A).v + sum_j sp(bc pre_h_j) - sp(bp pre_h_j)
            float bv = 0.f, sps = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const int i = w * 64 + lane;
                if (i < I && ((vb[w] >> lane) & 1ull)) bv += q.b[i] - q.bA[i];
            }
#pragma unroll
            for (int j = 0; j < NW; ++j)
                if (j * 64 + lane < H) sps += rbm_sp_diff(bc, bp, pre[j]);
            lw += (double)gm_wave_sum(rbm_logw_lane(bc - bp, bv, sps));
        }
        // h ~ made_prob(beta pre_h)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            const int k = j * 64 + lane;
            bool lit = false;
            if (k < H) {
                const float a = q.betas ? bc * pre[j] : pre[j];
                lit = ph_uniform(q.seed, (uint32_t)k, t, row, GM_RBM_TAG_H) < made_prob(a);
            }
            hb[j] = __ballot(lit);
        }
        // pre_v = b + the W rows of the lit hidden units
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int i = w * 64 + lane;
            pre[w] = i < I ? q.b[i] : 0.f;
        }
        rbm_accum_any<NW>(pre, hb, q.W, H, I, lane);
        // v ~ made_prob(beta pre_v + (1 - beta) b_A)
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int i = w * 64 + lane;
            bool lit = false;
            if (i < I) {
                const float a = q.betas ? rbm_temper_v(bc, pre[w], q.bA[i]) : pre[w];
                const float pv = made_prob(a);
                lit = ph_uniform(q.seed, (uint32_t)i, t, row, GM_RBM_TAG_V) < pv;
                if (last) {
                    if (q.p) q.p[r * q.ldp + i] = pv;
                    if (q.a) q.a[r * q.lda + i] = a;
                }
            }
            vb[w] = __ballot(lit);
        }
    }
    if (q.v) {
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const int i = w * 64 + lane;
            if (i < I) q.v[r * q.ldv + i] = ((vb[w] >> lane) & 1ull) ? 1.f : 0.f;
        }
    }
    if (q.logw && lane == 0) q.logw[r] = lw;
}

template <int NW>
void chain_launch(hipStream_t st, const ChainP& p) {
    hipLaunchKernelGGL(rbm_chain_kernel<NW>, dim3((unsigned)((p.n + 3) / 4)), dim3(256), 0, st, p);
}

struct GradP {
    const float* pre; int64_t ldpre; const float* V; int64_t ldv; const float* b;
    float* dA; int64_t ldd; float* part; float inv_b; int B, I, H;
};

__global__ __launch_bounds__(256) void rbm_grad_kernel(GradP p) {
    __shared__ float sh[4];
    const int64_t r = blockIdx.x;
    const bool pos = r < p.B;                          // a data row: F enters with +, its probabilities with -
    const float* pre = p.pre + r * p.ldpre;
    const float* v = p.V + r * p.ldv;
    float* dA = p.dA + r * p.ldd;
    const float sg = pos ? -p.inv_b : p.inv_b;
    float acc = 0.f;
    for (int j = threadIdx.x; j < p.H; j += 256) {
        const float a = pre[j];
        dA[j] = made_prob(a) * sg;
        acc -= rbm_sp(a);
    }
    for (int i = threadIdx.x; i < p.I; i += 256) acc -= p.b[i] * v[i];
    acc = gm_wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float F = ((sh[0] + sh[1]) + sh[2]) + sh[3];
        p.part[r] = pos ? F : -F;
    }
}

struct VbiasP {
    const float* V; int64_t ldv; float* g; float* pb; float* mb; float* vb;
    const float* sched; gm_slot sched_slot;
    float inv_b, omb1, b2, omb2, eps, wd;
    int B, I;
};

__global__ __launch_bounds__(64) void rbm_vbias_kernel(VbiasP p) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= p.I) return;
    const float* v0 = p.V + i;
    const float* vk = p.V + (int64_t)p.B * p.ldv + i;
    float acc = 0.f;
    for (int r0 = 0; r0 < p.B; r0 += 8) {
        float d[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = min(r0 + u, p.B - 1);
            d[u] = vk[(int64_t)r * p.ldv] - v0[(int64_t)r * p.ldv];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (r0 + u < p.B) acc += d[u];
    }
    const float g = acc * p.inv_b;
    if (p.g) p.g[i] = g;
    if (p.pb) {
        const int64_t si = gm_slot_index(p.sched_slot);
        adam_update(p.pb[i], g, p.mb[i], p.vb[i], p.sched[2 * si], p.sched[2 * si + 1], p.omb1, p.b2, p.omb2, p.eps,
                    p.wd, 0.f);
    }
}

struct TransP { const uint32_t* W; int64_t ldw; uint32_t* WT; int64_t ldt; int rows, cols; };

__global__ __launch_bounds__(256) void rbm_transpose_kernel(TransP p) {
    __shared__ uint32_t tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        if (r < p.rows && c < p.cols) tile[k][tx] = p.W[(int64_t)r * p.ldw + c];
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (r < p.rows && c < p.cols) p.WT[(int64_t)c * p.ldt + r] = tile[tx][k];
    }
}

struct UniP {
    float* u; int64_t ldu; uint64_t seed; PhClock clk; int64_t row0;
    uint32_t tag; int width;
};

__global__ __launch_bounds__(256) void rbm_uniform_kernel(UniP p) {
    const int64_t b = blockIdx.x;
    const uint32_t t = ph_step(p.clk);
    for (int e = threadIdx.x; e < p.width; e += 256)
        p.u[b * p.ldu + e] = ph_uniform(p.seed, (uint32_t)e, t, (uint32_t)(p.row0 + b), p.tag);
}

inline bool dim_ok(int d) { return d >= 1 && d <= GM_RBM_MAX_DIM; }

}  // namespace

extern "C" int gm_rbm_chain(void* stream, const gm_rbm_chain_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->W && a->WT && a->c && a->b && a->x && dim_ok(a->I) && dim_ok(a->H) && a->W != a->WT);
    GM_CHECK_ARG(a->n >= 1 && a->row0 >= 0 && a->row0 + a->n <= (1ll << 32) && a->ldx >= a->I);
    GM_CHECK_ARG(a->steps >= 0 && a->steps <= GM_RBM_MAX_STEPS && a->g_mul >= 0);
    GM_CHECK_ARG(!a->v0_out || a->ldv0 >= a->I);
    GM_CHECK_ARG(!a->v_out || (a->ldv >= a->I && a->v_out != a->v0_out));
    // v0_out and v_out may be x itself (a wave reads its row before it writes it); p_out and a_out may not
    GM_CHECK_ARG(!a->p_out || (a->ldp >= a->I && (const float*)a->p_out != a->x && a->p_out != a->v_out &&
                               a->p_out != a->v0_out));
    GM_CHECK_ARG(!a->a_out || (a->lda >= a->I && (const float*)a->a_out != a->x && a->a_out != a->v_out &&
                               a->a_out != a->v0_out && a->a_out != a->p_out));
    const bool temper = a->betas || a->b_A || a->logw;
    GM_CHECK_ARG(!temper || (a->betas && a->b_A && a->logw && a->steps >= 1));
    ChainP p{a->W, a->WT, a->c, a->b, a->x, a->ldx, a->v0_out, a->ldv0, a->v_out, a->ldv, a->p_out, a->ldp,
             a->a_out, a->lda, a->seed, a->row0, a->step_ctr, a->step_base, a->d_add, a->g_mul, a->g_add,
             a->betas, a->b_A, a->logw, a->n, a->I, a->H, a->steps};
    hipStream_t st = (hipStream_t)stream;
    const int m = a->I > a->H ? a->I : a->H;
    switch ((m + 63) / 64) {
    case 1: chain_launch<1>(st, p); break;
    case 2: chain_launch<2>(st, p); break;
    case 3: chain_launch<3>(st, p); break;
    case 4: chain_launch<4>(st, p); break;
    case 5: chain_launch<5>(st, p); break;
    case 6: chain_launch<6>(st, p); break;
    case 7: chain_launch<7>(st, p); break;
    case 8: chain_launch<8>(st, p); break;
    case 9: chain_launch<9>(st, p); break;
    case 10: chain_launch<10>(st, p); break;
    case 11: chain_launch<11>(st, p); break;
    case 12: chain_launch<12>(st, p); break;
    case 13: chain_launch<13>(st, p); break;
    case 14: chain_launch<14>(st, p); break;
    case 15: chain_launch<15>(st, p); break;
    default: chain_launch<16>(st, p); break;
    }
    GM_LAUNCH_RET();
}

extern "C" int gm_rbm_grad(void* stream, const float* pre, int64_t ldpre, const float* V, int64_t ldv, const float* b,
                           float* dA, int64_t ldd, float* part, float inv_b, int B, int I, int H) {
    GM_CHECK_ARG(pre && V && b && dA && part && B >= 1 && B <= (1 << 24) && dim_ok(I) && dim_ok(H));
    GM_CHECK_ARG(ldpre >= H && ldv >= I && ldd >= H && (const float*)dA != V && (const float*)dA != b);
    GM_CHECK_ARG(__builtin_isfinite(inv_b) && inv_b >= 0.f);
    GradP p{pre, ldpre, V, ldv, b, dA, ldd, part, inv_b, B, I, H};
    hipLaunchKernelGGL(rbm_grad_kernel, dim3((unsigned)(2 * B)), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_rbm_vbias(void* stream, const gm_rbm_vbias_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->V && a->B >= 1 && a->B <= (1 << 24) && dim_ok(a->I) && a->ldv >= a->I && (a->g || a->pb));
    GM_CHECK_ARG(__builtin_isfinite(a->inv_b) && a->inv_b >= 0.f);
    GM_CHECK_ARG(!a->pb || (a->mb && a->vb && a->sched && a->mb != a->vb && a->pb != a->mb && a->pb != a->vb));
    VbiasP p{a->V, a->ldv, a->g, a->pb, a->mb, a->vb, a->sched, a->sched_slot, a->inv_b, (float)(1.0 - a->beta1),
             (float)a->beta2, (float)(1.0 - a->beta2), (float)a->eps, (float)a->weight_decay, a->B, a->I};
    hipLaunchKernelGGL(rbm_vbias_kernel, dim3((unsigned)((a->I + 63) / 64)), dim3(64), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_rbm_transpose(void* stream, const float* W, int64_t ldw, float* WT, int64_t ldt, int rows, int cols) {
    GM_CHECK_ARG(W && WT && (const float*)WT != W && dim_ok(rows) && dim_ok(cols) && ldw >= cols && ldt >= rows);
    TransP p{reinterpret_cast<const uint32_t*>(W), ldw, reinterpret_cast<uint32_t*>(WT), ldt, rows, cols};
    hipLaunchKernelGGL(rbm_transpose_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32)), dim3(256),
                       0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}

extern "C" int gm_rbm_uniform(void* stream, float* u, int64_t ldu, uint64_t seed, uint32_t tag, const int64_t* step_ctr,
                              const int64_t* step_base, int64_t step_add, int64_t row0, int64_t rows, int width) {
    GM_CHECK_ARG(u && dim_ok(width) && ldu >= width && rows >= 1 && rows < (1ll << 31) && row0 >= 0 &&
                 row0 + rows <= (1ll << 32));
    GM_CHECK_ARG(tag == GM_RBM_TAG_D || tag == GM_RBM_TAG_H || tag == GM_RBM_TAG_V);
    UniP p{u, ldu, seed, PhClock{step_ctr, step_base, step_add}, row0, tag, width};
    hipLaunchKernelGGL(rbm_uniform_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
