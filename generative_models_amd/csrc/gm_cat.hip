// Gumbel-Softmax posterior of the categorical VAE (catvae.py holds the contract; gm_hip.h).  N
// categorical variables of C classes per sample row; rows are image-major (sample j of image b is row b k + j); the noise
// block and the counter layout are gm_philox.h's PhNoise, under tags of their own.
//
// Noise: element e = n C + c of a row is word e & 3 of the row's Philox block e >> 2, through ph_unit to u in (0, 1), and
//   g = -log(-log(u)) (finite for every word: 2^-24 <= u <= 1 - 2^-24).  Never stored: the backward regenerates it.
// One thread per (sample row, variable) segment: the C classes are walked in registers, pass 1 the maximum (and the
//   arg max, lowest index first), pass 2 the sum; the Philox block is recomputed whenever the walk enters a new one, so a
//   thread keeps four words, not C values.  cat_soft / cat_y are the ONE place that forms g, a = (l + g) / tau and the
//   softmax: the forward's y and the backward's y have the same bits.
// gm_cat_sample: G lanes per sample row (G a power of two <= 64, so a row's lanes share a wave), lane q the variables q,
//   q + G, ... ascending, the row's sum over its variables by a fixed butterfly: lp does not depend on where the row lands.
// gm_cat_reduce: one thread per (image, variable); nothing crosses lanes.
// No LDS, no atomics, fixed orders: the same bits on every run, graph or eager.
#include "gm_philox.h"

namespace {

// The Gumbel values of one noise row, element by element: the row's Philox block is recomputed when the walk leaves it.
struct CatG {
    uint64_t seed;
    uint32_t q0, step, row, tag, cur;
    uint4 w;
    __device__ __forceinline__ CatG(const PhNoise& n, uint32_t step_, uint32_t row_)
        : seed(n.seed), q0(n.q0), step(step_), row(row_), tag(n.tag), cur(0xFFFFFFFFu), w(make_uint4(0u, 0u, 0u, 0u)) {}
    __device__ __forceinline__ float at(uint32_t e) {
        const uint32_t blk = e >> 2;
        if (blk != cur) {
            w = PH_BLOCK(seed, q0 + blk, step, row, tag);
            cur = blk;
        }
        const uint32_t j = e & 3u;
        return -logf(-logf(ph_unit(PH_WORD(w, j))));
    }
};

struct CatSoft { float amax, S; int arg; };

// Pass 1: m = max_c (l_c + g_c) and its lowest index; pass 2 (when `sum`): S = sum_c exp((l_c + g_c) / tau - m / tau).
__device__ __forceinline__ CatSoft cat_soft(const float* l, CatG& G, uint32_t e0, int C, float tau, bool sum) {
#pragma clang fp contract(off)
    CatSoft s{0.f, 0.f, 0};
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) {
        const float v = l[c] + G.at(e0 + c);
        if (v > m) {
            m = v;
            s.arg = c;
        }
    }
    if (!sum) return s;
    s.amax = m / tau;
    for (int c = 0; c < C; ++c) {
        const float v = l[c] + G.at(e0 + c);
        s.S += expf(v / tau - s.amax);
    }
    return s;
}

// The unnormalised and the normalised relaxed sample of class c (lc = l_c, g = its Gumbel value).
__device__ __forceinline__ float cat_e(float lc, float g, float tau, const CatSoft& s) {
#pragma clang fp contract(off)
    const float v = lc + g;
    return expf(v / tau - s.amax);
}
__device__ __forceinline__ float cat_y(float lc, float g, float tau, const CatSoft& s) { return cat_e(lc, g, tau, s) / s.S; }

// q = softmax(l) through the max-subtracted log-sum-exp: lmax, log sum_c exp(l_c - lmax) and sum_c q_c log q_c.
struct CatQ { float lmax, lS, logS, qlq; };

__device__ __forceinline__ CatQ cat_q(const float* l, int C) {
#pragma clang fp contract(off)
    CatQ q{-INFINITY, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) q.lmax = fmaxf(q.lmax, l[c]);
    float w = 0.f;
    for (int c = 0; c < C; ++c) {
        const float d = l[c] - q.lmax, e = expf(d);
        q.lS += e;
        w += e * d;                                              // e = 0 contributes 0: d is finite
    }
    q.logS = logf(q.lS);
    q.qlq = w / q.lS - q.logS;
    return q;
}

struct CatP {
    const float* l; int64_t ldl;
    const float* tau_tab; gm_slot tau_slot; float tau;
    float* y; int64_t ldy;
    float* lp; float* kl; int32_t* codes;
    const float* dy; int64_t lddy;
    const float* wn;
    float* dl; int64_t lddl;
    int64_t rows; int k, N, C, mode, gshift;
};

__device__ __forceinline__ float cat_tau(const CatP& p) {
    return p.tau_tab ? p.tau_tab[gm_slot_index(p.tau_slot)] : p.tau;
}

__global__ __launch_bounds__(256) void cat_sample_kernel(CatP p, PhNoise n) {
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = gi >> p.gshift, rr = min(r, p.rows - 1);   // rows past the end redo the last one and store nothing
    const int G = 1 << p.gshift, q = (int)(gi & (G - 1));
    const bool on = r < p.rows;
    const int64_t b = rr / p.k;
    const int j = (int)(rr - b * p.k);
    const int C = p.C, mode = p.mode;
    CatG gen(n, ph_step(n.clk), (uint32_t)(b * n.kt + n.j0 + j));
    const float tau = mode == GM_CAT_RELAXED ? cat_tau(p) : 1.f;
    const float logC = logf((float)C);
    float acc = 0.f;
    for (int v = q; v < p.N; v += G) {
        const uint32_t e0 = (uint32_t)v * (uint32_t)C;
        float* yo = p.y + rr * p.ldy + e0;
        if (mode == GM_CAT_NOISE) {
            if (on)
                for (int c = 0; c < C; ++c) yo[c] = gen.at(e0 + c);
            continue;
        }
        const float* l = p.l + b * p.ldl + e0;
        const CatSoft s = cat_soft(l, gen, e0, C, tau, mode == GM_CAT_RELAXED);
        const CatQ qs = cat_q(l, C);
        if (mode == GM_CAT_DISCRETE)
            acc += (l[s.arg] - qs.lmax) - qs.logS;               // log q_n,z_n
        else
            acc += qs.qlq + logC;                                // KL_n
        if (!on) continue;
        if (mode == GM_CAT_RELAXED) {
            for (int c = 0; c < C; ++c) yo[c] = cat_y(l[c], gen.at(e0 + c), tau, s);
        } else {
            for (int c = 0; c < C; ++c) yo[c] = c == s.arg ? 1.f : 0.f;
            if (p.codes) p.codes[rr * p.N + v] = s.arg;
        }
    }
    if (mode == GM_CAT_NOISE) return;
    for (int o = G >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);     // the row's G lanes, inside one wave
    if (on && q == 0) {
        // DISCRETE: log p(z) - log q(z | x); else -KL.  kl (per image) is the same value from each of its k rows.
        if (mode == GM_CAT_DISCRETE) {
            p.lp[r] = -((float)p.N * logC) - acc;
        } else {
            p.lp[r] = -acc;
            if (p.kl && j == 0) p.kl[b] = acc;
        }
    }
}

__global__ __launch_bounds__(256) void cat_reduce_kernel(CatP p, PhNoise n) {
#pragma clang fp contract(off)
    const int64_t gi = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gi >= p.rows * p.N) return;
    const int64_t b = gi / p.N;
    const int v = (int)(gi - b * p.N), C = p.C;
    const uint32_t e0 = (uint32_t)v * (uint32_t)C;
    const float tau = cat_tau(p);
    const float* l = p.l + b * p.ldl + e0;
    const float* dy = p.dy + b * p.lddy + e0;
    float* dl = p.dl + b * p.lddl + e0;
    CatG gen(n, ph_step(n.clk), (uint32_t)(b * n.kt + n.j0));
    const CatSoft s = cat_soft(l, gen, e0, C, tau, true);
    const CatQ qs = cat_q(l, C);
    float ydy = 0.f;                                             // sum_c y_c dy_c
    for (int c = 0; c < C; ++c) ydy += cat_y(l[c], gen.at(e0 + c), tau, s) * dy[c];
    const float wn = p.wn[b];                                    // d loss / d lp = -wn, lp = -KL
    for (int c = 0; c < C; ++c) {
        const float y = cat_y(l[c], gen.at(e0 + c), tau, s);
        const float da = y * (dy[c] - ydy);
        const float d = l[c] - qs.lmax, qc = expf(d) / qs.lS;
        dl[c] = da / tau + wn * (qc * ((d - qs.logS) - qs.qlq));
    }
}

inline int cat_shape_ok(const gm_cat_args* a) {
    GM_CHECK_ARG(a != nullptr);
    GM_CHECK_ARG(a->B >= 1 && a->k >= 1 && a->k <= GM_IWAE_MAX_K && a->N >= 1 && a->C >= GM_CAT_MIN_C &&
                 a->C <= GM_CAT_MAX_C && (int64_t)a->N * a->C <= GM_CAT_MAX_NC);
    return 0;
}

inline int cat_tau_ok(const gm_cat_args* a) {
    GM_CHECK_ARG(a->tau_tab != nullptr || (a->tau > 0.f && a->tau < INFINITY));
    return 0;
}

}  // namespace

extern "C" int gm_cat_sample(void* stream, const gm_iwae_noise* na, const gm_cat_args* a) {
    int rc = cat_shape_ok(a);
    if (rc) return rc;
    const int W = a->N * a->C;
    GM_CHECK_ARG(a->mode >= GM_CAT_RELAXED && a->mode <= GM_CAT_NOISE);
    GM_CHECK_ARG(a->y && a->ldy >= W);
    if (a->mode != GM_CAT_NOISE) {
        GM_CHECK_ARG(a->logits && a->ldl >= W && a->lp);
        GM_CHECK_ARG((const float*)a->y != a->logits && (const float*)a->lp != a->logits && a->lp != a->y);
        GM_CHECK_ARG(!a->kl || (a->kl != a->lp && a->kl != a->y && (const float*)a->kl != a->logits));
    }
    GM_CHECK_ARG(a->mode != GM_CAT_DISCRETE || a->codes != nullptr);
    if (a->mode == GM_CAT_RELAXED && (rc = cat_tau_ok(a))) return rc;
    PhNoise n{};
    if ((rc = ph_noise_fill(na, a->B, a->k, &n))) return rc;
    int gshift = 0;
    while ((1 << gshift) < a->N && gshift < 6) ++gshift;
    CatP p{};
    p.l = a->logits; p.ldl = a->ldl;
    p.tau_tab = a->tau_tab; p.tau_slot = a->tau_slot; p.tau = a->tau;
    p.y = a->y; p.ldy = a->ldy; p.lp = a->lp; p.kl = a->kl;
    p.codes = a->mode == GM_CAT_DISCRETE ? a->codes : nullptr;
    p.rows = (int64_t)a->B * a->k; p.k = a->k; p.N = a->N; p.C = a->C; p.mode = a->mode; p.gshift = gshift;
    const int64_t blocks = ((p.rows << gshift) + 255) / 256;
    GM_CHECK_ARG(blocks < (1ll << 31));
    hipLaunchKernelGGL(cat_sample_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, n);
    GM_LAUNCH_RET();
}

extern "C" int gm_cat_reduce(void* stream, const gm_iwae_noise* na, const gm_cat_args* a) {
    int rc = cat_shape_ok(a);
    if (rc) return rc;
    const int W = a->N * a->C;
    GM_CHECK_ARG(a->k == 1);                                     // the relaxed backward is the k = 1 training batch's
    GM_CHECK_ARG(a->mode == GM_CAT_RELAXED || a->mode == GM_CAT_ST);
    GM_CHECK_ARG(a->logits && a->dzdec && a->wn && a->dlogits && a->ldl >= W && a->lddz >= W && a->lddl >= W);
    GM_CHECK_ARG((const float*)a->dlogits != a->logits && (const float*)a->dlogits != a->dzdec &&
                 (const float*)a->dlogits != a->wn);
    if ((rc = cat_tau_ok(a))) return rc;
    PhNoise n{};
    if ((rc = ph_noise_fill(na, a->B, 1, &n))) return rc;
    CatP p{};
    p.l = a->logits; p.ldl = a->ldl;
    p.tau_tab = a->tau_tab; p.tau_slot = a->tau_slot; p.tau = a->tau;
    p.dy = a->dzdec; p.lddy = a->lddz; p.wn = a->wn; p.dl = a->dlogits; p.lddl = a->lddl;
    p.rows = a->B; p.k = 1; p.N = a->N; p.C = a->C; p.mode = a->mode;
    const int64_t blocks = (p.rows * p.N + 255) / 256;
    hipLaunchKernelGGL(cat_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, n);
    GM_LAUNCH_RET();
}
