// The neural spline flow's arithmetic (nsf.py holds the contract; gm_hip.h), shared by both
// kernels of gm_nsf.hip: the ONE place that forms a pixel's widths, heights and slopes, its knots, its bin, xi, the
// forward value, the inverse value and the log-derivative, so that the forward, the backward and the inverse see the same
// knots and the same bin.  BINS is a compile-time parameter: every loop below unrolls fully, every array is indexed by
// constants and lives in registers, and the bin's six quantities are picked by select chains (no runtime index, so no
// scratch).  Plain C++ but for the function qualifiers: the arithmetic compiles for the host too.
#pragma once
#include <math.h>

#ifdef __HIPCC__
#define NSF_FN static __host__ __device__ __forceinline__
#else
#define NSF_FN static inline
#endif

#define NSF_MIN_BIN 1e-3f                      // m: the least width, height (as a share of 2 B) and slope
#define NSF_SLOPE_SHIFT 0.5397424172369522f    // c = log(exp(1 - m) - 1): theta_d = 0 gives slope 1

// What a pixel's 3 BINS - 1 parameters become: the two softmaxes (kept for the backward), the widths and heights, and
// the knots' slopes d[0] = d[BINS] = 1.
template <int BINS> struct NsfKnots { float pw[BINS], ph[BINS], w[BINS], h[BINS], d[BINS + 1]; };

// The bin of one value: its left knot (xk, yk), its width, height and the slopes at its two ends.
struct NsfBin { float xk, wk, yk, hk, dk, dk1; int k; };

// The rational-quadratic map at one point of a bin.
struct NsfPoint { float xi, s, r, q, A, D; };

// p = softmax(t) in its stable form (left-to-right sum) and the sizes 2 B (m + (1 - m BINS) p).
template <int BINS> NSF_FN void nsf_sizes(const float* t, float B, float* p, float* w) {
#pragma clang fp contract(off)
    const float share = (float)(1.0 - 1e-3 * BINS), two_b = 2.f * B;
    float mx = t[0];
#pragma unroll
    for (int i = 1; i < BINS; ++i) mx = fmaxf(mx, t[i]);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < BINS; ++i) {
        p[i] = expf(t[i] - mx);
        sum += p[i];
    }
#pragma unroll
    for (int i = 0; i < BINS; ++i) {
        p[i] = p[i] / sum;
        w[i] = two_b * (NSF_MIN_BIN + share * p[i]);
    }
}

NSF_FN float nsf_softplus(float a) {
#pragma clang fp contract(off)
    return fmaxf(a, 0.f) + log1pf(expf(-fabsf(a)));
}

NSF_FN float nsf_sigmoid(float a) {
#pragma clang fp contract(off)
    return 1.f / (1.f + expf(-a));
}

// th: the pixel's parameters, theta_w | theta_h | theta_d.
template <int BINS> NSF_FN void nsf_knots(const float* th, float B, NsfKnots<BINS>& K) {
#pragma clang fp contract(off)
    nsf_sizes<BINS>(th, B, K.pw, K.w);
    nsf_sizes<BINS>(th + BINS, B, K.ph, K.h);
    K.d[0] = 1.f;
    K.d[BINS] = 1.f;
#pragma unroll
    for (int i = 1; i < BINS; ++i) K.d[i] = NSF_MIN_BIN + nsf_softplus(th[2 * BINS + i - 1] + NSF_SLOPE_SHIFT);
}

// The bin of v among the x knots (on_y: among the y knots): the number of interior knots at or below v.  The knots
// ascend strictly (every width is at least 2 B m), so the last knot that passes the test is the bin's.
template <int BINS> NSF_FN NsfBin nsf_bin(const NsfKnots<BINS>& K, float B, float v, bool on_y) {
#pragma clang fp contract(off)
    NsfBin b{-B, K.w[0], -B, K.h[0], K.d[0], K.d[1], 0};
    float cw = 0.f, ch = 0.f;
#pragma unroll
    for (int i = 1; i < BINS; ++i) {
        cw += K.w[i - 1];
        ch += K.h[i - 1];
        const float xi = -B + cw, yi = -B + ch;
        const bool at = on_y ? (v >= yi) : (v >= xi);
        b.xk = at ? xi : b.xk;
        b.yk = at ? yi : b.yk;
        b.wk = at ? K.w[i] : b.wk;
        b.hk = at ? K.h[i] : b.hk;
        b.dk = at ? K.d[i] : b.dk;
        b.dk1 = at ? K.d[i + 1] : b.dk1;
        b.k = at ? i : b.k;
    }
    return b;
}

// xi and what the value, the log-derivative and the backward share.
NSF_FN NsfPoint nsf_point(const NsfBin& b, float xi) {
#pragma clang fp contract(off)
    NsfPoint p;
    p.xi = xi;
    p.s = b.hk / b.wk;
    const float om = 1.f - xi;
    p.r = xi * om;
    p.q = p.s + ((b.dk1 + b.dk) - 2.f * p.s) * p.r;
    p.A = p.s * (xi * xi) + b.dk * p.r;
    p.D = (b.dk1 * (xi * xi) + (2.f * p.s) * p.r) + b.dk * (om * om);
    return p;
}

NSF_FN NsfPoint nsf_point_of_x(const NsfBin& b, float x) {
#pragma clang fp contract(off)
    return nsf_point(b, fminf(fmaxf((x - b.xk) / b.wk, 0.f), 1.f));
}

NSF_FN float nsf_value(const NsfBin& b, const NsfPoint& p) {
#pragma clang fp contract(off)
    return b.yk + (b.hk * p.A) / p.q;
}

// log dy/dx = 2 log s + log D - 2 log q.
NSF_FN float nsf_logderiv(const NsfPoint& p) {
#pragma clang fp contract(off)
    return (2.f * logf(p.s) + logf(p.D)) - 2.f * logf(p.q);
}

// x of a y inside the bin b (found on the y knots): the root of the quadratic in its cancellation-free form.
NSF_FN float nsf_inverse(const NsfBin& b, float y) {
#pragma clang fp contract(off)
    const float s = b.hk / b.wk, dl = y - b.yk, t = (b.dk1 + b.dk) - 2.f * s;
    const float qa = b.hk * (s - b.dk) + dl * t, qb = b.hk * b.dk - dl * t, qc = -s * dl;
    const float disc = fmaxf(qb * qb - (4.f * qa) * qc, 0.f);
    const float xi = (2.f * qc) / (-qb - sqrtf(disc));
    return b.xk + xi * b.wk;
}

// One softmax's backward: gs[i] the cotangent of size i, already in t's place on return.  p: the softmax.
template <int BINS> NSF_FN void nsf_sizes_bwd(const float* p, float B, float* gs) {
#pragma clang fp contract(off)
    const float scale = (2.f * B) * (float)(1.0 - 1e-3 * BINS);
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < BINS; ++i) {
        gs[i] = scale * gs[i];
        dot += p[i] * gs[i];
    }
#pragma unroll
    for (int i = 0; i < BINS; ++i) gs[i] = p[i] * (gs[i] - dot);
}

// The pixel's backward, for x inside (-B, B): g the cotangent of y, c the log-derivative's; dth [3 BINS - 1] the
// parameters' gradients (every one written), the return value dx.  Through the map, the knots' running sums, both
// softmaxes and the softplus, whose derivative is formed as a sigmoid.
template <int BINS>
NSF_FN float nsf_backward(const float* th, const NsfKnots<BINS>& K, const NsfBin& b, float B, float x, float g, float c,
                          float* dth) {
#pragma clang fp contract(off)
    const NsfPoint p = nsf_point_of_x(b, x);
    const float xi = p.xi, om = 1.f - xi, r = p.r, q = p.q, s = p.s, q2 = q * q;
    const float xi2 = xi * xi, om2 = om * om, hr = b.hk * r;
    // near the identity d_k, d_{k+1} and s are neighbours: their differences are formed first, where they are exact
    const float u1 = b.dk1 - s, u0 = b.dk - s, t = u1 + u0;
    // y = yk + hk A / q, each partial with its cancelling terms taken out by hand
    const float y_xi = (b.hk * s) * p.D / q2;
    const float y_s = hr * (b.dk1 * xi2 - b.dk * om2) / q2;     // xi^2 q - A (1 - 2 r) = r (d_{k+1} xi^2 - d_k (1 - xi)^2)
    const float y_dk = hr * (s * om2 + b.dk1 * r) / q2;         // q - A = s (1 - xi)^2 + d_{k+1} r
    const float y_dk1 = -(hr * p.A) / q2;
    // ld = 2 log s + log D - 2 log q
    const float D_xi = 2.f * (xi * u1 - om * u0);
    const float ld_xi = D_xi / p.D - (2.f * (t * (1.f - 2.f * xi))) / q;
    const float ld_s = r * (((2.f * t) / (s * q) + 2.f / p.D) + 4.f / q);     // 2 / s - 2 / q = 2 t r / (s q)
    const float ld_dk = om2 / p.D - (2.f * r) / q;
    const float ld_dk1 = xi2 / p.D - (2.f * r) / q;
    const float G_xi = g * y_xi + c * ld_xi, G_s = g * y_s + c * ld_s;
    const float G_dk = g * y_dk + c * ld_dk, G_dk1 = g * y_dk1 + c * ld_dk1;
    // xi = (x - xk) / wk, s = hk / wk
    const float dx = G_xi / b.wk;
    const float G_xk = -dx;
    const float G_wk = -(G_xi * xi + G_s * s) / b.wk;
    const float G_hk = (g * p.A) / q + G_s / b.wk;
    const float G_yk = g;
    // the knots: xk = -B + w_0 + .. + w_{k-1}, yk likewise
#pragma unroll
    for (int i = 0; i < BINS; ++i) {
        dth[i] = i < b.k ? G_xk : (i == b.k ? G_wk : 0.f);
        dth[BINS + i] = i < b.k ? G_yk : (i == b.k ? G_hk : 0.f);
    }
    nsf_sizes_bwd<BINS>(K.pw, B, dth);
    nsf_sizes_bwd<BINS>(K.ph, B, dth + BINS);
    // the two slopes of the bin (an end knot's slope is the constant 1 and has no parameter)
    float a_lo = 0.f, a_hi = 0.f;
#pragma unroll
    for (int i = 1; i < BINS; ++i) {
        a_lo = i == b.k ? th[2 * BINS + i - 1] : a_lo;
        a_hi = i == b.k + 1 ? th[2 * BINS + i - 1] : a_hi;
    }
    const float g_lo = G_dk * nsf_sigmoid(a_lo + NSF_SLOPE_SHIFT), g_hi = G_dk1 * nsf_sigmoid(a_hi + NSF_SLOPE_SHIFT);
#pragma unroll
    for (int i = 1; i < BINS; ++i) dth[2 * BINS + i - 1] = i == b.k ? g_lo : (i == b.k + 1 ? g_hi : 0.f);
    return dx;
}
