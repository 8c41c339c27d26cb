// Label-weight gradient (+ Adam) of the class-conditional VAE's conditioned layers (cvae.py; gm_hip.h).
//
// A conditioned layer computes x W^T + b + E[:, y_m] (the split form of linear(cat[x, onehot(y)])), so the label weight's
// gradient is the bias gradient split by class: dE[n, c] = sum over rows m with y_m = c of dPre[m, n].
//
// One workgroup (4 waves) per (layer, 64-column block, class c).  Wave w walks the 64-row chunks w, w + 4, w + 8, ... of
// the batch: each lane reads one row's class, a ballot gives the chunk's rows of class c (a wave-uniform mask), and the
// wave adds those rows of its 64 columns in ascending order, four loads in flight at a time.  The four waves' partial
// sums are added in wave order.  Every (n, c) is owned by one thread, the order is fixed: the same bits on every run, in
// a graph or not, and a class absent from the batch keeps its exact 0.  Each dPre element is loaded by exactly one wave.
// The owning thread then writes the gradient and/or steps Adam on E[n, c] (torch's update, weight decay folded into the
// gradient) with the batch's schedule row -- the label weights need no launch of their own.
#include "gm_common.h"

namespace {

struct LabelGradP {
    gm_label_grad_args L0, L1;     // (separate fields: a dynamically indexed kernel-argument array would go to scratch)
    int items0;                    // workgroups of layer 0; the rest belong to layer 1
    gm_label_src lab;
    int M, C;
    const float* sched; gm_slot sched_slot;
    float omb1, b2, omb2, eps, wd;
};

__global__ __launch_bounds__(256) void label_grad_adam_kernel(LabelGradP p) {
    __shared__ float part[4][64];
    int item = blockIdx.x;
    const bool second = item >= p.items0;                   // workgroup-uniform
    if (second) item -= p.items0;
    const gm_label_grad_args a = second ? p.L1 : p.L0;
    const int nbk = (a.N + 63) >> 6;
    const int c = item / nbk, nb = item - c * nbk;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = nb * 64 + lane, nc = min(n, a.N - 1);
    const float* col = a.dPre + nc;
    float acc = 0.f;
    for (int m0 = 64 * w; m0 < p.M; m0 += 256) {
        const int m = m0 + lane;
        const int y = (m < p.M) ? gm_row_label(p.lab, m, p.C) : -1;
        unsigned long long mask = __ballot(y == c);
        while (mask) {                                       // wave-uniform
            int j[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                j[u] = mask ? __builtin_ctzll(mask) : -1;
                mask &= mask - 1;                            // (mask == 0 stays 0 after the wrap: 0 & ~0)
            }
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = col[(int64_t)(m0 + max(j[u], 0)) * a.ld];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (j[u] >= 0) acc += v[u];
        }
    }
    part[w][lane] = acc;
    __syncthreads();
    if (w != 0 || n >= a.N) return;
    const float g = ((part[0][lane] + part[1][lane]) + part[2][lane]) + part[3][lane];
    const int64_t o = (int64_t)n * p.C + c;                  // E is [N, C] row-major (nn.Linear(C, N).weight)
    if (a.gE) a.gE[o] = g;
    if (a.E) {
        const int64_t si = gm_slot_index(p.sched_slot);
        const float step_size = p.sched[2 * si], bc2_sqrt = p.sched[2 * si + 1];
        float P = a.E[o], Mm = a.mE[o], V = a.vE[o];
        adam_update(P, g, Mm, V, step_size, bc2_sqrt, p.omb1, p.b2, p.omb2, p.eps, p.wd, 0.f);
        a.E[o] = P; a.mE[o] = Mm; a.vE[o] = V;
    }
}

}  // namespace

extern "C" int gm_label_grad_adam(void* stream, const gm_label_grad_args* layers, int n_layers, gm_label_src lab, int M,
                                  int C, const float* sched, gm_slot sched_slot, double beta1, double beta2, double eps,
                                  double weight_decay) {
    GM_CHECK_ARG(layers && (n_layers == 1 || n_layers == 2) && lab.labels && M > 0 && C > 0 && C <= 32);
    bool adam = false;
    for (int i = 0; i < n_layers; ++i) {
        const gm_label_grad_args& a = layers[i];
        GM_CHECK_ARG(a.dPre && a.N > 0 && a.ld >= a.N && (a.gE || a.E));
        GM_CHECK_ARG(!a.E || (a.mE && a.vE));
        adam = adam || a.E;
    }
    GM_CHECK_ARG(!adam || sched);
    LabelGradP p{};
    p.L0 = layers[0];
    p.L1 = n_layers == 2 ? layers[1] : layers[0];
    p.items0 = ((p.L0.N + 63) / 64) * C;
    const int items1 = n_layers == 2 ? ((p.L1.N + 63) / 64) * C : 0;
    p.lab = lab; p.M = M; p.C = C;
    p.sched = sched; p.sched_slot = sched_slot;
    p.omb1 = (float)(1.0 - beta1); p.b2 = (float)beta2; p.omb2 = (float)(1.0 - beta2);
    p.eps = (float)eps; p.wd = (float)weight_decay;
    hipLaunchKernelGGL(label_grad_adam_kernel, dim3(p.items0 + items1), dim3(256), 0, (hipStream_t)stream, p);
    GM_LAUNCH_RET();
}
