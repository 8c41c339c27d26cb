/*
 * gm_hip.h -- C-ABI of libgm_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the hot
 * path of shayneobrien/generative-models (GAN Trainer.train/train_D/train_G, VAE compute_batch).
 *
 * The reference has no FFI of its own: its hot path bottoms out in
 * PyTorch ops.  Each entry point below therefore cites the reference call site whose torch op(s)
 * it replaces.  Conventions (all entry points):
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is
 *     asynchronous on it and allocation-free, so it can be captured into a hipGraph;
 *   - all pointers are raw DEVICE pointers owned by the caller (PyTorch), fp32 unless noted,
 *     matrices row-major with explicit leading dimensions in elements;
 *   - return 0 on success, a negative hipError_t on a launch error, GM_EINVAL on bad arguments;
 *   - nothing here falls back to a CPU path.
 *
 * "slot" arguments (ctr, mul, add, ring, stride): graph-replayable addressing of per-step data.
 * The effective pointer is  base + ((ctr ? *ctr : 0) * mul + add) % ring * stride  (ring <= 0
 * means no modulo).  `ctr` is a device int64 advanced by gm_tick() once per replayed graph, so a
 * captured graph walks through prefetched index / noise rings and the Adam step table without
 * host involvement.
 */
#ifndef GM_HIP_H
#define GM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GM_EINVAL (-10001)

/* activations (Generator/Discriminator.forward: ns_gan.py:43-46,57-60; w_gp_gan.py:59-62;
 * be_gan.py:73-76) */
enum { GM_ACT_ID = 0, GM_ACT_RELU = 1, GM_ACT_SIGMOID = 2 };

/* GAN loss variants */
enum {
    GM_LOSS_NS = 0,      /* ns_gan.py:191-192,214   (also InfoGAN D/G, DRAGAN first-order, RaGAN G) */
    GM_LOSS_MM = 1,      /* mm_gan.py:215-216,235 */
    GM_LOSS_W = 2,       /* w_gan.py:208,227 ; w_gp_gan.py:218 (first-order part),237 */
    GM_LOSS_LS = 3,      /* ls_gan.py:192-193,213 */
    GM_LOSS_RA = 4,      /* ra_gan.py:204-205 (D) ; :227 (G = NS) */
    GM_LOSS_FISHER = 5,  /* fisher_gan.py:214-223 (D) ; :246 (G) */
    GM_LOSS_F_TV = 6, GM_LOSS_F_FKL = 7, GM_LOSS_F_RKL = 8, GM_LOSS_F_PEARSON = 9,
    GM_LOSS_F_HELLINGER = 10, GM_LOSS_F_JS = 11   /* f_gan.py:99-142 */
};

typedef struct gm_slot {
    const int64_t* ctr;   /* device counter or NULL */
    int32_t mul, add, ring;
    int64_t stride;       /* elements */
} gm_slot;

/* ---- library ------------------------------------------------------------------------- */
int gm_version(void);
const char* gm_arch(void);                 /* "gfx950" */
const char* gm_last_error(void);

/* ---- per-graph tick: *ctr += inc (one thread).  Replaces the Python loop counters of
 * Trainer.train (ns_gan.py:117-126). */
int gm_tick(void* stream, int64_t* ctr, int64_t inc);

/* ---- dst[dst_slot + i] = src[src_slot + i], i < n (fp32 words).  The README extension contract at speed
 * (/root/reference/README.md:29-65): a user's train_D / train_G read ordinary tensors -- compute_noise's result
 * (ns_gan.py:218-220) -- and return a 0-dim loss; the graph that replays them copies the iteration's noise out of
 * the prefetched ring and its loss into the per-step history (the .item() of ns_gan.py:142,154) with this. */
int gm_copy_slot_f32(void* stream, const float* src, gm_slot src_slot, float* dst, gm_slot dst_slot, int64_t n);

/* ---- K1: batch gather.  Replaces DataLoader collate in process_batch (ns_gan.py:222-226):
 * out[b,:] = data[idx[b],:].  idx is int64 [B] at slot `idx_slot`. */
int gm_gather_rows(void* stream, const float* data, int64_t n_rows, const int64_t* idx,
                   gm_slot idx_slot, float* out, int64_t ld_out, int B, int row_elems);

/* ---- K2/K3: Y[M,N] = act(X[M,K] * W[N,K]^T + bias[N]).  Replaces nn.Linear + F.relu /
 * torch.sigmoid (ns_gan.py:44-45,58-59).  X may live in a ring (noise: ns_gan.py:218-220). */
int gm_linear_fwd(void* stream, const float* X, int64_t ldx, gm_slot x_slot, const float* W,
                  const float* bias, float* Y, int64_t ldy, int M, int K, int N, int act);

/* ---- K5/K6: dX[M,K] = dA[M,N] * W[N,K], then times act'(below) where `below` is the output
 * of the layer that produced X (epi: GM_ACT_ID none, GM_ACT_RELU mask below>0,
 * GM_ACT_SIGMOID below*(1-below)).  Replaces autograd's AddmmBackward + Relu/SigmoidBackward
 * inside Tensor.backward() (ns_gan.py:138,155). */
int gm_linear_bwd_dx(void* stream, const float* dA, int64_t lda, const float* W, float* dX,
                     int64_t ldx, const float* below, int64_t ld_below, int M, int K, int N,
                     int epi);

/* ---- K5: dW[N,K] (=|+=) dA[M,N]^T * X[M,K];  db[N] (=|+=) sum_m dA[m,:] (db may be NULL).
 * Replaces autograd's weight/bias gradient accumulation (ns_gan.py:138,155). */
int gm_linear_bwd_dw(void* stream, const float* dA, int64_t lda, const float* X, int64_t ldx,
                     gm_slot x_slot, float* dW, float* db, int M, int K, int N, int accumulate);

/* The three launches above with work riding in them (an epilogue term, the optimizer step, a batch gather, the critic
 * head, a second GEMM): gm_linear_fwd_ex / gm_linear_bwd_dx_ex / gm_linear_bwd_dw_ex further down, one descriptor each.
 * The plain entry points are those calls with only the base fields of the descriptor set. */

/* ---- K4: adversarial loss + its gradient w.r.t. the critic's PRE-activation output.
 * sx,sg: [B] post-activation scores D(x), D(G(z)) (sx NULL in generator mode).
 * out_act: activation that produced the scores (sigmoid, or relu for WGAN-GP).
 * hyper: host array of up to 8 floats (LS: a,b,c ; Fisher: rho ; [7]: weight of the penalty rows).
 * inv_b: fp32 1/B used for every mean and its gradient (1/B_global under data parallelism).
 * loss_out[slot]: scalar loss.  dax/dag: [B] gradients (dax NULL in generator mode).
 * aux_io: device state/extra terms (Fisher: lambda, moments; WGAN-GP: penalty rows) or NULL.
 * db_out: optional [1] gradient of the critic's output bias (sum of dax + sum of dag, each half
 *   accumulated in fp64 so that exactly-cancelling gradients stay exactly zero).
 * Replaces the torch elementwise/mean ops in train_D / train_G (appendix A.2 table). */
int gm_gan_loss(void* stream, int variant, int gen_mode, const float* sx, const float* sg, int B,
                int out_act, const float* hyper, int n_hyper, float inv_b, float* loss_out,
                gm_slot loss_slot, float* dax, float* dag, float* aux_io, float* db_out);
/* Data-parallel form of the two critic losses that are not a mean of per-sample terms:
 * RaGAN's mean(D(G(z))) inside the sigmoid (ra_gan.py:204) and Fisher's moments / lambda ascent
 * (fisher_gan.py:214-223,155-156) span the GLOBAL batch.  The loss runs in phases around
 * gm_allreduce_scalars of `pre` (device float[8]): Ra 1 | exchange pre[0] | 2 | exchange pre[1] | 3;
 * Fisher 1 | exchange pre[0..3] | 2.  loss_scale: 1 on the rank that reports a loss every rank
 * computes identically (Fisher), 0 elsewhere -- per-rank loss slots are summed over ranks. */
int gm_gan_loss_phase(void* stream, int variant, int gen_mode, const float* sx, const float* sg, int B,
                      int out_act, const float* hyper, int n_hyper, float inv_b, float* loss_out,
                      gm_slot loss_slot, float* dax, float* dag, float* aux_io, float* db_out,
                      int phase, float* pre, float loss_scale);

/* ---- K7 (+K8): Adam over one flat parameter buffer, exactly torch's _single_tensor_adam
 * (SURVEY.md section 3.5).  sched: device float2 table {step_size = lr/bc1, bc2_sqrt} indexed by
 * slot (the optimizer step number); clamp > 0 applies p = clamp(p, -clamp, clamp) afterwards
 * (w_gan.py:241-243).  betas/eps/weight_decay arrive as the Python doubles torch receives;
 * 1-beta is formed in double and then cast to fp32, like torch's scalar operands.
 * Replaces optim.Adam.step (ns_gan.py:139,156). */
int gm_adam(void* stream, float* p, const float* g, float* m, float* v, int64_t n,
            const float* sched, gm_slot sched_slot, double beta1, double beta2, double eps,
            double weight_decay, float clamp);

/* ---- K9: WGAN-GP interpolation  x_hat = eps*x + (1-eps)*G(z), eps [B] in a ring
 * (w_gp_gan.py:197-201). */
int gm_interp(void* stream, const float* eps, gm_slot eps_slot, const float* x, int64_t ldx,
              const float* g, int64_t ldg, float* out, int64_t ldo, int B, int I);

/* ---- K10 prologue: u[b,n] = [s_b>0]*[h[b,n]>0]*w2[n]: the vector that autograd.grad(D(x_hat),
 * x_hat) (w_gp_gan.py:207-212) pushes through the ReLU critic; grad = u * W1 is then one
 * gm_linear_bwd_dx call. */
int gm_gp_u(void* stream, const float* s, const float* h, int64_t ldh, const float* w2, float* u,
            int64_t ldu, int B, int H);

/* ---- K11: per-row ||g||_2, penalty rows pen[b] = (n_b - k)^2 and
 * gamma = d(lambda*mean((n-k)^2))/dg (0 where n_b == 0)  (w_gp_gan.py:215, dra_gan.py:220). */
int gm_gp_norm(void* stream, const float* g, int64_t ldg, float* gamma, int64_t ldm, float* pen,
               float lambda, float inv_b, float k, int B, int I);

/* ---- K12 tail: gw2[n] += sum_b [s_b>0][h[b,n]>0]*t[b,n]  (second backward into w2; the dW1 term
 * is gm_linear_bwd_dw(u, gamma, accumulate) and t = gamma*W1^T is gm_linear_fwd). */
int gm_gp_dw2(void* stream, const float* s, const float* h, int64_t ldh, const float* t,
              int64_t ldt, float* gw2, int B, int H);
/* same, STORING the sum (out[n] = ...) instead of accumulating */
int gm_gp_dw2_store(void* stream, const float* s, const float* h, int64_t ldh, const float* t,
                    int64_t ldt, float* out, int B, int H);
/* K10 prologue in one launch: the critic's N = 1 output layer on x_hat and the vector the input
 * gradient starts from -- s[b] = relu(h[b,:].w2 + b2), u[b,n] = [s_b>0][h[b,n]>0] w2[n]
 * (w_gp_gan.py:202-212: D(x_hat) and autograd.grad's seed through the ReLU critic). */
int gm_head_gp(void* stream, const float* h, int64_t ldh, const float* w2, const float* b2, float* s,
               float* u, int64_t ldu, int B, int H);

/* ---- BIR-VAE (bir_vae.py:86-97, 180-221).  reparam: z = mu + eps with the
 * host-drawn numpy noise (scale = set_var, :92-94).  mmd: partial[m] = row m's share of
 * sum k(x,x) + sum k(z,z) - 2 sum k(x,z) with the Gaussian kernel exp(-mean_d((a-b)^2)/dim) over the
 * prior sample x = torch.randn(z.shape) (:203), and (dz != NULL) dz = d(lambda*mmd)/dz. */
int gm_bir_reparam(void* stream, const float* mu, int64_t ldmu, const float* eps, gm_slot eps_slot,
                   float* z, int64_t ldz, int B, int Z);
int gm_bir_mmd(void* stream, const float* z, int64_t ldz, const float* prior, gm_slot prior_slot,
               float* partial, float* dz, int64_t lddz, int B, int Z, float lambda);

/* ---- K14: VAE.  ml = [mu | log_var] (B x 2Z, the two encoder heads packed side by side).
 * reparam: z = mu + eps*exp(lv/2) (vae.py:100-106), kl_out[slot] = sum 0.5*(mu^2+exp(lv)-lv-1)
 * (vae.py:210-212).  reparam_bwd: d(recon+kl)/d[mu|lv] from dz.  sqerr: per-row sums of
 * (x-xr)^2 (vae.py:203) + gradient w.r.t. the decoder's pre-sigmoid output. */
int gm_vae_reparam(void* stream, const float* ml, int64_t ldml, const float* eps, gm_slot eps_slot,
                   float* z, int64_t ldz, float* kl_out, gm_slot kl_slot, int B, int Z);
/* Wide form of gm_vae_reparam: many workgroups, the KL term left as ceil(B*Z/256) per-workgroup partial
 * sums in kl_part[0..n_part) for gm_sum_finalize2_tick to add up. */
int gm_vae_reparam_wide(void* stream, const float* ml, int64_t ldml, const float* eps, gm_slot eps_slot,
                        float* z, int64_t ldz, float* kl_part, int n_part, int B, int Z);
/* gm_vae_reparam_wide AND the decoder's first layer H = act(z W^T + b) (W: [N, Z], Z <= 32, Z % 4 == 0) as ONE
 * launch: vae.py:100-106 + the `F.relu(self.linear(z))` of the decoder (:113).  The reparameterisation workgroups
 * store z and the KL partials exactly as gm_vae_reparam_wide does; the GEMM workgroups form z from (mu, log_var, eps)
 * themselves.  Bit-identical to gm_vae_reparam_wide + gm_linear_fwd. */
int gm_vae_reparam_fwd(void* stream, const float* ml, int64_t ldml, const float* eps, gm_slot eps_slot,
                       float* z, int64_t ldz, float* kl_part, int n_part, int B, int Z, const float* W,
                       const float* bias, float* H, int64_t ldh, int N, int act);
/* The two narrow GEMMs in the middle of the VAE's backward pass as ONE launch (round 4): dz = dHdec W_d1
 * (W_d1: [Hd, Z], decoder layer 1), d loss / d [mu | log_var] from dz exactly as gm_dx_args' reparam epilogue
 * forms it (dml: [B, 2Z], written), dHe = (dml W_ml) . [He > 0] (W_ml: [2Z, Hd], the encoder's mu / log_var layer).
 * One workgroup per 16 rows; same summation orders as that launch followed by gm_linear_bwd_dx.
 * Z <= 32, Hd % 4 == 0.  dz itself is not stored. */
int gm_vae_bwd_mid(void* stream, const float* dHdec, int64_t lddh, const float* Wd1, const float* ml,
                   int64_t ldml, const float* eps, gm_slot eps_slot, float* dml, int64_t lddml,
                   const float* Wml, const float* He, int64_t ldhe, float* dHe, int64_t lddhe, int B, int Hd, int Z);
int gm_vae_reparam_bwd(void* stream, const float* ml, int64_t ldml, const float* eps,
                       gm_slot eps_slot, const float* dz, int64_t lddz, float* dml, int64_t ldd,
                       int B, int Z);
int gm_sqerr_sigmoid_bwd(void* stream, const float* x, int64_t ldx, const float* xr, int64_t ldr,
                         float* dA, int64_t lda, float* partial, int B, int I);
/* out[slot] = scale * sum(partial[0..n)) in a fixed order (deterministic loss reductions). */
int gm_sum_finalize(void* stream, const float* partial, int n, float scale, float* out,
                    gm_slot out_slot);
/* The same as the LAST launch of a step: also advances the device step counter `tick` by one (every
 * slot of the step has been resolved by then), saving the separate gm_tick launch. */
int gm_sum_finalize_tick(void* stream, const float* partial, int n, float scale, float* out,
                         gm_slot out_slot, int64_t* tick);
/* Two such sums in one launch (vae.py:203 and :212 of one batch), tick optional (may be NULL). */
int gm_sum_finalize2_tick(void* stream, const float* pa, int na, float scale_a, float* out_a, gm_slot slot_a,
                          const float* pb, int nb, float scale_b, float* out_b, gm_slot slot_b,
                          int64_t* tick);

/* ---- fused critic head (output_dim == 1, separable loss variants): replaces the N=1 GEMV
 * (`self.discriminate`, ns_gan.py:59), the loss lines of train_D / train_G (appendix A.2) and, in
 * the backward, the N=1 dW + K=1 dX launches.  H: hidden activations [R,Hd] (critic mode R=2B,
 * rows 0..B-1 real then B generated; generator mode R=B).  head_fwd_loss writes scores S[R],
 * dS[R] = d loss / d pre-activation, per-row loss terms and -- when dH is given -- dH = dS (x) w2
 * masked by H>0 while the row is hot; head_bwd writes gw2 = dS^T H, gb2 (fp64 half-sums), the loss
 * scalar, and dH when head_fwd_loss did not (its dH may be NULL; all-NULL outputs = scalars only). */
int gm_head_fwd_loss(void* stream, int variant, int gen_mode, const float* H, int64_t ldh,
                     const float* w2, const float* b2, int out_act, int B, int Hd,
                     const float* hyper, int n_hyper, float inv_b, const float* pen, float* S,
                     float* dS, float* rowloss, float* dH_or_null, int64_t lddh);
/* Same, and the LAST workgroup to finish also writes loss_out[slot] = inv_b * sum(rowloss) (fixed
 * order, fp64) and, when tick != NULL, advances the iteration counter: the generator step needs no
 * head_bwd launch.  done_ctr: one zero-initialised device word, re-armed by the kernel. */
int gm_head_fwd_loss_final(void* stream, int variant, int gen_mode, const float* H, int64_t ldh,
                           const float* w2, const float* b2, int out_act, int B, int Hd,
                           const float* hyper, int n_hyper, float inv_b, const float* pen, float* S,
                           float* dS, float* rowloss, float* dH_or_null, int64_t lddh,
                           float* loss_out, gm_slot loss_slot, unsigned int* done_ctr,
                           int64_t* tick_or_null);
int gm_head_bwd(void* stream, const float* H, int64_t ldh, const float* dS, const float* w2,
                const float* rowloss, float* dH, int64_t lddh, float* gw2, float* gb2,
                float* loss_out, gm_slot loss_slot, float inv_b, int gen_mode, int B, int Hd);

/* gm_head_bwd + optional Adam on (w2, b2) + optional per-graph tick (*tick += 1 once the loss
 * slot is written; later kernels of the same iteration then address slots with add - mul). */
int gm_head_bwd_fused(void* stream, const float* H, int64_t ldh, const float* dS, float* w2,
                      float* b2, const float* rowloss, float* dH, int64_t lddh, float* gw2,
                      float* gb2, float* loss_out, gm_slot loss_slot, float inv_b, int gen_mode,
                      int B, int Hd, int with_adam, float* mW, float* vW, float* mb, float* vb,
                      const float* sched, gm_slot sched_slot, double beta1, double beta2, double eps,
                      double weight_decay, float clamp, int64_t* tick);

/* ---- K16: BEGAN (be_gan.py:189-195, 212-258).  l1_rows: per-row L1 reconstruction error and its
 * gradient (coefficient 1/B for the first B rows, -K/B for the rest when K_dev is given);
 * began_dloss: DX, DG, D_loss = DX - K*DG from the row sums; began_update: convergence measure,
 * proportional control of K, the two ReduceLROnPlateau steps and the graph tick -- all on device
 * state (layout documented in csrc/gm_fused.hip), so the algorithm's per-step .item() syncs vanish. */
int gm_l1_rows(void* stream, const float* Y, int64_t ldy, const float* X, int64_t ldx, int R, int I,
               int B, const float* K_dev, float* dY, int64_t lddy, float* rowsum);
int gm_began_dloss(void* stream, const float* rows, int B, float* state, float* loss_out,
                   gm_slot loss_slot);
/* data parallel: B rows of this rank out of B_global (the means' denominator); DX / DG in the state
 * are then PARTIAL means: gm_allreduce_scalars(state + 1, 2) makes them global before began_update */
int gm_l1_rows_dp(void* stream, const float* Y, int64_t ldy, const float* X, int64_t ldx, int R, int I,
                  int B, int B_global, const float* K_dev, float* dY, int64_t lddy, float* rowsum);
int gm_began_dloss_dp(void* stream, const float* rows, int B, int B_global, float* state,
                      float* loss_out, gm_slot loss_slot);
int gm_began_update(void* stream, float* state, double* dstate, int64_t* istate, float gamma,
                    float lambda, int64_t patience, int64_t* tick);
/* gm_adam with a device-resident learning-rate scale (a power of two: exact). */
int gm_adam_scaled(void* stream, float* p, const float* g, float* m, float* v, int64_t n,
                   const float* sched, gm_slot sched_slot, double beta1, double beta2, double eps,
                   double weight_decay, float clamp, const float* lr_scale);
/* The critic head's backward and the first layer's weight gradient are independent once
 * gm_head_fwd_loss has written dH: gm_dw_adam_args.head runs the weight gradient (+ Adam) AND gm_head_bwd_fused
 * as ONE launch (the head workgroups ride in the GEMM's grid; 25 + 169 workgroups for the 784-400-1
 * critic at B = 256 -- one round of the 256 CUs); gm_dx_args.head carries them in an input-gradient launch.
 * This block mirrors gm_head_bwd_fused's arguments.  with_adam == 0: plain gradients, no optimizer step
 * (data-parallel runs all-reduce the gradients first). */
typedef struct gm_head_bwd_args {
    const float* H; int64_t ldh;
    const float* dS; float* w2; float* b2; const float* rowloss;
    float* dH; int64_t lddh;              /* NULL when gm_head_fwd_loss wrote it */
    float* gw2; float* gb2;
    float* loss_out; gm_slot loss_slot;
    float inv_b; int gen_mode, B, Hd;
    int with_adam; float* mW; float* vW; float* mb; float* vb;
    const float* sched; gm_slot sched_slot;
    double beta1, beta2, eps, weight_decay; float clamp;
    int64_t* tick;
    const float* gw2_add;                 /* optional [Hd]: added to gw2 before it is stored / stepped */
    /* optional (pen_t != NULL): gw2[c] += sum_{r < pen_rows} [pen_s[r] > 0][pen_h[r][c] > 0] pen_t[r][c] -- the
     * gradient penalty's second-backward share of w2's gradient (w_gp_gan.py:215) summed by the
     * head's own workgroups instead of a launch of gm_gp_dw2_store */
    const float* pen_s; const float* pen_h; int64_t pen_ldh; const float* pen_t; int64_t pen_ldt; int pen_rows;
    const float* gb2_add;                 /* optional [1]: added to gb2 before it is stored / stepped (DRAGAN's sigma''
                                           * path reaches the head bias, dra_gan.py:207-223; gm_dragan_head_bwd_store) */
} gm_head_bwd_args;
/* ---- FOLDED critic head (round 3): no launch for the N = 1 layer at all.
 * Discriminator.forward's second layer (ns_gan.py:59: `discrimination = sigmoid(self.discriminate(
 * activated))`, a [R, 400] x [400] product) is split over the launches on either side of it:
 *  - the head part of gm_fwd_args = gm_linear_fwd of the hidden layer whose epilogue also leaves, per
 *    32-column tile j of the hidden layer, part[r * ldp + j] = sum_{n in tile j} Y[r, n] * w2[n]
 *    (nparts = ceil(N / 32) <= 16 entries per row, rows ldp floats apart, ldp % 4 == 0, the unused
 *    entries of a row stay zero) and a snapshot snap[0..N) = w2, snap[N] = b2[0] of the head
 *    parameters it used (the consumers below may run in a launch that also steps w2 / b2);
 *  - the consumers rebuild, per row, score = act(sum_j part[r][j] + b2), the row's loss term and
 *    dS (the train_D / train_G loss lines: ns_gan.py:191-192,214 and the siblings gm_head_fwd_loss
 *    lists) in a prologue, and form dH[r, n] = dS_r * w2[n] * [Y[r, n] > 0] in registers while loading
 *    their A operand: gm_dw_adam_args.head + fold (critic step: layer-1 weight gradient + Adam,
 *    head backward workgroups riding: gw2, gb2, loss, Adam on (w2, b2)) and gm_dx_args.head + fold
 *    (generator step: dX through layer 1 + the loss / tick workgroup).  Both take the hidden
 *    activations H as dA where the unfolded form takes dH; head->dS / head->rowloss are not read.
 * Summation order of a score: 32-lane butterfly inside a tile, then tiles j = 0, 1, ... : fixed, so
 * results are bitwise reproducible run to run (they differ from gm_head_fwd_loss's order in the last
 * bits).  fold->S / dS / rowloss (optional, [R]) receive the per-row values for inspection. */
typedef struct gm_head_fold_args {
    const float* part; int64_t ldp; int nparts;
    const float* snap;
    int variant, out_act;
    float hyper[8]; int n_hyper;
    const float* pen;                     /* optional penalty rows added to the x rows' loss terms */
    float* S; float* dS; float* rowloss;  /* optional outputs */
} gm_head_fold_args;
/* gm_gather_rows with the BIT-PACKED resident dataset (utils.py:31 binarises MNIST): row r
 * = bits[r*words_per_row ...], pixel i = bit (i & 31) of word i >> 5; the gather expands to fp32 rows. */
int gm_gather_rows_bits(void* stream, const uint32_t* bits, int words_per_row, int64_t n_rows,
                        const int64_t* idx, gm_slot idx_slot, float* out, int64_t ld_out, int B,
                        int row_elems);
/* Bit-packed rows AS A GEMM OPERAND (the data is process_batch's, ns_gan.py:222-226, binarised by
 * utils.py:31): the gather copies the selected rows as WORDS (out_bits[b * words_per_row ..), 100 B per MNIST row
 * instead of 3136), and the folded critic step's two launches (the xbits fields of gm_fwd_args and gm_dw_adam_args)
 * read rows [0, rows) of X from that copy, expanding to 0.0f / 1.0f in registers -- the fp32 rows X[0 .. rows) are
 * neither written nor read.  Same MFMA sequence on the same values: results are bit-identical to the fp32-operand
 * launches.  rows % 32 == 0, K % 4 == 0 (a forward tile / reduction chunk is packed as a whole); one tile shape per
 * launch (32x32 forward, 32x48 weight gradient, operands through registers); anything else returns GM_EINVAL -- there
 * is no fp32 copy to fall back to. */
int gm_gather_rows_bits_packed(void* stream, const uint32_t* bits, int words_per_row, int64_t n_rows,
                               const int64_t* idx, gm_slot idx_slot, uint32_t* out_bits, int B);

/* ---- K13: DRAGAN penalty (dra_gan.py:198-223; derivation in SURVEY.md A.3).  std_all: unbiased std
 * of the whole real batch; xhat: delta*x + (1-delta)*(x + C*std*U); rows: per-row norm of the input
 * gradient s'*v (v = (m1.w2) W1 from gm_gp_u + gm_linear_bwd_dx), penalty rows, dv and da2 of the
 * second backward; head_bwd: the w2/b2 accumulations and da1.  Penalty rows are added to the loss by
 * gm_head_fwd_loss / gm_gan_loss with weight hyper[7]. */
/* ws: GM_STD_WS_BYTES of device memory (8-byte aligned), zeroed ONCE by the caller and then owned by these
 * calls (partial sums of the launch's 64 workgroups + their arrival counter; launches sharing a ws must be
 * stream-ordered). */
#define GM_STD_WS_BYTES 1088
int gm_std_all(void* stream, const float* X, int64_t ldx, int R, int I, float* out, void* ws);
/* data parallel: (sum x, sum x^2) of this rank's rows -> scalar all-reduce -> std of the global batch */
int gm_std_sums(void* stream, const float* X, int64_t ldx, int R, int I, float* out2, void* ws);
int gm_std_from_sums(void* stream, const float* sums2, int64_t n_total, float* out);
int gm_dragan_xhat(void* stream, const float* x, int64_t ldx, const float* delta, gm_slot delta_slot,
                   const float* U, gm_slot u_slot, const float* std_dev, float C, float* out,
                   int64_t ldo, int B, int I);
int gm_dragan_rows(void* stream, const float* s, const float* V, int64_t ldv, float* dv, int64_t lddv,
                   float* da2, float* pen, float lambda, float inv_b, float K_norm, int B, int I);
int gm_dragan_head_bwd(void* stream, const float* H, int64_t ldh, const float* T, int64_t ldt,
                       const float* da2, const float* w2, float* gw2, float* gb2, float* dA1,
                       int64_t ldd, int B, int Hd);
/* Fisher GAN (fisher_gan.py:155-156) on the folded critic head: gm_linear_bwd_dw_ex (head + fold) with variant
 * GM_LOSS_FISHER reads lambda = aux[0] in every workgroup and leaves lambda + rho * d loss / d lambda in aux[5]
 * (and the four moments in aux[1..4]); this launch makes it lambda.  aux: 8 floats. */
int gm_fisher_commit(void* stream, float* aux);
/* The same with gw2 / gb2 STORED instead of accumulated: the penalty's share of the head's gradient on its own, for
 * gm_head_bwd_args.gw2_add / gb2_add of the stacked critic step (the head's backward adds them before Adam). */
int gm_dragan_head_bwd_store(void* stream, const float* H, int64_t ldh, const float* T, int64_t ldt,
                             const float* da2, const float* w2, float* gw2, float* gb2, float* dA1,
                             int64_t ldd, int B, int Hd);

/* ---- K15: InfoGAN mutual-information loss (train_Q, info_gan.py:269-304): cross-entropy of the
 * categorical code + mean-squared error of the continuous code, and d loss / d q.  noise rows are
 * [z | one-hot c1 | c2] as built by compute_noise (info_gan.py:306-325). */
int gm_info_q_loss(void* stream, const float* q, int64_t ldq, const float* noise, gm_slot noise_slot,
                   int64_t ldn, int B, int z_dim, int disc_dim, int cont_dim, float lambda, float* dq,
                   int64_t lddq, float* loss_out, gm_slot loss_slot);
/* data parallel: this rank's B rows of a global batch of B_global (both means' denominator) */
int gm_info_q_loss_dp(void* stream, const float* q, int64_t ldq, const float* noise, gm_slot noise_slot,
                      int64_t ldn, int B, int B_global, int z_dim, int disc_dim, int cont_dim, float lambda,
                      float* dq, int64_t lddq, float* loss_out, gm_slot loss_slot);

/* ---- elementwise activation backward for the general autograd path:
 * dA = dY * act'(Y)  (Relu/SigmoidBackward, ns_gan.py:44-45). */
int gm_act_bwd(void* stream, const float* dY, const float* Y, float* dA, int64_t n, int act);

/* ---- stage-in of the per-iteration inputs the reference moves host->device every step
 * (`to_cuda` of the image batch indices and of the CPU-generated noise: ns_gan.py:220,225,
 * utils.py:10-14).  The host writes them into PINNED rings that mirror the device rings; this kernel
 * (first node of every captured graph) copies the slots [i, i+n_iters) of every segment, i resolved
 * from `slot` (stride ignored), host ring -> device ring.  src: device-visible address of pinned
 * host memory (gm_host_device_ptr). */
#define GM_STAGE_MAX_SEGS 8
typedef struct gm_stage_seg {
    const void* src;
    void* dst;
    int64_t bytes_per_iter;     /* bytes copied per iteration (all of its blocks) */
    /* An iteration's slot may consist of `blocks` equal pieces that are not adjacent in the source or
     * the destination: a data-parallel rank stages only ITS rows of every [B, w] draw of the global
     * batch (host ring: global batch; device ring: the rank's rows).  Piece q of iteration i is
     * bytes_per_iter / blocks bytes at src + (i * blocks + q) * src_block_stride, written to
     * dst + (i * blocks + q) * dst_block_stride.  blocks <= 1 and strides 0: one dense piece per
     * iteration (stride = bytes_per_iter), the single-rank layout. */
    int32_t blocks;
    int32_t reserved;
    int64_t src_block_stride, dst_block_stride;
} gm_stage_seg;
int gm_stage_in(void* stream, const gm_stage_seg* segs, int n_segs, gm_slot slot, int n_iters);
/* The same with a FILL GATE: the launch may be enqueued before the host has finished writing the
 * iterations' slots (ns_gan.py:218-226 draws them on the host one step at a time; here the host
 * writes a sub-chunk and then advances gate[0] = number of iterations written since configure).
 * ONE wave -- its own one-wave launch in front of the copy, same stream -- waits (system-scope loads of pinned
 * host memory) until gate[0] >= it + n_iters, it = index of `it_slot` (the absolute iteration); after
 * timeout_s seconds it raises gate[1] = 1 and the copy proceeds -- the host must check gate[1] before
 * trusting results.  (Polled from every workgroup of the copy the gate cost a serialized PCIe read per
 * workgroup, ~1 us per iteration staged: round 5.)
 * gate: device-visible address (gm_host_device_ptr) of two int64 in pinned host memory.
 * publish (optional, device memory): workgroup (0,0) stores `it` there -- a second stage-in that runs
 * on a forked branch of the graph, concurrently with iterations that advance the step counter, resolves
 * its slots from that word instead.  max_blocks (1..256): workgroups per segment (a concurrent
 * stage-in should leave the CUs to the iteration kernels). */
int gm_stage_in_gated(void* stream, const gm_stage_seg* segs, int n_segs, gm_slot slot, int n_iters,
                      const int64_t* gate, gm_slot it_slot, double timeout_s, int64_t* publish,
                      int max_blocks);
/* Device-side address of a pinned host allocation (hipHostGetDevicePointer). */
int gm_host_device_ptr(void* host_ptr, void** dev_ptr_out);

/* ---- C1 (NEW: the reference has no distributed code): gradient exchange of
 * the data-parallel step between the ranks of one node, as kernels that live inside the iteration's
 * hipGraph (csrc/gm_comm.hip).  Every rank creates a communicator (an exchange region in fine-grained
 * device memory), the 64-byte IPC handles are exchanged by the host (torch.distributed
 * all_gather_object), gm_comm_connect maps the peers.  gm_allreduce_f32: in-place SUM over ranks of
 * buf[0..n) (n % 4 == 0, 16-byte aligned), identical bits on every rank; gm_allreduce_adam_f32: same,
 * with optim.Adam.step (ns_gan.py:139,156) applied to (p, m, v) by the kernel that writes the reduced
 * gradient; gm_allreduce_scalars: up to 16 floats (the pre-reductions of the losses that are not a
 * mean of per-sample terms: ra_gan.py:204, fisher_gan.py:214-223, dra_gan.py:204, be_gan.py:189-195).
 * Waits are bounded; gm_comm_error reports an expired one. */
int gm_comm_create(int rank, int world, int64_t n_floats, void** comm_out, void* handle_out64);
int gm_comm_connect(void* comm, const void* all_handles /* world x 64 bytes, rank order */);
int gm_comm_destroy(void* comm);
int gm_comm_error(void* comm, int* flag_out);
/* *fine_grained_out = 1 when the exchange region is fine-grained device memory (peers on OTHER GPUs
 * may store into it while a kernel polls it), 0 when the runtime refused that allocation and the
 * region is plain device memory: valid only when every rank shares one device. */
int gm_comm_info(void* comm, int* fine_grained_out);
/* Exchange form.  0 (default): an all-reduce is ONE kernel (reduce-scatter, arrival counter, all-gather + Adam) that
 * READS the peers' buckets over the peer mappings; 1: the same as two launches (reduce, gather) -- ranks that share
 * one device must use 1 unless they also lower gm_comm_set_max_blocks: the one-kernel forms keep every rank's
 * workgroups spinning on peer flags, which starves the peers' GEMM workgroups when they run on the same CUs
 * (dp.PeerComm sets it from the ranks' device identities); 2: ONE kernel that moves the data by posted remote
 * WRITES only (every rank deposits its contributions in the slice owners' staging areas, owners write the reduced
 * slices into every rank's `out`): no xGMI read round trips.  All three give bit-identical sums (rank order). */
int gm_comm_set_exchange(void* comm, int form);
/* Upper bound on the workgroups of one exchange launch.  The one-kernel form needs ALL its workgroups co-resident
 * (each spins until every peer's last workgroup has arrived): the default (max_blocks = 0) is what the occupancy API
 * reports for this device or partition (CPX mode, HSA_CU_MASK), at most 320; ranks that share one device pass less. */
int gm_comm_set_max_blocks(void* comm, int max_blocks);
/* Bound (seconds of the 100 MHz wall clock, default 10) of every device-side wait of this communicator's later
 * launches; an expired wait raises gm_comm_error's flag instead of hanging the GPU.  The start-up self-check between
 * ranks on different devices runs with 2 s. */
int gm_comm_set_wait_seconds(void* comm, double seconds);
/* The region's own bucket (n_floats fp32, 256-byte aligned): a gradient buffer placed here is
 * all-reduced without a staging copy. */
int gm_comm_buffer(void* comm, void** ptr_out, int64_t* n_floats_out);
int gm_allreduce_f32(void* comm, void* stream, float* buf, int64_t n);
int gm_allreduce_adam_f32(void* comm, void* stream, float* grad, int64_t n, float* p, float* m,
                          float* v, const float* sched, gm_slot sched_slot, double beta1,
                          double beta2, double eps, double weight_decay, float clamp,
                          const float* lr_scale_or_null);
int gm_allreduce_scalars(void* comm, void* stream, float* vals, int k);
/* The same SUM as an RCCL collective that can be CAPTURED into the iteration's hipGraph (the fallback when peer
 * mappings are not available: GM_DP_COMM=rccl; round 1 launched torch.distributed all-reduces from the host between
 * segment graphs).  RCCL is not linked: its symbols are resolved at first use from the librccl the process already
 * carries (torch's).  uid128: 128 bytes (ncclUniqueId) made on rank 0 by gm_rccl_unique_id and handed to every rank
 * by the host; gm_rccl_comm_create is collective.  In place, fp32. */
int gm_rccl_available(void);          /* 1: ncclGetUniqueId / CommInitRank / AllReduce / CommDestroy all resolve here */
int gm_rccl_unique_id(void* uid128_out);
int gm_rccl_comm_create(int rank, int world, const void* uid128, void** rccl_comm_out);
int gm_rccl_allreduce_f32(void* rccl_comm, void* stream, float* buf, int64_t n);
int gm_rccl_comm_destroy(void* rccl_comm);

/* ---- HOST helper (no device work): first B entries of torch.randperm(n, generator=
 * Generator().manual_seed(seed)) in O(B): RandomSampler.__iter__ (torch/utils/data/sampler.py:160-185)
 * feeding process_batch (ns_gan.py:222-226).  mt19937 seeded with the low 32 bits of `seed`,
 * forward Fisher-Yates `z = random() % (n-i); swap(r[i], r[i+z])` as in ATen randperm_cpu.
 * Bit-exact sampling indices without materialising the 50 000-entry permutation. */
int gm_randperm_prefix(uint64_t seed, int64_t n, int B, int64_t* out_host);
/* HOST: advance a serialized torch CPU generator state (torch.get_rng_state(), 5056 bytes,
 * mt19937) by n 32-bit outputs without producing them.  Data-parallel ranks replay the reference's
 * global draw protocol (ns_gan.py:183,208,220) but materialise only their own rows of each noise
 * tensor; the draws belonging to other ranks' rows are skipped with this call. */
int gm_mt19937_skip(void* torch_cpu_rng_state, int64_t state_bytes, uint64_t n);

/* ---- HOST: replay of the reference's global-CPU-generator protocol for a run of iterations in
 * ONE call (csrc/gm_hostrng.cpp).  A program is the ordered list of draws of one iteration:
 *   GM_DRAW_SAMPLER  process_batch (ns_gan.py:222-226): DataLoader base seed + RandomSampler seed
 *                    (two int64 random_() draws), first n entries of randperm(a) -> int64 dst[n]
 *   GM_DRAW_NORMAL   torch.randn(n) on contiguous fp32, n >= 16 (ns_gan.py:220, vae.py:104)
 *   GM_DRAW_UNIFORM  torch.rand(n) fp32 (w_gp_gan.py:197, dra_gan.py:200,205)
 *   GM_DRAW_INFO     info_gan.py:312-323: [randn(n,a) | one_hot(randint(0,b,(n,))) | randn(n,c)]
 * executed n_iters times; iteration i writes to dst + i*iter_stride (host memory, e.g. pinned
 * staging).  [e0,e1) limits what is materialised (a data-parallel rank's rows) while the stream
 * advances as for the whole tensor.  Returns -10002 for shapes outside the restated ATen paths
 * (the caller then draws through torch).  The serialized state (torch.get_rng_state()) is
 * advanced in place. */
typedef struct gm_draw_op {
    int32_t kind;
    int32_t n;
    int64_t a;
    int32_t b, c;
    void* dst;
    int64_t iter_stride;
    int64_t e0, e1;
} gm_draw_op;
enum { GM_DRAW_SAMPLER = 0, GM_DRAW_NORMAL = 1, GM_DRAW_UNIFORM = 2, GM_DRAW_INFO = 3 };
int gm_host_replay(void* torch_cpu_rng_state, int64_t state_bytes, const gm_draw_op* ops, int n_ops,
                   int n_iters);
/* HOST: which restatement of ATen's float normal_fill the replay uses: 0 = scalar libm
 * (normal_fill_16<float>), 1 = avx_mathfun.h polynomials with the mul+add pairs contracted to FMAs,
 * 2 = same without contraction.  Python picks the one that reproduces torch bit for bit. */
int gm_host_replay_flavour(int flavour);
/* HOST: the same replay as a job for the library's fill worker (one persistent native thread, jobs run
 * in submission order on the caller-owned generator state buffer, which must stay valid until the job
 * is retired).  After the job's writes the worker stores *gate = gate_value (release) -- the fill gate
 * of gm_stage_in_gated -- when gate is non-null.  Returns the job id (> 0) or a negative error.
 * gm_fill_wait(id): block until job id is retired, returns the worker's sticky error (0 = none; after
 * an error later jobs are retired without running and without opening their gates).
 * gm_fill_completed(): id of the last retired job.  gm_fill_reset(): wait for everything submitted and
 * clear the sticky error.  Replaces one Python thread hop + two generator-state copies per sub-chunk
 * of ns_gan.py:183,208,222-226-style draws. */
int64_t gm_fill_submit(void* torch_cpu_rng_state, int64_t state_bytes, const gm_draw_op* ops, int n_ops,
                       int n_iters, int64_t* gate, int64_t gate_value);
int gm_fill_wait(int64_t id);
int64_t gm_fill_completed(void);
int gm_fill_reset(void);
/* HOST: size of the worker pool of gm_host_replay's Box-Muller stage (1 = caller only). */
int gm_host_replay_threads(int n_threads);
/* numpy's LEGACY global generator (np.random.normal of bir_vae.py:92-94): n values loc + scale * legacy_gauss as
 * float32, bit-identical to torch.from_numpy(np.random.normal(loc, scale, n)).float(); key[624] / pos / has_gauss /
 * gauss are np.random.get_state(legacy=True)'s fields, advanced in place.  The log / sqrt stage of the polar
 * method runs on n_threads. */
int gm_numpy_legacy_normal_f32(uint32_t* key, int32_t* pos, int32_t* has_gauss, double* gauss, double loc,
                               double scale, int64_t n, float* out, int n_threads);

/* ---- Gaussian Parzen-window log-likelihood (csrc/gm_eval.hip): the MNIST evaluation of the GAN paper that
 * ns_gan.py:1-5 / mm_gan.py:1-5 link (arXiv 1406.2661, table 1).  The reference has no evaluation of its own: its
 * runs end in loss curves and sample grids (ns_gan.py:228-281).  For query rows x (q [nq, d], ld ldq), sample rows
 * s_i (s [ns, d], ld lds) and each of the n_sigma bandwidths in `sigmas` (device fp32, each > 0):
 *     out[k, j] = logsumexp_i(-|x_j - s_i|^2 / (2 sigma_k^2)) - log ns - d log(sigma_k sqrt(2 pi))
 * fp32 in and out (out [n_sigma, nq], ld ldo), fp64 row norms and chunk combination.  The sample axis is cut into
 * fixed chunks of GM_PARZEN_CHUNK rows whose partial (max, sum) pairs go to `workspace` (caller-owned device memory,
 * 8-byte aligned, at least gm_parzen_workspace_bytes(nq, ns, n_sigma) =
 *     8 * n_sigma * nq * ceil(ns / GM_PARZEN_CHUNK) + 4 * (nq + ns)  bytes).
 * Bitwise deterministic, and a query's row does not depend on which other queries are in the call.
 * metrics.parzen_log_likelihood (Python) is the call site; trainers' parzen() selects sigma on the validation rows.
 * gm_parzen_workspace_bytes returns GM_EINVAL for nq, ns < 1 or n_sigma outside [1, GM_PARZEN_MAX_SIGMAS]. */
#define GM_PARZEN_CHUNK 128
#define GM_PARZEN_MAX_SIGMAS 16
int64_t gm_parzen_workspace_bytes(int nq, int ns, int n_sigma);
int gm_parzen_ll(void* stream, const float* q, int64_t ldq, int nq, const float* s, int64_t lds, int ns, int d,
                 const float* sigmas, int n_sigma, void* workspace, int64_t ws_bytes, float* out, int64_t ldo);

/* ---- class-conditional VAE (NEW: the reference's README lists "Models: CVAE" as to-do, README.md:95;
 * generative_models_amd/src/cvae.py).  A conditioned layer computes linear(cat[x, onehot(y)]) in its split form
 * x W^T + b + E[:, y], E = label.weight [N, C] (nn.Linear(C, N, bias=False)): the one-hot input is one column of E
 * per row, added where the bias is added.  Row m's class is  y_m = labels[idx ? idx_row[m] : m]  with
 * idx_row = idx + idx_slot's offset: the batch's row of the index ring its images were gathered through (int64),
 * labels the dataset's classes (int32).  Every label must lie in [0, C): the engine validates a dataset on the host
 * before its first launch; the kernels clamp the class they index E with all the same. */
typedef struct gm_label_src {
    const int32_t* labels;
    const int64_t* idx;       /* NULL: row m reads labels[m] */
    gm_slot idx_slot;
} gm_label_src;
/* gm_vae_reparam_fwd whose decoder-layer workgroups add E[:, y_m] before the activation: CVAE.forward's
 * reparameterisation + Decoder.linear/label (cvae.py), called from vae_engine.CVAEEngine._issue. */
int gm_vae_reparam_fwd_label(void* stream, const float* ml, int64_t ldml, const float* eps, gm_slot eps_slot,
                             float* z, int64_t ldz, float* kl_part, int n_part, int B, int Z, const float* W,
                             const float* bias, float* H, int64_t ldh, int N, int act, const float* E, int C,
                             gm_label_src lab);
/* Label-weight gradient of up to two conditioned layers in ONE launch: dE[n, c] = sum over rows m with y_m = c of
 * dPre[m, n] (dPre: d loss / d pre-activation, [M, N]), added in ascending m and combined in a fixed order -- no
 * atomics, the same bits on every run; a class absent from the batch gets exactly 0.  gE != NULL: the gradient is
 * written there [N, C].  E != NULL: Adam (torch's, weight decay folded into the gradient) steps (E, mE, vE) with the
 * schedule row sched[2 * slot .. +1] in the same launch.  Called from vae_engine.CVAEEngine._issue (both layers +
 * Adam) and ops._LabelLinear.backward (gradient only). */
typedef struct gm_label_grad_args {
    const float* dPre; int64_t ld; int N;
    float* gE;
    float* E; float* mE; float* vE;
} gm_label_grad_args;
int gm_label_grad_adam(void* stream, const gm_label_grad_args* layers, int n_layers, gm_label_src lab, int M, int C,
                       const float* sched, gm_slot sched_slot, double beta1, double beta2, double eps,
                       double weight_decay);

/* ---- adversarial autoencoder (NEW: the reference's README lists "adversarial autoencoder" as to-do;
 * generative_models_amd/aae.py).  The regularization phase of a batch of B rows: the latent critic
 * D: z (Z) -> relu(W1 z + b1) (H) -> sigmoid(w2 . h + b2) on the B prior rows z_real and the B encoder rows z_fake,
 * loss -mean(log(D(z_real) + 1e-8) + log(1 - D(z_fake) + 1e-8)), then the encoder's generator loss
 * -mean(log(D(encoder(x)) + 1e-8)).  Fused limits: 1 <= Z <= 32 with Z % 4 == 0, 1 <= H <= 512; every entry point
 * returns GM_EINVAL outside them.  No atomics: the same bits on every run. */
typedef struct gm_aae_critic_args {
    const float* z_real; gm_slot real_slot;   /* prior rows: z_real + real_slot's offset, B rows of Z floats */
    const float* z_fake; int64_t ld_fake;     /* the encoder's rows, B of them */
    int B, Z, H;
    float* W1; float* b1; float* w2; float* b2;          /* D.linear [H, Z], [H]; D.discriminate [1, H], [1] */
    float* gW1; float* gb1; float* gw2; float* gb2;      /* gradient outputs (all four, or none with Adam on) */
    float* mW1; float* vW1; float* mb1; float* vb1;      /* Adam moments (with sched) */
    float* mw2; float* vw2; float* mb2; float* vb2;
    const float* sched; gm_slot sched_slot;   /* NULL: gradients only, parameters untouched */
    double beta1, beta2, eps, weight_decay;
    float* loss_out; gm_slot loss_slot;       /* the batch's D loss (or NULL) */
    float* ws; int64_t ws_bytes;              /* workspace of gm_aae_critic_workspace_bytes(B, Z, H) bytes */
} gm_aae_critic_args;
/* Bytes of the critic step's workspace, -1 for a shape outside the fused limits. */
int64_t gm_aae_critic_workspace_bytes(int B, int Z, int H);
/* The whole discriminator phase (aae.py AAETrainer.train_D) in two launches: per 16-row block the forward, loss
 * terms and weight-gradient partials; then one thread per parameter element adds the partials in block order,
 * writes the gradient, steps Adam with the schedule row sched[2 * slot .. +1], and block 0 writes the loss.  Called
 * from vae_engine.AAEEngine._issue and ops_fused.aae_critic_step. */
int gm_aae_critic_step(void* stream, const gm_aae_critic_args* a);
typedef struct gm_aae_gen_args {
    const float* z; int64_t ldz;              /* the encoder's z rows [B, Z] */
    const float* He; int64_t ldhe;            /* the encoder's hidden rows [B, H] (after relu) */
    const float* W1; const float* b1; const float* w2; const float* b2;   /* D after its step */
    const float* Wz;                          /* encoder.z.weight [Z, H] */
    float* dz; int64_t lddz;                  /* out: d G_loss / d z [B, Z] */
    float* dHe; int64_t lddhe;                /* out: d G_loss / d (encoder hidden pre-activation) [B, H] */
    float* loss_part;                         /* out: B row terms -log(D(z) + 1e-8); G_loss is their sum / B */
    int B, Z, H;
} gm_aae_gen_args;
/* The generator phase's narrow part (aae.py AAETrainer.train_G) as ONE launch, 16 rows per workgroup: s = D(z),
 * dz = (dlogit w2 . [h > 0]) W1 and dHe = (dz Wz) . [He > 0].  Called from vae_engine.AAEEngine._issue and
 * ops_fused.aae_gen_mid. */
int gm_aae_gen_mid(void* stream, const gm_aae_gen_args* a);

/* ---- auxiliary-classifier GAN (NEW: Odena, Olah & Shlens, arXiv 1610.09585; generative_models_amd/acgan.py).  The
 * critic D: x -> h = relu(W1 x + b1) (Hd) carries two heads on the same h: the source head sigmoid(w2 . h + b2) with
 * ns_gan.py's loss, and a class head Wc h + bc (C logits) with a softmax cross-entropy against the row's label.
 * Critic mode (gen_mode 0): rows = 2B stacked [x; G(z, y)], rows [0, B) real and [B, 2B) fake, fake row B + m has
 * the class of row m;  loss = -mean(log(s_real + 1e-8) + log(1 - s_fake + 1e-8)) + class_weight (CE_real + CE_fake).
 * Generator mode (gen_mode 1): rows = B generated rows;  loss = -mean(log(s + 1e-8)) + class_weight CE.
 * Both CEs are means over B.  Row m's class comes through lab (gm_label_src) at row m mod B.
 * Limits: 1 <= C <= 32, Hd % 4 == 0, 4 <= Hd <= 1024, rows >= 1; H, w2, Wc and ws 16-byte aligned, ldh % 4 == 0.
 * Outside them, or with a NULL array, both entry points return GM_EINVAL before any launch.  No floating-point
 * atomics: the same bits on every run, in a graph or not. */
typedef struct gm_acgan_heads_args {
    const float* H; int64_t ldh;              /* the critic's hidden rows [rows, Hd] (after relu) */
    int rows, B, Hd, C, gen_mode;
    float* w2; float* b2;                     /* D.discriminate [1, Hd], [1] */
    float* Wc; float* bc;                     /* D.classify [C, Hd], [C] */
    gm_label_src lab;                         /* forward: the batch's classes */
    float class_weight;
    float* da2;                               /* [rows] d loss / d source logit: out of fwd, in of bwd */
    float* dq; int64_t lddq;                  /* [rows, C] class_weight (softmax - onehot) / B: out of fwd, in of bwd */
    /* forward: the iteration's loss values (loss_out NULL: none are written) */
    float* loss_out; gm_slot loss_slot;       /* the total above */
    float* ce_out; gm_slot ce_slot;           /* CE of rows [0, B) (or NULL) */
    float* acc_out; gm_slot acc_slot;         /* critic mode: how many real rows' first maximal logit is the label */
    /* backward */
    float* dPre; int64_t ldp;                 /* out [rows, Hd]: (da2 w2 + dq Wc) . [H > 0] */
    float* gw2; float* gb2; float* gWc; float* gbc;      /* critic mode: gradient outputs (all four, or none) */
    float* mw2; float* vw2; float* mb2; float* vb2;      /* Adam moments (with sched) */
    float* mWc; float* vWc; float* mbc; float* vbc;
    const float* sched; gm_slot sched_slot;   /* critic mode; NULL: gradients only, parameters untouched */
    double beta1, beta2, eps;
    float* ws; int64_t ws_bytes;              /* gm_acgan_heads_workspace_bytes(rows, Hd, C) bytes, zeroed once */
} gm_acgan_heads_args;
/* Bytes of the heads' workspace (shared by both directions), -1 for a shape outside the limits. */
int64_t gm_acgan_heads_workspace_bytes(int rows, int Hd, int C);
/* Both heads' forward and losses from one read of H, ONE launch: da2, dq and (loss_out given) the loss slots, the
 * rows' terms added in a fixed order by the last workgroup to finish.  Called from acgan.ACGANEngine._issue and
 * ops_fused.acgan_heads_fwd. */
int gm_acgan_heads_fwd(void* stream, const gm_acgan_heads_args* a);
/* Both heads' backward from one read of H: dPre in gm_head_bwd's place (consumed by gm_linear_bwd_dw_ex /
 * gm_linear_bwd_dx_ex unchanged); in critic mode a second launch adds the row blocks' partial gw2 / gb2 / gWc / gbc
 * in block order, writes them and steps Adam on the four tensors with sched[2 * slot .. +1].  Generator mode
 * refuses gradient outputs and a schedule (the critic is frozen).  Called from acgan.ACGANEngine._issue and
 * ops_fused.acgan_heads_bwd. */
int gm_acgan_heads_bwd(void* stream, const gm_acgan_heads_args* a);

/* ---- spectrally normalised hinge GAN (NEW: Miyato et al., arXiv 1802.05957; the hinge loss and two-time-scale Adam of
 * arXiv 1805.08318; generative_models_amd/sngan.py).  The critic D: x -> h = relu(Wbar x + b) -> s = w2bar . h + b2 with
 * Wbar = W / sigma and w2bar = w2 / ||w2||; sigma comes from ONE power-iteration step on W [H, I] per forward:
 *   v = W^T u / max(||W^T u||, 1e-12);  u' = W v / max(||W v||, 1e-12);  sigma = u'^T W v  (u', v constants of the backward).
 * Limits of all gm_sn_* calls: H % 4 == 0, 4 <= H <= 1024 (the head's float4 lanes; u and W v held in LDS), 1 <= I <= 8192
 * (W^T u, 32 KiB, held in one workgroup's LDS), rows >= 1; W, Wbar, G, gW contiguous [H, I]; H-row arrays and every
 * workspace 16-byte aligned, ldh % 4 == 0.  Outside them, or with a NULL array, every entry point returns GM_EINVAL before
 * any launch.  Sums are accumulated in fp64 in a fixed order; no floating-point atomics: the same bits on every run, in a
 * graph or not.  Workgroups exchange data only across kernel boundaries (the loss slot's arrival counter excepted). */
#define GM_SN_MAX_H 1024
#define GM_SN_MAX_I 8192
#define GM_SN_STAT_SIGMA 0      /* stats[4]: sigma, ||w2||, ||W^T u||, ||W v|| */
#define GM_SN_STAT_NW2 1
#define GM_SN_STAT_NT 2
#define GM_SN_STAT_NR 3
typedef struct gm_sn_power_args {
    const float* W; int H, I;                 /* D.linear.weight [H, I] */
    float* u;                                 /* [H] in; out (u') when update_u */
    float* v;                                 /* [I] out */
    float* Wbar;                              /* [H, I] out: W / sigma */
    const float* w2; float* w2bar;            /* D.discriminate.weight [H] in, w2 / ||w2|| out */
    float* stats;                             /* [4] out (GM_SN_STAT_*) */
    int update_u;                             /* 0 (eval mode): sigma = u^T W v with the stored u, u is not written */
    float* ws; int64_t ws_bytes;              /* gm_sn_power_workspace_bytes(H, I) */
} gm_sn_power_args;
int64_t gm_sn_power_workspace_bytes(int H, int I);      /* -1 for a shape outside the limits */
/* The power-iteration stage, three launches: t = W^T u (a workgroup per 16 columns walks all rows); W v = W t / ||t|| (a
 * wave per row, every workgroup re-derives ||t|| from t); then every workgroup re-derives ||W v||, u' and sigma and
 * writes its 8 rows of Wbar, workgroup 0 also u (update_u), v, w2bar and stats.  Called from sngan.SNGANEngine._power and
 * ops_fused.sn_power_iter. */
int gm_sn_power_iter(void* stream, const gm_sn_power_args* a);

typedef struct gm_sn_head_args {
    const float* H; int64_t ldh;              /* the critic's hidden rows [rows, Hd] (after relu) */
    int rows, B, Hd, gen_mode;                /* critic mode: rows = 2B stacked [x; G(z)]; generator mode: rows = B */
    const float* w2bar; const float* b2;      /* the normalised head [Hd], D.discriminate.bias [1] */
    float* s;                                 /* [rows] out of fwd: the logits */
    float* ds;                                /* [rows] d loss / d logit: out of fwd, in of bwd */
    float* loss_out; gm_slot loss_slot;       /* fwd: the hinge loss (or NULL) */
    float* dPre; int64_t ldp;                 /* bwd out [rows, Hd]: ds w2bar . [H > 0] */
    const float* stats;                       /* bwd, critic mode: the power stage's stats (||w2||) */
    float* gw2; float* gb2;                   /* bwd, critic mode: d loss / d w2 [Hd] (projected), d loss / d b2 [1] */
    float* ws; int64_t ws_bytes;              /* gm_sn_head_workspace_bytes(rows, Hd), zeroed once */
} gm_sn_head_args;
int64_t gm_sn_head_workspace_bytes(int rows, int Hd);   /* -1 for a shape outside the limits */
/* One launch: per row s = w2bar . h + b2, the hinge term and ds -- critic mode -[1 - s > 0] / B on real rows [0, B) and
 * +[1 + s > 0] / B on fake rows [B, 2B), loss = (sum relu(1 - s_real) + sum relu(1 + s_fake)) / B; generator mode
 * ds = -1 / B, loss = -sum s / B.  The rows' terms are added in fp64 in a fixed order by the last workgroup to finish.
 * Called from sngan.SNGANEngine._issue_D / _issue_G and ops_fused.sn_head_fwd. */
int gm_sn_head_fwd(void* stream, const gm_sn_head_args* a);
/* dPre in gm_head_bwd's place (consumed by gm_linear_bwd_dw / gm_linear_bwd_dx unchanged), one launch; in critic mode
 * each workgroup also writes its 8 rows' partial g = sum ds h and gb2, and a second one-workgroup launch adds them in
 * workgroup order and writes gw2 = (g - <g, w2bar> w2bar) / ||w2|| and gb2.  Generator mode refuses gw2 / gb2.  Called
 * from sngan.SNGANEngine._issue_D / _issue_G and ops_fused.sn_head_bwd. */
int gm_sn_head_bwd(void* stream, const gm_sn_head_args* a);

typedef struct gm_sn_grad_args {
    const float* G;                           /* d loss / d Wbar [H, I] (gm_linear_bwd_dw's output) */
    const float* Wbar; int H, I;
    const float* u; const float* v;           /* the forward's u' [H] and v [I] */
    const float* stats;                       /* the power stage's stats (sigma) */
    float* gW;                                /* out [H, I]: (G - <G, Wbar> u v^T) / sigma; may be G itself */
    float* ws; int64_t ws_bytes;              /* gm_sn_grad_workspace_bytes(H) */
} gm_sn_grad_args;
int64_t gm_sn_grad_workspace_bytes(int H);              /* -1 for a shape outside the limits */
/* The weight gradient's projection, two launches: per 8 rows a partial of c = <G, Wbar>; then every workgroup adds the
 * partials in workgroup order and writes its rows of gW.  Called from sngan.SNGANEngine._issue_D and
 * ops_fused.sn_grad. */
int gm_sn_grad(void* stream, const gm_sn_grad_args* a);

/* ---- Bayesian GAN (NEW: the reference's src/bayes_gan.py is a docstring and a TODO; generative_models_amd/bgan.py,
 * DESIGN.md section 14).  A device-side counter-based generator, the SGHMC update and the critic ensemble's head.
 *
 * Normal(seed, stream s, step t), element e: Philox4x32-10 with key (seed mod 2^32, seed >> 32) and counter
 * (e >> 2, t, s, 0) -> words (x0, x1, x2, x3); u(x) = (2 (x >> 9) + 1) 2^-24; lanes (0, 1) from (x0, x1) and
 * (2, 3) from (x2, x3) by Box-Muller r = sqrt(-2 ln u_a), phi = 2 pi u_b -> (r cos phi, r sin phi); element e takes
 * lane e & 3.  The step is t = (step ? *step : 0) + step_add (a device counter, so a replayed graph advances it). */
#define GM_SGHMC_MAX_SEGS 64
#define GM_BGAN_MAX_J 16
/* Philox4x32-10 raw words: out[4i..4i+3] = philox(ctr[4i..4i+3], key[2i..2i+1]) for i < n (known-answer tests). */
int gm_philox_raw(void* stream, const uint32_t* ctr, const uint32_t* key, uint32_t* out, int64_t n);
/* nstreams draws of n normals: out[j n + e] = Normal(seed, stream0 + j stream_stride, t) element e. */
int gm_philox_normal(void* stream, uint64_t seed, uint32_t stream0, uint32_t stream_stride, int nstreams,
                     const int64_t* step, int64_t step_add, float* out, int64_t n);
typedef struct gm_sghmc_seg {
    int64_t offset;           /* first element of the tensor in the flat buffers */
    int64_t numel;
    uint32_t stream;          /* the noise stream word of the tensor; elements numbered from 0 within it */
    uint32_t reserved;
} gm_sghmc_seg;
typedef struct gm_sghmc_args {
    float* theta; const float* grad; float* mom;   /* flat buffers of n_flat floats */
    int64_t n_flat;
    const gm_sghmc_seg* segs; int nseg;            /* HOST array of 1..GM_SGHMC_MAX_SEGS disjoint segments */
    const int64_t* step; int64_t step_add;         /* the noise step t (device counter or NULL) */
    const float* lr;                               /* device float: the learning rate eta */
    float friction;                                /* alpha, in [0, 1] */
    float prior;                                   /* 1 / (sigma^2 N): g <- g + theta prior */
    float noise;                                   /* 2 alpha / N: the noise std is sqrt(noise eta) */
    uint64_t seed;
} gm_sghmc_args;
/* One SGHMC step (Saatchi & Wilson 2017, Algorithm 1 with gamma-hat = 0) of every segment in ONE launch, one thread
 * per four elements: v <- (1 - alpha) v - eta (g + theta prior) + sqrt(noise eta) xi, theta <- theta + v, with
 * xi = Normal(seed, segment stream, t).  No atomics: the same bits on every run. */
int gm_sghmc_step(void* stream, const gm_sghmc_args* a);
typedef struct gm_bgan_head_args {
    float* h; int64_t ldh;          /* [R, Jd H] relu hidden rows of the stacked critics; overwritten by dH */
    const float* w2; const float* b2;   /* [Jd, H] second-layer weights, [Jd] biases */
    float* gw2; float* gb2;         /* out (mode 0): [Jd, H], [Jd] */
    float* loss_out; gm_slot loss_slot; /* out: mode 0 the Jd sums L_D^k, mode 1 the Jg sums L_G^j (or NULL) */
    float* ws; int64_t ws_bytes;    /* workspace of gm_bgan_head_workspace_bytes bytes */
    int mode;                       /* 0: critic update, R = (1 + Jg) B rows [x; G_0(z_0); ...]; 1: generator
                                       update, R = Jg B rows [G_0(z'_0); ...] */
    int B, Jg, Jd, H;
} gm_bgan_head_args;
/* Bytes of gm_bgan_head's workspace, -1 for a shape outside its limits (1 <= Jg, Jd <= 16, H % 4 == 0, H <= 1024). */
int64_t gm_bgan_head_workspace_bytes(int mode, int B, int Jg, int Jd, int H);
/* The critic ensemble's head in two launches: per critic k, logit = h[:, kH:(k+1)H] w2_k + b2_k, s = sigmoid; the
 * contract's loss terms (real rows weight 1/B, fake rows 1/(B Jg) in mode 0; 1/(B Jd) in mode 1, all with the 1e-8
 * terms); dH = dlogit w2_k [h > 0] in place; gw2, gb2 and the loss sums in a fixed order, no atomics. */
int gm_bgan_head(void* stream, const gm_bgan_head_args* a);

/* ---- Denoising VAE (NEW: the reference's README to-do list "denoising VAE"; generative_models_amd/dvae.py, DESIGN.md
 * section 15).  Input corruption x~ ~ p(x~ | x) on the device: Philox4x32-10 (the Bayesian GAN's generator) with key
 * (seed mod 2^32, seed >> 32) and counter (e >> 2, step, row, 0x44564145); pixel e of a row takes word e & 3.
 *   GM_NOISE_SALT_PEPPER, level p in [0, 1]: T = floor(p 2^31); u < T -> 0, else u - T < T -> 1, else x.
 *   GM_NOISE_GAUSSIAN, level sigma >= 0: fmaf(sigma, n, x), n the Box-Muller normal of that word (as gm_philox_normal).
 * Level 0 (or GM_NOISE_NONE) returns x bit for bit.  step = (step_ctr ? *step_ctr : 0) + (step_base ? *step_base : 0)
 * + step_add (truncated to 32 bits), so a captured graph reads a device counter plus a device base; row = row0 + the
 * row's position in the call.  A bad kind, a non-finite or negative level or p > 1 returns GM_EINVAL. */
#define GM_NOISE_NONE 0
#define GM_NOISE_SALT_PEPPER 1
#define GM_NOISE_GAUSSIAN 2
typedef struct gm_corrupt_args {
    int kind;                                 /* GM_NOISE_* */
    double level;                             /* p (salt-and-pepper) or sigma (gaussian) */
    uint64_t seed;
    const int64_t* step_ctr;                  /* device counter or NULL */
    const int64_t* step_base;                 /* device base or NULL */
    int64_t step_add;
    int64_t row0;                             /* batch position of the first row (>= 0) */
} gm_corrupt_args;
/* out[r][e] = corrupt(x[r][e]) for rows r < rows (rows ldx / ldo floats apart; in place when out == x, ldx == ldo). */
int gm_dvae_corrupt(void* stream, const gm_corrupt_args* a, const float* x, int64_t ldx, float* out, int64_t ldo,
                    int64_t rows, int row_elems);
/* gm_gather_rows / gm_gather_rows_bits that also write the corrupted copy of every gathered row to out_c (same ld_out;
 * out_c must be none of data, out).  out is exactly what the plain gather writes. */
int gm_gather_rows_corrupt(void* stream, const gm_corrupt_args* a, const float* data, int64_t n_rows,
                           const int64_t* idx, gm_slot idx_slot, float* out, float* out_c, int64_t ld_out, int B,
                           int row_elems);
int gm_gather_rows_bits_corrupt(void* stream, const gm_corrupt_args* a, const uint32_t* bits, int words_per_row,
                                int64_t n_rows, const int64_t* idx, gm_slot idx_slot, float* out, float* out_c,
                                int64_t ld_out, int B, int row_elems);

/* ---- the linear layers' launches with work riding in them: gm_linear_fwd / gm_linear_bwd_dx / gm_linear_bwd_dw taking
 * ONE descriptor each.  A zero-initialised descriptor with only its base fields set is the plain entry point.  The
 * optional blocks are selected by their pointers (all NULL / 0: block absent), and a descriptor offers exactly the
 * combinations a kernel implements: AT MOST ONE optional block per launch (plus the sub-fields a block names as its
 * own); anything else returns GM_EINVAL before a launch.  Descriptors are read on the host during the call only. */

/* One batch gather (gm_gather_rows and its siblings) riding in a GEMM's grid, or launched next to it where the GEMM's
 * tile configuration cannot carry it.  The gather only reads the index ring and the resident dataset, so any launch
 * that does not touch the gathered rows can carry it: they must be none of the GEMM's operands or outputs. */
typedef struct gm_gather_args {
    const float* data;                    /* fp32 dataset [n_rows, row_elems] ... */
    const uint32_t* bits; int words_per_row;  /* ... or the bit-packed one (gm_gather_rows_bits' layout): exactly one */
    int64_t n_rows; const int64_t* idx; gm_slot idx_slot;
    float* out; int64_t ld_out;           /* fp32 rows out[b, :] = data[idx[b], :] ... */
    uint32_t* out_bits;                   /* ... or the rows as words (gm_gather_rows_bits_packed; bits, forward only;
                                           * ld_out / row_elems unused): exactly one */
    int B, row_elems;
    /* forward only, both or neither: the gather also writes the corrupted copy of every row to out_c (same ld_out;
     * gm_gather_rows_corrupt / gm_gather_rows_bits_corrupt -- the VAE engine's [mu | log_var] forward carrying the NEXT
     * batch's rows); out_c must be none of data, out, the GEMM's operands or its output */
    const gm_corrupt_args* corrupt; float* out_c;
} gm_gather_args;

/* Y[M,N] = act(X W^T + bias) as gm_linear_fwd, and at most one of the blocks below. */
typedef struct gm_fwd_args {
    const float* X; int64_t ldx; gm_slot x_slot; const float* W; const float* bias;
    float* Y; int64_t ldy; int M, K, N, act;
    /* interp: the launch also writes WGAN-GP's interpolate for its first ip_rows output rows (w_gp_gan.py:197-201:
     * x_hat = eps * x + (1 - eps) * G(z), computed where G(z) is produced):
     *   ip_out[m][n] = ip_eps[m] * ip_x[m][n] + (1 - ip_eps[m]) * Y[m][n],  m < ip_rows
     * ip_eps: per-row uniforms (ring base + ip_slot).  Saves the separate gm_interp launch. */
    const float* ip_eps; gm_slot ip_slot; const float* ip_x; int64_t ip_ldx; float* ip_out; int64_t ip_ldo; int ip_rows;
    /* head part: the folded critic head's partial dots hd_part (rows hd_ldp floats apart) and parameter snapshot
     * hd_snap (gm_head_fold_args above); hd_part / hd_snap are neither X nor Y.  With xbits: the first xbits_rows rows
     * of X are read from the packed copy (gm_gather_rows_bits_packed's output, xbits_wpr words per row). */
    const float* hd_w2; const float* hd_b2; float* hd_part; int64_t hd_ldp; float* hd_snap;
    const uint32_t* xbits; int xbits_wpr, xbits_rows;
    /* sqerr (act == GM_ACT_SIGMOID, no x_slot): VAE / AE reconstruction loss where the reconstruction is produced
     * (vae.py:196-203: `recon_loss = torch.sum((images - outputs)**2)` behind Decoder.forward's sigmoid, vae.py:75-77;
     * ae.py:147-160).  The decoder's last layer also writes
     *   sq_dA[m][n] = d loss / d (pre-sigmoid output) = (-2 (x - x_hat) (1 - x_hat)) x_hat   (as gm_sqerr_sigmoid_bwd)
     *   sq_part[m * sq_ldp + j] = sum_{n in 32-column tile j} (x[m][n] - x_hat[m][n])^2,  j < ceil(N / 32) <= sq_ldp
     * with x = sq_target (entries j >= ceil(N / 32) of a row are not written; gm_sum_finalize* over the whole array
     * adds them up in a fixed order).  Replaces the separate gm_sqerr_sigmoid_bwd launch. */
    const float* sq_target; int64_t sq_ldt; float* sq_dA; int64_t sq_lda; float* sq_part; int64_t sq_ldp;
    /* label (no x_slot): Y = act(X W^T + b + lb_E[:, y_m]), lb_E [N, lb_C], 1 <= lb_C <= 32, y_m through lb
     * (gm_label_src): the first layers of CVAE Encoder.forward / Decoder.forward (cvae.py), called from
     * vae_engine.CVAEEngine._issue (encoder; decoder when Z > 32 or Z % 4 != 0) and ops._LabelLinear. */
    const float* lb_E; int lb_C; gm_label_src lb;
    /* gather: gm_linear_fwd and a batch gather as ONE launch (the engine uses the generator's first layer,
     * ns_gan.py:44 + :222-226) */
    const gm_gather_args* gather;
} gm_fwd_args;
int gm_linear_fwd_ex(void* stream, const gm_fwd_args* a);

/* dX[M,K] = (dA W) . act'(below) as gm_linear_bwd_dx, and at most one of the blocks below. */
typedef struct gm_dx_args {
    const float* dA; int64_t lda; const float* W; float* dX; int64_t ldx;
    const float* below; int64_t ld_below; int M, K, N, epi;
    /* add: an additive term before the activation gradient, dX = (dA*W + add_scale*add) * act'(below) (BEGAN's
     * generator sees G(z) both through D and directly in |D(G(z)) - G(z)|, be_gan.py:256) */
    const float* add; int64_t ldadd; float add_scale;
    /* head: the critic head's backward workgroups ride along (generator step: the single scalar workgroup that
     * writes the loss and ticks the iteration counter).  fold (with head only): the folded form, dA = the hidden
     * activations H (gm_head_fold_args above). */
    const gm_head_bwd_args* head; const gm_head_fold_args* fold;
    /* reparam (below == NULL, epi == GM_ACT_ID): VAE reparameterisation backward where dz is produced (vae.py:100-106
     * `z = mu + eps * exp(log_var/2)` and kl_divergence :210-212, autograd of both).  The GEMM runs through the
     * decoder's first layer (dX = dz = dA W, W: [N, Z], K = Z) and its epilogue also writes, with the expressions of
     * gm_vae_reparam_bwd,
     *   rp_dml[m][c] = dz + mu,   rp_dml[m][Z + c] = dz eps exp(lv/2) / 2 + (exp(lv) - 1) / 2
     * from rp_ml = [mu | log_var] and the noise rp_eps (+ rp_slot).  Replaces the separate gm_vae_reparam_bwd launch
     * (bit-identical results). */
    const float* rp_ml; int64_t rp_ldml; const float* rp_eps; gm_slot rp_slot; float* rp_dml; int64_t rp_ldd;
    /* gather: a batch gather to fp32 rows rides in the same launch (no out_bits, no corrupt) */
    const gm_gather_args* gather;
} gm_dx_args;
int gm_linear_bwd_dx_ex(void* stream, const gm_dx_args* a);

/* One weight gradient dW[N,K] = dA^T X, db = colsum(dA) as gm_linear_bwd_dw. */
typedef struct gm_dw_adam_args {
    const float* dA; int64_t lda; const float* X; int64_t ldx; gm_slot x_slot;
    float* dW; float* db; int M, K, N;
    /* sched != NULL: the optimizer folded into the gradient epilogue.  dW/db are written as usual and Adam (same
     * arithmetic as gm_adam) is applied to (pW,mW,vW)/(pb,mb,vb) by the thread that produced the
     * gradient element -- optim.Adam.step (ns_gan.py:139,156) without its own launch.  Single-GPU fast path only (under
     * data parallelism the all-reduce sits between gradient and optimizer).  sched == NULL: plain gradient. */
    float* pW; float* mW; float* vW; float* pb; float* mb; float* vb;
    const float* sched; gm_slot sched_slot;
    double beta1, beta2, eps, weight_decay; float clamp;
    int accumulate;                       /* dW / db += instead of = (plain single gradient only: no sched, head, pair) */
    int ones_from;                        /* with head, see below */
    /* head (single gradient only): gm_head_bwd_fused rides in the launch (gm_head_bwd_args above).  ones_from: a
     * STACKED reduction, the first ones_from rows of dA / X contribute to dW but not to db (WGAN-GP,
     * w_gp_gan.py:207-218: dW1 = [u ; dH]^T [gamma ; X] in one GEMM -- the penalty's second backward has no bias
     * term).  fold: the folded head, dA = the hidden activations H (ones_from == 0); with xbits the first xbits_rows
     * rows of X are read from the packed copy, as in gm_fwd_args. */
    const gm_head_bwd_args* head; const gm_head_fold_args* fold;
    const uint32_t* xbits; int xbits_wpr, xbits_rows;
} gm_dw_adam_args;
typedef struct gm_finalize2_args {
    const float* pa; int na; float scale_a; float* out_a; gm_slot slot_a;
    const float* pb; int nb; float scale_b; float* out_b; gm_slot slot_b;
    int64_t* tick; unsigned int* done;
} gm_finalize2_args;
/* What a PAIR of weight gradients may carry: either the layer-1 fields or fin. */
typedef struct gm_dw_tail {
    /* The generator's pair carrying the NEXT iteration's first layer: after the pair (second = the first layer's
     * dW1 + Adam, required), H[rows, second->N] = relu(z W1^T + b1) with the stepped W1, b1 -- z: rows x second->K at
     * z + the slot's offset, leading dimension ldz.  Bit-identical to the pair followed by gm_linear_fwd, which is what
     * runs where the pair cannot carry it.  H may be none of the pair's arrays. */
    const float* z; int64_t ldz; gm_slot z_slot; float* H; int64_t ldh; int rows;
    /* The pair as the LAST launch of a VAE batch (vae.py:162 + the loss sums of :203 / :212): one more workgroup adds
     * up the two partial arrays exactly as gm_sum_finalize2_tick does, and the last workgroup of the launch to finish
     * advances `tick` (every slot of the batch has been resolved by then).  done: one zero-initialised unsigned int
     * the launch counts its workgroups on and re-arms.  Falls back to separate launches when the pair cannot share a
     * tile. */
    const gm_finalize2_args* fin;
} gm_dw_tail;
/* second != NULL: two weight gradients over the same batch rows as ONE launch (the generator step's two weight
 * gradients are independent once d loss / d hidden is known; neither may consume what the other produces or updates).
 * Falls back to two launches when the pair cannot share a tile configuration.  tail (pair only) may be NULL. */
int gm_linear_bwd_dw_ex(void* stream, const gm_dw_adam_args* first, const gm_dw_adam_args* second,
                        const gm_dw_tail* tail);

/* ---- launch-plan query: what gm_linear_fwd_ex / gm_linear_bwd_dx_ex / gm_linear_bwd_dw_ex WOULD launch for a
 * descriptor, without launching and without a call into the HIP runtime (works on a host without a GPU; the pointers
 * are only looked at for their alignment).  The query runs the entry point's own argument checks and the same pure
 * decision (decide<MODE>: call -> launch plan) whose plan the entry point issues, so it cannot disagree with the launch.
 *   mode: GM_PLAN_MODE_FWD / _DX / _DW; args: a gm_fwd_args / gm_dx_args / gm_dw_adam_args (single gradient);
 *   plan: GM_PLAN_FIELDS ints, written on success (indices below).
 * Plain launches only (for the input gradient with or without `add`, for the weight gradient with or without Adam):
 * a descriptor with a riding block (interp, head part, sqerr, label, gather, head, fold, reparam, xbits, ones_from)
 * returns GM_EUNSUPPORTED; a descriptor the entry point refuses returns what the entry point returns. */
#define GM_EUNSUPPORTED (-10002)
#define GM_PLAN_MODE_FWD 0
#define GM_PLAN_MODE_DX 1
#define GM_PLAN_MODE_DW 2
/* kernel families */
#define GM_PLAN_LDS 1                     /* LDS macro-tile kernel (forward / input gradient over >= 1024 rows) */
#define GM_PLAN_K32 2                     /* forward over a reduction of at most 32 */
#define GM_PLAN_SPLIT 3                   /* 16-wave split reduction */
#define GM_PLAN_RIDING 4                  /* a kernel that carries riding work (not reported in detail) */
/* fields of the plan */
#define GM_PLAN_F_FAMILY 0
#define GM_PLAN_F_MODE 1
#define GM_PLAN_F_MI 2                    /* split reduction: tile = 16 MI x 16 NI (0 otherwise) */
#define GM_PLAN_F_NI 3
#define GM_PLAN_F_LDS_CFG 4               /* LDS: 1 = 64x64 tile, 2 = 32x64 tile (0 otherwise) */
#define GM_PLAN_F_LDS_STAGES 5            /* LDS: stages of the fully unrolled instantiation (13, 25), 0 = runtime loop */
#define GM_PLAN_F_VEC 6                   /* 16-byte loads of the k-contiguous operands */
#define GM_PLAN_F_XV 7                    /* 16-byte loads of the x-contiguous operands */
#define GM_PLAN_F_VEC_EPI 8               /* float4 epilogue */
#define GM_PLAN_F_DMA 9                   /* weight gradient: operand chunks by LDS-DMA */
#define GM_PLAN_F_SLOTS 10                /* the slot-resolving instantiation */
#define GM_PLAN_F_LAUNCHES 11             /* separate kernel launches */
#define GM_PLAN_F_GRID_X 12               /* of the last launch */
#define GM_PLAN_F_GRID_Y 13
#define GM_PLAN_F_BLOCK 14
#define GM_PLAN_FIELDS 16
int gm_linear_plan(int mode, const void* args, int32_t* plan);

/* ---- Primal-Dual Wasserstein GAN (csrc/gm_pdw.hip; pdwgan.py).  One wave per row, fixed
 * reduction order, no atomics.
 * The primal coupling (pdwgan.PDWGANEngine phase 1, after the decoder's output layer): per row of x [B, I] and its
 * reconstruction xr, n[b] = ||x_b - xr_b||_2 (n may be NULL), share[b] = n_b * inv_b (the row's share of mean_b n_b),
 * dA = d share / d (pre-sigmoid xr) = -(d_b * inv_b) xr (1 - xr) with d_b = (x_b - xr_b) / n_b (0 where n_b == 0),
 * xhat = t_b x + (1 - t_b) xr with t = the slot's row of the uniform ring (two rounded products and an add, as
 * gm_interp), xcopy = x.  dA / xhat / xcopy may each be NULL (validation passes all three NULL); xhat and xcopy are
 * row blocks of the critic's stacked input, so no gm_interp launch and no copy is needed. */
int gm_pdw_couple(void* stream, const float* x, int64_t ldx, const float* xr, int64_t ldr, const float* t,
                  gm_slot t_slot, float* n, float* share, float* dA, int64_t ldd, float* xhat, int64_t ldh,
                  float* xcopy, int64_t ldc, float inv_b, int B, int I);
/* The direction penalty (phase 2, in gm_gp_norm's place and with its conventions): g [B, I] = the critic's input
 * gradient at xhat, pen[b] = ||g_b - d_b||^2, gamma_b = lambda * inv_b * 2 (g_b - d_b), d_b rebuilt from x, xr and
 * n (gm_pdw_couple's); a row with x_b == xr_b has d_b = 0. */
int gm_pdw_dir(void* stream, const float* g, int64_t ldg, const float* x, int64_t ldx, const float* xr, int64_t ldr,
               const float* n, float* gamma, int64_t ldm, float* pen, float lambda, float inv_b, int B, int I);

/* ---- Importance-weighted autoencoder (csrc/gm_iwae.hip; iwae.py holds the contract).  k samples
 * per image, rows image-major: sample j of image b is row b * k + j of every [B*k, .] array.  Fixed reduction order, no
 * atomics.  Noise: Philox4x32-10 with key (seed mod 2^32, seed >> 32) and counter (c >> 2, step, row, tag) gives word
 * c & 3 (through gm_philox_normal's Box-Muller mapping) to latent c of noise row `row` = b * k_total + j0 + j, step =
 * (step_ctr ? *step_ctr : 0) + (step_base ? *step_base : 0) + step_add truncated to 32 bits.  k_total >= j0 + k lets
 * a caller run the samples of an image in chunks of k that draw what one call over k_total samples would.
 * Limits: 1 <= k <= 64, 1 <= Z <= 32; outside them, or with a NULL array, every entry point returns GM_EINVAL before
 * any launch. */
#define GM_IWAE_TAG_TRAIN 0x49574145u          /* "IWAE" */
#define GM_IWAE_TAG_EVAL 0x49574556u           /* "IWEV" */
#define GM_IWAE_MAX_K 64
#define GM_IWAE_MAX_Z 32
typedef struct gm_iwae_noise {
    uint64_t seed;
    uint32_t tag;                             /* the fourth counter word */
    const int64_t* step_ctr;                  /* device counter or NULL */
    const int64_t* step_base;                 /* device base or NULL */
    int64_t step_add;
    int64_t k_total;                          /* samples per image of the whole draw (>= j0 + k) */
    int64_t j0;                               /* first sample of this call (>= 0) */
    int64_t q0;                               /* first latent quad of this call (>= 0): its latent c is latent 4 q0 + c
                                               * of the row, so a row wider than the limit can be drawn in pieces */
} gm_iwae_noise;
/* z[b k + j] = mu_b + eps_j exp(lv_b / 2) (gm_reparam_z's roundings) from ml [B, 2Z] = [mu | lv], and
 * lp[b k + j] = 1/2 sum_c (eps_jc^2 - z_jc^2 + lv_bc): the part of log w_j that does not need the decoder. */
int gm_iwae_sample(void* stream, const gm_iwae_noise* n, const float* ml, int64_t ldml, float* z, int64_t ldz,
                   float* lp, int B, int k, int Z);
/* One workgroup per image: sq_j = ||x_b - xr_j||^2 over the image's k rows of xr [B*k, I] (the sigmoid output),
 * log w_j = lp_j - sq_j, m = max_j log w_j, s = sum_j exp(log w_j - m), wn_j = exp(log w_j - m) / s;
 * negL[b] = -(m + log s - log k), ess[b] = s^2 / sum_j exp(log w_j - m)^2 (= 1 / sum_j wn_j^2), wn [B*k];
 * dA [B*k, I] (training; NULL in evaluation) = wn_j * (-2 (x - xr_j) (1 - xr_j) xr_j), the gradient of sum_b negL
 * with respect to the pre-sigmoid output; ms [B, 2] (evaluation; may be NULL) = (m, s), so that chunks of samples
 * combine.  The image's k rows stay in LDS between the two passes while they fit in 64 KB, else they are re-read. */
int gm_iwae_weights(void* stream, const float* x, int64_t ldx, const float* xr, int64_t ldr, const float* lp,
                    float* negL, float* ess, float* wn, float* dA, int64_t lda, float* ms, int B, int k, int I);
/* dz_j = dzdec_j + wn_j z_j (z and eps rebuilt from ml and the counter, never read), dml [B, 2Z] = [sum_j dz_j |
 * sum_j dz_j eps_j exp(lv / 2) / 2 - 1/2], j ascending; dZ [B*k, Z] = dz when not NULL. */
int gm_iwae_reduce(void* stream, const gm_iwae_noise* n, const float* ml, int64_t ldml, const float* wn,
                   const float* dzdec, int64_t lddz, float* dml, int64_t lddml, float* dZ, int64_t lddZ, int B, int k,
                   int Z);

/* ---- Planar-flow posterior of the normalizing-flow VAE (csrc/gm_flow.hip; nfvae.py holds the contract, DESIGN.md
 * section 22).  gm_iwae_sample / gm_iwae_reduce with a chain of K planar layers between z_0 = mu + eps exp(lv / 2) and
 * the decoder; rows, noise block and limits on k and Z are the IWAE's.  Per layer, from the parameters alone:
 * s0 = w.u, u_hat = u + (m(s0) - s0) w / (|w|^2 + 1e-12) with m(x) = -1 + softplus(x), s = w.u_hat; per row:
 * t = tanh(w.z + b), logdet = log(1 + (1 - t^2) s), z <- z + u_hat t.  1 <= K <= 32.  Fixed reduction orders, no
 * atomics.  Out-of-range, NULL or aliased arguments return GM_EINVAL before any launch. */
#define GM_FLOW_MAX_K 32
#define GM_FLOW_PART_STRIDE 68                 /* floats per layer of a partial block */
typedef struct gm_flow_params {
    const float* u;                           /* [K, Z] contiguous */
    const float* w;                           /* [K, Z] contiguous */
    const float* b;                           /* [K] */
    int K;
} gm_flow_params;
/* z [B*k, Z] = z_K and lp[b k + j] = 1/2 |eps|^2 + 1/2 sum_c lv_c + sum_k logdet_k - 1/2 |z_K|^2. */
int gm_flow_sample(void* stream, const gm_iwae_noise* n, const gm_flow_params* f, const float* ml, int64_t ldml,
                   float* z, int64_t ldz, float* lp, int B, int k, int Z);
/* The backward of gm_flow_sample: eps and the chain rebuilt, then walked back from g_K = wn_j z_K + dzdec_j with
 * d loss / d logdet = -wn_j.  dml [B, 2Z] = [sum_j g_0 | sum_j g_0 eps_j exp(lv / 2) / 2 - 1/2], j ascending.  part
 * (16-byte aligned) takes ceil(B / 8) blocks of [K, GM_FLOW_PART_STRIDE] floats, one per workgroup of 8 images: per
 * layer the sums over the block's sample rows of d loss / d u_hat at [0, Z), of d loss / d w through a = w.z + b at
 * [32, 32 + Z), of d loss / d b at 64 and of d loss / d s at 65. */
int gm_flow_reduce(void* stream, const gm_iwae_noise* n, const gm_flow_params* f, const float* ml, int64_t ldml,
                   const float* wn, const float* dzdec, int64_t lddz, float* dml, int64_t lddml, float* part, int B,
                   int k, int Z);
typedef struct gm_flow_step_args {
    const float* part;                        /* gm_flow_reduce's partial blocks */
    int nparts;                               /* their number: ceil(B / 8) */
    float* u; float* w; float* b;             /* the parameters, stepped in place */
    float* gu; float* gw; float* gb;          /* the gradients, written when not NULL (all three or none) */
    float* mu; float* vu; float* mw; float* vw; float* mb; float* vb;      /* Adam moments */
    const float* sched;                       /* [steps, 2]: lr / (1 - b1^t), sqrt(1 - b2^t) (gm_adam's) */
    gm_slot sched_slot;
    double beta1, beta2, eps, weight_decay;
    int K, Z;
} gm_flow_step_args;
/* One workgroup: the partial blocks summed in ascending order, d loss / d u_hat (d s folded in) mapped through the
 * constraint onto u and w, then gm_adam's step on u, w and b at the schedule's slot. */
int gm_flow_step(void* stream, const gm_flow_step_args* a);

/* ---- Inverse-autoregressive-flow posterior of the IAF-VAE (csrc/gm_iaf.hip; iafvae.py holds the contract, DESIGN.md
 * section 31).  gm_iwae_sample / gm_iwae_reduce with a chain of K masked conditioners between z_0 = mu + eps exp(lv / 2)
 * and the decoder; rows, noise block and the limit on k are the IWAE's.  ml [B, 2Z + C] = [mu | lv | h], h the context.
 * Per layer and row: a = elu(W1 z + U h + b1) [F], m = W2[0:Z] a + b2[0:Z], s = W2[Z:2Z] a + b2[Z:2Z], g = sigmoid(s),
 * logdet = -sum softplus(-s), z <- g z + (1 - g) m.  The parameters hold the masked values (MADE's degrees, iafvae.py);
 * only gm_iaf_step reads the degrees.  Limits: 2 <= Z <= 32, 1 <= K <= 8, 4 <= F <= 64 with F % 4 == 0, 0 <= C <= 32,
 * 1 <= k <= 64.  Fixed reduction orders, no atomics.  Out-of-range, NULL or aliased arguments return GM_EINVAL before
 * any launch. */
#define GM_IAF_MIN_Z 2
#define GM_IAF_MAX_Z 32
#define GM_IAF_MAX_K 8
#define GM_IAF_MIN_F 4
#define GM_IAF_MAX_F 64
#define GM_IAF_MAX_C 32
#define GM_IAF_PART_ROWS 64                    /* sample rows per workgroup of gm_iaf_reduce */
/* floats per layer of a partial block: [d W1 (F Z) | d U (F C) | d b1 (F) | d W2 (2Z F) | d b2 (2Z)] */
#define GM_IAF_PART_STRIDE(Z, F, C) ((F) * (Z) + (F) * (C) + (F) + 2 * (Z) * (F) + 2 * (Z))
/* partial blocks of a batch: a workgroup of gm_iaf_reduce owns max(1, 64 / k) whole images */
#define GM_IAF_PARTS(B, k) \
    (((B) + (GM_IAF_PART_ROWS / (k) > 1 ? GM_IAF_PART_ROWS / (k) : 1) - 1) / (GM_IAF_PART_ROWS / (k) > 1 ? GM_IAF_PART_ROWS / (k) : 1))
typedef struct gm_iaf_params {
    const float* W1;                          /* [K, F, Z] contiguous */
    const float* U;                           /* [K, F, C] contiguous; ignored (may be NULL) when C == 0 */
    const float* b1;                          /* [K, F] */
    const float* W2;                          /* [K, 2Z, F], 16-byte aligned: rows 0 .. Z-1 the shift m, Z .. 2Z-1 the gate s */
    const float* b2;                          /* [K, 2Z] */
    int K, F, C;
} gm_iaf_params;
/* z [B*k, Z] = z_K and lp[b k + j] = 1/2 |eps|^2 + 1/2 sum_c lv_c + sum_l logdet_l - 1/2 |z_K|^2; ldml >= 2Z + C. */
int gm_iaf_sample(void* stream, const gm_iwae_noise* n, const gm_iaf_params* f, const float* ml, int64_t ldml,
                  float* z, int64_t ldz, float* lp, int B, int k, int Z);
/* The backward of gm_iaf_sample: eps and the chain rebuilt (the K layer inputs of the rows in flight kept in LDS), then
 * walked back from g_K = wn_j z_K + dzdec_j with d loss / d logdet = -wn_j.  dml [B, 2Z + C] = [sum_j g_0 | sum_j g_0
 * eps_j exp(lv / 2) / 2 - 1/2 | sum_j dh_j], j ascending.  part takes GM_IAF_PARTS(B, k) blocks of [K,
 * GM_IAF_PART_STRIDE(Z, F, C)] floats, one per workgroup: the sums over its rows, ascending, of the five gradients
 * (unmasked: gm_iaf_step applies the masks). */
int gm_iaf_reduce(void* stream, const gm_iwae_noise* n, const gm_iaf_params* f, const float* ml, int64_t ldml,
                  const float* wn, const float* dzdec, int64_t lddz, float* dml, int64_t lddml, float* part, int B,
                  int k, int Z);
typedef struct gm_iaf_step_args {
    const float* part;                        /* gm_iaf_reduce's partial blocks */
    int nparts;                               /* their number: GM_IAF_PARTS(B, k) */
    float* p[5];                              /* W1, U, b1, W2, b2: stepped in place (U's entries ignored when C == 0) */
    float* g[5];                              /* the gradients, written when not NULL (all or none) */
    float* m[5]; float* v[5];                 /* Adam moments, laid out like their parameters */
    const int32_t* m_in;                      /* [K, Z]: the layers' input degrees (the hidden ones follow MADE's rule) */
    const float* sched;                       /* [steps, 2]: lr / (1 - b1^t), sqrt(1 - b2^t) (gm_adam's) */
    gm_slot sched_slot;
    double beta1, beta2, eps, weight_decay;
    int K, Z, F, C;
} gm_iaf_step_args;
/* One thread per entry: the partial blocks summed in ascending order, then gm_adam's step at the schedule's slot.  A
 * masked entry (W1 (j, i) with m_h[j] < m_in[i]; W2 (d, j) with m_in[d] <= m_h[j]; m_h[j] = 1 + j (Z - 1) / F) is
 * skipped: it and its moments are left as they are (0.0), its gradient is written as 0.0. */
int gm_iaf_step(void* stream, const gm_iaf_step_args* a);

/* ---- beta-TCVAE (csrc/gm_tc.hip; tcvae.py holds the contract).  gm_iwae_sample / gm_iwae_reduce at
 * k = 1 with the KL term decomposed by minibatch-weighted sampling over every pair (sample i, posterior j) of the batch.
 * With l'(i, j, d) = -1/2 (lv_jd + (z_id - mu_jd)^2 exp(-lv_jd)) (log N(z_id; mu_jd, exp lv_jd) without -1/2 log 2 pi,
 * which cancels out of every term below), L = log_nm = log(N M), all sums over j including j = i:
 *   J_i = logsumexp_j sum_d l'(i, j, d)            D_id = logsumexp_j l'(i, j, d)
 *   mi_i = sum_d l'(i, i, d) - J_i + L             tc_i = J_i - sum_d D_id + (Z - 1) L
 *   dwkl_i = sum_d D_id - Z L + 1/2 |z_i|^2        lp_i = -(alpha mi_i + beta tc_i + gamma dwkl_i)
 * Rows and the noise block are the IWAE's (the IWAE's two tags: z is gm_iwae_sample's bit for bit).  No [B, B] or
 * [B, B, Z] array is formed; fixed reduction orders, no atomics.  Limits: k = 1, 1 <= Z <= GM_IWAE_MAX_Z, B >= 1,
 * alpha, beta, gamma finite and >= 0; outside them, or with a NULL or aliased array, both return GM_EINVAL before any
 * launch. */
/* z [B, Z], lp [B], the records lse_joint [B] = J and lse_dim [B, Z] = D for gm_tc_reduce, tc [B], and, where not NULL,
 * terms [B, 3] = (mi, tc, dwkl).  One launch, no dependency across the grid: an owner row reads its own z and every
 * row's [mu | lv].  Called from vae_engine.TCVAEEngine._sample (launch 3) and ops_fused.tc_sample. */
int gm_tc_sample(void* stream, const gm_iwae_noise* n, const float* ml, int64_t ldml, float* z, int64_t ldz, float* lp,
                 float* lse_joint, float* lse_dim, int64_t ldd, float* tc, float* terms, float alpha, float beta,
                 float gamma, float log_nm, int B, int k, int Z);
/* The backward of gm_tc_sample: dml [B, 2Z] = d sum_i (-wn_i lp_i) / d [mu | lv] + the reparameterised dzdec.  The
 * coefficient of l'(i, j, d) is wn_i ((beta - alpha) a_ij + (gamma - beta) c_ijd), a_i. = softmax_j sum_d l' (from J),
 * c_i.d = softmax_j l' (from D); row r sums its terms as sample i = r into dz_r and as posterior j = r (z read from z
 * [B, Z]) into dmu_r, dlv_r in one workgroup, then dz_r + gamma wn_r z_r + dzdec_r goes through the reparameterisation
 * (eps rebuilt from the counter) and the alpha term leaves -alpha wn_r / 2 on lv.  One writer per element.  Called from
 * vae_engine.TCVAEEngine._reduce (launch 10) and ops_fused.tc_reduce. */
int gm_tc_reduce(void* stream, const gm_iwae_noise* n, const float* ml, int64_t ldml, const float* z, int64_t ldz,
                 const float* lse_joint, const float* lse_dim, int64_t ldd, const float* wn, const float* dzdec,
                 int64_t lddz, float* dml, int64_t lddml, float alpha, float beta, float gamma, int B, int k, int Z);

/* ---- Gumbel-Softmax posterior of the categorical VAE (csrc/gm_cat.hip; catvae.py holds the contract, DESIGN.md
 * section 23).  N categorical variables of C classes per sample row, rows image-major, gm_iwae_noise's counter layout
 * under the two tags below: element e = n C + c of noise row `row` is word e & 3 of Philox counter (q0 + (e >> 2), step,
 * row, tag), mapped to u in (0, 1) as every uniform here, g = -log(-log(u)).  With l = logits [N, C] of the row's image:
 *   a = (l + g) / tau, y = softmax_c(a), q = softmax_c(l), KL_n = sum_c q_nc (log q_nc + log C).
 * Limits: 2 <= C <= 64, N C <= 1024, 1 <= k <= 64; outside them, or with a NULL or aliased array, both entry points
 * return GM_EINVAL before any launch.  No atomics, fixed orders. */
#define GM_CAT_TAG_TRAIN 0x43415454u           /* "CATT" */
#define GM_CAT_TAG_EVAL 0x43415445u            /* "CATE" */
#define GM_CAT_MIN_C 2
#define GM_CAT_MAX_C 64
#define GM_CAT_MAX_NC 1024
#define GM_CAT_RELAXED 0                       /* y = the relaxed sample, lp = -sum_n KL_n */
#define GM_CAT_ST 1                            /* y = onehot(argmax_c (l + g)), lowest index first; lp as RELAXED */
#define GM_CAT_DISCRETE 2                      /* y as ST, lp = -N log C - sum_n log q_n,z_n, codes written */
#define GM_CAT_NOISE 3                         /* y = g itself; logits, lp, kl unused */
typedef struct gm_cat_args {
    const float* logits; int64_t ldl;         /* [B, N C] */
    const float* tau_tab;                     /* device table read at tau_slot's index (gm_adam's schedule scheme) ... */
    gm_slot tau_slot;
    float tau;                                /* ... or, with tau_tab NULL, the temperature itself (> 0) */
    int B, k, N, C, mode;
    /* gm_cat_sample */
    float* y; int64_t ldy;                    /* [B k, N C]: the decoder's input */
    float* lp;                                /* [B k] */
    float* kl;                                /* [B] = sum_n KL_n per image, or NULL (not written in DISCRETE mode) */
    int32_t* codes;                           /* [B k, N], DISCRETE mode only */
    /* gm_cat_reduce (k = 1) */
    const float* dzdec; int64_t lddz;         /* [B, N C]: d loss / d y */
    const float* wn;                          /* [B]: -d loss / d lp */
    float* dlogits; int64_t lddl;             /* [B, N C], every element written */
} gm_cat_args;
/* Tau is read in RELAXED mode only. */
int gm_cat_sample(void* stream, const gm_iwae_noise* n, const gm_cat_args* a);
/* The backward of RELAXED and of ST (the straight-through estimator uses the relaxed one), g regenerated:
 * da_c = y_c (dy_c - sum_c' y_c' dy_c'), dl_c = da_c / tau + wn q_c (log q_c - sum_c' q_c' log q_c'); y has
 * gm_cat_sample's bits. */
int gm_cat_reduce(void* stream, const gm_iwae_noise* n, const gm_cat_args* a);

/* ---- Denoising diffusion (csrc/gm_ddpm.hip, gm_ddpm.h; ddpm.py holds the contract).  One
 * 256-thread workgroup per row, fixed reduction orders, no floating-point atomics.  Noise: Philox4x32-10 with key
 * (seed mod 2^32, seed >> 32); batch row `row` = row0 + the row's position in the call, step = (step_ctr ? *step_ctr :
 * 0) + (step_base ? *step_base : 0) + step_add truncated to 32 bits.
 *   timestep: word 0 of counter (0, step, row, tag_t), t = mulhi(word, T);
 *   noise of pixels 4q .. 4q + 3: counter (q, step, row, tag_e) through gm_philox_normal's Box-Muller mapping;
 *   x_t = fmaf(s1[t], n, sa[t] * fmaf(2, x, -1)) for an image pixel x in [0, 1].
 * Training draws under (GM_DDPM_TAG_T, GM_DDPM_TAG_E), validation under (GM_DDPM_TAG_V, GM_DDPM_TAG_VE), the sampler's
 * z under GM_DDPM_TAG_S with counter (q, sampler step, sample row, GM_DDPM_TAG_S).
 * Limits: 1 <= I <= 8192, 4 <= E <= 128 with E % 4 == 0, 2 <= T <= 4096; outside them, or with a NULL array, every
 * entry point returns GM_EINVAL before any launch.  Rows that are not 16-byte aligned multiples of 4 floats take an
 * element-by-element path in the same kernels. */
#define GM_DDPM_TAG_T 0x44445054u              /* "DDPT" */
#define GM_DDPM_TAG_E 0x4444504Du              /* "DDPM" */
#define GM_DDPM_TAG_V 0x44445056u              /* "DDPV" */
#define GM_DDPM_TAG_VE 0x44445057u             /* "DDPW" */
#define GM_DDPM_TAG_S 0x44445053u              /* "DDPS" */
#define GM_DDPM_MAX_I 8192
#define GM_DDPM_MIN_E 4
#define GM_DDPM_MAX_E 128
#define GM_DDPM_MAX_T 4096
typedef struct gm_ddpm_noise {
    uint64_t seed;
    uint32_t tag_t, tag_e;                    /* the fourth counter word of the timestep draw and of the noise draw */
    const int64_t* step_ctr;                  /* device counter or NULL */
    const int64_t* step_base;                 /* device base or NULL */
    int64_t step_add;
    int64_t row0;                             /* batch position of the first row (>= 0) */
} gm_ddpm_noise;
typedef struct gm_ddpm_tables {               /* fp32 device tables, built on the host in fp64 and rounded once */
    const float* sa; const float* s1;         /* [T]: sqrt(alpha_bar_t), sqrt(1 - alpha_bar_t) */
    const float* temb;                        /* [T, E]: the sinusoidal embedding of t */
    int T, E;
} gm_ddpm_tables;
typedef struct gm_ddpm_out {
    float* xin; int64_t ldin;                 /* [rows, >= I + E]: row = [x_t | temb[t]], the denoiser's input */
    float* eps; int64_t lde;                  /* [rows, >= I]: the noise */
    int32_t* t;                               /* [rows]: the timestep (may be NULL) */
} gm_ddpm_out;
/* The forward process of `rows` image rows x (ldx floats apart). */
int gm_ddpm_qsample(void* stream, const gm_ddpm_noise* n, const gm_ddpm_tables* s, const gm_ddpm_out* o,
                    const float* x, int64_t ldx, int64_t rows, int I);
/* gm_gather_rows / gm_gather_rows_bits and the forward process of every gathered row in one launch: out is exactly what
 * the plain gather writes, o what gm_ddpm_qsample writes for those rows (o's arrays are none of data, out). */
int gm_gather_rows_qsample(void* stream, const gm_ddpm_noise* n, const gm_ddpm_tables* s, const gm_ddpm_out* o,
                           const float* data, int64_t n_rows, const int64_t* idx, gm_slot idx_slot, float* out,
                           int64_t ld_out, int B, int row_elems);
int gm_gather_rows_bits_qsample(void* stream, const gm_ddpm_noise* n, const gm_ddpm_tables* s, const gm_ddpm_out* o,
                                const uint32_t* bits, int words_per_row, int64_t n_rows, const int64_t* idx,
                                gm_slot idx_slot, float* out, int64_t ld_out, int B, int row_elems);
/* L_simple (Ho et al., arXiv 2006.11239 eq. 14) of one batch: part[b] = sum_e (out - eps)^2 of row b (fp32, fixed
 * order; gm_sum_finalize* scales and adds them up) and, when dA is not NULL, dA = (2 scale) (out - eps) -- with scale =
 * 1 / (B I) the gradient of the batch's mean squared error. */
int gm_ddpm_loss(void* stream, const float* out, int64_t ldo, const float* eps, int64_t lde, float* dA, int64_t lda,
                 float* part, float scale, int B, int I);
/* One sampler step in place on xin, generalised form of Song et al., arXiv 2010.02502 eq. 12, with the coefficients of
 * row s = slot's index of the table coef [S, 8] = (s1_t, sa_t, sa_prev, dir, sigma, t_next, t, 0):
 *   x0 = (x_t - s1_t eps) / sa_t (clamped to [-1, 1] when clip);  eps' = (x_t - sa_t x0) / s1_t;
 *   x_prev = sa_prev x0 + dir eps' + sigma z,  z from counter (q, s, row, GM_DDPM_TAG_S); sigma == 0 draws nothing.
 * temb[t_next] goes into the rows' tails (t_next < 0: the tail stays).  traj (may be NULL): x_prev also to traj +
 * (s + 1) traj_stride, rows I floats apart.  done (may be NULL): one zero-initialised unsigned int the launch counts its
 * workgroups on and re-arms; the last workgroup to arrive advances tick (may be NULL; needs done). */
typedef struct gm_ddpm_reverse_args {
    float* xin; int64_t ldin;
    const float* eps; int64_t lde;            /* the denoiser's output [rows, >= I] */
    const float* coef; gm_slot slot;          /* slot.stride == 8 */
    const float* temb;
    float* traj; int64_t traj_stride;
    uint64_t seed;
    int64_t* tick; unsigned int* done;
    int rows, I, E, T, S, clip;
} gm_ddpm_reverse_args;
int gm_ddpm_reverse(void* stream, const gm_ddpm_reverse_args* a);
/* The sampler's start: xin[:, :I] = z from counter (q, step, row, GM_DDPM_TAG_S), tails temb[t]; traj (may be NULL)
 * takes the same rows, I floats apart. */
int gm_ddpm_prior(void* stream, float* xin, int64_t ldin, const float* temb, uint64_t seed, int64_t step, int t,
                  float* traj, int rows, int I, int E, int T);

/* ---- masked autoregressive model, MADE (Germain et al., arXiv 1502.03509; made.py holds the contract; csrc/gm_made.hip,
 * the sampling rule in csrc/gm_made.h) ----------------------------------------------------------------------------------
 * A 784 -> H -> 784 MLP whose weights are masked by the degrees m_in [I] (a permutation of 1 .. I) and m_h [H] (in
 * [1, I - 1]), int32 device vectors: linear.weight [H, I] keeps (k, i) iff m_h[k] >= m_in[i], out.weight [I, H] keeps
 * (d, k) iff m_in[d] > m_h[k].  No mask is ever stored as a matrix. */
#define GM_MADE_TAG_S 0x4D414453u             /* "MADS": the sampler's fourth counter word */
#define GM_MADE_MIN_I 2
#define GM_MADE_MAX_I 8192
#define GM_MADE_MAX_H 1024
/* The Bernoulli-logit loss of one batch (made.py MADEEngine._issue, MADETrainer.log_likelihood): part[b] = sum_d
 * softplus(a) - x a of row b, softplus(a) = max(a, 0) + log1p(exp(-|a|)) (fp32, fixed order; gm_sum_finalize* scales and
 * adds them up) and, when dA is not NULL, dA = (sigmoid(a) - x) scale -- with scale = 1 / B the gradient of the batch's
 * mean negative log-likelihood in nats per image. */
int gm_made_bce(void* stream, const float* logits, int64_t lda, const float* x, int64_t ldx, float* dA, int64_t ldd,
                float* part, float scale, int B, int I);
/* Zeroes W and Adam's moments m, v (both NULL, or both given) at the masked entries of both layers in one launch
 * (made.py MADEEngine._issue, behind the weight-gradient + Adam launch whose epilogue steps every entry).  Every other
 * entry is left as it is; no weight is read. */
typedef struct gm_made_mask_args {
    float* W1; float* m1; float* v1;          /* linear.weight [H, I] and its moments */
    float* W2; float* m2; float* v2;          /* out.weight [I, H] and its moments */
    const int32_t* m_in; const int32_t* m_h;
    int I, H;
} gm_made_mask_args;
int gm_made_mask(void* stream, const gm_made_mask_args* a);
/* The ancestral sampler in one launch (made.py MADETrainer.sample / complete).  Pixels are drawn in order of degree,
 * inv_order[t] the pixel of degree t + 1; for pixel d of row r:
 *   a = b2[d] + sum_k [m_h[k] < m_in[d]] W2[d, k] relu(h_k)   (lane-local sums in ascending k, then the wave butterfly);
 *   x = 1 iff u < 1 / (1 + expf(-a)) in fp32, u = ph_unit of word d & 3 of Philox4x32-10 at counter (d >> 2, 0, r,
 *   GM_MADE_TAG_S) under key (seed mod 2^32, seed >> 32);   h_k += x W1T[d, k] for every k with m_h[k] >= m_in[d],
 * h starting from b1.  W1T [I, H] is linear.weight transposed (rows H floats apart, like W2's).  The first n_known
 * positions take x from `given` instead of drawing it.  p (may be NULL) receives the conditionals sigmoid(a).  A row's
 * bits depend on (seed, r) and the weights alone, not on n or the grid. */
typedef struct gm_made_sample_args {
    const float* W2; const float* b2;         /* out.weight [I, H], out.bias [I] */
    const float* W1T; const float* b1;        /* linear.weight^T [I, H], linear.bias [H] */
    const int32_t* m_h; const int32_t* inv_order;
    float* x; int64_t ldx;                    /* [n, >= I]: the samples, 0 or 1 (given's value at a known pixel) */
    float* p; int64_t ldp;                    /* [n, >= I] or NULL */
    const float* given; int64_t ldg;          /* [n, >= I]; may be NULL when n_known == 0 */
    uint64_t seed;
    int64_t n;
    int I, H, n_known;                        /* 0 <= n_known <= I */
} gm_made_sample_args;
int gm_made_sample(void* stream, const gm_made_sample_args* a);
/* u[b, d] = the sampler's uniform of pixel d of sample row row0 + b (made.py MADETrainer._sample_general: the sampler of
 * an edited model runs I forward passes under the same rule). */
int gm_made_uniform(void* stream, float* u, int64_t ldu, uint64_t seed, int64_t row0, int64_t rows, int I);

/* ---- RealNVP coupling flow (Dinh, Sohl-Dickstein & Bengio, arXiv 1605.08803; realnvp.py holds the contract; DESIGN.md
 * section 24; csrc/gm_nvp.hip, the shared arithmetic in csrc/gm_nvp.h) -----------------------------------------------
 * An image of D pixels lives as two dense row-major halves A [rows, Da] and B [rows, Db], Da = ceil(D / 2), Db =
 * floor(D / 2): GM_NVP_CHECKER A = the even-indexed pixels, B = the odd ones; GM_NVP_HALF A = the first Da pixels, B =
 * the rest.  Every kernel runs one 256-thread workgroup per row with fixed reduction orders (no floating-point atomics),
 * by 16-byte accesses where a row's width is a multiple of 4 and its base and leading dimension allow them, element by
 * element otherwise.  Out-of-limit fields and NULL return GM_EINVAL before any launch. */
#define GM_NVP_TAG_TRAIN 0x4E565044u           /* "NVPD": the training dequantisation noise */
#define GM_NVP_TAG_EVAL 0x4E565056u            /* "NVPV": validation and log_likelihood */
#define GM_NVP_TAG_S 0x4E565053u               /* "NVPS": the sampler's normals */
#define GM_NVP_MIN_D 2
#define GM_NVP_MAX_D 8192
#define GM_NVP_MAX_H 1024
#define GM_NVP_MAX_K 16
#define GM_NVP_MAX_LEVELS 65536
#define GM_NVP_MAX_S_CAP 8
#define GM_NVP_CHECKER 0
#define GM_NVP_HALF 1
#define GM_NVP_PRE 0                           /* gm_nvp_pre: dequantise + logit + split */
#define GM_NVP_NOISE 1                         /* gm_nvp_pre: u itself, as [B, D] */
#define GM_NVP_POST 0                          /* gm_nvp_post: halves -> image */
#define GM_NVP_PRIOR 1                         /* gm_nvp_post: the sampler's starting normals -> halves */
/* Pixel e of row r with value x in [0, 1]:  q = floor(x (levels - 1) + 0.5) clamped to [0, levels - 1];  v = (q + u) /
 * levels, vc = ((levels - 1 - q) + (1 - u)) / levels (= 1 - v, formed without cancellation; 1 - u is exact);  w = alpha +
 * (1 - 2 alpha) v, wc = alpha + (1 - 2 alpha) vc;  y = log(w) - log(wc);  logdet[r] = sum_e log(1 - 2 alpha) - log(w) -
 * log(wc).  u = ph_unit of word e & 3 of Philox4x32-10 at counter (e >> 2, step, row0 + r, tag) under key (seed mod 2^32,
 * seed >> 32), step = (step_ctr ? *step_ctr : 0) + (step_base ? *step_base : 0) + step_add truncated to 32 bits
 * (gm_corrupt_args' scheme).  GM_NVP_NOISE writes u [B, D] alone. */
typedef struct gm_nvp_pre_args {
    const float* x; int64_t ldx;              /* [B, >= D] */
    float* ya; int64_t lda;                   /* [B, >= Da] */
    float* yb; int64_t ldb;                   /* [B, >= Db] */
    float* logdet;                            /* [B] */
    float* u; int64_t ldu;                    /* GM_NVP_NOISE: [B, >= D] */
    uint64_t seed;
    const int64_t* step_ctr; const int64_t* step_base; int64_t step_add;
    int64_t row0;                             /* batch position of the first row (>= 0) */
    uint32_t tag;
    float alpha;
    int levels, mask, mode, B, D;
} gm_nvp_pre_args;
int gm_nvp_pre(void* stream, const gm_nvp_pre_args* a);
/* One affine coupling on the transformed half (width Dt):  s = s_cap tanh(st[:, :Dt]), t = st[:, Dt:];
 *   forward:  out = in exp(s) + t,  logdet[r] += sum_j s_j (a plain read-add-write by the row's owner);
 *   inverse:  out = (in - t) exp(-s);  logdet is not touched (may be NULL). */
typedef struct gm_nvp_couple_args {
    const float* st; int64_t ldst;            /* [B, >= 2 Dt] */
    const float* inp; int64_t ldin;           /* [B, >= Dt] */
    float* out; int64_t ldout;                /* [B, >= Dt]; none of st, inp */
    float* logdet;                            /* [B] (forward) */
    float s_cap;
    int inverse, B, Dt;
} gm_nvp_couple_args;
int gm_nvp_couple(void* stream, const gm_nvp_couple_args* a);
/* part[r] = 0.5 sum z^2 - logdet[r] + cst over both halves of row r (cst = 0.5 D log(2 pi) + D log(levels), from the
 * host) and, when dza is not NULL, dza = za scale, dzb = zb scale. */
typedef struct gm_nvp_loss_args {
    const float* za; int64_t ldza; const float* zb; int64_t ldzb;
    const float* logdet; float* part;
    float* dza; int64_t lddza; float* dzb; int64_t lddzb;       /* both NULL or both given */
    float cst, scale;
    int B, Da, Db;
} gm_nvp_loss_args;
int gm_nvp_loss(void* stream, const gm_nvp_loss_args* a);
/* The coupling's backward.  g = g0 (+ g1 when not NULL) is the transformed half's cotangent, c the log-determinant's:
 *   dst[:, :Dt] = (g x exp(s) + c) s_cap (1 - tanh^2(st_s)),  dst[:, Dt:] = g,  dx = g exp(s) (dx may be NULL). */
typedef struct gm_nvp_couple_bwd_args {
    const float* st; int64_t ldst;            /* [B, >= 2 Dt] */
    const float* x; int64_t ldx;              /* [B, >= Dt]: the coupling's input */
    const float* g0; int64_t ldg0; const float* g1; int64_t ldg1;
    float* dst; int64_t lddst;                /* [B, >= 2 Dt] */
    float* dx; int64_t lddx;                  /* [B, >= Dt] or NULL */
    float c, s_cap;
    int B, Dt;
} gm_nvp_couple_bwd_args;
int gm_nvp_couple_bwd(void* stream, const gm_nvp_couple_bwd_args* a);
/* GM_NVP_POST:  x[r, e] = clamp((sigmoid(y) - alpha) / (1 - 2 alpha), 0, 1), y the half's entry of pixel e.
 * GM_NVP_PRIOR: the halves' entry of pixel e of row r = temperature * the Box-Muller normal (ph_normal4's word pairing)
 * of element e of Philox counter (e >> 2, 0, row0 + r, GM_NVP_TAG_S); x, alpha unused. */
typedef struct gm_nvp_post_args {
    float* ya; int64_t lda; float* yb; int64_t ldb;             /* read (POST) or written (PRIOR) */
    float* x; int64_t ldx;                    /* POST: [B, >= D] */
    uint64_t seed; int64_t row0;
    float alpha, temperature;
    int mask, mode, B, D;
} gm_nvp_post_args;
int gm_nvp_post(void* stream, const gm_nvp_post_args* a);

/* ---- neural spline flow, NSF (Durkan, Bortoli, Murray & Papamakarios, arXiv 1906.04032; nsf.py holds the contract;
 * DESIGN.md section 37; csrc/gm_nsf.hip, the shared arithmetic in csrc/gm_nsf.h) ---------------------------------------
 * RealNVP's halves, preprocessing, loss, post-processing and noise (the gm_nvp_* kernels above, unchanged) around
 * couplings whose element-wise map is a monotone rational-quadratic spline with linear tails.  ST [B, >= P Dt], P =
 * 3 bins - 1, is parameter-major: column p Dt + j is parameter p of pixel j of the transformed half; parameters
 * 0 .. bins - 1 are theta_w, the next bins theta_h, the last bins - 1 theta_d.  With T = tail_bound, m = 1e-3:
 *   w_i = 2 T (m + (1 - m bins) softmax(theta_w)_i), x_i = -T + (w_0 + .. + w_{i-1}); h_i, y_i likewise of theta_h;
 *   d_0 = d_bins = 1, d_i = m + softplus(theta_d_{i-1} + log(exp(1 - m) - 1)).
 * A pixel with x <= -T or x >= T passes unchanged (log-derivative 0, parameter gradients 0).  Otherwise, in the bin k =
 * #{1 <= i < bins: x >= x_i}, xi = (x - x_k) / w_k clamped to [0, 1], s = h_k / w_k, q = s + (d_{k+1} + d_k - 2 s)
 * xi (1 - xi):  y = y_k + h_k (s xi^2 + d_k xi (1 - xi)) / q,  log dy/dx = 2 log s + log(d_{k+1} xi^2 + 2 s xi (1 - xi) +
 * d_k (1 - xi)^2) - 2 log q.  One 256-thread workgroup per row, a pixel per thread at a time, dword accesses only: any
 * leading dimension >= the width is legal.  bins is one of 4, 8, 16.  Out-of-limit fields, NULL and an output that is
 * an input return GM_EINVAL before any launch. */
#define GM_NSF_MIN_BINS 4
#define GM_NSF_MAX_BINS 16
#define GM_NSF_MAX_TAIL 64
/* forward:  out = the spline of inp, logdet[r] += sum_j log dy/dx (a plain read-add-write by the row's owner);
 * inverse:  out = the spline's inverse of inp (the bin found on the y knots);  logdet is not touched (may be NULL). */
typedef struct gm_nsf_couple_args {
    const float* st; int64_t ldst;            /* [B, >= P Dt] */
    const float* inp; int64_t ldin;           /* [B, >= Dt] */
    float* out; int64_t ldout;                /* [B, >= Dt]; none of st, inp */
    float* logdet;                            /* [B] (forward) */
    float tail_bound;                         /* in (0, GM_NSF_MAX_TAIL] */
    int inverse, B, Dt, bins;
} gm_nsf_couple_args;
int gm_nsf_couple(void* stream, const gm_nsf_couple_args* a);
/* The coupling's backward.  g = g0 (+ g1 when not NULL) is the transformed half's cotangent, c the log-determinant's:
 * dst = d(g . y + c sum_j log dy/dx) / d st, every one of its P Dt columns written (zeros for a pixel in the tails), and
 * dx = the same with respect to x (g itself in the tails; dx may be NULL). */
typedef struct gm_nsf_couple_bwd_args {
    const float* st; int64_t ldst;            /* [B, >= P Dt] */
    const float* x; int64_t ldx;              /* [B, >= Dt]: the coupling's input */
    const float* g0; int64_t ldg0; const float* g1; int64_t ldg1;
    float* dst; int64_t lddst;                /* [B, >= P Dt] */
    float* dx; int64_t lddx;                  /* [B, >= Dt] or NULL */
    float c, tail_bound;
    int B, Dt, bins;
} gm_nsf_couple_bwd_args;
int gm_nsf_couple_bwd(void* stream, const gm_nsf_couple_bwd_args* a);

/* ---- masked autoregressive flow, MAF (Papamakarios, Pavlakou & Murray, arXiv 1705.07057; maf.py holds the contract;
 * DESIGN.md section 30; csrc/gm_maf.hip, the shared arithmetic in csrc/gm_maf.h) ------------------------------------------
 * K layers, each a D -> H -> 2 D MLP masked by the degrees m_in [D] (a permutation of 1 .. D) and m_h [H] (in [1, D - 1]),
 * int32 device vectors: linear.weight [H, D] keeps (j, i) iff m_h[j] >= m_in[i]; both halves of out.weight [2 D, H] (rows
 * 0 .. D - 1 the shift m, rows D .. 2 D - 1 the log-scale pre-activation a) keep (d, j) iff m_in[d] > m_h[j].  A layer
 * maps y to u = (y - m) exp(-s), s = s_cap tanh(a), and subtracts sum_d s_d from the log-determinant.  The preprocessing,
 * the loss and the post-processing are gm_nvp_pre / gm_nvp_loss / gm_nvp_post on the GM_NVP_HALF split with both halves
 * inside one [B, D] array (yb = ya + ceil(D / 2), lda = ldb = D), under the tags below.  Out-of-limit fields, NULL and
 * aliased outputs return GM_EINVAL before any launch. */
#define GM_MAF_TAG_TRAIN 0x4D414644u           /* "MAFD": the training dequantisation noise */
#define GM_MAF_TAG_EVAL 0x4D414656u            /* "MAFV": validation, encode and log_likelihood */
#define GM_MAF_MIN_D 2
#define GM_MAF_MAX_D 8192
#define GM_MAF_MAX_H 1024
#define GM_MAF_MAX_K 16
/* One layer, data -> noise (maf.py MAFEngine._issue, MAFTrainer._forward_rows):  s = s_cap tanh(ma[:, D:]) (nvp_s),
 *   u = (y - ma[:, :D]) exp(-s),  logdet[r] -= sum_d s_d (a plain read-add-write by the row's owner).  One 256-thread
 * workgroup per row, fixed reduction order; 16-byte accesses where D % 4 == 0 and every base and leading dimension allow
 * them, element by element otherwise, with the same bits. */
typedef struct gm_maf_couple_args {
    const float* y; int64_t ldy;              /* [B, >= D]: the layer's input */
    const float* ma; int64_t ldma;            /* [B, >= 2 D]: [m | a], the masked MLP's output */
    float* u; int64_t ldu;                    /* [B, >= D]; none of y, ma */
    float* logdet;                            /* [B] */
    float s_cap;                              /* in (0, GM_NVP_MAX_S_CAP] */
    int B, D;
} gm_maf_couple_args;
int gm_maf_couple(void* stream, const gm_maf_couple_args* a);
/* The layer's backward (maf.py MAFEngine._issue).  g = dL/du, c the log-determinant's cotangent (-1 / B in training):
 *   dout[:, :D] = -g exp(-s),  dout[:, D:] = (-(g u) - c) s_cap (1 - tanh^2(a)) with 1 - tanh^2 as 4 e / (1 + e)^2,
 *   e = exp(-2 |a|),  dy = g exp(-s) (the direct cotangent of the layer's input; dy may be NULL). */
typedef struct gm_maf_couple_bwd_args {
    const float* ma; int64_t ldma;            /* [B, >= 2 D] */
    const float* u; int64_t ldu;              /* [B, >= D]: the layer's output */
    const float* g; int64_t ldg;              /* [B, >= D] */
    float* dout; int64_t lddout;              /* [B, >= 2 D]; none of the inputs */
    float* dy; int64_t lddy;                  /* [B, >= D] or NULL; none of the inputs, not dout */
    float c, s_cap;
    int B, D;
} gm_maf_couple_bwd_args;
int gm_maf_couple_bwd(void* stream, const gm_maf_couple_bwd_args* a);
/* Zeroes W and Adam's moments m, v (both NULL, or both given) at the masked entries of one layer's linear.weight and of
 * both halves of its out.weight in one launch (maf.py MAFEngine._issue, behind the weight-gradient + Adam launch whose
 * epilogue steps every entry; MAFEngine.configure).  Every other entry is left as it is; no weight is read. */
typedef struct gm_maf_mask_args {
    float* W1; float* m1; float* v1;          /* linear.weight [H, D] and its moments */
    float* W2; float* m2; float* v2;          /* out.weight [2 D, H] and its moments */
    const int32_t* m_in; const int32_t* m_h;
    int D, H;
} gm_maf_mask_args;
int gm_maf_mask(void* stream, const gm_maf_mask_args* a);
/* One layer's inverse, noise -> data, in one launch (maf.py MAFTrainer.sample / decode).  Pixels are solved in order of
 * degree, inv_order[t] (clamped into [0, D - 1]) the pixel of degree t + 1; for pixel d of row r at position t:
 *   m = b2[d] + sum_j [m_h[j] <= t] W2[d, j] relu(h_j),  a = b2[D + d] + sum_j [m_h[j] <= t] W2[D + d, j] relu(h_j)
 *   (lane-local sums in ascending j, then the wave butterfly);   s = s_cap tanh(a);   y = u exp(s) + m, the product
 *   rounded before the add;   h_j += y W1T[d, j] for every j with m_h[j] > t,
 * h starting from b1.  W1T [D, H] is linear.weight transposed (rows H floats apart, like W2's).  s (may be NULL) receives
 * the log-scales.  One wave per row: a row's bits depend on its u and the weights alone, not on n or the grid. */
typedef struct gm_maf_invert_args {
    const float* u; int64_t ldu;              /* [n, >= D] */
    float* y; int64_t ldy;                    /* [n, >= D]; not u */
    float* s; int64_t lds;                    /* [n, >= D] or NULL; neither u nor y */
    const float* W2; const float* b2;         /* out.weight [2 D, H], out.bias [2 D] */
    const float* W1T; const float* b1;        /* linear.weight^T [D, H], linear.bias [H] */
    const int32_t* m_h; const int32_t* inv_order;
    float s_cap;
    int64_t n;                                /* 1 <= n <= 2^32 */
    int D, H;
} gm_maf_invert_args;
int gm_maf_invert(void* stream, const gm_maf_invert_args* a);

/* ---- binary restricted Boltzmann machine (Smolensky 1986; Hinton 2002; Tieleman 2008; rbm.py holds the contract;
 * DESIGN.md section 25; csrc/gm_rbm.hip, the noise rule and the pinned arithmetic in csrc/gm_rbm.h) --------------------
 * W [H, I] (linear.weight), c [H] (linear.bias), b [I] (vbias); WT [I, H] is W transposed (gm_rbm_transpose).
 * The noise rule: the uniform of unit e of chain row r at step t under tag T is ph_unit of word e & 3 of Philox4x32-10
 * at counter (e >> 2, t, r, T) under key (seed mod 2^32, seed >> 32); a unit is lit iff u < 1 / (1 + expf(-a)) in fp32.
 * The sum rule: pre_h[j] = c[j], then += WT[i, j] for the lit pixels i in ascending order; pre_v[i] = b[i], then +=
 * W[j, i] for the lit hidden units j in ascending order; one fp32 accumulator per unit. */
#define GM_RBM_TAG_D 0x52424D44u              /* "RBMD": the binarisation of the input rows, t = the batch step */
#define GM_RBM_TAG_H 0x52424D48u              /* "RBMH": hidden draws, t = the Gibbs step */
#define GM_RBM_TAG_V 0x52424D56u              /* "RBMV": visible draws, t = the Gibbs step */
#define GM_RBM_MAX_DIM 1024                   /* 1 <= I, H <= 1024 */
#define GM_RBM_MAX_STEPS (1 << 24)
/* A Gibbs chain per row in ONE launch.  With C = (step_ctr ? *step_ctr : 0) + (step_base ? *step_base : 0):
 *   v = v0 = (u_D < x) at t = C + d_add (truncated to 32 bits);  then for s = 0 .. steps - 1, at t = C g_mul + g_add + s:
 *   h ~ sigmoid(pre_h(v)),  v ~ sigmoid(pre_v(h)).   steps = 0 binarises only (p_out, a_out are then left untouched).
 * v0_out, v_out: 0 / 1 floats (either may be x itself);  p_out, a_out: the conditionals of the LAST visible draw and
 * their logits.  Every output is optional.  Chain row = row0 + the row's position: a row's bits do not depend on n.
 * Tempering (all three of betas, b_A, logw, or none; steps >= 1): betas[steps + 1] a device table; step s forms pre_h,
 * adds (betas[s+1] - betas[s]) (b - b_A).v + sum_j sp(betas[s+1] pre_h_j) - sp(betas[s] pre_h_j) to the row's log-weight
 * (sp(a) = max(a, 0) + log1pf(expf(-|a|)); fp32 per lane, the wave butterfly, then fp64 across steps), draws h from
 * sigmoid(betas[s+1] pre_h) and v from sigmoid(betas[s+1] pre_v + (1 - betas[s+1]) b_A).  logw[r] receives the sum. */
typedef struct gm_rbm_chain_args {
    const float* W; const float* WT; const float* c; const float* b;
    const float* x; int64_t ldx;              /* [n, >= I] in [0, 1] */
    float* v0_out; int64_t ldv0;              /* [n, >= I] or NULL */
    float* v_out; int64_t ldv;                /* [n, >= I] or NULL */
    float* p_out; int64_t ldp;                /* [n, >= I] or NULL */
    float* a_out; int64_t lda;                /* [n, >= I] or NULL */
    uint64_t seed;
    int64_t row0;                             /* chain row of the first row (>= 0) */
    const int64_t* step_ctr; const int64_t* step_base;          /* device words or NULL */
    int64_t d_add, g_mul, g_add;              /* host parts of the binarisation step and of the first Gibbs step */
    const float* betas; const float* b_A; double* logw;         /* the tempering block */
    int64_t n;
    int I, H, steps;
} gm_rbm_chain_args;
int gm_rbm_chain(void* stream, const gm_rbm_chain_args* a);
/* From pre [2B, H] = linear(V) of the stacked V = [v0; vk] [2B, I]:  dA [2B, H] = [-sigmoid(pre0); +sigmoid(prek)] inv_b
 * (dA may be pre itself) and part[r] = +F(v0_r) for r < B, -F(vk_r) otherwise, F(v) = -b.v - sum_j sp(pre_j): inv_b times
 * their sum is the batch's free-energy gap (gm_sum_finalize*). */
int gm_rbm_grad(void* stream, const float* pre, int64_t ldpre, const float* V, int64_t ldv, const float* b, float* dA,
                int64_t ldd, float* part, float inv_b, int B, int I, int H);
/* The visible bias: g[i] = inv_b sum_{r < B} (V[B + r, i] - V[r, i]), rows in ascending order; g (may be NULL) receives
 * it; with pb (then mb, vb, sched too) Adam steps b in the same launch by gm_adam's arithmetic. */
typedef struct gm_rbm_vbias_args {
    const float* V; int64_t ldv;              /* [2B, >= I] */
    float* g;                                 /* [I] or NULL */
    float* pb; float* mb; float* vb;          /* [I] each, or all NULL */
    const float* sched; gm_slot sched_slot;
    double beta1, beta2, eps, weight_decay;
    float inv_b;
    int B, I;
} gm_rbm_vbias_args;
int gm_rbm_vbias(void* stream, const gm_rbm_vbias_args* a);
/* WT [cols, rows] = W [rows, cols]^T, 32-bit words copied bit for bit (rows ldw / ldt floats apart). */
int gm_rbm_transpose(void* stream, const float* W, int64_t ldw, float* WT, int64_t ldt, int rows, int cols);
/* u[r, e] = the rule's uniform of unit e < width of chain row row0 + r under `tag`, at step (step_ctr ? *step_ctr : 0) +
 * (step_base ? *step_base : 0) + step_add truncated to 32 bits. */
int gm_rbm_uniform(void* stream, float* u, int64_t ldu, uint64_t seed, uint32_t tag, const int64_t* step_ctr,
                   const int64_t* step_base, int64_t step_add, int64_t row0, int64_t rows, int width);

/* ---- Vector quantisation of the VQ-VAE (csrc/gm_vq.hip; vqvae.py holds the contract).  N
 * variables of D floats per row, a codebook E [K, D].  Per row and variable n: c_n = argmin_k sum_d (z_e,n,d - E_k,d)^2,
 * the lowest index winning a tie, 0 when no distance compares less (NaN); z_q = E[c]; qerr = sum_n ||z_e,n - E_c_n||^2
 * from the direct differences; lp = -(1 + beta) qerr.
 * Limits: 4 <= D <= 64 with D % 4 == 0, N D <= 1024, 2 <= K <= 1024, K D <= 16384 (the codebook in 64 KB of LDS);
 * outside them, or with a NULL or aliased array, the entry points return GM_EINVAL before any launch.  No floating-point
 * atomics, fixed orders: the same bits on every run, and a row's outputs do not depend on where the row lands. */
#define GM_VQ_MIN_D 4
#define GM_VQ_MAX_D 64
#define GM_VQ_MAX_ND 1024
#define GM_VQ_MIN_K 2
#define GM_VQ_MAX_K 1024
#define GM_VQ_MAX_KD 16384
typedef struct gm_vq_args {
    const float* ze; int64_t ldz;             /* [B, N D]: the encoder's output */
    const float* E; int64_t lde;              /* [K, D]: the codebook */
    int32_t* codes; int64_t ldc;              /* [B, N]: written by gm_vq_quantise, read by gm_vq_reduce */
    float beta;                               /* the commitment cost: finite, >= 0 */
    int B, N, D, K;
    /* gm_vq_quantise */
    float* zq; int64_t ldq;                   /* [B, N D] = E[codes]: the decoder's input */
    float* qerr;                              /* [B] */
    float* lp;                                /* [B] = -(1 + beta) qerr */
    /* gm_vq_reduce */
    const float* dzdec; int64_t lddz;         /* [B, N D]: d loss / d z_q */
    const float* wn;                          /* [B]: -d loss / d lp (1 at k = 1) */
    float* dml; int64_t lddml;                /* [B, N D], every element written */
} gm_vq_args;
/* One wave per row, the codebook in LDS: lanes are (variable slot, share of the K codes); the search compares the direct
 * squared distances, each summed over d ascending. */
int gm_vq_quantise(void* stream, const gm_vq_args* a);
/* dml = dzdec + 2 beta wn (z_e - E[codes]): the decoder's input gradient passed straight through, plus the commitment
 * term.  A code outside [0, K) is clamped into it before E is read. */
int gm_vq_reduce(void* stream, const gm_vq_args* a);
typedef struct gm_vq_step_args {
    const float* ze; int64_t ldz;             /* [B, N D] */
    const int32_t* codes; int64_t ldc;        /* [B, N] */
    float* E; float* m; float* v;             /* [K, D] contiguous: the codebook, stepped in place, and its Adam moments */
    float* grad;                              /* [K, D] or NULL: d loss / d E = 2 (n_k E_k - s_k), before weight decay */
    int32_t* nk;                              /* [K] or NULL: n_k, the (row, variable) pairs assigned to code k */
    int32_t* usage;                           /* [K] or NULL: n_k is added to it (one plain integer add per code) */
    const float* sched;                       /* [steps, 2] (gm_adam's), or NULL: gradient and counts only, E untouched */
    gm_slot sched_slot;
    double beta1, beta2, eps, weight_decay;
    int B, N, D, K;
} gm_vq_step_args;
/* One 256-thread workgroup per code: wave w scans quarter w of the B N codes (pair b N + n ascending) and adds the
 * matching rows of z_e in that order; the four partial sums are combined ((0 + 1) + 2) + 3.  The order depends on (B, N)
 * alone.  Then gm_adam's step on E_k at the schedule's slot.  Launch it behind the last reader of E. */
int gm_vq_step(void* stream, const gm_vq_step_args* a);

/* ---- Generative moment matching network (csrc/gm_gmmn.hip; gmmn.py holds the contract).  The
 * kernel maximum mean discrepancy of generated rows X [N, I] and data rows Y [M, I] (each with a leading dimension of
 * its own) under k(a, b) = sum_s exp(-|a - b|^2 / (2 sigma_s^2)), R = [X; Y], T = N + M:
 *   mmd2 = sum_ij k(x_i, x_j) / N^2 - 2 sum_ij k(x_i, y_j) / (N M) + sum_jl k(y_j, y_l) / M^2        (diagonals in)
 *   w(d2) = sum_s exp(-d2 / (2 sigma_s^2)) / sigma_s^2
 *   C[i, j] = -(2 / N^2) w(|x_i - x_j|^2), j < N;   C[i, N + j] = +(2 / (N M)) w(|x_i - y_j|^2);   r_i = sum_j C[i, j]
 *   d mmd2 / d x_i = r_i x_i - (C R)_i.
 * d^2 = |a|^2 + |b|^2 - 2 a.b comes from the Gram form on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 accumulate) over
 * the rows less X's first row, each norm formed by the same MFMA sequence as the dot products; it is clamped at 0 and is
 * exactly 0 for a row against itself and for any two equal rows.  Every sum of kernel values or coefficients is fp64 in
 * a fixed order; no atomics, one writer per element.  Limits: N, M >= 1, N + M < 2^31, 1 <= I <= GM_MMD_MAX_I,
 * 1 <= n_sigma <= GM_MMD_MAX_SIGMAS, leading dimensions >= the row length; outside them, or with a NULL array or a
 * workspace that is too small or not 8-byte aligned, every entry point returns GM_EINVAL before any launch. */
#define GM_MMD_CHUNK 128                       /* partner rows per workgroup */
#define GM_MMD_MAX_SIGMAS 16
#define GM_MMD_MAX_I 8192
#define GM_GMMN_MAX_Z 8192
#define GM_GMMN_MAX_B 2048                     /* training batch: C [B, 2B] is 32 MB there */
#define GM_GMMN_TAG_T 0x474D4D54u              /* "GMMT": the training prior */
#define GM_GMMN_TAG_V 0x474D4D56u              /* "GMMV": the validation prior */
#define GM_GMMN_TAG_S 0x474D4D53u              /* "GMMS": sample(n, seed) */
/* Bytes of caller-owned device workspace of gm_mmd_pairs / gm_mmd_finalize:
 *     40 * ceil(T / 256) * ceil(T / GM_MMD_CHUNK) + (grad ? 8 * ceil(T / GM_MMD_CHUNK) * N : 0) + 4 * 256 * (T / 256 + 1)
 * (T / 256 the integer quotient: the row norms, padded with zeros past every tile of the grid). */
int64_t gm_mmd_workspace_bytes(int N, int M, int grad);
/* z [B, Z] = fmaf(2, u, -1): u the uniform of word e & 3 of Philox block (q0 + (e >> 2), step, b * k_total + j0, tag) of
 * the noise block (gm_iwae_noise's layout with k_total = 1 and j0 the first row's position).  1 <= Z <= GM_GMMN_MAX_Z. */
int gm_gmmn_prior(void* stream, const gm_iwae_noise* n, float* z, int64_t ldz, int B, int Z);
/* Two launches: the row norms, then every tile's pairs.  Leaves the block sums (and, with C, the chunk shares of r) in the
 * workspace for gm_mmd_finalize.  C [N, >= T] (NULL: no gradient; nothing of size N x M is written) takes the
 * coefficients; with ldc % 4 == 0 and C 16-byte aligned they are stored four at a time.  Rc [T, I] (contiguous, caller-
 * owned) takes the centred rows R - mu, mu = X's first row, which both the distances and the product with C are formed
 * from: distances do not change under the shift, r_i x_i - (C R)_i = r_i (x_i - mu) - (C (R - mu))_i about any origin, and
 * about a generated row the sums that cancel in either stay small when the generator has collapsed. */
int gm_mmd_pairs(void* stream, const float* X, int64_t ldx, int N, const float* Y, int64_t ldy, int M, int I,
                 const float* sigmas, int n_sigma, float* C, int64_t ldc, float* Rc, void* workspace, int64_t ws_bytes);
/* stats [10] (fp64, device): mmd2, loss = sqrt(mmd2 + 1e-8) (sqrt_loss) or mmd2, 1 / (2 loss) (or 1), the three block sums
 * xx, xy, yy with their diagonals, xx and yy without them, the xx and yy diagonals (N n_sigma and M n_sigma exactly).
 * grad: r [N] as well (the workspace is the one gm_mmd_pairs filled with a C).  loss_out (may be NULL): the loss as a
 * float. */
int gm_mmd_finalize(void* stream, int N, int M, int n_sigma, int sqrt_loss, int grad, const void* workspace,
                    int64_t ws_bytes, double* stats, float* r, float* loss_out);
/* dA [N, I] = gscale stats[2] (r_i (x - mu) - P) (sigmoid: times x (1 - x), the gradient entering the generator's output
 * layer), P = C (R - mu); mu [I] (NULL: 0, P = C R).  N <= 65535. */
int gm_mmd_grad(void* stream, const float* X, int64_t ldx, const float* mu, const float* P, int64_t ldp, const float* r,
                const double* stats, float gscale, int sigmoid, float* dA, int64_t lda, int N, int I);

/* ---- Flow matching: a continuous normalizing flow trained by velocity regression, with an exact-divergence likelihood
 * (csrc/gm_fm.hip, gm_fm.h; flowmatch.py holds the contract).  The row kernels run one 256-thread
 * workgroup per row with fixed reduction orders; nothing uses floating-point atomics.  Noise: Philox4x32-10 with key
 * (seed mod 2^32, seed >> 32), batch row `row` = row0 + the row's position in the call, step as in gm_ddpm_noise:
 *   dequantisation uniform of pixel e: word e & 3 of counter (e >> 2, step, row, tag_d) (gm_nvp_pre's rule and bits);
 *   grid index: j = mulhi(word 0 of counter (0, step, row, tag_t), T + 1);
 *   y0 of pixels 4q .. 4q + 3: counter (q, step, row, tag_n) through gm_philox_normal's Box-Muller mapping;
 *   y_t = fmaf(tt[j], y1, tc[j] * y0),  u = y1 - y0.
 * Limits: gm_ddpm's on I, E and T, 1 <= H <= GM_FM_MAX_H; outside them, or with a NULL array, every entry point
 * returns GM_EINVAL before any launch. */
#define GM_FM_TAG_D 0x464D5444u                /* "FMTD": training, dequantisation */
#define GM_FM_TAG_T 0x464D5454u                /* "FMTT": training, time */
#define GM_FM_TAG_N 0x464D544Eu                /* "FMTN": training, normals */
#define GM_FM_TAG_VD 0x464D5644u               /* "FMVD": validation, dequantisation */
#define GM_FM_TAG_VT 0x464D5654u               /* "FMVT": validation, time */
#define GM_FM_TAG_VN 0x464D564Eu               /* "FMVN": validation, normals */
#define GM_FM_MAX_H 1024
typedef struct gm_fm_noise {
    uint64_t seed;
    uint32_t tag_d, tag_t, tag_n;
    const int64_t* step_ctr;                  /* device counter or NULL */
    const int64_t* step_base;                 /* device base or NULL */
    int64_t step_add;
    int64_t row0;                             /* batch position of the first row (>= 0) */
} gm_fm_noise;
typedef struct gm_fm_tables {                 /* fp32 device tables over the grid t_j = j / T, j = 0 .. T */
    const float* tt; const float* tc;         /* [T + 1]: j / T and (T - j) / T */
    const float* temb;                        /* [T + 1, E] */
    int T, E;
} gm_fm_tables;
typedef struct gm_fm_out {
    float* xin; int64_t ldin;                 /* [rows, >= I + E]: row = [y_t | temb[j]], the field's input */
    float* u; int64_t ldu;                    /* [rows, >= I]: the regression target y1 - y0 */
    float* logdet;                            /* [rows]: the preprocessing log-determinant (gm_nvp_pre's) */
    int32_t* j;                               /* [rows]: the grid index (may be NULL) */
    float* y1; int64_t ldy1;                  /* [rows, >= I] (may be NULL): the preprocessed rows */
    float* y0; int64_t ldy0;                  /* [rows, >= I] (may be NULL): the normals */
    float alpha; int levels;                  /* gm_nvp_pre's settings */
} gm_fm_out;
/* The path sample of `rows` image rows x in [0, 1] (ldx floats apart). */
int gm_fm_qsample(void* stream, const gm_fm_noise* n, const gm_fm_tables* s, const gm_fm_out* o, const float* x,
                  int64_t ldx, int64_t rows, int I);
/* gm_gather_rows / gm_gather_rows_bits and the path sample of every gathered row in one launch. */
int gm_gather_rows_fm_qsample(void* stream, const gm_fm_noise* n, const gm_fm_tables* s, const gm_fm_out* o,
                              const float* data, int64_t n_rows, const int64_t* idx, gm_slot idx_slot, float* out,
                              int64_t ld_out, int B, int row_elems);
int gm_gather_rows_bits_fm_qsample(void* stream, const gm_fm_noise* n, const gm_fm_tables* s, const gm_fm_out* o,
                                   const uint32_t* bits, int words_per_row, int64_t n_rows, const int64_t* idx,
                                   gm_slot idx_slot, float* out, int64_t ld_out, int B, int row_elems);
/* The exact divergence of the three-layer field from the ReLU patterns of its forward pass:
 *   div[b] = sum_{i, j} [H2[b, i] > 0] Q[i, j] [H1[b, j] > 0]        (-0.0, 0.0 and NaN are not lit)
 * on v_mfma_f32_32x32x2_f32 (exact fp32).  One wave owns 32 rows b and 32 indices i (tile t = i / 32) over all j and
 * writes part[t * B + b]; tiles = ceil(H / 32).  div (may be NULL) = the tiles' partials added in order by a second
 * launch; with div NULL gm_fm_stage adds them.  One writer per output, no atomics, no workgroup waits on another.
 * 1 <= B <= 2^30.  Q must be finite: an entry meets the 0 / 1 pattern as a product inside the MFMA, so a NaN or an
 * infinity in Q reaches every row's result, unlit units included (0 * inf = NaN). */
typedef struct gm_fm_div_args {
    const float* H1; int64_t ld1;             /* [B, >= H] */
    const float* H2; int64_t ld2;             /* [B, >= H] */
    const float* Q; int64_t ldq;              /* [H, >= H] */
    float* part; int64_t part_floats;         /* >= ceil(H / 32) * B floats */
    float* div;                               /* [B] or NULL */
    int B, H;
} gm_fm_div_args;
int gm_fm_div(void* stream, const gm_fm_div_args* a);
/* One solver stage on `rows` rows, its coefficients row s = slot's index of the table tab [S, 8] = (h a, h b, first,
 * last, j_next or -1, j_eval, 0, 0); k the field at this evaluation, d = sum_p div[p * div_stride + row] its divergence:
 *   acc = first ? hb k : fmaf(hb, k, acc);   last: base += acc, y = base;   otherwise: y = fmaf(ha, k, base);
 * y goes to xin[:, :I]; (lbase, lacc) = L[row, 0 .. 1] follow the same rule with d (div NULL: L is left alone);
 * temb[j_next] goes into the rows' tails (j_next < 0: the tail stays).  traj (may be NULL): on a step's last stage y
 * also to traj + (s / stages + 1) traj_stride, rows I floats apart.  done / tick as in gm_ddpm_reverse. */
typedef struct gm_fm_stage_args {
    const float* k; int64_t ldk;              /* [rows, >= I] */
    float* base; int64_t ldb;                 /* [rows, >= I] */
    float* acc; int64_t lda;                  /* [rows, >= I] */
    float* xin; int64_t ldin;                 /* [rows, >= I + E] */
    float* L;                                 /* [rows, 2] (needed with div) */
    const float* div; int64_t div_stride; int div_parts;
    const float* tab; gm_slot slot;           /* slot.stride == 8 */
    const float* temb;                        /* [T + 1, E] */
    float* traj; int64_t traj_stride;
    int64_t* tick; unsigned int* done;
    int rows, I, E, T, S, stages;
} gm_fm_stage_args;
int gm_fm_stage(void* stream, const gm_fm_stage_args* a);

/* ---- Sliced Wasserstein distance (csrc/gm_sw.hip; swg.py holds the contract).  For each of P unit
 * directions theta_p the projections a = X theta_p [N] of the generated rows and b = Y theta_p [M] of the data rows are
 * sorted ascending and matched by rank:
 *   W_p = (1 / (N M)) sum_ij w_ij (a_(i) - b_(j))^2,   w_ij = max(0, min((i+1) M, (j+1) N) - max(i M, j N))
 *   swd2 = (1 / P) sum_p W_p,   d swd2 / d a_i = (2 / (P N M)) sum_j w_ij (a_(i) - b_(j))
 * Elements compare by (value, original row) lexicographically: the order is numpy's stable argsort and unique.  The
 * sort is a data-oblivious compare-exchange network in LDS; padding up to a power of two compares above every real
 * element and is never written out.  Differences are fp32, their squares and every sum fp64 in a fixed order; no
 * atomics, one writer per element.  Outside the limits, with a NULL array, a leading dimension below the width, a short
 * workspace or a misaligned fp64 pointer every entry point returns GM_EINVAL before any launch. */
#define GM_SW_MAX_P 8192                       /* projections per call */
#define GM_SW_MAX_B 2048                       /* rows per side with a gradient: (value, row) pairs, 32 KiB of LDS */
#define GM_SW_MAX_ROWS 16384                   /* rows per side without one: values only, 128 KiB of LDS */
#define GM_SWG_TAG_T 0x53574754u               /* "SWGT": the training prior */
#define GM_SWG_TAG_V 0x53574756u               /* "SWGV": the validation prior */
#define GM_SWG_TAG_S 0x53574753u               /* "SWGS": sample(n, seed) */
#define GM_SWG_TAG_DT 0x53574454u              /* "SWDT": the training directions */
#define GM_SWG_TAG_DV 0x53574456u              /* "SWDV": the validation directions */
#define GM_SWG_TAG_DM 0x5357444Du              /* "SWDM": the metric's directions */
/* Bytes of caller-owned device workspace of gm_sw_sort / gm_sw_finalize: 8 P, the column sums. */
int64_t gm_sw_workspace_bytes(int P);
/* Theta [P, I]: row p is the I normals of Philox blocks (q0 + (e >> 2), step, j0 + p, tag) of the noise block
 * (gm_iwae_noise's layout with k_total = 1 and j0 the first row's position; Box-Muller pairs as everywhere), scaled to unit
 * 2-norm; the norm is summed in fp64 in a fixed order, and a row whose norm is 0 is left at 0.  1 <= I <= GM_MMD_MAX_I. */
int gm_sw_directions(void* stream, const gm_iwae_noise* n, float* Theta, int64_t ldt, int P, int I);
/* Pr [P, >= N + M]: row p holds a_p in columns [0, N) and b_p in [N, N + M).  ws[p] = W_p N M.  Ct [P, >= N] (NULL: no
 * gradient, values only) takes d swd2 / d a_i at Ct[p, i], the row's original position; nothing else of Ct is touched.
 * With Ct 1 <= N, M <= GM_SW_MAX_B, without 1 <= N, M <= GM_SW_MAX_ROWS.  ws is the same, bit for bit, either way. */
int gm_sw_sort(void* stream, const float* Pr, int64_t ldp, int P, int N, int M, float* Ct, int64_t ldc, void* ws,
               int64_t ws_bytes);
/* stats [2] (fp64, device): swd2 = sum_p ws[p] / (P N M) and sqrt(swd2).  loss_out (may be NULL): swd2 as a float. */
int gm_sw_finalize(void* stream, int P, int N, int M, const void* ws, int64_t ws_bytes, double* stats, float* loss_out);

/* ---- graph capture helpers (HIP graphs instead of a tracing compiler) ------------------ */
int gm_graph_begin(void* stream);
int gm_graph_end(void* stream, void** graph_exec_out);
int gm_graph_launch(void* graph_exec, void* stream);
int gm_graph_destroy(void* graph_exec);

/* ---- side streams + cross-stream dependencies, so independent kernels of one iteration become
 * parallel branches of the captured hipGraph */
int gm_stream_create(void** stream_out);
int gm_stream_destroy(void* stream);
int gm_stream_wait_event(void* stream, void* ev);

/* ---- diagnostics: dependent v_mfma_f32_32x32x2_f32 chain on 256 workgroups; out2[0] = shader
 * cycles (s_memtime), out2[1] = 100 MHz wall-clock ticks spanned by block 0. */
int gm_clock_probe(void* stream, int iters, unsigned long long* out2, float* sink);

/* ---- timing helpers for bench.py (HIP events on the launch stream) --------------------- */
int gm_event_create(void** ev_out);
int gm_event_record(void* ev, void* stream);
int gm_event_sync(void* ev);
int gm_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms_out);
int gm_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* GM_HIP_H */
