"""Inverse autoregressive flow VAE, IAF-VAE (Kingma, Salimans, Jozefowicz, Chen, Sutskever & Welling, "Improved Variational
Inference with Inverse Autoregressive Flow", arXiv 1606.04934): vae.py's Encoder and Decoder with a chain of K inverse
autoregressive layers between the encoder's Gaussian and the decoder, every layer a masked two-layer conditioner (MADE's
degrees) that also reads a context vector from the encoder, trained on the k-sample bound of iwae.py.  MAF (maf.py)
turned round: shift and gate of latent i are computed from the EARLIER latents of the layer's INPUT, so sampling and its
density take one parallel pass and only the never-needed inverse is sequential.  Exported by src/iaf_vae.py as Encoder /
Decoder / IAFVAE / IAFVAETrainer.

Model.  IAFVAE(image_size=784, hidden_dim=400, z_dim=20, num_flows=4, flow_hidden=64, context_dim=20) is vae.py's
Encoder and Decoder (state_dict keys kept: a VAE / IWAE checkpoint loads with strict=False); with context_dim C > 0 the
encoder gains `context = Linear(H, C)` (keys encoder.context.*), built AFTER the encoder and the decoder and BEFORE the
flow, so the same manual_seed gives a VAE's weights.  `flow` holds the K layers' stacked parameters W1 [K, F, Z],
U [K, F, C] (absent when C = 0), b1 [K, F], W2 [K, 2Z, F], b2 [K, 2Z] -- rows 0 .. Z-1 of W2 / b2 give the shift m, rows
Z .. 2Z-1 the gate pre-activation s -- and the persistent int32 buffer m_in [K, Z], so a checkpoint carries the order.
Arguments that are no integers, num_flows < 1, flow_hidden < 1 or > 1024, context_dim < 0, z_dim < 2 raise
IAFVAEError(GMError, ValueError).  Fused path (vae_engine.IAFVAEEngine): 2 <= Z <= 32, 1 <= K <= 8,
4 <= F <= 64 with F % 4 == 0, 0 <= C <= 32, 1 <= k <= 64; other valid sizes train on the general path.

Degrees and masks: MADE's rule (made.degrees / made.masks, as maf.degrees stacks them).  m_h[j] = 1 + floor(j (Z - 1) /
F) in every layer; layer 0's m_in[i] = i + 1, layer l's the reverse of layer l - 1's, Z + 1 - m_in.  W1 keeps (j, i) iff
m_h[j] >= m_in[i]; both halves of W2 keep (d, j) iff m_in[d] > m_h[j]; U is unmasked.  The parameters HOLD the masked
values: masked entries are exactly 0.0 after construction and after every optimiser step on every path, and so are
their Adam moments.

Initialisation.  Per layer one nn.Linear(Z + C, F)'s default draws: its weight's first Z columns are W1 (then the mask),
the other C are U, its bias b1.  W2 = 0, b2's m half = 0, b2's s half = 2.0: the paper's "forget-gate" start, g ~= 0.88.

Forward.  Per sample row, with [mu | lv | h] = encoder(x_b) (head width 2Z + C):

    z_0 = mu + eps * exp(lv / 2)
    for l = 0 .. K-1:
        a  = elu(W1_l z + U_l h + b1_l)                          elu with alpha = 1, the paper's choice
        m  = W2m_l a + b2m_l ;  s = W2s_l a + b2s_l
        g  = sigmoid(s) ;  logdet_l = -sum_i softplus(-s_i)      (= sum_i log g_i)
        z  <- g * z + (1 - g) * m
    lp    = 1/2 ||eps||^2 + 1/2 sum_c lv_c + sum_l logdet_l - 1/2 ||z_K||^2
    log w = -||x_b - decoder(z_K)||^2 + lp

L_k = logsumexp_j(log w_j) - log k, the loss sum_b -L_k(x_b), wn = softmax_j(log w_j), ess = 1 / sum_j wn_j^2 and the
reported likelihood L_k - (I / 2) log(pi) are exactly iwae.py's.

Backward (the kernels' closed forms; the reference takes its gradients from autograd).  g_K = wn_j z_K + dzdec_j and
d loss / d logdet = -wn_j; the chain is walked last layer to first, gz' the cotangent of a layer's output:
    dm = gz' (1 - g)        ds = gz' (z - m) g (1 - g) - wn (1 - g)        da = elu'(a) (W2m^T dm + W2s^T ds)
    gz = gz' g + W1^T da    dh += U^T da
dmu and dlv are iwae.py's formulas on g_0 summed over j ascending; d loss / d [mu | lv | h] = [dmu | dlv | dh].

Noise: iwae.py's rule unchanged -- the same counter layout, tags and Box-Muller mapping; `noise_steps` travels in
checkpoints; eps is never stored, the backward regenerates it.

log q.  posterior_samples returns log q(z_K | x) = -lp - 1/2 ||z_K||^2 - (Z / 2) log(2 pi).

General path (an overridden compute_batch or evaluate, an edited model, sizes outside the fused limits): autograd over
ops.fused_linear with weight * mask (`iaf_chain`), eps from ops_fused.iwae_normals (the same counter stream), FlatAdam.

With context_dim = 0 iwae.log_likelihood would accept this model (its Encoder and Decoder are vae.py's) and score it
with the flow left out of q; with a context layer it refuses the encoder.  IAFVAETrainer.log_likelihood is its own
implementation and shadows it."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, made
from ._lib import (IAF_MAX_C, IAF_MAX_F, IAF_MAX_K, IAF_MAX_Z, IAF_MIN_F, IAF_MIN_Z, IWAE_MAX_K, MADE_MAX_H,  # noqa: F401
                   GMError)
from .iwae import LL_BATCH, LL_CHUNK, TAG_EVAL, TAG_TRAIN, IWAETrainer, check_k_seed
from .metrics import IWAEResult
from .trainers import Decoder, Encoder, FlatAdam, _lin, _stock_module, stock, stock_model, to_cuda  # noqa: F401


class IAFVAEError(GMError, ValueError):
    """A bad num_flows, flow_hidden, context_dim or z_dim: a ValueError, and a GMError like the package's other
    refusals."""


def check_config(z_dim, num_flows, flow_hidden, context_dim):
    """(Z, K, F, C) validated; else IAFVAEError."""
    Z, K, F, C = (_lib.check_int(v, n, IAFVAEError) for v, n in ((z_dim, "z_dim"), (num_flows, "num_flows"),
                                                                 (flow_hidden, "flow_hidden"),
                                                                 (context_dim, "context_dim")))
    if Z < IAF_MIN_Z:
        raise IAFVAEError("z_dim must be >= %d (an autoregressive layer over one latent is the identity), got %d"
                          % (IAF_MIN_Z, Z))
    if K < 1:
        raise IAFVAEError("num_flows must be >= 1, got %d" % K)
    if not 1 <= F <= MADE_MAX_H:
        raise IAFVAEError("flow_hidden must lie in [1, %d], got %d" % (MADE_MAX_H, F))
    if C < 0:
        raise IAFVAEError("context_dim must be >= 0, got %d" % C)
    return Z, K, F, C


def fused_sizes(Z, K, F, C):
    """True iff the flow's sizes fit the fused kernels."""
    return (IAF_MIN_Z <= Z <= IAF_MAX_Z and 1 <= K <= IAF_MAX_K and IAF_MIN_F <= F <= IAF_MAX_F and F % 4 == 0
            and 0 <= C <= IAF_MAX_C)


def degrees(z_dim, flow_hidden, num_flows):
    """([m_in of layer 0, ..., m_in of layer K - 1], m_h): int32 arrays; made.degrees' natural order, consecutive layers
    reversed as maf.degrees stacks them."""
    try:
        m_in, m_h = made.degrees(z_dim, flow_hidden)
    except made.MADEError as e:
        raise IAFVAEError(str(e)) from None
    ins = [m_in]
    for _ in range(1, num_flows):
        ins.append((z_dim + 1 - ins[-1]).astype(np.int32))
    return ins, m_h


def flow_masks(m_in, flow_hidden):
    """(M1 [K, F, Z], M2 [K, 2Z, F]) boolean tensors on m_in's device, from the degree buffer m_in [K, Z]."""
    K, Z = m_in.shape
    m_h = torch.from_numpy(made.degrees(Z, flow_hidden)[1]).to(m_in.device)
    M1, M2 = zip(*(made.masks(m_in[l], m_h) for l in range(K)))
    return torch.stack(M1), torch.stack([torch.cat([m, m]) for m in M2])


def _linear(x, W, b):
    from . import ops
    if x.is_cuda:
        return ops.fused_linear(x.contiguous(), W.contiguous(), b, "id")
    return nn.functional.linear(x, W, b)                        # the CPU tests' arithmetic; no trainer reaches it


def iaf_chain(z, h, flow):
    """(z_K [rows, Z], sum_l logdet_l [rows]) of z [rows, Z] with context h [rows, C] (None when C = 0) through the K
    layers of `flow` (anything with W1, U, b1, W2, b2, m_in: the IAFFlow module, or tensors of another dtype).  Torch,
    differentiable; the weights enter as weight * mask, so masked gradients are zero."""
    K, F, Z = flow.W1.shape
    M1, M2 = flow_masks(flow.m_in, F)
    ld = z.new_zeros(z.shape[0])
    U = getattr(flow, "U", None)
    for l in range(K):
        W, x = flow.W1[l] * M1[l].to(z.dtype), z
        if U is not None:
            W, x = torch.cat([W, U[l]], 1), torch.cat([z, h], 1)
        a = nn.functional.elu(_linear(x, W, flow.b1[l]))
        ms = _linear(a, flow.W2[l] * M2[l].to(z.dtype), flow.b2[l])
        m, s = ms[:, :Z], ms[:, Z:]
        g = torch.sigmoid(s)
        ld = ld - nn.functional.softplus(-s).sum(1)
        z = g * z + (1.0 - g) * m
    return z, ld


@stock_model
class IAFFlow(nn.Module):
    """The K layers' stacked parameters and the degree buffer m_in [K, Z]; forward is iaf_chain."""

    def __init__(self, num_flows, z_dim, flow_hidden, context_dim):
        super().__init__()
        K, Z, F, C = num_flows, z_dim, flow_hidden, context_dim
        ins, _ = degrees(Z, F, K)
        lins = [nn.Linear(Z + C, F) for _ in range(K)]           # nn.Linear's default draws, layer by layer
        W = torch.stack([lin.weight.detach() for lin in lins])
        self.W1 = nn.Parameter(W[:, :, :Z].clone())
        if C:
            self.U = nn.Parameter(W[:, :, Z:].clone())
        self.b1 = nn.Parameter(torch.stack([lin.bias.detach() for lin in lins]))
        self.W2 = nn.Parameter(torch.zeros(K, 2 * Z, F))
        b2 = torch.zeros(K, 2 * Z)
        b2[:, Z:] = 2.0                                          # the forget-gate start: g = sigmoid(2) ~= 0.88
        self.b2 = nn.Parameter(b2)
        self.register_buffer("m_in", torch.from_numpy(np.stack(ins).astype(np.int32)))
        self.apply_masks()

    def masks(self):
        """(M1 [K, F, Z], M2 [K, 2Z, F]) as float32 tensors on the buffer's device."""
        M1, M2 = flow_masks(self.m_in, self.W1.shape[1])
        return M1.to(torch.float32), M2.to(torch.float32)

    @torch.no_grad()
    def apply_masks(self):
        """Zeroes the masked entries of W1 and W2 in place (the constructor's last step)."""
        M1, M2 = self.masks()
        self.W1.mul_(M1)
        self.W2.mul_(M2)

    def tensors(self):
        """(W1, U or None, b1, W2, b2)."""
        return self.W1, getattr(self, "U", None), self.b1, self.W2, self.b2

    def forward(self, z, h=None):
        return iaf_chain(z, h, self)


@stock_model
class IAFVAE(nn.Module):
    """vae.VAE's modules and state_dict keys plus encoder.context and `flow`; forward draws one CPU-generator sample as
    vae.VAE does and sends it through the flow."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20, num_flows=4, flow_hidden=64, context_dim=20):
        Z, K, F, C = check_config(z_dim, num_flows, flow_hidden, context_dim)
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = image_size, hidden_dim, Z
        self.num_flows, self.flow_hidden, self.context_dim = K, F, C
        self.encoder = Encoder(image_size=image_size, hidden_dim=hidden_dim, z_dim=Z)
        self.decoder = Decoder(z_dim=Z, hidden_dim=hidden_dim, image_size=image_size)
        if C:                                                    # after the two networks: a VAE's draws come first
            self.encoder.context = nn.Linear(hidden_dim, C)
        self.flow = IAFFlow(K, Z, F, C)
        self.shape = int(image_size ** 0.5)

    def encode(self, x):
        """(mu, log_var, h): h [n, C] the flow's context, None when C = 0."""
        enc = self.encoder
        he = _lin(enc.linear, x, "relu")
        return _lin(enc.mu, he, "id"), _lin(enc.log_var, he, "id"), (_lin(enc.context, he, "id") if self.context_dim
                                                                     else None)

    def forward(self, x):
        mu, log_var, h = self.encode(x)
        z, _ = self.flow(self.reparameterize(mu, log_var), h)
        return self.decoder(z), mu, log_var

    def reparameterize(self, mu, log_var):
        epsilon = to_cuda(torch.randn(mu.shape))
        return mu + epsilon * torch.exp(log_var / 2)


def _encoder_stock(enc, C):
    """True iff enc is vae.py's Encoder with exactly its three layers plus, when C > 0, the context layer."""
    names = ["linear", "mu", "log_var"] + (["context"] if C else [])
    return (type(enc) is Encoder and [n for n, _ in enc.named_children()] == names
            and all(type(c) is nn.Linear for c in enc.children())
            and (not C or (enc.context.out_features == C and enc.context.in_features == enc.mu.in_features)))


def _flow_stock(model):
    """True iff model.flow is the IAFFlow this module ships with parameters and degrees of the model's shape."""
    fl = getattr(model, "flow", None)
    Z, K, F, C = (getattr(model, n, -1) for n in ("z_dim", "num_flows", "flow_hidden", "context_dim"))
    names = ["W1"] + (["U"] if C else []) + ["b1", "W2", "b2"]
    if type(fl) is not IAFFlow or list(fl.children()) or [n for n, _ in fl.named_parameters()] != names:
        return False
    if [n for n, _ in fl.named_buffers()] != ["m_in"] or fl.m_in.dtype != torch.int32 or tuple(fl.m_in.shape) != (K, Z):
        return False
    shapes = [(K, F, Z)] + ([(K, F, C)] if C else []) + [(K, F), (K, 2 * Z, F), (K, 2 * Z)]
    if [tuple(p.shape) for p in fl.parameters()] != shapes:
        return False
    return np.array_equal(fl.m_in.cpu().numpy(), np.stack(degrees(Z, F, K)[0]))


@stock
class IAFVAETrainer(IWAETrainer):
    """IWAETrainer on the IAF posterior: histories `losses` and `ess`, the epoch line, best_val_loss / best_model,
    checkpoints (+ k, seed, num_flows, flow_hidden, context_dim and the training batches taken), sample / parzen from the
    unchanged prior z ~ N(0, I), its own log_likelihood and posterior_samples.  One GPU only."""

    _one_gpu = "IAFVAETrainer"

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, k=1, seed=0):
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz, k=k, seed=seed)

    def _stock(self):
        m = self.model
        if not (self._hooks_stock() and type(m) is IAFVAE and self.k <= IWAE_MAX_K):
            return False
        Z, K, F, C = m.z_dim, m.num_flows, m.flow_hidden, m.context_dim
        if not (fused_sizes(Z, K, F, C) and _encoder_stock(getattr(m, "encoder", None), C)
                and _stock_module(getattr(m, "decoder", None), 2) and type(m.decoder) is Decoder and _flow_stock(m)):
            return False
        if [n for n, _ in m.named_children()] != ["encoder", "decoder", "flow"]:
            return False
        return (self._loader_ok(self.train_iter) and self._loader_ok(self.val_iter)
                and self.train_iter.batch_size == self.val_iter.batch_size)

    def _engine_class(self):
        from .engine import IAFVAEEngine
        return IAFVAEEngine

    def compute_batch(self, batch):
        """(sum_b -L_k, mean ess) of a batch (general path: autograd over the fused linear kernels and iaf_chain, eps from
        the contract's counter stream)."""
        from . import ops_fused as of_
        images, _ = batch
        x = to_cuda(images.view(images.shape[0], -1))
        if not x.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: no GPU is visible")
        b, k = x.shape[0], self.k
        mu, lv, h = self.model.encode(x)
        Z = mu.shape[1]
        train, step = self._noise_step()
        eps = of_.iwae_normals(b, k, Z, self.seed, step, TAG_TRAIN if train else TAG_EVAL, device=x.device)
        eps = eps.view(b, k, Z)
        z0 = mu[:, None, :] + eps * torch.exp(lv / 2)[:, None, :]
        hr = None if h is None else h[:, None, :].expand(b, k, h.shape[1]).reshape(b * k, -1)
        z, ld = self.model.flow(z0.reshape(b * k, Z), hr)
        xr = self.model.decoder(z).view(b, k, -1)
        z, ld = z.view(b, k, Z), ld.view(b, k)
        logw = (-((x[:, None, :] - xr) ** 2).sum(-1) - 0.5 * (z ** 2).sum(-1) + 0.5 * (eps ** 2).sum(-1)
                + 0.5 * lv.sum(-1)[:, None] + ld)
        loss = -(torch.logsumexp(logw, 1) - math.log(k)).sum()
        ess = 1.0 / (torch.softmax(logw.detach(), 1) ** 2).sum(1)
        return loss, ess.mean()

    # ---- evaluation under the flow posterior ------------------------------------------------------------------------
    def _eval_setup(self, images, what):
        m = self.model
        enc, dec = getattr(m, "encoder", None), getattr(m, "decoder", None)
        C = getattr(m, "context_dim", 0)
        if not (type(m) is IAFVAE and _encoder_stock(enc, C) and type(dec) is Decoder and _stock_module(dec, 2)
                and _flow_stock(m)):
            raise GMError("%s needs IAFVAE's encoder, decoder and flow unchanged" % what)
        if images is None:
            images = self.test_iter.dataset.tensors[0]
        x = images.reshape(images.shape[0], -1)
        if not torch.cuda.is_available():
            raise GMError("%s runs on the MI355X only: no GPU is visible" % what)
        dev = enc.linear.weight.device
        if dev.type != "cuda":
            raise GMError("%s: the model is not on the GPU" % what)
        x = x.to(dev, torch.float32).contiguous()
        if not fused_sizes(m.z_dim, m.num_flows, m.flow_hidden, C):
            raise GMError("%s supports the fused kernels' sizes only (got z_dim %d, num_flows %d, flow_hidden %d, "
                          "context_dim %d)" % (what, m.z_dim, m.num_flows, m.flow_hidden, C))
        if enc.linear.weight.shape[1] != x.shape[1]:
            raise GMError("%s: images of %d pixels for a model of %d" % (what, x.shape[1], enc.linear.weight.shape[1]))
        return x, dev, m.z_dim

    def _head_block(self):
        """The packed head [mu ; log_var ; context] of the encoder as one layer, like the engine's."""
        enc = self.model.encoder
        lins = [enc.mu, enc.log_var] + ([enc.context] if self.model.context_dim else [])
        return (torch.cat([l.weight.detach() for l in lins]).contiguous(),
                torch.cat([l.bias.detach() for l in lins]).contiguous())

    def _encode(self, xb, He, ml, head):
        from . import ops
        enc, b = self.model.encoder, xb.shape[0]
        ops.linear_fwd(xb, enc.linear.weight.detach().contiguous(), enc.linear.bias.detach().contiguous(), He, "relu",
                       M=b)
        ops.linear_fwd(He, head[0], head[1], ml, "id", M=b)
        return ml[:b]                                                      # [mu | lv | h]

    def _flow_block(self):
        from . import ops_fused as of_
        self._flow_keep = tuple(None if p is None else p.detach().contiguous() for p in self.model.flow.tensors())
        return of_.iaf_params(*self._flow_keep)                            # alive while launches read them

    def log_likelihood(self, images=None, k=500, seed=0):
        """metrics.IWAEResult(ll_mean, ll_stderr, k, n) over `images` ([n, ...]; None: the whole test_iter's dataset):
        log p(x) ~= L_k(x) - (I / 2) log(pi) from k samples per image of the FLOW posterior.  The NF-VAE's schedule: the
        encoder once per batch of LL_BATCH images (noise step = the batch's index, TAG_EVAL, row b * k + j over the whole
        k), the samples through gm_iaf_sample, the decoder and gm_iwae_weights in chunks of at most LL_CHUNK, the chunks'
        (max, sum) combined in fp64.  The global generator, the model's mode and the parameters are untouched."""
        from . import ops
        from . import ops_fused as of_
        k, seed = check_k_seed(k, seed)
        x, dev, Z = self._eval_setup(images, "log_likelihood")
        enc, dec = self.model.encoder, self.model.decoder
        n, I = x.shape
        H, Hd, Wh = enc.linear.weight.shape[0], dec.linear.weight.shape[0], 2 * Z + self.model.context_dim
        w = lambda p: p.detach().contiguous()
        nb, kc = min(LL_BATCH, n), min(LL_CHUNK, k)
        z_ = lambda *s: torch.empty(*s, device=dev)
        He, ml_, Zs, lp, Hdec, Xr = z_(nb, H), z_(nb, Wh), z_(nb * kc, Z), z_(nb * kc), z_(nb * kc, Hd), z_(nb * kc, I)
        negL, ess, wn = z_(nb), z_(nb), z_(nb * kc)
        flow, head = self._flow_block(), self._head_block()
        L = np.empty(n, dtype=np.float64)
        for step, lo in enumerate(range(0, n, nb)):
            b = min(nb, n - lo)
            xb = x[lo:lo + b]
            ml = self._encode(xb, He, ml_, head)
            parts = []
            for j0 in range(0, k, kc):
                c = min(kc, k - j0)
                ms = z_(b, 2)
                of_.iaf_sample(ml, Zs, lp, of_.iwae_noise(seed, TAG_EVAL, k, j0=j0, step=step), flow, b, c, Z)
                ops.linear_fwd(Zs, w(dec.linear.weight), w(dec.linear.bias), Hdec, "relu", M=b * c)
                ops.linear_fwd(Hdec, w(dec.recon.weight), w(dec.recon.bias), Xr, "sigmoid", M=b * c)
                of_.iwae_weights(xb, Xr, lp, negL, ess, wn, b, c, ms=ms)
                parts.append(ms)
            ms = torch.stack(parts).cpu().numpy().astype(np.float64)           # [chunks, b, 2]: one sync per batch
            mx = ms[..., 0].max(0)
            L[lo:lo + b] = mx + np.log((ms[..., 1] * np.exp(ms[..., 0] - mx)).sum(0)) - math.log(k)
        ll = L - 0.5 * I * math.log(math.pi)
        return IWAEResult(float(ll.mean()), float(ll.std()) / math.sqrt(n), k, n)

    def posterior_samples(self, images, k, seed=0):
        """(z [n, k, Z] float32, log_q [n, k] float64) on the CPU: k samples per image of q(z_K | x) and their log
        density, log_q = -lp - 1/2 ||z_K||^2 - (Z / 2) log(2 pi) from gm_iaf_sample's lp.  The noise is
        log_likelihood's (TAG_EVAL, step = the batch's index, row b * k + j)."""
        from . import ops_fused as of_
        k, seed = check_k_seed(k, seed)
        x, dev, Z = self._eval_setup(images, "posterior_samples")
        n = x.shape[0]
        H, Wh = self.model.encoder.linear.weight.shape[0], 2 * Z + self.model.context_dim
        nb, kc = min(LL_BATCH, n), min(LL_CHUNK, k)
        z_ = lambda *s: torch.empty(*s, device=dev)
        He, ml_, Zs, lp = z_(nb, H), z_(nb, Wh), z_(nb * kc, Z), z_(nb * kc)
        flow, head = self._flow_block(), self._head_block()
        zo, lq = torch.empty(n, k, Z), torch.empty(n, k, dtype=torch.float64)
        for step, lo in enumerate(range(0, n, nb)):
            b = min(nb, n - lo)
            ml = self._encode(x[lo:lo + b], He, ml_, head)
            for j0 in range(0, k, kc):
                c = min(kc, k - j0)
                of_.iaf_sample(ml, Zs, lp, of_.iwae_noise(seed, TAG_EVAL, k, j0=j0, step=step), flow, b, c, Z)
                zc = Zs[:b * c].view(b, c, Z).cpu()
                zo[lo:lo + b, j0:j0 + c] = zc
                lq[lo:lo + b, j0:j0 + c] = (-lp[:b * c].view(b, c).cpu().double() - 0.5 * (zc.double() ** 2).sum(-1)
                                            - 0.5 * Z * math.log(2 * math.pi))
        return zo, lq


__all__ = ["Encoder", "Decoder", "IAFVAE", "IAFVAETrainer", "IAFVAEError", "IAFFlow", "iaf_chain", "degrees",
           "flow_masks", "FlatAdam"]
