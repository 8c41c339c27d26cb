"""Normalizing-flow VAE (Rezende & Mohamed, "Variational Inference with Normalizing Flows", arXiv 1505.05770): vae.py's
Encoder and Decoder with a chain of K planar flows between the encoder's Gaussian and the decoder, trained on the
k-sample bound of iwae.py.  Exported by src/nf_vae.py as Encoder / Decoder / NFVAE / NFVAETrainer.

Model.  NFVAE(image_size=784, hidden_dim=400, z_dim=20, num_flows=8) is vae.py's Encoder and Decoder unchanged
(state_dict keys kept: a VAE / IWAE checkpoint loads with strict=False) plus a `flow` module with parameters u [K, Z],
w [K, Z], b [K]; u, w ~ N(0, 0.01^2) from the global generator AFTER the encoder and decoder are built (the same
manual_seed gives a VAE's weights), b = 0.  num_flows < 1 raises NFVAEError(GMError, ValueError).
Fused path: 1 <= K <= 32, 1 <= Z <= 32, 1 <= k <= 64 (vae_engine.NFVAEEngine).

Forward.  Per sample row, with [mu | lv] = encoder(x_b):

    z_0 = mu + eps * exp(lv / 2)
    for k = 1 .. K:
        s0   = w_k . u_k
        u^_k = u_k + (m(s0) - s0) w_k / (||w_k||^2 + 1e-12)        m(x) = -1 + softplus(x)
        a    = w_k . z + b_k         t = tanh(a)                   s = w_k . u^_k   (> -1)
        D    = 1 + (1 - t^2) s  (> 0)   logdet_k = log D           z <- z + u^_k t
    lp    = 1/2 ||eps||^2 + 1/2 sum_c lv_c + sum_k logdet_k - 1/2 ||z_K||^2
    log w = -||x_b - decoder(z_K)||^2 + lp

u^_k depends on the parameters only.  L_k = logsumexp_j(log w_j) - log k, the loss sum_b -L_k(x_b), wn = softmax_j(log
w_j) and ess = 1 / sum_j wn_j^2 are exactly iwae.py's, and so is the reported likelihood L_k - (I / 2) log(pi).
Gradients are those of this forward (the kernels use the closed forms: d loss / d logdet = -wn_j, the chain walked back
from g_K = wn_j z_K + dzdec_j, dmu = sum_j g_0, dlv iwae.py's formula on g_0).

Noise: iwae.py's rule unchanged -- the same counter layout, tags and Box-Muller mapping; `noise_steps` travels in
checkpoints; eps is never stored, the backward regenerates it.

log q.  posterior_samples returns log q(z_K | x) = -lp - 1/2 ||z_K||^2 - (Z / 2) log(2 pi).

General path (an overridden compute_batch or evaluate, an edited model, K, Z or k outside the limits): autograd over
ops.fused_linear, eps from ops_fused.iwae_normals (the same counter stream), the chain (`planar_chain`) in torch.

iwae.log_likelihood would accept this model (its Encoder and Decoder are vae.py's) and score it with the flow left out
of q; NFVAETrainer.log_likelihood is its own implementation and shadows it."""
import math

import numpy as np
import torch
import torch.nn as nn

from ._lib import FLOW_MAX_K, IWAE_MAX_K, IWAE_MAX_Z, GMError
from .iwae import LL_BATCH, LL_CHUNK, TAG_EVAL, TAG_TRAIN, IWAETrainer, check_k_seed
from .metrics import IWAEResult
from .trainers import Decoder, Encoder, FlatAdam, _stock_module, stock, stock_model, to_cuda  # noqa: F401


class NFVAEError(GMError, ValueError):
    """A bad num_flows: a ValueError, and a GMError like the package's other refusals."""


def flow_constants(u, w):
    """(u^ [K, Z], s [K]) of the contract from u, w [K, Z] (torch, any dtype; differentiable)."""
    s0 = (w * u).sum(1)
    coef = (-1.0 + nn.functional.softplus(s0) - s0) / ((w * w).sum(1) + 1e-12)
    uh = u + coef[:, None] * w
    return uh, (w * uh).sum(1)


def planar_chain(z, u, w, b):
    """(z_K [rows, Z], sum_k logdet_k [rows]) of z [rows, Z] through the K planar layers (torch; differentiable)."""
    uh, s = flow_constants(u, w)
    ld = z.new_zeros(z.shape[0])
    for k in range(u.shape[0]):
        t = torch.tanh(z @ w[k] + b[k])
        ld = ld + torch.log(1.0 + (1.0 - t * t) * s[k])
        z = z + t[:, None] * uh[k]
    return z, ld


@stock_model
class PlanarFlow(nn.Module):
    """The K planar layers' parameters u [K, Z], w [K, Z], b [K]; forward is planar_chain."""

    def __init__(self, num_flows, z_dim):
        super().__init__()
        self.u = nn.Parameter(torch.randn(num_flows, z_dim) * 0.01)
        self.w = nn.Parameter(torch.randn(num_flows, z_dim) * 0.01)
        self.b = nn.Parameter(torch.zeros(num_flows))

    def forward(self, z):
        return planar_chain(z, self.u, self.w, self.b)


@stock_model
class NFVAE(nn.Module):
    """vae.VAE's modules and state_dict keys plus `flow`; forward draws one CPU-generator sample as vae.VAE does and
    sends it through the flow."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20, num_flows=8):
        if isinstance(num_flows, bool) or not isinstance(num_flows, (int, np.integer)) or num_flows < 1:
            raise NFVAEError("num_flows must be an integer >= 1, got %r" % (num_flows,))
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim, self.num_flows = image_size, hidden_dim, z_dim, int(num_flows)
        self.encoder = Encoder(image_size=image_size, hidden_dim=hidden_dim, z_dim=z_dim)
        self.decoder = Decoder(z_dim=z_dim, hidden_dim=hidden_dim, image_size=image_size)
        self.flow = PlanarFlow(int(num_flows), z_dim)        # after the two networks: a VAE's draws come first
        self.shape = int(image_size ** 0.5)

    def forward(self, x):
        mu, log_var = self.encoder(x)
        z, _ = self.flow(self.reparameterize(mu, log_var))
        return self.decoder(z), mu, log_var

    def reparameterize(self, mu, log_var):
        epsilon = to_cuda(torch.randn(mu.shape))
        return mu + epsilon * torch.exp(log_var / 2)


def _flow_stock(model):
    """True iff model.flow is the PlanarFlow this module ships with parameters of the model's shape."""
    fl = getattr(model, "flow", None)
    if type(fl) is not PlanarFlow or list(fl.children()) or [n for n, _ in fl.named_parameters()] != ["u", "w", "b"]:
        return False
    K, Z = fl.u.shape[0], getattr(model, "z_dim", -1)
    return tuple(fl.u.shape) == (K, Z) and tuple(fl.w.shape) == (K, Z) and tuple(fl.b.shape) == (K,)


@stock
class NFVAETrainer(IWAETrainer):
    """IWAETrainer on the flow posterior: histories `losses` and `ess`, the epoch line, best_val_loss / best_model,
    checkpoints (+ k, seed, num_flows and the training batches taken), sample / parzen from the unchanged prior
    z ~ N(0, I), its own log_likelihood and posterior_samples.  One GPU only."""

    _one_gpu = "NFVAETrainer"

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, k=1, seed=0):
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz, k=k, seed=seed)

    def _stock(self):
        return (_flow_stock(self.model) and 1 <= self.model.flow.u.shape[0] <= FLOW_MAX_K and super()._stock())

    def _engine_class(self):
        from .engine import NFVAEEngine
        return NFVAEEngine

    def compute_batch(self, batch):
        """(sum_b -L_k, mean ess) of a batch (general path: autograd over the fused linear kernels and the chain in
        torch, eps from the contract's counter stream)."""
        from . import ops_fused as of_
        images, _ = batch
        x = to_cuda(images.view(images.shape[0], -1))
        if not x.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: no GPU is visible")
        b, k = x.shape[0], self.k
        mu, lv = self.model.encoder(x)
        Z = mu.shape[1]
        train, step = self._noise_step()
        eps = of_.iwae_normals(b, k, Z, self.seed, step, TAG_TRAIN if train else TAG_EVAL, device=x.device)
        eps = eps.view(b, k, Z)
        z0 = mu[:, None, :] + eps * torch.exp(lv / 2)[:, None, :]
        z, ld = self.model.flow(z0.reshape(b * k, Z))
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
        if not (type(enc) is Encoder and type(dec) is Decoder and _stock_module(enc, 3) and _stock_module(dec, 2)
                and _flow_stock(m)):
            raise GMError("%s needs NFVAE's encoder, decoder and flow unchanged" % what)
        if images is None:
            images = self.test_iter.dataset.tensors[0]
        x = images.reshape(images.shape[0], -1)
        if not torch.cuda.is_available():
            raise GMError("%s runs on the MI355X only: no GPU is visible" % what)
        dev = enc.linear.weight.device
        if dev.type != "cuda":
            raise GMError("%s: the model is not on the GPU" % what)
        x = x.to(dev, torch.float32).contiguous()
        Z, K = enc.mu.weight.shape[0], m.flow.u.shape[0]
        if not (1 <= Z <= IWAE_MAX_Z and 1 <= K <= FLOW_MAX_K):
            raise GMError("%s supports 1 <= z_dim <= %d and 1 <= num_flows <= %d (got %d, %d)"
                          % (what, IWAE_MAX_Z, FLOW_MAX_K, Z, K))
        if enc.linear.weight.shape[1] != x.shape[1]:
            raise GMError("%s: images of %d pixels for a model of %d" % (what, x.shape[1], enc.linear.weight.shape[1]))
        return x, dev, Z

    def _encode(self, xb, He, mu_, lv_):
        from . import ops
        enc, b = self.model.encoder, xb.shape[0]
        w = lambda p: p.detach().contiguous()
        ops.linear_fwd(xb, w(enc.linear.weight), w(enc.linear.bias), He, "relu", M=b)
        ops.linear_fwd(He, w(enc.mu.weight), w(enc.mu.bias), mu_, "id", M=b)
        ops.linear_fwd(He, w(enc.log_var.weight), w(enc.log_var.bias), lv_, "id", M=b)
        return torch.cat([mu_[:b], lv_[:b]], 1)                            # [mu | lv], as the engine's packed layer

    def _flow_block(self):
        from . import ops_fused as of_
        fl = self.model.flow
        self._flow_keep = tuple(p.detach().contiguous() for p in (fl.u, fl.w, fl.b))   # alive while launches read them
        return of_.flow_params(*self._flow_keep)

    def log_likelihood(self, images=None, k=500, seed=0):
        """metrics.IWAEResult(ll_mean, ll_stderr, k, n) over `images` ([n, ...]; None: the whole test_iter's dataset):
        log p(x) ~= L_k(x) - (I / 2) log(pi) from k samples per image of the FLOW posterior.  iwae.log_likelihood's
        schedule: the encoder once per batch of LL_BATCH images (noise step = the batch's index, TAG_EVAL, row b * k + j
        over the whole k), the samples through gm_flow_sample, the decoder and gm_iwae_weights in chunks of at most 64,
        the chunks' (max, sum) combined in fp64.  The global generator, the model's mode and the parameters are
        untouched."""
        from . import ops
        from . import ops_fused as of_
        k, seed = check_k_seed(k, seed)
        x, dev, Z = self._eval_setup(images, "log_likelihood")
        enc, dec = self.model.encoder, self.model.decoder
        n, I = x.shape
        H, Hd = enc.linear.weight.shape[0], dec.linear.weight.shape[0]
        w = lambda p: p.detach().contiguous()
        nb, kc = min(LL_BATCH, n), min(LL_CHUNK, k)
        z_ = lambda *s: torch.empty(*s, device=dev)
        He, mu_, lv_, Zs, lp, Hdec, Xr = (z_(nb, H), z_(nb, Z), z_(nb, Z), z_(nb * kc, Z), z_(nb * kc), z_(nb * kc, Hd),
                                          z_(nb * kc, I))
        negL, ess, wn = z_(nb), z_(nb), z_(nb * kc)
        flow = self._flow_block()
        L = np.empty(n, dtype=np.float64)
        for step, lo in enumerate(range(0, n, nb)):
            b = min(nb, n - lo)
            xb = x[lo:lo + b]
            ml = self._encode(xb, He, mu_, lv_)
            parts = []
            for j0 in range(0, k, kc):
                c = min(kc, k - j0)
                ms = z_(b, 2)
                of_.flow_sample(ml, Zs, lp, of_.iwae_noise(seed, TAG_EVAL, k, j0=j0, step=step), flow, b, c, Z)
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
        density, log_q = -lp - 1/2 ||z_K||^2 - (Z / 2) log(2 pi) from gm_flow_sample's lp.  The noise is
        log_likelihood's (TAG_EVAL, step = the batch's index, row b * k + j)."""
        from . import ops_fused as of_
        k, seed = check_k_seed(k, seed)
        x, dev, Z = self._eval_setup(images, "posterior_samples")
        n = x.shape[0]
        H = self.model.encoder.linear.weight.shape[0]
        nb, kc = min(LL_BATCH, n), min(LL_CHUNK, k)
        z_ = lambda *s: torch.empty(*s, device=dev)
        He, mu_, lv_, Zs, lp = z_(nb, H), z_(nb, Z), z_(nb, Z), z_(nb * kc, Z), z_(nb * kc)
        flow = self._flow_block()
        zo, lq = torch.empty(n, k, Z), torch.empty(n, k, dtype=torch.float64)
        for step, lo in enumerate(range(0, n, nb)):
            b = min(nb, n - lo)
            ml = self._encode(x[lo:lo + b], He, mu_, lv_)
            for j0 in range(0, k, kc):
                c = min(kc, k - j0)
                of_.flow_sample(ml, Zs, lp, of_.iwae_noise(seed, TAG_EVAL, k, j0=j0, step=step), flow, b, c, Z)
                zc = Zs[:b * c].view(b, c, Z).cpu()
                zo[lo:lo + b, j0:j0 + c] = zc
                lq[lo:lo + b, j0:j0 + c] = (-lp[:b * c].view(b, c).cpu().double() - 0.5 * (zc.double() ** 2).sum(-1)
                                            - 0.5 * Z * math.log(2 * math.pi))
        return zo, lq


__all__ = ["Encoder", "Decoder", "NFVAE", "NFVAETrainer", "NFVAEError", "PlanarFlow", "planar_chain", "flow_constants",
           "FlatAdam"]
