"""Categorical VAE trained through the Gumbel-Softmax / Concrete relaxation (Jang, Gu & Poole, "Categorical
Reparameterization with Gumbel-Softmax", arXiv 1611.01144; Maddison, Mnih & Teh, "The Concrete Distribution", arXiv
1611.00712): N categorical latent variables of C classes between an MLP encoder and vae.py's decoder.  Exported by
src/cat_vae.py as Encoder / Decoder / CatVAE / CatVAETrainer.

Model.  CatVAE(image_size=784, hidden_dim=400, num_vars=20, num_classes=10): `encoder` has `linear` (I -> H, relu) and
`logits` (H -> N C); `decoder` is vae.py's Decoder unchanged with z_dim = N C (state_dict keys decoder.linear.*,
decoder.recon.* kept).  num_vars < 1 or num_classes < 2 raises CatVAEError(GMError, ValueError).
Fused path: 2 <= C <= 64, N C <= 1024, k <= 64 per launch (vae_engine.CatVAEEngine); outside the
limits the general path runs.

Noise.  iwae.py's counter layout unchanged -- seed, tag, step = *ctr + *base + step, noise row b * k_total + j0 + j --
under two tags no other model uses (0x43415454 training, 0x43415445 validation and evaluation).  Element e = n C + c of
a row is word e mod 4 of the row's Philox block e div 4, mapped as every uniform of the package to u in (0, 1)
(u = (2 (word >> 9) + 1) 2^-24, between 2^-24 and 1 - 2^-24); the Gumbel value is g = -log(-log(u)), finite for every
word.  The noise is never stored: the backward regenerates it.

Forward.  Per sample row, with l = logits [N, C] and temperature tau:

    a_nc = (l_nc + g_nc) / tau              y_n = softmax_c(a_n)          (relaxed)
    q_n  = softmax_c(l_n)                   KL_n = sum_c q_nc (log q_nc + log C)

  RELAXED  (training): the decoder's input is y, lp = -sum_n KL_n.
  ST       (training with hard=True, and every validation batch): the decoder's input is onehot(argmax_c (l_nc + g_nc)),
           the lowest index winning a tie, the arg max taken on the fp32 sum before the division; lp as RELAXED; the
           backward is the relaxed one (the straight-through estimator).
  DISCRETE (likelihood evaluation): the decoder's input is that one-hot z, lp = -N log C - sum_n log q_n,z_n, which is
           log p(z) - log q(z | x); the codes [rows, N] are written as int32.

Softmax and log q go through the max-subtracted log-sum-exp: q = 0 contributes 0, never NaN.

Loss.  The package's likelihood convention: log w = -||x - decoder(.)||^2 + lp.  Training uses k = 1 and the loss
sum_b -log w (gm_iwae_weights as it stands; at k = 1 it gives wn = 1).  Reported likelihood: L_k - (I / 2) log(pi), as
for the IWAE.

Backward: the closed form of the forward.  With dy = d loss / d (decoder input), which already carries wn:

    da_c = y_c (dy_c - sum_c' y_c' dy_c')
    dl_c = da_c / tau + q_c (log q_c - sum_c' q_c' log q_c')

In ST mode the same, with the relaxed y.  y in the backward has the forward's bits (one shared device function).

Temperature.  tau_t = max(tau_min, tau0 exp(-anneal_rate t)), t the global training-batch index (`noise_steps`, which
travels in checkpoints), computed in fp64 on the host and rounded to fp32 (`temperature`); the engine uploads the run's
values as a device table indexed like the Adam schedule.  tau_min <= 0, tau0 < tau_min or anneal_rate < 0 raises
CatVAEError.  Validation and evaluation read no temperature.

General path (an overridden compute_batch or evaluate, an edited model, sizes outside the limits): autograd over
ops.fused_linear, the relaxation in torch on ops_fused.catvae_gumbels (the same counter stream); ST mode there is
y_hard + (y - y.detach()).

iwae.log_likelihood refuses this model (its encoder is not vae.py's); CatVAETrainer.log_likelihood is the evaluator for
the discrete posterior."""
import math

import numpy as np
import torch
import torch.nn as nn

from ._lib import (CAT_DISCRETE, CAT_MAX_C, CAT_MAX_NC, CAT_MIN_C, CAT_TAG_EVAL, CAT_TAG_TRAIN, IWAE_MAX_K,
                   GMError)
from .iwae import LL_BATCH, LL_CHUNK, IWAETrainer, check_k_seed
from .metrics import IWAEResult
from .trainers import Decoder, FlatAdam, _decode_rows, _lin, _stock_module, stock, stock_model, to_cuda  # noqa: F401

TAG_TRAIN, TAG_EVAL = CAT_TAG_TRAIN, CAT_TAG_EVAL


class CatVAEError(GMError, ValueError):
    """A bad num_vars, num_classes or temperature setting: a ValueError, and a GMError like the package's other
    refusals."""


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_temperature(tau0, tau_min, anneal_rate):
    """(tau0, tau_min, anneal_rate) as floats; CatVAEError unless 0 < tau_min <= tau0 and anneal_rate >= 0 (all
    finite)."""
    try:
        tau0, tau_min, anneal_rate = float(tau0), float(tau_min), float(anneal_rate)
    except (TypeError, ValueError):
        raise CatVAEError("the temperature settings must be numbers") from None
    if not all(math.isfinite(v) for v in (tau0, tau_min, anneal_rate)):
        raise CatVAEError("the temperature settings must be finite")
    if tau_min <= 0.0:
        raise CatVAEError("tau_min must be > 0, got %r" % tau_min)
    if tau0 < tau_min:
        raise CatVAEError("tau0 (%r) must be >= tau_min (%r)" % (tau0, tau_min))
    if anneal_rate < 0.0:
        raise CatVAEError("anneal_rate must be >= 0, got %r" % anneal_rate)
    return tau0, tau_min, anneal_rate


def temperature(t, tau0=1.0, tau_min=0.5, anneal_rate=3e-5):
    """tau_t = max(tau_min, tau0 exp(-anneal_rate t)) of training batch t (0-based, over the trainer's life): computed
    in fp64 and rounded to fp32, returned as a Python float."""
    tau0, tau_min, anneal_rate = check_temperature(tau0, tau_min, anneal_rate)
    if not _is_int(t) or t < 0:
        raise CatVAEError("t (the training batch's index) must be an integer >= 0, got %r" % (t,))
    return float(np.float32(max(tau_min, tau0 * math.exp(-anneal_rate * int(t)))))


@stock_model
class Encoder(nn.Module):
    """x -> relu(linear) -> logits [., N C]."""

    def __init__(self, image_size, hidden_dim, num_vars, num_classes):
        super().__init__()
        self.linear = nn.Linear(image_size, hidden_dim)
        self.logits = nn.Linear(hidden_dim, num_vars * num_classes)

    def forward(self, x):
        return _lin(self.logits, _lin(self.linear, x, "relu"), "id")


def gumbel_softmax(logits, g, tau, num_vars, num_classes, hard=False):
    """The contract's decoder input from logits and Gumbel noise g [rows, N C] (torch; differentiable): the relaxed y,
    or with hard=True the straight-through y_hard + (y - y.detach())."""
    s = (logits + g).view(-1, num_vars, num_classes)
    y = torch.softmax(s / tau, -1)
    if hard:
        y = nn.functional.one_hot(s.argmax(-1), num_classes).to(y.dtype) + (y - y.detach())
    return y.reshape(-1, num_vars * num_classes)


def categorical_kl(logits, num_vars, num_classes):
    """sum_n KL(q_n || uniform) per row [rows] (torch; differentiable)."""
    lq = torch.log_softmax(logits.view(-1, num_vars, num_classes), -1)
    return (lq.exp() * (lq + math.log(num_classes))).sum((1, 2))


@stock_model
class CatVAE(nn.Module):
    """Encoder (linear, logits) and vae.py's Decoder on z_dim = N C; forward draws one relaxed sample at tau = 1 from
    the global CPU generator (as vae.VAE draws its eps) and returns (reconstruction, logits)."""

    def __init__(self, image_size=784, hidden_dim=400, num_vars=20, num_classes=10):
        if not _is_int(num_vars) or num_vars < 1:
            raise CatVAEError("num_vars must be an integer >= 1, got %r" % (num_vars,))
        if not _is_int(num_classes) or num_classes < 2:
            raise CatVAEError("num_classes must be an integer >= 2, got %r" % (num_classes,))
        super().__init__()
        self.image_size, self.hidden_dim = image_size, hidden_dim
        self.num_vars, self.num_classes = int(num_vars), int(num_classes)
        self.z_dim = self.num_vars * self.num_classes
        self.encoder = Encoder(image_size, hidden_dim, self.num_vars, self.num_classes)
        self.decoder = Decoder(z_dim=self.z_dim, hidden_dim=hidden_dim, image_size=image_size)
        self.shape = int(image_size ** 0.5)

    def forward(self, x):
        logits = self.encoder(x)
        u = torch.rand(logits.shape).clamp_(2.0 ** -24, 1.0 - 2.0 ** -24)
        g = to_cuda(-torch.log(-torch.log(u)))
        return self.decoder(gumbel_softmax(logits, g, 1.0, self.num_vars, self.num_classes)), logits


def _fused_sizes(N, C):
    return N >= 1 and CAT_MIN_C <= C <= CAT_MAX_C and N * C <= CAT_MAX_NC


@stock
class CatVAETrainer(IWAETrainer):
    """IWAETrainer's loop at k = 1 on the categorical posterior: histories `losses` and `kl_loss` (sums per batch), the
    epoch line, best_val_loss / best_model, checkpoints (+ num_vars, num_classes, seed, hard, the temperature settings and
    the training batches taken), sample / parzen from uniform one-hot codes, log_likelihood / posterior_codes under the
    discrete posterior, codes and decode.  One GPU only."""

    _series = (("losses", "recon"), ("kl_loss", "kl"))
    _line = "Epoch[%d/%d], Loss: %.4f, KL Div: %.4f, Val Loss: %.4f"
    _one_gpu = "CatVAETrainer"

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, seed=0, hard=False):
        if not isinstance(hard, (bool, np.bool_)):
            raise CatVAEError("hard must be a bool, got %r" % (hard,))
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz, k=1, seed=seed)
        self.hard = bool(hard)
        self.tau0, self.tau_min, self.anneal_rate = 1.0, 0.5, 3e-5
        self.losses, self.kl_loss = [], []

    def _sizes(self):
        m = self.model
        return int(getattr(m, "num_vars", 0)), int(getattr(m, "num_classes", 0))

    def _model_stock(self):
        """True iff the model is CatVAE with this module's Encoder and vae.py's Decoder unchanged, of its own sizes."""
        m = self.model
        enc, dec = getattr(m, "encoder", None), getattr(m, "decoder", None)
        if not (type(m).__dict__.get("_gm_stock_model", False) and type(enc) is Encoder and type(dec) is Decoder
                and _stock_module(enc, 2) and _stock_module(dec, 2)):
            return False
        N, C = self._sizes()
        return (N >= 1 and C >= 2 and enc.logits.weight.shape[0] == N * C and dec.linear.weight.shape[1] == N * C
                and enc.logits.weight.shape[1] == enc.linear.weight.shape[0])

    def _stock(self):
        return (self._hooks_stock() and self._model_stock() and _fused_sizes(*self._sizes()) and self.k == 1
                and self._loader_ok(self.train_iter) and self._loader_ok(self.val_iter)
                and self.train_iter.batch_size == self.val_iter.batch_size)

    def _engine_class(self):
        from .engine import CatVAEEngine
        return CatVAEEngine

    def train(self, num_epochs, lr=1e-3, weight_decay=1e-5, tau0=1.0, tau_min=0.5, anneal_rate=3e-5, quiet=False):
        """vae.py's train loop on the relaxed (hard=True: straight-through) bound; batch t of the trainer's life runs at
        temperature(t, tau0, tau_min, anneal_rate)."""
        self.tau0, self.tau_min, self.anneal_rate = check_temperature(tau0, tau_min, anneal_rate)
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    def compute_batch(self, batch):
        """(sum_b -log w, sum_b KL) of a batch (general path: autograd over the fused linear kernels, the relaxation in
        torch on the contract's counter stream -- the training stream and temperature while the model trains, the
        validation stream and the one-hot sample otherwise)."""
        from . import ops_fused as of_
        images, _ = batch
        x = to_cuda(images.view(images.shape[0], -1))
        if not x.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: no GPU is visible")
        b = x.shape[0]
        N, C = self._sizes()
        logits = self.model.encoder(x)
        if self.model.training:
            g = of_.catvae_gumbels(b, 1, N, C, self.seed, self.noise_steps, TAG_TRAIN, device=x.device)
            tau = temperature(self.noise_steps, self.tau0, self.tau_min, self.anneal_rate)
            self.noise_steps += 1
            z = gumbel_softmax(logits, g, tau, N, C, hard=self.hard)
        else:
            g = of_.catvae_gumbels(b, 1, N, C, self.seed, self._eval_step, TAG_EVAL, device=x.device)
            self._eval_step += 1
            z = nn.functional.one_hot((logits + g).view(b, N, C).argmax(-1), C).to(logits.dtype).reshape(b, N * C)
        kl = categorical_kl(logits, N, C).sum()
        loss = ((x - self.model.decoder(z)) ** 2).sum() + kl
        return loss, kl.detach()

    def _viz_epoch(self, epoch):
        pass                                         # vae.py's sample plot draws z ~ N(0, I): not this model's prior

    def viz_loss(self):
        """The training loss (sum_b -log w per batch) over the epochs."""
        from . import viz
        viz.one_loss_curve(self, "-log w")

    # ---- codes, samples ------------------------------------------------------------------------------------------------
    def decode(self, codes):
        """Images [n, image_size] of codes [n, N] (integers in [0, C)) through the decoder; bad codes raise
        ValueError.  No autograd, no mode change, no RNG use."""
        N, C = self._sizes()
        c = torch.as_tensor(codes)
        if c.dim() != 2 or c.shape[1] != N:
            raise ValueError("codes must be [n, %d], got %s" % (N, tuple(c.shape)))
        if c.dtype == torch.bool or c.is_floating_point() or c.is_complex():
            raise ValueError("codes must be integers (got %s)" % c.dtype)
        c = c.cpu().long()
        if c.numel() and (int(c.min()) < 0 or int(c.max()) >= C):
            raise ValueError("codes must lie in [0, %d): found %d .. %d" % (C, int(c.min()), int(c.max())))
        z = nn.functional.one_hot(c, C).to(torch.float32).reshape(c.shape[0], N * C)
        if c.shape[0] == 0:
            return torch.empty(0, self.model.decoder.recon.weight.shape[0])
        return _decode_rows(self.model.decoder, z)

    def sample(self, n, seed=0):
        """n decoded samples [n, image_size]: uniform codes from torch.Generator().manual_seed(seed) through the
        decoder; the global generator and the model's mode are untouched."""
        N, C = self._sizes()
        gen = torch.Generator().manual_seed(int(seed))
        return self.decode(torch.randint(0, C, (int(n), N), generator=gen))

    # ---- evaluation under the discrete posterior ----------------------------------------------------------------------
    def _eval_setup(self, images, what):
        if not self._model_stock():
            raise GMError("%s needs CatVAE's encoder and decoder unchanged" % what)
        N, C = self._sizes()
        if not _fused_sizes(N, C):
            raise GMError("%s supports %d <= num_classes <= %d and num_vars * num_classes <= %d (got %d, %d)"
                          % (what, CAT_MIN_C, CAT_MAX_C, CAT_MAX_NC, N, C))
        if images is None:
            images = self.test_iter.dataset.tensors[0]
        x = images.reshape(images.shape[0], -1)
        if not torch.cuda.is_available():
            raise GMError("%s runs on the MI355X only: no GPU is visible" % what)
        enc = self.model.encoder
        dev = enc.linear.weight.device
        if dev.type != "cuda":
            raise GMError("%s: the model is not on the GPU" % what)
        x = x.to(dev, torch.float32).contiguous()
        if enc.linear.weight.shape[1] != x.shape[1]:
            raise GMError("%s: images of %d pixels for a model of %d" % (what, x.shape[1], enc.linear.weight.shape[1]))
        return x, dev, N, C

    def _encode(self, xb, He, Lg):
        from . import ops
        enc, b = self.model.encoder, xb.shape[0]
        w = lambda p: p.detach().contiguous()
        ops.linear_fwd(xb, w(enc.linear.weight), w(enc.linear.bias), He, "relu", M=b)
        ops.linear_fwd(He, w(enc.logits.weight), w(enc.logits.bias), Lg, "id", M=b)
        return Lg

    def codes(self, images):
        """argmax_c l as [n, N] int64 on the CPU: the posterior's mode, variable by variable (no noise)."""
        x, dev, N, C = self._eval_setup(images, "codes")
        n, H = x.shape[0], self.model.encoder.linear.weight.shape[0]
        nb = min(LL_BATCH, max(1, n))
        He, Lg = torch.empty(nb, H, device=dev), torch.empty(nb, N * C, device=dev)
        out = torch.empty(n, N, dtype=torch.int64)
        for lo in range(0, n, nb):
            b = min(nb, n - lo)
            self._encode(x[lo:lo + b], He, Lg)
            out[lo:lo + b] = Lg[:b].view(b, N, C).argmax(-1).cpu()
        return out

    def log_likelihood(self, images=None, k=500, seed=0):
        """metrics.IWAEResult(ll_mean, ll_stderr, k, n) over `images` ([n, ...]; None: the whole test_iter's dataset):
        log p(x) ~= L_k(x) - (I / 2) log(pi) from k codes per image drawn from q(z | x), importance weights
        log w = -||x - decoder(onehot z)||^2 + log p(z) - log q(z | x).  iwae.log_likelihood's schedule: the encoder once
        per batch of LL_BATCH images (noise step = the batch's index, the evaluation tag, row b * k + j over the whole
        k), the samples through gm_cat_sample (DISCRETE), the decoder and gm_iwae_weights in chunks of at most 64, the
        chunks' (max, sum) combined in fp64.  The global generator, the model's mode and the parameters are
        untouched."""
        from . import ops
        from . import ops_fused as of_
        k, seed = check_k_seed(k, seed)
        x, dev, N, C = self._eval_setup(images, "log_likelihood")
        enc, dec = self.model.encoder, self.model.decoder
        n, I = x.shape
        H, Hd, W = enc.linear.weight.shape[0], dec.linear.weight.shape[0], N * C
        w = lambda p: p.detach().contiguous()
        nb, kc = min(LL_BATCH, n), min(LL_CHUNK, k)
        z_ = lambda *s: torch.empty(*s, device=dev)
        He, Lg, Zs, lp, Hdec, Xr = z_(nb, H), z_(nb, W), z_(nb * kc, W), z_(nb * kc), z_(nb * kc, Hd), z_(nb * kc, I)
        negL, ess, wn = z_(nb), z_(nb), z_(nb * kc)
        codes = torch.empty(nb * kc, N, dtype=torch.int32, device=dev)
        L = np.empty(n, dtype=np.float64)
        for step, lo in enumerate(range(0, n, nb)):
            b = min(nb, n - lo)
            xb = x[lo:lo + b]
            self._encode(xb, He, Lg)
            parts = []
            for j0 in range(0, k, kc):
                c = min(kc, k - j0)
                ms = z_(b, 2)
                of_.cat_sample(Lg, Zs, lp, of_.iwae_noise(seed, TAG_EVAL, k, j0=j0, step=step), b, c, N, C, CAT_DISCRETE,
                               codes=codes)
                ops.linear_fwd(Zs, w(dec.linear.weight), w(dec.linear.bias), Hdec, "relu", M=b * c)
                ops.linear_fwd(Hdec, w(dec.recon.weight), w(dec.recon.bias), Xr, "sigmoid", M=b * c)
                of_.iwae_weights(xb, Xr, lp, negL, ess, wn, b, c, ms=ms)
                parts.append(ms)
            ms = torch.stack(parts).cpu().numpy().astype(np.float64)           # [chunks, b, 2]: one sync per batch
            mx = ms[..., 0].max(0)
            L[lo:lo + b] = mx + np.log((ms[..., 1] * np.exp(ms[..., 0] - mx)).sum(0)) - math.log(k)
        ll = L - 0.5 * I * math.log(math.pi)
        return IWAEResult(float(ll.mean()), float(ll.std()) / math.sqrt(n), k, n)

    def posterior_codes(self, images, k, seed=0):
        """(codes [n, k, N] int64, log_q [n, k] float64) on the CPU: k draws per image from q(z | x) and their log
        probability sum_n log q_n,z_n, from gm_cat_sample's lp (= -N log C - log q).  The noise is log_likelihood's (the
        evaluation tag, step = the batch's index, row b * k + j)."""
        from . import ops_fused as of_
        k, seed = check_k_seed(k, seed)
        x, dev, N, C = self._eval_setup(images, "posterior_codes")
        n, H, W = x.shape[0], self.model.encoder.linear.weight.shape[0], N * C
        nb, kc = min(LL_BATCH, n), min(LL_CHUNK, k)
        z_ = lambda *s: torch.empty(*s, device=dev)
        He, Lg, Zs, lp = z_(nb, H), z_(nb, W), z_(nb * kc, W), z_(nb * kc)
        cd = torch.empty(nb * kc, N, dtype=torch.int32, device=dev)
        out, lq = torch.empty(n, k, N, dtype=torch.int64), torch.empty(n, k, dtype=torch.float64)
        for step, lo in enumerate(range(0, n, nb)):
            b = min(nb, n - lo)
            self._encode(x[lo:lo + b], He, Lg)
            for j0 in range(0, k, kc):
                c = min(kc, k - j0)
                of_.cat_sample(Lg, Zs, lp, of_.iwae_noise(seed, TAG_EVAL, k, j0=j0, step=step), b, c, N, C, CAT_DISCRETE,
                               codes=cd)
                out[lo:lo + b, j0:j0 + c] = cd[:b * c].view(b, c, N).cpu().long()
                lq[lo:lo + b, j0:j0 + c] = -lp[:b * c].view(b, c).cpu().double() - N * math.log(C)
        return out, lq


assert LL_CHUNK <= IWAE_MAX_K

__all__ = ["Encoder", "Decoder", "CatVAE", "CatVAETrainer", "CatVAEError", "temperature", "check_temperature",
           "gumbel_softmax", "categorical_kl", "FlatAdam"]
