"""Vector-quantised VAE (van den Oord, Vinyals & Kavukcuoglu, "Neural Discrete Representation Learning", arXiv
1711.00937): N latent variables, each one of K codebook vectors of D floats, between an MLP encoder and vae.py's decoder,
with a MADE over the codes' bits as the second-stage prior.  Exported by src/vq_vae.py as Encoder / Decoder / VQVAE /
VQVAETrainer / VQVAEError / code_bits / bits_code.

Model.  VQVAE(image_size=784, hidden_dim=400, num_vars=16, code_dim=16, num_codes=128): `encoder` has `linear` (I -> H,
relu) and `embed` (H -> N D); `codebook` is nn.Embedding(K, D), initialised uniform in (-1/K, 1/K); `decoder` is vae.py's
Decoder unchanged with z_dim = N D (state_dict keys encoder.linear.*, encoder.embed.*, codebook.weight,
decoder.linear.*, decoder.recon.*).  num_vars < 1, code_dim < 1 or num_codes < 2 raises VQVAEError(GMError, ValueError).
Fused path: 4 <= D <= 64 with D % 4 == 0, N D <= 1024, 2 <= K <= 1024, K D <= 16384 (vae_engine.VQVAEEngine; DESIGN.md
section 28); outside the limits the general path runs.

Forward.  For each image and each variable n, with z_e,n slice n of the `embed` output and E the codebook:

    c_n  = argmin_k sum_d (z_e,n,d - E_k,d)^2      the lowest index winning a tie; 0 when no distance compares less (NaN)
    z_q  = E[c]                                    the decoder's input
    qerr = sum_n ||z_e,n - E_c_n||^2               from the direct differences against the winner

An out-of-range code is never written.

Loss.  The package's likelihood convention: log w = -||x - decoder(z_q)||^2 + lp with lp = -(1 + beta) qerr; the loss of a
batch is sum_b -log w.  beta is the commitment cost (default 0.25): finite and >= 0, else VQVAEError.  In the paper's terms
qerr is both the codebook loss ||sg[z_e] - e||^2 and the commitment loss ||z_e - sg[e]||^2, the second weighted by beta.

Backward: the closed form of that loss under the straight-through estimator.

    d loss / d z_e = dzdec + 2 beta wn (z_e - E_c)       dzdec the decoder's input gradient, passed straight through;
                                                          wn = 1 at k = 1
    d loss / d E_k = 2 (n_k E_k - s_k)                    n_k the (image, variable) pairs of the batch assigned to k,
                                                          s_k the sum of their z_e: the codebook term only -- the
                                                          decoder's gradient does not reach the codebook

The codebook is an ordinary parameter of the one flat Adam, with weight decay like every other parameter.  EMA codebook
updates and dead-code restarts are not implemented; n_k and s_k are what an EMA update would need.

Noise.  Nothing is drawn in training, validation or evaluation; the global CPU generator is untouched by them.
(Constructing a model or fitting a prior initialises weights and shuffles data through it, as everywhere.)

General path (an overridden compute_batch or evaluate, an edited model, sizes outside the limits): autograd over
ops.fused_linear, the quantisation in torch as z_e + (z_q - z_e).detach() plus the two stop-gradient terms
||sg[z_e] - E_c||^2 + beta ||z_e - sg[E_c]||^2.

Prior.  fit_prior() writes every code as L = log2 K bits, most significant first, variable n in bits n L .. n L + L - 1
(code_bits / bits_code), and trains a MADE(image_size = N L) on them; K must be a power of two, so every bit pattern is a
valid code.  sample() then decodes codes drawn from the MADE (without a prior: uniform codes), and log_likelihood()
reports the lower bound -||x - decoder(E[c(x)])||^2 - (I / 2) log(pi) + log p_MADE(bits(c(x))): a bound because the
posterior is a point mass at c(x).

iwae.log_likelihood refuses this model (its encoder is not vae.py's); VQVAETrainer.log_likelihood is its evaluator."""
import math

import numpy as np
import torch
import torch.nn as nn

from ._lib import MADE_MAX_I, MADE_MIN_I, GMError
from .iwae import IWAETrainer
from .metrics import VQResult
from .trainers import Decoder, FlatAdam, _decode_rows, _lin, _stock_module, stock, stock_model, to_cuda  # noqa: F401

ROWS = 1024                      # images per launch group of codes / reconstruct / log_likelihood


class VQVAEError(GMError, ValueError):
    """A bad num_vars, code_dim, num_codes, beta or prior setting: a ValueError, and a GMError like the package's other
    refusals."""


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_beta(beta):
    """beta as a float; VQVAEError unless it is a finite number >= 0."""
    try:
        beta = float(beta)
    except (TypeError, ValueError):
        raise VQVAEError("beta (the commitment cost) must be a number") from None
    if not math.isfinite(beta) or beta < 0.0:
        raise VQVAEError("beta (the commitment cost) must be finite and >= 0, got %r" % beta)
    return beta


def _code_length(K):
    if not _is_int(K) or K < 2 or K & (K - 1):
        raise VQVAEError("num_codes must be a power of two >= 2 to be written as bits, got %r" % (K,))
    return int(K).bit_length() - 1


def code_bits(codes, num_codes):
    """codes [n, N] (integers in [0, K)) as bits [n, N L] float32, L = log2 K: variable n in bits n L .. n L + L - 1, most
    significant first."""
    L = _code_length(num_codes)
    c = torch.as_tensor(codes)
    if c.dim() != 2 or c.dtype == torch.bool or c.is_floating_point() or c.is_complex():
        raise VQVAEError("codes must be an integer tensor [n, N]")
    c = c.cpu().long()
    if c.numel() and (int(c.min()) < 0 or int(c.max()) >= num_codes):
        raise VQVAEError("codes must lie in [0, %d)" % num_codes)
    shifts = torch.arange(L - 1, -1, -1, dtype=torch.int64)
    return ((c[:, :, None] >> shifts) & 1).to(torch.float32).reshape(c.shape[0], c.shape[1] * L)


def bits_code(bits, num_codes):
    """The inverse of code_bits: bits [n, N L] of zeros and ones (any dtype) -> codes [n, N] int64."""
    L = _code_length(num_codes)
    b = torch.as_tensor(bits).cpu()
    if b.dim() != 2 or b.shape[1] % L:
        raise VQVAEError("bits must be [n, N * %d], got %s" % (L, tuple(b.shape)))
    if b.numel() and not bool(((b == 0) | (b == 1)).all()):
        raise VQVAEError("bits must be zeros and ones")
    w = 1 << torch.arange(L - 1, -1, -1, dtype=torch.int64)
    return (b.to(torch.int64).view(b.shape[0], -1, L) * w).sum(-1)


@stock_model
class Encoder(nn.Module):
    """x -> relu(linear) -> embed [., N D]."""

    def __init__(self, image_size, hidden_dim, num_vars, code_dim):
        super().__init__()
        self.linear = nn.Linear(image_size, hidden_dim)
        self.embed = nn.Linear(hidden_dim, num_vars * code_dim)

    def forward(self, x):
        return _lin(self.embed, _lin(self.linear, x, "relu"), "id")


def nearest_codes(z_e, E, num_vars):
    """argmin_k ||z_e,n - E_k||^2 per row and variable [rows, N] int64 (torch; the direct squared differences)."""
    z = z_e.detach().view(z_e.shape[0], num_vars, 1, -1)
    return ((z - E.detach()[None, None]) ** 2).sum(-1).argmin(-1)


def quantise_st(z_e, E, num_vars):
    """The contract's quantisation in torch (differentiable): (the decoder's input z_e + (z_q - z_e).detach() [rows, N D],
    codes [rows, N], the codebook term ||sg[z_e] - E_c||^2 and the commitment term ||z_e - sg[E_c]||^2, each [rows])."""
    rows = z_e.shape[0]
    codes = nearest_codes(z_e, E, num_vars)
    z_q = E[codes].reshape(rows, -1)
    cb = ((z_e.detach() - z_q) ** 2).sum(1)
    cm = ((z_e - z_q.detach()) ** 2).sum(1)
    return z_e + (z_q - z_e).detach(), codes, cb, cm


@stock_model
class VQVAE(nn.Module):
    """Encoder (linear, embed), the codebook and vae.py's Decoder on z_dim = N D; forward returns (reconstruction, z_e,
    codes) through the straight-through quantisation."""

    def __init__(self, image_size=784, hidden_dim=400, num_vars=16, code_dim=16, num_codes=128):
        if not _is_int(num_vars) or num_vars < 1:
            raise VQVAEError("num_vars must be an integer >= 1, got %r" % (num_vars,))
        if not _is_int(code_dim) or code_dim < 1:
            raise VQVAEError("code_dim must be an integer >= 1, got %r" % (code_dim,))
        if not _is_int(num_codes) or num_codes < 2:
            raise VQVAEError("num_codes must be an integer >= 2, got %r" % (num_codes,))
        super().__init__()
        self.image_size, self.hidden_dim = image_size, hidden_dim
        self.num_vars, self.code_dim, self.num_codes = int(num_vars), int(code_dim), int(num_codes)
        self.z_dim = self.num_vars * self.code_dim
        self.encoder = Encoder(image_size, hidden_dim, self.num_vars, self.code_dim)
        self.codebook = nn.Embedding(self.num_codes, self.code_dim)
        with torch.no_grad():
            self.codebook.weight.uniform_(-1.0 / self.num_codes, 1.0 / self.num_codes)
        self.decoder = Decoder(z_dim=self.z_dim, hidden_dim=hidden_dim, image_size=image_size)
        self.shape = int(image_size ** 0.5)

    def forward(self, x):
        z_e = self.encoder(x)
        z, codes, _, _ = quantise_st(z_e, self.codebook.weight, self.num_vars)
        return self.decoder(z), z_e, codes


def _fused_sizes(N, D, K):
    from . import ops_fused as of_
    return of_.vq_fused_sizes(N, D, K)


@stock
class VQVAETrainer(IWAETrainer):
    """IWAETrainer's loop at k = 1 on the quantised posterior: histories `losses` (sum_b -log w per batch) and `vq_loss`
    (sum_b qerr per batch), the epoch line, best_val_loss / best_model, checkpoints (+ num_vars, code_dim, num_codes and
    beta in the config, checked under strict=True; the prior's weights, order and hidden width when one is fitted),
    codes / decode / reconstruct / code_usage, fit_prior, sample / parzen and log_likelihood.  One GPU only."""

    _series = (("losses", "recon"), ("vq_loss", "kl"))
    _history = ("prior_state",)
    _line = "Epoch[%d/%d], Loss: %.4f, VQ Loss: %.4f, Val Loss: %.4f"
    _one_gpu = "VQVAETrainer"

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, beta=0.25):
        self.beta = check_beta(beta)                     # before anything runs
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz, k=1, seed=0)
        del self.ess
        self.losses, self.vq_loss = [], []
        self.prior = None

    def _sizes(self):
        m = self.model
        return int(getattr(m, "num_vars", 0)), int(getattr(m, "code_dim", 0)), int(getattr(m, "num_codes", 0))

    def _model_stock(self):
        """True iff the model is VQVAE with this module's Encoder, a plain nn.Embedding and vae.py's Decoder unchanged, of
        its own sizes."""
        m = self.model
        enc, dec, cb = getattr(m, "encoder", None), getattr(m, "decoder", None), getattr(m, "codebook", None)
        if not (type(m).__dict__.get("_gm_stock_model", False) and type(enc) is Encoder and type(dec) is Decoder
                and type(cb) is nn.Embedding and _stock_module(enc, 2) and _stock_module(dec, 2)
                and len(list(m.children())) == 3):
            return False
        N, D, K = self._sizes()
        return (N >= 1 and D >= 1 and K >= 2 and tuple(cb.weight.shape) == (K, D) and cb.padding_idx is None
                and cb.max_norm is None and enc.embed.weight.shape[0] == N * D and dec.linear.weight.shape[1] == N * D
                and enc.embed.weight.shape[1] == enc.linear.weight.shape[0])

    def _stock(self):
        return (self._hooks_stock() and self._model_stock() and _fused_sizes(*self._sizes()) and self.k == 1
                and self._loader_ok(self.train_iter) and self._loader_ok(self.val_iter)
                and self.train_iter.batch_size == self.val_iter.batch_size)

    def _engine_class(self):
        from .engine import VQVAEEngine
        return VQVAEEngine

    def train(self, num_epochs, lr=1e-3, weight_decay=1e-5, quiet=False):
        """vae.py's train loop on the quantised bound; the codebook steps with every other parameter."""
        self.beta = check_beta(self.beta)
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    def compute_batch(self, batch):
        """(sum_b -log w, sum_b qerr) of a batch (general path: autograd over the fused linear kernels, the quantisation
        in torch with the straight-through estimator and the two stop-gradient terms)."""
        images, _ = batch
        x = to_cuda(images.view(images.shape[0], -1))
        if not x.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: no GPU is visible")
        if self.model.training:
            self.noise_steps += 1                        # training batches taken (nothing is drawn)
        z, _, cb, cm = quantise_st(self.model.encoder(x), self.model.codebook.weight, self._sizes()[0])
        loss = ((x - self.model.decoder(z)) ** 2).sum() + cb.sum() + self.beta * cm.sum()
        return loss, cb.sum().detach()

    def _viz_epoch(self, epoch):
        pass                                             # vae.py's sample plot draws z ~ N(0, I): not this model's prior

    def viz_loss(self):
        """The training loss (sum_b -log w per batch) over the epochs."""
        from . import viz
        viz.one_loss_curve(self, "-log w")

    # ---- codes, decoding, reconstruction ------------------------------------------------------------------------------
    def _rows(self, images, what):
        if not self._model_stock():
            raise GMError("%s needs VQVAE's encoder, codebook and decoder unchanged" % what)
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
        return x, dev

    def _quantise(self, x, dev, decode=False):
        """(codes [n, N] int64 on the CPU, the decoder's output [n, I] on the device or None) of device rows x: the
        encoder's two GEMMs and gm_vq_quantise per group of ROWS images (sizes outside the kernel's limits: the general
        path's torch quantisation).  No autograd, no mode change, no RNG use."""
        from . import ops
        from . import ops_fused as of_
        enc, dec, E = self.model.encoder, self.model.decoder, self.model.codebook.weight.detach().contiguous()
        N, D, K = self._sizes()
        n, H = x.shape[0], enc.linear.weight.shape[0]
        nb = min(ROWS, max(1, n))
        w = lambda p: p.detach().contiguous()
        z_ = lambda *s: torch.empty(*s, device=dev)
        He, Ze, Zq, qerr, lp = z_(nb, H), z_(nb, N * D), z_(nb, N * D), z_(nb), z_(nb)
        cd = torch.empty(nb, N, dtype=torch.int32, device=dev)
        codes, out = torch.empty(n, N, dtype=torch.int64), []
        torch.cuda.synchronize()
        for lo in range(0, n, nb):
            b = min(nb, n - lo)
            ops.linear_fwd(x[lo:lo + b], w(enc.linear.weight), w(enc.linear.bias), He, "relu", M=b)
            ops.linear_fwd(He, w(enc.embed.weight), w(enc.embed.bias), Ze, "id", M=b)
            if _fused_sizes(N, D, K):
                of_.vq_quantise(Ze, E, Zq, cd, qerr, lp, self.beta, b, N, D)
                codes[lo:lo + b] = cd[:b].cpu().long()
            else:
                c = nearest_codes(Ze[:b], E, N)
                Zq[:b] = E[c].reshape(b, N * D)
                codes[lo:lo + b] = c.cpu()
            if decode:
                out.append(_decode_rows(dec, Zq[:b]))
        return codes, (torch.cat(out) if out else (z_(0, dec.recon.weight.shape[0]) if decode else None))

    def codes(self, images):
        """The nearest code of every variable as [n, N] int64 on the CPU, computed by gm_vq_quantise."""
        x, dev = self._rows(images, "codes")
        return self._quantise(x, dev)[0]

    def reconstruct(self, images):
        """decoder(E[codes(images)]) as [n, image_size] on the device."""
        x, dev = self._rows(images, "reconstruct")
        return self._quantise(x, dev, decode=True)[1]

    def decode(self, codes):
        """Images [n, image_size] of codes [n, N] (integers in [0, K)) through the codebook and the decoder; bad codes
        raise ValueError.  No autograd, no mode change, no RNG use."""
        N, D, K = self._sizes()
        c = torch.as_tensor(codes)
        if c.dim() != 2 or c.shape[1] != N:
            raise ValueError("codes must be [n, %d], got %s" % (N, tuple(c.shape)))
        if c.dtype == torch.bool or c.is_floating_point() or c.is_complex():
            raise ValueError("codes must be integers (got %s)" % c.dtype)
        c = c.cpu().long()
        if c.numel() and (int(c.min()) < 0 or int(c.max()) >= K):
            raise ValueError("codes must lie in [0, %d): found %d .. %d" % (K, int(c.min()), int(c.max())))
        if c.shape[0] == 0:
            return torch.empty(0, self.model.decoder.recon.weight.shape[0])
        E = self.model.codebook.weight.detach()
        return _decode_rows(self.model.decoder, E[c.to(E.device)].reshape(c.shape[0], N * D))

    @staticmethod
    def _perplexity(counts):
        p = counts.double() / max(1, int(counts.sum()))
        p = p[p > 0]
        return float(torch.exp(-(p * p.log()).sum()))

    def code_usage(self, images=None):
        """(counts [K] int64 -- how often each code is chosen over the images' n N variables -- and the perplexity
        exp(-sum_k p_k log p_k) of p = counts / (n N)); images=None: the whole test_iter's dataset."""
        counts = torch.bincount(self.codes(images).reshape(-1), minlength=self._sizes()[2])
        return counts, self._perplexity(counts)

    def epoch_usage(self):
        """code_usage's pair over the last training epoch's batches, from the fused engine's running count."""
        if self._engine is None:
            raise GMError("epoch_usage needs a train() call on the fused engine")
        counts = self._engine.usage.cpu().long()
        return counts, self._perplexity(counts)

    # ---- the prior ------------------------------------------------------------------------------------------------------
    def _prior_shape(self):
        N, _, K = self._sizes()
        L = _code_length(K)
        if not MADE_MIN_I <= N * L <= MADE_MAX_I:
            raise VQVAEError("the codes' %d bits are outside MADE's range [%d, %d]" % (N * L, MADE_MIN_I, MADE_MAX_I))
        return N * L

    def fit_prior(self, num_epochs=5, hidden_dim=400, lr=1e-3, batch_size=512, order="natural"):
        """Fits the second stage: encodes the train / val / test images once, writes their codes as bits (code_bits) and
        trains MADE(image_size = N log2 K, hidden_dim, order) on them with MADETrainer, which is kept as self.prior and
        returned.  num_codes not a power of two, or N log2 K outside MADE's range, raises VQVAEError."""
        from .made import MADE, MADEError, MADETrainer
        I = self._prior_shape()
        K = self._sizes()[2]

        def loader(it):
            bits = code_bits(self.codes(it.dataset.tensors[0]), K)
            ds = torch.utils.data.TensorDataset(bits, torch.zeros(bits.shape[0], dtype=torch.int64))
            return torch.utils.data.DataLoader(ds, batch_size=int(batch_size), shuffle=True)
        try:
            prior = MADE(I, hidden_dim, order=order)
        except MADEError as e:
            raise VQVAEError("fit_prior: %s" % e) from None
        tr = MADETrainer(prior, loader(self.train_iter), loader(self.val_iter), loader(self.test_iter))
        tr.train(num_epochs, lr=lr, quiet=True)
        self.prior = tr
        return tr

    @property
    def prior_state(self):
        """What a checkpoint carries of the prior: None, or its sizes, order and weights."""
        if getattr(self, "prior", None) is None:
            return None
        m = self.prior.model
        return {"image_size": int(m.image_size), "hidden_dim": int(m.hidden_dim), "order": str(m.order),
                "order_seed": int(m.order_seed), "model": {k: v.detach().cpu() for k, v in m.state_dict().items()}}

    @prior_state.setter
    def prior_state(self, st):
        if st is None:
            self.prior = None
            return
        from .made import MADE, MADETrainer
        if int(st["image_size"]) != self._prior_shape():
            raise GMError("the checkpoint's prior is over %d bits, this model's codes have %d"
                          % (int(st["image_size"]), self._prior_shape()))
        m = MADE(int(st["image_size"]), int(st["hidden_dim"]), order=st["order"], order_seed=int(st["order_seed"]))
        m.load_state_dict(st["model"])
        ds = torch.utils.data.TensorDataset(torch.zeros(1, m.image_size), torch.zeros(1, dtype=torch.int64))
        dl = lambda: torch.utils.data.DataLoader(ds, batch_size=1, shuffle=True)
        self.prior = MADETrainer(m, dl(), dl(), dl())

    # ---- samples and likelihood -------------------------------------------------------------------------------------------
    def sample(self, n, seed=0):
        """n decoded samples [n, image_size].  With a prior: codes from self.prior.sample(n, seed) through bits_code;
        without one: uniform codes from torch.Generator().manual_seed(seed).  The global generator and the model's mode
        are untouched."""
        N, _, K = self._sizes()
        if self.prior is not None:
            return self.decode(bits_code(self.prior.sample(int(n), seed), K))
        gen = torch.Generator().manual_seed(int(seed))
        return self.decode(torch.randint(0, K, (int(n), N), generator=gen))

    def log_likelihood(self, images=None):
        """metrics.VQResult(ll_mean, ll_stderr, recon_mean, prior_mean, n) over `images` ([n, ...]; None: the whole
        test_iter's dataset): per image -||x - decoder(E[c(x)])||^2 - (I / 2) log(pi) + log p_MADE(bits(c(x))), a lower
        bound on log p(x) (the posterior is a point mass).  GMError when no prior is fitted."""
        if self.prior is None:
            raise GMError("log_likelihood needs a prior over the codes: call fit_prior() first")
        x, dev = self._rows(images, "log_likelihood")
        codes, xr = self._quantise(x, dev, decode=True)
        n, I = x.shape
        recon = -((x.double() - xr.double()) ** 2).sum(1).cpu() - 0.5 * I * math.log(math.pi)
        prior = self.prior.log_likelihood_rows(code_bits(codes, self._sizes()[2])).double()
        ll = recon + prior
        return VQResult(float(ll.mean()), float(ll.std(unbiased=False)) / math.sqrt(n), float(recon.mean()),
                        float(prior.mean()), n)


__all__ = ["Encoder", "Decoder", "VQVAE", "VQVAETrainer", "VQVAEError", "code_bits", "bits_code", "check_beta",
           "nearest_codes", "quantise_st", "FlatAdam"]
