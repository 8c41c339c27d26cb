"""Importance-weighted autoencoder (Burda, Grosse & Salakhutdinov, "Importance Weighted Autoencoders", arXiv
1509.00519): vae.py's Encoder, Decoder and VAE, state_dict keys unchanged (a VAE checkpoint's weights load into an
IWAE), trained on the k-sample bound.  Exported by src/iwae.py as Encoder / Decoder / IWAE / IWAETrainer.

The contract.  For image x_b and sample j < k, with [mu | lv] = encoder(x_b):

    eps_j ~ N(0, I_Z)         z_j = mu + eps_j * exp(lv / 2)        xr_j = decoder(z_j)
    log w_j = -||x_b - xr_j||^2 - 1/2 ||z_j||^2 + 1/2 ||eps_j||^2 + 1/2 sum_c lv_c
    L_k(x_b) = logsumexp_j(log w_j) - log k            loss = sum_b -L_k(x_b)

Relation to vae.py: the reconstruction term is vae.py's summed squared error, that is, a Gaussian decoder with variance
1/2; the (2 pi)^(Z/2) factors of prior and posterior cancel.  At k = 1 the loss is the VAE's recon + KL with the KL
estimated from the sample instead of in closed form.

Gradients, with wn = softmax_j(log w_j):  d loss / d log w_j = -wn_j;
    dA_j (pre-sigmoid output) = wn_j * (-2 (x - xr_j) (1 - xr_j) xr_j);      dz_j = wn_j z_j + (dHdec_j Wd1);
    dmu = sum_j dz_j;                     dlv_c = sum_j dz_jc eps_jc exp(lv_c / 2) / 2 - 1/2.
Diagnostic: ess_b = 1 / sum_j wn_j^2 (1 at k = 1, at most k).
Reported likelihood: log p(x_b) ~= L_k(x_b) - (I / 2) log(pi), the second term the Gaussian decoder's normaliser.

Noise: drawn on the device, never from the CPU generator (as the DVAE's).  Philox4x32-10 with key (seed mod 2^32,
seed >> 32) and counter (c >> 2, step, row, TAG) gives word c & 3 to latent c of sample row `row` = b * k + j (b the
batch position: rows are image-major, an image's k samples adjacent); the Box-Muller mapping is gm_philox_normal's.
TAG = 0x49574145 for training, `step` the 0-based training batch count over the trainer's life (`noise_steps`, saved in
checkpoints); TAG = 0x49574556 for validation and log_likelihood, `step` the batch index within the call, with the
caller's seed.  eps is never stored: the backward regenerates it from the counter.

`iwae_noise_reference` / `iwae_reference` below are the same rule in numpy and fp64 (the tests' oracle), built on
dvae.philox4x32_10 and dvae.box_muller_normals.

Fused path: vae_engine.IWAEEngine (1 <= k <= 64, 1 <= Z <= 32).  An overridden compute_batch or
evaluate, an edited model, k > 64 or Z > 32: the general loop below -- autograd over ops.fused_linear, eps from
ops_fused.iwae_normals (the same counter stream), the log-sum-exp in torch."""
import math

import numpy as np
import torch

from . import _lib, philox
from ._lib import IWAE_MAX_K, IWAE_MAX_Z, IWAE_TAG_EVAL, IWAE_TAG_TRAIN, GMError
from .metrics import IWAEResult
from .trainers import VAE, Decoder, Encoder, FlatAdam, VAETrainer, _stock_module, stock, stock_model, to_cuda  # noqa: F401

TAG_TRAIN, TAG_EVAL = IWAE_TAG_TRAIN, IWAE_TAG_EVAL
LL_CHUNK = IWAE_MAX_K            # samples per launch group of log_likelihood
LL_BATCH = 256                   # images per batch of log_likelihood (its noise step is the batch's index)


class IWAEError(GMError, ValueError):
    """A bad k or seed: a ValueError, and a GMError like the package's other refusals."""


def check_k_seed(k, seed):
    """(k, seed) validated: an integer k >= 1 and an integer seed in [0, 2^64); else IWAEError."""
    k, seed = _lib.check_int(k, "k", IWAEError), _lib.check_int(seed, "seed", IWAEError)
    if k < 1:
        raise IWAEError("k (samples per image) must be >= 1, got %d" % k)
    return k, _lib.check_seed(seed, error=IWAEError)


# ---- the rule in numpy and fp64 (the tests' reference; also a CPU reading of what the device computes) ---------------
def iwae_noise_reference(n_rows, Z, seed, step, tag):
    """eps [n_rows, Z] float64: the normals of sample rows 0 .. n_rows - 1 at `step` under `tag`."""
    return philox.normals(n_rows, Z, seed, step, tag)


def iwae_reference(params, x, eps, k):
    """The contract in numpy, fp64.  params: the model's state_dict (10 names: the eight tensors of the engine, the
    packed [mu ; log_var] layer under its two halves' names); x [B, I]; eps [B k, Z] image-major.  Returns a dict:
    L [B] (= L_k), ess [B], grads (d sum_b -L_k / d every tensor, by state_dict name), and the intermediates the kernel
    tests compare: logw, wn [B, k], z [B k, Z], lp [B k], dA [B k, I], dzdec [B k, Z], dml [B, 2Z]."""
    P = {n: np.asarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v, dtype=np.float64)
         for n, v in params.items()}
    x = np.asarray(x, dtype=np.float64)
    B, I = x.shape
    eps = np.asarray(eps, dtype=np.float64).reshape(B, k, -1)
    Z = eps.shape[2]
    W1, b1 = P["encoder.linear.weight"], P["encoder.linear.bias"]
    Wm, bm, Wl, bl = P["encoder.mu.weight"], P["encoder.mu.bias"], P["encoder.log_var.weight"], P["encoder.log_var.bias"]
    Wd1, bd1, Wd2, bd2 = (P["decoder.linear.weight"], P["decoder.linear.bias"], P["decoder.recon.weight"],
                          P["decoder.recon.bias"])
    h = np.maximum(x @ W1.T + b1, 0.0)
    mu, lv = h @ Wm.T + bm, h @ Wl.T + bl
    sd = np.exp(lv / 2)
    z = mu[:, None, :] + eps * sd[:, None, :]
    hd = np.maximum(z @ Wd1.T + bd1, 0.0)
    xr = 1.0 / (1.0 + np.exp(-(hd @ Wd2.T + bd2)))
    d = x[:, None, :] - xr
    lp = 0.5 * ((eps ** 2).sum(-1) - (z ** 2).sum(-1) + lv.sum(-1)[:, None])
    logw = lp - (d ** 2).sum(-1)
    m = logw.max(1, keepdims=True)
    e = np.exp(logw - m)
    s = e.sum(1, keepdims=True)
    wn = e / s
    L = (m + np.log(s))[:, 0] - math.log(k)
    ess = 1.0 / (wn ** 2).sum(1)
    # backward of sum_b -L_k
    dA = wn[..., None] * (-2.0 * d * (1.0 - xr) * xr)
    dA2, hd2, z2 = dA.reshape(B * k, I), hd.reshape(B * k, -1), z.reshape(B * k, Z)
    dhd = (dA2 @ Wd2) * (hd2 > 0)
    dzdec = dhd @ Wd1
    dz = dzdec.reshape(B, k, Z) + wn[..., None] * z
    dmu = dz.sum(1)
    dlv = (dz * eps * sd[:, None, :]).sum(1) / 2 - 0.5
    dh = (dmu @ Wm + dlv @ Wl) * (h > 0)
    grads = {"encoder.linear.weight": dh.T @ x, "encoder.linear.bias": dh.sum(0),
             "encoder.mu.weight": dmu.T @ h, "encoder.mu.bias": dmu.sum(0),
             "encoder.log_var.weight": dlv.T @ h, "encoder.log_var.bias": dlv.sum(0),
             "decoder.linear.weight": dhd.T @ z2, "decoder.linear.bias": dhd.sum(0),
             "decoder.recon.weight": dA2.T @ hd2, "decoder.recon.bias": dA2.sum(0)}
    return {"L": L, "ess": ess, "grads": grads, "logw": logw, "wn": wn, "z": z2, "lp": lp.reshape(-1), "dA": dA2,
            "dzdec": dzdec, "dml": np.concatenate([dmu, dlv], axis=1), "ml": np.concatenate([mu, lv], axis=1),
            "xr": xr.reshape(B * k, I)}


# ---- log p(x) by importance sampling, for every trainer whose model is vae.py's Encoder and Decoder ------------------
def log_likelihood(trainer, images=None, k=500, seed=0):
    """VAETrainer.log_likelihood: metrics.IWAEResult(ll_mean, ll_stderr, k, n) over `images` ([n, ...]; None: the whole
    test_iter's dataset), log p(x) ~= L_k(x) - (I / 2) log(pi) from k samples per image.  The encoder runs once per
    batch of LL_BATCH images (noise step = the batch's index, TAG_EVAL, row b * k + j over the whole k), the samples go
    through the decoder and gm_iwae_weights in chunks of at most 64, and the chunks' (max, sum) are combined in fp64.
    The global generator, the model's mode and the parameters are untouched."""
    from . import ops
    from . import ops_fused as of_
    k, seed = check_k_seed(k, seed)
    m = trainer.model
    enc, dec = getattr(m, "encoder", None), getattr(m, "decoder", None)
    if not (type(enc) is Encoder and type(dec) is Decoder and _stock_module(enc, 3) and _stock_module(dec, 2)):
        raise GMError("log_likelihood needs vae.py's Encoder and Decoder unchanged (%s's encoder is deterministic, "
                      "label-fed or edited)" % type(trainer).__name__)
    if images is None:
        images = trainer.test_iter.dataset.tensors[0]
    x = images.reshape(images.shape[0], -1)
    if not torch.cuda.is_available():
        raise GMError("log_likelihood runs on the MI355X only: no GPU is visible")
    dev = enc.linear.weight.device
    if dev.type != "cuda":
        raise GMError("log_likelihood: the model is not on the GPU")
    x = x.to(dev, torch.float32).contiguous()
    n, I = x.shape
    Z = enc.mu.weight.shape[0]
    if not 1 <= Z <= IWAE_MAX_Z:
        raise GMError("log_likelihood supports 1 <= z_dim <= %d (got %d)" % (IWAE_MAX_Z, Z))
    if enc.linear.weight.shape[1] != I:
        raise GMError("log_likelihood: images of %d pixels for a model of %d" % (I, enc.linear.weight.shape[1]))
    H, Hd = enc.linear.weight.shape[0], dec.linear.weight.shape[0]
    w = lambda p: p.detach().contiguous()
    nb, kc = min(LL_BATCH, n), min(LL_CHUNK, k)
    z_ = lambda *s: torch.empty(*s, device=dev)
    He, mu_, lv_, Zs, lp, Hdec, Xr = (z_(nb, H), z_(nb, Z), z_(nb, Z), z_(nb * kc, Z), z_(nb * kc), z_(nb * kc, Hd),
                                      z_(nb * kc, I))
    negL, ess, wn = z_(nb), z_(nb), z_(nb * kc)
    L = np.empty(n, dtype=np.float64)
    for step, lo in enumerate(range(0, n, nb)):
        b = min(nb, n - lo)
        xb = x[lo:lo + b]
        ops.linear_fwd(xb, w(enc.linear.weight), w(enc.linear.bias), He, "relu", M=b)
        ops.linear_fwd(He, w(enc.mu.weight), w(enc.mu.bias), mu_, "id", M=b)
        ops.linear_fwd(He, w(enc.log_var.weight), w(enc.log_var.bias), lv_, "id", M=b)
        ml = torch.cat([mu_[:b], lv_[:b]], 1)                              # [mu | lv], as the engine's packed layer
        parts = []
        for j0 in range(0, k, kc):
            c = min(kc, k - j0)
            ms = z_(b, 2)
            of_.iwae_sample(ml, Zs, lp, of_.iwae_noise(seed, TAG_EVAL, k, j0=j0, step=step), b, c, Z)
            ops.linear_fwd(Zs, w(dec.linear.weight), w(dec.linear.bias), Hdec, "relu", M=b * c)
            ops.linear_fwd(Hdec, w(dec.recon.weight), w(dec.recon.bias), Xr, "sigmoid", M=b * c)
            of_.iwae_weights(xb, Xr, lp, negL, ess, wn, b, c, ms=ms)
            parts.append(ms)
        ms = torch.stack(parts).cpu().numpy().astype(np.float64)           # [chunks, b, 2]: one sync per batch
        mx = ms[..., 0].max(0)
        L[lo:lo + b] = mx + np.log((ms[..., 1] * np.exp(ms[..., 0] - mx)).sum(0)) - math.log(k)
    ll = L - 0.5 * I * math.log(math.pi)
    return IWAEResult(float(ll.mean()), float(ll.std()) / math.sqrt(n), k, n)


# ---- modules and trainer -------------------------------------------------------------------------------------------
@stock_model
class IWAE(VAE):
    """vae.VAE unchanged (modules, state_dict keys, forward with one CPU-generator sample, reparameterize): what makes
    it importance-weighted is the trainer's loss."""


@stock
class IWAETrainer(VAETrainer):
    """VAETrainer on the k-sample bound: histories `losses` (sum_b -L_k per batch) and `ess` (mean per batch), the
    epoch line (mean loss, mean ess, validation loss), best_val_loss / best_model as VAETrainer, checkpoints (+ k, seed,
    the number of training batches taken, so a resumed run continues the noise stream).  One GPU only."""
    _hook_names = ("compute_batch", "evaluate")
    _series = (("losses", "recon"), ("ess", "kl"))               # the engine's `kl` slots hold the mean ess
    _batch = "loss+stat"
    _line = "Epoch[%d/%d], Loss: %.4f, ESS: %.4f, Val Loss: %.4f"
    _one_gpu = "IWAETrainer"
    _engine_reads_trainer = True

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, k=5, seed=0):
        self.k, self.seed = check_k_seed(k, seed)              # before anything runs
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)
        self.losses, self.ess = [], []
        self.noise_steps = 0             # training batches taken: the next one's noise step
        self._eval_step = 0              # batch index within an evaluate() call

    def _stock(self):
        Z = getattr(self.model, "z_dim", 0)
        return super()._stock() and self.k <= IWAE_MAX_K and 1 <= Z <= IWAE_MAX_Z

    def compute_batch(self, batch):
        """(sum_b -L_k, mean ess) of a batch (general path: autograd over the fused linear kernels, eps from the
        contract's counter stream -- the training stream while the model trains, the validation one otherwise)."""
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
        z = mu[:, None, :] + eps * torch.exp(lv / 2)[:, None, :]
        xr = self.model.decoder(z.reshape(b * k, Z)).view(b, k, -1)
        logw = (-((x[:, None, :] - xr) ** 2).sum(-1) - 0.5 * (z ** 2).sum(-1) + 0.5 * (eps ** 2).sum(-1)
                + 0.5 * lv.sum(-1)[:, None])
        loss = -(torch.logsumexp(logw, 1) - math.log(k)).sum()
        ess = 1.0 / (torch.softmax(logw.detach(), 1) ** 2).sum(1)
        return loss, ess.mean()

    def evaluate(self, iterator):
        """Mean over the batches of sum_b -L_k on the validation stream (batch i at noise step i)."""
        self._eval_step = 0
        with torch.no_grad():
            return np.mean([self.compute_batch(batch)[0].item() for batch in iterator])

    def _general_optimizer(self, lr, weight_decay):
        # through this module's FlatAdam name: replacing iwae.FlatAdam is how this family's general optimiser is observed
        return FlatAdam(self.model.parameters(), lr, weight_decay=weight_decay)

    def _engine_class(self):
        from .engine import IWAEEngine
        return IWAEEngine

    def viz_loss(self):
        """The training loss (sum_b -L_k per batch) over the epochs."""
        from . import viz
        viz.one_loss_curve(self, "-L_k")


__all__ = ["Encoder", "Decoder", "IWAE", "IWAETrainer", "IWAEError", "iwae_noise_reference", "iwae_reference",
           "log_likelihood", "FlatAdam"]
