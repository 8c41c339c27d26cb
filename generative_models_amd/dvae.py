"""Denoising VAE (the reference's README to-do list, "Models: ... denoising VAE"; Im, Ahn, Memisevic & Bengio,
"Denoising Criterion for Variational Auto-Encoding Framework", arXiv 1511.06406): every training image x is corrupted
into x~ ~ p(x~ | x), the encoder sees x~ and the decoder is scored on the clean x,

    loss = sum((x - decoder(z))^2) + KL(q(z | x~) || N(0, I)),   z = mu(x~) + eps * exp(log_var(x~) / 2),

one corruption and one z per image.  vae.py's modules, state_dict keys and RNG protocol (loader shuffles, torch.randn
eps per batch) are unchanged: the corruption is drawn on the device from a counter-based generator keyed on
(seed, step, row, pixel) and never touches the global CPU generator.  Exported by src/dvae.py as Encoder / Decoder /
DVAE / DVAETrainer / corrupt.

The rule (gm_hip.h, csrc/gm_dvae.h; `corrupt_reference` below is the same rule in numpy): Philox4x32-10 with key
(seed mod 2^32, seed >> 32) and counter (e >> 2, step, row, 0x44564145) gives word e & 3 to pixel e of batch row `row`
at training batch `step` (0-based over the trainer's lifetime);
  salt_pepper, level p in [0, 1]: T = floor(p 2^31); u < T -> 0, else u - T < T -> 1 (unsigned), else x;
  gaussian, level sigma >= 0: fmaf(sigma, n, x), n the Box-Muller normal of the word (the Bayesian GAN's mapping);
level 0 is the identity, bit for bit.

Fused path: vae_engine.DVAEEngine (8 launches per training batch, as the VAE); an overridden hook or an edited model:
VAETrainer's general loop, whose compute_batch corrupts with gm_dvae_corrupt at the same step numbers."""
import math

import numpy as np
import torch

from . import philox
from ._lib import NOISE, GMError, check_seed
from .philox import box_muller_normals, philox4x32_10  # noqa: F401  (imported from here by other modules and tests)
from .trainers import VAE, Decoder, Encoder, FlatAdam, VAETrainer, stock, stock_model, to_cuda  # noqa: F401

CTR_TAG = 0x44564145          # "DVAE": the fourth counter word
_FLT_MAX = float(np.finfo(np.float32).max)


class NoiseError(GMError, ValueError):
    """A bad noise setting (name, level or seed): a ValueError, and a GMError like the package's other refusals."""


def check_noise(noise, level, seed):
    """(noise, level, seed) validated: a known noise name, a finite level in [0, 1] (salt_pepper) or >= 0 (gaussian),
    an integer seed in [0, 2^64); else NoiseError."""
    if not isinstance(noise, str) or noise not in NOISE:
        raise NoiseError("noise must be one of %s, got %r" % (sorted(NOISE), noise))
    if isinstance(level, (bool, np.bool_)):
        raise NoiseError("level must be a number")
    try:
        level = float(level)
    except (TypeError, ValueError):
        raise NoiseError("level must be a number, got %r" % (level,)) from None
    if not math.isfinite(level) or abs(level) > _FLT_MAX:
        raise NoiseError("level must be finite (in fp32), got %r" % level)
    if noise == "salt_pepper" and not 0.0 <= level <= 1.0:
        raise NoiseError("salt_pepper level (the replaced fraction) must lie in [0, 1], got %r" % level)
    if noise == "gaussian" and level < 0.0:
        raise NoiseError("gaussian level (the noise's standard deviation) must be >= 0, got %r" % level)
    return noise, level, check_seed(seed, error=NoiseError)


def corrupt(images, noise="salt_pepper", level=0.25, seed=0, step=0, row0=0):
    """The corrupted copy of `images` ([n, ...], flattened to rows) that the fused step feeds the encoder at training
    batch `step`, row i being batch position row0 + i: one gm_dvae_corrupt launch.  Returns a float32 device tensor
    [n, pixels]; the global CPU generator is untouched."""
    from . import ops_fused
    noise, level, seed = check_noise(noise, level, seed)
    step, row0 = int(step), int(row0)
    if step < 0 or row0 < 0:
        raise NoiseError("step and row0 must be >= 0")
    x = images.reshape(images.shape[0], -1)
    if not x.is_cuda:
        x = to_cuda(x)
        if not x.is_cuda:
            raise GMError("corrupt runs on the MI355X only: no GPU is visible")
    x = x.to(torch.float32).contiguous()
    return ops_fused.dvae_corrupt(x, ops_fused.corrupt_args(noise, level, seed, step=step, row0=row0))


# ---- the rule in numpy (the tests' reference; also a CPU reading of what the device computes) ------------------------
def corruption_words(n_rows, row_elems, seed, step, row0=0):
    """The uint32 word of every pixel: [n_rows, row_elems]."""
    return philox.words(n_rows, row_elems, seed, step, CTR_TAG, row0)


def sp_threshold(p):
    """T = floor(p 2^31), in 64-bit on the host."""
    return int(math.floor(float(p) * 2.0 ** 31))


def corrupt_reference(x, noise, level, seed, step, row0=0):
    """The rule in numpy: x [n, I] float32 -> the corrupted float32 rows (gaussian in fp64 and rounded once: the
    device's logf / sincospif are within a few ulp of it)."""
    noise, level, seed = check_noise(noise, level, seed)
    x = np.asarray(x, dtype=np.float32)
    n, I = x.shape
    if level == 0.0:
        return x.copy()
    nq4 = 4 * ((I + 3) // 4)
    words = corruption_words(n, nq4, seed, step, row0)
    if noise == "salt_pepper":
        T = np.uint64(sp_threshold(level))
        u = words[:, :I].astype(np.uint64)
        out = x.copy()
        out[u < T] = 0.0
        out[(u >= T) & (u - T < T)] = 1.0
        return out
    nrm = box_muller_normals(words)[:, :I]
    return (np.float64(np.float32(level)) * nrm + x.astype(np.float64)).astype(np.float32)


# ---- modules and trainer ----------------------------------------------------------------------------------------------
@stock_model
class DVAE(VAE):
    """vae.VAE unchanged (modules, state_dict keys, forward, reparameterize): what makes it denoising is what the
    trainer feeds the encoder."""


@stock
class DVAETrainer(VAETrainer):
    """VAETrainer with corrupted encoder inputs on training batches: same RNG protocol, histories (recon_loss,
    kl_loss), epoch line, best_val_loss on clean validation images, checkpoints (+ the noise settings and the number of
    training batches taken, so a resumed run continues the noise stream).  One GPU only."""

    _one_gpu = "DVAETrainer"
    _engine_reads_trainer = True

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, noise="salt_pepper", level=0.25, seed=0):
        self.noise, self.level, self.seed = check_noise(noise, level, seed)     # before anything runs
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)
        self.noise_steps = 0             # training batches taken: the next one's noise step

    def compute_batch(self, batch):
        """vae.py:193-208 with the encoder fed corrupt(images) on training batches (general path)."""
        images, _ = batch
        images = to_cuda(images.view(images.shape[0], -1))
        x_in = images
        if self.model.training:
            x_in = corrupt(images, self.noise, self.level, self.seed, step=self.noise_steps)
            self.noise_steps += 1
        outputs, mu, log_var = self.model(x_in)
        recon_loss = torch.sum((images - outputs) ** 2)
        return recon_loss, self.kl_divergence(mu, log_var)

    def _engine_class(self):
        from .engine import DVAEEngine
        return DVAEEngine

    def denoise(self, images, batch=1024):
        """(noisy, recon): noisy = the corruption of `images` as training batch step 0 sees it (corrupt(images, ...,
        step=0)), recon = sigmoid(decoder(mu(encoder(noisy)))) -- the mean decoding, no sampling.  Device tensors
        [n, pixels]; the global generator and the model's mode are untouched."""
        noisy = corrupt(images, self.noise, self.level, self.seed, step=0)
        torch.cuda.synchronize()
        with torch.no_grad():
            recon = torch.cat([self.model.decoder(self.model.encoder(noisy[i:i + batch])[0])
                               for i in range(0, noisy.shape[0], batch)])
        return noisy, recon


__all__ = ["Encoder", "Decoder", "DVAE", "DVAETrainer", "NoiseError", "corrupt", "corrupt_reference", "FlatAdam"]
