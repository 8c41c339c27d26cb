"""Adversarial autoencoder (Makhzani et al. 2015, arXiv 1511.05644; the reference's README to-do list, README.md:95
"adversarial autoencoder"): ae.py's reconstruction loop plus a latent critic that pushes the encoder's codes towards
N(0, I).  Exported by src/aae.py as Encoder / Decoder / Discriminator / AAE / AAETrainer.

Each batch runs three phases in this order ("reconstruction phase, then regularization phase: discriminator, then
generator", Makhzani section 2):
  1. compute_batch: recon_loss = sum (x - decoder(encoder(x)))^2; Adam(encoder + decoder, lr, weight_decay) steps;
  2. train_D: z_real = torch.randn(b, z_dim) (the batch's only draw), z_fake = encoder(x).detach() with the encoder
     after phase 1, D_loss = -mean(log(D(z_real) + 1e-8) + log(1 - D(z_fake) + 1e-8)); Adam(discriminator, D_lr);
  3. train_G: G_loss = -mean(log(D(encoder(x)) + 1e-8)) with D after phase 2; Adam(encoder, G_lr) with its own moments.
Validation computes the reconstruction loss only.  Fused path: vae_engine.AAEEngine; anything overridden or edited,
or shapes outside the fused kernels' limits: autograd over ops.fused_linear + three FlatAdams."""
import numpy as np
import torch
import torch.nn as nn

from ._lib import GMError
from .trainers import EPS, FlatAdam, VAETrainer, _TwoLayer, _lin, _stock_module, stock, stock_model, to_cuda

# a checkpoint's history keys: AAETrainer._series' lists, num_epochs, best_val_loss (what save_checkpoint derives)
HISTORY = ("recon_loss", "Dlosses", "Glosses", "num_epochs", "best_val_loss")
# what optim_state() adds to a checkpoint besides the AE / D moments ("m", "v") and the run settings
OPTIM_FIELDS = ("m", "v", "step", "config", "mG", "vG", "steps")


@stock_model
class Encoder(nn.Module):
    """Deterministic encoder: linear (I -> H, relu), then z (H -> Z, identity)."""

    def __init__(self, image_size, hidden_dim, z_dim):
        super().__init__()
        self.linear = nn.Linear(image_size, hidden_dim)
        self.z = nn.Linear(hidden_dim, z_dim)

    def forward(self, x):
        return _lin(self.z, _lin(self.linear, x, "relu"), "id")


@stock_model
class Decoder(_TwoLayer):
    """vae.py:64-77: linear (Z -> H, relu), then recon (H -> I, sigmoid)."""
    _names = ("linear", "recon")

    def __init__(self, z_dim, hidden_dim, image_size):
        super().__init__()
        self._build(z_dim, hidden_dim, image_size)

    def forward(self, z):
        return super().forward(z)


@stock_model
class Discriminator(_TwoLayer):
    """The latent critic with ns_gan.py's Discriminator names: linear (Z -> H, relu), then discriminate (H -> 1,
    sigmoid)."""
    _names = ("linear", "discriminate")

    def __init__(self, z_dim, hidden_dim, output_dim=1):
        super().__init__()
        self._build(z_dim, hidden_dim, output_dim)

    def forward(self, z):
        return super().forward(z)


@stock_model
class AAE(nn.Module):
    """.encoder / .decoder / .discriminator; forward(x) is the reconstruction decoder(encoder(x))."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20):
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = image_size, hidden_dim, z_dim
        self.encoder = Encoder(image_size, hidden_dim, z_dim)
        self.decoder = Decoder(z_dim, hidden_dim, image_size)
        self.discriminator = Discriminator(z_dim, hidden_dim, 1)
        self.shape = int(image_size ** 0.5)

    def forward(self, x):
        return self.decoder(self.encoder(x))


@stock
class AAETrainer(VAETrainer):
    """The three-phase loop above with VAETrainer's protocol: next(iter(test_iter)) at construction, the sampler's
    permutation per pass, best_model / best_val_loss on the validation reconstruction loss, viz=True adds one
    randn(36, z_dim) per epoch (sample_images)."""
    _gm_stock_class = True
    _hook_names = ("compute_batch", "train_D", "train_G", "evaluate")
    _series = (("recon_loss", "recon"), ("Dlosses", "dloss"), ("Glosses", "gloss"))
    _batch = "loss"             # the validation loss is vrecon alone, the epoch line has no total
    _hands_force_dp = False
    _line = "Epoch[%d/%d], Reconst Loss: %.4f, D Loss: %.4f, G Loss: %.4f, Val Loss: %.4f"

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False):
        self.model = to_cuda(model)
        self.name = model.__class__.__name__
        self.train_iter, self.val_iter, self.test_iter = train_iter, val_iter, test_iter
        self.best_val_loss = 1e10
        self.debugging_image, _ = next(iter(test_iter))          # (consumes RNG, as every VAE-family trainer)
        self.viz = viz
        self.recon_loss, self.Dlosses, self.Glosses = [], [], []
        self.num_epochs = 0
        self._engine = None
        self.use_graph = True

    # ---- reference-style hooks (the general path) -----------------------------------------------------------
    def compute_batch(self, batch):
        """Reconstruction phase: sum of squared errors of decoder(encoder(x))."""
        images, _ = batch
        images = to_cuda(images.view(images.shape[0], -1))
        return torch.sum((images - self.model(images)) ** 2)

    def train_D(self, images):
        """Regularization phase, discriminator: prior samples are real, encoder codes are fake."""
        m = self.model
        z_real = to_cuda(torch.randn(images.shape[0], m.z_dim))
        z_fake = m.encoder(images).detach()
        D_real, D_fake = m.discriminator(z_real), m.discriminator(z_fake)
        return -torch.mean(torch.log(D_real + EPS) + torch.log(1 - D_fake + EPS))

    def train_G(self, images):
        """Regularization phase, generator: the encoder learns to fool the discriminator."""
        m = self.model
        return -torch.mean(torch.log(m.discriminator(m.encoder(images)) + EPS))

    def evaluate(self, iterator):
        """Mean reconstruction loss over the iterator's batches (draws nothing beyond the loader's permutation)."""
        return np.mean([self.compute_batch(batch).item() for batch in iterator])

    # ---- path selection -----------------------------------------------------------------------------------------
    def _stock(self):
        if not self._hooks_stock():
            return False
        m = self.model
        if not type(m).__dict__.get("_gm_stock_model", False):
            return False                               # a subclass may have changed forward
        enc, dec, dis = (getattr(m, n, None) for n in ("encoder", "decoder", "discriminator"))
        if not (isinstance(enc, Encoder) and isinstance(dec, Decoder) and isinstance(dis, Discriminator)
                and all(_stock_module(x, 2) for x in (enc, dec, dis))):
            return False                               # edited / subclassed networks: general path
        from .engine import AAEEngine               # (engine first: it imports vae_engine's classes)
        if not AAEEngine.fused_ok(m):
            return False                               # outside the fused kernels' limits: general path
        return (self._loader_ok(self.train_iter) and self._loader_ok(self.val_iter)
                and self.train_iter.batch_size == self.val_iter.batch_size)

    def _engine_class(self):
        from .engine import AAEEngine
        return AAEEngine

    def train(self, num_epochs, lr=1e-3, D_lr=2e-4, G_lr=2e-4, weight_decay=1e-5, quiet=False):
        """num_epochs passes of the three-phase loop; lr / weight_decay: the autoencoder's Adam, D_lr / G_lr: the
        discriminator's and the generator's (no weight decay)."""
        from . import dp
        if dp.current()[0] > 1:                      # (not _one_gpu: this refusal never looked at force_dp)
            raise GMError("AAETrainer runs on one GPU: data parallelism is not implemented for it")
        if self._stock():
            return self._train_fused(num_epochs, lr, weight_decay, quiet, D_lr=D_lr, G_lr=G_lr)
        # GENERAL path: the three phases over autograd, three optimizers
        m = self.model
        ae_opt = FlatAdam(list(m.encoder.parameters()) + list(m.decoder.parameters()), lr, weight_decay=weight_decay)
        d_opt = FlatAdam(m.discriminator.parameters(), D_lr)
        g_opt = FlatAdam(m.encoder.parameters(), G_lr)
        for epoch in range(1, num_epochs + 1):
            self.model.train()
            recon, d, g = [], [], []
            for batch in self.train_iter:
                images = to_cuda(batch[0].view(batch[0].shape[0], -1))
                ae_opt.zero_grad()
                r = self.compute_batch(batch)
                r.backward()
                ae_opt.step()
                d_opt.zero_grad()
                dl = self.train_D(images)
                dl.backward()
                d_opt.step()
                g_opt.zero_grad()
                gl = self.train_G(images)
                gl.backward()
                g_opt.step()
                recon.append(r.item()); d.append(dl.item()); g.append(gl.item())
            self.model.eval()
            val_loss = self.evaluate(self.val_iter)
            self._end_epoch(epoch, num_epochs, (recon, d, g), val_loss, quiet)

    def viz_loss(self):
        from . import viz
        viz.vae_viz_loss(self, "none")


__all__ = ["Encoder", "Decoder", "Discriminator", "AAE", "AAETrainer", "FlatAdam"]
