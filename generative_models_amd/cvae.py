"""Class-conditional VAE (the first entry of the reference's to-do list, README.md:95 "Models: CVAE"): vae.py's model
and trainer with the class label fed to the encoder's and the decoder's first layers.  Exported by src/cvae.py as
Encoder / Decoder / CVAE / CVAETrainer.

A conditioned layer is linear(cat[x, onehot(y)]), computed in its split form x W^T + b + E[:, y] with E the weight of a
bias-free nn.Linear(C, H) named `label`: the one-hot input only selects one column of E per row.  Fused path:
vae_engine.CVAEEngine; anything overridden or edited: autograd over ops.label_linear / ops.fused_linear + FlatAdam."""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import GMError
from .trainers import (FlatAdam, VAETrainer, _lin, _stock_module, stock, stock_model, to_cuda)
from .engine import validate_labels


class LabelError(GMError, ValueError):
    """A bad class label in a sampling call: a ValueError, and a GMError like the package's other refusals."""


def _labels_arg(labels, n, num_classes):
    """Labels of a sampling call as an int64 CPU tensor of n classes: None -> arange(n) % C (class-balanced); an int ->
    that class for every row; a sequence / tensor of n integers in [0, C) otherwise (else LabelError)."""
    if labels is None:
        return torch.arange(n) % num_classes
    if isinstance(labels, (bool, np.bool_)):
        raise LabelError("labels must be integers")
    if isinstance(labels, (int, np.integer)):
        labels = [int(labels)] * n
    try:
        y = torch.as_tensor(labels).reshape(-1)
    except (TypeError, ValueError, RuntimeError) as e:
        raise LabelError("labels must be integers: %s" % e) from None
    if y.numel() != n:
        raise LabelError("expected %d labels, got %d" % (n, y.numel()))
    return validate_labels(y, num_classes, error=LabelError).to(torch.int64)


def _layer(first, label, x, y, act):
    if not x.is_cuda:
        raise GMError("generative_models_amd computes on MI355X only: got a %s tensor and there is "
                      "no CPU fallback (move the model and inputs with to_cuda)" % x.device)
    if not y.is_cuda:
        y = validate_labels(y, label.weight.shape[1])        # host labels: checked here, on the way in
    return ops.label_linear(x, first.weight, first.bias, label.weight, y, act)


@stock_model
class Encoder(nn.Module):
    """vae.py:47-61 conditioned on the class: relu(linear(x) + label(onehot(y))), then the mu / log_var heads."""

    def __init__(self, image_size, hidden_dim, z_dim, num_classes):
        super().__init__()
        self.linear = nn.Linear(image_size, hidden_dim)
        self.label = nn.Linear(num_classes, hidden_dim, bias=False)
        self.mu = nn.Linear(hidden_dim, z_dim)
        self.log_var = nn.Linear(hidden_dim, z_dim)

    def forward(self, x, y):
        h = _layer(self.linear, self.label, x, y, "relu")
        return _lin(self.mu, h, "id"), _lin(self.log_var, h, "id")


@stock_model
class Decoder(nn.Module):
    """vae.py:64-77 conditioned on the class: sigmoid(recon(relu(linear(z) + label(onehot(y)))))."""

    def __init__(self, z_dim, hidden_dim, image_size, num_classes):
        super().__init__()
        self.linear = nn.Linear(z_dim, hidden_dim)
        self.label = nn.Linear(num_classes, hidden_dim, bias=False)
        self.recon = nn.Linear(hidden_dim, image_size)

    def forward(self, z, y):
        return _lin(self.recon, _layer(self.linear, self.label, z, y, "relu"), "sigmoid")


@stock_model
class CVAE(nn.Module):
    """Conditional VAE (Sohn et al. 2015, Kingma et al. 2014 M2's conditioning): vae.py:80-106 with the class y given
    to both networks.

    Each conditioned layer is stored split: `linear` (weight W, bias b) on the data input and `label` (weight E,
    no bias) on the one-hot class.  linear(x) + label(onehot(y)) equals the usual concatenated form
    nn.Linear(in + C, H) applied to cat[x, onehot(y)] with weight [linear.weight | label.weight] and bias
    linear.bias; label(onehot(y)) is column y of E, which is how the kernels compute it."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20, num_classes=10):
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = image_size, hidden_dim, z_dim
        self.num_classes = num_classes
        self.encoder = Encoder(image_size, hidden_dim, z_dim, num_classes)
        self.decoder = Decoder(z_dim, hidden_dim, image_size, num_classes)
        self.shape = int(image_size ** 0.5)

    def forward(self, x, y):
        mu, log_var = self.encoder(x, y)
        z = self.reparameterize(mu, log_var)
        return self.decoder(z, y), mu, log_var

    def reparameterize(self, mu, log_var):
        """vae.py:100-106: epsilon from torch.randn(mu.shape) on the global CPU generator."""
        epsilon = to_cuda(torch.randn(mu.shape))
        return mu + epsilon * torch.exp(log_var / 2)


@stock
class CVAETrainer(VAETrainer):
    """VAETrainer with labels: batches are (images, labels), the networks see the class, sampling asks for one.  Same
    RNG protocol, history attributes, epoch line, checkpoints; fused engine CVAEEngine."""

    def compute_batch(self, batch):
        """vae.py:193-208 with the batch's classes (general path: autograd over the HIP linear kernels)."""
        images, labels = batch
        images = to_cuda(images.view(images.shape[0], -1))
        outputs, mu, log_var = self.model(images, labels)
        recon_loss = torch.sum((images - outputs) ** 2)
        return recon_loss, self.kl_divergence(mu, log_var)

    def _loader_ok(self, it):
        return super()._loader_ok(it) and len(it.dataset.tensors) >= 2

    def _stock(self):
        if not self._hooks_stock():
            return False
        m = self.model
        if not type(m).__dict__.get("_gm_stock_model", False):
            return False                               # a subclass may have changed forward / reparameterize
        enc, dec = getattr(m, "encoder", None), getattr(m, "decoder", None)
        if not (isinstance(enc, Encoder) and isinstance(dec, Decoder)
                and _stock_module(enc, 4) and _stock_module(dec, 3)
                and enc.label.bias is None and dec.label.bias is None):
            return False                               # edited / subclassed networks: general path
        return (self._loader_ok(self.train_iter) and self._loader_ok(self.val_iter)
                and self.train_iter.batch_size == self.val_iter.batch_size)

    def _engine_class(self):
        from .engine import CVAEEngine
        return CVAEEngine

    def _device_labels(self, loader):
        """The dataset's classes as an int32 device tensor, validated on the host once per dataset."""
        cache = self.__dict__.setdefault("_label_cache", {})
        key = id(loader.dataset)
        if key not in cache:
            y = validate_labels(loader.dataset.tensors[1], self.model.num_classes)
            cache[key] = y.to(next(self.model.parameters()).device)
        return cache[key]

    def _device_data(self, loader):
        return super()._device_data(loader), self._device_labels(loader)

    def train(self, num_epochs, lr=1e-3, weight_decay=1e-5, quiet=False):
        """vae.py:127-191 with labels."""
        if self._stock():
            self._device_labels(self.train_iter)       # bad labels raise here, before anything is launched
            self._device_labels(self.val_iter)
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    # ---- conditional sampling ------------------------------------------------------------------------------------
    def _decode(self, z, y, batch=1024):
        torch.cuda.synchronize()
        with torch.no_grad():
            return torch.cat([self.model.decoder(to_cuda(z[i:i + batch]), y[i:i + batch])
                              for i in range(0, z.shape[0], batch)])

    def sample(self, n, seed=0, labels=None):
        """n decoded samples [n, image_size] of the given classes (None: arange(n) % num_classes; an int: that class
        for all): z ~ N(0, I) from torch.Generator().manual_seed(seed); the global generator and the model's mode are
        untouched."""
        n = int(n)
        y = _labels_arg(labels, n, self.model.num_classes)
        gen = torch.Generator().manual_seed(int(seed))
        return self._decode(torch.randn(n, self.model.z_dim, generator=gen), y)

    def sample_images(self, epoch=-100, num_images=36, save=True, labels=None):
        """vae.py:254-276 for chosen classes (None: arange(num_images) % num_classes): z ~ N(0, I) from the global
        CPU generator, decoded, written as <viz_dir>/sample_<epoch>.png."""
        import os
        from . import viz
        y = _labels_arg(labels, int(num_images), self.model.num_classes)
        z = torch.randn(num_images, self.model.z_dim)
        images = viz._to_host_images(self._decode(z, y), self.model.shape)
        if save:
            viz.write_png_gray(os.path.join(viz._outdir(self, self.viz_dir), "sample_%d.png" % epoch),
                               viz.make_grid(images, int(num_images ** 0.5)))
        return images

    def reconstruct_images(self, images, labels, epoch, save=True):
        """vae.py:225-252 with the images' classes: real.png + reconst_<epoch>.png (eps drawn as the model does)."""
        import os
        from . import viz
        y = _labels_arg(labels, images.shape[0], self.model.num_classes)
        with torch.no_grad():
            out = self.model(to_cuda(images.reshape(images.shape[0], -1)), y)[0]
        side = int(round(out.shape[1] ** 0.5))
        rec = viz._to_host_images(out, side)
        if save:
            d = viz._outdir(self, self.viz_dir)
            grid = int(rec.shape[0] ** 0.5)
            viz.write_png_gray(os.path.join(d, "real.png"),
                               viz.make_grid(viz._to_host_images(images.reshape(images.shape[0], -1), side), grid))
            viz.write_png_gray(os.path.join(d, "reconst_%d.png" % epoch), viz.make_grid(rec, grid))
        return rec

    def sample_interpolated_images(self):
        raise GMError("CVAETrainer: interpolation plots are defined for the unconditional VAE; use "
                      "sample_images(labels=...)")

    def explore_latent_space(self, num_epochs=3):
        raise GMError("CVAETrainer: explore_latent_space is defined for the unconditional VAE")

    def make_all(self):
        raise GMError("CVAETrainer: make_all is defined for the unconditional VAE; use sample_images(labels=...)")


__all__ = ["Encoder", "Decoder", "CVAE", "CVAETrainer", "LabelError", "FlatAdam"]
