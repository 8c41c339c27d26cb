"""beta-TCVAE (Chen, Li, Grosse & Duvenaud, "Isolating Sources of Disentanglement in VAEs", arXiv 1802.04942): vae.py's
Encoder, Decoder and VAE, state_dict keys unchanged (a VAE or IWAE checkpoint loads), trained on the ELBO with its KL
term split into index-code mutual information, total correlation and dimension-wise KL, each with a weight of its own.
alpha = beta = gamma is the beta-VAE (Higgins et al., ICLR 2017), all three 1 the VAE with a sampled KL.  Exported by
src/tc_vae.py as Encoder / Decoder / TCVAE / TCVAETrainer.

The contract.  A batch of M images out of a dataset of N; [mu_i | lv_i] = encoder(x_i), one sample per image:

    eps_i ~ N(0, I_Z)        z_i = mu_i + exp(lv_i / 2) eps_i        l(i, j, d) = log N(z_id; mu_jd, exp(lv_jd))

    lqzx_i  = sum_d l(i, i, d)                                       log q(z_i | x_i)
    lpz_i   = sum_d log N(z_id; 0, 1)                                log p(z_i)
    lqz_i   = logsumexp_j sum_d l(i, j, d) - log(N M)                log q(z_i), minibatch-weighted sampling
    lprod_i = sum_d [ logsumexp_j l(i, j, d) - log(N M) ]            log prod_d q(z_id)
    mi_i = lqzx_i - lqz_i        tc_i = lqz_i - lprod_i        dwkl_i = lprod_i - lpz_i

    lp_i = -(alpha mi_i + beta tc_i + gamma dwkl_i)
    loss = sum_i -(log p(x_i | z_i) + lp_i),     log p(x_i | z_i) = -||x_i - decoder(z_i)||^2   (iwae.py's, at k = 1)

Every sum over j runs over the whole batch, j = i included.  With alpha = beta = gamma = 1 the pair terms cancel and
lp_i is iwae.py's 1/2 sum_d (eps_id^2 - z_id^2 + lv_id).  At Z = 1 the two logsumexps coincide and tc = 0.

Gradients flow through z_i (so to mu_i and lv_i) and through the partner parameters mu_j, lv_j of every pair.  The
coefficient of l(i, j, d) in -lp_i is (beta - alpha) a_ij + (gamma - beta) c_ijd (+ alpha at j = i), with a_i. the
softmax over j of sum_d l(i, j, d) and c_i.d the softmax over j of l(i, j, d) (`pair_coefficients`); -gamma lpz adds
gamma z_i to d / d z_i; the alpha term's derivatives cancel through the reparameterisation except for -alpha / 2 on lv.

The records of the fused path leave the -1/2 log(2 pi) of every l out (it cancels out of mi, tc and dwkl):
lse_joint_i = logsumexp_j sum_d l'(i, j, d), lse_dim_id = logsumexp_j l'(i, j, d), l' = l + 1/2 log(2 pi).

Noise: iwae.py's rule unchanged at k = 1 -- the same counter layout, the IWAE's two tags and Box-Muller mapping, so z
is gm_iwae_sample's bit for bit; `noise_steps` travels in checkpoints; eps is never stored, the backward regenerates it.

N is `dataset_size` (default: len(train_iter.dataset)) for a training batch and the size of the iterator's own dataset
in a validation or test pass; M is the batch's own size (the ragged last batch has its own log(N M)).

Fused path: vae_engine.TCVAEEngine (k = 1, 1 <= Z <= 32): the IWAE's 12 launches with
gm_tc_sample and gm_tc_reduce as launches 3 and 10.  An overridden compute_batch or evaluate, an edited model or Z > 32:
the general loop -- autograd over ops.fused_linear, eps from ops_fused.iwae_normals (the same counter stream),
`batch_objective` below in torch."""
import math

import numpy as np
import torch

from . import _lib
from ._lib import IWAE_MAX_Z, GMError
from .iwae import TAG_EVAL, TAG_TRAIN, IWAETrainer
from .metrics import TCResult
from .trainers import VAE, Decoder, Encoder, FlatAdam, _decode_rows, _stock_module, stock, stock_model, to_cuda  # noqa: F401

LOG_2PI = math.log(2.0 * math.pi)


class TCVAEError(GMError, ValueError):
    """A bad alpha, beta, gamma, dataset_size or dim: a ValueError, and a GMError like the package's other refusals."""


def check_weights(alpha, beta, gamma):
    """(alpha, beta, gamma) validated: finite numbers >= 0; else TCVAEError."""
    out = []
    for v, nm in ((alpha, "alpha"), (beta, "beta"), (gamma, "gamma")):
        v = _lib.check_real(v, nm, TCVAEError)
        if v < 0:
            raise TCVAEError("%s must be >= 0, got %r" % (nm, v))
        out.append(v)
    return tuple(out)


def check_dataset_size(n):
    n = _lib.check_int(n, "dataset_size", TCVAEError)
    if n < 1:
        raise TCVAEError("dataset_size must be >= 1, got %d" % n)
    return n


# ---- the contract in torch (the general path's arithmetic; differentiable, any dtype and device) ---------------------
def pair_log_density(z, mu, lv):
    """l [M, M, Z]: l[i, j, d] = log N(z_id; mu_jd, exp(lv_jd))."""
    d = z[:, None, :] - mu[None, :, :]
    return -0.5 * (LOG_2PI + lv[None, :, :] + d * d * torch.exp(-lv)[None, :, :])


def decomposition_terms(z, mu, lv, log_nm):
    """(mi, tc, dwkl), each [M], of the samples z [M, Z] under the batch's posteriors mu, lv [M, Z]."""
    l = pair_log_density(z, mu, lv)
    lqzx = torch.diagonal(l, dim1=0, dim2=1).sum(0)
    lpz = (-0.5 * (LOG_2PI + z * z)).sum(1)
    lqz = torch.logsumexp(l.sum(2), 1) - log_nm
    lprod = (torch.logsumexp(l, 1) - log_nm).sum(1)
    return lqzx - lqz, lqz - lprod, lprod - lpz


def pair_coefficients(z, mu, lv, alpha, beta, gamma):
    """w [M, M, Z]: the coefficient of l(i, j, d) in -lp_i, (beta - alpha) a_ij + (gamma - beta) c_ijd + alpha [i = j]."""
    l = pair_log_density(z, mu, lv)
    a = torch.softmax(l.sum(2), 1)
    c = torch.softmax(l, 1)
    eye = torch.eye(z.shape[0], dtype=z.dtype, device=z.device)
    return (beta - alpha) * a[:, :, None] + (gamma - beta) * c + alpha * eye[:, :, None]


def batch_objective(mu, lv, eps, x, decode, alpha, beta, gamma, log_nm):
    """(loss, (mi, tc, dwkl, recon) each [M]) of one batch from the encoder's outputs: z = mu + exp(lv / 2) eps,
    loss = sum_i (||x_i - decode(z_i)||^2 + alpha mi_i + beta tc_i + gamma dwkl_i)."""
    z = mu + eps * torch.exp(lv / 2)
    mi, tc, dw = decomposition_terms(z, mu, lv, log_nm)
    recon = ((x - decode(z)) ** 2).sum(1)
    return (recon + alpha * mi + beta * tc + gamma * dw).sum(), (mi, tc, dw, recon)


# ---- modules and trainer -------------------------------------------------------------------------------------------
@stock_model
class TCVAE(VAE):
    """vae.VAE unchanged (modules, state_dict keys, forward with one CPU-generator sample, reparameterize): what makes
    it a beta-TCVAE is the trainer's loss."""


@stock
class TCVAETrainer(IWAETrainer):
    """IWAETrainer's loop at k = 1 on the decomposed bound: histories `losses` (the batch's loss) and `tc` (the batch's
    mean total correlation), the epoch line, best_val_loss / best_model, checkpoints (+ alpha, beta, gamma, dataset_size,
    seed and the training batches taken: a resume under other settings is refused), sample / parzen / log_likelihood
    as the VAE's (q is the plain Gaussian), decomposition and traverse.  One GPU only."""

    _series = (("losses", "recon"), ("tc", "kl"))                # the engine's `kl` slots hold the mean tc
    _line = "Epoch[%d/%d], Loss: %.4f, TC: %.4f, Val Loss: %.4f"
    _one_gpu = "TCVAETrainer"

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, alpha=1.0, beta=6.0, gamma=1.0,
                 dataset_size=None, seed=0):
        self.alpha, self.beta, self.gamma = check_weights(alpha, beta, gamma)        # before anything runs
        if dataset_size is not None:
            dataset_size = check_dataset_size(dataset_size)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz, k=1, seed=seed)
        self.dataset_size = len(train_iter.dataset) if dataset_size is None else dataset_size
        self.losses, self.tc = [], []
        self._eval_n = None              # the dataset size of the evaluate() pass under way

    def _engine_class(self):
        from .engine import TCVAEEngine
        return TCVAEEngine

    def _stock(self):
        return self.k == 1 and super()._stock()

    def compute_batch(self, batch):
        """(loss, mean tc) of a batch (general path: autograd over the fused linear kernels, eps from the contract's
        counter stream -- the training stream and dataset_size while the model trains, the validation stream and the
        evaluated iterator's own dataset size otherwise -- and batch_objective in torch)."""
        from . import ops_fused as of_
        images, _ = batch
        x = to_cuda(images.view(images.shape[0], -1))
        if not x.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: no GPU is visible")
        b = x.shape[0]
        mu, lv = self.model.encoder(x)
        train, step = self._noise_step()
        eps = of_.iwae_normals(b, 1, mu.shape[1], self.seed, step, TAG_TRAIN if train else TAG_EVAL, device=x.device)
        n = self.dataset_size if train or self._eval_n is None else self._eval_n
        loss, (_, tc, _, _) = batch_objective(mu, lv, eps, x, self.model.decoder, self.alpha, self.beta, self.gamma,
                                              math.log(n * b))
        return loss, tc.detach().mean()

    def evaluate(self, iterator):
        """Mean over the batches of the loss on the validation stream (batch i at noise step i), N the iterator's own
        dataset size."""
        self._eval_n = len(iterator.dataset)
        try:
            return super().evaluate(iterator)
        finally:
            self._eval_n = None

    def viz_loss(self):
        """The training loss per batch over the epochs."""
        from . import viz
        viz.one_loss_curve(self, "loss")

    # ---- evaluation -------------------------------------------------------------------------------------------------
    def _eval_setup(self, what):
        m = self.model
        enc, dec = getattr(m, "encoder", None), getattr(m, "decoder", None)
        if not (type(enc) is Encoder and type(dec) is Decoder and _stock_module(enc, 3) and _stock_module(dec, 2)):
            raise GMError("%s needs vae.py's Encoder and Decoder unchanged" % what)
        if not torch.cuda.is_available():
            raise GMError("%s runs on the MI355X only: no GPU is visible" % what)
        dev = enc.linear.weight.device
        if dev.type != "cuda":
            raise GMError("%s: the model is not on the GPU" % what)
        return enc, dec, dev

    def decomposition(self, images=None):
        """metrics.TCResult(mi, tc, dw_kl, recon, n): the three terms of the KL and the reconstruction error per image
        over `images` ([n, ...]; None: the whole test_iter's dataset), taken in order in batches of test_iter's batch
        size with N = n -- means over the batches weighted by batch size.  Evaluation noise: TAG_EVAL, the trainer's
        seed, step = the batch's index.  The global generator, the model's mode and the parameters are untouched."""
        from . import ops
        from . import ops_fused as of_
        enc, dec, dev = self._eval_setup("decomposition")
        if images is None:
            images = self.test_iter.dataset.tensors[0]
        x = images.reshape(images.shape[0], -1).to(dev, torch.float32).contiguous()
        n, I = x.shape
        Z = enc.mu.weight.shape[0]
        if not 1 <= Z <= IWAE_MAX_Z:
            raise GMError("decomposition supports 1 <= z_dim <= %d (got %d)" % (IWAE_MAX_Z, Z))
        if n < 1 or enc.linear.weight.shape[1] != I:
            raise GMError("decomposition: %d images of %d pixels for a model of %d" % (n, I, enc.linear.weight.shape[1]))
        H, Hd = enc.linear.weight.shape[0], dec.linear.weight.shape[0]
        w = lambda p: p.detach().contiguous()
        nb = min(int(self.test_iter.batch_size), n)
        z_ = lambda *s: torch.empty(*s, device=dev)
        He, mu_, lv_, Zs, lp, Hdec, Xr = z_(nb, H), z_(nb, Z), z_(nb, Z), z_(nb, Z), z_(nb), z_(nb, Hd), z_(nb, I)
        lsej, lsed, tcr = of_.tc_records(nb, Z, device=dev)
        terms = z_(nb, 3)
        acc = torch.zeros(4, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()                     # after the engines' last Adam step
        for step, lo in enumerate(range(0, n, nb)):
            b = min(nb, n - lo)
            xb = x[lo:lo + b]
            ops.linear_fwd(xb, w(enc.linear.weight), w(enc.linear.bias), He, "relu", M=b)
            ops.linear_fwd(He, w(enc.mu.weight), w(enc.mu.bias), mu_, "id", M=b)
            ops.linear_fwd(He, w(enc.log_var.weight), w(enc.log_var.bias), lv_, "id", M=b)
            ml = torch.cat([mu_[:b], lv_[:b]], 1)                              # [mu | lv], as the engine's packed layer
            of_.tc_sample(ml, Zs, lp, lsej, lsed, tcr, of_.iwae_noise(self.seed, TAG_EVAL, 1, step=step), self.alpha,
                          self.beta, self.gamma, math.log(n * b), b, Z, terms=terms)
            ops.linear_fwd(Zs, w(dec.linear.weight), w(dec.linear.bias), Hdec, "relu", M=b)
            ops.linear_fwd(Hdec, w(dec.recon.weight), w(dec.recon.bias), Xr, "sigmoid", M=b)
            acc[:3] += terms[:b].double().sum(0)
            acc[3] += ((xb - Xr[:b]).double() ** 2).sum()
        mi, tc, dw, recon = (acc / n).cpu().tolist()                           # the one sync
        return TCResult(mi, tc, dw, recon, n)

    def traverse(self, image, dim, values):
        """The decoder's output [len(values), image_size] with coordinate `dim` of mu(image) set to each of `values`
        (the other coordinates stay at the image's posterior mean).  No autograd, no mode change, no RNG use."""
        enc, dec, dev = self._eval_setup("traverse")
        Z = enc.mu.weight.shape[0]
        dim = _lib.check_int(dim, "dim", TCVAEError)
        if not 0 <= dim < Z:
            raise TCVAEError("dim must lie in [0, %d), got %d" % (Z, dim))
        vals = torch.as_tensor(np.asarray(values, dtype=np.float32).reshape(-1))
        x = torch.as_tensor(image).reshape(1, -1).to(dev, torch.float32)
        torch.cuda.synchronize()
        with torch.no_grad():
            mu, _ = enc(x)
        z = mu.detach().cpu().repeat(vals.numel(), 1)
        z[:, dim] = vals
        return _decode_rows(dec, z)


__all__ = ["Encoder", "Decoder", "TCVAE", "TCVAETrainer", "TCVAEError", "pair_log_density", "decomposition_terms",
           "pair_coefficients", "batch_objective", "FlatAdam"]
