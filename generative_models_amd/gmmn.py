"""Generative moment matching network (Li, Swersky & Zemel, "Generative Moment Matching Networks", arXiv 1502.02761;
Dziugaite, Roy & Ghahramani, "Training generative neural networks via Maximum Mean Discrepancy optimization", arXiv
1505.03906): ns_gan.py's generator trained without a critic, on the kernel maximum mean discrepancy between a batch of its
samples and a batch of images.  Exported by src/gmmn.py as Generator / GMMN / GMMNTrainer.

The contract.  GMMN(image_size I, hidden_dim H, z_dim Z) holds G = trainers.Generator(I, H, Z) unchanged: x =
sigmoid(generate(relu(linear(z)))); state_dict keys G.linear.*, G.generate.* (an NSGAN checkpoint's generator loads with
strict=False).

Prior and noise (gm_hip.h, csrc/gm_gmmn.hip; `uniforms_reference` below is the same rule in numpy through philox.py, bit
for bit).  z is uniform on (-1, 1):  z[e] = fmaf(2, u, -1), u = ph_unit(word e & 3 of Philox block (e >> 2, step, row, tag))
under the trainer's `seed` -- exact in fp32.  Training: tag TAG_T = "GMMT", `step` the 0-based training batch count over
the trainer's life (`noise_steps`, saved in checkpoints; on the device ctr + nbase, DDPM's scheme), `row` the row's
position in the batch.  Validation: TAG_V = "GMMV", `step` the batch's index within the pass -- the validation loss is a
deterministic function of the weights.  sample(n, seed): TAG_S = "GMMS" under the sampling seed, step 0.  The global CPU
generator is touched by the loaders' shuffles only.

Loss.  Bandwidths `sigmas` (default SIGMAS, the paper's data-space set; 1 to metrics.MAX_SIGMAS values > 0),
k(a, b) = sum_s exp(-|a - b|^2 / (2 sigma_s^2)); generated rows x_1..x_N, data rows y_1..y_M (N = M = b in training):

    mmd2 = (1/N^2) sum_ij k(x_i, x_j) - (2/(N M)) sum_ij k(x_i, y_j) + (1/M^2) sum_jl k(y_j, y_l)

the biased V-statistic with its diagonals in;  loss = sqrt(mmd2 + 1e-8) when sqrt_loss (the paper's choice, the default),
else mmd2.  With w(d2) = sum_s exp(-d2 / (2 sigma_s^2)) / sigma_s^2,  C[i, j] = -(2/N^2) w(|x_i - x_j|^2) for j < N,
C[i, N + j] = +(2/(N M)) w(|x_i - y_j|^2),  r_i = sum_j C[i, j] and R = [X; Y]:

    d mmd2 / d x_i = r_i x_i - (C R)_i        (times 1 / (2 loss) under the square root)

and the gradient entering `generate` is that times x (1 - x).  The kernels evaluate it about mu = x_1, the first generated
row, as r_i (x_i - mu) - (C (R - mu))_i: the same number about any origin, and about a generated row the products that
cancel in it are small when the generator has collapsed (and vanish when every row is equal).

Numerical rules of the kernels: d^2 in the Gram form |a|^2 + |b|^2 - 2 a.b of the rows less mu (distances do not change)
on FP32-input MFMAs with fp32 accumulation, clamped at 0; two equal rows have d^2 = 0 exactly, so the pair (i, i) of the
xx and yy blocks has d^2 = 0 exactly (its kernel value is the number of bandwidths, bit for bit); every sum of kernel
values or coefficients in fp64 in a fixed order; no atomics, one writer per element: two runs, and graph against eager,
agree bit for bit.

Fused path: GMMNEngine below -- 12 launches per training batch, 7 per validation batch.  Training
batches of at most MAX_B = GM_GMMN_MAX_B rows (C [b, 2b] is 32 MB there); I <= 8192.  One GPU only: the statistic couples
every row of the batch.  An overridden compute_batch / evaluate or an edited model: the general loop -- autograd over
ops.fused_linear and ops_fused.mmd_loss on the same noise stream."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, philox, viz
from ._lib import GMMN_MAX_B, GMMN_MAX_Z, GMMN_TAG_S, GMMN_TAG_T, GMMN_TAG_V, MMD_MAX_I, MMD_MAX_SIGMAS, GMError
from .trainers import FlatAdam, Generator, OneLossTrainer, _stock_module, stock, stock_model  # noqa: F401
from .engine import GeneratorMatchEngine, _align4

TAG_T, TAG_V, TAG_S = GMMN_TAG_T, GMMN_TAG_V, GMMN_TAG_S
SIGMAS = (2.0, 5.0, 10.0, 20.0, 40.0, 80.0)      # the paper's data-space bandwidths (= metrics.MMD_SIGMAS)
MAX_B = GMMN_MAX_B


class GMMNError(GMError, ValueError):
    """A bad shape, bandwidth set, seed, sample count or batch size: a ValueError, and a GMError like the package's
    other refusals."""


def _int(v, name):
    return _lib.check_int(v, name, GMMNError)


def check_seed(seed):
    return _lib.check_seed(seed, error=GMMNError)


def check_sigmas(sigmas):
    """The bandwidths as a tuple of floats (None: SIGMAS): 1 to MMD_MAX_SIGMAS finite values > 0; else GMMNError."""
    from . import ops_fused as of_
    if sigmas is None:
        return SIGMAS
    if isinstance(sigmas, (str, bytes)) or isinstance(sigmas, (bool, np.bool_)):
        raise GMMNError("sigmas must be numbers, got %r" % (sigmas,))
    return tuple(float(s) for s in of_.mmd_sigmas(sigmas, None, "GMMN", GMMNError))


def generator_shape(image_size, hidden_dim, z_dim, error):
    """(I, H, Z) of a generator-matching model validated against the kernels' limits; else `error`."""
    I, H, Z = (_lib.check_int(v, n, error) for v, n in ((image_size, "image_size"), (hidden_dim, "hidden_dim"),
                                                        (z_dim, "z_dim")))
    if not 1 <= I <= MMD_MAX_I:
        raise error("image_size must lie in [1, %d], got %d" % (MMD_MAX_I, I))
    if H < 1:
        raise error("hidden_dim must be >= 1, got %d" % H)
    if not 1 <= Z <= GMMN_MAX_Z:
        raise error("z_dim must lie in [1, %d], got %d" % (GMMN_MAX_Z, Z))
    return I, H, Z


def check_shape(image_size, hidden_dim, z_dim):
    return generator_shape(image_size, hidden_dim, z_dim, GMMNError)


def check_batch(b):
    b = _int(b, "batch size")
    if not 1 <= b <= MAX_B:
        raise GMMNError("a GMMN trains on batches of 1 to %d rows (the coefficient array is [b, 2b]), got %d" % (MAX_B, b))
    return b


def uniforms_reference(n_rows, Z, seed, step, tag=TAG_T, row0=0):
    """The prior rows [n_rows, Z] float32 of rows row0 .. at `step` under `tag`: 2 u - 1 of philox.py's uniforms (exact in
    fp32, so equal to the device's fmaf bit for bit)."""
    u = philox.unit_uniforms(philox.words(n_rows, Z, seed, step, tag, row0))
    return (np.float32(2.0) * u - np.float32(1.0)).astype(np.float32)


# ---- modules ---------------------------------------------------------------------------------------------------------
class GeneratorModel(nn.Module):
    """One Generator: z in (-1, 1)^Z -> relu -> sigmoid -> I pixels.  GMMN below and swg.SWG are this model, each under its
    own name, stock mark and error class."""
    _error = GMError

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20):
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = generator_shape(image_size, hidden_dim, z_dim, self._error)
        self.G = Generator(self.image_size, self.hidden_dim, self.z_dim)
        self.shape = int(self.image_size ** 0.5)

    def forward(self, z):
        return self.G(z)


@stock_model
class GMMN(GeneratorModel):
    """One Generator: z in (-1, 1)^Z -> relu -> sigmoid -> I pixels."""
    _error = GMMNError


def generator_fused_ok(model):
    """True iff the model is a shipped generator-matching model itself (GMMN, swg.SWG) with its Generator unchanged and
    consistent shapes."""
    g = getattr(model, "G", None)
    if not (type(model).__dict__.get("_gm_stock_model", False) and type(g) is Generator and _stock_module(g, 2)):
        return False
    I, H, Z = model.image_size, model.hidden_dim, model.z_dim
    return (tuple(g.linear.weight.shape) == (H, Z) and tuple(g.generate.weight.shape) == (I, H)
            and g.linear.bias is not None and g.generate.bias is not None and 1 <= I <= MMD_MAX_I
            and 1 <= Z <= GMMN_MAX_Z)


gmmn_fused_ok = generator_fused_ok


# ---- engine ----------------------------------------------------------------------------------------------------------
class GMMNEngine(GeneratorMatchEngine):
    """The GMMN on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  Per
    training batch, 12 launches: 1. gm_gather_rows[_bits] (Y, the lower half of R);  2. gm_gmmn_prior (z);  3.-4. the two
    generator forwards (X, the upper half of R);  5.-6. gm_mmd_pairs (row norms, then every tile: block sums, C, the
    shares of r; the norms launch also leaves the centred rows R - mu, mu = x_1);  7. gm_mmd_finalize (mmd2, loss,
    1 / (2 loss), r);  8. P = C (R - mu) through ops.linear_bwd_dx (reduction length 2b, output width I);
    9. gm_mmd_grad (dA);  10. dH = dA Wgen [H > 0];  11. the two weight gradients + Adam as a pair;  12. the loss record
    with the counter tick.  Every input gradient is issued before the launch that steps the weights it reads.  A
    validation batch is launches 1-7 without C and r, and the record.  The noise step of a training batch is ctr + nbase
    (DDPMEngine's scheme), of a validation batch ctr.  One GPU only."""

    one_gpu = "the GMMN engine"
    fused_ok = staticmethod(gmmn_fused_ok)
    refusal = ("GMMN", "gmmn.GMMN", "Generator")     # the trainer: seed, sigmas, sqrt_loss and noise_steps
    noise_builder, tags = "gmmn_noise", (TAG_T, TAG_V)
    sig = None

    def _buffers(self, B):
        from . import ops_fused as of_
        check_batch(B)
        I, H, Z = self.I, self.H, self.Z
        z = lambda *s: torch.zeros(*s, device=self.device)
        self.Rb = z(2 * B, I)                        # R = [X; Y]: a batch of b rows uses rows [0, b) and [b, 2b)
        self.Rc = z(2 * B, I)                        # R - mu, mu = X's first row: what the distances and C (R - mu) read
        self.Zb, self.Hg = z(B, Z), z(B, H)
        self.C = z(B, _align4(2 * B))
        self.P, self.dA, self.dH = z(B, I), z(B, I), z(B, H)
        self.r, self.lossf = z(B), z(1)
        self.stats = torch.zeros(10, dtype=torch.float64, device=self.device)
        self.ws = of_.mmd_workspace(B, B, True, self.device)

    def _settings(self):
        t = self.trainer
        return {"sigmas": tuple(t.sigmas), "sqrt_loss": bool(t.sqrt_loss), "seed": int(t.seed)}

    def _graph_args(self):
        return (self.sig.data_ptr(),) if self.sig is not None else ()

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        from . import ops_fused as of_
        check_batch(B)
        sig = tuple(self.trainer.sigmas)
        if self.sig is None or self._sig_values != sig:
            self.sig, self._sig_values = of_.mmd_sigmas(sig, self.device, "GMMN", GMMNError), sig
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: Y, z, X, the statistic (+ its gradient, the backward and Adam when train)."""
        from . import ops_fused as of_
        X, Y = self._forward(st, t, b, train)
        of_.mmd_pairs(X, Y, self.sig, self.ws, C=self.C if train else None, Rc=self.Rc, N=b, M=b, stream=st)
        of_.mmd_finalize(b, b, self.sig.numel(), self.trainer.sqrt_loss, self.ws, self.stats,
                         r=self.r if train else None, loss_out=self.lossf, stream=st)
        if train:
            ops.linear_bwd_dx(self.C[:b, :2 * b], self.Rc[:2 * b], self.P, M=b, stream=st)
            of_.mmd_grad(X, self.P, self.r, self.stats, self.dA, N=b, sigmoid=True, mu=X[:1], stream=st)
        self._tail(st, t, b, train)


# ---- trainers --------------------------------------------------------------------------------------------------------
@stock
class GeneratorMatchTrainer(OneLossTrainer):
    """What the trainers of the two generator-matching models share (GMMN here, SWG in swg.py): the prior under the
    contract's Philox noise, the sampler, the constructor's batch-size check and step counters, and the refusals of a
    likelihood and a reconstruction.  A subclass names its engine, _error, _check_batch, the ops_fused builder of its
    noise, its sampling tag and the two refusals' words, and supplies compute_batch and viz_loss."""
    _engine_reads_trainer = True
    _engine_type = None         # the engine class
    _check_batch = None         # staticmethod(<module>.check_batch)
    _noise_builder = _tag_sample = None
    _no_likelihood = _no_encoder = None

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False):
        if getattr(train_iter, "batch_size", None) is not None:
            self._check_batch(train_iter.batch_size)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)
        self.noise_steps = 0                         # training batches taken: the next one's noise step
        self._eval_step = 0                          # batch index within an evaluate() call

    def _noise(self, seed, tag, step, row0=0):
        from . import ops_fused as of_
        return getattr(of_, self._noise_builder)(self.seed if seed is None else seed, tag, step=step, row0=row0)

    def prior(self, n, step, tag, seed=None, row0=0):
        """The prior rows [n, Z] of (seed, step, tag) on the model's device (gm_gmmn_prior)."""
        from . import ops_fused as of_
        z = torch.empty(n, self.model.z_dim, device=self._device())
        return of_.gmmn_prior(z, self._noise(seed, tag, step, row0))

    def _engine_class(self):
        return self._engine_type

    def train(self, num_epochs, lr=1e-3, weight_decay=0.0, quiet=False):
        """VAETrainer.train with these models' defaults."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    # ---- sampling ---------------------------------------------------------------------------------------------------
    SAMPLE_BLOCK = 1024          # sample() runs the generator on whole blocks of this many rows

    def sample(self, n, seed=0):
        """n samples [n, I] in [0, 1]: row r is the generator on the prior row r of (seed, the sampling tag, step 0),
        whatever n -- the generator always runs on whole blocks of SAMPLE_BLOCK rows (the last one is cut after the fact),
        so a row's launches, and its bits, do not depend on n.  Runs after a device synchronise; the global generator,
        the model's mode and the parameters are untouched."""
        n, seed = _lib.check_int(n, "n", self._error), _lib.check_seed(seed, error=self._error)
        if n < 1:
            raise self._error("n must be >= 1, got %d" % n)
        self._device()
        torch.cuda.synchronize()                     # after the engine's last Adam step
        out = []
        with torch.no_grad():
            for lo in range(0, n, self.SAMPLE_BLOCK):
                out.append(self.model(self.prior(self.SAMPLE_BLOCK, 0, self._tag_sample, seed=seed, row0=lo)))
        return torch.cat(out)[:n].contiguous()

    # ---- visualisation ----------------------------------------------------------------------------------------------
    def sample_images(self, epoch=-100, num_images=36, save=True):
        return viz.made_sample_images(self, epoch, num_images, save, self.viz_dir)

    def log_likelihood(self, images=None, k=500, seed=0):
        raise GMError(self._no_likelihood)

    def reconstruct_images(self, images, epoch, save=True):
        raise GMError(self._no_encoder)


@stock
class GMMNTrainer(GeneratorMatchTrainer):
    """Trains a GMMN on the kernel MMD and samples from it.  Histories: `losses` (one per training batch); the epoch line
    (mean training loss, validation loss); best_val_loss / best_model as the other one-loss trainers; checkpoints
    (+ sigmas, sqrt_loss, seed in the optimizer state's config, checked under strict=True, and the number of training
    batches taken, so a resumed run continues the noise stream bit for bit).  One GPU only."""
    _line = "Epoch[%d/%d], MMD Loss: %.6f, Val Loss: %.6f"
    _one_gpu = "GMMNTrainer"
    _error = GMMNError
    _fused_ok = staticmethod(gmmn_fused_ok)
    _engine_type = GMMNEngine
    _check_batch = staticmethod(check_batch)
    _noise_builder, _tag_sample = "gmmn_noise", TAG_S
    _no_likelihood = "a GMMN has no likelihood and no encoder; parzen() and mmd() score its samples"
    _no_encoder = "a GMMN has no encoder"

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, sigmas=None, sqrt_loss=True, seed=0):
        self.seed = check_seed(seed)                 # before anything runs
        self.sigmas = check_sigmas(sigmas)
        if isinstance(sqrt_loss, (bool, np.bool_)) is False:
            raise GMMNError("sqrt_loss must be a bool, got %r" % (sqrt_loss,))
        self.sqrt_loss = bool(sqrt_loss)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)

    def compute_batch(self, batch):
        """The MMD loss of a batch against as many samples (general path: autograd over the fused linear kernels and
        ops_fused.mmd_loss; z from the contract's counter stream -- the training stream while the model trains, the
        validation one otherwise)."""
        from . import ops_fused as of_
        x = self._flat_batch(batch)
        train, step = self._noise_step()
        z = self.prior(check_batch(x.shape[0]), step, TAG_T if train else TAG_V)
        return of_.mmd_loss(self.model(z), x, self.sigmas, self.sqrt_loss)

    def viz_loss(self):
        viz.one_loss_curve(self, "MMD loss")


__all__ = ["Generator", "GMMN", "GMMNTrainer", "GMMNEngine", "GMMNError", "uniforms_reference", "check_sigmas",
           "SIGMAS", "MAX_B", "TAG_T", "TAG_V", "TAG_S", "FlatAdam"]
