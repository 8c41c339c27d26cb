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
from .engine import VAEEngine, _align4, _Linear

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


def check_shape(image_size, hidden_dim, z_dim):
    I, H, Z = _int(image_size, "image_size"), _int(hidden_dim, "hidden_dim"), _int(z_dim, "z_dim")
    if not 1 <= I <= MMD_MAX_I:
        raise GMMNError("image_size must lie in [1, %d], got %d" % (MMD_MAX_I, I))
    if H < 1:
        raise GMMNError("hidden_dim must be >= 1, got %d" % H)
    if not 1 <= Z <= GMMN_MAX_Z:
        raise GMMNError("z_dim must lie in [1, %d], got %d" % (GMMN_MAX_Z, Z))
    return I, H, Z


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
@stock_model
class GMMN(nn.Module):
    """One Generator: z in (-1, 1)^Z -> relu -> sigmoid -> I pixels."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20):
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = check_shape(image_size, hidden_dim, z_dim)
        self.G = Generator(self.image_size, self.hidden_dim, self.z_dim)
        self.shape = int(self.image_size ** 0.5)

    def forward(self, z):
        return self.G(z)


def gmmn_fused_ok(model):
    """True iff the model is GMMN itself with its Generator unchanged and consistent shapes."""
    g = getattr(model, "G", None)
    if not (type(model).__dict__.get("_gm_stock_model", False) and type(g) is Generator and _stock_module(g, 2)):
        return False
    I, H, Z = model.image_size, model.hidden_dim, model.z_dim
    return (tuple(g.linear.weight.shape) == (H, Z) and tuple(g.generate.weight.shape) == (I, H)
            and g.linear.bias is not None and g.generate.bias is not None and 1 <= I <= MMD_MAX_I
            and 1 <= Z <= GMMN_MAX_Z)


# ---- engine ----------------------------------------------------------------------------------------------------------
class GMMNEngine(VAEEngine):
    """The GMMN on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  Per
    training batch, 12 launches: 1. gm_gather_rows[_bits] (Y, the lower half of R);  2. gm_gmmn_prior (z);  3.-4. the two
    generator forwards (X, the upper half of R);  5.-6. gm_mmd_pairs (row norms, then every tile: block sums, C, the
    shares of r; the norms launch also leaves the centred rows R - mu, mu = x_1);  7. gm_mmd_finalize (mmd2, loss,
    1 / (2 loss), r);  8. P = C (R - mu) through ops.linear_bwd_dx (reduction length 2b, output width I);
    9. gm_mmd_grad (dA);  10. dH = dA Wgen [H > 0];  11. the two weight gradients + Adam as a pair;  12. the loss record
    with the counter tick.  Every input gradient is issued before the launch that steps the weights it reads.  A validation batch is launches 1-7 without C and r, and the record.  The noise step of a
    training batch is ctr + nbase (DDPMEngine's scheme), of a validation batch ctr.  One GPU only."""

    has_eps = False
    one_gpu = "the GMMN engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        if not gmmn_fused_ok(model):
            raise GMError("GMMNEngine: the model is not gmmn.GMMN with its Generator unchanged; GMMNTrainer trains "
                          "such models on the general path")
        g = model.G
        self._init_flat(model, device, use_graph, [g.linear.weight, g.linear.bias, g.generate.weight, g.generate.bias])
        self._bind_trainer(trainer)                  # seed, sigmas, sqrt_loss and noise_steps are read from it
        self.L1, self.L2 = _Linear(self.fp, g.linear), _Linear(self.fp, g.generate)
        self.I, self.H, self.Z = model.image_size, model.hidden_dim, model.z_dim
        self.sig = None

    def _alloc(self, B):
        if self._bufB == B:
            return
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
        self._bufB = B
        self.graphs = {}

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
        L1, L2, tr = self.L1, self.L2, self.trainer
        idx_slot = self._slot(t, 1, 0, self.R, self.B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        X, Y = self.Rb[:b], self.Rb[b:2 * b]
        ops.gather_rows(self.data, self.idx_ring.view(-1), Y, B=b, idx_slot=idx_slot, stream=st)
        of_.gmmn_prior(self.Zb, of_.gmmn_noise(tr.seed, TAG_T if train else TAG_V, **self._clock(t, train)), B=b,
                       Z=self.Z, stream=st)
        ops.linear_fwd(self.Zb, L1.W, L1.b, self.Hg, "relu", M=b, stream=st)
        ops.linear_fwd(self.Hg, L2.W, L2.b, X, "sigmoid", M=b, stream=st)
        of_.mmd_pairs(X, Y, self.sig, self.ws, C=self.C if train else None, Rc=self.Rc, N=b, M=b, stream=st)
        of_.mmd_finalize(b, b, self.sig.numel(), tr.sqrt_loss, self.ws, self.stats, r=self.r if train else None,
                         loss_out=self.lossf, stream=st)
        if train:
            adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
            ops.linear_bwd_dx(self.C[:b, :2 * b], self.Rc[:2 * b], self.P, M=b, stream=st)
            of_.mmd_grad(X, self.P, self.r, self.stats, self.dA, N=b, sigmoid=True, mu=X[:1], stream=st)
            # dH reads the output layer's weights BEFORE the pair's Adam updates them
            ops.linear_bwd_dx(self.dA, L2.W, self.dH, below=self.Hg, epi="relu", M=b, stream=st)
            ops.linear_bwd_dw_adam_pair(dict(dA=self.dA, X=self.Hg, lin=L2, adam=adam, M=b),
                                        dict(dA=self.dH, X=self.Zb, lin=L1, adam=adam, M=b),
                                        weight_decay=self.wd, stream=st)
        of_.sum_finalize(self.lossf, 1, self.recon if train else self.vrecon, out_slot=loss_slot,
                         tick=self.ctr if self.use_graph else None, stream=st)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class GMMNTrainer(OneLossTrainer):
    """Trains a GMMN on the kernel MMD and samples from it.  Histories: `losses` (one per training batch); the epoch line
    (mean training loss, validation loss); best_val_loss / best_model as the other one-loss trainers; checkpoints
    (+ sigmas, sqrt_loss, seed in the optimizer state's config, checked under strict=True, and the number of training
    batches taken, so a resumed run continues the noise stream bit for bit).  One GPU only."""
    _line = "Epoch[%d/%d], MMD Loss: %.6f, Val Loss: %.6f"
    _one_gpu = "GMMNTrainer"
    _error = GMMNError
    _fused_ok = staticmethod(gmmn_fused_ok)

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, sigmas=None, sqrt_loss=True, seed=0):
        self.seed = check_seed(seed)                 # before anything runs
        self.sigmas = check_sigmas(sigmas)
        if isinstance(sqrt_loss, (bool, np.bool_)) is False:
            raise GMMNError("sqrt_loss must be a bool, got %r" % (sqrt_loss,))
        self.sqrt_loss = bool(sqrt_loss)
        if getattr(train_iter, "batch_size", None) is not None:
            check_batch(train_iter.batch_size)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)
        self.noise_steps = 0                         # training batches taken: the next one's noise step
        self._eval_step = 0                          # batch index within an evaluate() call

    def prior(self, n, step, tag, seed=None, row0=0):
        """The prior rows [n, Z] of (seed, step, tag) on the model's device (gm_gmmn_prior)."""
        from . import ops_fused as of_
        z = torch.empty(n, self.model.z_dim, device=self._device())
        return of_.gmmn_prior(z, of_.gmmn_noise(self.seed if seed is None else seed, tag, step=step, row0=row0))

    def compute_batch(self, batch):
        """The MMD loss of a batch against as many samples (general path: autograd over the fused linear kernels and
        ops_fused.mmd_loss; z from the contract's counter stream -- the training stream while the model trains, the
        validation one otherwise)."""
        from . import ops_fused as of_
        x = self._flat_batch(batch)
        train, step = self._noise_step()
        z = self.prior(check_batch(x.shape[0]), step, TAG_T if train else TAG_V)
        return of_.mmd_loss(self.model(z), x, self.sigmas, self.sqrt_loss)

    def _engine_class(self):
        import functools
        return functools.partial(GMMNEngine, trainer=self)

    def train(self, num_epochs, lr=1e-3, weight_decay=0.0, quiet=False):
        """VAETrainer.train with this model's defaults."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    # ---- sampling ---------------------------------------------------------------------------------------------------
    SAMPLE_BLOCK = 1024          # sample() runs the generator on whole blocks of this many rows

    def sample(self, n, seed=0):
        """n samples [n, I] in [0, 1]: row r is the generator on the prior row r of (seed, TAG_S, step 0), whatever n --
        the generator always runs on whole blocks of SAMPLE_BLOCK rows (the last one is cut after the fact), so a row's
        launches, and its bits, do not depend on n.  Runs after a device synchronise; the global generator, the model's
        mode and the parameters are untouched."""
        n, seed = _int(n, "n"), check_seed(seed)
        if n < 1:
            raise GMMNError("n must be >= 1, got %d" % n)
        self._device()
        torch.cuda.synchronize()                     # after the engine's last Adam step
        out = []
        with torch.no_grad():
            for lo in range(0, n, self.SAMPLE_BLOCK):
                out.append(self.model(self.prior(self.SAMPLE_BLOCK, 0, TAG_S, seed=seed, row0=lo)))
        return torch.cat(out)[:n].contiguous()

    # ---- visualisation ----------------------------------------------------------------------------------------------
    def sample_images(self, epoch=-100, num_images=36, save=True):
        return viz.made_sample_images(self, epoch, num_images, save, self.viz_dir)

    def log_likelihood(self, images=None, k=500, seed=0):
        raise GMError("a GMMN has no likelihood and no encoder; parzen() and mmd() score its samples")

    def reconstruct_images(self, images, epoch, save=True):
        raise GMError("a GMMN has no encoder")

    def viz_loss(self):
        viz.one_loss_curve(self, "MMD loss")


__all__ = ["Generator", "GMMN", "GMMNTrainer", "GMMNEngine", "GMMNError", "uniforms_reference", "check_sigmas",
           "SIGMAS", "MAX_B", "TAG_T", "TAG_V", "TAG_S", "FlatAdam"]
