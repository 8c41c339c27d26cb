"""Sliced-Wasserstein generator (Deshpande, Zhang & Schwing, "Generative Modeling using the Sliced Wasserstein Distance",
arXiv 1803.11188; Kolouri et al., arXiv 1804.01947; Wu et al., arXiv 1706.02631; the "SWD" score of Karras et al., arXiv
1710.10196): ns_gan.py's generator trained without a critic, on the sliced squared 2-Wasserstein distance between a batch
of its samples and a batch of images.  Exported by src/swg.py as Generator / SWG / SWGTrainer.

The contract.  SWG(image_size I, hidden_dim H, z_dim Z) holds G = trainers.Generator(I, H, Z) unchanged: x =
sigmoid(generate(relu(linear(z)))); state_dict keys G.linear.*, G.generate.* (an NSGAN or GMMN checkpoint's generator loads
with strict=False).

Prior.  The GMMN's: z uniform on (-1, 1), z[e] = fmaf(2, u, -1), u = ph_unit(word e & 3 of Philox block (e >> 2, step, row,
tag)) under the trainer's `seed`, drawn by gm_gmmn_prior (gmmn.uniforms_reference is the same rule in numpy, bit for bit)
under tags of its own: TAG_T = "SWGT" (training: `step` the 0-based training batch count over the trainer's life,
`noise_steps`, saved in checkpoints; on the device ctr + nbase), TAG_V = "SWGV" (validation: `step` the batch's index
within the pass), TAG_S = "SWGS" (sample(n, seed), step 0).  The global CPU generator is touched by the loaders' shuffles
only.

Directions.  Theta [P, I], P = num_projections (default 1024, 1 to MAX_P = GM_SW_MAX_P): row p is the I normals of the
Philox stream at (seed, step, row = p, tag) -- Box-Muller pairs as in gm_philox.h -- scaled to unit 2-norm, the norm summed
in fp64 in a fixed order (groups of 64 consecutive squares, the groups in ascending order).  A row whose norm is 0 is left
at 0 (its projections are all equal, and it adds nothing to loss or gradient).  TAG_DT = "SWDT": fresh directions every
training batch, step = the batch's noise step; TAG_DV = "SWDV": step = the batch's index in the pass, so the validation
loss is a deterministic function of the weights; TAG_DM = "SWDM": metrics.sliced_wasserstein, under its own seed, step 0.
`directions_reference` below is the rule in fp64 numpy.

Loss.  Generated rows x_1..x_N, data rows y_1..y_M (N = M = b in training).  For direction p, a = X theta_p and
b = Y theta_p, each sorted ascending; the squared 2-Wasserstein distance of the two empirical measures on the line is

    W_p = (1 / (N M)) sum_ij w_ij (a_(i) - b_(j))^2,     w_ij = max(0, min((i+1) M, (j+1) N) - max(i M, j N))

over integers i in [0, N), j in [0, M): only j from floor(i M / N) to floor(((i+1) M - 1) / N) have w_ij > 0, and for
N = M it is the usual rank matching, w_ii = N.  Then

    loss = swd2 = (1/P) sum_p W_p,        d loss / d a_i = (2 / (P N M)) sum_j w_ij (a_(i) - b_(j))

stored at the row's original position, Ct[p, i];  dX = Ct^T Theta, and the gradient entering `generate` is dX times
x (1 - x).  There is no square root in the training loss; the metric reports swd2 and swd = sqrt(swd2).

Order.  Elements compare by (value, original row index) lexicographically: the sorted order is numpy's
argsort(kind="stable") and unique, so a collapsed generator (all rows equal) gives its tied rows the same partners in
every run and on every work mapping.  Padding up to a power of two compares above every real element and is never
written out.  The network is data-oblivious: a NaN among the values gives unspecified numbers, but every real index is
still written exactly once and nothing outside Ct[p, 0:N] is touched.

Numerical rules of the kernels: projections from the FP32-input MFMA GEMM (ops.linear_fwd with Theta as the row operand
and R = [X; Y] as the weight operand, so a projection's values are contiguous); a_(i) - b_(j) in fp32; its square times
w_ij accumulated in fp64 in a fixed order; the P column sums closed in fp64 in a fixed order in the finalize launch; no
atomics, one writer per element: two runs, graph against eager, and a resumed run against an uninterrupted one agree bit
for bit.

Fused path: SWGEngine below -- 13 launches per training batch, 9 per validation batch.  Training
batches of at most MAX_B = GM_SW_MAX_B rows; I <= 8192.  One GPU only: the statistic couples every row of the batch.  An
overridden compute_batch / evaluate or an edited model: the general loop -- autograd over ops.fused_linear and
ops_fused.sw_loss on the same noise."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, philox, viz
from ._lib import (GMMN_MAX_Z, MMD_MAX_I, SW_MAX_B, SW_MAX_P, SW_MAX_ROWS, SWG_TAG_DM, SWG_TAG_DT, SWG_TAG_DV, SWG_TAG_S,
                   SWG_TAG_T, SWG_TAG_V, GMError)
from .trainers import FlatAdam, Generator, OneLossTrainer, _stock_module, stock, stock_model  # noqa: F401
from .engine import VAEEngine, _align4, _Linear
from .gmmn import uniforms_reference  # noqa: F401  (the prior's rule)

TAG_T, TAG_V, TAG_S = SWG_TAG_T, SWG_TAG_V, SWG_TAG_S
TAG_DT, TAG_DV, TAG_DM = SWG_TAG_DT, SWG_TAG_DV, SWG_TAG_DM
MAX_B, MAX_P, MAX_ROWS = SW_MAX_B, SW_MAX_P, SW_MAX_ROWS
NUM_PROJECTIONS = 1024


class SWGError(GMError, ValueError):
    """A bad shape, projection count, seed, sample count or batch size: a ValueError, and a GMError like the package's
    other refusals."""


def _int(v, name):
    return _lib.check_int(v, name, SWGError)


def check_seed(seed):
    return _lib.check_seed(seed, error=SWGError)


def check_projections(P):
    P = _int(P, "num_projections")
    if not 1 <= P <= MAX_P:
        raise SWGError("num_projections must lie in [1, %d], got %d" % (MAX_P, P))
    return P


def check_shape(image_size, hidden_dim, z_dim):
    I, H, Z = _int(image_size, "image_size"), _int(hidden_dim, "hidden_dim"), _int(z_dim, "z_dim")
    if not 1 <= I <= MMD_MAX_I:
        raise SWGError("image_size must lie in [1, %d], got %d" % (MMD_MAX_I, I))
    if H < 1:
        raise SWGError("hidden_dim must be >= 1, got %d" % H)
    if not 1 <= Z <= GMMN_MAX_Z:
        raise SWGError("z_dim must lie in [1, %d], got %d" % (GMMN_MAX_Z, Z))
    return I, H, Z


def check_batch(b):
    b = _int(b, "batch size")
    if not 1 <= b <= MAX_B:
        raise SWGError("an SWG trains on batches of 1 to %d rows (a projection's (value, row) pairs are sorted in LDS), "
                       "got %d" % (MAX_B, b))
    return b


def directions_reference(P, I, seed, step, tag=TAG_DT, row0=0):
    """The unit directions [P, I] float64 of rows row0 .. at `step` under `tag`: philox.py's Box-Muller normals over the
    row's 2-norm; a row of zeros stays zero.  The device forms the normals in fp32."""
    n = philox.normals(P, I, seed, step, tag, row0)
    norm = np.sqrt((n * n).sum(axis=1, keepdims=True))
    return np.where(norm > 0, n / np.where(norm > 0, norm, 1.0), 0.0)


# ---- modules ---------------------------------------------------------------------------------------------------------
@stock_model
class SWG(nn.Module):
    """One Generator: z in (-1, 1)^Z -> relu -> sigmoid -> I pixels."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20):
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = check_shape(image_size, hidden_dim, z_dim)
        self.G = Generator(self.image_size, self.hidden_dim, self.z_dim)
        self.shape = int(self.image_size ** 0.5)

    def forward(self, z):
        return self.G(z)


def swg_fused_ok(model):
    """True iff the model is SWG itself with its Generator unchanged and consistent shapes."""
    g = getattr(model, "G", None)
    if not (type(model).__dict__.get("_gm_stock_model", False) and type(g) is Generator and _stock_module(g, 2)):
        return False
    I, H, Z = model.image_size, model.hidden_dim, model.z_dim
    return (tuple(g.linear.weight.shape) == (H, Z) and tuple(g.generate.weight.shape) == (I, H)
            and g.linear.bias is not None and g.generate.bias is not None and 1 <= I <= MMD_MAX_I
            and 1 <= Z <= GMMN_MAX_Z)


# ---- engine ----------------------------------------------------------------------------------------------------------
class SWGEngine(VAEEngine):
    """The SWG on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  Per
    training batch, 13 launches: 1. gm_gather_rows[_bits] (Y, the lower half of R);  2. gm_gmmn_prior (z);  3.-4. the two
    generator forwards (X, the upper half of R);  5. gm_sw_directions (Theta);  6. Pr = Theta R^T through ops.linear_fwd
    ([P, 2b]: a projection's values contiguous);  7. gm_sw_sort (the column sums, Ct);  8. gm_sw_finalize (the loss);
    9. dX = Ct^T Theta through ops.linear_bwd_dw without Adam;  10. the sigmoid's backward through ops.act_bwd (dA);
    11. dH = dA Wgen;  12. the two weight gradients + Adam as a pair;  13. the loss record with the counter tick.  Every
    input gradient is issued before the launch that steps the weights it reads.  A validation batch is launches 1-8
    without Ct, and the record.  The noise step of a training batch is ctr + nbase (DDPMEngine's scheme), of a
    validation batch ctr.  One GPU only."""

    has_eps = False
    one_gpu = "the SWG engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        if not swg_fused_ok(model):
            raise GMError("SWGEngine: the model is not swg.SWG with its Generator unchanged; SWGTrainer trains "
                          "such models on the general path")
        g = model.G
        self._init_flat(model, device, use_graph, [g.linear.weight, g.linear.bias, g.generate.weight, g.generate.bias])
        self._bind_trainer(trainer)                  # seed, num_projections and noise_steps are read from it
        self.L1, self.L2 = _Linear(self.fp, g.linear), _Linear(self.fp, g.generate)
        self.I, self.H, self.Z = model.image_size, model.hidden_dim, model.z_dim
        self._bufP = None

    def _alloc(self, B):
        P = check_projections(self.trainer.num_projections)
        if self._bufB == B and self._bufP == P:
            return
        from . import ops_fused as of_
        check_batch(B)
        I, H, Z = self.I, self.H, self.Z
        z = lambda *s: torch.zeros(*s, device=self.device)
        self.Rb = z(2 * B, I)                        # R = [X; Y]: a batch of b rows uses rows [0, b) and [b, 2b)
        self.Zb, self.Hg = z(B, Z), z(B, H)
        self.Theta = z(P, I)
        self.Pr = z(P, _align4(2 * B))               # row p: a_p in columns [0, b), b_p in [b, 2b)
        self.Ct = z(P, _align4(B))
        self.dX, self.dA, self.dH = z(B, I), z(B, I), z(B, H)
        self.lossf = z(1)
        self.stats = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.ws = of_.sw_workspace(P, self.device)
        self._bufB, self._bufP = B, P
        self.graphs = {}

    def _settings(self):
        t = self.trainer
        return {"num_projections": int(t.num_projections), "seed": int(t.seed)}

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        check_batch(B)
        check_projections(self.trainer.num_projections)
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: Y, z, X, the directions, the statistic (+ its gradient, the backward and Adam when
        train)."""
        from . import ops_fused as of_
        L1, L2, tr, P = self.L1, self.L2, self.trainer, self._bufP
        idx_slot = self._slot(t, 1, 0, self.R, self.B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        X, Y = self.Rb[:b], self.Rb[b:2 * b]
        ops.gather_rows(self.data, self.idx_ring.view(-1), Y, B=b, idx_slot=idx_slot, stream=st)
        of_.gmmn_prior(self.Zb, of_.sw_noise(tr.seed, TAG_T if train else TAG_V, **self._clock(t, train)), B=b, Z=self.Z,
                       stream=st)
        ops.linear_fwd(self.Zb, L1.W, L1.b, self.Hg, "relu", M=b, stream=st)
        ops.linear_fwd(self.Hg, L2.W, L2.b, X, "sigmoid", M=b, stream=st)
        of_.sw_directions(self.Theta, of_.sw_noise(tr.seed, TAG_DT if train else TAG_DV, **self._clock(t, train)),
                          stream=st)
        Pr = self.Pr[:, :2 * b]
        ops.linear_fwd(self.Theta, self.Rb[:2 * b], None, Pr, "id", stream=st)
        of_.sw_sort(Pr, b, b, self.ws, Ct=self.Ct if train else None, stream=st)
        of_.sw_finalize(P, b, b, self.ws, self.stats, loss_out=self.lossf, stream=st)
        if train:
            adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
            ops.linear_bwd_dw(self.Ct[:, :b], self.Theta, self.dX[:b], None, stream=st)
            ops.act_bwd(self.dX[:b], X, self.dA[:b], "sigmoid", stream=st)
            # dH reads the output layer's weights BEFORE the pair's Adam updates them
            ops.linear_bwd_dx(self.dA, L2.W, self.dH, below=self.Hg, epi="relu", M=b, stream=st)
            ops.linear_bwd_dw_adam_pair(dict(dA=self.dA, X=self.Hg, lin=L2, adam=adam, M=b),
                                        dict(dA=self.dH, X=self.Zb, lin=L1, adam=adam, M=b),
                                        weight_decay=self.wd, stream=st)
        of_.sum_finalize(self.lossf, 1, self.recon if train else self.vrecon, out_slot=loss_slot,
                         tick=self.ctr if self.use_graph else None, stream=st)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class SWGTrainer(OneLossTrainer):
    """Trains an SWG on the sliced Wasserstein distance and samples from it.  Histories: `losses` (one per training
    batch); the epoch line (mean training loss, validation loss); best_val_loss / best_model as the other one-loss
    trainers; checkpoints (+ num_projections, seed in the optimizer state's config, checked under strict=True, and the
    number of training batches taken, so a resumed run continues the noise streams bit for bit).  One GPU only."""
    _line = "Epoch[%d/%d], SWD Loss: %.6f, Val Loss: %.6f"
    _one_gpu = "SWGTrainer"
    _error = SWGError
    _fused_ok = staticmethod(swg_fused_ok)

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, num_projections=NUM_PROJECTIONS, seed=0):
        self.seed = check_seed(seed)                 # before anything runs
        self.num_projections = check_projections(num_projections)
        if getattr(train_iter, "batch_size", None) is not None:
            check_batch(train_iter.batch_size)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)
        self.noise_steps = 0                         # training batches taken: the next one's noise step
        self._eval_step = 0                          # batch index within an evaluate() call

    def prior(self, n, step, tag, seed=None, row0=0):
        """The prior rows [n, Z] of (seed, step, tag) on the model's device (gm_gmmn_prior)."""
        from . import ops_fused as of_
        z = torch.empty(n, self.model.z_dim, device=self._device())
        return of_.gmmn_prior(z, of_.sw_noise(self.seed if seed is None else seed, tag, step=step, row0=row0))

    def directions(self, step, tag, seed=None, P=None, row0=0):
        """The unit directions [P, I] of (seed, step, tag) on the model's device (gm_sw_directions)."""
        from . import ops_fused as of_
        th = torch.empty(self.num_projections if P is None else P, self.model.image_size, device=self._device())
        return of_.sw_directions(th, of_.sw_noise(self.seed if seed is None else seed, tag, step=step, row0=row0))

    def compute_batch(self, batch):
        """The sliced Wasserstein loss of a batch against as many samples (general path: autograd over the fused linear
        kernels and ops_fused.sw_loss; z and Theta from the contract's counter streams -- the training streams while the
        model trains, the validation ones otherwise)."""
        from . import ops_fused as of_
        x = self._flat_batch(batch)
        train, step = self._noise_step()
        z = self.prior(check_batch(x.shape[0]), step, TAG_T if train else TAG_V)
        return of_.sw_loss(self.model(z), x, self.directions(step, TAG_DT if train else TAG_DV))

    def _engine_class(self):
        import functools
        return functools.partial(SWGEngine, trainer=self)

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
            raise SWGError("n must be >= 1, got %d" % n)
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
        raise GMError("an SWG has no likelihood and no encoder; parzen(), mmd() and swd() score its samples")

    def reconstruct_images(self, images, epoch, save=True):
        raise GMError("an SWG has no encoder")

    def viz_loss(self):
        viz.one_loss_curve(self, "SWD loss")


__all__ = ["Generator", "SWG", "SWGTrainer", "SWGEngine", "SWGError", "directions_reference", "uniforms_reference",
           "check_projections", "check_batch", "check_seed", "check_shape", "swg_fused_ok", "NUM_PROJECTIONS", "MAX_B",
           "MAX_P", "MAX_ROWS", "TAG_T", "TAG_V", "TAG_S", "TAG_DT", "TAG_DV", "TAG_DM", "FlatAdam"]
