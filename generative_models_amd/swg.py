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

from . import _lib, ops, philox, viz
from ._lib import (SW_MAX_B, SW_MAX_P, SW_MAX_ROWS, SWG_TAG_DM, SWG_TAG_DT, SWG_TAG_DV, SWG_TAG_S, SWG_TAG_T, SWG_TAG_V,
                   GMError)
from .trainers import FlatAdam, Generator, stock, stock_model  # noqa: F401
from .engine import GeneratorMatchEngine, _align4
from .gmmn import GeneratorMatchTrainer, GeneratorModel, generator_fused_ok, generator_shape
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
    return generator_shape(image_size, hidden_dim, z_dim, SWGError)


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
class SWG(GeneratorModel):
    """One Generator: z in (-1, 1)^Z -> relu -> sigmoid -> I pixels."""
    _error = SWGError


swg_fused_ok = generator_fused_ok


# ---- engine ----------------------------------------------------------------------------------------------------------
class SWGEngine(GeneratorMatchEngine):
    """The SWG on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  Per
    training batch, 13 launches: 1. gm_gather_rows[_bits] (Y, the lower half of R);  2. gm_gmmn_prior (z);  3.-4. the two
    generator forwards (X, the upper half of R);  5. gm_sw_directions (Theta);  6. Pr = Theta R^T through ops.linear_fwd
    ([P, 2b]: a projection's values contiguous);  7. gm_sw_sort (the column sums, Ct);  8. gm_sw_finalize (the loss);
    9. dX = Ct^T Theta through ops.linear_bwd_dw without Adam;  10. the sigmoid's backward through ops.act_bwd (dA);
    11. dH = dA Wgen;  12. the two weight gradients + Adam as a pair;  13. the loss record with the counter tick.  Every
    input gradient is issued before the launch that steps the weights it reads.  A validation batch is launches 1-8
    without Ct, and the record.  The noise step of a training batch is ctr + nbase (DDPMEngine's scheme), of a
    validation batch ctr.  One GPU only."""

    one_gpu = "the SWG engine"
    fused_ok = staticmethod(swg_fused_ok)
    refusal = ("SWG", "swg.SWG", "Generator")        # the trainer: seed, num_projections and noise_steps
    noise_builder, tags = "sw_noise", (TAG_T, TAG_V)
    _bufP = None

    def _alloc_key(self, B):
        return B, check_projections(self.trainer.num_projections)

    def _buffers(self, B):
        from . import ops_fused as of_
        check_batch(B)
        I, H, Z, P = self.I, self.H, self.Z, int(self.trainer.num_projections)
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
        self._bufP = P

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
        tr, P = self.trainer, self._bufP
        X, Y = self._forward(st, t, b, train)
        of_.sw_directions(self.Theta, of_.sw_noise(tr.seed, TAG_DT if train else TAG_DV, **self._clock(t, train)),
                          stream=st)
        Pr = self.Pr[:, :2 * b]
        ops.linear_fwd(self.Theta, self.Rb[:2 * b], None, Pr, "id", stream=st)
        of_.sw_sort(Pr, b, b, self.ws, Ct=self.Ct if train else None, stream=st)
        of_.sw_finalize(P, b, b, self.ws, self.stats, loss_out=self.lossf, stream=st)
        if train:
            ops.linear_bwd_dw(self.Ct[:, :b], self.Theta, self.dX[:b], None, stream=st)
            ops.act_bwd(self.dX[:b], X, self.dA[:b], "sigmoid", stream=st)
        self._tail(st, t, b, train)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class SWGTrainer(GeneratorMatchTrainer):
    """Trains an SWG on the sliced Wasserstein distance and samples from it.  Histories: `losses` (one per training
    batch); the epoch line (mean training loss, validation loss); best_val_loss / best_model as the other one-loss
    trainers; checkpoints (+ num_projections, seed in the optimizer state's config, checked under strict=True, and the
    number of training batches taken, so a resumed run continues the noise streams bit for bit).  One GPU only."""
    _line = "Epoch[%d/%d], SWD Loss: %.6f, Val Loss: %.6f"
    _one_gpu = "SWGTrainer"
    _error = SWGError
    _fused_ok = staticmethod(swg_fused_ok)
    _engine_type = SWGEngine
    _check_batch = staticmethod(check_batch)
    _noise_builder, _tag_sample = "sw_noise", TAG_S
    _no_likelihood = "an SWG has no likelihood and no encoder; parzen(), mmd() and swd() score its samples"
    _no_encoder = "an SWG has no encoder"

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, num_projections=NUM_PROJECTIONS, seed=0):
        self.seed = check_seed(seed)                 # before anything runs
        self.num_projections = check_projections(num_projections)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)

    def directions(self, step, tag, seed=None, P=None, row0=0):
        """The unit directions [P, I] of (seed, step, tag) on the model's device (gm_sw_directions)."""
        from . import ops_fused as of_
        th = torch.empty(self.num_projections if P is None else P, self.model.image_size, device=self._device())
        return of_.sw_directions(th, self._noise(seed, tag, step, row0))

    def compute_batch(self, batch):
        """The sliced Wasserstein loss of a batch against as many samples (general path: autograd over the fused linear
        kernels and ops_fused.sw_loss; z and Theta from the contract's counter streams -- the training streams while the
        model trains, the validation ones otherwise)."""
        from . import ops_fused as of_
        x = self._flat_batch(batch)
        train, step = self._noise_step()
        z = self.prior(check_batch(x.shape[0]), step, TAG_T if train else TAG_V)
        return of_.sw_loss(self.model(z), x, self.directions(step, TAG_DT if train else TAG_DV))

    def viz_loss(self):
        viz.one_loss_curve(self, "SWD loss")


__all__ = ["Generator", "SWG", "SWGTrainer", "SWGEngine", "SWGError", "directions_reference", "uniforms_reference",
           "check_projections", "check_batch", "check_seed", "check_shape", "swg_fused_ok", "NUM_PROJECTIONS", "MAX_B",
           "MAX_P", "MAX_ROWS", "TAG_T", "TAG_V", "TAG_S", "TAG_DT", "TAG_DV", "TAG_DM", "FlatAdam"]
