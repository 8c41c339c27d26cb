"""Flow matching / rectified flow (Lipman et al., "Flow Matching for Generative Modeling", arXiv 2210.02747; Liu, Gong &
Liu, "Flow Straight and Fast", arXiv 2209.03003): a continuous normalizing flow (CNF) on the collection's MLPs, trained by
regressing a velocity field on the straight path between noise and data, sampled by an ODE solver, and scored with the
EXACT divergence of the field.  Exported by src/flow_matching.py as VelocityField / FlowMatching / FlowMatchingTrainer.

The contract.

Model.  FlowMatching(image_size I = 784, hidden_dim H = 400, time_dim E = 32, T = 1000) holds one VelocityField `field`:
linear = Linear(I + E, H), hidden = Linear(H, H), out = Linear(H, I);   v(y, t_j) = out(relu(hidden(relu(linear(cat[y,
temb[j]]))))) (the Denoiser's shape).  out.weight and out.bias are zero at construction: a fresh model is the identity
flow.  Limits: 1 <= I <= 8192, 1 <= H <= 1024, E a multiple of 4 in [4, 128], 2 <= T <= 4096; anything else raises
FlowMatchError(GMError, ValueError) in the constructor.

Time grid.  Time lives on the grid t_j = j / T, j = 0 .. T.  Tables (built on the host in fp64, rounded once to fp32,
non-persistent buffers: no device transcendental is part of the contract):  tt[j] = j / T;  tc[j] = (T - j) / T;
temb[j] = [sin(1000 t_j f_i) | cos(1000 t_j f_i)], f_i = exp(-ln(1e4) i / (E/2)) (the DDPM's frequencies).

Preprocessing is realnvp.preprocess unchanged: dequantise with `levels`, logit with `alpha` (both the trainer's settings,
as in MAFTrainer).  The device's element function is nvp_pre_elem of csrc/gm_nvp.h, so y1 and logdet_pre are gm_nvp_pre's
bits.

Path and loss (the optimal-transport / rectified path).  y0 ~ N(0, 1), y1 the preprocessed image:
  y_t = fmaf(tt[j], y1, tc[j] * y0)  (j = 0 gives y0 and j = T gives y1 exactly);   target u = y1 - y0;
  loss = sum (v - u)^2 / (b I) per batch (gm_ddpm_loss with eps := u);  d loss / d v = 2 (v - u) / (b I).

Noise.  Philox4x32-10 with key (seed mod 2^32, seed >> 32), batch row `row` at batch `step`:
  dequantisation uniform of pixel e: ph_unit of word e & 3 of counter (e >> 2, step, row, TAG_D) (RealNVP's indexing);
  j = mulhi(word 0 of counter (0, step, row, TAG_T), T + 1) -- integer arithmetic, bit-identical in numpy;
  y0 of pixels 4q .. 4q + 3: the Box-Muller normals of counter (q, step, row, TAG_N).
Training: TAG_D = "FMTD", TAG_T = "FMTT", TAG_N = "FMTN", `step` the 0-based training batch count over the trainer's
life (`noise_steps`, saved in checkpoints), `row` the row's position in the whole batch.  Validation, encode and
log_likelihood: "FMVD", "FMVT", "FMVN", `step` the batch's index within the pass.  The sampler's prior is
gm_nvp_post's PRIOR mode (the flows' stream "NVPS", indexed by row and element), reused as MAFTrainer uses it.  The
global CPU generator is touched by the loaders' shuffles only.

Solvers.  "euler", "heun" and "rk4" with their classical tableaus (every a sub-diagonal: a stage reads the previous
stage only), `steps` uniform steps in direction +1 (0 -> 1: sample, decode) or -1 (1 -> 0: encode, likelihood).  Every
evaluation time is a grid point: steps must divide T for euler and heun, 2 steps must divide T for rk4, else
FlowMatchError.  ode_table(T, steps, solver, direction) -> [n_eval, 8] fp64 rows (h a, h b, first, last, j_next or -1,
j_eval, 0, 0), indexed on the device by a device counter.

Stage rule (csrc/gm_fm.h fm_stage1, every rounding pinned).  With k the field at this evaluation:
  Acc = first ? hb k : fmaf(hb, k, Acc);   last stage of a step: Base += Acc, y = Base;   else y = fmaf(ha, k, Base);
the row's log-determinant pair (LBase, LAcc) follows the same rule with the divergence d; the tail of the next input
row becomes temb[j_next].

Likelihood.  For this field div_y v = tr(W3 D2 W2 D1 W1y) = m2^T Q m1 with Q[i, j] = W2[i, j] (W1y W3)[j, i], W1y =
W1[:, :I], m1 = [H1 > 0], m2 = [H2 > 0] the ReLU patterns of the forward pass that has just run (relu'(0) = 0: -0.0 and
0.0 are not lit, the backward GEMMs' convention).  Q is formed once per call; gm_fm_div evaluates the bilinear form on
the FP32 MFMAs.  Integrate 1 -> 0 from y1: z = y(0), l = LBase = integral_1^0 div dt;
  nll = 0.5 sum z^2 + 0.5 I log 2 pi - logdet_pre - l + I log(levels)   (gm_nvp_loss with logdet = logdet_pre + l).
This is the likelihood of the CONTINUOUS flow to the solver's accuracy, not of the discrete map the solver computes:
the divergence is exact at every evaluation, the time integral is not.  Compare two values of `steps`.

Fused path: FlowMatchEngine below -- 10 launches per training batch (gather + path sample, three forwards, the loss,
two input gradients, the out / hidden weight gradients as a pair with Adam, the first layer's weight gradient with Adam,
the loss sum with the counter tick), 5 per validation batch; a field evaluation of the solver is three forwards and
gm_fm_stage (4 launches), under the likelihood three forwards, gm_fm_div and gm_fm_stage (5).  An overridden
compute_batch / evaluate or an edited model: the general loop -- autograd over ops.fused_linear on gm_fm_qsample's
rows."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, philox, realnvp
from ._lib import (DDPM_MAX_E, DDPM_MAX_I, DDPM_MAX_T, DDPM_MIN_E, FM_MAX_H, FM_TAG_D, FM_TAG_N, FM_TAG_T, FM_TAG_VD,
                   FM_TAG_VN, FM_TAG_VT, GMError)
from .trainers import FlatAdam, _dataset_rows, _lin, _stock_module, stock, stock_model  # noqa: F401
from .engine import TimeRegressionEngine, _align4
from .realnvp import nll_constant, nll_rows, postprocess, preprocess  # noqa: F401

TAG_D, TAG_T, TAG_N, TAG_VD, TAG_VT, TAG_VN = FM_TAG_D, FM_TAG_T, FM_TAG_N, FM_TAG_VD, FM_TAG_VT, FM_TAG_VN
GRAPH_EVALS = 32                 # field evaluations per captured graph, at most
TIME_SCALE = 1000.0              # the embedding's argument is 1000 t_j: the DDPM's range of timesteps
# solver -> (a of the sub-diagonal, b, c): stage i + 1 is evaluated at Base + h a[i] k_i, time t + c[i + 1] h
TABLEAUS = {
    "euler": ((), (1.0,), (0.0,)),
    "heun": ((1.0,), (0.5, 0.5), (0.0, 1.0)),
    "rk4": ((0.5, 0.5, 1.0), (1.0 / 6.0, 1.0 / 3.0, 1.0 / 3.0, 1.0 / 6.0), (0.0, 0.5, 0.5, 1.0)),
}
SOLVERS = tuple(TABLEAUS)


class FlowMatchError(GMError, ValueError):
    """A bad image size, width, time_dim, T, alpha, levels, seed, n, temperature, steps or solver: a ValueError, and a
    GMError like the package's other refusals."""


def _int(v, name):
    return _lib.check_int(v, name, FlowMatchError)


def check_seed(seed):
    return _lib.check_seed(seed, error=FlowMatchError)


def check_shape(image_size, hidden_dim, time_dim, T):
    """(I, H, E, T) validated against the kernels' limits; else FlowMatchError."""
    I, H = _int(image_size, "image_size"), _int(hidden_dim, "hidden_dim")
    E, T = _int(time_dim, "time_dim"), _int(T, "T")
    if not 1 <= I <= DDPM_MAX_I:
        raise FlowMatchError("image_size must lie in [1, %d], got %d" % (DDPM_MAX_I, I))
    if not 1 <= H <= FM_MAX_H:
        raise FlowMatchError("hidden_dim must lie in [1, %d], got %d" % (FM_MAX_H, H))
    if not (DDPM_MIN_E <= E <= DDPM_MAX_E and E % 4 == 0):
        raise FlowMatchError("time_dim must be a multiple of 4 in [%d, %d], got %d" % (DDPM_MIN_E, DDPM_MAX_E, E))
    if not 2 <= T <= DDPM_MAX_T:
        raise FlowMatchError("T must lie in [2, %d], got %d" % (DDPM_MAX_T, T))
    return I, H, E, T


def check_settings(alpha, levels):
    """(alpha, levels) validated against gm_nvp_pre's limits; else FlowMatchError."""
    return realnvp.check_flow_settings(alpha, levels, 1.0, FlowMatchError)[:2]


def check_solver(T, steps, solver):
    """(steps, solver) validated: a known solver whose every evaluation time is a grid point; else FlowMatchError."""
    steps = _int(steps, "steps")
    if not isinstance(solver, str) or solver not in TABLEAUS:
        raise FlowMatchError("solver must be one of %s, got %r" % (SOLVERS, solver))
    if steps < 1:
        raise FlowMatchError("steps must be >= 1, got %d" % steps)
    need = 2 * steps if solver == "rk4" else steps
    if T % need != 0:
        raise FlowMatchError("%s needs %s to divide T = %d (every evaluation time is a grid point), got steps = %d"
                             % (solver, "2 steps" if solver == "rk4" else "steps", T, steps))
    return steps, solver


# ---- the tables and the rule in numpy and fp64 (the tests' reference; a CPU reading of what the device computes) -----
def tables(T, E):
    """The grid tables in fp64: dict(tt, tc [T + 1], temb [T + 1, E])."""
    j = np.arange(T + 1, dtype=np.float64)
    f = np.exp(-math.log(1e4) * np.arange(E // 2, dtype=np.float64) / (E // 2))
    arg = (TIME_SCALE * j / T)[:, None] * f[None, :]
    return {"tt": j / T, "tc": (T - j) / T, "temb": np.concatenate([np.sin(arg), np.cos(arg)], axis=1)}


def ode_table(T, steps, solver="heun", direction=1):
    """coef [n_eval, 8] float64, n_eval = steps * stages: rows (h a, h b, first, last, j_next or -1, j_eval, 0, 0) of
    `steps` uniform steps from t = 0 to 1 (direction +1) or from 1 to 0 (-1); h = direction / steps."""
    steps, solver = check_solver(T, steps, solver)
    if direction not in (1, -1):
        raise FlowMatchError("direction must be +1 or -1, got %r" % (direction,))
    a, b, c = TABLEAUS[solver]
    ns = len(b)
    h = float(direction) / steps
    span = T // steps
    js = []
    for n in range(steps):
        j0 = n * span if direction == 1 else T - n * span
        for i in range(ns):
            off = c[i] * span
            assert off == int(off)
            js.append(j0 + direction * int(off))
    coef = np.zeros((steps * ns, 8), dtype=np.float64)
    for r in range(steps * ns):
        i = r % ns
        last = i == ns - 1
        coef[r] = (0.0 if last else h * a[i], h * b[i], float(i == 0), float(last),
                   -1.0 if r == steps * ns - 1 else float(js[r + 1]), float(js[r]), 0.0, 0.0)
    return coef


def grid_index_reference(n_rows, T, seed, step, tag=TAG_T, row0=0):
    """j [n_rows] int64 of batch rows row0 .. at `step`: mulhi(word 0 of counter (0, step, row, tag), T + 1)."""
    w = philox.words(n_rows, 1, seed, step, tag, row0)[:, 0].astype(np.uint64)
    return ((w * np.uint64(T + 1)) >> np.uint64(32)).astype(np.int64)


def uniforms_reference(n, I, seed, step, tag=TAG_D, row0=0):
    """u [n, I] float32: the dequantisation noise by the contract's rule, bit for bit."""
    return philox.unit_uniforms(philox.words(n, I, seed, step, tag, row0))


def normals_reference(n, I, seed, step, tag=TAG_N, row0=0):
    """y0 [n, I] float64 by the contract's rule (the device rounds to fp32)."""
    return philox.normals(n, I, seed, step, tag, row0)


def path_reference(y1, y0, j, T):
    """(y_t, u) in fp32 numpy exactly as the device forms them from fp32 y1, y0 [n, I] and j [n]: y_t = fmaf(tt, y1,
    tc * y0) -- the product rounded to fp32, the fused multiply-add evaluated in fp64 and rounded once (exact: a
    product of two fp32 values and an fp32 addend fit fp64's 53 bits up to one rounding) -- and u = y1 - y0."""
    tab = tables(T, 4)
    tt = tab["tt"].astype(np.float32)[j][:, None]
    tc = tab["tc"].astype(np.float32)[j][:, None]
    y1, y0 = np.asarray(y1, np.float32), np.asarray(y0, np.float32)
    p = (tc * y0).astype(np.float32)
    yt = (tt.astype(np.float64) * y1.astype(np.float64) + p.astype(np.float64)).astype(np.float32)
    return yt, (y1 - y0).astype(np.float32)


def divergence_matrix(W1, W2, W3, I):
    """Q [H, H] with div_y v = m2^T Q m1:  Q[i, j] = W2[i, j] (W1[:, :I] W3)[j, i]  (torch tensors, any dtype)."""
    return W2 * (W1[:, :I] @ W3).t()


# ---- modules ---------------------------------------------------------------------------------------------------------
@stock_model
class VelocityField(nn.Module):
    """v: [y | temb[j]] (I + E wide) -> relu -> relu -> I, `out` starting at zero."""

    def __init__(self, image_size, hidden_dim, time_dim):
        super().__init__()
        self.linear = nn.Linear(image_size + time_dim, hidden_dim)
        self.hidden = nn.Linear(hidden_dim, hidden_dim)
        self.out = nn.Linear(hidden_dim, image_size)
        with torch.no_grad():
            self.out.weight.zero_()
            self.out.bias.zero_()

    def forward(self, xin):
        return _lin(self.out, _lin(self.hidden, _lin(self.linear, xin, "relu"), "relu"), "id")


@stock_model
class FlowMatching(nn.Module):
    """One VelocityField and the grid tables (non-persistent buffers: state_dict holds the field's six tensors)."""

    def __init__(self, image_size=784, hidden_dim=400, time_dim=32, T=1000):
        super().__init__()
        self.image_size, self.hidden_dim, self.time_dim, self.T = check_shape(image_size, hidden_dim, time_dim, T)
        self.field = VelocityField(self.image_size, self.hidden_dim, self.time_dim)
        self.shape = int(self.image_size ** 0.5)
        for name, v in tables(self.T, self.time_dim).items():
            self.register_buffer(name, torch.from_numpy(v.astype(np.float32)), persistent=False)

    def forward(self, y, j):
        """v(y, t_j): y [n, I] in logit space, j [n] integer grid indices in [0, T]."""
        return self.field(torch.cat([y, self.temb[j.long()]], dim=1).contiguous())


def flowmatch_fused_ok(model):
    """True iff the model is FlowMatching itself with its VelocityField unchanged and consistent shapes."""
    f = getattr(model, "field", None)
    if not (type(model).__dict__.get("_gm_stock_model", False) and type(model) is FlowMatching
            and type(f) is VelocityField and _stock_module(f, 3)):
        return False
    if not all(isinstance(getattr(model, n, None), torch.Tensor) for n in ("tt", "tc", "temb")):
        return False
    try:
        I, H, E, T = check_shape(model.image_size, model.hidden_dim, model.time_dim, model.T)
    except (FlowMatchError, AttributeError):
        return False
    return (tuple(f.linear.weight.shape) == (H, I + E) and tuple(f.hidden.weight.shape) == (H, H)
            and tuple(f.out.weight.shape) == (I, H) and tuple(model.temb.shape) == (T + 1, E)
            and model.tt.numel() == T + 1 and model.tc.numel() == T + 1
            and all(l.bias is not None for l in (f.linear, f.hidden, f.out)))


# ---- engine ----------------------------------------------------------------------------------------------------------
class FlowMatchEngine(TimeRegressionEngine):
    """Flow matching on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter), the
    DDPM engine's launch shape.  Per training batch, 10 launches: 1. gm_gather_rows[_bits]_fm_qsample (clean rows,
    [y_t | temb[j]], u, logdet_pre, j);  2.-4. the three forwards;  5. gm_ddpm_loss with eps := u (dA, row partials);
    6. dH2 = dA Wout [H2 > 0];  7. dH1 = dH2 Whid [H1 > 0];  8. the out / hidden weight gradients + Adam as a pair;  9. the
    first layer's weight gradient + Adam;  10. the loss sum with the counter tick.  Every input gradient is issued
    before the launch that steps the weights it reads.  A validation batch is launches 1-5 (no dA) and the sum.  The
    noise step of a training batch is ctr + nbase (a device word configure() writes from the trainer's count of
    training batches, so the step is never baked into a graph), of a validation batch ctr (the batch's index in the
    pass).  One GPU only."""

    one_gpu = "the flow-matching engine"
    fused_ok = staticmethod(flowmatch_fused_ok)
    refusal = ("FlowMatch", "flowmatch.FlowMatching", "VelocityField")   # the trainer: seed, alpha, levels, noise_steps
    net, tables = "field", ("tt", "tc", "temb")
    table_builder, noise_builder = "fm_tables", "fm_noise"
    target, steps, rows = "U", "jq", ("logdet",)

    def _settings(self):
        m, tr = self.model, self.trainer
        return {"T": int(m.T), "time_dim": int(m.time_dim), "alpha": float(tr.alpha), "levels": int(tr.levels),
                "seed": int(tr.seed)}

    def _gather_sample(self, st, b, noise, idx_slot):
        from . import ops_fused as of_
        tr = self.trainer
        of_.gather_rows_fm_qsample(self.data, self.idx_ring.view(-1), self.X, self.Xin_full, self.U, self.logdet,
                                   self.jq, noise, self.tab, tr.alpha, tr.levels, B=b, idx_slot=idx_slot, stream=st)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class FlowMatchTrainer(realnvp.DequantFlowTrainer):
    """Trains a FlowMatching model on the velocity regression and samples, encodes, decodes and scores with an ODE
    solver: a DequantFlowTrainer whose code is z itself, whose alpha and levels are the trainer's (as MAFTrainer's) and
    whose training loss is the regression loss, not the NLL.  Histories: `losses` (one per training batch); the epoch
    line (mean training loss, validation loss); best_val_loss / best_model as the other VAE-family trainers;
    checkpoints (+ T, time_dim, alpha, levels, seed in the optimizer state's config, checked under strict=True, and the
    number of training batches taken, so a resumed run continues the noise stream bit for bit).  log_likelihood is the
    likelihood of the continuous flow to the solver's accuracy (the module's docstring): compare two values of
    `steps`.  One GPU only."""
    _line = "Epoch[%d/%d], Loss: %.6f, Val Loss: %.6f"
    _one_gpu = "FlowMatchTrainer"
    _error = FlowMatchError
    _fused_ok = staticmethod(flowmatch_fused_ok)
    _tag_train, _tag_eval = TAG_D, TAG_VD

    def __init__(self, model, train_iter, val_iter, test_iter, seed=0, alpha=0.05, levels=256, viz=False):
        self.seed = check_seed(seed)                 # both before anything runs, the seed's refusal first
        self.alpha, self.levels = check_settings(alpha, levels)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz, seed=self.seed)
        self._solver = {}

    def _settings_ok(self):
        try:
            check_settings(self.alpha, self.levels)
            return True
        except FlowMatchError:
            return False

    def _stock(self):
        return super()._stock() and self._settings_ok()

    def _flow_settings(self):
        return self.alpha, self.levels, 1.0

    def _tables(self):
        from . import ops_fused as of_
        m = self.model
        return of_.fm_tables(m.tt, m.tc, m.temb)

    def compute_batch(self, batch):
        """The regression loss of a batch (general path: autograd over the fused linear kernels; y_t, u and j from
        gm_fm_qsample on the contract's counter stream -- the training stream while the model trains, the validation
        one otherwise)."""
        from . import ops_fused as of_
        x = self._flat_batch(batch)
        train, step = self._noise_step()
        xin, u, _ld, _j = of_.fm_qsample(x, of_.fm_noise(self.seed, train, step=step), self._tables(), self.alpha,
                                         self.levels)
        out = self.model.field(xin)
        return torch.sum((u - out) ** 2) / (x.shape[0] * x.shape[1])

    def _engine_class(self):
        return FlowMatchEngine

    def train(self, num_epochs, lr=1e-3, weight_decay=0.0, quiet=False):
        """VAETrainer.train with this model's defaults."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    # ---- the field and its divergence as ops ---------------------------------------------------------------------------
    def _weights(self):
        f = self.model.field
        return [p.detach() for p in (f.linear.weight, f.linear.bias, f.hidden.weight, f.hidden.bias, f.out.weight,
                                     f.out.bias)]

    def divergence_matrix(self):
        """Q [H, H] float32 on the device from the current weights: P = W1y W3 through ops.linear_fwd on a transposed
        copy of out.weight, then one elementwise product with hidden.weight."""
        m = self.model
        w = self._weights()
        I, H = m.image_size, m.hidden_dim
        P = torch.empty(H, H, device=w[0].device)
        ops.linear_fwd(w[0][:, :I], w[4].t().contiguous(), torch.zeros(H, device=w[0].device), P, "id")
        return (w[2] * P.t()).contiguous()

    def _field_rows(self, y, j):
        m = self.model
        y = y.reshape(y.shape[0], -1)
        if y.shape[1] != m.image_size:
            raise FlowMatchError("rows have %d elements, the model %d" % (y.shape[1], m.image_size))
        y = y.to(self._device(), torch.float32)
        if torch.is_tensor(j):
            j = j.to(y.device).long().reshape(-1)
        else:
            j = torch.full((y.shape[0],), _int(j, "j"), dtype=torch.int64, device=y.device)
        if j.numel() != y.shape[0] or int(j.min()) < 0 or int(j.max()) > m.T:
            raise FlowMatchError("j must hold one grid index in [0, T = %d] per row" % m.T)
        return torch.cat([y, m.temb[j]], dim=1).contiguous()

    def velocity(self, y, j):
        """v(y, t_j) [n, I] of logit-space rows y at grid index j (an integer or one per row)."""
        xin = self._field_rows(y, j)
        with torch.no_grad():
            return self.model.field(xin).contiguous()

    def divergence(self, y, j):
        """div_y v(y, t_j) [n], exact: two forwards and gm_fm_div on their ReLU patterns (a stock model only)."""
        from . import ops_fused as of_
        if not flowmatch_fused_ok(self.model):
            raise GMError("divergence needs flowmatch.FlowMatching with its VelocityField unchanged")
        xin = self._field_rows(y, j)
        w, n, H = self._weights(), xin.shape[0], self.model.hidden_dim
        H1, H2 = torch.empty(n, H, device=xin.device), torch.empty(n, H, device=xin.device)
        ops.linear_fwd(xin, w[0], w[1], H1, "relu")
        ops.linear_fwd(H1, w[2], w[3], H2, "relu")
        return of_.fm_div(H1, H2, self.divergence_matrix())

    # ---- the solver ------------------------------------------------------------------------------------------------------
    def _solve(self, y, direction, steps, solver, with_div=False, return_trajectory=False):
        """(y_end [n, I], l [n] or None, trajectory or None): `steps` steps of `solver` from the device rows y in
        `direction`, l the integral of the divergence along the way.  A stock model replays a hipGraph of G <= 32 field
        evaluations n_eval / G times over a device counter (use_graph = False: launch by launch, same bits)."""
        from . import ops_fused as of_
        m = self.model
        coef64 = ode_table(m.T, steps, solver, direction)
        S, stages = coef64.shape[0], len(TABLEAUS[solver][1])
        n, dev = y.shape[0], y.device
        I, E, H = m.image_size, m.time_dim, m.hidden_dim
        fused = flowmatch_fused_ok(m)
        if with_div and not fused:
            raise GMError("the likelihood needs flowmatch.FlowMatching with its VelocityField unchanged (the exact "
                          "divergence is that field's)")
        c = self._solver
        if c.get("n") != n or c.get("dev") != dev:
            z = lambda *s: torch.empty(*s, device=dev)
            c.clear()
            c.update(n=n, dev=dev, Xin=z(n, _align4(I + E)), H1=z(n, H), H2=z(n, H), Out=z(n, I), Base=z(n, I),
                     Acc=z(n, I), L=z(n, 2), part=z(of_.fm_div_tiles(H), n), Q=z(H, H),
                     ctr=torch.zeros(1, dtype=torch.int64, device=dev),
                     done=torch.zeros(1, dtype=torch.int32, device=dev), coef={}, graph=None)
        Xin_full = c["Xin"]
        Xin = Xin_full[:, :I + E]
        ck = (S, solver, direction)
        if ck not in c["coef"]:
            c["coef"][ck] = torch.empty(S, 8, device=dev)
        coef = c["coef"][ck]
        coef.copy_(torch.from_numpy(coef64.astype(np.float32)))
        Xin_full[:, :I].copy_(y)
        Xin_full[:, I:I + E].copy_(m.temb[int(coef64[0, 5])].expand(n, E))
        c["Base"].copy_(y)
        c["L"].zero_()
        traj = None
        if return_trajectory:
            traj = torch.empty(steps + 1, n, I, device=dev)
            traj[0].copy_(y)
        w = self._weights() if fused else None
        Q = c["Q"]                                   # one buffer, so that the likelihood's graph can be kept as well
        if with_div:
            Q.copy_(self.divergence_matrix())
        tiles = of_.fm_div_tiles(H)

        def step(st, slot=None, s=0, tick=None):
            if fused:
                ops.linear_fwd(Xin, w[0], w[1], c["H1"], "relu", stream=st)
                ops.linear_fwd(c["H1"], w[2], w[3], c["H2"], "relu", stream=st)
                ops.linear_fwd(c["H2"], w[4], w[5], c["Out"], "id", stream=st)
                out = c["Out"]
            else:
                with torch.no_grad():
                    out = m.field(Xin.contiguous()).contiguous()
            part = None
            if with_div:
                part = of_.fm_div(c["H1"], c["H2"], Q, part=c["part"], finish=False, stream=st)
            of_.fm_stage(out, c["Base"], c["Acc"], Xin_full, coef, m.temb, I, stages, L=c["L"], div=part,
                         div_parts=tiles, slot=slot, step=s, traj=traj, tick=tick,
                         done=c["done"] if tick is not None else None, stream=st)

        torch.cuda.synchronize()
        if fused and self.use_graph:
            G = max(g for g in range(1, min(S, GRAPH_EVALS) + 1) if S % g == 0)
            key = (S, G, solver, direction, bool(with_div), coef.data_ptr(), m.temb.data_ptr(), Q.data_ptr()) \
                + tuple(t.data_ptr() for t in w)
            c["ctr"].zero_()
            c["done"].zero_()
            if traj is not None or c["graph"] is None or c["graph"][0] != key:
                slot = ops.slot(c["ctr"].data_ptr(), 1, 0, 0, 8)
                g = ops.Graph().capture(lambda st: [step(st, slot=slot, tick=c["ctr"]) for _ in range(G)])
                if traj is None:
                    c["graph"] = (key, g)
            else:
                g = c["graph"][1]
            for _ in range(S // G):
                g.launch()
        else:
            for s in range(S):
                step(None, s=s)
        torch.cuda.synchronize()
        return c["Base"].clone(), (c["L"][:, 0].clone() if with_div else None), traj

    def _check_n(self, n, seed, temperature):
        E = FlowMatchError
        n, seed = _lib.check_int(n, "n", E), check_seed(seed)
        temperature = _lib.check_real(temperature, "temperature", E)
        if not 1 <= n < 1 << 31:
            raise E("n must lie in [1, 2^31), got %d" % n)
        if temperature < 0.0:
            raise E("temperature must be >= 0, got %r" % temperature)
        return n, seed, temperature

    def _prior(self, n, seed, temperature):
        """The sampler's starting normals z [n, I]: gm_nvp_post's PRIOR mode under the HALF split."""
        from . import ops_fused as of_
        I = self.model.image_size
        z = torch.empty(n, I, device=self._device())
        of_.nvp_prior(*of_.maf_halves(z, I), n, I, seed, "half", temperature=temperature)
        return z

    def _post(self, y):
        """x [n, I] in [0, 1] of logit-space rows: gm_nvp_post."""
        from . import ops_fused as of_
        I = self.model.image_size
        x = torch.empty(y.shape[0], I, device=y.device)
        of_.nvp_post(*of_.maf_halves(y, I), x, y.shape[0], self.alpha, "half")
        return x

    def sample(self, n, seed=0, temperature=1.0, steps=50, solver="heun", return_trajectory=False):
        """n samples [n, I] float32 in [0, 1]: the prior's normals (indexed by row and element: rows 0 .. 4 of
        sample(300) are sample(5)) times the temperature, integrated 0 -> 1, then gm_nvp_post.  return_trajectory:
        (samples, trajectory [steps + 1, n, I]) in logit space, y(0) first.  The global generator, the model's mode and
        the parameters are untouched."""
        n, seed, temperature = self._check_n(n, seed, temperature)
        steps, solver = check_solver(self.model.T, steps, solver)
        self._device()
        torch.cuda.synchronize()
        y, _l, traj = self._solve(self._prior(n, seed, temperature), 1, steps, solver,
                                  return_trajectory=return_trajectory)
        x = self._post(y)
        torch.cuda.synchronize()
        return (x, traj) if return_trajectory else x

    def _forward_rows(self, x, seed, tag, step, row0=0, steps=100, solver="rk4"):
        """(z [n, I], nll [n]) of device rows x under the dequantisation noise of (seed, tag, step, row0 ..):
        gm_nvp_pre, the solver 1 -> 0 with the divergence, gm_nvp_loss."""
        from . import ops_fused as of_
        I, n = self.model.image_size, x.shape[0]
        y1, logdet = torch.empty(n, I, device=x.device), torch.empty(n, device=x.device)
        of_.nvp_pre(x, *of_.maf_halves(y1, I), logdet, n, seed, tag, self.alpha, self.levels, "half", step=step,
                    row0=row0)
        z, l, _ = self._solve(y1, -1, steps, solver, with_div=True)
        part = torch.empty(n, device=x.device)
        of_.nvp_loss(*of_.maf_halves(z, I), logdet + l, part, n, float(np.float32(nll_constant(I, self.levels))))
        return z, part

    def _inverse_rows(self, z, steps=100, solver="rk4"):
        return self._post(self._solve(z, 1, steps, solver)[0])

    def encode(self, images, seed=0, batch=1024, steps=100, solver="rk4"):
        """(z [n, I], log_px [n]): y(0) of every image's y1 under the validation stream's dequantisation noise of
        `seed` (step 0, row = the image's position in `images`) and the bound on its log-probability in nats."""
        seed = check_seed(seed)
        steps, solver = check_solver(self.model.T, steps, solver)
        x = self._rows(images)
        zs, lls = [], []
        for i in range(0, x.shape[0], batch):
            z, nll = self._forward_rows(x[i:i + batch], seed, self._tag_eval, 0, row0=i, steps=steps, solver=solver)
            zs.append(z)
            lls.append(-nll)
        torch.cuda.synchronize()
        return torch.cat(zs), torch.cat(lls)

    def decode(self, z, batch=1024, steps=100, solver="rk4"):
        """x [n, I] in [0, 1] of latent codes z [n, I]: encode's inverse to the solver's accuracy (and up to the
        dequantisation noise inside a grey level)."""
        steps, solver = check_solver(self.model.T, steps, solver)
        z = z.reshape(z.shape[0], -1)
        if z.shape[1] != self.model.image_size:
            raise FlowMatchError("codes have %d elements, the model %d" % (z.shape[1], self.model.image_size))
        z = z.to(self._device(), torch.float32).contiguous()
        out = [self._inverse_rows(z[i:i + batch], steps, solver) for i in range(0, z.shape[0], batch)]
        torch.cuda.synchronize()
        return torch.cat(out)

    def log_likelihood_rows(self, images=None, seed=1, batch=1024, steps=100, solver="rk4"):
        """The bound on log p(x) per image in nats under the continuous flow, a float64 CPU tensor [n]: batch i of
        `batch` rows at step i of the validation stream under `seed`."""
        seed = check_seed(seed)
        steps, solver = check_solver(self.model.T, steps, solver)
        x = self._rows(_dataset_rows(self.test_iter) if images is None else images)
        out = [-self._forward_rows(x[i:i + batch], seed, self._tag_eval, i // batch, steps=steps, solver=solver)[1]
               for i in range(0, x.shape[0], batch)]
        torch.cuda.synchronize()
        return torch.cat(out).double().cpu()

    def log_likelihood(self, images=None, seed=1, batch=1024, steps=100, solver="rk4"):
        """log_likelihood_rows -> metrics.NLLResult(ll_mean, ll_stderr, n)."""
        return self._nll_result(self.log_likelihood_rows(images, seed, batch, steps, solver))

    viz_steps = 50               # solver steps of the per-epoch sample grid (the largest divisor of T up to it)

    def sample_images(self, epoch=-100, num_images=36, save=True):
        from . import viz
        T = self.model.T
        steps = max(s for s in range(1, min(T, self.viz_steps) + 1) if T % s == 0)
        return viz.ddpm_sample_images(self, epoch, num_images, save, self.viz_dir, steps=steps)

    def viz_loss(self):
        from . import viz
        viz.one_loss_curve(self, "velocity regression loss")


__all__ = ["VelocityField", "FlowMatching", "FlowMatchTrainer", "FlowMatchEngine", "FlowMatchError", "tables",
           "ode_table", "grid_index_reference", "uniforms_reference", "normals_reference", "path_reference",
           "divergence_matrix", "flowmatch_fused_ok", "check_solver", "TABLEAUS", "SOLVERS", "FlatAdam"]
