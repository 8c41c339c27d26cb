"""RealNVP coupling flow (Dinh, Sohl-Dickstein & Bengio, "Density estimation using Real NVP", arXiv 1605.08803; its additive
ancestor NICE, arXiv 1410.8516) with MLP conditioners: the collection's invertible model -- an exact density for
grey-level data, sampling in one pass, and a latent code that is a bijection of the image.  Exported by src/real_nvp.py
as RealNVP / RealNVPTrainer.

The contract.

Model.  RealNVP(image_size D = 784, hidden_dim H = 400, num_couplings K = 4, mask = "checker", alpha = 0.05, levels = 256,
s_cap = 2.0).  Limits: 2 <= D <= 8192, 1 <= H <= 1024, 1 <= K <= 16, 0 <= alpha < 0.5, 2 <= levels <= 65536,
0 < s_cap <= 8; anything else raises RealNVPError(GMError, ValueError) in the constructor.

Split.  "checker": half A is the even-indexed pixels, half B the odd ones.  "half": half A is the first ceil(D / 2)
pixels, half B the rest.  Da = ceil(D / 2), Db = floor(D / 2).  The halves live in two separate contiguous row-major
buffers throughout, so every GEMM operand is dense.

Couplings.  couplings = ModuleList of K Coupling modules, each linear = Linear(Dc, H) and out = Linear(H, 2 Dt).  Even k
(0-based) transforms B conditioned on A, odd k transforms A conditioned on B.  st = out(relu(linear(x_c)));
s = s_cap tanh(st[:, :Dt]), t = st[:, Dt:];  y_t = x_t exp(s) + t, y_c = x_c;  logdet += sum_j s_j.  out.weight and
out.bias are zero at construction, so a fresh model is the identity flow.  state_dict keys:
couplings.{k}.linear.{weight,bias} and couplings.{k}.out.{weight,bias}.

Preprocessing.  For pixel e of row r with value x in [0, 1]:  q = floor(x (levels - 1) + 0.5);  v = (q + u) / levels;
w = alpha + (1 - 2 alpha) v;  y = log(w) - log1p(-w);  the element's log-determinant is log(1 - 2 alpha) - log(w) -
log1p(-w).  (In fp32, on the device and in `preprocess` below alike, 1 - w is alpha + (1 - 2 alpha) vc with vc =
((levels - 1 - q) + (1 - u)) / levels: 1 - u is exact and nothing cancels, so both logarithms are finite for every word
even at alpha = 0.)  u is ph_unit (csrc/gm_philox.h) of word e & 3 of Philox4x32-10 at counter (e >> 2, step, row, TAG)
under key (seed mod 2^32, seed >> 32); e is the pixel's index in the unsplit image, row the row's position in the whole
batch.  Training: TAG_TRAIN = "NVPD", step = the count of training batches taken.  Validation and log_likelihood:
TAG_EVAL = "NVPV", step = the batch's index in that pass, so a validation number is reproducible.  u is never 0 or 1, so
alpha = 0 is legal.

Loss.  Per row  nll_r = 0.5 sum z^2 + 0.5 D log(2 pi) - logdet_pre_r - logdet_r + D log(levels)  in nats per image: the
negative of the dequantisation bound on the discrete image's log-probability.  The batch loss is the mean over rows;
gradients are of that mean: dz = z / b, and the log-determinant's cotangent is -1 / b.

Sampling.  z of element e of sample row r is the Box-Muller normal (ph_box_muller, ph_normal4's word pairing) of Philox
counter (e >> 2, 0, r, TAG_S = "NVPS"): indexed by row and element, so a row does not depend on n.  z *= temperature; the
couplings are inverted last to first, x_t = (y_t - t) exp(-s);  x = clamp((sigmoid(y) - alpha) / (1 - 2 alpha), 0, 1).

Fused path: RealNVPEngine below (csrc/gm_nvp.hip) -- per training batch the gather, gm_nvp_pre,
K x (two forwards, gm_nvp_couple), gm_nvp_loss, K x (gm_nvp_couple_bwd, the two input gradients -- the first coupling
needs only one -- and both weight gradients + Adam as a pair) and the loss sum with the counter tick: 7 K + 3 launches.
A validation batch is the forward and the sum; sampling is gm_nvp_post's PRIOR mode, K x (two forwards, the inverse
couple) and gm_nvp_post: 3 K + 2 launches.  An overridden compute_batch / evaluate or an edited model: the general loop --
autograd over ops.fused_linear plus torch ops on the same u (gm_nvp_pre's NOISE mode)."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, philox, viz
from ._lib import (NVP_MAX_D, NVP_MAX_H, NVP_MAX_K, NVP_MAX_LEVELS, NVP_MAX_S_CAP, NVP_MIN_D, NVP_TAG_EVAL, NVP_TAG_S,
                   NVP_TAG_TRAIN, GMError)
from .trainers import FlatAdam, OneLossTrainer, _dataset_rows, _stock_module, stock, stock_model  # noqa: F401
from .engine import OneNetEngine, _Linear

TAG_TRAIN, TAG_EVAL, TAG_S = NVP_TAG_TRAIN, NVP_TAG_EVAL, NVP_TAG_S
MASKS = ("checker", "half")


class RealNVPError(GMError, ValueError):
    """A bad image size, width, coupling count, mask, alpha, levels, s_cap, seed, n or temperature: a ValueError, and a
    GMError like the package's other refusals."""


def _int(v, name):
    return _lib.check_int(v, name, RealNVPError)


def check_seed(seed, name="seed"):
    return _lib.check_seed(seed, name, RealNVPError)


def check_flow_settings(alpha, levels, s_cap, error):
    """(alpha, levels, s_cap) of a dequantising flow, validated against the gm_nvp kernels' limits -- in fp32 too, where
    the kernels compute; else `error`."""
    alpha, s_cap = _lib.check_real(alpha, "alpha", error), _lib.check_real(s_cap, "s_cap", error)
    levels = _lib.check_int(levels, "levels", error)
    if not (0.0 <= alpha < 0.5 and float(np.float32(alpha)) < 0.5):
        raise error("alpha must lie in [0, 0.5), got %r" % alpha)
    if not 2 <= levels <= NVP_MAX_LEVELS:
        raise error("levels must lie in [2, %d], got %d" % (NVP_MAX_LEVELS, levels))
    if not (0.0 < s_cap <= NVP_MAX_S_CAP and float(np.float32(s_cap)) > 0.0):
        raise error("s_cap must lie in (0, %d], got %r" % (NVP_MAX_S_CAP, s_cap))
    return alpha, levels, s_cap


def check_coupling_shape(image_size, hidden_dim, num_couplings, mask, error):
    """(D, H, K, mask) of a coupling flow over two halves, validated against the kernels' limits; else `error`."""
    D, H, K = (_lib.check_int(v, n, error) for v, n in ((image_size, "image_size"), (hidden_dim, "hidden_dim"),
                                                        (num_couplings, "num_couplings")))
    if not NVP_MIN_D <= D <= NVP_MAX_D:
        raise error("image_size must lie in [%d, %d], got %d" % (NVP_MIN_D, NVP_MAX_D, D))
    if not 1 <= H <= NVP_MAX_H:
        raise error("hidden_dim must lie in [1, %d], got %d" % (NVP_MAX_H, H))
    if not 1 <= K <= NVP_MAX_K:
        raise error("num_couplings must lie in [1, %d], got %d" % (NVP_MAX_K, K))
    if not isinstance(mask, str) or mask not in MASKS:
        raise error("mask must be one of %s, got %r" % (MASKS, mask))
    return D, H, K, mask


def check_config(image_size, hidden_dim, num_couplings, mask, alpha, levels, s_cap):
    """(D, H, K, mask, alpha, levels, s_cap) validated against the kernels' limits; else RealNVPError."""
    return (check_coupling_shape(image_size, hidden_dim, num_couplings, mask, RealNVPError)
            + check_flow_settings(alpha, levels, s_cap, RealNVPError))


# ---- the split and the noise rules in numpy (the tests' reference reads the same contract) ----------------------------
def split_indices(D, mask="checker"):
    """(A, B): the pixel indices of the two halves, int64, each ascending; together they partition 0 .. D - 1."""
    D = _int(D, "image_size")
    if mask not in MASKS:
        raise RealNVPError("mask must be one of %s, got %r" % (MASKS, mask))
    e = np.arange(D, dtype=np.int64)
    if mask == "checker":
        return e[0::2].copy(), e[1::2].copy()
    Da = (D + 1) // 2
    return e[:Da].copy(), e[Da:].copy()


def philox_words(n, D, seed, step, tag, row0=0):
    """The uint32 word of pixel e of rows row0 ..: word e & 3 of counter (e >> 2, step, row, tag); [n, D]."""
    return philox.words(n, D, seed, step, tag, row0)


def uniforms_reference(n, D, seed, step, tag=TAG_TRAIN, row0=0):
    """u [n, D] float32: the dequantisation noise by the contract's rule, bit for bit."""
    return philox.unit_uniforms(philox.words(n, D, seed, step, tag, row0))


def normals_reference(n, D, seed, row0=0):
    """z [n, D] float64: the sampler's starting normals by the contract's rule (the device rounds to fp32)."""
    return philox.normals(n, D, seed, 0, TAG_S, row0)


def nll_constant(D, levels):
    """0.5 D log(2 pi) + D log(levels)."""
    return 0.5 * D * math.log(2.0 * math.pi) + D * math.log(levels)


def preprocess(x, u, alpha, levels):
    """(y [n, D], logdet [n]) of pixel rows x in [0, 1] and noise u in (0, 1), by torch ops in x's dtype: the general
    path's (and the fp32 statement of the kernel's) dequantise + logit."""
    top = float(levels - 1)
    q = torch.clamp(torch.floor(x * top + 0.5), 0.0, top)
    v = (q + u) / levels
    vc = ((top - q) + (1.0 - u)) / levels
    w, wc = alpha + (1.0 - 2.0 * alpha) * v, alpha + (1.0 - 2.0 * alpha) * vc
    lw, lwc = torch.log(w), torch.log(wc)
    return lw - lwc, ((math.log(1.0 - 2.0 * alpha) - lw) - lwc).sum(1)


def postprocess(y, alpha):
    """x = clamp((sigmoid(y) - alpha) / (1 - 2 alpha), 0, 1)."""
    return torch.clamp((torch.sigmoid(y) - alpha) / (1.0 - 2.0 * alpha), 0.0, 1.0)


# ---- modules ---------------------------------------------------------------------------------------------------------
@stock_model
class Coupling(nn.Module):
    """One conditioner: linear (Dc -> H, relu) and out (H -> 2 Dt), out starting at zero."""

    def __init__(self, cond_dim, trans_dim, hidden_dim):
        super().__init__()
        self.linear = nn.Linear(cond_dim, hidden_dim)
        self.out = nn.Linear(hidden_dim, 2 * trans_dim)
        with torch.no_grad():
            self.out.weight.zero_()
            self.out.bias.zero_()

    def forward(self, x_c):
        """st [n, 2 Dt] of the conditioning half."""
        if not x_c.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: got a %s tensor and there is no CPU "
                          "fallback (move the model and inputs with to_cuda)" % x_c.device)
        h = ops.fused_linear(x_c.contiguous(), self.linear.weight, self.linear.bias, "relu")
        return ops.fused_linear(h, self.out.weight, self.out.bias, "id")


class CouplingFlow(nn.Module):
    """K couplings over the two halves of a logit-space image: the split, the alternation (even k transforms B) and the
    two directions, shared by RealNVP and nsf.SplineFlow.  A subclass sets image_size, num_couplings, mask and
    `couplings`, and supplies the element-wise map: _transform(k, x_t, x_c) -> (y_t, its log-determinant per row) and
    _untransform(k, y_t, x_c) -> x_t, by autograd-able torch ops."""

    def _halves(self, make):
        """Da, Db and `couplings` = make(Dc, Dt) for every k."""
        D = self.image_size
        self.Da, self.Db = (D + 1) // 2, D // 2
        dims = [(self.Da, self.Db) if k % 2 == 0 else (self.Db, self.Da) for k in range(self.num_couplings)]
        self.couplings = nn.ModuleList([make(dc, dt) for dc, dt in dims])
        self.shape = int(D ** 0.5)

    def split(self, y):
        """(a [n, Da], b [n, Db]) of y [n, D]."""
        ia, ib = split_indices(self.image_size, self.mask)
        return (y[:, torch.from_numpy(ia).to(y.device)].contiguous(),
                y[:, torch.from_numpy(ib).to(y.device)].contiguous())

    def merge(self, a, b):
        """y [n, D] of the halves."""
        ia, ib = split_indices(self.image_size, self.mask)
        y = torch.empty(a.shape[0], self.image_size, dtype=a.dtype, device=a.device)
        y[:, torch.from_numpy(ia).to(a.device)] = a
        y[:, torch.from_numpy(ib).to(a.device)] = b
        return y

    def flow(self, y):
        """(z [n, D], logdet [n]) of logit-space rows y, by autograd-able torch ops over the fused linear kernels."""
        h = list(self.split(y))
        logdet = torch.zeros(y.shape[0], dtype=y.dtype, device=y.device)
        for k in range(len(self.couplings)):
            t = 1 - (k & 1)                          # even k transforms B
            h[t], ld = self._transform(k, h[t], h[1 - t])
            logdet = logdet + ld
        return self.merge(h[0], h[1]), logdet

    def inverse(self, z):
        """y [n, D] with flow(y)[0] == z: the couplings inverted last to first."""
        h = list(self.split(z))
        for k in reversed(range(len(self.couplings))):
            t = 1 - (k & 1)
            h[t] = self._untransform(k, h[t], h[1 - t])
        return self.merge(h[0], h[1])

    def forward(self, y):
        return self.flow(y)


@stock_model
class RealNVP(CouplingFlow):
    """K affine couplings over the two halves of a logit-space image."""

    def __init__(self, image_size=784, hidden_dim=400, num_couplings=4, mask="checker", alpha=0.05, levels=256,
                 s_cap=2.0):
        super().__init__()
        (self.image_size, self.hidden_dim, self.num_couplings, self.mask, self.alpha, self.levels,
         self.s_cap) = check_config(image_size, hidden_dim, num_couplings, mask, alpha, levels, s_cap)
        self._halves(lambda dc, dt: Coupling(dc, dt, self.hidden_dim))

    def _st(self, k, x_c):
        st = self.couplings[k](x_c)
        dt = st.shape[1] // 2
        return self.s_cap * torch.tanh(st[:, :dt]), st[:, dt:]

    def _transform(self, k, x_t, x_c):
        s, sh = self._st(k, x_c)
        return x_t * torch.exp(s) + sh, s.sum(1)

    def _untransform(self, k, y_t, x_c):
        s, sh = self._st(k, x_c)
        return (y_t - sh) * torch.exp(-s)


def realnvp_fused_ok(model):
    """True iff the model is RealNVP itself with its couplings unchanged and consistent shapes and settings."""
    if not type(model).__dict__.get("_gm_stock_model", False) or type(model) is not RealNVP:
        return False
    kids = list(model.children())
    cs = getattr(model, "couplings", None)
    if len(kids) != 1 or kids[0] is not cs or type(cs) is not nn.ModuleList:
        return False
    try:
        D, H, K, mask, alpha, levels, s_cap = check_config(model.image_size, model.hidden_dim, model.num_couplings,
                                                           model.mask, model.alpha, model.levels, model.s_cap)
    except (RealNVPError, AttributeError):
        return False
    if len(cs) != K:
        return False
    Da, Db = (D + 1) // 2, D // 2
    for k, c in enumerate(cs):
        dc, dt = (Da, Db) if k % 2 == 0 else (Db, Da)
        if not (type(c) is Coupling and _stock_module(c, 2) and type(getattr(c, "linear", None)) is nn.Linear
                and type(getattr(c, "out", None)) is nn.Linear and c.linear.bias is not None and c.out.bias is not None
                and tuple(c.linear.weight.shape) == (H, dc) and tuple(c.out.weight.shape) == (2 * dt, H)):
            return False
    return True


def nll_rows(z, logdet_pre, logdet, D, levels):
    """The rows' negative log-likelihood in nats per image, by torch ops."""
    return 0.5 * (z * z).sum(1) + nll_constant(D, levels) - logdet_pre - logdet


# ---- engine ----------------------------------------------------------------------------------------------------------
class RealNVPEngine(OneNetEngine):
    """RealNVP on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  Per
    training batch: 1. gm_gather_rows[_bits];  2. gm_nvp_pre;  3. K x (H1 = relu(linear(x_c)), ST = out(H1),
    gm_nvp_couple);  4. gm_nvp_loss (dZ, row partials);  5. for k = K - 1 .. 0: gm_nvp_couple_bwd, dH = dST Wout [H1 > 0],
    for k > 0 the conditioning half's cotangent dH Wlin + its direct cotangent in the GEMM's epilogue -- both input
    gradients BEFORE the pair that steps the coupling's weights -- and the two weight gradients + Adam as a pair;
    6. the loss sum with the counter tick.  Every coupling keeps its H1, ST and output half: nothing is recomputed.  A
    validation batch is launches 1-4 (no dZ) and the sum.  The noise step of a training batch is ctr + nbase (DDPMEngine's
    scheme), of a validation batch ctr (the batch's index in the pass).  No host noise ring, every batch its own gather.
    One GPU only."""

    one_gpu = "the RealNVP engine"
    fused_ok = staticmethod(realnvp_fused_ok)
    refusal = ("RealNVP", "realnvp.RealNVP", "couplings")        # the trainer: seed and noise_steps

    def _params(self, model):
        return [p for c in model.couplings for p in (c.linear.weight, c.linear.bias, c.out.weight, c.out.bias)]

    def _setup(self, model):
        self.C = [(_Linear(self.fp, c.linear), _Linear(self.fp, c.out)) for c in model.couplings]
        self.D, self.H, self.K = model.image_size, model.hidden_dim, model.num_couplings
        self.Da, self.Db = model.Da, model.Db
        self.I = self.D

    def _dt(self, k):
        return self.Db if k % 2 == 0 else self.Da

    # ---- the element-wise map of a coupling (nsf.SplineFlowEngine swaps these three) ---------------------------------------
    def _st_width(self, dt):
        """Columns of a conditioner's output for a transformed half of dt pixels."""
        return 2 * dt

    def _couple(self, st, k, xt, b):
        """Y[k] of the coupling's input xt and ST[k]; the rows' log-determinant grows."""
        from . import ops_fused as of_
        of_.nvp_couple(self.ST[k], xt, self.Y[k], b, self._dt(k), self.model.s_cap, logdet=self.logdet, stream=st)

    def _couple_bwd(self, st, k, xt, g, dST, b, c):
        """dST and dX[k] of the output half's cotangent g and the log-determinant's c."""
        from . import ops_fused as of_
        of_.nvp_couple_bwd(self.ST[k], xt, g, dST, b, self._dt(k), self.model.s_cap, c, dx=self.dX[k], stream=st)

    def _buffers(self, B):
        z = lambda *s: torch.zeros(*s, device=self.device)
        D, H, K, Da, Db = self.D, self.H, self.K, self.Da, self.Db
        self.X, self.Y0 = z(B, D), (z(B, Da), z(B, Db))
        self.H1 = [z(B, H) for _ in range(K)]
        self.ST = [z(B, self._st_width(self._dt(k))) for k in range(K)]
        self.Y = [z(B, self._dt(k)) for k in range(K)]
        self.logdet, self.part = z(B), z(B)
        self.dZ = (z(B, Da), z(B, Db))
        self.dST = (z(B, self._st_width(Da)), z(B, self._st_width(Db)))      # by the transformed half: A's, B's
        self.dH = z(B, H)
        self.dX = [z(B, self._dt(k)) if k >= 2 else None for k in range(K)]          # d loss / d (coupling k's input)
        self.G = [z(B, self._dt(k - 1)) if k >= 1 else None for k in range(K)]       # cotangent of coupling k's x_c

    def _settings(self):
        m = self.model
        return {"mask": str(m.mask), "alpha": float(m.alpha), "levels": int(m.levels), "s_cap": float(m.s_cap),
                "seed": int(self.trainer.seed)}

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        """VAEEngine.configure: the settings above are compared with a checkpoint's before anything is allocated or
        reset, and are launch arguments of the graphs, with the seed."""
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)

    def _chain(self):
        """Per coupling k: (index of the transformed half, its input x_t, the conditioning half x_c), and the final
        halves (Za, Zb)."""
        cur = [self.Y0[0], self.Y0[1]]
        steps = []
        for k in range(self.K):
            t = 1 - (k & 1)
            steps.append((t, cur[t], cur[1 - t]))
            cur[t] = self.Y[k]
        return steps, cur

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: preprocessing, the K couplings, the loss (+ backward and Adam when train)."""
        from . import ops_fused as of_
        m, K = self.model, self.K
        idx_slot = self._slot(t, 1, 0, self.R, self.B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        ops.gather_rows(self.data, self.idx_ring.view(-1), self.X, B=b, idx_slot=idx_slot, stream=st)
        of_.nvp_pre(self.X, self.Y0[0], self.Y0[1], self.logdet, b, self.trainer.seed,
                    TAG_TRAIN if train else TAG_EVAL, m.alpha, m.levels, m.mask, stream=st, **self._clock(t, train))
        steps, (Za, Zb) = self._chain()
        for k, (th, xt, xc) in enumerate(steps):
            L1, L2 = self.C[k]
            ops.linear_fwd(xc, L1.W, L1.b, self.H1[k], "relu", M=b, stream=st)
            ops.linear_fwd(self.H1[k], L2.W, L2.b, self.ST[k], "id", M=b, stream=st)
            self._couple(st, k, xt, b)
        scale = float(np.float32(1.0 / b))
        cst = float(np.float32(nll_constant(self.D, m.levels)))
        of_.nvp_loss(Za, Zb, self.logdet, self.part, b, cst, scale=scale, dza=self.dZ[0] if train else None,
                     dzb=self.dZ[1] if train else None, stream=st)
        if train:
            adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
            for k in range(K - 1, -1, -1):
                th, xt, xc = steps[k]
                L1, L2 = self.C[k]
                dST = self.dST[th]
                g = self.dZ[th] if k == K - 1 else self.G[k + 1]
                self._couple_bwd(st, k, xt, g, dST, b, -scale)
                # both input gradients read the coupling's weights BEFORE the paired dW(+Adam) launch updates them
                ops.linear_bwd_dx(dST, L2.W, self.dH, below=self.H1[k], epi="relu", M=b, stream=st)
                if k > 0:
                    direct = self.dZ[1 - th] if k == K - 1 else self.dX[k + 1]
                    ops.linear_bwd_dx(self.dH, L1.W, self.G[k], M=b, add=direct, stream=st)
                ops.linear_bwd_dw_adam_pair(dict(dA=dST, X=self.H1[k], lin=L2, adam=adam, M=b),
                                            dict(dA=self.dH, X=xc, lin=L1, adam=adam, M=b),
                                            weight_decay=self.wd, stream=st)
        of_.sum_finalize(self.part, b, self.recon if train else self.vrecon, scale=scale, out_slot=loss_slot,
                         tick=self.ctr if self.use_graph else None, stream=st)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class DequantFlowTrainer(OneLossTrainer):
    """What the trainers of the two flows over dequantised grey-level images share (RealNVP here, MAF in maf.py): one
    protocol around two sets of kernels.  Rows are dequantised and taken to logit space under the contract's Philox
    noise -- the training stream at step `noise_steps` while the model trains, the validation stream at the batch's
    index otherwise; encode runs at step 0 with row0 = the image's position; log_likelihood_rows runs batch i at step i;
    sample is the prior's normals times the temperature through the inverse flow, between two synchronises.

    A latent travels between the hooks as a `code`: z [n, D] itself by default, the pair of halves for RealNVP, which
    merges and splits only where a public method takes or returns z.  A subclass names _tag_train, _tag_eval and _error
    and supplies _flow_settings() -> (alpha, levels, s_cap), _model_flow(y) -> (z, logdet) by autograd-able ops,
    _forward_rows(x, seed, tag, step, row0) -> (code, nll [n]), _inverse_rows(code) -> x and _prior(n, seed,
    temperature) -> code."""
    _line = "Epoch[%d/%d], NLL: %.6f, Val NLL: %.6f"
    _tag_train = _tag_eval = None
    _engine_reads_trainer = True

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, seed=0):
        self.seed = self._check_seed(seed)           # before anything runs
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)
        self.noise_steps = 0                         # training batches taken: the next one's noise step
        self._eval_step = 0                          # batch index within an evaluate() call

    def _check_seed(self, seed):
        return _lib.check_seed(seed, "seed", self._error)

    def _code_to_z(self, code):
        return code

    def _z_to_code(self, z):
        return z

    def compute_batch(self, batch):
        """The batch's NLL in nats per image (general path: autograd over the fused linear kernels; u from gm_nvp_pre's
        NOISE mode on the contract's counter stream -- the training stream while the model trains, the validation one
        otherwise)."""
        from . import ops_fused as of_
        x = self._flat_batch(batch)
        alpha, levels, _ = self._flow_settings()
        train, step = self._noise_step()
        u = of_.nvp_uniforms(x.shape[0], x.shape[1], self.seed, self._tag_train if train else self._tag_eval, step=step,
                             device=x.device)
        y, ld0 = preprocess(x, u, alpha, levels)
        z, ld = self._model_flow(y)
        return nll_rows(z, ld0, ld, x.shape[1], levels).sum() / x.shape[0]

    # ---- sampling and scoring ------------------------------------------------------------------------------------------
    def sample(self, n, seed=0, temperature=1.0):
        """n samples [n, D] float32 in [0, 1]: the contract's normals (indexed by row and element: rows 0 .. 4 of
        sample(300) are sample(5)) times the temperature through the inverse flow.  Runs after a device synchronise; the
        global generator, the model's mode and the parameters are untouched."""
        E = self._error
        n, seed = _lib.check_int(n, "n", E), self._check_seed(seed)
        temperature = _lib.check_real(temperature, "temperature", E)
        if not 1 <= n < 1 << 31:
            raise E("n must lie in [1, 2^31), got %d" % n)
        if temperature < 0.0:
            raise E("temperature must be >= 0, got %r" % temperature)
        self._device()
        torch.cuda.synchronize()
        x = self._inverse_rows(self._prior(n, seed, temperature))
        torch.cuda.synchronize()
        return x

    def encode(self, images, seed=0, batch=1024):
        """(z [n, D], log_px [n]): the latent code of every image under the validation stream's noise of `seed` (step 0,
        row = the image's position in `images`) and the dequantisation bound on its log-probability in nats."""
        seed = self._check_seed(seed)
        x = self._rows(images)
        torch.cuda.synchronize()
        zs, lls = [], []
        for i in range(0, x.shape[0], batch):
            code, nll = self._forward_rows(x[i:i + batch], seed, self._tag_eval, 0, row0=i)
            zs.append(self._code_to_z(code))
            lls.append(-nll)
        torch.cuda.synchronize()
        return torch.cat(zs), torch.cat(lls)

    def decode(self, z, batch=1024):
        """x [n, D] in [0, 1] of latent codes z [n, D]: encode's inverse (up to the dequantisation noise inside a
        grey level)."""
        z = z.reshape(z.shape[0], -1)
        if z.shape[1] != self.model.image_size:
            raise self._error("codes have %d elements, the model %d" % (z.shape[1], self.model.image_size))
        z = z.to(self._device(), torch.float32).contiguous()
        torch.cuda.synchronize()
        out = [self._inverse_rows(self._z_to_code(z[i:i + batch])) for i in range(0, z.shape[0], batch)]
        torch.cuda.synchronize()
        return torch.cat(out)

    def log_likelihood_rows(self, images=None, seed=1, batch=1024):
        """The bound on log p(x) per image in nats, a float64 CPU tensor [n]: batch i of `batch` rows at step i of the
        validation stream under `seed`."""
        seed = self._check_seed(seed)
        x = self._rows(_dataset_rows(self.test_iter) if images is None else images)
        torch.cuda.synchronize()
        out = [-self._forward_rows(x[i:i + batch], seed, self._tag_eval, i // batch)[1]
               for i in range(0, x.shape[0], batch)]
        torch.cuda.synchronize()
        return torch.cat(out).double().cpu()

    def log_likelihood(self, images=None, seed=1, batch=1024):
        """The dequantisation bound on log p(x) of every image in nats (images=None: the whole test_iter) ->
        metrics.NLLResult(ll_mean, ll_stderr, n)."""
        return self._nll_result(self.log_likelihood_rows(images, seed, batch))

    def bits_per_dim(self, res):
        """A log_likelihood result (or a mean log-likelihood in nats) in bits per pixel."""
        ll = res.ll_mean if hasattr(res, "ll_mean") else float(res)
        return -ll / (self.model.image_size * math.log(2.0))

    # ---- visualisation ---------------------------------------------------------------------------------------------------
    def sample_images(self, epoch=-100, num_images=36, save=True):
        return viz.realnvp_sample_images(self, epoch, num_images, save, self.viz_dir)

    def reconstruct_images(self, images, epoch, save=True):
        raise GMError("a flow reconstructs exactly: decode(encode(images)[0]) returns the dequantised images")

    def viz_loss(self):
        viz.one_loss_curve(self, "NLL (nats per image)")


@stock
class CouplingFlowTrainer(DequantFlowTrainer):
    """What the trainers of the two coupling flows share (RealNVP here, the neural spline flow in nsf.py): a
    DequantFlowTrainer whose code is the pair of halves, over a model with split, merge, inverse and `couplings` of
    (linear, out) conditioners.  On device rows the flow is gm_nvp_pre, K x (the conditioner's two GEMMs, the coupling's
    launch) and gm_nvp_loss; its inverse the couplings last to first and gm_nvp_post (3 K + 2 launches with the prior's
    for a stock model).  A subclass supplies _couple_rows(st, inp, out, logdet=None, inverse=False), the coupling's one
    launch."""
    _tag_train, _tag_eval = TAG_TRAIN, TAG_EVAL

    def _model_flow(self, y):
        return self.model(y)

    def _code_to_z(self, code):
        return self.model.merge(*code)

    def _z_to_code(self, z):
        return self.model.split(z)

    # ---- the flow on device rows, no autograd --------------------------------------------------------------------------
    def _st(self, k, xc):
        """ST of coupling k on device rows xc: the two GEMM launches."""
        c = self.model.couplings[k]
        h = torch.empty(xc.shape[0], c.linear.weight.shape[0], device=xc.device)
        st = torch.empty(xc.shape[0], c.out.weight.shape[0], device=xc.device)
        ops.linear_fwd(xc, c.linear.weight.detach(), c.linear.bias.detach(), h, "relu")
        ops.linear_fwd(h, c.out.weight.detach(), c.out.bias.detach(), st, "id")
        return st

    def _forward_rows(self, x, seed, tag, step, row0=0):
        """((za, zb), nll [n]) of device rows x under the noise of (seed, tag, step, row0 ..): the kernels for a stock
        model, the model's own forward on the same u otherwise."""
        from . import ops_fused as of_
        m, n = self.model, x.shape[0]
        with torch.no_grad():
            if not self._fused_ok(m):
                u = of_.nvp_uniforms(n, m.image_size, seed, tag, step=step, row0=row0, device=x.device)
                y, ld0 = preprocess(x, u, m.alpha, m.levels)
                z, ld = m(y)
                return m.split(z), nll_rows(z, ld0, ld, m.image_size, m.levels)
            h = [torch.empty(n, m.Da, device=x.device), torch.empty(n, m.Db, device=x.device)]
            logdet, part = torch.empty(n, device=x.device), torch.empty(n, device=x.device)
            of_.nvp_pre(x, h[0], h[1], logdet, n, seed, tag, m.alpha, m.levels, m.mask, step=step, row0=row0)
            for k in range(m.num_couplings):
                t = 1 - (k & 1)
                out = torch.empty_like(h[t])
                self._couple_rows(self._st(k, h[1 - t]), h[t], out, logdet=logdet)
                h[t] = out
            of_.nvp_loss(h[0], h[1], logdet, part, n, float(np.float32(nll_constant(m.image_size, m.levels))))
            return (h[0], h[1]), part

    def _inverse_rows(self, code):
        """x [n, D] in [0, 1] of latent halves (za, zb): the couplings inverted last to first, then gm_nvp_post."""
        from . import ops_fused as of_
        za, zb = code
        m, n = self.model, za.shape[0]
        with torch.no_grad():
            if not self._fused_ok(m):
                return postprocess(m.inverse(m.merge(za, zb)), m.alpha).contiguous()
            h = [za, zb]
            for k in reversed(range(m.num_couplings)):
                t = 1 - (k & 1)
                out = torch.empty_like(h[t])
                self._couple_rows(self._st(k, h[1 - t]), h[t], out, inverse=True)
                h[t] = out
            x = torch.empty(n, m.image_size, device=za.device)
            of_.nvp_post(h[0], h[1], x, n, m.alpha, m.mask)
            return x

    def _prior(self, n, seed, temperature):
        """The sampler's starting halves (za, zb): gm_nvp_post's PRIOR mode."""
        from . import ops_fused as of_
        dev, m = self._device(), self.model
        za, zb = torch.empty(n, m.Da, device=dev), torch.empty(n, m.Db, device=dev)
        of_.nvp_prior(za, zb, n, m.image_size, seed, m.mask, temperature=temperature)
        return za, zb


@stock
class RealNVPTrainer(CouplingFlowTrainer):
    """Trains a RealNVP on its exact (dequantised) negative log-likelihood; samples, encodes and decodes: a
    DequantFlowTrainer whose code is the pair of halves (sampling is 3 K + 2 launches for a stock model).  Histories:
    `losses` (the NLL in nats per image, one per training batch); the epoch line (mean training NLL, validation NLL);
    best_val_loss / best_model as the other VAE-family trainers; checkpoints (+ mask, alpha, levels, s_cap, seed in the
    optimizer state's config, checked under strict=True, and the number of training batches taken, so a resumed run
    continues the noise stream bit for bit).  One GPU only."""
    _one_gpu = "RealNVPTrainer"
    _error = RealNVPError
    _fused_ok = staticmethod(realnvp_fused_ok)

    def _flow_settings(self):
        m = self.model
        return m.alpha, m.levels, m.s_cap

    def _engine_class(self):
        return RealNVPEngine

    def train(self, num_epochs, lr=1e-3, weight_decay=0.0, quiet=False):
        """VAETrainer.train with this model's defaults."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    def _couple_rows(self, st, inp, out, logdet=None, inverse=False):
        from . import ops_fused as of_
        of_.nvp_couple(st, inp, out, inp.shape[0], inp.shape[1], self.model.s_cap, logdet=logdet, inverse=inverse)

    def interpolate(self, a, b, steps=8, seed=0):
        """[steps, D]: the decoded line from image a to image b in z."""
        steps = _int(steps, "steps")
        if steps < 2:
            raise RealNVPError("steps must be >= 2, got %d" % steps)
        z, _ = self.encode(torch.stack([a.reshape(-1), b.reshape(-1)]), seed=seed)
        w = torch.linspace(0.0, 1.0, steps, device=z.device)[:, None]
        return self.decode((1.0 - w) * z[0:1] + w * z[1:2])


__all__ = ["Coupling", "CouplingFlow", "CouplingFlowTrainer", "RealNVP", "RealNVPTrainer", "RealNVPEngine",
           "RealNVPError", "split_indices", "philox_words",
           "uniforms_reference", "normals_reference", "preprocess", "postprocess", "nll_constant", "realnvp_fused_ok"]
