"""Neural spline flow (Durkan, Bortoli, Murray & Papamakarios, "Neural Spline Flows", arXiv 1906.04032) with MLP
conditioners: RealNVP's coupling flow with the affine map x exp(s) + t replaced by a monotone rational-quadratic spline
per pixel -- an element-wise transform that can bend, still inverted in closed form, so sampling, encode / decode and the
exact dequantised likelihood stay.  Exported by src/spline_flow.py as SplineFlow / SplineFlowTrainer.

The contract.

Model.  SplineFlow(image_size D = 784, hidden_dim H = 400, num_couplings K = 4, num_bins = 8, tail_bound = 3.0, mask =
"checker", alpha = 0.05, levels = 256).  D, H, K, mask, alpha and levels have RealNVP's limits (realnvp.py); num_bins is
4, 8 or 16; 0 < tail_bound <= 64, in fp32 too; anything else raises SplineFlowError(GMError, ValueError) in the
constructor.  There is no s_cap.

Split, halves, alternation, preprocessing.  RealNVP's contract, bit for bit: the "checker" / "half" split into two dense
half buffers, even k (0-based) transforms B conditioned on A, the dequantise + logit preprocessing under the Philox noise
of the streams "NVPD" (training, step = the count of training batches taken) and "NVPV" (validation and log_likelihood,
step = the batch's index), the loss, and the sampler's normals ("NVPS") -- the same kernels (gm_nvp_pre, gm_nvp_loss,
gm_nvp_post) and the same tags.

Coupling k.  linear = Linear(Dc, H) with relu, then out = Linear(H, P Dt), P = 3 bins - 1; out.weight and out.bias are
zero at construction.  Column p Dt + j of out's output ST is parameter p of pixel j (parameter-major: RealNVP's [s | t]
layout, every parameter load coalesced across a wave); parameters 0 .. bins - 1 are theta_w, the next bins theta_h, the
last bins - 1 theta_d.  state_dict keys: couplings.{k}.linear.{weight,bias} and couplings.{k}.out.{weight,bias}.

Spline of one pixel.  B = tail_bound, m = MIN_BIN = 1e-3 for all three minima (the paper's defaults; fixed).
w_i = 2 B (m + (1 - m bins) softmax(theta_w)_i);  knots x_0 = -B, x_i = -B + (w_0 + .. + w_{i-1}) summed left to right,
x_bins = B exactly;  heights h_i and knots y_i likewise from theta_h.  d_0 = d_bins = 1 and, for 1 <= i < bins, d_i =
m + softplus(theta_d_{i-1} + c), c = log(exp(1 - m) - 1): theta = 0 gives slope 1, so a fresh model is the identity flow
to rounding.  If x <= -B or x >= B:  y = x, the pixel's log-determinant is 0, the gradient of every one of its P
parameters is 0 and dx = g.  Otherwise the bin k is the number of interior knots x_1 .. x_{bins-1} with x >= x_i;
xi = (x - x_k) / w_k clamped to [0, 1], s = h_k / w_k, q = s + (d_{k+1} + d_k - 2 s) xi (1 - xi), and
    y = y_k + h_k (s xi^2 + d_k xi (1 - xi)) / q,
    log dy/dx = 2 log s + log(d_{k+1} xi^2 + 2 s xi (1 - xi) + d_k (1 - xi)^2) - 2 log q.
Inverse: the bin is found on the y knots in the same way; with dl = y - y_k and t = d_{k+1} + d_k - 2 s:  a = h_k (s -
d_k) + dl t, b = h_k d_k - dl t, c = -s dl, xi = 2 c / (-b - sqrt(max(b^2 - 4 a c, 0))), x = x_k + xi w_k.  The row's
logdet gains the sum over j.  (Eq. 4-8 of the paper with linear tails.)  The softplus and both softmaxes are computed in
their stable forms.

Loss, gradients, sampling, encode / decode, log_likelihood.  RealNVP's contract: nll_r = 0.5 sum z^2 + 0.5 D log(2 pi) -
logdet_pre_r - logdet_r + D log(levels), the batch loss its mean, dz = z / b, the log-determinant's cotangent -1 / b;
samples are the "NVPS" normals times the temperature through the couplings inverted last to first.

Fused path: SplineFlowEngine below (csrc/gm_nsf.hip, the arithmetic in csrc/gm_nsf.h) -- RealNVP's
batch with the two coupling launches swapped for gm_nsf_couple / gm_nsf_couple_bwd and ST / dST P Dt wide: 7 K + 3
launches per training batch, 3 K + 4 per validation batch, 3 K + 2 for sampling.  An overridden compute_batch / evaluate
or an edited model: the general loop -- autograd over ops.fused_linear plus the torch ops of `spline` below on the same
u."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops
from ._lib import NSF_MAX_BINS, NSF_MAX_TAIL, NSF_MIN_BINS, GMError
from .realnvp import (CouplingFlow, CouplingFlowTrainer, RealNVPEngine, check_coupling_shape, check_flow_settings)
from .trainers import _stock_module, stock, stock_model

MIN_BIN = 1e-3                                   # m: csrc/gm_nsf.h NSF_MIN_BIN
SLOPE_SHIFT = math.log(math.exp(1.0 - MIN_BIN) - 1.0)
BINS = (NSF_MIN_BINS, 8, NSF_MAX_BINS)


class SplineFlowError(GMError, ValueError):
    """A bad image size, width, coupling count, bin count, tail bound, mask, alpha, levels, seed, n or temperature: a
    ValueError, and a GMError like the package's other refusals."""


def check_config(image_size, hidden_dim, num_couplings, num_bins, tail_bound, mask, alpha, levels):
    """(D, H, K, bins, tail_bound, mask, alpha, levels) validated against the kernels' limits; else SplineFlowError."""
    D, H, K, mask = check_coupling_shape(image_size, hidden_dim, num_couplings, mask, SplineFlowError)
    bins = _lib.check_int(num_bins, "num_bins", SplineFlowError)
    tail = _lib.check_real(tail_bound, "tail_bound", SplineFlowError)
    if bins not in BINS:
        raise SplineFlowError("num_bins must be one of %s, got %d" % (BINS, bins))
    if not (0.0 < tail <= NSF_MAX_TAIL and 0.0 < float(np.float32(tail)) <= NSF_MAX_TAIL):
        raise SplineFlowError("tail_bound must lie in (0, %d], got %r" % (NSF_MAX_TAIL, tail))
    alpha, levels, _ = check_flow_settings(alpha, levels, 1.0, SplineFlowError)
    return D, H, K, bins, tail, mask, alpha, levels


# ---- the spline by torch ops: the general path's, and the fp32 statement of the kernel's --------------------------------
def _sizes(theta, B):
    return 2 * B * (MIN_BIN + (1 - MIN_BIN * theta.shape[-1]) * torch.softmax(theta, -1))


def _knots(w, B):
    """[..., bins + 1]: -B, the running sums of w taken left to right, B."""
    out, c = [torch.full_like(w[..., 0], -B)], torch.zeros_like(w[..., 0])
    for i in range(w.shape[-1] - 1):
        c = c + w[..., i]
        out.append(-B + c)
    out.append(torch.full_like(w[..., 0], B))
    return torch.stack(out, -1)


def _bin_of(st, v, bins, B, on_y):
    """The quantities of every pixel's bin, (x_k, w_k, y_k, h_k, d_k, d_{k+1}), found on the x knots or on the y knots."""
    P, dt = 3 * bins - 1, v.shape[1]
    th = st[:, :P * dt].reshape(st.shape[0], P, dt).permute(0, 2, 1)
    w, h = _sizes(th[..., :bins], B), _sizes(th[..., bins:2 * bins], B)
    a = th[..., 2 * bins:] + SLOPE_SHIFT
    one = torch.ones_like(w[..., :1])
    d = torch.cat([one, MIN_BIN + (torch.clamp(a, min=0.0) + torch.log1p(torch.exp(-a.abs()))), one], -1)
    xs, ys = _knots(w, B), _knots(h, B)
    k = (v[..., None] >= (ys if on_y else xs)[..., 1:bins]).sum(-1, keepdim=True)
    pick = lambda t, k: torch.gather(t, -1, k)[..., 0]
    return pick(xs, k), pick(w, k), pick(ys, k), pick(h, k), pick(d, k), pick(d, k + 1)


def spline(st, x, bins, tail_bound):
    """(y [n, Dt], the rows' sum of log dy/dx [n]) of x [n, Dt] under the parameter-major rows st [n, P Dt]."""
    B = float(tail_bound)
    inside = (x > -B) & (x < B)
    xin = torch.where(inside, x, torch.zeros_like(x))
    xk, wk, yk, hk, dk, dk1 = _bin_of(st, xin, bins, B, False)
    xi = torch.clamp((xin - xk) / wk, 0.0, 1.0)
    s, r = hk / wk, xi * (1 - xi)
    q = s + (dk1 + dk - 2 * s) * r
    y = yk + hk * (s * xi * xi + dk * r) / q
    ld = 2 * torch.log(s) + torch.log(dk1 * xi * xi + 2 * s * r + dk * (1 - xi) * (1 - xi)) - 2 * torch.log(q)
    return torch.where(inside, y, x), torch.where(inside, ld, torch.zeros_like(ld)).sum(1)


def spline_inverse(st, y, bins, tail_bound):
    """x [n, Dt] with spline(st, x)[0] == y."""
    B = float(tail_bound)
    inside = (y > -B) & (y < B)
    yin = torch.where(inside, y, torch.zeros_like(y))
    xk, wk, yk, hk, dk, dk1 = _bin_of(st, yin, bins, B, True)
    s, dl = hk / wk, yin - yk
    t = dk1 + dk - 2 * s
    a, b, c = hk * (s - dk) + dl * t, hk * dk - dl * t, -s * dl
    xi = 2 * c / (-b - torch.sqrt(torch.clamp(b * b - 4 * a * c, min=0.0)))
    return torch.where(inside, xk + xi * wk, y)


# ---- modules ---------------------------------------------------------------------------------------------------------
@stock_model
class SplineCoupling(nn.Module):
    """One conditioner: linear (Dc -> H, relu) and out (H -> (3 bins - 1) Dt), out starting at zero."""

    def __init__(self, cond_dim, trans_dim, hidden_dim, num_bins):
        super().__init__()
        self.linear = nn.Linear(cond_dim, hidden_dim)
        self.out = nn.Linear(hidden_dim, (3 * num_bins - 1) * trans_dim)
        with torch.no_grad():
            self.out.weight.zero_()
            self.out.bias.zero_()

    def forward(self, x_c):
        """ST [n, P Dt] of the conditioning half, parameter-major."""
        if not x_c.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: got a %s tensor and there is no CPU "
                          "fallback (move the model and inputs with to_cuda)" % x_c.device)
        h = ops.fused_linear(x_c.contiguous(), self.linear.weight, self.linear.bias, "relu")
        return ops.fused_linear(h, self.out.weight, self.out.bias, "id")


@stock_model
class SplineFlow(CouplingFlow):
    """K rational-quadratic spline couplings over the two halves of a logit-space image."""

    def __init__(self, image_size=784, hidden_dim=400, num_couplings=4, num_bins=8, tail_bound=3.0, mask="checker",
                 alpha=0.05, levels=256):
        super().__init__()
        (self.image_size, self.hidden_dim, self.num_couplings, self.num_bins, self.tail_bound, self.mask, self.alpha,
         self.levels) = check_config(image_size, hidden_dim, num_couplings, num_bins, tail_bound, mask, alpha, levels)
        self._halves(lambda dc, dt: SplineCoupling(dc, dt, self.hidden_dim, self.num_bins))

    def _transform(self, k, x_t, x_c):
        return spline(self.couplings[k](x_c), x_t, self.num_bins, self.tail_bound)

    def _untransform(self, k, y_t, x_c):
        return spline_inverse(self.couplings[k](x_c), y_t, self.num_bins, self.tail_bound)


def spline_fused_ok(model):
    """True iff the model is SplineFlow itself with its couplings unchanged and consistent shapes and settings."""
    if not type(model).__dict__.get("_gm_stock_model", False) or type(model) is not SplineFlow:
        return False
    kids = list(model.children())
    cs = getattr(model, "couplings", None)
    if len(kids) != 1 or kids[0] is not cs or type(cs) is not nn.ModuleList:
        return False
    try:
        D, H, K, bins = check_config(model.image_size, model.hidden_dim, model.num_couplings, model.num_bins,
                                     model.tail_bound, model.mask, model.alpha, model.levels)[:4]
    except (SplineFlowError, AttributeError):
        return False
    if len(cs) != K:
        return False
    Da, Db = (D + 1) // 2, D // 2
    for k, c in enumerate(cs):
        dc, dt = (Da, Db) if k % 2 == 0 else (Db, Da)
        if not (type(c) is SplineCoupling and _stock_module(c, 2) and type(getattr(c, "linear", None)) is nn.Linear
                and type(getattr(c, "out", None)) is nn.Linear and c.linear.bias is not None and c.out.bias is not None
                and tuple(c.linear.weight.shape) == (H, dc) and tuple(c.out.weight.shape) == ((3 * bins - 1) * dt, H)):
            return False
    return True


# ---- engine ----------------------------------------------------------------------------------------------------------
class SplineFlowEngine(RealNVPEngine):
    """RealNVPEngine's batch -- the gather, gm_nvp_pre, K x (two forwards, the coupling), gm_nvp_loss, K x (the
    coupling's backward, the two input gradients, both weight gradients + Adam as a pair), the loss sum with the counter
    tick: 7 K + 3 launches, a validation batch 3 K + 4 -- with gm_nsf_couple / gm_nsf_couple_bwd as the coupling's two
    launches and ST / dST (3 bins - 1) Dt wide.  One GPU only."""

    one_gpu = "the neural spline flow engine"
    fused_ok = staticmethod(spline_fused_ok)
    refusal = ("SplineFlow", "nsf.SplineFlow", "couplings")

    def _st_width(self, dt):
        return (3 * self.model.num_bins - 1) * dt

    def _couple(self, st, k, xt, b):
        from . import ops_fused as of_
        m = self.model
        of_.nsf_couple(self.ST[k], xt, self.Y[k], b, self._dt(k), m.num_bins, m.tail_bound, logdet=self.logdet, stream=st)

    def _couple_bwd(self, st, k, xt, g, dST, b, c):
        from . import ops_fused as of_
        m = self.model
        of_.nsf_couple_bwd(self.ST[k], xt, g, dST, b, self._dt(k), m.num_bins, m.tail_bound, c, dx=self.dX[k], stream=st)

    def _settings(self):
        m = self.model
        return {"mask": str(m.mask), "alpha": float(m.alpha), "levels": int(m.levels), "num_bins": int(m.num_bins),
                "tail_bound": float(m.tail_bound), "seed": int(self.trainer.seed)}


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class SplineFlowTrainer(CouplingFlowTrainer):
    """Trains a SplineFlow on its exact (dequantised) negative log-likelihood; samples, encodes and decodes: RealNVP's
    trainer protocol (sample, encode, decode, log_likelihood, bits_per_dim; sampling is 3 K + 2 launches for a stock
    model).  Histories: `losses` (the NLL in nats per image, one per training batch); the epoch line (mean training NLL,
    validation NLL); checkpoints (+ mask, alpha, levels, num_bins, tail_bound, seed in the optimizer state's config,
    checked under strict=True, and the number of training batches taken, so a resumed run continues the noise stream
    bit for bit).  One GPU only."""
    _one_gpu = "SplineFlowTrainer"
    _error = SplineFlowError
    _fused_ok = staticmethod(spline_fused_ok)

    def _flow_settings(self):
        m = self.model
        return m.alpha, m.levels, None               # no s_cap

    def _engine_class(self):
        return SplineFlowEngine

    def train(self, num_epochs, lr=1e-3, weight_decay=0.0, quiet=False):
        """VAETrainer.train with this model's defaults."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    def _couple_rows(self, st, inp, out, logdet=None, inverse=False):
        from . import ops_fused as of_
        m = self.model
        of_.nsf_couple(st, inp, out, inp.shape[0], inp.shape[1], m.num_bins, m.tail_bound, logdet=logdet, inverse=inverse)


__all__ = ["SplineCoupling", "SplineFlow", "SplineFlowTrainer", "SplineFlowEngine", "SplineFlowError", "spline",
           "spline_inverse", "spline_fused_ok", "check_config", "MIN_BIN"]
