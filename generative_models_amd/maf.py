"""Masked autoregressive flow, MAF (Papamakarios, Pavlakou & Murray, "Masked Autoregressive Flow for Density Estimation",
arXiv 1705.07057): a stack of MADEs (made.py) with Gaussian conditionals -- an invertible flow over dequantised grey-level
images in which every pixel is conditioned on every earlier pixel.  RealNVP (realnvp.py) is the special case whose
conditioner sees one half of the image.  Exported by src/maf.py as MAF / MAFTrainer.

The contract.

Model.  MAF(image_size D = 784, hidden_dim H = 400, num_layers K = 5, order = "natural", order_seed = 0).  Limits:
2 <= D <= 8192, 1 <= H <= 1024, 1 <= K <= 16; anything else raises MAFError(GMError, ValueError) in the constructor.
layers = ModuleList of K MAFLayer modules, each linear = Linear(D, H), out = Linear(H, 2 D) -- rows 0 .. D - 1 of out the
shift m, rows D .. 2 D - 1 the log-scale pre-activation a -- and two persistent int32 buffers m_in [D] and m_h [H] in the
state_dict (a checkpoint carries the order).  state_dict keys: layers.{k}.linear.{weight,bias}, layers.{k}.out.{weight,
bias}, layers.{k}.m_in, layers.{k}.m_h.  out.weight and out.bias are zero at construction, so a fresh model is the
identity flow.

Degrees.  m_h[j] = 1 + floor(j (D - 1) / H), MADE's rule, the same in every layer.  Layer 0's m_in is the order (made.py:
"natural" m_in[i] = i + 1; "random" 1 + numpy.random.RandomState(order_seed).permutation(D)); layer k's is the reverse of
layer k - 1's, D + 1 - m_in.  Masks, computed from the degrees wherever they are needed, never stored as matrices on the
device:  linear.weight keeps (j, i) iff m_h[j] >= m_in[i];  both halves of out.weight keep (d, j) iff m_in[d] > m_h[j].
The pixel of degree 1 sees nothing: its shift and log-scale are its biases.

Masked parameters.  The parameters hold the masked values: the masked entries of linear.weight and out.weight are
exactly 0.0 after construction and after every optimiser step, on every path, so a forward pass needs no mask.

Layer map, data -> noise.  h = relu(linear(y));  [m | a] = out(h);  s = s_cap tanh(a) (nvp_s of csrc/gm_nvp.h);
u = (y - m) exp(-s);  logdet -= sum_d s_d.  The layers apply in order 0 .. K - 1; z is the last layer's u.
Inverse, in order of degree:  y_d = u_d exp(s_d) + m_d, the product rounded before the add, where m_d and s_d read the y
of lower degree only; the layers are inverted last to first.

Preprocessing, post-processing, noise.  RealNVP's (realnvp.py), with the trainer's alpha, levels and s_cap (0 <= alpha <
0.5, 2 <= levels <= 65536, 0 < s_cap <= 8):  y = logit(alpha + (1 - 2 alpha) (q + u) / levels) with its log-determinant,
u = ph_unit of word e & 3 of Philox4x32-10 at counter (e >> 2, step, row, TAG) under key (seed mod 2^32, seed >> 32).
Training: TAG_TRAIN = "MAFD", step = the count of training batches taken.  Validation, encode and log_likelihood:
TAG_EVAL = "MAFV", step = the batch's index in that pass.  x = clamp((sigmoid(y) - alpha) / (1 - 2 alpha), 0, 1).

Prior and loss.  z ~ N(0, I).  Per row  nll_r = 0.5 |z|^2 - logdet_pre_r - logdet_r + cst,  cst = 0.5 D log(2 pi) +
D log(levels), in nats per image; the batch loss is the mean over rows: dz = z / b, the log-determinant's cotangent
-1 / b.

Sampling.  z of element e of sample row r is RealNVP's sampler normal (the Box-Muller value of Philox counter (e >> 2,
0, r, realnvp.TAG_S)) times the temperature: indexed by row and element, so a row's bits depend on (seed, row) and the
weights alone.

Fused path: MAFEngine below (csrc/gm_maf.hip) -- per training batch the gather, gm_nvp_pre, K x (two
forwards, gm_maf_couple), gm_nvp_loss, K x (gm_maf_couple_bwd, the input gradients, both weight gradients + Adam as a pair,
gm_maf_mask) and the loss sum with the counter tick: 8 K + 3 launches.  Sampling is the prior normals, K x gm_maf_invert
(one launch per layer: a row's H pre-activations stay in registers and are updated pixel by pixel) and gm_nvp_post: K + 2
launches plus the K transposed copies of linear.weight.  An overridden compute_batch / evaluate or an edited model: the
general loop -- autograd over ops.fused_linear with weight * mask and torch ops on the same u -- and a sampler of D passes
per layer."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, made, ops, realnvp
from ._lib import MAF_MAX_D, MAF_MAX_H, MAF_MAX_K, MAF_MIN_D, MAF_TAG_EVAL, MAF_TAG_TRAIN, GMError
from .trainers import FlatAdam, _stock_module, stock, stock_model  # noqa: F401
from .engine import OneNetEngine, _Linear

TAG_TRAIN, TAG_EVAL, TAG_S = MAF_TAG_TRAIN, MAF_TAG_EVAL, realnvp.TAG_S
ORDERS = made.ORDERS


class MAFError(GMError, ValueError):
    """A bad image size, width, layer count, order, alpha, levels, s_cap, seed, n or temperature: a ValueError, and a
    GMError like the package's other refusals."""


def _int(v, name):
    return _lib.check_int(v, name, MAFError)


def check_seed(seed, name="seed"):
    return _lib.check_seed(seed, name, MAFError)


def check_config(image_size, hidden_dim, num_layers, order, order_seed):
    """(D, H, K, order, order_seed) validated against the kernels' limits; else MAFError."""
    D, H, K = _int(image_size, "image_size"), _int(hidden_dim, "hidden_dim"), _int(num_layers, "num_layers")
    if not MAF_MIN_D <= D <= MAF_MAX_D:
        raise MAFError("image_size must lie in [%d, %d], got %d" % (MAF_MIN_D, MAF_MAX_D, D))
    if not 1 <= H <= MAF_MAX_H:
        raise MAFError("hidden_dim must lie in [1, %d], got %d" % (MAF_MAX_H, H))
    if not 1 <= K <= MAF_MAX_K:
        raise MAFError("num_layers must lie in [1, %d], got %d" % (MAF_MAX_K, K))
    if not isinstance(order, str) or order not in ORDERS:
        raise MAFError("order must be one of %s, got %r" % (ORDERS, order))
    order_seed = _int(order_seed, "order_seed")
    if not 0 <= order_seed < 1 << 32:
        raise MAFError("order_seed must lie in [0, 2^32), got %d" % order_seed)
    return D, H, K, order, order_seed


def check_settings(alpha, levels, s_cap):
    """(alpha, levels, s_cap) of a trainer, validated against the kernels' limits; else MAFError."""
    return realnvp.check_flow_settings(alpha, levels, s_cap, MAFError)


# ---- the degrees and the masks in numpy (the tests' reference reads the same contract) ---------------------------------
def degrees(image_size, hidden_dim, num_layers, order="natural", order_seed=0):
    """([m_in of layer 0, ..., m_in of layer K - 1], m_h): int32 arrays."""
    D, H, K, order, order_seed = check_config(image_size, hidden_dim, num_layers, order, order_seed)
    m_in, m_h = made.degrees(D, H, order, order_seed)
    ins = [m_in]
    for _ in range(1, K):
        ins.append((D + 1 - ins[-1]).astype(np.int32))
    return ins, m_h


def masks(m_in, m_h):
    """(M1 [H, D], M2 [D, H]) boolean, from the degree vectors; M2 masks both halves of out.weight."""
    return made.masks(m_in, m_h)


def inverse_order(m_in):
    """inv_order [D] int32: the pixel of degree t + 1 at position t; MAFError when m_in is no permutation."""
    try:
        return made.inverse_order(m_in)
    except made.MADEError as e:
        raise MAFError(str(e)) from None


def uniforms_reference(n, D, seed, step, tag=TAG_TRAIN, row0=0):
    """u [n, D] float32: the dequantisation noise by the contract's rule, bit for bit."""
    return realnvp.uniforms_reference(n, D, seed, step, tag, row0)


def normals_reference(n, D, seed, row0=0):
    """z [n, D] float64: the sampler's starting normals by the contract's rule (the device rounds to fp32)."""
    return realnvp.normals_reference(n, D, seed, row0)


nll_constant, preprocess, postprocess, nll_rows = (realnvp.nll_constant, realnvp.preprocess, realnvp.postprocess,
                                                   realnvp.nll_rows)


# ---- modules ---------------------------------------------------------------------------------------------------------
@stock_model
class MAFLayer(nn.Module):
    """One MADE with Gaussian conditionals: linear (D -> H, relu) and out (H -> 2 D, [m | a]), both masked by the degree
    buffers m_in / m_h; out starts at zero."""

    def __init__(self, m_in, m_h):
        super().__init__()
        D, H = int(m_in.size), int(m_h.size)
        self.linear = nn.Linear(D, H)
        self.out = nn.Linear(H, 2 * D)
        self.register_buffer("m_in", torch.from_numpy(np.ascontiguousarray(m_in, dtype=np.int32)))
        self.register_buffer("m_h", torch.from_numpy(np.ascontiguousarray(m_h, dtype=np.int32)))
        with torch.no_grad():
            self.out.weight.zero_()
            self.out.bias.zero_()
        self.apply_masks()

    def masks(self):
        """(M1 [H, D], M2 [2 D, H]) as float32 tensors on the buffers' device, computed on the spot."""
        M1, M2 = masks(self.m_in, self.m_h)
        return M1.to(torch.float32), torch.cat([M2, M2]).to(torch.float32)

    @torch.no_grad()
    def apply_masks(self):
        """Zeroes the masked entries of both weights in place (the constructor's last step)."""
        M1, M2 = self.masks()
        self.linear.weight.mul_(M1)
        self.out.weight.mul_(M2)

    def forward(self, y):
        """[m | a] [n, 2 D] of y [n, D]; the weights enter as weight * mask, so masked gradients are zero."""
        if not y.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: got a %s tensor and there is no CPU "
                          "fallback (move the model and inputs with to_cuda)" % y.device)
        M1, M2 = self.masks()
        h = ops.fused_linear(y.contiguous(), self.linear.weight * M1, self.linear.bias, "relu")
        return ops.fused_linear(h, self.out.weight * M2, self.out.bias, "id")


@stock_model
class MAF(nn.Module):
    """K masked autoregressive layers over a logit-space image, consecutive layers in reversed pixel order."""

    def __init__(self, image_size=784, hidden_dim=400, num_layers=5, order="natural", order_seed=0):
        super().__init__()
        (self.image_size, self.hidden_dim, self.num_layers, self.order,
         self.order_seed) = check_config(image_size, hidden_dim, num_layers, order, order_seed)
        ins, m_h = degrees(self.image_size, self.hidden_dim, self.num_layers, self.order, self.order_seed)
        self.layers = nn.ModuleList([MAFLayer(m_in, m_h) for m_in in ins])
        self.shape = int(self.image_size ** 0.5)

    def flow(self, y, s_cap):
        """(z [n, D], logdet [n]) of logit-space rows y, by autograd-able torch ops over the fused linear kernels."""
        D = self.image_size
        logdet = torch.zeros(y.shape[0], dtype=y.dtype, device=y.device)
        for layer in self.layers:
            ma = layer(y)
            s = s_cap * torch.tanh(ma[:, D:])
            y = (y - ma[:, :D]) * torch.exp(-s)
            logdet = logdet - s.sum(1)
        return y, logdet

    def inverse(self, z, s_cap):
        """y [n, D] with flow(y)[0] == z: the layers inverted last to first, each through D passes in order of degree."""
        D = self.image_size
        with torch.no_grad():
            for layer in reversed(self.layers):
                inv = inverse_order(layer.m_in)
                y = torch.zeros_like(z)
                for t in range(D):
                    d = int(inv[t])
                    ma = layer(y)
                    y[:, d] = z[:, d] * torch.exp(s_cap * torch.tanh(ma[:, D + d])) + ma[:, d]
                z = y
        return z

    def forward(self, y, s_cap=2.0):
        return self.flow(y, s_cap)


def maf_fused_ok(model):
    """True iff the model is MAF itself with its layers unchanged and consistent shapes and degree buffers."""
    if not type(model).__dict__.get("_gm_stock_model", False) or type(model) is not MAF:
        return False
    kids = list(model.children())
    ls = getattr(model, "layers", None)
    if len(kids) != 1 or kids[0] is not ls or type(ls) is not nn.ModuleList:
        return False
    try:
        D, H, K, _, _ = check_config(model.image_size, model.hidden_dim, model.num_layers, model.order, model.order_seed)
    except (MAFError, AttributeError):
        return False
    if len(ls) != K:
        return False
    for c in ls:
        if not (type(c) is MAFLayer and _stock_module(c, 2) and type(getattr(c, "linear", None)) is nn.Linear
                and type(getattr(c, "out", None)) is nn.Linear and c.linear.bias is not None and c.out.bias is not None
                and tuple(c.linear.weight.shape) == (H, D) and tuple(c.out.weight.shape) == (2 * D, H)):
            return False
        m_in, m_h = getattr(c, "m_in", None), getattr(c, "m_h", None)
        if not (all(torch.is_tensor(t) and t.dtype == torch.int32 for t in (m_in, m_h)) and m_in.numel() == D
                and m_h.numel() == H):
            return False
    return True


# ---- engine ----------------------------------------------------------------------------------------------------------
class MAFEngine(OneNetEngine):
    """MAF on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  Per training
    batch: 1. gm_gather_rows[_bits];  2. gm_nvp_pre (the HALF split with both halves inside Y[0]);  3. K x (H1 =
    relu(linear(Y[k])), MA = out(H1), gm_maf_couple -> Y[k + 1]);  4. gm_nvp_loss (dZ, row partials);  5. for k = K - 1 ..
    0: gm_maf_couple_bwd (dOUT and the direct cotangent dY), dH = dOUT Wout [H1 > 0], for k > 0 the input's cotangent
    dH Wlin + dY in the GEMM's epilogue -- both input gradients BEFORE the pair that steps the layer's weights -- the two
    weight gradients + Adam as a pair, and gm_maf_mask: the pair's epilogue steps every entry, masked ones included, so
    W and both moments are zeroed at the masked entries;  6. the loss sum with the counter tick.  Every layer keeps its
    H1, MA and output: nothing is recomputed.  A validation batch is launches 1-4 (no dZ) and the sum.  The noise step
    of a training batch is ctr + nbase, of a validation batch ctr (the batch's index in the pass).  The degree vectors
    are launch arguments: the graphs are dropped when the model's buffers move.  One GPU only."""

    one_gpu = "the MAF engine"
    fused_ok = staticmethod(maf_fused_ok)
    refusal = ("MAF", "maf.MAF", "layers")       # the trainer: seed, alpha, levels, s_cap and noise_steps

    def _params(self, model):
        return [p for c in model.layers for p in (c.linear.weight, c.linear.bias, c.out.weight, c.out.bias)]

    def _setup(self, model):
        self.C = [(_Linear(self.fp, c.linear), _Linear(self.fp, c.out)) for c in model.layers]
        self.D, self.H, self.K = model.image_size, model.hidden_dim, model.num_layers
        self.I = self.D

    def _buffers(self, B):
        z = lambda *s: torch.zeros(*s, device=self.device)
        D, H, K = self.D, self.H, self.K
        self.X = z(B, D)
        self.Y = [z(B, D) for _ in range(K + 1)]     # Y[0]: the preprocessed rows; Y[k + 1]: layer k's u
        self.H1 = [z(B, H) for _ in range(K)]
        self.MA = [z(B, 2 * D) for _ in range(K)]
        self.logdet, self.part = z(B), z(B)
        self.dZ, self.dOUT, self.dH, self.dY = z(B, D), z(B, 2 * D), z(B, H), z(B, D)
        self.G = (z(B, D), z(B, D))                  # the cotangent of layer k's input lives in G[k % 2]

    def _settings(self):
        m, tr = self.model, self.trainer
        return {"order": str(m.order), "order_seed": int(m.order_seed), "alpha": float(tr.alpha),
                "levels": int(tr.levels), "s_cap": float(tr.s_cap), "seed": int(tr.seed)}

    def _graph_args(self):
        return tuple(t.data_ptr() for c in self.model.layers for t in (c.m_in, c.m_h))

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        """VAEEngine.configure: the settings above are compared with a checkpoint's before anything is allocated or
        reset, and are launch arguments of the graphs, with the seed.  Whatever was loaded into the model, training starts
        from masked weights (resumed moments are masked already)."""
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)
        from . import ops_fused as of_
        for (L1, L2), c in zip(self.C, self.model.layers):
            of_.maf_mask(L1.W, L2.W, c.m_in, c.m_h)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: preprocessing, the K layers, the loss (+ backward, Adam and the masks when train)."""
        from . import ops_fused as of_
        m, tr, K, D = self.model, self.trainer, self.K, self.D
        idx_slot = self._slot(t, 1, 0, self.R, self.B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        ops.gather_rows(self.data, self.idx_ring.view(-1), self.X, B=b, idx_slot=idx_slot, stream=st)
        of_.nvp_pre(self.X, *of_.maf_halves(self.Y[0], D), self.logdet, b, tr.seed, TAG_TRAIN if train else TAG_EVAL,
                    tr.alpha, tr.levels, "half", stream=st, **self._clock(t, train))
        for k, (L1, L2) in enumerate(self.C):
            ops.linear_fwd(self.Y[k], L1.W, L1.b, self.H1[k], "relu", M=b, stream=st)
            ops.linear_fwd(self.H1[k], L2.W, L2.b, self.MA[k], "id", M=b, stream=st)
            of_.maf_couple(self.Y[k], self.MA[k], self.Y[k + 1], self.logdet, b, D, tr.s_cap, stream=st)
        scale = float(np.float32(1.0 / b))
        cst = float(np.float32(nll_constant(D, tr.levels)))
        dza, dzb = of_.maf_halves(self.dZ, D) if train else (None, None)
        of_.nvp_loss(*of_.maf_halves(self.Y[K], D), self.logdet, self.part, b, cst, scale=scale, dza=dza, dzb=dzb,
                     stream=st)
        if train:
            adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
            for k in range(K - 1, -1, -1):
                L1, L2 = self.C[k]
                c = m.layers[k]
                g = self.dZ if k == K - 1 else self.G[(k + 1) % 2]
                of_.maf_couple_bwd(self.MA[k], self.Y[k + 1], g, self.dOUT, b, D, tr.s_cap, -scale,
                                   dy=self.dY if k > 0 else None, stream=st)
                # both input gradients read the layer's weights BEFORE the paired dW(+Adam) launch updates them
                ops.linear_bwd_dx(self.dOUT, L2.W, self.dH, below=self.H1[k], epi="relu", M=b, stream=st)
                if k > 0:
                    ops.linear_bwd_dx(self.dH, L1.W, self.G[k % 2], M=b, add=self.dY, stream=st)
                ops.linear_bwd_dw_adam_pair(dict(dA=self.dOUT, X=self.H1[k], lin=L2, adam=adam, M=b),
                                            dict(dA=self.dH, X=self.Y[k], lin=L1, adam=adam, M=b),
                                            weight_decay=self.wd, stream=st)
                of_.maf_mask(L1.W, L2.W, c.m_in, c.m_h, moments1=(L1.mW, L1.vW), moments2=(L2.mW, L2.vW), stream=st)
        of_.sum_finalize(self.part, b, self.recon if train else self.vrecon, scale=scale, out_slot=loss_slot,
                         tick=self.ctr if self.use_graph else None, stream=st)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class MAFTrainer(realnvp.DequantFlowTrainer):
    """Trains a MAF on its exact (dequantised) negative log-likelihood; samples, encodes and decodes: a
    DequantFlowTrainer (realnvp.py) whose code is z itself and whose alpha, levels and s_cap are the trainer's
    (sampling is K + 2 launches plus the K transposed copies for a stock model).  Histories: `losses` (the NLL in nats
    per image, one per training batch); the epoch line (mean training NLL, validation NLL); best_val_loss / best_model
    as the other VAE-family trainers; checkpoints (+ order, order_seed, alpha, levels, s_cap, seed in the optimizer
    state's config, checked under strict=True, and the number of training batches taken, so a resumed run continues the
    noise stream bit for bit).  One GPU only."""
    _one_gpu = "MAFTrainer"
    _error = MAFError
    _fused_ok = staticmethod(maf_fused_ok)
    _tag_train, _tag_eval = TAG_TRAIN, TAG_EVAL

    def __init__(self, model, train_iter, val_iter, test_iter, seed=0, alpha=0.05, levels=256, s_cap=2.0, viz=False):
        self.seed = check_seed(seed)                 # both before anything runs, the seed's refusal first
        self.alpha, self.levels, self.s_cap = check_settings(alpha, levels, s_cap)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz, seed=self.seed)

    def _settings_ok(self):
        try:
            check_settings(self.alpha, self.levels, self.s_cap)
            return True
        except MAFError:
            return False

    def _stock(self):
        return super()._stock() and self._settings_ok()

    def _flow_settings(self):
        return self.alpha, self.levels, self.s_cap

    def _model_flow(self, y):
        return self.model(y, self.s_cap)

    def _engine_class(self):
        return MAFEngine

    def train(self, num_epochs, lr=1e-3, weight_decay=0.0, quiet=False):
        """VAETrainer.train with this model's defaults (general path: weight * mask in the forward keeps every masked
        gradient, Adam moment and entry at zero)."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    # ---- the flow on device rows, no autograd --------------------------------------------------------------------------
    def _forward_rows(self, x, seed, tag, step, row0=0):
        """(z [n, D], nll [n]) of device rows x under the noise of (seed, tag, step, row0 ..): the kernels for a stock
        model, the model's own forward on the same u otherwise."""
        from . import ops_fused as of_
        m, n, D = self.model, x.shape[0], self.model.image_size
        with torch.no_grad():
            if not maf_fused_ok(m):
                u = of_.nvp_uniforms(n, D, seed, tag, step=step, row0=row0, device=x.device)
                y, ld0 = preprocess(x, u, self.alpha, self.levels)
                z, ld = m(y, self.s_cap)
                return z.contiguous(), nll_rows(z, ld0, ld, D, self.levels)
            y = torch.empty(n, D, device=x.device)
            logdet, part = torch.empty(n, device=x.device), torch.empty(n, device=x.device)
            of_.nvp_pre(x, *of_.maf_halves(y, D), logdet, n, seed, tag, self.alpha, self.levels, "half", step=step,
                        row0=row0)
            for c in m.layers:
                h = torch.empty(n, m.hidden_dim, device=x.device)
                ma, u = torch.empty(n, 2 * D, device=x.device), torch.empty(n, D, device=x.device)
                ops.linear_fwd(y, c.linear.weight.detach(), c.linear.bias.detach(), h, "relu")
                ops.linear_fwd(h, c.out.weight.detach(), c.out.bias.detach(), ma, "id")
                of_.maf_couple(y, ma, u, logdet, n, D, self.s_cap)
                y = u
            of_.nvp_loss(*of_.maf_halves(y, D), logdet, part, n, float(np.float32(nll_constant(D, self.levels))))
            return y, part

    def _invert_rows(self, z):
        """y [n, D] in logit space of latent rows z: the layers inverted last to first, one gm_maf_invert launch each for
        a stock model, D passes per layer otherwise."""
        from . import ops_fused as of_
        m = self.model
        with torch.no_grad():
            if not maf_fused_ok(m):
                return m.inverse(z, self.s_cap).contiguous()
            for c in reversed(m.layers):
                inv = torch.from_numpy(inverse_order(c.m_in)).to(z.device)
                W1T = c.linear.weight.detach().t().contiguous()
                z = of_.maf_invert(z, c.out.weight.detach(), c.out.bias.detach(), W1T, c.linear.bias.detach(), c.m_h, inv,
                                   self.s_cap)
            return z

    def _inverse_rows(self, z):
        """x [n, D] in [0, 1] of latent rows z: the inverse flow, then gm_nvp_post."""
        from . import ops_fused as of_
        D = self.model.image_size
        y = self._invert_rows(z)
        if not maf_fused_ok(self.model):
            return postprocess(y, self.alpha).contiguous()
        x = torch.empty(y.shape[0], D, device=y.device)
        of_.nvp_post(*of_.maf_halves(y, D), x, y.shape[0], self.alpha, "half")
        return x

    def _prior(self, n, seed, temperature):
        """The sampler's starting normals z [n, D]: gm_nvp_post's PRIOR mode under the HALF split."""
        from . import ops_fused as of_
        D = self.model.image_size
        z = torch.empty(n, D, device=self._device())
        of_.nvp_prior(*of_.maf_halves(z, D), n, D, seed, "half", temperature=temperature)
        return z


__all__ = ["MAFLayer", "MAF", "MAFTrainer", "MAFEngine", "MAFError", "degrees", "masks", "inverse_order",
           "uniforms_reference", "normals_reference", "preprocess", "postprocess", "nll_constant", "maf_fused_ok",
           "FlatAdam"]
