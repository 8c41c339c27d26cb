"""Masked autoencoder for distribution estimation, MADE (Germain, Gregor, Murray & Larochelle, "MADE: Masked Autoencoder
for Distribution Estimation", arXiv 1502.03509) on the collection's MLP: the one model here with a tractable likelihood.
Exported by src/made.py as MADE / MADETrainer.

The contract.  MADE(image_size I = 784, hidden_dim H = 400, order = "natural", order_seed = 0) holds linear = Linear(I, H)
and out = Linear(H, I).  Logits a = out(relu(linear(x))); forward(x) returns them;  p(x) = prod_d Bernoulli(x_d;
sigmoid(a_d)).  Limits: 2 <= I <= 8192, 1 <= H <= 1024; anything else raises MADEError(GMError, ValueError) in the
constructor.

Degrees.  Two persistent int32 buffers, m_in [I] and m_h [H], in the state_dict (a checkpoint carries the order).  m_in is
a permutation of 1 .. I: "natural" m_in[i] = i + 1; "random" 1 + numpy.random.RandomState(order_seed).permutation(I) (the
global generators are untouched).  m_h[k] = 1 + floor(k (I - 1) / H): deterministic, ascending, in [1, I - 1].  Masks are
computed from the degrees wherever they are needed, never stored as matrices on the device:
  M1[k, i] = (m_h[k] >= m_in[i]),   M2[d, k] = (m_in[d] > m_h[k]).
The pixel of degree 1 sees nothing: its logit is its bias.

Masked parameters.  The parameters hold the masked values: the entries of linear.weight and out.weight where the mask is
0 are exactly 0.0 after construction and after every optimiser step, on every path.

Loss, per batch of b rows:  loss = (1 / b) sum_{r,d} [softplus(a) - x a] in nats per image, softplus(a) = max(a, 0) +
log1p(exp(-|a|));  d loss / d a = (sigmoid(a) - x) / b.  Validation: the same sum without the gradient.

Sampler.  Pixels are drawn in order of degree.  The uniform of pixel d of sample row r is ph_unit (csrc/gm_philox.h) of
word d & 3 of Philox4x32-10 at counter (d >> 2, 0, r, TAG_MS = "MADS") under key (seed mod 2^32, seed >> 32);  x_d = 1
iff u_d < 1 / (1 + expf(-a_d)), compared in fp32.  The rule is indexed by pixel and row, so the work mapping cannot change
a bit (`uniforms_reference` below is the same rule in numpy).  Completion: with n_known = j the pixels of degree <= j are
copied from a given row and the rest are drawn by the same rule.

Fused path: MADEEngine below -- 8 launches per training batch (gather, two forwards, gm_made_bce, dH, both weight
gradients + Adam as a pair, gm_made_mask, the loss sum with the counter tick), 5 per validation batch; sampling is ONE
launch, gm_made_sample, which keeps the H pre-activations of a row in registers and updates them pixel by pixel: a whole
sample costs 2 I H multiply-adds per row, one forward pass, where the naive sampler pays I of them.  An overridden
compute_batch / evaluate or an edited model: the general loop -- autograd over ops.fused_linear with weight * mask
(masked gradients, and so masked entries, stay zero without the mask kernel) and a sampler of I forward passes under the
same uniform rule."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, philox, viz
from ._lib import MADE_MAX_H, MADE_MAX_I, MADE_MIN_I, MADE_TAG_S, GMError
from .trainers import FlatAdam, OneLossTrainer, _dataset_rows, _stock_module, stock, stock_model  # noqa: F401
from .engine import OneNetEngine, _Linear

TAG_MS = MADE_TAG_S
ORDERS = ("natural", "random")


class MADEError(GMError, ValueError):
    """A bad image size, hidden width, order, seed, n or n_known: a ValueError, and a GMError like the package's other
    refusals."""


def _int(v, name):
    return _lib.check_int(v, name, MADEError)


def check_seed(seed, name="seed"):
    return _lib.check_seed(seed, name, MADEError)


def check_shape(image_size, hidden_dim):
    """(I, H) validated against the kernels' limits; else MADEError."""
    I, H = _int(image_size, "image_size"), _int(hidden_dim, "hidden_dim")
    if not MADE_MIN_I <= I <= MADE_MAX_I:
        raise MADEError("image_size must lie in [%d, %d], got %d" % (MADE_MIN_I, MADE_MAX_I, I))
    if not 1 <= H <= MADE_MAX_H:
        raise MADEError("hidden_dim must lie in [1, %d], got %d" % (MADE_MAX_H, H))
    return I, H


def check_order(order, order_seed):
    if order not in ORDERS:
        raise MADEError("order must be one of %s, got %r" % (ORDERS, order))
    order_seed = _int(order_seed, "order_seed")
    if not 0 <= order_seed < 1 << 32:
        raise MADEError("order_seed must lie in [0, 2^32), got %d" % order_seed)
    return order, order_seed


def check_known(n_known, I):
    n_known = _int(n_known, "n_known")
    if not 0 <= n_known <= I:
        raise MADEError("n_known must lie in [0, I = %d], got %d" % (I, n_known))
    return n_known


# ---- the degrees, the masks and the uniform rule in numpy (the tests' reference reads the same contract) ---------------
def degrees(image_size, hidden_dim, order="natural", order_seed=0):
    """(m_in [I], m_h [H]) int32."""
    I, H = check_shape(image_size, hidden_dim)
    order, order_seed = check_order(order, order_seed)
    if order == "natural":
        m_in = np.arange(1, I + 1, dtype=np.int32)
    else:
        m_in = (1 + np.random.RandomState(order_seed).permutation(I)).astype(np.int32)
    m_h = (1 + (np.arange(H, dtype=np.int64) * (I - 1)) // H).astype(np.int32)
    return m_in, m_h


def masks(m_in, m_h):
    """(M1 [H, I], M2 [I, H]) boolean, from the degree vectors (numpy arrays or tensors on any device)."""
    if torch.is_tensor(m_in):
        return m_h[:, None] >= m_in[None, :], m_in[:, None] > m_h[None, :]
    m_in, m_h = np.asarray(m_in), np.asarray(m_h)
    return m_h[:, None] >= m_in[None, :], m_in[:, None] > m_h[None, :]


def inverse_order(m_in):
    """inv_order [I] int32: the pixel of degree t + 1 at position t."""
    m = np.asarray(m_in.cpu() if torch.is_tensor(m_in) else m_in, dtype=np.int64)
    inv = np.empty(m.size, dtype=np.int32)
    if not np.array_equal(np.sort(m), np.arange(1, m.size + 1)):
        raise MADEError("m_in is not a permutation of 1 .. %d" % m.size)
    inv[m - 1] = np.arange(m.size, dtype=np.int32)
    return inv


def uniforms_reference(n, I, seed, row0=0):
    """u [n, I] float32: the sampler's uniforms of sample rows row0 .. by the contract's rule, bit for bit."""
    return philox.unit_uniforms(philox.words(n, I, seed, 0, TAG_MS, row0))


# ---- module ----------------------------------------------------------------------------------------------------------
@stock_model
class MADE(nn.Module):
    """linear (I -> H, relu) and out (H -> I), both masked by the degree buffers m_in / m_h."""

    def __init__(self, image_size=784, hidden_dim=400, order="natural", order_seed=0):
        super().__init__()
        self.image_size, self.hidden_dim = check_shape(image_size, hidden_dim)
        self.order, self.order_seed = check_order(order, order_seed)
        self.linear = nn.Linear(self.image_size, self.hidden_dim)
        self.out = nn.Linear(self.hidden_dim, self.image_size)
        m_in, m_h = degrees(self.image_size, self.hidden_dim, self.order, self.order_seed)
        self.register_buffer("m_in", torch.from_numpy(m_in))
        self.register_buffer("m_h", torch.from_numpy(m_h))
        self.shape = int(self.image_size ** 0.5)
        self.apply_masks()

    def masks(self):
        """(M1 [H, I], M2 [I, H]) as float32 tensors on the buffers' device, computed on the spot."""
        M1, M2 = masks(self.m_in, self.m_h)
        return M1.to(torch.float32), M2.to(torch.float32)

    @torch.no_grad()
    def apply_masks(self):
        """Zeroes the masked entries of both weights in place (the constructor's last step)."""
        M1, M2 = self.masks()
        self.linear.weight.mul_(M1)
        self.out.weight.mul_(M2)

    def forward(self, x):
        """The logits of x [n, I]; the weights enter as weight * mask, so masked gradients are zero."""
        if not x.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: got a %s tensor and there is no CPU "
                          "fallback (move the model and inputs with to_cuda)" % x.device)
        M1, M2 = self.masks()
        h = ops.fused_linear(x, self.linear.weight * M1, self.linear.bias, "relu")
        return ops.fused_linear(h, self.out.weight * M2, self.out.bias, "id")


def made_fused_ok(model):
    """True iff the model is MADE itself with its two layers unchanged and consistent shapes and degree buffers."""
    if not _stock_module(model, 2):
        return False
    lin, out = getattr(model, "linear", None), getattr(model, "out", None)
    if not (type(lin) is nn.Linear and type(out) is nn.Linear and lin.bias is not None and out.bias is not None):
        return False
    H, I = lin.weight.shape
    m_in, m_h = getattr(model, "m_in", None), getattr(model, "m_h", None)
    return (tuple(out.weight.shape) == (I, H) and MADE_MIN_I <= I <= MADE_MAX_I and 1 <= H <= MADE_MAX_H
            and getattr(model, "image_size", None) == I and getattr(model, "hidden_dim", None) == H
            and all(torch.is_tensor(t) and t.dtype == torch.int32 for t in (m_in, m_h))
            and m_in.numel() == I and m_h.numel() == H)


def nll_rows(logits, x):
    """softplus(a) - x a summed over a row, by autograd-able torch ops (the general path's loss); softplus as
    -logsigmoid(-a): the contract's value, and a gradient of sigmoid(a) at a = 0 too."""
    return (-torch.nn.functional.logsigmoid(-logits) - x * logits).sum(1)


# ---- engine ----------------------------------------------------------------------------------------------------------
class MADEEngine(OneNetEngine):
    """MADE on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  Per training
    batch, 8 launches: 1. gm_gather_rows[_bits];  2. H1 = relu(linear(X));  3. A = out(H1);  4. gm_made_bce (dA, row
    partials);  5. dH = dA Wout [H1 > 0], before the launch that steps Wout;  6. both weight gradients + Adam as a pair;
    7. gm_made_mask: the pair's epilogue steps every entry, masked ones included, so W and both moments are zeroed at
    the masked entries -- the optimiser state equals that of the general path, whose masked gradients are zero;  8. the
    loss sum with the counter tick.  A validation batch is launches 1-4 (no dA) and the sum.  The degree vectors are
    launch arguments: the graphs are dropped when the model's buffers move.  No eps ring, every batch its own gather.
    One GPU only."""

    one_gpu = "the MADE engine"
    fused_ok = staticmethod(made_fused_ok)
    refusal = ("MADE", "made.MADE", "layers")
    binds_trainer = False       # no noise: nothing to read from the trainer

    def _params(self, model):
        return [model.linear.weight, model.linear.bias, model.out.weight, model.out.bias]

    def _setup(self, model):
        self.L1, self.L2 = _Linear(self.fp, model.linear), _Linear(self.fp, model.out)
        self.I, self.H = model.image_size, model.hidden_dim

    def _buffers(self, B):
        z = lambda *s: torch.zeros(*s, device=self.device)
        self.X, self.H1, self.A = z(B, self.I), z(B, self.H), z(B, self.I)
        self.dA, self.dH, self.part = z(B, self.I), z(B, self.H), z(B)

    def _settings(self):
        return {"order": str(self.model.order), "order_seed": int(self.model.order_seed)}

    def _graph_args(self):
        return self.model.m_in.data_ptr(), self.model.m_h.data_ptr()     # the degree vectors are launch arguments

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        m = self.model
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)
        from . import ops_fused as of_
        # whatever was loaded into the model, training starts from masked weights (resumed moments are masked already)
        of_.made_mask(self.L1.W, self.L2.W, m.m_in, m.m_h)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: forward, the Bernoulli-logit loss (+ backward, Adam and the masks when train)."""
        from . import ops_fused as of_
        L1, L2, m = self.L1, self.L2, self.model
        idx_slot = self._slot(t, 1, 0, self.R, self.B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        ops.gather_rows(self.data, self.idx_ring.view(-1), self.X, B=b, idx_slot=idx_slot, stream=st)
        ops.linear_fwd(self.X, L1.W, L1.b, self.H1, "relu", M=b, stream=st)
        ops.linear_fwd(self.H1, L2.W, L2.b, self.A, "id", M=b, stream=st)
        scale = float(np.float32(1.0 / b))
        of_.made_bce(self.A, self.X, self.part, b, scale, dA=self.dA if train else None, stream=st)
        if train:
            adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
            # dH reads out.weight BEFORE the paired dW(+Adam) launch updates it
            ops.linear_bwd_dx(self.dA, L2.W, self.dH, below=self.H1, epi="relu", M=b, stream=st)
            ops.linear_bwd_dw_adam_pair(dict(dA=self.dA, X=self.H1, lin=L2, adam=adam, M=b),
                                        dict(dA=self.dH, X=self.X, lin=L1, adam=adam, M=b),
                                        weight_decay=self.wd, stream=st)
            of_.made_mask(L1.W, L2.W, m.m_in, m.m_h, moments1=(L1.mW, L1.vW), moments2=(L2.mW, L2.vW), stream=st)
        of_.sum_finalize(self.part, b, self.recon if train else self.vrecon, scale=scale, out_slot=loss_slot,
                         tick=self.ctr if self.use_graph else None, stream=st)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class MADETrainer(OneLossTrainer):
    """Trains a MADE on its exact negative log-likelihood and samples from it.  Histories: `losses` (the NLL in nats per
    image, one per training batch); the epoch line (mean training NLL, validation NLL); best_val_loss / best_model as
    the other VAE-family trainers; checkpoints (+ order, order_seed in the optimizer state's config, checked under
    strict=True; resuming is bit-identical).  One GPU only."""
    _line = "Epoch[%d/%d], NLL: %.6f, Val NLL: %.6f"
    _one_gpu = "MADETrainer"
    _error = MADEError
    _fused_ok = staticmethod(made_fused_ok)

    def compute_batch(self, batch):
        """The batch's NLL in nats per image (general path: autograd over the fused linear kernels with weight *
        mask)."""
        x = self._flat_batch(batch)
        return nll_rows(self.model(x), x).sum() / x.shape[0]

    def _engine_class(self):
        return MADEEngine

    def train(self, num_epochs, lr=1e-3, weight_decay=0.0, quiet=False):
        """VAETrainer.train with this model's defaults (general path: weight * mask in the forward keeps every masked
        gradient, Adam moment and entry at zero)."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    # ---- sampling and scoring ------------------------------------------------------------------------------------------
    def _logits(self, x):
        """The model's logits of device rows x, no autograd: the two GEMM launches for a stock model, its own forward
        otherwise."""
        m = self.model
        with torch.no_grad():
            if made_fused_ok(m):
                h = torch.empty(x.shape[0], m.hidden_dim, device=x.device)
                a = torch.empty(x.shape[0], m.image_size, device=x.device)
                ops.linear_fwd(x, m.linear.weight.detach(), m.linear.bias.detach(), h, "relu")
                ops.linear_fwd(h, m.out.weight.detach(), m.out.bias.detach(), a, "id")
                return a
            return m(x).contiguous()

    def _draw(self, n, seed, return_probs, given, n_known):
        from . import ops_fused as of_
        m = self.model
        dev = self._device()
        torch.cuda.synchronize()
        I = m.image_size
        inv = inverse_order(m.m_in)
        x = torch.empty(n, I, device=dev)
        p = torch.empty(n, I, device=dev) if return_probs else None
        if made_fused_ok(m):
            with torch.no_grad():
                W1T = m.linear.weight.detach().t().contiguous()
            of_.made_sample(m.out.weight.detach(), m.out.bias.detach(), W1T, m.linear.bias.detach(), m.m_h,
                            torch.from_numpy(inv).to(dev), n, seed, x=x, p=p, given=given, n_known=n_known)
        else:
            self._sample_general(x, p, inv, seed, given, n_known)
        torch.cuda.synchronize()
        return (x, p) if return_probs else x

    def _sample_general(self, x, p, inv, seed, given, n_known):
        """An edited model's sampler: I forward passes of the model under the same uniform rule."""
        from . import ops_fused as of_
        n, I = x.shape
        u = of_.made_uniform(n, I, seed, device=x.device)
        x.zero_()
        mode = self.model.training
        self.model.eval()
        try:
            with torch.no_grad():
                for t in range(I):
                    d = int(inv[t])
                    a = self.model(x)[:, d]
                    pd = 1.0 / (1.0 + torch.exp(-a))
                    x[:, d] = given[:, d] if t < n_known else (u[:, d] < pd).to(torch.float32)
                    if p is not None:
                        p[:, d] = pd
        finally:
            self.model.train(mode)

    def sample(self, n, seed=0, return_probs=False):
        """n samples [n, I] float32 in {0, 1}, drawn pixel by pixel in order of degree under the contract's uniform rule
        -- in one launch for a stock model (gm_made_sample), through I forward passes otherwise; return_probs: (samples,
        the conditionals [n, I] each pixel was drawn from).  Runs after a device synchronise; the global generator, the
        model's mode and the parameters are untouched."""
        n, seed = _int(n, "n"), check_seed(seed)
        if n < 1:
            raise MADEError("n must be >= 1, got %d" % n)
        return self._draw(n, seed, bool(return_probs), None, 0)

    def complete(self, images, n_known, seed=0, *, return_probs=False):
        """images [n, pixels] with the pixels of degree <= n_known kept and the rest drawn by the sampler's rule;
        return_probs: (completed, the conditionals [n, I])."""
        n_known, seed = check_known(n_known, self.model.image_size), check_seed(seed)
        x = self._rows(images)
        return self._draw(x.shape[0], seed, bool(return_probs), x, n_known)

    def log_likelihood(self, images=None, batch=1024):
        """The exact log p(x) of every image in nats (images=None: the whole test_iter) -> metrics.NLLResult(ll_mean,
        ll_stderr, n), from gm_made_bce's row partials."""
        return self._nll_result(self.log_likelihood_rows(images, batch))

    def log_likelihood_rows(self, images=None, batch=1024):
        """log p(x) per image, a float64 CPU tensor [n]."""
        from . import ops_fused as of_
        x = self._rows(_dataset_rows(self.test_iter) if images is None else images)
        torch.cuda.synchronize()
        part = torch.empty(x.shape[0], device=x.device)
        for i in range(0, x.shape[0], batch):
            xb = x[i:i + batch]
            of_.made_bce(self._logits(xb), xb, part[i:], xb.shape[0], 1.0)
        torch.cuda.synchronize()
        return -part.double().cpu()

    # ---- visualisation, checkpoints -----------------------------------------------------------------------------------
    def sample_images(self, epoch=-100, num_images=36, save=True):
        return viz.made_sample_images(self, epoch, num_images, save, self.viz_dir)

    def reconstruct_images(self, images, epoch, save=True):
        raise GMError("a MADE has no latent code: complete(images, n_known) redraws the pixels after the first n_known")

    def viz_loss(self):
        viz.one_loss_curve(self, "NLL (nats per image)")


__all__ = ["MADE", "MADETrainer", "MADEEngine", "MADEError", "degrees", "masks", "inverse_order", "uniforms_reference",
           "made_fused_ok", "FlatAdam"]
