"""Binary restricted Boltzmann machine (Smolensky 1986; Hinton 2002, contrastive divergence; Tieleman 2008, persistent
CD; Salakhutdinov & Murray 2008, annealed importance sampling) on the collection's 784 <-> 400 layer pair with tied
weights: the collection's energy-based model.  Exported by src/rbm.py as RBM / RBMTrainer.

The contract.  RBM(image_size I = 784, hidden_dim H = 400) holds linear = Linear(I, H) -- its weight is W [H, I], its bias
c [H] -- and vbias = Parameter(zeros(I)), written b.  Limits: 1 <= I, H <= 1024; anything else raises RBMError(GMError,
ValueError).  E(v, h) = -b.v - c.h - h.W v;  F(v) = -b.v - sum_j softplus(c_j + W_j.v), softplus(a) = max(a, 0) +
log1p(exp(-|a|)).

Loss of a batch of B rows:  mean_b [F(v0_b) - F(vk_b)] with v0 and vk held constant.  Its gradient is the CD / PCD update
(hidden PROBABILITIES in both statistics, Hinton's recipe; vk itself a sample), so the fused path, the general autograd
path and the tests' fp64 oracle descend the same scalar; it is also the history `losses` (the free-energy gap, one value
per batch).  v0 = (u < x), the stochastic binarisation of the batch ({0, 1} data pass unchanged: the uniforms lie
strictly inside (0, 1)).  mode="cd": vk is k Gibbs steps from v0.  mode="pcd": vk is k steps from a persistent buffer of
B chains that lives across batches, initialised from the first batch's v0 and carried by checkpoints.  Optimizer: the
collection's Adam; weight_decay is applied as gm_adam applies it, to every tensor it steps -- W, c and b alike.

The noise rule.  The uniform of unit e of chain row r at step t under tag T is ph_unit (csrc/gm_philox.h) of word e & 3
of Philox4x32-10 at counter (e >> 2, t, r, T) under key (seed mod 2^32, seed >> 32): T = "RBMD" the binarisation (t = the
batch step), "RBMH" / "RBMV" the hidden / visible draws (t = the Gibbs step).  A unit is lit iff u < 1 / (1 +
expf(-a)) in fp32.  Training batch T (counted over every train() call of the trainer) binarises at t = T and runs its
Gibbs steps at t = T k .. T k + k - 1; chain row = the row's position in the batch.  Validation binarises at t = the
batch's index in the pass and takes its one Gibbs step at the same t, under the key seed + 0x9E3779B97F4A7C15 (mod 2^64):
a fixed stream.  The sum rule: pre_h[j] = c[j], then += W[j, i] for the lit pixels i in ascending order; pre_v[i] = b[i],
then += W[j, i] for the lit hidden units j in ascending order; one fp32 accumulator per unit (`uniforms_reference`
below is the noise rule in numpy).

Fused path: RBMEngine below; sampling, Gibbs steps and annealed importance sampling are ONE launch of gm_rbm_chain
each.  An overridden compute_batch / evaluate or an edited model: the general loop -- autograd of the same gap through
ops.fused_linear, the chain composed from torch operations on the same uniforms (gm_rbm_uniform)."""
import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, philox, viz
from ._lib import RBM_MAX_DIM, RBM_MAX_STEPS, RBM_TAG_D, RBM_TAG_H, RBM_TAG_V, GMError
from .trainers import FlatAdam, OneLossTrainer, _dataset_rows, _stock_module, stock, stock_model  # noqa: F401
from .engine import OneNetEngine, _Linear

_M64 = (1 << 64) - 1
MODES = ("cd", "pcd")
EVAL_KEY = 0x9E3779B97F4A7C15          # validation and log_likelihood binarise under seed + EVAL_KEY (mod 2^64)
MAX_K = 4096


class RBMError(GMError, ValueError):
    """A bad image size, hidden width, k, mode, seed, n, steps or beta schedule: a ValueError, and a GMError like the
    package's other refusals."""


def _int(v, name):
    return _lib.check_int(v, name, RBMError)


def check_seed(seed, name="seed"):
    return _lib.check_seed(seed, name, RBMError)


def check_shape(image_size, hidden_dim):
    """(I, H) validated against the kernels' limits; else RBMError."""
    I, H = _int(image_size, "image_size"), _int(hidden_dim, "hidden_dim")
    if not 1 <= I <= RBM_MAX_DIM:
        raise RBMError("image_size must lie in [1, %d], got %d" % (RBM_MAX_DIM, I))
    if not 1 <= H <= RBM_MAX_DIM:
        raise RBMError("hidden_dim must lie in [1, %d], got %d" % (RBM_MAX_DIM, H))
    return I, H


def check_steps(steps, lo=0, name="steps"):
    steps = _int(steps, name)
    if not lo <= steps <= RBM_MAX_STEPS:
        raise RBMError("%s must lie in [%d, %d], got %d" % (name, lo, RBM_MAX_STEPS, steps))
    return steps


def check_k_mode(k, mode):
    k = _int(k, "k")
    if not 1 <= k <= MAX_K:
        raise RBMError("k must lie in [1, %d], got %d" % (MAX_K, k))
    if mode not in MODES:
        raise RBMError("mode must be one of %s, got %r" % (MODES, mode))
    return k, mode


def default_betas():
    """Salakhutdinov & Murray's three-segment schedule: 500 betas spaced uniformly over [0, 0.5), 4 000 over [0.5, 0.9)
    and 10 000 over [0.9, 1]: 14 500 in all, float32."""
    return np.concatenate([np.linspace(0.0, 0.5, 500, endpoint=False), np.linspace(0.5, 0.9, 4000, endpoint=False),
                           np.linspace(0.9, 1.0, 10000)]).astype(np.float32)


def check_betas(betas):
    """A float32 array ascending from 0 to 1 with >= 2 entries: None -> default_betas(), an int n -> n betas uniformly
    spaced, an array as it is; else RBMError."""
    if betas is None:
        return default_betas()
    if isinstance(betas, (int, np.integer)) and not isinstance(betas, (bool, np.bool_)):
        if not 2 <= int(betas) <= RBM_MAX_STEPS:
            raise RBMError("betas must lie in [2, %d] when an integer, got %d" % (RBM_MAX_STEPS, int(betas)))
        return np.linspace(0.0, 1.0, int(betas)).astype(np.float32)
    b = np.asarray(betas, dtype=np.float32).reshape(-1)
    if b.size < 2 or b.size > RBM_MAX_STEPS or b[0] != 0.0 or b[-1] != 1.0 or not np.all(np.diff(b) >= 0.0):
        raise RBMError("betas must ascend from 0 to 1 (at least 2, at most %d entries)" % RBM_MAX_STEPS)
    return b


def uniforms_reference(n, width, seed, tag, t=0, row0=0):
    """u [n, width] float32: the rule's uniforms of chain rows row0 .. under `tag` at step t, bit for bit."""
    return philox.unit_uniforms(philox.words(n, width, seed, t, tag, row0))


def softplus(a):
    """max(a, 0) + log1p(exp(-|a|)) as -logsigmoid(-a): the contract's value, autograd gives sigmoid(a)."""
    return -torch.nn.functional.logsigmoid(-a)


# ---- module ----------------------------------------------------------------------------------------------------------
@stock_model
class RBM(nn.Module):
    """linear (I -> H: W and the hidden bias c) and vbias (the visible bias b)."""

    def __init__(self, image_size=784, hidden_dim=400):
        super().__init__()
        self.image_size, self.hidden_dim = check_shape(image_size, hidden_dim)
        self.linear = nn.Linear(self.image_size, self.hidden_dim)
        self.vbias = nn.Parameter(torch.zeros(self.image_size))
        self.shape = int(self.image_size ** 0.5)

    @staticmethod
    def _device_rows(x):
        if not x.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: got a %s tensor and there is no CPU "
                          "fallback (move the model and inputs with to_cuda)" % x.device)
        return x

    def hidden_logits(self, v):
        """c + W v of rows v [n, I]."""
        return ops.fused_linear(self._device_rows(v), self.linear.weight, self.linear.bias, "id")

    def visible_logits(self, h):
        """b + W^T h of rows h [n, H]."""
        return ops.fused_linear(self._device_rows(h), self.linear.weight.t().contiguous(), self.vbias, "id")

    def free_energy(self, v):
        """F(v) [n], autograd-able."""
        return -(v @ self.vbias) - softplus(self.hidden_logits(v)).sum(1)

    def forward(self, v):
        """p(h = 1 | v) of rows v [n, I]."""
        return torch.sigmoid(self.hidden_logits(v))


def rbm_fused_ok(model):
    """True iff the model is RBM itself with its layer and bias unchanged and consistent shapes."""
    if not _stock_module(model, 1):
        return False
    lin, vb = getattr(model, "linear", None), getattr(model, "vbias", None)
    if not (type(lin) is nn.Linear and lin.bias is not None and isinstance(vb, nn.Parameter)):
        return False
    H, I = lin.weight.shape
    return (1 <= I <= RBM_MAX_DIM and 1 <= H <= RBM_MAX_DIM and tuple(vb.shape) == (I,)
            and getattr(model, "image_size", None) == I and getattr(model, "hidden_dim", None) == H)


# ---- engine ----------------------------------------------------------------------------------------------------------
class RBMEngine(OneNetEngine):
    """The RBM on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  A CD-k
    training batch is 8 launches: 1. gm_gather_rows[_bits];  2. gm_rbm_chain: v0 and vk into the stacked V = [v0; vk]
    [2b, I];  3. pre = linear(V), one forward GEMM over 2b rows;  4. gm_rbm_grad: dA = [-p0; +pk] / b and the signed
    free energies;  5. gm_linear_bwd_dw_ex with Adam in the epilogue: dW = dA^T V and dc = colsum(dA) in one stacked
    reduction, W and c stepped;  6. gm_rbm_vbias: the visible bias' gradient and its Adam step in the launch;
    7. gm_rbm_transpose: WT for the next batch's chain;  8. the loss sum with the counter tick.  A PCD batch is 10: the
    chain launch on the data runs with steps = 0 (v0 alone), a second one advances the persistent chains in place,
    and gm_copy_slot_f32 stacks them under v0.  A validation batch is 4: gather, a k = 1 chain with a_out and v0_out,
    gm_made_bce of the logits against v0 (the one-step reconstruction cross-entropy, nats per image), the sum.  The
    Gibbs step of a training batch is (ctr + nbase) k: ctr the engine's device counter, nbase a device word configure()
    writes from the trainer's count of training batches, so a graph captured in one train() call serves the next.
    No eps ring.  One GPU only."""

    one_gpu = "the RBM engine"
    fused_ok = staticmethod(rbm_fused_ok)
    refusal = ("RBM", "rbm.RBM", "layer")        # the trainer: k, mode, seed and noise_steps

    def _params(self, model):
        return [model.linear.weight, model.linear.bias, model.vbias]

    def _setup(self, model):
        self.L = _Linear(self.fp, model.linear)
        self.I, self.H = model.image_size, model.hidden_dim
        o = self.fp.offsets[2]
        self.vb, self.m_vb, self.v_vb = self.fp.views[2], self.fp.m[o:o + self.I], self.fp.v[o:o + self.I]
        self.WT = torch.zeros(self.I, self.H, device=self.device)
        self.pcd_ready = False

    def _buffers(self, B):
        z = lambda *s: torch.zeros(*s, device=self.device)
        self.X, self.V, self.PRE, self.dA = z(B, self.I), z(2 * B, self.I), z(2 * B, self.H), z(2 * B, self.H)
        self.part, self.A, self.Vv, self.vpart = z(2 * B), z(B, self.I), z(B, self.I), z(B)
        self.P = z(B, self.I)                        # the persistent chains (mode "pcd")
        self.pcd_ready = False

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        from . import ops_fused as of_
        tr = self.trainer
        self.k, self.mode, self.seed = int(tr.k), str(tr.mode), int(tr.seed)
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)
        if resume is not None and resume.get("pcd") is not None:
            if tuple(resume["pcd"].shape) != tuple(self.P.shape):
                raise GMError("checkpoint's persistent chains %s do not match this run's %s"
                              % (tuple(resume["pcd"].shape), tuple(self.P.shape)))
            self.P.copy_(resume["pcd"])
            self.pcd_ready = True
        elif int(tr.noise_steps) == 0:
            self.pcd_ready = False                   # a fresh run: the first batch's v0 starts the chains
        of_.rbm_transpose(self.L.W, self.WT)

    def _settings(self):
        return {"k": self.k, "mode": self.mode, "seed": self.seed}

    def optim_state(self):
        st = super().optim_state()
        if self.mode == "pcd" and self.pcd_ready:
            st["pcd"] = self.P.detach().cpu().clone()
        return st

    def _steps(self, t):
        """The step sources of the batch at ring step t: graphs read ctr + nbase, eager launches t + nbase."""
        if self.use_graph:
            return dict(step_ctr=self.ctr, step_base=self.nbase, d_add=0, g_mul=self.k, g_add=0)
        return dict(step_base=self.nbase, d_add=t, g_mul=self.k, g_add=t * self.k)

    def run_pass(self, data, perm, train, t0):
        if train and self.mode == "pcd" and not self.pcd_ready:
            from . import ops_fused as of_
            b = min(self.B, perm.numel())
            ops.gather_rows(data, perm[:b].to(self.device), self.X, B=b)
            self.P.zero_()
            of_.rbm_chain(self.L.W, self.WT, self.L.b, self.vb, self.X, 0, self.seed, n=b, v0_out=self.P,
                          step_base=self.nbase, d_add=t0)
            self.pcd_ready = True
        return super().run_pass(data, perm, train, t0)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: the chain, then (train) the stacked statistics, Adam on W, c and b, the transpose."""
        from . import ops_fused as of_
        L = self.L
        idx_slot = self._slot(t, 1, 0, self.R, self.B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        scale = float(np.float32(1.0 / b))
        tick = self.ctr if self.use_graph else None
        ops.gather_rows(self.data, self.idx_ring.view(-1), self.X, B=b, idx_slot=idx_slot, stream=st)
        if not train:
            src = dict(step_ctr=self.ctr) if self.use_graph else dict(d_add=t, g_add=t)
            of_.rbm_chain(L.W, self.WT, L.b, self.vb, self.X, 1, (self.seed + EVAL_KEY) & _M64, n=b, v0_out=self.Vv,
                          a_out=self.A, stream=st, **src)
            of_.made_bce(self.A, self.Vv, self.vpart, b, 1.0, stream=st)
            of_.sum_finalize(self.vpart, b, self.vrecon, scale=scale, out_slot=loss_slot, tick=tick, stream=st)
            return
        V = self.V[:2 * b]
        if self.mode == "cd":
            of_.rbm_chain(L.W, self.WT, L.b, self.vb, self.X, self.k, self.seed, n=b, v0_out=V[:b], v_out=V[b:],
                          stream=st, **self._steps(t))
        else:
            of_.rbm_chain(L.W, self.WT, L.b, self.vb, self.X, 0, self.seed, n=b, v0_out=V[:b], stream=st,
                          **self._steps(t))
            of_.rbm_chain(L.W, self.WT, L.b, self.vb, self.P, self.k, self.seed, n=b, v_out=self.P, stream=st,
                          **self._steps(t))
            ops.copy_slot(self.P, V[b:], b * self.I, stream=st)
        ops.linear_fwd(V, L.W, L.b, self.PRE, "id", M=2 * b, stream=st)
        of_.rbm_grad(self.PRE, V, self.vb, self.dA, self.part, b, scale, stream=st)
        adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
        ops.linear_bwd_dw_adam(self.dA, V, L, adam, M=2 * b, weight_decay=self.wd, stream=st)
        of_.rbm_vbias(V, b, self.I, scale, g=self.fp.gviews[2], adam=dict(p=self.vb, m=self.m_vb, v=self.v_vb, **adam),
                      weight_decay=self.wd, stream=st)
        of_.rbm_transpose(L.W, self.WT, stream=st)
        of_.sum_finalize(self.part, 2 * b, self.recon, scale=scale, out_slot=loss_slot, tick=tick, stream=st)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class RBMTrainer(OneLossTrainer):
    """Trains an RBM by CD-k or PCD-k and samples from it.  Histories: `losses` (the free-energy gap, one per training
    batch) and `recon_loss` (the validation pass' one-step reconstruction cross-entropy in nats per image, one per
    epoch); best_val_loss / best_model on the latter; checkpoints carry the weights, Adam's state, the counters and the
    PCD chains, and resuming is bit-identical.  One GPU only."""
    _history = ("recon_loss",)
    _line = "Epoch[%d/%d], Free-energy gap: %.6f, Val recon CE: %.6f"
    _one_gpu = "RBMTrainer"
    _engine_reads_trainer = True
    _error = RBMError
    _fused_ok = staticmethod(rbm_fused_ok)

    def __init__(self, model, train_iter, val_iter, test_iter, seed=0, k=1, mode="cd", viz=False):
        self.seed = check_seed(seed)
        self.k, self.mode = check_k_mode(k, mode)
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)
        self.noise_steps = 0                         # training batches so far: the noise rule's batch step
        self._general_chains = None

    # ---- the chain on either path ---------------------------------------------------------------------------------------
    def _weights(self):
        """(W, WT, c, b) of a stock model as contiguous device tensors; WT by gm_rbm_transpose."""
        from . import ops_fused as of_
        m = self.model
        W = m.linear.weight.detach().contiguous()
        WT = of_.rbm_transpose(W, torch.empty(W.shape[1], W.shape[0], device=W.device))
        return W, WT, m.linear.bias.detach().contiguous(), m.vbias.detach().contiguous()

    def _chain_general(self, x, steps, seed, dstep=0, g0=0, want=()):
        """The chain composed from torch operations through the model's own layers, on the rule's uniforms: a dict
        with v0, v and what `want` names of p, a (those of the last visible draw)."""
        from . import ops_fused as of_
        n, I = x.shape
        H = self.model.hidden_dim
        uni = lambda w, tag, t: of_.rbm_uniform(n, w, seed, tag, step=t, device=x.device)
        with torch.no_grad():
            v = (uni(I, RBM_TAG_D, dstep) < x).to(torch.float32)
            out = {"v0": v}
            for s in range(steps):
                ph = 1.0 / (1.0 + torch.exp(-self.model.hidden_logits(v)))
                h = (uni(H, RBM_TAG_H, g0 + s) < ph).to(torch.float32)
                a = self.model.visible_logits(h)
                pv = 1.0 / (1.0 + torch.exp(-a))
                v = (uni(I, RBM_TAG_V, g0 + s) < pv).to(torch.float32)
                out.update(p=pv, a=a)
            out["v"] = v
        return out

    def _run_chain(self, x, steps, seed, want_p=False):
        """(v, p or None) after `steps` Gibbs steps from the binarisation of device rows x: one launch for a stock
        model, the torch composition otherwise."""
        from . import ops_fused as of_
        torch.cuda.synchronize()
        n, I = x.shape
        if rbm_fused_ok(self.model):
            v = torch.empty(n, I, device=x.device)
            p = torch.empty(n, I, device=x.device) if want_p else None
            W, WT, c, b = self._weights()
            of_.rbm_chain(W, WT, c, b, x, steps, seed, v_out=v, p_out=p)
        else:
            mode = self.model.training
            self.model.eval()
            try:
                r = self._chain_general(x, steps, seed)
            finally:
                self.model.train(mode)
            v, p = r["v"], r.get("p") if want_p else None
        torch.cuda.synchronize()
        return v, p

    # ---- the general path's batch ---------------------------------------------------------------------------------------
    def compute_batch(self, batch, train=True):
        """The batch's free-energy gap (general path: autograd through the model's own layers; v0 and vk constants).
        Training batches advance the trainer's batch step and, under "pcd", its persistent chains."""
        x = self._flat_batch(batch)
        T = self.noise_steps + self._general_t
        if not train:
            r = self._chain_general(x, 1, (self.seed + EVAL_KEY) & _M64, dstep=self._general_t, g0=self._general_t)
            self._general_t += 1
            return (softplus(r["a"]) - r["v0"] * r["a"]).sum() / x.shape[0]
        r = self._chain_general(x, self.k if self.mode == "cd" else 0, self.seed, dstep=T, g0=T * self.k)
        vk = r["v"]
        if self.mode == "pcd":
            if self._general_chains is None:
                self._general_chains = r["v0"].clone()
            P = self._general_chains
            b = x.shape[0]
            vk = self._chain_general(P[:b], self.k, self.seed, dstep=T, g0=T * self.k)["v"]
            P[:b] = vk
        self._general_t += 1
        return (self.model.free_energy(r["v0"]) - self.model.free_energy(vk)).mean()

    def evaluate(self, iterator):
        """Mean over the batches of the one-step reconstruction cross-entropy in nats per image."""
        self._general_t = 0
        with torch.no_grad():
            return np.mean([self.compute_batch(batch, train=False).item() for batch in iterator])

    def _engine_class(self):
        return RBMEngine

    def train(self, num_epochs, lr=1e-3, weight_decay=0.0, quiet=False):
        """VAETrainer.train with this model's defaults."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    def _begin_general_epoch(self, epoch):
        self._general_t = (epoch - 1) * len(self.train_iter)     # the epoch's first batch step within this train() call

    def _after_train(self, fused, steps):
        self.noise_steps += steps                    # on both paths: the general compute_batch reads _general_t instead

    def _end_epoch(self, epoch, num_epochs, series, val_loss, quiet):
        self.recon_loss.append(float(val_loss))
        super()._end_epoch(epoch, num_epochs, series, val_loss, quiet)

    # ---- sampling and scoring ------------------------------------------------------------------------------------------
    def sample(self, n, seed=0, steps=1000, return_probs=False):
        """n samples [n, I] float32 in {0, 1}: chains started from Bernoulli(1/2) pixels (x filled with 0.5) and run
        for `steps` >= 1 Gibbs steps under the contract's noise rule -- ONE launch for a stock model;  return_probs:
        (samples, the conditionals [n, I] of the last visible draw).  Runs after a device synchronise; the global
        generator, the model's mode and the parameters are untouched."""
        n, seed, steps = _int(n, "n"), check_seed(seed), check_steps(steps, 1)
        if n < 1:
            raise RBMError("n must be >= 1, got %d" % n)
        x = torch.full((n, self.model.image_size), 0.5, device=self._device())
        v, p = self._run_chain(x, steps, seed, want_p=bool(return_probs))
        return (v, p) if return_probs else v

    def gibbs(self, images, steps, seed=0):
        """The state [n, I] after `steps` >= 0 Gibbs steps from the binarisation of images (steps = 0: the binarisation
        itself)."""
        steps, seed = check_steps(steps), check_seed(seed)
        return self._run_chain(self._rows(images), steps, seed)[0]

    def hidden(self, images):
        """p(h = 1 | v) [n, H] of the images as they are (no binarisation)."""
        x = self._rows(images)
        m = self.model
        with torch.no_grad():
            if rbm_fused_ok(m):
                out = torch.empty(x.shape[0], m.hidden_dim, device=x.device)
                ops.linear_fwd(x, m.linear.weight.detach(), m.linear.bias.detach(), out, "sigmoid")
                return out
            return m(x).contiguous()

    def _free_energy_rows(self, x):
        """F of device rows x, float32 [n]: the forward GEMM and gm_rbm_grad's row partials for a stock model."""
        from . import ops_fused as of_
        m = self.model
        with torch.no_grad():
            if not rbm_fused_ok(m):
                return m.free_energy(x)
            n = x.shape[0]
            V = torch.cat([x, x]).contiguous()
            pre = torch.empty(2 * n, m.hidden_dim, device=x.device)
            part = torch.empty(2 * n, device=x.device)
            ops.linear_fwd(V, m.linear.weight.detach(), m.linear.bias.detach(), pre, "id")
            of_.rbm_grad(pre, V, m.vbias.detach().contiguous(), pre, part, n, 1.0)
            return part[:n].clone()

    def free_energy(self, images):
        """F(v) [n] of the images as they are, a float32 device tensor."""
        return self._free_energy_rows(self._rows(images))

    def base_rate_bias(self):
        """b_A [I] float32 (host): the logit of the Laplace-smoothed training-pixel means, (sum + 1) / (n + 2)."""
        x = _dataset_rows(self.train_iter).double()
        m = (x.sum(0) + 1.0) / (x.shape[0] + 2.0)
        return (torch.log(m) - torch.log1p(-m)).to(torch.float32)

    def ais(self, chains=512, betas=None, seed=0, b_A=None):
        """Annealed importance sampling from the base-rate RBM (bias b_A, no weights) to the model: (log-weights
        float64 [chains] on the host, b_A).  The chains start from the base-rate RBM's own distribution -- x filled
        with sigmoid(b_A), binarised by the rule -- and take ONE launch of len(betas) - 1 tempered steps."""
        from . import ops_fused as of_
        chains, seed, betas = _int(chains, "chains"), check_seed(seed), check_betas(betas)
        if chains < 2:
            raise RBMError("chains must be >= 2, got %d" % chains)
        if not rbm_fused_ok(self.model):
            raise GMError("annealed importance sampling runs on the fused chain kernel: the model is not rbm.RBM with "
                          "its layer unchanged")
        dev = self._device()
        b_A = self.base_rate_bias() if b_A is None else torch.as_tensor(b_A, dtype=torch.float32).reshape(-1)
        if b_A.numel() != self.model.image_size or not bool(torch.isfinite(b_A).all()):
            raise RBMError("b_A must hold %d finite values" % self.model.image_size)
        torch.cuda.synchronize()
        W, WT, c, b = self._weights()
        x = torch.sigmoid(b_A.double()).to(torch.float32).to(dev).repeat(chains, 1).contiguous()
        logw = torch.zeros(chains, dtype=torch.float64, device=dev)
        of_.rbm_chain(W, WT, c, b, x, betas.size - 1, seed, betas=torch.from_numpy(betas).to(dev),
                      b_A=b_A.to(dev).contiguous(), logw=logw)
        torch.cuda.synchronize()
        return logw.cpu(), b_A

    def log_likelihood(self, images=None, chains=512, betas=None, seed=0):
        """The AIS estimate of log p(v) in nats over the images (None: the whole test_iter), binarised by the
        evaluation stream -> metrics.AISResult(ll_mean, ll_stderr, log_z, log_z_stderr, chains, n_betas, n).
        betas: None -> default_betas() (Salakhutdinov & Murray's 14 500: 500 over [0, 0.5), 4 000 over [0.5, 0.9),
        10 000 over [0.9, 1]); an int n -> n uniformly spaced; or an ascending array from 0 to 1.  log Z_A = H log 2 +
        sum softplus(b_A); log Z = log mean w + log Z_A in fp64 on the host; ll = -F(v) - log Z.  ll_stderr is the
        images' spread alone, log_z_stderr the delta-method error of log mean w."""
        from . import metrics
        from . import ops_fused as of_
        betas = check_betas(betas)
        logw, b_A = self.ais(chains, betas, seed)
        lw = logw.numpy()
        mx = lw.max()
        w = np.exp(lw - mx)
        log_z_a = self.model.hidden_dim * np.log(2.0) + float(softplus(b_A.double()).sum())
        log_z = mx + np.log(w.mean()) + log_z_a
        log_z_se = float(w.std() / (w.mean() * np.sqrt(w.size)))
        x = _dataset_rows(self.test_iter) if images is None else images
        x = self._rows(x)
        W, WT, c, b = self._weights()
        v0 = torch.empty_like(x)
        of_.rbm_chain(W, WT, c, b, x, 0, (check_seed(seed) + EVAL_KEY) & _M64, v0_out=v0)
        ll = -self._free_energy_rows(v0).double().cpu() - log_z
        return metrics.AISResult(float(ll.mean()), float(ll.std(unbiased=False)) / float(np.sqrt(ll.numel())),
                                 float(log_z), log_z_se, int(chains), int(betas.size), int(ll.numel()))

    def parzen(self, n_samples=10000, sigmas=None, n_val=10000, seed=0):
        """Parzen-window log-likelihood of the test images under n_samples chain samples (sample(n_samples, seed)) ->
        metrics.ParzenResult."""
        from .trainers import _parzen
        return _parzen(self, n_samples, sigmas, n_val, seed)

    def mmd(self, n_samples=10000, sigmas=None, seed=0):
        """Kernel maximum mean discrepancy (metrics.mmd) between sample(n_samples, seed) and the test images ->
        metrics.MMDResult; sigmas None: the GMMN paper's data-space bandwidths; the unbiased statistic."""
        from .trainers import _mmd
        return _mmd(self, n_samples, sigmas, seed)

    def swd(self, n_samples=10000, n_projections=1024, seed=0):
        """Sliced Wasserstein distance (metrics.sliced_wasserstein) between sample(n_samples, seed) and the test images
        over n_projections random unit directions -> metrics.SWDResult."""
        from .trainers import _swd
        return _swd(self, n_samples, n_projections, seed)

    # ---- visualisation, checkpoints -----------------------------------------------------------------------------------
    def sample_images(self, epoch=-100, num_images=36, save=True):
        return viz.made_sample_images(self, epoch, num_images, save, self.viz_dir)

    def reconstruct_images(self, images, epoch, save=True):
        raise GMError("an RBM has no decoder: gibbs(images, steps) runs the chain from the images")

    def viz_loss(self):
        viz.one_loss_curve(self, "free-energy gap")


__all__ = ["RBM", "RBMTrainer", "RBMEngine", "RBMError", "rbm_fused_ok", "uniforms_reference", "default_betas",
           "check_betas", "FlatAdam"]
