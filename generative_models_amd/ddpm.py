"""Denoising diffusion probabilistic model (Ho, Jain & Abbeel, "Denoising Diffusion Probabilistic Models", arXiv
2006.11239) with the generalised sampler of Song, Meng & Ermon ("Denoising Diffusion Implicit Models", arXiv 2010.02502)
on the collection's MLPs.  Exported by src/ddpm.py as Denoiser / DDPM / DDPMTrainer.

The contract.  DDPM(image_size I, hidden_dim H, time_dim E, T) holds one Denoiser: linear = Linear(I + E, H), hidden =
Linear(H, H), out = Linear(H, I);   eps_theta(x_t, t) = out(relu(hidden(relu(linear(cat[x_t, temb[t]]))))).

Tables (computed once on the host in fp64, rounded once to fp32, non-persistent buffers: no device transcendental is part
of the contract):  beta = min(linspace(1e-4 * 1000 / T, 0.02 * 1000 / T, T), 0.999) (the cap, Nichol & Dhariwal's, is
reached below T = 21 only, where the scaled linear schedule would pass 1);  ab = cumprod(1 - beta);  sa = sqrt(ab);
s1 = sqrt(1 - ab);  temb[t, j] = sin(t f_j), temb[t, E/2 + j] = cos(t f_j), f_j = exp(-ln(1e4) j / (E/2)).
Images in [0, 1] enter as x0 = fmaf(2, x, -1).

Noise (gm_hip.h, csrc/gm_ddpm.h; `timesteps_reference` / `noise_reference` / `qsample_reference` below are the same rule
in numpy).  Philox4x32-10 with key (seed mod 2^32, seed >> 32):
  timestep of batch row `row` at batch `step`: word 0 of counter (0, step, row, TAG_T), t = mulhi(word, T) -- integer
    arithmetic, bit-identical on the device and in numpy;
  noise of pixels 4q .. 4q + 3: counter (q, step, row, TAG_E), the Box-Muller mapping of gm_philox_normal on words
    (0, 1) and (2, 3);
  x_t[e] = fmaf(s1[t], n[e], sa[t] * x0[e]).
Training: TAG_T = "DDPT", TAG_E = "DDPM", `step` the 0-based training batch count over the trainer's life
(`noise_steps`, saved in checkpoints), `row` the row's position in the whole batch.  Validation: TAG_V = "DDPV" for the
timestep and TAG_VE = "DDPW" for the noise, `step` the batch's index within the pass -- the validation loss is a
deterministic function of the weights, comparable across epochs.  The global CPU generator is touched by the loaders'
shuffles only.

Loss (L_simple, Ho et al. eq. 14):  loss = sum_{b,e} (eps - eps_theta)^2 / (b I) per batch;  d loss / d out =
2 (out - eps) / (b I).

Sampler (Song et al. eq. 12), timesteps tau_0 > tau_1 > ... an evenly spaced sub-sequence of T - 1 .. 0 (`steps` of
them; None: all T), at step s with t = tau_s, ab_prev = ab[tau_{s+1}] (1 at the last step):
  x0_hat = (x_t - s1_t eps_theta) / sa_t, clamped to [-1, 1] when `clip`;   eps' = (x_t - sa_t x0_hat) / s1_t;
  sigma = eta sqrt((1 - ab_prev) / (1 - ab_t)) sqrt(1 - ab_t / ab_prev);   dir = sqrt(1 - ab_prev - sigma^2);
  x_prev = sa_prev x0_hat + dir eps' + sigma z.
eta = 1 over all T steps is DDPM's ancestral sampler with the posterior variance, eta = 0 deterministic DDIM; the last
step has sigma = 0 and returns x0_hat.  z of pixels 4q .. 4q + 3 of sample row r at step s: counter (q, s, r, TAG_S =
"DDPS") under the sampling seed; x_T: the same counter at s = `steps`.  The coefficients (s1_t, sa_t, sa_prev, dir,
sigma, tau_{s+1}, tau_s, 0) form a device table [steps, 8] built on the host in fp64 (`reverse_table`), indexed by a
device counter: a hipGraph of G steps is captured once and replayed steps / G times.

Fused path: DDPMEngine below -- 10 launches per training batch (gather + q-sample, three forwards, loss, two input
gradients, the out / hidden weight gradients as a pair with Adam, the first layer's weight gradient with Adam, the loss
sum with the counter tick), 5 per validation batch, 4 per sampler step (three forwards, the reverse step).  Limits of the
kernels: E % 4 == 0, 4 <= E <= 128, 2 <= T <= 4096, I <= 8192 (the model's constructor refuses anything else).  An
overridden compute_batch / evaluate or an edited model: the general loop -- autograd over ops.fused_linear on the same
noise stream (gm_ddpm_qsample as an op)."""
import math

import numpy as np
import torch
import torch.nn as nn

from . import _lib, ops, philox, viz
from ._lib import (DDPM_MAX_E, DDPM_MAX_I, DDPM_MAX_T, DDPM_MIN_E, DDPM_TAG_E, DDPM_TAG_S, DDPM_TAG_T, DDPM_TAG_V,
                   DDPM_TAG_VE, GMError)
from .trainers import FlatAdam, OneLossTrainer, _lin, _stock_module, stock, stock_model, to_cuda  # noqa: F401
from .engine import TimeRegressionEngine, _align4

TAG_T, TAG_E, TAG_V, TAG_VE, TAG_S = DDPM_TAG_T, DDPM_TAG_E, DDPM_TAG_V, DDPM_TAG_VE, DDPM_TAG_S
BETA_MAX = 0.999                 # cap of the scaled linear schedule (reached below T = 21 only)
GRAPH_STEPS = 32                 # sampler steps per captured graph, at most


class DDPMError(GMError, ValueError):
    """A bad T, time_dim, image size, seed, steps or eta: a ValueError, and a GMError like the package's other
    refusals."""


def _int(v, name):
    return _lib.check_int(v, name, DDPMError)


def check_seed(seed):
    return _lib.check_seed(seed, error=DDPMError)


def check_shape(image_size, time_dim, T):
    """(I, E, T) validated against the kernels' limits; else DDPMError."""
    I, E, T = _int(image_size, "image_size"), _int(time_dim, "time_dim"), _int(T, "T")
    if not 1 <= I <= DDPM_MAX_I:
        raise DDPMError("image_size must lie in [1, %d], got %d" % (DDPM_MAX_I, I))
    if not (DDPM_MIN_E <= E <= DDPM_MAX_E and E % 4 == 0):
        raise DDPMError("time_dim must be a multiple of 4 in [%d, %d], got %d" % (DDPM_MIN_E, DDPM_MAX_E, E))
    if not 2 <= T <= DDPM_MAX_T:
        raise DDPMError("T must lie in [2, %d], got %d" % (DDPM_MAX_T, T))
    return I, E, T


def check_sampler(T, steps, eta):
    """(steps, eta) validated: steps None (= T) or an integer in [1, T], eta a finite number >= 0; else DDPMError."""
    steps = T if steps is None else _int(steps, "steps")
    if not 1 <= steps <= T:
        raise DDPMError("steps must lie in [1, T = %d], got %d" % (T, steps))
    if isinstance(eta, (bool, np.bool_)) or not isinstance(eta, (int, float, np.integer, np.floating)):
        raise DDPMError("eta must be a number, got %r" % (eta,))
    eta = float(eta)
    if not (math.isfinite(eta) and eta >= 0.0):
        raise DDPMError("eta must be finite and >= 0, got %r" % eta)
    return steps, eta


# ---- the tables and the rule in numpy and fp64 (the tests' reference; a CPU reading of what the device computes) -----
def tables(T, E):
    """The schedule and embedding tables in fp64: dict(beta, ab, sa, s1 [T], temb [T, E])."""
    beta = np.minimum(np.linspace(1e-4 * 1000.0 / T, 0.02 * 1000.0 / T, T, dtype=np.float64), BETA_MAX)
    ab = np.cumprod(1.0 - beta)
    f = np.exp(-math.log(1e4) * np.arange(E // 2, dtype=np.float64) / (E // 2))
    arg = np.arange(T, dtype=np.float64)[:, None] * f[None, :]
    return {"beta": beta, "ab": ab, "sa": np.sqrt(ab), "s1": np.sqrt(1.0 - ab),
            "temb": np.concatenate([np.sin(arg), np.cos(arg)], axis=1)}


def timestep_sequence(T, steps):
    """tau [steps]: T - 1 = tau_0 > ... evenly spaced over T - 1 .. 0 (steps == T: every timestep; 1: T - 1 alone)."""
    if steps == 1:
        return np.array([T - 1], dtype=np.int64)
    return np.floor(np.linspace(T - 1, 0, steps) + 0.5).astype(np.int64)


def reverse_table(T, steps=None, eta=1.0):
    """(coef [steps, 8] float64, tau [steps]): rows (s1_t, sa_t, sa_prev, dir, sigma, tau_{s+1} or -1, tau_s, 0)."""
    steps, eta = check_sampler(T, steps, eta)
    ab = tables(T, 4)["ab"]
    tau = timestep_sequence(T, steps)
    coef = np.zeros((steps, 8), dtype=np.float64)
    for s, t in enumerate(tau):
        last = s == steps - 1
        abt, abp = ab[t], (1.0 if last else ab[tau[s + 1]])
        sigma = eta * math.sqrt((1.0 - abp) / (1.0 - abt)) * math.sqrt(1.0 - abt / abp)
        d2 = 1.0 - abp - sigma * sigma
        if d2 < -1e-12:
            raise DDPMError("eta = %r makes sigma^2 exceed 1 - alpha_bar_prev at step %d" % (eta, s))
        coef[s] = (math.sqrt(1.0 - abt), math.sqrt(abt), math.sqrt(abp), math.sqrt(max(d2, 0.0)), sigma,
                   -1.0 if last else float(tau[s + 1]), float(t), 0.0)
    return coef, tau


def timesteps_reference(n_rows, T, seed, step, tag=TAG_T, row0=0):
    """t [n_rows] int64 of batch rows row0 .. at `step`: mulhi(word 0 of counter (0, step, row, tag), T)."""
    w = philox.words(n_rows, 1, seed, step, tag, row0)[:, 0].astype(np.uint64)
    return ((w * np.uint64(T)) >> np.uint64(32)).astype(np.int64)


def noise_reference(n_rows, I, seed, step, tag=TAG_E, row0=0):
    """The normals [n_rows, I] float64 of rows row0 .. at `step` under `tag` (TAG_S: the sampler's z at step `step`)."""
    return philox.normals(n_rows, I, seed, step, tag, row0)


def qsample_reference(x, T, E, seed, step, train=True, row0=0):
    """The rule in numpy: x [n, I] float32 in [0, 1] -> (t [n] int64, eps [n, I] float64, x_t [n, I] float64, temb
    rows [n, E] float32), x_t from the fp32 tables and the fp64 normals (the device's logf / sincospif are within a few
    ulp of them)."""
    x = np.asarray(x, dtype=np.float32)
    n, I = x.shape
    tab = tables(T, E)
    tags = (TAG_T, TAG_E) if train else (TAG_V, TAG_VE)
    t = timesteps_reference(n, T, seed, step, tags[0], row0)
    eps = noise_reference(n, I, seed, step, tags[1], row0)
    sa, s1 = tab["sa"].astype(np.float32).astype(np.float64), tab["s1"].astype(np.float32).astype(np.float64)
    x0 = 2.0 * x.astype(np.float64) - 1.0
    return t, eps, sa[t][:, None] * x0 + s1[t][:, None] * eps, tab["temb"].astype(np.float32)[t]


# ---- modules ---------------------------------------------------------------------------------------------------------
@stock_model
class Denoiser(nn.Module):
    """eps_theta: [x_t | temb[t]] (I + E wide) -> relu -> relu -> I."""

    def __init__(self, image_size, hidden_dim, time_dim):
        super().__init__()
        self.linear = nn.Linear(image_size + time_dim, hidden_dim)
        self.hidden = nn.Linear(hidden_dim, hidden_dim)
        self.out = nn.Linear(hidden_dim, image_size)

    def forward(self, xin):
        return _lin(self.out, _lin(self.hidden, _lin(self.linear, xin, "relu"), "relu"), "id")


@stock_model
class DDPM(nn.Module):
    """One Denoiser and the fixed tables (non-persistent buffers: state_dict holds the denoiser's six tensors)."""

    def __init__(self, image_size=784, hidden_dim=400, time_dim=32, T=1000):
        super().__init__()
        self.image_size, self.time_dim, self.T = check_shape(image_size, time_dim, T)
        self.hidden_dim = _int(hidden_dim, "hidden_dim")
        if self.hidden_dim < 1:
            raise DDPMError("hidden_dim must be >= 1")
        self.denoiser = Denoiser(self.image_size, self.hidden_dim, self.time_dim)
        self.shape = int(self.image_size ** 0.5)
        for name, v in tables(self.T, self.time_dim).items():
            self.register_buffer(name, torch.from_numpy(v.astype(np.float32)), persistent=False)

    def forward(self, x_t, t):
        """eps_theta(x_t, t): x_t [n, I] in the model's [-1, 1] scale, t [n] integer timesteps."""
        return self.denoiser(torch.cat([x_t, self.temb[t.long()]], dim=1).contiguous())


def ddpm_fused_ok(model):
    """True iff the model is DDPM itself with its Denoiser unchanged and consistent shapes."""
    d = getattr(model, "denoiser", None)
    if not (type(model).__dict__.get("_gm_stock_model", False) and type(d) is Denoiser and _stock_module(d, 3)):
        return False
    if not all(isinstance(getattr(model, n, None), torch.Tensor) for n in ("sa", "s1", "temb")):
        return False
    I, E, T = model.image_size, model.time_dim, model.T
    H = d.linear.weight.shape[0]
    return (tuple(d.linear.weight.shape) == (H, I + E) and tuple(d.hidden.weight.shape) == (H, H)
            and tuple(d.out.weight.shape) == (I, H) and tuple(model.temb.shape) == (T, E)
            and model.sa.numel() == T and model.s1.numel() == T
            and all(l.bias is not None for l in (d.linear, d.hidden, d.out)))


# ---- engine ----------------------------------------------------------------------------------------------------------
class DDPMEngine(TimeRegressionEngine):
    """The DDPM on the VAE engine's epoch machinery (index ring, multi-batch hipGraphs over a device counter).  Per
    training batch, 10 launches: 1. gm_gather_rows[_bits]_qsample (clean rows, [x_t | temb[t]], eps, t);  2.-4. the three
    forwards;  5. gm_ddpm_loss (dA, row partials);  6. dH2 = dA Wout [H2 > 0];  7. dH1 = dH2 Whid [H1 > 0];  8. the
    out / hidden weight gradients + Adam as a pair;  9. the first layer's weight gradient + Adam;  10. the loss sum with
    the counter tick.  Every input gradient is issued before the launch that steps the weights it reads.  A validation
    batch is launches 1-5 (no dA) and the sum.  The noise step of a training batch is ctr + nbase (DVAEEngine's scheme:
    nbase a device word configure() writes from the trainer's count of training batches, so the step is never baked
    into a graph), of a validation batch ctr (the batch's index in the pass).  No host noise ring, every batch its own
    gather.  One GPU only."""

    one_gpu = "the DDPM engine"
    fused_ok = staticmethod(ddpm_fused_ok)
    refusal = ("DDPM", "ddpm.DDPM", "Denoiser")  # the trainer: seed and noise_steps
    net, tables = "denoiser", ("sa", "s1", "temb")
    table_builder, noise_builder = "ddpm_tables", "ddpm_noise"
    target, steps = "Eps", "tq"

    def _settings(self):
        m = self.model
        return {"T": int(m.T), "time_dim": int(m.time_dim), "seed": int(self.trainer.seed)}

    def _gather_sample(self, st, b, noise, idx_slot):
        from . import ops_fused as of_
        of_.gather_rows_qsample(self.data, self.idx_ring.view(-1), self.X, self.Xin_full, self.Eps, self.tq, noise,
                                self.tab, B=b, idx_slot=idx_slot, stream=st)


# ---- trainer ---------------------------------------------------------------------------------------------------------
@stock
class DDPMTrainer(OneLossTrainer):
    """Trains a DDPM on L_simple and samples from it.  Histories: `losses` (one per training batch); the epoch line
    (mean training loss, validation loss); best_val_loss / best_model as the other VAE-family trainers; checkpoints
    (+ T, time_dim, seed in the optimizer state's config, checked under strict=True, and the number of training batches
    taken, so a resumed run continues the noise stream bit for bit).  One GPU only."""
    _line = "Epoch[%d/%d], Loss: %.6f, Val Loss: %.6f"
    _one_gpu = "DDPMTrainer"
    _engine_reads_trainer = True
    _error = DDPMError
    _fused_ok = staticmethod(ddpm_fused_ok)

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, *, seed=0):
        self.seed = check_seed(seed)                 # before anything runs
        super().__init__(model, train_iter, val_iter, test_iter, viz=viz)
        self.noise_steps = 0                         # training batches taken: the next one's noise step
        self._eval_step = 0                          # batch index within an evaluate() call
        self._sampler = {}

    def _tables(self):
        from . import ops_fused as of_
        m = self.model
        return of_.ddpm_tables(m.sa, m.s1, m.temb)

    def compute_batch(self, batch):
        """L_simple of a batch (general path: autograd over the fused linear kernels; x_t, eps and t from
        gm_ddpm_qsample on the contract's counter stream -- the training stream while the model trains, the validation
        one otherwise)."""
        from . import ops_fused as of_
        x = self._flat_batch(batch)
        train, step = self._noise_step()
        xin, eps, _t = of_.ddpm_qsample(x, of_.ddpm_noise(self.seed, train, step=step), self._tables())
        out = self.model.denoiser(xin)
        return torch.sum((eps - out) ** 2) / (x.shape[0] * x.shape[1])

    def _engine_class(self):
        return DDPMEngine

    def train(self, num_epochs, lr=2e-4, weight_decay=0.0, quiet=False):
        """VAETrainer.train with this model's defaults."""
        return super().train(num_epochs, lr=lr, weight_decay=weight_decay, quiet=quiet)

    # ---- sampling ---------------------------------------------------------------------------------------------------
    def sample(self, n, seed=0, steps=None, eta=1.0, clip=True, return_trajectory=False):
        """n samples [n, I] in [0, 1] -- (x + 1) / 2 clamped -- from `steps` sampler steps (None: all T) at `eta`
        (1: ancestral DDPM, 0: deterministic DDIM); return_trajectory: (samples, trajectory [steps + 1, n, I]), the
        trajectory x_T, ..., x_0 in the model's [-1, 1] scale.  Runs after a device synchronise; the global generator,
        the model's mode and the parameters are untouched.  A stock model replays a hipGraph of G <= 32 steps steps / G
        times over a device counter (use_graph = False: launch by launch, same bits)."""
        from . import ops_fused as of_
        n, seed, m = _int(n, "n"), check_seed(seed), self.model
        if n < 1:
            raise DDPMError("n must be >= 1, got %d" % n)
        S, eta = check_sampler(m.T, steps, eta)
        coef64, tau = reverse_table(m.T, S, eta)
        if not torch.cuda.is_available():
            raise GMError("sample runs on the MI355X only: no GPU is visible")
        dev = next(m.parameters()).device
        if dev.type != "cuda":
            raise GMError("sample: the model is not on the GPU")
        torch.cuda.synchronize()
        I, E, H = m.image_size, m.time_dim, m.hidden_dim
        fused = ddpm_fused_ok(m)
        c = self._sampler
        if c.get("n") != n or c.get("dev") != dev:
            z = lambda *s: torch.empty(*s, device=dev)
            c.clear()
            c.update(n=n, dev=dev, Xin=z(n, _align4(I + E)), H1=z(n, H), H2=z(n, H), Out=z(n, I),
                     ctr=torch.zeros(1, dtype=torch.int64, device=dev),
                     done=torch.zeros(1, dtype=torch.int32, device=dev), coef={}, graph=None)
        Xin_full = c["Xin"]
        Xin = Xin_full[:, :I + E]
        if S not in c["coef"]:
            c["coef"][S] = torch.empty(S, 8, device=dev)
        coef = c["coef"][S]
        coef.copy_(torch.from_numpy(coef64.astype(np.float32)))
        traj = torch.empty(S + 1, n, I, device=dev) if return_trajectory else None
        of_.ddpm_prior(Xin_full, m.temb, I, seed, step=S, t=int(tau[0]), traj=traj)
        d = m.denoiser
        w = [p.detach() for p in (d.linear.weight, d.linear.bias, d.hidden.weight, d.hidden.bias, d.out.weight,
                                  d.out.bias)] if fused else None

        def step(st, slot=None, s=0, tick=None):
            if fused:
                ops.linear_fwd(Xin, w[0], w[1], c["H1"], "relu", stream=st)
                ops.linear_fwd(c["H1"], w[2], w[3], c["H2"], "relu", stream=st)
                ops.linear_fwd(c["H2"], w[4], w[5], c["Out"], "id", stream=st)
                out = c["Out"]
            else:
                with torch.no_grad():
                    out = d(Xin.contiguous()).contiguous()
            of_.ddpm_reverse(Xin_full, out, coef, m.temb, I, seed, clip=clip, slot=slot, step=s, traj=traj, tick=tick,
                             done=c["done"] if tick is not None else None, stream=st)

        if fused and self.use_graph:
            G = max(g for g in range(1, min(S, GRAPH_STEPS) + 1) if S % g == 0)
            key = (S, G, eta, bool(clip), seed, coef.data_ptr(), m.temb.data_ptr()) + tuple(t.data_ptr() for t in w)
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
        out = ((Xin_full[:, :I] + 1.0) / 2.0).clamp_(0.0, 1.0)
        return (out, traj) if return_trajectory else out

    def denoise(self, images, t, seed=None, batch=1024):
        """(noisy, x0_hat) in [0, 1]: `images` taken to timestep t with the training stream's noise at step 0 (seed:
        the trainer's by default), and the one-shot estimate x0_hat = (x_t - s1_t eps_theta(x_t, t)) / sa_t clamped to
        [-1, 1].  Device tensors [n, pixels]; the global generator and the model's mode are untouched."""
        from . import ops_fused as of_
        m = self.model
        t = _int(t, "t")
        if not 0 <= t < m.T:
            raise DDPMError("t must lie in [0, T = %d), got %d" % (m.T, t))
        x = images.reshape(images.shape[0], -1)
        x = to_cuda(x).to(torch.float32).contiguous()
        if not x.is_cuda:
            raise GMError("denoise runs on the MI355X only: no GPU is visible")
        seed = self.seed if seed is None else check_seed(seed)
        _xin, eps, _t = of_.ddpm_qsample(x, of_.ddpm_noise(seed, True, step=0), self._tables())
        torch.cuda.synchronize()
        sa, s1 = float(m.sa[t]), float(m.s1[t])
        xt = sa * (2.0 * x - 1.0) + s1 * eps
        tt = torch.full((min(batch, x.shape[0]),), t, dtype=torch.int64, device=x.device)
        with torch.no_grad():
            e = torch.cat([m(xt[i:i + batch], tt[:xt[i:i + batch].shape[0]]) for i in range(0, x.shape[0], batch)])
        x0 = ((xt - s1 * e) / sa).clamp_(-1.0, 1.0)
        to01 = lambda v: ((v + 1.0) / 2.0).clamp_(0.0, 1.0)
        return to01(xt), to01(x0)

    # ---- visualisation, checkpoints -----------------------------------------------------------------------------------
    viz_steps = 50               # sampler steps of the per-epoch sample grid (min(T, viz_steps))

    def sample_images(self, epoch=-100, num_images=36, save=True):
        return viz.ddpm_sample_images(self, epoch, num_images, save, self.viz_dir,
                                      steps=min(self.model.T, self.viz_steps))

    def log_likelihood(self, images=None, k=500, seed=0):
        raise GMError("log_likelihood needs vae.py's Encoder and Decoder unchanged (a DDPM has neither); parzen() "
                      "scores its samples")

    def reconstruct_images(self, images, epoch, save=True):
        raise GMError("a DDPM has no encoder: denoise(images, t) returns the one-shot estimate of a noised image")

    def viz_loss(self):
        viz.one_loss_curve(self, "L_simple")


__all__ = ["Denoiser", "DDPM", "DDPMTrainer", "DDPMEngine", "DDPMError", "tables", "reverse_table",
           "timesteps_reference", "noise_reference", "qsample_reference", "FlatAdam"]
