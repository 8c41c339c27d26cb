"""Bayesian GAN (Saatchi & Wilson 2017, arXiv 1705.09558; the reference's src/bayes_gan.py is a docstring and a TODO,
its README to-do list names it, README.md:95).  J_g generator samples and J_d critic samples from the posterior,
each moved by SGHMC (stochastic-gradient Hamiltonian Monte Carlo) with fresh Gaussian noise on every step.
Exported by src/bayes_gan.py as Generator / Discriminator / BayesGAN / BayesGANTrainer.

The contract, per iteration of ns_gan.py's loop (ns_gan.py:94-170, same sampler protocol):
  D_steps critic updates, each on its own process_batch(train_iter):
    z_j = Normal(latent(0, j), t_D) [b, Z], x~_j = G_j(z_j) (no gradient to G),
    L_D^k = -(1/b) sum_i [log(D_k(x_i) + eps) + (1/J_g) sum_j log(1 - D_k(x~_j,i) + eps)],
    every critic one SGHMC step with g = grad L_D^k + theta / (sigma^2 N), recorded loss mean_k L_D^k;
  one generator update: z'_j = Normal(latent(1, j), t_G),
    L_G^j = -(1/b)(1/J_d) sum_k sum_i log(D_k(G_j(z'_j,i)) + eps), every generator one SGHMC step, loss mean_j L_G^j.
  SGHMC per element: v <- (1 - alpha) v - eta g + sqrt(2 alpha eta / N) xi ; theta <- theta + v, with
    xi = Normal(param(side, sample, tensor), t) -- the Philox generator of csrc/gm_bgan.hip.
Fused path: BayesGANEngine (hipGraphs of whole iterations, critics stacked into one [J_d H, I] layer).  Overridden
hooks, edited modules or shapes outside BayesGANEngine.fused_ok: autograd over ops.fused_linear + FlatSGHMC, which
calls the same SGHMC kernel, so both paths draw the same noise."""
import numpy as np
import torch
import torch.nn as nn

from . import ops, ops_fused
from ._lib import GMError, slot
from .ops_fused import bgan_stream_latent, bgan_stream_param
from .ring_engine import ChunkedReplay, reference_loader_ok
from .trainers import (CHECKPOINT_VERSION, EPS, Discriminator, GANTrainer, Generator, _decode_rows, _load_checkpoint,
                       _parzen, _plain, _stock_module, stock, stock_model)

MAX_J = 16
HISTORY = ("Glosses", "Dlosses", "num_epochs")
_SECOND = {"G": "generate", "D": "discriminate"}


@stock_model
class BayesGAN(nn.Module):
    """.G: nn.ModuleList of num_gen ns_gan.py Generators, .D: nn.ModuleList of num_disc ns_gan.py Discriminators
    (built in the order G.0 .. G.{J_g-1}, D.0 .., so a seed fixes the weights), .z_dim / .image_size / .hidden_dim /
    .shape as on NSGAN."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20, num_gen=4, num_disc=2):
        super().__init__()
        for name, j in (("num_gen", num_gen), ("num_disc", num_disc)):
            if not (isinstance(j, (int, np.integer)) and 1 <= j <= MAX_J):
                raise ValueError("%s must be an integer in [1, %d], got %r" % (name, MAX_J, j))
        self.image_size, self.hidden_dim, self.z_dim = image_size, hidden_dim, z_dim
        self.num_gen, self.num_disc = int(num_gen), int(num_disc)
        self.G = nn.ModuleList([Generator(image_size, hidden_dim, z_dim) for _ in range(num_gen)])
        self.D = nn.ModuleList([Discriminator(image_size, hidden_dim, 1) for _ in range(num_disc)])
        self.shape = int(image_size ** 0.5)


def _tensors(net, side):
    """The four SGHMC tensors of one sample, in stream-word order."""
    second = getattr(net, _SECOND[side])
    return [net.linear.weight, net.linear.bias, second.weight, second.bias]


class FlatSGHMC:
    """The general path's SGHMC optimizer: one gm_sghmc_step launch over a private flat copy of the samples' tensors,
    segment table (offset, numel, param(side, sample, tensor)), so it draws exactly the fused engine's noise."""

    def __init__(self, nets, side, seed, lr, friction, prior, noise, momenta=None):
        self.params = [p for net in nets for p in _tensors(net, "D" if side == 0 else "G")]
        dev = self.params[0].device
        self.offs, segs, o = [], [], 0
        for k, net in enumerate(nets):
            for ti, p in enumerate(_tensors(net, "D" if side == 0 else "G")):
                self.offs.append(o)
                segs.append((o, p.numel(), bgan_stream_param(side, k, ti)))
                o += (p.numel() + 3) // 4 * 4
        self.segs = ops_fused.sghmc_segments(segs)
        self.flat, self.grad, self.v = (torch.zeros(o, device=dev) for _ in range(3))
        if momenta is not None:
            for p, off, m in zip(self.params, self.offs, momenta):
                self.v[off:off + p.numel()].copy_(m.reshape(-1))
        self.seed, self.friction, self.prior, self.noise = seed, friction, prior, noise
        self.lr = torch.tensor([lr], dtype=torch.float32, device=dev)

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    @torch.no_grad()
    def step(self, t):
        for p, o in zip(self.params, self.offs):
            k = p.numel()
            self.flat[o:o + k].copy_(p.data.reshape(-1))
            if p.grad is None:
                self.grad[o:o + k].zero_()
            else:
                self.grad[o:o + k].copy_(p.grad.reshape(-1))
        ops_fused.sghmc_step(self.flat, self.grad, self.v, self.segs, self.lr, self.friction, self.prior, self.noise,
                             self.seed, t=t)
        for p, o in zip(self.params, self.offs):
            p.data.copy_(self.flat[o:o + p.numel()].view(p.shape))

    def momenta(self):
        return [self.v[o:o + p.numel()].view(p.shape).detach().cpu().clone() for p, o in zip(self.params, self.offs)]


class BayesGANEngine(ChunkedReplay):
    """The fused path.  Critics stacked: their linear.weight / .bias are one [J_d H, I] matrix and one [J_d H] vector,
    their second layers one [J_d, H] and one [J_d] (FlatParams groups, the modules' parameters stay views), so the
    critic forward over the (1 + J_g) b rows [x; x~_0; ...] is one linear_fwd, dW1 of every critic one linear_bwd_dw
    and the generators' dX one linear_bwd_dx that sums over the critics.  Generators: per-sample launches of the plain
    ops into row slices of shared buffers.  Latent draws and SGHMC noise come from the device Philox generator with
    the step counters t_D / t_G on the device; batch rows through the sampler protocol replayed on the host
    (draw_sampler_indices) into an index ring read by gather_rows.  Whole iterations are captured as hipGraphs of
    `graph_iters` iterations (and of 1 for the tail)."""

    @staticmethod
    def fused_ok(model):
        """The fused kernels' limits: 1 <= J_g, J_d <= 16 (stream words), H % 4 == 0 and H <= 1024 (gm_bgan_head's
        register tile), and the ns_gan.py modules at the model's sizes (the plain GEMMs take any shape)."""
        H, I, Z = model.hidden_dim, model.image_size, model.z_dim
        Jg, Jd = len(model.G), len(model.D)
        return (1 <= Jg <= MAX_J and 1 <= Jd <= MAX_J and H % 4 == 0 and 0 < H <= 1024 and I > 0 and Z > 0
                and all(tuple(g.linear.weight.shape) == (H, Z) and tuple(g.generate.weight.shape) == (I, H)
                        for g in model.G)
                and all(tuple(d.linear.weight.shape) == (H, I) and tuple(d.discriminate.weight.shape) == (1, H)
                        for d in model.D))

    def __init__(self, model, data, B, device, use_graph=True):
        from .engine import FlatParams, _Linear
        self.model, self.data, self.B, self.dev, self.use_graph = model, data, B, device, use_graph
        self.Jg, self.Jd = len(model.G), len(model.D)
        self.H, self.I, self.Z = model.hidden_dim, model.image_size, model.z_dim
        Jg, Jd, H, I, Z = self.Jg, self.Jd, self.H, self.I, self.Z
        D, G = model.D, model.G
        self.fD = FlatParams([tuple(d.linear.weight for d in D), tuple(d.linear.bias for d in D),
                              tuple(d.discriminate.weight for d in D), tuple(d.discriminate.bias for d in D)], device)
        self.fG = FlatParams([p for g in G for p in _tensors(g, "G")], device)
        o = self.fD.offsets
        pD = self.fD.params
        at = lambda t, i, n: t[o[i]:o[i] + n]
        self.W1, self.gW1 = (at(t, 0, Jd * H * I).view(Jd * H, I) for t in (self.fD.flat, self.fD.grad))
        self.b1, self.gb1 = (at(t, Jd, Jd * H) for t in (self.fD.flat, self.fD.grad))
        self.w2, self.gw2 = (at(t, 2 * Jd, Jd * H).view(Jd, H) for t in (self.fD.flat, self.fD.grad))
        self.b2, self.gb2 = (at(t, 3 * Jd, Jd) for t in (self.fD.flat, self.fD.grad))
        idx = {id(p): i for i, p in enumerate(pD)}
        self.segD = ops_fused.sghmc_segments(
            [(o[idx[id(p)]], p.numel(), bgan_stream_param(0, k, ti))
             for k, d in enumerate(D) for ti, p in enumerate(_tensors(d, "D"))])
        self.gen = [(_Linear(self.fG, g.linear), _Linear(self.fG, g.generate)) for g in G]
        oG = {id(p): off for p, off in zip(self.fG.params, self.fG.offsets)}
        self.segG = ops_fused.sghmc_segments(
            [(oG[id(p)], p.numel(), bgan_stream_param(1, k, ti))
             for k, g in enumerate(G) for ti, p in enumerate(_tensors(g, "G"))])
        z = lambda *s: torch.zeros(*s, device=device)
        R = (1 + Jg) * B
        self.X = z(R, I)                 # [x; G_0(z_0); ...]
        self.Zb = z(Jg * B, Z)
        self.HG = z(Jg * B, H)
        self.dHG = z(Jg * B, H)
        self.Hd = z(R, Jd * H)
        self.dXf = z(Jg * B, I)
        self.wsD = ops_fused.bgan_head_workspace(0, B, Jg, Jd, H, device)
        self.wsG = ops_fused.bgan_head_workspace(1, B, Jg, Jd, H, device)
        self.ctr = torch.zeros(2, dtype=torch.int64, device=device)      # t_D, t_G
        self.lr = z(2)                                                  # D_lr, G_lr
        self.steps_planned = 0

    # ---- one iteration's launches -------------------------------------------------------------------------------
    def _gen_forward(self, s, Xf):
        B, H = self.B, self.H
        for j, (l1, l2) in enumerate(self.gen):
            r = slice(j * B, (j + 1) * B)
            ops.linear_fwd(self.Zb[r], l1.W, l1.b, self.HG[r], "relu", stream=s)
            ops.linear_fwd(self.HG[r], l2.W, l2.b, Xf[r], "sigmoid", stream=s)

    def _issue(self, s, i):
        """One iteration; its place i in the chunk is not read (the ring rows are addressed by t_D on the device)."""
        B, Jg, Jd, Z = self.B, self.Jg, self.Jd, self.Z
        tD, tG = self.ctr[0:1], self.ctr[1:2]
        Xf = self.X[B:]
        for _ in range(self.D_steps):
            ops_fused.philox_normal(self.seed, bgan_stream_latent(0, 0), 0, B * Z, out=self.Zb, nstreams=Jg,
                                    stream_stride=16, step=tD, stream=s)
            ops.gather_rows(self.data, self.idx, self.X[:B], idx_slot=slot(tD.data_ptr(), 1, 0, self.ring, B),
                            stream=s)
            self._gen_forward(s, Xf)
            ops.linear_fwd(self.X, self.W1, self.b1, self.Hd, "relu", stream=s)
            ops_fused.bgan_head(self.Hd, self.w2, self.b2, 0, B, Jg, Jd, self.wsD, gw2=self.gw2, gb2=self.gb2,
                                loss_out=self.dloss, loss_slot=slot(tD.data_ptr(), 1, 0, self.dloss.shape[0], Jd),
                                stream=s)
            ops.linear_bwd_dw(self.Hd, self.X, self.gW1, self.gb1, stream=s)
            ops_fused.sghmc_step(self.fD.flat, self.fD.grad, self.fD.v, self.segD, self.lr[0:1], self.friction,
                                 self.priorD, self.noise, self.seed, step=tD, stream=s)
            ops.tick(tD, stream=s)
        ops_fused.philox_normal(self.seed, bgan_stream_latent(1, 0), 0, B * Z, out=self.Zb, nstreams=Jg,
                                stream_stride=16, step=tG, stream=s)
        self._gen_forward(s, Xf)
        HdG = self.Hd[:Jg * B]
        ops.linear_fwd(Xf, self.W1, self.b1, HdG, "relu", stream=s)
        ops_fused.bgan_head(HdG, self.w2, self.b2, 1, B, Jg, Jd, self.wsG, loss_out=self.gloss,
                            loss_slot=slot(tG.data_ptr(), 1, 0, self.gloss.shape[0], Jg), stream=s)
        ops.linear_bwd_dx(HdG, self.W1, self.dXf, below=Xf, epi="sigmoid", stream=s)
        for j, (l1, l2) in enumerate(self.gen):
            r = slice(j * B, (j + 1) * B)
            ops.linear_bwd_dw(self.dXf[r], self.HG[r], l2.gW, l2.gb, stream=s)
            ops.linear_bwd_dx(self.dXf[r], l2.W, self.dHG[r], below=self.HG[r], epi="relu", stream=s)
            ops.linear_bwd_dw(self.dHG[r], self.Zb[r], l1.gW, l1.gb, stream=s)
        ops_fused.sghmc_step(self.fG.flat, self.fG.grad, self.fG.v, self.segG, self.lr[1:2], self.friction,
                             self.priorG, self.noise, self.seed, step=tG, stream=s)
        ops.tick(tG, stream=s)

    # ---- run settings, host draws, replay ----------------------------------------------------------------------
    def configure(self, n_iters, G_lr, D_lr, D_steps, friction, prior_std, N, seed, t_D, t_G, momenta=None):
        for f in (self.fD, self.fG):
            f.rebind()
        self.D_steps, self.seed = int(D_steps), int(seed)
        self.friction = float(friction)
        self.priorD = self.priorG = 1.0 / (float(prior_std) ** 2 * N)
        self.noise = 2.0 * float(friction) / N
        self.t_D, self.t_G = int(t_D), int(t_G)
        self.lr.copy_(torch.tensor([D_lr, G_lr], dtype=torch.float32))
        self.ctr.copy_(torch.tensor([self.t_D, self.t_G], dtype=torch.int64))
        self.fD.v.zero_()
        self.fG.v.zero_()
        if momenta is not None:
            self._load_momenta(momenta)
        self.dloss = torch.zeros(max(1, n_iters * self.D_steps), self.Jd, device=self.dev)
        self.gloss = torch.zeros(max(1, n_iters), self.Jg, device=self.dev)
        self.ring = max(1, self.graph_iters) * self.D_steps
        self.idx = torch.zeros(self.ring, self.B, dtype=torch.int64, device=self.dev)
        self._new_rings(self.idx)
        self.t_D0, self.t_G0 = self.t_D, self.t_G
        self.steps_planned = n_iters

    def _params(self):
        return ([p for d in self.model.D for p in _tensors(d, "D")], [p for g in self.model.G for p in _tensors(g, "G")])

    def _load_momenta(self, momenta):
        for f, plist, vs in zip((self.fD, self.fG), self._params(), (momenta["vD"], momenta["vG"])):
            off = {id(p): o for p, o in zip(f.params, f.offsets)}
            for p, v in zip(plist, vs):
                f.v[off[id(p)]:off[id(p)] + p.numel()].copy_(v.reshape(-1).to(self.dev))

    def momenta(self):
        out = {}
        for f, plist, name in zip((self.fD, self.fG), self._params(), ("vD", "vG")):
            off = {id(p): o for p, o in zip(f.params, f.offsets)}
            out[name] = [f.v[off[id(p)]:off[id(p)] + p.numel()].view(p.shape).detach().cpu().clone() for p in plist]
        return out

    def _host_draws(self, k):
        """The global generator's draws of k iterations in NSGANTrainer's order: per critic update the sampler's
        (draw_sampler_indices, into the index ring) and the b x Z normals NSGAN's compute_noise takes, then the
        generator update's b x Z -- the latter are advanced past, never used."""
        from .engine import draw_sampler_indices
        n = self.data.shape[0]
        t = self.t_D
        with self._staging() as (host,):
            for _ in range(k):
                for _ in range(self.D_steps):
                    draw_sampler_indices(n, self.B, host[t % self.ring].numpy())
                    torch.randn(self.B, self.Z)
                    t += 1
                torch.randn(self.B, self.Z)
            self.idx.copy_(host, non_blocking=True)

    def _after_chunk(self, k):
        self.t_D += k * self.D_steps
        self.t_G += k

    def losses(self, it0, it1):
        """(G losses, D losses) of iterations [it0, it1) of this train() call: mean_j L_G^j, and per iteration the
        mean over its critic updates of mean_k L_D^k (one read-back)."""
        nD, nG = self.dloss.shape[0], self.gloss.shape[0]
        dl = self.dloss.cpu().double().numpy()
        gl = self.gloss.cpu().double().numpy()
        G, D = [], []
        for it in range(it0, it1):
            G.append(float(np.mean(gl[(self.t_G0 + it) % nG])))
            D.append(float(np.mean([np.mean(dl[(self.t_D0 + it * self.D_steps + d) % nD])
                                    for d in range(self.D_steps)])))
        return G, D


@stock
class BayesGANTrainer(GANTrainer):
    """ns_gan.py's Trainer surface for the Bayesian GAN: train(num_epochs, G_lr, D_lr, D_steps, friction, prior_std,
    dataset_size, quiet), sample / parzen (a mixture over the generator samples), generate_images, checkpoints.
    seed: the key of the device generator; t_D / t_G: the critic / generator update counters (they never reset, so no
    noise is drawn twice)."""
    _STOCK = ("train_D", "train_G", "process_batch", "compute_noise", "latent")

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False, seed=0):
        super().__init__(model, train_iter, val_iter, test_iter, viz)
        self.seed = int(seed)
        self.t_D, self.t_G = 0, 0
        self._state = None                       # the momenta of the last train() call

    # ---- hooks (the general path) -------------------------------------------------------------------------------
    def latent(self, phase, j, b):
        """The contract's z of generator j: Normal(latent(phase, j), t_D (phase 0) or t_G (phase 1)) as [b, z_dim]."""
        Z = self.model.z_dim
        t = self.t_D if phase == 0 else self.t_G
        dev = next(self.model.parameters()).device
        return ops_fused.philox_normal(self.seed, bgan_stream_latent(phase, j), t, b * Z, device=dev).view(b, Z)

    def train_D(self, images):
        """[J_d] tensor of L_D^k."""
        m = self.model
        b, Jg = images.shape[0], len(m.G)
        with torch.no_grad():
            fakes = [m.G[j](self.latent(0, j, b)) for j in range(Jg)]
        out = []
        for d in m.D:
            fake = sum(torch.mean(torch.log(1 - d(x) + EPS)) for x in fakes) / Jg
            out.append(-(torch.mean(torch.log(d(images) + EPS)) + fake))
        return torch.stack(out)

    def train_G(self, images):
        """[J_g] tensor of L_G^j against the critics as they stand."""
        m = self.model
        b, Jd = images.shape[0], len(m.D)
        out = []
        for j, g in enumerate(m.G):
            x = g(self.latent(1, j, b))
            out.append(-sum(torch.mean(torch.log(d(x) + EPS)) for d in m.D) / Jd)
        return torch.stack(out)

    # ---- path selection ---------------------------------------------------------------------------------------
    def _stock(self):
        if not self._stock_prefix():
            return False
        m = self.model
        G, D = getattr(m, "G", None), getattr(m, "D", None)
        if not (type(G) is nn.ModuleList and type(D) is nn.ModuleList and len(G) and len(D)):
            return False
        if not (all(type(g) is Generator and _stock_module(g) for g in G)
                and all(type(d) is Discriminator and _stock_module(d) for d in D)):
            return False                               # edited / subclassed networks: general path
        if not BayesGANEngine.fused_ok(m):
            return False
        return reference_loader_ok(self.train_iter)

    def _make_engine(self, data, loader, dev):
        return BayesGANEngine(self.model, data, loader.batch_size, dev, use_graph=self.use_graph)

    def _nsgan_noise_cursor(self, b):
        """Advance the global generator past the b x z_dim normals NSGANTrainer's compute_noise takes at this point of
        its loop; the values are not used (the latent draws come from the device generator)."""
        torch.randn(b, self.model.z_dim)

    # ---- the loop -------------------------------------------------------------------------------------------------
    def train(self, num_epochs, G_lr=1e-3, D_lr=1e-3, D_steps=1, friction=0.1, prior_std=1.0, dataset_size=None,
              quiet=False):
        from . import dp
        if dp.current()[0] > 1:
            raise GMError("BayesGANTrainer runs on one GPU: data parallelism is not implemented for it")
        if not 0.0 <= friction <= 1.0 or prior_std <= 0:
            raise ValueError("friction must lie in [0, 1] and prior_std be positive")
        N = int(dataset_size) if dataset_size is not None else len(self.train_iter.dataset)
        epoch_steps = int(np.ceil(len(self.train_iter) / D_steps))
        resume = self.__dict__.pop("_resume_optim", None)
        momenta = None if resume is None else {"vD": resume["vD"], "vG": resume["vG"]}
        if self._stock():
            eng = self._get_engine()
            eng.use_graph = self.use_graph
            eng.configure(num_epochs * epoch_steps, G_lr, D_lr, D_steps, friction, prior_std, N, self.seed,
                          self.t_D, self.t_G, momenta)
            self._state = eng
            for epoch in range(1, num_epochs + 1):
                self.model.train()
                it0 = (epoch - 1) * epoch_steps
                eng.run(epoch_steps)
                self.t_D, self.t_G = eng.t_D, eng.t_G
                G_losses, D_losses = eng.losses(it0, it0 + epoch_steps)
                self._end_epoch(epoch, num_epochs, G_losses, D_losses, quiet)
                self._viz_epoch(epoch)
            return
        # GENERAL path: the hooks over autograd, one FlatSGHMC per side
        m = self.model
        prior, noise = 1.0 / (float(prior_std) ** 2 * N), 2.0 * float(friction) / N
        d_opt = FlatSGHMC(list(m.D), 0, self.seed, D_lr, friction, prior, noise, momenta and momenta["vD"])
        g_opt = FlatSGHMC(list(m.G), 1, self.seed, G_lr, friction, prior, noise, momenta and momenta["vG"])
        self._state = (d_opt, g_opt)
        for epoch in range(1, num_epochs + 1):
            m.train()
            G_losses, D_losses = [], []
            for _ in range(epoch_steps):
                step = []
                for _ in range(D_steps):
                    images = self.process_batch(self.train_iter)
                    self._nsgan_noise_cursor(images.shape[0])
                    d_opt.zero_grad()
                    L = self.train_D(images)
                    L.sum().backward()
                    d_opt.step(self.t_D)
                    self.t_D += 1
                    step.append(L.mean().item())
                D_losses.append(np.mean(step))
                self._nsgan_noise_cursor(images.shape[0])
                g_opt.zero_grad()
                L = self.train_G(images)
                L.sum().backward()
                g_opt.step(self.t_G)
                self.t_G += 1
                G_losses.append(L.mean().item())
            self._end_epoch(epoch, num_epochs, G_losses, D_losses, quiet)
            self._viz_epoch(epoch)

    # ---- sampling ---------------------------------------------------------------------------------------------
    def sample(self, n, seed=0):
        """n images [n, image_size] of the posterior mixture: z from torch.Generator().manual_seed(seed) (never the
        global generator), row i from G_{i mod J_g}."""
        gen = torch.Generator().manual_seed(int(seed))
        z = torch.randn(int(n), self.model.z_dim, generator=gen)
        J = len(self.model.G)
        out = None
        for j, g in enumerate(self.model.G):
            if j >= n:
                break
            y = _decode_rows(g, z[j::J])
            if out is None:
                out = torch.empty(int(n), y.shape[1], device=y.device)
            out[j::J] = y
        return out

    def parzen(self, n_samples=10000, sigmas=None, n_val=10000, seed=0):
        """Parzen-window log-likelihood of the test images under the mixture's samples (metrics.parzen_evaluate)."""
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

    def generate_images(self, epoch, num_outputs=36, save=True):
        """A grid of mixture samples (sample(num_outputs, seed=epoch): no global draw), saved as
        ../viz/<name>/reconst_<epoch>.png."""
        import os
        from . import viz
        m = self.model
        images = self.sample(num_outputs, seed=epoch).view(num_outputs, m.shape, m.shape).cpu().numpy()
        grid = int(num_outputs ** 0.5)
        if save:
            out = os.path.join(self.viz_dir if self.viz_dir is not None else os.path.join("..", "viz"), self.name)
            os.makedirs(out, exist_ok=True)
            viz.write_png_gray(os.path.join(out, "reconst_%d.png" % epoch), viz.make_grid(images, grid))
        return images

    # ---- checkpoints ------------------------------------------------------------------------------------------
    def _momenta(self):
        st = self._state
        if st is None:
            raise GMError("save_checkpoint needs a finished train() call")
        if isinstance(st, BayesGANEngine):
            return st.momenta()
        return {"vD": st[0].momenta(), "vG": st[1].momenta()}

    def save_checkpoint(self, savepath, collective=True):
        """Weights (state_dict keys as save_model), the SGHMC momenta, seed, t_D, t_G, the global CPU generator's
        state and the histories.  After load_checkpoint() the next train() continues as if the run had not stopped."""
        optim = dict(self._momenta(), t_D=self.t_D, t_G=self.t_G, seed=self.seed)
        state = {"version": CHECKPOINT_VERSION, "name": self.name,
                 "model": {k: v.detach().cpu() for k, v in self.model.state_dict().items()},
                 "optim": optim, "rng": torch.get_rng_state(),
                 "history": {n: _plain(getattr(self, n)) for n in HISTORY}}
        torch.save(state, savepath)

    def load_checkpoint(self, loadpath, strict=True):
        _load_checkpoint(self, loadpath, strict)
        r = self._resume_optim
        self.t_D, self.t_G, self.seed = int(r["t_D"]), int(r["t_G"]), int(r["seed"])


__all__ = ["Generator", "Discriminator", "BayesGAN", "BayesGANTrainer", "BayesGANEngine", "FlatSGHMC"]
