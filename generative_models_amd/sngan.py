"""Spectrally normalised hinge GAN: ns_gan.py's model and loop with a critic whose Lipschitz constant is bounded by
construction (spectral normalisation, Miyato et al. 2018, arXiv 1802.05957), the hinge loss and the two learning rates
with Adam betas (0, 0.9) of the Self-attention GAN (Zhang et al. 2018, arXiv 1805.08318) -- SAGAN's three parts that fit
an MLP; there is no attention.  Exported by src/sn_gan.py as Generator / Discriminator / SNGAN / SNGANTrainer.

The contract:
  * Generator: ns_gan.py's, unchanged and unconditioned (trainers.Generator); it is not normalised.
  * Discriminator: `linear` (I -> H), `discriminate` (H -> 1) and a registered buffer `u` [H], initialised as
    normalize(randn(H)) from the global CPU generator at construction, after the two layers' own initialisation
    (torch.nn.utils.spectral_norm does the same): ONE draw more than an ns_gan.py model makes.  state_dict keys:
    ns_gan.py's plus `D.u`.  The output is the raw logit, no sigmoid.
  * D.forward(x), with W = linear.weight, b = linear.bias, w2 = discriminate.weight, b2 = discriminate.bias:
    in training mode one power-iteration step without gradient,
        v = W^T u / max(||W^T u||, 1e-12);   u' = W v / max(||W v||, 1e-12);   u <- u'
    then sigma = u'^T W v with u' and v held constant for the backward, and
        Wbar = W / sigma;  w2bar = w2 / ||w2||;  h = relu(x Wbar^T + b);  s = h . w2bar + b2.
    (A one-row matrix's spectral norm is its 2-norm: the head needs no state.)  Eval mode uses the stored u, recomputes
    v and sigma = u^T W v from it and does not write u.  sigma = 0 is outside the contract, as it is in torch.  One
    forward on the stacked rows agrees with torch.nn.utils.spectral_norm(nn.Linear) exactly.
  * The backward in closed form, G = d loss / d Wbar and g = d loss / d w2bar:
        gW = (G - <G, Wbar> u' v^T) / sigma;      gw2 = (g - <g, w2bar> w2bar) / ||w2||.
  * Loop and RNG: ns_gan.py:94-170 exactly (the sampler's draws, randn(B, Z) in train_D, randn(B, Z) in train_G).  A
    critic step calls D once, on the stacked [x; G(z)]: one power iteration.  The generator step calls D once, on
    G(z'): another power iteration, no critic update.  At D_steps = 1, u advances twice per iteration.
  * D_loss = mean(relu(1 - s(x))) + mean(relu(1 + s(G(z)))), G(z) detached;  G_loss = -mean(s(G(z'))).
  * Two Adams (G.parameters(), D.parameters()) created per train() call:
    train(num_epochs, G_lr=1e-4, D_lr=4e-4, D_steps=1, betas=(0.0, 0.9)).  Glosses / Dlosses with NSGAN's semantics.
Fused path: SNGANEngine below (stock modules and hooks, H % 4 == 0, H <= 1024, I <= 8192); otherwise autograd over the
module's own forward (the power iteration and W / sigma as torch ops, the matrix products ops.fused_linear) and two
FlatAdams."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, ops_fused
from ._lib import GMError, slot
from .trainers import FlatAdam, GANTrainer, Generator, _stock_module, stock, stock_model, to_cuda
from .engine import FlatParams, _Linear
from .ring_engine import TwoAdamRingEngine, reference_loader_ok

MAX_H, MAX_I = ops_fused.SN_MAX_H, ops_fused.SN_MAX_I
NORM_EPS = 1e-12


@stock_model
class Discriminator(nn.Module):
    """ns_gan.py:49-60 with both layers spectrally normalised and a raw logit out (the contract above)."""

    def __init__(self, image_size, hidden_dim, output_dim=1):
        super().__init__()
        self.linear = nn.Linear(image_size, hidden_dim)
        self.discriminate = nn.Linear(hidden_dim, output_dim)
        self.register_buffer("u", F.normalize(torch.randn(hidden_dim), dim=0, eps=NORM_EPS))

    def forward(self, x):
        if not x.is_cuda:
            raise GMError("generative_models_amd computes on MI355X only: got a %s tensor and there is no CPU "
                          "fallback (move the model and inputs with to_cuda)" % x.device)
        W, w2 = self.linear.weight, self.discriminate.weight
        with torch.no_grad():
            u = self.u.clone()
            v = F.normalize(torch.mv(W.t(), u), dim=0, eps=NORM_EPS)
            if self.training:
                u = F.normalize(torch.mv(W, v), dim=0, eps=NORM_EPS)
                self.u.copy_(u)
        sigma = torch.dot(u, torch.mv(W, v))
        h = ops.fused_linear(x, W / sigma, self.linear.bias, "relu")
        return ops.fused_linear(h, w2 / torch.linalg.vector_norm(w2), self.discriminate.bias, "id")


@stock_model
class SNGAN(nn.Module):
    """.G .D .z_dim .shape (+ the constructor arguments as attributes)."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20):
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = image_size, hidden_dim, z_dim
        self.G = Generator(image_size, hidden_dim, z_dim)
        self.D = Discriminator(image_size, hidden_dim, 1)
        self.shape = int(image_size ** 0.5)


def sngan_fused_ok(model):
    """True iff an SNGAN's shapes fit the spectral-norm kernels: H % 4 == 0, 4 <= H <= 1024 (the head's float4 lanes; u
    and W v in LDS), 1 <= I <= 8192 (W^T u in one workgroup's LDS), one critic output, equal hidden widths."""
    G, D = model.G, model.D
    H, I = D.linear.weight.shape
    Z = G.linear.weight.shape[1]
    return (4 <= H <= MAX_H and H % 4 == 0 and 1 <= I <= MAX_I and Z > 0
            and tuple(D.discriminate.weight.shape) == (1, H) and tuple(D.u.shape) == (H,)
            and tuple(G.linear.weight.shape) == (H, Z) and tuple(G.generate.weight.shape) == (I, H))


class SNGANEngine(TwoAdamRingEngine):
    """The fused path.  Batch rows and both steps' noise come from the sampler / randn protocol replayed on the host
    (draw_sampler_indices, normal_ on the global generator) into rings of `graph_iters` iterations, uploaded per chunk;
    whole iterations are captured as hipGraphs of `graph_iters` iterations (and of 1 for the tail), each launch reading
    its own ring row.  Step counters on the device address the Adam schedules and the loss slots.
    Per D step, 15 launches: gather_rows; G's two layers into the stacked [x; G(z)]; gm_sn_power_iter (3); the critic's
    hidden layer on the 2B rows with Wbar in W's place; gm_sn_head_fwd; gm_sn_head_bwd (rows + combine, gw2 and gb2 into
    D's flat gradient); the plain weight gradient G = dPre^T X into a scratch [H, I], its bias gradient straight into the
    flat buffer; gm_sn_grad (2); ONE flat Adam over D's four tensors; the tick.
    Per G step, 12: gm_sn_power_iter (3); G's two layers; the critic's hidden layer; the head's forward and backward in
    generator mode; dX through Wbar (sigmoid epilogue) and through G.generate (relu epilogue); G's paired weight
    gradients + Adam; the tick.  One GPU only."""

    fused_ok = staticmethod(sngan_fused_ok)

    def __init__(self, model, data, B, device, use_graph=True, world_size=1):
        if world_size > 1:
            raise GMError("the SN-GAN engine runs on one GPU: data parallelism is not implemented for it")
        if not sngan_fused_ok(model):
            raise GMError("SNGANEngine: shapes outside the spectral-norm kernels' limits (H %% 4 == 0, H <= 1024, "
                          "I <= 8192, equal hidden widths); SNGANTrainer trains these on the general path")
        self.model, self.data, self.B, self.dev, self.use_graph = model, data, B, device, use_graph
        G, D = model.G, model.D
        self.H, self.I = D.linear.weight.shape
        self.Z = G.linear.weight.shape[1]
        self.fG = FlatParams(list(G.parameters()), device)
        self.fD = FlatParams(list(D.parameters()), device)
        self.G1, self.G2 = _Linear(self.fG, G.linear), _Linear(self.fG, G.generate)
        self.D1, self.D2 = _Linear(self.fD, D.linear), _Linear(self.fD, D.discriminate)
        z = lambda *s: torch.zeros(*s, device=device)
        H, I = self.H, self.I
        self.X, self.Hg, self.Hd, self.dPre = z(2 * B, I), z(B, H), z(2 * B, H), z(2 * B, H)
        self.s, self.ds = z(2 * B), z(2 * B)
        self.dXg, self.dHg = z(B, I), z(B, H)
        self.Wbar, self.Gw, self.v, self.w2bar, self.stats = z(H, I), z(H, I), z(I), z(H), z(4)
        self.ws_p = ops_fused.sn_power_workspace(H, I, device)
        self.ws_h = ops_fused.sn_head_workspace(2 * B, H, device)
        self.ws_g = ops_fused.sn_grad_workspace(H, device)
        self.ctr = torch.zeros(2, dtype=torch.int64, device=device)      # D steps, G steps of this train() call

    # ---- one iteration's launches -------------------------------------------------------------------------------
    def _power(self, s, update_u=True):
        ops_fused.sn_power_iter(self.D1.W, self.u, self.v, self.Wbar, self.D2.W, self.w2bar, self.stats, self.ws_p,
                                update_u=update_u, stream=s)

    def _issue_D(self, s, k):
        """One critic step on ring row k."""
        B, G1, G2, D1, D2 = self.B, self.G1, self.G2, self.D1, self.D2
        sl = slot(self.ctr[0:1].data_ptr(), 1, 0, 0, 1)
        ops.gather_rows(self.data, self.idx[k], self.X[:B], stream=s)
        ops.linear_fwd(self.zD[k], G1.W, G1.b, self.Hg, "relu", stream=s)
        ops.linear_fwd(self.Hg, G2.W, G2.b, self.X[B:], "sigmoid", stream=s)
        self._power(s)
        ops.linear_fwd(self.X, self.Wbar, D1.b, self.Hd, "relu", stream=s)
        ops_fused.sn_head_fwd(self.Hd, self.w2bar, D2.b, B, False, self.s, self.ds, self.ws_h, loss_out=self.dloss,
                              loss_slot=sl, stream=s)
        ops_fused.sn_head_bwd(self.Hd, self.w2bar, B, False, self.ds, self.dPre, self.ws_h, stats=self.stats,
                              grads=(D2.gW, D2.gb), stream=s)
        ops.linear_bwd_dw(self.dPre, self.X, self.Gw, D1.gb, stream=s)
        ops_fused.sn_grad(self.Gw, self.Wbar, self.u, self.v, self.stats, D1.gW, self.ws_g, stream=s)
        fD = self.fD
        ops.adam(fD.flat, fD.grad, fD.m, fD.v, self.schedD, sched_slot=sl, betas=self.betas, stream=s)
        ops.tick(self.ctr[0:1], stream=s)

    def _issue_G(self, s, k, kd):
        """The generator step on noise row k (the critic's row kd is not read: the generator is unconditioned)."""
        B, G1, G2, D1, D2 = self.B, self.G1, self.G2, self.D1, self.D2
        sl = slot(self.ctr[1:2].data_ptr(), 1, 0, 0, 1)
        z, Xg, Hd, dPre = self.zG[k], self.X[B:], self.Hd[:B], self.dPre[:B]
        self._power(s)
        ops.linear_fwd(z, G1.W, G1.b, self.Hg, "relu", stream=s)
        ops.linear_fwd(self.Hg, G2.W, G2.b, Xg, "sigmoid", stream=s)
        ops.linear_fwd(Xg, self.Wbar, D1.b, Hd, "relu", stream=s)
        ops_fused.sn_head_fwd(Hd, self.w2bar, D2.b, B, True, self.s, self.ds, self.ws_h, loss_out=self.gloss,
                              loss_slot=sl, stream=s)
        ops_fused.sn_head_bwd(Hd, self.w2bar, B, True, self.ds, dPre, self.ws_h, stream=s)
        ops.linear_bwd_dx(dPre, self.Wbar, self.dXg, below=Xg, epi="sigmoid", stream=s)
        ops.linear_bwd_dx(self.dXg, G2.W, self.dHg, below=self.Hg, epi="relu", stream=s)
        adam = dict(sched=self.schedG, sched_slot=sl)
        ops.linear_bwd_dw_adam_pair(dict(dA=self.dXg, X=self.Hg, lin=G2, adam=adam),
                                    dict(dA=self.dHg, X=z, lin=G1, adam=adam), betas=self.betas, stream=s)
        ops.tick(self.ctr[1:2], stream=s)

    launches_per_iteration = staticmethod(lambda D_steps=1: 15 * D_steps + 12)

    # ---- run settings ---------------------------------------------------------------------------------------------
    def _configure_extra(self, betas):
        self.betas = (float(betas[0]), float(betas[1]))
        self.u = self.model.D.u                        # (load_state_dict keeps the buffer; .to() may have moved it)
        if not (self.u.is_cuda and self.u.is_contiguous() and self.u.dtype == torch.float32):
            raise GMError("SNGANEngine: D.u must be a contiguous float32 device buffer")
        return {"beta1": self.betas[0], "beta2": self.betas[1]}


@stock
class SNGANTrainer(GANTrainer):
    """ns_gan.py's Trainer surface for the SN-GAN: train(num_epochs, G_lr, D_lr, D_steps, betas), Glosses / Dlosses,
    sigma(); sample / generate_images / parzen / checkpoints are GANTrainer's (the generator is plain; the model's
    state_dict carries D.u)."""
    _STOCK = ("train_D", "train_G", "process_batch", "compute_noise")

    # ---- hooks (the general path) -------------------------------------------------------------------------------
    def train_D(self, images):
        """The contract's D_loss: one critic forward on the stacked [x; G(z)]."""
        m = self.model
        b = images.shape[0]
        fake = m.G(self.compute_noise(b, m.z_dim)).detach()
        s = m.D(torch.cat([images, fake]))
        return torch.mean(torch.relu(1 - s[:b])) + torch.mean(torch.relu(1 + s[b:]))

    def train_G(self, images):
        """The contract's G_loss."""
        m = self.model
        return -torch.mean(m.D(m.G(self.compute_noise(images.shape[0], m.z_dim))))

    # ---- path selection ---------------------------------------------------------------------------------------
    def _stock(self):
        if not self._stock_prefix():
            return False
        m = self.model
        G, D = getattr(m, "G", None), getattr(m, "D", None)
        if not (type(G) is Generator and type(D) is Discriminator and _stock_module(G, 2) and _stock_module(D, 2)):
            return False                               # edited / subclassed networks: general path
        if not sngan_fused_ok(m):
            return False                               # outside the kernels' limits: general path
        return reference_loader_ok(self.train_iter)

    def _make_engine(self, data, loader, dev):
        return SNGANEngine(self.model, data, loader.batch_size, dev, use_graph=self.use_graph)

    # ---- the loop -------------------------------------------------------------------------------------------------
    def train(self, num_epochs, G_lr=1e-4, D_lr=4e-4, D_steps=1, betas=(0.0, 0.9)):
        """ns_gan.py:94 with SAGAN's two time scales and Adam betas."""
        from . import dp
        if dp.current()[0] > 1:
            raise GMError("SNGANTrainer runs on one GPU: data parallelism is not implemented for it")
        epoch_steps = int(np.ceil(len(self.train_iter) / D_steps))
        if self._stock():
            eng = self._get_engine()
            eng.use_graph = self.use_graph
            eng.configure(num_epochs * epoch_steps, G_lr, D_lr, D_steps, betas=betas,
                          resume=self.__dict__.pop("_resume_optim", None))
            for epoch in range(1, num_epochs + 1):
                self.model.train()
                it0 = (epoch - 1) * epoch_steps
                eng.run(epoch_steps)
                G_losses, D_losses = eng.losses(it0, it0 + epoch_steps)
                self._end_epoch(epoch, num_epochs, G_losses, D_losses)
                self._viz_epoch(epoch)
            return
        # GENERAL path: the hooks over autograd, the reference's loop
        if self.__dict__.get("_resume_optim") is not None:
            raise GMError("load_checkpoint() restored optimizer state, but this trainer runs the general path "
                          "(overridden hooks / edited networks), whose optimizers start fresh")
        m = self.model
        G_opt = FlatAdam(m.G.parameters(), G_lr, betas=betas)
        D_opt = FlatAdam(m.D.parameters(), D_lr, betas=betas)
        for epoch in range(1, num_epochs + 1):
            m.train()
            G_losses, D_losses = [], []
            for _ in range(epoch_steps):
                step = []
                for _ in range(D_steps):
                    images = self.process_batch(self.train_iter)
                    D_opt.zero_grad()
                    D_loss = self.train_D(images)
                    D_loss.backward()
                    D_opt.step()
                    step.append(D_loss.item())
                D_losses.append(np.mean(step))
                G_opt.zero_grad()
                G_loss = self.train_G(images)
                G_losses.append(G_loss.item())
                G_loss.backward()
                G_opt.step()
            self._end_epoch(epoch, num_epochs, G_losses, D_losses)
            self._viz_epoch(epoch)

    def sigma(self, exact=False):
        """The spectral norm of D.linear.weight: the running estimate u^T W v with v = normalize(W^T u) from the stored
        u (what an eval-mode forward divides by; never above the true value), or with exact=True the largest singular
        value by torch.linalg.svdvals on the host.  Draws nothing and leaves u as it is."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        D = self.model.D
        W = D.linear.weight.detach().cpu().double()
        if exact:
            return float(torch.linalg.svdvals(W)[0])
        u = D.u.detach().cpu().double()
        v = F.normalize(W.t() @ u, dim=0, eps=NORM_EPS)
        return float(u @ (W @ v))


__all__ = ["Generator", "Discriminator", "SNGAN", "SNGANTrainer", "SNGANEngine", "sngan_fused_ok", "FlatAdam"]
