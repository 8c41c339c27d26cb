"""Primal-Dual Wasserstein GAN (Gemici, Akata, Welling 2018, arXiv 1805.09575; the last model of the reference's README
to-do list that fits its MLPs, README.md:95): an encoder E, a decoder / generator G and a critic D.  The primal couples
every image with its own reconstruction; the dual's gradient penalty runs on the interpolates between the two and
pushes the critic's input gradient there towards the unit vector from the reconstruction to the image -- norm AND
direction, where WGAN-GP asks for norm 1 only.  Exported by src/pdw_gan.py as PDWGAN / PDWGANTrainer.

Each batch x (b rows) runs three phases in this order, one Adam step each (E_lr, D_lr, G_lr; default betas and eps);
every draw comes from the global CPU generator in the order numbered here:
  1. primal (compute_batch): z = E(x), x~ = G(z), n_b = ||x_b - x~_b||, d_b = (x_b - x~_b) / n_b (0 where n_b == 0);
     (1) p = torch.randn(b, Z); L_E = mean_b n_b + lambda_z * mmd(z, p) (bir_vae.py:201-221: sums of kernel values);
     the gradient runs through G into E only; Adam(E).
  2. dual (train_D): x~ and d of phase 1, detached (the encoder BEFORE its step); (2) t = torch.rand(b, 1),
     x^ = t x + (1 - t) x~; (3) z_c = torch.randn(b, Z);
     L_D = mean D(G(z_c)) - mean D(x) + lambda_gp * mean_b ||grad_x^ D(x^_b) - d_b||^2; Adam(D).
  3. generator (train_G): (4) z_g = torch.randn(b, Z); L_G = -mean D(G(z_g)) with the stepped critic; Adam(G).
Validation is mean_b n_b and draws nothing.  Fused path: PDWGANEngine below; anything overridden or edited, or shapes
outside the fused kernels' limits: autograd over ops.fused_linear + three FlatAdams in the same order."""
import numpy as np
import torch
import torch.nn as nn

from . import ops
from ._lib import GMError
from .aae import Encoder
from .trainers import (CriticReLU, FlatAdam, Generator, VAETrainer, _decode_rows, _epoch_order, _stock_module, stock,
                       stock_model, to_cuda)
from .engine import VAEEngine               # (engine first: it imports vae_engine's classes)

HISTORY = ("Elosses", "Dlosses", "Glosses", "num_epochs", "best_val_loss")
OPTIM_FIELDS = ("m", "v", "step", "config", "steps")
# lambda_z: BIR-VAE's weight on the same MMD, moved to this loss's scale.  bir_vae.py adds 1000 * mmd to a
# reconstruction SUM over the reference's batch of 100 rows; L_E holds the reconstruction MEAN, so the same balance
# per row is 1000 / 100.
LAMBDA_Z = 10.0


@stock_model
class PDWGAN(nn.Module):
    """.E (aae.Encoder: I -> H relu, H -> Z), .G (Generator: Z -> H relu, H -> I sigmoid), .D (CriticReLU: I -> H
    relu, H -> 1 relu), built in this order; forward(x) is the reconstruction G(E(x))."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20):
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = image_size, hidden_dim, z_dim
        self.E = Encoder(image_size, hidden_dim, z_dim)
        self.G = Generator(image_size, hidden_dim, z_dim)
        self.D = CriticReLU(image_size, hidden_dim, 1)
        self.shape = int(image_size ** 0.5)

    def forward(self, x):
        return self.G(self.E(x))


def pdw_fused_ok(model):
    """True iff a PDWGAN's shapes fit the fused batch: 1 <= Z <= 32 with Z % 4 == 0, hidden width <= 512, the
    generator's and the critic's hidden widths equal to the encoder's, one critic output (the AAE's limits)."""
    E, G, D = model.E, model.G, model.D
    Z, H = E.z.weight.shape
    I = E.linear.weight.shape[1]
    return (0 < Z <= 32 and Z % 4 == 0 and 0 < H <= 512 and tuple(E.linear.weight.shape) == (H, I)
            and tuple(G.linear.weight.shape) == (H, Z) and tuple(G.generate.weight.shape) == (I, H)
            and tuple(D.linear.weight.shape) == (H, I) and tuple(D.discriminate.weight.shape) == (1, H))


def host_draws(dst, sizes, B, Z):
    """The contract's four draws for each batch of a chunk, in order, on the global CPU generator: dst["prior"][k]
    (randn(b, Z)), dst["t"][k] (rand(b, 1)), dst["zc"][k], dst["zg"][k] (randn(b, Z)) for batch k of sizes[k] rows.
    dst: contiguous fp32 CPU tensors [>= len(sizes), B, Z] / [>= len(sizes), B].  Full batches go through the C replay
    of the draw program where it is available (engine.HostReplay), everything else through torch itself."""
    from ._lib import DRAW_NORMAL, DRAW_UNIFORM
    from .engine import HostReplay

    def program(b, k, stride):
        bz = b * Z
        return [HostReplay.op(DRAW_NORMAL, bz, dst["prior"][k], stride * Z * 4),
                HostReplay.op(DRAW_UNIFORM, b, dst["t"][k], stride * 4),
                HostReplay.op(DRAW_NORMAL, bz, dst["zc"][k], stride * Z * 4),
                HostReplay.op(DRAW_NORMAL, bz, dst["zg"][k], stride * Z * 4)]
    nfull = 0
    while nfull < len(sizes) and sizes[nfull] == B:
        nfull += 1
    start = 0
    if nfull and B >= 16 and HostReplay.available() and HostReplay.run(program(B, 0, B), nfull):
        start = nfull
    for k in range(start, len(sizes)):
        b = sizes[k]
        if b >= 16 and HostReplay.available() and HostReplay.run(program(b, k, 0), 1):
            continue
        dst["prior"][k].view(-1)[:b * Z].normal_()
        dst["t"][k].view(-1)[:b].uniform_()
        dst["zc"][k].view(-1)[:b * Z].normal_()
        dst["zg"][k].view(-1)[:b * Z].normal_()


class PDWGANEngine(VAEEngine):
    """One PD-WGAN batch on the VAE engine's machinery (rings, host draws, multi-batch hipGraphs, ragged last batch):
    one FlatParams over the 12 tensors, three disjoint Adam segments (E, G, D) with three schedules on the device
    step counter.  26 launches per training batch (27 for a graph's first batch, which gathers its own rows):
      1. primal, 10: E forward x 2 (the second carries the next batch's gather), G forward x 2, gm_pdw_couple (n,
         the loss share, d L_E / d pre-sigmoid x~, x^ and the copy of x into the critic's stacked input), gm_bir_mmd,
         dX x 3 (through G into E), E's paired weight gradients + Adam(E);
      2. dual, 9: G(z_c) x 2 into the stacked input [x^ ; x ; G(z_c)], the critic's hidden layer on its 3b rows,
         gm_head_gp, g = u W1, gm_pdw_dir (in gm_gp_norm's place; gamma over the consumed x^ rows), t = gamma W1^T,
         the head's forward + loss, the stacked dW1 = [u ; dH]^T [gamma ; x ; G(z_c)] with the head's backward, the
         penalty's share of gw2 and both Adam(D) steps;
      3. generator, 7: G(z_g) x 2, the critic's hidden layer, the head in generator mode, dX through D (carrying the
         loss scalar), dX through G's output layer, G's paired weight gradients + Adam(G) with the loss sums of
         phase 1 and the counter tick.
    One GPU only; the fused shapes only (pdw_fused_ok) -- the trainer takes the general path outside them."""

    has_eps = False
    fused_ok = staticmethod(pdw_fused_ok)

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False):
        if world_size > 1 or force_dp:
            raise GMError("the PD-WGAN engine runs on one GPU: data parallelism is not implemented for it")
        if not pdw_fused_ok(model):
            raise GMError("PDWGANEngine: shapes outside the fused kernels' limits (Z <= 32, Z % 4 == 0, H <= 512, equal "
                          "hidden widths); PDWGANTrainer trains these on the general path")
        from .engine import FlatParams, _Linear
        self.model, self.device, self.use_graph = model, device, use_graph
        E, G, D = model.E, model.G, model.D
        plist = [E.linear.weight, E.linear.bias, E.z.weight, E.z.bias,
                 G.linear.weight, G.linear.bias, G.generate.weight, G.generate.bias,
                 D.linear.weight, D.linear.bias, D.discriminate.weight, D.discriminate.bias]
        self._dp_init(plist, 1, 0, None, False)
        self.fp = FlatParams(plist, device)
        fp = self.fp
        self.E1, self.EZ = _Linear(fp, E.linear), _Linear(fp, E.z)
        self.G1, self.G2 = _Linear(fp, G.linear), _Linear(fp, G.generate)
        self.C1, self.C2 = _Linear(fp, D.linear), _Linear(fp, D.discriminate)
        self.Z, self.H = E.z.weight.shape
        self.I = E.linear.weight.shape[1]
        self._drawing = True
        self._common_init(device)

    def phase_grads(self):
        """The three phases' gradients of the last training batch: {"e": 4 tensors, "d": 4, "g": 4}, keyed by the
        model's state_dict names (views of the flat gradient buffer's three segments)."""
        names = {id(p): n for n, p in self.model.named_parameters()}
        out = {"e": {}, "d": {}, "g": {}}
        for p, gv in zip(self.fp.params, self.fp.gviews):
            n = names[id(p)]
            out[n[0].lower()][n] = gv
        return out

    def _alloc(self, B):
        if self._bufB == B:
            return
        dev, I, H, Z = self.device, self.I, self.H, self.Z
        z = lambda *s: torch.zeros(*s, device=dev)
        # primal
        self.X, self.He, self.Zs = z(B, I), z(B, H), z(B, Z)
        self.Xb = (self.X, z(B, I))
        self.Hdec, self.Xr, self.dA = z(B, H), z(B, I), z(B, I)
        self.dHdec, self.dZ, self.dZm, self.dHe = z(B, H), z(B, Z), z(B, Z), z(B, H)
        self.nrm, self.part, self.partm = z(B), z(B), z(B)
        # dual: row blocks of b rows each (b = the batch at hand, the ragged one included), x^ / gamma first
        self.XX3, self.HH3, self.DU = z(3 * B, I), z(3 * B, H), z(3 * B, H)
        self.Hc, self.Sh, self.Gr, self.T, self.pen = z(B, H), z(B), z(B, I), z(B, H), z(B)
        self.S2, self.dS, self.rowloss = z(2 * B), z(2 * B), z(2 * B)
        # generator
        self.Hg, self.Xg, self.Hd3, self.dHd3 = z(B, H), z(B, I), z(B, H), z(B, H)
        self.S3, self.dS3, self.rowloss3 = z(B), z(B), z(B)
        self.dXg, self.dHg = z(B, I), z(B, H)
        self._bufB = B
        self.graphs = {}

    def configure(self, B, n_train_steps, E_lr, G_lr=1e-4, D_lr=1e-4, lambda_z=LAMBDA_Z, lambda_gp=10.0, resume=None):
        # (compared with a checkpoint's settings by VAEEngine.configure, like its own; as settings they are part of
        # the graphs' key too, so a train() call with other learning rates captures its graphs anew)
        self._run_settings = {"G_lr": float(G_lr), "D_lr": float(D_lr), "lambda_z": float(lambda_z),
                              "lambda_gp": float(lambda_gp)}
        from .engine import GANEngine
        super().configure(B, n_train_steps, E_lr, 0.0, resume=resume)
        self.lambda_z, self.lambda_gp = float(lambda_z), float(lambda_gp)
        n = max(1, n_train_steps)
        self.sched_G = GANEngine._pbuf(self, "sched_G", ops.adam_schedule(G_lr, n, start=self.step0 + 1))
        self.sched_D = GANEngine._pbuf(self, "sched_D", ops.adam_schedule(D_lr, n, start=self.step0 + 1))
        self.dloss = GANEngine._pbuf(self, "dloss", n)
        self.gloss = GANEngine._pbuf(self, "gloss", n)
        if getattr(self, "_draw_B", None) != B or "prior" not in self.stage[0]:
            R, Z, dev = self.R, self.Z, self.device
            self.prior_ring, self.zc_ring, self.zg_ring = (torch.zeros(R, B, Z, device=dev) for _ in range(3))
            self.t_ring = torch.zeros(R, B, device=dev)
            for s in self.stage:
                for k in ("prior", "zc", "zg"):
                    s[k] = torch.zeros(R, B, Z).pin_memory()
                s["t"] = torch.zeros(R, B).pin_memory()
            self._draw_B = B
            self._moved = True
        lam = (self.lambda_z, self.lambda_gp)              # launch arguments of the captured graphs
        if self._moved or getattr(self, "_lam_key", None) != lam:
            self.graphs = {}
        self._lam_key = lam

    def _settings(self):
        return self._run_settings

    def optim_state(self):
        st = super().optim_state()
        # one Adam step per batch for each of the three optimizers (their moments: the three segments of m / v)
        st.update(steps={"E": st["step"], "D": st["step"], "G": st["step"]})
        return st

    def run_pass(self, data, perm, train, t0):
        self._drawing = bool(train)                  # validation draws nothing
        return super().run_pass(data, perm, train, t0)

    def _draw_chunk(self, s, sizes):
        if self._drawing:
            host_draws(s, sizes, self.B, self.Z)

    def _upload_chunk(self, s, r, cnt):
        if self._drawing:
            for k, ring in (("prior", self.prior_ring), ("t", self.t_ring), ("zc", self.zc_ring),
                            ("zg", self.zg_ring)):
                ring[r:r + cnt].copy_(s[k][:cnt], non_blocking=True)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: the primal's forward (+ when training: its backward + Adam(E), the dual step, the
        generator step)."""
        from . import ops_fused as of_
        R, B, Z = self.R, self.B, self.Z
        E1, EZ, G1, G2, C1, C2 = self.E1, self.EZ, self.G1, self.G2, self.C1, self.C2
        idx_slot = self._slot(t, 1, 0, R, B)
        z_slot = self._slot(t, 1, 0, R, B * Z)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        tick = self.ctr if self.use_graph else None
        inv_b = float(np.float32(1.0) / np.float32(b))
        X, own, nxt = self._gather_plan(pos, of)
        if own:
            ops.gather_rows(self.data, self.idx_ring.view(-1), X, B=b, idx_slot=idx_slot, stream=st)
        # ---- 1. primal: x~ = G(E(x)), L_E = mean ||x - x~|| + lambda_z mmd(z), Adam(E)
        ops.linear_fwd(X, E1.W, E1.b, self.He, "relu", M=b, stream=st)
        self._fwd_with_prefetch(st, t, 0, b, self.He, EZ, self.Zs, "id", nxt)
        ops.linear_fwd(self.Zs, G1.W, G1.b, self.Hdec, "relu", M=b, stream=st)
        ops.linear_fwd(self.Hdec, G2.W, G2.b, self.Xr, "sigmoid", M=b, stream=st)
        if not train:
            of_.pdw_couple(X, self.Xr, self.part, b, inv_b=inv_b, stream=st)
            of_.sum_finalize(self.part, b, self.vrecon, out_slot=loss_slot, tick=tick, stream=st)
            return
        Xh, Xc, Xf = self.XX3[:b], self.XX3[b:2 * b], self.XX3[2 * b:3 * b]      # [x^ (later gamma) ; x ; G(z_c)]
        of_.pdw_couple(X, self.Xr, self.part, b, inv_b=inv_b, n=self.nrm, t=self.t_ring.view(-1),
                       t_slot=self._slot(t, 1, 0, R, B), dA=self.dA, xhat=Xh, xcopy=Xc, stream=st)
        of_.bir_mmd(self.Zs, self.prior_ring.view(-1), self.partm, self.dZm, b, Z, self.lambda_z, prior_slot=z_slot,
                    stream=st)
        sched_slot = self._slot(t, 1, 0, 0, 1)
        # (every dX reads a layer's weights; G's are not stepped before phase 3, E's by this phase's last launch)
        ops.linear_bwd_dx(self.dA, G2.W, self.dHdec, below=self.Hdec, epi="relu", M=b, stream=st)
        ops.linear_bwd_dx(self.dHdec, G1.W, self.dZ, M=b, add=self.dZm, add_scale=1.0, stream=st)
        ops.linear_bwd_dx(self.dZ, EZ.W, self.dHe, below=self.He, epi="relu", M=b, stream=st)
        eadam = dict(sched=self.sched, sched_slot=sched_slot)
        ops.linear_bwd_dw_adam_pair(dict(dA=self.dHe, X=X, lin=E1, adam=eadam, M=b),
                                    dict(dA=self.dZ, X=self.He, lin=EZ, adam=eadam, M=b), stream=st)
        # ---- 2. dual: the critic on [x^ ; x ; G(z_c)], the direction penalty's second backward, Adam(D)
        zc = self.zc_ring.view(-1, Z)
        ops.linear_fwd(zc, G1.W, G1.b, self.Hc, "relu", M=b, x_slot=z_slot, stream=st)
        ops.linear_fwd(self.Hc, G2.W, G2.b, Xf, "sigmoid", M=b, stream=st)
        ops.linear_fwd(self.XX3, C1.W, C1.b, self.HH3, "relu", M=3 * b, stream=st)
        Hh, Hd = self.HH3[:b], self.HH3[b:3 * b]
        U, dHd = self.DU[:b], self.DU[b:3 * b]
        Sh, Gr, T, pen = self.Sh[:b], self.Gr[:b], self.T[:b], self.pen[:b]
        of_.head_gp(Hh, C2.W, C2.b, Sh, U, stream=st)                          # D(x^) and the seed u
        ops.linear_bwd_dx(U, C1.W, Gr, M=b, stream=st)                         # g = u W1
        Gam = Xh                                                               # x^ is consumed: gamma takes its rows
        of_.pdw_dir(Gr, X, self.Xr, self.nrm, Gam, pen, self.lambda_gp, inv_b, stream=st)
        ops.linear_fwd(Gam, C1.W, None, T, "id", M=b, stream=st)               # t = gamma W1^T, before W1 is stepped
        hyper = (0.0,) * 7 + (self.lambda_gp,)
        of_.head_fwd_loss("w", False, Hd, C2.W, C2.b, "relu", b, hyper, inv_b, pen, self.S2, self.dS, self.rowloss,
                          dH=dHd, stream=st)
        dadam = dict(sched=self.sched_D, sched_slot=sched_slot)
        head = dict(H=Hd, dS=self.dS, lin=C2, rowloss=self.rowloss, loss_out=self.dloss, loss_slot=loss_slot,
                    inv_b=inv_b, B=b, adam=dadam, pen=dict(s=Sh, h=Hh, t=T))
        ops.linear_bwd_dw_adam_head(self.DU, self.XX3, C1, dadam, head, M=3 * b, ones_from=b, stream=st)
        # ---- 3. generator: -mean D(G(z_g)) through the stepped critic, Adam(G)
        zg = self.zg_ring.view(-1, Z)
        ops.linear_fwd(zg, G1.W, G1.b, self.Hg, "relu", M=b, x_slot=z_slot, stream=st)
        ops.linear_fwd(self.Hg, G2.W, G2.b, self.Xg, "sigmoid", M=b, stream=st)
        ops.linear_fwd(self.Xg, C1.W, C1.b, self.Hd3, "relu", M=b, stream=st)
        of_.head_fwd_loss("w", True, self.Hd3, C2.W, C2.b, "relu", b, (), inv_b, None, self.S3, self.dS3,
                          self.rowloss3, dH=self.dHd3, stream=st)
        ops.linear_bwd_dx_head(self.dHd3, C1.W, self.dXg,
                               dict(H=self.Hd3, dS=self.dS3, lin=C2, rowloss=self.rowloss3, loss_out=self.gloss,
                                    loss_slot=loss_slot, inv_b=inv_b, B=b, gen_mode=True, tick=None),
                               below=self.Xg, epi="sigmoid", M=b, stream=st)
        ops.linear_bwd_dx(self.dXg, G2.W, self.dHg, below=self.Hg, epi="relu", M=b, stream=st)
        gadam = dict(sched=self.sched_G, sched_slot=sched_slot)
        # the batch's LAST launch: G's weight gradients + Adam(G), phase 1's two loss sums, the counter tick
        ops.linear_bwd_dw_adam_pair_finalize(
            dict(dA=self.dXg, X=self.Hg, lin=G2, adam=gadam, M=b),
            dict(dA=self.dHg, X=zg, lin=G1, adam=gadam, M=b, x_slot=z_slot),
            dict(pa=self.part, na=b, out_a=self.recon, slot_a=loss_slot, pb=self.partm, nb=b,
                 scale_b=self.lambda_z, out_b=self.kl, slot_b=loss_slot, done=self.fin_done, tick=tick),
            stream=st)


@stock
class PDWGANTrainer(VAETrainer):
    """The three-phase loop above with the AAE trainer's protocol: next(iter(test_iter)) at construction, the
    sampler's permutation per pass, best_model / best_val_loss on the validation mean ||x - x~||, viz=True adds one
    randn(36, z_dim) per epoch (generate_images)."""
    _gm_stock_class = True
    _hook_names = ("compute_batch", "train_D", "train_G", "evaluate")

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False):
        self.model = to_cuda(model)
        self.name = model.__class__.__name__
        self.train_iter, self.val_iter, self.test_iter = train_iter, val_iter, test_iter
        self.best_val_loss = 1e10
        self.debugging_image, _ = next(iter(test_iter))          # (consumes RNG, as every VAE-family trainer)
        self.viz = viz
        self.Elosses, self.Dlosses, self.Glosses = [], [], []
        self.num_epochs = 0
        self.lambda_z, self.lambda_gp = LAMBDA_Z, 10.0
        self._coupling = None
        self._engine = None
        self.use_graph = True

    # ---- reference-style hooks (the general path) -----------------------------------------------------------
    def compute_kernel(self, x, y):
        """bir_vae.py:210-221."""
        x_size, y_size, dim = x.size(0), y.size(0), x.size(1)
        tx = x.unsqueeze(1).expand(x_size, y_size, dim)
        ty = y.unsqueeze(0).expand(x_size, y_size, dim)
        return torch.exp(-torch.div(torch.mean(torch.pow(tx - ty, 2), dim=2), dim))

    def maximum_mean_discrepancy(self, z, prior):
        """bir_vae.py:201-208 against the given prior rows."""
        return self.compute_kernel(prior, prior).sum() + self.compute_kernel(z, z).sum() \
            - 2 * self.compute_kernel(prior, z).sum()

    def _couple(self, images):
        """(x~, n, d) of the primal coupling; d = 0 on a row the reconstruction hits exactly."""
        recon = self.model(images)
        diff = images - recon
        n = diff.norm(2, dim=1)
        d = torch.where(n.unsqueeze(1) > 0, diff / n.unsqueeze(1).clamp_min(1e-38), torch.zeros_like(diff))
        return recon, n, d

    def compute_batch(self, batch):
        """Primal phase: mean_b ||x_b - G(E(x_b))|| + lambda_z * mmd(E(x), randn(b, Z)); leaves the coupling
        (x~, d), detached, for train_D."""
        images, _ = batch
        images = to_cuda(images.view(images.shape[0], -1))
        m = self.model
        z = m.E(images)
        recon = m.G(z)
        diff = images - recon
        n = diff.norm(2, dim=1)
        prior = to_cuda(torch.randn(images.shape[0], m.z_dim))
        nd = n.detach().unsqueeze(1)
        d = torch.where(nd > 0, diff.detach() / nd.clamp_min(1e-38), torch.zeros_like(nd))
        self._coupling = (recon.detach(), d)
        return torch.mean(n) + self.lambda_z * self.maximum_mean_discrepancy(z, prior)

    def train_D(self, images):
        """Dual phase: the Wasserstein critic loss + lambda_gp * mean ||grad D(x^) - d||^2 on the interpolates between
        the images and their phase-1 reconstructions."""
        m = self.model
        if self._coupling is None or self._coupling[0].shape != images.shape:
            with torch.no_grad():
                recon, _, d = self._couple(images)
            self._coupling = (recon, d)
        recon, d = self._coupling
        t = to_cuda(torch.rand(images.shape[0], 1))
        x_hat = (t * images + (1 - t) * recon).requires_grad_(True)
        g_out = m.G(to_cuda(torch.randn(images.shape[0], m.z_dim))).detach()
        sg, sx = m.D(g_out), m.D(images)
        d_hat = m.D(x_hat)
        grads = torch.autograd.grad(outputs=d_hat, inputs=x_hat, grad_outputs=torch.ones_like(d_hat),
                                    create_graph=True, retain_graph=True, only_inputs=True)[0]
        pen = torch.mean(torch.sum((grads - d) ** 2, dim=1))
        return torch.mean(sg) - torch.mean(sx) + self.lambda_gp * pen

    def train_G(self, images):
        """Generator phase: -mean D(G(z_g)), z_g = randn(b, Z)."""
        m = self.model
        return -torch.mean(m.D(m.G(to_cuda(torch.randn(images.shape[0], m.z_dim)))))

    def evaluate(self, iterator):
        """Mean over the iterator's batches of mean_b ||x_b - G(E(x_b))|| (draws nothing beyond the loader's
        permutation)."""
        out = []
        with torch.no_grad():
            for images, _ in iterator:
                images = to_cuda(images.view(images.shape[0], -1))
                out.append(self._couple(images)[1].mean().item())
        return np.mean(out)

    def compute_noise(self, batch_size, z_dim):
        return to_cuda(torch.randn(batch_size, z_dim))

    # ---- path selection -----------------------------------------------------------------------------------------
    def _stock(self):
        if not self._hooks_stock():
            return False
        m = self.model
        if not type(m).__dict__.get("_gm_stock_model", False):
            return False                               # a subclass may have changed forward
        E, G, D = (getattr(m, n, None) for n in ("E", "G", "D"))
        if not (type(E) is Encoder and type(G) is Generator and type(D) is CriticReLU
                and all(_stock_module(x, 2) for x in (E, G, D))):
            return False                               # edited / subclassed networks: general path
        if not pdw_fused_ok(m):
            return False                               # outside the fused kernels' limits: general path
        return (self._loader_ok(self.train_iter) and self._loader_ok(self.val_iter)
                and self.train_iter.batch_size == self.val_iter.batch_size)

    def _engine_class(self):
        return PDWGANEngine

    def train(self, num_epochs, E_lr=1e-4, G_lr=1e-4, D_lr=1e-4, lambda_z=LAMBDA_Z, lambda_gp=10.0, quiet=False):
        """num_epochs passes of the three-phase loop: one Adam step of E, D and G per batch (E_lr / D_lr / G_lr);
        lambda_z weighs the latent MMD in the encoder's loss, lambda_gp the direction penalty in the critic's."""
        from copy import deepcopy
        from . import dp
        if dp.current()[0] > 1:
            raise GMError("PDWGANTrainer runs on one GPU: data parallelism is not implemented for it")
        self.lambda_z, self.lambda_gp = float(lambda_z), float(lambda_gp)
        if self._stock():
            if not torch.cuda.is_available():
                raise GMError("no MI355X visible: the fused step engine has no CPU fallback")
            if self._engine is None:
                self._engine = self._engine_class()(self.model, next(self.model.parameters()).device,
                                                    use_graph=self.use_graph)
            eng = self._engine
            eng.use_graph = self.use_graph
            steps = len(self.train_iter)
            eng.configure(self.train_iter.batch_size, num_epochs * steps, E_lr, G_lr=G_lr, D_lr=D_lr,
                          lambda_z=lambda_z, lambda_gp=lambda_gp, resume=self.__dict__.pop("_resume_optim", None))
            tdata, vdata = self._device_data(self.train_iter), self._device_data(self.val_iter)
            nval = len(self.val_iter)
            eng.alloc_val(nval)
            for epoch in range(1, num_epochs + 1):
                self.model.train()
                t0 = (epoch - 1) * steps
                eng.run_pass(tdata, _epoch_order(self.train_iter), True, t0)
                self.model.eval()
                eng.run_pass(vdata, _epoch_order(self.val_iter), False, 0)
                rec, mmd = eng.read_losses(eng.recon, t0, steps), eng.read_losses(eng.kl, t0, steps)     # one sync
                e = [float(a) + float(b) for a, b in zip(rec, mmd)]
                d = [float(x) for x in eng.read_losses(eng.dloss, t0, steps)]
                g = [float(x) for x in eng.read_losses(eng.gloss, t0, steps)]
                val_loss = np.mean([float(x) for x in eng.read_losses(eng.vrecon, 0, nval)])
                self._end_epoch_pdw(epoch, num_epochs, e, d, g, val_loss, deepcopy, quiet)
            return
        # GENERAL path: the three phases over autograd, three optimizers
        m = self.model
        e_opt, d_opt, g_opt = FlatAdam(m.E.parameters(), E_lr), FlatAdam(m.D.parameters(), D_lr), \
            FlatAdam(m.G.parameters(), G_lr)
        for epoch in range(1, num_epochs + 1):
            self.model.train()
            e, d, g = [], [], []
            for batch in self.train_iter:
                images = to_cuda(batch[0].view(batch[0].shape[0], -1))
                e_opt.zero_grad()
                el = self.compute_batch(batch)
                el.backward()
                e_opt.step()
                d_opt.zero_grad()
                dl = self.train_D(images)
                dl.backward()
                d_opt.step()
                g_opt.zero_grad()
                gl = self.train_G(images)
                gl.backward()
                g_opt.step()
                self._coupling = None
                e.append(el.item()); d.append(dl.item()); g.append(gl.item())
            self.model.eval()
            val_loss = self.evaluate(self.val_iter)
            self._end_epoch_pdw(epoch, num_epochs, e, d, g, val_loss, deepcopy, quiet)

    def _end_epoch_pdw(self, epoch, num_epochs, e, d, g, val_loss, deepcopy, quiet):
        self.Elosses.extend(e)
        self.Dlosses.extend(d)
        self.Glosses.extend(g)
        if val_loss < self.best_val_loss:
            self.best_model = deepcopy(self.model)
            self.best_val_loss = val_loss
        if not quiet:
            print("Epoch[%d/%d], E Loss: %.4f, D Loss: %.4f, G Loss: %.4f, Val Loss: %.4f"
                  % (epoch, num_epochs, np.mean(e), np.mean(d), np.mean(g), val_loss))
        self.num_epochs += 1
        self._viz_epoch(epoch)

    # ---- sampling, reconstruction, evaluation, pictures -----------------------------------------------------------
    def _viz_epoch(self, epoch):
        if self.viz:
            self.generate_images(epoch)              # one randn(36, z_dim) from the global generator

    def sample(self, n, seed=0):
        """n generated samples [n, image_size]: z ~ N(0, I) from torch.Generator().manual_seed(seed) through model.G;
        the global generator and the model's mode are untouched."""
        gen = torch.Generator().manual_seed(int(seed))
        return _decode_rows(self.model.G, torch.randn(int(n), self.model.z_dim, generator=gen))

    def reconstruct(self, images):
        """G(E(images)) as [n, image_size] (images: [n, ...] on any device); no autograd, no RNG use."""
        x = images.reshape(images.shape[0], -1).to(torch.float32)
        return _decode_rows(self.model, x)

    def generate_images(self, epoch, num_outputs=36, save=True):
        from . import viz
        return viz.generate_images(self, epoch, num_outputs, save, self.viz_dir)

    def viz_loss(self):
        from . import viz
        viz.viz_loss(self)

    def save_checkpoint(self, savepath, collective=True):
        """Weights, the three optimizers' moments and step counts, the RNG cursor and the histories (a finished
        train() call on the fused engine)."""
        from .trainers import _save_checkpoint
        _save_checkpoint(self, savepath, tuple(n for n in HISTORY if hasattr(self, n)), collective=collective)


__all__ = ["PDWGAN", "PDWGANTrainer", "PDWGANEngine"]
