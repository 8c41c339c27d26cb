"""Auxiliary-classifier GAN (Odena, Olah & Shlens 2017, arXiv 1610.09585): ns_gan.py's model and loop with the class
label fed to the generator's first layer and a second, C-way head on the critic -- the GAN family's counterpart of the
CVAE.  Exported by src/ac_gan.py as Generator / Discriminator / ACGAN / ACGANTrainer.

The contract:
  * Generator: `linear` (Z -> H), `label` (nn.Linear(C, H, bias=False), the split form of cvae.py), `generate`
    (H -> I); forward(z, y) = sigmoid(generate(relu(linear(z) + label.weight[:, y]))).
  * Discriminator: `linear` (I -> H), `discriminate` (H -> 1), `classify` (H -> C); forward(x) =
    (sigmoid(discriminate(h)), classify(h)) with h = relu(linear(x)): s(x) and c(x) below.
  * Loop and RNG: ns_gan.py:94-170 exactly.  process_batch is next(iter(train_iter)) and keeps the labels;
    compute_noise is torch.randn(B, Z) on the global CPU generator, once in train_D and once in train_G; a run leaves
    the global generator where an NSGANTrainer run of the same length leaves it.
  * Fake rows take the class of the batch in hand: G(z, y) with y the real batch's labels, in both steps; train_G
    reuses the last train_D batch.  No label is drawn.
  * D_loss = -mean(log(s(x) + 1e-8) + log(1 - s(G(z, y)) + 1e-8)) + class_weight (CE(c(x), y) + CE(c(G(z, y)), y)),
    G(z, y) detached;  G_loss = -mean(log(s(G(z', y)) + 1e-8)) + class_weight CE(c(G(z', y)), y);  CE is
    F.cross_entropy with mean reduction.
  * Two Adams (G.parameters(), D.parameters()) with torch's defaults, created per train() call (ns_gan.py:107-110).
  * Glosses / Dlosses are the totals, Dlosses with NSGAN's np.mean over D_steps; class_losses is CE(c(x), y) of each
    iteration's last D step.  The epoch line is NSGAN's.
Fused path: ACGANEngine below (stock modules, 1 <= C <= 32, H % 4 == 0, H <= 1024, stock hooks); otherwise autograd
over ops.label_linear / ops.fused_linear + FlatAdam, with F.cross_entropy on a fused_linear(..., "id") class head."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, ops_fused
from ._lib import GMError, slot
from .trainers import (EPS, FlatAdam, GANTrainer, _dataset_rows, _lin, _parzen, _save_checkpoint, _stock_module, stock,
                       stock_model, to_cuda)
from .cvae import LabelError, _labels_arg, _layer
from .engine import FlatParams, _Linear, validate_labels
from .ring_engine import TwoAdamRingEngine, reference_loader_ok

HISTORY = ("Glosses", "Dlosses", "class_losses", "num_epochs")
MAX_C, MAX_H = 32, 1024


@stock_model
class Generator(nn.Module):
    """ns_gan.py:35-46 conditioned on the class: sigmoid(generate(relu(linear(z) + label(onehot(y)))))."""

    def __init__(self, image_size, hidden_dim, z_dim, num_classes):
        super().__init__()
        self.linear = nn.Linear(z_dim, hidden_dim)
        self.label = nn.Linear(num_classes, hidden_dim, bias=False)
        self.generate = nn.Linear(hidden_dim, image_size)

    def forward(self, z, y):
        if self.label.weight.shape[1] <= MAX_C:
            h = _layer(self.linear, self.label, z, y, "relu")
        else:
            # more classes than the label block of the forward kernel takes (32): the GEMM on the HIP kernel, the
            # selected column of E added by torch (the general path only; the fused engine refuses C > 32)
            if not y.is_cuda:
                y = validate_labels(y, self.label.weight.shape[1])
            h = torch.relu(_lin(self.linear, z, "id") + self.label.weight[:, y.to(z.device).long()].T)
        return _lin(self.generate, h, "sigmoid")


@stock_model
class Discriminator(nn.Module):
    """ns_gan.py:49-60 plus the class head: (sigmoid(discriminate(h)), classify(h)), h = relu(linear(x))."""

    def __init__(self, image_size, hidden_dim, num_classes, output_dim=1):
        super().__init__()
        self.linear = nn.Linear(image_size, hidden_dim)
        self.discriminate = nn.Linear(hidden_dim, output_dim)
        self.classify = nn.Linear(hidden_dim, num_classes)

    def forward(self, x):
        h = _lin(self.linear, x, "relu")
        return _lin(self.discriminate, h, "sigmoid"), _lin(self.classify, h, "id")


@stock_model
class ACGAN(nn.Module):
    """.G .D .z_dim .num_classes .shape (+ the constructor arguments as attributes)."""

    def __init__(self, image_size=784, hidden_dim=400, z_dim=20, num_classes=10):
        super().__init__()
        self.image_size, self.hidden_dim, self.z_dim = image_size, hidden_dim, z_dim
        self.num_classes = num_classes
        self.G = Generator(image_size, hidden_dim, z_dim, num_classes)
        self.D = Discriminator(image_size, hidden_dim, num_classes, 1)
        self.shape = int(image_size ** 0.5)


def acgan_fused_ok(model):
    """True iff an ACGAN's shapes fit the fused heads: 1 <= C <= 32, H % 4 == 0, H <= 1024, one source output, the
    generator's hidden width equal to the critic's (the plain GEMMs take any I and Z)."""
    G, D = model.G, model.D
    C, H = D.classify.weight.shape
    I, Z = D.linear.weight.shape[1], G.linear.weight.shape[1]
    return (1 <= C <= MAX_C and 4 <= H <= MAX_H and H % 4 == 0 and I > 0 and Z > 0
            and tuple(D.linear.weight.shape) == (H, I) and tuple(D.discriminate.weight.shape) == (1, H)
            and tuple(G.linear.weight.shape) == (H, Z) and tuple(G.label.weight.shape) == (H, C)
            and G.label.bias is None and tuple(G.generate.weight.shape) == (I, H))


class ACGANEngine(TwoAdamRingEngine):
    """The fused path.  Batch rows and both steps' noise come from the sampler / randn protocol replayed on the host
    (draw_sampler_indices, normal_ on the global generator) into rings of `graph_iters` iterations, uploaded per chunk;
    whole iterations are captured as hipGraphs of `graph_iters` iterations (and of 1 for the tail), each launch reading
    its own ring row.  Step counters on the device address the Adam schedules and the loss slots.
    Per D step, 10 launches: gather_rows; G's conditioned first layer (gm_fwd_args' label block) and its output layer
    into the stacked [x; G(z, y)]; the critic's hidden layer on the 2B rows; gm_acgan_heads_fwd; gm_acgan_heads_bwd
    (rows + combine, Adam on the four head tensors); D.linear's weight gradient with Adam in its epilogue; the tick.
    Per G step, 10: G's two layers; the critic's hidden layer; the heads' forward and backward in generator mode; dX
    through D.linear (sigmoid epilogue) and through G.generate (relu epilogue); G's paired weight gradients + Adam;
    gm_label_grad_adam for G.label; the tick.  One GPU only."""

    fused_ok = staticmethod(acgan_fused_ok)

    def __init__(self, model, data, labels, B, device, use_graph=True, world_size=1):
        if world_size > 1:
            raise GMError("the AC-GAN engine runs on one GPU: data parallelism is not implemented for it")
        if not acgan_fused_ok(model):
            raise GMError("ACGANEngine: shapes outside the fused heads' limits (1 <= C <= 32, H %% 4 == 0, H <= 1024, "
                          "equal hidden widths); ACGANTrainer trains these on the general path")
        self.model, self.data, self.labels, self.B, self.dev, self.use_graph = model, data, labels, B, device, use_graph
        G, D = model.G, model.D
        self.C, self.H = D.classify.weight.shape
        self.I, self.Z = D.linear.weight.shape[1], G.linear.weight.shape[1]
        self.fG = FlatParams(list(G.parameters()), device)
        self.fD = FlatParams(list(D.parameters()), device)
        self.G1, self.G2 = _Linear(self.fG, G.linear), _Linear(self.fG, G.generate)
        self.D1, self.D2, self.Dc = (_Linear(self.fD, l) for l in (D.linear, D.discriminate, D.classify))
        i = [k for k, p in enumerate(self.fG.params) if p is G.label.weight][0]
        o, n = self.fG.offsets[i], G.label.weight.numel()
        self.E, self.gE, self.mE, self.vE = self.fG.views[i], self.fG.gviews[i], self.fG.m[o:o + n].view(self.H, self.C), \
            self.fG.v[o:o + n].view(self.H, self.C)
        z = lambda *s: torch.zeros(*s, device=device)
        H, I, C = self.H, self.I, self.C
        self.X, self.Hg, self.Hd, self.dPre = z(2 * B, I), z(B, H), z(2 * B, H), z(2 * B, H)
        self.da2, self.dq = z(2 * B), z(2 * B, C)
        self.dXg, self.dHg = z(B, I), z(B, H)
        self.ws = ops_fused.acgan_heads_workspace(2 * B, H, C, device)
        self.ctr = torch.zeros(2, dtype=torch.int64, device=device)      # D steps, G steps of this train() call
        self.inv_b = float(np.float32(1.0) / np.float32(B))

    # ---- one iteration's launches -------------------------------------------------------------------------------
    def _heads(self):
        D2, Dc = self.D2, self.Dc
        return (D2.W, D2.b, Dc.W, Dc.b)

    def _issue_D(self, s, k):
        """One critic step on ring row k."""
        B, G1, G2, D1, D2, Dc = self.B, self.G1, self.G2, self.D1, self.D2, self.Dc
        idx = self.idx[k]
        lab = ops.label_src(self.labels, idx)
        tD = self.ctr[0:1].data_ptr()
        sl = slot(tD, 1, 0, 0, 1)
        ops.gather_rows(self.data, idx, self.X[:B], stream=s)
        ops.linear_fwd_label(self.zD[k], G1.W, G1.b, self.E, lab, self.Hg, "relu", stream=s)
        ops.linear_fwd(self.Hg, G2.W, G2.b, self.X[B:], "sigmoid", stream=s)
        ops.linear_fwd(self.X, D1.W, D1.b, self.Hd, "relu", stream=s)
        ops_fused.acgan_heads_fwd(self.Hd, *self._heads(), lab, B, False, self.class_weight, self.da2, self.dq, self.ws,
                                  loss_out=self.dloss, loss_slot=sl, ce_out=self.closs, ce_slot=sl, acc_out=self.dacc,
                                  acc_slot=sl, stream=s)
        adam = dict(sched=self.schedD, sched_slot=sl)
        ops_fused.acgan_heads_bwd(self.Hd, *self._heads(), B, False, self.da2, self.dq, self.dPre, self.ws,
                                  grads=(D2.gW, D2.gb, Dc.gW, Dc.gb), adam=adam,
                                  moments=(D2.mW, D2.vW, D2.mb, D2.vb, Dc.mW, Dc.vW, Dc.mb, Dc.vb), stream=s)
        ops.linear_bwd_dw_adam(self.dPre, self.X, D1, adam, stream=s)
        ops.tick(self.ctr[0:1], stream=s)

    def _issue_G(self, s, k, kd):
        """The generator step on noise row k, with the classes of the iteration's last critic batch (ring row kd)."""
        B, G1, G2, D1 = self.B, self.G1, self.G2, self.D1
        lab = ops.label_src(self.labels, self.idx[kd])
        sl = slot(self.ctr[1:2].data_ptr(), 1, 0, 0, 1)
        z, Xg, Hd, dPre = self.zG[k], self.X[B:], self.Hd[:B], self.dPre[:B]
        ops.linear_fwd_label(z, G1.W, G1.b, self.E, lab, self.Hg, "relu", stream=s)
        ops.linear_fwd(self.Hg, G2.W, G2.b, Xg, "sigmoid", stream=s)
        ops.linear_fwd(Xg, D1.W, D1.b, Hd, "relu", stream=s)
        ops_fused.acgan_heads_fwd(Hd, *self._heads(), lab, B, True, self.class_weight, self.da2, self.dq, self.ws,
                                  loss_out=self.gloss, loss_slot=sl, stream=s)
        ops_fused.acgan_heads_bwd(Hd, *self._heads(), B, True, self.da2, self.dq, dPre, self.ws, stream=s)
        ops.linear_bwd_dx(dPre, D1.W, self.dXg, below=Xg, epi="sigmoid", stream=s)
        ops.linear_bwd_dx(self.dXg, G2.W, self.dHg, below=self.Hg, epi="relu", stream=s)
        adam = dict(sched=self.schedG, sched_slot=sl)
        ops.linear_bwd_dw_adam_pair(dict(dA=self.dXg, X=self.Hg, lin=G2, adam=adam),
                                    dict(dA=self.dHg, X=z, lin=G1, adam=adam), stream=s)
        ops.label_grad_adam([dict(dPre=self.dHg, gE=self.gE, E=self.E, mE=self.mE, vE=self.vE)], lab, B, self.C,
                            adam=adam, stream=s)
        ops.tick(self.ctr[1:2], stream=s)

    launches_per_iteration = staticmethod(lambda D_steps=1: 10 * D_steps + 10)

    # ---- run settings, losses -----------------------------------------------------------------------------------
    d_step_losses = ("closs", "dacc")

    def _configure_extra(self, class_weight):
        self.class_weight = float(class_weight)
        return {"class_weight": self.class_weight}

    def losses(self, it0, it1):
        """(G losses, D losses, class losses) of iterations [it0, it1) of this train() call: the totals, D's as the
        mean over the iteration's critic steps, and CE(c(x), y) of its last critic step."""
        G, D = super().losses(it0, it1)
        d, cl = self.D_steps, self.closs.cpu().numpy()
        return G, D, [float(cl[it * d + d - 1]) for it in range(it0, it1)]


@stock
class ACGANTrainer(GANTrainer):
    """ns_gan.py's Trainer surface for the AC-GAN: train(num_epochs, G_lr, D_lr, D_steps, class_weight), the histories
    Glosses / Dlosses / class_losses, sample / generate_images / parzen with chosen classes, accuracy(), checkpoints."""
    _STOCK = ("train_D", "train_G", "process_batch", "compute_noise")

    def __init__(self, model, train_iter, val_iter, test_iter, viz=False):
        super().__init__(model, train_iter, val_iter, test_iter, viz)
        self.class_losses = []
        self.class_weight = 1.0

    # ---- hooks (the general path) -------------------------------------------------------------------------------
    def process_batch(self, iterator):
        """ns_gan.py:222-226, keeping the labels: (images [b, I] on the device, labels [b] on the host)."""
        images, labels = next(iter(iterator))
        return to_cuda(images.view(images.shape[0], -1)), labels

    def train_D(self, images, labels):
        """The contract's D_loss; leaves CE(c(x), y) in self._class_loss."""
        m = self.model
        y = to_cuda(labels).long()
        fake = m.G(self.compute_noise(images.shape[0], m.z_dim), labels).detach()
        sx, cx = m.D(images)
        sg, cg = m.D(fake)
        ce = F.cross_entropy(cx, y)
        self._class_loss = ce.detach()
        return -torch.mean(torch.log(sx + EPS) + torch.log(1 - sg + EPS)) + self.class_weight * (ce + F.cross_entropy(cg, y))

    def train_G(self, images, labels):
        """The contract's G_loss on the batch in hand."""
        m = self.model
        sg, cg = m.D(m.G(self.compute_noise(images.shape[0], m.z_dim), labels))
        return -torch.mean(torch.log(sg + EPS)) + self.class_weight * F.cross_entropy(cg, to_cuda(labels).long())

    # ---- path selection ---------------------------------------------------------------------------------------
    def _stock(self):
        if not self._stock_prefix():
            return False
        m = self.model
        G, D = getattr(m, "G", None), getattr(m, "D", None)
        if not (type(G) is Generator and type(D) is Discriminator and _stock_module(G, 3) and _stock_module(D, 3)
                and G.label.bias is None):
            return False                               # edited / subclassed networks: general path
        if not acgan_fused_ok(m):
            return False                               # outside the fused heads' limits: general path
        return reference_loader_ok(self.train_iter, labelled=True)

    def _device_labels(self, loader):
        """The dataset's classes as an int32 device tensor, validated on the host once per dataset."""
        cache = self.__dict__.setdefault("_label_cache", {})
        key = id(loader.dataset)
        if key not in cache:
            y = validate_labels(loader.dataset.tensors[1], self.model.num_classes)
            cache[key] = y if not torch.cuda.is_available() else y.to(next(self.model.parameters()).device)
        return cache[key]

    def _make_engine(self, data, loader, dev):
        return ACGANEngine(self.model, data, self._device_labels(loader), loader.batch_size, dev,
                           use_graph=self.use_graph)

    # ---- the loop -------------------------------------------------------------------------------------------------
    def train(self, num_epochs, G_lr=2e-4, D_lr=2e-4, D_steps=1, class_weight=1.0):
        """ns_gan.py:94 with the class head's weight."""
        from . import dp
        if dp.current()[0] > 1:
            raise GMError("ACGANTrainer runs on one GPU: data parallelism is not implemented for it")
        self.class_weight = float(class_weight)
        epoch_steps = int(np.ceil(len(self.train_iter) / D_steps))
        if self._stock():
            self._device_labels(self.train_iter)       # bad labels raise here, before anything is launched
            eng = self._get_engine()
            eng.use_graph = self.use_graph
            eng.configure(num_epochs * epoch_steps, G_lr, D_lr, D_steps, class_weight=class_weight,
                          resume=self.__dict__.pop("_resume_optim", None))
            for epoch in range(1, num_epochs + 1):
                self.model.train()
                it0 = (epoch - 1) * epoch_steps
                eng.run(epoch_steps)
                G_losses, D_losses, C_losses = eng.losses(it0, it0 + epoch_steps)
                self.class_losses.extend(C_losses)
                self._end_epoch(epoch, num_epochs, G_losses, D_losses)
                self._viz_epoch(epoch)
            return
        # GENERAL path: the hooks over autograd, the reference's loop
        if self.__dict__.get("_resume_optim") is not None:
            raise GMError("load_checkpoint() restored optimizer state, but this trainer runs the general path "
                          "(overridden hooks / edited networks), whose optimizers start fresh")
        if reference_loader_ok(self.train_iter, labelled=True):
            validate_labels(self.train_iter.dataset.tensors[1], self.model.num_classes)
        m = self.model
        G_opt, D_opt = FlatAdam(m.G.parameters(), G_lr), FlatAdam(m.D.parameters(), D_lr)
        for epoch in range(1, num_epochs + 1):
            m.train()
            G_losses, D_losses = [], []
            for _ in range(epoch_steps):
                step = []
                for _ in range(D_steps):
                    images, labels = self.process_batch(self.train_iter)
                    D_opt.zero_grad()
                    self._class_loss = None
                    D_loss = self.train_D(images, labels)
                    D_loss.backward()
                    D_opt.step()
                    step.append(D_loss.item())
                D_losses.append(np.mean(step))
                self.class_losses.append(float("nan") if self._class_loss is None else float(self._class_loss))
                G_opt.zero_grad()
                G_loss = self.train_G(images, labels)
                G_losses.append(G_loss.item())
                G_loss.backward()
                G_opt.step()
            self._end_epoch(epoch, num_epochs, G_losses, D_losses)
            self._viz_epoch(epoch)

    # ---- sampling, evaluation, pictures -------------------------------------------------------------------------
    def _generate(self, z, y, batch=1024):
        torch.cuda.synchronize()
        with torch.no_grad():
            return torch.cat([self.model.G(to_cuda(z[i:i + batch]), y[i:i + batch]) for i in range(0, z.shape[0], batch)])

    def sample(self, n, seed=0, labels=None):
        """n generated samples [n, image_size] of the given classes (None: arange(n) % num_classes; an int: that class
        for all): z ~ N(0, I) from torch.Generator().manual_seed(seed); the global generator and the model's mode are
        untouched."""
        n = int(n)
        y = _labels_arg(labels, n, self.model.num_classes)
        gen = torch.Generator().manual_seed(int(seed))
        return self._generate(torch.randn(n, self.model.z_dim, generator=gen), y)

    def parzen(self, n_samples=10000, sigmas=None, n_val=10000, seed=0):
        """Parzen-window log-likelihood of the test images under n_samples class-balanced samples."""
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

    def generate_images(self, epoch, num_outputs=36, save=True, labels=None):
        """ns_gan.py:228-262 for chosen classes (None: arange(num_outputs) % num_classes): compute_noise's draw from
        the global generator, saved as ../viz/<name>/reconst_<epoch>.png."""
        import os
        from . import viz
        m = self.model
        y = _labels_arg(labels, int(num_outputs), m.num_classes)
        z = self.compute_noise(num_outputs, m.z_dim)
        images = self._generate(z, y).view(num_outputs, m.shape, m.shape).float().cpu().numpy()
        if save:
            out = os.path.join(self.viz_dir if self.viz_dir is not None else os.path.join("..", "viz"), self.name)
            os.makedirs(out, exist_ok=True)
            viz.write_png_gray(os.path.join(out, "reconst_%d.png" % epoch),
                               viz.make_grid(images, int(num_outputs ** 0.5)))
        return images

    def accuracy(self, iterator=None, batch=1024):
        """The critic's class-head accuracy on the iterator's dataset (default test_iter): the share of rows whose
        largest class logit is their label.  Reads the dataset's tensors; draws nothing."""
        it = self.test_iter if iterator is None else iterator
        x = _dataset_rows(it).to(torch.float32)
        y = validate_labels(it.dataset.tensors[1], self.model.num_classes).to(torch.int64)
        torch.cuda.synchronize()
        hits = 0
        with torch.no_grad():
            for i in range(0, x.shape[0], batch):
                logits = self.model.D(to_cuda(x[i:i + batch].contiguous()))[1]
                hits += int((logits.argmax(1).cpu() == y[i:i + batch]).sum())
        return hits / max(1, x.shape[0])

    def save_checkpoint(self, savepath, collective=True):
        """Weights, both Adam states and step counts, the RNG cursor and the three histories (a finished train() call
        on the fused engine)."""
        _save_checkpoint(self, savepath, HISTORY, collective=collective)


__all__ = ["Generator", "Discriminator", "ACGAN", "ACGANTrainer", "ACGANEngine", "LabelError", "FlatAdam"]
