"""What the stand-alone GAN step engines (acgan.py, sngan.py, bgan.py) share: the replay of whole iterations in chunks
of `graph_iters` (ChunkedReplay), and on top of it NSGAN's loop with two Adams fed from host-drawn rings
(TwoAdamRingEngine).  A new model on the NSGAN loop writes __init__ (buffers, _Linear views, workspaces), _issue_D,
_issue_G, launches_per_iteration / fused_ok and, for settings of its own, _configure_extra.  Plus three helpers the
trainers share: nsgan_order_draws, reference_loader_ok, device_rows."""
import contextlib

import numpy as np
import torch

from . import ops
from ._lib import GMError
from .engine import draw_sampler_indices


def nsgan_order_draws(n, B, D_steps, k, idx, zD, zG):
    """The global generator's draws of k iterations in NSGANTrainer's order, into host tensors: per critic step the
    sampler's (draw_sampler_indices, row i * D_steps + j of idx [.., B]) and compute_noise's randn(B, Z) (the same row
    of zD), then the generator step's randn(B, Z) (row i of zG)."""
    for i in range(k):
        for r in range(i * D_steps, (i + 1) * D_steps):
            draw_sampler_indices(n, B, idx[r].numpy())
            zD[r].normal_()
        zG[i].normal_()


def reference_loader_ok(it, labelled=False):
    """True iff `it` is the reference's loader, whose draws the host replays: a shuffling DataLoader over a
    TensorDataset on the global generator, no workers, batches no larger than the dataset (and, with labelled, a
    second tensor to take the classes from)."""
    data = torch.utils.data
    return bool(isinstance(it, data.DataLoader) and isinstance(it.dataset, data.TensorDataset)
                and (not labelled or len(it.dataset.tensors) >= 2)
                and isinstance(it.sampler, data.RandomSampler)
                and it.sampler.generator is None and it.generator is None
                and not it.sampler.replacement and it.num_workers == 0
                and it.batch_size is not None and it.batch_size <= len(it.dataset))


def device_rows(loader, dev):
    """The loader's images as contiguous float32 rows [n, I] on the device."""
    imgs = loader.dataset.tensors[0]
    return imgs.reshape(imgs.shape[0], -1).to(dev, torch.float32).contiguous()


class ChunkedReplay:
    """Whole iterations replayed in chunks: hipGraphs of `graph_iters` iterations while that many remain, then of 1.
    Before each chunk _host_draws(k) puts the chunk's host draws on the device, through pinned buffers held twice so
    that one chunk's draws are made while the previous chunk's copies may still be in flight.
    Subclasses: _issue(s, i) (iteration i of a chunk on stream s), _host_draws(k), optionally _after_chunk(k); their
    configure() calls _new_rings()."""

    graph_iters = 16

    def _new_rings(self, *rings):
        """Once per configure(): two pinned host copies of the device rings, and no graphs (they hold the addresses
        of the last call's buffers)."""
        self.graphs = {}
        self._staged = [tuple(torch.zeros(r.shape, dtype=r.dtype).pin_memory() for r in rings) for _ in range(2)]
        self._staged_ev, self._stage = [None, None], 0

    @contextlib.contextmanager
    def _staging(self):
        """The pinned host tensors to draw into; the body ends with its copy_(non_blocking=True) calls to the device."""
        b = self._stage
        if self._staged_ev[b] is not None:
            self._staged_ev[b].synchronize()           # the copies that last read these pinned buffers have finished
        yield self._staged[b]
        ev = torch.cuda.Event()
        ev.record()
        self._staged_ev[b] = ev
        self._stage = 1 - b

    def _graph(self, k):
        g = self.graphs.get(k)
        if g is None:
            def body(s):
                for i in range(k):
                    self._issue(s, i)
            g = self.graphs[k] = ops.Graph().capture(body)
        return g

    def _after_chunk(self, k):
        pass

    def run(self, n_iters):
        done, K = 0, max(1, self.graph_iters)
        while done < n_iters:
            k = K if n_iters - done >= K else 1
            self._host_draws(k)
            if self.use_graph:
                self._graph(k).launch()
            else:
                s = ops.stream_ptr()
                for i in range(k):
                    self._issue(s, i)
            self._after_chunk(k)
            done += k


class TwoAdamRingEngine(ChunkedReplay):
    """NSGAN's loop on two flat Adams (fG, fD: FlatParams of the subclass).  Batch rows and both steps' noise come
    from the sampler / randn protocol replayed on the host into rings of `graph_iters` iterations (idx, zD: one row
    per critic step; zG: one per iteration), uploaded per chunk; each launch reads its own ring row.  Step counters
    on the device (ctr: D steps, G steps of this train() call) address the Adam schedules and the loss slots.
    Subclasses: _issue_D(s, k) (one critic step on ring row k), _issue_G(s, k, kd) (the generator step on noise row k;
    kd is the iteration's last critic row), and optionally betas, d_step_losses, _configure_extra."""

    betas = (0.9, 0.999)
    d_step_losses = ()                                 # names of further buffers with one slot per critic step
    steps_planned = None

    def _configure_extra(self):
        """Takes configure()'s further keyword settings, checks what the subclass must check before a resume, and
        returns the settings as they go into run_config (a checkpoint's optim.config)."""
        return {}

    def _issue(self, s, i):
        """Iteration i of a chunk."""
        d = self.D_steps
        for j in range(d):
            self._issue_D(s, i * d + j)
        self._issue_G(s, i, i * d + d - 1)

    def configure(self, n_iters, G_lr, D_lr, D_steps, resume=None, **settings):
        """Once per train(): fresh Adam state (the reference's optimizers are locals of train()), schedules, loss
        buffers, rings.  resume: a checkpoint's optim_state() -- moments restored, schedules continued."""
        dev, B, Z = self.dev, self.B, self.Z
        self.D_steps = int(D_steps)
        self.step0 = {"G": 0, "D": 0}
        for fp in (self.fG, self.fD):
            fp.rebind(); fp.reset_state(); fp.grad.zero_()
        self.run_config = {"B": int(B), "D_steps": int(D_steps), "G_lr": float(G_lr), "D_lr": float(D_lr),
                           **self._configure_extra(**settings)}
        if resume is not None:
            saved = resume.get("config")
            if saved is not None and not resume.get("lenient", False):
                diff = {k: (saved[k], v) for k, v in self.run_config.items() if k in saved and saved[k] != v}
                if diff:
                    raise GMError("checkpoint was written by a run with different settings (saved, now): %s -- "
                                  "load_checkpoint(path, strict=False) overrides" % diff)
            for net, fp in (("G", self.fG), ("D", self.fD)):
                st = resume[net]
                if st["m"].numel() != fp.m.numel():
                    raise GMError("checkpoint optimizer state does not match this model")
                fp.m.copy_(st["m"]); fp.v.copy_(st["v"])
                self.step0[net] = int(st["step"])
        nD, nG = max(1, n_iters * self.D_steps), max(1, n_iters)
        self.steps_planned = {"G": n_iters, "D": n_iters * self.D_steps}
        sched = lambda lr, n, net: torch.from_numpy(
            ops.adam_schedule(lr, n, betas=self.betas, start=self.step0[net] + 1)).to(dev)
        self.schedD, self.schedG = sched(D_lr, nD, "D"), sched(G_lr, nG, "G")
        for name in ("dloss",) + tuple(self.d_step_losses):
            setattr(self, name, torch.zeros(nD, device=dev))
        self.gloss = torch.zeros(nG, device=dev)
        self.ctr.zero_()
        K = max(1, self.graph_iters)
        R = K * self.D_steps
        self.idx = torch.zeros(R, B, dtype=torch.int64, device=dev)
        self.zD, self.zG = torch.zeros(R, B, Z, device=dev), torch.zeros(K, B, Z, device=dev)
        self._new_rings(self.idx, self.zD, self.zG)
        self.done = 0

    def optim_state(self):
        torch.cuda.synchronize()
        cpu = lambda t: t.detach().cpu().clone()
        st = {net: {"m": cpu(fp.m), "v": cpu(fp.v), "step": self.step0[net] + self.steps_planned[net]}
              for net, fp in (("G", self.fG), ("D", self.fD))}
        st["config"] = dict(self.run_config)
        return st

    def _host_draws(self, k):
        d = self.D_steps
        with self._staging() as (hi, hd, hg):
            nsgan_order_draws(self.data.shape[0], self.B, d, k, hi, hd, hg)
            self.idx[:k * d].copy_(hi[:k * d], non_blocking=True)
            self.zD[:k * d].copy_(hd[:k * d], non_blocking=True)
            self.zG[:k].copy_(hg[:k], non_blocking=True)

    def _after_chunk(self, k):
        self.done += k

    def losses(self, it0, it1):
        """(G losses, D losses) of iterations [it0, it1) of this train() call, D's as the mean over the iteration's
        critic steps (one read-back)."""
        d = self.D_steps
        dl, gl = self.dloss.cpu().numpy(), self.gloss.cpu().numpy()
        G = [float(gl[it]) for it in range(it0, it1)]
        D = [np.mean([float(dl[it * d + j]) for j in range(d)]) for it in range(it0, it1)]
        return G, D

    def phase_grads(self):
        """The last critic step's and the last generator step's gradients: {"d": {...}, "g": {...}}, keyed by the
        model's state_dict names (views of the flat gradient buffers)."""
        names = {id(p): n for n, p in self.model.named_parameters()}
        out = {"d": {}, "g": {}}
        for key, fp in (("d", self.fD), ("g", self.fG)):
            for p, gv in zip(fp.params, fp.gviews):
                out[key][names[id(p)]] = gv
        return out
