"""vae.py / ae.py / bir_vae.py `compute_batch` + train loop + evaluate on hipGraphs: VAEEngine and the two engines
that reuse its machinery (AEEngine: no sampling, no KL; BIRVAEEngine: numpy's generator, MMD instead of KL)."""
import numpy as np
import torch

from . import ops
from ._lib import GMError
from .engine import CHUNK, FlatParams, GANEngine, HostReplay, NumpyReplay, _Linear, _align4


class VAEEngine:
    """vae.py:144-167 (train loop) + :214-223 (evaluate) as hipGraphs: one graph per distinct
    batch size (full batches and the ragged last one, 50 000 mod 512 = 336), a device step counter
    selecting index rows / eps rows / Adam-schedule rows / loss slots."""

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None,
                 force_dp=False):
        self.model, self.device, self.use_graph = model, device, use_graph
        enc, dec = model.encoder, model.decoder
        hw, hb, Z = self._head(enc)
        plist = [enc.linear.weight, enc.linear.bias, hw, hb,
                 dec.linear.weight, dec.linear.bias, dec.recon.weight, dec.recon.bias] + self._extra_params(model)
        self._dp_init(plist, world_size, rank, process_group, force_dp)
        self.fp = FlatParams(plist, device, grad_alloc=self._grad_alloc)
        fp = self.fp
        self.E1, self.D1, self.D2 = _Linear(fp, enc.linear), _Linear(fp, dec.linear), \
            _Linear(fp, dec.recon)
        H = hw[0].shape[1]
        Wh = sum(w.shape[0] for w in hw)             # the packed head's width (the VAE's: 2 Z)
        self.Z, self.H, self.I = Z, H, enc.linear.weight.shape[1]
        i_w = [i for i, p in enumerate(fp.params) if p is hw[0]][0]
        i_b = [i for i, p in enumerate(fp.params) if p is hb[0]][0]
        o_w, o_b = fp.offsets[i_w], fp.offsets[i_b]

        class _Packed:          # [mu ; log_var] as one 2Z x H layer
            W = fp.flat[o_w:o_w + Wh * H].view(Wh, H)
            b = fp.flat[o_b:o_b + Wh]
            gW = fp.grad[o_w:o_w + Wh * H].view(Wh, H)
            gb = fp.grad[o_b:o_b + Wh]
            mW, vW = fp.m[o_w:o_w + Wh * H], fp.v[o_w:o_w + Wh * H]
            mb, vb = fp.m[o_b:o_b + Wh], fp.v[o_b:o_b + Wh]
        self.ML = _Packed
        self._common_init(device)

    has_eps = True              # the VAE draws eps per batch (vae.py:104); the plain AE does not

    def _head(self, enc):
        """The encoder's head as the packed layer behind its first one: (weights, biases, latent width) -- the tensors
        packed row block after row block, the width what the decoder reads.  (CatVAEEngine: the logits layer alone.)"""
        return (enc.mu.weight, enc.log_var.weight), (enc.mu.bias, enc.log_var.bias), enc.mu.weight.shape[0]

    def _extra_params(self, model):
        """Parameters a subclass packs behind the encoder's and the decoder's (NFVAEEngine: the flow's)."""
        return []

    # ---- data parallel: every batch's rows are split over the ranks; the losses are
    # SUMS (vae.py:203,212), so the gradient all-reduce is a plain sum with no 1/N and the per-rank
    # loss slots add up to the reference's values -------------------------------------------------
    def _dp_init(self, plist, world, rank, pg, force_dp):
        import os
        self.world, self.rank, self.pg, self.force_dp = world, rank, pg, bool(force_dp)
        self.comm, self._grad_alloc = None, None
        if world > 1 or force_dp:
            if os.environ.get("GM_DP_COMM", "peer") != "peer":
                raise GMError("data-parallel VAE / AE exchange gradients with the in-graph peer "
                              "communicator (GM_DP_COMM=peer)")
            from . import dp
            n = 0
            for item in plist:
                for q in (item if isinstance(item, (tuple, list)) else (item,)):
                    n += q.numel()
                n = _align4(n)
            self.comm = dp.PeerComm(n, world, rank, pg)
            ok = self.comm.selfcheck(self.device)
            if world > 1:
                import torch.distributed as dist
                flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
                if dist.get_backend(pg) == "nccl":
                    flag = flag.to(self.device)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=pg)
                ok = bool(flag.item())
            if not ok:
                raise GMError("peer exchange self-check failed: data-parallel VAE / AE needs hipIpc peer "
                              "mappings between the ranks' GPUs")
            self._grad_alloc = lambda k: self.comm.grad_buffer()[:k]

    def _dp(self):
        return self.world > 1 or self.force_dp

    def _rows(self, b):
        """Rows [lo, hi) of a batch of b rows owned by this rank (ragged batches split as evenly as
        integer division allows)."""
        return b * self.rank // self.world, b * (self.rank + 1) // self.world

    def read_losses(self, buf, lo, n):
        """Loss slots [lo, lo+n) summed over ranks (each rank holds its rows' partial sums)."""
        t = buf[lo:lo + n]
        if self.world > 1:
            import torch.distributed as dist
            from . import dp
            self.comm.check()
            t = t.cpu() if dist.get_backend(self.pg) != "nccl" else t.clone()
            dp.allreduce_sum_(t, self.pg)
        return t.cpu().numpy()

    one_gpu = None              # an engine without data parallelism names itself here ("the MADE engine")

    def _refuse_dp(self, world_size, force_dp):
        if world_size > 1 or force_dp:
            raise GMError("%s runs on one GPU: data parallelism is not implemented for it" % self.one_gpu)

    def _init_flat(self, model, device, use_graph, plist):
        """What a one-GPU engine over a parameter list of its own starts with (after _refuse_dp and its model check): the
        flat parameter / gradient / moment buffers over `plist` and the epoch machinery's state."""
        self.model, self.device, self.use_graph = model, device, use_graph
        self._dp_init(plist, 1, 0, None, False)
        self.fp = FlatParams(plist, device)
        self._common_init(device)

    def _bind_trainer(self, trainer):
        """The trainer a device-noise engine reads its seed and noise_steps from, and the device word configure() writes
        the latter to: a training batch's noise step is ctr + nbase, so it is never baked into a graph."""
        self.trainer = trainer
        self.nbase = torch.zeros(1, dtype=torch.int64, device=self.device)

    def _clock(self, t, train, add=0):
        """The noise-clock keywords of the batch at ring step t (+ add), for the ops_fused noise builders: a graph reads
        the device counter ctr, an eager launch passes t; a training batch adds nbase on the device, a validation batch
        (whose step is its index in the pass) has no base."""
        base = self.nbase if train else None
        if self.use_graph:
            return dict(step=add, step_ctr=self.ctr, step_base=base)
        return dict(step=t + add, step_ctr=None, step_base=base)

    def _settings(self):
        """The run's settings beside B, lr and weight_decay: saved in checkpoints, compared on resume, and launch
        arguments of the captured graphs (a change drops them)."""
        return {}

    def _graph_args(self):
        """Device addresses the captured graphs hold beside the engine's own buffers and the dataset (MADEEngine: the
        degree vectors; DDPMEngine: the tables): a change drops the graphs."""
        return ()

    def _common_init(self, device):
        from . import _respect_cpu_quota
        _respect_cpu_quota(force=False)             # once per process, when the first engine is built
        self.ctr = torch.zeros(1, dtype=torch.int64, device=device)
        self.graphs = {}
        self._bufB = None
        import os
        self.fuse_adam = True
        self.pair_dw = True
        self.graph_iters = max(1, int(os.environ.get("GM_GRAPH_ITERS", "32")))   # batches per graph
        self.prefetch_gather = True
        # launch fusions of round 3 (each replaces a ~5 us latency-bound launch by an epilogue)
        self.fuse_sqerr = True
        self.fuse_reparam_bwd = True
        self.fuse_reparam_fwd = True
        self.fuse_bwd_mid = True
        self.fin_in_dw = True
        self.fin_done = torch.zeros(1, dtype=torch.int32, device=device)
        self.trainer = None                          # _bind_trainer sets it

    def _alloc(self, B):
        if self._bufB == B:
            return
        dev, I, H, Z = self.device, self.I, self.H, self.Z
        z = lambda *s: torch.zeros(*s, device=dev)
        self.X, self.He, self.ml, self.Zs = z(B, I), z(B, H), z(B, 2 * Z), z(B, Z)
        self.Xb = (self.X, z(B, I))                 # batch i of a multi-batch graph reads Xb[i % 2]
        self.Hdec, self.Xr, self.dA = z(B, H), z(B, I), z(B, I)
        self.dHdec, self.dZ, self.dml, self.dHe = z(B, H), z(B, Z), z(B, 2 * Z), z(B, H)
        self.part = z(B)
        self._sq_alloc(B)
        self.part_kl = z((B * Z + 255) // 256)
        self._bufB = B
        self.graphs = {}

    def _slot(self, t, mul, add, ring, stride):
        if self.use_graph:
            return ops.slot(self.ctr.data_ptr(), mul, add, ring, stride)
        i = t * mul + add
        if ring > 0:
            i %= ring
        return ops.slot(0, 0, i, 0, stride)

    # -- reconstruction loss in the decoder's last forward (ops.linear_fwd_sqerr; GM_VAE_FUSE_SQERR=0: the
    # separate gm_sqerr_sigmoid_bwd launch) -- per (row, 32-column tile) partials, rows ldp floats apart
    def _sq_alloc(self, B):
        ldp = _align4((self.I + 31) // 32)
        self.part2 = torch.zeros(B, ldp, device=self.device)

    def _recon_fwd(self, st, x_in, lin, X, b):
        """x_hat = sigmoid(lin(x_in)), dA = d sum((X - x_hat)^2) / d (pre-sigmoid), and the loss partials.
        Returns (partials tensor, number of floats to sum)."""
        from . import ops_fused as of_
        if self.fuse_sqerr:
            ops.linear_fwd_sqerr(x_in, lin.W, lin.b, self.Xr, X, self.dA, self.part2, M=b, stream=st)
            return self.part2, b * self.part2.shape[1]
        ops.linear_fwd(x_in, lin.W, lin.b, self.Xr, "sigmoid", M=b, stream=st)
        of_.sqerr_sigmoid_bwd(X, self.Xr, self.dA, self.part, b, stream=st)
        return self.part, b

    def _gather_plan(self, pos, of):
        """Batch `pos` of a graph of `of` equal-size batches: (its image buffer, whether it gathers its
        own rows, the buffer the NEXT batch's rows are prefetched into or None).  Inside a multi-batch
        graph the gather of batch i+1 rides in a small forward GEMM of batch i (ops.linear_fwd_gather:
        extra workgroups of that launch), so only the graph's first batch pays a gather launch."""
        X = self.Xb[pos % 2]
        nxt = self.Xb[(pos + 1) % 2] if (self.prefetch_gather and pos + 1 < of) else None
        return X, (pos == 0 or not self.prefetch_gather), nxt

    def _encoder_rows(self, X, train):
        """The rows the encoder's first layer reads for the batch whose clean rows are X: X itself."""
        return X

    def _gather_own(self, st, t, lo, b, X, idx_slot, train):
        """The batch's own gather launch (the first batch of a graph, or every batch without prefetching)."""
        ops.gather_rows(self.data, self.idx_ring.view(-1)[lo:], X, B=b, idx_slot=idx_slot, stream=st)

    def _fwd_with_prefetch(self, st, t, lo, b, x, lin, y, act, nxt, train=True):
        """linear_fwd, carrying the gather of the next batch's rows (ring slot t + 1) when asked to."""
        if nxt is None:
            ops.linear_fwd(x, lin.W, lin.b, y, act, M=b, stream=st)
        else:
            ops.linear_fwd_gather(x, lin.W, lin.b, y, act, self.data, self.idx_ring.view(-1)[lo:], nxt, M=b,
                                  B=b, idx_slot=self._slot(t, 1, 1, self.R, self.B), stream=st)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: forward + losses (+ backward + Adam when train)."""
        from . import ops_fused as of_
        of = max(1, of)
        R, B, Z = self.R, self.B, self.Z
        E1, ML, D1, D2 = self.E1, self.ML, self.D1, self.D2
        idx_slot = self._slot(t, 1, 0, R, B)
        eps_slot = self._slot(t, 1, 0, R, B * Z)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        recon_out, kl_out = (self.recon, self.kl) if train else (self.vrecon, self.vkl)
        lo, hi = self._rows(b)                       # this rank's rows of the batch
        b = hi - lo
        X, own, nxt = self._gather_plan(pos, of)
        Xe = self._encoder_rows(X, train)            # what the encoder reads (DVAEEngine: the corrupted rows)
        if own:
            self._gather_own(st, t, lo, b, X, idx_slot, train)
        ops.linear_fwd(Xe, E1.W, E1.b, self.He, "relu", M=b, stream=st)
        self._fwd_with_prefetch(st, t, lo, b, self.He, ML, self.ml, "id", nxt, train=train)
        eps_base = self.eps_ring.view(-1)[lo * Z:]
        if self.fuse_reparam_fwd and Z <= 32 and Z % 4 == 0:
            # reparameterisation + the decoder's first layer: ONE launch (the GEMM workgroups form z from
            # (mu, log_var, eps) themselves; bit-identical to the two launches)
            n_kl = of_.vae_reparam_fwd(self.ml, eps_base, self.Zs, self.part_kl, b, Z, D1.W, D1.b, self.Hdec, "relu",
                                       eps_slot=eps_slot, stream=st)
        else:
            n_kl = of_.vae_reparam_wide(self.ml, eps_base, self.Zs, self.part_kl, b, Z, eps_slot=eps_slot, stream=st)
            ops.linear_fwd(self.Zs, D1.W, D1.b, self.Hdec, "relu", M=b, stream=st)
        part, n_part = self._recon_fwd(st, self.Hdec, D2, X, b)
        if train:
            sched_slot = self._slot(t, 1, 0, 0, 1)
            if self.fuse_adam and not self._dp():
                # Adam (weight_decay 1e-5, vae.py:139-142) folded into every dW epilogue; each dX
                # GEMM reads a layer's weights BEFORE that layer's dW launch updates them
                adam = dict(sched=self.sched, sched_slot=sched_slot)
                dw = lambda dA, X, lin: ops.linear_bwd_dw_adam(dA, X, lin, adam, M=b,
                                                               weight_decay=self.wd, stream=st)
            else:
                adam = None
                dw = lambda dA, X, lin: ops.linear_bwd_dw(dA, X, lin.gW, lin.gb, M=b, stream=st)
            if self.pair_dw:
                # weight gradients of two layers as ONE launch once both their inputs exist (the dX
                # GEMMs that still read those weights are issued first)
                dw2 = lambda a1, a2: ops.linear_bwd_dw_adam_pair(
                    dict(dA=a1[0], X=a1[1], lin=a1[2], adam=adam, M=b),
                    dict(dA=a2[0], X=a2[1], lin=a2[2], adam=adam, M=b),
                    weight_decay=self.wd if adam is not None else 0.0, stream=st)
            else:
                dw2 = lambda a1, a2: (dw(*a1), dw(*a2))
            ops.linear_bwd_dx(self.dA, D2.W, self.dHdec, below=self.Hdec, epi="relu", M=b, stream=st)
            # gm_vae_bwd_mid keeps ONE hidden width (decoder's = encoder's) of at most 512 in its workgroup; other
            # models (hidden_dim 800 / 1024, unequal widths) take the two generic dX launches below
            mid = (self.fuse_bwd_mid and self.fuse_reparam_bwd and Z <= 32 and self.H % 4 == 0 and self.H <= 512
                   and D1.W.shape[0] == self.H and ML.W.shape[1] == self.H)
            if mid:
                # dz, d loss / d [mu | log_var] and dHe: the two narrow GEMMs between the decoder's and the encoder's
                # wide ones as ONE launch, 16 rows per workgroup (reads D1.W and ML.W before the pairs step them)
                of_.vae_bwd_mid(self.dHdec, D1.W, self.ml, eps_base, self.dml, ML.W, self.He, self.dHe, b,
                                eps_slot=eps_slot, stream=st)
            elif self.fuse_reparam_bwd:
                # dz and, in the same launch's epilogue, d loss / d [mu | log_var] (vae.py:100-106,210-212)
                ops.linear_bwd_dx_reparam(self.dHdec, D1.W, self.dZ, self.ml, eps_base, self.dml, M=b,
                                          eps_slot=eps_slot, stream=st)
            else:
                ops.linear_bwd_dx(self.dHdec, D1.W, self.dZ, M=b, stream=st)
            dw2((self.dA, self.Hdec, D2), (self.dHdec, self.Zs, D1))
            if not self.fuse_reparam_bwd:
                of_.vae_reparam_bwd(self.ml, eps_base, self.dZ, self.dml, b, Z,
                                   eps_slot=eps_slot, stream=st)
            if not mid:
                ops.linear_bwd_dx(self.dml, ML.W, self.dHe, below=self.He, epi="relu", M=b, stream=st)
            if self.fin_in_dw and self.pair_dw and adam is not None and not self._dp():
                # the batch's LAST launch: the encoder's two weight gradients + Adam, both loss sums (vae.py:203, :212)
                # in one more workgroup of the same grid, the counter tick by the last workgroup to finish
                ops.linear_bwd_dw_adam_pair_finalize(
                    dict(dA=self.dHe, X=Xe, lin=E1, adam=adam, M=b), dict(dA=self.dml, X=self.He, lin=ML, adam=adam, M=b),
                    dict(pa=part, na=n_part, out_a=recon_out, slot_a=loss_slot, pb=self.part_kl, nb=n_kl, out_b=kl_out,
                         slot_b=loss_slot, done=self.fin_done, tick=self.ctr if self.use_graph else None),
                    weight_decay=self.wd, stream=st)
                return
            dw2((self.dHe, Xe, E1), (self.dml, self.He, ML))    # (the big GEMM first: its tile shape serves both)
            self._optimizer_step(st, sched_slot)
        # both loss sums (vae.py:203, :212) are the step's LAST launch, which also carries the counter tick
        of_.sum_finalize2(part, n_part, recon_out, loss_slot, self.part_kl, n_kl, kl_out, loss_slot,
                          tick=self.ctr if self.use_graph else None, stream=st)

    def _optimizer_step(self, st, sched_slot):
        """optimizer.step() (vae.py:162) when it is not fused into the dW epilogues: data parallel ->
        gradient SUM over ranks + Adam in the exchange's gather kernel."""
        if self._dp():
            self.comm.allreduce_adam(self.fp.grad, self.fp.flat, self.fp.m, self.fp.v, self.sched, sched_slot,
                                     weight_decay=self.wd, stream=st)
        elif not self.fuse_adam:
            ops.adam(self.fp.flat, self.fp.grad, self.fp.m, self.fp.v, self.sched, sched_slot,
                     weight_decay=self.wd, stream=st)

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        dev = self.device
        settings = self._settings()
        config = {"B": int(B), "lr": float(lr), "weight_decay": float(weight_decay)}
        config.update(settings)
        if resume is not None:                       # see GANEngine.configure; refused BEFORE anything is touched
            saved = resume.get("config")
            if saved is not None and not resume.get("lenient", False):
                diff = {k: (saved[k], config[k]) for k in config if k in saved and saved[k] != config[k]}
                if diff:
                    raise GMError("checkpoint was written by a run with different settings (saved, now): "
                                  "%s; load_checkpoint(path, strict=False) overrides" % diff)
            if resume["m"].numel() != self.fp.m.numel():
                raise GMError("checkpoint optimizer state does not match this model")
        self._alloc(B)
        self.B, self.wd = B, float(weight_decay)
        self.fp.rebind()
        self.fp.reset_state()
        self.fp.grad.zero_()
        self.step0 = 0
        self.run_config = config
        if resume is not None:
            self.fp.m.copy_(resume["m"]); self.fp.v.copy_(resume["v"])
            self.step0 = int(resume["step"])
        self.steps_planned = n_train_steps
        # buffers whose addresses the captured graphs hold are kept across train() calls (grow-only),
        # so a second train() with the same batch size / weight decay replays instead of re-capturing
        self._moved = False
        self.sched = GANEngine._pbuf(self, "sched", ops.adam_schedule(lr, max(1, n_train_steps),
                                                                      start=self.step0 + 1))
        self.recon = GANEngine._pbuf(self, "recon", max(1, n_train_steps))
        self.kl = GANEngine._pbuf(self, "kl", max(1, n_train_steps))
        self.R = CHUNK
        if getattr(self, "_ring_B", None) != B:
            self.idx_ring = torch.zeros(self.R, B, dtype=torch.int64, device=dev)
            self.stage = [dict(idx=torch.zeros(self.R, B, dtype=torch.int64).pin_memory(), event=None)
                          for _ in range(2)]
            if self.has_eps:                         # the host-drawn eps: a device ring and its two pinned halves
                self.eps_ring = torch.zeros(self.R, B, self.Z, device=dev)
                for st in self.stage:
                    st["eps"] = torch.zeros(self.R, B, self.Z).pin_memory()
            self._ring_B = B
            self._moved = True
        # the settings' values and the subclass's extra addresses are launch arguments of the graphs
        vkey = (B, self.wd, self.use_graph, self.fuse_adam, self.pair_dw, self.prefetch_gather,
                tuple(settings.values()), self._graph_args())
        if self._moved or getattr(self, "_vkey", None) != vkey:
            self.graphs = {}
        self._vkey = vkey
        self.t_train = 0
        if self.trainer is not None:
            self.nbase.fill_(int(self.trainer.noise_steps))

    def optim_state(self):
        torch.cuda.synchronize()
        return {"m": self.fp.m.detach().cpu().clone(), "v": self.fp.v.detach().cpu().clone(),
                "step": self.step0 + self.steps_planned, "config": dict(self.run_config)}

    def _data_key(self):
        """What a captured graph reads besides its own buffers: the pass's dataset."""
        return self.data.data_ptr()

    def _graph(self, b, train, k=1):
        """hipGraph of k consecutive batches of size b (the device counter advances per batch)."""
        key = (b, train, self._data_key(), k)
        if key not in self.graphs:
            torch.cuda.synchronize()
            # full batches: every power-of-two size at once (an epoch's chunking asks for different
            # sizes from pass to pass; capturing them one by one would land inside later passes)
            sizes = [k]
            if b == self.B and self.use_graph:
                sizes, n = [], 1
                while n <= self.graph_iters:
                    sizes.append(n)
                    n *= 2
                if k not in sizes:
                    sizes.append(k)
            for n in sizes:
                kk = (b, train, self._data_key(), n)
                if kk not in self.graphs:
                    self.graphs[kk] = ops.Graph().capture(
                        lambda st, n=n: [self._issue(st, 0, b, train, pos=i, of=n) for i in range(n)])
        return self.graphs[key]

    def run_pass(self, data, perm, train, t0):
        """One pass over `data` in the order `perm` (host int64 tensor): batches of B rows, last
        one ragged.  Global eps draws (vae.py:104) happen here, batch by batch, in order.
        t0: first loss/schedule slot.  Returns number of batches."""
        self.data = data
        B, R = self.B, self.R
        n = perm.numel()
        nb = (n + B - 1) // B
        self.ctr.fill_(t0)
        done, which = 0, 0
        while done < nb:
            t = t0 + done
            cnt = min(R - (t % R), nb - done)
            s = self.stage[which]
            which ^= 1
            if s["event"] is not None:
                s["event"].synchronize()
            sizes = [min(B, n - (done + k) * B) for k in range(cnt)]
            lo = done * B
            hi = min(n, lo + cnt * B)
            s["idx"].view(-1)[:hi - lo].copy_(perm[lo:hi])    # rows of B indices, last one ragged
            self._draw_chunk(s, sizes)
            r = t % R
            self.idx_ring[r:r + cnt].copy_(s["idx"][:cnt], non_blocking=True)
            self._upload_chunk(s, r, cnt)
            ev = torch.cuda.Event()
            ev.record()
            s["event"] = ev
            k = 0
            while k < len(sizes):
                b = sizes[k]
                if not self.use_graph:
                    self._issue(ops.stream_ptr(), t + k, b, train)
                    k += 1
                    continue
                run = 1
                while k + run < len(sizes) and sizes[k + run] == b:
                    run += 1
                # the run of equal-size batches as power-of-two graphs, largest first (each size is
                # captured once, on first use): only a graph's FIRST batch pays its own gather launch
                piece = 1
                while piece * 2 <= min(run, self.graph_iters):
                    piece *= 2
                self._graph(b, train, piece).launch()
                k += piece
            done += cnt
        return nb

    def _torch_normal_rows(self, dst, sizes):
        """torch.randn(b, Z) per batch of the chunk (global CPU generator, in order) into dst[k]: the
        full batches in one C call (HostReplay), a ragged last batch on its own."""
        B, Z = self.B, self.Z
        nfull = sum(1 for b in sizes if b == B)
        from ._lib import DRAW_NORMAL
        replay = HostReplay.available() and B * Z >= 16
        if replay and nfull:
            replay = HostReplay.run([HostReplay.op(DRAW_NORMAL, B * Z, dst, B * Z * 4)], nfull)
        for k, b in enumerate(sizes):
            if replay and b == B:
                continue
            if replay and b * Z >= 16 and HostReplay.run([HostReplay.op(DRAW_NORMAL, b * Z, dst[k], 0)], 1):
                continue
            dst[k].view(-1)[:b * Z].normal_()

    def _draw_chunk(self, s, sizes):
        """HOST draws of the chunk's batches, in the reference's order (vae.py:104)."""
        if self.has_eps:
            self._torch_normal_rows(s["eps"], sizes)

    def _upload_chunk(self, s, r, cnt):
        if self.has_eps:
            self.eps_ring[r:r + cnt].copy_(s["eps"][:cnt], non_blocking=True)

    def alloc_val(self, n):
        if getattr(self, "vrecon", None) is None or self.vrecon.numel() < n:
            self.vrecon = torch.zeros(n, device=self.device)
            self.vkl = torch.zeros(n, device=self.device)
            self.graphs = {k: g for k, g in self.graphs.items() if k[1]}   # drop eval graphs


class AEEngine(VAEEngine):
    """ae.py:104-164 on the VAE engine's machinery: encoder layer (relu),
    decoder layer (sigmoid), squared-error loss; no sampling, so no eps ring and no KL term."""

    has_eps = False

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None,
                 force_dp=False):
        self.model, self.device, self.use_graph = model, device, use_graph
        enc, dec = model.encoder, model.decoder
        plist = [enc.linear.weight, enc.linear.bias, dec.linear.weight, dec.linear.bias]
        self._dp_init(plist, world_size, rank, process_group, force_dp)
        self.fp = FlatParams(plist, device, grad_alloc=self._grad_alloc)
        self.E1, self.D2 = _Linear(self.fp, enc.linear), _Linear(self.fp, dec.linear)
        self.H, self.I = enc.linear.weight.shape
        self._common_init(device)

    def _alloc(self, B):
        if self._bufB == B:
            return
        z = lambda *s: torch.zeros(*s, device=self.device)
        self.X, self.He, self.Xr, self.dA = z(B, self.I), z(B, self.H), z(B, self.I), z(B, self.I)
        self.Xb = (self.X, z(B, self.I))
        self.dHe, self.part = z(B, self.H), z(B)
        self._sq_alloc(B)
        self._bufB = B
        self.graphs = {}

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: ae.py:147-160 (+ backward and Adam when train)."""
        from . import ops_fused as of_
        E1, D2 = self.E1, self.D2
        idx_slot = self._slot(t, 1, 0, self.R, self.B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        lo, hi = self._rows(b)                       # this rank's rows of the batch
        b = hi - lo
        X, own, nxt = self._gather_plan(pos, of)
        if own:
            ops.gather_rows(self.data, self.idx_ring.view(-1)[lo:], X, B=b, idx_slot=idx_slot, stream=st)
        self._fwd_with_prefetch(st, t, lo, b, X, E1, self.He, "relu", nxt)
        part, n_part = self._recon_fwd(st, self.He, D2, X, b)
        if train:
            sched_slot = self._slot(t, 1, 0, 0, 1)
            adam = dict(sched=self.sched, sched_slot=sched_slot) if (self.fuse_adam and not self._dp()) else None
            # dH reads the decoder weights before the paired dW launch updates them
            ops.linear_bwd_dx(self.dA, D2.W, self.dHe, below=self.He, epi="relu", M=b, stream=st)
            ops.linear_bwd_dw_adam_pair(dict(dA=self.dA, X=self.He, lin=D2, adam=adam, M=b),
                                        dict(dA=self.dHe, X=X, lin=E1, adam=adam, M=b),
                                        weight_decay=self.wd if adam is not None else 0.0, stream=st)
            self._optimizer_step(st, sched_slot)
        of_.sum_finalize(part, n_part, self.recon if train else self.vrecon, out_slot=loss_slot,
                        tick=self.ctr if self.use_graph else None, stream=st)


class BIRVAEEngine(VAEEngine):
    """bir_vae.py:119-232: encoder 784->400->mu, z = mu + eps with eps ~
    N(0, set_var) from NUMPY's global RNG (drawn on the host exactly as the reference does,
    bir_vae.py:92-94 -- a variance used as a standard deviation is part of the contract), decoder,
    loss = sum (x - x_hat)^2 + 1000 * MMD(z) with the Gaussian-kernel MMD against
    x = torch.randn(z.shape) (:203, global torch CPU generator).  `kl` / `vkl` hold the MMD terms."""

    LAMBDA = 1000.0

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None,
                 force_dp=False):
        if world_size > 1 or force_dp:
            raise GMError("BIR-VAE's MMD couples every pair of rows of the batch: it does not shard on "
                          "the batch axis (run it on one GPU)")
        self.model, self.device, self.use_graph = model, device, use_graph
        enc, dec = model.encoder, model.decoder
        plist = [enc.linear.weight, enc.linear.bias, enc.mu.weight, enc.mu.bias,
                 dec.linear.weight, dec.linear.bias, dec.recon.weight, dec.recon.bias]
        self._dp_init(plist, 1, 0, None, False)
        self.fp = FlatParams(plist, device)
        fp = self.fp
        self.E1, self.MU = _Linear(fp, enc.linear), _Linear(fp, enc.mu)
        self.D1, self.D2 = _Linear(fp, dec.linear), _Linear(fp, dec.recon)
        self.Z, self.H = enc.mu.weight.shape
        self.I = enc.linear.weight.shape[1]
        self.set_var = float(model.set_var)
        self._common_init(device)

    def _alloc(self, B):
        if self._bufB == B:
            return
        dev, I, H, Z = self.device, self.I, self.H, self.Z
        z = lambda *s: torch.zeros(*s, device=dev)
        self.X, self.He, self.Mu, self.Zs = z(B, I), z(B, H), z(B, Z), z(B, Z)
        self.Xb = (self.X, z(B, I))
        self.Hdec, self.Xr, self.dA = z(B, H), z(B, I), z(B, I)
        self.dHdec, self.dZ, self.dZm, self.dHe = z(B, H), z(B, Z), z(B, Z), z(B, H)
        self.part, self.partm = z(B), z(B)
        self._sq_alloc(B)
        self._bufB = B
        self.graphs = {}

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)
        if getattr(self, "_prior_B", None) != B or "prior" not in self.stage[0]:
            self.prior_ring = torch.zeros(self.R, B, self.Z, device=self.device)
            for s in self.stage:
                s["prior"] = torch.zeros(self.R, B, self.Z).pin_memory()
            self._prior_B = B
            self.graphs = {}

    def _draw_chunk(self, s, sizes):
        import numpy as np
        Z = self.Z
        # model(images) -> reparameterize: np.random.normal(0, set_var, mu.shape).float(), batch after batch on
        # numpy's global generator: replayed in C for the whole chunk (NumpyReplay), else through numpy itself
        if not (NumpyReplay.available() and NumpyReplay.fill(self.set_var, s["eps"], self.B, Z, sizes)):
            for k, b in enumerate(sizes):
                e = np.random.normal(loc=0.0, scale=self.set_var, size=(b, Z))
                s["eps"][k].view(-1)[:b * Z].copy_(torch.from_numpy(e).float().view(-1))
        # maximum_mean_discrepancy: torch.randn(z.shape) -- a different generator, order-independent
        self._torch_normal_rows(s["prior"], sizes)

    def _upload_chunk(self, s, r, cnt):
        self.eps_ring[r:r + cnt].copy_(s["eps"][:cnt], non_blocking=True)
        self.prior_ring[r:r + cnt].copy_(s["prior"][:cnt], non_blocking=True)

    def _issue(self, st, t, b, train, pos=0, of=1):
        from . import ops_fused as of_
        R, B, Z = self.R, self.B, self.Z
        E1, MU, D1, D2 = self.E1, self.MU, self.D1, self.D2
        idx_slot = self._slot(t, 1, 0, R, B)
        eps_slot = self._slot(t, 1, 0, R, B * Z)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        recon_out, mmd_out = (self.recon, self.kl) if train else (self.vrecon, self.vkl)
        X, own, nxt = self._gather_plan(pos, of)
        if own:
            ops.gather_rows(self.data, self.idx_ring.view(-1), X, B=b, idx_slot=idx_slot, stream=st)
        ops.linear_fwd(X, E1.W, E1.b, self.He, "relu", M=b, stream=st)
        self._fwd_with_prefetch(st, t, 0, b, self.He, MU, self.Mu, "id", nxt)
        of_.bir_reparam(self.Mu, self.eps_ring.view(-1), self.Zs, b, Z, eps_slot=eps_slot, stream=st)
        ops.linear_fwd(self.Zs, D1.W, D1.b, self.Hdec, "relu", M=b, stream=st)
        part, n_part = self._recon_fwd(st, self.Hdec, D2, X, b)
        of_.bir_mmd(self.Zs, self.prior_ring.view(-1), self.partm, self.dZm if train else None, b, Z,
                   self.LAMBDA, prior_slot=eps_slot, stream=st)
        if train:
            sched_slot = self._slot(t, 1, 0, 0, 1)
            adam = dict(sched=self.sched, sched_slot=sched_slot) if self.fuse_adam else None
            dw2 = lambda a1, a2: ops.linear_bwd_dw_adam_pair(
                dict(dA=a1[0], X=a1[1], lin=a1[2], adam=adam, M=b),
                dict(dA=a2[0], X=a2[1], lin=a2[2], adam=adam, M=b),
                weight_decay=self.wd if adam is not None else 0.0, stream=st)
            # every dX reads a layer's weights BEFORE that layer's dW(+Adam) launch updates them
            ops.linear_bwd_dx(self.dA, D2.W, self.dHdec, below=self.Hdec, epi="relu", M=b, stream=st)
            # d loss / d z = decoder path + d(1000 * mmd)/dz ; z = mu + eps -> d/d mu is the same
            ops.linear_bwd_dx(self.dHdec, D1.W, self.dZ, M=b, add=self.dZm, add_scale=1.0, stream=st)
            dw2((self.dA, self.Hdec, D2), (self.dHdec, self.Zs, D1))
            ops.linear_bwd_dx(self.dZ, MU.W, self.dHe, below=self.He, epi="relu", M=b, stream=st)
            dw2((self.dZ, self.He, MU), (self.dHe, X, E1))
            self._optimizer_step(st, sched_slot)
        # reconstruction sum and 1000 * MMD in the step's last launch, which also carries the tick
        of_.sum_finalize2(part, n_part, recon_out, loss_slot, self.partm, b, mmd_out, loss_slot,
                          scale_b=self.LAMBDA, tick=self.ctr if self.use_graph else None, stream=st)


def validate_labels(labels, num_classes, error=GMError):
    """Host check of a dataset's classes, once per dataset and before any launch that reads them: integral values in
    [0, num_classes), else `error`.  Returns them as an int32 CPU tensor.  (The kernels index the label weights with
    these.)"""
    y = torch.as_tensor(labels).reshape(-1)
    if y.is_floating_point():
        if not bool(torch.isfinite(y).all()) or not bool((y == torch.round(y)).all()):
            raise error("class labels must be integers")
    elif y.dtype == torch.bool or y.is_complex():
        raise error("class labels must be integers (got %s)" % y.dtype)
    if y.numel() and (int(y.min()) < 0 or int(y.max()) >= num_classes):
        raise error("class labels must lie in [0, %d): found %d .. %d" % (num_classes, int(y.min()), int(y.max())))
    return y.to(torch.int32)


class CVAEEngine(VAEEngine):
    """The class-conditional VAE (cvae.py) on the VAE engine's batch: the encoder's and the decoder's first layers take
    E[:, y_m] in their forward epilogues (ops.linear_fwd_label, gm_vae_reparam_fwd_label), row m's class read through
    the batch's row of the index ring -- no gather of its own -- and one more launch (gm_label_grad_adam) forms both
    label weights' gradients by class and steps them with Adam.  9 launches per batch (the VAE's 8 + that one).
    One GPU only; the fused form of the VAE batch only (configure() refuses the toggles that would turn off fused
    Adam / paired weight gradients); the decoder's and the middle launches fall back to the VAE's generic forms
    outside their limits (Z > 32 or Z % 4 != 0, hidden width > 512)."""

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None,
                 force_dp=False):
        if world_size > 1 or force_dp:
            raise GMError("the CVAE engine runs on one GPU: data parallelism is not implemented for it")
        self.model, self.device, self.use_graph = model, device, use_graph
        enc, dec = model.encoder, model.decoder
        self.C = enc.label.weight.shape[1]
        if not 1 <= self.C <= 32:
            raise GMError("the CVAE engine supports 1 <= num_classes <= 32 (got %d)" % self.C)
        # each label weight is [its layer's width, C]: the kernels index E[n * C + c] for every output column n
        for lab, lin in ((enc.label, enc.linear), (dec.label, dec.linear)):
            if tuple(lab.weight.shape) != (lin.weight.shape[0], self.C):
                raise GMError("a label layer's weight must be [%d, %d] (its linear layer's width x num_classes), got %s"
                              % (lin.weight.shape[0], self.C, tuple(lab.weight.shape)))
        plist = [enc.linear.weight, enc.linear.bias,
                 (enc.mu.weight, enc.log_var.weight), (enc.mu.bias, enc.log_var.bias),
                 dec.linear.weight, dec.linear.bias, dec.recon.weight, dec.recon.bias,
                 enc.label.weight, dec.label.weight]
        self._dp_init(plist, 1, 0, None, False)
        self.fp = FlatParams(plist, device)
        fp = self.fp
        self.E1, self.D1, self.D2 = _Linear(fp, enc.linear), _Linear(fp, dec.linear), _Linear(fp, dec.recon)
        Z, H = enc.mu.weight.shape
        self.Z, self.H, self.I = Z, H, enc.linear.weight.shape[1]
        i_w = [i for i, p in enumerate(fp.params) if p is enc.mu.weight][0]
        i_b = [i for i, p in enumerate(fp.params) if p is enc.mu.bias][0]
        o_w, o_b = fp.offsets[i_w], fp.offsets[i_b]

        class _Packed:          # [mu ; log_var] as one 2Z x H layer
            W = fp.flat[o_w:o_w + 2 * Z * H].view(2 * Z, H)
            b = fp.flat[o_b:o_b + 2 * Z]
            gW = fp.grad[o_w:o_w + 2 * Z * H].view(2 * Z, H)
            gb = fp.grad[o_b:o_b + 2 * Z]
            mW, vW = fp.m[o_w:o_w + 2 * Z * H], fp.v[o_w:o_w + 2 * Z * H]
            mb, vb = fp.m[o_b:o_b + 2 * Z], fp.v[o_b:o_b + 2 * Z]
        self.ML = _Packed

        def label_views(p):     # (E, m, v) of a label weight [H, C]
            i = [k for k, q in enumerate(fp.params) if q is p][0]
            o = fp.offsets[i]
            return dict(E=fp.views[i], gE=fp.gviews[i], mE=fp.m[o:o + p.numel()].view(p.shape),
                        vE=fp.v[o:o + p.numel()].view(p.shape))
        self.LE, self.LD = label_views(enc.label.weight), label_views(dec.label.weight)
        self.labels = None
        self._common_init(device)

    def _data_key(self):
        return self.data.data_ptr(), self.labels.data_ptr()       # the graphs read the labels too

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        off = [f for f in ("fuse_adam", "pair_dw", "fin_in_dw", "fuse_reparam_bwd") if not getattr(self, f)]
        if off:
            raise GMError("the CVAE engine runs the fused VAE batch only (Adam in the weight-gradient epilogues, paired "
                          "weight gradients); these cannot be turned off for it: %s" % ", ".join(off))
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)

    def run_pass(self, data, perm, train, t0):
        """data: (images, labels) -- the labels an int32 device tensor that validate_labels has passed."""
        images, self.labels = data
        if self.labels.dtype != torch.int32 or self.labels.numel() != images.shape[0]:
            raise GMError("CVAE labels: one validated int32 class per image")
        return super().run_pass(images, perm, train, t0)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: CVAE.forward + losses (+ backward + Adam when train); VAEEngine._issue with the label
        terms."""
        from . import ops_fused as of_
        of = max(1, of)
        R, B, Z = self.R, self.B, self.Z
        E1, ML, D1, D2 = self.E1, self.ML, self.D1, self.D2
        idx_slot = self._slot(t, 1, 0, R, B)
        eps_slot = self._slot(t, 1, 0, R, B * Z)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        recon_out, kl_out = (self.recon, self.kl) if train else (self.vrecon, self.vkl)
        idx = self.idx_ring.view(-1)
        lab = ops.label_src(self.labels, idx, idx_slot)         # y_m = labels[idx_ring[slot][m]]
        X, own, nxt = self._gather_plan(pos, of)
        if own:
            ops.gather_rows(self.data, idx, X, B=b, idx_slot=idx_slot, stream=st)
        ops.linear_fwd_label(X, E1.W, E1.b, self.LE["E"], lab, self.He, "relu", M=b, stream=st)
        self._fwd_with_prefetch(st, t, 0, b, self.He, ML, self.ml, "id", nxt)
        eps_base = self.eps_ring.view(-1)
        if self.fuse_reparam_fwd and Z <= 32 and Z % 4 == 0:
            n_kl = of_.vae_reparam_fwd_label(self.ml, eps_base, self.Zs, self.part_kl, b, Z, D1.W, D1.b, self.Hdec,
                                             "relu", self.LD["E"], lab, eps_slot=eps_slot, stream=st)
        else:
            n_kl = of_.vae_reparam_wide(self.ml, eps_base, self.Zs, self.part_kl, b, Z, eps_slot=eps_slot, stream=st)
            ops.linear_fwd_label(self.Zs, D1.W, D1.b, self.LD["E"], lab, self.Hdec, "relu", M=b, stream=st)
        part, n_part = self._recon_fwd(st, self.Hdec, D2, X, b)
        if not train:
            of_.sum_finalize2(part, n_part, recon_out, loss_slot, self.part_kl, n_kl, kl_out, loss_slot,
                              tick=self.ctr if self.use_graph else None, stream=st)
            return
        adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
        ops.linear_bwd_dx(self.dA, D2.W, self.dHdec, below=self.Hdec, epi="relu", M=b, stream=st)
        mid = (self.fuse_bwd_mid and Z <= 32 and self.H % 4 == 0 and self.H <= 512 and D1.W.shape[0] == self.H
               and ML.W.shape[1] == self.H)
        if mid:
            of_.vae_bwd_mid(self.dHdec, D1.W, self.ml, eps_base, self.dml, ML.W, self.He, self.dHe, b,
                            eps_slot=eps_slot, stream=st)
        else:
            ops.linear_bwd_dx_reparam(self.dHdec, D1.W, self.dZ, self.ml, eps_base, self.dml, M=b,
                                      eps_slot=eps_slot, stream=st)
        ops.linear_bwd_dw_adam_pair(dict(dA=self.dA, X=self.Hdec, lin=D2, adam=adam, M=b),
                                    dict(dA=self.dHdec, X=self.Zs, lin=D1, adam=adam, M=b),
                                    weight_decay=self.wd, stream=st)
        if not mid:
            ops.linear_bwd_dx(self.dml, ML.W, self.dHe, below=self.He, epi="relu", M=b, stream=st)
        # both label weights: gradient by class (d loss / d pre-activation of the two conditioned layers) + Adam
        # (the gradients also land in the flat gradient buffer, like every other layer's)
        ops.label_grad_adam([dict(dPre=self.dHe, **self.LE), dict(dPre=self.dHdec, **self.LD)], lab, b, self.C,
                            adam=adam, weight_decay=self.wd, stream=st)
        ops.linear_bwd_dw_adam_pair_finalize(
            dict(dA=self.dHe, X=X, lin=E1, adam=adam, M=b), dict(dA=self.dml, X=self.He, lin=ML, adam=adam, M=b),
            dict(pa=part, na=n_part, out_a=recon_out, slot_a=loss_slot, pb=self.part_kl, nb=n_kl, out_b=kl_out,
                 slot_b=loss_slot, done=self.fin_done, tick=self.ctr if self.use_graph else None),
            weight_decay=self.wd, stream=st)


class DVAEEngine(VAEEngine):
    """The denoising VAE (dvae.py) on the VAE engine's batch.  Three differences, training batches only:
      * the batch's gathers are the corrupting ones (gm_gather_rows[_bits]_corrupt for a graph's first batch, the
        corrupting gather riding in the [mu | log_var] forward for the others), which write the clean rows to Xb and
        their corruption to the double-buffered Xcb;
      * the encoder's first layer reads the corrupted rows, in its forward and in its weight gradient;
      * nothing else: the reconstruction loss still reads the clean rows.
    Still 8 launches per batch.  The noise step of a training batch is ctr + nbase (+ 1 for the riding gather, which
    fills the NEXT batch): ctr is the engine's device counter, nbase a device word configure() writes from the
    trainer's count of training batches, so a graph captured in one train() call serves the next.  Validation batches
    are the VAE's, clean.  One GPU only."""

    one_gpu = "the DVAE engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        super().__init__(model, device, use_graph=use_graph)
        self._bind_trainer(trainer)                  # noise, level, seed and noise_steps are read from it

    def _alloc(self, B):
        if self._bufB == B:
            return
        super()._alloc(B)
        self.Xcb = (torch.zeros(B, self.I, device=self.device), torch.zeros(B, self.I, device=self.device))

    def _settings(self):
        tr = self.trainer
        return {"noise": tr.noise, "level": float(tr.level), "seed": int(tr.seed)}

    def _xc(self, X):
        return self.Xcb[0] if X is self.Xb[0] else self.Xcb[1]

    def _cargs(self, t, add):
        """The corruption of the training batch at ring step t (+ add)."""
        from . import ops_fused as of_
        tr = self.trainer
        return of_.corrupt_args(tr.noise, tr.level, tr.seed, **self._clock(t, True, add))

    def _encoder_rows(self, X, train):
        return self._xc(X) if train else X

    def _gather_own(self, st, t, lo, b, X, idx_slot, train):
        if not train:
            return super()._gather_own(st, t, lo, b, X, idx_slot, train)
        from . import ops_fused as of_
        of_.gather_rows_corrupt(self.data, self.idx_ring.view(-1)[lo:], X, self._xc(X), self._cargs(t, 0), B=b,
                                idx_slot=idx_slot, stream=st)

    def _fwd_with_prefetch(self, st, t, lo, b, x, lin, y, act, nxt, train=True):
        if not train or nxt is None:
            return super()._fwd_with_prefetch(st, t, lo, b, x, lin, y, act, nxt, train=train)
        from . import ops_fused as of_
        of_.linear_fwd_gather_corrupt(x, lin.W, lin.b, y, act, self.data, self.idx_ring.view(-1)[lo:], nxt,
                                      self._xc(nxt), self._cargs(t, 1), M=b, B=b,
                                      idx_slot=self._slot(t, 1, 1, self.R, self.B), stream=st)


class IWAEEngine(VAEEngine):
    """The importance-weighted autoencoder (iwae.py holds the contract) on the VAE engine's batch: the encoder runs on
    the batch's B rows, the decoder on its B k sample rows (image-major).  12 launches per training batch:
      1. encoder layer 1;  2. [mu | log_var], carrying the next batch's gather;  3. gm_iwae_sample (z, lp);
      4. decoder layer 1 on B k rows;  5. decoder output, sigmoid;  6. gm_iwae_weights (-L_k, ess, wn, weighted dA);
      7. decoder dX with relu;  8. dzdec = dHdec Wd1;  9. the decoder's paired dW + Adam with M = B k;
      10. gm_iwae_reduce (dml);  11. dX through [mu | log_var];  12. the encoder's paired dW + Adam, whose finalize
      block sums the per-image -L_k (-> `recon`) and ess / b (-> `kl`) and ticks the counter.
    A validation batch is launches 1-6 in evaluation mode and the two sums.  The noise step of a training batch is
    ctr + nbase (DVAEEngine's scheme), of a validation batch ctr (the batch's index in the pass).  One GPU only."""

    has_eps = False              # the noise is drawn on the device: no host eps ring
    one_gpu = "the IWAE engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        k = int(trainer.k)
        self._check_limits(model, k)
        super().__init__(model, device, use_graph=use_graph)
        self._bind_trainer(trainer)                  # seed and noise_steps are read from it
        self.k = k

    def _check_limits(self, model, k):
        """GMError unless k and the latent width fit the sampling kernels."""
        from ._lib import IWAE_MAX_K, IWAE_MAX_Z
        Z = model.encoder.mu.weight.shape[0]
        if not (1 <= k <= IWAE_MAX_K and 1 <= Z <= IWAE_MAX_Z):
            raise GMError("IWAEEngine: 1 <= k <= %d and 1 <= z_dim <= %d (got k=%d, z_dim=%d); IWAETrainer trains "
                          "these on the general path" % (IWAE_MAX_K, IWAE_MAX_Z, k, Z))

    def _alloc(self, B):
        if self._bufB == B:
            return
        dev, I, H, Z, k = self.device, self.I, self.H, self.Z, self.k
        Hd, Wh = self.D1.W.shape[0], self.ML.W.shape[0]          # Wh: the head's width (2 Z; CatVAEEngine: Z)
        z = lambda *s: torch.zeros(*s, device=dev)
        self.X, self.He, self.ml = z(B, I), z(B, H), z(B, Wh)
        self.Xb = (self.X, z(B, I))
        self.Zs, self.lp, self.wn = z(B * k, Z), z(B * k), z(B * k)
        self.Hdec, self.Xr, self.dA = z(B * k, Hd), z(B * k, I), z(B * k, I)
        self.dHdec, self.dzdec = z(B * k, Hd), z(B * k, Z)
        self.negL, self.essb = z(B), z(B)
        self.dml, self.dHe = z(B, Wh), z(B, H)
        self._bufB = B
        self.graphs = {}

    def _settings(self):
        return {"k": self.k, "seed": int(self.trainer.seed)}

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        k = int(self.trainer.k)
        if k != self.k:
            raise GMError("IWAETrainer.k changed after the engine was built (%d -> %d)" % (self.k, k))
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)

    def _noise(self, t, train):
        """The batch's noise stream: the training tag at the training clock, or the evaluation tag at the batch's index
        in the pass (_clock)."""
        from . import ops_fused as of_
        return of_.iwae_noise(self.trainer.seed, self._tags()[0 if train else 1], self.k, **self._clock(t, train))

    def _tags(self):
        """The noise stream's (training, evaluation) tags."""
        from ._lib import IWAE_TAG_EVAL, IWAE_TAG_TRAIN
        return IWAE_TAG_TRAIN, IWAE_TAG_EVAL

    def _sample(self, st, nz, b, t=0, train=True):
        """Launch 3: z and lp of the batch's b k sample rows (t, train: the batch's ring step and kind, for a
        subclass whose sampling depends on them)."""
        from . import ops_fused as of_
        of_.iwae_sample(self.ml, self.Zs, self.lp, nz, b, self.k, self.Z, stream=st)

    def _second_sum(self, b):
        """What the batch's second sum reads: (per-image buffer, scale) -- the mean effective sample size."""
        return self.essb, 1.0 / b

    def _reduce(self, st, nz, b, adam):
        """Launch 10: d loss / d [mu | lv] from dzdec and the weights."""
        from . import ops_fused as of_
        of_.iwae_reduce(self.ml, self.wn, self.dzdec, self.dml, nz, b, self.k, self.Z, stream=st)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: forward on b k sample rows + -L_k, ess (+ backward + Adam when train)."""
        from . import ops_fused as of_
        of = max(1, of)
        R, B, k = self.R, self.B, self.k
        E1, ML, D1, D2 = self.E1, self.ML, self.D1, self.D2
        idx_slot = self._slot(t, 1, 0, R, B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        loss_out, ess_out = (self.recon, self.kl) if train else (self.vrecon, self.vkl)
        tick = self.ctr if self.use_graph else None
        X, own, nxt = self._gather_plan(pos, of)
        if own:
            self._gather_own(st, t, 0, b, X, idx_slot, train)
        ops.linear_fwd(X, E1.W, E1.b, self.He, "relu", M=b, stream=st)
        self._fwd_with_prefetch(st, t, 0, b, self.He, ML, self.ml, "id", nxt, train=train)
        nz = self._noise(t, train)
        self._sample(st, nz, b, t, train)
        ops.linear_fwd(self.Zs, D1.W, D1.b, self.Hdec, "relu", M=b * k, stream=st)
        ops.linear_fwd(self.Hdec, D2.W, D2.b, self.Xr, "sigmoid", M=b * k, stream=st)
        of_.iwae_weights(X, self.Xr, self.lp, self.negL, self.essb, self.wn, b, k, dA=self.dA if train else None,
                         stream=st)
        sum_b, scale_b = self._second_sum(b)
        if not train:
            of_.sum_finalize2(self.negL, b, loss_out, loss_slot, sum_b, b, ess_out, loss_slot, scale_b=scale_b,
                              tick=tick, stream=st)
            return
        adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
        # every dX reads a layer's weights BEFORE that layer's dW(+Adam) launch updates them
        ops.linear_bwd_dx(self.dA, D2.W, self.dHdec, below=self.Hdec, epi="relu", M=b * k, stream=st)
        ops.linear_bwd_dx(self.dHdec, D1.W, self.dzdec, M=b * k, stream=st)
        ops.linear_bwd_dw_adam_pair(dict(dA=self.dA, X=self.Hdec, lin=D2, adam=adam, M=b * k),
                                    dict(dA=self.dHdec, X=self.Zs, lin=D1, adam=adam, M=b * k),
                                    weight_decay=self.wd, stream=st)
        self._reduce(st, nz, b, adam)
        ops.linear_bwd_dx(self.dml, ML.W, self.dHe, below=self.He, epi="relu", M=b, stream=st)
        ops.linear_bwd_dw_adam_pair_finalize(
            dict(dA=self.dHe, X=X, lin=E1, adam=adam, M=b), dict(dA=self.dml, X=self.He, lin=ML, adam=adam, M=b),
            dict(pa=self.negL, na=b, out_a=loss_out, slot_a=loss_slot, pb=sum_b, nb=b, scale_b=scale_b,
                 out_b=ess_out, slot_b=loss_slot, done=self.fin_done, tick=tick),
            weight_decay=self.wd, stream=st)


class NFVAEEngine(IWAEEngine):
    """The normalizing-flow VAE (nfvae.py holds the contract): IWAEEngine's batch with a chain of K planar layers between
    z_0 and the decoder.  13 launches per training batch: the IWAE's 12 with launch 3 replaced by gm_flow_sample (z_K,
    lp with the log-determinants) and launch 10 by gm_flow_reduce (dml and the flow's partial gradient blocks), and
    gm_flow_step (the blocks' sum, the constraint's backward, Adam on u, w, b at the batch's schedule slot) behind
    gm_flow_reduce, which is the last reader of the flow's parameters.  The flow's parameters, gradients and moments
    are views of the engine's flat buffers like every other parameter.  One GPU only."""

    one_gpu = "the NF-VAE engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        from ._lib import FLOW_MAX_K
        K = int(model.flow.u.shape[0])
        if not 1 <= K <= FLOW_MAX_K:
            raise GMError("NFVAEEngine: 1 <= num_flows <= %d (got %d); NFVAETrainer trains these on the general path"
                          % (FLOW_MAX_K, K))
        super().__init__(model, device, use_graph=use_graph, trainer=trainer)
        self.K = K
        fp, fl = self.fp, model.flow
        ix = [[i for i, p in enumerate(fp.params) if p is q][0] for q in (fl.u, fl.w, fl.b)]
        seg = lambda buf, i: buf[fp.offsets[i]:fp.offsets[i] + fp.params[i].numel()]
        self.FU, self.FW, self.Fb = (fp.views[i] for i in ix)
        self.Fgrads = tuple(seg(fp.grad, i) for i in ix)
        self.Fmoments = tuple(seg(buf, i) for i in ix for buf in (fp.m, fp.v))

    def _extra_params(self, model):
        fl = model.flow
        return [fl.u, fl.w, fl.b]

    def _settings(self):
        return dict(num_flows=self.K, **super()._settings())

    def _alloc(self, B):
        if self._bufB == B:
            return
        super()._alloc(B)
        from . import ops_fused as of_
        self.fpart = of_.flow_parts(B, self.K, device=self.device)

    def _flow(self):
        from . import ops_fused as of_
        return of_.flow_params(self.FU, self.FW, self.Fb)

    def _sample(self, st, nz, b, t=0, train=True):
        from . import ops_fused as of_
        of_.flow_sample(self.ml, self.Zs, self.lp, nz, self._flow(), b, self.k, self.Z, stream=st)

    def _reduce(self, st, nz, b, adam):
        from . import ops_fused as of_
        of_.flow_reduce(self.ml, self.wn, self.dzdec, self.dml, self.fpart, nz, self._flow(), b, self.k, self.Z,
                        stream=st)
        of_.flow_step(self.fpart, b, self.FU, self.FW, self.Fb, self.Fmoments, adam["sched"], adam["sched_slot"],
                      grads=self.Fgrads, weight_decay=self.wd, stream=st)


class IAFVAEEngine(IWAEEngine):
    """The inverse-autoregressive-flow VAE (iafvae.py holds the contract): IWAEEngine's batch with a chain of K masked
    conditioners between z_0 and the decoder, and the encoder's head widened to [mu ; log_var ; context] (2Z + C rows:
    launches 2, 11 and 12 carry the context and its gradient with no launch of their own).  13 launches per training
    batch: the IWAE's 12 with launch 3 replaced by gm_iaf_sample (z_K, lp with the log-determinants) and launch 10 by
    gm_iaf_reduce (d loss / d [mu | lv | h] and the flow's partial gradient blocks), and gm_iaf_step (the blocks' sum,
    the masks, Adam on W1, U, b1, W2, b2 at the batch's schedule slot) behind gm_iaf_reduce, which is the last reader of
    the flow's parameters.  The flow's parameters, gradients and moments are views of the engine's flat buffers like
    every other parameter.  One GPU only."""

    one_gpu = "the IAF-VAE engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        from .iafvae import _flow_stock, fused_sizes
        sizes = tuple(int(getattr(model, n, -1)) for n in ("z_dim", "num_flows", "flow_hidden", "context_dim"))
        if not (fused_sizes(*sizes) and _flow_stock(model)):
            raise GMError("IAFVAEEngine: the fused kernels take 2 <= z_dim <= 32, 1 <= num_flows <= 8, 4 <= flow_hidden "
                          "<= 64 in multiples of 4 and 0 <= context_dim <= 32 with IAFVAE's own flow (got %s); "
                          "IAFVAETrainer trains these on the general path" % (sizes,))
        self.K, self.F, self.C = sizes[1:]
        super().__init__(model, device, use_graph=use_graph, trainer=trainer)
        fp, fl = self.fp, model.flow
        self.Fparams, self.Fgrads, self.Fmoments = [], [], []
        seg = lambda buf, i: buf[fp.offsets[i]:fp.offsets[i] + fp.params[i].numel()]
        for q in fl.tensors():                                   # W1, U (None when C = 0), b1, W2, b2
            if q is None:
                self.Fparams.append(None), self.Fgrads.append(None), self.Fmoments.append(None)
                continue
            i = [j for j, p in enumerate(fp.params) if p is q][0]
            self.Fparams.append(fp.views[i])
            self.Fgrads.append(seg(fp.grad, i))
            self.Fmoments.append((seg(fp.m, i), seg(fp.v, i)))
        self.m_in = fl.m_in.to(device).contiguous()

    def _head(self, enc):
        lins = [enc.mu, enc.log_var] + ([enc.context] if hasattr(enc, "context") else [])
        return tuple(l.weight for l in lins), tuple(l.bias for l in lins), enc.mu.weight.shape[0]

    def _extra_params(self, model):
        return [p for p in model.flow.tensors() if p is not None]

    def _settings(self):
        return dict(num_flows=self.K, flow_hidden=self.F, context_dim=self.C, **super()._settings())

    def _graph_args(self):
        return (self.m_in.data_ptr(),)

    def _alloc(self, B):
        if self._bufB == B:
            return
        super()._alloc(B)
        from . import ops_fused as of_
        self.fpart = of_.iaf_parts(B, self.k, self.K, self.Z, self.F, self.C, device=self.device)

    def _flow(self):
        from . import ops_fused as of_
        return of_.iaf_params(*self.Fparams)

    def _sample(self, st, nz, b, t=0, train=True):
        from . import ops_fused as of_
        of_.iaf_sample(self.ml, self.Zs, self.lp, nz, self._flow(), b, self.k, self.Z, stream=st)

    def _reduce(self, st, nz, b, adam):
        from . import ops_fused as of_
        of_.iaf_reduce(self.ml, self.wn, self.dzdec, self.dml, self.fpart, nz, self._flow(), b, self.k, self.Z,
                       stream=st)
        of_.iaf_step(self.fpart, b, self.k, self.Fparams, self.m_in, self.Fmoments, adam["sched"], adam["sched_slot"],
                     grads=self.Fgrads, weight_decay=self.wd, stream=st)


class TCVAEEngine(IWAEEngine):
    """The beta-TCVAE (tcvae.py holds the contract): IWAEEngine's 12-launch batch at k = 1 with
    launch 3 replaced by gm_tc_sample (z, lp = -(alpha mi + beta tc + gamma dwkl) from every pair of the batch, the two
    logsumexp records and the per-image tc) and launch 10 by gm_tc_reduce (d loss / d [mu | lv] through the sample and
    through every partner's parameters).  The finalize block sums -log w (-> `recon`) and tc / b (-> `kl`).  log(N b) is
    a launch argument: N the trainer's dataset_size for a training batch, the pass's own dataset for a validation batch
    (a graph is keyed by its batch size, its kind and its dataset, so each holds one value).  One GPU only."""

    one_gpu = "the TCVAE engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        super().__init__(model, device, use_graph=use_graph, trainer=trainer)

    def _check_limits(self, model, k):
        from ._lib import IWAE_MAX_Z
        Z = model.encoder.mu.weight.shape[0]
        if k != 1 or not 1 <= Z <= IWAE_MAX_Z:
            raise GMError("TCVAEEngine: k = 1 and 1 <= z_dim <= %d (got k=%d, z_dim=%d); TCVAETrainer trains these on "
                          "the general path" % (IWAE_MAX_Z, k, Z))

    def _alloc(self, B):
        if self._bufB == B:
            return
        super()._alloc(B)
        from . import ops_fused as of_
        self.lse_joint, self.lse_dim, self.tcrow = of_.tc_records(B, self.Z, device=self.device)

    def _settings(self):
        tr = self.trainer
        return dict(alpha=float(tr.alpha), beta=float(tr.beta), gamma=float(tr.gamma),
                    dataset_size=int(tr.dataset_size), **super()._settings())

    def _second_sum(self, b):
        return self.tcrow, 1.0 / b

    def _coef(self):
        tr = self.trainer
        return float(tr.alpha), float(tr.beta), float(tr.gamma)

    def _log_nm(self, b, train):
        """log(N b): N the training set's size (the trainer's dataset_size) or the size of the pass's own dataset."""
        import math
        n = int(self.trainer.dataset_size) if train else int(self.data.shape[0])
        return math.log(n * b)

    def _sample(self, st, nz, b, t=0, train=True):
        from . import ops_fused as of_
        of_.tc_sample(self.ml, self.Zs, self.lp, self.lse_joint, self.lse_dim, self.tcrow, nz, *self._coef(),
                      self._log_nm(b, train), b, self.Z, stream=st)

    def _reduce(self, st, nz, b, adam):
        from . import ops_fused as of_
        of_.tc_reduce(self.ml, self.Zs, self.lse_joint, self.lse_dim, self.wn, self.dzdec, self.dml, nz, *self._coef(),
                      b, self.Z, stream=st)


class CatVAEEngine(IWAEEngine):
    """The categorical VAE (catvae.py holds the contract): IWAEEngine's 12-launch batch at k = 1 with the `logits` layer
    (width N C) as the encoder's head instead of the packed [mu | log_var], launch 3 replaced by gm_cat_sample (the
    relaxed sample, or the straight-through one-hot with hard=True and in every validation batch; lp = -KL and the
    per-image KL) and launch 10 by gm_cat_reduce (d loss / d logits, the Gumbel noise regenerated).  The finalize block
    sums -L (-> `recon`) and the per-image KL (-> `kl`), scale 1.  The temperature of training batch t is entry t of a
    device table laid out and indexed like the Adam schedule (one float per batch of the train() call), so a replayed
    graph needs no host update; validation reads none.  One GPU only."""

    one_gpu = "the categorical VAE engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        self.N, self.C = int(model.num_vars), int(model.num_classes)
        super().__init__(model, device, use_graph=use_graph, trainer=trainer)

    def _check_limits(self, model, k):
        from ._lib import CAT_MAX_C, CAT_MAX_NC, CAT_MIN_C
        if k != 1 or not (self.N >= 1 and CAT_MIN_C <= self.C <= CAT_MAX_C and self.N * self.C <= CAT_MAX_NC):
            raise GMError("CatVAEEngine: k = 1, %d <= num_classes <= %d and num_vars * num_classes <= %d (got k=%d, "
                          "num_vars=%d, num_classes=%d); CatVAETrainer trains these on the general path"
                          % (CAT_MIN_C, CAT_MAX_C, CAT_MAX_NC, k, self.N, self.C))

    def _head(self, enc):
        return (enc.logits.weight,), (enc.logits.bias,), enc.logits.weight.shape[0]

    def _tags(self):
        from ._lib import CAT_TAG_EVAL, CAT_TAG_TRAIN
        return CAT_TAG_TRAIN, CAT_TAG_EVAL

    def _alloc(self, B):
        if self._bufB == B:
            return
        super()._alloc(B)
        self.klrow = torch.zeros(B, device=self.device)

    def _settings(self):
        tr = self.trainer
        now = super()._settings()
        now.update(num_vars=self.N, num_classes=self.C, hard=bool(tr.hard), tau0=float(tr.tau0),
                   tau_min=float(tr.tau_min), anneal_rate=float(tr.anneal_rate))
        return now

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        from .catvae import temperature
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)
        tr = self.trainer
        t0 = int(tr.noise_steps)
        taus = np.array([temperature(t0 + i, tr.tau0, tr.tau_min, tr.anneal_rate)
                         for i in range(max(1, n_train_steps))], dtype=np.float32)
        self._moved = False
        self.tau_tab = GANEngine._pbuf(self, "tau", taus)
        if self._moved:
            self.graphs = {}

    def _second_sum(self, b):
        return self.klrow, 1.0

    def _sample(self, st, nz, b, t=0, train=True):
        from . import ops_fused as of_
        from ._lib import CAT_RELAXED, CAT_ST
        relaxed = train and not self.trainer.hard
        of_.cat_sample(self.ml, self.Zs, self.lp, nz, b, 1, self.N, self.C, CAT_RELAXED if relaxed else CAT_ST,
                       tau_tab=self.tau_tab if relaxed else None,
                       tau_slot=self._slot(t, 1, 0, 0, 1) if relaxed else ops.slot(), kl=self.klrow, stream=st)

    def _reduce(self, st, nz, b, adam):
        from . import ops_fused as of_
        of_.cat_reduce(self.ml, self.dzdec, self.wn, self.dml, nz, b, self.N, self.C, tau_tab=self.tau_tab,
                       tau_slot=adam["sched_slot"], stream=st)


class VQVAEEngine(IWAEEngine):
    """The vector-quantised VAE (vqvae.py holds the contract): IWAEEngine's 12-launch batch at k = 1 with the `embed`
    layer (width N D) as the encoder's head, launch 3 replaced by gm_vq_quantise (z_q = the nearest codebook rows, the
    codes, qerr and lp = -(1 + beta) qerr; nothing is drawn) and launch 10 by gm_vq_reduce (d loss / d z_e: the decoder's
    input gradient straight through plus the commitment term), and gm_vq_step (n_k, s_k, the codebook's gradient and
    Adam at the batch's schedule slot) behind gm_vq_reduce, which is the last reader of the codebook: 13 launches.  The
    finalize block sums -log w (-> `recon`) and qerr (-> `kl`), scale 1.  The codebook, its gradient and its moments are
    views of the engine's flat buffers like every other parameter.  Training and validation write separate `codes`
    buffers; `usage` [K] counts the epoch's assignments (run_pass zeroes it before a training pass, gm_vq_step adds to
    it, so a replayed graph needs no host update).  One GPU only."""

    one_gpu = "the VQ-VAE engine"

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        self.N, self.D, self.K = int(model.num_vars), int(model.code_dim), int(model.num_codes)
        super().__init__(model, device, use_graph=use_graph, trainer=trainer)
        fp, cb = self.fp, model.codebook.weight
        i = [j for j, p in enumerate(fp.params) if p is cb][0]
        seg = lambda buf: buf[fp.offsets[i]:fp.offsets[i] + cb.numel()]
        self.CB, self.CBgrad, self.CBmoments = fp.views[i], seg(fp.grad), (seg(fp.m), seg(fp.v))
        self.nk = torch.zeros(self.K, dtype=torch.int32, device=device)
        self.usage = torch.zeros(self.K, dtype=torch.int32, device=device)

    def _check_limits(self, model, k):
        from . import ops_fused as of_
        if k != 1 or not of_.vq_fused_sizes(self.N, self.D, self.K):
            raise GMError("VQVAEEngine: k = 1 and (num_vars, code_dim, num_codes) inside the quantisation kernels' limits "
                          "(got k=%d, %d, %d, %d); VQVAETrainer trains these on the general path"
                          % (k, self.N, self.D, self.K))

    def _head(self, enc):
        return (enc.embed.weight,), (enc.embed.bias,), enc.embed.weight.shape[0]

    def _extra_params(self, model):
        return [model.codebook.weight]

    def _alloc(self, B):
        if self._bufB == B:
            return
        super()._alloc(B)
        self.qerr = torch.zeros(B, device=self.device)
        self.codes_train = torch.zeros(B, self.N, dtype=torch.int32, device=self.device)
        self.codes_val = torch.zeros(B, self.N, dtype=torch.int32, device=self.device)

    def _settings(self):
        return dict(num_vars=self.N, code_dim=self.D, num_codes=self.K, beta=float(self.trainer.beta))

    def _noise(self, t, train):
        return None                                  # nothing is drawn

    def run_pass(self, data, perm, train, t0):
        if train:
            self.usage.zero_()
        return super().run_pass(data, perm, train, t0)

    def _second_sum(self, b):
        return self.qerr, 1.0

    def _sample(self, st, nz, b, t=0, train=True):
        from . import ops_fused as of_
        of_.vq_quantise(self.ml, self.CB, self.Zs, self.codes_train if train else self.codes_val, self.qerr, self.lp,
                        self.trainer.beta, b, self.N, self.D, stream=st)

    def _reduce(self, st, nz, b, adam):
        from . import ops_fused as of_
        of_.vq_reduce(self.ml, self.CB, self.codes_train, self.dzdec, self.wn, self.dml, self.trainer.beta, b, self.N,
                      self.D, stream=st)
        of_.vq_step(self.ml, self.codes_train, self.CB, b, self.N, self.D, moments=self.CBmoments, sched=adam["sched"],
                    sched_slot=adam["sched_slot"], grad=self.CBgrad, nk=self.nk, usage=self.usage,
                    weight_decay=self.wd, stream=st)


def aae_fused_ok(model):
    """True iff an AAE's shapes fit the fused kernels (gm_aae.hip): 1 <= Z <= 32 with Z % 4 == 0, hidden width <= 512,
    the decoder's and the discriminator's hidden widths equal to the encoder's, one discriminator output."""
    enc, dec, dis = model.encoder, model.decoder, model.discriminator
    Z, H = enc.z.weight.shape
    return (0 < Z <= 32 and Z % 4 == 0 and 0 < H <= 512 and tuple(enc.linear.weight.shape)[0] == H
            and tuple(dec.linear.weight.shape) == (H, Z) and tuple(dis.linear.weight.shape) == (H, Z)
            and tuple(dis.discriminate.weight.shape) == (1, H) and dec.recon.weight.shape[1] == H)


class AAEEngine(VAEEngine):
    """The adversarial autoencoder (aae.py) on the VAE engine's batch: three phases per batch, in this order.
      1. reconstruction: the AE's forward and backward on the existing launches, Adam(AE) in the weight-gradient
         epilogues (gradients: the flat gradient buffer's encoder / decoder segments);
      2. discriminator: the encoder forward again (its weights just changed), then gm_aae_critic_step on the batch's
         prior rows (torch.randn(b, Z), host-replayed into the prior ring) and the encoder rows -- D's gradient in the
         flat gradient buffer's discriminator segment, Adam(D) in the same launches;
      3. generator: gm_aae_gen_mid with D as phase 2 left it, then the encoder's paired weight gradients with the
         G optimizer's own moments and schedule (gradients: `gG`), the loss sums and the counter tick.
    One GPU only; the fused shapes only (aae_fused_ok) -- the trainer takes the general path outside them."""

    has_eps = False
    fused_ok = staticmethod(aae_fused_ok)

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False):
        if world_size > 1 or force_dp:
            raise GMError("the AAE engine runs on one GPU: data parallelism is not implemented for it")
        if not aae_fused_ok(model):
            raise GMError("AAEEngine: shapes outside the fused kernels' limits (Z <= 32, Z % 4 == 0, H <= 512, equal "
                          "hidden widths); AAETrainer trains these on the general path")
        self.model, self.device, self.use_graph = model, device, use_graph
        enc, dec, dis = model.encoder, model.decoder, model.discriminator
        plist = [enc.linear.weight, enc.linear.bias, enc.z.weight, enc.z.bias,
                 dec.linear.weight, dec.linear.bias, dec.recon.weight, dec.recon.bias,
                 dis.linear.weight, dis.linear.bias, dis.discriminate.weight, dis.discriminate.bias]
        self._dp_init(plist, 1, 0, None, False)
        self.fp = FlatParams(plist, device)
        fp = self.fp
        self.E1, self.EZ = _Linear(fp, enc.linear), _Linear(fp, enc.z)
        self.D1, self.D2 = _Linear(fp, dec.linear), _Linear(fp, dec.recon)
        self.C1, self.C2 = _Linear(fp, dis.linear), _Linear(fp, dis.discriminate)
        self.Z, self.H = enc.z.weight.shape
        self.I = enc.linear.weight.shape[1]
        # the generator phase's optimizer: its own moments and its own gradient buffer over the encoder's tensors
        self.gG, self.mG, self.vG = (torch.zeros(fp.n, device=device) for _ in range(3))
        self.G1, self.GZ = self._g_linear(enc.linear), self._g_linear(enc.z)
        self._drawing = True
        self._common_init(device)

    def _g_linear(self, lin):
        g = _Linear(self.fp, lin, m=self.mG, v=self.vG)
        ow = self.fp.offsets[[i for i, p in enumerate(self.fp.params) if p is lin.weight][0]]
        ob = self.fp.offsets[[i for i, p in enumerate(self.fp.params) if p is lin.bias][0]]
        g.gW = self.gG[ow:ow + lin.weight.numel()].view(lin.weight.shape)
        g.gb = self.gG[ob:ob + lin.bias.numel()]
        return g

    def phase_grads(self):
        """The three phases' gradients of the last training batch: {"ae": 8 tensors, "d": 4, "g": 4}, keyed by the
        model's state_dict names (views of the engine's buffers)."""
        names = {id(p): n for n, p in self.model.named_parameters()}
        out = {"ae": {}, "d": {}, "g": {}}
        for p, gv in zip(self.fp.params, self.fp.gviews):
            n = names[id(p)]
            out["d" if n.startswith("discriminator.") else "ae"][n] = gv
        for pre, g in (("encoder.linear.", self.G1), ("encoder.z.", self.GZ)):
            out["g"][pre + "weight"], out["g"][pre + "bias"] = g.gW, g.gb
        return out

    def _alloc(self, B):
        if self._bufB == B:
            return
        dev, I, H, Z = self.device, self.I, self.H, self.Z
        z = lambda *s: torch.zeros(*s, device=dev)
        self.X, self.He, self.Zs = z(B, I), z(B, H), z(B, Z)
        self.Xb = (self.X, z(B, I))
        self.Hdec, self.Xr, self.dA = z(B, H), z(B, I), z(B, I)
        self.dHdec, self.dZ, self.dHe = z(B, H), z(B, Z), z(B, H)
        self.part = z(B)
        self._sq_alloc(B)
        # regularization phase: the encoder's rows after phase 1, the generator's dz / dHe and its row losses
        self.He2, self.Zf, self.dZg, self.dHeg, self.gpart = z(B, H), z(B, Z), z(B, Z), z(B, H), z(B)
        from . import ops_fused as of_
        self.ws = of_.aae_critic_workspace(B, Z, H, dev)
        self._bufB = B
        self.graphs = {}

    def configure(self, B, n_train_steps, lr, weight_decay, D_lr=2e-4, G_lr=2e-4, resume=None):
        if resume is not None and resume.get("config") is not None and not resume.get("lenient", False):
            saved = resume["config"]
            now = {"D_lr": float(D_lr), "G_lr": float(G_lr)}
            diff = {k: (saved[k], now[k]) for k in now if k in saved and saved[k] != now[k]}
            if diff:
                raise GMError("checkpoint was written by a run with different settings (saved, now): %s; "
                              "load_checkpoint(path, strict=False) overrides" % diff)
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)
        self.run_config.update(D_lr=float(D_lr), G_lr=float(G_lr))
        self.gG.zero_()
        self.mG.zero_()
        self.vG.zero_()
        if resume is not None:
            if resume["mG"].numel() != self.mG.numel():
                raise GMError("checkpoint optimizer state does not match this model")
            self.mG.copy_(resume["mG"]); self.vG.copy_(resume["vG"])
        n = max(1, n_train_steps)
        self.sched_D = GANEngine._pbuf(self, "sched_D", ops.adam_schedule(D_lr, n, start=self.step0 + 1))
        self.sched_G = GANEngine._pbuf(self, "sched_G", ops.adam_schedule(G_lr, n, start=self.step0 + 1))
        self.dloss = GANEngine._pbuf(self, "dloss", n)
        self.gloss = GANEngine._pbuf(self, "gloss", n)
        if getattr(self, "_prior_B", None) != B or "prior" not in self.stage[0]:
            self.prior_ring = torch.zeros(self.R, B, self.Z, device=self.device)
            for s in self.stage:
                s["prior"] = torch.zeros(self.R, B, self.Z).pin_memory()
            self._prior_B = B
            self._moved = True
        if self._moved:
            self.graphs = {}

    def optim_state(self):
        st = super().optim_state()
        # one Adam step per batch for each of the three optimizers: their step counts are equal
        st.update(mG=self.mG.detach().cpu().clone(), vG=self.vG.detach().cpu().clone(),
                  steps={"AE": st["step"], "D": st["step"], "G": st["step"]})
        return st

    def run_pass(self, data, perm, train, t0):
        self._drawing = bool(train)                  # validation draws nothing (reconstruction loss only)
        return super().run_pass(data, perm, train, t0)

    def _draw_chunk(self, s, sizes):
        if self._drawing:                            # train_D: torch.randn(b, z_dim), the batch's only draw
            self._torch_normal_rows(s["prior"], sizes)

    def _upload_chunk(self, s, r, cnt):
        if self._drawing:
            self.prior_ring[r:r + cnt].copy_(s["prior"][:cnt], non_blocking=True)

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: reconstruction (+ when training: backward + Adam(AE), the critic step, the generator
        step)."""
        from . import ops_fused as of_
        R, B, Z = self.R, self.B, self.Z
        E1, EZ, D1, D2, C1, C2 = self.E1, self.EZ, self.D1, self.D2, self.C1, self.C2
        idx_slot = self._slot(t, 1, 0, R, B)
        prior_slot = self._slot(t, 1, 0, R, B * Z)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        tick = self.ctr if self.use_graph else None
        X, own, nxt = self._gather_plan(pos, of)
        if own:
            ops.gather_rows(self.data, self.idx_ring.view(-1), X, B=b, idx_slot=idx_slot, stream=st)
        # ---- 1. reconstruction: sum (x - decoder(encoder(x)))^2, Adam(AE)
        ops.linear_fwd(X, E1.W, E1.b, self.He, "relu", M=b, stream=st)
        self._fwd_with_prefetch(st, t, 0, b, self.He, EZ, self.Zs, "id", nxt)
        ops.linear_fwd(self.Zs, D1.W, D1.b, self.Hdec, "relu", M=b, stream=st)
        part, n_part = self._recon_fwd(st, self.Hdec, D2, X, b)
        if not train:
            of_.sum_finalize(part, n_part, self.vrecon, out_slot=loss_slot, tick=tick, stream=st)
            return
        sched_slot = self._slot(t, 1, 0, 0, 1)
        ae = dict(sched=self.sched, sched_slot=sched_slot)
        pair = lambda a1, a2: ops.linear_bwd_dw_adam_pair(
            dict(dA=a1[0], X=a1[1], lin=a1[2], adam=ae, M=b), dict(dA=a2[0], X=a2[1], lin=a2[2], adam=ae, M=b),
            weight_decay=self.wd, stream=st)
        # every dX reads a layer's weights BEFORE that layer's dW(+Adam) launch updates them
        ops.linear_bwd_dx(self.dA, D2.W, self.dHdec, below=self.Hdec, epi="relu", M=b, stream=st)
        ops.linear_bwd_dx(self.dHdec, D1.W, self.dZ, M=b, stream=st)
        pair((self.dA, self.Hdec, D2), (self.dHdec, self.Zs, D1))
        ops.linear_bwd_dx(self.dZ, EZ.W, self.dHe, below=self.He, epi="relu", M=b, stream=st)
        pair((self.dHe, X, E1), (self.dZ, self.He, EZ))
        # ---- 2. discriminator on z_real (prior ring) and z_fake = encoder(x) with the stepped encoder, Adam(D)
        ops.linear_fwd(X, E1.W, E1.b, self.He2, "relu", M=b, stream=st)
        ops.linear_fwd(self.He2, EZ.W, EZ.b, self.Zf, "id", M=b, stream=st)
        of_.aae_critic_step(self.prior_ring.view(-1), self.Zf, b, C1.W, C1.b, C2.W, C2.b, self.ws,
                            grads=(C1.gW, C1.gb, C2.gW, C2.gb), adam=dict(sched=self.sched_D, sched_slot=sched_slot),
                            moments=(C1.mW, C1.vW, C1.mb, C1.vb, C2.mW, C2.vW, C2.mb, C2.vb), loss_out=self.dloss,
                            real_slot=prior_slot, loss_slot=loss_slot, stream=st)
        # ---- 3. generator: -mean(log(D(encoder(x)) + 1e-8)) through the stepped D (the encoder is unchanged since 2)
        of_.aae_gen_mid(self.Zf, self.He2, C1.W, C1.b, C2.W, C2.b, EZ.W, self.dZg, self.dHeg, self.gpart, b, stream=st)
        gadam = dict(sched=self.sched_G, sched_slot=sched_slot)
        # the batch's LAST launch: the encoder's weight gradients + Adam(G), both loss sums, the counter tick
        ops.linear_bwd_dw_adam_pair_finalize(
            dict(dA=self.dHeg, X=X, lin=self.G1, adam=gadam, M=b), dict(dA=self.dZg, X=self.He2, lin=self.GZ,
                                                                         adam=gadam, M=b),
            dict(pa=part, na=n_part, out_a=self.recon, slot_a=loss_slot, pb=self.gpart, nb=b, scale_b=1.0 / b,
                 out_b=self.gloss, slot_b=loss_slot, done=self.fin_done, tick=tick),
            weight_decay=0.0, stream=st)
