"""What the engines of the one-network models share (made.py, maf.py, realnvp.py, ddpm.py, rbm.py, gmmn.py, flowmatch.py,
swg.py): one network, one Adam, noise drawn on the device from a counter, all on VAEEngine's epoch machinery.
OneNetEngine is the set-up (constructor prologue, the guard around the batch buffers); on top of it the two step bodies
that more than one model runs: TimeRegressionEngine (DDPM, flow matching) and GeneratorMatchEngine (GMMN, SWG).  A new
model writes its docstring (the launch list), one_gpu, fused_ok, refusal, _params, _setup, _buffers, _issue and, for
settings of its own, _settings, _graph_args and configure."""
import numpy as np
import torch

from . import ops
from ._lib import GMError
from .engine import VAEEngine, _align4, _Linear


class OneNetEngine(VAEEngine):
    """A one-GPU engine over a parameter list of its own, with no host noise ring.  A subclass declares fused_ok (the
    model's fused-path test), refusal (the words of the refusal of any other model: ("DDPM", "ddpm.DDPM", "Denoiser")),
    binds_trainer, and supplies _params(model) -> the parameters in flat order, _setup(model) -> the _Linear views and
    sizes, and _buffers(B) -> the batch buffers."""

    has_eps = False
    fused_ok = None             # staticmethod(<module>.<model>_fused_ok)
    refusal = None              # (name, the stock model, what of it must be unchanged)
    binds_trainer = True        # reads seed, settings and noise_steps from its trainer (MADEEngine draws no noise)

    def __init__(self, model, device, use_graph=True, world_size=1, rank=0, process_group=None, force_dp=False,
                 trainer=None):
        self._refuse_dp(world_size, force_dp)
        if not self.fused_ok(model):
            raise GMError("%sEngine: the model is not %s with its %s unchanged; %sTrainer trains such models on the "
                          "general path" % (self.refusal + self.refusal[:1]))
        self._init_flat(model, device, use_graph, self._params(model))
        if self.binds_trainer:
            self._bind_trainer(trainer)
        self._setup(model)

    def _alloc_key(self, B):
        """What the batch buffers were sized by (SWGEngine: the number of projections too)."""
        return B

    def _alloc(self, B):
        key = self._alloc_key(B)
        if self._bufB == key:
            return
        self._buffers(B)
        self._bufB = key
        self.graphs = {}


class TimeRegressionEngine(OneNetEngine):
    """A time-conditioned three-layer regression: the network `net` of the model (linear, hidden, out) on [x_t | temb]
    against a target the first launch forms with x_t.  10 launches per training batch: 1. the subclass's gather-and-
    sample;  2.-4. the three forwards;  5. gm_ddpm_loss (dA, row partials);  6. dH2 = dA Wout [H2 > 0];  7. dH1 =
    dH2 Whid [H1 > 0];  8. the out / hidden weight gradients + Adam as a pair;  9. the first layer's weight gradient +
    Adam;  10. the loss sum with the counter tick.  A subclass names net, its table buffers, the ops_fused builders of
    the table and noise arguments, the target and step buffers (and further per-row buffers), and supplies
    _gather_sample and _settings."""

    net = None                  # the model's attribute holding the three layers
    tables = ()                 # the model's table buffers: launch arguments of the graphs
    table_builder = noise_builder = None
    target, steps, rows = None, None, ()

    def _params(self, model):
        n = getattr(model, self.net)
        return [n.linear.weight, n.linear.bias, n.hidden.weight, n.hidden.bias, n.out.weight, n.out.bias]

    def _setup(self, model):
        n = getattr(model, self.net)
        self.L1, self.L2, self.L3 = _Linear(self.fp, n.linear), _Linear(self.fp, n.hidden), _Linear(self.fp, n.out)
        self.I, self.E, self.T, self.H = model.image_size, model.time_dim, model.T, n.linear.weight.shape[0]

    def _buffers(self, B):
        I, E, H = self.I, self.E, self.H
        z = lambda *s: torch.zeros(*s, device=self.device)
        self.X, self.Xin_full = z(B, I), z(B, _align4(I + E))
        self.Xin = self.Xin_full[:, :I + E]          # the first layer's operand: K = I + E, rows _align4(I + E) apart
        setattr(self, self.target, z(B, I))
        setattr(self, self.steps, torch.zeros(B, dtype=torch.int32, device=self.device))
        self.H1, self.H2, self.Out = z(B, H), z(B, H), z(B, I)
        self.dA, self.dH2, self.dH1 = z(B, I), z(B, H), z(B, H)
        for name in self.rows + ("part",):
            setattr(self, name, z(B))

    def _graph_args(self):
        return tuple(getattr(self.model, n).data_ptr() for n in self.tables)     # launch arguments of the graphs

    def configure(self, B, n_train_steps, lr, weight_decay, resume=None):
        super().configure(B, n_train_steps, lr, weight_decay, resume=resume)
        from . import ops_fused as of_
        self.tab = getattr(of_, self.table_builder)(*(getattr(self.model, n) for n in self.tables))

    def _noise(self, t, train):
        from . import ops_fused as of_
        return getattr(of_, self.noise_builder)(self.trainer.seed, train, **self._clock(t, train))

    def _issue(self, st, t, b, train, pos=0, of=1):
        """One batch of size b: the sample, forward, the regression loss (+ backward + Adam when train)."""
        from . import ops_fused as of_
        L1, L2, L3 = self.L1, self.L2, self.L3
        idx_slot = self._slot(t, 1, 0, self.R, self.B)
        loss_slot = self._slot(t, 1, 0, 0, 1)
        self._gather_sample(st, b, self._noise(t, train), idx_slot)
        ops.linear_fwd(self.Xin, L1.W, L1.b, self.H1, "relu", M=b, stream=st)
        ops.linear_fwd(self.H1, L2.W, L2.b, self.H2, "relu", M=b, stream=st)
        ops.linear_fwd(self.H2, L3.W, L3.b, self.Out, "id", M=b, stream=st)
        scale = float(np.float32(1.0 / (b * self.I)))
        of_.ddpm_loss(self.Out, getattr(self, self.target), self.part, b, scale, dA=self.dA if train else None,
                      stream=st)
        if train:
            adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
            # every dX reads a layer's weights BEFORE that layer's dW(+Adam) launch updates them
            ops.linear_bwd_dx(self.dA, L3.W, self.dH2, below=self.H2, epi="relu", M=b, stream=st)
            ops.linear_bwd_dx(self.dH2, L2.W, self.dH1, below=self.H1, epi="relu", M=b, stream=st)
            ops.linear_bwd_dw_adam_pair(dict(dA=self.dA, X=self.H2, lin=L3, adam=adam, M=b),
                                        dict(dA=self.dH2, X=self.H1, lin=L2, adam=adam, M=b),
                                        weight_decay=self.wd, stream=st)
            ops.linear_bwd_dw_adam(self.dH1, self.Xin, L1, adam, M=b, weight_decay=self.wd, stream=st)
        of_.sum_finalize(self.part, b, self.recon if train else self.vrecon, scale=scale, out_slot=loss_slot,
                         tick=self.ctr if self.use_graph else None, stream=st)


class GeneratorMatchEngine(OneNetEngine):
    """trainers.Generator trained without a critic on a statistic between a batch of its samples X and a batch of
    images Y, stacked as R = [X; Y].  A subclass's _issue is _forward (gather into the lower half of R, the prior, the
    two generator forwards), its statistic leaving the loss in lossf and, when training, the gradient entering
    `generate` in dA, then _tail (when training dH and the two weight gradients + Adam as a pair; the loss record).  It
    names the ops_fused builder of the prior's noise and its (training, validation) tags."""

    noise_builder, tags = None, None

    def _params(self, model):
        g = model.G
        return [g.linear.weight, g.linear.bias, g.generate.weight, g.generate.bias]

    def _setup(self, model):
        self.L1, self.L2 = _Linear(self.fp, model.G.linear), _Linear(self.fp, model.G.generate)
        self.I, self.H, self.Z = model.image_size, model.hidden_dim, model.z_dim

    def _forward(self, st, t, b, train):
        """Launches 1-4: Y, z, X.  Returns (X, Y), views of R's halves."""
        from . import ops_fused as of_
        L1, L2 = self.L1, self.L2
        X, Y = self.Rb[:b], self.Rb[b:2 * b]
        ops.gather_rows(self.data, self.idx_ring.view(-1), Y, B=b, idx_slot=self._slot(t, 1, 0, self.R, self.B),
                        stream=st)
        noise = getattr(of_, self.noise_builder)(self.trainer.seed, self.tags[0 if train else 1],
                                                 **self._clock(t, train))
        of_.gmmn_prior(self.Zb, noise, B=b, Z=self.Z, stream=st)
        ops.linear_fwd(self.Zb, L1.W, L1.b, self.Hg, "relu", M=b, stream=st)
        ops.linear_fwd(self.Hg, L2.W, L2.b, X, "sigmoid", M=b, stream=st)
        return X, Y

    def _tail(self, st, t, b, train):
        """The last launches: dH and the pair when training, the loss record."""
        from . import ops_fused as of_
        L1, L2 = self.L1, self.L2
        if train:
            adam = dict(sched=self.sched, sched_slot=self._slot(t, 1, 0, 0, 1))
            # dH reads the output layer's weights BEFORE the pair's Adam updates them
            ops.linear_bwd_dx(self.dA, L2.W, self.dH, below=self.Hg, epi="relu", M=b, stream=st)
            ops.linear_bwd_dw_adam_pair(dict(dA=self.dA, X=self.Hg, lin=L2, adam=adam, M=b),
                                        dict(dA=self.dH, X=self.Zb, lin=L1, adam=adam, M=b),
                                        weight_decay=self.wd, stream=st)
        of_.sum_finalize(self.lossf, 1, self.recon if train else self.vrecon, out_slot=self._slot(t, 1, 0, 0, 1),
                         tick=self.ctr if self.use_graph else None, stream=st)
