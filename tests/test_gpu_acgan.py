"""Auxiliary-classifier GAN on the MI355X: the two head kernels against fp64, both steps' gradients against fp64
autograd, the fused engine against a plain-torch CPU loop of acgan.py's contract that replays the RNG protocol, a
wrong-label oracle the engine must NOT match, determinism, resume, the general path, sampling and accuracy.

Bounds are tests/test_gpu_aae.py's (1e-5 losses, 5e-5 parameters, 1.5e-6 of a tensor's scale for lockstep gradients,
2e-5 of a tensor's max for a kernel against fp64).  Plain-torch fp32 on the CPU (heads_ref(..., dtype=float32)) stays
inside the kernel bound against fp64 at every shape of SHAPES in both modes: worst dq 2.1e-6, dPre 1.5e-6, gWc 5.2e-7,
gb2 4.3e-7, da2 2.1e-7 of the tensor's max, losses 1.3e-7; no bound was widened."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import ac_gan  # noqa: E402
from generative_models_amd import ops, ops_fused  # noqa: E402

DEV = "cuda"
EPS = 1e-8


# ---- the head kernels against fp64 ------------------------------------------------------------------------------------
def heads_case(B, Hd, C, gen_mode, seed):
    """Hidden rows with dead columns and exact zeros, head weights scaled so that the largest source logit is +-7 (closer
    to 1, 1 - s has no fp32 digits left: test_gpu_aae.py) and the largest class logit +-30 (a log-softmax that does not
    subtract the maximum loses it there); labels with one class absent (C > 1)."""
    g = torch.Generator().manual_seed(seed)
    rows = B if gen_mode else 2 * B
    H = F.relu(torch.randn(rows, Hd, generator=g))
    H[:, : Hd // 4] = 0.0                                # columns whose h is 0 on every row (b1 << 0)
    w2, b2 = torch.randn(1, Hd, generator=g), torch.randn(1, generator=g)
    Wc, bc = torch.randn(C, Hd, generator=g), torch.randn(C, generator=g)
    k = 7.0 / (H.double() @ w2.double().T + b2.double()).abs().max().item()
    w2, b2 = (w2.double() * k).float(), (b2.double() * k).float()
    k = 30.0 / (H.double() @ Wc.double().T + bc.double()).abs().max().item()
    Wc, bc = (Wc.double() * k).float(), (bc.double() * k).float()
    y = torch.randint(0, max(1, C - 1), (B,), generator=g)          # class C - 1 never appears
    return H, w2, b2, Wc, bc, y


def heads_ref(H, w2, b2, Wc, bc, y, B, gen_mode, cw, dtype=torch.float64):
    """The contract's loss on the hidden rows with autograd: (total, CE of rows [0, B), correct real rows, da2, dq,
    dPre, [gw2, gb2, gWc, gbc])."""
    H, w2, b2, Wc, bc = (t.to(dtype).clone().requires_grad_() for t in (H, w2, b2, Wc, bc))
    a2, q = (H @ w2.T + b2)[:, 0], H @ Wc.T + bc
    a2.retain_grad(); q.retain_grad()
    s = torch.sigmoid(a2)
    if gen_mode:
        ce = F.cross_entropy(q, y)
        total = -torch.mean(torch.log(s + EPS)) + cw * ce
        correct = 0
    else:
        ce = F.cross_entropy(q[:B], y)
        total = -torch.mean(torch.log(s[:B] + EPS) + torch.log(1 - s[B:] + EPS)) + cw * (ce + F.cross_entropy(q[B:], y))
        correct = int((q[:B].argmax(1) == y).sum())
    total.backward()
    dPre = H.grad * (H > 0).to(dtype)
    return total.item(), ce.item(), correct, a2.grad, q.grad, dPre, [w2.grad, b2.grad, Wc.grad, bc.grad]


SHAPES = [(1, 4, 1), (37, 36, 3), (133, 400, 10), (64, 1024, 32), (2 * 37, 48, 10)]


def _run_heads(B, Hd, C, gen_mode, cw, through_ring=False, adam=None):
    H, w2, b2, Wc, bc, y = heads_case(B, Hd, C, gen_mode, 1000 * Hd + 10 * B + C + int(gen_mode))
    rows = H.shape[0]
    d = lambda t: t.to(DEV).contiguous()
    dH, dw = d(H), [d(t) for t in (w2, b2, Wc, bc)]
    if through_ring:                                     # classes read through row 1 of a two-row index ring
        perm = torch.randperm(3 * B, generator=torch.Generator().manual_seed(B))[:B]
        labels = torch.full((3 * B,), C - 1, dtype=torch.int32)
        labels[perm] = y.to(torch.int32)
        ring = torch.stack([torch.zeros(B, dtype=torch.int64), perm]).to(DEV)
        lab = ops.label_src(labels.to(DEV), ring.view(-1), ops.slot(0, 0, 1, 0, B))
    else:
        lab = ops.label_src(y.to(torch.int32).to(DEV))
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    da2, dq, dPre, out = nan(rows), nan(rows, C), nan(rows, Hd), nan(3)
    ws = ops_fused.acgan_heads_workspace(rows, Hd, C, DEV)
    ops_fused.acgan_heads_fwd(dH, *dw, lab, B, gen_mode, cw, da2, dq, ws, loss_out=out, ce_out=out,
                              ce_slot=ops.slot(0, 0, 1, 0, 1), acc_out=out, acc_slot=ops.slot(0, 0, 2, 0, 1))
    grads = None if gen_mode else [nan(*t.shape) for t in (w2, b2, Wc, bc)]
    ops_fused.acgan_heads_bwd(dH, *dw, B, gen_mode, da2, dq, dPre, ws, grads=grads)
    torch.cuda.synchronize()
    return (H, w2, b2, Wc, bc, y), dH, dw, (da2, dq, dPre, out, grads), ws


@pytest.mark.parametrize("gen_mode", [False, True], ids=["D", "G"])
@pytest.mark.parametrize("B,Hd,C", SHAPES)
def test_heads_forward_and_backward_vs_fp64(B, Hd, C, gen_mode):
    cw = 0.7
    case, dH, dw, (da2, dq, dPre, out, grads), ws = _run_heads(B, Hd, C, gen_mode, cw, through_ring=(B == 37))
    H, w2, b2, Wc, bc, y = case
    total, ce, correct, da2_r, dq_r, dPre_r, g_r = heads_ref(*case, B, gen_mode, cw)
    got = out.cpu().double()
    print("loss", got[0].item(), total, "ce", got[1].item(), ce, "correct", got[2].item(), correct)
    assert abs(got[0].item() - total) <= 2e-5 * max(1.0, abs(total))
    assert abs(got[1].item() - ce) <= 2e-5 * max(1.0, abs(ce))
    assert got[2].item() == correct                      # exact

    def close(t, r, name):
        err = (t.cpu().double() - r).abs().max().item()
        print(name, err, r.abs().max().item())
        assert err <= 2e-5 * max(r.abs().max().item(), 1e-30), (name, err)
    close(da2, da2_r, "da2")
    close(dq, dq_r, "dq")
    close(dPre, dPre_r, "dPre")
    assert torch.all(dPre.cpu()[H == 0] == 0)            # exactly 0 where the hidden unit is off
    if C > 1:
        assert torch.all(dq.cpu()[:, C - 1] >= 0)        # the absent class only ever pushes its logit down
    if gen_mode:
        return
    for t, r, n in zip(grads, g_r, ("gw2", "gb2", "gWc", "gbc")):
        close(t.view(r.shape), r, n)
    assert torch.all(grads[0].cpu().view(-1)[: Hd // 4] == 0) and torch.all(grads[2].cpu()[:, : Hd // 4] == 0)
    # one Adam step on the four head tensors in the same call, against torch.optim.Adam fed the kernel's own gradient
    sched = torch.from_numpy(ops.adam_schedule(2e-4, 1)).to(DEV)
    mom = [torch.zeros_like(t) for t in dw for _ in range(2)]
    ops_fused.acgan_heads_bwd(dH, *dw, B, False, da2, dq, dPre, ws, grads=grads,
                              adam=dict(sched=sched, sched_slot=ops.NO_SLOT), moments=mom)
    torch.cuda.synchronize()
    ps = [nn.Parameter(t.clone()) for t in (w2, b2, Wc, bc)]
    opt = torch.optim.Adam(ps, lr=2e-4)
    for p, gg in zip(ps, grads):
        p.grad = gg.cpu().clone().view(p.shape)
    opt.step()
    for p, t in zip(ps, dw):
        assert (t.cpu() - p.detach()).abs().max().item() <= 1e-6


# ---- the trainer against a plain-torch oracle ----------------------------------------------------------------------
def loaders(batch, n_train, n_test, side, C, seed=7):
    """Loaders over a private generator's images and classes; they shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, 1, side, side), 0.3), generator=g)
        y = torch.randint(0, C, (n,), generator=g)
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, y), batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_test), mk(n_test)


class Oracle(nn.Module):
    """The AC-GAN as plain torch layers on the CPU, initialised from the product model's weights."""
    NAMES = {"g1": "G.linear", "gl": "G.label", "g2": "G.generate", "d1": "D.linear", "d2": "D.discriminate",
             "dc": "D.classify"}

    def __init__(self, m, dtype=torch.float32):
        super().__init__()
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        for a, n in self.NAMES.items():
            w, b = sd[n + ".weight"], sd.get(n + ".bias")
            with torch.random.fork_rng(devices=[]):      # (nn.Linear's own initialisation draws)
                lin = nn.Linear(w.shape[1], w.shape[0], bias=b is not None)
            with torch.no_grad():
                lin.weight.copy_(w)
                if b is not None:
                    lin.bias.copy_(b)
            setattr(self, a, lin.to(dtype))

    def G(self, z, y):
        return torch.sigmoid(self.g2(F.relu(self.g1(z) + self.gl.weight[:, y].T)))

    def D(self, x):
        h = F.relu(self.d1(x))
        return torch.sigmoid(self.d2(h))[:, 0], self.dc(h)

    def gparams(self):
        return list(self.g1.parameters()) + list(self.gl.parameters()) + list(self.g2.parameters())

    def dparams(self):
        return list(self.d1.parameters()) + list(self.d2.parameters()) + list(self.dc.parameters())

    def d_loss(self, x, y, z, cw, roll=0):
        C = self.dc.weight.shape[0]
        fake = self.G(z, (y + roll) % C).detach()
        (sx, cx), (sg, cg) = self.D(x), self.D(fake)
        ce = F.cross_entropy(cx, y)
        return -torch.mean(torch.log(sx + EPS) + torch.log(1 - sg + EPS)) + cw * (ce + F.cross_entropy(cg, y)), ce

    def g_loss(self, y, z, cw, roll=0):
        C = self.dc.weight.shape[0]
        sg, cg = self.D(self.G(z, (y + roll) % C))
        return -torch.mean(torch.log(sg + EPS)) + cw * F.cross_entropy(cg, y)

    def state(self):
        out = {}
        for a, n in self.NAMES.items():
            for k, p in getattr(self, a).named_parameters():
                out[n + "." + k] = p
        return out


def oracle_train(o, its, epochs, G_lr=2e-4, D_lr=2e-4, D_steps=1, class_weight=1.0, roll=0):
    """ns_gan.py:94-170 with acgan.py's losses.  roll: the generator is fed every label moved on by `roll` classes
    (wrong, for the sensitivity test)."""
    Z = o.g1.weight.shape[1]
    G_opt, D_opt = torch.optim.Adam(o.gparams(), lr=G_lr), torch.optim.Adam(o.dparams(), lr=D_lr)
    steps = int(np.ceil(len(its[0]) / D_steps))
    Gl, Dl, Cl = [], [], []
    for _ in range(epochs):
        for _ in range(steps):
            step = []
            for _ in range(D_steps):
                x, y = next(iter(its[0]))
                x = x.view(x.shape[0], -1)
                D_opt.zero_grad()
                d, ce = o.d_loss(x, y, torch.randn(x.shape[0], Z), class_weight, roll)
                d.backward()
                D_opt.step()
                step.append(d.item())
            Dl.append(np.mean(step)); Cl.append(ce.item())
            G_opt.zero_grad()
            g = o.g_loss(y, torch.randn(x.shape[0], Z), class_weight, roll)
            g.backward()
            G_opt.step()
            Gl.append(g.item())
    return Gl, Dl, Cl


def product(cfg, its, epochs, use_graph=True, trainer_cls=None, **kw):
    torch.manual_seed(1234)
    m = ac_gan.ACGAN(cfg["I"], cfg["H"], cfg["Z"], cfg["C"])
    tr = (trainer_cls or ac_gan.ACGANTrainer)(m, *its)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs, **kw)
    torch.cuda.synchronize()
    return tr, m


def lclose(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= tol, (err.max(), got[:4], ref[:4])


SMALL = dict(I=64, H=48, Z=8, C=3, side=8, batch=32, n_train=200, n_test=48, epochs=2)
FULL = dict(I=784, H=400, Z=20, C=10, side=28, batch=256, n_train=6 * 256, n_test=64, epochs=1)

_ORACLE = {}


def oracle_run(cfg, roll=0, **kw):
    """The oracle's run of a configuration, computed once and shared."""
    key = (tuple(sorted(cfg.items())), roll, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        torch.manual_seed(99)
        its = loaders(cfg["batch"], cfg["n_train"], cfg["n_test"], cfg["side"], cfg["C"])
        torch.manual_seed(1234)
        o = Oracle(ac_gan.ACGAN(cfg["I"], cfg["H"], cfg["Z"], cfg["C"]))
        res = oracle_train(o, its, cfg["epochs"], roll=roll, **kw)
        _ORACLE[key] = (o, res, torch.get_rng_state())
    return _ORACLE[key]


def product_run(cfg, trainer_cls=None, use_graph=True, **kw):
    torch.manual_seed(99)
    its = loaders(cfg["batch"], cfg["n_train"], cfg["n_test"], cfg["side"], cfg["C"])
    tr, m = product(cfg, its, cfg["epochs"], use_graph=use_graph, trainer_cls=trainer_cls, **kw)
    return tr, m, its


def param_gap(m, o):
    ref = o.state()
    return max((v.cpu() - ref[k].detach()).abs().max().item() for k, v in m.state_dict().items())


def check_parity(tr, m, o, res, o_rng, tol_w=5e-5):
    Gl, Dl, Cl = res
    lclose(tr.Dlosses, Dl)
    lclose(tr.Glosses, Gl)
    lclose(tr.class_losses, Cl)
    assert torch.equal(torch.get_rng_state(), o_rng)
    ref = o.state()
    assert set(ref) == set(m.state_dict())
    for k, v in m.state_dict().items():
        assert (v.cpu() - ref[k].detach()).abs().max().item() <= tol_w, k


@pytest.mark.parametrize("cfg,kw", [(SMALL, {}), (SMALL, dict(D_steps=2, class_weight=0.5)), (FULL, {})],
                         ids=["64-48-8-C3-b32", "64-48-8-C3-b32-Dsteps2", "784-400-20-C10-b256"])
def test_engine_vs_oracle(cfg, kw):
    o, res, o_rng = oracle_run(cfg, **kw)
    tr, m, _ = product_run(cfg, **kw)
    assert type(tr._engine).__name__ == "ACGANEngine"
    check_parity(tr, m, o, res, o_rng)


def test_sensitivity_to_the_label_feed():
    """At lr 1e-2 the engine matches the contract's oracle and NOT one whose generator sees every label moved on by
    one class: the parity test would notice a wrong label feed."""
    cfg, kw = dict(SMALL, epochs=1), dict(G_lr=1e-2, D_lr=1e-2)
    tr, m, _ = product_run(cfg, **kw)
    o, res, o_rng = oracle_run(cfg, **kw)
    bad, _, _ = oracle_run(cfg, roll=1, **kw)
    right, wrong = param_gap(m, o), param_gap(m, bad)
    print("gap to the oracle", right, "gap to the rolled oracle", wrong)
    assert wrong > 10 * 5e-5, wrong                      # ten times the parity bound


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["64-48-8-C3-b32", "784-400-20-C10-b256"])
def test_teacher_forced_step_gradients_vs_fp64(cfg):
    """One iteration with G_lr = D_lr = 0: the parameters come out bitwise unchanged, and the D step's 6 and the G
    step's 5 gradients match fp64 autograd at the initial weights within 1.5e-6 of each tensor's scale."""
    b = cfg["batch"]
    its = loaders(b, b, 16, cfg["side"], cfg["C"])
    torch.manual_seed(1234)
    m = ac_gan.ACGAN(cfg["I"], cfg["H"], cfg["Z"], cfg["C"])
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    o = Oracle(m, torch.float64)
    tr = ac_gan.ACGANTrainer(m, *its)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1, G_lr=0.0, D_lr=0.0, class_weight=0.8)
    torch.cuda.synchronize()
    assert type(tr._engine).__name__ == "ACGANEngine"
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), init[k]), k
    got = tr._engine.phase_grads()
    assert [len(got[p]) for p in ("d", "g")] == [6, 5]
    torch.set_rng_state(st)
    x, y = next(iter(its[0]))
    x = x.view(b, -1).double()
    zD, zG = torch.randn(b, cfg["Z"]).double(), torch.randn(b, cfg["Z"]).double()
    ref = o.state()
    names = {id(p): k for k, p in ref.items()}
    d, _ = o.d_loss(x, y, zD, 0.8)
    gd = dict(zip([names[id(p)] for p in o.dparams()], torch.autograd.grad(d, o.dparams())))
    g = o.g_loss(y, zG, 0.8)
    gg = dict(zip([names[id(p)] for p in o.gparams()], torch.autograd.grad(g, o.gparams())))
    for phase, refs in (("d", gd), ("g", gg)):
        assert set(refs) == set(got[phase])
        for k, r in refs.items():
            scale = r.abs().max().item()
            assert scale > 0, (phase, k)
            err = (got[phase][k].cpu().double() - r).abs().max().item()
            print(phase, k, err / scale)
            assert err <= 1.5e-6 * scale, (phase, k, err, scale)


def _snapshot(tr, m):
    return (list(tr.Glosses), list(tr.Dlosses), list(tr.class_losses),
            {k: v.cpu().clone() for k, v in m.state_dict().items()}, torch.get_rng_state())


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and torch.equal(a[4], b[4])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("D_steps", [1, 2])
def test_bitwise_runs_graph_eager_and_resume(tmp_path, D_steps):
    """Ring rows i * D_steps + j across the boundary between the graph of 16 and the tail, and across a resume."""
    cfg = dict(SMALL, n_train=32 * 18 * D_steps)             # 18 iterations an epoch: a graph of 16 and two of 1
    runs = []
    for use_graph in (True, True, False):
        tr, m, _ = product_run(cfg, use_graph=use_graph, D_steps=D_steps)
        runs.append(_snapshot(tr, m))
    _same(runs[0], runs[1])
    _same(runs[0], runs[2])
    # train(1) + save + load into a fresh trainer + train(1) == train(2)
    tr, m, its = product_run(dict(cfg, epochs=1), D_steps=D_steps)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    assert set(ck["history"]) == {"Glosses", "Dlosses", "class_losses", "num_epochs"}
    assert ck["optim"]["G"]["step"] == 18 and ck["optim"]["D"]["step"] == 18 * D_steps
    state = torch.get_rng_state()
    m2 = ac_gan.ACGAN(cfg["I"], cfg["H"], cfg["Z"], cfg["C"]).to(DEV)
    tr2 = ac_gan.ACGANTrainer(m2, *its)
    tr2.load_checkpoint(path)
    assert torch.equal(torch.get_rng_state(), state)
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1, D_steps=D_steps)
    torch.cuda.synchronize()
    _same(runs[0], _snapshot(tr2, m2))


def test_general_path_when_train_D_overridden():
    class Mine(ac_gan.ACGANTrainer):
        def train_D(self, images, labels):
            return super().train_D(images, labels)
    cfg = dict(SMALL, n_train=96, epochs=1)
    o, res, o_rng = oracle_run(cfg)
    tr, m, _ = product_run(cfg, trainer_cls=Mine)
    assert tr._engine is None
    check_parity(tr, m, o, res, o_rng)


def test_general_path_with_forty_classes():
    cfg = dict(SMALL, C=40, n_train=96, epochs=1)
    o, res, o_rng = oracle_run(cfg)
    tr, m, _ = product_run(cfg)
    assert tr._engine is None
    check_parity(tr, m, o, res, o_rng)


def test_sample_accuracy_and_parzen():
    cfg = dict(SMALL, n_train=128, epochs=1)
    tr, m, its = product_run(cfg, G_lr=1e-2, D_lr=1e-2)
    o = Oracle(m)
    st = torch.get_rng_state()
    labels = [2, 0, 1, 1, 2, 0, 0]
    s1, s2 = tr.sample(7, seed=3, labels=labels), tr.sample(7, seed=3, labels=labels)
    assert s1.shape == (7, 64) and torch.equal(s1, s2)
    assert not torch.equal(s1, tr.sample(7, seed=4, labels=labels))
    assert torch.equal(st, torch.get_rng_state())        # the global generator is untouched
    z = torch.randn(7, cfg["Z"], generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert (s1.cpu() - o.G(z, torch.tensor(labels))).abs().max().item() <= 2e-5
        assert (tr.sample(7, seed=3).cpu() - o.G(z, torch.arange(7) % 3)).abs().max().item() <= 2e-5
        assert (tr.sample(7, seed=3, labels=1).cpu() - o.G(z, torch.ones(7, dtype=torch.int64))).abs().max().item() <= 2e-5
    for bad in (3, [0, 1], True):                        # a label of C, a wrong count, a bool
        with pytest.raises(ac_gan.LabelError):
            tr.sample(7, seed=3, labels=bad)
    x, y = its[2].dataset.tensors
    with torch.no_grad():
        logits = o.D(x.view(x.shape[0], -1))[1]
    top2 = logits.topk(2, dim=1).values
    assert (top2[:, 0] - top2[:, 1]).min().item() > 1e-5 # no two logits of a row tie (fp32 noise is ~1e-6)
    hits = int((logits.argmax(1) == y).sum())
    assert tr.accuracy() == hits / x.shape[0] == tr.accuracy(its[2])      # exact
    assert torch.equal(st, torch.get_rng_state())
    r = tr.parzen(n_samples=200, n_val=32)
    assert type(r).__name__ == "ParzenResult" and all(math.isfinite(v) for v in (r.sigma, r.ll_mean, r.ll_stderr))
    images = tr.generate_images(0, num_outputs=4, save=False, labels=[0, 1, 2, 0])
    assert images.shape == (4, 8, 8) and np.isfinite(images).all()
