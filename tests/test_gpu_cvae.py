"""Class-conditional VAE on the MI355X: the fused engine against a plain-torch CPU loop of the concatenated form that
replays VAETrainer's RNG protocol, the two new kernels against fp64, determinism, resume, conditioning, the general
path and label validation."""
import contextlib
import io
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

import cvae  # noqa: E402
from generative_models_amd import ops  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"


def loaders(batch, n_train, n_val, n_test, side, C, seed=7, disjoint=False):
    """(images, labels) loaders; the data come from a private generator, the loaders shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        y = torch.randint(0, C, (n,), generator=g)
        if disjoint:                       # class 0 lights the top half, class 1 the bottom half
            x = torch.zeros(n, 1, side, side)
            on = torch.bernoulli(torch.full((n, 1, side // 2, side), 0.8), generator=g)
            for i in range(n):
                if y[i] == 0:
                    x[i, :, :side // 2] = on[i]
                else:
                    x[i, :, side // 2:] = on[i]
        else:
            x = torch.bernoulli(torch.full((n, 1, side, side), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, y)
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


class Oracle(nn.Module):
    """The CVAE in its concatenated form: Linear(I + C, H) on cat[x, onehot(y)], Linear(Z + C, H) on cat[z, onehot(y)]."""

    def __init__(self, m):
        super().__init__()
        e, d = m.encoder, m.decoder
        cat = lambda a, b: nn.Parameter(torch.cat([a.detach().cpu(), b.detach().cpu()], 1).clone())
        self.C = m.num_classes
        self.e1 = nn.Linear(1, 1); self.e1.weight = cat(e.linear.weight, e.label.weight)
        self.e1.bias = nn.Parameter(e.linear.bias.detach().cpu().clone())
        self.mu = nn.Linear(1, 1); self.mu.weight = nn.Parameter(e.mu.weight.detach().cpu().clone())
        self.mu.bias = nn.Parameter(e.mu.bias.detach().cpu().clone())
        self.lv = nn.Linear(1, 1); self.lv.weight = nn.Parameter(e.log_var.weight.detach().cpu().clone())
        self.lv.bias = nn.Parameter(e.log_var.bias.detach().cpu().clone())
        self.d1 = nn.Linear(1, 1); self.d1.weight = cat(d.linear.weight, d.label.weight)
        self.d1.bias = nn.Parameter(d.linear.bias.detach().cpu().clone())
        self.rc = nn.Linear(1, 1); self.rc.weight = nn.Parameter(d.recon.weight.detach().cpu().clone())
        self.rc.bias = nn.Parameter(d.recon.bias.detach().cpu().clone())

    def forward(self, x, y):
        oh = F.one_hot(y, self.C).float()
        h = F.relu(self.e1(torch.cat([x, oh], 1)))
        mu, lv = self.mu(h), self.lv(h)
        z = mu + torch.randn(mu.shape) * torch.exp(lv / 2)
        return torch.sigmoid(self.rc(F.relu(self.d1(torch.cat([z, oh], 1))))), mu, lv

    def split_state(self, I, Z):
        return {"encoder.linear.weight": self.e1.weight[:, :I], "encoder.linear.bias": self.e1.bias,
                "encoder.label.weight": self.e1.weight[:, I:], "encoder.mu.weight": self.mu.weight,
                "encoder.mu.bias": self.mu.bias, "encoder.log_var.weight": self.lv.weight,
                "encoder.log_var.bias": self.lv.bias, "decoder.linear.weight": self.d1.weight[:, :Z],
                "decoder.linear.bias": self.d1.bias, "decoder.label.weight": self.d1.weight[:, Z:],
                "decoder.recon.weight": self.rc.weight, "decoder.recon.bias": self.rc.bias}


def oracle_train(o, its, epochs, lr=1e-3, wd=1e-5):
    """VAETrainer's protocol on the oracle: next(iter(test)) first, then per epoch a training and a validation pass."""
    next(iter(its[2]))
    opt = torch.optim.Adam(o.parameters(), lr=lr, weight_decay=wd)
    recon, kl, best = [], [], 1e10
    for _ in range(epochs):
        for x, y in its[0]:
            opt.zero_grad()
            out, mu, lv = o(x.view(x.shape[0], -1), y)
            r = torch.sum((x.view(x.shape[0], -1) - out) ** 2)
            k = torch.sum(0.5 * (mu ** 2 + torch.exp(lv) - lv - 1))
            (r + k).backward()
            opt.step()
            recon.append(r.item()); kl.append(k.item())
        vals = []
        for x, y in its[1]:
            out, mu, lv = o(x.view(x.shape[0], -1), y)
            vals.append((torch.sum((x.view(x.shape[0], -1) - out) ** 2)
                         + torch.sum(0.5 * (mu ** 2 + torch.exp(lv) - lv - 1))).item())
        best = min(best, float(np.mean(vals)))
    return recon, kl, best


def product(cfg, its, epochs, use_graph=True, trainer_cls=None):
    torch.manual_seed(1234)
    m = cvae.CVAE(cfg["I"], cfg["H"], cfg["Z"], cfg["C"])
    tr = (trainer_cls or cvae.CVAETrainer)(m, *its)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs)
    torch.cuda.synchronize()
    return tr, m


def lclose(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= tol, (err.max(), got[:4], ref[:4])


SMALL = dict(I=64, H=48, Z=8, C=3, side=8, batch=32, n_train=200, n_val=48, n_test=48, epochs=2)
FULL = dict(I=784, H=400, Z=20, C=10, side=28, batch=512, n_train=3 * 512 + 336, n_val=512, n_test=64, epochs=1)
# outside the fused launches' limits: Z % 4 != 0 (decoder layer 1 as vae_reparam_wide + ops.linear_fwd_label), and
# Z > 32 with a hidden width > 512 (that, plus the two generic dX launches instead of gm_vae_bwd_mid)
ODD_Z = dict(I=64, H=48, Z=6, C=3, side=8, batch=32, n_train=200, n_val=48, n_test=48, epochs=2)
WIDE = dict(I=64, H=520, Z=40, C=5, side=8, batch=32, n_train=80, n_val=32, n_test=32, epochs=1)


def parity(cfg, trainer_cls=None, tol_w=5e-5):
    mk = lambda: loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"], cfg["C"])
    torch.manual_seed(99)
    its = mk()
    torch.manual_seed(1234)
    init = cvae.CVAE(cfg["I"], cfg["H"], cfg["Z"], cfg["C"])
    with torch.random.fork_rng(devices=[]):                # (the oracle's placeholder layers draw)
        o = Oracle(init)
    recon, kl, best = oracle_train(o, its, cfg["epochs"])
    o_rng = torch.get_rng_state()
    torch.manual_seed(99)
    its = mk()
    tr, m = product(cfg, its, cfg["epochs"], trainer_cls=trainer_cls)
    lclose(np.array(tr.recon_loss) / 100, np.array(recon) / 100)
    lclose(tr.kl_loss, kl)
    assert abs(tr.best_val_loss - best) <= 1e-5 * max(1, abs(best))
    assert torch.equal(torch.get_rng_state(), o_rng)
    ref = o.split_state(cfg["I"], cfg["Z"])
    for k, v in m.state_dict().items():
        assert (v.cpu() - ref[k].detach()).abs().max().item() <= tol_w, k
    return tr


@pytest.mark.parametrize("cfg", [SMALL, FULL, ODD_Z, WIDE],
                         ids=["small-C3-ragged", "784-400-20-C10-b512", "z6-fallback", "z40-h520-fallback"])
def test_cvae_engine_vs_oracle(cfg):
    tr = parity(cfg)
    assert type(tr._engine).__name__ == "CVAEEngine"


@pytest.mark.parametrize("cfg", [SMALL, FULL, ODD_Z, WIDE], ids=["small", "784-400-20-C10-b512", "z6", "z40-h520"])
def test_teacher_forced_step_gradients_vs_fp64(cfg):
    """One training batch through CVAEEngine from known weights: every gradient it leaves in the flat gradient buffer
    (all 12 tensors, both label.weight included) against fp64 autograd of the concatenated form on the same images,
    labels and eps, within 1.5e-6 of each tensor's scale."""
    from generative_models_amd import trainers
    b = cfg["batch"]
    its = loaders(b, b, b, 16, cfg["side"], cfg["C"])
    torch.manual_seed(1234)
    m = cvae.CVAE(cfg["I"], cfg["H"], cfg["Z"], cfg["C"])
    init = {k: v.detach().clone().double() for k, v in m.state_dict().items()}
    tr = cvae.CVAETrainer(m, *its)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    torch.cuda.synchronize()
    fp = tr._engine.fp
    got = {k: fp.gviews[[i for i, q in enumerate(fp.params) if q is p][0]].cpu().double()
           for k, p in m.named_parameters()}
    assert len(got) == 12
    # the batch's rows and eps, replayed from the RNG protocol: the pass's permutation, then randn(b, Z)
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    eps = torch.randn(b, cfg["Z"]).double()
    x = its[0].dataset.tensors[0][perm].reshape(b, -1).double()
    oh = F.one_hot(its[0].dataset.tensors[1][perm], cfg["C"]).double()
    P = {k: v.clone().requires_grad_() for k, v in init.items()}
    cat = lambda w, e: torch.cat([P[w], P[e]], 1)
    h = F.relu(torch.cat([x, oh], 1) @ cat("encoder.linear.weight", "encoder.label.weight").T + P["encoder.linear.bias"])
    mu = h @ P["encoder.mu.weight"].T + P["encoder.mu.bias"]
    lv = h @ P["encoder.log_var.weight"].T + P["encoder.log_var.bias"]
    z = mu + eps * torch.exp(lv / 2)
    hd = F.relu(torch.cat([z, oh], 1) @ cat("decoder.linear.weight", "decoder.label.weight").T
                + P["decoder.linear.bias"])
    out = torch.sigmoid(hd @ P["decoder.recon.weight"].T + P["decoder.recon.bias"])
    loss = torch.sum((x - out) ** 2) + torch.sum(0.5 * (mu ** 2 + torch.exp(lv) - lv - 1))
    loss.backward()
    for k, g in got.items():
        ref = P[k].grad
        scale = ref.abs().max().item()
        assert scale > 0, k
        err = (g - ref).abs().max().item()
        assert err <= 1.5e-6 * scale, (k, err, scale)


def test_cvae_general_path_when_hook_overridden():
    class Mine(cvae.CVAETrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    cfg = dict(SMALL, n_train=96, epochs=1)
    tr = parity(cfg, trainer_cls=Mine)
    assert tr._engine is None


@pytest.mark.parametrize("act", ["id", "relu", "sigmoid"])
@pytest.mark.parametrize("C", [1, 3, 10, 17])
def test_linear_fwd_label_vs_fp64(act, C):
    g = torch.Generator().manual_seed(C)
    for M, K, N in [(1, 2, 5), (7, 20, 400), (64, 32, 5), (336, 784, 400), (512, 20, 400), (2048, 784, 400)]:
        x, W = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5
        b, E = torch.randn(N, generator=g), torch.randn(N, C, generator=g)
        y = torch.randint(0, C, (M,), generator=g)
        ref = x.double() @ W.double().T + b.double() + E.double()[:, y].T
        ref = {"id": ref, "relu": ref.clamp_min(0), "sigmoid": torch.sigmoid(ref)}[act]
        out = torch.empty(M, N, device=DEV)
        lab = y.to(DEV, torch.int32)
        ops.linear_fwd_label(x.to(DEV), W.to(DEV), b.to(DEV), E.to(DEV), ops.label_src(lab), out, act)
        err = (out.cpu().double() - ref).abs().max().item()
        assert err <= 2e-5 * max(1.0, ref.abs().max().item()), (M, K, N, err)
        # through an index ring row: labels[idx[m]]
        perm = torch.randperm(M, generator=g)
        out2 = torch.empty(M, N, device=DEV)
        ops.linear_fwd_label(x.to(DEV), W.to(DEV), b.to(DEV), E.to(DEV),
                             ops.label_src(lab, perm.to(DEV)), out2, act)
        ref2 = x.double() @ W.double().T + b.double() + E.double()[:, y[perm]].T
        ref2 = {"id": ref2, "relu": ref2.clamp_min(0), "sigmoid": torch.sigmoid(ref2)}[act]
        assert (out2.cpu().double() - ref2).abs().max().item() <= 2e-5 * max(1.0, ref2.abs().max().item())


@pytest.mark.parametrize("C", [1, 3, 10, 17])
def test_reparam_fwd_label_vs_fp64(C):
    from generative_models_amd import ops_fused
    g = torch.Generator().manual_seed(10 + C)
    for M, Z, N in [(1, 4, 5), (7, 20, 400), (336, 20, 400), (512, 32, 400)]:
        ml, eps = torch.randn(M, 2 * Z, generator=g) * 0.5, torch.randn(M, Z, generator=g)
        W, b, E = torch.randn(N, Z, generator=g) / Z ** 0.5, torch.randn(N, generator=g), torch.randn(N, C, generator=g)
        y = torch.randint(0, C, (M,), generator=g)
        z, H = torch.empty(M, Z, device=DEV), torch.empty(M, N, device=DEV)
        part = torch.empty((M * Z + 255) // 256, device=DEV)
        ops_fused.vae_reparam_fwd_label(ml.to(DEV), eps.to(DEV), z, part, M, Z, W.to(DEV), b.to(DEV), H, "relu",
                                        E.to(DEV), ops.label_src(y.to(DEV, torch.int32)))
        zr = ml[:, :Z].double() + eps.double() * torch.exp(ml[:, Z:].double() / 2)
        ref = (zr @ W.double().T + b.double() + E.double()[:, y].T).clamp_min(0)
        assert (H.cpu().double() - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("C", [1, 3, 10, 17])
def test_label_grad_vs_fp64_and_absent_classes(C):
    g = torch.Generator().manual_seed(20 + C)
    for M, N in [(1, 5), (7, 400), (64, 5), (336, 400), (512, 400), (2048, 400)]:
        d0, d1 = torch.randn(M, N, generator=g), torch.randn(M, 400, generator=g)
        y = torch.randint(0, max(1, C - 1) if C > 2 else C, (M,), generator=g)  # C > 2: the last class is absent
        lab = ops.label_src(y.to(DEV, torch.int32))
        g0, g1 = torch.empty(N, C, device=DEV), torch.empty(400, C, device=DEV)
        ops.label_grad_adam([dict(dPre=d0.to(DEV), gE=g0), dict(dPre=d1.to(DEV), gE=g1)], lab, M, C)
        oh = F.one_hot(y, C).double()
        for got, d in ((g0, d0), (g1, d1)):
            ref = d.double().T @ oh
            assert (got.cpu().double() - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())
            absent = oh.sum(0) == 0
            assert torch.all(got.cpu()[:, absent] == 0)
        # Adam in the same launch: an absent class moves by weight decay alone
        E = torch.randn(N, C, generator=g)
        Ed, mE, vE = E.to(DEV), torch.zeros(N, C, device=DEV), torch.zeros(N, C, device=DEV)
        sched = torch.from_numpy(ops.adam_schedule(1e-3, 1)).to(DEV)
        ops.label_grad_adam([dict(dPre=d0.to(DEV), E=Ed, mE=mE, vE=vE)], lab, M, C,
                            adam=dict(sched=sched, sched_slot=ops.NO_SLOT), weight_decay=1e-5)
        p = nn.Parameter(E.clone())
        opt = torch.optim.Adam([p], lr=1e-3, weight_decay=1e-5)
        p.grad = g0.cpu().clone()
        opt.step()
        assert (Ed.cpu() - p.detach()).abs().max().item() <= 1e-6


def test_cvae_bitwise_eager_graph_and_resume(tmp_path):
    cfg = SMALL
    mk = lambda: loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"], cfg["C"])
    runs = []
    for use_graph in (True, True, False):
        torch.manual_seed(99)
        tr, m = product(cfg, mk(), 2, use_graph=use_graph)
        runs.append((tr.recon_loss, tr.kl_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
                     torch.get_rng_state()))
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and torch.equal(r[3], runs[0][3])
        for k in r[2]:
            assert torch.equal(r[2][k], runs[0][2][k]), k
    # train(1) + save + load into a fresh trainer + train(1) == train(2)
    torch.manual_seed(99)
    its = mk()
    tr, m = product(cfg, its, 1)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    state = torch.get_rng_state()
    m2 = cvae.CVAE(cfg["I"], cfg["H"], cfg["Z"], cfg["C"]).to(DEV)
    tr2 = cvae.CVAETrainer(m2, *its)                        # (draws: init, next(iter(test_iter)))
    tr2.load_checkpoint(path)
    assert torch.equal(torch.get_rng_state(), state)        # the checkpoint carries the protocol cursor
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    assert tr2.recon_loss == runs[0][0] and tr2.kl_loss == runs[0][1]
    assert torch.equal(torch.get_rng_state(), runs[0][3])
    for k, v in m2.state_dict().items():
        assert torch.equal(v.cpu(), runs[0][2][k]), k


def test_conditioning_controls_the_samples():
    its = loaders(32, 1024, 64, 64, 8, 2, disjoint=True)
    torch.manual_seed(5)
    m = cvae.CVAE(64, 64, 4, 2)
    tr = cvae.CVAETrainer(m, *its)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(10, lr=3e-3)
    for c in (0, 1):
        s = tr.sample(200, seed=3, labels=c).cpu()
        top, bottom = s[:, :32].sum().item(), s[:, 32:].sum().item()
        share = (top if c == 0 else bottom) / (top + bottom)
        # measured: 0.977 (class 0) and 0.974 (class 1); 0.5 would mean no conditioning
        assert share > 0.9, (c, share)
    assert not torch.allclose(tr.sample(50, seed=4, labels=0), tr.sample(50, seed=4, labels=1))
    # parzen() scores class-balanced samples; sampling leaves the global generator alone
    st = torch.get_rng_state()
    tr.sample(10)
    assert torch.equal(st, torch.get_rng_state())


def test_bad_labels_raise_before_any_launch():
    its = loaders(16, 64, 16, 16, 8, 3)
    its[0].dataset.tensors[1][5] = 3                       # == C
    torch.manual_seed(1)
    m = cvae.CVAE(64, 32, 4, 3).to(DEV)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    tr = cvae.CVAETrainer(m, *its)
    with pytest.raises(GMError):
        tr.train(1)
    assert tr._engine is None
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    with pytest.raises(ValueError):
        tr.sample(4, labels=[0, 1, 2, 3])


def test_label_ops_refuse_arrays_that_do_not_fit():
    lab = ops.label_src(torch.zeros(8, dtype=torch.int32, device=DEV))
    dP = torch.zeros(8, 16, device=DEV)
    for bad in (torch.zeros(12, 3, device=DEV), torch.zeros(16, 4, device=DEV), torch.zeros(3, 16, device=DEV).T):
        with pytest.raises(GMError):
            ops.label_grad_adam([dict(dPre=dP, gE=bad)], lab, 8, 3)
    for bad in (torch.zeros(12, 3, device=DEV), torch.zeros(3, 16, device=DEV).T):
        with pytest.raises(GMError):
            ops.linear_fwd_label(torch.zeros(8, 4, device=DEV), torch.zeros(16, 4, device=DEV), None, bad, lab,
                                 torch.zeros(8, 16, device=DEV), "relu")
    with pytest.raises(GMError):                           # more rows than labels
        ops.label_grad_adam([dict(dPre=torch.zeros(9, 16, device=DEV), gE=torch.zeros(16, 3, device=DEV))], lab, 9, 3)
