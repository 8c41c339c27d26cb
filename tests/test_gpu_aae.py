"""Adversarial autoencoder on the MI355X: the fused engine against a plain-torch CPU loop of the three-phase contract
that replays the RNG protocol, the phase order, every phase's gradient against fp64, the two new kernels against fp64,
determinism, resume, the general path and sampling."""
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

import aae  # noqa: E402
from generative_models_amd import ops, ops_fused, trainers  # noqa: E402

DEV = "cuda"
EPS = 1e-8


def loaders(batch, n_train, n_val, n_test, side, seed=7):
    """Loaders over a private generator's images; they shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, 1, side, side), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


class Oracle(nn.Module):
    """The AAE as plain torch layers on the CPU, initialised from the product model's weights."""

    def __init__(self, m):
        super().__init__()
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        mk = lambda pre: self._lin(sd[pre + ".weight"], sd[pre + ".bias"])
        self.e1, self.ez = mk("encoder.linear"), mk("encoder.z")
        self.d1, self.d2 = mk("decoder.linear"), mk("decoder.recon")
        self.c1, self.c2 = mk("discriminator.linear"), mk("discriminator.discriminate")

    @staticmethod
    def _lin(w, b):
        with torch.random.fork_rng(devices=[]):      # (nn.Linear's own initialisation draws)
            lin = nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(w); lin.bias.copy_(b)
        return lin

    def enc(self, x):
        return self.ez(F.relu(self.e1(x)))

    def dec(self, z):
        return torch.sigmoid(self.d2(F.relu(self.d1(z))))

    def D(self, z):
        return torch.sigmoid(self.c2(F.relu(self.c1(z))))

    def state(self):
        names = {"e1": "encoder.linear", "ez": "encoder.z", "d1": "decoder.linear", "d2": "decoder.recon",
                 "c1": "discriminator.linear", "c2": "discriminator.discriminate"}
        out = {}
        for a, n in names.items():
            out[n + ".weight"], out[n + ".bias"] = getattr(self, a).weight, getattr(self, a).bias
        return out


def oracle_train(o, its, epochs, lr=1e-3, D_lr=2e-4, G_lr=2e-4, wd=1e-5, order="right"):
    """The contract's loop.  order="stale_encoder": phase 2 sees the encoder from BEFORE phase 1;
    order="stale_D": phase 3 sees D from BEFORE phase 2 (both wrong, for the phase-order test)."""
    next(iter(its[2]))
    enc_p = list(o.e1.parameters()) + list(o.ez.parameters())
    ae_opt = torch.optim.Adam(enc_p + list(o.d1.parameters()) + list(o.d2.parameters()), lr=lr, weight_decay=wd)
    d_opt = torch.optim.Adam(list(o.c1.parameters()) + list(o.c2.parameters()), lr=D_lr)
    g_opt = torch.optim.Adam(enc_p, lr=G_lr)
    recon, dls, gls, best = [], [], [], 1e10
    for _ in range(epochs):
        for x, _ in its[0]:
            x = x.view(x.shape[0], -1)
            z_stale = o.enc(x).detach()
            ae_opt.zero_grad()
            r = torch.sum((x - o.dec(o.enc(x))) ** 2)
            r.backward()
            ae_opt.step()
            z_real = torch.randn(x.shape[0], o.ez.weight.shape[0])
            z_fake = z_stale if order == "stale_encoder" else o.enc(x).detach()
            D_old = [p.detach().clone() for p in (o.c1.weight, o.c1.bias, o.c2.weight, o.c2.bias)]
            d_opt.zero_grad()
            d = -torch.mean(torch.log(o.D(z_real) + EPS) + torch.log(1 - o.D(z_fake) + EPS))
            d.backward()
            d_opt.step()
            g_opt.zero_grad()
            z = o.enc(x)
            if order == "stale_D":
                s = torch.sigmoid(F.linear(F.relu(F.linear(z, D_old[0], D_old[1])), D_old[2], D_old[3]))
            else:
                s = o.D(z)
            g = -torch.mean(torch.log(s + EPS))
            g.backward()
            g_opt.step()
            recon.append(r.item()); dls.append(d.item()); gls.append(g.item())
        with torch.no_grad():
            vals = [torch.sum((x.view(x.shape[0], -1) - o.dec(o.enc(x.view(x.shape[0], -1)))) ** 2).item()
                    for x, _ in its[1]]
        best = min(best, float(np.mean(vals)))
    return recon, dls, gls, best


def product(cfg, its, epochs, use_graph=True, trainer_cls=None, **kw):
    torch.manual_seed(1234)
    m = aae.AAE(cfg["I"], cfg["H"], cfg["Z"])
    tr = (trainer_cls or aae.AAETrainer)(m, *its)
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


SMALL = dict(I=64, H=48, Z=8, side=8, batch=32, n_train=200, n_val=48, n_test=48, epochs=2)
FULL = dict(I=784, H=400, Z=20, side=28, batch=512, n_train=3 * 512 + 336, n_val=512, n_test=64, epochs=1)
WIDE = dict(I=64, H=520, Z=40, side=8, batch=32, n_train=80, n_val=32, n_test=32, epochs=1)


def run_both(cfg, trainer_cls=None, order="right", **kw):
    mk = lambda: loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"])
    torch.manual_seed(99)
    its = mk()
    torch.manual_seed(1234)
    o = Oracle(aae.AAE(cfg["I"], cfg["H"], cfg["Z"]))
    res = oracle_train(o, its, cfg["epochs"], order=order, **kw)
    o_rng = torch.get_rng_state()
    torch.manual_seed(99)
    its = mk()
    tr, m = product(cfg, its, cfg["epochs"], trainer_cls=trainer_cls, **kw)
    return tr, m, o, res, o_rng


def check_parity(tr, m, o, res, o_rng, tol_w=5e-5):
    recon, dls, gls, best = res
    lclose(np.array(tr.recon_loss) / 100, np.array(recon) / 100)
    lclose(tr.Dlosses, dls)
    lclose(tr.Glosses, gls)
    assert abs(tr.best_val_loss - best) <= 1e-5 * max(1, abs(best))
    assert torch.equal(torch.get_rng_state(), o_rng)
    ref = o.state()
    for k, v in m.state_dict().items():
        assert (v.cpu() - ref[k].detach()).abs().max().item() <= tol_w, k


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["64-48-8-b32-ragged", "784-400-20-b512"])
def test_aae_engine_vs_oracle(cfg):
    tr, m, o, res, o_rng = run_both(cfg)
    assert type(tr._engine).__name__ == "AAEEngine"
    check_parity(tr, m, o, res, o_rng)


@pytest.mark.parametrize("wrong", ["stale_encoder", "stale_D"])
def test_phase_order(wrong):
    """The engine matches the contract's order and NOT an oracle in which phase 2 sees the encoder before phase 1's
    step, or phase 3 sees D before phase 2's step (larger learning rates, so that one step moves the losses)."""
    cfg, lrs = dict(SMALL, epochs=1), dict(lr=1e-2, D_lr=1e-2, G_lr=1e-2)
    tr, m, o, res, o_rng = run_both(cfg, **lrs)
    check_parity(tr, m, o, res, o_rng)
    _, _, _, bad, _ = run_both(cfg, order=wrong, **lrs)
    moved = bad[1] if wrong == "stale_encoder" else bad[2]
    mine = tr.Dlosses if wrong == "stale_encoder" else tr.Glosses
    err = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(mine, moved))
    assert err > 1e-4, err                              # ten times the parity bound


def _phase_grads_fp64(x, z_real, init):
    P = {k: v.clone().requires_grad_() for k, v in init.items()}
    lin = lambda t, n: t @ P[n + ".weight"].T + P[n + ".bias"]
    enc = lambda t: lin(F.relu(lin(t, "encoder.linear")), "encoder.z")
    D = lambda t: torch.sigmoid(lin(F.relu(lin(t, "discriminator.linear")), "discriminator.discriminate"))
    out = {}
    r = torch.sum((x - torch.sigmoid(lin(F.relu(lin(enc(x), "decoder.linear")), "decoder.recon"))) ** 2)
    ks = [k for k in P if not k.startswith("discriminator.")]
    out["ae"] = dict(zip(ks, torch.autograd.grad(r, [P[k] for k in ks])))
    d = -torch.mean(torch.log(D(z_real) + EPS) + torch.log(1 - D(enc(x).detach()) + EPS))
    ks = [k for k in P if k.startswith("discriminator.")]
    out["d"] = dict(zip(ks, torch.autograd.grad(d, [P[k] for k in ks])))
    g = -torch.mean(torch.log(D(enc(x)) + EPS))
    ks = [k for k in P if k.startswith("encoder.")]
    out["g"] = dict(zip(ks, torch.autograd.grad(g, [P[k] for k in ks])))
    return out


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["small", "784-400-20-b512"])
def test_teacher_forced_phase_gradients_vs_fp64(cfg):
    """One training batch with lr = D_lr = G_lr = 0: the parameters come out bitwise unchanged, and the three phases'
    gradients (4 + 4 + 4 encoder / decoder / D tensors, plus the generator phase's 4 encoder tensors) match fp64
    autograd at the initial weights within 1.5e-6 of each tensor's scale."""
    b = cfg["batch"]
    its = loaders(b, b, b, 16, cfg["side"])
    torch.manual_seed(1234)
    m = aae.AAE(cfg["I"], cfg["H"], cfg["Z"])
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = aae.AAETrainer(m, *its)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1, lr=0.0, D_lr=0.0, G_lr=0.0)
    torch.cuda.synchronize()
    assert type(tr._engine).__name__ == "AAEEngine"
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), init[k]), k
    got = tr._engine.phase_grads()
    assert [len(got[p]) for p in ("ae", "d", "g")] == [8, 4, 4]
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    z_real = torch.randn(b, cfg["Z"]).double()
    x = its[0].dataset.tensors[0][perm].reshape(b, -1).double()
    ref = _phase_grads_fp64(x, z_real, {k: v.double() for k, v in init.items()})
    for phase in ("ae", "d", "g"):
        for k, r in ref[phase].items():
            scale = r.abs().max().item()
            assert scale > 0, (phase, k)
            err = (got[phase][k].cpu().double() - r).abs().max().item()
            assert err <= 1.5e-6 * scale, (phase, k, err, scale)


def _critic_case(b, Z, H, g):
    """D weights with dead hidden columns (b1 << 0), prior and encoder rows, the largest logit scaled to +-7."""
    W1 = torch.randn(H, Z, generator=g) / Z ** 0.5
    b1 = torch.randn(H, generator=g) * 0.1
    b1[: H // 4] = -50.0                                # columns whose h is 0 on every row
    w2 = torch.randn(1, H, generator=g) * (3.0 / H ** 0.5)
    b2 = torch.randn(1, generator=g)
    zr, zf = torch.randn(b, Z, generator=g), torch.randn(b, Z, generator=g) * 2.0
    # logits within +-7 (s down to 1e-3 and up to 0.999): closer to 1, 1 - s itself has no fp32 digits left
    logit = torch.cat([F.relu(z.double() @ W1.double().T + b1.double()) @ w2.double().T + b2.double() for z in (zr, zf)])
    k = 7.0 / logit.abs().max().item()
    return W1, b1, (w2.double() * k).float(), (b2.double() * k).float(), zr, zf


def _D64(z, W1, b1, w2, b2):
    return torch.sigmoid(F.relu(z @ W1.T + b1) @ w2.T + b2)


@pytest.mark.parametrize("Z", [4, 20, 32])
@pytest.mark.parametrize("b", [1, 37, 512])
def test_critic_step_vs_fp64(Z, b):
    H = 400
    g = torch.Generator().manual_seed(100 * Z + b)
    W1, b1, w2, b2, zr, zf = _critic_case(b, Z, H, g)
    P = [t.double().requires_grad_() for t in (W1, b1, w2, b2)]
    s_r, s_f = _D64(zr.double(), *P), _D64(zf.double(), *P)
    loss = -torch.mean(torch.log(s_r + EPS) + torch.log(1 - s_f + EPS))
    ref = torch.autograd.grad(loss, P)
    d = lambda t: t.to(DEV).contiguous()
    ws = ops_fused.aae_critic_workspace(b, Z, H, DEV)
    grads = [torch.full(t.shape, float("nan"), device=DEV) for t in (W1, b1, w2, b2)]
    out = torch.zeros(1, device=DEV)
    dW = [d(t) for t in (W1, b1, w2, b2)]
    # the prior rows through a slot: row block 1 of a two-block ring
    ring = torch.cat([torch.randn(b, Z, generator=g), zr]).to(DEV)
    ops_fused.aae_critic_step(ring.view(-1), d(zf), b, *dW, ws, grads=grads, loss_out=out,
                              real_slot=ops.slot(0, 0, 1, 0, b * Z))
    torch.cuda.synchronize()
    assert abs(out.item() - loss.item()) <= 2e-5 * max(1.0, abs(loss.item())), (out.item(), loss.item())
    for gg, r, n in zip(grads, ref, ("W1", "b1", "w2", "b2")):
        err = (gg.cpu().double() - r).abs().max().item()
        assert err <= 2e-5 * max(r.abs().max().item(), 1e-6), (n, err)
    assert torch.all(grads[0].cpu()[: H // 4] == 0) and torch.all(grads[1].cpu()[: H // 4] == 0)
    # one Adam step in the same launches, against torch.optim.Adam fed the kernel's own gradient
    sched = torch.from_numpy(ops.adam_schedule(2e-4, 1)).to(DEV)
    mom = [torch.zeros_like(t) for t in dW for _ in range(2)]
    ops_fused.aae_critic_step(ring.view(-1), d(zf), b, *dW, ws, grads=grads, real_slot=ops.slot(0, 0, 1, 0, b * Z),
                              adam=dict(sched=sched, sched_slot=ops.NO_SLOT), moments=mom)
    ps = [nn.Parameter(t.clone()) for t in (W1, b1, w2, b2)]
    opt = torch.optim.Adam(ps, lr=2e-4)
    for p, gg in zip(ps, grads):
        p.grad = gg.cpu().clone()
    opt.step()
    for p, t in zip(ps, dW):
        assert (t.cpu() - p.detach()).abs().max().item() <= 1e-6


@pytest.mark.parametrize("Z", [4, 20, 32])
@pytest.mark.parametrize("b", [1, 37, 512])
def test_gen_mid_vs_fp64(Z, b):
    H = 400
    g = torch.Generator().manual_seed(7 * Z + b)
    W1, b1, w2, b2, _, z = _critic_case(b, Z, H, g)
    He = F.relu(torch.randn(b, H, generator=g))          # some He == 0: masked
    Wz = torch.randn(Z, H, generator=g) / H ** 0.5
    zd = z.double().requires_grad_()
    s = _D64(zd, W1.double(), b1.double(), w2.double(), b2.double())
    terms = -torch.log(s + EPS)
    (dz_ref,) = torch.autograd.grad(terms.mean(), zd)
    dHe_ref = (dz_ref @ Wz.double()) * (He > 0).double()
    d = lambda t: t.to(DEV).contiguous()
    dz, dHe = torch.full((b, Z), float("nan"), device=DEV), torch.full((b, H), float("nan"), device=DEV)
    part = torch.zeros(b, device=DEV)
    ops_fused.aae_gen_mid(d(z), d(He), d(W1), d(b1), d(w2), d(b2), d(Wz), dz, dHe, part, b)
    torch.cuda.synchronize()
    loss = part.cpu().double().sum().item() / b
    assert abs(loss - terms.mean().item()) <= 2e-5 * max(1.0, abs(terms.mean().item()))
    # 1e-4: a row with s = 0.999 carries 1 - s in fp32 (torch's SigmoidBackward does too), ~6e-5 relative
    for got, r, n in ((dz, dz_ref, "dz"), (dHe, dHe_ref, "dHe")):
        err = (got.cpu().double() - r).abs().max().item()
        assert err <= 1e-4 * max(r.abs().max().item(), 1e-6), (n, err)
    assert torch.all(dHe.cpu()[He == 0] == 0)


def test_aae_bitwise_eager_graph_and_resume(tmp_path):
    cfg = SMALL
    mk = lambda: loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"])
    runs = []
    for use_graph in (True, True, False):
        torch.manual_seed(99)
        tr, m = product(cfg, mk(), 2, use_graph=use_graph)
        runs.append((tr.recon_loss, tr.Dlosses, tr.Glosses, {k: v.cpu().clone() for k, v in m.state_dict().items()},
                     torch.get_rng_state()))
    for r in runs[1:]:
        assert r[0] == runs[0][0] and r[1] == runs[0][1] and r[2] == runs[0][2] and torch.equal(r[4], runs[0][4])
        for k in r[3]:
            assert torch.equal(r[3][k], runs[0][3][k]), k
    # train(1) + save + load into a fresh trainer + train(1) == train(2)
    torch.manual_seed(99)
    its = mk()
    tr, m = product(cfg, its, 1)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    from generative_models_amd import aae as pkg
    assert set(pkg.OPTIM_FIELDS) <= set(ck["optim"]) and set(ck["history"]) == set(pkg.HISTORY)
    assert ck["optim"]["steps"] == {"AE": 7, "D": 7, "G": 7}
    state = torch.get_rng_state()
    m2 = aae.AAE(cfg["I"], cfg["H"], cfg["Z"]).to(DEV)
    tr2 = aae.AAETrainer(m2, *its)
    tr2.load_checkpoint(path)
    assert torch.equal(torch.get_rng_state(), state)
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    assert tr2.recon_loss == runs[0][0] and tr2.Dlosses == runs[0][1] and tr2.Glosses == runs[0][2]
    assert torch.equal(torch.get_rng_state(), runs[0][4])
    for k, v in m2.state_dict().items():
        assert torch.equal(v.cpu(), runs[0][3][k]), k


def test_aae_general_path_when_train_G_overridden():
    class Mine(aae.AAETrainer):
        def train_G(self, images):
            return super().train_G(images)
    tr, m, o, res, o_rng = run_both(dict(SMALL, n_train=96, epochs=1), trainer_cls=Mine)
    assert tr._engine is None
    check_parity(tr, m, o, res, o_rng)


def test_aae_general_path_outside_fused_limits():
    tr, m, o, res, o_rng = run_both(WIDE)
    assert tr._engine is None
    check_parity(tr, m, o, res, o_rng)


def test_sample_and_parzen():
    its = loaders(32, 128, 64, 64, 8)
    torch.manual_seed(5)
    tr, m = product(dict(I=64, H=48, Z=8), its, 1)
    params = {k: v.clone() for k, v in m.state_dict().items()}
    st = torch.get_rng_state()
    s1, s2 = tr.sample(20, seed=3), tr.sample(20, seed=3)
    assert s1.shape == (20, 64) and torch.equal(s1, s2)
    assert torch.equal(st, torch.get_rng_state())
    for k, v in m.state_dict().items():
        assert torch.equal(v, params[k]), k
    r = tr.parzen(n_samples=200, n_val=32)
    assert type(r).__name__ == "ParzenResult" and all(math.isfinite(v) for v in (r.sigma, r.ll_mean, r.ll_stderr))
