"""Primal-Dual Wasserstein GAN on the MI355X: the two row kernels against fp64, the fused engine against a plain-torch
fp64 restatement of the three-phase contract (pdwgan.py's docstring) that replays the RNG protocol, every phase's
gradient against fp64 autograd, the phase order, determinism, resume, the general path and the sampling surface."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import pdw_gan  # noqa: E402
from generative_models_amd import ops, ops_fused, trainers  # noqa: E402
from generative_models_amd import pdwgan as pkg  # noqa: E402

DEV = "cuda"
BAND = 1e-3                 # "near a ReLU kink": a pre-activation within this of 0


def loaders(batch, n_train, n_val, n_test, side, seed=7):
    """Loaders over a private generator's images; they shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, 1, side, side), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


# ---- the oracle: the contract in fp64 (an fp32 CPU run would be the less accurate side) ----------------------------
def relu_at(a, thr=0.0):
    """relu whose mask is (a > thr): thr = +-BAND moves every near-kink decision one way or the other."""
    return a * (a > thr).to(a.dtype)


class Net:
    """The three MLPs on a dict of fp64 tensors keyed by the model's state_dict names."""

    def __init__(self, P, thr=0.0):
        self.P, self.thr, self.pre = P, thr, []

    def lin(self, x, n):
        return x @ self.P[n + ".weight"].T + self.P[n + ".bias"]

    def hid(self, x, n):
        a = self.lin(x, n)
        self.pre.append(a.detach())
        return relu_at(a, self.thr)

    def E(self, x):
        return self.lin(self.hid(x, "E.linear"), "E.z")

    def G(self, z):
        return torch.sigmoid(self.lin(self.hid(z, "G.linear"), "G.generate"))

    def D(self, x):
        return self.hid(self.hid(x, "D.linear"), "D.discriminate")


def mmd64(z, p):
    def k(x, y):
        dim = x.shape[1]
        return torch.exp(-((x.unsqueeze(1) - y.unsqueeze(0)) ** 2).mean(2) / dim)
    return k(p, p).sum() + k(z, z).sum() - 2 * k(p, z).sum()


def couple64(x, xr):
    diff = x - xr
    n = diff.norm(dim=1)
    d = torch.where(n.unsqueeze(1) > 0, diff / n.unsqueeze(1).clamp_min(1e-300), torch.zeros_like(diff))
    return n, d


def phase_losses(net, x, draws, lz, lgp, coupling=None, penalty="direction"):
    """(L_E, coupling) / L_D / L_G as three closures' values; draws = (p, t, zc, zg) in fp64."""
    p, t, zc, zg = draws
    z = net.E(x)
    xr = net.G(z)
    n, d = couple64(x, xr)
    LE = n.mean() + lz * mmd64(z, p)
    xr_d, d = (xr.detach(), d.detach()) if coupling is None else coupling
    xh = (t * x + (1 - t) * xr_d).requires_grad_(True)

    def LD():
        g = torch.autograd.grad(net.D(xh).sum(), xh, create_graph=True)[0]
        pen = ((g - d) ** 2).sum(1).mean() if penalty == "direction" else ((g.norm(dim=1) - 1) ** 2).mean()
        return net.D(net.G(zc).detach()).mean() - net.D(x).mean() + lgp * pen

    def LG():
        return -net.D(net.G(zg)).mean()
    return LE, LD, LG


def oracle_train(P, its, epochs, E_lr=1e-4, G_lr=1e-4, D_lr=1e-4, lambda_z=pkg.LAMBDA_Z, lambda_gp=10.0,
                 wrong=None):
    """The contract's loop.  wrong="rerun_encoder": the critic is fed the coupling of the encoder AFTER its step;
    wrong="norm_only": WGAN-GP's norm penalty on the same interpolates (both wrong, for the phase-order test)."""
    next(iter(its[2]))
    keys = lambda pre: [P[k] for k in P if k.startswith(pre)]
    e_opt, d_opt, g_opt = (torch.optim.Adam(keys(pre), lr=lr) for pre, lr in (("E.", E_lr), ("D.", D_lr), ("G.", G_lr)))
    Z = P["E.z.weight"].shape[0]
    net = Net(P)
    el, dl, gl, best = [], [], [], 1e10
    for _ in range(epochs):
        for x, _ in its[0]:
            x = x.view(x.shape[0], -1).double()
            b = x.shape[0]
            p = torch.randn(b, Z).double()
            # (the draws happen in the contract's order: p here, then t, z_c, z_g below)
            z = net.E(x)
            xr = net.G(z)
            n, d = couple64(x, xr)
            LE = n.mean() + lambda_z * mmd64(z, p)
            coupling = (xr.detach(), d.detach())
            for o in (e_opt, d_opt, g_opt):
                o.zero_grad()
            LE.backward()
            e_opt.step()
            if wrong == "rerun_encoder":
                with torch.no_grad():
                    xr2 = net.G(net.E(x))
                    coupling = (xr2, couple64(x, xr2)[1])
            t = torch.rand(b, 1).double()
            zc = torch.randn(b, Z).double()
            xh = (t * x + (1 - t) * coupling[0]).requires_grad_(True)
            g = torch.autograd.grad(net.D(xh).sum(), xh, create_graph=True)[0]
            pen = ((g - coupling[1]) ** 2).sum(1).mean() if wrong != "norm_only" else ((g.norm(dim=1) - 1) ** 2).mean()
            LD = net.D(net.G(zc).detach()).mean() - net.D(x).mean() + lambda_gp * pen
            d_opt.zero_grad()
            LD.backward()
            d_opt.step()
            zg = torch.randn(b, Z).double()
            LG = -net.D(net.G(zg)).mean()
            g_opt.zero_grad()
            LG.backward()
            g_opt.step()
            el.append(LE.item()); dl.append(LD.item()); gl.append(LG.item())
        with torch.no_grad():
            vals = []
            for x, _ in its[1]:
                x = x.view(x.shape[0], -1).double()
                vals.append(couple64(x, net.G(net.E(x)))[0].mean().item())
        best = min(best, float(np.mean(vals)))
    return el, dl, gl, best


def live_critic(sd_or_model):
    """Raise the critic's output bias: at its initialisation the ReLU critic is 0 on most rows (the reference's
    critic, w_gp_gan.py:49-62), which leaves the generator phase nothing to do."""
    with torch.no_grad():
        sd = sd_or_model if isinstance(sd_or_model, dict) else sd_or_model.state_dict()
        sd["D.discriminate.bias"].fill_(1.0)


def product(cfg, its, epochs, use_graph=True, trainer_cls=None, prep=None, **kw):
    torch.manual_seed(1234)
    m = pdw_gan.PDWGAN(cfg["I"], cfg["H"], cfg["Z"])
    if prep is not None:
        prep(m)
    tr = (trainer_cls or pdw_gan.PDWGANTrainer)(m, *its)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs, **kw)
    torch.cuda.synchronize()
    return tr, m


def lclose(got, ref, tol=1e-5, what=""):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print("%s: max relative error %.3g (bound %.1g)" % (what, err.max(), tol))
    assert err.max() <= tol, (what, err.max(), got[:4], ref[:4])


SMALL = dict(I=64, H=48, Z=8, side=8, batch=32, n_train=200, n_val=48, n_test=48, epochs=1)
FULL = dict(I=784, H=400, Z=20, side=28, batch=512, n_train=3 * 512 + 336, n_val=512, n_test=64, epochs=1)
ODD = dict(I=64, H=48, Z=6, side=8, batch=32, n_train=160, n_val=32, n_test=32, epochs=1)


def run_both(cfg, trainer_cls=None, wrong=None, prep=None, **kw):
    mk = lambda: loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"])
    torch.manual_seed(99)
    its = mk()
    torch.manual_seed(1234)
    m0 = pdw_gan.PDWGAN(cfg["I"], cfg["H"], cfg["Z"])
    if prep is not None:
        prep(m0)
    P = {k: v.detach().cpu().double().clone().requires_grad_() for k, v in m0.state_dict().items()}
    res = oracle_train(P, its, cfg["epochs"], wrong=wrong, **kw)
    o_rng = torch.get_rng_state()
    torch.manual_seed(99)
    its = mk()
    tr, m = product(cfg, its, cfg["epochs"], trainer_cls=trainer_cls, prep=prep, **kw)
    return tr, m, P, res, o_rng


def check_parity(tr, m, P, res, o_rng, tol_w=5e-5):
    el, dl, gl, best = res
    lclose(tr.Elosses, el, what="Elosses")
    lclose(tr.Dlosses, dl, what="Dlosses")
    lclose(tr.Glosses, gl, what="Glosses")
    print("val %.8g vs %.8g" % (tr.best_val_loss, best))
    assert abs(tr.best_val_loss - best) <= 1e-5 * max(1, abs(best))
    assert torch.equal(torch.get_rng_state(), o_rng)
    worst = 0.0
    for k, v in m.state_dict().items():
        err = (v.cpu().double() - P[k].detach()).abs().max().item()
        worst = max(worst, err)
        assert err <= tol_w, (k, err)
    print("parameters: max abs error %.3g (bound %.1g)" % (worst, tol_w))


# ---- the two kernels -------------------------------------------------------------------------------------------------
def _rows(b, I, g):
    x = torch.bernoulli(torch.full((b, I), 0.3), generator=g)
    xr = torch.sigmoid(torch.randn(b, I, generator=g))
    if b > 1:
        xr[b // 2] = x[b // 2]                              # a row the reconstruction hits exactly: d = 0
    return x, xr


@pytest.mark.parametrize("I", [13, 64, 784])
@pytest.mark.parametrize("b", [1, 37, 512])
def test_pdw_couple_vs_fp64(I, b):
    """n, the loss share, d L_E / d (pre-sigmoid x~), x^ and the copy of x, each within 2e-5 of its scale (the AAE
    kernels' bound); the t rows through a slot (row block 1 of a two-block ring)."""
    g = torch.Generator().manual_seed(1000 * I + b)
    x, xr = _rows(b, I, g)
    t = torch.rand(b, generator=g)
    ring = torch.cat([torch.rand(b, generator=g), t]).to(DEV)
    xd, rd = x.double(), xr.double().requires_grad_()
    n_ref, d_ref = couple64(xd, rd)
    # d share / d (pre-sigmoid x~): sigmoid' = x~ (1 - x~)
    dA_ref = (-(d_ref.detach() / b) * (xr.double() * (1 - xr.double())))
    xh_ref = t.double().unsqueeze(1) * xd + (1 - t.double().unsqueeze(1)) * xr.double()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    n, share, dA, xh, xc = nan(b), nan(b), nan(b, I), nan(b, I), nan(b, I)
    ops_fused.pdw_couple(x.to(DEV), xr.to(DEV), share, b, n=n, t=ring, t_slot=ops.slot(0, 0, 1, 0, b), dA=dA, xhat=xh,
                         xcopy=xc)
    torch.cuda.synchronize()
    for got, ref, nm in ((n, n_ref.detach(), "n"), (share, n_ref.detach() / b, "share"), (dA, dA_ref, "dA"),
                         (xh, xh_ref, "xhat")):
        got = got.cpu().double()
        assert torch.isfinite(got).all(), nm
        err, scale = (got - ref).abs().max().item(), max(ref.abs().max().item(), 1e-6)
        print("couple I=%d b=%d %s: %.3g of scale" % (I, b, nm, err / scale))
        assert err <= 2e-5 * scale, (nm, err, scale)
    assert torch.equal(xc.cpu(), x)
    if b > 1:
        assert n.cpu()[b // 2].item() == 0 and torch.all(dA.cpu()[b // 2] == 0)
    else:
        assert n.cpu()[0].item() > 0 and bool((dA.cpu()[0] != 0).any())
    # the share-only form validation uses
    share2 = nan(b)
    ops_fused.pdw_couple(x.to(DEV), xr.to(DEV), share2, b)
    torch.cuda.synchronize()
    assert torch.equal(share2.cpu(), share.cpu())


@pytest.mark.parametrize("I", [13, 64, 784])
@pytest.mark.parametrize("b", [1, 37, 512])
def test_pdw_dir_vs_fp64(I, b):
    """pen and gamma within 2e-5 of their scales; on the row with x == x~ (b > 1): d = 0, gamma = (2 lambda / b) g, no NaN."""
    g = torch.Generator().manual_seed(77 * I + b)
    x, xr = _rows(b, I, g)
    gr = torch.randn(b, I, generator=g) / I ** 0.5
    lam, inv_b = 10.0, float(np.float32(1.0) / np.float32(b))
    n_ref, d_ref = couple64(x.double(), xr.double())
    gd = gr.double().requires_grad_()
    pen_ref = ((gd - d_ref) ** 2).sum(1)
    (gam_ref,) = torch.autograd.grad(lam * pen_ref.mean(), gd)
    gam, pen = torch.full((b, I), float("nan"), device=DEV), torch.full((b,), float("nan"), device=DEV)
    ops_fused.pdw_dir(gr.to(DEV), x.to(DEV), xr.to(DEV), n_ref.float().to(DEV), gam, pen, lam, inv_b)
    torch.cuda.synchronize()
    for got, ref, nm in ((pen, pen_ref.detach(), "pen"), (gam, gam_ref, "gamma")):
        got = got.cpu().double()
        assert torch.isfinite(got).all(), nm
        err, scale = (got - ref).abs().max().item(), max(ref.abs().max().item(), 1e-6)
        print("dir I=%d b=%d %s: %.3g of scale" % (I, b, nm, err / scale))
        assert err <= 2e-5 * scale, (nm, err, scale)
    if b > 1:
        r = b // 2
        assert (gam.cpu()[r].double() - 2 * lam / b * gr[r].double()).abs().max().item() <= 2e-5 * gam_ref.abs().max().item()


# ---- teacher-forced phase gradients ----------------------------------------------------------------------------------
def kink_free_weights(m, cfg):
    """Teacher-forced inputs whose hidden pre-activations stay clear of the ReLU kinks.  Every hidden unit's bias is
    moved to +c or -c (alternating: live and dead units both occur), c several standard deviations of the layer's
    pre-activation, and the critic's output bias so that its pre-activation sits near +2.  The encoder's first layer
    reads binary images, so there the masks can also differ from row to row without coming near a kink: every second
    PAIR of its units gets the weight -+2c on pixel 0 and so has the pre-activation +-c (1 - 2 x0) + the layer's own
    small term -- live on the rows with x0 = 0 and dead on the others, or the reverse.  The generator's and the
    critic's first layers read continuous rows (z, G(z), the interpolates): a unit switched by such an input crosses
    its kink somewhere along it, and at 512 rows x 400 units some (row, unit) pairs always land within 1e-3 of it
    (tried: 25 pairs, which mark 57 % of D.linear.weight), so those two keep one mask per unit here; their row-varying
    masks are exercised by the epoch tests at natural weights.  The oracle below still measures and caps what is left.
    With the critic's masks alike on every row and all its outputs live, the Wasserstein terms' +1/b and -1/b cancel
    in the critic's bias gradients: the oracle's are exactly 0, and the test measures those two against their layer's
    weight-gradient scale."""
    with torch.no_grad():
        c = 4.0
        H = m.E.linear.bias.numel()
        sign = torch.ones(H)
        sign[1::2] = -1.0
        switch = (torch.arange(H) % 4) >= 2
        for lin in (m.E.linear, m.G.linear, m.D.linear):
            lin.bias.copy_(c * sign)
        m.E.linear.weight[switch, 0] = -2.0 * c * sign[switch]
        # the critic's output: 2 + the rows' own variation around the live units' common level c
        m.D.discriminate.bias.fill_(2.0 - c * m.D.discriminate.weight[0, 0::2].sum().item())


def phase_grads_fp64(P0, x, draws, lz, lgp, thr):
    P = {k: v.clone().requires_grad_() for k, v in P0.items()}
    net = Net(P, thr)
    LE, LD, LG = phase_losses(net, x, draws, lz, lgp)
    out = {}
    for name, loss, pre in (("e", LE, "E."), ("d", LD(), "D."), ("g", LG(), "G.")):
        ks = [k for k in P if k.startswith(pre)]
        out[name] = dict(zip(ks, torch.autograd.grad(loss, [P[k] for k in ks])))
    return out, net.pre


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["64-48-8-b32", "784-400-20-b512"])
def test_teacher_forced_phase_gradients_vs_fp64(cfg):
    """One training batch with E_lr = G_lr = D_lr = 0: the parameters come out bitwise unchanged, and the three
    phases' gradients match fp64 autograd within 1e-5 of each tensor's scale, outside the elements the oracle marks
    as depending on a pre-activation within 1e-3 of a ReLU kink: those whose fp64 gradient changes when every such
    decision is moved one way (mask a > +1e-3) or the other (a > -1e-3).  The marked share is capped at 5 %."""
    b = cfg["batch"]
    its = loaders(b, b, b, 16, cfg["side"])
    torch.manual_seed(1234)
    m = pdw_gan.PDWGAN(cfg["I"], cfg["H"], cfg["Z"])
    kink_free_weights(m, cfg)
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tr = pdw_gan.PDWGANTrainer(m, *its)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1, E_lr=0.0, G_lr=0.0, D_lr=0.0)
    torch.cuda.synchronize()
    assert type(tr._engine).__name__ == "PDWGANEngine"
    for k, v in m.state_dict().items():
        assert torch.equal(v.cpu(), init[k]), k
    got = tr._engine.phase_grads()
    assert [len(got[p]) for p in ("e", "d", "g")] == [4, 4, 4]
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    Z = cfg["Z"]
    draws = (torch.randn(b, Z).double(), torch.rand(b, 1).double(), torch.randn(b, Z).double(),
             torch.randn(b, Z).double())
    x = its[0].dataset.tensors[0][perm].reshape(b, -1).double()
    P0 = {k: v.double() for k, v in init.items()}
    ref, pre = phase_grads_fp64(P0, x, draws, pkg.LAMBDA_Z, 10.0, 0.0)
    hi, _ = phase_grads_fp64(P0, x, draws, pkg.LAMBDA_Z, 10.0, BAND)
    lo, _ = phase_grads_fp64(P0, x, draws, pkg.LAMBDA_Z, 10.0, -BAND)
    near = sum(int((a.abs() < BAND).sum()) for a in pre)
    print("pre-activations within %.0e of a kink: %d of %d" % (BAND, near, sum(a.numel() for a in pre)))
    for phase in ("e", "d", "g"):
        for k, r in ref[phase].items():
            marked = hi[phase][k] != lo[phase][k]
            share = marked.double().mean().item()
            assert share <= 0.05, (phase, k, share)
            scale = r.abs().max().item()
            if scale == 0:                                  # (the critic's biases here: see kink_free_weights)
                scale = ref[phase][k.replace(".bias", ".weight")].abs().max().item()
            assert scale > 0, (phase, k)
            err = ((got[phase][k].cpu().double() - r).abs() * (~marked)).max().item()
            print("%s %s: %.3g of scale, marked %.3g" % (phase, k, err / scale, share))
            assert err <= 1e-5 * scale, (phase, k, err, scale)


# ---- the engine against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["64-48-8-b32-ragged", "784-400-20-b512-ragged"])
def test_pdwgan_engine_vs_oracle(cfg):
    tr, m, P, res, o_rng = run_both(cfg)
    assert type(tr._engine).__name__ == "PDWGANEngine"
    check_parity(tr, m, P, res, o_rng)


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["64-48-8-b32-ragged", "784-400-20-b512-ragged"])
def test_pdwgan_engine_vs_oracle_live_critic(cfg):
    """The same with the critic's output bias raised to 1, so that D(G(z)) > 0 and the generator phase has a gradient
    (and a loss that is not 0) from the first batch on."""
    tr, m, P, res, o_rng = run_both(cfg, prep=live_critic)
    assert min(abs(g) for g in tr.Glosses) > 0
    check_parity(tr, m, P, res, o_rng)


@pytest.mark.parametrize("wrong", ["rerun_encoder", "norm_only"])
def test_phase_order(wrong):
    """The engine matches the contract and NOT an oracle whose critic sees the coupling of the encoder after its step,
    or whose penalty is WGAN-GP's norm-only one (larger learning rates, so that one step moves the losses)."""
    cfg, lrs = dict(SMALL), dict(E_lr=1e-2, G_lr=1e-2, D_lr=1e-2)
    tr, m, P, res, o_rng = run_both(cfg, **lrs)
    check_parity(tr, m, P, res, o_rng)
    _, _, _, bad, _ = run_both(cfg, wrong=wrong, **lrs)
    err = max(abs(a - b) / max(1.0, abs(b)) for a, b in zip(tr.Dlosses, bad[1]))
    print("%s: D losses differ by %.3g" % (wrong, err))
    assert err > 1e-4, err                              # ten times the parity bound


def test_pdwgan_bitwise_eager_graph_and_resume(tmp_path):
    cfg = SMALL
    mk = lambda: loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"])
    runs = []
    for use_graph in (True, True, False):
        torch.manual_seed(99)
        tr, m = product(cfg, mk(), 2, use_graph=use_graph)
        runs.append((tr.Elosses, tr.Dlosses, tr.Glosses, {k: v.cpu().clone() for k, v in m.state_dict().items()},
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
    assert set(pkg.OPTIM_FIELDS) <= set(ck["optim"]) and set(ck["history"]) == set(pkg.HISTORY)
    assert ck["optim"]["steps"] == {"E": 7, "D": 7, "G": 7}
    state = torch.get_rng_state()
    m2 = pdw_gan.PDWGAN(cfg["I"], cfg["H"], cfg["Z"]).to(DEV)
    tr2 = pdw_gan.PDWGANTrainer(m2, *its)
    tr2.load_checkpoint(path)
    assert torch.equal(torch.get_rng_state(), state)
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    assert tr2.Elosses == runs[0][0] and tr2.Dlosses == runs[0][1] and tr2.Glosses == runs[0][2]
    assert torch.equal(torch.get_rng_state(), runs[0][4])
    for k, v in m2.state_dict().items():
        assert torch.equal(v.cpu(), runs[0][3][k]), k


def _general_vs_fused(cfg_fused, trainer_cls):
    """5 batches: the general path (an overridden hook) against the fused engine, losses and parameters <= 1e-5."""
    cfg = dict(cfg_fused, n_train=5 * cfg_fused["batch"])
    mk = lambda: loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"])
    torch.manual_seed(99)
    tf, mf = product(cfg, mk(), 1)
    rng = torch.get_rng_state()
    torch.manual_seed(99)
    tg, mg = product(cfg, mk(), 1, trainer_cls=trainer_cls)
    assert type(tf._engine).__name__ == "PDWGANEngine" and tg._engine is None
    assert torch.equal(torch.get_rng_state(), rng)
    for a, b, nm in ((tg.Elosses, tf.Elosses, "E"), (tg.Dlosses, tf.Dlosses, "D"), (tg.Glosses, tf.Glosses, "G")):
        lclose(a, b, what="general vs fused " + nm)
    assert abs(tg.best_val_loss - tf.best_val_loss) <= 1e-5 * max(1, abs(tf.best_val_loss))
    for k, v in mg.state_dict().items():
        assert (v - mf.state_dict()[k]).abs().max().item() <= 1e-5, k


def test_pdwgan_general_path_when_train_D_overridden():
    class Mine(pdw_gan.PDWGANTrainer):
        def train_D(self, images):
            return super().train_D(images)
    _general_vs_fused(SMALL, Mine)


def test_pdwgan_general_path_at_z6_vs_oracle():
    """Z = 6 is outside the fused limits (Z % 4), so there is no fused run to compare with: the general path, over 5
    batches, against the fp64 oracle, losses and parameters both at the general-vs-fused bound of 1e-5."""
    tr, m, P, res, o_rng = run_both(ODD)
    assert tr._engine is None
    check_parity(tr, m, P, res, o_rng, tol_w=1e-5)


def test_sample_reconstruct_parzen():
    its = loaders(32, 128, 64, 64, 8)
    torch.manual_seed(5)
    tr, m = product(dict(I=64, H=48, Z=8), its, 1)
    params = {k: v.clone() for k, v in m.state_dict().items()}
    st = torch.get_rng_state()
    s1, s2 = tr.sample(20, seed=3), tr.sample(20, seed=3)
    assert s1.shape == (20, 64) and torch.equal(s1, s2)
    rec = tr.reconstruct(its[2].dataset.tensors[0][:10])
    assert rec.shape == (10, 64) and bool(((rec >= 0) & (rec <= 1)).all())
    assert torch.equal(st, torch.get_rng_state())
    for k, v in m.state_dict().items():
        assert torch.equal(v, params[k]), k
    r = tr.parzen(n_samples=200, n_val=32)
    assert type(r).__name__ == "ParzenResult" and all(math.isfinite(v) for v in (r.sigma, r.ll_mean, r.ll_stderr))
    imgs = tr.generate_images(0, num_outputs=4, save=False)
    assert imgs.shape == (4, 8, 8)
