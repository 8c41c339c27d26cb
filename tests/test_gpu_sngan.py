"""Spectrally normalised hinge GAN on the MI355X: the power-iteration, head and gradient-projection kernels against fp64,
the flat Adam at both beta pairs, both steps' gradients against fp64 autograd, the fused engine against a plain-torch CPU
loop of sngan.py's contract (tests/sngan_reference.py) that replays the RNG protocol, an oracle with a frozen u the
engine must NOT match, determinism, resume, the general path, sampling and sigma().

Bounds are tests/test_gpu_aae.py's: 2e-5 of a tensor's max for a kernel against fp64, 1e-5 for losses, 5e-5 for
parameters and u, 1.5e-6 of a tensor's scale for lockstep gradients.  Every test first recomputes what fp32 alone costs
a plain-torch critic step against fp64 on the CPU (sngan_reference.fp32_allowance: worst loss 7.2e-8, gW 2.8e-7, gb
2.9e-7, gw2 2.6e-7, u 2.3e-7, v 3.6e-7, sigma 9.6e-8, s 4.2e-7 of the tensor's max over (B, I, H) = (4, 16, 8), (8, 20,
12), (5, 36, 24), (16, 784, 400)) and asserts that it is inside the bound it uses; no bound was widened."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import sn_gan  # noqa: E402
import sngan_reference as ref  # noqa: E402
from generative_models_amd import ops, ops_fused  # noqa: E402

DEV = "cuda"
KERNEL_TOL, LOSS_TOL, PARAM_TOL, LOCKSTEP_TOL = ref.KERNEL_TOL, ref.LOSS_TOL, ref.PARAM_TOL, ref.LOCKSTEP_TOL


@pytest.fixture(autouse=True)
def _allowance():
    """fp32 against fp64 in plain torch on the CPU stays inside the tightest bound used here."""
    a = ref.fp32_allowance()
    assert max(a.values()) <= LOCKSTEP_TOL, a


def close(got, want, name, tol=KERNEL_TOL):
    want = want.double()
    err = (got.detach().cpu().double().reshape(want.shape) - want).abs().max().item()
    scale = want.abs().max().item()
    print(name, "err", err, "max", scale)
    assert err <= tol * max(scale, 1e-30), (name, err, scale)


d = lambda t: t.float().to(DEV).contiguous()


# ---- the power iteration against fp64 -------------------------------------------------------------------------------
def run_power(W, u, w2, update=True, calls=1):
    """gm_sn_power_iter on fp32 copies: (u out, v, Wbar, w2bar, stats) as CPU tensors."""
    H, I = W.shape
    dW, du, dw2 = d(W), d(u), d(w2)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    v, Wbar, w2bar, stats = nan(I), nan(H, I), nan(H), nan(4)
    ws = ops_fused.sn_power_workspace(H, I, DEV)
    for _ in range(calls):
        ops_fused.sn_power_iter(dW, du, v, Wbar, dw2, w2bar, stats, ws, update_u=update)
    torch.cuda.synchronize()
    return [t.cpu() for t in (du, v, Wbar, w2bar, stats)]


def power_ref(W, u, w2, update=True):
    W, u, w2 = W.float().double(), u.float().double(), w2.float().double()       # the kernel's fp32 inputs, exactly
    u1, v = ref.power_step(W, u, update)
    sigma = u1 @ (W @ v)
    return u1, v, W / sigma, w2 / w2.norm(), sigma.item()


def check_power(W, u, w2, update=True):
    got = run_power(W, u, w2, update)
    u1, v, Wbar, w2bar, sigma = power_ref(W, u, w2, update)
    close(got[0], u1, "u")
    close(got[1], v, "v")
    close(got[2], Wbar, "Wbar")
    close(got[3], w2bar, "w2bar")
    st = got[4].double()
    assert abs(st[ops_fused.SN_SIGMA].item() - sigma) <= KERNEL_TOL * abs(sigma)
    assert abs(st[ops_fused.SN_NW2].item() - w2.float().double().norm().item()) <= KERNEL_TOL * w2.norm().item()
    return got, sigma


POWER_SHAPES = [(8, 16), (12, 20), (24, 36), (1024, 100), (400, 784)]


def power_case(H, I, seed=0):
    g = torch.Generator().manual_seed(1000 * H + I + seed)
    W = (torch.rand(H, I, generator=g) * 2 - 1) / I ** 0.5
    u = F.normalize(torch.randn(H, generator=g), dim=0)
    w2 = (torch.rand(H, generator=g) * 2 - 1) / H ** 0.5
    return W, u, w2


@pytest.mark.parametrize("H,I", POWER_SHAPES)
def test_power_iteration_vs_fp64(H, I):
    W, u, w2 = power_case(H, I)
    check_power(W, u, w2)
    # one zero row and one zero column: u' and v are exactly 0 there, Wbar too
    W[H // 2, :] = 0.0
    W[:, I // 3] = 0.0
    got, _ = check_power(W, u, w2)
    assert got[0][H // 2].item() == 0.0 and got[1][I // 3].item() == 0.0
    assert torch.all(got[2][H // 2, :] == 0) and torch.all(got[2][:, I // 3] == 0)
    # rank one: sigma is ||a|| ||b|| after a single step
    g = torch.Generator().manual_seed(H)
    a, b = torch.randn(H, generator=g), torch.randn(I, generator=g)
    W1 = torch.outer(a, b)
    got, _ = check_power(W1, u, w2)
    exact = (a.double().norm() * b.double().norm()).item()
    assert abs(got[4][ops_fused.SN_SIGMA].item() - exact) <= KERNEL_TOL * exact
    # eval mode: sigma from the stored u, which is left bit-unchanged
    got, _ = check_power(W, u, w2, update=False)
    assert torch.equal(got[0], u.float())


def test_power_iteration_converges_from_below():
    """A 24 x 36 W with singular values (2, 1, 1/2, ...): after 30 calls sigma is 2 within the kernel bound, and no call
    on the way exceeds the exact value by more than the bound."""
    g = torch.Generator().manual_seed(3)
    Q1, _ = torch.linalg.qr(torch.randn(24, 24, generator=g, dtype=torch.float64))
    Q2, _ = torch.linalg.qr(torch.randn(36, 36, generator=g, dtype=torch.float64))
    sv = torch.tensor([2.0] + [1.0 / k for k in range(1, 24)], dtype=torch.float64)
    W = ((Q1 * sv) @ Q2[:, :24].t()).float()
    exact = torch.linalg.svdvals(W.double())[0].item()
    assert abs(exact - 2.0) <= 1e-6
    _, u, w2 = power_case(24, 36)
    dW, du, dw2 = d(W), d(u), d(w2)
    z = lambda *s: torch.zeros(*s, device=DEV)
    v, Wbar, w2bar, stats = z(36), z(24, 36), z(24), z(4)
    ws = ops_fused.sn_power_workspace(24, 36, DEV)
    sig = []
    for _ in range(30):
        ops_fused.sn_power_iter(dW, du, v, Wbar, dw2, w2bar, stats, ws)
        sig.append(stats[:1].clone())
    sig = torch.cat(sig).cpu().double()
    print(sig)
    assert sig.max().item() <= exact * (1 + KERNEL_TOL)
    assert abs(sig[-1].item() - 2.0) <= KERNEL_TOL * 2.0
    close(Wbar, W.double() / 2.0, "Wbar")


# ---- the head against fp64 ---------------------------------------------------------------------------------------------
def head_case(B, Hd, gen_mode):
    """Hidden rows with dead columns and exact zeros; in critic mode both hinge branches occur in each half and every row
    is at least 1e-3 from its kink (a condition on the inputs: the first seed that meets it on the fp64 reference)."""
    rows = B if gen_mode else 2 * B
    for seed in range(10000):
        g = torch.Generator().manual_seed(100000 * Hd + 100 * B + seed)
        H = F.relu(torch.randn(rows, Hd, generator=g))
        H[:, : Hd // 4] = 0.0                            # columns whose h is 0 on every row
        w2 = torch.randn(Hd, generator=g)
        b2 = torch.randn(1, generator=g) * 0.5
        H = H * (2.5 / (H.double() @ (w2.double() / w2.double().norm())).abs().max().item())
        s = H.double() @ (w2.double() / w2.double().norm()) + b2.double()
        if gen_mode:
            return H, w2, b2
        on_r, on_f = (1 - s[:B]) > 0, (1 + s[B:]) > 0
        if on_r.any() and (~on_r).any() and on_f.any() and (~on_f).any() and ref.kink_distance(s, B) >= 1e-3:
            return H, w2, b2
    raise AssertionError("no seed meets the condition")


def head_ref(H, w2, b2, B, gen_mode):
    H, w2, b2 = (t.double().clone().requires_grad_() for t in (H, w2, b2))
    s = H @ (w2 / w2.norm()) + b2
    s.retain_grad()
    loss = ref.g_loss(s) if gen_mode else ref.d_loss(s, B)
    loss.backward()
    return loss.item(), s.detach(), s.grad, H.grad * (H > 0).double(), w2.grad, b2.grad


@pytest.mark.parametrize("gen_mode", [False, True], ids=["D", "G"])
@pytest.mark.parametrize("Hd", [8, 24, 400])
@pytest.mark.parametrize("B", [3, 8, 16])
def test_head_forward_and_backward_vs_fp64(B, Hd, gen_mode):
    H, w2, b2 = head_case(B, Hd, gen_mode)
    rows = H.shape[0]
    loss, s_r, ds_r, dPre_r, gw2_r, gb2_r = head_ref(H, w2, b2, B, gen_mode)
    if not gen_mode:                                     # asserted on the reference: both branches in each half, no row
        on_r, on_f = (1 - s_r[:B]) > 0, (1 + s_r[B:]) > 0        # within 1e-3 of its kink
        assert on_r.any() and (~on_r).any() and on_f.any() and (~on_f).any()
        assert ref.kink_distance(s_r, B) >= 1e-3
    nw2 = w2.double().norm()
    w2bar = (w2.double() / nw2).float()
    stats = torch.tensor([1.0, nw2.item(), 1.0, 1.0])
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    dH, s, ds, dPre, out = d(H), nan(rows), nan(rows), nan(rows, Hd), nan(1)
    ws = ops_fused.sn_head_workspace(rows, Hd, DEV)
    for _ in range(2):                                   # twice: the arrival counter re-arms itself
        out.fill_(float("nan"))
        ops_fused.sn_head_fwd(dH, d(w2bar), d(b2), B, gen_mode, s, ds, ws, loss_out=out)
    grads = None if gen_mode else (nan(1, Hd), nan(1))
    ops_fused.sn_head_bwd(dH, d(w2bar), B, gen_mode, ds, dPre, ws, stats=d(stats), grads=grads)
    torch.cuda.synchronize()
    print("loss", out.item(), loss)
    assert abs(out.item() - loss) <= LOSS_TOL * max(1.0, abs(loss))
    close(s, s_r, "s")
    assert torch.equal(ds.cpu(), ds_r.float())           # -1/B, 0 or +1/B: exact, every row
    close(dPre, dPre_r, "dPre")
    assert torch.all(dPre.cpu()[H == 0] == 0)            # exactly 0 where the hidden unit is off
    if gen_mode:
        return
    close(grads[0], gw2_r, "gw2")
    assert abs(grads[1].item() - gb2_r.item()) <= KERNEL_TOL
    # orthogonal to w2, up to the rounding of its terms
    assert abs((grads[0].cpu().double().view(-1) * w2.double()).sum().item()) <= KERNEL_TOL * gw2_r.abs().max().item() * nw2.item()


# ---- the gradient's projection and the flat Adam ---------------------------------------------------------------------
@pytest.mark.parametrize("H,I", POWER_SHAPES)
def test_grad_projection_vs_fp64(H, I):
    W, u, w2 = power_case(H, I, seed=1)
    g = torch.Generator().manual_seed(H + I)
    G = torch.randn(H, I, generator=g) * 1e-2
    u1, v, Wbar, _, sigma = power_ref(W, u, w2)
    Wbar32, u32, v32 = Wbar.float(), u1.float(), v.float()
    stats = torch.tensor([sigma, 1.0, 1.0, 1.0])
    want = ref.closed_gW(G.double(), Wbar32.double(), u32.double(), v32.double(), float(stats[0].double()))
    gW = torch.full((H, I), float("nan"), device=DEV)
    ops_fused.sn_grad(d(G), d(Wbar32), d(u32), d(v32), d(stats), gW, ops_fused.sn_grad_workspace(H, DEV))
    torch.cuda.synchronize()
    close(gW, want, "gW")
    # a G along Wbar (what scaling W would change) has no gradient left: <G, Wbar> u v^T cancels it up to rounding
    gW2 = torch.full((H, I), float("nan"), device=DEV)
    c = torch.outer(u32, v32)
    ops_fused.sn_grad(d(c), d(Wbar32), d(u32), d(v32), d(stats), gW2, ops_fused.sn_grad_workspace(H, DEV))
    cc = (c.double() * Wbar32.double()).sum()
    want2 = (c.double() - cc * c.double()) / sigma        # two terms of size |c| / sigma that cancel
    assert (gW2.cpu().double() - want2).abs().max().item() <= KERNEL_TOL * c.abs().max().item() / sigma


@pytest.mark.parametrize("betas", [(0.0, 0.9), (0.9, 0.999)], ids=["b0-0.9", "b0.9-0.999"])
def test_flat_adam_vs_torch_at_both_beta_pairs(betas):
    """Three steps of ops.adam over a flat buffer against torch.optim.Adam fed the same gradients.  One fp32 rounding of
    a parameter of size ~1 is 6e-8; three steps stay within 1e-6 (tests/test_gpu_acgan.py's bound for one)."""
    g = torch.Generator().manual_seed(11)
    n, lr = 1000, 4e-4
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 10 ** float(k - 2) for k in range(3)]
    grads[1][:10] = 0.0
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=lr, betas=betas)
    dp, m, v = d(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    sched = torch.from_numpy(ops.adam_schedule(lr, 3, betas=betas)).to(DEV)
    for k, gg in enumerate(grads):
        p.grad = gg.clone()
        opt.step()
        ops.adam(dp, d(gg), m, v, sched, sched_slot=ops.slot(0, 0, k, 0, 1), betas=betas)
    torch.cuda.synchronize()
    err = (dp.cpu() - p.detach()).abs().max().item()
    print("adam", betas, err)
    assert err <= 1e-6
    assert (dp.cpu() - p0).abs().max().item() > 0.5 * lr     # it moved


# ---- the trainer against the plain-torch oracle ------------------------------------------------------------------------
def loaders(batch, n_train, n_test, side, seed=7):
    """Loaders over a private generator's images; they shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, 1, side, side), 0.3), generator=g)
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64)),
                                           batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_test), mk(n_test)


SMALL = dict(I=16, H=8, Z=4, side=4, batch=8, n_train=32, n_test=16, epochs=1)           # 4 iterations
FULL = dict(I=784, H=400, Z=20, side=28, batch=16, n_train=32, n_test=16, epochs=1)      # 2 iterations
MODEL_SEED, DATA_SEED = 1234, 99

_ORACLE = {}


def oracle_run(cfg, dtype=torch.float32, freeze_u=False, **kw):
    """The oracle's run of a configuration, computed once and shared: (oracle, (Glosses, Dlosses), RNG state after)."""
    key = (tuple(sorted(cfg.items())), dtype, freeze_u, tuple(sorted(kw.items())))
    if key not in _ORACLE:
        torch.manual_seed(DATA_SEED)
        its = loaders(cfg["batch"], cfg["n_train"], cfg["n_test"], cfg["side"])
        torch.manual_seed(MODEL_SEED)
        o = ref.Oracle(sn_gan.SNGAN(cfg["I"], cfg["H"], cfg["Z"]), dtype, freeze_u)
        res = ref.oracle_train(o, its[0], cfg["epochs"], **kw)
        _ORACLE[key] = (o, res, torch.get_rng_state())
    return _ORACLE[key]


def product_run(cfg, trainer_cls=None, use_graph=True, **kw):
    torch.manual_seed(DATA_SEED)
    its = loaders(cfg["batch"], cfg["n_train"], cfg["n_test"], cfg["side"])
    torch.manual_seed(MODEL_SEED)
    m = sn_gan.SNGAN(cfg["I"], cfg["H"], cfg["Z"])
    tr = (trainer_cls or sn_gan.SNGANTrainer)(m, *its)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(cfg["epochs"], **kw)
    torch.cuda.synchronize()
    return tr, m, its


def lclose(got, want, tol=LOSS_TOL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert err.max() <= tol, (err.max(), got[:4], want[:4])


def param_gap(m, o):
    st = o.state()
    return max((v.cpu().double() - st[k].double()).abs().max().item() for k, v in m.state_dict().items())


def check_parity(tr, m, o, res, o_rng):
    Gl, Dl = res
    lclose(tr.Dlosses, Dl)
    lclose(tr.Glosses, Gl)
    assert torch.equal(torch.get_rng_state(), o_rng)
    st = o.state()
    assert set(st) == set(m.state_dict())
    for k, v in m.state_dict().items():                  # the parameters and u
        gap = (v.cpu().double() - st[k].double()).abs().max().item()
        print(k, gap)
        assert gap <= PARAM_TOL, (k, gap)


def no_kink_nearby(cfg, **kw):
    """On the oracle's fp64 run no critic-step row comes within 1e-4 of a hinge kink over the compared steps."""
    o64, _, _ = oracle_run(cfg, dtype=torch.float64, **kw)
    print("closest hinge kink", o64.min_kink)
    assert o64.min_kink >= 1e-4, o64.min_kink


@pytest.mark.parametrize("cfg,kw", [(SMALL, {}), (SMALL, dict(D_steps=2)), (FULL, {})],
                         ids=["16-8-4-b8", "16-8-4-b8-Dsteps2", "784-400-20-b16"])
def test_engine_vs_oracle(cfg, kw):
    if kw:
        cfg = dict(cfg, n_train=64)                      # 4 iterations of 2 critic steps
    no_kink_nearby(cfg, **kw)
    o, res, o_rng = oracle_run(cfg, **kw)
    tr, m, _ = product_run(cfg, **kw)
    assert type(tr._engine).__name__ == "SNGANEngine"
    assert len(tr.Glosses) == (4 if cfg["H"] == 8 else 2)
    check_parity(tr, m, o, res, o_rng)


def test_an_oracle_that_never_updates_u_does_not_match():
    """At lr 1e-2 the engine is far from an oracle whose u stays at its initial value in every forward: the parity test
    would notice a power iteration that does not run (or runs once per iteration instead of twice)."""
    kw = dict(G_lr=1e-2, D_lr=1e-2)
    tr, m, _ = product_run(SMALL, **kw)
    o, _, _ = oracle_run(SMALL, **kw)
    bad, _, _ = oracle_run(SMALL, freeze_u=True, **kw)
    right, wrong = param_gap(m, o), param_gap(m, bad)
    print("gap to the oracle", right, "gap to the frozen-u oracle", wrong)
    assert wrong > 10 * PARAM_TOL, wrong                 # ten times the parity bound
    st = bad.state()
    w_gap = max((v.cpu().double() - st[k].double()).abs().max().item() for k, v in m.state_dict().items() if k != "D.u")
    assert w_gap > 10 * PARAM_TOL, w_gap                 # in the weights too, not only in u itself


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["16-8-4-b8", "784-400-20-b16"])
def test_teacher_forced_step_gradients_vs_fp64(cfg):
    """One iteration with G_lr = D_lr = 0: the parameters come out bitwise unchanged, u has advanced twice, and both
    steps' gradients match fp64 autograd at the initial weights within 1.5e-6 of each tensor's scale."""
    b = cfg["batch"]
    its = loaders(b, b, 16, cfg["side"])
    torch.manual_seed(MODEL_SEED)
    m = sn_gan.SNGAN(cfg["I"], cfg["H"], cfg["Z"])
    init = {k: v.detach().clone() for k, v in m.state_dict().items()}
    o = ref.Oracle(m, torch.float64)
    tr = sn_gan.SNGANTrainer(m, *its)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1, G_lr=0.0, D_lr=0.0)
    torch.cuda.synchronize()
    assert type(tr._engine).__name__ == "SNGANEngine"
    for k, v in m.state_dict().items():
        assert k == "D.u" or torch.equal(v.cpu(), init[k]), k
    got = tr._engine.phase_grads()
    assert [len(got[p]) for p in ("d", "g")] == [4, 4]
    torch.set_rng_state(st)
    x, _ = next(iter(its[0]))
    x = x.view(b, -1).double()
    zD, zG = torch.randn(b, cfg["Z"]).double(), torch.randn(b, cfg["Z"]).double()
    dl = o.d_loss(x, zD)
    assert o.min_kink >= 1e-4
    gd = dict(zip(o.D_KEYS, torch.autograd.grad(dl, o.dparams())))
    gg = dict(zip(o.G_KEYS, torch.autograd.grad(o.g_loss(zG), o.gparams())))
    close(m.D.u, o.u, "u after two power iterations", PARAM_TOL)
    lclose(tr.Dlosses, [dl.item()])
    for phase, refs in (("d", gd), ("g", gg)):
        assert set(refs) == set(got[phase])
        for k, r in refs.items():
            scale = r.abs().max().item()
            assert scale > 0 or k == "D.discriminate.bias", (phase, k)      # (gb2 is 0 while every hinge term is active)
            err = (got[phase][k].cpu().double() - r).abs().max().item()
            print(phase, k, err / max(scale, 1e-30))
            assert err <= LOCKSTEP_TOL * (scale if scale > 0 else 1.0 / b), (phase, k, err, scale)


def _snapshot(tr, m):
    return (list(tr.Glosses), list(tr.Dlosses), {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state())


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[3], b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize("D_steps", [1, 2])
def test_bitwise_runs_graph_eager_and_resume(tmp_path, D_steps):
    """Ring rows i * D_steps + j across the boundary between the graph of 16 and the tail, and across a resume."""
    cfg = dict(SMALL, n_train=8 * 18 * D_steps, epochs=2)    # 18 iterations an epoch: a graph of 16 and two of 1
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
    assert set(ck["history"]) == {"Glosses", "Dlosses", "num_epochs"} and "D.u" in ck["model"]
    assert ck["optim"]["G"]["step"] == 18 and ck["optim"]["D"]["step"] == 18 * D_steps
    assert ck["optim"]["config"]["beta1"] == 0.0 and ck["optim"]["config"]["beta2"] == 0.9
    state = torch.get_rng_state()
    m2 = sn_gan.SNGAN(cfg["I"], cfg["H"], cfg["Z"]).to(DEV)
    tr2 = sn_gan.SNGANTrainer(m2, *its)
    tr2.load_checkpoint(path)
    assert torch.equal(torch.get_rng_state(), state)
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1, D_steps=D_steps)
    torch.cuda.synchronize()
    _same(runs[0], _snapshot(tr2, m2))


def test_general_path_when_train_D_overridden():
    class Mine(sn_gan.SNGANTrainer):
        def train_D(self, images):
            return super().train_D(images)
    no_kink_nearby(SMALL)
    o, res, o_rng = oracle_run(SMALL)
    tr, m, _ = product_run(SMALL, trainer_cls=Mine)
    assert tr._engine is None
    check_parity(tr, m, o, res, o_rng)


def test_general_path_outside_the_limits():
    cfg = dict(SMALL, H=10)                              # H % 4 != 0
    no_kink_nearby(cfg)
    o, res, o_rng = oracle_run(cfg)
    tr, m, _ = product_run(cfg)
    assert tr._engine is None
    check_parity(tr, m, o, res, o_rng)


def test_sample_parzen_sigma_and_eval_forward():
    tr, m, its = product_run(SMALL, G_lr=1e-2, D_lr=1e-2)
    o = ref.Oracle(m)
    st = torch.get_rng_state()
    s1, s2 = tr.sample(7, seed=3), tr.sample(7, seed=3)
    assert s1.shape == (7, 16) and torch.equal(s1, s2) and not torch.equal(s1, tr.sample(7, seed=4))
    z = torch.randn(7, SMALL["Z"], generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        assert (s1.cpu() - o.G(z)).abs().max().item() <= KERNEL_TOL
    r = tr.parzen(n_samples=64, n_val=16)
    assert type(r).__name__ == "ParzenResult" and all(math.isfinite(v) for v in (r.sigma, r.ll_mean, r.ll_stderr))
    images = tr.generate_images(0, num_outputs=4, save=False)
    assert images.shape == (4, 4, 4) and np.isfinite(images).all()
    torch.set_rng_state(st)
    # the running estimate never exceeds the exact spectral norm; an eval-mode forward leaves u alone and matches the
    # contract's eval forward
    est, exact = tr.sigma(), tr.sigma(exact=True)
    print("sigma", est, exact)
    assert 0 < est <= exact * (1 + KERNEL_TOL)
    u0 = m.D.u.clone()
    x = its[2].dataset.tensors[0].view(-1, 16)
    m.eval()
    with torch.no_grad():
        s_eval = m.D(x.to(DEV))[:, 0]
    assert torch.equal(m.D.u, u0)
    p = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    want, _ = ref.critic(x.double(), p["D.linear.weight"], p["D.linear.bias"], p["D.discriminate.weight"],
                         p["D.discriminate.bias"], p["D.u"], training=False)
    close(s_eval, want, "eval logits")
    m.train()
    with torch.no_grad():
        m.D(x.to(DEV))
    assert not torch.equal(m.D.u, u0)                    # a training-mode forward advances u
    assert torch.equal(st, torch.get_rng_state())        # nothing here drew from the global generator
