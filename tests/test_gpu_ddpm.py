"""Denoising diffusion on the MI355X: the q-sample kernels against the numpy rule and the plain gather, the loss and the
reverse-step kernels against fp64, the fused engine against an fp64 CPU loop that replays DDPMTrainer's RNG protocol on
the device's (checked) rows, gradients against fp64 autograd, determinism and resume, the general path, the sampler step
by step, and learning itself."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))
sys.path.insert(0, HERE)

import ddpm  # noqa: E402
import ddpm_reference as R  # noqa: E402
from generative_models_amd import ops, trainers  # noqa: E402
from generative_models_amd import ddpm as gddpm  # noqa: E402
from generative_models_amd import ops_fused as of_  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"


def _tables(T, E):
    tab = gddpm.tables(T, E)
    dev = {k: torch.from_numpy(tab[k].astype(np.float32)).to(DEV) for k in ("sa", "s1", "temb")}
    return of_.ddpm_tables(dev["sa"], dev["s1"], dev["temb"]), dev


def _data(packed, n, I, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.bernoulli(torch.full((n, I), 0.3), generator=g) if packed else torch.rand(n, I, generator=g)
    return x, (ops.PackedData(x.to(DEV)) if packed else x.to(DEV))


# ---- q-sample ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,I,E,T", [(37, 64, 8, 50), (5, 30, 4, 2), (64, 784, 32, 1000)],
                         ids=["37x64", "5x30-scalar-tails", "64x784"])
def test_qsample_against_the_rule(b, I, E, T):
    tab, _ = _tables(T, E)
    g = torch.Generator().manual_seed(b)
    x = torch.rand(b, I, generator=g)
    for train in (True, False):
        for seed, step, row0 in [(0, 0, 0), ((1 << 64) - 1, 77, 3), (0x123456789ABCDEF, 1 << 20, 511)]:
            xin, eps, t = of_.ddpm_qsample(x.to(DEV), of_.ddpm_noise(seed, train, step=step, row0=row0), tab)
            R.close_rule(xin.cpu().numpy(), eps.cpu().numpy(), t.cpu().numpy(), x.numpy(), T, E, seed, step, train, row0)
    nz = of_.ddpm_noise(9, True, step=3)
    a, b2 = of_.ddpm_qsample(x.to(DEV), nz, tab), of_.ddpm_qsample(x.to(DEV), nz, tab)
    assert all(torch.equal(u, v) for u, v in zip(a, b2))       # two calls: the same bits
    assert all(torch.equal(u, v) for u, v in zip(a, of_.ddpm_qsample(x.to(DEV), of_.ddpm_noise(9, True,
                                                                                                step=(1 << 32) + 3), tab)))
    # strided rows in and out: nothing written past a row's I + E (xin) / I (eps) floats, nor past row b
    big = torch.rand(b + 2, I + 9, generator=g).to(DEV)
    xs = big[:b, 3:3 + I]
    xin = torch.full((b + 2, I + E + 5), -7.0, device=DEV)
    eps = torch.full((b + 2, I + 3), -7.0, device=DEV)
    t = torch.full((b + 2,), -7, dtype=torch.int32, device=DEV)
    of_.ddpm_qsample(xs, nz, tab, xin=xin[:b], eps=eps[:b], t=t)
    want = of_.ddpm_qsample(xs.contiguous(), nz, tab)
    assert torch.equal(xin[:b, :I + E], want[0]) and torch.equal(eps[:b, :I], want[1]) and torch.equal(t[:b], want[2])
    assert torch.all(xin[:, I + E:] == -7.0) and torch.all(eps[:, I:] == -7.0)
    assert torch.all(xin[b:] == -7.0) and torch.all(eps[b:] == -7.0) and torch.all(t[b:] == -7)
    # a device counter plus a device base equals the same step given as a value
    ctr = torch.tensor([40], dtype=torch.int64, device=DEV)
    base = torch.tensor([1000], dtype=torch.int64, device=DEV)
    via = of_.ddpm_qsample(x.to(DEV), of_.ddpm_noise(11, True, step=2, step_ctr=ctr, step_base=base), tab)
    assert all(torch.equal(u, v) for u, v in zip(via, of_.ddpm_qsample(x.to(DEV), of_.ddpm_noise(11, True, step=1042), tab)))
    assert not torch.equal(via[1], of_.ddpm_qsample(x.to(DEV), of_.ddpm_noise(11, True, step=1041), tab)[1])


@pytest.mark.parametrize("packed", [True, False], ids=["bits", "fp32"])
@pytest.mark.parametrize("I,E,T", [(64, 8, 50), (30, 4, 2), (784, 32, 1000)])
def test_gathering_qsample_equals_gather_then_qsample(packed, I, E, T):
    tab, _ = _tables(T, E)
    x, data = _data(packed, 300, I)
    g = torch.Generator().manual_seed(I)
    B = 64
    idx = torch.randint(0, x.shape[0], (3, B), generator=g).to(DEV)
    ctr = torch.tensor([5], dtype=torch.int64, device=DEV)
    base = torch.tensor([100], dtype=torch.int64, device=DEV)
    ld = (I + E + 3) // 4 * 4
    for b in (B, 37, 5):
        slot = ops.slot(ctr.data_ptr(), 1, 0, 3, B)              # idx slot: row ctr % 3 of the ring
        X, ref = torch.full((B, I), -1.0, device=DEV), torch.full((B, I), -1.0, device=DEV)
        xin, eps = torch.full((B, ld), -1.0, device=DEV), torch.full((B, I), -1.0, device=DEV)
        t = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        for train in (True, False):
            of_.gather_rows_qsample(data, idx.view(-1), X, xin, eps, t,
                                    of_.ddpm_noise(77, train, step_ctr=ctr, step_base=base), tab, B=b, idx_slot=slot)
            ops.gather_rows(data, idx.view(-1), ref, B=b, idx_slot=slot)
            assert torch.equal(X, ref)                          # the clean rows: exactly the plain gather's
            want = of_.ddpm_qsample(ref[:b].contiguous(), of_.ddpm_noise(77, train, step=105), tab)
            assert torch.equal(xin[:b, :I + E], want[0]) and torch.equal(eps[:b], want[1]) and torch.equal(t[:b], want[2])
            assert torch.all(xin[b:] == -1.0) and torch.all(eps[b:] == -1.0) and torch.all(t[b:] == -1)
            assert torch.all(xin[:, I + E:] == -1.0)


def test_qsample_statistics_over_a_million_draws():
    T, E, n, I = 50, 8, 1 << 20, 4                             # 2^20 timesteps, 2^22 normals
    tab, _ = _tables(T, E)
    x = torch.full((n, I), 0.5, device=DEV)                    # x0 = 0: x_t = s1_t eps
    xin, eps, t = of_.ddpm_qsample(x, of_.ddpm_noise(123, True, step=9), tab)
    cnt = torch.bincount(t.long(), minlength=T).double().cpu().numpy()
    p = 1.0 / T
    assert cnt.sum() == n and np.all(np.abs(cnt - n * p) <= 5 * (n * p * (1 - p)) ** 0.5), cnt
    e = eps.double()
    N = n * I
    m, v = e.mean().item(), e.var().item()
    assert abs(m) <= 5 / N ** 0.5 and abs(v - 1) <= 5 * (2 / N) ** 0.5, (m, v)
    ku = ((e - m) ** 4).mean().item() / v ** 2
    assert abs(ku - 3) <= 5 * (24 / N) ** 0.5, ku
    e2 = of_.ddpm_qsample(x, of_.ddpm_noise(123, True, step=10), tab)[1].double()
    assert abs((e * e2).mean().item()) <= 5 / N ** 0.5          # steps are uncorrelated
    assert abs((e[:, 0] * (t.double() - (T - 1) / 2)).mean().item()) <= 5 * ((T * T - 1) / 12 / n) ** 0.5   # t and eps too


# ---- loss ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,I", [(37, 64), (5, 30), (512, 784)])
def test_loss_kernel_against_fp64(b, I):
    g = torch.Generator().manual_seed(I)
    out, eps = torch.randn(b, I, generator=g), torch.randn(b, I, generator=g)
    scale = float(np.float32(1.0 / (b * I)))
    part, dA, res = torch.zeros(b + 1, device=DEV), torch.full((b + 1, I), -7.0, device=DEV), torch.zeros(1, device=DEV)
    runs = []
    for _ in range(2):
        of_.ddpm_loss(out.to(DEV), eps.to(DEV), part, b, scale, dA=dA)
        of_.sum_finalize(part, b, res, scale=scale)
        runs.append((dA.clone(), part.clone(), res.clone()))
    assert all(torch.equal(u, v) for u, v in zip(*runs))         # run to run: the same bits
    d = out.double() - eps.double()
    ref_dA = 2.0 * scale * d
    assert (dA[:b].cpu().double() - ref_dA).abs().max().item() <= R.GRAD_TOL * ref_dA.abs().max().item()
    assert torch.all(dA[b:] == -7.0) and part[b].item() == 0.0
    rows = (d ** 2).sum(1)
    assert ((part[:b].cpu().double() - rows).abs() / rows).max().item() <= R.LOSS_TOL
    ref = rows.sum().item() * scale
    assert abs(res.item() - ref) <= R.LOSS_TOL * max(1.0, abs(ref))
    part2 = torch.zeros(b, device=DEV)
    of_.ddpm_loss(out.to(DEV), eps.to(DEV), part2, b, scale)   # validation: no dA
    assert torch.equal(part2, part[:b])


# ---- reverse step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,I,E,T", [(33, 64, 8, 50), (5, 30, 4, 2)])
def test_reverse_step_against_fp64(n, I, E, T):
    _, dev = _tables(T, E)
    temb = dev["temb"]
    g = torch.Generator().manual_seed(n)
    S = min(T, 10)
    ld = (I + E + 3) // 4 * 4
    for eta in (0.0, 0.5, 1.0):
        coef64, tau = gddpm.reverse_table(T, S, eta)
        coef = torch.from_numpy(coef64.astype(np.float32)).to(DEV)
        c32 = coef.cpu().double().numpy()
        for clip in (True, False):
            for s in sorted({S // 2, S - 1}):                    # a middle step and the last one
                xt, e = 1.5 * torch.randn(n, I, generator=g), torch.randn(n, I, generator=g)
                outs = []
                for seed in (5, 6):
                    xin = torch.full((n + 1, ld + 4), -7.0, device=DEV)
                    xin[:n, :I] = xt.to(DEV)
                    of_.ddpm_reverse(xin[:, :ld], e.to(DEV), coef, temb, I, seed, clip=clip, step=s, rows=n)
                    outs.append(xin)
                    z = gddpm.noise_reference(n, I, seed, s, gddpm.TAG_S) if coef64[s, 4] != 0 else np.zeros((n, I))
                    ref = R.reverse_step(xt.double().numpy(), e.double().numpy(), z, c32[s], clip)
                    got = xin[:n, :I].cpu().double().numpy()
                    scale = np.maximum(1.0, np.abs(ref).max(1, keepdims=True))
                    assert (np.abs(got - ref) / scale).max() <= R.STEP_TOL, (eta, clip, s)
                    if s < S - 1:                                # the tail: temb[t_next], bit for bit
                        assert torch.equal(xin[:n, I:I + E], temb[int(tau[s + 1])].expand(n, E))
                    else:
                        assert torch.all(xin[:n, I:I + E] == -7.0)
                    assert torch.all(xin[n:] == -7.0) and torch.all(xin[:, I + E:] == -7.0)
                same = torch.equal(outs[0], outs[1])
                assert same == (coef64[s, 4] == 0), (eta, s)     # eta = 0 and the last step: no bit depends on the seed
                if coef64[s, 4] != 0 and not clip:               # z itself, against the rule: the two seeds' difference
                    dz = gddpm.noise_reference(n, I, 5, s, gddpm.TAG_S) - gddpm.noise_reference(n, I, 6, s, gddpm.TAG_S)
                    got = (outs[0][:n, :I].double() - outs[1][:n, :I].double()).cpu().numpy() / c32[s, 4]
                    assert np.abs(got - dz).max() <= 20 * R.STEP_TOL / c32[s, 4]
    # a slot over a device counter, the tick by the launch, the trajectory rows
    coef64, tau = gddpm.reverse_table(T, S, 1.0)
    coef = torch.from_numpy(coef64.astype(np.float32)).to(DEV)
    ctr, done = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    xt, e = torch.randn(n, I, generator=g).to(DEV), torch.randn(n, I, generator=g).to(DEV)
    a, b = torch.zeros(n, ld, device=DEV), torch.zeros(n, ld, device=DEV)
    a[:, :I], b[:, :I] = xt, xt
    traj = torch.full((S + 1, n, I), -7.0, device=DEV)
    for s in range(2):
        of_.ddpm_reverse(a, e, coef, temb, I, 3, slot=ops.slot(ctr.data_ptr(), 1, 0, 0, 8), traj=traj, tick=ctr, done=done)
        of_.ddpm_reverse(b, e, coef, temb, I, 3, step=s)
        assert torch.equal(a, b) and ctr.item() == s + 1 and done.item() == 0
        assert torch.equal(traj[s + 1], a[:, :I])
    assert torch.all(traj[0] == -7.0) and torch.all(traj[3:] == -7.0)
    xin = torch.zeros(n, ld, device=DEV)
    of_.ddpm_prior(xin, temb, I, 3, step=S, t=int(tau[0]), traj=traj[0])
    z = gddpm.noise_reference(n, I, 3, S, gddpm.TAG_S)
    assert (np.abs(xin[:, :I].cpu().double().numpy() - z) / np.maximum(1.0, np.abs(z))).max() <= R.NORMAL_TOL
    assert torch.equal(xin[:, I:I + E], temb[int(tau[0])].expand(n, E)) and torch.equal(traj[0], xin[:, :I])


# ---- the engine against the fp64 oracle ------------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, side, seed=7, binary=True):
    """Image loaders; the data come from a private generator, the loaders shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, side * side), 0.3), generator=g) if binary else \
            torch.rand(n, side * side, generator=g)
        ds = torch.utils.data.TensorDataset(x.view(n, 1, side, side), torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


SMALL = dict(I=64, H=48, E=8, T=50, side=8, batch=32, n_train=200, n_val=48, n_test=48, epochs=2)
SMALL_FP32 = dict(SMALL, binary=False)
ODD = dict(SMALL, I=49, side=7, E=4)                        # I and I + E no multiples of 4: the scalar tails
FULL = dict(I=784, H=400, E=32, T=1000, side=28, batch=512, n_train=3 * 512 + 336, n_val=512, n_test=64, epochs=1)


def mk_loaders(cfg):
    return loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"], binary=cfg.get("binary", True))


def mk_model(cfg):
    torch.manual_seed(1234)
    return ddpm.DDPM(cfg["I"], cfg["H"], cfg["E"], cfg["T"])


def product(cfg, its, epochs, seed=0, use_graph=True, trainer_cls=None, model=None):
    m = mk_model(cfg) if model is None else model
    tr = (trainer_cls or ddpm.DDPMTrainer)(m, *its, seed=seed)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs)
    torch.cuda.synchronize()
    return tr, m


def device_rows(cfg, seed):
    """The oracle's source of rows: the device's q-sample of a batch, each row checked against the numpy rule."""
    tab, _ = _tables(cfg["T"], cfg["E"])
    I, E = cfg["I"], cfg["E"]

    def rows(x, step, train):
        xin, eps, t = of_.ddpm_qsample(x.to(DEV), of_.ddpm_noise(seed, train, step=step), tab)
        R.close_rule(xin.cpu().numpy(), eps.cpu().numpy(), t.cpu().numpy(), x.numpy(), cfg["T"], E, seed, step, train)
        return xin[:, :I + E].cpu().double(), eps.cpu().double()
    return rows


def lclose(got, ref, tol=R.LOSS_TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= tol, (err.max(), got[:4], ref[:4])


def parity(cfg, trainer_cls=None, seed=5):
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    init = mk_model(cfg)
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    losses, best, P = R.oracle_train(init.state_dict(), its, cfg["epochs"], device_rows(cfg, seed))
    o_rng = torch.get_rng_state()
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, cfg["epochs"], seed=seed, trainer_cls=trainer_cls, model=init)
    print("losses", tr.losses[:3], losses[:3], "best", tr.best_val_loss, best)
    lclose(tr.losses, losses)
    assert abs(tr.best_val_loss - best) <= R.LOSS_TOL * max(1, abs(best))
    assert torch.equal(torch.get_rng_state(), o_rng)           # the loaders' shuffles and nothing else
    assert tr.noise_steps == cfg["epochs"] * len(its[0]) and tr.num_epochs == cfg["epochs"]
    worst = {k: (v.cpu().double() - P[k]).abs().max().item() for k, v in m.state_dict().items()}
    print("max |w - oracle|", worst)
    assert max(worst.values()) <= R.PARAM_TOL, worst
    return tr


@pytest.mark.parametrize("cfg", [SMALL, SMALL_FP32, ODD, FULL], ids=["small-ragged", "small-fp32", "49-4-tails",
                                                                     "784-400-32-b512"])
def test_engine_vs_fp64_oracle(cfg):
    tr = parity(cfg)
    assert type(tr._engine).__name__ == "DDPMEngine"


@pytest.mark.parametrize("cfg", [SMALL, ODD, FULL], ids=["small", "49-4-tails", "784-400-32-b512"])
def test_teacher_forced_batch_gradients_vs_fp64(cfg):
    """One training batch through DDPMEngine from known weights: every gradient it leaves in the flat gradient buffer
    against fp64 autograd on the device's rows of that batch, within 1.5e-6 of each tensor's scale."""
    b = cfg["batch"]
    its = loaders(b, b, b, 16, cfg["side"])
    m = mk_model(cfg)
    init = R.f64(m.state_dict())
    tr = ddpm.DDPMTrainer(m, *its, seed=3)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    torch.cuda.synchronize()
    fp = tr._engine.fp
    got = {k: fp.gviews[[i for i, q in enumerate(fp.params) if q is p][0]].cpu().double()
           for k, p in m.named_parameters()}
    assert len(got) == 6
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].reshape(b, -1)
    xin, eps = device_rows(cfg, 3)(x, 0, True)
    loss, grads, _ = R.loss_and_grads(init, xin, eps)
    assert abs(tr.losses[0] - loss) <= R.LOSS_TOL * max(1.0, abs(loss))
    for k, gk in got.items():
        scale = grads[k].abs().max().item()
        assert scale > 0, k
        err = (gk - grads[k]).abs().max().item()
        assert err <= R.GRAD_TOL * scale, (k, err, scale)


def snapshot(tr, m):
    return (list(tr.losses), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state(), tr.noise_steps)


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
    assert torch.equal(a[3], b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_bitwise_reproducibility_and_resume(tmp_path):
    cfg = SMALL
    runs = []
    for use_graph in (True, True, False):                   # graph twice (same seed), then eager
        torch.manual_seed(99)
        runs.append(snapshot(*product(cfg, mk_loaders(cfg), 2, use_graph=use_graph)))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    torch.manual_seed(99)
    other = snapshot(*product(cfg, mk_loaders(cfg), 2, seed=6))
    assert other[0] != runs[0][0] and any(not torch.equal(other[2][k], runs[0][2][k]) for k in other[2])
    # train(1) + save + load into a fresh trainer + train(1) == train(2): the noise stream and Adam's steps continue
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 1)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    m2 = ddpm.DDPM(cfg["I"], cfg["H"], cfg["E"], cfg["T"]).to(DEV)
    tr2 = ddpm.DDPMTrainer(m2, *its, seed=0)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == len(its[0])
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    same(snapshot(tr2, m2), runs[0])
    # a checkpoint of other settings is refused under strict=True, taken under strict=False
    for bad in (dict(seed=1), dict(T=60), dict(E=4)):
        c2 = dict(cfg, **{k: v for k, v in bad.items() if k != "seed"})
        t3 = ddpm.DDPMTrainer(ddpm.DDPM(c2["I"], c2["H"], c2["E"], c2["T"]).to(DEV), *its, seed=bad.get("seed", 0))
        if "E" in bad:
            with pytest.raises(RuntimeError):
                t3.load_checkpoint(path)                       # the first layer's shape differs
            continue
        t3.load_checkpoint(path)
        with pytest.raises(GMError):
            t3.train(1)
    t3 = ddpm.DDPMTrainer(ddpm.DDPM(cfg["I"], cfg["H"], cfg["E"], cfg["T"]).to(DEV), *its, seed=1)
    t3.load_checkpoint(path, strict=False)
    with contextlib.redirect_stdout(io.StringIO()):
        t3.train(1)


def test_general_path_agrees_with_the_fused_run():
    class Mine(ddpm.DDPMTrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    cfg = dict(SMALL, n_train=96)
    tr = parity(cfg, trainer_cls=Mine)
    assert tr._engine is None


# ---- the sampler ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained_small():
    cfg = SMALL
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 2)
    return cfg, tr, m


@pytest.mark.parametrize("eta,clip", [(1.0, True), (0.0, True), (0.5, False)])
def test_sampler_step_by_step(trained_small, eta, clip):
    cfg, tr, m = trained_small
    I, E, T, n, S = cfg["I"], cfg["E"], cfg["T"], 33, 10
    before = {k: v.clone() for k, v in m.state_dict().items()}
    st, mode = torch.get_rng_state(), m.training
    out, traj = tr.sample(n, seed=4, steps=S, eta=eta, clip=clip, return_trajectory=True)
    assert torch.equal(st, torch.get_rng_state()) and m.training == mode
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert tuple(out.shape) == (n, I) and tuple(traj.shape) == (S + 1, n, I)
    assert out.min().item() >= 0.0 and out.max().item() <= 1.0
    assert torch.equal(out, ((traj[-1] + 1) / 2).clamp(0, 1))
    coef64, tau = gddpm.reverse_table(T, S, eta)
    c32 = coef64.astype(np.float32).astype(np.float64)
    P = R.f64(m.state_dict())
    temb = m.temb.cpu().double()
    z0 = gddpm.noise_reference(n, I, 4, S, gddpm.TAG_S)
    assert (np.abs(traj[0].cpu().double().numpy() - z0) / np.maximum(1, np.abs(z0))).max() <= R.NORMAL_TOL
    for s in range(S):                                          # teacher-forced: the device's x_t into the fp64 step
        xt = traj[s].cpu().double()
        e = R.forward(P, torch.cat([xt, temb[int(tau[s])].expand(n, E)], 1)).numpy()
        z = gddpm.noise_reference(n, I, 4, s, gddpm.TAG_S) if coef64[s, 4] != 0 else 0.0
        ref = R.reverse_step(xt.numpy(), e, z, c32[s], clip)
        err = np.abs(traj[s + 1].cpu().double().numpy() - ref) / np.maximum(1.0, np.abs(ref).max(1, keepdims=True))
        assert err.max() <= R.STEP_TOL, (s, err.max())
    # graph replay == launch by launch, the cached graph == the first capture, another seed differs (unless eta = 0)
    a = tr.sample(n, seed=4, steps=S, eta=eta, clip=clip)
    assert torch.equal(a, out) and torch.equal(tr.sample(n, seed=4, steps=S, eta=eta, clip=clip), out)
    tr.use_graph = False
    try:
        o2, t2 = tr.sample(n, seed=4, steps=S, eta=eta, clip=clip, return_trajectory=True)
    finally:
        tr.use_graph = True
    assert torch.equal(o2, out) and torch.equal(t2, traj)
    assert torch.equal(tr.sample(n, seed=5, steps=S, eta=eta, clip=clip), out) == (False)


def test_sampler_all_steps_is_the_ancestral_sampler(trained_small):
    cfg, tr, m = trained_small
    I, E, T, n = cfg["I"], cfg["E"], cfg["T"], 9
    out, traj = tr.sample(n, seed=1, steps=None, eta=1.0, clip=False, return_trajectory=True)
    assert tuple(traj.shape) == (T + 1, n, I)                   # 50 steps: two graphs of 25
    P, temb, tab = R.f64(m.state_dict()), m.temb.cpu().double(), gddpm.tables(T, E)
    for s in (0, 17, T - 2):                                    # x_{t-1} = mean(x_t, x0_hat) + sqrt(beta~_t) z, eq. 6 / 7
        t = T - 1 - s
        xt = traj[s].cpu().double()
        e = R.forward(P, torch.cat([xt, temb[t].expand(n, E)], 1)).numpy()
        x0 = (xt.numpy() - tab["s1"][t] * e) / tab["sa"][t]
        c0, ct, var = R.posterior(T, t)
        ref = c0 * x0 + ct * xt.numpy() + np.sqrt(var) * gddpm.noise_reference(n, I, 1, s, gddpm.TAG_S)
        err = np.abs(traj[s + 1].cpu().double().numpy() - ref) / np.maximum(1.0, np.abs(ref).max(1, keepdims=True))
        assert err.max() <= R.STEP_TOL, (s, err.max())
    xt = traj[T - 1].cpu().double()                             # the last step returns x0_hat
    e = R.forward(P, torch.cat([xt, temb[0].expand(n, E)], 1)).numpy()
    ref = (xt.numpy() - tab["s1"][0] * e) / tab["sa"][0]
    assert (np.abs(traj[T].cpu().double().numpy() - ref) / np.maximum(1.0, np.abs(ref).max(1, keepdims=True))).max() \
        <= R.STEP_TOL
    assert torch.equal(tr.sample(n, seed=1, clip=False), out)


def test_parzen_denoise_and_the_general_sampler(trained_small):
    cfg, tr, m = trained_small
    st = torch.get_rng_state()
    res = tr.parzen(n_samples=64, n_val=32)
    assert np.isfinite([res.sigma, res.ll_mean, res.ll_stderr]).all() and np.isfinite(res.val_means).all()
    clean = tr.test_iter.dataset.tensors[0].reshape(48, -1)
    noisy, x0 = tr.denoise(clean, 10)
    assert torch.equal(st, torch.get_rng_state())
    assert tuple(noisy.shape) == tuple(x0.shape) == (48, cfg["I"]) and 0.0 <= x0.min().item() <= x0.max().item() <= 1.0
    # an edited model samples launch by launch through its own forward: the same steps, within one step's bound each

    class MyDen(ddpm.Denoiser):
        pass
    m2 = ddpm.DDPM(cfg["I"], cfg["H"], cfg["E"], cfg["T"])
    m2.denoiser = MyDen(cfg["I"], cfg["H"], cfg["E"])
    m2.load_state_dict(m.state_dict())
    t2 = ddpm.DDPMTrainer(m2, tr.train_iter, tr.val_iter, tr.test_iter)
    torch.set_rng_state(st)
    assert not gddpm.ddpm_fused_ok(m2)
    a, b = t2.sample(7, seed=2, steps=5, eta=0.0), tr.sample(7, seed=2, steps=5, eta=0.0)
    assert (a - b).abs().max().item() <= 5 * 10 * R.STEP_TOL
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        tr.viz_dir = d
        try:
            imgs = tr.generate_images(3, num_outputs=4)
        finally:
            tr.viz_dir = None
        assert imgs.shape == (4, 8, 8) and os.path.isfile(os.path.join(d, "DDPM", "sample_3.png"))


def test_learning_on_bands():
    """The 16 band patterns of test_denoising (16 x 16 images, two adjacent rows or columns lit): the validation loss
    after a few epochs is below the first epoch's and below 1.0, the expected loss of the zero predictor (E eps^2 = 1)."""
    g = torch.Generator().manual_seed(0)

    def bands(n):
        x = torch.zeros(n, 1, 16, 16)
        k = torch.randint(0, 16, (n,), generator=g)
        for i in range(n):
            j = 2 * (int(k[i]) % 8)
            if k[i] < 8:
                x[i, 0, j:j + 2, :] = 1.0
            else:
                x[i, 0, :, j:j + 2] = 1.0
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64)),
                                           batch_size=64, shuffle=True)
    its = bands(2048), bands(256), bands(256)
    torch.manual_seed(5)
    m = ddpm.DDPM(256, 128, 16, 100)
    tr = ddpm.DDPMTrainer(m, *its, seed=2)
    vals = []
    for _ in range(6):
        with contextlib.redirect_stdout(io.StringIO()):
            tr.train(1, lr=2e-3)
        vals.append(tr.best_val_loss)
    m.eval()
    last = tr.evaluate(its[1])
    print("validation loss by epoch (best so far)", vals, "last", last)
    assert last < vals[0] and last < 1.0, (vals, last)
