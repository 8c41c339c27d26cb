"""The masked autoregressive model on the MI355X: the loss and mask kernels against fp64 and bit patterns, normalisation
and the autoregressive property on the device, the fused engine against an fp64 CPU loop that replays MADETrainer's RNG
protocol, gradients against fp64 autograd, determinism, resume and the general path, the one-launch sampler against the
numpy uniform rule and the fp64 conditionals, completion, and learning itself.  tests/made_reference.py is the reference
of every comparison; the code under test never is."""
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
sys.path.insert(0, HERE)

import made  # noqa: E402
import made_reference as R  # noqa: E402
from generative_models_amd import ops, trainers  # noqa: E402
from generative_models_amd import made as gmade  # noqa: E402
from generative_models_amd import ops_fused as of_  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"


# ---- gm_made_bce -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,I", [(5, 49), (37, 64), (64, 784)])
def test_bce_kernel_against_fp64(b, I):
    g = torch.Generator().manual_seed(I)
    a = (torch.rand(b, I, generator=g) * 2 - 1) * 30.0           # logits up to +-30: both softplus branches
    a[0, :4] = torch.tensor([30.0, -30.0, 0.0, -0.0])
    x = torch.bernoulli(torch.full((b, I), 0.4), generator=g)
    scale = float(np.float32(1.0 / b))
    part, dA, res = torch.zeros(b + 1, device=DEV), torch.full((b + 1, I), -7.0, device=DEV), torch.zeros(1, device=DEV)
    runs = []
    for _ in range(2):
        of_.made_bce(a.to(DEV), x.to(DEV), part, b, scale, dA=dA)
        of_.sum_finalize(part, b, res, scale=scale)
        runs.append((dA.clone(), part.clone(), res.clone()))
    assert all(torch.equal(u, v) for u, v in zip(*runs))         # run to run: the same bits
    ref_dA = (torch.sigmoid(a.double()) - x.double()) * scale
    err = (dA[:b].cpu().double() - ref_dA).abs().max().item()
    print("dA err / scale", err / ref_dA.abs().max().item())
    assert err <= R.GRAD_TOL * ref_dA.abs().max().item()
    assert torch.all(dA[b:] == -7.0) and part[b].item() == 0.0
    rows = R.nll_rows(a.double(), x.double())
    rel = ((part[:b].cpu().double() - rows).abs() / rows.clamp(min=1.0)).max().item()
    ref = rows.sum().item() * scale
    print("row err", rel, "loss", res.item(), ref)
    assert rel <= R.LOSS_TOL
    assert abs(res.item() - ref) <= R.LOSS_TOL * max(1.0, abs(ref))
    part2 = torch.zeros(b, device=DEV)
    of_.made_bce(a.to(DEV), x.to(DEV), part2, b, scale)          # validation: no dA
    assert torch.equal(part2, part[:b])
    # strided rows (no 16-byte path) give the same bits as contiguous ones of the element path's order
    big_a, big_x = torch.zeros(b, I + 3, device=DEV), torch.zeros(b, I + 5, device=DEV)
    big_a[:, 1:1 + I], big_x[:, 2:2 + I] = a.to(DEV), x.to(DEV)
    part3, dA3 = torch.zeros(b, device=DEV), torch.full((b, I + 1), -7.0, device=DEV)
    of_.made_bce(big_a[:, 1:1 + I], big_x[:, 2:2 + I], part3, b, scale, dA=dA3[:, :I])
    assert torch.equal(dA3[:, :I], dA[:b]) and torch.all(dA3[:, I] == -7.0)
    assert ((part3.cpu().double() - rows).abs() / rows.clamp(min=1.0)).max().item() <= R.LOSS_TOL


# ---- gm_made_mask ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["natural", "random"])
@pytest.mark.parametrize("I,H", [(49, 32), (64, 70), (784, 400)])
def test_mask_kernel_zeroes_masked_entries_only(I, H, order):
    m_in, m_h = R.degrees(I, H, order, 9)
    M1, M2 = (m.bool() for m in R.masks(m_in, m_h))
    g = torch.Generator().manual_seed(I + H)
    mk = lambda *s: (torch.rand(*s, generator=g) + 0.5) * (torch.randint(0, 2, s, generator=g) * 2 - 1).float()
    host = [mk(H, I), mk(H * I), mk(H * I), mk(I, H), mk(I * H), mk(I * H)]
    dev = [t.to(DEV) for t in host]
    di, dh = torch.from_numpy(m_in.astype(np.int32)).to(DEV), torch.from_numpy(m_h.astype(np.int32)).to(DEV)
    of_.made_mask(dev[0], dev[3], di, dh, moments1=(dev[1], dev[2]), moments2=(dev[4], dev[5]))
    torch.cuda.synchronize()
    for t, h, M in zip(dev, host, (M1, M1.reshape(-1), M1.reshape(-1), M2, M2.reshape(-1), M2.reshape(-1))):
        t = t.cpu()
        assert torch.all(t[~M] == 0.0) and not torch.any(torch.signbit(t[~M]))     # exactly +0.0
        assert torch.equal(t[M].view(torch.int32), h[M].view(torch.int32))         # every other entry: bit-unchanged
    # without moments: the weights alone
    w1, w2 = host[0].to(DEV), host[3].to(DEV)
    of_.made_mask(w1, w2, di, dh)
    assert torch.equal(w1, dev[0]) and torch.equal(w2, dev[3])


def test_uniform_kernel_is_the_numpy_rule():
    for n, I, seed, row0 in [(5, 49, 0, 0), (37, 784, (1 << 64) - 1, 3), (300, 10, 0x123456789ABCDEF, 1 << 20)]:
        u = of_.made_uniform(n, I, seed, row0=row0, device=DEV).cpu().numpy()
        assert u.tobytes() == R.uniforms(n, I, seed, row0).tobytes()


# ---- loaders, models, runs ---------------------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, shape, seed=7, binary=True):
    """Image loaders; the data come from a private generator, the loaders shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)
    I = shape[0] * shape[1]

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g) if binary else torch.rand(n, I, generator=g)
        ds = torch.utils.data.TensorDataset(x.view(n, 1, *shape), torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


SMALL = dict(I=49, H=32, shape=(7, 7), batch=16, n_train=11 * 16 + 7, n_val=40, n_test=24, order="natural")
SMALL_FP32 = dict(SMALL, binary=False)
SMALL_RANDOM = dict(SMALL, order="random")
FULL = dict(I=784, H=400, shape=(28, 28), batch=512, n_train=11 * 512 + 336, n_val=512 + 100, n_test=64, order="natural")
FULL_FP32 = dict(FULL, binary=False)


def mk_loaders(cfg):
    return loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["shape"], binary=cfg.get("binary", True))


def mk_model(cfg):
    torch.manual_seed(1234)
    return made.MADE(cfg["I"], cfg["H"], cfg["order"], 3)


def product(cfg, its, epochs, use_graph=True, trainer_cls=None, model=None, **kw):
    m = mk_model(cfg) if model is None else model
    tr = (trainer_cls or made.MADETrainer)(m, *its)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs, **kw)
    torch.cuda.synchronize()
    return tr, m


def device_rows(cfg):
    """The oracle's source of rows: the device's gather of a batch (packed or fp32 resident), checked to be the batch."""
    def rows(x):
        data = ops.PackedData(x.to(DEV)) if cfg.get("binary", True) else x.to(DEV).contiguous()
        out = torch.full((x.shape[0], x.shape[1]), -1.0, device=DEV)
        ops.gather_rows(data, torch.arange(x.shape[0], device=DEV), out)
        assert torch.equal(out.cpu(), x.float())
        return out.cpu().double()
    return rows


def lclose(got, ref, tol=R.LOSS_TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print("loss err", err.max())
    assert err.max() <= tol, (err.max(), got[:4], ref[:4])


def masked_zero(m):
    M1, M2 = R.masks(m.m_in.cpu().numpy(), m.m_h.cpu().numpy())
    return bool(torch.all(m.linear.weight.detach().cpu()[M1 == 0] == 0.0)
                and torch.all(m.out.weight.detach().cpu()[M2 == 0] == 0.0))


def parity(cfg, trainer_cls=None):
    """12 batches (the last one ragged) of one epoch against the fp64 oracle: per-batch losses, the validation loss, the
    weights, the RNG protocol."""
    init = mk_model(cfg)
    M = R.masks(init.m_in.numpy(), init.m_h.numpy())
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    assert len(its[0]) == 12
    losses, best, P, state = R.oracle_train(init.state_dict(), M, its, 1, device_rows(cfg))
    o_rng = torch.get_rng_state()
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 1, trainer_cls=trainer_cls, model=init)
    print("losses", tr.losses[:3], losses[:3], "best", tr.best_val_loss, best)
    lclose(tr.losses, losses)
    assert abs(tr.best_val_loss - best) <= R.LOSS_TOL * max(1, abs(best))
    assert torch.equal(torch.get_rng_state(), o_rng)           # the loaders' shuffles and nothing else
    assert tr.num_epochs == 1 and len(tr.losses) == 12
    worst = {k: (m.state_dict()[k].cpu().double() - P[k]).abs().max().item() for k in R.NAMES}
    print("max |w - oracle|", worst)
    assert max(worst.values()) <= R.PARAM_TOL, worst
    assert masked_zero(m)
    return tr, state


# ---- normalisation and the autoregressive property on the device -------------------------------------------------------
@pytest.mark.parametrize("order", ["natural", "random"])
def test_normalisation_on_the_device(order):
    """I = 10, H = 7: after 20 training batches on the fused engine, exp(log_likelihood) over all 1024 images sums to 1
    within 1e-5 -- which fails if any mask is wrong on the fused path."""
    cfg = dict(I=10, H=7, shape=(2, 5), batch=16, n_train=20 * 16, n_val=32, n_test=16, order=order)
    torch.manual_seed(5)
    tr, m = product(cfg, mk_loaders(cfg), 1, lr=1e-2)
    assert type(tr._engine).__name__ == "MADEEngine" and len(tr.losses) == 20 and masked_zero(m)
    x = torch.tensor([[(v >> i) & 1 for i in range(10)] for v in range(1024)], dtype=torch.float32)
    ll = tr.log_likelihood_rows(x)
    total = torch.exp(ll).sum().item()
    print("sum of p(x) over all images", total)
    assert abs(total - 1.0) <= 1e-5
    ref = -R.nll_rows(R.logits(R.f64(m.state_dict()), x.double()), x.double())
    assert ((ll - ref).abs() / ref.abs().clamp(min=1.0)).max().item() <= R.LOSS_TOL
    res = tr.log_likelihood(x)
    assert res.n == 1024 and abs(res.ll_mean - ref.mean().item()) <= R.LOSS_TOL * abs(ref.mean().item())
    assert abs(res.ll_stderr - ref.std(unbiased=False).item() / 32.0) <= 1e-4
    assert tr.log_likelihood().n == 16                          # the default: the whole test_iter


@pytest.mark.parametrize("cfg", [SMALL_RANDOM, FULL], ids=["49-32-random", "784-400"])
def test_autoregressive_property_on_the_device(cfg):
    """Flipping pixel i leaves bit-identical every logit d with m_in[d] <= m_in[i] (the pixel's own included)."""
    torch.manual_seed(3)
    its = loaders(cfg["batch"], 2 * cfg["batch"], cfg["batch"], 8, cfg["shape"])
    tr, m = product(cfg, its, 1)
    m_in = m.m_in.cpu().numpy()
    x = torch.bernoulli(torch.full((9, cfg["I"]), 0.5), generator=torch.Generator().manual_seed(1)).to(DEV)
    base = tr._logits(x).cpu()
    order = np.argsort(m_in)
    for i in sorted({int(order[0]), int(order[cfg["I"] // 2]), int(order[-2]), int(order[-1]), 0}):
        y = x.clone()
        y[:, i] = 1.0 - y[:, i]
        got = tr._logits(y).cpu()
        same = torch.from_numpy(m_in <= m_in[i])
        assert torch.equal(got[:, same].view(torch.int32), base[:, same].view(torch.int32)), i
        later = torch.from_numpy(m_in > m_in[i])
        if later.any() and m_in[i] <= m.m_h.max().item():
            assert not torch.equal(got[:, later], base[:, later]), i      # and the later ones do see it


# ---- the engine against the fp64 oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [SMALL, SMALL_FP32, SMALL_RANDOM, FULL, FULL_FP32],
                         ids=["49-32-b16-bits", "49-32-b16-fp32", "49-32-b16-random", "784-400-b512-bits",
                              "784-400-b512-fp32"])
def test_engine_vs_fp64_oracle(cfg):
    tr, _ = parity(cfg)
    assert type(tr._engine).__name__ == "MADEEngine"
    assert type(tr._device_data(tr.train_iter)).__name__ == ("PackedData" if cfg.get("binary", True) else "Tensor")


@pytest.mark.parametrize("cfg", [SMALL, SMALL_FP32, FULL], ids=["49-32-b16", "49-32-b16-fp32", "784-400-b512"])
def test_teacher_forced_batch_gradients_vs_fp64(cfg):
    """One training batch through MADEEngine from known weights: the gradients it leaves in the flat gradient buffer
    against fp64 autograd through weight * mask on that batch, within 1.5e-6 of each tensor's scale.  The weight-gradient
    GEMMs compute the masked entries too (gm_made_mask discards their effect), so the weights' gradients are compared
    under the mask."""
    b = cfg["batch"]
    its = loaders(b, b, b, 16, cfg["shape"], binary=cfg.get("binary", True))
    m = mk_model(cfg)
    init = R.f64(m.state_dict())
    M = R.masks(m.m_in.numpy(), m.m_h.numpy())
    tr = made.MADETrainer(m, *its)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    torch.cuda.synchronize()
    fp = tr._engine.fp
    got = {k: fp.gviews[[i for i, q in enumerate(fp.params) if q is p][0]].cpu().double()
           for k, p in m.named_parameters()}
    assert len(got) == 4
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].reshape(b, -1)
    loss, grads, _ = R.loss_and_grads(init, x, M)
    assert abs(tr.losses[0] - loss) <= R.LOSS_TOL * max(1.0, abs(loss))
    got["linear.weight"], got["out.weight"] = got["linear.weight"] * M[0], got["out.weight"] * M[1]
    for k, gk in got.items():
        scale = grads[k].abs().max().item()
        assert scale > 0, k
        err = (gk - grads[k]).abs().max().item()
        print(k, "grad err / scale", err / scale)
        assert err <= R.GRAD_TOL * scale, (k, err, scale)


def snapshot(tr, m):
    eng = tr._engine
    return (list(tr.losses), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state(), eng.fp.m.cpu().clone(), eng.fp.v.cpu().clone())


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_bitwise_reproducibility_and_resume(tmp_path):
    cfg = SMALL_RANDOM
    runs = []
    for use_graph in (True, True, False):                   # graph twice, then eager
        torch.manual_seed(99)
        runs.append(snapshot(*product(cfg, mk_loaders(cfg), 2, use_graph=use_graph)))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    # train(1) + save + load into a fresh trainer + train(1) == train(2): Adam's steps and the shuffles continue
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 1)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    m2 = made.MADE(cfg["I"], cfg["H"], "random", 3).to(DEV)
    tr2 = made.MADETrainer(m2, *its)
    tr2.load_checkpoint(path)
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    same(snapshot(tr2, m2), runs[0])
    # a checkpoint of another order is refused under strict=True, taken under strict=False (its degrees come along)
    for kw in (dict(order="natural"), dict(order="random", order_seed=4)):
        t3 = made.MADETrainer(made.MADE(cfg["I"], cfg["H"], **kw).to(DEV), *its)
        t3.load_checkpoint(path)
        with pytest.raises(GMError):
            t3.train(1)
    t3 = made.MADETrainer(made.MADE(cfg["I"], cfg["H"]).to(DEV), *its)
    t3.load_checkpoint(path, strict=False)
    with contextlib.redirect_stdout(io.StringIO()):
        t3.train(1)
    assert torch.equal(t3.model.m_in.cpu(), m.m_in.cpu()) and masked_zero(t3.model)


def test_a_refused_resume_leaves_the_engine_as_it_was(tmp_path):
    """A trainer that has trained loads a checkpoint written under another order: train() refuses it ("different
    settings") before anything is touched -- the engine's parameters and both Adam moments are bit for bit what they
    were before the call."""
    cfg = dict(SMALL, n_train=2 * 16, n_val=16)             # two training batches
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, _ = product(cfg, its, 1)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    t2, _ = product(dict(cfg, order="random"), its, 1)
    t2.load_checkpoint(path)
    fp = t2._engine.fp
    torch.cuda.synchronize()
    before = [t.cpu().clone() for t in (fp.flat, fp.m, fp.v)]
    assert float(before[1].abs().sum()) > 0 and float(before[2].sum()) > 0
    with pytest.raises(GMError, match="different settings"):
        t2.train(1)
    torch.cuda.synchronize()
    for b, t in zip(before, (fp.flat, fp.m, fp.v)):
        assert torch.equal(b, t.cpu())


def test_general_path_agrees_with_the_fused_run():
    class Mine(made.MADETrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    cfg = SMALL_RANDOM
    tg, _ = parity(cfg, trainer_cls=Mine)                      # against the oracle
    assert tg._engine is None and masked_zero(tg.model)
    tf, state = parity(cfg)                                    # the fused run: same data, same shuffles
    worst = {k: (tg.model.state_dict()[k].cpu() - tf.model.state_dict()[k].cpu()).abs().max().item() for k in R.NAMES}
    print("general vs fused weights", worst)
    assert max(worst.values()) <= R.PARAM_TOL
    fp, opt = tf._engine.fp, tg._general_opt
    assert fp.m.numel() == opt.m.numel()                       # the same flat layout
    dm, dv = (fp.m - opt.m).abs().max().item(), (fp.v - opt.v).abs().max().item()
    print("general vs fused moments", dm, dv)
    assert dm <= R.PARAM_TOL and dv <= R.PARAM_TOL
    # both against the oracle's Adam state, and exactly zero at the masked entries on both paths
    M = R.masks(tf.model.m_in.cpu().numpy(), tf.model.m_h.cpu().numpy())
    for lin, name, Mk in ((tf._engine.L1, "linear.weight", M[0]), (tf._engine.L2, "out.weight", M[1])):
        mW, vW = lin.mW.cpu().view(Mk.shape), lin.vW.cpu().view(Mk.shape)
        assert torch.all(mW[Mk == 0] == 0.0) and torch.all(vW[Mk == 0] == 0.0)
        assert (mW.double() - state[name]["exp_avg"]).abs().max().item() <= R.PARAM_TOL
        assert (vW.double() - state[name]["exp_avg_sq"]).abs().max().item() <= R.PARAM_TOL
    o = 0
    for p, Mk in zip(tg.model.parameters(), (M[0], None, M[1], None)):
        if Mk is not None:
            mW = opt.m[o:o + p.numel()].cpu().view(Mk.shape)
            assert torch.all(mW[Mk == 0] == 0.0)
        o += (p.numel() + 3) // 4 * 4


# ---- the sampler -----------------------------------------------------------------------------------------------------------
class EditedMADE(made.MADE):
    """The same network as a user subclass: trained and sampled on the general path."""


def _case(name, cls=None):
    n, I, H, order, seed = R.SAMPLER_CASES[name]
    sd, P, m_in = R.case_weights(I, H, order)
    m = (cls or made.MADE)(I, H, order, R.ORDER_SEED)
    m.load_state_dict(sd)
    its = loaders(8, 16, 8, 8, (1, I))
    return n, I, seed, P, m_in, made.MADETrainer(m, *its)


@pytest.mark.parametrize("name", list(R.SAMPLER_CASES))
def test_sampler_against_the_rule_and_the_fp64_conditionals(name):
    n, I, seed, P, m_in, tr = _case(name)
    m = tr.model
    before = {k: v.clone() for k, v in m.state_dict().items()}
    st, mode = torch.get_rng_state(), m.training
    x, p = tr.sample(n, seed=seed, return_probs=True)
    assert torch.equal(st, torch.get_rng_state()) and m.training == mode
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert tuple(x.shape) == tuple(p.shape) == (n, I) and x.dtype == torch.float32
    u = R.uniforms(n, I, seed)
    und = R.check_sample(x.cpu(), p.cpu(), P, u, m_in)             # (a), (b), (c) and the cap
    print(name, "undecided", int(und.sum()), "lit", x.mean().item())
    x2, p2 = tr.sample(n, seed=seed, return_probs=True)            # two calls: the same bits
    assert torch.equal(x2, x) and torch.equal(p2, p) and torch.equal(tr.sample(n, seed=seed), x)
    assert not torch.equal(tr.sample(n, seed=seed + 1), x)
    # rows do not depend on n or on the workgroup a row lands in
    for k in sorted({1, 5, min(n, 7)}):
        xs, ps = tr.sample(k, seed=seed, return_probs=True)
        assert torch.equal(xs, x[:k]) and torch.equal(ps, p[:k]), k
    # the general sampler (I forward passes of an edited model): (a)-(c) on its own x, and the fused bits on every row
    # without an undecided pixel
    _, _, _, _, _, tg = _case(name, EditedMADE)
    assert not gmade.made_fused_ok(tg.model)
    xg, pg = tg.sample(n, seed=seed, return_probs=True)
    und_g = R.check_sample(xg.cpu(), pg.cpu(), P, u, m_in)
    rows = ~(und.any(1) | und_g.any(1))
    assert rows.sum() >= 0.9 * n
    assert torch.equal(xg.cpu()[rows], x.cpu()[rows])


def test_rows_are_independent_of_n():
    """Rows 0-4 of the n = 300 call equal the n = 5 call under the same weights."""
    n, I, seed, P, m_in, tr = _case("300x49x32-random")
    big, small = tr.sample(300, seed=seed, return_probs=True), tr.sample(5, seed=seed, return_probs=True)
    assert torch.equal(big[0][:5], small[0]) and torch.equal(big[1][:5], small[1])


@pytest.mark.parametrize("name", ["300x49x32-random", "64x784x400"])
def test_completion(name):
    n, I, seed, P, m_in, tr = _case(name)
    g = torch.Generator().manual_seed(2)
    given = torch.bernoulli(torch.full((n, I), 0.5), generator=g)
    x = tr.sample(n, seed=seed)
    assert torch.equal(tr.complete(given, 0, seed=seed), x)         # n_known = 0: the sampler
    assert torch.equal(tr.complete(given, I, seed=seed).cpu(), given)   # n_known = I: the input
    order = np.argsort(m_in)
    u = R.uniforms(n, I, seed)
    for j in (1, I // 2, I - 1):
        y, p = tr.complete(given.view(n, 1, 1, I), j, seed=seed, return_probs=True)
        assert torch.equal(y.cpu()[:, order[:j]], given[:, order[:j]])      # the known pixels are kept
        R.check_sample(y.cpu(), p.cpu(), P, u, m_in, n_known=j)                # the rest: (a), (b), (c)
        assert torch.equal(tr.complete(given, j, seed=seed), y)
    # the general path completes by the same rule
    _, _, _, _, _, tg = _case(name, EditedMADE)
    j = I // 2
    yg, pg = tg.complete(given, j, seed=seed, return_probs=True)
    assert torch.equal(yg.cpu()[:, order[:j]], given[:, order[:j]])
    R.check_sample(yg.cpu(), pg.cpu(), P, u, m_in, n_known=j)


def test_parzen_and_images(tmp_path):
    n, I, seed, P, m_in, tr = _case("64x64x70")
    tr.model.shape = 8
    st = torch.get_rng_state()
    res = tr.parzen(n_samples=64, n_val=8)
    assert np.isfinite([res.sigma, res.ll_mean, res.ll_stderr]).all() and np.isfinite(res.val_means).all()
    assert torch.equal(st, torch.get_rng_state())
    tr.viz_dir = str(tmp_path)
    imgs = tr.generate_images(3, num_outputs=4)
    assert imgs.shape == (4, 8, 8) and os.path.isfile(os.path.join(str(tmp_path), "MADE", "sample_3.png"))


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_learning_on_bands():
    """The 16 band patterns tests/test_gpu_ddpm.py learns on (16 x 16 images, two adjacent rows or columns lit), each 128
    times in the training set, so the empirical distribution is uniform over 16 images and its entropy is log 16 exactly.
    On the training set the NLL falls below that of the independent-Bernoulli model fitted in closed form, and after no
    epoch is it below log 16 - 1e-3: a normalised model cannot beat the entropy of the data."""
    def bands(reps):
        x = torch.zeros(16 * reps, 1, 16, 16)
        for i in range(16 * reps):
            k = i % 16
            j = 2 * (k % 8)
            if k < 8:
                x[i, 0, j:j + 2, :] = 1.0
            else:
                x[i, 0, :, j:j + 2] = 1.0
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(16 * reps, dtype=torch.int64)),
                                           batch_size=64, shuffle=True)
    its = bands(128), bands(16), bands(16)
    x = its[0].dataset.tensors[0].reshape(2048, -1)
    q = x.double().mean(0)
    ent = -(torch.xlogy(q, q) + torch.xlogy(1 - q, 1 - q))
    indep = ent.sum().item()                                    # the fitted independent model's NLL on its own data
    torch.manual_seed(5)
    m = made.MADE(256, 128)
    tr = made.MADETrainer(m, *its)
    nll = []
    for _ in range(6):
        with contextlib.redirect_stdout(io.StringIO()):
            tr.train(1, lr=2e-3)
        nll.append(-tr.log_likelihood(x).ll_mean)
    print("training-set NLL by epoch", nll, "independent", indep, "log 16", math.log(16))
    assert nll[-1] < indep and nll[-1] < nll[0]
    assert min(nll) >= math.log(16) - 1e-3
