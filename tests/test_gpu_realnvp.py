"""The RealNVP coupling flow on the MI355X: every kernel of csrc/gm_nvp.hip against fp64 on the device's own noise (both
paths of each, saturated tanh, s_cap = 8, canary rows), the fused engine against an fp64 CPU loop that replays
RealNVPTrainer's protocol, one batch's gradients against fp64 autograd, determinism, resume, the general path, the exact
encode / decode round trip, sampling and the likelihood, and learning itself.  tests/realnvp_reference.py is the reference
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

import real_nvp  # noqa: E402
import realnvp_reference as R  # noqa: E402
from generative_models_amd import ops, trainers  # noqa: E402
from generative_models_amd import ops_fused as of_  # noqa: E402
from generative_models_amd import realnvp as gnvp  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
CANARY = -7.0
DS = [7, 10, 16, 784]            # halves 4 / 3 (element path, odd split), 5 / 5 (unaligned rows), 8 / 8 (vector path), 392
BS = [1, 5, 16]


def rel(got, ref):
    """max |got - ref| relative to the reference tensor's scale."""
    ref = torch.as_tensor(ref).double()
    return (got.detach().cpu().double() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)


def canary(rows, width):
    return torch.full((rows, width), CANARY, device=DEV)


def grey(b, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.floor(torch.rand(b, D, generator=g) * 256.0) / 255.0
    x[0, :2] = torch.tensor([0.0, 1.0])
    return x.clamp(0.0, 1.0)


# ---- gm_nvp_pre ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["checker", "half"])
@pytest.mark.parametrize("D", DS)
def test_pre_kernel_against_fp64(D, mask):
    Da, Db = (D + 1) // 2, D // 2
    for b in BS:
        for alpha, levels, tag, step, row0 in ((0.05, 256, gnvp.TAG_TRAIN, 3, 0), (0.0, 16, gnvp.TAG_EVAL, 0, 1 << 20)):
            seed = (9 << 32) | (D + b)
            x = grey(b, D, D + b) if levels == 256 else torch.floor(grey(b, D, D) * 15.0 + 0.5) / 15.0
            u = of_.nvp_uniforms(b, D, seed, tag, step=step, row0=row0, device=DEV)
            assert u.cpu().numpy().tobytes() == gnvp.uniforms_reference(b, D, seed, step, tag, row0).tobytes()
            ya, yb, ld = canary(b + 1, Da), canary(b + 1, Db), torch.full((b + 1,), CANARY, device=DEV)
            of_.nvp_pre(x.to(DEV), ya, yb, ld, b, seed, tag, alpha, levels, mask, step=step, row0=row0)
            ry, rld = R.pre(x, u.cpu(), alpha, levels)
            ra, rb = R.split(ry, mask)
            errs = rel(ya[:b], ra), rel(yb[:b], rb), rel(ld[:b], rld)
            print(D, mask, b, alpha, "pre err / scale", errs)
            assert max(errs) <= R.LOSS_TOL
            assert torch.isfinite(ya[:b]).all() and torch.isfinite(yb[:b]).all()
            assert torch.all(ya[b] == CANARY) and torch.all(yb[b] == CANARY) and ld[b].item() == CANARY
            # the step from a device counter plus a device base, and rows that are no multiple of 16 bytes: same bits
            ctr = torch.tensor([step - 1], dtype=torch.int64, device=DEV)
            base = torch.tensor([1], dtype=torch.int64, device=DEV)
            bx, ba, bb = canary(b, D + 3), canary(b, Da + 1), canary(b, Db + 3)
            bx[:, 1:1 + D] = x.to(DEV)
            ld2 = torch.zeros(b, device=DEV)
            of_.nvp_pre(bx[:, 1:1 + D], ba[:, 1:], bb[:, 1:1 + Db], ld2, b, seed, tag, alpha, levels, mask, step=0,
                        step_ctr=ctr, step_base=base, row0=row0)
            assert torch.equal(ba[:, 1:], ya[:b]) and torch.equal(bb[:, 1:1 + Db], yb[:b]) and torch.equal(ld2, ld[:b])
            assert torch.all(ba[:, 0] == CANARY) and torch.all(bb[:, 0] == CANARY) and torch.all(bb[:, 1 + Db:] == CANARY)


# ---- gm_nvp_couple ---------------------------------------------------------------------------------------------------------
def couple_inputs(b, Dt, seed):
    """ST with st_s up to +-30 (tanh saturated at both ends) and t up to +-30, x_t of logit scale."""
    g = torch.Generator().manual_seed(seed)
    st = (torch.rand(b, 2 * Dt, generator=g) * 2 - 1) * 30.0
    st[:, :Dt] *= (torch.rand(b, Dt, generator=g) < 0.5).float() * 0.97 + 0.03       # half of them inside +-0.9
    st[0, 0] = 30.0
    st[0, Dt - 1] = -30.0
    x = torch.randn(b, Dt, generator=g) * 3.0
    return st, x


@pytest.mark.parametrize("Dt", [3, 4, 5, 8, 392])
def test_couple_kernel_forward_inverse_and_round_trip(Dt):
    cap = 8.0
    for b in BS:
        st, x = couple_inputs(b, Dt, Dt + b)
        ld0 = torch.randn(b, generator=torch.Generator().manual_seed(b))
        y, ld = canary(b + 1, Dt), torch.full((b + 1,), CANARY, device=DEV)
        ld[:b] = ld0.to(DEV)
        of_.nvp_couple(st.to(DEV), x.to(DEV), y, b, Dt, cap, logdet=ld)
        ry, rs = R.couple(st.double(), x.double(), cap)
        errs = rel(y[:b], ry), rel(ld[:b], ld0.double() + rs)
        print(Dt, b, "couple err / scale", errs)
        assert max(errs) <= R.LOSS_TOL
        assert torch.all(y[b] == CANARY) and ld[b].item() == CANARY
        # the inverse against fp64 on the device's own y, and log-determinant untouched
        xi = canary(b + 1, Dt)
        of_.nvp_couple(st.to(DEV), y[:b], xi, b, Dt, cap, inverse=True)
        ri = R.couple_inv(st.double(), y[:b].cpu().double(), cap)
        print(Dt, b, "inverse err / scale", rel(xi[:b], ri))
        assert rel(xi[:b], ri) <= R.LOSS_TOL and torch.all(xi[b] == CANARY)
        # inverse o forward returns x_t.  Each of y = fl(fl(x e^s) + t) and d = fl(y - t) is one rounding of a value of
        # magnitude <= |y| + |t|, the two exponentials and the products a few ulp each: |x' - x| <= 2^-23 ((|y| + |t|)
        # e^-s + 4 |x|)
        s = cap * torch.tanh(st[:, :Dt].double())
        bound = 2.0 ** -23 * ((ry.abs() + st[:, Dt:].double().abs()) * torch.exp(-s) + 4.0 * x.double().abs())
        gap = (xi[:b].cpu().double() - x.double()).abs()
        print(Dt, b, "round trip, worst gap / bound", (gap / bound).max().item())
        assert torch.all(gap <= bound)
        # unaligned views: the element path gives the vector path's bits
        bst, bx_, by = canary(b, 2 * Dt + 1), canary(b, Dt + 3), canary(b, Dt + 2)
        bst[:, 1:], bx_[:, 2:2 + Dt] = st.to(DEV), x.to(DEV)
        ld2 = ld0.to(DEV).clone()
        of_.nvp_couple(bst[:, 1:], bx_[:, 2:2 + Dt], by[:, 1:1 + Dt], b, Dt, cap, logdet=ld2)
        assert torch.equal(by[:, 1:1 + Dt], y[:b]) and torch.equal(ld2, ld[:b])
        assert torch.all(by[:, 0] == CANARY) and torch.all(by[:, 1 + Dt] == CANARY)


@pytest.mark.parametrize("Dt", [3, 4, 5, 8, 392])
def test_couple_bwd_kernel_one_and_two_addends(Dt):
    cap = 8.0
    for b in BS:
        st, x = couple_inputs(b, Dt, 100 + Dt + b)
        g = torch.Generator().manual_seed(Dt)
        g0, g1 = torch.randn(b, Dt, generator=g), torch.randn(b, Dt, generator=g)
        c = -float(np.float32(1.0 / b))
        for two in (False, True):
            dst, dx = canary(b + 1, 2 * Dt), canary(b + 1, Dt)
            of_.nvp_couple_bwd(st.to(DEV), x.to(DEV), g0.to(DEV), dst, b, Dt, cap, c, g1=g1.to(DEV) if two else None, dx=dx)
            gg = (g0 + g1).double() if two else g0.double()           # the kernel sums the addends in fp32
            rdst, rdx = R.couple_bwd(st.double(), x.double(), gg, c, cap)
            errs = rel(dst[:b, :Dt], rdst[:, :Dt]), rel(dst[:b, Dt:], rdst[:, Dt:]), rel(dx[:b], rdx)
            print(Dt, b, two, "couple_bwd err / scale", errs)
            assert max(errs) <= R.LOSS_TOL
            assert torch.all(dst[b] == CANARY) and torch.all(dx[b] == CANARY)
            dst2 = canary(b, 2 * Dt)
            of_.nvp_couple_bwd(st.to(DEV), x.to(DEV), g0.to(DEV), dst2, b, Dt, cap, c, g1=g1.to(DEV) if two else None)
            assert torch.equal(dst2, dst[:b])                          # without dx: the same dST
        # the closed form is autograd's (on st / 10: no saturated tanh, where fp64's own 1 - tanh^2 cancels)
        stg, xg = (st.double() / 10).requires_grad_(True), x.double().requires_grad_(True)
        y, s = R.couple(stg, xg, cap)
        ((y * g0.double()).sum() + c * s.sum()).backward()
        rdst, rdx = R.couple_bwd(st.double() / 10, x.double(), g0.double(), c, cap)
        assert rel(rdst, stg.grad) <= 1e-12 and rel(rdx, xg.grad) <= 1e-12


# ---- gm_nvp_loss -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", DS)
def test_loss_kernel_against_fp64(D):
    Da, Db = (D + 1) // 2, D // 2
    for b in BS:
        g = torch.Generator().manual_seed(D * b)
        za, zb, ld = torch.randn(b, Da, generator=g) * 2, torch.randn(b, Db, generator=g) * 2, torch.randn(b, generator=g) * D
        cst, scale = float(np.float32(R.nll_const(D, 256))), float(np.float32(1.0 / b))
        part, dza, dzb = torch.full((b + 1,), CANARY, device=DEV), canary(b + 1, Da), canary(b + 1, Db)
        of_.nvp_loss(za.to(DEV), zb.to(DEV), ld.to(DEV), part, b, cst, scale=scale, dza=dza, dzb=dzb)
        ref = 0.5 * ((za.double() ** 2).sum(1) + (zb.double() ** 2).sum(1)) - ld.double() + R.nll_const(D, 256)
        errs = rel(part[:b], ref), rel(dza[:b], za.double() / b), rel(dzb[:b], zb.double() / b)
        print(D, b, "loss err / scale", errs)
        assert errs[0] <= R.LOSS_TOL and max(errs[1:]) <= R.GRAD_TOL
        assert part[b].item() == CANARY and torch.all(dza[b] == CANARY) and torch.all(dzb[b] == CANARY)
        part2 = torch.zeros(b, device=DEV)
        of_.nvp_loss(za.to(DEV), zb.to(DEV), ld.to(DEV), part2, b, cst)       # validation: no dz
        assert torch.equal(part2, part[:b])


# ---- gm_nvp_post and its PRIOR mode ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["checker", "half"])
@pytest.mark.parametrize("D", DS)
def test_post_and_prior_kernels_against_fp64(D, mask):
    Da, Db = (D + 1) // 2, D // 2
    for b in BS:
        seed, row0 = (3 << 32) | D, 5
        za, zb = canary(b + 1, Da), canary(b + 1, Db)
        of_.nvp_prior(za, zb, b, D, seed, mask, temperature=0.7, row0=row0)
        rz = torch.from_numpy(gnvp.normals_reference(b, D, seed, row0)) * 0.7
        ra, rb = R.split(rz, mask)
        errs = rel(za[:b], ra), rel(zb[:b], rb)
        print(D, mask, b, "prior err / scale", errs)
        assert max(errs) <= R.LOSS_TOL and torch.all(za[b] == CANARY) and torch.all(zb[b] == CANARY)
        # logit-space halves of scale +-12 (both ends clamp at alpha = 0.05) -> the image
        g = torch.Generator().manual_seed(D + b)
        y = (torch.rand(b, D, generator=g) * 2 - 1) * 12.0
        y[0, :2] = torch.tensor([12.0, -12.0])
        ya, yb = (t.contiguous().to(DEV) for t in R.split(y, mask))
        x = canary(b + 1, D)
        of_.nvp_post(ya, yb, x, b, 0.05, mask)
        ref = R.post(y.double(), 0.05)
        err = (x[:b].cpu().double() - ref).abs().max().item()
        print(D, mask, b, "post err", err)
        assert err <= R.LOSS_TOL and x[:b].min().item() == 0.0 and x[:b].max().item() == 1.0
        assert torch.all(x[b] == CANARY)
        bx, ba = canary(b, D + 1), canary(b, Da + 1)
        ba[:, 1:] = ya
        of_.nvp_post(ba[:, 1:], yb, bx[:, 1:], b, 0.05, mask)                  # unaligned rows: the same bits
        assert torch.equal(bx[:, 1:], x[:b]) and torch.all(bx[:, 0] == CANARY)


# ---- loaders, models, runs -------------------------------------------------------------------------------------------------
def loaders(cfg, seed=7):
    """Image loaders; the data come from a private generator, the loaders shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)
    D = cfg["D"]

    def mk(n):
        if cfg.get("binary", False):
            x = torch.bernoulli(torch.full((n, D), 0.3), generator=g)
        else:
            x = torch.floor(torch.rand(n, D, generator=g) * 256.0) / 255.0
        ds = torch.utils.data.TensorDataset(x.view(n, 1, *cfg["shape"]), torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=cfg["batch"], shuffle=True)
    return mk(cfg["n_train"]), mk(cfg["n_val"]), mk(cfg["n_test"])


SMALL = dict(D=12, H=8, K=3, shape=(3, 4), batch=16, n_train=40, n_val=24, n_test=16, mask="checker")
SMALL_BITS = dict(SMALL, binary=True)
SMALL_HALF = dict(SMALL, mask="half", D=14, shape=(2, 7))
FULL = dict(D=784, H=400, K=4, shape=(28, 28), batch=512, n_train=3 * 512 + 200, n_val=512 + 100, n_test=64,
            mask="checker")
FULL_BITS = dict(FULL, binary=True)
SEED = 21
# The weights' bound of the 784-400 case on fp32 data, the one comparison that cannot meet 5e-5 (measured: 5.03e-5; the
# bit-packed case 3.9e-5).  Adam divides by sqrt(v) + 1e-8, so an entry whose gradient is of the size of its own fp32 error
# moves by a share of lr that no gradient bound controls, and among 160 000 weights per layer a few such entries exist.
# The same loop in fp32 torch on the same rows and noise (realnvp_reference.oracle_train with dtype=torch.float32)
# deviates from the fp64 run by 5.3e-5 to 1.9e-2 of a tensor's scale at this shape, depending on the data and on the
# host's summation order; the allowance is 4 x the smallest of those measurements.  Every other
# comparison of weights keeps 5e-5.
FULL_PARAM_TOL = 4 * 5.3e-5


def flow_cfg(cfg, m):
    return dict(K=cfg["K"], s_cap=m.s_cap, mask=m.mask, alpha=m.alpha, levels=m.levels)


def mk_model(cfg, cls=None, fresh=False):
    torch.manual_seed(1234)
    m = (cls or real_nvp.RealNVP)(cfg["D"], cfg["H"], cfg["K"], cfg["mask"])
    if not fresh:                                    # non-zero out layers: every gradient path carries something
        # st of order 1 at H = 8; at H = 400 a flow near the identity, as training meets it (at 0.5 / sqrt(H) the first
        # loss is 1e4 to 6e5 nats and most tanh are saturated)
        scale = 0.5 if cfg["H"] < 64 else 0.05
        m.load_state_dict(R.random_weights(cfg["D"], cfg["H"], cfg["K"], seed=cfg["D"], out_scale=scale))
    return m


def product(cfg, its, epochs, use_graph=True, trainer_cls=None, model=None, **kw):
    m = mk_model(cfg) if model is None else model
    tr = (trainer_cls or real_nvp.RealNVPTrainer)(m, *its, seed=SEED)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs, **kw)
    torch.cuda.synchronize()
    return tr, m


def device_rows(cfg):
    """The oracle's source of rows: the device's gather of a batch (packed or fp32 resident), checked to be the batch."""
    def rows(x):
        data = ops.PackedData(x.to(DEV)) if cfg.get("binary", False) else x.to(DEV).contiguous()
        out = torch.full((x.shape[0], x.shape[1]), -1.0, device=DEV)
        ops.gather_rows(data, torch.arange(x.shape[0], device=DEV), out)
        assert torch.equal(out.cpu(), x.float())
        return out.cpu().double()
    return rows


def device_noise(D, seed=SEED):
    return lambda tag, step, b: of_.nvp_uniforms(b, D, seed, tag, step=step, device=DEV).cpu().double()


def lclose(got, ref, tol=R.LOSS_TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print("loss err", err.max())
    assert err.max() <= tol, (err.max(), got[:4], ref[:4])


def parity(cfg, trainer_cls=None, epochs=1):
    """One epoch (the last batch ragged) against the fp64 oracle: per-batch losses, the validation loss, the weights, the
    RNG protocol."""
    init = mk_model(cfg)
    P0 = R.f64(init.state_dict())
    torch.manual_seed(99)
    its = loaders(cfg)
    nb = len(its[0])
    assert cfg["n_train"] % cfg["batch"] != 0                  # a ragged last batch
    losses, vals, P, state = R.oracle_train(P0, flow_cfg(cfg, init), its, epochs, device_rows(cfg), device_noise(cfg["D"]))
    o_rng = torch.get_rng_state()
    torch.manual_seed(99)
    its = loaders(cfg)
    tr, m = product(cfg, its, epochs, trainer_cls=trainer_cls, model=init)
    print("losses", tr.losses[:3], losses[:3], "best", tr.best_val_loss, min(vals))
    lclose(tr.losses, losses)
    assert abs(tr.best_val_loss - min(vals)) <= R.LOSS_TOL * max(1, abs(min(vals)))
    assert torch.equal(torch.get_rng_state(), o_rng)           # the loaders' shuffles and nothing else
    assert tr.num_epochs == epochs and len(tr.losses) == nb * epochs and tr.noise_steps == nb * epochs
    worst = {k: rel(m.state_dict()[k], P[k]) for k in R.keys(cfg["K"])}
    print("max |w - oracle| / scale", max(worst.values()))
    if cfg["D"] == 784:
        print("per tensor", {k: "%.2e" % v for k, v in worst.items()})
    tol = FULL_PARAM_TOL if cfg["D"] == 784 and not cfg.get("binary", False) else R.PARAM_TOL
    assert max(worst.values()) <= tol, worst
    return tr, state


@pytest.mark.parametrize("cfg", [SMALL, SMALL_BITS, SMALL_HALF, FULL, FULL_BITS],
                         ids=["12-8-K3-b16-fp32", "12-8-K3-b16-bits", "14-8-K3-b16-half", "784-400-K4-b512-fp32",
                              "784-400-K4-b512-bits"])
def test_engine_vs_fp64_oracle(cfg):
    tr, _ = parity(cfg)
    assert type(tr._engine).__name__ == "RealNVPEngine"
    assert type(tr._device_data(tr.train_iter)).__name__ == ("PackedData" if cfg.get("binary", False) else "Tensor")


@pytest.mark.parametrize("cfg", [SMALL, SMALL_HALF, FULL], ids=["12-8-K3-b16", "14-8-K3-b16-half", "784-400-K4-b512"])
def test_one_batch_gradients_vs_fp64(cfg):
    """One training batch through RealNVPEngine from known non-zero weights: the gradients it leaves in the flat gradient
    buffer against fp64 autograd on that batch and the device's own noise, within 1.5e-6 of each tensor's scale."""
    b = cfg["batch"]
    its = loaders(dict(cfg, n_train=b, n_val=b, n_test=16))
    m = mk_model(cfg)
    init = R.f64(m.state_dict())
    tr = real_nvp.RealNVPTrainer(m, *its, seed=SEED)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    torch.cuda.synchronize()
    fp = tr._engine.fp
    got = {k: fp.gviews[[i for i, q in enumerate(fp.params) if q is p][0]].cpu().double() for k, p in m.named_parameters()}
    assert len(got) == 4 * cfg["K"]
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].reshape(b, -1).double()
    loss, grads = R.loss_and_grads(init, x, device_noise(cfg["D"])(R.TAG_TRAIN, 0, b), flow_cfg(cfg, m))
    assert abs(tr.losses[0] - loss) <= R.LOSS_TOL * max(1.0, abs(loss))
    for k, gk in got.items():
        scale = grads[k].abs().max().item()
        assert scale > 0, k
        err = (gk - grads[k]).abs().max().item()
        print(k, "grad err / scale", err / scale)
        assert err <= R.GRAD_TOL * scale, (k, err, scale)


def snapshot(tr, m):
    eng = tr._engine
    return (list(tr.losses), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state(), eng.fp.m.cpu().clone(), eng.fp.v.cpu().clone(), tr.noise_steps)


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[6] == b[6]
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_bitwise_reproducibility_and_resume(tmp_path):
    cfg = SMALL
    runs = []
    for use_graph in (True, True, False):                   # graph twice, then eager
        torch.manual_seed(99)
        runs.append(snapshot(*product(cfg, loaders(cfg), 2, use_graph=use_graph)))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    # train(1) + save + load into a fresh trainer + train(1) == train(2): Adam's steps, the shuffles and the noise stream
    torch.manual_seed(99)
    its = loaders(cfg)
    tr, m = product(cfg, its, 1)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    m2 = real_nvp.RealNVP(cfg["D"], cfg["H"], cfg["K"]).to(DEV)
    tr2 = real_nvp.RealNVPTrainer(m2, *its, seed=SEED)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == len(its[0])
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    same(snapshot(tr2, m2), runs[0])
    # a checkpoint of other settings is refused under strict=True, taken under strict=False
    for model, seed in ((real_nvp.RealNVP(cfg["D"], cfg["H"], cfg["K"], alpha=0.1), SEED),
                        (real_nvp.RealNVP(cfg["D"], cfg["H"], cfg["K"], "half"), SEED),
                        (real_nvp.RealNVP(cfg["D"], cfg["H"], cfg["K"]), SEED + 1)):
        t3 = real_nvp.RealNVPTrainer(model.to(DEV), *its, seed=seed)
        t3.load_checkpoint(path)
        with pytest.raises(GMError, match="different settings"):
            t3.train(1)
    t3 = real_nvp.RealNVPTrainer(real_nvp.RealNVP(cfg["D"], cfg["H"], cfg["K"], s_cap=3.0).to(DEV), *its, seed=SEED)
    t3.load_checkpoint(path, strict=False)
    with contextlib.redirect_stdout(io.StringIO()):
        t3.train(1)
    assert len(t3.losses) == 2 * len(its[0]) and np.isfinite(t3.losses).all()


def test_general_path_agrees_with_the_fused_run():
    """Weights and Adam's moments after 5 batches (one epoch of 4 full batches and a ragged one)."""
    class Mine(real_nvp.RealNVPTrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    cfg = dict(SMALL, n_train=4 * 16 + 9)
    tg, _ = parity(cfg, trainer_cls=Mine)                      # against the oracle
    assert tg._engine is None and len(tg.losses) == 5
    tf, state = parity(cfg)                                    # the fused run: same data, same shuffles
    worst = {k: rel(tg.model.state_dict()[k], tf.model.state_dict()[k].cpu()) for k in R.keys(cfg["K"])}
    print("general vs fused weights", max(worst.values()))
    assert max(worst.values()) <= R.PARAM_TOL
    fp, opt = tf._engine.fp, tg._general_opt
    assert fp.m.numel() == opt.m.numel()                       # the same flat layout
    dm, dv = (fp.m - opt.m).abs().max().item(), (fp.v - opt.v).abs().max().item()
    sm, sv = fp.m.abs().max().item(), fp.v.abs().max().item()
    print("general vs fused moments / scale", dm / sm, dv / sv)
    assert dm <= R.PARAM_TOL * sm and dv <= R.PARAM_TOL * sv
    for k, (L1, L2) in enumerate(tf._engine.C):                # and the fused moments against the oracle's Adam state
        for lin, name in ((L1, "couplings.%d.linear.weight" % k), (L2, "couplings.%d.out.weight" % k)):
            assert rel(lin.mW.view_as(state[name]["exp_avg"]), state[name]["exp_avg"]) <= R.PARAM_TOL
            assert rel(lin.vW.view_as(state[name]["exp_avg_sq"]), state[name]["exp_avg_sq"]) <= R.PARAM_TOL


# ---- encode, decode, sample, likelihood ---------------------------------------------------------------------------------------
class EditedRealNVP(real_nvp.RealNVP):
    """The same network as a user subclass: scored and sampled on the general path."""


def _case(cfg, cls=None):
    m = mk_model(cfg, cls)
    return real_nvp.RealNVPTrainer(m, *loaders(dict(cfg, n_train=16, n_val=16, n_test=24, batch=8)), seed=SEED), m


@pytest.mark.parametrize("cfg", [SMALL, SMALL_HALF], ids=["12-8-K3", "14-8-K3-half"])
def test_encode_decode_round_trip_is_exact(cfg):
    """decode(encode(x)[0]) returns the dequantised, requantised image: floor(x_hat levels) == q on every pixel; the codes
    and log p(x) against fp64 on the device's own noise."""
    tr, m = _case(cfg)
    n, D = 16, cfg["D"]
    x = grey(n, D, 5)
    st, mode = torch.get_rng_state(), m.training
    z, lp = tr.encode(x.view(n, 1, *cfg["shape"]), seed=4)
    xh = tr.decode(z)
    assert torch.equal(st, torch.get_rng_state()) and m.training == mode
    assert tuple(z.shape) == (n, D) and tuple(lp.shape) == (n,) and tuple(xh.shape) == (n, D)
    q = R.quantise(x, m.levels)
    assert torch.equal(torch.floor(xh.cpu().double() * m.levels), q)
    u = of_.nvp_uniforms(n, D, 4, gnvp.TAG_EVAL, step=0, device=DEV).cpu()
    P = R.f64(m.state_dict())
    rz, rlp = R.encode(P, x, u, flow_cfg(cfg, m))
    print("encode err / scale", rel(z, rz), rel(lp, rlp))
    assert rel(z, rz) <= R.LOSS_TOL and rel(lp, rlp) <= R.LOSS_TOL
    assert (xh.cpu().double() - R.decode(P, rz, flow_cfg(cfg, m))).abs().max().item() <= R.LOSS_TOL
    # rows are indexed by their position in the call: a batch boundary moves no row to another noise
    z2, lp2 = tr.encode(x, seed=4, batch=5)
    assert rel(z2, rz) <= R.LOSS_TOL and rel(lp2, rlp) <= R.LOSS_TOL
    assert torch.equal(torch.floor(tr.decode(z2, batch=7).cpu().double() * m.levels), q)
    # the general path (an edited model) on the same noise
    tg, mg = _case(cfg, EditedRealNVP)
    assert not gnvp.realnvp_fused_ok(mg) and gnvp.realnvp_fused_ok(m)
    zg, lpg = tg.encode(x, seed=4)
    assert rel(zg, rz) <= R.LOSS_TOL and rel(lpg, rlp) <= R.LOSS_TOL
    assert torch.equal(torch.floor(tg.decode(zg).cpu().double() * m.levels), q)
    line = tr.interpolate(x[0], x[1], 5)
    assert tuple(line.shape) == (5, D)
    assert torch.equal(torch.floor(line[0].cpu().double() * m.levels), q[0])
    assert torch.equal(torch.floor(line[-1].cpu().double() * m.levels), q[1])


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["12-8-K3", "784-400-K4"])
def test_sample_rows_do_not_depend_on_n(cfg):
    tr, m = _case(cfg)
    st = torch.get_rng_state()
    big, small = tr.sample(300, seed=6), tr.sample(5, seed=6)
    assert torch.equal(st, torch.get_rng_state())
    assert torch.equal(big[:5], small) and tuple(big.shape) == (300, cfg["D"])     # rows 0-4 of sample(300) == sample(5)
    assert big.min().item() >= 0.0 and big.max().item() <= 1.0
    assert not torch.equal(tr.sample(5, seed=7), small)
    # against fp64 from the rule's normals, temperature included
    P = R.f64(m.state_dict())
    for temp in (1.0, 0.5):
        ref = R.decode(P, torch.from_numpy(gnvp.normals_reference(5, cfg["D"], 6)) * temp, flow_cfg(cfg, m))
        err = (tr.sample(5, seed=6, temperature=temp).cpu().double() - ref).abs().max().item()
        print("sample err", temp, err)
        assert err <= R.LOSS_TOL
    tg, _ = _case(cfg, EditedRealNVP)
    assert (tg.sample(5, seed=6).cpu().double() - R.decode(P, torch.from_numpy(gnvp.normals_reference(5, cfg["D"], 6)),
                                                           flow_cfg(cfg, m))).abs().max().item() <= R.LOSS_TOL
    for bad in (dict(n=0), dict(n=2.0), dict(n=3, seed=-1), dict(n=3, temperature=-1.0), dict(n=3, temperature=float("nan"))):
        with pytest.raises(gnvp.RealNVPError):
            tr.sample(**bad)


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["12-8-K3", "784-400-K4"])
def test_log_likelihood_equals_the_oracles(cfg):
    tr, m = _case(cfg)
    x = tr.test_iter.dataset.tensors[0].reshape(24, -1)
    res = tr.log_likelihood(seed=3, batch=10)                  # the whole test_iter: batches of 10, 10, 4 rows
    noise = device_noise(cfg["D"], seed=3)
    P = R.f64(m.state_dict())
    ref = torch.cat([-R.nll_rows(P, x[i:i + 10].double(), noise(R.TAG_EVAL, i // 10, min(10, 24 - i)), flow_cfg(cfg, m))
                     for i in range(0, 24, 10)])
    rows = tr.log_likelihood_rows(seed=3, batch=10)
    print("ll err / scale", rel(rows, ref), res.ll_mean, ref.mean().item())
    assert rel(rows, ref) <= R.LOSS_TOL
    assert res.n == 24 and abs(res.ll_mean - ref.mean().item()) <= R.LOSS_TOL * abs(ref.mean().item())
    assert abs(res.ll_stderr - ref.std(unbiased=False).item() / math.sqrt(24)) <= R.LOSS_TOL * ref.abs().max().item()
    assert abs(tr.bits_per_dim(res) + res.ll_mean / (cfg["D"] * math.log(2.0))) < 1e-12
    again = tr.log_likelihood(seed=3, batch=10)
    assert again == res and tr.log_likelihood(seed=4, batch=10) != res      # reproducible, and the seed matters


def test_parzen_and_images(tmp_path):
    cfg = dict(SMALL, D=16, shape=(4, 4))
    tr, m = _case(cfg)
    st = torch.get_rng_state()
    res = tr.parzen(n_samples=64, n_val=8)
    assert np.isfinite([res.sigma, res.ll_mean, res.ll_stderr]).all() and np.isfinite(res.val_means).all()
    assert torch.equal(st, torch.get_rng_state())
    tr.viz_dir = str(tmp_path)
    imgs = tr.generate_images(3, num_outputs=4)
    assert imgs.shape == (4, 4, 4) and os.path.isfile(os.path.join(str(tmp_path), "RealNVP", "sample_3.png"))


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_learning_on_four_patterns():
    """64 rows at D = 16 made of 4 fixed grey-level patterns, 38 epochs of 4 fused batches of 16 (152 >= the 150 batches
    the fp64 reference's own training needs in tests/test_realnvp_cpu.py): the NLL of the 64 rows on the validation
    stream (seed 5, batch i at step i) ends below the identity flow's on the same stream."""
    D, H, K, b = 16, 8, 4, 16
    x = R.pattern_data(64, D).view(64, 1, 4, 4)
    mk = lambda: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(64, dtype=torch.int64)),
                                             batch_size=b, shuffle=True)
    torch.manual_seed(1234)
    m = real_nvp.RealNVP(D, H, K)
    tr = real_nvp.RealNVPTrainer(m, mk(), mk(), mk(), seed=5)
    cfg = dict(K=K, s_cap=m.s_cap, mask=m.mask, alpha=m.alpha, levels=m.levels)
    flat = x.reshape(64, D)
    ident = -tr.log_likelihood(flat, seed=5, batch=b).ll_mean           # a fresh model is the identity flow
    noise = device_noise(D, seed=5)
    ref = np.mean([R.nll_rows(R.f64(m.state_dict()), flat[i:i + b].double(), noise(R.TAG_EVAL, i // b, b), cfg).mean().item()
                   for i in range(0, 64, b)])
    assert abs(ident - ref) <= R.LOSS_TOL * abs(ref)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(38, lr=1e-3)
    val = -tr.log_likelihood(flat, seed=5, batch=b).ll_mean
    print("identity NLL", ident, "after 152 batches", val, "best validation", tr.best_val_loss)
    assert type(tr._engine).__name__ == "RealNVPEngine" and len(tr.losses) == 152 and np.isfinite(tr.losses).all()
    assert val < ident
