"""The masked autoregressive flow on the MI355X: every kernel of csrc/gm_maf.hip against fp64 (both paths of the row
kernels, saturated tanh, s_cap = 8, canary rows; the mask kernel's bit patterns; the one-launch inverse at every chunk
edge and register count, teacher-forced, causal, independent of n, in both orders and with reversed degrees, and its round
trip), the fused engine against an fp64 CPU loop that replays MAFTrainer's protocol, one batch's gradients against fp64
autograd, masked entries and moments, determinism, resume, the general path, encode / decode, sampling and the likelihood,
and learning itself.  tests/maf_reference.py is the reference of every comparison; the code under test never is."""
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

import maf  # noqa: E402
import maf_reference as R  # noqa: E402
from generative_models_amd import maf as gmaf  # noqa: E402
from generative_models_amd import ops, trainers  # noqa: E402
from generative_models_amd import ops_fused as of_  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
CANARY = -7.0
DS = [2, 7, 10, 16, 784]         # one ragged quad, element path, unaligned a half, the vector path, the full image
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


# ---- gm_maf_couple, gm_maf_couple_bwd ------------------------------------------------------------------------------------
def couple_inputs(b, D, seed):
    """[m | a] with m and a up to +-30 (tanh saturated at both ends), y of logit scale."""
    g = torch.Generator().manual_seed(seed)
    ma = (torch.rand(b, 2 * D, generator=g) * 2 - 1) * 30.0
    ma[:, D:] *= (torch.rand(b, D, generator=g) < 0.5).float() * 0.97 + 0.03        # half of the a inside +-0.9
    ma[0, D] = 30.0
    ma[0, 2 * D - 1] = -30.0
    return ma, torch.randn(b, D, generator=g) * 3.0


@pytest.mark.parametrize("D", DS)
def test_couple_kernel_against_fp64(D):
    cap = 8.0
    for b in BS:
        ma, y = couple_inputs(b, D, D + b)
        ld0 = torch.randn(b, generator=torch.Generator().manual_seed(b))
        u, ld = canary(b + 1, D), torch.full((b + 1,), CANARY, device=DEV)
        ld[:b] = ld0.to(DEV)
        of_.maf_couple(y.to(DEV), ma.to(DEV), u, ld, b, D, cap)
        ru, rs = R.couple(ma.double(), y.double(), cap)
        errs = rel(u[:b], ru), rel(ld[:b], ld0.double() - rs)
        print(D, b, "couple err / scale", errs)
        assert max(errs) <= R.LOSS_TOL
        assert torch.all(u[b] == CANARY) and ld[b].item() == CANARY
        # unaligned views: the element path gives the 16-byte path's bits
        bma, by, bu = canary(b, 2 * D + 1), canary(b, D + 3), canary(b, D + 2)
        bma[:, 1:], by[:, 2:2 + D] = ma.to(DEV), y.to(DEV)
        ld2 = ld0.to(DEV).clone()
        of_.maf_couple(by[:, 2:2 + D], bma[:, 1:], bu[:, 1:1 + D], ld2, b, D, cap)
        assert torch.equal(bu[:, 1:1 + D], u[:b]) and torch.equal(ld2, ld[:b])
        assert torch.all(bu[:, 0] == CANARY) and torch.all(bu[:, 1 + D] == CANARY)


@pytest.mark.parametrize("D", DS)
def test_couple_bwd_kernel_against_fp64(D):
    cap = 8.0
    for b in BS:
        ma, y = couple_inputs(b, D, 100 + D + b)
        g = torch.randn(b, D, generator=torch.Generator().manual_seed(D))
        u = torch.randn(b, D, generator=torch.Generator().manual_seed(D + 1)) * 3.0
        c = -float(np.float32(1.0 / b))
        dout, dy = canary(b + 1, 2 * D), canary(b + 1, D)
        of_.maf_couple_bwd(ma.to(DEV), u.to(DEV), g.to(DEV), dout, b, D, cap, c, dy=dy)
        rdout, rdy = R.couple_bwd(ma.double(), u.double(), g.double(), c, cap)
        errs = rel(dout[:b, :D], rdout[:, :D]), rel(dout[:b, D:], rdout[:, D:]), rel(dy[:b], rdy)
        print(D, b, "couple_bwd err / scale", errs)
        assert max(errs) <= R.LOSS_TOL
        assert torch.all(dout[b] == CANARY) and torch.all(dy[b] == CANARY)
        dout2 = canary(b, 2 * D)
        of_.maf_couple_bwd(ma.to(DEV), u.to(DEV), g.to(DEV), dout2, b, D, cap, c)
        assert torch.equal(dout2, dout[:b])                        # without dy: the same dout
        bma, bu, bg, bd, bdy = canary(b, 2 * D + 1), canary(b, D + 3), canary(b, D + 1), canary(b, 2 * D + 2), canary(b, D + 2)
        bma[:, 1:], bu[:, 2:2 + D], bg[:, 1:] = ma.to(DEV), u.to(DEV), g.to(DEV)
        of_.maf_couple_bwd(bma[:, 1:], bu[:, 2:2 + D], bg[:, 1:], bd[:, 1:1 + 2 * D], b, D, cap, c, dy=bdy[:, 1:1 + D])
        assert torch.equal(bd[:, 1:1 + 2 * D], dout[:b]) and torch.equal(bdy[:, 1:1 + D], dy[:b])
        assert torch.all(bd[:, 0] == CANARY) and torch.all(bd[:, 1 + 2 * D] == CANARY)
        assert torch.all(bdy[:, 0] == CANARY) and torch.all(bdy[:, 1 + D] == CANARY)


# ---- gm_maf_mask -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["natural", "random"])
@pytest.mark.parametrize("D,H", [(2, 1), (7, 5), (130, 70)])
def test_mask_kernel_bit_patterns(D, H, order):
    """Masked entries become +0.0 (all bits clear), every other entry keeps its bits -- NaNs included: no weight is read."""
    ins, m_h = gmaf.degrees(D, H, 2, order, 4)
    for m_in in ins:                                             # the order and its reverse
        M1, M2 = R.masks(m_in, m_h)
        g = torch.Generator().manual_seed(D)
        mk = lambda *s: torch.randint(1, (1 << 31) - 1, s, generator=g, dtype=torch.int32)     # arbitrary non-zero bit patterns
        W1, m1, v1, W2, m2, v2 = mk(H, D), mk(H * D), mk(H * D), mk(2 * D, H), mk(2 * D * H), mk(2 * D * H)
        dev = [t.to(DEV).view(torch.float32) for t in (W1, m1, v1, W2, m2, v2)]
        mi, mh = torch.from_numpy(m_in).to(DEV), torch.from_numpy(m_h).to(DEV)
        of_.maf_mask(dev[0], dev[3], mi, mh, moments1=(dev[1], dev[2]), moments2=(dev[4], dev[5]))
        for got, src, M in zip(dev, (W1, m1, v1, W2, m2, v2), (M1, M1, M1, M2, M2, M2)):
            want = torch.where(M.reshape(src.shape) == 1, src, torch.zeros_like(src))
            assert torch.equal(got.view(torch.int32).cpu(), want)
        W1b, W2b = W1.to(DEV).view(torch.float32), W2.to(DEV).view(torch.float32)
        of_.maf_mask(W1b, W2b, mi, mh)                           # without moments: the same weights
        assert torch.equal(W1b.view(torch.int32), dev[0].view(torch.int32))
        assert torch.equal(W2b.view(torch.int32), dev[3].view(torch.int32))


# ---- gm_maf_invert ---------------------------------------------------------------------------------------------------------
INV_D = [2, 7, 63, 64, 65, 130]                                  # the 64-position chunk's edges
INV_H = [1, 5, 64, 65, 70, 400, 1024]                            # NJ = 1, 2 with a partial last register, 7, 16
INV_N = [1, 4, 5]                                                # a partial workgroup
CAP = 2.0


def layer_args(P, k):
    g = lambda n: P["layers.%d.%s" % (k, n)]
    W1T = g("linear.weight").t().contiguous().to(DEV)
    inv = torch.from_numpy(R.inv_order(g("m_in").numpy()).astype(np.int32)).to(DEV)
    return (g("out.weight").to(DEV), g("out.bias").to(DEV), W1T, g("linear.bias").to(DEV), g("m_h").to(DEV), inv)


def teacher_forced(P64, k, u, y, cap=CAP):
    """(y', s) of fp64 from the device's own y: one masked forward pass, then y' = u exp(s) + m."""
    D = u.shape[1]
    ma = R.ma_of(P64, k, y.cpu().double())
    s = cap * torch.tanh(ma[:, D:])
    return u.cpu().double() * torch.exp(s) + ma[:, :D], s, ma[:, :D]


@pytest.mark.parametrize("D", INV_D)
def test_invert_kernel_teacher_forced_causal_and_canaries(D):
    """(a) on the device's own y the fp64 s_d and u_d exp(s_d) + m_d agree with the device's s and y within 1e-5 of each
    tensor's scale (the kernel returns y and s; m is pinned through them: m = y - u exp(s));  (b) changing u at position t
    leaves y at every earlier position bit-identical;  (d) both orders, and the layer with reversed degrees."""
    worst = 0.0
    for H in INV_H:
        for order in ("natural", "random"):
            sd = R.random_weights(D, H, 2, order, 11, seed=D + H, out_scale=0.5)
            P64 = R.f64(sd)
            for k in (0, 1):
                args = layer_args(sd, k)
                inv = args[5].long()
                for n in INV_N:
                    u = torch.randn(n, D, generator=torch.Generator().manual_seed(n + D)).to(DEV)
                    ybuf, sbuf = canary(n + 1, D + 3), canary(n + 1, D + 1)
                    y, s = ybuf[:n, 1:1 + D], sbuf[:n, :D]
                    of_.maf_invert(u, *args, CAP, n=n, y=y, s=s)
                    assert torch.isfinite(y).all()
                    ry, rs, _ = teacher_forced(P64, k, u, y)
                    errs = rel(y, ry), rel(s, rs)
                    worst = max(worst, *errs)
                    assert max(errs) <= R.LOSS_TOL, (D, H, order, k, n, errs)
                    assert torch.all(ybuf[n] == CANARY) and torch.all(ybuf[:, 0] == CANARY) and \
                        torch.all(ybuf[:, 1 + D:] == CANARY) and torch.all(sbuf[n] == CANARY) and torch.all(sbuf[:, D] == CANARY)
                    y2 = of_.maf_invert(u, *args, CAP, n=n)                      # without s, dense rows: the same bits
                    assert torch.equal(y2, y)
                    t = D // 2
                    u3 = u.clone()
                    u3[:, inv[t]] += 1.0
                    y3 = of_.maf_invert(u3, *args, CAP)
                    assert torch.equal(y3[:, inv[:t]], y[:, inv[:t]]) and not torch.equal(y3[:, inv[t]], y[:, inv[t]])
    print(D, "invert teacher-forced worst err / scale", worst)


@pytest.mark.parametrize("D,H", [(65, 70), (130, 400), (130, 1024)])
def test_invert_rows_do_not_depend_on_n(D, H):
    """(c) rows 0-4 of n = 300 equal n = 5 bit for bit; an out-of-range table entry is clamped, never followed."""
    sd = R.random_weights(D, H, 1, "random", 2, seed=D, out_scale=0.5)
    args = layer_args(sd, 0)
    u = torch.randn(300, D, generator=torch.Generator().manual_seed(3)).to(DEV)
    big, small = of_.maf_invert(u, *args, CAP), of_.maf_invert(u[:5].contiguous(), *args, CAP)
    assert torch.equal(big[:5], small) and torch.isfinite(big).all()
    bad = args[5].clone()
    bad[0], bad[1] = -5, D + 1000
    out = canary(6, D)
    of_.maf_invert(u[:5].contiguous(), *args[:5], bad, CAP, n=5, y=out)
    assert torch.all(out[5] == CANARY)


# The round trip's allowance: 4 x the deviation of the same chain in fp32 torch from fp64 (DESIGN.md section 24's margin).
ROUND_TRIP_MARGIN = 4.0


@pytest.mark.parametrize("D,H", [(7, 5), (65, 70), (130, 400), (130, 1024)])
def test_invert_round_trip(D, H):
    """(e) gm_maf_invert(forward(y)) against y, out weights of scale 0.05 / sqrt(H).  The yardstick is the same chain in
    fp32 torch on the CPU (forward, then the sequential inverse) against fp64 on the same y; the device may deviate from
    y by 4 x that.  Measured on an MI355X: see DESIGN.md section 30."""
    n = 5
    sd = R.random_weights(D, H, 1, "random", 9, seed=D + H, out_scale=0.05)
    P64, P32 = R.f64(sd), R.to_dtype(R.f64(sd), torch.float32)
    y = torch.randn(n, D, generator=torch.Generator().manual_seed(D)) * 2.0
    y64 = R.invert_layer(P64, 0, R.forward(P64, y.double(), 1, CAP)[0], CAP)[0]
    assert (y64 - y.double()).abs().max().item() <= 1e-12
    y32 = R.invert_layer(P32, 0, R.forward(P32, y, 1, CAP)[0], CAP)[0]
    yard = rel(y32, y64)
    c = {k: v.to(DEV) for k, v in sd.items()}
    h, ma, u = torch.empty(n, H, device=DEV), torch.empty(n, 2 * D, device=DEV), torch.empty(n, D, device=DEV)
    ops.linear_fwd(y.to(DEV), c["layers.0.linear.weight"], c["layers.0.linear.bias"], h, "relu")
    ops.linear_fwd(h, c["layers.0.out.weight"], c["layers.0.out.bias"], ma, "id")
    of_.maf_couple(y.to(DEV), ma, u, torch.zeros(n, device=DEV), n, D, CAP)
    back = of_.maf_invert(u, *layer_args(sd, 0), CAP)
    err = rel(back, y)
    print(D, H, "round trip err / scale", err, "fp32 torch yardstick", yard, "bound", ROUND_TRIP_MARGIN * yard)
    assert yard > 0 and err <= ROUND_TRIP_MARGIN * yard


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


SMALL = dict(D=12, H=8, K=3, shape=(3, 4), batch=16, n_train=40, n_val=24, n_test=16, order="natural")
SMALL_RANDOM = dict(SMALL, order="random")
FULL = dict(D=784, H=400, K=2, shape=(28, 28), batch=512, n_train=3 * 512 + 200, n_val=512 + 100, n_test=64,
            order="natural")
FULL_BITS = dict(FULL, binary=True)
SEED = 21
S_CAP = 2.0
# The weights of the 784-400 case on fp32 data, the one comparison that cannot meet 5e-5 (measured on an MI355X: 0.out.weight
# 3.0e-2, 1.out.weight 1.0e-3, 0.linear.weight 4.7e-4, 1.linear.weight 3.7e-5, every bias below 1.5e-6; the bit-packed case
# 7.5e-6).  Adam divides by sqrt(v) + 1e-8, so an entry whose gradient is of the size of 1e-8 and of its own fp32 error moves
# by a share of lr that no gradient bound controls -- and here lr (1e-3) is 0.4 of the out weights' scale (0.05 / sqrt(H)),
# so one such entry among 627 200 shows at the percent level.  The yardstick is the same loop in fp32 torch on the same rows
# and noise (maf_reference.oracle_train with dtype=torch.float32) against the fp64 run, per weight tensor, measured on the
# CPU with one thread and with eight (the same figures); the allowance is 4 x that (DESIGN.md sections 24 and 30).  The
# biases and every other comparison of weights keep 5e-5.
FULL_YARDSTICK = {"layers.0.linear.weight": 8.84e-4, "layers.0.out.weight": 1.69e-2, "layers.1.linear.weight": 5.34e-3,
                  "layers.1.out.weight": 8.23e-3}


def flow_cfg(cfg, tr):
    return dict(K=cfg["K"], s_cap=tr.s_cap, alpha=tr.alpha, levels=tr.levels)


CFG0 = dict(s_cap=S_CAP, alpha=0.05, levels=256)


def mk_model(cfg, cls=None, fresh=False):
    torch.manual_seed(1234)
    m = (cls or maf.MAF)(cfg["D"], cfg["H"], cfg["K"], cfg["order"], 3)
    if not fresh:                                    # non-zero out layers: every gradient path carries something
        scale = 0.5 if cfg["H"] < 64 else 0.05       # (a flow near the identity at H = 400, as training meets it)
        m.load_state_dict(R.random_weights(cfg["D"], cfg["H"], cfg["K"], cfg["order"], 3, seed=cfg["D"], out_scale=scale))
    return m


def product(cfg, its, epochs, use_graph=True, trainer_cls=None, model=None, **kw):
    m = mk_model(cfg) if model is None else model
    tr = (trainer_cls or maf.MAFTrainer)(m, *its, seed=SEED, s_cap=S_CAP)
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
    losses, vals, P, state = R.oracle_train(P0, dict(CFG0, K=cfg["K"]), its, epochs, device_rows(cfg),
                                            device_noise(cfg["D"]))
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
    tol = {k: R.PARAM_TOL for k in worst}
    if cfg["D"] == 784 and not cfg.get("binary", False):
        tol.update({k: 4 * v for k, v in FULL_YARDSTICK.items()})
    assert all(worst[k] <= tol[k] for k in worst), (worst, tol)
    return tr, state


@pytest.mark.parametrize("cfg", [SMALL, SMALL_RANDOM, FULL, FULL_BITS],
                         ids=["12-8-K3-b16-fp32", "12-8-K3-b16-random", "784-400-K2-b512-fp32", "784-400-K2-b512-bits"])
def test_engine_vs_fp64_oracle(cfg):
    tr, _ = parity(cfg)
    assert type(tr._engine).__name__ == "MAFEngine"
    assert type(tr._device_data(tr.train_iter)).__name__ == ("PackedData" if cfg.get("binary", False) else "Tensor")


@pytest.mark.parametrize("cfg", [SMALL, SMALL_RANDOM, FULL], ids=["12-8-K3-b16", "12-8-K3-b16-random", "784-400-K2-b512"])
def test_one_batch_gradients_vs_fp64(cfg):
    """One training batch through MAFEngine from known non-zero weights: the gradients it leaves in the flat gradient
    buffer against fp64 autograd on that batch and the device's own noise, within 1.5e-6 of each tensor's scale.  The
    dense weight-gradient GEMMs also fill the masked entries, which gm_maf_mask then discards: the comparison is over the
    kept entries (the reference's masked gradients are zero)."""
    b = cfg["batch"]
    its = loaders(dict(cfg, n_train=b, n_val=b, n_test=16))
    m = mk_model(cfg)
    init = R.f64(m.state_dict())
    tr = maf.MAFTrainer(m, *its, seed=SEED, s_cap=S_CAP)
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
    loss, grads = R.loss_and_grads(init, x, device_noise(cfg["D"])(R.TAG_TRAIN, 0, b), flow_cfg(cfg, tr))
    assert abs(tr.losses[0] - loss) <= R.LOSS_TOL * max(1.0, abs(loss))
    for k, gk in got.items():
        if k.endswith("weight"):
            M1, M2 = R.layer_masks(init, int(k.split(".")[1]))
            gk = gk.view_as(grads[k]) * (M1 if "linear" in k else M2)
        scale = grads[k].abs().max().item()
        assert scale > 0, k
        err = (gk.view_as(grads[k]) - grads[k]).abs().max().item()
        print(k, "grad err / scale", err / scale)
        assert err <= R.GRAD_TOL * scale, (k, err, scale)


def test_masked_entries_and_their_moments_stay_exactly_zero():
    """After 3 fused batches -- from weights loaded UNMASKED, which configure() masks once -- every masked entry of both
    weights and of both Adam moments is exactly 0, and the kept ones moved."""
    cfg = dict(SMALL_RANDOM, n_train=3 * 16, n_val=16)
    m = mk_model(cfg)
    with torch.no_grad():
        for c in m.layers:                                       # whatever was loaded
            c.linear.weight.add_(0.25)
            c.out.weight.add_(0.25)
    torch.manual_seed(99)
    tr, m = product(cfg, loaders(cfg), 1, model=m)
    assert len(tr.losses) == 3 and np.isfinite(tr.losses).all()
    for (L1, L2), c in zip(tr._engine.C, m.layers):
        M1, M2 = (t.to(DEV) for t in R.masks(c.m_in.cpu().numpy(), c.m_h.cpu().numpy()))
        for lin, M in ((L1, M1), (L2, M2)):
            assert lin.W[M == 1].abs().min().item() > 0
            for t in (lin.W, lin.mW.view_as(lin.W), lin.vW.view_as(lin.W)):
                assert not t[M == 0].any() and t[M == 1].any()


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
    cfg = SMALL_RANDOM
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
    new = lambda **kw: maf.MAF(cfg["D"], cfg["H"], cfg["K"], **dict(dict(order=cfg["order"], order_seed=3), **kw)).to(DEV)
    m2 = new()
    tr2 = maf.MAFTrainer(m2, *its, seed=SEED, s_cap=S_CAP)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == len(its[0])
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    same(snapshot(tr2, m2), runs[0])
    # a checkpoint of other settings is refused under strict=True, taken under strict=False
    for model, kw in ((new(), dict(seed=SEED, s_cap=S_CAP, alpha=0.1)), (new(), dict(seed=SEED + 1, s_cap=S_CAP)),
                      (new(), dict(seed=SEED, s_cap=S_CAP, levels=64)), (new(order_seed=4), dict(seed=SEED, s_cap=S_CAP))):
        t3 = maf.MAFTrainer(model, *its, **kw)
        t3.load_checkpoint(path)
        with pytest.raises(GMError, match="different settings"):
            t3.train(1)
    t3 = maf.MAFTrainer(new(), *its, seed=SEED, s_cap=3.0)
    t3.load_checkpoint(path, strict=False)
    with contextlib.redirect_stdout(io.StringIO()):
        t3.train(1)
    assert len(t3.losses) == 2 * len(its[0]) and np.isfinite(t3.losses).all()


def test_general_path_agrees_with_the_fused_run():
    """Weights and Adam's moments after 5 batches (one epoch of 4 full batches and a ragged one)."""
    class Mine(maf.MAFTrainer):
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
        for lin, name in ((L1, "layers.%d.linear.weight" % k), (L2, "layers.%d.out.weight" % k)):
            assert rel(lin.mW.view_as(state[name]["exp_avg"]), state[name]["exp_avg"]) <= R.PARAM_TOL
            assert rel(lin.vW.view_as(state[name]["exp_avg_sq"]), state[name]["exp_avg_sq"]) <= R.PARAM_TOL
    for c in tg.model.layers:                                  # the general path keeps the masked entries at zero too
        M1, M2 = (t.to(DEV) for t in R.masks(c.m_in.cpu().numpy(), c.m_h.cpu().numpy()))
        assert not c.linear.weight[M1 == 0].any() and not c.out.weight[M2 == 0].any()


# ---- encode, decode, sample, likelihood ---------------------------------------------------------------------------------------
class EditedMAF(maf.MAF):
    """The same network as a user subclass: scored and sampled on the general path."""


def _case(cfg, cls=None):
    m = mk_model(cfg, cls)
    return maf.MAFTrainer(m, *loaders(dict(cfg, n_train=16, n_val=16, n_test=24, batch=8)), seed=SEED, s_cap=S_CAP), m


@pytest.mark.parametrize("cfg", [SMALL, SMALL_RANDOM], ids=["12-8-K3", "12-8-K3-random"])
def test_encode_against_fp64_and_decode_requantises(cfg):
    """The codes and log p(x) against fp64 on the device's own noise; decode(encode(x)[0]) returns the dequantised,
    requantised image: floor(x_hat levels) == q on every pixel."""
    tr, m = _case(cfg)
    n, D = 16, cfg["D"]
    x = grey(n, D, 5)
    st, mode = torch.get_rng_state(), m.training
    z, lp = tr.encode(x.view(n, 1, *cfg["shape"]), seed=4)
    xh = tr.decode(z)
    assert torch.equal(st, torch.get_rng_state()) and m.training == mode
    assert tuple(z.shape) == (n, D) and tuple(lp.shape) == (n,) and tuple(xh.shape) == (n, D)
    q = R.quantise(x, tr.levels)
    assert torch.equal(torch.floor(xh.cpu().double() * tr.levels), q)
    u = of_.nvp_uniforms(n, D, 4, gmaf.TAG_EVAL, step=0, device=DEV).cpu()
    P = R.f64(m.state_dict())
    rz, rlp = R.encode(P, x, u, flow_cfg(cfg, tr))
    print("encode err / scale", rel(z, rz), rel(lp, rlp))
    assert rel(z, rz) <= R.LOSS_TOL and rel(lp, rlp) <= R.LOSS_TOL
    # rows are indexed by their position in the call: a batch boundary moves no row to another noise
    z2, lp2 = tr.encode(x, seed=4, batch=5)
    assert rel(z2, rz) <= R.LOSS_TOL and rel(lp2, rlp) <= R.LOSS_TOL
    assert torch.equal(torch.floor(tr.decode(z2, batch=7).cpu().double() * tr.levels), q)
    # the general path (an edited model) on the same noise
    tg, mg = _case(cfg, EditedMAF)
    assert not gmaf.maf_fused_ok(mg) and gmaf.maf_fused_ok(m)
    zg, lpg = tg.encode(x, seed=4)
    assert rel(zg, rz) <= R.LOSS_TOL and rel(lpg, rlp) <= R.LOSS_TOL
    assert torch.equal(torch.floor(tg.decode(zg).cpu().double() * tr.levels), q)


@pytest.mark.parametrize("cfg", [SMALL_RANDOM, FULL], ids=["12-8-K3-random", "784-400-K2"])
def test_sample_against_the_general_sampler_and_rows_do_not_depend_on_n(cfg):
    """sample(n) through gm_maf_invert against the general D-pass sampler on the same normals, teacher-forced: layer by
    layer, on the fused sampler's own y, the general model's forward pass gives s and y' = u exp(s) + m within 1e-5 of the
    tensor's scale (at 12-8 both samplers are also held, free-running, to fp64 from the rule's normals).  Rows 0-4 of sample(300) are sample(5); samples lie in [0, 1]."""
    tr, m = _case(cfg)
    tg, mg = _case(cfg, EditedMAF)
    D = cfg["D"]
    st = torch.get_rng_state()
    big, small = tr.sample(300, seed=6), tr.sample(5, seed=6)
    assert torch.equal(st, torch.get_rng_state())
    assert torch.equal(big[:5], small) and tuple(big.shape) == (300, D)
    assert big.min().item() >= 0.0 and big.max().item() <= 1.0
    assert not torch.equal(tr.sample(5, seed=7), small)
    z = torch.empty(5, D, device=DEV)
    of_.nvp_prior(*of_.maf_halves(z, D), 5, D, 6, "half", temperature=0.5)
    assert rel(z, torch.from_numpy(gmaf.normals_reference(5, D, 6)) * 0.5) <= R.LOSS_TOL
    with torch.no_grad():
        for c, cg in zip(reversed(m.layers), reversed(mg.layers)):
            inv = torch.from_numpy(gmaf.inverse_order(c.m_in)).to(DEV)
            s = torch.empty(5, D, device=DEV)
            y = of_.maf_invert(z, c.out.weight.detach(), c.out.bias.detach(), c.linear.weight.detach().t().contiguous(),
                               c.linear.bias.detach(), c.m_h, inv, S_CAP, s=s)
            ma = cg(y)                                           # the general sampler's pass, on the fused y
            sg = S_CAP * torch.tanh(ma[:, D:])
            yg = z * torch.exp(sg) + ma[:, :D]
            errs = rel(y, yg.cpu()), rel(s, sg.cpu())
            print("sample, teacher-forced err / scale", errs)
            assert max(errs) <= R.LOSS_TOL
            z = y
    half = tr.sample(5, seed=6, temperature=0.5)
    x = torch.empty(5, D, device=DEV)
    of_.nvp_post(*of_.maf_halves(z, D), x, 5, tr.alpha, "half")
    assert torch.equal(half, x)                                  # sample() is this chain
    if D <= 16:                                                  # both samplers, free-running, against fp64 from the rule's normals
        ref = R.decode(R.f64(m.state_dict()), torch.from_numpy(gmaf.normals_reference(5, D, 6)) * 0.5, flow_cfg(cfg, tr))
        errs = (half.cpu().double() - ref).abs().max().item(), \
            (tg.sample(5, seed=6, temperature=0.5).cpu().double() - ref).abs().max().item()
        print("sample err, fused and general", errs)
        assert max(errs) <= R.LOSS_TOL
    for bad in (dict(n=0), dict(n=2.0), dict(n=3, seed=-1), dict(n=3, temperature=-1.0), dict(n=3, temperature=float("nan"))):
        with pytest.raises(gmaf.MAFError):
            tr.sample(**bad)


@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["12-8-K3", "784-400-K2"])
def test_log_likelihood_equals_the_oracles(cfg):
    tr, m = _case(cfg)
    x = tr.test_iter.dataset.tensors[0].reshape(24, -1)
    res = tr.log_likelihood(seed=3, batch=10)                  # the whole test_iter: batches of 10, 10, 4 rows
    noise = device_noise(cfg["D"], seed=3)
    P = R.f64(m.state_dict())
    ref = torch.cat([-R.nll_rows(P, x[i:i + 10].double(), noise(R.TAG_EVAL, i // 10, min(10, 24 - i)), flow_cfg(cfg, tr))
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
    assert imgs.shape == (4, 4, 4) and os.path.isfile(os.path.join(str(tmp_path), "MAF", "sample_3.png"))


# ---- learning ----------------------------------------------------------------------------------------------------------------
def test_learning_on_four_patterns():
    """64 rows at D = 16 made of 4 fixed grey-level patterns, 38 epochs of 4 fused batches of 16 (152 >= the 150 batches
    the fp64 reference's own training needs in tests/test_maf_cpu.py): the NLL of the 64 rows on the validation stream
    (seed 5, batch i at step i) ends below the identity flow's on the same stream.  Both numbers are printed and recorded
    in DESIGN.md section 30."""
    D, H, K, b = 16, 8, 2, 16
    x = R.pattern_data(64, D).view(64, 1, 4, 4)
    mk = lambda: torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(64, dtype=torch.int64)),
                                             batch_size=b, shuffle=True)
    torch.manual_seed(1234)
    m = maf.MAF(D, H, K)
    tr = maf.MAFTrainer(m, mk(), mk(), mk(), seed=5)
    cfg = dict(K=K, s_cap=tr.s_cap, alpha=tr.alpha, levels=tr.levels)
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
    assert type(tr._engine).__name__ == "MAFEngine" and len(tr.losses) == 152 and np.isfinite(tr.losses).all()
    assert val < ident
