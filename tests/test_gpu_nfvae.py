"""Normalizing-flow VAE on the MI355X: the three flow kernels against the fp64 contract (tests/nfvae_reference.py) on the
device's own eps, the engine against fp64 training, determinism (run to run, graph against eager, resume), the general
path, log_likelihood (and that it is not iwae.log_likelihood's number), posterior_samples and a learning check.

Inputs.  The flow's parameters are drawn N(0, 0.3^2) under a fixed seed (at the initialisation's 0.01 every layer is
nearly the identity), and every test asserts min D >= 0.2 over its rows and layers on the fp64 reference: near D = 0 the
logarithm is ill-conditioned and agreement says nothing.

Bounds.  For what tests/test_gpu_iwae.py bounds (losses, ess, dml, the encoder's and decoder's gradients and weights) its
scheme and bases are used: max(base, 4 x the deviation of the same contract run in fp32 torch on the CPU from the fp64
reference), bases 1e-5 (loss sums), 1.5e-6 of max-abs (gradients), 5e-5 (weights).  For the new quantities (z_K, lp,
log q, the flow's gradients and parameters) the allowance is 4 x that fp32 deviation floored at 1.5e-6 of max-abs.  The
factor 4 is the project's margin for another, equally valid fp32 summation order.  Every comparison prints its error and
its allowance."""
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

import nf_vae  # noqa: E402
import nfvae_reference as R  # noqa: E402
from generative_models_amd import ops_fused, trainers  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd._lib import FLOW_PART_STRIDE, GMError  # noqa: E402

DEV = "cuda"
T_LOSS, T_GRAD, T_PARAM = 1e-5, 1.5e-6, 5e-5             # test_gpu_iwae.py's bases (module docstring)
MIN_D = 0.2
ROW_CASES = [(5, 1, 1, 7), (20, 3, 3, 7), (32, 32, 2, 16), (20, 8, 5, 130)]          # (Z, K, k, B)


def dev32(a):
    return torch.as_tensor(np.asarray(a, dtype=np.float32)).to(DEV).contiguous()


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        out = fn(*a, **kw)
    torch.cuda.synchronize()
    return out


def scaled_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)


def allowance(base, ref, f32):
    """max(base, 4 x the fp32 CPU run's deviation from the fp64 reference), in units of the tensor's max-abs."""
    return max(base, 4.0 * scaled_err(f32, ref))


def check(tag, name, got, ref, f32, base=T_GRAD):
    tol, err = allowance(base, ref, f32), scaled_err(got, ref)
    print("%s %s: err %.3g allowed %.3g (fp32 cpu %.3g)" % (tag, name, err, tol, scaled_err(f32, ref)))
    assert err <= tol, (tag, name, err, tol)
    return err


def row_inputs(Z, K, k, B):
    g = torch.Generator().manual_seed(1000 * Z + 10 * K + k)
    ml = torch.randn(B, 2 * Z, generator=g)
    ml[:, Z:] = ml[:, Z:] * 0.5 - 1.0
    flow = R.flow_params(K, Z, seed=K + Z)
    wn = torch.softmax(3 * torch.randn(B, k, generator=g), 1).reshape(-1)
    dzdec = torch.randn(B * k, Z, generator=g)
    return ml, flow, wn, dzdec


def dev_flow(flow):
    t = tuple(dev32(flow[n]) for n in R.FLOW)
    return t, ops_fused.flow_params(*t)


# ---- kernels against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Z,K,k,B", ROW_CASES)
def test_flow_sample_vs_fp64(Z, K, k, B):
    ml, flow, _, _ = row_inputs(Z, K, k, B)
    seed, step, tag = 0x123456789ABCDEF, 77, giwae.TAG_TRAIN
    noise = ops_fused.iwae_noise(seed, tag, k, step=step)
    mld = ml.to(DEV)

    def run(fl, m=mld):
        z, lp = torch.full((B * k, Z), 7.0, device=DEV), torch.full((B * k,), 7.0, device=DEV)
        ops_fused.flow_sample(m, z, lp, noise, fl, B, k, Z)
        torch.cuda.synchronize()
        return z.cpu(), lp.cpu()
    # the noise is iwae_normals' stream bit for bit: with w = 0 and b = 0 every layer adds u^ tanh(0) = 0 whatever K, and
    # with mu = 0, lv = 0 the kernel's z_0 = eps is what comes out
    eps = ops_fused.iwae_normals(B, k, Z, seed, step, tag)
    keep, ident = dev_flow({"flow.u": flow["flow.u"], "flow.w": np.zeros((K, Z)), "flow.b": np.zeros(K)})
    z_id, lp_id = run(ident, torch.zeros(B, 2 * Z, device=DEV))
    assert torch.equal(z_id, eps.cpu())
    half = 0.5 * (eps.cpu().double().numpy() ** 2).sum(1).max()           # lp = 1/2 |eps|^2 - 1/2 |eps|^2 in fp32
    assert np.abs(lp_id.numpy()).max() <= 4 * np.finfo(np.float32).eps * half
    keep, fl = dev_flow(flow)
    z, lp = run(fl)
    z2, lp2 = run(fl)
    assert torch.equal(z, z2) and torch.equal(lp, lp2)
    e = eps.cpu().double().numpy()
    ref = R.rows_reference(ml, e, flow, k)
    f32 = R.rows_reference(ml, e, flow, k, torch.float32)
    print("sample Z=%d K=%d k=%d B=%d: min D %.3f" % (Z, K, k, B, ref["minD"]))
    assert ref["minD"] >= MIN_D
    for name, got in (("z", z), ("lp", lp)):
        check("sample Z=%d K=%d k=%d B=%d" % (Z, K, k, B), name, got.numpy(), ref[name], f32[name])


def _reduce_step(ml, flow, wn, dzdec, Z, K, k, B, seed, step, lr=1e-3, wd=1e-5):
    (u, w, b), fl = dev_flow(flow)
    noise = ops_fused.iwae_noise(seed, giwae.TAG_TRAIN, k, step=step)
    dml = torch.full((B, 2 * Z), 7.0, device=DEV)
    part = ops_fused.flow_parts(B, K, device=DEV).fill_(7.0)
    n = K * Z
    mom = [torch.zeros(c, device=DEV) for c in (n, n, n, n, K, K)]
    grads = [torch.full((c,), 7.0, device=DEV) for c in (n, n, K)]
    sched = torch.from_numpy(trainers.ops.adam_schedule(lr, 1)).to(DEV)
    ops_fused.flow_reduce(ml.to(DEV), wn.to(DEV), dzdec.to(DEV), dml, part, noise, fl, B, k, Z)
    ops_fused.flow_step(part, B, u, w, b, mom, sched, grads=grads, weight_decay=wd)
    torch.cuda.synchronize()
    assert part.shape == ((B + 7) // 8, K, FLOW_PART_STRIDE)
    return {"dml": dml.cpu(), "flow.u": grads[0].view(K, Z).cpu(), "flow.w": grads[1].view(K, Z).cpu(),
            "flow.b": grads[2].cpu(), "p": [t.cpu() for t in (u, w, b)], "mom": [t.cpu() for t in mom]}


@pytest.mark.parametrize("Z,K,k,B", ROW_CASES)
def test_flow_reduce_and_step_vs_fp64(Z, K, k, B):
    ml, flow, wn, dzdec = row_inputs(Z, K, k, B)
    seed, step, lr, wd = 9, 5, 1e-3, 1e-5
    tag = "reduce Z=%d K=%d k=%d B=%d" % (Z, K, k, B)
    eps = ops_fused.iwae_normals(B, k, Z, seed, step, giwae.TAG_TRAIN).cpu().double().numpy()   # the device's own
    ref = R.rows_reference(ml, eps, flow, k, wn=wn, dzdec=dzdec)
    f32 = R.rows_reference(ml, eps, flow, k, torch.float32, wn=wn, dzdec=dzdec)
    assert ref["minD"] >= MIN_D
    got = _reduce_step(ml, flow, wn, dzdec, Z, K, k, B, seed, step, lr, wd)
    for name in ("dml",) + R.FLOW:
        check(tag, name, got[name].numpy(), ref[name], f32[name])
    # one Adam step on those gradients is FlatAdam's, bit for bit (the same schedule, the same arithmetic)
    ps = [torch.nn.Parameter(dev32(flow[n])) for n in R.FLOW]
    for p, n in zip(ps, R.FLOW):
        p.grad = got[n].to(DEV).reshape(p.shape)
    opt = trainers.FlatAdam(ps, lr, weight_decay=wd)
    opt.step()
    torch.cuda.synchronize()
    for i, (p, o) in enumerate(zip(ps, opt.offs)):
        c = p.numel()
        assert torch.equal(got["p"][i].reshape(-1), p.detach().cpu().reshape(-1)), R.FLOW[i]
        assert not torch.equal(got["p"][i].reshape(-1), dev32(flow[R.FLOW[i]]).cpu().reshape(-1))    # and it moved
        assert torch.equal(got["mom"][2 * i], opt.m[o:o + c].cpu()) and torch.equal(got["mom"][2 * i + 1],
                                                                                   opt.v[o:o + c].cpu()), R.FLOW[i]
    # run to run: the same bits
    again = _reduce_step(ml, flow, wn, dzdec, Z, K, k, B, seed, step, lr, wd)
    for name in ("dml",) + R.FLOW:
        assert torch.equal(again[name], got[name]), name
    for a, b_ in zip(again["p"] + again["mom"], got["p"] + got["mom"]):
        assert torch.equal(a, b_)


def test_flow_reduce_does_not_depend_on_where_a_row_lands():
    """The noise row is the batch position, so the same image at another position draws another eps.  With lv = -200 the
    standard deviation is 0 in fp32 and z_0 = mu whatever eps: then rotating the batch by 3 images moves every image to
    another lane group and most to another workgroup, and d loss / d mu of each image must keep its bits (its k samples
    are summed in the same order wherever it lands); the flow's gradients are the same sums in another order."""
    Z, K, k, B = 20, 8, 5, 130
    ml, flow, wn, dzdec = row_inputs(Z, K, k, B)
    ml[:, Z:] = -200.0
    a = _reduce_step(ml, flow, wn, dzdec, Z, K, k, B, 9, 5)
    sh = 3
    rot = lambda t, rows: torch.roll(t.reshape(B, rows, -1), sh, 0).reshape(t.shape)
    b = _reduce_step(torch.roll(ml, sh, 0), flow, rot(wn, k), rot(dzdec, k), Z, K, k, B, 9, 5)
    assert torch.equal(torch.roll(a["dml"], sh, 0), b["dml"])
    assert torch.all(a["dml"][:, Z:] == -0.5)
    eps = np.zeros((B * k, Z))
    ref = R.rows_reference(ml, eps, flow, k, wn=wn, dzdec=dzdec)
    f32 = R.rows_reference(ml, eps, flow, k, torch.float32, wn=wn, dzdec=dzdec)
    assert ref["minD"] >= MIN_D
    for name in R.FLOW:
        check("rotated", name, b[name].numpy(), ref[name], f32[name])
        check("unrotated", name, a[name].numpy(), ref[name], f32[name])


# ---- the engine against fp64 training -----------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, I, seed=7):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


def make_model(I, H, Z, K, seed=1234):
    torch.manual_seed(seed)
    m = nf_vae.NFVAE(I, H, Z, K)
    f = R.flow_params(K, Z, seed=K + Z)
    with torch.no_grad():
        for n in R.FLOW:
            getattr(m.flow, n.split(".")[1]).copy_(torch.as_tensor(f[n], dtype=torch.float32))
    return m, {n: v.detach().clone().double().numpy() for n, v in m.state_dict().items()}


def engine_views(tr, what):
    """{state_dict name: tensor} of the engine's flat gradient buffer or moments."""
    fp = tr._engine.fp
    out = {}
    for n, p in tr.model.named_parameters():
        i = [j for j, q in enumerate(fp.params) if q is p][0]
        o = fp.offsets[i]
        out[n] = getattr(fp, what)[o:o + p.numel()].view(p.shape).cpu()
    return out


@pytest.mark.parametrize("I,H,Z,K,k,batch,n_train", [(49, 32, 5, 3, 1, 16, 89), (49, 32, 5, 3, 3, 16, 89),
                                                      (784, 400, 20, 8, 1, 512, 1536)])
def test_engine_vs_fp64_training(I, H, Z, K, k, batch, n_train):
    """One epoch on the fused engine (6 batches of 16 with a ragged last one of 9, or 3 of 512) against Adam on the fp64
    reference's gradients, batch by batch on the device's own eps: losses, ess, every parameter.  The fp32 yardstick is
    the same loop with float32 arithmetic and float32 parameters and moments."""
    its = loaders(batch, n_train, batch, 16, I)
    m, P = make_model(I, H, Z, K)
    tr = nf_vae.NFVAETrainer(m, *its, k=k, seed=3)
    st = torch.get_rng_state()
    quiet(tr.train, 1)
    assert type(tr._engine).__name__ == "NFVAEEngine" and tr._engine.run_config["num_flows"] == K
    nb = (n_train + batch - 1) // batch
    assert len(tr.losses) == len(tr.ess) == nb and tr.noise_steps == nb
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].double().numpy()
    batches = [x[i:i + batch] for i in range(0, n_train, batch)]
    eps_of = lambda t, b: ops_fused.iwae_normals(b, k, Z, 3, t, giwae.TAG_TRAIN).cpu().double().numpy()
    Pr, Lr, Er = R.train_reference(P, batches, eps_of, k, 1e-3, 1e-5)
    P32, L32, E32 = R.train_reference(P, batches, eps_of, k, 1e-3, 1e-5, torch.float32)
    assert R.model_reference(P, batches[0], eps_of(0, batches[0].shape[0]), k)["minD"] >= MIN_D
    assert R.model_reference(Pr, batches[-1], eps_of(nb - 1, batches[-1].shape[0]), k)["minD"] >= MIN_D
    tag = "engine %s K=%d k=%d" % ((I, H, Z), K, k)
    for t in range(nb):
        for name, got, ref, f32 in (("loss", tr.losses, Lr, L32), ("ess", tr.ess, Er, E32)):
            check(tag, "%s[%d]" % (name, t), got[t], ref[t], f32[t], T_LOSS)
    got = {n: v.detach().cpu().double().numpy() for n, v in m.state_dict().items()}
    for n in R.ENC_DEC:                                                   # test_gpu_iwae.py's absolute weight bound
        err, tol = np.abs(got[n] - Pr[n]).max(), max(T_PARAM, 4 * np.abs(P32[n] - Pr[n]).max())
        print("%s %s: err %.3g allowed %.3g" % (tag, n, err, tol))
        assert err <= tol, (n, err, tol)
    for n in R.FLOW:
        assert np.abs(Pr[n] - P[n]).max() > 1e-4                          # the flow trained
        check(tag, n, got[n], Pr[n], P32[n])


def test_one_fused_batch_gradients_vs_fp64():
    """One batch with Adam's lr = 0 (the parameters stay, the gradients land in the flat gradient buffer): loss, ess and
    the thirteen gradients against autograd on the fp64 reference."""
    I, H, Z, K, k, b = 130, 24, 6, 5, 4, 17
    its = loaders(b, b, b, 16, I)
    m, P = make_model(I, H, Z, K)
    tr = nf_vae.NFVAETrainer(m, *its, k=k, seed=3)
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
    for n, v in m.state_dict().items():
        assert np.array_equal(v.cpu().double().numpy(), P[n]), n          # lr = 0: nothing moved
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    eps = ops_fused.iwae_normals(b, k, Z, 3, 0, giwae.TAG_TRAIN).cpu().double().numpy()
    ref, f32 = R.model_reference(P, x, eps, k), R.model_reference(P, x, eps, k, torch.float32)
    assert ref["minD"] >= MIN_D
    check("batch", "loss", tr.losses[0], -ref["L"].sum(), -f32["L"].sum(), T_LOSS)
    check("batch", "ess", tr.ess[0], ref["ess"].mean(), f32["ess"].mean(), T_LOSS)
    got = engine_views(tr, "grad")
    assert sorted(got) == sorted(R.KEYS)
    for n in R.KEYS:
        check("batch", n, got[n].numpy(), ref["grads"][n], f32["grads"][n])


# ---- determinism ----------------------------------------------------------------------------------------------------------
def _trained_small(k=3, seed=0, epochs=1, cls=None, use_graph=True, n_train=96, I=64, H=48, Z=8, K=4, batch=32, its=None):
    its = its or loaders(batch, n_train, 48, 48, I)
    m, _ = make_model(I, H, Z, K)
    tr = (cls or nf_vae.NFVAETrainer)(m, *its, k=k, seed=seed)
    tr.use_graph = use_graph
    quiet(tr.train, epochs)
    return tr, m, its


def snapshot(tr, m):
    return (list(tr.losses), list(tr.ess), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state())


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert torch.equal(a[4], b[4])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_bitwise_reproducibility_graph_eager_and_resume(tmp_path):
    cfg = dict(n_train=300, batch=64)                       # 300 rows, bs 64: four full batches and one of 44
    runs = []
    for use_graph in (True, True, False):                   # graph twice, then eager
        torch.manual_seed(99)
        tr, m, _ = _trained_small(epochs=3, use_graph=use_graph, **cfg)
        runs.append(snapshot(tr, m))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    assert len(runs[0][0]) == 15 and all(math.isfinite(v) for v in runs[0][0] + runs[0][1])
    # 2 epochs + checkpoint + a fresh trainer's resumed epoch == 3 epochs
    torch.manual_seed(99)
    tr, m, its = _trained_small(epochs=2, **cfg)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    assert ck["optim"]["config"]["num_flows"] == 4 and ck["optim"]["config"]["k"] == 3
    assert ck["history"]["noise_steps"] == 10 and "flow.u" in ck["model"]
    m2 = nf_vae.NFVAE(64, 48, 8, 4).to(DEV)
    tr2 = nf_vae.NFVAETrainer(m2, *its, k=3, seed=0)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 10 and tr2.losses == runs[0][0][:10]
    quiet(tr2.train, 1)
    same(snapshot(tr2, m2), runs[0])
    # other settings: refused under strict, taken otherwise
    ck["optim"]["config"]["num_flows"] = 5
    other = str(tmp_path / "ck5.pt")
    torch.save(ck, other)
    for p, kw in ((other, dict(k=3, seed=0)), (path, dict(k=2, seed=0)), (path, dict(k=3, seed=1))):
        t3 = nf_vae.NFVAETrainer(nf_vae.NFVAE(64, 48, 8, 4).to(DEV), *its, **kw)
        t3.load_checkpoint(p)
        with pytest.raises(GMError):
            t3.train(1)
    t3 = nf_vae.NFVAETrainer(nf_vae.NFVAE(64, 48, 8, 4).to(DEV), *its, k=3, seed=0)
    t3.load_checkpoint(other, strict=False)
    quiet(t3.train, 1)


# ---- paths ------------------------------------------------------------------------------------------------------------------
class Mine(nf_vae.NFVAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_general_path_agrees_with_the_fused_run(monkeypatch):
    """Parameters within test_gpu_iwae.py's 5e-5; the moments (sums of three gradients, of their squares) within 1e-4 of
    their max-abs, the bound that test puts on the two paths' losses."""
    made = []

    class Keep(trainers.FlatAdam):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(giwae, "FlatAdam", Keep)
    out = []
    for cls in (nf_vae.NFVAETrainer, Mine):
        torch.manual_seed(99)
        tr, m, _ = _trained_small(cls=cls, n_train=96, batch=32)          # 3 batches
        assert (tr._engine is None) == (cls is Mine) and len(tr.losses) == 3 and tr.noise_steps == 3
        out.append((tr, {k: v.cpu() for k, v in m.state_dict().items()}))
    (a, wa), (b, wb) = out
    assert len(made) == 1
    for n in wa:
        err = (wa[n] - wb[n]).abs().max().item()
        print("general path %s: %.3g" % (n, err))
        assert err <= T_PARAM, n
    for u, v in zip(a.losses + a.ess + [a.best_val_loss], b.losses + b.ess + [b.best_val_loss]):
        assert abs(u - v) <= 1e-4 * max(1.0, abs(v)), (u, v)
    opt = made[0]
    for what, flat in (("m", opt.m), ("v", opt.v)):
        fused = engine_views(a, what)
        for (n, p), o in zip(b.model.named_parameters(), opt.offs):
            err = scaled_err(flat[o:o + p.numel()].cpu().numpy(), fused[n].reshape(-1).numpy())
            print("general path %s of %s: %.3g" % (what, n, err))
            assert err <= 1e-4, (what, n, err)
    # K above the fused limit: the general path, same interface
    torch.manual_seed(99)
    tr, m, _ = _trained_small(K=33, n_train=64, batch=32)
    assert tr._engine is None and len(tr.losses) == 2 and all(math.isfinite(v) for v in tr.losses + tr.ess)


# ---- log_likelihood and posterior_samples ------------------------------------------------------------------------------
def test_log_likelihood_and_posterior_samples():
    I, H, Z, K, n, k = 130, 24, 6, 3, 17, 130               # 130 samples: chunks of 64, 64 and 2
    its = loaders(16, 32, 16, n, I)
    m, P = make_model(I, H, Z, K)
    tr = nf_vae.NFVAETrainer(m, *its, k=1, seed=0)
    tr.model.train()
    x = its[2].dataset.tensors[0]
    before = {k_: v.detach().cpu().clone() for k_, v in tr.model.state_dict().items()}
    torch.manual_seed(4)
    rng = torch.get_rng_state()
    res = tr.log_likelihood(k=k, seed=1)                                   # images=None: the whole test_iter
    assert torch.equal(torch.get_rng_state(), rng) and tr.model.training
    for k_, v in tr.model.state_dict().items():
        assert torch.equal(v.cpu(), before[k_]), k_
    assert (res.k, res.n) == (k, n) and type(res).__name__ == "IWAEResult"
    eps = ops_fused.iwae_normals(n, k, Z, 1, 0, giwae.TAG_EVAL).cpu().double().numpy()
    ref = R.model_reference(P, x.double().numpy(), eps, k)
    f32 = R.model_reference(P, x.double().numpy(), eps, k, torch.float32)
    assert ref["minD"] >= MIN_D
    ll = ref["L"] - 0.5 * I * math.log(math.pi)
    tol = allowance(T_LOSS, ref["L"], f32["L"]) * np.abs(ref["L"]).max()
    print("log_likelihood: mean %.6f ref %.6f allowed %.3g" % (res.ll_mean, ll.mean(), tol))
    assert abs(res.ll_mean - ll.mean()) <= tol
    assert abs(res.ll_stderr - ll.std() / math.sqrt(n)) <= tol
    assert tr.log_likelihood(x, k=k, seed=1) == res                        # bitwise: same seed, explicit images
    assert tr.log_likelihood(x, k=k, seed=2).ll_mean != res.ll_mean
    # the trap: iwae.log_likelihood takes this model and scores it with the flow left out of q
    wrong = giwae.log_likelihood(tr, x, k, 1)
    print("log_likelihood: iwae.log_likelihood on the same model gives %.6f" % wrong.ll_mean)
    assert abs(wrong.ll_mean - ll.mean()) > tol and abs(res.ll_mean - wrong.ll_mean) > tol
    # posterior_samples: the same stream, z_K and log q(z_K | x)
    z, lq = tr.posterior_samples(x, k, seed=1)
    assert z.shape == (n, k, Z) and lq.shape == (n, k) and z.dtype == torch.float32 and lq.dtype == torch.float64
    check("posterior_samples", "z", z.reshape(n * k, Z).numpy(), ref["z"], f32["z"])
    check("posterior_samples", "log_q", lq.reshape(-1).numpy(), ref["log_q"], f32["log_q"])
    z2, lq2 = tr.posterior_samples(x, k, seed=1)
    assert torch.equal(z, z2) and torch.equal(lq, lq2)


# ---- learning check -----------------------------------------------------------------------------------------------------
def test_learning_on_bands():
    """The 16 band patterns tests/test_gpu_made.py learns on (16 x 16 images, two adjacent rows or columns lit)."""
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
    its = bands(64), bands(16), bands(16)
    torch.manual_seed(5)
    tr = nf_vae.NFVAETrainer(nf_vae.NFVAE(256, 128, 8, 4), *its, k=1, seed=0)
    quiet(tr.train, 5)
    assert type(tr._engine).__name__ == "NFVAEEngine"
    assert len(tr.losses) == 80 and all(math.isfinite(v) for v in tr.losses + tr.ess)
    first, last = np.mean(tr.losses[:10]), np.mean(tr.losses[-10:])
    print("learning: first 10 %.3f last 10 %.3f" % (first, last))
    assert last < first
