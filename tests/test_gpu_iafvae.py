"""IAF-VAE on the MI355X: the three flow kernels against the fp64 contract (tests/iafvae_reference.py) on the device's own
eps, the engine against fp64 training, determinism (run to run, graph against eager, resume), the general path,
log_likelihood (and that it is not iwae.log_likelihood's number), posterior_samples and a learning check.

Inputs.  The flow's parameters are drawn under a fixed seed with std 1 / sqrt(fan_in) before masking, biases N(0, 0.3^2)
with +1 on the gate half (iafvae_reference.flow_params); every row test asserts on the fp64 reference max |s| <= 8 (a
saturated gate has no bits left in 1 - g) and max |z_K - z_0| >= 0.4 (an identity kernel cannot pass).

Bounds.  tests/test_gpu_nfvae.py's scheme.  For what tests/test_gpu_iwae.py bounds (losses, ess, the encoder's and
decoder's gradients and weights) its bases are used: max(base, 4 x the deviation of the same contract run in fp32 torch
on the CPU from the fp64 reference), bases 1e-5 (loss sums), 1.5e-6 of max-abs (gradients), 5e-5 (weights).  For the new
quantities (z_K, lp, log q, the flow's gradients and parameters, dh) the allowance is 4 x that fp32 deviation floored at
1.5e-6 of max-abs.  The factor 4 is the project's margin for another, equally valid fp32 summation order.  Every
comparison prints its error and its allowance."""
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

import iaf_vae  # noqa: E402
import iafvae_reference as R  # noqa: E402
from generative_models_amd import ops_fused, trainers  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
T_LOSS, T_GRAD, T_PARAM = 1e-5, 1.5e-6, 5e-5             # test_gpu_iwae.py's bases (module docstring)


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


def conditioned(tag, ref):
    print("%s: max |s| %.2f, max |z_K - z_0| %.2f" % (tag, ref["smax"], ref["move"]))
    assert ref["smax"] <= R.S_CAP and ref["move"] >= R.MIN_MOVE, (tag, ref["smax"], ref["move"])


def row_inputs(Z, K, F, C, k, B):
    """iafvae_reference.row_inputs with wn rounded to float32, as the device reads it."""
    ml, flow, wn, dzdec = R.row_inputs(Z, K, F, C, k, B)
    return ml, flow, wn.float(), dzdec


def dev_flow(flow):
    t = tuple(dev32(flow[n]) if n in flow else None for n in R.FLOW_ALL)
    return t, ops_fused.iaf_params(*t)


# ---- kernels against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Z,K,F,C,k,B", R.ROW_CASES)
def test_iaf_sample_vs_fp64(Z, K, F, C, k, B):
    ml, flow, _, _ = row_inputs(Z, K, F, C, k, B)
    seed, step, tag = 0x123456789ABCDEF, 77, giwae.TAG_TRAIN
    noise = ops_fused.iwae_noise(seed, tag, k, step=step)
    mld = ml.to(DEV)
    name = "sample Z=%d K=%d F=%d C=%d k=%d B=%d" % (Z, K, F, C, k, B)

    def run(fl, m=mld):
        z, lp = torch.full((B * k, Z), 7.0, device=DEV), torch.full((B * k,), 7.0, device=DEV)
        ops_fused.iaf_sample(m, z, lp, noise, fl, B, k, Z)
        torch.cuda.synchronize()
        return z.cpu(), lp.cpu()
    # the noise is iwae_normals' stream bit for bit: with W2 = 0, b2m = 0 and b2s = 40 the gate is exactly 1.0 in fp32 and
    # every layer returns its input whatever K; with mu = 0, lv = 0 the kernel's z_0 = eps is what comes out
    eps = ops_fused.iwae_normals(B, k, Z, seed, step, tag)
    ident = dict(flow)
    ident["flow.W2"] = np.zeros((K, 2 * Z, F))
    ident["flow.b2"] = np.concatenate([np.zeros((K, Z)), np.full((K, Z), 40.0)], axis=1)
    keep, idf = dev_flow(ident)
    zero = torch.zeros(B, 2 * Z + C, device=DEV)
    zero[:, 2 * Z:] = mld[:, 2 * Z:]
    z_id, lp_id = run(idf, zero)
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
    conditioned(name, ref)
    for q, got in (("z", z), ("lp", lp)):
        check(name, q, got.numpy(), ref[q], f32[q])


def _reduce_step(ml, flow, wn, dzdec, Z, K, F, C, k, B, seed, step, lr=1e-3, wd=1e-5):
    params, fl = dev_flow(flow)
    noise = ops_fused.iwae_noise(seed, giwae.TAG_TRAIN, k, step=step)
    W = 2 * Z + C
    dml = torch.full((B, W), 7.0, device=DEV)
    part = ops_fused.iaf_parts(B, k, K, Z, F, C, device=DEV).fill_(7.0)
    assert part.shape == (ops_fused.iaf_nparts(B, k), K, ops_fused.iaf_part_stride(Z, F, C))
    mom = [None if p is None else (torch.zeros(p.numel(), device=DEV), torch.zeros(p.numel(), device=DEV))
           for p in params]
    grads = [None if p is None else torch.full((p.numel(),), 7.0, device=DEV) for p in params]
    m_in = torch.as_tensor(R.degrees(Z, F, K)[0], dtype=torch.int32).to(DEV)
    sched = torch.from_numpy(trainers.ops.adam_schedule(lr, 1)).to(DEV)
    ops_fused.iaf_reduce(ml.to(DEV), wn.to(DEV), dzdec.to(DEV), dml, part, noise, fl, B, k, Z)
    ops_fused.iaf_step(part, B, k, params, m_in, mom, sched, grads=grads, weight_decay=wd)
    torch.cuda.synchronize()
    out = {"dml": dml.cpu(), "p": {}, "m": {}, "v": {}}
    for n, p, g, mv in zip(R.FLOW_ALL, params, grads, mom):
        if p is not None:
            out[n] = g.view(p.shape).cpu()
            out["p"][n], out["m"][n], out["v"][n] = p.cpu(), mv[0].view(p.shape).cpu(), mv[1].view(p.shape).cpu()
    return out


@pytest.mark.parametrize("Z,K,F,C,k,B", R.ROW_CASES)
def test_iaf_reduce_and_step_vs_fp64(Z, K, F, C, k, B):
    ml, flow, wn, dzdec = row_inputs(Z, K, F, C, k, B)
    seed, step, lr, wd = 9, 5, 1e-3, 1e-5
    tag = "reduce Z=%d K=%d F=%d C=%d k=%d B=%d" % (Z, K, F, C, k, B)
    eps = ops_fused.iwae_normals(B, k, Z, seed, step, giwae.TAG_TRAIN).cpu().double().numpy()   # the device's own
    ref = R.rows_reference(ml, eps, flow, k, wn=wn, dzdec=dzdec)
    f32 = R.rows_reference(ml, eps, flow, k, torch.float32, wn=wn, dzdec=dzdec)
    conditioned(tag, ref)
    got = _reduce_step(ml, flow, wn, dzdec, Z, K, F, C, k, B, seed, step, lr, wd)
    names = R.flow_keys(C)
    check(tag, "dml[mu|lv]", got["dml"][:, :2 * Z].numpy(), ref["dml"][:, :2 * Z], f32["dml"][:, :2 * Z])
    if C:
        check(tag, "dml[dh]", got["dml"][:, 2 * Z:].numpy(), ref["dml"][:, 2 * Z:], f32["dml"][:, 2 * Z:])
    for n in names:
        check(tag, n, got[n].numpy(), ref[n], f32[n])
    M1, M2 = R.masks(Z, F, K)
    # one Adam step on those gradients is FlatAdam's, bit for bit (the same schedule, the same arithmetic)
    ps = [torch.nn.Parameter(dev32(flow[n])) for n in names]
    for p, n in zip(ps, names):
        p.grad = got[n].to(DEV).reshape(p.shape)
    opt = trainers.FlatAdam(ps, lr, weight_decay=wd)
    opt.step()
    torch.cuda.synchronize()
    P0 = {n: flow[n] for n in names}
    zero = {n: np.zeros_like(flow[n]) for n in names}
    Pr, Mr, Vr = R.adam_reference(P0, {n: ref[n] for n in names}, zero, zero, 1, lr, wd)
    P32, M32, V32 = R.adam_reference(P0, {n: f32[n] for n in names}, zero, zero, 1, lr, wd)
    for i, (p, o, n) in enumerate(zip(ps, opt.offs, names)):
        c = p.numel()
        assert torch.equal(got["p"][n].reshape(-1), p.detach().cpu().reshape(-1)), n
        assert not torch.equal(got["p"][n].reshape(-1), dev32(flow[n]).cpu().reshape(-1))            # and it moved
        assert torch.equal(got["m"][n].reshape(-1), opt.m[o:o + c].cpu()), n
        assert torch.equal(got["v"][n].reshape(-1), opt.v[o:o + c].cpu()), n
        # the stepped state against Adam on the fp64 gradients
        check(tag, n + " stepped", got["p"][n].numpy(), Pr[n], P32[n])
        check(tag, n + " m", got["m"][n].numpy(), Mr[n], M32[n])
        check(tag, n + " v", got["v"][n].numpy(), Vr[n], V32[n])
    for n, M in (("flow.W1", M1), ("flow.W2", M2)):                      # masked entries and their moments: exactly 0.0
        for what in (got[n], got["p"][n], got["m"][n], got["v"][n]):
            assert not what.numpy()[~M].any(), n
    # run to run: the same bits
    again = _reduce_step(ml, flow, wn, dzdec, Z, K, F, C, k, B, seed, step, lr, wd)
    assert torch.equal(again["dml"], got["dml"])
    for n in names:
        assert torch.equal(again[n], got[n]), n
        for w in ("p", "m", "v"):
            assert torch.equal(again[w][n], got[w][n]), (w, n)


def test_iaf_reduce_does_not_depend_on_where_a_row_lands():
    """test_gpu_nfvae.py's construction.  The noise row is the batch position, so the same image at another position
    draws another eps.  With lv = -200 the standard deviation is 0 in fp32 and z_0 = mu whatever eps: then rotating the
    batch by 3 images moves every image to other lanes and most to another workgroup, and d loss / d [mu | lv | h] of each
    image must keep its bits; the flow's gradients are the same sums in another order."""
    Z, K, F, C, k, B = R.ROW_CASES[2]
    ml, flow, wn, dzdec = row_inputs(Z, K, F, C, k, B)
    ml[:, Z:2 * Z] = -200.0
    a = _reduce_step(ml, flow, wn, dzdec, Z, K, F, C, k, B, 9, 5)
    sh = 3
    rot = lambda t, rows: torch.roll(t.reshape(B, rows, -1), sh, 0).reshape(t.shape)
    b = _reduce_step(torch.roll(ml, sh, 0), flow, rot(wn, k), rot(dzdec, k), Z, K, F, C, k, B, 9, 5)
    assert torch.equal(torch.roll(a["dml"], sh, 0), b["dml"])
    assert torch.all(a["dml"][:, Z:2 * Z] == -0.5) and a["dml"][:, 2 * Z:].abs().max() > 0
    eps = np.zeros((B * k, Z))
    ref = R.rows_reference(ml, eps, flow, k, wn=wn, dzdec=dzdec)
    f32 = R.rows_reference(ml, eps, flow, k, torch.float32, wn=wn, dzdec=dzdec)
    conditioned("rotated", ref)
    for n in R.flow_keys(C):
        check("rotated", n, b[n].numpy(), ref[n], f32[n])
        check("unrotated", n, a[n].numpy(), ref[n], f32[n])


# ---- the engine against fp64 training -----------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, I, seed=7):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


def make_model(I, H, Z, K, F, C, seed=1234):
    torch.manual_seed(seed)
    m = iaf_vae.IAFVAE(I, H, Z, K, F, C)
    f = R.flow_params(K, Z, F, C, seed=K + Z + R.FLOW_SEED)
    with torch.no_grad():
        for n in R.flow_keys(C):
            getattr(m.flow, n.split(".")[1]).copy_(torch.as_tensor(f[n], dtype=torch.float32))
    return m, {n: v.detach().clone().double().numpy() for n, v in m.state_dict().items() if n != "flow.m_in"}


def engine_views(tr, what):
    """{state_dict name: tensor} of the engine's flat gradient buffer or moments."""
    fp = tr._engine.fp
    out = {}
    for n, p in tr.model.named_parameters():
        i = [j for j, q in enumerate(fp.params) if q is p][0]
        o = fp.offsets[i]
        out[n] = getattr(fp, what)[o:o + p.numel()].view(p.shape).cpu()
    return out


def masked_zero(tag, tensors, Z, K, F):
    M1, M2 = R.masks(Z, F, K)
    for n, M in (("flow.W1", M1), ("flow.W2", M2)):
        assert not np.asarray(tensors[n])[~M].any(), (tag, n)


@pytest.mark.parametrize("I,H,Z,K,F,C,k", [(49, 32, 5, 3, 12, 4, 1), (49, 32, 5, 3, 12, 4, 3), (49, 32, 5, 3, 12, 0, 3)])
def test_engine_vs_fp64_training(I, H, Z, K, F, C, k):
    """One epoch on the fused engine (6 batches of 16 with a ragged last one of 9) against Adam on the fp64 reference's
    gradients, batch by batch on the device's own eps: losses, ess, every parameter.  The fp32 yardstick is the same loop
    with float32 arithmetic and float32 parameters and moments."""
    batch, n_train = 16, 89
    its = loaders(batch, n_train, batch, 16, I)
    m, P = make_model(I, H, Z, K, F, C)
    tr = iaf_vae.IAFVAETrainer(m, *its, k=k, seed=3)
    st = torch.get_rng_state()
    quiet(tr.train, 1)
    cfg = tr._engine.run_config
    assert type(tr._engine).__name__ == "IAFVAEEngine"
    assert (cfg["num_flows"], cfg["flow_hidden"], cfg["context_dim"]) == (K, F, C)
    nb = (n_train + batch - 1) // batch
    assert len(tr.losses) == len(tr.ess) == nb and tr.noise_steps == nb
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].double().numpy()
    batches = [x[i:i + batch] for i in range(0, n_train, batch)]
    eps_of = lambda t, b: ops_fused.iwae_normals(b, k, Z, 3, t, giwae.TAG_TRAIN).cpu().double().numpy()
    Pr, Lr, Er = R.train_reference(P, batches, eps_of, k, 1e-3, 1e-5)
    P32, L32, E32 = R.train_reference(P, batches, eps_of, k, 1e-3, 1e-5, torch.float32)
    tag = "engine %s K=%d F=%d C=%d k=%d" % ((I, H, Z), K, F, C, k)
    conditioned(tag + " first batch", R.model_reference(P, batches[0], eps_of(0, batches[0].shape[0]), k))
    conditioned(tag + " last batch", R.model_reference(Pr, batches[-1], eps_of(nb - 1, batches[-1].shape[0]), k))
    for t in range(nb):
        for name, got, ref, f32 in (("loss", tr.losses, Lr, L32), ("ess", tr.ess, Er, E32)):
            check(tag, "%s[%d]" % (name, t), got[t], ref[t], f32[t], T_LOSS)
    got = {n: v.detach().cpu().double().numpy() for n, v in m.state_dict().items()}
    for n in R.enc_dec(C):                                                # test_gpu_iwae.py's absolute weight bound
        err, tol = np.abs(got[n] - Pr[n]).max(), max(T_PARAM, 4 * np.abs(P32[n] - Pr[n]).max())
        print("%s %s: err %.3g allowed %.3g" % (tag, n, err, tol))
        assert err <= tol, (n, err, tol)
    for n in R.flow_keys(C):
        assert np.abs(Pr[n] - P[n]).max() > 1e-4                          # the flow trained
        check(tag, n, got[n], Pr[n], P32[n])
    masked_zero(tag, got, Z, K, F)
    masked_zero(tag + " m", {n: v.numpy() for n, v in engine_views(tr, "m").items()}, Z, K, F)
    masked_zero(tag + " v", {n: v.numpy() for n, v in engine_views(tr, "v").items()}, Z, K, F)


def test_one_fused_batch_gradients_vs_fp64():
    """One batch with Adam's lr = 0 (the parameters stay, the gradients land in the flat gradient buffer): loss, ess and
    every gradient against autograd on the fp64 reference."""
    I, H, Z, K, F, C, k, b = 130, 24, 6, 3, 16, 5, 4, 17
    its = loaders(b, b, b, 16, I)
    m, P = make_model(I, H, Z, K, F, C)
    tr = iaf_vae.IAFVAETrainer(m, *its, k=k, seed=3)
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
    for n, v in m.state_dict().items():
        if n != "flow.m_in":
            assert np.array_equal(v.cpu().double().numpy(), P[n]), n      # lr = 0: nothing moved
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    eps = ops_fused.iwae_normals(b, k, Z, 3, 0, giwae.TAG_TRAIN).cpu().double().numpy()
    ref, f32 = R.model_reference(P, x, eps, k), R.model_reference(P, x, eps, k, torch.float32)
    conditioned("batch", ref)
    check("batch", "loss", tr.losses[0], -ref["L"].sum(), -f32["L"].sum(), T_LOSS)
    check("batch", "ess", tr.ess[0], ref["ess"].mean(), f32["ess"].mean(), T_LOSS)
    got = engine_views(tr, "grad")
    assert sorted(got) == sorted(R.keys(C))
    for n in R.keys(C):
        check("batch", n, got[n].numpy(), ref["grads"][n], f32["grads"][n])
    masked_zero("batch", {n: v.numpy() for n, v in got.items()}, Z, K, F)


# ---- determinism ----------------------------------------------------------------------------------------------------------
SMALL = dict(I=64, H=48, Z=8, K=3, F=16, C=6)


def _trained_small(k=3, seed=0, epochs=1, cls=None, use_graph=True, n_train=96, batch=32, its=None, **kw):
    s = dict(SMALL, **kw)
    its = its or loaders(batch, n_train, 48, 48, s["I"])
    m, _ = make_model(s["I"], s["H"], s["Z"], s["K"], s["F"], s["C"])
    tr = (cls or iaf_vae.IAFVAETrainer)(m, *its, k=k, seed=seed)
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
    new = lambda: iaf_vae.IAFVAE(SMALL["I"], SMALL["H"], SMALL["Z"], SMALL["K"], SMALL["F"], SMALL["C"]).to(DEV)
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
    c = ck["optim"]["config"]
    assert (c["num_flows"], c["flow_hidden"], c["context_dim"], c["k"]) == (SMALL["K"], SMALL["F"], SMALL["C"], 3)
    assert ck["history"]["noise_steps"] == 10 and "flow.W1" in ck["model"] and "flow.m_in" in ck["model"]
    m2 = new()
    tr2 = iaf_vae.IAFVAETrainer(m2, *its, k=3, seed=0)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 10 and tr2.losses == runs[0][0][:10]
    quiet(tr2.train, 1)
    same(snapshot(tr2, m2), runs[0])
    # other settings: refused under strict before any state changes, taken otherwise
    ck["optim"]["config"]["flow_hidden"] = 12
    other = str(tmp_path / "ck12.pt")
    torch.save(ck, other)
    for p, kw in ((other, dict(k=3, seed=0)), (path, dict(k=2, seed=0)), (path, dict(k=3, seed=1))):
        m3 = new()
        t3 = iaf_vae.IAFVAETrainer(m3, *its, **kw)
        t3.load_checkpoint(p)
        before = {n: v.cpu().clone() for n, v in m3.state_dict().items()}
        with pytest.raises(GMError):
            t3.train(1)
        for n, v in m3.state_dict().items():
            assert torch.equal(v.cpu(), before[n]), n
        assert t3.noise_steps == 10
    t3 = iaf_vae.IAFVAETrainer(new(), *its, k=3, seed=0)
    t3.load_checkpoint(other, strict=False)
    quiet(t3.train, 1)


# ---- paths ------------------------------------------------------------------------------------------------------------------
class Mine(iaf_vae.IAFVAETrainer):
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
    for cls in (iaf_vae.IAFVAETrainer, Mine):
        torch.manual_seed(99)
        tr, m, _ = _trained_small(cls=cls, n_train=96, batch=32)          # 3 batches
        assert (tr._engine is None) == (cls is Mine) and len(tr.losses) == 3 and tr.noise_steps == 3
        out.append((tr, {k: v.cpu() for k, v in m.state_dict().items()}))
    (a, wa), (b, wb) = out
    assert len(made) == 1
    for n in wa:
        err = (wa[n].double() - wb[n].double()).abs().max().item()
        print("general path %s: %.3g" % (n, err))
        assert err <= T_PARAM, n
    masked_zero("general path", {n: v.numpy() for n, v in wb.items()}, SMALL["Z"], SMALL["K"], SMALL["F"])
    for u, v in zip(a.losses + a.ess + [a.best_val_loss], b.losses + b.ess + [b.best_val_loss]):
        assert abs(u - v) <= 1e-4 * max(1.0, abs(v)), (u, v)
    opt = made[0]
    for what, flat in (("m", opt.m), ("v", opt.v)):
        fused = engine_views(a, what)
        for (n, p), o in zip(b.model.named_parameters(), opt.offs):
            err = scaled_err(flat[o:o + p.numel()].cpu().numpy(), fused[n].reshape(-1).numpy())
            print("general path %s of %s: %.3g" % (what, n, err))
            assert err <= 1e-4, (what, n, err)
    # sizes outside the fused limits (K = 9; F = 6 is no multiple of 4): the general path, same interface
    for kw in (dict(K=9), dict(F=6)):
        torch.manual_seed(99)
        tr, m, _ = _trained_small(n_train=64, batch=32, **kw)
        assert tr._engine is None and len(tr.losses) == 2 and all(math.isfinite(v) for v in tr.losses + tr.ess)


# ---- log_likelihood and posterior_samples ------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [5, 0])
def test_log_likelihood_and_posterior_samples(C):
    I, H, Z, K, F, n, k = 130, 24, 6, 3, 16, 17, 130         # 130 samples: chunks of 64, 64 and 2
    its = loaders(16, 32, 16, n, I)
    m, P = make_model(I, H, Z, K, F, C)
    tr = iaf_vae.IAFVAETrainer(m, *its, k=1, seed=0)
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
    conditioned("log_likelihood", ref)
    ll = ref["L"] - 0.5 * I * math.log(math.pi)
    tol = allowance(T_LOSS, ref["L"], f32["L"]) * np.abs(ref["L"]).max()
    print("log_likelihood: mean %.6f ref %.6f allowed %.3g" % (res.ll_mean, ll.mean(), tol))
    assert abs(res.ll_mean - ll.mean()) <= tol
    assert abs(res.ll_stderr - ll.std() / math.sqrt(n)) <= tol
    assert tr.log_likelihood(x, k=k, seed=1) == res                        # bitwise: same seed, explicit images
    assert tr.log_likelihood(x, k=k, seed=2).ll_mean != res.ll_mean
    if C:
        # an encoder with a context layer is not vae.py's any more: iwae.log_likelihood refuses it
        with pytest.raises(GMError):
            giwae.log_likelihood(tr, x, k, 1)
    else:
        # the trap: iwae.log_likelihood takes this model and scores it with the flow left out of q
        wrong = giwae.log_likelihood(tr, x, k, 1)
        print("log_likelihood: trainer %.6f, iwae.log_likelihood on the same model %.6f" % (res.ll_mean, wrong.ll_mean))
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
    """The 16 band patterns tests/test_gpu_made.py learns on (16 x 16 images, two adjacent rows or columns lit): the
    validation loss after training is below the fresh model's."""
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
    tr = iaf_vae.IAFVAETrainer(iaf_vae.IAFVAE(256, 128, 8, 2, 16, 8), *its, k=1, seed=0)
    tr.model.eval()
    fresh = float(tr.evaluate(its[1]))                                    # the general path's evaluation of the fresh model
    quiet(tr.train, 5)
    assert type(tr._engine).__name__ == "IAFVAEEngine"
    assert len(tr.losses) == 80 and all(math.isfinite(v) for v in tr.losses + tr.ess)
    print("learning: fresh validation loss %.3f, after training %.3f (best %.3f)" % (fresh, tr.evaluate(its[1]),
                                                                                     tr.best_val_loss))
    assert tr.best_val_loss < fresh and float(tr.evaluate(its[1])) < fresh
