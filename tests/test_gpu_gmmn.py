"""The GMMN on the MI355X: the MMD kernels (gm_mmd_pairs / gm_mmd_finalize / gm_mmd_grad with C R through the GEMM
kernels), the prior, GMMNEngine, the general path, metrics.mmd and the trainers' mmd().

Bounds: test_gpu_tcvae.py's rule -- an error, in units of the reference tensor's max-abs, may be 4 x the deviation of the
float32 CPU run of gmmn_reference.py's Gram form (`mmd_gram`) from the fp64 direct-difference reference, and at least the
bases 1e-5 (loss sums), 1.5e-6 (gradients), 5e-5 (weights, absolute).  Every error is printed beside its allowance."""
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

import gmmn  # noqa: E402
import gmmn_reference as R  # noqa: E402
from generative_models_amd import gmmn as ggmmn  # noqa: E402
from generative_models_amd import metrics, ops, ops_fused, trainers  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
T_LOSS, T_GRAD, T_PARAM = 1e-5, 1.5e-6, 5e-5              # test_gpu_tcvae.py's bases
# (N, M, I): one pair; I below a k-stage and no multiple of 4; across the 32-row MFMA tile with a ragged k; the
# workload's row length over three partner chunks; one row past the kernel's 256-row block (and past a 128-partner chunk)
CASES = [(1, 1, 1), (5, 7, 3), (33, 31, 50), (65, 130, 784), (257, 130, 24)]
REGIMES = ("spread", "collapsed")


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        out = fn(*a, **kw)
    torch.cuda.synchronize()
    return out


def scaled_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)


def check(tag, name, got, ref, f32, base=T_GRAD):
    """test_gpu_tcvae.py's check: max(base, 4 x the fp32 CPU run's deviation), in units of the tensor's max-abs."""
    tol, err = max(base, 4.0 * scaled_err(f32, ref)), scaled_err(got, ref)
    print("%s %s: err %.3g allowed %.3g (fp32 cpu %.3g)" % (tag, name, err, tol, scaled_err(f32, ref)))
    assert err <= tol, (tag, name, err, tol)
    return err


def rows(N, M, I, regime):
    g = torch.Generator().manual_seed(7919 * N + 31 * M + I)
    Y = torch.rand(M, I, generator=g)
    if regime == "spread":
        X = torch.rand(N, I, generator=g)
    else:                                                   # mode collapse: one base row, and a data row equal to X[0]
        X = torch.rand(1, I, generator=g) + 1e-3 * torch.randn(N, I, generator=g)
        Y[0] = X[0]
    return X.contiguous(), Y.contiguous()


def case_sigmas(I):
    return [math.sqrt(I / 6.0) * f for f in (0.5, 1.0, 2.0)]


def strided(x, pad):
    """x's values in a device buffer whose rows are x.shape[1] + pad apart."""
    buf = torch.full((x.shape[0], x.shape[1] + pad), 7.0, device=DEV)
    buf[:, :x.shape[1]] = x.to(DEV)
    return buf[:, :x.shape[1]]


def run_kernels(X, Y, sigmas, sqrt_loss=True, ldc_pad=4, pads=(3, 5)):
    """pairs + finalize + C R + grad on the device; X and Y at leading dimensions of their own, C's rows T rounded up to
    4, + ldc_pad apart (a pad that is no multiple of 4 takes the element-wise stores)."""
    N, M, I = X.shape[0], Y.shape[0], X.shape[1]
    T = N + M
    Xd, Yd = strided(X, pads[0]), strided(Y, pads[1])
    sig = ops_fused.mmd_sigmas(sigmas, DEV)
    ws = ops_fused.mmd_workspace(N, M, True, DEV)
    Cb = torch.full((N, (T + 3) // 4 * 4 + ldc_pad), 9.0, device=DEV)
    stats = torch.zeros(10, dtype=torch.float64, device=DEV)
    r, loss = torch.zeros(N, device=DEV), torch.zeros(1, device=DEV)
    Rc = torch.full((T + 1, I), 5.0, device=DEV)
    ops_fused.mmd_pairs(Xd, Yd, sig, ws, C=Cb, Rc=Rc)
    ops_fused.mmd_finalize(N, M, len(sigmas), sqrt_loss, ws, stats, r=r, loss_out=loss)
    P, dA = torch.zeros(N, I, device=DEV), strided(torch.zeros(N, I), 2)
    ops.linear_bwd_dx(Cb[:, :T], Rc[:T], P, M=N)
    ops_fused.mmd_grad(Xd, P, r, stats, dA, sigmoid=True, mu=Xd[:1])
    torch.cuda.synchronize()
    assert torch.equal(Rc[:T].cpu(), torch.cat([X, Y], 0) - X[:1]) and bool((Rc[T] == 5.0).all())
    assert bool((Cb[:, T:] == 9.0).all()) and bool((Xd.as_strided((N, pads[0]), Xd.stride(), I) == 7.0).all())
    st = stats.cpu().numpy()
    return {"mmd2": st[0], "loss": st[1], "inv": st[2], "sxx": st[3], "sxy": st[4], "syy": st[5], "sxx_off": st[6],
            "syy_off": st[7], "dxx": st[8], "dyy": st[9], "loss32": float(loss.item()), "r": r.cpu().numpy(),
            "C": Cb[:, :T].cpu().numpy(), "dA": dA.cpu().numpy()}


def compare(tag, got, ref, f32, S, N, M):
    for name in ("mmd2", "loss", "sxx_off", "syy_off", "sxy"):
        check(tag, name, got[name], float(ref[name]), float(f32[name]), T_LOSS)
    for name in ("r", "C", "dA"):
        check(tag, name, got[name], ref[name].numpy(), f32[name].numpy())
    for v in got.values():
        assert np.all(np.isfinite(v)), tag
    # a row against itself has d^2 = 0 exactly: its kernel value is the number of bandwidths, bit for bit
    assert got["dxx"] == float(N * S) and got["dyy"] == float(M * S), (tag, got["dxx"], got["dyy"])
    assert got["loss32"] == float(np.float32(got["loss"]))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("N,M,I", CASES)
def test_mmd_kernels_vs_fp64(N, M, I, regime):
    """Every output of the three MMD launches and the GEMM between them against the fp64 direct-difference reference, at
    leading dimensions of their own, with C stored four at a time and element by element.  Measured on an MI355X (worst
    over the cases, in units of max-abs): spread -- mmd2 7.6e-7, C 7.3e-7 of 1.5e-6, r 2.6e-6 of
    1.35e-5, dA 1.3e-6; collapsed -- mmd2 4.1e-8, C 1.8e-7, r 9.9e-8, dA 3.2e-7 where the fp32 CPU run deviates by 9.7e-6,
    and exactly 0 at (1, 1, 1).  No wider bound than the rule's was needed in the collapsed regime."""
    X, Y = rows(N, M, I, regime)
    sig = case_sigmas(I)
    ref, f32 = R.mmd_reference(X, Y, sig), R.mmd_gram(X, Y, sig)
    share = ref["xy_share"].numpy()
    print("xy shares", share)
    assert share.min() >= 0.05                              # every bandwidth matters on these inputs
    tag = "%s %s" % ((N, M, I), regime)
    got = run_kernels(X, Y, sig)
    compare(tag, got, ref, f32, len(sig), N, M)
    if N == 1:
        assert got["sxx"] == float(len(sig))
    got2 = run_kernels(X, Y, sig, ldc_pad=1, pads=(0, 1))   # element-wise C stores; the same numbers
    for k in got:
        assert np.array_equal(got[k], got2[k]), (tag, k)
    got3 = run_kernels(X, Y, sig, sqrt_loss=False)
    assert got3["mmd2"] == got["mmd2"] and got3["loss"] == got["mmd2"] and got3["inv"] == 1.0
    ref3, f323 = R.mmd_reference(X, Y, sig, False), R.mmd_gram(X, Y, sig, False)
    check(tag, "dA (mmd2)", got3["dA"], ref3["dA"].numpy(), f323["dA"].numpy())


def test_mmd_kernels_default_bandwidths():
    N, M, I = 65, 130, 784
    for regime in REGIMES:
        X, Y = rows(N, M, I, regime)
        sig = list(ggmmn.SIGMAS)
        assert sig == [2.0, 5.0, 10.0, 20.0, 40.0, 80.0]
        compare("default sigmas %s" % regime, run_kernels(X, Y, sig), R.mmd_reference(X, Y, sig), R.mmd_gram(X, Y, sig),
                6, N, M)


# ---- the prior ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,Z", [(1, 1), (5, 7), (33, 20), (3, 130)])
def test_prior_is_philox_bit_for_bit(n, Z):
    for seed, step, tag, row0 in ((0, 0, ggmmn.TAG_T, 0), (2 ** 40 + 5, 7, ggmmn.TAG_V, 0), (9, 0, ggmmn.TAG_S, 1000)):
        z = strided(torch.zeros(n, Z), 3)
        ops_fused.gmmn_prior(z, ops_fused.gmmn_noise(seed, tag, step=step, row0=row0))
        want = ggmmn.uniforms_reference(n, Z, seed, step, tag, row0)
        assert np.array_equal(z.cpu().numpy(), want) and np.abs(want).max() < 1.0
    # the step as device words: ctr + base + add
    ctr = torch.tensor([3], dtype=torch.int64, device=DEV)
    base = torch.tensor([40], dtype=torch.int64, device=DEV)
    z = torch.zeros(n, Z, device=DEV)
    ops_fused.gmmn_prior(z, ops_fused.gmmn_noise(1, ggmmn.TAG_T, step=2, step_ctr=ctr, step_base=base))
    assert np.array_equal(z.cpu().numpy(), ggmmn.uniforms_reference(n, Z, 1, 45, ggmmn.TAG_T))


# ---- the engine against fp64 training -------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, I, seed=7, binary=True):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g) if binary else torch.rand(n, I, generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


def make_model(I, H, Z, seed=1234):
    torch.manual_seed(seed)
    m = gmmn.GMMN(I, H, Z)
    return m, {n: v.detach().clone().double().numpy() for n, v in m.state_dict().items()}


def engine_views(tr, what):
    fp = tr._engine.fp
    out = {}
    for n, p in tr.model.named_parameters():
        i = [j for j, q in enumerate(fp.params) if q is p][0]
        o = fp.offsets[i]
        out[n] = getattr(fp, what)[o:o + p.numel()].view(p.shape).cpu()
    return out


def z_of(seed, tag, Z):
    return lambda t, b: ggmmn.uniforms_reference(b, Z, seed, t, tag).astype(np.float64)


@pytest.mark.parametrize("I,H,Z,batch,n_train,sqrt_loss", [(12, 16, 5, 7, 39, True), (12, 16, 5, 7, 39, False),
                                                           (784, 400, 20, 64, 357, True)])
def test_engine_vs_fp64_training(I, H, Z, batch, n_train, sqrt_loss):
    """One epoch on the fused engine (five full batches and a ragged sixth) against Adam on the fp64 reference's
    gradients, batch by batch on the device's own prior rows: the losses and every parameter; then the validation pass on
    the validation stream.  The fp32 yardstick is the same loop in float32 on the kernels' Gram form."""
    n_val = 2 * batch + 3
    its = loaders(batch, n_train, n_val, 16, I, binary=I == 784)
    sig = None if I == 784 else case_sigmas(I)
    m, P = make_model(I, H, Z)
    tr = gmmn.GMMNTrainer(m, *its, sigmas=sig, sqrt_loss=sqrt_loss, seed=3)
    sigmas = list(tr.sigmas)
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=1e-3, weight_decay=1e-5)
    assert type(tr._engine).__name__ == "GMMNEngine"
    nb = (n_train + batch - 1) // batch
    assert nb == 6 and len(tr.losses) == nb and tr.noise_steps == nb
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    xv = its[1].dataset.tensors[0][trainers._epoch_order(its[1])].double().numpy()
    batches = [x[i:i + batch] for i in range(0, n_train, batch)]
    zt = z_of(3, ggmmn.TAG_T, Z)
    Pr, Lr = R.train_reference(P, batches, zt, sigmas, sqrt_loss, 1e-3, 1e-5)
    P32, L32 = R.train_reference(P, batches, zt, sigmas, sqrt_loss, 1e-3, 1e-5, torch.float32)
    tag = "engine %s bs=%d sqrt=%s" % ((I, H, Z), batch, sqrt_loss)
    for t in range(nb):
        check(tag, "loss[%d]" % t, tr.losses[t], Lr[t], L32[t], T_LOSS)
    got = {n: v.detach().cpu().double().numpy() for n, v in m.state_dict().items()}
    for n in R.KEYS:
        err, tol = np.abs(got[n] - Pr[n]).max(), max(T_PARAM, 4 * np.abs(P32[n] - Pr[n]).max())
        print("%s %s: err %.3g allowed %.3g" % (tag, n, err, tol))
        assert err <= tol, (n, err, tol)
        assert np.abs(Pr[n] - P[n]).max() > 1e-4                          # and it trained
    zv = z_of(3, ggmmn.TAG_V, Z)
    vb = [xv[i:i + batch] for i in range(0, n_val, batch)]
    val = lambda dt: float(np.mean([R.model_reference(got, zv(t, len(b_)), b_, sigmas, sqrt_loss, dt)["loss"]
                                    for t, b_ in enumerate(vb)]))
    check(tag, "val loss", tr.best_val_loss, val(torch.float64), val(torch.float32), T_LOSS)


def test_one_full_size_fused_batch_gradients_vs_fp64():
    """One 784-400-20 batch of 512 with Adam's lr = 0 (the parameters stay, the gradients land in the flat gradient
    buffer): the loss and the four weight gradients against the fp64 reference."""
    I, H, Z, b = 784, 400, 20, 512
    its = loaders(b, b, b, 16, I)
    m, P = make_model(I, H, Z)
    tr = gmmn.GMMNTrainer(m, *its, seed=3)
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
    for n, v in m.state_dict().items():
        assert np.array_equal(v.cpu().double().numpy(), P[n]), n          # lr = 0: nothing moved
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    z = ggmmn.uniforms_reference(b, Z, 3, 0, ggmmn.TAG_T).astype(np.float64)
    ref = R.model_reference(P, z, x, tr.sigmas)
    f32 = R.model_reference(P, z, x, tr.sigmas, dtype=torch.float32)
    check("batch", "loss", tr.losses[0], ref["loss"], f32["loss"], T_LOSS)
    got = engine_views(tr, "grad")
    assert sorted(got) == sorted(R.KEYS)
    for n in R.KEYS:
        check("batch", n, got[n].numpy(), ref["grads"][n], f32["grads"][n])


# ---- determinism ----------------------------------------------------------------------------------------------------
def _trained_small(epochs=1, cls=None, use_graph=True, n_train=96, I=64, H=48, Z=8, batch=32, its=None, **kw):
    its = its or loaders(batch, n_train, 48, 48, I)
    m, _ = make_model(I, H, Z)
    kw.setdefault("sigmas", case_sigmas(I))
    tr = (cls or gmmn.GMMNTrainer)(m, *its, **kw)
    tr.use_graph = use_graph
    quiet(tr.train, epochs)
    return tr, m, its


def snapshot(tr, m):
    return (list(tr.losses), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state())


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    assert torch.equal(a[3], b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_bitwise_reproducibility_graph_eager_and_resume(tmp_path):
    cfg = dict(n_train=300, batch=64)                       # 300 rows, bs 64: four full batches and one of 44
    runs = []
    for use_graph in (True, True, False):                   # graph twice, then eager
        torch.manual_seed(99)
        tr, m, _ = _trained_small(epochs=2, use_graph=use_graph, **cfg)
        runs.append(snapshot(tr, m))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    assert len(runs[0][0]) == 10 and all(math.isfinite(v) for v in runs[0][0])
    # 1 epoch + checkpoint + a fresh trainer's resumed epoch == 2 epochs
    torch.manual_seed(99)
    tr, m, its = _trained_small(epochs=1, **cfg)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    conf = ck["optim"]["config"]
    assert tuple(conf["sigmas"]) == tuple(case_sigmas(64)) and conf["sqrt_loss"] is True and conf["seed"] == 0
    assert ck["history"]["noise_steps"] == 5 and len(ck["history"]["losses"]) == 5
    sig = case_sigmas(64)
    m2 = gmmn.GMMN(64, 48, 8).to(DEV)
    tr2 = gmmn.GMMNTrainer(m2, *its, sigmas=sig)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 5 and tr2.losses == runs[0][0][:5]
    quiet(tr2.train, 1)
    same(snapshot(tr2, m2), runs[0])
    # other settings: refused under strict, taken otherwise
    for kw in (dict(sigmas=sig[:2]), dict(sigmas=sig, sqrt_loss=False), dict(sigmas=sig, seed=1)):
        t3 = gmmn.GMMNTrainer(gmmn.GMMN(64, 48, 8).to(DEV), *its, **kw)
        t3.load_checkpoint(path)
        with pytest.raises(GMError, match="different settings"):
            t3.train(1)
    t3 = gmmn.GMMNTrainer(gmmn.GMMN(64, 48, 8).to(DEV), *its, sigmas=sig[:2])
    t3.load_checkpoint(path, strict=False)
    quiet(t3.train, 1)


# ---- paths ----------------------------------------------------------------------------------------------------------
class Mine(gmmn.GMMNTrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_general_path_gradients_agree_with_the_fused_run():
    """One batch at lr = 0 on both paths (one ragged-free batch of 67 rows, both `sqrt_loss` settings): the fused engine's
    flat gradient buffer and autograd's .grad on the general path, each against the fp64 reference and against each other
    within the gradient bound (1.5e-6 of max-abs, or 4 x the fp32 CPU deviation); the two losses within the loss bound."""
    I, H, Z, b = 130, 24, 6, 67
    for sq in (True, False):
        grads, losses = {}, {}
        for cls in (gmmn.GMMNTrainer, Mine):
            its = loaders(b, b, b, 16, I, binary=False)
            m, P = make_model(I, H, Z)
            tr = cls(m, *its, sigmas=case_sigmas(I), sqrt_loss=sq, seed=3)
            torch.manual_seed(99)
            st = torch.get_rng_state()
            quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
            assert (tr._engine is None) == (cls is Mine) and len(tr.losses) == 1
            if cls is Mine:
                grads[cls] = {n: p.grad.detach().cpu().numpy() for n, p in m.named_parameters()}
            else:
                grads[cls] = {n: v.numpy() for n, v in engine_views(tr, "grad").items()}
            losses[cls] = tr.losses[0]
        torch.set_rng_state(st)
        x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
        z = ggmmn.uniforms_reference(b, Z, 3, 0, ggmmn.TAG_T).astype(np.float64)
        ref = R.model_reference(P, z, x, case_sigmas(I), sq)
        f32 = R.model_reference(P, z, x, case_sigmas(I), sq, dtype=torch.float32)
        tag = "paths sqrt=%s" % sq
        for cls, nm in ((gmmn.GMMNTrainer, "fused"), (Mine, "general")):
            check(tag, nm + " loss", losses[cls], ref["loss"], f32["loss"], T_LOSS)
            for n in R.KEYS:
                check(tag, "%s %s" % (nm, n), grads[cls][n], ref["grads"][n], f32["grads"][n])
        check(tag, "general loss vs fused", losses[Mine], losses[gmmn.GMMNTrainer], f32["loss"] - ref["loss"] +
              losses[gmmn.GMMNTrainer], T_LOSS)
        for n in R.KEYS:                                    # the two paths against each other, the same allowance
            check(tag, "general vs fused " + n, grads[Mine][n], grads[gmmn.GMMNTrainer][n],
                  grads[gmmn.GMMNTrainer][n] + (f32["grads"][n] - ref["grads"][n]))


def test_general_path_agrees_with_the_fused_run():
    """Three training batches and the validation pass on both paths: parameters within 5e-5 (the weight base), the loss
    histories and the validation loss within 1e-5 (the loss base)."""
    out = []
    for cls in (gmmn.GMMNTrainer, Mine):
        torch.manual_seed(99)
        tr, m, _ = _trained_small(cls=cls, n_train=96, batch=32)          # 3 batches
        assert (tr._engine is None) == (cls is Mine) and len(tr.losses) == 3 and tr.noise_steps == 3
        out.append((tr, {k: v.cpu() for k, v in m.state_dict().items()}))
    (a, wa), (b, wb) = out
    for n in wa:
        err = (wa[n] - wb[n]).abs().max().item()
        print("general path %s: %.3g" % (n, err))
        assert err <= T_PARAM, n
    for u, v in zip(a.losses + [a.best_val_loss], b.losses + [b.best_val_loss]):
        print("general path loss: %.9g fused %.9g" % (v, u))
        assert abs(u - v) <= T_LOSS * abs(v), (u, v)


def test_mmd_loss_function_gradient_and_refusals():
    X, Y = rows(33, 31, 50, "spread")
    sig = case_sigmas(50)
    for sq in (True, False):
        xs = X.to(DEV).requires_grad_(True)
        loss = ops_fused.mmd_loss(xs, Y.to(DEV), sig, sq)
        (3.0 * loss).backward()
        ref, f32 = R.mmd_reference(X, Y, sig, sq), R.mmd_gram(X, Y, sig, sq)
        check("mmd_loss", "loss", loss.item(), float(ref["loss"]), float(f32["loss"]), T_LOSS)
        check("mmd_loss", "dX", xs.grad.cpu().numpy(), 3.0 * ref["dX"].numpy(), 3.0 * f32["dX"].numpy())
    with pytest.raises(GMError, match="samples only"):
        ops_fused.mmd_loss(X.to(DEV), Y.to(DEV).requires_grad_(True), sig)
    with pytest.raises(GMError):
        ops_fused.mmd_loss(X, Y, sig)                       # host tensors: no CPU fallback


# ---- sampling and the score ---------------------------------------------------------------------------------------
def test_sample_is_reproducible_and_independent_of_n():
    tr, m, _ = _trained_small()
    st, mode = torch.get_rng_state(), m.training
    a, b, c, d = tr.sample(40, seed=5), tr.sample(40, seed=5), tr.sample(17, seed=5), tr.sample(40, seed=6)
    assert torch.equal(torch.get_rng_state(), st) and m.training == mode
    assert a.shape == (40, 64) and torch.equal(a, b) and not torch.equal(a, d)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    assert torch.equal(a[:17], c)                           # row r depends on (seed, r) alone: whole blocks, whatever n
    e = tr.sample(1030, seed=5)                             # past one block
    assert e.shape == (1030, 64) and torch.equal(e[:40], a) and torch.equal(e[1024:], tr.sample(1100, seed=5)[1024:1030])
    z = tr.prior(40, 0, ggmmn.TAG_S, seed=5)
    assert np.array_equal(z.cpu().numpy(), ggmmn.uniforms_reference(40, 8, 5, 0, ggmmn.TAG_S))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(gmmn.GMMNError):
            tr.sample(bad)
    res = tr.mmd(n_samples=40, seed=5)
    assert type(res).__name__ == "MMDResult" and (res.n_samples, res.n_data) == (40, 48) and math.isfinite(res.mmd2)
    assert type(tr.parzen(n_samples=40, n_val=48)).__name__ == "ParzenResult"


def test_metrics_mmd_vs_reference_and_ordering():
    N, M, I = 200, 300, 784
    X, Y = rows(N, M, I, "spread")
    X = (0.7 * X + 0.1).contiguous()                        # another distribution than Y's
    ref, f32 = R.mmd_reference(X, Y, metrics.MMD_SIGMAS, False), R.mmd_gram(X, Y, metrics.MMD_SIGMAS, False)
    b = metrics.mmd(X.to(DEV), Y.to(DEV), unbiased=False)
    u = metrics.mmd(X.to(DEV), Y.to(DEV))
    check("metrics.mmd", "biased", b.mmd2, float(ref["mmd2"]), float(f32["mmd2"]), T_LOSS)
    check("metrics.mmd", "unbiased", u.mmd2, R.unbiased_of(ref), R.unbiased_of(f32), T_LOSS)
    assert (u.n_samples, u.n_data) == (N, M) and u.mmd == math.sqrt(max(u.mmd2, 0.0)) and u.mmd2 < b.mmd2
    # one distribution against itself scores below a shifted copy
    g = torch.Generator().manual_seed(3)
    x = torch.rand(400, I, generator=g).to(DEV)
    same_d = metrics.mmd(x[:200], x[200:])
    shifted = metrics.mmd(x[:200], (x[200:] * 0.9 + 0.1).contiguous())
    print("mmd2 same %.3g shifted %.3g" % (same_d.mmd2, shifted.mmd2))
    assert same_d.mmd2 < shifted.mmd2 and abs(same_d.mmd2) < 0.1 * shifted.mmd2
    with pytest.raises(GMError):
        metrics.mmd(x[:1], x[1:])                           # the unbiased statistic needs two rows of each
    with pytest.raises(GMError):
        metrics.mmd(x[:5], x[5:10], sigmas=[1.0, 0.0])
    assert math.isfinite(metrics.mmd(x[:1], x[1:3], unbiased=False).mmd2)


def test_gan_trainer_mmd_on_an_untrained_nsgan():
    import ns_gan
    its = loaders(16, 64, 48, 48, 64)
    torch.manual_seed(1)
    tr = ns_gan.NSGANTrainer(ns_gan.NSGAN(image_size=64, hidden_dim=48, z_dim=8), *its)
    res = tr.mmd(n_samples=50, seed=2)
    assert type(res).__name__ == "MMDResult" and (res.n_samples, res.n_data) == (50, 48) and res.mmd2 > 0
    assert res == tr.mmd(n_samples=50, seed=2)
    # the generator's weights load into a GMMN
    g = gmmn.GMMN(64, 48, 8)
    missing = g.load_state_dict(tr.model.state_dict(), strict=False)
    assert not missing.missing_keys and all(k.startswith("D.") for k in missing.unexpected_keys)


# ---- learning check -------------------------------------------------------------------------------------------------
def test_learning_on_bands():
    """The 16 band patterns tests/test_gpu_nfvae.py learns on (16 x 16 images, two adjacent rows or columns lit): over 320
    batches of 64 the validation loss (evaluate() on the validation stream, taken before training and after every 5
    epochs) falls, and the unbiased mmd2 of 2 000 samples against the held-out rows is below the untrained generator's.
    Measured on an MI355X: training loss 1.471 (first 10 batches) -> 0.490 (last 10), validation loss 1.500, 0.956, 0.709, 0.560, 0.496,
    unbiased mmd2 2.216 untrained -> 0.177 trained."""
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
    tr = gmmn.GMMNTrainer(gmmn.GMMN(256, 128, 8), *its, seed=0)
    before = tr.mmd(n_samples=2000, seed=1)

    def val():
        tr.model.eval()
        return float(tr.evaluate(tr.val_iter))
    vals = [val()]
    for _ in range(4):
        quiet(tr.train, 5)
        vals.append(val())
    assert type(tr._engine).__name__ == "GMMNEngine"
    assert len(tr.losses) == 320 and all(math.isfinite(v) for v in tr.losses)
    after = tr.mmd(n_samples=2000, seed=1)
    first, last = np.mean(tr.losses[:10]), np.mean(tr.losses[-10:])
    print("learning: training loss first 10 %.4f last 10 %.4f; validation loss untrained and after 5 / 10 / 15 / 20 epochs "
          "%s; unbiased mmd2 untrained %.5f trained %.5f" % (first, last, " ".join("%.4f" % v for v in vals), before.mmd2,
                                                             after.mmd2))
    assert last < first and vals[-1] < vals[1] < vals[0] and after.mmd2 < before.mmd2
