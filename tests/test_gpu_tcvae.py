"""beta-TCVAE on the MI355X: the two pair kernels against the fp64 contract (tests/tcvae_reference.py) on the device's own
eps, their bitwise properties, the engine against fp64 training, determinism (graph against eager, resume), the general
path, decomposition / traverse / log_likelihood and a learning check.

Inputs.  Two regimes from a seeded generator: "isolated" (mu ~ N(0, 1), lv = 0.5 n - 1: each sample sits under its own
posterior, a_ii near 1) and "overlapping" (mu = 0.3 n, lv = 0.3 n: the posteriors cover each other).  In the overlapping
regime at B >= 7 the test asserts on the fp64 reference that the mean over rows of max_j a_ij is at most 0.5: otherwise
the off-diagonal sums would not be exercised.

Bounds.  tests/test_gpu_nfvae.py's `check`: 4 x the deviation of the same contract run in fp32 torch on the CPU from the
fp64 reference, floored at 1.5e-6 of the tensor's max-abs; for what tests/test_gpu_iwae.py bounds, its bases: 1e-5 (loss
sums), 1.5e-6 of max-abs (gradients), 5e-5 (weights).  Every comparison prints its error and its allowance."""
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

import tc_vae  # noqa: E402
import tcvae_reference as R  # noqa: E402
from generative_models_amd import ops_fused, trainers  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
T_LOSS, T_GRAD, T_PARAM = 1e-5, 1.5e-6, 5e-5             # test_gpu_iwae.py's bases (module docstring)
N_DATA = 60000
SHAPES = [(1, 2), (5, 7), (20, 65), (32, 130), (20, 512)]    # (Z, B): one lane of work, a ragged partner tail, a crossing
#                                                             of the wave boundary, the Z limit, the workload's own B
COEF, COEF2 = (1.0, 6.0, 1.0), (2.0, 0.5, 3.0)
ROW_CASES = [(Z, B, reg, COEF) for Z, B in SHAPES for reg in ("isolated", "overlapping")] + \
    [(20, 65, "overlapping", COEF2)]                       # once with both coefficient signs


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


def row_inputs(Z, B, regime):
    g = torch.Generator().manual_seed(1000 * Z + B)
    n = torch.randn(B, 2 * Z, generator=g)
    ml = 0.3 * n if regime == "overlapping" else torch.cat([n[:, :Z], 0.5 * n[:, Z:] - 1.0], 1)
    return ml.contiguous(), torch.randn(B, Z, generator=g)


def run_rows(ml, dzdec, coef, seed, step, Z, B, terms=True):
    noise = ops_fused.iwae_noise(seed, giwae.TAG_TRAIN, 1, step=step)
    f = lambda *s: torch.full(s, 7.0, device=DEV)
    mld = ml.to(DEV)
    z, lp, lsej, lsed, tc, tm, dml = f(B, Z), f(B), f(B), f(B, Z), f(B), f(B, 3), f(B, 2 * Z)
    ops_fused.tc_sample(mld, z, lp, lsej, lsed, tc, noise, *coef, math.log(N_DATA * B), B, Z,
                        terms=tm if terms else None)
    ops_fused.tc_reduce(mld, z, lsej, lsed, torch.ones(B, device=DEV), dzdec.to(DEV), dml, noise, *coef, B, Z)
    torch.cuda.synchronize()
    return {"z": z.cpu(), "lp": lp.cpu(), "lse_joint": lsej.cpu(), "lse_dim": lsed.cpu(), "tc": tc.cpu(),
            "terms": tm.cpu(), "dml": dml.cpu()}


# ---- the row kernels against the reference --------------------------------------------------------------------------
@pytest.mark.parametrize("Z,B,regime,coef", ROW_CASES)
def test_pair_kernels_vs_fp64(Z, B, regime, coef):
    ml, dzdec = row_inputs(Z, B, regime)
    seed, step = 0x123456789ABCDEF, 77
    tag = "rows Z=%d B=%d %s %s" % (Z, B, regime, coef)
    eps = ops_fused.iwae_normals(B, 1, Z, seed, step, giwae.TAG_TRAIN).cpu().double().numpy()     # the device's own
    L, wn = math.log(N_DATA * B), torch.ones(B)
    ref = R.rows_reference(ml, eps, coef, L, wn=wn, dzdec=dzdec)
    f32 = R.rows_reference(ml, eps, coef, L, torch.float32, wn=wn, dzdec=dzdec)
    print("%s: mean max_j a_ij %.3f" % (tag, ref["amax"]))
    if regime == "overlapping" and B >= 7:
        assert ref["amax"] <= 0.5
    got = run_rows(ml, dzdec, coef, seed, step, Z, B)
    for name in ("z", "lp", "terms", "lse_joint", "lse_dim", "dml"):
        check(tag, name, got[name].numpy(), ref[name], f32[name])
    assert torch.equal(got["tc"], got["terms"][:, 1])
    if Z == 1:                                            # one latent: no total correlation, to lp's allowance
        tol = allowance(T_GRAD, ref["lp"], f32["lp"]) * np.abs(ref["lp"]).max()
        print("%s tc: max |tc| %.3g allowed %.3g" % (tag, got["tc"].abs().max().item(), tol))
        assert got["tc"].abs().max().item() <= tol
    # run to run, and without the optional terms: the same bits
    again = run_rows(ml, dzdec, coef, seed, step, Z, B, terms=False)
    for name in ("z", "lp", "lse_joint", "lse_dim", "tc", "dml"):
        assert torch.equal(again[name], got[name]), name
    assert torch.all(again["terms"] == 7.0)


@pytest.mark.parametrize("Z,B", SHAPES)
@pytest.mark.parametrize("regime", ["isolated", "overlapping"])
def test_z_is_the_iwaes_bit_for_bit_and_unit_weights_give_its_lp(Z, B, regime):
    ml, dzdec = row_inputs(Z, B, regime)
    seed, step = 5, 3
    noise = ops_fused.iwae_noise(seed, giwae.TAG_TRAIN, 1, step=step)
    z_iw, lp_iw = torch.empty(B, Z, device=DEV), torch.empty(B, device=DEV)
    ops_fused.iwae_sample(ml.to(DEV), z_iw, lp_iw, noise, B, 1, Z)
    eps = ops_fused.iwae_normals(B, 1, Z, seed, step, giwae.TAG_TRAIN)
    got = run_rows(ml, dzdec, (1.0, 1.0, 1.0), seed, step, Z, B)
    assert torch.equal(got["z"], z_iw.cpu())
    mld = ml.to(DEV)
    zero = run_rows(torch.zeros(B, 2 * Z), dzdec, (1.0, 1.0, 1.0), seed, step, Z, B)
    assert torch.equal(zero["z"], eps.cpu())                # mu = 0, lv = 0: z = 0 + 1 eps, iwae_normals' stream
    e = eps.cpu().double().numpy()
    L = math.log(N_DATA * B)
    ref, f32 = R.rows_reference(ml, e, (1.0, 1.0, 1.0), L), R.rows_reference(ml, e, (1.0, 1.0, 1.0), L, torch.float32)
    tol = allowance(T_GRAD, ref["lp"], f32["lp"])
    err = scaled_err(got["lp"].numpy(), lp_iw.cpu().numpy())
    print("unit weights Z=%d B=%d %s: |lp - iwae lp| %.3g allowed %.3g" % (Z, B, regime, err, tol))
    assert err <= tol
    # and the backward is the IWAE's: the pair coefficients vanish
    dml_iw = torch.empty(B, 2 * Z, device=DEV)
    ops_fused.iwae_reduce(mld, torch.ones(B, device=DEV), dzdec.to(DEV), dml_iw, noise, B, 1, Z)
    refb = R.rows_reference(ml, e, (1.0, 1.0, 1.0), L, wn=torch.ones(B), dzdec=dzdec)
    f32b = R.rows_reference(ml, e, (1.0, 1.0, 1.0), L, torch.float32, wn=torch.ones(B), dzdec=dzdec)
    check("unit weights", "dml", got["dml"].numpy(), refb["dml"], f32b["dml"])
    check("unit weights", "iwae dml", dml_iw.cpu().numpy(), refb["dml"], f32b["dml"])


# ---- the engine against fp64 training -------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, I, seed=7):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


def make_model(I, H, Z, seed=1234):
    torch.manual_seed(seed)
    m = tc_vae.TCVAE(I, H, Z)
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


def eps_of(seed, tag, Z):
    return lambda t, b: ops_fused.iwae_normals(b, 1, Z, seed, t, tag).cpu().double().numpy()


@pytest.mark.parametrize("I,H,Z", [(12, 16, 5), (784, 400, 20)])
@pytest.mark.parametrize("batch,n_train", [(7, 39), (64, 357)])
def test_engine_vs_fp64_training(I, H, Z, batch, n_train):
    """One epoch on the fused engine (five full batches and a ragged sixth) against Adam on the fp64 reference's
    gradients, batch by batch on the device's own eps: losses, the tc history, every parameter; then the validation
    pass, whose N is the validation set's size.  The fp32 yardstick is the same loop with float32 arithmetic and
    float32 parameters and moments."""
    n_val = 2 * batch + 3
    its = loaders(batch, n_train, n_val, 16, I)
    m, P = make_model(I, H, Z)
    tr = tc_vae.TCVAETrainer(m, *its, seed=3)
    assert (tr.alpha, tr.beta, tr.gamma, tr.dataset_size) == (1.0, 6.0, 1.0, n_train)
    coef = (tr.alpha, tr.beta, tr.gamma)
    st = torch.get_rng_state()
    quiet(tr.train, 1)
    assert type(tr._engine).__name__ == "TCVAEEngine" and tr._engine.run_config["beta"] == 6.0
    nb = (n_train + batch - 1) // batch
    assert nb == 6 and len(tr.losses) == len(tr.tc) == nb and tr.noise_steps == nb
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    xv = its[1].dataset.tensors[0][trainers._epoch_order(its[1])].double().numpy()
    batches = [x[i:i + batch] for i in range(0, n_train, batch)]
    e_train = eps_of(3, giwae.TAG_TRAIN, Z)
    Pr, Lr, Tr, _ = R.train_reference(P, batches, e_train, coef, n_train, 1e-3, 1e-5)
    P32, L32, T32, _ = R.train_reference(P, batches, e_train, coef, n_train, 1e-3, 1e-5, torch.float32)
    tag = "engine %s bs=%d" % ((I, H, Z), batch)
    for t in range(nb):
        for name, got, ref, f32 in (("loss", tr.losses, Lr, L32), ("tc", tr.tc, Tr, T32)):
            check(tag, "%s[%d]" % (name, t), got[t], ref[t], f32[t], T_LOSS)
    got = {n: v.detach().cpu().double().numpy() for n, v in m.state_dict().items()}
    for n in R.KEYS:                                                      # test_gpu_iwae.py's absolute weight bound
        err, tol = np.abs(got[n] - Pr[n]).max(), max(T_PARAM, 4 * np.abs(P32[n] - Pr[n]).max())
        print("%s %s: err %.3g allowed %.3g" % (tag, n, err, tol))
        assert err <= tol, (n, err, tol)
        assert np.abs(Pr[n] - P[n]).max() > 1e-4                          # and it trained
    # the validation pass: the trained weights (the engine's own), the evaluation stream, N = the validation set's size
    e_val = eps_of(3, giwae.TAG_EVAL, Z)
    vb = [xv[i:i + batch] for i in range(0, n_val, batch)]
    val = lambda N, dt: float(np.mean([R.model_reference(got, b_, e_val(t, b_.shape[0]), coef, N, dt)["loss"]
                                       for t, b_ in enumerate(vb)]))
    ref, f32, other = val(n_val, torch.float64), val(n_val, torch.float32), val(n_train, torch.float64)
    check(tag, "val loss", tr.best_val_loss, ref, f32, T_LOSS)
    assert abs(other - ref) > 100 * T_LOSS * abs(ref)                     # the training set's N would have shown


def test_one_fused_batch_gradients_vs_fp64():
    """One batch with Adam's lr = 0 (the parameters stay, the gradients land in the flat gradient buffer): loss, tc and
    the ten gradients against autograd on the fp64 reference, both coefficient signs."""
    I, H, Z, b, N = 130, 24, 6, 67, 500
    its = loaders(b, b, b, 16, I)
    m, P = make_model(I, H, Z)
    tr = tc_vae.TCVAETrainer(m, *its, alpha=2.0, beta=0.5, gamma=3.0, dataset_size=N, seed=3)
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
    for n, v in m.state_dict().items():
        assert np.array_equal(v.cpu().double().numpy(), P[n]), n          # lr = 0: nothing moved
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    eps = ops_fused.iwae_normals(b, 1, Z, 3, 0, giwae.TAG_TRAIN).cpu().double().numpy()
    ref, f32 = R.model_reference(P, x, eps, COEF2, N), R.model_reference(P, x, eps, COEF2, N, torch.float32)
    check("batch", "loss", tr.losses[0], ref["loss"], f32["loss"], T_LOSS)
    check("batch", "tc", tr.tc[0], ref["tc"], f32["tc"], T_LOSS)
    got = engine_views(tr, "grad")
    assert sorted(got) == sorted(R.KEYS)
    for n in R.KEYS:
        check("batch", n, got[n].numpy(), ref["grads"][n], f32["grads"][n])


# ---- determinism ----------------------------------------------------------------------------------------------------
def _trained_small(epochs=1, cls=None, use_graph=True, n_train=96, I=64, H=48, Z=8, batch=32, its=None, **kw):
    its = its or loaders(batch, n_train, 48, 48, I)
    m, _ = make_model(I, H, Z)
    tr = (cls or tc_vae.TCVAETrainer)(m, *its, **kw)
    tr.use_graph = use_graph
    quiet(tr.train, epochs)
    return tr, m, its


def snapshot(tr, m):
    return (list(tr.losses), list(tr.tc), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
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
        tr, m, _ = _trained_small(epochs=2, use_graph=use_graph, **cfg)
        runs.append(snapshot(tr, m))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    assert len(runs[0][0]) == 10 and all(math.isfinite(v) for v in runs[0][0] + runs[0][1])
    # 1 epoch + checkpoint + a fresh trainer's resumed epoch == 2 epochs
    torch.manual_seed(99)
    tr, m, its = _trained_small(epochs=1, **cfg)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    assert ck["optim"]["config"]["beta"] == 6.0 and ck["optim"]["config"]["dataset_size"] == 300
    assert ck["history"]["noise_steps"] == 5 and len(ck["history"]["tc"]) == 5
    m2 = tc_vae.TCVAE(64, 48, 8).to(DEV)
    tr2 = tc_vae.TCVAETrainer(m2, *its)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 5 and tr2.losses == runs[0][0][:5] and tr2.tc == runs[0][1][:5]
    quiet(tr2.train, 1)
    same(snapshot(tr2, m2), runs[0])
    # other settings: refused under strict, taken otherwise
    for kw in (dict(beta=4.0), dict(alpha=0.5), dict(gamma=2.0), dict(dataset_size=301), dict(seed=1)):
        t3 = tc_vae.TCVAETrainer(tc_vae.TCVAE(64, 48, 8).to(DEV), *its, **kw)
        t3.load_checkpoint(path)
        with pytest.raises(GMError, match="different settings"):
            t3.train(1)
    t3 = tc_vae.TCVAETrainer(tc_vae.TCVAE(64, 48, 8).to(DEV), *its, beta=4.0)
    t3.load_checkpoint(path, strict=False)
    quiet(t3.train, 1)


# ---- paths ----------------------------------------------------------------------------------------------------------
class Mine(tc_vae.TCVAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_general_path_agrees_with_the_fused_run():
    """Three training batches and the validation pass (48 rows against 96: its own N) on both paths: parameters within
    test_gpu_iwae.py's 5e-5, the histories within 1e-4, the bound that test puts on the two paths' losses."""
    out = []
    for cls in (tc_vae.TCVAETrainer, Mine):
        torch.manual_seed(99)
        tr, m, _ = _trained_small(cls=cls, n_train=96, batch=32)          # 3 batches
        assert (tr._engine is None) == (cls is Mine) and len(tr.losses) == len(tr.tc) == 3 and tr.noise_steps == 3
        out.append((tr, {k: v.cpu() for k, v in m.state_dict().items()}))
    (a, wa), (b, wb) = out
    for n in wa:
        err = (wa[n] - wb[n]).abs().max().item()
        print("general path %s: %.3g" % (n, err))
        assert err <= T_PARAM, n
    for u, v in zip(a.losses + a.tc + [a.best_val_loss], b.losses + b.tc + [b.best_val_loss]):
        assert abs(u - v) <= 1e-4 * max(1.0, abs(v)), (u, v)
    # Z above the fused limit: the general path, same interface
    torch.manual_seed(99)
    tr, m, _ = _trained_small(Z=33, n_train=64, batch=32)
    assert tr._engine is None and len(tr.losses) == 2 and all(math.isfinite(v) for v in tr.losses + tr.tc)


# ---- decomposition, traverse, log_likelihood -----------------------------------------------------------------------
def test_decomposition_traverse_and_log_likelihood():
    I, H, Z, n, batch = 130, 24, 6, 130, 64                 # 130 test images: batches of 64, 64 and 2
    its = loaders(batch, 64, 64, n, I)
    m, P = make_model(I, H, Z)
    tr = tc_vae.TCVAETrainer(m, *its, alpha=2.0, beta=0.5, gamma=3.0, seed=4)
    tr.model.train()
    x = its[2].dataset.tensors[0]
    before = {k_: v.detach().cpu().clone() for k_, v in tr.model.state_dict().items()}
    torch.manual_seed(4)
    rng = torch.get_rng_state()
    res = tr.decomposition()                                # images=None: the whole test_iter
    assert torch.equal(torch.get_rng_state(), rng) and tr.model.training
    for k_, v in tr.model.state_dict().items():
        assert torch.equal(v.cpu(), before[k_]), k_
    assert type(res).__name__ == "TCResult" and res.n == n
    e_val = eps_of(4, giwae.TAG_EVAL, Z)
    xs = x.double().numpy()

    def ref_of(dt):
        tot = np.zeros(4)
        for t, lo in enumerate(range(0, n, batch)):
            xb = xs[lo:lo + batch]
            r = R.model_reference(P, xb, e_val(t, xb.shape[0]), COEF2, n, dt)
            tot += np.concatenate([r["terms"].sum(0), [r["recon"].sum()]])
        return tot / n
    ref, f32 = ref_of(torch.float64), ref_of(torch.float32)
    for name, got, r_, f_ in zip(("mi", "tc", "dw_kl", "recon"), res[:4], ref, f32):
        check("decomposition", name, got, r_, f_, T_LOSS)
    assert tr.decomposition(x) == res                       # bitwise: explicit images
    sub = tr.decomposition(x[:70])
    assert sub.n == 70 and sub.mi != res.mi                 # another N and other batches
    # traverse: mu(image) with one coordinate replaced, through the decoder
    vals = [-2.0, 0.0, 1.5]
    out = tr.traverse(x[3], 2, vals)
    assert tuple(out.shape) == (3, I) and out.dtype == torch.float32
    W = {n_: torch.as_tensor(v) for n_, v in P.items()}
    h = torch.relu(x[3:4].double() @ W["encoder.linear.weight"].T + W["encoder.linear.bias"])
    z = (h @ W["encoder.mu.weight"].T + W["encoder.mu.bias"]).repeat(3, 1)
    z[:, 2] = torch.tensor(vals, dtype=torch.float64)
    want = torch.sigmoid(torch.relu(z @ W["decoder.linear.weight"].T + W["decoder.linear.bias"])
                         @ W["decoder.recon.weight"].T + W["decoder.recon.bias"])
    err = (out.cpu().double() - want).abs().max().item()
    print("traverse: err %.3g" % err)
    assert err <= 1e-5
    assert not torch.equal(out[0], out[1]) and tr.model.training
    for bad in (-1, Z, 1.0, True):
        with pytest.raises(tc_vae.TCVAEError):
            tr.traverse(x[3], bad, vals)
    ll = tr.log_likelihood(x[:17], k=70, seed=1)
    assert type(ll).__name__ == "IWAEResult" and (ll.k, ll.n) == (70, 17) and math.isfinite(ll.ll_mean)
    assert ll == giwae.log_likelihood(tr, x[:17], 70, 1)    # q is the plain Gaussian: the VAE's estimate


# ---- learning check -------------------------------------------------------------------------------------------------
def test_learning_on_bands_and_beta_lowers_the_total_correlation():
    """The 16 band patterns tests/test_gpu_nfvae.py learns on (16 x 16 images, two adjacent rows or columns lit), the
    same size and duration: the loss falls, and the validation total correlation after training at beta = 6 is below
    that of the same model trained at beta = 1 from the same seed.

    Measured on an MI355X: the loss falls from 19303 to 17421 (beta = 6) and from 3776 to 1894 (beta = 1); the validation
    total correlation is 38.8175 against 38.8178.  Both sit at (Z - 1) log N = 7 log 256 = 38.816, the estimator's value
    when a batch's posteriors coincide: 80 batches on 16 distinct patterns leave the two runs 3e-4 apart, so this check
    holds by a small margin (the runs are bitwise reproducible)."""
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
    tcs = {}
    for beta in (6.0, 1.0):
        its = bands(64), bands(16), bands(16)
        torch.manual_seed(5)
        tr = tc_vae.TCVAETrainer(tc_vae.TCVAE(256, 128, 8), *its, beta=beta, seed=0)
        quiet(tr.train, 5)
        assert type(tr._engine).__name__ == "TCVAEEngine"
        assert len(tr.losses) == 80 and all(math.isfinite(v) for v in tr.losses + tr.tc)
        first, last = np.mean(tr.losses[:10]), np.mean(tr.losses[-10:])
        tcs[beta] = tr.decomposition(its[1].dataset.tensors[0]).tc
        print("learning beta=%g: first 10 %.3f last 10 %.3f, validation tc %.4f" % (beta, first, last, tcs[beta]))
        assert last < first
    assert tcs[6.0] < tcs[1.0]
