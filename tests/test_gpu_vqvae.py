"""VQ-VAE on the MI355X: the three quantisation kernels against the fp64 contract (tests/vqvae_reference.py), the engine
against fp64 training, determinism (run to run, graph against eager, resume), the general path, codes / decode /
reconstruct / code_usage, the MADE prior (sample, log_likelihood, checkpoint) and a learning check.

Bounds.  tests/test_gpu_catvae.py's scheme and test_gpu_iwae.py's bases: max(base, 4 x the deviation of the same contract
run in fp32 torch on the CPU from the fp64 reference), bases 1e-5 (loss sums), 1.5e-6 of max-abs (gradients, z_q, qerr,
lp), 5e-5 (weights).  Every comparison prints its error and its allowance.

Near-ties.  A choice whose fp64 gap between the best and the second-best squared distance is below 1e-4 can differ in
fp32, and agreement there says nothing: such variables are left out of exact comparisons (at most 0.2 % of variables and
2 % of rows may be; the share is asserted on the reference).  Values that depend on the choice (z_q, qerr, lp, dml, n_k,
dE) are compared with the reference evaluated on the device's own codes."""
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

import vq_vae  # noqa: E402
import vqvae_reference as R  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd import ops, ops_fused, trainers  # noqa: E402
from generative_models_amd import vqvae as gvq  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
T_LOSS, T_GRAD, T_PARAM = 1e-5, 1.5e-6, 5e-5             # test_gpu_iwae.py's bases (module docstring)
MIN_GAP, MAX_VARS_OUT, MAX_ROWS_OUT = 1e-4, 2e-3, 2e-2
ROW_CASES = [(1, 4, 2, 7), (3, 4, 5, 7), (7, 8, 33, 33), (16, 16, 128, 130), (8, 64, 256, 16), (49, 4, 16, 9),
             (16, 16, 1024, 16),                          # (N, D, K, B)
             (5, 12, 9, 6), (3, 24, 17, 5)]               # code widths that are no power of two: the kernel's other path
BETA = 0.25


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


def near_ties(tag, gap):
    """Boolean [rows, N]: the variables kept (fp64 gap >= 1e-4); asserts the share left out."""
    keep = gap >= MIN_GAP
    v_out, r_out = 1.0 - keep.mean(), 1.0 - keep.all(1).mean()
    print("%s: near-ties left out: %.3g of variables, %.3g of rows (min gap %.3g)" % (tag, v_out, r_out, gap.min()))
    assert v_out <= MAX_VARS_OUT and r_out <= MAX_ROWS_OUT, (tag, v_out, r_out)
    return keep


_INPUTS = {}


def row_inputs(N, D, K, B):
    """z_e [B, N D], E [K, D] ~ N(0, 1), the fp64 reference and its fp32 yardstick: computed once."""
    key = (N, D, K, B)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(1000 * N + 10 * D + K)
        ze, E = torch.randn(B, N * D, generator=gen), torch.randn(K, D, generator=gen)
        _INPUTS[key] = (ze, E, R.rows_reference(ze, E, N, BETA))
    return _INPUTS[key]


def run_quantise(ze, E, N, D, beta=BETA, ldz=None, lde=None):
    """gm_vq_quantise on padded buffers (leading dimensions of their own when asked): z_q, codes, qerr, lp on the CPU."""
    B, K, W = ze.shape[0], E.shape[0], N * D
    zp = torch.full((B, ldz or W), 7.0, device=DEV)
    zp[:, :W] = ze.to(DEV)
    Ep = torch.full((K, lde or D), 7.0, device=DEV)
    Ep[:, :D] = E.to(DEV)
    zq, codes = torch.full((B, W + 3), 7.0, device=DEV), torch.full((B, N + 2), 7, dtype=torch.int32, device=DEV)
    qerr, lp = torch.full((B + 1,), 7.0, device=DEV), torch.full((B + 1,), 7.0, device=DEV)
    ops_fused.vq_quantise(zp[:, :W], Ep[:, :D], zq[:, :W], codes[:, :N], qerr, lp, beta, B, N, D)
    torch.cuda.synchronize()
    assert torch.all(zq[:, W:] == 7.0) and torch.all(codes[:, N:] == 7)        # nothing past the row
    assert float(qerr[B]) == 7.0 and float(lp[B]) == 7.0                       # nothing past the batch
    return zq[:, :W].cpu().contiguous(), codes[:, :N].cpu().contiguous(), qerr[:B].cpu(), lp[:B].cpu()


def run_reduce(ze, E, codes, dz, wn, N, D, beta=BETA):
    B, W = ze.shape[0], N * D
    dml = torch.full((B, W + 1), 7.0, device=DEV)
    dzp = torch.full((B, W + 2), 7.0, device=DEV)
    dzp[:, :W] = dz.to(DEV)
    ops_fused.vq_reduce(ze.to(DEV), E.to(DEV), codes.to(DEV, torch.int32).contiguous(), dzp[:, :W], wn.to(DEV),
                        dml[:, :W], beta, B, N, D)
    torch.cuda.synchronize()
    assert torch.all(dml[:, W:] == 7.0)
    return dml[:, :W].cpu().contiguous()


def run_step(ze, E, codes, N, D, lr=1e-3, wd=1e-5):
    """gm_vq_step from zero moments at step 1: (E after, gradient, n_k, usage after starting at 5, m, v) on the CPU."""
    B, K = ze.shape[0], E.shape[0]
    Ed = E.to(DEV).clone().contiguous()
    m, v, g = torch.zeros(K, D, device=DEV), torch.zeros(K, D, device=DEV), torch.full((K, D), 7.0, device=DEV)
    nk = torch.full((K,), 7, dtype=torch.int32, device=DEV)
    usage = torch.full((K,), 5, dtype=torch.int32, device=DEV)
    sched = torch.from_numpy(ops.adam_schedule(lr, 1)).to(DEV)
    ops_fused.vq_step(ze.to(DEV), codes.to(DEV, torch.int32).contiguous(), Ed, B, N, D, moments=(m, v), sched=sched,
                      grad=g, nk=nk, usage=usage, weight_decay=wd)
    torch.cuda.synchronize()
    return Ed.cpu(), g.cpu(), nk.cpu(), usage.cpu(), m.cpu(), v.cpu()


# ---- kernels against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,D,K,B", ROW_CASES)
def test_quantise_vs_fp64(N, D, K, B):
    ze, E, ref = row_inputs(N, D, K, B)
    tag = "quantise N=%d D=%d K=%d B=%d" % (N, D, K, B)
    keep = near_ties(tag, ref["gap"])
    zq, codes, qerr, lp = run_quantise(ze, E, N, D)
    zq2, codes2, qerr2, lp2 = run_quantise(ze, E, N, D, ldz=N * D + 5, lde=D + 3)
    for a, b in ((zq, zq2), (codes, codes2), (qerr, qerr2), (lp, lp2)):
        assert torch.equal(a, b)                                            # run to run, under any leading dimension
    cd = codes.numpy()
    assert cd.min() >= 0 and cd.max() < K
    assert (cd[keep] == ref["codes"][keep]).all()
    assert torch.equal(zq, E[codes.long()].reshape(B, N * D))               # bitwise the codebook's rows
    own = R.rows_reference(ze, E, N, BETA, codes=cd)                        # the reference on the device's own codes
    own32 = R.rows_reference(ze, E, N, BETA, torch.float32, codes=cd)
    check(tag, "qerr", qerr.numpy(), own["qerr"], own32["qerr"])
    check(tag, "lp", lp.numpy(), own["lp"], own32["lp"])
    # rotating the batch by 3 rows rotates every output bitwise: a row's outputs do not depend on where it lands
    rz, rc, rq, rl = run_quantise(torch.roll(ze, 3, 0), E, N, D)
    assert torch.equal(rz, torch.roll(zq, 3, 0)) and torch.equal(rc, torch.roll(codes, 3, 0))
    assert torch.equal(rq, torch.roll(qerr, 3, 0)) and torch.equal(rl, torch.roll(lp, 3, 0))
    # another beta changes lp alone
    _, c0, q0, l0 = run_quantise(ze, E, N, D, beta=0.0)
    assert torch.equal(c0, codes) and torch.equal(q0, qerr) and torch.equal(l0, -qerr)


@pytest.mark.parametrize("N,D,K,B", ROW_CASES)
def test_reduce_and_step_vs_fp64(N, D, K, B):
    ze, E, _ = row_inputs(N, D, K, B)
    tag = "reduce/step N=%d D=%d K=%d B=%d" % (N, D, K, B)
    _, codes, _, _ = run_quantise(ze, E, N, D)
    cd = codes.numpy()
    gen = torch.Generator().manual_seed(7 + N)
    dz, wn = torch.randn(B, N * D, generator=gen), torch.rand(B, generator=gen) + 0.5
    for w in (torch.ones(B), wn):
        own = R.rows_reference(ze, E, N, BETA, dzdec=dz, wn=w, codes=cd)
        own32 = R.rows_reference(ze, E, N, BETA, torch.float32, dzdec=dz, wn=w, codes=cd)
        dml = run_reduce(ze, E, codes, dz, w, N, D)
        assert torch.equal(dml, run_reduce(ze, E, codes, dz, w, N, D))
        check(tag, "dml", dml.numpy(), own["dml"], own32["dml"])
    E1, g, nk, usage, m, v = run_step(ze, E, codes, N, D)
    again = run_step(ze, E, codes, N, D)
    for a, b in zip((E1, g, nk, usage, m, v), again):
        assert torch.equal(a, b)                                            # bitwise run to run
    assert (nk.numpy() == own["n_k"]).all() and int(nk.sum()) == B * N      # exact
    assert (usage.numpy() == own["n_k"] + 5).all()
    check(tag, "dE", g.numpy(), own["dE"], own32["dE"])
    unused = own["n_k"] == 0
    if K > B * N:
        assert unused.sum() >= K - B * N
    assert (g.numpy()[unused] == 0.0).all()                                 # nobody chose it: a gradient of exactly 0
    P, G, Z = {"E": E.double().numpy()}, {"E": own["dE"]}, {"E": np.zeros((K, D))}
    Pr = R.adam_reference(P, G, Z, Z, 1, 1e-3, 1e-5)[0]["E"]
    P32 = R.adam_reference({"E": E.numpy()}, {"E": own32["dE"]}, Z, Z, 1, 1e-3, 1e-5)[0]["E"].astype(np.float32)
    err, tol = np.abs(E1.double().numpy() - Pr).max(), max(T_PARAM, 4 * np.abs(P32 - Pr).max())
    print("%s E after one Adam step: err %.3g allowed %.3g" % (tag, err, tol))
    assert err <= tol and np.abs(Pr - P["E"]).max() > 1e-4
    # without a schedule: the gradient and the counts only, E untouched
    Ed, g2 = E.to(DEV).clone(), torch.empty(K, D, device=DEV)
    ops_fused.vq_step(ze.to(DEV), codes.to(DEV), Ed, B, N, D, grad=g2)
    assert torch.equal(Ed.cpu(), E) and torch.equal(g2.cpu(), g)


@pytest.mark.parametrize("N,D,K,B", [(3, 4, 5, 7), (16, 16, 128, 130)])
def test_every_row_on_the_same_code(N, D, K, B):
    """One code at the data, the others far away: n_k = B N on it (2080 pairs over the step kernel's four waves in the
    larger case) and 0 elsewhere."""
    gen = torch.Generator().manual_seed(5)
    ze = 0.1 * torch.randn(B, N * D, generator=gen)
    E = 50.0 + torch.randn(K, D, generator=gen)
    E[2] = 0.01 * torch.randn(D, generator=gen)
    zq, codes, qerr, lp = run_quantise(ze, E, N, D)
    assert torch.all(codes == 2)
    own, own32 = R.rows_reference(ze, E, N, BETA, codes=codes.numpy()), \
        R.rows_reference(ze, E, N, BETA, torch.float32, codes=codes.numpy())
    assert (own["codes"] == R.rows_reference(ze, E, N, BETA)["codes"]).all()
    check("one code", "qerr", qerr.numpy(), own["qerr"], own32["qerr"])
    E1, g, nk, usage, _, _ = run_step(ze, E, codes, N, D)
    assert int(nk[2]) == B * N and int(nk.sum()) == B * N
    check("one code", "dE", g.numpy(), own["dE"], own32["dE"])
    assert torch.count_nonzero(g) == D and torch.equal(torch.count_nonzero(g, 1) > 0, torch.arange(K) == 2)


@pytest.mark.parametrize("N,D,K,B", [(3, 4, 5, 7), (49, 4, 16, 9), (16, 16, 128, 130)])
def test_ties_and_bad_input(N, D, K, B):
    ze, E, _ = row_inputs(N, D, K, B)
    # exact ties: two identical codebook rows -- the lower index wins (the two sit in different lanes when the K codes
    # are shared among lanes, in one lane otherwise)
    E2 = E.clone()
    E2[K - 1], E2[3 % K] = E2[0], E2[1]
    _, codes, _, _ = run_quantise(ze, E2, N, D)
    ref = R.rows_reference(ze, E2, N, BETA)
    dup = {K - 1, 3 % K} - {0, 1}
    assert not (set(np.unique(codes.numpy()).tolist()) & dup)
    assert set(np.unique(codes.numpy()).tolist()) & {0, 1}                  # the originals are chosen
    keep = ref["gap"] >= MIN_GAP                                            # a tied winner has gap 0: compare where it is clear
    assert (codes.numpy()[keep] == ref["codes"][keep]).all()
    tied = np.isin(ref["codes"], [0, 1])
    assert (codes.numpy()[tied & (ref["gap"] == 0)] == ref["codes"][tied & (ref["gap"] == 0)]).all()
    # a NaN row: code 0, never an index >= K; the other rows are untouched
    zn = ze.clone()
    zn[2 % B] = float("nan")
    zq, cn, qerr, _ = run_quantise(zn, E, N, D)
    _, c0, q0, _ = run_quantise(ze, E, N, D)
    assert torch.all(cn[2 % B] == 0) and int(cn.min()) >= 0 and int(cn.max()) < K
    others = torch.arange(B) != 2 % B
    assert torch.equal(cn[others], c0[others]) and torch.equal(qerr[others], q0[others]) and math.isnan(float(qerr[2 % B]))
    assert torch.equal(zq[2 % B], E[0].repeat(N))
    En = E.clone()
    En[1] = float("nan")                                                    # a NaN code is never chosen
    _, cn, _, _ = run_quantise(ze, En, N, D)
    assert not bool((cn == 1).any()) and int(cn.min()) >= 0 and int(cn.max()) < K
    # +-1e4 stays finite
    gen = torch.Generator().manual_seed(11)
    zb = torch.where(torch.rand(B, N * D, generator=gen) < 0.5, -1e4, 1e4)
    Eb = torch.where(torch.rand(K, D, generator=gen) < 0.5, -1e4, 1e4)
    zq, cb, qerr, lp = run_quantise(zb, Eb, N, D)
    assert torch.isfinite(qerr).all() and torch.isfinite(lp).all() and torch.isfinite(zq).all()
    own, own32 = R.rows_reference(zb, Eb, N, BETA, codes=cb.numpy()), \
        R.rows_reference(zb, Eb, N, BETA, torch.float32, codes=cb.numpy())
    check("1e4", "qerr", qerr.numpy(), own["qerr"], own32["qerr"])
    assert (own["qerr"] <= R.rows_reference(zb, Eb, N, BETA)["qerr"] * (1 + 1e-6)).all()      # a nearest code all the same
    dz = torch.randn(B, N * D, generator=gen)
    dml = run_reduce(zb, Eb, cb, dz, torch.ones(B), N, D)
    E1, g, _, _, _, _ = run_step(zb, Eb, cb, N, D)
    assert torch.isfinite(dml).all() and torch.isfinite(g).all() and torch.isfinite(E1).all()
    # a code outside [0, K) handed to gm_vq_reduce is clamped, never read past the codebook
    bad = cb.clone()
    bad[0, 0], bad[B - 1, N - 1] = -3, K + 5
    dml = run_reduce(zb, Eb, bad, dz, torch.ones(B), N, D)
    assert torch.isfinite(dml).all()


# ---- the engine against fp64 -----------------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, I, seed=7):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


def make_model(I, H, N, D, K, seed=1234, scale=4.0):
    """VQVAE under a fixed seed, the codebook widened to uniform (-1, 1) and the embed layer by `scale`, so that the codes
    in use are many and the choices clear."""
    torch.manual_seed(seed)
    m = vq_vae.VQVAE(I, H, N, D, K)
    with torch.no_grad():
        m.codebook.weight.mul_(K)
        m.encoder.embed.weight.mul_(scale)
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


@pytest.mark.parametrize("I,H,N,D,K,b", [(130, 24, 6, 4, 8, 17), (784, 400, 16, 16, 128, 512)])
def test_one_fused_batch_gradients_vs_fp64(I, H, N, D, K, b):
    """One batch with Adam's lr = 0 (the parameters stay, the gradients land in the flat gradient buffer): loss, vq_loss
    and the nine gradients against the fp64 reference evaluated on the engine's training codes, which agree with the fp64
    arg min within the near-tie cap; then the validation batch of the same call, on the validation codes buffer."""
    its = loaders(b, b, b, 16, I)
    m, P = make_model(I, H, N, D, K)
    tr = vq_vae.VQVAETrainer(m, *its)
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
    assert type(tr._engine).__name__ == "VQVAEEngine"
    for n, v in m.state_dict().items():
        assert np.array_equal(v.cpu().double().numpy(), P[n]), n          # lr = 0: nothing moved
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    xv = its[1].dataset.tensors[0][trainers._epoch_order(its[1])].double().numpy()
    eng = tr._engine
    ct, cv = eng.codes_train[:b].cpu().numpy(), eng.codes_val[:b].cpu().numpy()
    tag = "batch %s" % ((I, H, N, D, K, b),)
    free = R.model_reference(P, x, N, BETA, grads=False)
    keep = near_ties(tag, free["gap"])
    assert (ct[keep] == free["codes"][keep]).all() and len(np.unique(ct)) > 1
    ref, f32 = R.model_reference(P, x, N, BETA, codes=ct), R.model_reference(P, x, N, BETA, torch.float32, codes=ct)
    check(tag, "loss", tr.losses[0], ref["loss"], f32["loss"], T_LOSS)
    check(tag, "vq_loss", tr.vq_loss[0], ref["vq"], f32["vq"], T_LOSS)
    got = engine_views(tr, "grad")
    assert sorted(got) == sorted(R.KEYS)
    for n in R.KEYS:
        check(tag, n, got[n].numpy(), ref["grads"][n], f32["grads"][n])
    nk = np.bincount(ct.reshape(-1), minlength=K)
    assert (eng.nk.cpu().numpy() == nk).all() and (eng.usage.cpu().numpy() == nk).all()
    counts, perp = tr.epoch_usage()
    assert counts.tolist() == nk.tolist() and 1.0 <= perp <= K
    # validation: the same parameters, the validation buffer's codes
    freev = R.model_reference(P, xv, N, BETA, grads=False)
    keepv = near_ties(tag + " validation", freev["gap"])
    assert (cv[keepv] == freev["codes"][keepv]).all()
    rv = R.model_reference(P, xv, N, BETA, codes=cv, grads=False)
    rv32 = R.model_reference(P, xv, N, BETA, torch.float32, codes=cv, grads=False)
    check(tag + " validation", "loss", tr.best_val_loss, rv["loss"], rv32["loss"], T_LOSS)


EPOCH_SEED = 1237


def test_engine_vs_fp64_training():
    """One epoch at (I, H, N, D, K) = (49, 32, 3, 4, 5), bs 16 over 89 rows (five full batches and a ragged one of 9)
    against Adam on the fp64 reference's gradients: losses and vq_loss batch by batch (batch t's are a function of every
    parameter after batch t - 1), every parameter after the epoch, and the last batch's codes.  Nothing is random on the
    device, so the reference runs on its own choices and asserts that their smallest gap over all batches is >= 1e-4: a
    statement about the inputs.  The model seed was picked on the CPU: with 1237 the smallest gap is 1.43e-2 and all five
    codes are in use (1234 leaves two codes unused, 1235 meets a gap of 7.0e-5)."""
    I, H, N, D, K, batch, n_train = 49, 32, 3, 4, 5, 16, 89
    its = loaders(batch, n_train, batch, 16, I)
    m, P = make_model(I, H, N, D, K, seed=EPOCH_SEED)
    tr = vq_vae.VQVAETrainer(m, *its)
    st = torch.get_rng_state()
    quiet(tr.train, 1)
    assert type(tr._engine).__name__ == "VQVAEEngine"
    nb = (n_train + batch - 1) // batch
    assert len(tr.losses) == len(tr.vq_loss) == nb and tr.noise_steps == nb
    after = torch.get_rng_state()
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].double().numpy()
    batches = [x[i:i + batch] for i in range(0, n_train, batch)]
    trail, Lr, Vr, gap = R.train_reference(P, batches, N, BETA, 1e-3, 1e-5)
    trail32, L32, V32, _ = R.train_reference(P, batches, N, BETA, 1e-3, 1e-5, dtype=torch.float32)
    print("epoch: the reference's smallest gap over %d batches: %.3g" % (nb, gap))
    assert gap >= MIN_GAP
    for t in range(nb):
        for name, got, ref, f32 in (("loss", tr.losses, Lr, L32), ("vq_loss", tr.vq_loss, Vr, V32)):
            check("epoch", "%s[%d]" % (name, t), got[t], ref[t], f32[t], T_LOSS)
    got = {n: v.detach().cpu().double().numpy() for n, v in m.state_dict().items()}
    Pr, P32 = trail[-1], trail32[-1]
    for n in R.KEYS:
        assert np.abs(Pr[n] - P[n]).max() > 1e-4                          # it trained
        err, tol = np.abs(got[n] - Pr[n]).max(), max(T_PARAM, 4 * np.abs(P32[n] - Pr[n]).max())
        print("epoch %s: err %.3g allowed %.3g" % (n, err, tol))
        assert err <= tol, (n, err, tol)
    last = R.model_reference(trail[-2], batches[-1], N, BETA, grads=False)
    assert (tr._engine.codes_train[:9].cpu().numpy() == last["codes"]).all()
    # the global CPU generator: two epoch orders and nothing else
    torch.set_rng_state(st)
    trainers._epoch_order(its[0]), trainers._epoch_order(its[1])
    assert torch.equal(torch.get_rng_state(), after)


# ---- determinism -----------------------------------------------------------------------------------------------------
def _trained_small(epochs=1, cls=None, use_graph=True, n_train=96, I=64, H=48, N=4, D=4, K=8, batch=32, its=None,
                   beta=BETA):
    its = its or loaders(batch, n_train, 48, 48, I)
    m, _ = make_model(I, H, N, D, K)
    tr = (cls or vq_vae.VQVAETrainer)(m, *its, beta=beta)
    tr.use_graph = use_graph
    quiet(tr.train, epochs)
    return tr, m, its


def snapshot(tr, m):
    return (list(tr.losses), list(tr.vq_loss), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
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
    conf = ck["optim"]["config"]
    assert (conf["num_vars"], conf["code_dim"], conf["num_codes"], conf["beta"]) == (4, 4, 8, BETA)
    assert ck["history"]["noise_steps"] == 10 and "codebook.weight" in ck["model"] and ck["history"]["prior_state"] is None
    new = lambda **kw: vq_vae.VQVAETrainer(vq_vae.VQVAE(64, 48, 4, 4, 8).to(DEV), *its, **dict(dict(beta=BETA), **kw))
    tr2 = new()
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 10 and tr2.losses == runs[0][0][:10] and tr2.vq_loss == runs[0][1][:10]
    quiet(tr2.train, 1)
    same(snapshot(tr2, tr2.model), runs[0])
    # other settings: refused under strict, taken otherwise
    ck["optim"]["config"]["num_codes"] = 16
    other = str(tmp_path / "ck16.pt")
    torch.save(ck, other)
    for p, kw in ((other, {}), (path, dict(beta=0.5))):
        t3 = new(**kw)
        t3.load_checkpoint(p)
        with pytest.raises(GMError):
            t3.train(1)
    t3 = new()
    t3.load_checkpoint(other, strict=False)
    quiet(t3.train, 1)


# ---- paths -----------------------------------------------------------------------------------------------------------
class Mine(vq_vae.VQVAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_general_path_agrees_with_the_fused_run(monkeypatch):
    """test_gpu_catvae.py's general-path bounds: parameters within 5e-5; losses and the moments within 1e-4 of their
    max-abs.  Sizes over the kernels' limits (K D = 32 768) have no fused run to agree with: their first batch's loss is
    compared with the fp64 reference instead, to 1e-4."""
    made = []

    class Keep(trainers.FlatAdam):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(giwae, "FlatAdam", Keep)
    out = []
    for cls in (vq_vae.VQVAETrainer, Mine):
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
    for u, v in zip(a.losses + a.vq_loss + [a.best_val_loss], b.losses + b.vq_loss + [b.best_val_loss]):
        assert abs(u - v) <= 1e-4 * max(1.0, abs(v)), (u, v)
    opt = made[0]
    for what, flat in (("m", opt.m), ("v", opt.v)):
        fused = engine_views(a, what)
        for (n, p), o in zip(b.model.named_parameters(), opt.offs):
            err = scaled_err(flat[o:o + p.numel()].cpu().numpy(), fused[n].reshape(-1).numpy())
            print("general path %s of %s: %.3g" % (what, n, err))
            assert err <= 1e-4, (what, n, err)
    # K D above the fused limit: the general path, same interface
    torch.manual_seed(99)
    its = loaders(32, 64, 48, 48, 64)
    m, P = make_model(64, 48, 2, 32, 1024)
    tr = vq_vae.VQVAETrainer(m, *its)
    st = torch.get_rng_state()
    quiet(tr.train, 1)
    assert tr._engine is None and len(tr.losses) == 2 and all(math.isfinite(v) for v in tr.losses + tr.vq_loss)
    assert math.isfinite(tr.best_val_loss)
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()[:32]
    ref = R.model_reference(P, x, 2, BETA, grads=False)
    print("over the limit: loss %.6f ref %.6f vq %.6f ref %.6f (min gap %.3g)"
          % (tr.losses[0], ref["loss"], tr.vq_loss[0], ref["vq"], ref["min_gap"]))
    assert ref["min_gap"] >= MIN_GAP
    assert abs(tr.losses[0] - ref["loss"]) <= 1e-4 * ref["loss"] and abs(tr.vq_loss[0] - ref["vq"]) <= 1e-4 * ref["vq"]


# ---- codes, decode, reconstruct, code_usage --------------------------------------------------------------------------
def test_codes_decode_reconstruct_and_usage():
    I, H, N, D, K, n = 64, 48, 4, 4, 8, 37
    its = loaders(16, 32, 16, n, I)
    m, P = make_model(I, H, N, D, K)
    tr = vq_vae.VQVAETrainer(m, *its)
    tr.model.train()
    x = its[2].dataset.tensors[0]
    rng = torch.get_rng_state()
    c = tr.codes(x)
    rec = tr.reconstruct(x)
    counts, perp = tr.code_usage(x)
    counts0, perp0 = tr.code_usage()                                       # images=None: the test set
    s = tr.sample(21, seed=5)
    assert torch.equal(torch.get_rng_state(), rng) and tr.model.training
    for k_, v in tr.model.state_dict().items():
        assert np.array_equal(v.cpu().double().numpy(), P[k_]), k_
    assert c.shape == (n, N) and c.dtype == torch.int64 and int(c.min()) >= 0 and int(c.max()) < K
    ref = R.model_reference(P, x.double().numpy(), N, BETA, grads=False)
    keep = near_ties("codes", ref["gap"])
    assert (c.numpy()[keep] == ref["codes"][keep]).all()
    assert counts.dtype == torch.int64 and counts.shape == (K,) and int(counts.sum()) == n * N
    assert counts.tolist() == np.bincount(c.numpy().reshape(-1), minlength=K).tolist()
    assert counts0.tolist() == counts.tolist() and perp0 == perp and 1.0 <= perp <= K
    p = counts.double() / counts.sum()
    assert abs(perp - math.exp(-(p[p > 0] * p[p > 0].log()).sum())) <= 1e-12 * K
    # reconstruct is decode of codes; decode against the fp64 decoder
    d = tr.decode(c)
    assert rec.shape == (n, I) and rec.is_cuda and torch.equal(rec, d)
    Pt = {k_: R.as_t(P[k_]) for k_ in R.KEYS}
    xr = R._decode(Pt, Pt["codebook.weight"][c].reshape(n, N * D)).numpy()
    assert np.abs(d.cpu().double().numpy() - xr).max() <= 1e-5
    for bad in (c[:, :3], c.float(), c - K, c + K, c == 0):
        with pytest.raises(ValueError):
            tr.decode(bad)
    # without a prior: uniform codes from a private generator
    cd = torch.randint(0, K, (21, N), generator=torch.Generator().manual_seed(5))
    assert s.shape == (21, I) and torch.equal(s, tr.decode(cd)) and not torch.equal(s, tr.sample(21, seed=6))
    assert float(s.min()) >= 0.0 and float(s.max()) <= 1.0
    pz = tr.parzen(n_samples=64, sigmas=[0.2], n_val=16, seed=0)
    assert math.isfinite(pz.ll_mean)
    with pytest.raises(GMError):
        tr.log_likelihood(x)                                               # no prior yet
    with pytest.raises(GMError):
        giwae.log_likelihood(tr, x, 3, 0)                                  # the encoder is not vae.py's


# ---- the prior and the learning check --------------------------------------------------------------------------------
def bands(reps):
    """The 16 band patterns tests/test_gpu_made.py learns on (16 x 16 images, two adjacent rows or columns lit)."""
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


_BANDS = {}


def trained_on_bands():
    """VQVAE(256, 128, 8, 4, 16) trained 5 epochs on the bands (2048 rows in batches of 64: 160 batches), then
    fit_prior(3, hidden_dim=64): once for both tests."""
    if not _BANDS:
        its = bands(128), bands(16), bands(16)
        torch.manual_seed(5)
        tr = vq_vae.VQVAETrainer(vq_vae.VQVAE(256, 128, 8, 4, 16), *its)
        quiet(tr.train, 5)
        assert type(tr._engine).__name__ == "VQVAEEngine"
        with pytest.raises(GMError):
            tr.log_likelihood()                                            # before fit_prior
        prior = quiet(tr.fit_prior, 3, hidden_dim=64)
        _BANDS.update(tr=tr, its=its, prior=prior)
    return _BANDS["tr"], _BANDS["its"], _BANDS["prior"]


def test_learning_on_bands():
    """The codebook starts inside (-1/K, 1/K), as the paper's does, and the encoder's outputs leave it behind at first:
    in fp64 on the CPU qerr climbs from 0.6 to about 1500 per image around batch 45 before the codebook catches up, and the
    loss is back under its first value from about batch 85 on (about 28 per image against 63 at batches 120 to 200).  The
    160 batches of this run end well past that transient; 80 would end inside it."""
    tr, _, _ = trained_on_bands()
    assert len(tr.losses) == 160 and all(math.isfinite(v) for v in tr.losses + tr.vq_loss)
    first, last = np.mean(tr.losses[:10]), np.mean(tr.losses[-10:])
    counts, perp = tr.code_usage()
    print("learning: first 10 %.3f last 10 %.3f, perplexity %.3f, epoch perplexity %.3f"
          % (first, last, perp, tr.epoch_usage()[1]))
    assert last < first and perp > 1.0 and int(counts.sum()) == 256 * 8


def test_prior_sampling_likelihood_and_checkpoint(tmp_path):
    tr, its, prior = trained_on_bands()
    N, K, L = 8, 16, 4
    assert prior is tr.prior and type(prior).__name__ == "MADETrainer" and prior.model.image_size == N * L
    assert prior.model.hidden_dim == 64 and len(prior.losses) == 3 * 4     # 2048 rows in batches of 512
    mode, rng = tr.model.training, torch.get_rng_state()
    s = tr.sample(33, seed=3)
    assert s.shape == (33, 256) and float(s.min()) >= 0.0 and float(s.max()) <= 1.0
    assert torch.equal(s, tr.sample(33, seed=3)) and not torch.equal(s, tr.sample(33, seed=4))
    bits = prior.sample(33, seed=3)
    assert bits.shape == (33, N * L)
    assert torch.equal(s, tr.decode(vq_vae.bits_code(bits, K)))
    res = tr.log_likelihood()
    assert torch.equal(torch.get_rng_state(), rng) and tr.model.training == mode
    assert type(res).__name__ == "VQResult" and res.n == 256 and all(math.isfinite(v) for v in res[:4])
    xt = its[2].dataset.tensors[0]
    rows = prior.log_likelihood_rows(vq_vae.code_bits(tr.codes(xt), K))
    assert abs(res.prior_mean - float(rows.mean())) <= 1e-12 * abs(res.prior_mean)
    assert abs(res.recon_mean + res.prior_mean - res.ll_mean) <= 1e-9 * abs(res.ll_mean)
    assert res.prior_mean <= 0.0 and res.recon_mean <= -0.5 * 256 * math.log(math.pi)
    assert tr.log_likelihood(xt) == res
    pz = tr.parzen(n_samples=64, sigmas=[0.2], n_val=16, seed=0)
    assert math.isfinite(pz.ll_mean)
    # K = 5 is no power of two
    t5 = vq_vae.VQVAETrainer(vq_vae.VQVAE(256, 128, 8, 4, 5), *its)
    with pytest.raises(gvq.VQVAEError):
        t5.fit_prior(1)
    # a checkpoint round-trips the prior
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    ps = ck["history"]["prior_state"]
    assert (ps["image_size"], ps["hidden_dim"], ps["order"]) == (N * L, 64, "natural") and "linear.weight" in ps["model"]
    tr2 = vq_vae.VQVAETrainer(vq_vae.VQVAE(256, 128, 8, 4, 16), *its)
    assert tr2.prior is None
    tr2.load_checkpoint(path)
    assert tr2.prior is not None and torch.equal(tr2.sample(33, seed=3), s)
    assert tr2.log_likelihood(xt) == res
