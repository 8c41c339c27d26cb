"""Categorical VAE on the MI355X: the two Gumbel-Softmax kernels against the fp64 contract (tests/catvae_reference.py) on
the device's own noise, the engine against fp64 training, determinism (run to run, graph against eager, resume), the
general path, posterior_codes and log_likelihood, sample / decode / codes and a learning check.

Bounds.  test_gpu_iwae.py's / test_gpu_nfvae.py's scheme and bases: max(base, 4 x the deviation of the same contract run
in fp32 torch on the CPU from the fp64 reference), bases 1e-5 (loss sums), 1.5e-6 of max-abs (gradients, y, lp, kl,
log_q), 5e-5 (weights).  The factor 4 is the project's margin for another, equally valid fp32 evaluation order.  Every
comparison prints its error and its allowance.

Near-ties.  A hard choice whose top-two gap of l + g is small can differ between fp32 and fp64, and agreement there says
nothing: where hard choices are compared, a variable whose fp64 gap is below 1e-4 is left out (at most 0.2 % of variables
and 2 % of sample rows may be); outside that set codes and one-hots match exactly.  Tests that need every choice right
assert min gap >= 1e-4 on the reference -- an assertion about the inputs."""
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

import cat_vae  # noqa: E402
import catvae_reference as R  # noqa: E402
from generative_models_amd import catvae as gcat  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd import ops_fused, trainers  # noqa: E402
from generative_models_amd._lib import CAT_DISCRETE, CAT_RELAXED, CAT_ST, GMError  # noqa: E402

DEV = "cuda"
T_LOSS, T_GRAD, T_PARAM = 1e-5, 1.5e-6, 5e-5             # test_gpu_iwae.py's bases (module docstring)
MIN_GAP, MAX_VARS_OUT, MAX_ROWS_OUT = 1e-4, 2e-3, 2e-2
ROW_CASES = [(1, 2, 1, 7), (3, 5, 3, 7), (7, 3, 2, 33), (20, 10, 1, 130), (30, 10, 64, 16), (16, 64, 2, 9)]  # (N, C, k, B)
TAUS = (1.0, 0.5, 0.1)
SEED, STEP = 0x123456789ABCDEF, 77


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


def row_inputs(N, C, k, B):
    """logits ~ N(0, 1.5^2), dy ~ N(0, 1) for the case's B k rows, and the device's own Gumbel noise: computed once."""
    key = (N, C, k, B)
    if key not in _INPUTS:
        gen = torch.Generator().manual_seed(1000 * N + 10 * C + k)
        l = torch.randn(B, N * C, generator=gen) * 1.5
        g = ops_fused.catvae_gumbels(B, k, N, C, SEED, STEP, gcat.TAG_TRAIN).cpu()
        _INPUTS[key] = (l, g, g.double().numpy())
    return _INPUTS[key]


def run_sample(l, B, k, N, C, mode, tau=None, seed=SEED, step=STEP, tag=None, ldl=None):
    W = N * C
    lpad = torch.full((B, ldl or W), 7.0, device=DEV)          # a leading dimension of its own when asked
    lpad[:, :W] = l.to(DEV)
    y, lp = torch.full((B * k, W + 3), 7.0, device=DEV), torch.full((B * k,), 7.0, device=DEV)
    kl = torch.full((B,), 7.0, device=DEV)
    codes = torch.full((B * k, N), 7, dtype=torch.int32, device=DEV)
    noise = ops_fused.iwae_noise(seed, gcat.TAG_TRAIN if tag is None else tag, k, step=step)
    ops_fused.cat_sample(lpad[:, :W], y[:, :W], lp, noise, B, k, N, C, mode, tau=tau, kl=kl,
                         codes=codes if mode == CAT_DISCRETE else None)
    torch.cuda.synchronize()
    assert torch.all(y[:, W:] == 7.0)                          # nothing past the row
    return y[:, :W].cpu().contiguous(), lp.cpu(), kl.cpu(), codes.cpu()


def run_reduce(l, dy, wn, B, N, C, tau, seed=SEED, step=STEP):
    W = N * C
    dl = torch.full((B, W + 1), 7.0, device=DEV)
    noise = ops_fused.iwae_noise(seed, gcat.TAG_TRAIN, 1, step=step)
    ops_fused.cat_reduce(l.to(DEV), dy.to(DEV), wn.to(DEV), dl[:, :W], noise, B, N, C, tau=tau)
    torch.cuda.synchronize()
    assert torch.all(dl[:, W:] == 7.0)
    return dl[:, :W].cpu().contiguous()


# ---- noise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,k,B", ROW_CASES)
def test_noise_mode_is_the_gumbel_of_the_philox_words(N, C, k, B):
    """g = -log(-log(u)) of the contract's words.  Allowance: two fp32 logarithms, each within 2 ulp -- the inner one's
    relative error is an absolute error of g, the outer one's scales with |g|: 2^-22 (1 + |g|); or 4 x numpy's float32
    evaluation's deviation where that is larger."""
    _, g, _ = row_inputs(N, C, k, B)
    words = R.philox_words(B * k, N * C, SEED, STEP, gcat.TAG_TRAIN)
    ref, f32 = R.gumbel(words), R.gumbel(words, np.float32).astype(np.float64)
    assert np.isfinite(g.numpy()).all() and g.shape == (B * k, N * C)
    err = np.abs(g.double().numpy() - ref)
    tol = np.maximum(2.0 ** -22 * (1.0 + np.abs(ref)), 4.0 * np.abs(f32 - ref).max())
    print("noise N=%d C=%d k=%d B=%d: max err %.3g (fp32 numpy %.3g), g in [%.3f, %.3f]"
          % (N, C, k, B, err.max(), np.abs(f32 - ref).max(), ref.min(), ref.max()))
    assert (err <= tol).all()
    again = ops_fused.catvae_gumbels(B, k, N, C, SEED, STEP, gcat.TAG_TRAIN).cpu()
    assert torch.equal(again, g)                                # bitwise stable run to run
    other = ops_fused.catvae_gumbels(B, k, N, C, SEED, STEP, gcat.TAG_EVAL).cpu()
    assert not torch.equal(other, g)                            # the tag is part of the stream
    # RELAXED at l = 0, tau = 1 is the softmax of that noise
    y, lp, kl, _ = run_sample(torch.zeros(B, N * C), B, k, N, C, CAT_RELAXED, tau=1.0)
    sm = torch.softmax(g.double().view(B * k, N, C), -1).reshape(B * k, N * C).numpy()
    sm32 = torch.softmax(g.view(B * k, N, C), -1).reshape(B * k, N * C).numpy()
    check("noise N=%d C=%d" % (N, C), "softmax(g)", y.numpy(), sm, sm32)
    assert np.abs(lp.numpy()).max() <= 1e-5 * N and np.abs(kl.numpy()).max() <= 1e-5 * N     # KL = 0 at equal logits


def test_gumbels_beyond_the_fused_limits_continue_the_same_stream():
    """C = 65 and k = 70 go in pieces: every element is the word the contract names."""
    N, C, k, B = 17, 65, 70, 3
    g = ops_fused.catvae_gumbels(B, k, N, C, 5, 2, gcat.TAG_EVAL).cpu().double().numpy()
    ref = R.gumbel(R.philox_words(B * k, N * C, 5, 2, gcat.TAG_EVAL))
    assert g.shape == ref.shape and (np.abs(g - ref) <= 2.0 ** -22 * (1.0 + np.abs(ref))).all()


# ---- kernels against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,k,B", ROW_CASES)
def test_sample_vs_fp64(N, C, k, B):
    l, g, g64 = row_inputs(N, C, k, B)
    tag = "sample N=%d C=%d k=%d B=%d" % (N, C, k, B)
    for tau in TAUS:
        ref = R.rows_reference(l, g64, N, C, k, tau)
        f32 = R.rows_reference(l, g64, N, C, k, tau, torch.float32)
        y, lp, kl, _ = run_sample(l, B, k, N, C, CAT_RELAXED, tau=tau, ldl=N * C + 5)
        y2, lp2, kl2, _ = run_sample(l, B, k, N, C, CAT_RELAXED, tau=tau)
        assert torch.equal(y, y2) and torch.equal(lp, lp2) and torch.equal(kl, kl2)       # run to run, any ld
        t = "%s tau=%g" % (tag, tau)
        check(t, "y", y.numpy(), ref["y"], f32["y"])
        check(t, "lp", lp.numpy(), ref["lp"], f32["lp"])
        check(t, "kl", kl.numpy(), ref["kl"], f32["kl"])
        assert np.abs(y.double().view(B * k, N, C).sum(-1).numpy() - 1.0).max() <= 4 * C * 2.0 ** -24
    ref = R.rows_reference(l, g64, N, C, k, 1.0)
    f32 = R.rows_reference(l, g64, N, C, k, 1.0, torch.float32)
    keep = near_ties(tag, ref["gap"])
    for mode in (CAT_ST, CAT_DISCRETE):
        y, lp, kl, codes = run_sample(l, B, k, N, C, mode)
        oh = y.view(B * k, N, C).numpy()
        assert set(np.unique(oh)) <= {0.0, 1.0} and (oh.sum(-1) == 1.0).all()
        assert (oh[keep] == ref["onehot"].reshape(B * k, N, C)[keep]).all()
        if mode == CAT_ST:
            check(tag + " ST", "lp", lp.numpy(), ref["lp"], f32["lp"])
            check(tag + " ST", "kl", kl.numpy(), ref["kl"], f32["kl"])
            assert torch.all(codes == 7)                        # codes are DISCRETE's
        else:
            cd = codes.numpy()
            assert (cd[keep] == ref["codes"][keep]).all() and (oh.argmax(-1) == cd).all()
            assert torch.all(kl == 7.0)                         # kl is not DISCRETE's
            own = R.rows_reference(l, g64, N, C, k, 1.0, codes=cd)            # the reference on the device's own codes
            own32 = R.rows_reference(l, g64, N, C, k, 1.0, torch.float32, codes=cd)
            check(tag + " DISCRETE", "lp", lp.numpy(), own["lp_discrete"], own32["lp_discrete"])


@pytest.mark.parametrize("N,C,k,B", ROW_CASES)
def test_reduce_vs_fp64(N, C, k, B):
    """gm_cat_reduce is the k = 1 batch's backward: the case's B k sample rows are taken as B k images of one sample."""
    l0, _, _ = row_inputs(N, C, k, B)
    rows = B * k
    gen = torch.Generator().manual_seed(7 + N)
    l = (l0.repeat_interleave(k, 0) + 0.1 * torch.randn(rows, N * C, generator=gen)).contiguous()
    dy = torch.randn(rows, N * C, generator=gen)
    wn = torch.ones(rows)
    g = ops_fused.catvae_gumbels(rows, 1, N, C, SEED, STEP, gcat.TAG_TRAIN).cpu().double().numpy()
    tag = "reduce N=%d C=%d rows=%d" % (N, C, rows)
    for tau in TAUS:
        for hard in (False, True):
            ref = R.rows_reference(l, g, N, C, 1, tau, dy=dy, hard=hard)
            f32 = R.rows_reference(l, g, N, C, 1, tau, torch.float32, dy=dy, hard=hard)
            dl = run_reduce(l, dy, wn, rows, N, C, tau)
            assert torch.equal(dl, run_reduce(l, dy, wn, rows, N, C, tau))
            check("%s tau=%g %s" % (tag, tau, "ST" if hard else "RELAXED"), "dlogits", dl.numpy(), ref["dlogits"],
                  f32["dlogits"])
    # a weight other than 1 scales the KL part alone
    wn2 = torch.rand(rows, generator=gen) + 0.5
    ref = R.rows_reference(l, g, N, C, 1, 0.5, dy=dy, wn=wn2)
    f32 = R.rows_reference(l, g, N, C, 1, 0.5, torch.float32, dy=dy, wn=wn2)
    check(tag + " wn", "dlogits", run_reduce(l, dy, wn2, rows, N, C, 0.5).numpy(), ref["dlogits"], f32["dlogits"])


def test_backward_y_has_the_forwards_bits():
    """With dy = the unit vector of class c0 of every variable, da_c = y_c ([c = c0] - y_c0); with wn = 0 the KL part is
    gone and tau = 1 leaves dl = da: from the forward's y these are one multiply and one subtract in fp32, so equality
    to 2 ulp of y says the backward rebuilt the same y, noise included."""
    N, C, k, B = 20, 10, 1, 130
    l, g, _ = row_inputs(N, C, k, B)
    y, _, _, _ = run_sample(l, B, 1, N, C, CAT_RELAXED, tau=1.0)
    dy = torch.zeros(B, N, C)
    dy[:, :, 3] = 1.0
    dl = run_reduce(l, dy.view(B, N * C), torch.zeros(B), B, N, C, 1.0).view(B, N, C)
    yv = y.view(B, N, C)
    exp = yv * (dy - yv[:, :, 3:4])
    assert (dl - exp).abs().max().item() <= 4 * 2.0 ** -24
    assert torch.equal(dl[:, :, 0], yv[:, :, 0] * (0.0 - yv[:, :, 3]))      # y_0 * (0 - ydy) with ydy = y_3 exactly


def test_reduce_does_not_depend_on_where_a_row_lands():
    """The noise row is the batch position, so the same image at another position draws other noise; the test needs
    logits whose y does not depend on the noise.  g lies in [-2.8, 16.7], so with one class at +60 and the others at -60
    the runner-up's exponent is at most -(120 - 19.5) / tau: at tau = 0.5 that is below -200 and exp() is 0 in fp32
    (the smallest subnormal is exp(-103.3)), y is exactly one-hot and da exactly 0.  Rotating the batch by 3 rows moves
    every image to other lanes and most to another workgroup; dlogits must rotate bitwise.  Part 2 keeps the KL part
    alive: the top class at 0 and the others at -60 (q = exp(-60) = 8.8e-27 is a normal fp32 number), tau = 0.25, so that
    y is still exactly one-hot and dlogits is the KL part alone -- non-zero, noise-free, and compared with fp64."""
    N, C, B, sh = 20, 10, 130, 3
    gen = torch.Generator().manual_seed(3)
    top = torch.randint(0, C, (B, N), generator=gen)
    dy = torch.randn(B, N * C, generator=gen)
    wn = torch.ones(B)
    for hi, lo, tau in ((60.0, -60.0, 0.5), (0.0, -60.0, 0.25)):
        l = torch.full((B, N, C), lo)
        l.scatter_(2, top[..., None], hi)
        l = l.view(B, N * C)
        a = run_reduce(l, dy, wn, B, N, C, tau)
        b = run_reduce(torch.roll(l, sh, 0), torch.roll(dy, sh, 0), wn, B, N, C, tau)
        assert torch.equal(torch.roll(a, sh, 0), b)
        g = ops_fused.catvae_gumbels(B, 1, N, C, SEED, STEP, gcat.TAG_TRAIN).cpu().double().numpy()
        # the contract's closed form is the reference here: autograd reaches these 1e-24 values as differences of O(1)
        # terms, which float64 cannot hold (tests/test_catvae_cpu.py checks the two against each other at ordinary scales)
        ref = R.dlogits_closed(l, g, N, C, tau, dy)
        f32 = R.dlogits_closed(l, g, N, C, tau, dy, dtype=torch.float32)
        if hi == 0.0:
            assert a.abs().max().item() > 1e-26 and torch.count_nonzero(a) == a.numel()     # the KL part is there
            check("rotation, KL part", "dlogits", a.numpy(), ref, f32)
        else:
            assert np.abs(ref).max() < 1e-40 and a.abs().max().item() < 1e-40
    # the forward: lp and kl of a row keep their bits wherever the row lands (ST: the noise decides only the one-hot)
    l = torch.randn(B, N * C, generator=gen) * 1.5
    _, lp, kl, _ = run_sample(l, B, 1, N, C, CAT_ST)
    _, lp2, kl2, _ = run_sample(torch.roll(l, sh, 0), B, 1, N, C, CAT_ST)
    assert torch.equal(torch.roll(lp, sh, 0), lp2) and torch.equal(torch.roll(kl, sh, 0), kl2)


@pytest.mark.parametrize("N,C,k,B", [(3, 5, 3, 7), (20, 10, 1, 130)])
def test_extreme_logits_stay_finite(N, C, k, B):
    gen = torch.Generator().manual_seed(11)
    l = torch.where(torch.rand(B, N * C, generator=gen) < 0.5, -60.0, 60.0)
    l[0] = 60.0                                                 # a row of all-equal extremes too
    g = ops_fused.catvae_gumbels(B, k, N, C, SEED, STEP, gcat.TAG_TRAIN).cpu().double().numpy()
    for tau in TAUS:
        ref = R.rows_reference(l, g, N, C, k, tau)
        f32 = R.rows_reference(l, g, N, C, k, tau, torch.float32)
        y, lp, kl, _ = run_sample(l, B, k, N, C, CAT_RELAXED, tau=tau)
        for t in (y, lp, kl):
            assert torch.isfinite(t).all()
        tag = "extreme N=%d C=%d tau=%g" % (N, C, tau)
        check(tag, "y", y.numpy(), ref["y"], f32["y"])
        check(tag, "lp", lp.numpy(), ref["lp"], f32["lp"])
        check(tag, "kl", kl.numpy(), ref["kl"], f32["kl"])
    for mode in (CAT_ST, CAT_DISCRETE):
        y, lp, kl, codes = run_sample(l, B, k, N, C, mode)
        assert torch.isfinite(y).all() and torch.isfinite(lp).all()
    rows = B * k
    lr = l.repeat_interleave(k, 0).contiguous()
    dy = torch.randn(rows, N * C, generator=gen)
    g1 = ops_fused.catvae_gumbels(rows, 1, N, C, SEED, STEP, gcat.TAG_TRAIN).cpu().double().numpy()
    for tau in TAUS:
        ref = R.rows_reference(lr, g1, N, C, 1, tau, dy=dy)
        f32 = R.rows_reference(lr, g1, N, C, 1, tau, torch.float32, dy=dy)
        dl = run_reduce(lr, dy, torch.ones(rows), rows, N, C, tau)
        assert torch.isfinite(dl).all()
        check("extreme N=%d C=%d tau=%g" % (N, C, tau), "dlogits", dl.numpy(), ref["dlogits"], f32["dlogits"])


# ---- the engine against fp64 training -----------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, I, seed=7):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


def make_model(I, H, N, C, seed=1234, scale=1.0):
    """CatVAE under a fixed seed; `scale` widens the logits layer so that the posterior is not nearly uniform."""
    torch.manual_seed(seed)
    m = cat_vae.CatVAE(I, H, N, C)
    with torch.no_grad():
        m.encoder.logits.weight.mul_(scale)
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


ANNEAL = dict(tau0=1.0, tau_min=0.5, anneal_rate=0.4)        # 1, 0.67, then the floor from batch 2 on


@pytest.mark.parametrize("I,H,N,C,batch,n_train", [(49, 32, 3, 5, 16, 89), (784, 400, 20, 10, 512, 1536)])
def test_engine_vs_fp64_training(I, H, N, C, batch, n_train):
    """One epoch on the fused engine (6 batches of 16 with a ragged last one of 9, or 3 of 512) against Adam on the fp64
    reference's gradients, batch by batch on the device's own noise and the temperatures the engine uploaded: losses, KL
    sums, every parameter.  The fp32 yardstick is the same loop with float32 arithmetic, parameters and moments."""
    its = loaders(batch, n_train, batch, 16, I)
    m, P = make_model(I, H, N, C, scale=4.0)
    tr = cat_vae.CatVAETrainer(m, *its, seed=3)
    st = torch.get_rng_state()
    quiet(tr.train, 1, **ANNEAL)
    assert type(tr._engine).__name__ == "CatVAEEngine"
    nb = (n_train + batch - 1) // batch
    assert len(tr.losses) == len(tr.kl_loss) == nb and tr.noise_steps == nb
    taus = [cat_vae.temperature(t, **ANNEAL) for t in range(nb)]
    assert tr._engine.tau_tab.cpu().tolist() == taus and taus[0] == 1.0 and taus[1] < 1.0 and taus[-1] == 0.5
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].double().numpy()
    batches = [x[i:i + batch] for i in range(0, n_train, batch)]
    g_of = lambda t, b: ops_fused.catvae_gumbels(b, 1, N, C, 3, t, gcat.TAG_TRAIN).cpu().double().numpy()
    Pr, Lr, Kr, _ = R.train_reference(P, batches, g_of, N, C, taus, 1e-3, 1e-5)
    P32, L32, K32, _ = R.train_reference(P, batches, g_of, N, C, taus, 1e-3, 1e-5, dtype=torch.float32)
    tag = "engine %s" % ((I, H, N, C),)
    assert min(Kr) > 1e-3 * batch / 16                                     # the KL term is live
    for t in range(nb):
        for name, got, ref, f32 in (("loss", tr.losses, Lr, L32), ("kl", tr.kl_loss, Kr, K32)):
            check(tag, "%s[%d]" % (name, t), got[t], ref[t], f32[t], T_LOSS)
    got = {n: v.detach().cpu().double().numpy() for n, v in m.state_dict().items()}
    for n in R.KEYS:                                                      # test_gpu_iwae.py's absolute weight bound
        assert np.abs(Pr[n] - P[n]).max() > 1e-4                          # it trained
        err, tol = np.abs(got[n] - Pr[n]).max(), max(T_PARAM, 4 * np.abs(P32[n] - Pr[n]).max())
        print("%s %s: err %.3g allowed %.3g" % (tag, n, err, tol))
        assert err <= tol, (n, err, tol)


@pytest.mark.parametrize("hard", [False, True])
def test_one_fused_batch_gradients_vs_fp64(hard):
    """One batch with Adam's lr = 0 (the parameters stay, the gradients land in the flat gradient buffer): loss, KL and
    the eight gradients against autograd on the fp64 reference; then the validation batch of the same call (the
    straight-through forward on the evaluation stream)."""
    I, H, N, C, b = 130, 24, 6, 5, 17
    its = loaders(b, b, b, 16, I)
    m, P = make_model(I, H, N, C, scale=4.0)
    tr = cat_vae.CatVAETrainer(m, *its, seed=3, hard=hard)
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=0.0, weight_decay=0.0, tau0=0.7, tau_min=0.5, anneal_rate=0.0)
    for n, v in m.state_dict().items():
        assert np.array_equal(v.cpu().double().numpy(), P[n]), n          # lr = 0: nothing moved
    torch.set_rng_state(st)
    x = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    xv = its[1].dataset.tensors[0][trainers._epoch_order(its[1])].double().numpy()
    g = ops_fused.catvae_gumbels(b, 1, N, C, 3, 0, gcat.TAG_TRAIN).cpu().double().numpy()
    tau = cat_vae.temperature(0, 0.7, 0.5, 0.0)
    mode = "hard" if hard else "relaxed"
    ref, f32 = R.model_reference(P, x, g, N, C, tau, mode), R.model_reference(P, x, g, N, C, tau, mode, torch.float32)
    print("batch %s: min gap %.3g" % (mode, ref["min_gap"]))
    if hard:
        assert ref["min_gap"] >= MIN_GAP
    check("batch " + mode, "loss", tr.losses[0], ref["loss"], f32["loss"], T_LOSS)
    check("batch " + mode, "kl", tr.kl_loss[0], ref["kl"], f32["kl"], T_LOSS)
    got = engine_views(tr, "grad")
    assert sorted(got) == sorted(R.KEYS)
    for n in R.KEYS:
        check("batch " + mode, n, got[n].numpy(), ref["grads"][n], f32["grads"][n])
    # validation: the ST forward on (seed, step 0, the evaluation tag)
    gv = ops_fused.catvae_gumbels(b, 1, N, C, 3, 0, gcat.TAG_EVAL).cpu().double().numpy()
    rv, rv32 = R.model_reference(P, xv, gv, N, C, 1.0, "eval"), R.model_reference(P, xv, gv, N, C, 1.0, "eval", torch.float32)
    print("validation: min gap %.3g" % rv["min_gap"])
    assert rv["min_gap"] >= MIN_GAP
    check("validation", "loss", tr.best_val_loss, rv["loss"], rv32["loss"], T_LOSS)


# ---- determinism ----------------------------------------------------------------------------------------------------------
def _trained_small(seed=0, hard=False, epochs=1, cls=None, use_graph=True, n_train=96, I=64, H=48, N=4, C=6, batch=32,
                   its=None, **tkw):
    its = its or loaders(batch, n_train, 48, 48, I)
    m, _ = make_model(I, H, N, C, scale=4.0)
    tr = (cls or cat_vae.CatVAETrainer)(m, *its, seed=seed, hard=hard)
    tr.use_graph = use_graph
    quiet(tr.train, epochs, **(tkw or dict(tau0=1.0, tau_min=0.5, anneal_rate=0.05)))
    return tr, m, its


def snapshot(tr, m):
    return (list(tr.losses), list(tr.kl_loss), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state())


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert torch.equal(a[4], b[4])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("hard", [False, True])
def test_bitwise_reproducibility_graph_eager_and_resume(tmp_path, hard):
    cfg = dict(n_train=300, batch=64, hard=hard)            # 300 rows, bs 64: four full batches and one of 44
    runs = []
    for use_graph in (True, True, False):                   # graph twice, then eager
        torch.manual_seed(99)
        tr, m, _ = _trained_small(epochs=3, use_graph=use_graph, **cfg)
        runs.append(snapshot(tr, m))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    assert len(runs[0][0]) == 15 and all(math.isfinite(v) for v in runs[0][0] + runs[0][1])
    # 2 epochs + checkpoint + a fresh trainer's resumed epoch == 3 epochs (the temperature follows noise_steps)
    torch.manual_seed(99)
    tr, m, its = _trained_small(epochs=2, **cfg)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    conf = ck["optim"]["config"]
    assert (conf["num_vars"], conf["num_classes"], conf["seed"], conf["hard"]) == (4, 6, 0, hard)
    assert (conf["tau0"], conf["tau_min"], conf["anneal_rate"]) == (1.0, 0.5, 0.05)
    assert ck["history"]["noise_steps"] == 10 and "encoder.logits.weight" in ck["model"]
    new = lambda **kw: cat_vae.CatVAETrainer(cat_vae.CatVAE(64, 48, 4, 6).to(DEV), *its,
                                             **dict(dict(seed=0, hard=hard), **kw))
    tr2 = new()
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 10 and tr2.losses == runs[0][0][:10] and tr2.kl_loss == runs[0][1][:10]
    quiet(tr2.train, 1, tau0=1.0, tau_min=0.5, anneal_rate=0.05)
    same(snapshot(tr2, tr2.model), runs[0])
    # other settings: refused under strict, taken otherwise
    ck["optim"]["config"]["num_classes"] = 7
    other = str(tmp_path / "ck7.pt")
    torch.save(ck, other)
    good = dict(tau0=1.0, tau_min=0.5, anneal_rate=0.05)
    for p, kw, tkw in ((other, {}, good), (path, dict(seed=1), good), (path, dict(hard=not hard), good),
                       (path, {}, dict(good, tau0=0.9)), (path, {}, dict(good, tau_min=0.4)),
                       (path, {}, dict(good, anneal_rate=0.0))):
        t3 = new(**kw)
        t3.load_checkpoint(p)
        with pytest.raises(GMError):
            t3.train(1, **tkw)
    t3 = new()
    t3.load_checkpoint(other, strict=False)
    quiet(t3.train, 1, **good)


# ---- paths ------------------------------------------------------------------------------------------------------------------
class Mine(cat_vae.CatVAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_general_path_agrees_with_the_fused_run(monkeypatch):
    """test_gpu_nfvae.py's bounds: parameters within 5e-5; losses and the moments within 1e-4 of their max-abs."""
    made = []

    class Keep(trainers.FlatAdam):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(giwae, "FlatAdam", Keep)
    out = []
    for cls in (cat_vae.CatVAETrainer, Mine):
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
    for u, v in zip(a.losses + a.kl_loss + [a.best_val_loss], b.losses + b.kl_loss + [b.best_val_loss]):
        assert abs(u - v) <= 1e-4 * max(1.0, abs(v)), (u, v)
    opt = made[0]
    for what, flat in (("m", opt.m), ("v", opt.v)):
        fused = engine_views(a, what)
        for (n, p), o in zip(b.model.named_parameters(), opt.offs):
            err = scaled_err(flat[o:o + p.numel()].cpu().numpy(), fused[n].reshape(-1).numpy())
            print("general path %s of %s: %.3g" % (what, n, err))
            assert err <= 1e-4, (what, n, err)
    # hard=True on the general path: it runs and stays finite
    torch.manual_seed(99)
    tr, m, _ = _trained_small(cls=Mine, hard=True, n_train=64, batch=32)
    assert tr._engine is None and len(tr.losses) == 2 and all(math.isfinite(v) for v in tr.losses + tr.kl_loss)
    # C above the fused limit: the general path, same interface
    torch.manual_seed(99)
    tr, m, _ = _trained_small(N=2, C=65, n_train=64, batch=32)
    assert tr._engine is None and len(tr.losses) == 2 and all(math.isfinite(v) for v in tr.losses + tr.kl_loss)
    assert math.isfinite(tr.best_val_loss)


# ---- posterior_codes and log_likelihood ---------------------------------------------------------------------------------
def test_posterior_codes_and_log_likelihood():
    I, H, N, C, n, k = 130, 24, 6, 5, 17, 130               # 130 samples: chunks of 64, 64 and 2
    its = loaders(16, 32, 16, n, I)
    m, P = make_model(I, H, N, C, scale=4.0)
    tr = cat_vae.CatVAETrainer(m, *its, seed=0)
    tr.model.train()
    x = its[2].dataset.tensors[0]
    before = {k_: v.detach().cpu().clone() for k_, v in tr.model.state_dict().items()}
    torch.manual_seed(4)
    rng = torch.get_rng_state()
    res = tr.log_likelihood(k=k, seed=1)                                   # images=None: the whole test_iter
    codes, lq = tr.posterior_codes(x, k, seed=1)
    assert torch.equal(torch.get_rng_state(), rng) and tr.model.training
    for k_, v in tr.model.state_dict().items():
        assert torch.equal(v.cpu(), before[k_]), k_
    assert (res.k, res.n) == (k, n) and type(res).__name__ == "IWAEResult"
    assert codes.shape == (n, k, N) and lq.shape == (n, k) and codes.dtype == torch.int64 and lq.dtype == torch.float64
    assert int(codes.min()) >= 0 and int(codes.max()) < C
    # the codes are the fp64 arg max on the device's own noise, near-ties aside
    g = ops_fused.catvae_gumbels(n, k, N, C, 1, 0, gcat.TAG_EVAL).cpu().double().numpy()
    rc, gap = R.posterior_gaps(P, x.double().numpy(), g, N, C, k)
    keep = near_ties("posterior_codes", gap.reshape(n * k, N)).reshape(n, k, N)
    assert (codes.numpy()[keep] == rc[keep]).all()
    assert len(np.unique(codes.numpy().reshape(-1, N), axis=0)) > k          # the posterior is not a point mass
    # log q and the likelihood: the reference evaluated on the device's own codes
    ref = R.discrete_reference(P, x.double().numpy(), codes.numpy(), N, C)
    f32 = R.discrete_reference(P, x.double().numpy(), codes.numpy(), N, C, torch.float32)
    check("posterior_codes", "log_q", lq.reshape(-1).numpy(), ref["log_q"].reshape(-1), f32["log_q"].reshape(-1))
    ll = ref["L"] - 0.5 * I * math.log(math.pi)
    tol = allowance(T_LOSS, ref["L"], f32["L"]) * np.abs(ref["L"]).max()
    print("log_likelihood: mean %.6f ref %.6f allowed %.3g" % (res.ll_mean, ll.mean(), tol))
    assert abs(res.ll_mean - ll.mean()) <= tol
    assert abs(res.ll_stderr - ll.std() / math.sqrt(n)) <= tol
    assert tr.log_likelihood(x, k=k, seed=1) == res                        # bitwise: same seed, explicit images
    assert tr.log_likelihood(x, k=k, seed=2).ll_mean != res.ll_mean
    c2, lq2 = tr.posterior_codes(x, k, seed=1)
    assert torch.equal(codes, c2) and torch.equal(lq, lq2)
    with pytest.raises(GMError):
        giwae.log_likelihood(tr, x, k, 1)                                  # the encoder is not vae.py's


def test_sample_decode_and_codes():
    I, H, N, C = 64, 48, 4, 6
    its = loaders(16, 32, 16, 16, I)
    m, P = make_model(I, H, N, C, scale=4.0)
    tr = cat_vae.CatVAETrainer(m, *its, seed=0)
    rng = torch.get_rng_state()
    s = tr.sample(37, seed=5)
    assert torch.equal(torch.get_rng_state(), rng)
    assert s.shape == (37, I) and s.is_cuda and float(s.min()) >= 0.0 and float(s.max()) <= 1.0
    assert torch.equal(s, tr.sample(37, seed=5)) and not torch.equal(s, tr.sample(37, seed=6))
    cd = torch.randint(0, C, (37, N), generator=torch.Generator().manual_seed(5))
    d = tr.decode(cd)
    assert torch.equal(d, s)                                               # sample is decode of uniform codes
    z = torch.nn.functional.one_hot(cd, C).double().reshape(37, N * C)
    xr = R._decode({n: R.as_t(P[n]) for n in R.KEYS}, z).numpy()
    assert np.abs(d.cpu().double().numpy() - xr).max() <= 1e-5
    for bad in (cd[:, :3], cd.float(), cd - 1, cd + C - 1 + (cd == 0)):
        with pytest.raises(ValueError):
            tr.decode(bad)
    # codes: the arg max of the logits, variable by variable
    x = its[2].dataset.tensors[0]
    c = tr.codes(x)
    l = R._encode({n: R.as_t(P[n]) for n in R.KEYS}, x.double()).view(-1, N, C)
    top = torch.topk(l, 2, -1).values
    keep = ((top[..., 0] - top[..., 1]) >= MIN_GAP).numpy()
    assert c.shape == (16, N) and c.dtype == torch.int64 and keep.mean() >= 1 - MAX_VARS_OUT
    assert (c.numpy()[keep] == l.argmax(-1).numpy()[keep]).all()
    p = tr.parzen(n_samples=64, sigmas=[0.2], n_val=16, seed=0)
    assert math.isfinite(p.ll_mean)


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
    tr = cat_vae.CatVAETrainer(cat_vae.CatVAE(256, 128, 8, 4), *its, seed=0)
    quiet(tr.train, 5)
    assert type(tr._engine).__name__ == "CatVAEEngine"
    assert len(tr.losses) == 80 and all(math.isfinite(v) for v in tr.losses + tr.kl_loss)
    first, last = np.mean(tr.losses[:10]), np.mean(tr.losses[-10:])
    print("learning: first 10 %.3f last 10 %.3f" % (first, last))
    assert last < first
