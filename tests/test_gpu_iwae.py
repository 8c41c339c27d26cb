"""Importance-weighted autoencoder on the MI355X: the three kernels against the numpy contract (iwae.iwae_reference), one
fused training batch against fp64 on the device's own eps, k = 1 / expectation / Jensen properties, determinism (run to
run, graph against eager, resume), the general path, log_likelihood and a learning check.

Bounds.  Where test_gpu_dvae.py has a bound for the same comparison it is used: 4e-6 of the normal's scale for the
drawn values, 1e-5 relative for loss sums, 1.5e-6 of a tensor's max-abs for gradients, 5e-5 for parameters of the
fused against the general path.  A softmax over k samples of log w ~ -100 .. -300 amplifies the fp32 rounding of the
784-term squared errors (an absolute error d in log w is a relative error d in every weight), so those comparisons take
max(that bound, 4 x the deviation of a plain-torch fp32 CPU run of the same batch from the fp64 reference), per tensor
and scaled by its max-abs: measured inside the test, never chosen (`fp32_allowance`)."""
import contextlib
import io
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import aae  # noqa: E402
import cvae  # noqa: E402
import dvae  # noqa: E402
import iwae  # noqa: E402
import vae  # noqa: E402
from generative_models_amd import ops_fused, trainers  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
T_NORMAL, T_LOSS, T_GRAD, T_PARAM = 4e-6, 1e-5, 1.5e-6, 5e-5         # test_gpu_dvae.py's bounds (module docstring)
NAMES = ("encoder.linear.weight", "encoder.linear.bias", "encoder.mu.weight", "encoder.mu.bias",
         "encoder.log_var.weight", "encoder.log_var.bias", "decoder.linear.weight", "decoder.linear.bias",
         "decoder.recon.weight", "decoder.recon.bias")


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


def torch_iwae(P, x, eps, k, dtype):
    """The contract in plain torch on the CPU in `dtype` (autograd for the gradients): dict of L, ess, wn, dA, dml and
    the ten gradients -- the fp32 run of this is the yardstick of `fp32_allowance`."""
    P = {n: torch.as_tensor(np.asarray(v), dtype=dtype).clone().requires_grad_() for n, v in P.items()}
    x = torch.as_tensor(np.asarray(x), dtype=dtype)
    B = x.shape[0]
    e = torch.as_tensor(np.asarray(eps), dtype=dtype).view(B, k, -1)
    h = F.relu(x @ P["encoder.linear.weight"].T + P["encoder.linear.bias"])
    mu = h @ P["encoder.mu.weight"].T + P["encoder.mu.bias"]
    lv = h @ P["encoder.log_var.weight"].T + P["encoder.log_var.bias"]
    ml = torch.cat([mu, lv], 1)
    ml.retain_grad()
    z = ml[:, None, :e.shape[2]] + e * torch.exp(ml[:, None, e.shape[2]:] / 2)
    hd = F.relu(z @ P["decoder.linear.weight"].T + P["decoder.linear.bias"])
    a = hd @ P["decoder.recon.weight"].T + P["decoder.recon.bias"]
    a.retain_grad()
    xr = torch.sigmoid(a)
    logw = (-((x[:, None] - xr) ** 2).sum(-1) - 0.5 * (z ** 2).sum(-1) + 0.5 * (e ** 2).sum(-1)
            + 0.5 * ml[:, e.shape[2]:].sum(-1)[:, None])
    L = torch.logsumexp(logw, 1) - math.log(k)
    (-L.sum()).backward()
    wn = torch.softmax(logw.detach(), 1)
    out = {"L": L.detach(), "ess": 1.0 / (wn ** 2).sum(1), "wn": wn, "dA": a.grad.reshape(B * k, -1), "dml": ml.grad,
           "xr": xr.detach().reshape(B * k, -1)}
    out.update({n: v.grad for n, v in P.items()})
    return {n: v.double().numpy() for n, v in out.items()}


def fp32_allowance(base, ref, f32, name):
    """max(base, 4 x the fp32 CPU run's deviation from the fp64 reference), in units of the tensor's max-abs."""
    return max(base, 4.0 * scaled_err(f32[name], ref))


def model_params(I, H, Z, seed=1234, gain=1.0):
    torch.manual_seed(seed)
    m = iwae.IWAE(I, H, Z)
    if gain != 1.0:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(gain)
    return m, {n: v.detach().clone().double().numpy() for n, v in m.state_dict().items()}


# ---- kernels against the reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("B,k,Z", [(17, 5, 20), (64, 2, 6), (1, 64, 1), (3, 1, 32)])
def test_sample_vs_numpy_rule(B, k, Z):
    g = torch.Generator().manual_seed(B * 100 + k)
    ml = torch.randn(B, 2 * Z, generator=g)
    ml[:, Z:] = ml[:, Z:] * 0.5 - 1.0
    seed, step, tag = 0x123456789ABCDEF, 77, giwae.TAG_TRAIN
    eps = giwae.iwae_noise_reference(B * k, Z, seed, step, tag)
    mu, lv = ml[:, :Z].double().numpy(), ml[:, Z:].double().numpy()
    sd = np.exp(lv / 2)
    zr = (np.repeat(mu, k, 0) + eps * np.repeat(sd, k, 0))
    lpr = 0.5 * ((eps ** 2).sum(1) - (zr ** 2).sum(1) + np.repeat(lv.sum(1), k))
    # test_gpu_dvae.py's gaussian bound on z, and that bound pushed through lp (+ the fp32 rounding of its Z terms)
    dz = T_NORMAL * (np.maximum(1, np.abs(zr)) + np.repeat(sd, k, 0) * np.maximum(1, np.abs(eps)))
    de = T_NORMAL * np.maximum(1, np.abs(eps))
    dlp = (np.abs(eps) * de + np.abs(zr) * dz).sum(1) + 1e-6 * (eps ** 2 + zr ** 2 + np.abs(np.repeat(lv, k, 0))).sum(1)
    mld = ml.to(DEV)

    def run(noise):
        z, lp = torch.full((B * k, Z), 7.0, device=DEV), torch.full((B * k,), 7.0, device=DEV)
        ops_fused.iwae_sample(mld, z, lp, noise, B, k, Z)
        torch.cuda.synchronize()
        return z.cpu(), lp.cpu()
    z, lp = run(ops_fused.iwae_noise(seed, tag, k, step=step))
    assert np.all(np.abs(z.double().numpy() - zr) <= dz), np.abs(z.double().numpy() - zr).max()
    assert np.all(np.abs(lp.double().numpy() - lpr) <= dlp), np.abs(lp.double().numpy() - lpr).max()
    # a device step counter plus a base against the same step given as a value; step is 32 bits wide
    ctr, base = torch.tensor([70], device=DEV), torch.tensor([4], device=DEV)
    z2, lp2 = run(ops_fused.iwae_noise(seed, tag, k, step=3, step_ctr=ctr, step_base=base))
    assert torch.equal(z2, z) and torch.equal(lp2, lp)
    z3, _ = run(ops_fused.iwae_noise(seed, tag, k, step=step + (1 << 32)))
    assert torch.equal(z3, z)
    z4, _ = run(ops_fused.iwae_noise(seed, giwae.TAG_EVAL, k, step=step))
    assert not torch.equal(z4, z)
    # chunks of a larger draw: samples j0 .. j0 + k of k_total are the rows b k_total + j0 + j
    if k > 1:
        kt = k + 3
        full = giwae.iwae_noise_reference(B * kt, Z, seed, step, tag).reshape(B, kt, Z)[:, 2:2 + k].reshape(B * k, Z)
        z5, _ = run(ops_fused.iwae_noise(seed, tag, kt, j0=2, step=step))
        zr5 = np.repeat(mu, k, 0) + full * np.repeat(sd, k, 0)
        assert np.all(np.abs(z5.double().numpy() - zr5) <= T_NORMAL * (np.maximum(1, np.abs(zr5))
                      + np.repeat(sd, k, 0) * np.maximum(1, np.abs(full))))
    # iwae_normals (the general path's eps) is the same stream
    e = ops_fused.iwae_normals(B, k, Z, seed, step, tag).cpu().double().numpy()
    assert np.all(np.abs(e - eps) <= T_NORMAL * np.maximum(1, np.abs(eps)))


def _weights(x, xr, lp, B, k, train=True):
    I = x.shape[1]
    negL, ess, wn = (torch.full((n,), 7.0, device=DEV) for n in (B, B, B * k))
    dA = torch.full((B * k, I), 7.0, device=DEV) if train else None
    ms = torch.full((B, 2), 7.0, device=DEV)
    ops_fused.iwae_weights(x, xr, lp, negL, ess, wn, B, k, dA=dA, ms=ms)
    torch.cuda.synchronize()
    c = lambda t: None if t is None else t.cpu().double().numpy()
    return c(negL), c(ess), c(wn).reshape(B, k), c(dA), c(ms)


def _weights_reference(x, xr, lp, B, k):
    x, xr, lp = (np.asarray(t.cpu().numpy(), dtype=np.float64) for t in (x, xr, lp))
    d = x[:, None, :] - xr.reshape(B, k, -1)
    logw = lp.reshape(B, k) - (d ** 2).sum(-1)
    m = logw.max(1, keepdims=True)
    e = np.exp(logw - m)
    wn = e / e.sum(1, keepdims=True)
    xr3 = xr.reshape(B, k, -1)
    return {"logw": logw, "L": (m + np.log(e.sum(1, keepdims=True)))[:, 0] - math.log(k), "wn": wn,
            "ess": 1 / (wn ** 2).sum(1), "dA": (wn[..., None] * (-2 * d * (1 - xr3) * xr3)).reshape(B * k, -1)}


def _weights_fp32_cpu(x, xr, lp, B, k):
    x, xr, lp = x.cpu(), xr.cpu(), lp.cpu()
    xr3 = xr.view(B, k, -1)
    d = x[:, None, :] - xr3
    logw = lp.view(B, k) - (d ** 2).sum(-1)
    wn = torch.softmax(logw, 1)
    out = {"L": torch.logsumexp(logw, 1) - math.log(k), "wn": wn, "ess": 1 / (wn ** 2).sum(1),
           "dA": (wn[..., None] * (-2 * d * (1 - xr3) * xr3)).reshape(B * k, -1)}
    return {n: v.double().numpy() for n, v in out.items()}


@pytest.mark.parametrize("B,k,I", [(17, 5, 784), (64, 2, 130), (1, 64, 784), (3, 64, 130), (5, 1, 784), (2, 20, 784),
                                   (2, 21, 784)])
def test_weights_vs_reference_on_realistic_inputs(B, k, I):
    """log w about -110 .. -300 with a spread across j above 100: an unshifted softmax returns 0 / NaN here.  Covers the
    16-byte and the element-wise loads (I = 130), the rows kept in LDS (k I <= 16192 floats: k <= 20 at I = 784) and
    re-read (k = 21, 64), evaluation mode (no dA)."""
    g = torch.Generator().manual_seed(B + k + I)
    x = torch.bernoulli(torch.full((B, I), 0.3), generator=g)
    sharp = torch.linspace(0.15, 0.45, k).repeat(B)[:, None]            # per-sample reconstruction quality
    xr = (x.repeat_interleave(k, 0) * (1 - 2 * sharp) + sharp + 0.05 * (torch.rand(B * k, I, generator=g) - 0.5))
    xr = xr.clamp(1e-3, 1 - 1e-3)
    lp = -120.0 + 3.0 * torch.randn(B * k, generator=g)
    x, xr, lp = x.to(DEV), xr.to(DEV).contiguous(), lp.to(DEV)
    ref = _weights_reference(x, xr, lp, B, k)
    assert ref["logw"].max() < -104 and ref["logw"].min() > -320
    assert np.exp(ref["logw"]).astype(np.float32).max() == 0                    # the unshifted exp is 0 in fp32
    if k >= 5 and I == 784:
        assert (ref["logw"].max(1) - ref["logw"].min(1)).min() > 100            # the spread across an image's samples
    f32 = _weights_fp32_cpu(x, xr, lp, B, k)
    negL, ess, wn, dA, ms = _weights(x, xr, lp, B, k)
    for a in (negL, ess, wn, dA, ms):
        assert np.all(np.isfinite(a))
    got = {"L": -negL, "ess": ess, "wn": wn, "dA": dA}
    for n, base in (("L", T_LOSS), ("ess", T_LOSS), ("wn", T_GRAD), ("dA", T_GRAD)):
        tol, err = fp32_allowance(base, ref[n], f32, n), scaled_err(got[n], ref[n])
        print("weights B=%d k=%d I=%d %s: err %.3g allowed %.3g" % (B, k, I, n, err, tol))
        assert err <= tol, (n, err, tol)
    # (max, sum) give L back, and evaluation mode (no dA) writes the same numbers
    assert np.allclose(ms[:, 0] + np.log(ms[:, 1]) - math.log(k), -negL, rtol=1e-6, atol=1e-5)
    e = _weights(x, xr, lp, B, k, train=False)
    assert np.array_equal(e[0], negL) and np.array_equal(e[1], ess) and np.array_equal(e[2], wn)
    assert np.array_equal(e[4], ms)


@pytest.mark.parametrize("k,I", [(5, 784), (64, 130), (2, 130)])
def test_weights_dominant_and_equal_rows(k, I):
    B = 6
    g = torch.Generator().manual_seed(k)
    x = torch.bernoulli(torch.full((B, I), 0.3), generator=g)
    row = torch.rand(B, I, generator=g).clamp(0.01, 0.99)
    xr = row.repeat_interleave(k, 0).contiguous()                       # all k rows of an image equal
    lp = torch.randn(B, generator=g).repeat_interleave(k).contiguous()
    lp = lp.view(B, k).clone()
    lp[B // 2:, k - 1] += 200.0                                         # images B/2 ..: the last sample dominates
    lp = lp.view(-1)
    x, xr, lp = x.to(DEV), xr.to(DEV), lp.to(DEV)
    ref = _weights_reference(x, xr, lp, B, k)
    negL, ess, wn, dA, ms = _weights(x, xr, lp, B, k)
    h = B // 2
    assert np.array_equal(wn[:h].astype(np.float32), np.full((h, k), np.float32(1.0) / np.float32(k)))   # 1 / k exactly
    assert np.array_equal(ess[:h], np.full(h, float(k)))
    assert np.array_equal(wn[h:, k - 1], np.ones(B - h)) and np.all(wn[h:, :k - 1] == 0)
    assert np.array_equal(ess[h:], np.ones(B - h))
    f32 = _weights_fp32_cpu(x, xr, lp, B, k)
    for n, base, got in (("L", T_LOSS, -negL), ("dA", T_GRAD, dA)):
        assert scaled_err(got, ref[n]) <= fp32_allowance(base, ref[n], f32, n), n
    assert np.all(np.isfinite(dA)) and np.all(dA[h * k:].reshape(B - h, k, I)[:, :k - 1] == 0)


@pytest.mark.parametrize("B,k,Z", [(17, 5, 20), (64, 2, 6), (1, 64, 1), (3, 1, 32)])
def test_reduce_vs_reference(B, k, Z):
    g = torch.Generator().manual_seed(B + k + Z)
    ml = torch.randn(B, 2 * Z, generator=g)
    ml[:, Z:] = ml[:, Z:] * 0.5 - 1.0
    wn = torch.softmax(3 * torch.randn(B, k, generator=g), 1).reshape(-1)
    dzdec = torch.randn(B * k, Z, generator=g)
    seed, step, tag = 9, 5, giwae.TAG_TRAIN
    nz = ops_fused.iwae_noise(seed, tag, k, step=step)
    eps = ops_fused.iwae_normals(B, k, Z, seed, step, tag).cpu().double().numpy().reshape(B, k, Z)   # the device's own
    mu, lv = ml[:, :Z].double().numpy(), ml[:, Z:].double().numpy()
    sd = np.exp(lv / 2)
    z = mu[:, None] + eps * sd[:, None]
    dz = dzdec.double().numpy().reshape(B, k, Z) + wn.double().numpy().reshape(B, k, 1) * z
    ref = np.concatenate([dz.sum(1), (dz * eps * sd[:, None]).sum(1) / 2 - 0.5], 1)
    dml, dZ = torch.full((B, 2 * Z), 7.0, device=DEV), torch.full((B * k, Z), 7.0, device=DEV)
    ops_fused.iwae_reduce(ml.to(DEV), wn.to(DEV), dzdec.to(DEV), dml, nz, B, k, Z, dZ=dZ)
    dml2 = torch.full((B, 2 * Z), 7.0, device=DEV)
    ops_fused.iwae_reduce(ml.to(DEV), wn.to(DEV), dzdec.to(DEV), dml2, nz, B, k, Z)
    torch.cuda.synchronize()
    assert torch.equal(dml, dml2)
    # fp32 sums of k terms: k rounding errors of the running sum's size, on top of test_gpu_dvae.py's gradient bound
    terms = np.concatenate([np.abs(dz).sum(1), np.abs(dz * eps * sd[:, None]).sum(1) / 2 + 0.5], 1)
    tol = T_GRAD * np.abs(ref).max() + (k + 4) * 6e-8 * terms
    assert np.all(np.abs(dml.cpu().double().numpy() - ref) <= tol), np.abs(dml.cpu().double().numpy() - ref).max()
    assert scaled_err(dZ.cpu().numpy(), dz.reshape(B * k, Z)) <= T_GRAD


# ---- one fused training batch against fp64 ------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, I, seed=7, binary=True):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g) if binary else torch.rand(n, I, generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


BATCH_CASES = [(784, 400, 20, 5, 64, True), (130, 24, 6, 2, 17, False), (130, 24, 1, 64, 1, False),
               (784, 400, 20, 1, 64, True), (130, 24, 6, 64, 17, False)]


@pytest.mark.parametrize("I,H,Z,k,b,binary", BATCH_CASES, ids=lambda v: str(int(v)))
def test_one_fused_batch_vs_fp64(I, H, Z, k, b, binary):
    """One training batch through IWAEEngine (Adam's lr = 0: the parameters stay, the gradients land in the flat
    gradient buffer): loss, ess and the ten gradients against iwae_reference in fp64 on the device's own eps.  k = 1 is
    the `loss and gradients equal the k = 1 reference` property."""
    its = loaders(b, b, b, 16, I, binary=binary)
    m, P = model_params(I, H, Z)
    tr = iwae.IWAETrainer(m, *its, k=k, seed=3)
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
    assert type(tr._engine).__name__ == "IWAEEngine"
    fp = tr._engine.fp
    got = {n: fp.gviews[[i for i, q in enumerate(fp.params) if q is p][0]].cpu().double().numpy()
           for n, p in m.named_parameters()}
    assert len(got) == 10
    for n, v in m.state_dict().items():
        assert np.array_equal(v.cpu().double().numpy(), P[n]), n          # lr = 0: nothing moved
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].reshape(b, -1).double().numpy()
    eps = ops_fused.iwae_normals(b, k, Z, 3, 0, giwae.TAG_TRAIN).cpu().double().numpy()
    ref = giwae.iwae_reference(P, x, eps, k)
    f32 = torch_iwae(P, x, eps, k, torch.float32)
    f32["loss"], f32["ess_mean"] = -f32["L"].sum(), f32["ess"].mean()
    refs = dict(ref["grads"], loss=-ref["L"].sum(), ess_mean=ref["ess"].mean())
    got.update(loss=tr.losses[0], ess_mean=tr.ess[0])
    assert len(tr.losses) == 1 and len(tr.ess) == 1 and 1 - 1e-6 <= tr.ess[0] <= k * (1 + 1e-6)
    if k == 1:
        assert tr.ess[0] == 1.0
    for n in ("loss", "ess_mean") + NAMES:
        base = T_LOSS if n in ("loss", "ess_mean") else T_GRAD
        tol, err = fp32_allowance(base, refs[n], f32, n), scaled_err(got[n], refs[n])
        print("batch %s k=%d b=%d %s: err %.3g allowed %.3g (fp32 cpu %.3g)"
              % ((I, H, Z), k, b, n, err, tol, scaled_err(f32[n], refs[n])))
        assert err <= tol, (n, err, tol)


# ---- properties ---------------------------------------------------------------------------------------------------------
def _trained_small(k=5, seed=0, epochs=1, cls=None, use_graph=True, n_train=96, I=64, H=48, Z=8, batch=32, its=None):
    its = its or loaders(batch, n_train, 48, 48, I)
    torch.manual_seed(1234)
    m = iwae.IWAE(I, H, Z)
    tr = (cls or iwae.IWAETrainer)(m, *its, k=k, seed=seed)
    tr.use_graph = use_graph
    quiet(tr.train, epochs)
    return tr, m, its


def test_expected_k1_loss_is_the_vae_loss():
    """E[loss] at k = 1 over 64 seeds against the VAE's recon + KL (64 draws of its eps) on the same weights."""
    its = loaders(32, 64, 32, 32, 64)
    torch.manual_seed(5)
    m = vae.VAE(64, 48, 8)
    tr = vae.VAETrainer(m, *its)
    x = its[2].dataset.tensors[0]
    n, I = x.shape
    mine = np.array([-(tr.log_likelihood(x, k=1, seed=s).ll_mean + 0.5 * I * math.log(math.pi)) * n for s in range(64)])
    P = {k_: v.detach().cpu().double() for k_, v in m.state_dict().items()}
    xd = x.double()
    h = F.relu(xd @ P["encoder.linear.weight"].T + P["encoder.linear.bias"])
    mu = h @ P["encoder.mu.weight"].T + P["encoder.mu.bias"]
    lv = h @ P["encoder.log_var.weight"].T + P["encoder.log_var.bias"]
    kl = torch.sum(0.5 * (mu ** 2 + torch.exp(lv) - lv - 1)).item()
    gen = torch.Generator().manual_seed(0)
    theirs = []
    for _ in range(64):
        z = mu + torch.randn(mu.shape, generator=gen).double() * torch.exp(lv / 2)
        hd = F.relu(z @ P["decoder.linear.weight"].T + P["decoder.linear.bias"])
        out = torch.sigmoid(hd @ P["decoder.recon.weight"].T + P["decoder.recon.bias"])
        theirs.append(torch.sum((xd - out) ** 2).item() + kl)
    theirs = np.array(theirs)
    se = math.sqrt(mine.var() / mine.size + theirs.var() / theirs.size)
    assert abs(mine.mean() - theirs.mean()) <= 5 * se, (mine.mean(), theirs.mean(), se)


def test_jensen_on_the_device():
    """For the same batch and noise, L_8 >= the mean of the eight single-sample log w, both from gm_iwae_weights."""
    B, k, I, Z = 17, 8, 130, 6
    m, _ = model_params(I, 24, Z, gain=2.0)
    m = m.to(DEV)
    x = torch.rand(B, I, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        mu, lv = m.encoder(x)
        ml = torch.cat([mu, lv], 1).contiguous()
        z, lp = torch.empty(B * k, Z, device=DEV), torch.empty(B * k, device=DEV)
        ops_fused.iwae_sample(ml, z, lp, ops_fused.iwae_noise(4, giwae.TAG_EVAL, k), B, k, Z)
        xr = m.decoder(z).contiguous()
    negL8, ess, _, _, _ = _weights(x, xr, lp, B, k, train=False)
    single, ess1, _, _, _ = _weights(x.repeat_interleave(k, 0).contiguous(), xr, lp, B * k, 1, train=False)
    logw = -single.reshape(B, k)
    assert np.array_equal(ess1, np.ones(B * k))
    slack = 4 * np.finfo(np.float32).eps * np.abs(logw).max()
    assert np.all(-negL8 >= logw.mean(1) - slack)
    assert np.all(-negL8 <= logw.max(1) + slack) and np.all(ess >= 1 - 1e-6) and np.all(ess <= k * (1 + 1e-6))


# ---- determinism ----------------------------------------------------------------------------------------------------------
def snapshot(tr, m):
    return (list(tr.losses), list(tr.ess), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state())


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert torch.equal(a[4], b[4])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_bitwise_reproducibility_graph_eager_and_resume(tmp_path):
    cfg = dict(k=5, n_train=300, batch=64)                  # 300 rows, bs 64: four full batches and one of 44
    runs = []
    for use_graph in (True, True, False):                   # graph twice, then eager
        torch.manual_seed(99)
        tr, m, _ = _trained_small(epochs=3, use_graph=use_graph, **cfg)
        runs.append(snapshot(tr, m))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    assert len(runs[0][0]) == 15 and all(math.isfinite(v) for v in runs[0][0] + runs[0][1])
    torch.manual_seed(99)
    tr, m, _ = _trained_small(epochs=3, seed=6, **cfg)
    assert snapshot(tr, m)[0] != runs[0][0]                 # another seed: another noise stream
    # 2 epochs + checkpoint + a fresh trainer's resumed epoch == 3 epochs
    torch.manual_seed(99)
    tr, m, its = _trained_small(epochs=2, **cfg)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    m2 = iwae.IWAE(64, 48, 8).to(DEV)
    tr2 = iwae.IWAETrainer(m2, *its, k=5, seed=0)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 2 * len(its[0]) == 10 and tr2.losses == runs[0][0][:10]
    quiet(tr2.train, 1)
    same(snapshot(tr2, m2), runs[0])
    for bad in (dict(k=4, seed=0), dict(k=5, seed=1)):      # other settings: refused under strict, taken otherwise
        t3 = iwae.IWAETrainer(iwae.IWAE(64, 48, 8).to(DEV), *its, **bad)
        t3.load_checkpoint(path)
        with pytest.raises(GMError):
            t3.train(1)
    t3 = iwae.IWAETrainer(iwae.IWAE(64, 48, 8).to(DEV), *its, k=5, seed=1)
    t3.load_checkpoint(path, strict=False)
    quiet(t3.train, 1)


def test_a_refused_resume_leaves_the_engine_as_it_was(tmp_path):
    """A trainer that has trained loads a checkpoint written under another seed: train() refuses it ("different
    settings") before anything is touched -- the engine's parameters and both Adam moments are bit for bit what they
    were before the call."""
    cfg = dict(k=2, n_train=2 * 16, I=49, H=32, Z=8, batch=16)          # two training batches
    torch.manual_seed(99)
    tr, _, its = _trained_small(seed=0, **cfg)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    t2, _, _ = _trained_small(seed=1, its=its, **cfg)
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


# ---- paths ------------------------------------------------------------------------------------------------------------------
class Mine(iwae.IWAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_general_path_agrees_with_the_fused_run():
    out = []
    for cls in (iwae.IWAETrainer, Mine):
        torch.manual_seed(99)
        tr, m, _ = _trained_small(cls=cls, n_train=96, batch=32)          # 3 batches
        assert (tr._engine is None) == (cls is Mine) and len(tr.losses) == 3 and tr.noise_steps == 3
        out.append((tr, {k: v.cpu() for k, v in m.state_dict().items()}))
    (a, wa), (b, wb) = out
    for n in wa:
        assert (wa[n] - wb[n]).abs().max().item() <= T_PARAM, n
    for u, v in zip(a.losses + a.ess + [a.best_val_loss], b.losses + b.ess + [b.best_val_loss]):
        assert abs(u - v) <= 1e-4 * max(1.0, abs(v)), (u, v)
    assert b.losses[-1] < b.losses[0]                                     # and it trains
    # k above the fused limit: the general path, same interface
    torch.manual_seed(99)
    tr, m, _ = _trained_small(k=70, n_train=64, batch=32)
    assert tr._engine is None and len(tr.losses) == 2 and all(math.isfinite(v) for v in tr.losses + tr.ess)


# ---- log_likelihood -----------------------------------------------------------------------------------------------------
def test_log_likelihood():
    I, H, Z, n, k = 130, 24, 6, 17, 128
    its = loaders(16, 32, 16, n, I, binary=False)
    m, P = model_params(I, H, Z, gain=2.0)
    tr = vae.VAETrainer(vae.VAE(I, H, Z), *its)
    tr.model.load_state_dict(m.state_dict())
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
    # two chunks of 64 against the reference over the same 128 samples (the device's own eps, rows b * 128 + j)
    eps = ops_fused.iwae_normals(n, k, Z, 1, 0, giwae.TAG_EVAL).cpu().double().numpy()
    ref = giwae.iwae_reference(P, x.double().numpy(), eps, k)
    ll = ref["L"] - 0.5 * I * math.log(math.pi)
    f32 = torch_iwae(P, x.numpy(), eps, k, torch.float32)
    tol = fp32_allowance(T_LOSS, ref["L"], f32, "L") * np.abs(ref["L"]).max()
    print("log_likelihood: mean %.6f ref %.6f allowed %.3g" % (res.ll_mean, ll.mean(), tol))
    assert abs(res.ll_mean - ll.mean()) <= tol
    assert abs(res.ll_stderr - ll.std() / math.sqrt(n)) <= tol
    again = tr.log_likelihood(x, k=k, seed=1)
    assert again == res                                                    # bitwise: same seed, explicit images
    assert tr.log_likelihood(x, k=k, seed=2).ll_mean != res.ll_mean
    # DVAE trainers have it, the label-fed / deterministic encoders refuse
    td = dvae.DVAETrainer(dvae.DVAE(I, H, Z), *its)
    td.model.load_state_dict(m.state_dict())
    assert td.log_likelihood(x, k=k, seed=1) == res
    for t in (cvae.CVAETrainer(cvae.CVAE(I, H, Z, 3), *its), aae.AAETrainer(aae.AAE(I, H, Z), *its)):
        with pytest.raises(GMError):
            t.log_likelihood(x, k=4)


# ---- learning check -----------------------------------------------------------------------------------------------------
def test_learning_on_the_synthetic_set():
    its = trainers.get_data(BATCH_SIZE=64, root=os.path.join(HERE, "no_such_dir"), n_train=6400, n_val=640, n_test=64)
    torch.manual_seed(0)
    tr = iwae.IWAETrainer(iwae.IWAE(784, 400, 20), *its, k=5, seed=0)
    tr.model.eval()
    v0 = tr.evaluate(its[1])                                               # the validation loss at initialisation
    quiet(tr.train, 3)
    assert type(tr._engine).__name__ == "IWAEEngine"
    assert len(tr.losses) == len(tr.ess) == 300 and all(math.isfinite(v) for v in tr.losses + tr.ess)
    assert math.isfinite(tr.best_val_loss) and tr.best_val_loss < v0, (tr.best_val_loss, v0)
    assert all(1 - 1e-6 <= e <= 5 * (1 + 1e-6) for e in tr.ess)
    assert np.mean(tr.losses[-100:]) < np.mean(tr.losses[:100])
