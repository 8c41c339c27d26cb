"""Importance-weighted autoencoder without a GPU: module surface and state_dict round trip with the VAE, k / seed
validation, the numpy reference (the GPU tests' oracle) against torch autograd in fp64, the noise rule's known answers,
the C-ABI of the new kernels and its refusals, fused / general path selection."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import iwae  # noqa: E402
import vae  # noqa: E402
from generative_models_amd import _lib, metrics, ops_fused  # noqa: E402
from generative_models_amd import dvae as gdvae  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402



def _loaders(n=40, batch=8, side=4):
    x = torch.bernoulli(torch.full((n, 1, side, side), 0.5))
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, k=5, seed=0):
    tr = object.__new__(cls or iwae.IWAETrainer)      # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.k, tr.seed = giwae.check_k_seed(k, seed)
    return tr


def test_module_surface_and_state_dict_round_trip_with_the_vae():
    torch.manual_seed(3)
    d = iwae.IWAE(16, 12, 4)
    torch.manual_seed(3)
    v = vae.VAE(16, 12, 4)
    assert [n for n, _ in d.named_modules()] == [n for n, _ in v.named_modules()]
    assert list(d.state_dict()) == list(v.state_dict())
    for k in v.state_dict():                                   # same construction order: same initial weights
        assert torch.equal(d.state_dict()[k], v.state_dict()[k]), k
    assert isinstance(d, vae.VAE) and iwae.Encoder is vae.Encoder and iwae.Decoder is vae.Decoder
    d2 = iwae.IWAE(16, 12, 4)
    d2.load_state_dict(v.state_dict())                         # a VAE checkpoint's weights load into an IWAE
    v2 = vae.VAE(16, 12, 4)
    v2.load_state_dict(d2.state_dict())
    assert type(d).forward is vae.VAE.forward and type(d).reparameterize is vae.VAE.reparameterize
    assert (d.image_size, d.hidden_dim, d.z_dim, d.shape) == (16, 12, 4, 4)
    for name in ("sample", "parzen", "log_likelihood", "save_checkpoint", "load_checkpoint", "sample_images",
                 "reconstruct_images"):
        assert callable(getattr(iwae.IWAETrainer, name))
    assert iwae.IWAETrainer.log_likelihood is vae.VAETrainer.log_likelihood
    sig = inspect.signature(iwae.IWAETrainer.__init__).parameters
    assert list(sig)[1:] == ["model", "train_iter", "val_iter", "test_iter", "viz", "k", "seed"]
    assert sig["k"].kind is inspect.Parameter.KEYWORD_ONLY and sig["k"].default == 5 and sig["seed"].default == 0
    sig = inspect.signature(vae.VAETrainer.log_likelihood).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("images", None), ("k", 500), ("seed", 0)]
    import generative_models_amd as pkg
    assert pkg.IWAE is giwae.IWAE and pkg.IWAETrainer is giwae.IWAETrainer
    assert pkg.IWAEEngine.__name__ == "IWAEEngine"
    assert metrics.IWAEResult._fields == ("ll_mean", "ll_stderr", "k", "n")


@pytest.mark.parametrize("bad", [dict(k=0), dict(k=-3), dict(k=2.0), dict(k="5"), dict(k=True), dict(k=None),
                                 dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(seed=False)])
def test_bad_k_or_seed_raise_before_anything_runs(bad):
    with pytest.raises(ValueError) as ei:
        iwae.IWAETrainer(None, None, None, None, **bad)          # raises before touching the model or the loaders
    assert isinstance(ei.value, _lib.GMError)
    tr = _trainer(iwae.IWAE(16, 8, 4))
    with pytest.raises(ValueError) as ei:
        tr.log_likelihood(torch.zeros(2, 16), **dict(dict(k=4, seed=0), **bad))
    assert isinstance(ei.value, _lib.GMError)
    assert giwae.check_k_seed(np.int64(7), (1 << 64) - 1) == (7, (1 << 64) - 1)


def _ptr(a):
    return ctypes.pointer(a)


def test_new_symbols_declared_bound_and_reject_bad_arguments():
    lib = _lib.load()
    E, p = _lib.GM_EINVAL, 64                                   # p: a non-null placeholder, never dereferenced here
    nz = lambda **kw: _ptr(ops_fused.iwae_noise(1, giwae.TAG_TRAIN, kw.pop("k_total", 5), **kw))
    n5 = nz()
    # gm_iwae_sample(stream, noise, ml, ldml, z, ldz, lp, B, k, Z)
    for k, Z in ((0, 4), (65, 4), (5, 33), (5, 0), (-1, 4)):
        assert lib.gm_iwae_sample(None, nz(k_total=max(k, 1)), p, 2 * max(Z, 1), 2 * p, max(Z, 1), 3 * p, 4, k, Z) == E
    for bad in ((None, 8, 2 * p, 4, 3 * p, 4, 5, 4), (p, 8, None, 4, 3 * p, 4, 5, 4), (p, 8, 2 * p, 4, None, 4, 5, 4),
                (p, 7, 2 * p, 4, 3 * p, 4, 5, 4), (p, 8, 2 * p, 3, 3 * p, 4, 5, 4), (p, 8, 2 * p, 4, 3 * p, 0, 5, 4)):
        assert lib.gm_iwae_sample(None, n5, *bad) == E, bad
    assert lib.gm_iwae_sample(None, None, p, 8, 2 * p, 4, 3 * p, 4, 5, 4) == E
    assert lib.gm_iwae_sample(None, nz(k_total=4), p, 8, 2 * p, 4, 3 * p, 4, 5, 4) == E       # k_total < k
    assert lib.gm_iwae_sample(None, nz(k_total=8, j0=4), p, 8, 2 * p, 4, 3 * p, 4, 5, 4) == E  # j0 + k > k_total
    assert lib.gm_iwae_sample(None, nz(j0=-1, k_total=9), p, 8, 2 * p, 4, 3 * p, 4, 5, 4) == E
    assert lib.gm_iwae_sample(None, nz(k_total=1 << 31), p, 8, 2 * p, 4, 3 * p, 4, 5, 4) == E  # rows past 2^32
    # gm_iwae_weights(stream, x, ldx, xr, ldr, lp, negL, ess, wn, dA, lda, ms, B, k, I)
    ok = [p, 8, 2 * p, 8, 3 * p, 4 * p, 5 * p, 6 * p, 7 * p, 8, None, 4, 5, 8]
    for i, v in ((0, None), (2, None), (4, None), (5, None), (6, None), (7, None), (1, 7), (3, 7), (9, 7), (8, p),
                 (8, 2 * p), (12, 0), (12, 65), (11, 0), (13, 0)):
        bad = list(ok)
        bad[i] = v
        assert lib.gm_iwae_weights(None, *bad) == E, (i, v)
    # gm_iwae_reduce(stream, noise, ml, ldml, wn, dzdec, lddz, dml, lddml, dZ, lddZ, B, k, Z)
    ok = [p, 8, 2 * p, 3 * p, 4, 4 * p, 8, None, 0, 4, 5, 4]
    for i, v in ((0, None), (2, None), (3, None), (5, None), (1, 7), (4, 3), (6, 7), (10, 0), (10, 65), (11, 33),
                 (11, 0), (9, 0)):
        bad = list(ok)
        bad[i] = v
        assert lib.gm_iwae_reduce(None, n5, *bad) == E, (i, v)
    bad = list(ok)
    bad[7], bad[8] = 3 * p, 4                                   # dZ may not be dzdec
    assert lib.gm_iwae_reduce(None, n5, *bad) == E
    bad[7], bad[8] = 5 * p, 3                                   # ld < Z
    assert lib.gm_iwae_reduce(None, n5, *bad) == E
    assert lib.gm_iwae_reduce(None, None, *ok) == E
    with pytest.raises(_lib.GMError):
        ops_fused.iwae_noise(1 << 64, giwae.TAG_EVAL, 5)


# ---- the numpy reference against torch autograd (fp64) -----------------------------------------------------------------
def _autograd(P, x, eps, k):
    P = {n: v.clone().requires_grad_() for n, v in P.items()}
    B = x.shape[0]
    h = F.relu(x @ P["encoder.linear.weight"].T + P["encoder.linear.bias"])
    mu = h @ P["encoder.mu.weight"].T + P["encoder.mu.bias"]
    lv = h @ P["encoder.log_var.weight"].T + P["encoder.log_var.bias"]
    e = eps.view(B, k, -1)
    z = mu[:, None] + e * torch.exp(lv / 2)[:, None]
    hd = F.relu(z @ P["decoder.linear.weight"].T + P["decoder.linear.bias"])
    xr = torch.sigmoid(hd @ P["decoder.recon.weight"].T + P["decoder.recon.bias"])
    # log p(x | z) + log p(z) - log q(z | x) with the contract's constants dropped
    logw = (-((x[:, None] - xr) ** 2).sum(-1) - 0.5 * (z ** 2).sum(-1)
            + (0.5 * ((z - mu[:, None]) / torch.exp(lv / 2)[:, None]) ** 2).sum(-1) + 0.5 * lv.sum(-1)[:, None])
    L = torch.logsumexp(logw, 1) - math.log(k)
    (-L.sum()).backward()
    return L.detach(), logw.detach(), {n: v.grad for n, v in P.items()}


@pytest.mark.parametrize("k", [1, 4])
def test_reference_against_fp64_autograd(k):
    torch.manual_seed(11)
    m = iwae.IWAE(7, 5, 3).double()
    with torch.no_grad():
        for p_ in m.parameters():
            p_.mul_(3.0)                                       # spread the weights: a k-sample softmax far from uniform
    P = {n: v.detach().clone() for n, v in m.state_dict().items()}
    B = 6
    x = torch.rand(B, 7, dtype=torch.float64)
    eps = giwae.iwae_noise_reference(B * k, 3, seed=5, step=2, tag=giwae.TAG_TRAIN)
    ref = giwae.iwae_reference(P, x.numpy(), eps, k)
    L, logw, grads = _autograd(P, x, torch.from_numpy(eps), k)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert rel(ref["L"], L.numpy()) <= 1e-12
    assert rel(-ref["L"].sum(), -L.sum().item()) <= 1e-12
    assert set(ref["grads"]) == set(grads) and len(grads) == 10          # 8 tensors, [mu ; log_var] under two names each
    for n, g in grads.items():
        assert rel(ref["grads"][n], g.numpy()) <= 1e-12, n
    # Jensen, exact on the same samples: L_k >= mean_j log w_j
    assert np.all(ref["L"] >= ref["logw"].mean(1) - 1e-12 * np.abs(ref["logw"]).max())
    assert np.all(ref["ess"] >= 1 - 1e-12) and np.all(ref["ess"] <= k + 1e-12)
    if k == 1:
        assert np.array_equal(ref["ess"], np.ones(B)) and np.array_equal(ref["wn"], np.ones((B, 1)))
        assert np.allclose(ref["L"], ref["logw"][:, 0], rtol=1e-15, atol=0)
    else:
        assert ref["ess"].min() < k - 1e-3                     # the weights are not uniform in this case


def test_k1_loss_is_the_vae_loss_with_a_sampled_kl():
    """At k = 1: -log w = ||x - xr||^2 + (1/2 ||z||^2 - 1/2 ||eps||^2 - 1/2 sum lv), the bracket a one-sample estimate
    of the closed-form KL; its mean over many eps agrees with the closed form."""
    torch.manual_seed(2)
    m = iwae.IWAE(7, 5, 3).double()
    P = m.state_dict()
    x = torch.rand(1, 7, dtype=torch.float64).repeat(4096, 1).numpy()
    eps = giwae.iwae_noise_reference(4096, 3, seed=0, step=0, tag=giwae.TAG_EVAL)
    ref = giwae.iwae_reference(P, x, eps, 1)
    mu, lv = ref["ml"][0, :3], ref["ml"][0, 3:]
    kl = 0.5 * (mu ** 2 + np.exp(lv) - lv - 1).sum()
    est = -ref["lp"]
    assert abs(est.mean() - kl) <= 5 * est.std() / math.sqrt(est.size)


def test_noise_reference_known_answers_and_layout():
    seed, step = 0x0123456789ABCDEF, 77
    Z, rows = 6, 3                                             # Z = 6: a partial second Philox word group
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    for tag in (giwae.TAG_TRAIN, giwae.TAG_EVAL):
        e = giwae.iwae_noise_reference(rows, Z, seed, step, tag)
        assert e.shape == (rows, Z) and e.dtype == np.float64
        for r in range(rows):
            for c in range(Z):
                w = gdvae.philox4x32_10(np.array([c >> 2, step, r, tag], np.uint64), key)
                n = gdvae.box_muller_normals(w[None, :])[0]
                assert e[r, c] == n[c & 3], (r, c)
    assert (giwae.TAG_TRAIN, giwae.TAG_EVAL) == (0x49574145, 0x49574556)
    a = giwae.iwae_noise_reference(4, 8, 1, 0, giwae.TAG_TRAIN)
    assert not np.array_equal(a, giwae.iwae_noise_reference(4, 8, 1, 0, giwae.TAG_EVAL))
    assert not np.array_equal(a, giwae.iwae_noise_reference(4, 8, 2, 0, giwae.TAG_TRAIN))
    assert not np.array_equal(a, giwae.iwae_noise_reference(4, 8, 1, 1, giwae.TAG_TRAIN))
    assert np.array_equal(a[:2], giwae.iwae_noise_reference(2, 8, 1, 0, giwae.TAG_TRAIN))     # rows are counters
    assert np.array_equal(a[:, :5], giwae.iwae_noise_reference(4, 5, 1, 0, giwae.TAG_TRAIN))  # so are latents
    assert np.array_equal(a, giwae.iwae_noise_reference(4, 8, 1, 1 << 32, giwae.TAG_TRAIN))   # step is 32 bits wide
    # Philox known answer (Random123's kat_vectors: counter 0, key 0)
    z4 = gdvae.philox4x32_10(np.zeros(4, np.uint64), np.zeros(2, np.uint64))
    assert [int(v) for v in z4] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_fused_and_general_path_selection():
    mk = lambda: iwae.IWAE(16, 8, 4)
    assert _trainer(mk())._stock()
    assert _trainer(mk(), k=64)._stock() and not _trainer(mk(), k=65)._stock()
    assert _trainer(iwae.IWAE(16, 8, 32))._stock() and not _trainer(iwae.IWAE(16, 8, 33))._stock()

    class Mine(iwae.IWAETrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    assert not _trainer(mk(), Mine)._stock()
    tr = _trainer(mk())
    tr.evaluate = lambda it: 0.0                               # an instance attribute overrides a hook too
    assert not tr._stock()

    class MyEnc(iwae.Encoder):
        pass
    m = mk()
    m.encoder = MyEnc(16, 8, 4)                                # a subclassed module
    assert not _trainer(m)._stock()
    m = mk()
    m.decoder.extra = nn.Linear(2, 2)                          # an edited network
    assert not _trainer(m)._stock()

    class MyIWAE(iwae.IWAE):
        pass
    assert not _trainer(MyIWAE(16, 8, 4))._stock()
    from generative_models_amd.engine import IWAEEngine
    tr = _trainer(mk())
    assert tr._engine_class() is IWAEEngine and tr._engine_kwargs() == {"trainer": tr}


def test_data_parallelism_and_out_of_scope_models_are_refused():
    from generative_models_amd.engine import IWAEEngine
    tr = _trainer(iwae.IWAE(16, 8, 4))
    with pytest.raises(_lib.GMError):
        IWAEEngine(tr.model, "cpu", world_size=2, rank=0, trainer=tr)
    with pytest.raises(_lib.GMError):
        IWAEEngine(tr.model, "cpu", force_dp=True, trainer=tr)
    tr.force_dp = True
    tr._engine = None
    with pytest.raises(_lib.GMError):
        tr.train(1)
    # log_likelihood: vae.py's Encoder and Decoder only -- refused with a reason before anything runs
    import aae
    import cvae
    for mod, cls, model in ((cvae, cvae.CVAETrainer, cvae.CVAE(16, 8, 4, 3)), (aae, aae.AAETrainer, aae.AAE(16, 8, 4))):
        t = object.__new__(cls)
        t.model = model
        with pytest.raises(_lib.GMError, match="Encoder and Decoder"):
            t.log_likelihood(torch.zeros(2, 16), k=4)
