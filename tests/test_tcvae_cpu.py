"""The beta-TCVAE without a GPU: the reference's closed-form pair coefficients against autograd, the collapse to the IWAE's
lp at alpha = beta = gamma = 1, tc = 0 at Z = 1, the package's torch composition against the reference, the module
surface and VAE checkpoints, the trainer's refusals, the C-ABI of the two new kernels and its refusals, path selection,
the data-parallel refusal and the checkpoint config's strict check."""
import ctypes
import inspect
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))
sys.path.insert(0, HERE)

import tc_vae  # noqa: E402
import tcvae_reference as R  # noqa: E402
from generative_models_amd import _lib, ops_fused  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd import tcvae as gtc  # noqa: E402

SHAPES = [(1, 2), (5, 7), (20, 65), (32, 130), (20, 512)]            # (Z, B): the GPU tests' shapes
LOG_NM = lambda B: math.log(60000 * B)


def _inputs(Z, B, overlapping=False, seed=0):
    g = torch.Generator().manual_seed(1000 * Z + B + seed)
    n = torch.randn(B, 2 * Z, generator=g, dtype=torch.float64)
    ml = 0.3 * n if overlapping else torch.cat([n[:, :Z], 0.5 * n[:, Z:] - 1.0], 1)
    return ml, torch.randn(B, Z, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("Z,B", SHAPES[:4])
@pytest.mark.parametrize("coef", [(1.0, 6.0, 1.0), (2.0, 0.5, 3.0)])
def test_closed_form_pair_coefficients_agree_with_autograd(Z, B, coef):
    ml, eps = _inputs(Z, B, overlapping=True)
    mu, lv = ml[:, :Z], ml[:, Z:]
    z = mu + eps * torch.exp(lv / 2)
    w = R.analytic_coefficients(R.pair_l(z, mu, lv), *coef)
    g = R.autograd_coefficients(z, mu, lv, *coef, LOG_NM(B))
    assert (w - g).abs().max().item() <= 1e-13 * max(1.0, w.abs().max().item())
    assert torch.equal(gtc.pair_coefficients(z, mu, lv, *coef), w)            # the package's statement of it
    if B >= 7 and coef == (2.0, 0.5, 3.0):
        assert (w < 0).any() and (w > 0).any()                               # both signs occur


@pytest.mark.parametrize("Z,B", SHAPES)
@pytest.mark.parametrize("overlapping", [False, True])
def test_unit_weights_give_the_iwaes_lp_and_one_latent_has_no_total_correlation(Z, B, overlapping):
    ml, eps = _inputs(Z, B, overlapping)
    r = R.rows_reference(ml, eps, (1.0, 1.0, 1.0), LOG_NM(B))
    lp_iwae = 0.5 * ((eps ** 2).sum(1) - torch.as_tensor(r["z"] ** 2).sum(1) + ml[:, Z:].sum(1))
    err = np.abs(r["lp"] - lp_iwae.numpy()).max()
    print("Z=%d B=%d: |lp - iwae lp| %.3g" % (Z, B, err))
    assert err <= 1e-12
    if Z == 1:
        assert np.abs(R.rows_reference(ml, eps, (1.0, 6.0, 1.0), LOG_NM(B))["terms"][:, 1]).max() <= 1e-14
    # the records are the logsumexps without the 2 pi constants
    mi, tc, dw = r["terms"].T
    L = LOG_NM(B)
    assert np.allclose(tc, r["lse_joint"] - r["lse_dim"].sum(1) + (Z - 1) * L, rtol=0, atol=1e-11)
    assert np.allclose(dw, r["lse_dim"].sum(1) - Z * L + 0.5 * (r["z"] ** 2).sum(1), rtol=0, atol=1e-11)


def _plain_model(I=12, H=16, Z=5, seed=3):
    torch.manual_seed(seed)
    m = tc_vae.TCVAE(I, H, Z)
    return m, {n: v.detach().clone().double() for n, v in m.state_dict().items()}


def test_general_path_arithmetic_equals_the_reference_on_the_cpu():
    """batch_objective is what compute_batch runs behind the encoder; fed the encoder's outputs in plain torch it must
    give the reference's loss, terms and gradients."""
    I, H, Z, B, N, coef = 12, 16, 5, 7, 60000, (2.0, 0.5, 3.0)
    _, P = _plain_model(I, H, Z)
    g = torch.Generator().manual_seed(1)
    x = torch.bernoulli(torch.full((B, I), 0.3, dtype=torch.float64), generator=g)
    eps = torch.randn(B, Z, generator=g, dtype=torch.float64)
    ref = R.model_reference(P, x, eps, coef, N)
    Q = {n: v.clone().requires_grad_() for n, v in P.items()}
    h = torch.relu(x @ Q["encoder.linear.weight"].T + Q["encoder.linear.bias"])
    mu = h @ Q["encoder.mu.weight"].T + Q["encoder.mu.bias"]
    lv = h @ Q["encoder.log_var.weight"].T + Q["encoder.log_var.bias"]
    dec = lambda z: torch.sigmoid(torch.relu(z @ Q["decoder.linear.weight"].T + Q["decoder.linear.bias"])
                                  @ Q["decoder.recon.weight"].T + Q["decoder.recon.bias"])
    loss, (mi, tc, dw, recon) = gtc.batch_objective(mu, lv, eps, x, dec, *coef, math.log(N * B))
    loss.backward()
    assert abs(loss.item() - ref["loss"]) <= 1e-11 * abs(ref["loss"])
    assert np.allclose(torch.stack([mi, tc, dw], 1).detach().numpy(), ref["terms"], rtol=0, atol=1e-11)
    assert np.allclose(recon.detach().numpy(), ref["recon"], rtol=0, atol=1e-11)
    for n in R.KEYS:
        scale = max(1.0, np.abs(ref["grads"][n]).max())
        assert np.abs(Q[n].grad.numpy() - ref["grads"][n]).max() <= 1e-11 * scale, n


def test_module_surface_and_vae_checkpoints():
    for n in ("Encoder", "Decoder", "TCVAE", "TCVAETrainer", "TCVAEError"):
        assert hasattr(tc_vae, n), n
    sig = inspect.signature(tc_vae.TCVAE.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("image_size", 784), ("hidden_dim", 400), ("z_dim", 20)]
    T = tc_vae.TCVAETrainer
    sig = inspect.signature(T.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[6:]] == [
        ("alpha", 1.0), ("beta", 6.0), ("gamma", 1.0), ("dataset_size", None), ("seed", 0)]
    assert all(p.kind is p.KEYWORD_ONLY for p in list(sig.values())[6:])
    assert issubclass(T, giwae.IWAETrainer) and T._series == (("losses", "recon"), ("tc", "kl"))
    assert T._line == "Epoch[%d/%d], Loss: %.4f, TC: %.4f, Val Loss: %.4f"
    for name in ("decomposition", "traverse", "log_likelihood", "sample", "parzen", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(T, name)), name
    assert "log_likelihood" not in T.__dict__                                 # the VAE's: q is the plain Gaussian
    assert issubclass(gtc.TCVAEError, _lib.GMError) and issubclass(gtc.TCVAEError, ValueError)
    from generative_models_amd import metrics
    assert metrics.TCResult._fields == ("mi", "tc", "dw_kl", "recon", "n")
    import generative_models_amd as pkg
    from generative_models_amd import engine, trainers
    assert pkg.TCVAE is gtc.TCVAE and pkg.TCVAETrainer is T and pkg.TCVAEEngine is engine.TCVAEEngine
    assert issubclass(engine.TCVAEEngine, engine.IWAEEngine)
    for f in ("_check_limits", "_alloc", "_second_sum", "_settings", "_sample", "_reduce"):
        assert f in engine.TCVAEEngine.__dict__, f
    assert "_issue" not in engine.TCVAEEngine.__dict__                         # the IWAE's twelve launches
    assert gtc.__doc__ and "The contract." in gtc.__doc__ and "lse_joint" in gtc.__doc__
    # a VAE's and an IWAE's state_dict load, and the same seed gives a VAE's weights
    torch.manual_seed(11)
    vae = trainers.VAE(49, 32, 5)
    torch.manual_seed(11)
    m = tc_vae.TCVAE(49, 32, 5)
    assert list(m.state_dict()) == list(R.KEYS) == list(vae.state_dict())
    for n, v in vae.state_dict().items():
        assert torch.equal(v, m.state_dict()[n]), n
    m2 = tc_vae.TCVAE(49, 32, 5)
    m2.load_state_dict(vae.state_dict())
    m2.load_state_dict(giwae.IWAE(49, 32, 5).state_dict())


@pytest.mark.parametrize("kw", [dict(alpha=-1.0), dict(beta=-0.5), dict(gamma=float("nan")), dict(beta=float("inf")),
                                dict(alpha="1"), dict(gamma=True), dict(dataset_size=0), dict(dataset_size=-3),
                                dict(dataset_size=2.5), dict(dataset_size=True), dict(seed=-1), dict(seed=1.5)])
def test_trainer_refusals(kw):
    err = gtc.TCVAEError if "seed" not in kw else _lib.GMError
    with pytest.raises(err) as ei:
        tc_vae.TCVAETrainer(tc_vae.TCVAE(16, 8, 5), None, None, None, **kw)          # before anything is touched
    assert isinstance(ei.value, ValueError) and isinstance(ei.value, _lib.GMError)


def test_new_symbols_are_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "gm_hip.h")).read()
    assert "vae_engine.TCVAEEngine._sample" in hdr and "vae_engine.TCVAEEngine._reduce" in hdr
    from generative_models_amd import _build
    assert "gm_tc.hip" in _build.SOURCES and "gm_gemm.hip" == _build.SOURCES[0]


def test_kernels_reject_null_out_of_limit_and_aliased_arguments():
    """Host arrays stand in for device ones: every call below must return before it launches anything."""
    lib = _lib.load()
    a = [np.zeros(1 << 12, dtype=np.float32) for _ in range(12)]
    p = lambda i: a[i].ctypes.data
    B, Z = 6, 5
    noise = ops_fused.iwae_noise(1, giwae.TAG_TRAIN, 1)
    nz = lambda **kw: ctypes.byref(ops_fused.iwae_noise(1, giwae.TAG_TRAIN, **dict(dict(k_total=1), **kw)))

    def sample(noise_=None, ml=p(0), ldml=2 * Z, z=p(1), ldz=Z, lp=p(2), lsej=p(3), lsed=p(4), ldd=Z, tc=p(5),
               terms=p(6), alpha=1.0, beta=6.0, gamma=1.0, log_nm=10.0, B=B, k=1, Z=Z):
        return lib.gm_tc_sample(None, noise_ if noise_ is not None else ctypes.byref(noise), ml, ldml, z, ldz, lp, lsej,
                                lsed, ldd, tc, terms, alpha, beta, gamma, log_nm, B, k, Z)

    def reduce(noise_=None, ml=p(0), ldml=2 * Z, z=p(1), ldz=Z, lsej=p(3), lsed=p(4), ldd=Z, wn=p(7), dzdec=p(8),
               lddz=Z, dml=p(9), lddml=2 * Z, alpha=1.0, beta=6.0, gamma=1.0, B=B, k=1, Z=Z):
        return lib.gm_tc_reduce(None, noise_ if noise_ is not None else ctypes.byref(noise), ml, ldml, z, ldz, lsej,
                                lsed, ldd, wn, dzdec, lddz, dml, lddml, alpha, beta, gamma, B, k, Z)

    for fn in (sample, reduce):
        for kw in (dict(B=0), dict(B=-1), dict(k=0), dict(k=2), dict(Z=0), dict(Z=33), dict(ml=None), dict(z=None),
                   dict(lsej=None), dict(lsed=None), dict(ldml=2 * Z - 1), dict(ldz=Z - 1), dict(ldd=Z - 1),
                   dict(alpha=-1.0), dict(beta=float("nan")), dict(gamma=float("inf")), dict(beta=-0.0 - 1e-3)):
            assert fn(**kw) == _lib.GM_EINVAL, (fn.__name__, kw)
            assert b"bad argument" in lib.gm_last_error()
        assert fn(noise_=ctypes.POINTER(ops_fused.IwaeNoise)()) == _lib.GM_EINVAL
        assert fn(noise_=nz(k_total=0)) == _lib.GM_EINVAL and fn(noise_=nz(j0=1)) == _lib.GM_EINVAL
    for kw in (dict(lp=None), dict(tc=None), dict(log_nm=float("nan")), dict(z=p(0)), dict(lp=p(0)), dict(lsed=p(0)),
               dict(lp=p(1)), dict(tc=p(2)), dict(lsej=p(5)), dict(terms=p(4)), dict(terms=p(0)), dict(lsed=p(1))):
        assert sample(**kw) == _lib.GM_EINVAL, kw
    for kw in (dict(wn=None), dict(dzdec=None), dict(dml=None), dict(lddz=Z - 1), dict(lddml=2 * Z - 1),
               dict(dml=p(0)), dict(dml=p(1)), dict(dml=p(3)), dict(dml=p(4)), dict(dml=p(7)), dict(dml=p(8))):
        assert reduce(**kw) == _lib.GM_EINVAL, kw
    for t in a:
        assert not t.any()                                                # nothing was written
    with pytest.raises(_lib.GMError):
        _lib.call("gm_tc_reduce", None, None, None, 0, None, 0, None, None, 0, None, None, 0, None, 0, 1.0, 1.0, 1.0,
                  1, 1, 1)


# ---- path selection and the engine's host side --------------------------------------------------------------------------
def _loaders(n=40, batch=8, side=4):
    x = torch.rand(n, 1, side, side)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, **kw):
    tr = object.__new__(cls or tc_vae.TCVAETrainer)         # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.k, tr.seed, tr.noise_steps, tr._engine = 1, 0, 0, None
    tr.alpha, tr.beta, tr.gamma, tr.dataset_size = 1.0, 6.0, 1.0, 40
    for n, v in kw.items():
        setattr(tr, n, v)
    return tr


class _Mine(tc_vae.TCVAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_path_selection():
    assert _trainer(tc_vae.TCVAE(16, 8, 5))._stock() and _trainer(tc_vae.TCVAE(16, 8, 32))._stock()
    assert _trainer(tc_vae.TCVAE(16, 8, 1))._stock()
    assert not _trainer(tc_vae.TCVAE(16, 8, 33))._stock()                          # above the kernels' Z
    assert not _trainer(tc_vae.TCVAE(16, 8, 5), cls=_Mine)._stock()                # an overridden hook
    m = tc_vae.TCVAE(16, 8, 5)
    m.encoder.extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock()                                                # an edited encoder

    class Sub(tc_vae.TCVAE):
        pass
    assert not _trainer(Sub(16, 8, 5))._stock()                                    # a subclassed model


def test_engine_refuses_data_parallelism_and_other_settings_on_resume():
    from generative_models_amd.engine import TCVAEEngine
    m = tc_vae.TCVAE(16, 8, 5)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            TCVAEEngine(m, "cpu", trainer=_trainer(m), **kw)
    tr = _trainer(m)
    tr.force_dp = True
    with pytest.raises(_lib.GMError, match="one GPU"):
        tr.train(1)
    with pytest.raises(_lib.GMError, match="general path"):
        TCVAEEngine(tc_vae.TCVAE(16, 8, 33), "cpu", trainer=_trainer(m))
    with pytest.raises(_lib.GMError, match="general path"):
        TCVAEEngine(m, "cpu", trainer=_trainer(m, k=2))
    tr = _trainer(m, seed=9, beta=4.0)
    eng = TCVAEEngine(m, "cpu", trainer=tr)
    now = eng._settings()
    assert now == {"alpha": 1.0, "beta": 4.0, "gamma": 1.0, "dataset_size": 40, "k": 1, "seed": 9}
    n = eng.fp.m.numel()
    for key, other in (("alpha", 2.0), ("beta", 6.0), ("gamma", 0.0), ("dataset_size", 41), ("seed", 0)):
        saved = dict(now, B=8, lr=1e-3, weight_decay=1e-5)
        saved[key] = other
        resume = {"m": torch.zeros(n), "v": torch.zeros(n), "step": 5, "config": saved}
        with pytest.raises(_lib.GMError, match="different settings") as ei:
            eng.configure(8, 5, 1e-3, 1e-5, resume=resume)
        assert key in str(ei.value)
    # log(N b): the trainer's dataset_size for a training batch, the pass's own dataset for a validation batch
    eng.data = torch.zeros(13, 16)
    assert eng._log_nm(8, True) == math.log(40 * 8) and eng._log_nm(5, False) == math.log(13 * 5)
