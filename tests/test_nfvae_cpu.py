"""The normalizing-flow VAE without a GPU: module surface and state_dict keys, a VAE's weights loading with strict=False,
constructor and argument refusals, the fp64 reference's log-determinants against the autograd Jacobian, the constraint
(s > -1, D > 0) under adversarial u, the C-ABI of the new kernels and its refusals, fused / general path
selection, the data-parallel refusal, and that NFVAETrainer.log_likelihood is not iwae.log_likelihood."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))
sys.path.insert(0, HERE)

import nf_vae  # noqa: E402
import nfvae_reference as R  # noqa: E402
import vae  # noqa: E402
from generative_models_amd import _lib, metrics, ops_fused  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd import nfvae as gnf  # noqa: E402



def _loaders(n=40, batch=8, side=4):
    x = torch.bernoulli(torch.full((n, 1, side, side), 0.5))
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, k=1):
    tr = object.__new__(cls or nf_vae.NFVAETrainer)      # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.k, tr.seed = k, 0
    return tr


def test_module_surface_and_state_dict_keys():
    m = nf_vae.NFVAE(16, 12, 5, 3)
    assert list(m.state_dict()) == list(R.KEYS)
    assert list(m.state_dict())[:10] == list(vae.VAE(16, 12, 5).state_dict())
    assert (tuple(m.flow.u.shape), tuple(m.flow.w.shape), tuple(m.flow.b.shape)) == ((3, 5), (3, 5), (3,))
    assert (m.image_size, m.hidden_dim, m.z_dim, m.num_flows, m.shape) == (16, 12, 5, 3, 4)
    assert torch.count_nonzero(m.flow.b) == 0 and 0 < m.flow.u.abs().max() < 0.06 and 0 < m.flow.w.abs().max() < 0.06
    sig = inspect.signature(nf_vae.NFVAE.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("image_size", 784), ("hidden_dim", 400),
                                                                  ("z_dim", 20), ("num_flows", 8)]
    sig = inspect.signature(nf_vae.NFVAETrainer.__init__).parameters
    assert (sig["k"].default, sig["seed"].default, sig["viz"].default) == (1, 0, False)
    assert sig["k"].kind is inspect.Parameter.KEYWORD_ONLY and sig["seed"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(nf_vae.NFVAETrainer.train).parameters
    assert (sig["lr"].default, sig["weight_decay"].default) == (1e-3, 1e-5)
    sig = inspect.signature(nf_vae.NFVAETrainer.log_likelihood).parameters
    assert (sig["images"].default, sig["k"].default, sig["seed"].default) == (None, 500, 0)
    sig = inspect.signature(nf_vae.NFVAETrainer.posterior_samples).parameters
    assert [n for n in sig][1:] == ["images", "k", "seed"] and sig["seed"].default == 0
    for name in ("sample", "parzen", "log_likelihood", "posterior_samples", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(nf_vae.NFVAETrainer, name))
    for name in ("Encoder", "Decoder", "NFVAE", "NFVAETrainer", "get_data", "to_cuda"):
        assert hasattr(nf_vae, name), name
    assert nf_vae.Encoder is vae.Encoder and nf_vae.Decoder is vae.Decoder
    assert issubclass(gnf.NFVAEError, _lib.GMError) and issubclass(gnf.NFVAEError, ValueError)
    import generative_models_amd as pkg
    from generative_models_amd.engine import IWAEEngine, NFVAEEngine
    assert pkg.NFVAE is gnf.NFVAE and pkg.NFVAETrainer is gnf.NFVAETrainer and pkg.NFVAEEngine is NFVAEEngine
    assert issubclass(NFVAEEngine, IWAEEngine) and issubclass(gnf.NFVAETrainer, giwae.IWAETrainer)
    for f in ("_sample", "_reduce", "_alloc", "_extra_params"):
        assert f in NFVAEEngine.__dict__
    assert metrics.IWAEResult._fields == ("ll_mean", "ll_stderr", "k", "n")


def test_same_seed_gives_a_vaes_weights_and_a_vae_state_dict_loads():
    torch.manual_seed(11)
    v = vae.VAE(16, 12, 5)
    torch.manual_seed(11)
    m = nf_vae.NFVAE(16, 12, 5, 4)
    for n, t in v.state_dict().items():
        assert torch.equal(m.state_dict()[n], t), n
    m2 = nf_vae.NFVAE(16, 12, 5, 4)
    flow_before = {n: t.clone() for n, t in m2.flow.state_dict().items()}
    res = m2.load_state_dict(v.state_dict(), strict=False)
    assert sorted(res.missing_keys) == sorted(R.FLOW) and not res.unexpected_keys
    for n, t in v.state_dict().items():
        assert torch.equal(m2.state_dict()[n], t), n
    for n, t in flow_before.items():
        assert torch.equal(m2.flow.state_dict()[n], t)
    with pytest.raises(RuntimeError):
        m2.load_state_dict(v.state_dict())


@pytest.mark.parametrize("bad", [0, -1, 2.0, True, None])
def test_constructor_refusals(bad):
    with pytest.raises(gnf.NFVAEError):
        nf_vae.NFVAE(16, 12, 5, num_flows=bad)
    with pytest.raises(ValueError):
        nf_vae.NFVAE(16, 12, 5, num_flows=bad)


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=1.5), dict(k=True), dict(seed=-1), dict(seed=1 << 64)])
def test_trainer_argument_refusals(kw):
    with pytest.raises(giwae.IWAEError):
        nf_vae.NFVAETrainer(nf_vae.NFVAE(16, 12, 5, 2), *_loaders(), **kw)


@pytest.mark.parametrize("Z,K", [(5, 3), (20, 8)])
def test_reference_logdet_is_the_jacobians(Z, K):
    f = R.flow_params(K, Z, 0)
    u, w, b = (torch.tensor(f[n]) for n in R.FLOW)
    z = torch.randn(6, Z, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 1.5
    zk, ld, D = R.chain(z, u, w, b)
    assert D.min() >= 0.2
    for i in range(z.shape[0]):
        J = torch.autograd.functional.jacobian(lambda v: R.chain(v[None], u, w, b)[0][0], z[i])
        sign, logabs = torch.linalg.slogdet(J)
        assert sign == 1 and abs(float(ld[i] - logabs)) <= 1e-12, (i, float(ld[i] - logabs))
    # the package's torch chain (the general path) is the same function
    zk2, ld2 = gnf.planar_chain(z, u, w, b)
    assert torch.allclose(zk2, zk, rtol=0, atol=1e-14) and torch.allclose(ld2, ld, rtol=0, atol=1e-14)


@pytest.mark.parametrize("Z,K", [(5, 3), (20, 8), (32, 32)])
def test_constraint_keeps_the_layers_invertible_for_adversarial_u(Z, K):
    """s = w . u^ > -1 and D > 0 where the raw u would give w . u far below -1.  w is drawn at the tests' input scale
    (std 0.3), so u = -5 w has w . u = -5 |w|^2 down to about -20.  (The contract's 1e-12 in the denominator and the
    underflow of softplus bound the claim from below: in float64 s falls to -1 once softplus(s0) < |s0| 1e-12 / |w|^2,
    near s0 = -25; in float32 -1 + softplus(s0) rounds to -1 below s0 = -16.6, where D = t^2.)"""
    g = torch.Generator().manual_seed(3)
    w = torch.randn(K, Z, generator=g, dtype=torch.float64) * 0.3
    z = torch.randn(64, Z, generator=g, dtype=torch.float64) * 2
    n2 = (w * w).sum(1, keepdim=True)
    for u in (-5.0 * w, -10.0 * w / n2, -20.0 * w / n2, torch.randn(K, Z, generator=g, dtype=torch.float64) * 3, -w):
        uh, s = R.u_hat(u, w)
        assert torch.all(s > -1), float(s.min())
        _, ld, D = R.chain(z, u, w, torch.zeros(K, dtype=torch.float64))
        assert torch.all(D > 0) and torch.all(torch.isfinite(ld)), float(D.min())
    assert ((w * (-10.0 * w / n2)).sum(1) + 10).abs().max() < 1e-12          # unconstrained: w . u = -10, far below -1
    assert (w * (-5.0 * w)).sum(1).min() < -1


def test_new_symbols_are_declared_and_bound():
    assert (_lib.FLOW_MAX_K, _lib.FLOW_PART_STRIDE) == (32, 68)


def _blocks():
    """Host arrays standing in for device ones: every call below must return before it launches anything."""
    a = [np.zeros(4096, dtype=np.float32) for _ in range(16)]
    p = lambda i: a[i].ctypes.data
    return a, p


def test_row_kernels_reject_null_out_of_range_and_aliased_arguments():
    lib = _lib.load()
    a, p = _blocks()
    noise = ops_fused.IwaeNoise(0, giwae.TAG_TRAIN, None, None, 0, 2, 0, 0)
    fl = ops_fused.FlowParams(p(0), p(1), p(2), 3)
    nz, fp = ctypes.byref(noise), ctypes.byref(fl)
    B, k, Z = 4, 2, 5

    def sample(nz=nz, fp=fp, ml=p(3), ldml=2 * Z, z=p(4), ldz=Z, lp=p(5), B=B, k=k, Z=Z):
        return lib.gm_flow_sample(None, nz, fp, ml, ldml, z, ldz, lp, B, k, Z)

    def reduce(nz=nz, fp=fp, ml=p(3), ldml=2 * Z, wn=p(6), dz=p(7), lddz=Z, dml=p(8), lddml=2 * Z, part=p(9), B=B, k=k,
               Z=Z):
        return lib.gm_flow_reduce(None, nz, fp, ml, ldml, wn, dz, lddz, dml, lddml, part, B, k, Z)
    bad_flows = [ops_fused.FlowParams(None, p(1), p(2), 3), ops_fused.FlowParams(p(0), None, p(2), 3),
                 ops_fused.FlowParams(p(0), p(1), None, 3), ops_fused.FlowParams(p(0), p(1), p(2), 0),
                 ops_fused.FlowParams(p(0), p(1), p(2), 33), ops_fused.FlowParams(p(0), p(0), p(2), 3),
                 ops_fused.FlowParams(p(0), p(1), p(1), 3)]
    bad_noise = [ops_fused.IwaeNoise(0, 1, None, None, 0, 1, 0, 0),       # k_total < k
                 ops_fused.IwaeNoise(0, 1, None, None, 0, 2, -1, 0), ops_fused.IwaeNoise(0, 1, None, None, 0, 2, 0, -1)]
    cases = [dict(nz=None), dict(fp=None), dict(ml=None), dict(B=0), dict(k=0), dict(k=65), dict(Z=0), dict(Z=33),
             dict(ldml=2 * Z - 1)]
    cases += [dict(fp=ctypes.byref(f)) for f in bad_flows] + [dict(nz=ctypes.byref(n)) for n in bad_noise]
    for fn, extra in ((sample, [dict(z=None), dict(lp=None), dict(ldz=Z - 1), dict(z=p(3)), dict(lp=p(3)),
                                dict(z=p(0)), dict(lp=p(2)), dict(lp=p(4))]),
                      (reduce, [dict(wn=None), dict(dz=None), dict(dml=None), dict(part=None), dict(lddz=Z - 1),
                                dict(lddml=2 * Z - 1), dict(dml=p(3)), dict(dml=p(7)), dict(part=p(8)), dict(part=p(7)),
                                dict(dml=p(1)), dict(part=p(0)), dict(part=p(9) + 4)])):
        for kw in cases + extra:
            assert fn(**kw) == _lib.GM_EINVAL, (fn.__name__, kw)
            assert b"bad argument" in lib.gm_last_error()
    for t in a:
        assert not t.any()                                               # nothing was written


def test_step_rejects_null_out_of_range_and_aliased_arguments():
    lib = _lib.load()
    a, p = _blocks()
    names = [n for n, _ in ops_fused.FlowStepArgs._fields_]

    def args(**kw):
        v = dict(part=p(0), nparts=1, u=p(1), w=p(2), b=p(3), gu=p(4), gw=p(5), gb=p(6), mu=p(7), vu=p(8), mw=p(9),
                 vw=p(10), mb=p(11), vb=p(12), sched=p(13), sched_slot=_lib.NO_SLOT, beta1=0.9, beta2=0.999, eps=1e-8,
                 weight_decay=0.0, K=3, Z=5)
        v.update(kw)
        return ops_fused.FlowStepArgs(*[v[n] for n in names])
    assert lib.gm_flow_step(None, None) == _lib.GM_EINVAL
    cases = [dict(K=0), dict(K=33), dict(Z=0), dict(Z=33), dict(nparts=0), dict(gu=None), dict(gw=None, gb=None),
             dict(part=p(0) + 4), dict(w=p(1)), dict(mu=p(8)), dict(gb=p(3)), dict(vb=p(0))]
    cases += [{n: None} for n in ("part", "u", "w", "b", "mu", "vu", "mw", "vw", "mb", "vb", "sched")]
    for kw in cases:
        assert lib.gm_flow_step(None, ctypes.byref(args(**kw))) == _lib.GM_EINVAL, kw
        assert b"bad argument" in lib.gm_last_error()
    for t in a:
        assert not t.any()
    with pytest.raises(_lib.GMError):
        _lib.call("gm_flow_step", None, None)


class _Mine(nf_vae.NFVAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


class _MyFlow(gnf.PlanarFlow):
    pass


def test_path_selection():
    assert _trainer(nf_vae.NFVAE(16, 12, 5, 3))._stock()
    assert _trainer(nf_vae.NFVAE(16, 12, 32, 32), k=64)._stock()                   # the limits themselves
    assert not _trainer(nf_vae.NFVAE(16, 12, 5, 33))._stock()                      # K above the limit
    assert not _trainer(nf_vae.NFVAE(16, 12, 33, 3))._stock()                      # Z above the limit
    assert not _trainer(nf_vae.NFVAE(16, 12, 5, 3), k=65)._stock()                 # k above the limit
    assert not _trainer(nf_vae.NFVAE(16, 12, 5, 3), cls=_Mine)._stock()            # an overridden hook
    m = nf_vae.NFVAE(16, 12, 5, 3)
    m.flow = _MyFlow(3, 5)
    assert not _trainer(m)._stock()                                                # an edited flow
    m = nf_vae.NFVAE(16, 12, 5, 3)
    m.flow.extra = torch.nn.Parameter(torch.zeros(1))
    assert not _trainer(m)._stock()
    m = nf_vae.NFVAE(16, 12, 5, 3)
    m.flow.u = torch.nn.Parameter(torch.zeros(3, 4))
    assert not _trainer(m)._stock()
    m = nf_vae.NFVAE(16, 12, 5, 3)
    m.encoder.extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock()                                                # an edited encoder

    class Sub(nf_vae.NFVAE):
        pass
    assert not _trainer(Sub(16, 12, 5, 3))._stock()                                # a subclassed model


def test_data_parallel_is_refused():
    from generative_models_amd.engine import NFVAEEngine
    m = nf_vae.NFVAE(16, 12, 5, 3)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            NFVAEEngine(m, "cpu", trainer=_trainer(m), **kw)
    tr = _trainer(m)
    tr.force_dp = True
    with pytest.raises(_lib.GMError, match="one GPU"):
        tr.train(1)


def test_log_likelihood_is_the_trainers_own():
    from generative_models_amd.trainers import VAETrainer
    own = nf_vae.NFVAETrainer.__dict__["log_likelihood"]
    assert own is not VAETrainer.__dict__["log_likelihood"] and own is not giwae.log_likelihood
    assert "log_likelihood" not in giwae.IWAETrainer.__dict__                      # the IWAE inherits the VAE's
    src = inspect.getsource(own)
    assert "flow_sample" in src and "iwae.log_likelihood(" not in src and "iwae_sample" not in src
    assert "flow_sample" in inspect.getsource(nf_vae.NFVAETrainer.posterior_samples)
    # the trap itself: iwae.log_likelihood's model check would let an NFVAE through
    from generative_models_amd.trainers import Decoder, Encoder, _stock_module
    m = nf_vae.NFVAE(16, 12, 5, 3)
    assert type(m.encoder) is Encoder and type(m.decoder) is Decoder
    assert _stock_module(m.encoder, 3) and _stock_module(m.decoder, 2)
