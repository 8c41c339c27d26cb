"""The IAF-VAE without a GPU: module surface and state_dict keys, the degrees and masks against maf's helpers, the fp64
reference's per-layer Jacobians (triangular in the layer's degree order; their determinants pin logdet), the contract's
closed-form backward against autograd, masked entries through optimiser steps, VAE checkpoints, the constructor's and the
trainer's refusals, the C-ABI of the new kernels and its refusals, path selection, the data-parallel
refusal and the checkpoint config's strict check."""
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

import iaf_vae  # noqa: E402
import iafvae_reference as R  # noqa: E402
from generative_models_amd import _lib, ops_fused, philox  # noqa: E402
from generative_models_amd import iafvae as giaf  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd import maf as gmaf  # noqa: E402


def _loaders(n=40, batch=8, side=4):
    x = torch.rand(n, 1, side, side)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, k=3):
    tr = object.__new__(cls or iaf_vae.IAFVAETrainer)       # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.k, tr.seed, tr.noise_steps, tr._engine = k, 0, 0, None
    return tr


def test_module_surface_and_state_dict_keys():
    assert sorted(n for n in ("Encoder", "Decoder", "IAFVAE", "IAFVAETrainer") if hasattr(iaf_vae, n)) == sorted(
        ("Encoder", "Decoder", "IAFVAE", "IAFVAETrainer"))
    m = iaf_vae.IAFVAE(49, 32, 5, 3, 12, 4)
    assert list(m.state_dict()) == list(R.enc_dec(4)[:8]) + list(R.enc_dec(4)[8:]) + list(R.flow_keys(4)) + ["flow.m_in"]
    sd = m.state_dict()
    assert [tuple(sd[n].shape) for n in R.flow_keys(4)] == [(3, 12, 5), (3, 12, 4), (3, 12), (3, 10, 12), (3, 10)]
    assert sd["flow.m_in"].dtype == torch.int32 and tuple(sd["flow.m_in"].shape) == (3, 5)
    m0 = iaf_vae.IAFVAE(49, 32, 5, 3, 12, 0)
    assert list(m0.state_dict()) == list(R.enc_dec(0)) + list(R.flow_keys(0)) + ["flow.m_in"]
    assert not hasattr(m0.encoder, "context") and "flow.U" not in m0.state_dict()
    sig = inspect.signature(iaf_vae.IAFVAE.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [
        ("image_size", 784), ("hidden_dim", 400), ("z_dim", 20), ("num_flows", 4), ("flow_hidden", 64), ("context_dim", 20)]
    T = iaf_vae.IAFVAETrainer
    sig = inspect.signature(T.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[6:]] == [("k", 1), ("seed", 0)]
    assert issubclass(T, giwae.IWAETrainer) and T._series == (("losses", "recon"), ("ess", "kl"))
    for name in ("log_likelihood", "posterior_samples", "sample", "parzen", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(T, name)), name
    assert "log_likelihood" in T.__dict__ and "posterior_samples" in T.__dict__        # its own, shadowing iwae's
    assert issubclass(giaf.IAFVAEError, _lib.GMError) and issubclass(giaf.IAFVAEError, ValueError)
    import generative_models_amd as pkg
    from generative_models_amd import engine
    assert pkg.IAFVAE is giaf.IAFVAE and pkg.IAFVAETrainer is T and pkg.IAFVAEEngine is engine.IAFVAEEngine
    assert issubclass(engine.IAFVAEEngine, engine.IWAEEngine)
    for f in ("_head", "_extra_params", "_settings", "_alloc", "_sample", "_reduce"):
        assert f in engine.IAFVAEEngine.__dict__, f
    assert giaf.__doc__ and "Forward." in giaf.__doc__ and "Backward" in giaf.__doc__
    # the initialisation: W2 = 0, b2 = [0 | 2], so a fresh flow gates with g = sigmoid(2) and shifts by 0
    assert not sd["flow.W2"].any() and not sd["flow.b2"][:, :5].any() and torch.all(sd["flow.b2"][:, 5:] == 2.0)
    z = torch.randn(6, 5)
    zk, ld = m.flow(z, torch.randn(6, 4))
    g = torch.sigmoid(torch.tensor(2.0))
    assert torch.allclose(zk, z * g ** 3, atol=1e-6) and torch.allclose(ld, torch.full((6,), 15 * float(torch.log(g))))


@pytest.mark.parametrize("Z,F,K", [(2, 4, 1), (5, 12, 2), (20, 64, 4), (32, 64, 8), (7, 10, 3)])
def test_degrees_and_masks_are_mades(Z, F, K):
    ins, m_h = giaf.degrees(Z, F, K)
    ins2, m_h2 = gmaf.degrees(Z, F, K)
    assert all(np.array_equal(a, b) for a, b in zip(ins, ins2)) and np.array_equal(m_h, m_h2) and len(ins) == K
    m_in_r, m_h_r = R.degrees(Z, F, K)
    assert np.array_equal(np.stack(ins), m_in_r) and np.array_equal(m_h, m_h_r)
    assert np.array_equal(ins[0], np.arange(1, Z + 1))
    for l in range(1, K):
        assert np.array_equal(ins[l], Z + 1 - ins[l - 1])
    fl = giaf.IAFFlow(K, Z, F, 3)
    assert np.array_equal(fl.m_in.numpy(), m_in_r)
    M1, M2 = giaf.flow_masks(fl.m_in, F)
    R1, R2 = R.masks(Z, F, K)
    assert np.array_equal(M1.numpy(), R1) and np.array_equal(M2.numpy(), R2)
    for l in range(K):
        a1, a2 = gmaf.masks(ins[l], m_h)
        assert np.array_equal(R1[l], a1) and np.array_equal(R2[l], np.concatenate([a2, a2]))
    # a fresh flow: masked entries exactly 0.0, the others drawn
    assert not fl.W1.detach().numpy()[~R1].any() and np.all(fl.W1.detach().numpy()[R1] != 0.0)
    assert not fl.W2.detach().numpy().any()


@pytest.mark.parametrize("Z,K,F,C", [(2, 1, 4, 0), (5, 2, 12, 3), (6, 3, 8, 2)])
def test_reference_jacobians_are_triangular_and_pin_logdet(Z, K, F, C):
    flow = {n: torch.as_tensor(v) for n, v in R.flow_params(K, Z, F, C, seed=3).items()}
    M1, M2 = (torch.as_tensor(m, dtype=torch.float64) for m in R.masks(Z, F, K))
    m_in, _ = R.degrees(Z, F, K)
    g = torch.Generator().manual_seed(5)
    z0 = torch.randn(1, Z, generator=g, dtype=torch.float64)
    h = torch.randn(1, C, generator=g, dtype=torch.float64) if C else None
    _, ld, _, traj = R.chain(z0, h, flow, M1, M2)
    total = torch.eye(Z, dtype=torch.float64)
    for l in range(K):
        U = flow["flow.U"][l] if C else None
        f = lambda z: R.layer(z[None], h, flow["flow.W1"][l] * M1[l], U, flow["flow.b1"][l], flow["flow.W2"][l] * M2[l],
                              flow["flow.b2"][l])[0][0]
        J = torch.autograd.functional.jacobian(f, traj[l][0])
        order = np.argsort(m_in[l])                              # position t holds the latent of degree t + 1
        Jo = J[order][:, order]
        assert torch.equal(torch.triu(Jo, 1), torch.zeros_like(Jo)), l             # d z'_i / d z_j = 0 unless deg j <= deg i
        assert Jo.abs().min() >= 0 and torch.all(torch.diagonal(Jo) > 0)
        total = J @ total
    sign, logabs = np.linalg.slogdet(total.numpy())
    assert sign > 0 and abs(logabs - float(ld)) <= 1e-10


@pytest.mark.parametrize("case", R.ROW_CASES)
def test_closed_form_backward_agrees_with_autograd(case):
    Z, K, F, C, k, B = case
    ml, flow, wn, dzdec = R.row_inputs(*case)
    eps = philox.normals(B * k, Z, 9, 5, giwae.TAG_TRAIN)
    ref = R.rows_reference(ml, eps, flow, k, wn=wn, dzdec=dzdec)
    assert ref["smax"] <= R.S_CAP and ref["move"] >= R.MIN_MOVE
    got = R.closed_form_backward(ml, eps, flow, k, wn, dzdec)
    assert sorted(got) == sorted(("dml",) + R.flow_keys(C))
    for n, v in got.items():
        err = np.abs(v - ref[n]).max()
        assert err <= 1e-10, (n, err)
    M1, M2 = R.masks(Z, F, K)
    assert not ref["flow.W1"][~M1].any() and not ref["flow.W2"][~M2].any()          # masked gradients are zero


def test_masked_entries_stay_zero_through_adam_steps_with_weight_decay():
    """The general path's arithmetic on the CPU: autograd through iaf_chain (weight * mask), Adam with L2 weight decay."""
    torch.manual_seed(3)
    Z, K, F, C = 5, 3, 12, 4
    fl = giaf.IAFFlow(K, Z, F, C)
    with torch.no_grad():
        fl.W2.copy_(torch.randn(K, 2 * Z, F) * 0.3)
        fl.apply_masks()
    M1, M2 = (m.numpy() for m in giaf.flow_masks(fl.m_in, F))
    names = ["W1", "U", "b1", "W2", "b2"]
    P = {n: getattr(fl, n).detach().double().numpy() for n in names}
    Mo, Vo = ({n: np.zeros_like(v) for n, v in P.items()} for _ in range(2))
    start = {n: v.copy() for n, v in P.items()}
    for step in range(1, 4):
        z, h = torch.randn(9, Z), torch.randn(9, C)
        zk, ld = giaf.iaf_chain(z, h, fl)
        ((zk * torch.randn(9, Z)).sum() - ld.sum()).backward()
        G = {n: getattr(fl, n).grad.double().numpy() for n in names}
        assert not G["W1"][~M1].any() and not G["W2"][~M2].any() and G["W1"][M1].any() and G["W2"][M2].any()
        P, Mo, Vo = R.adam_reference(P, G, Mo, Vo, step, 1e-3, 1e-5)
        with torch.no_grad():
            for n in names:
                getattr(fl, n).copy_(torch.as_tensor(P[n], dtype=torch.float32))
                getattr(fl, n).grad = None
        for n, M in (("W1", M1), ("W2", M2)):
            for what in (P, Mo, Vo):
                assert not what[n][~M].any(), (n, step)
            assert not getattr(fl, n).detach().numpy()[~M].any()
    assert all(np.abs(P[n] - start[n]).max() > 1e-4 for n in names)                # and everything else moved


def test_vae_checkpoint_loads_and_the_same_seed_gives_a_vaes_weights():
    from generative_models_amd import trainers
    torch.manual_seed(11)
    vae = trainers.VAE(49, 32, 5)
    torch.manual_seed(11)
    m = iaf_vae.IAFVAE(49, 32, 5, 3, 12, 4)
    for n, v in vae.state_dict().items():
        assert torch.equal(m.state_dict()[n], v), n                                 # built after: a VAE's draws come first
    torch.manual_seed(12)
    m2 = iaf_vae.IAFVAE(49, 32, 5, 2, 8, 0)
    res = m2.load_state_dict(vae.state_dict(), strict=False)
    assert not res.unexpected_keys and sorted(res.missing_keys) == sorted(list(R.flow_keys(0)) + ["flow.m_in"])
    x = torch.rand(6, 49)
    lin = torch.nn.functional.linear
    mu = lambda e: lin(torch.relu(lin(x, e.linear.weight, e.linear.bias)), e.mu.weight, e.mu.bias)
    assert torch.equal(mu(m2.encoder), mu(vae.encoder))
    with pytest.raises(RuntimeError):
        m2.load_state_dict(vae.state_dict())                                         # strict: the flow is missing


@pytest.mark.parametrize("kw", [
    dict(num_flows=0), dict(num_flows=-1), dict(num_flows=2.0), dict(num_flows=True), dict(num_flows=None),
    dict(flow_hidden=0), dict(flow_hidden=1025), dict(flow_hidden=8.0), dict(flow_hidden="8"),
    dict(context_dim=-1), dict(context_dim=1.5), dict(context_dim=False), dict(z_dim=1), dict(z_dim=0), dict(z_dim=5.0)])
def test_constructor_refusals(kw):
    args = dict(image_size=16, hidden_dim=8, z_dim=5, num_flows=2, flow_hidden=8, context_dim=3)
    args.update(kw)
    with pytest.raises(giaf.IAFVAEError):
        iaf_vae.IAFVAE(**args)
    with pytest.raises(ValueError):
        iaf_vae.IAFVAE(**args)


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=2.0), dict(k=True), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5)])
def test_trainer_refusals(kw):
    """k and seed are validated before anything runs (no loader is touched)."""
    with pytest.raises(_lib.GMError):
        iaf_vae.IAFVAETrainer(iaf_vae.IAFVAE(16, 8, 5, 2, 8, 3), None, None, None, **kw)


def test_new_symbols_are_declared_and_bound():
    assert (_lib.IAF_MIN_Z, _lib.IAF_MAX_Z, _lib.IAF_MAX_K, _lib.IAF_MIN_F, _lib.IAF_MAX_F, _lib.IAF_MAX_C) == (
        2, 32, 8, 4, 64, 32)
    from generative_models_amd import _build
    assert "gm_iaf.hip" in _build.SOURCES and "gm_gemm.hip" == _build.SOURCES[0]
    # the exported block geometry: a workgroup owns max(1, 64 // k) whole images
    assert [ops_fused.iaf_nparts(B, k) for B, k in ((7, 1), (130, 5), (16, 2), (512, 64), (512, 33), (65, 1))] == [
        1, 11, 1, 512, 512, 2]
    assert ops_fused.iaf_part_stride(32, 64, 32) == 8320 and ops_fused.iaf_part_stride(2, 4, 0) == 8 + 4 + 16 + 4


def _mk(ct, base, **kw):
    v = dict(base)
    v.update(kw)
    return ct(*[v[n] for n, _ in ct._fields_])


def test_kernels_reject_null_out_of_limit_and_aliased_arguments():
    """Host arrays stand in for device ones: every call below must return before it launches anything."""
    lib = _lib.load()
    a = [np.zeros(1 << 15, dtype=np.float32) for _ in range(24)]
    iv = np.zeros(64, dtype=np.int32)
    p = lambda i: a[i].ctypes.data
    B, k, Z, K, F, C = 4, 3, 5, 2, 8, 3
    W = 2 * Z + C
    noise = ops_fused.iwae_noise(1, giwae.TAG_TRAIN, k)
    fpb = dict(W1=p(0), U=p(1), b1=p(2), W2=p(3), b2=p(4), K=K, F=F, C=C)
    fl = lambda **kw: ctypes.byref(_mk(ops_fused.IafParams, fpb, **kw))
    nz = lambda **kw: ctypes.byref(ops_fused.iwae_noise(1, giwae.TAG_TRAIN, **dict(dict(k_total=k), **kw)))

    def sample(noise_=None, flow=None, ml=p(5), ldml=W, z=p(6), ldz=Z, lp=p(7), B=B, k=k, Z=Z):
        return lib.gm_iaf_sample(None, noise_ if noise_ is not None else ctypes.byref(noise),
                                 flow if flow is not None else fl(), ml, ldml, z, ldz, lp, B, k, Z)

    def reduce(noise_=None, flow=None, ml=p(5), ldml=W, wn=p(8), dzdec=p(9), lddz=Z, dml=p(10), lddml=W, part=p(11),
               B=B, k=k, Z=Z):
        return lib.gm_iaf_reduce(None, noise_ if noise_ is not None else ctypes.byref(noise),
                                 flow if flow is not None else fl(), ml, ldml, wn, dzdec, lddz, dml, lddml, part, B, k, Z)

    bad_flows = [dict(K=0), dict(K=9), dict(F=0), dict(F=6), dict(F=68), dict(C=-1), dict(C=33), dict(W1=None),
                 dict(U=None), dict(b1=None), dict(W2=None), dict(b2=None), dict(W2=p(0)), dict(b2=p(2)), dict(U=p(0))]
    for fn in (sample, reduce):
        for kw in bad_flows:
            assert fn(flow=fl(**kw)) == _lib.GM_EINVAL, (fn.__name__, kw)
            assert b"bad argument" in lib.gm_last_error()
        for kw in (dict(B=0), dict(k=0), dict(k=65), dict(Z=1), dict(Z=33), dict(ml=None), dict(ldml=W - 1)):
            assert fn(**kw) == _lib.GM_EINVAL, (fn.__name__, kw)
        assert fn(noise_=ctypes.POINTER(ops_fused.IwaeNoise)()) == _lib.GM_EINVAL
        assert fn(flow=ctypes.POINTER(ops_fused.IafParams)()) == _lib.GM_EINVAL
        assert fn(noise_=nz(k_total=k - 1)) == _lib.GM_EINVAL and fn(noise_=nz(j0=1)) == _lib.GM_EINVAL
    for kw in (dict(z=None), dict(lp=None), dict(ldz=Z - 1), dict(z=p(5)), dict(lp=p(5)), dict(lp=p(6)), dict(z=p(0)),
               dict(lp=p(3)), dict(ml=p(1))):
        assert sample(**kw) == _lib.GM_EINVAL, kw
    for kw in (dict(wn=None), dict(dzdec=None), dict(dml=None), dict(part=None), dict(lddz=Z - 1), dict(lddml=W - 1),
               dict(dml=p(5)), dict(dml=p(9)), dict(dml=p(8)), dict(part=p(5)), dict(part=p(9)), dict(part=p(8)),
               dict(part=p(10)), dict(dml=p(0)), dict(part=p(3)), dict(wn=p(2)), dict(dzdec=p(4))):
        assert reduce(**kw) == _lib.GM_EINVAL, kw
    # C = 0: U is ignored, NULL or not
    assert sample(flow=fl(C=0, U=None), ldml=2 * Z - 1) == _lib.GM_EINVAL

    arr = lambda idx: (ctypes.c_void_p * 5)(*[p(i) for i in idx])
    stp = dict(part=p(11), nparts=2, p=arr(range(0, 5)), g=arr(range(12, 17)), m=arr(range(17, 22)),
               v=(ctypes.c_void_p * 5)(p(22), p(23), p(5), p(6), p(7)), m_in=iv.ctypes.data, sched=p(8),
               sched_slot=_lib.NO_SLOT, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-5, K=K, Z=Z, F=F, C=C)
    assert lib.gm_iaf_step(None, None) == _lib.GM_EINVAL and b"bad argument" in lib.gm_last_error()
    part_g = arr(range(12, 17))
    part_g[3] = None
    alias_m = arr(range(17, 22))
    alias_m[2] = p(0)
    no_u = arr(range(0, 5))
    no_u[1] = None
    for kw in (dict(K=0), dict(K=9), dict(Z=1), dict(Z=33), dict(F=2), dict(F=10), dict(F=68), dict(C=-1), dict(C=33),
               dict(nparts=0), dict(part=None), dict(m_in=None), dict(sched=None), dict(g=part_g), dict(m=alias_m),
               dict(p=no_u), dict(part=p(0))):
        assert lib.gm_iaf_step(None, ctypes.byref(_mk(ops_fused.IafStepArgs, stp, **kw))) == _lib.GM_EINVAL, kw
        assert b"bad argument" in lib.gm_last_error()
    for t in a:
        assert not t.any()                                                # nothing was written
    with pytest.raises(_lib.GMError):
        _lib.call("gm_iaf_step", None, None)


class _Mine(iaf_vae.IAFVAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_path_selection():
    mk = lambda Z=5, K=2, F=8, C=3: iaf_vae.IAFVAE(16, 8, Z, K, F, C)
    assert _trainer(mk())._stock() and _trainer(mk(C=0))._stock()
    assert _trainer(mk(Z=2, K=1, F=4, C=0), k=1)._stock() and _trainer(mk(Z=32, K=8, F=64, C=32), k=64)._stock()
    assert not _trainer(mk(), cls=_Mine)._stock()                                  # an overridden hook
    for kw in (dict(Z=33), dict(K=9), dict(F=6), dict(F=68), dict(F=2), dict(C=33)):
        assert not _trainer(mk(**kw))._stock(), kw                                 # valid, outside the fused limits
    assert not _trainer(mk(), k=65)._stock()
    m = mk()
    m.encoder.extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock()                                                # an edited encoder
    m = mk(C=0)
    m.encoder.context = torch.nn.Linear(8, 3)
    assert not _trainer(m)._stock()                                                # a context the model does not declare
    m = mk()
    m.flow.W2 = torch.nn.Parameter(torch.zeros(2, 10, 9))
    assert not _trainer(m)._stock()                                                # a flow tensor of another shape
    m = mk()
    m.flow.m_in = m.flow.m_in.flip(0)
    assert not _trainer(m)._stock()                                                # another order than the degree rule's
    m = mk()
    m.norm = torch.nn.BatchNorm1d(16)
    assert not _trainer(m)._stock()                                                # another layer

    class Sub(iaf_vae.IAFVAE):
        pass
    assert not _trainer(Sub(16, 8, 5, 2, 8, 3))._stock()                           # a subclassed model


def test_data_parallel_and_sizes_are_refused_by_the_engine():
    from generative_models_amd.engine import IAFVAEEngine
    m = iaf_vae.IAFVAE(16, 8, 5, 2, 8, 3)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            IAFVAEEngine(m, "cpu", trainer=_trainer(m), **kw)
    tr = _trainer(m)
    tr.force_dp = True
    with pytest.raises(_lib.GMError, match="one GPU"):
        tr.train(1)
    m = iaf_vae.IAFVAE(16, 8, 5, 9, 8, 3)
    with pytest.raises(_lib.GMError, match="general path"):
        IAFVAEEngine(m, "cpu", trainer=_trainer(m))


def test_engine_packs_the_head_and_the_flow_and_checks_the_checkpoint_config():
    from generative_models_amd.engine import IAFVAEEngine
    m = iaf_vae.IAFVAE(16, 8, 5, 2, 8, 3)
    tr = _trainer(m, k=3)
    tr.seed = 9
    eng = IAFVAEEngine(m, "cpu", trainer=tr)
    assert tuple(eng.ML.W.shape) == (13, 8) and eng.Z == 5                          # [mu ; log_var ; context]
    assert torch.equal(eng.ML.W[10:], m.encoder.context.weight.detach())
    for q, v in zip(m.flow.tensors(), eng.Fparams):
        assert q.data_ptr() == v.data_ptr()                                        # views of the flat buffer
    e0 = IAFVAEEngine(iaf_vae.IAFVAE(16, 8, 5, 2, 8, 0), "cpu", trainer=tr)
    assert tuple(e0.ML.W.shape) == (10, 8) and e0.Fparams[1] is None
    now = eng._settings()
    assert now == {"num_flows": 2, "flow_hidden": 8, "context_dim": 3, "k": 3, "seed": 9}
    n = eng.fp.m.numel()
    for key, other in (("num_flows", 3), ("flow_hidden", 12), ("context_dim", 0), ("k", 2), ("seed", 0)):
        saved = dict(now, B=8, lr=1e-3, weight_decay=1e-5)
        saved[key] = other
        resume = {"m": torch.zeros(n), "v": torch.zeros(n), "step": 5, "config": saved}
        with pytest.raises(_lib.GMError, match="different settings") as ei:
            eng.configure(8, 5, 1e-3, 1e-5, resume=resume)
        assert key in str(ei.value)
