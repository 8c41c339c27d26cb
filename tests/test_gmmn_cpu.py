"""The GMMN without a GPU: the reference's analytic gradient against fp64 autograd, its Gram form against its direct
differences, the unbiased statistic against a double loop, the prior rule against philox.py, the module surface and an
NSGAN generator's weights, the refusals, the C-ABI of the new kernels and its refusals, the resource table's new rows,
path selection, and mmd() on every trainer that has parzen()."""
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "generative_models_amd", "src"))
sys.path.insert(0, HERE)

import gmmn  # noqa: E402
import gmmn_reference as R  # noqa: E402
from generative_models_amd import _lib, metrics, ops_fused, philox  # noqa: E402
from generative_models_amd import gmmn as gg  # noqa: E402

KERNELS = ("gmmn_prior_kernel", "mmd_norms_kernel", "mmd_pairs_kernel", "mmd_finalize_kernel", "mmd_grad_kernel")


def _rows(N, M, I, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * N + M)
    return torch.rand(N, I, generator=g, dtype=torch.float64), torch.rand(M, I, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("N,M,I", [(1, 1, 1), (5, 7, 3), (6, 4, 9), (33, 31, 50)])
@pytest.mark.parametrize("sqrt_loss", [True, False])
def test_analytic_gradient_agrees_with_autograd(N, M, I, sqrt_loss):
    X, Y = _rows(N, M, I)
    sig = [np.sqrt(I / 6.0) * f for f in (0.5, 1.0, 2.0)]
    ref = R.mmd_reference(X, Y, sig, sqrt_loss)
    loss, g = R.autograd_dX(X, Y, sig, sqrt_loss)
    assert abs(float(ref["loss"] - loss)) <= 1e-14
    assert (ref["dX"] - g).abs().max().item() <= 1e-12 * max(1.0, g.abs().max().item())
    assert torch.equal(ref["dA"], ref["dX"] * X * (1 - X))
    assert torch.equal(ref["diag_xx"], torch.full((N,), float(len(sig)), dtype=torch.float64))
    gram = R.mmd_gram(X, Y, sig, sqrt_loss, torch.float64)                # the kernels' form, same contract
    for k in ("mmd2", "loss", "r", "C", "dX", "dA", "sxx_off", "syy_off"):
        a, b = ref[k], gram[k]
        assert (a - b).abs().max().item() <= 1e-10 * max(1.0, a.abs().max().item()), k
    assert ref["mmd2"] >= 0.0                                             # the V-statistic


@pytest.mark.parametrize("N,M", [(2, 2), (3, 6), (6, 5)])
def test_unbiased_statistic_against_a_double_loop(N, M):
    X, Y = _rows(N, M, 4, seed=3)
    sig = [0.5, 1.0, 3.0]
    ref = R.mmd_reference(X, Y, sig)
    assert abs(R.unbiased_of(ref) - R.unbiased_loops(X, Y, sig)) <= 1e-13
    assert metrics.MMDResult._fields == ("mmd2", "mmd", "n_samples", "n_data")
    assert metrics.MMD_SIGMAS == gg.SIGMAS == (2.0, 5.0, 10.0, 20.0, 40.0, 80.0)
    assert metrics.MAX_SIGMAS == _lib.MMD_MAX_SIGMAS == 16


@pytest.mark.parametrize("n,Z", [(1, 1), (4, 7), (9, 20), (2, 130)])
def test_uniforms_reference_is_philox(n, Z):
    for seed, step, tag, row0 in ((0, 0, gg.TAG_T, 0), (2 ** 40 + 5, 7, gg.TAG_V, 3), (9, 0, gg.TAG_S, 1000)):
        z = gg.uniforms_reference(n, Z, seed, step, tag, row0)
        w = philox.words(n, Z, seed, step, tag, row0).astype(np.uint64)
        u = (2.0 * (w >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24      # ph_unit, exactly
        assert z.dtype == np.float32 and z.shape == (n, Z)
        assert np.array_equal(z.astype(np.float64), 2.0 * u - 1.0)                 # fmaf(2, u, -1) is exact
        assert np.abs(z).max() < 1.0
        for e in (0, Z - 1):                                                       # word e & 3 of block e >> 2, by hand
            ctr = np.array([[e >> 2, step, row0 + n - 1, tag]], dtype=np.uint64)
            key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
            word = philox.philox4x32_10(ctr, key)[0, e & 3]
            assert z[n - 1, e] == np.float32(2.0 * ((2 * (int(word) >> 9) + 1) * 2.0 ** -24) - 1.0)
    assert (gg.TAG_T, gg.TAG_V, gg.TAG_S) == (0x474D4D54, 0x474D4D56, 0x474D4D53)
    assert [t.to_bytes(4, "big") for t in (gg.TAG_T, gg.TAG_V, gg.TAG_S)] == [b"GMMT", b"GMMV", b"GMMS"]


def test_module_surface_and_an_nsgan_generators_weights():
    for n in ("Generator", "GMMN", "GMMNTrainer", "GMMNError"):
        assert hasattr(gmmn, n), n
    sig = inspect.signature(gmmn.GMMN.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("image_size", 784), ("hidden_dim", 400), ("z_dim", 20)]
    T = gmmn.GMMNTrainer
    sig = inspect.signature(T.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[6:]] == [("sigmas", None), ("sqrt_loss", True), ("seed", 0)]
    assert all(p.kind is p.KEYWORD_ONLY for p in list(sig.values())[6:])
    tp = inspect.signature(T.train).parameters
    assert (tp["lr"].default, tp["weight_decay"].default) == (1e-3, 0.0)
    from generative_models_amd import engine, trainers
    assert issubclass(T, trainers.OneLossTrainer) and T._series == (("losses", "recon"),)
    assert issubclass(gg.GMMNEngine, engine.VAEEngine) and "_issue" in gg.GMMNEngine.__dict__
    for name in ("sample", "sample_images", "parzen", "mmd", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(T, name)), name
    assert issubclass(gg.GMMNError, _lib.GMError) and issubclass(gg.GMMNError, ValueError)
    import generative_models_amd as pkg
    assert pkg.GMMN is gg.GMMN and pkg.GMMNTrainer is T and pkg.GMMNEngine is gg.GMMNEngine
    assert gg.__doc__ and "The contract." in gg.__doc__ and "r_i x_i - (C R)_i" in gg.__doc__
    torch.manual_seed(11)
    m = gmmn.GMMN(49, 32, 5)
    assert list(m.state_dict()) == list(R.KEYS) and type(m.G) is trainers.Generator is gmmn.Generator
    import ns_gan
    gan = ns_gan.NSGAN(image_size=49, hidden_dim=32, z_dim=5)
    res = m.load_state_dict(gan.state_dict(), strict=False)
    assert not res.missing_keys and res.unexpected_keys and all(k.startswith("D.") for k in res.unexpected_keys)
    for k in R.KEYS:
        assert torch.equal(m.state_dict()[k], gan.state_dict()[k]), k


@pytest.mark.parametrize("kw", [dict(sigmas=[]), dict(sigmas=[1.0, 0.0]), dict(sigmas=[-2.0]), dict(sigmas=[float("nan")]),
                                dict(sigmas=[float("inf")]), dict(sigmas=list(range(1, 18))), dict(sigmas="2"),
                                dict(sigmas=["a"]), dict(sqrt_loss=1), dict(sqrt_loss=None), dict(seed=-1),
                                dict(seed=1.5)])
def test_trainer_refusals(kw):
    with pytest.raises(gg.GMMNError) as ei:
        gmmn.GMMNTrainer(gmmn.GMMN(16, 8, 5), None, None, None, **kw)    # before anything is touched
    assert isinstance(ei.value, ValueError) and isinstance(ei.value, _lib.GMError)


def test_model_and_batch_size_refusals():
    for args in ((0, 8, 5), (8193, 8, 5), (16, 0, 5), (16, 8, 0), (16, 8, 8193), (16.0, 8, 5), (16, 8, True)):
        with pytest.raises(gg.GMMNError):
            gmmn.GMMN(*args)
    assert gg.MAX_B == _lib.GMMN_MAX_B == 2048
    assert gg.check_batch(2048) == 2048 and gg.check_sigmas(None) == gg.SIGMAS and gg.check_sigmas([3]) == (3.0,)
    for b in (0, 2049, 2.0, True):
        with pytest.raises(gg.GMMNError):
            gg.check_batch(b)
    x = torch.rand(20, 16)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(20, dtype=torch.int64))
    big = torch.utils.data.DataLoader(ds, batch_size=2049, shuffle=True)
    with pytest.raises(gg.GMMNError, match="2048"):
        gmmn.GMMNTrainer(gmmn.GMMN(16, 8, 5), big, big, big)
    with pytest.raises(_lib.GMError, match="samples only"):
        ops_fused.mmd_loss(x, x.clone().requires_grad_(True), [1.0])
    with pytest.raises(_lib.GMError):
        metrics.mmd(x, x)                                                 # host rows: no CPU fallback


def test_new_symbols_are_declared_and_bound():
    lib = _lib.load()
    from generative_models_amd import _build
    assert "gm_gmmn.hip" in _build.SOURCES and "gm_gemm.hip" == _build.SOURCES[0]
    # the workspace formula of the header
    for N, M, grad in ((1, 1, 0), (5, 7, 1), (512, 512, 1), (10000, 10000, 0)):
        T = N + M
        nch, nqb = -(-T // 128), -(-T // 256)
        assert lib.gm_mmd_workspace_bytes(N, M, grad) == 40 * nqb * nch + (8 * nch * N if grad else 0) + \
            4 * (T // 256 + 1) * 256
    for bad in ((0, 1, 0), (1, 0, 0), (-1, 5, 1), (2 ** 30, 2 ** 30, 0)):
        assert lib.gm_mmd_workspace_bytes(*bad) == _lib.GM_EINVAL


def test_kernels_reject_null_and_out_of_limit_arguments():
    """Host arrays stand in for device ones: every call below must return before it launches anything."""
    lib = _lib.load()
    a = [np.zeros(1 << 14, dtype=np.float64) for _ in range(8)]
    p = lambda i: a[i].ctypes.data
    N, M, I, S = 6, 5, 7, 3
    noise = ops_fused.gmmn_noise(1, gg.TAG_T)
    nz = lambda **kw: ctypes.byref(ops_fused.iwae_noise(1, gg.TAG_T, **dict(dict(k_total=1), **kw)))

    def prior(noise_=None, z=p(0), ldz=I, B=N, Z=I):
        return lib.gm_gmmn_prior(None, noise_ if noise_ is not None else ctypes.byref(noise), z, ldz, B, Z)

    def pairs(X=p(0), ldx=I, N=N, Y=p(1), ldy=I, M=M, I=I, sig=p(2), S=S, C=p(3), ldc=N + M, Rc=p(7), ws=p(4),
              wsb=1 << 17):
        return lib.gm_mmd_pairs(None, X, ldx, N, Y, ldy, M, I, sig, S, C, ldc, Rc, ws, wsb)

    def fin(N=N, M=M, S=S, sq=1, grad=1, ws=p(4), wsb=1 << 17, stats=p(5), r=p(6), loss=p(7)):
        return lib.gm_mmd_finalize(None, N, M, S, sq, grad, ws, wsb, stats, r, loss)

    def grad(X=p(0), ldx=I, P=p(1), ldp=I, r=p(6), stats=p(5), dA=p(3), lda=I, N=N, I=I):
        return lib.gm_mmd_grad(None, X, ldx, X, P, ldp, r, stats, 1.0, 1, dA, lda, N, I)

    cases = {
        prior: (dict(z=None), dict(B=0), dict(Z=0), dict(Z=8193), dict(ldz=I - 1), dict(noise_=nz(k_total=0)),
                dict(noise_=ctypes.POINTER(ops_fused.IwaeNoise)())),
        pairs: (dict(X=None), dict(Y=None), dict(sig=None), dict(ws=None), dict(Rc=None), dict(N=0), dict(M=0), dict(N=-1), dict(I=0),
                dict(I=8193), dict(S=0), dict(S=17), dict(ldx=I - 1), dict(ldy=I - 1), dict(ldc=N + M - 1), dict(wsb=8),
                dict(ws=p(4) + 4), dict(N=2 ** 30, M=2 ** 30)),
        fin: (dict(ws=None), dict(stats=None), dict(N=0), dict(M=0), dict(S=0), dict(S=17), dict(r=None), dict(wsb=8),
              dict(ws=p(4) + 4), dict(stats=p(5) + 4)),
        grad: (dict(X=None), dict(P=None), dict(r=None), dict(stats=None), dict(dA=None), dict(N=0), dict(N=65536),
               dict(I=0), dict(I=8193), dict(ldx=I - 1), dict(ldp=I - 1), dict(lda=I - 1), dict(stats=p(5) + 4)),
    }
    for fn, kws in cases.items():
        for kw in kws:
            assert fn(**kw) == _lib.GM_EINVAL, (fn.__name__, kw)
            assert b"bad argument" in lib.gm_last_error()
    assert pairs(C=None, ldc=0, wsb=8) == _lib.GM_EINVAL                # no gradient: still a workspace
    for t in a:
        assert not t.any()                                               # nothing was written
    with pytest.raises(_lib.GMError):
        _lib.call("gm_mmd_grad", None, None, 0, None, None, 0, None, None, 1.0, 1, None, 0, 1, 1)


def test_resource_table_has_the_new_kernels_without_scratch_or_spills():
    table = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))
    for k in KERNELS:
        rows = [v for n, v in table.items() if n.split("<")[0] == k]
        assert len(rows) == 1, k
        assert rows[0]["scratch"] == 0 and rows[0]["spills"] == 0, (k, rows[0])
    assert table["mmd_pairs_kernel"]["lds"] <= 80 * 1024                 # two workgroups per CU


# ---- path selection and the engine's host side ----------------------------------------------------------------------
def _loaders(n=40, batch=8, side=4):
    x = torch.rand(n, 1, side, side)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, **kw):
    tr = object.__new__(cls or gmmn.GMMNTrainer)            # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.seed, tr.noise_steps, tr._engine = 0, 0, None
    tr.sigmas, tr.sqrt_loss = gg.SIGMAS, True
    for n, v in kw.items():
        setattr(tr, n, v)
    return tr


class _Mine(gmmn.GMMNTrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_path_selection():
    assert _trainer(gmmn.GMMN(16, 8, 5))._stock() and _trainer(gmmn.GMMN(16, 8, 1))._stock()
    assert not _trainer(gmmn.GMMN(16, 8, 5), cls=_Mine)._stock()                 # an overridden hook
    m = gmmn.GMMN(16, 8, 5)
    m.G.extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock()                                              # an edited generator

    class Sub(gmmn.GMMN):
        pass
    assert not _trainer(Sub(16, 8, 5))._stock()                                  # a subclassed model


def test_engine_refuses_data_parallelism_and_other_settings_on_resume():
    m = gmmn.GMMN(16, 8, 5)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            gg.GMMNEngine(m, "cpu", trainer=_trainer(m), **kw)
    tr = _trainer(m)
    tr.force_dp = True
    with pytest.raises(_lib.GMError, match="one GPU"):
        tr.train(1)
    bad = gmmn.GMMN(16, 8, 5)
    bad.G.extra = torch.nn.Linear(2, 2)
    with pytest.raises(_lib.GMError, match="general path"):
        gg.GMMNEngine(bad, "cpu", trainer=_trainer(m))
    tr = _trainer(m, seed=9, sigmas=(1.0, 4.0), sqrt_loss=False)
    eng = gg.GMMNEngine(m, "cpu", trainer=tr)
    now = eng._settings()
    assert now == {"sigmas": (1.0, 4.0), "sqrt_loss": False, "seed": 9}
    n = eng.fp.m.numel()
    for key, other in (("sigmas", (1.0, 5.0)), ("sqrt_loss", True), ("seed", 0)):
        saved = dict(now, B=8, lr=1e-3, weight_decay=0.0)
        saved[key] = other
        resume = {"m": torch.zeros(n), "v": torch.zeros(n), "step": 5, "config": saved}
        with pytest.raises(_lib.GMError, match="different settings") as ei:
            eng.configure(8, 5, 1e-3, 0.0, resume=resume)
        assert key in str(ei.value)
    with pytest.raises(gg.GMMNError, match="2048"):
        eng.configure(2049, 5, 1e-3, 0.0)


def test_mmd_is_on_every_trainer_that_has_parzen():
    from generative_models_amd import acgan, bgan, rbm, trainers
    for cls in (trainers.GANTrainer, trainers.VAETrainer, trainers.AutoencoderTrainer, rbm.RBMTrainer,
                acgan.ACGANTrainer, bgan.BayesGANTrainer, gmmn.GMMNTrainer):
        assert callable(getattr(cls, "parzen")) and callable(getattr(cls, "mmd")), cls
        p = inspect.signature(cls.mmd).parameters
        assert [(n, q.default) for n, q in list(p.items())[1:]] == [("n_samples", 10000), ("sigmas", None), ("seed", 0)]
    assert callable(trainers._mmd) and callable(trainers._parzen)
    ae = object.__new__(trainers.AutoencoderTrainer)
    with pytest.raises(_lib.GMError, match="no prior"):
        ae.mmd()
