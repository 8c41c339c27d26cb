"""The SWG without a GPU: the reference's overlap form against the replicate-and-sort form and against fp64 autograd, the
order of tied elements, the directions' rule, the module surface and other generators' weights, the refusals, the C-ABI
of the new kernels and its refusals, the resource table's new rows, path selection, the checkpoint settings, and swd() on
every trainer that has parzen()."""
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

import swg  # noqa: E402
import swg_reference as R  # noqa: E402
from generative_models_amd import _lib, metrics, ops_fused, philox  # noqa: E402
from generative_models_amd import swg as sg  # noqa: E402

KERNELS = ("sw_directions_kernel", "sw_sort_kernel", "sw_finalize_kernel")


@pytest.mark.parametrize("N,M", [(1, 1), (3, 5), (5, 3), (1, 6), (7, 7), (10, 4), (64, 65)])
def test_reference_against_replicate_and_sort(N, M):
    rng = np.random.default_rng(100 * N + M)
    a, b = rng.standard_normal((3, N)), rng.standard_normal((3, M)) + 0.3
    ref = R.sw_reference(a, b)
    for p in range(3):
        assert abs(ref["W"][p] - R.sw_loops(a[p], b[p])) <= 1e-14 * max(1.0, ref["W"][p])
    assert abs(ref["swd2"] - ref["W"].mean()) <= 1e-15
    i, j, w = R.segments(N, M)
    assert w.sum() == N * M and w.min() >= 1 and len(w) <= N + M - 1
    for r in range(N):                                        # the contract's range of partners, and its weights
        js = j[i == r]
        assert js[0] == (r * M) // N and js[-1] == ((r + 1) * M - 1) // N and np.array_equal(js, np.arange(js[0], js[-1] + 1))
        assert all(wv == min((r + 1) * M, (jv + 1) * N) - max(r * M, jv * N) for jv, wv in zip(js, w[i == r]))
        assert w[i == r].sum() == M
    if N == M:
        assert np.array_equal(w, np.full(N, N)) and np.array_equal(i, j)


@pytest.mark.parametrize("N,M,I,P", [(7, 7, 5, 4), (33, 33, 12, 9), (5, 8, 6, 3), (9, 4, 3, 5)])
def test_reference_gradient_against_autograd(N, M, I, P):
    g = torch.Generator().manual_seed(N + 10 * M)
    X, Y = torch.rand(N, I, generator=g, dtype=torch.float64), torch.rand(M, I, generator=g, dtype=torch.float64)
    Th = R.directions_reference(P, I, 3, 0, sg.TAG_DT)
    a, b = Th @ X.numpy().T, Th @ Y.numpy().T
    ref = R.sw_reference(a, b)
    loss, dX = R.autograd_dX(X, Y, Th)
    assert abs(ref["swd2"] - loss) <= 1e-15
    assert np.abs(ref["Ct"].T @ Th - dX).max() <= 1e-14 * max(1.0, np.abs(dX).max())
    if N == M:                                                # the usual rank matching
        Xt = X.clone().requires_grad_(True)
        tt = torch.as_tensor(Th)
        l2 = ((torch.sort(tt @ Xt.T, dim=1)[0] - torch.sort(tt @ Y.T, dim=1)[0]) ** 2).mean()
        l2.backward()
        assert abs(float(l2.detach()) - ref["swd2"]) <= 1e-15 and np.abs(Xt.grad.numpy() - dX).max() <= 1e-14


def test_ties_follow_the_index_order():
    N = 9
    a = np.full((1, N), 0.25)
    b = np.arange(N, dtype=np.float64)[None, ::-1].copy()
    ref = R.sw_reference(a, b)
    assert np.array_equal(ref["order_a"][0], np.arange(N)) and np.array_equal(ref["rank_a"][0], np.arange(N))
    assert np.array_equal(ref["order_b"][0], np.arange(N)[::-1])
    # row i of a is matched with the i-th smallest b: the coefficients ascend with the index
    assert np.allclose(ref["Ct"][0], 2.0 / (N * N) * N * (0.25 - np.arange(N)), rtol=0, atol=1e-15)
    z = np.array([[0.0, -0.0, 0.0, -0.0]])
    assert np.array_equal(R.sw_reference(z, z)["order_a"][0], np.arange(4))      # -0.0 == +0.0: the index decides
    assert R.sw_reference(z, z)["swd2"] == 0.0


@pytest.mark.parametrize("P,I", [(1, 1), (3, 5), (4, 784), (2, 130)])
def test_directions_reference_is_philox(P, I):
    for seed, step, tag, row0 in ((0, 0, sg.TAG_DT, 0), (2 ** 40 + 5, 7, sg.TAG_DV, 3), (9, 0, sg.TAG_DM, 256)):
        th = sg.directions_reference(P, I, seed, step, tag, row0)
        n = philox.normals(P, I, seed, step, tag, row0)
        assert th.shape == (P, I) and np.allclose((th * th).sum(1), 1.0, rtol=0, atol=1e-14)
        assert np.allclose(th * np.sqrt((n * n).sum(1, keepdims=True)), n, rtol=1e-14, atol=0)
        assert np.array_equal(th, R.directions_reference(P, I, seed, step, tag, row0))
        assert np.array_equal(th[-1:], sg.directions_reference(1, I, seed, step, tag, row0 + P - 1))   # row p alone
    tags = (sg.TAG_T, sg.TAG_V, sg.TAG_S, sg.TAG_DT, sg.TAG_DV, sg.TAG_DM)
    assert tags == (0x53574754, 0x53574756, 0x53574753, 0x53574454, 0x53574456, 0x5357444D)
    assert [t.to_bytes(4, "big") for t in tags] == [b"SWGT", b"SWGV", b"SWGS", b"SWDT", b"SWDV", b"SWDM"]


def test_module_surface_and_other_generators_weights():
    for n in ("Generator", "SWG", "SWGTrainer", "SWGError"):
        assert hasattr(swg, n), n
    sig = inspect.signature(swg.SWG.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("image_size", 784), ("hidden_dim", 400), ("z_dim", 20)]
    T = swg.SWGTrainer
    sig = inspect.signature(T.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[6:]] == [("num_projections", 1024), ("seed", 0)]
    assert all(p.kind is p.KEYWORD_ONLY for p in list(sig.values())[6:])
    tp = inspect.signature(T.train).parameters
    assert (tp["lr"].default, tp["weight_decay"].default) == (1e-3, 0.0)
    from generative_models_amd import engine, trainers
    assert issubclass(T, trainers.OneLossTrainer) and T._series == (("losses", "recon"),)
    assert issubclass(sg.SWGEngine, engine.VAEEngine) and "_issue" in sg.SWGEngine.__dict__
    for name in ("sample", "sample_images", "parzen", "mmd", "swd", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(T, name)), name
    assert issubclass(sg.SWGError, _lib.GMError) and issubclass(sg.SWGError, ValueError)
    import generative_models_amd as pkg
    assert pkg.SWG is sg.SWG and pkg.SWGTrainer is T and pkg.SWGEngine is sg.SWGEngine
    assert sg.__doc__ and "The contract." in sg.__doc__ and "w_ij = max(0, min((i+1) M, (j+1) N) - max(i M, j N))" in sg.__doc__
    assert "is left\nat 0" in sg.__doc__                                  # the zero-norm row
    for name in ("sw_noise", "sw_directions", "sw_workspace", "sw_sort", "sw_finalize", "sw_loss"):
        assert callable(getattr(ops_fused, name)), name
    torch.manual_seed(11)
    m = swg.SWG(49, 32, 5)
    assert list(m.state_dict()) == list(R.KEYS) and type(m.G) is trainers.Generator is swg.Generator
    import gmmn
    import ns_gan
    for other in (ns_gan.NSGAN(image_size=49, hidden_dim=32, z_dim=5), gmmn.GMMN(49, 32, 5)):
        res = m.load_state_dict(other.state_dict(), strict=False)
        assert not res.missing_keys and all(k.startswith("D.") for k in res.unexpected_keys)
        for k in R.KEYS:
            assert torch.equal(m.state_dict()[k], other.state_dict()[k]), k
    tr = object.__new__(T)
    for fn in (tr.log_likelihood, lambda: tr.reconstruct_images(None, 0)):
        with pytest.raises(_lib.GMError):
            fn()


@pytest.mark.parametrize("kw", [dict(num_projections=0), dict(num_projections=8193), dict(num_projections=2.0),
                                dict(num_projections=True), dict(num_projections=None), dict(seed=-1), dict(seed=1.5)])
def test_trainer_refusals(kw):
    with pytest.raises(sg.SWGError) as ei:
        swg.SWGTrainer(swg.SWG(16, 8, 5), None, None, None, **kw)        # before anything is touched
    assert isinstance(ei.value, ValueError) and isinstance(ei.value, _lib.GMError)


def test_model_and_batch_size_refusals():
    for args in ((0, 8, 5), (8193, 8, 5), (16, 0, 5), (16, 8, 0), (16, 8, 8193), (16.0, 8, 5), (16, 8, True)):
        with pytest.raises(sg.SWGError):
            swg.SWG(*args)
    assert sg.MAX_B == _lib.SW_MAX_B == 2048 and sg.MAX_P == _lib.SW_MAX_P == 8192
    assert sg.MAX_ROWS == _lib.SW_MAX_ROWS == 16384
    assert sg.check_batch(2048) == 2048 and sg.check_projections(8192) == 8192 and sg.check_projections(1) == 1
    for b in (0, 2049, 2.0, True):
        with pytest.raises(sg.SWGError):
            sg.check_batch(b)
    x = torch.rand(20, 16)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(20, dtype=torch.int64))
    big = torch.utils.data.DataLoader(ds, batch_size=2049, shuffle=True)
    with pytest.raises(sg.SWGError, match="2048"):
        swg.SWGTrainer(swg.SWG(16, 8, 5), big, big, big)
    with pytest.raises(_lib.GMError, match="samples only"):
        ops_fused.sw_loss(x, x.clone().requires_grad_(True), x)
    with pytest.raises(_lib.GMError):
        ops_fused.sw_loss(x, x, x)                                       # host rows: no CPU fallback
    with pytest.raises(_lib.GMError):
        metrics.sliced_wasserstein(x, x)
    assert metrics.SWDResult._fields == ("swd2", "swd", "n_projections", "n_samples", "n_data")
    p = inspect.signature(metrics.sliced_wasserstein).parameters
    assert [(n, q.default) for n, q in p.items()] == [("samples", p["samples"].empty), ("data", p["data"].empty),
                                                      ("n_projections", 1024), ("seed", 0)]
    assert metrics.SWD_BLOCK == 256


def test_new_symbols_are_declared_and_bound():
    lib = _lib.load()
    from generative_models_amd import _build
    assert "gm_sw.hip" in _build.SOURCES and _build.SOURCES[0] == "gm_gemm.hip" and _build.SOURCES[-1] == "gm_fm.hip"
    assert os.path.isfile(os.path.join(ROOT, "generative_models_amd", "csrc", "gm_sw.hip"))
    for P in (1, 5, 1024, 8192):                                         # the workspace formula of the header
        assert lib.gm_sw_workspace_bytes(P) == 8 * P
    for bad in (0, -1, 8193, 2 ** 30):
        assert lib.gm_sw_workspace_bytes(bad) == _lib.GM_EINVAL
        assert b"bad argument" in lib.gm_last_error()


def test_kernels_reject_null_and_out_of_limit_arguments():
    """Host arrays stand in for device ones: every call below must return before it launches anything."""
    lib = _lib.load()
    a = [np.zeros(1 << 14, dtype=np.float64) for _ in range(6)]
    p = lambda i: a[i].ctypes.data
    P, N, M, I = 5, 6, 4, 7
    noise = ops_fused.sw_noise(1, sg.TAG_DT)
    nz = lambda **kw: ctypes.byref(ops_fused.iwae_noise(1, sg.TAG_DT, **dict(dict(k_total=1), **kw)))

    def dirs(noise_=None, th=p(0), ldt=I, P=P, I=I):
        return lib.gm_sw_directions(None, noise_ if noise_ is not None else ctypes.byref(noise), th, ldt, P, I)

    def sort(Pr=p(1), ldp=N + M, P=P, N=N, M=M, Ct=p(2), ldc=N, ws=p(3), wsb=8 * P):
        return lib.gm_sw_sort(None, Pr, ldp, P, N, M, Ct, ldc, ws, wsb)

    def fin(P=P, N=N, M=M, ws=p(3), wsb=8 * P, stats=p(4), loss=p(5)):
        return lib.gm_sw_finalize(None, P, N, M, ws, wsb, stats, loss)

    cases = {
        dirs: (dict(th=None), dict(P=0), dict(P=8193), dict(I=0), dict(I=8193), dict(ldt=I - 1),
               dict(noise_=nz(k_total=0)), dict(noise_=nz(k_total=2)), dict(noise_=nz(j0=-1)),
               dict(noise_=nz(j0=2 ** 32 - P + 1)), dict(noise_=nz(q0=-1)), dict(noise_=nz(q0=2 ** 31)),
               dict(noise_=ctypes.POINTER(ops_fused.IwaeNoise)())),
        sort: (dict(Pr=None), dict(ws=None), dict(P=0), dict(P=8193), dict(N=0), dict(M=0), dict(N=-1), dict(N=2049, ldp=4096),
               dict(M=2049, ldp=4096), dict(Ct=None, ldc=0, N=16385, ldp=1 << 15), dict(Ct=None, ldc=0, M=16385, ldp=1 << 15),
               dict(ldp=N + M - 1), dict(ldc=N - 1), dict(wsb=8 * P - 1), dict(wsb=0), dict(ws=p(3) + 4)),
        fin: (dict(ws=None), dict(stats=None), dict(P=0), dict(P=8193), dict(N=0), dict(M=0), dict(N=16385), dict(M=16385),
              dict(wsb=8 * P - 1), dict(ws=p(3) + 4), dict(stats=p(4) + 4)),
    }
    for fn, kws in cases.items():
        for kw in kws:
            assert fn(**kw) == _lib.GM_EINVAL, (fn.__name__, kw)
            assert b"bad argument" in lib.gm_last_error()
    assert sort(Ct=None, ldc=0, wsb=8) == _lib.GM_EINVAL                # no gradient: still a workspace
    for t in a:
        assert not t.any()                                               # nothing was written
    with pytest.raises(_lib.GMError):
        _lib.call("gm_sw_sort", None, None, 0, 1, 1, 1, None, 0, None, 0)


def test_resource_table_has_the_new_kernels_without_scratch_or_spills():
    table = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))
    for k in KERNELS:
        rows = [v for n, v in table.items() if n.split("<")[0] == k]
        assert len(rows) == (2 if k == "sw_sort_kernel" else 1), k       # with and without (value, row) pairs
        for row in rows:
            assert row["scratch"] == 0 and row["spills"] == 0, (k, row)


# ---- path selection and the engine's host side ----------------------------------------------------------------------
def _loaders(n=40, batch=8, side=4):
    x = torch.rand(n, 1, side, side)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, **kw):
    tr = object.__new__(cls or swg.SWGTrainer)              # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.seed, tr.noise_steps, tr._engine = 0, 0, None
    tr.num_projections = 64
    for n, v in kw.items():
        setattr(tr, n, v)
    return tr


class _Mine(swg.SWGTrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_path_selection():
    assert _trainer(swg.SWG(16, 8, 5))._stock() and _trainer(swg.SWG(16, 8, 1))._stock()
    assert not _trainer(swg.SWG(16, 8, 5), cls=_Mine)._stock()                   # an overridden hook
    m = swg.SWG(16, 8, 5)
    m.G.extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock()                                              # an edited generator

    class Sub(swg.SWG):
        pass
    assert not _trainer(Sub(16, 8, 5))._stock()                                  # a subclassed model
    assert sg.swg_fused_ok(swg.SWG(16, 8, 5)) and not sg.swg_fused_ok(m)


def test_engine_refuses_data_parallelism_and_other_settings_on_resume():
    m = swg.SWG(16, 8, 5)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            sg.SWGEngine(m, "cpu", trainer=_trainer(m), **kw)
    tr = _trainer(m)
    tr.force_dp = True
    with pytest.raises(_lib.GMError, match="one GPU"):
        tr.train(1)
    bad = swg.SWG(16, 8, 5)
    bad.G.extra = torch.nn.Linear(2, 2)
    with pytest.raises(_lib.GMError, match="general path"):
        sg.SWGEngine(bad, "cpu", trainer=_trainer(m))
    tr = _trainer(m, seed=9, num_projections=130)
    eng = sg.SWGEngine(m, "cpu", trainer=tr)
    now = eng._settings()
    assert now == {"num_projections": 130, "seed": 9}                    # what a checkpoint's config carries
    n = eng.fp.m.numel()
    for key, other in (("num_projections", 131), ("seed", 0)):
        saved = dict(now, B=8, lr=1e-3, weight_decay=0.0)
        saved[key] = other
        resume = {"m": torch.zeros(n), "v": torch.zeros(n), "step": 5, "config": saved}
        with pytest.raises(_lib.GMError, match="different settings") as ei:
            eng.configure(8, 5, 1e-3, 0.0, resume=resume)
        assert key in str(ei.value)
    with pytest.raises(sg.SWGError, match="2048"):
        eng.configure(2049, 5, 1e-3, 0.0)
    tr.num_projections = 9000
    with pytest.raises(sg.SWGError, match="8192"):
        eng.configure(8, 5, 1e-3, 0.0)


class _DoneEngine:
    """What save_checkpoint reads of an engine after a finished train(): the optimizer state with the run's config (the
    moments of a real SWGEngine built on the host, its own settings)."""

    def __init__(self, eng, B=8, lr=1e-3, weight_decay=0.0, step=5):
        self.steps_planned = step
        self._state = {"m": torch.full_like(eng.fp.m, 0.25), "v": torch.full_like(eng.fp.v, 0.5), "step": step,
                       "config": dict(eng._settings(), B=B, lr=lr, weight_decay=weight_decay)}

    def optim_state(self):
        return dict(self._state)


def test_checkpoint_config_and_noise_clock_round_trip(tmp_path):
    """save_checkpoint -> file -> load_checkpoint on the host: num_projections, seed and noise_steps come back as they
    were written, the loss history with them, and the next run's configure() refuses other settings."""
    m = swg.SWG(16, 8, 5)
    tr = _trainer(m, seed=9, num_projections=130, noise_steps=7, name="SWG", num_epochs=1, best_val_loss=0.125)
    tr.losses = [0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625, 0.0078125]
    tr._engine = _DoneEngine(sg.SWGEngine(m, "cpu", trainer=tr))
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    assert ck["optim"]["config"] == {"num_projections": 130, "seed": 9, "B": 8, "lr": 1e-3, "weight_decay": 0.0}
    assert ck["history"] == {"losses": tr.losses, "num_epochs": 1, "best_val_loss": 0.125, "noise_steps": 7}
    m2 = swg.SWG(16, 8, 5)
    tr2 = _trainer(m2, seed=9, num_projections=130, name="SWG")
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 7 and tr2.losses == tr.losses and tr2.best_val_loss == 0.125 and tr2.num_epochs == 1
    for k, v in m.state_dict().items():
        assert torch.equal(m2.state_dict()[k], v), k
    assert tr2._noise_step() == (True, 7) and tr2.noise_steps == 8          # the next training batch's noise step
    res = tr2._resume_optim
    assert res["config"] == ck["optim"]["config"] and res["step"] == 5 and res["lenient"] is False
    assert torch.equal(res["m"], torch.full_like(res["m"], 0.25)) and torch.equal(res["v"], torch.full_like(res["v"], 0.5))
    for kw in (dict(num_projections=131), dict(seed=8)):                    # another run's settings: refused on resume
        other = _trainer(m2, **dict(dict(seed=9, num_projections=130), **kw))
        with pytest.raises(_lib.GMError, match="different settings"):
            sg.SWGEngine(m2, "cpu", trainer=other).configure(8, 5, 1e-3, 0.0, resume=res)


def test_swd_is_on_every_trainer_that_has_parzen():
    import gmmn
    from generative_models_amd import acgan, bgan, rbm, trainers
    for cls in (trainers.GANTrainer, trainers.VAETrainer, trainers.AutoencoderTrainer, rbm.RBMTrainer,
                acgan.ACGANTrainer, bgan.BayesGANTrainer, gmmn.GMMNTrainer, swg.SWGTrainer):
        assert callable(getattr(cls, "parzen")) and callable(getattr(cls, "mmd")) and callable(getattr(cls, "swd")), cls
        p = inspect.signature(cls.swd).parameters
        assert [(n, q.default) for n, q in list(p.items())[1:]] == [("n_samples", 10000), ("n_projections", 1024),
                                                                    ("seed", 0)]
    assert callable(trainers._swd)
    ae = object.__new__(trainers.AutoencoderTrainer)
    with pytest.raises(_lib.GMError, match="no prior"):
        ae.swd()
