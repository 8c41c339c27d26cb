"""The restricted Boltzmann machine without a GPU: module surface and state_dict keys, known answers of the noise rule
against the other Philox restatements, the CD gradient against autograd of the free-energy gap, the fp64 AIS restatement
against the exact partition function of the small cases, the fp32 restatement's own deviation (the figure the GPU file's
log-weight tolerance is four times of), the undecided rows of every chain case the GPU file runs, argument validation,
the C-ABI of the new kernels and its refusals, fused / general path selection and the data-parallel refusal.  The
library has no CPU fallback, so training, the general path and the checkpoint round trip run in tests/test_gpu_rbm.py."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))
sys.path.insert(0, HERE)

import rbm  # noqa: E402
import rbm_reference as R  # noqa: E402
from generative_models_amd import _lib, metrics, ops_fused  # noqa: E402
from generative_models_amd import dvae as gdvae  # noqa: E402
from generative_models_amd import made as gmade  # noqa: E402
from generative_models_amd import rbm as grbm  # noqa: E402



def _loaders(n=40, batch=8, side=4):
    x = torch.bernoulli(torch.full((n, 1, side, side), 0.5))
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, **kw):
    tr = object.__new__(cls or rbm.RBMTrainer)       # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.seed, tr.k, tr.mode = kw.get("seed", 0), kw.get("k", 1), kw.get("mode", "cd")
    return tr


def test_module_surface_and_state_dict_keys():
    m = rbm.RBM(16, 12)
    assert sorted(m.state_dict()) == ["linear.bias", "linear.weight", "vbias"]
    assert (tuple(m.linear.weight.shape), tuple(m.vbias.shape)) == ((12, 16), (16,))
    assert torch.all(m.vbias == 0) and (m.image_size, m.hidden_dim, m.shape) == (16, 12, 4)
    sig = inspect.signature(rbm.RBM.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("image_size", 784), ("hidden_dim", 400)]
    sig = inspect.signature(rbm.RBMTrainer.__init__).parameters
    assert (sig["seed"].default, sig["k"].default, sig["mode"].default) == (0, 1, "cd")
    sig = inspect.signature(rbm.RBMTrainer.train).parameters
    assert (sig["lr"].default, sig["weight_decay"].default) == (1e-3, 0.0)
    sig = inspect.signature(rbm.RBMTrainer.sample).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("n", inspect.Parameter.empty), ("seed", 0),
                                                                  ("steps", 1000), ("return_probs", False)]
    sig = inspect.signature(rbm.RBMTrainer.log_likelihood).parameters
    assert (sig["images"].default, sig["chains"].default, sig["seed"].default) == (None, 512, 0)
    for name in ("sample", "gibbs", "hidden", "free_energy", "log_likelihood", "parzen", "sample_images", "viz_loss",
                 "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(rbm.RBMTrainer, name))
    assert metrics.AISResult._fields == ("ll_mean", "ll_stderr", "log_z", "log_z_stderr", "chains", "n_betas", "n")
    assert issubclass(rbm.RBMError, _lib.GMError) and issubclass(rbm.RBMError, ValueError)
    import generative_models_amd as pkg
    assert pkg.RBM is grbm.RBM and pkg.RBMTrainer is grbm.RBMTrainer and pkg.RBMEngine is grbm.RBMEngine
    from generative_models_amd.engine import VAEEngine
    from generative_models_amd.trainers import VAETrainer
    assert issubclass(grbm.RBMEngine, VAEEngine) and issubclass(grbm.RBMTrainer, VAETrainer)
    for f in ("_buffers", "_issue", "configure", "optim_state"):     # _alloc, the guard around _buffers: the shared base's
        assert f in grbm.RBMEngine.__dict__


def test_noise_rule_known_answers():
    seed = 0x0123456789ABCDEF
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    for tag in (R.TAG_D, R.TAG_H, R.TAG_V):
        u = grbm.uniforms_reference(3, 10, seed, tag, t=7, row0=2)     # width 10: a partial third Philox word group
        assert u.dtype == np.float32 and u.shape == (3, 10)
        assert np.array_equal(u, R.uniforms(3, 10, seed, tag, 7, 2))
        for r in range(3):
            for e in range(10):
                w = gdvae.philox4x32_10(np.array([e >> 2, 7, r + 2, tag], np.uint64), key)
                assert u[r, e] == np.float32((2 * (int(w[e & 3]) >> 9) + 1) * 2.0 ** -24)
        assert 0.0 < u.min() and u.max() < 1.0
    assert (R.TAG_D, R.TAG_H, R.TAG_V) == tuple(int.from_bytes(s, "big") for s in (b"RBMD", b"RBMH", b"RBMV"))
    assert (_lib.RBM_TAG_D, _lib.RBM_TAG_H, _lib.RBM_TAG_V) == (R.TAG_D, R.TAG_H, R.TAG_V)
    # the Philox known answer the other counter streams' tests pin (Random123's kat_vectors: counter 0, key 0)
    z4 = gdvae.philox4x32_10(np.zeros(4, np.uint64), np.zeros(2, np.uint64))
    assert [int(v) for v in z4] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    # at t = 0 the counter differs from MADE's in the tag alone: the same restatement reproduces MADE's stream
    assert np.array_equal(R.uniforms(4, 9, 5, gmade.TAG_MS, 0, 1), gmade.uniforms_reference(4, 9, 5, row0=1))
    a = R.uniforms(4, 8, 1, R.TAG_H, 3)
    assert np.array_equal(a[2:], R.uniforms(2, 8, 1, R.TAG_H, 3, row0=2))           # rows are counters
    assert np.array_equal(a[:, :5], R.uniforms(4, 5, 1, R.TAG_H, 3))                # so are units
    assert not np.array_equal(a, R.uniforms(4, 8, 1, R.TAG_H, 4))                   # and steps
    assert not np.array_equal(a, R.uniforms(4, 8, 1, R.TAG_V, 3))
    from generative_models_amd import ddpm as gddpm
    tags = {R.TAG_D, R.TAG_H, R.TAG_V, gmade.TAG_MS, gddpm.TAG_T, gddpm.TAG_E, gddpm.TAG_S, gdvae.CTR_TAG, 0}
    assert len(tags) == 9                                        # distinct streams


def test_cd_gradient_is_autograd_of_the_gap():
    W, c, b = R.case_weights(13, 7, 3)
    g = np.random.RandomState(4)
    v0, vk = (g.random_sample((6, 13)) < 0.5).astype(np.float64), (g.random_sample((6, 13)) < 0.5).astype(np.float64)
    loss, dW, dc, db = R.cd_grads(W, c, b, v0, vk)
    P = [torch.tensor(t, dtype=torch.float64, requires_grad=True) for t in (W, c, b)]
    F = lambda v: -(v @ P[2]) - torch.nn.functional.softplus(v @ P[0].t() + P[1]).sum(1)
    gap = (F(torch.from_numpy(v0)) - F(torch.from_numpy(vk))).mean()
    gap.backward()
    assert abs(gap.item() - loss) <= 1e-12
    for ref, t in zip((dW, dc, db), P):
        assert np.abs(ref - t.grad.numpy()).max() <= 1e-14
    # the module's own free energy (the general path's loss) is the same function
    m = rbm.RBM(13, 7).double()
    with torch.no_grad():
        m.linear.weight.copy_(P[0]), m.linear.bias.copy_(P[1]), m.vbias.copy_(P[2])
    m.hidden_logits = lambda v: v @ m.linear.weight.t() + m.linear.bias      # (the fused layer needs the GPU)
    assert np.abs(m.free_energy(torch.from_numpy(v0)).detach().numpy() - R.free_energy(W, c, b, v0)).max() <= 1e-12


def _ais_start(b_A, n):
    return np.repeat((1.0 / (1.0 + np.exp(-b_A.astype(np.float64)))).astype(np.float32)[None], n, 0)


@pytest.fixture(scope="module")
def ais_runs():
    out = {}
    for name in R.AIS_CASES:
        W, c, b, b_A, seed = R.ais_case(name)
        x, betas = _ais_start(b_A, R.AIS_CHAINS), R.uniform_betas(R.AIS_BETAS)
        out[name] = tuple(R.chain(W, c, b, x, R.AIS_BETAS - 1, seed, betas=betas, b_A=b_A, dtype=dt)
                          for dt in (np.float64, np.float32))
    return out


@pytest.mark.parametrize("name", list(R.AIS_CASES))
def test_fp64_ais_lands_on_the_exact_partition_function(name, ais_runs):
    """The case seeds and the schedule are sound: 256 chains x 500 uniformly spaced betas in fp64 land within 2 of their
    own standard errors of log Z by enumeration."""
    W, c, b, b_A, _ = R.ais_case(name)
    log_z, se = R.ais_log_z(ais_runs[name][0]["logw"], b_A, W.shape[0])
    exact = R.exact_log_z(W, c, b)
    print(name, "log Z AIS", log_z, "+-", se, "exact", exact)
    assert abs(log_z - exact) <= 2 * se and se < 0.05
    # the enumeration itself: over the visible states of a tiny model it is the same number
    Wt, ct, bt = R.case_weights(6, 3, 1, scale=1.0)
    vs = ((np.arange(64)[:, None] >> np.arange(6)[None, :]) & 1).astype(np.float64)
    assert abs(np.log(np.exp(-R.free_energy(Wt, ct, bt, vs)).sum()) - R.exact_log_z(Wt, ct, bt)) <= 1e-12
    # and the base-rate RBM's partition function
    assert abs(R.log_z_base(b_A, 3) - R.exact_log_z(np.zeros((3, b_A.size)), np.zeros(3), b_A)) <= 1e-10


def test_fp32_ais_restatement_deviation(ais_runs):
    """How far the fp32 restatement (pinned sum order and rounding) strays from fp64 on the same uniforms over the rows
    decided in both: the GPU file allows the device four times the largest figure, AIS_RESTATEMENT_DEV."""
    worst = 0.0
    for name, (r64, r32) in ais_runs.items():
        ok = ~(r64["und"] | r32["und"])
        dev = np.abs(r64["logw"] - r32["logw"])[ok].max()
        print(name, "decided rows", int(ok.sum()), "of", ok.size, "deviation", dev)
        assert ok.sum() >= 0.5 * ok.size
        worst = max(worst, dev)
    assert 0.5 * R.AIS_RESTATEMENT_DEV <= worst <= R.AIS_RESTATEMENT_DEV
    assert R.AIS_LOGW_TOL == 4 * R.AIS_RESTATEMENT_DEV


@pytest.mark.parametrize("case", list(R.CHAIN_CASES))
def test_chain_cases_are_decided(case):
    """What tests/test_gpu_rbm.py relies on, with the reference alone: the small cases have no undecided row, 784-400 at
    most 5 %; the chains are not frozen; and between decided rows the fp32 restatement makes the fp64 run's decisions,
    its logits within 1e-4 of fp64's."""
    n, I, H, steps, seed = R.CHAIN_CASES[case]
    W, c, b = R.case_weights(I, H, seed)
    x = R.case_input(n, I, seed)
    r64 = R.chain(W, c, b, x, steps, seed, row0=3, dstep=5, g0=11)
    r32 = R.chain(W, c, b, x, steps, seed, row0=3, dstep=5, g0=11, dtype=np.float32)
    print(case, "undecided rows", int(r64["und"].sum()), "of", n, "max |logit|", np.abs(r64["a"]).max())
    assert r64["und"].sum() <= R.UNDECIDED_SHARE.get(case, 0.0) * n
    ok = ~(r64["und"] | r32["und"])
    for k in ("v0", "v", "h"):
        assert np.array_equal(r64[k][ok], r32[k][ok])
    assert np.abs(r64["a"] - r32["a"])[ok].max() <= 1e-4 and np.abs(r64["p"] - r32["p"])[ok].max() <= R.STEP_TOL
    assert np.abs(r64["a"]).max() <= 16.0
    assert np.array_equal(r64["v0"][x == 0.0], np.zeros((x == 0.0).sum(), bool)) and r64["v0"][x == 1.0].all()
    if I > 1:
        assert 0.05 < r64["v"].mean() < 0.95 and 0.05 < r64["h"].mean() < 0.95


@pytest.mark.parametrize("bad", [dict(image_size=0), dict(image_size=1025), dict(image_size=16.0), dict(image_size=True),
                                 dict(hidden_dim=0), dict(hidden_dim=1025), dict(hidden_dim="8")])
def test_bad_model_arguments_raise(bad):
    with pytest.raises(ValueError) as ei:
        rbm.RBM(**dict(dict(image_size=16, hidden_dim=8), **bad))
    assert isinstance(ei.value, _lib.GMError) and isinstance(ei.value, rbm.RBMError)


def test_limits_are_accepted():
    assert rbm.RBM(1, 1).vbias.shape == (1,)
    assert grbm.check_shape(1024, 1024) == (1024, 1024)


def test_bad_trainer_arguments_raise_before_anything_runs():
    its = _loaders()
    for kw in (dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(k=0), dict(k=4097), dict(k=True), dict(k=1.0),
               dict(mode="sml"), dict(mode=None)):
        with pytest.raises(ValueError) as ei:
            rbm.RBMTrainer(rbm.RBM(16, 8), *its, **kw)
        assert isinstance(ei.value, _lib.GMError), kw
    tr = _trainer(rbm.RBM(16, 8))
    for kw in (dict(seed=-1), dict(seed=None), dict(n=0), dict(n=2.5), dict(n=True), dict(steps=0), dict(steps=-1),
               dict(steps=1.0), dict(steps=(1 << 24) + 1)):
        with pytest.raises(ValueError) as ei:
            tr.sample(**dict(dict(n=4), **kw))
        assert isinstance(ei.value, _lib.GMError), kw
    for kw in (dict(steps=-1), dict(steps=None), dict(seed=1 << 64)):
        with pytest.raises(ValueError):
            tr.gibbs(torch.zeros(2, 16), **dict(dict(steps=1), **kw))
    with pytest.raises(ValueError):
        tr.gibbs(torch.zeros(2, 15), 1)                          # another image size
    for betas in (1, 0, True, [0.0], [0.1, 1.0], [0.0, 0.9], [0.0, 0.6, 0.5, 1.0], (1 << 24) + 1):
        with pytest.raises(ValueError):
            grbm.check_betas(betas)
    for kw in (dict(chains=1), dict(chains=2.0), dict(seed=-1), dict(betas=[0.5, 1.0])):
        with pytest.raises(ValueError):
            tr.ais(**kw)
    b = grbm.check_betas(None)
    assert b.dtype == np.float32 and b.size == 14500 and b[0] == 0.0 and b[-1] == 1.0 and np.all(np.diff(b) > 0)
    assert b[500] == np.float32(0.5) and b[4500] == np.float32(0.9)
    assert np.array_equal(grbm.check_betas(5), np.linspace(0, 1, 5).astype(np.float32))


def _ptr(a):
    return ctypes.pointer(a)


def test_new_symbols_declared_bound_and_reject_bad_arguments():
    lib = _lib.load()
    assert (_lib.RBM_MAX_DIM, _lib.RBM_MAX_STEPS) == (1024, 1 << 24)
    E_, p = _lib.GM_EINVAL, 64                                  # p: a non-null placeholder, never dereferenced here

    def chain(**kw):
        a = ops_fused.RbmChainArgs()
        a.W, a.WT, a.c, a.b, a.x, a.ldx = p, 2 * p, 3 * p, 4 * p, 5 * p, 16
        a.seed, a.n, a.I, a.H, a.steps, a.g_mul = 1, 4, 16, 8, 2, 1
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gm_rbm_chain(None, _ptr(a))
    for kw in (dict(W=None), dict(WT=None), dict(c=None), dict(b=None), dict(x=None), dict(WT=p), dict(ldx=15),
               dict(n=0), dict(row0=-1), dict(row0=(1 << 32) - 3), dict(I=0), dict(I=1025), dict(H=0), dict(H=1025),
               dict(steps=-1), dict(steps=(1 << 24) + 1), dict(g_mul=-1), dict(v0_out=6 * p, ldv0=15),
               dict(v_out=6 * p, ldv=15), dict(v_out=6 * p, ldv=16, v0_out=6 * p, ldv0=16), dict(p_out=6 * p, ldp=15),
               dict(p_out=5 * p, ldp=16), dict(a_out=6 * p, lda=15), dict(a_out=5 * p, lda=16),
               dict(a_out=6 * p, lda=16, p_out=6 * p, ldp=16), dict(p_out=6 * p, ldp=16, v_out=6 * p, ldv=16),
               dict(betas=7 * p), dict(betas=7 * p, b_A=8 * p), dict(b_A=8 * p, logw=9 * p),
               dict(betas=7 * p, b_A=8 * p, logw=9 * p, steps=0)):
        assert chain(**kw) == E_, kw
    assert b"bad argument" in lib.gm_last_error()
    assert lib.gm_rbm_chain(None, None) == E_
    # gm_rbm_grad(stream, pre, ldpre, V, ldv, b, dA, ldd, part, inv_b, B, I, H)
    ok = [p, 8, 2 * p, 16, 3 * p, 4 * p, 8, 5 * p, 0.25, 4, 16, 8]
    for i, v in ((0, None), (2, None), (4, None), (5, None), (7, None), (1, 7), (3, 15), (6, 7), (5, 2 * p), (9, 0),
                 (10, 0), (10, 1025), (11, 0), (11, 1025), (8, float("nan")), (8, -1.0)):
        bad = list(ok)
        bad[i] = v
        assert lib.gm_rbm_grad(None, *bad) == E_, (i, v)

    def vbias(**kw):
        a = ops_fused.RbmVbiasArgs()
        a.V, a.ldv, a.g, a.pb, a.mb, a.vb, a.sched, a.inv_b, a.B, a.I = p, 16, 2 * p, 3 * p, 4 * p, 5 * p, 6 * p, 0.25, 4, 16
        a.beta1, a.beta2, a.eps = 0.9, 0.999, 1e-8
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gm_rbm_vbias(None, _ptr(a))
    for kw in (dict(V=None), dict(ldv=15), dict(B=0), dict(I=0), dict(I=1025), dict(g=None, pb=None), dict(mb=None),
               dict(vb=None), dict(sched=None), dict(mb=5 * p), dict(mb=3 * p), dict(inv_b=float("inf"))):
        assert vbias(**kw) == E_, kw
    assert lib.gm_rbm_vbias(None, None) == E_
    # gm_rbm_transpose(stream, W, ldw, WT, ldt, rows, cols)
    ok = [p, 16, 2 * p, 8, 8, 16]
    for i, v in ((0, None), (2, None), (2, p), (1, 15), (3, 7), (4, 0), (4, 1025), (5, 0), (5, 1025)):
        bad = list(ok)
        bad[i] = v
        assert lib.gm_rbm_transpose(None, *bad) == E_, (i, v)
    # gm_rbm_uniform(stream, u, ldu, seed, tag, step_ctr, step_base, step_add, row0, rows, width)
    ok = [p, 16, 1, R.TAG_H, None, None, 0, 0, 4, 16]
    for i, v in ((0, None), (1, 15), (3, 0), (3, gmade.TAG_MS), (7, -1), (8, 0), (8, 1 << 31), (9, 0), (9, 1025),
                 (7, (1 << 32) - 3)):
        bad = list(ok)
        bad[i] = v
        assert lib.gm_rbm_uniform(None, *bad) == E_, (i, v)


def test_fused_and_general_path_selection():
    mk = lambda: rbm.RBM(16, 8)
    assert _trainer(mk())._stock()
    assert _trainer(rbm.RBM(15, 7), k=3, mode="pcd")._stock()    # odd widths stay on the fused path

    class Mine(rbm.RBMTrainer):
        def compute_batch(self, batch, train=True):
            return super().compute_batch(batch, train)
    assert not _trainer(mk(), Mine)._stock()
    tr = _trainer(mk())
    tr.evaluate = lambda it: 0.0                               # an instance attribute overrides a hook too
    assert not tr._stock()

    class MyRBM(rbm.RBM):
        pass
    assert not _trainer(MyRBM(16, 8))._stock()                 # a subclassed model
    m = mk()
    m.extra = nn.Linear(2, 2)                                  # an edited network
    assert not _trainer(m)._stock()
    m = mk()
    m.vbias = nn.Parameter(torch.zeros(15))                    # a bias of another shape
    assert not _trainer(m)._stock()
    assert _trainer(mk())._engine_class() is grbm.RBMEngine
    with pytest.raises(_lib.GMError):
        grbm.RBMEngine(MyRBM(16, 8), "cpu")                    # the engine itself refuses an edited model


def test_data_parallelism_and_cpu_runs_are_refused():
    tr = _trainer(rbm.RBM(16, 8))
    with pytest.raises(_lib.GMError):
        grbm.RBMEngine(tr.model, "cpu", world_size=2, rank=0)
    with pytest.raises(_lib.GMError):
        grbm.RBMEngine(tr.model, "cpu", force_dp=True)
    tr.force_dp = True
    tr._engine = None
    with pytest.raises(_lib.GMError):
        tr.train(1)
    with pytest.raises(_lib.GMError):
        tr.reconstruct_images(torch.zeros(2, 16), 0)
    if not torch.cuda.is_available():                          # no CPU fallback: a refusal, not an eager computation
        tr.force_dp = False
        for call in (lambda: tr.train(1), lambda: tr.sample(2, steps=1), lambda: tr.hidden(torch.zeros(2, 16)),
                     lambda: tr.model(torch.zeros(2, 16))):
            with pytest.raises(_lib.GMError):
                call()
