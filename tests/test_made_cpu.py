"""The masked autoregressive model without a GPU: module surface and state_dict keys, the degrees and the autoregressive
property of the masks, masked entries at construction, normalisation of the fp64 reference over all 1024 images of a
10-pixel model, known answers of the uniform rule, argument validation, the C-ABI of the new kernels and its refusals,
fused / general path selection, the data-parallel refusal, and the undecided-pixel counts of the sampler cases the GPU
file runs."""
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

import made  # noqa: E402
import made_reference as R  # noqa: E402
from generative_models_amd import _lib, metrics, ops_fused  # noqa: E402
from generative_models_amd import dvae as gdvae  # noqa: E402
from generative_models_amd import made as gmade  # noqa: E402



def _loaders(n=40, batch=8, side=4):
    x = torch.bernoulli(torch.full((n, 1, side, side), 0.5))
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None):
    tr = object.__new__(cls or made.MADETrainer)      # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    return tr


def test_module_surface_and_state_dict_keys():
    m = made.MADE(16, 12)
    assert sorted(m.state_dict()) == sorted(R.KEYS)
    assert (tuple(m.linear.weight.shape), tuple(m.out.weight.shape)) == ((12, 16), (16, 12))
    assert (m.image_size, m.hidden_dim, m.order, m.order_seed, m.shape) == (16, 12, "natural", 0, 4)
    assert m.m_in.dtype == torch.int32 and m.m_h.dtype == torch.int32
    assert {n for n, _ in m.named_buffers()} == {"m_in", "m_h"}      # no mask matrix is stored
    sig = inspect.signature(made.MADE.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("image_size", 784), ("hidden_dim", 400),
                                                                  ("order", "natural"), ("order_seed", 0)]
    sig = inspect.signature(made.MADETrainer.train).parameters
    assert (sig["lr"].default, sig["weight_decay"].default) == (1e-3, 0.0)
    sig = inspect.signature(made.MADETrainer.sample).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("n", inspect.Parameter.empty), ("seed", 0),
                                                                  ("return_probs", False)]
    sig = inspect.signature(made.MADETrainer.complete).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("images", inspect.Parameter.empty),
                                                                  ("n_known", inspect.Parameter.empty), ("seed", 0),
                                                                  ("return_probs", False)]
    assert inspect.signature(made.MADETrainer.log_likelihood).parameters["images"].default is None
    for name in ("sample", "complete", "log_likelihood", "parzen", "generate_images", "sample_images", "save_checkpoint",
                 "load_checkpoint"):
        assert callable(getattr(made.MADETrainer, name))
    assert metrics.NLLResult._fields == ("ll_mean", "ll_stderr", "n")
    assert issubclass(made.MADEError, _lib.GMError) and issubclass(made.MADEError, ValueError)
    import generative_models_amd as pkg
    assert pkg.MADE is gmade.MADE and pkg.MADETrainer is gmade.MADETrainer and pkg.MADEEngine is gmade.MADEEngine
    from generative_models_amd.engine import VAEEngine
    from generative_models_amd.trainers import VAETrainer
    assert issubclass(gmade.MADEEngine, VAEEngine) and issubclass(gmade.MADETrainer, VAETrainer)
    for f in ("_buffers", "_issue", "configure"):    # _alloc, the guard around _buffers, is the shared base's
        assert f in gmade.MADEEngine.__dict__
    # a checkpoint carries the order: the degrees travel in the state_dict
    m2 = made.MADE(16, 12, order="random", order_seed=3)
    m.load_state_dict(m2.state_dict())
    assert torch.equal(m.m_in, m2.m_in) and not torch.equal(m.m_in, made.MADE(16, 12).m_in)


@pytest.mark.parametrize("I,H", [(2, 1), (10, 7), (49, 32), (784, 400), (8192, 1024)])
def test_degrees(I, H):
    st, nst = torch.get_rng_state(), np.random.get_state()[1].copy()
    for order in ("natural", "random"):
        m_in, m_h = gmade.degrees(I, H, order, 4)
        rin, rh = R.degrees(I, H, order, 4)
        assert m_in.dtype == np.int32 and m_h.dtype == np.int32
        assert np.array_equal(m_in, rin) and np.array_equal(m_h, rh)
        assert np.array_equal(np.sort(m_in), np.arange(1, I + 1))                  # a permutation of 1 .. I
        assert np.all(np.diff(m_h) >= 0) and m_h.min() >= 1 and m_h.max() <= I - 1   # ascending, in [1, I - 1]
        assert m_h[0] == 1
        inv = gmade.inverse_order(m_in)
        assert np.array_equal(m_in[inv], np.arange(1, I + 1))
    assert np.array_equal(gmade.degrees(I, H)[0], np.arange(1, I + 1))
    if I > 4:
        assert not np.array_equal(gmade.degrees(I, H, "random", 0)[0], gmade.degrees(I, H, "random", 1)[0])
    assert torch.equal(st, torch.get_rng_state()) and np.array_equal(nst, np.random.get_state()[1])   # untouched
    if I <= 784:
        m = made.MADE(I, H, "random", 4)
        assert np.array_equal(m.m_in.numpy(), R.degrees(I, H, "random", 4)[0]) and np.array_equal(m.m_h.numpy(), rh)


@pytest.mark.parametrize("order", ["natural", "random"])
@pytest.mark.parametrize("I,H", [(2, 1), (10, 7), (49, 32), (784, 400)])
def test_masks_are_autoregressive(I, H, order):
    m_in, m_h = gmade.degrees(I, H, order, 2)
    M1, M2 = gmade.masks(m_in, m_h)
    r1, r2 = R.masks(m_in, m_h)
    assert M1.shape == (H, I) and M2.shape == (I, H)
    assert np.array_equal(M1, r1.numpy() != 0) and np.array_equal(M2, r2.numpy() != 0)
    paths = M2.astype(np.int64) @ M1.astype(np.int64)              # paths[d, i]: hidden units joining pixel i to output d
    allowed = m_in[None, :] < m_in[:, None]                        # allowed[d, i] = m_in[i] < m_in[d]
    assert not np.any(paths[~allowed])                             # no path unless the pixel comes strictly before
    first = int(np.argmin(m_in))
    assert not paths[first].any()                                  # the pixel of degree 1 sees nothing
    # the model's own masks (torch, from its buffers) are the same
    if I <= 49:
        m = made.MADE(I, H, order, 2)
        t1, t2 = m.masks()
        assert torch.equal(t1, r1.float()) and torch.equal(t2, r2.float())


@pytest.mark.parametrize("order", ["natural", "random"])
def test_masked_entries_are_zero_after_construction(order):
    torch.manual_seed(0)
    m = made.MADE(49, 32, order, 1)
    M1, M2 = R.masks(m.m_in.numpy(), m.m_h.numpy())
    assert torch.all(m.linear.weight[M1 == 0] == 0.0) and torch.all(m.out.weight[M2 == 0] == 0.0)
    assert torch.all(m.linear.weight[M1 == 1] != 0.0) and torch.all(m.out.weight[M2 == 1] != 0.0)


@pytest.mark.parametrize("order", ["natural", "random"])
def test_reference_is_normalised_over_all_images(order):
    """I = 10, H = 7, random weights, fp64: sum over all 1024 images of exp(ll) = 1 to 1e-12 -- and not with one mask
    entry opened."""
    I, H = 10, 7
    torch.manual_seed(1)
    m_in, m_h = R.degrees(I, H, order, 3)
    M = R.masks(m_in, m_h)
    P = {"linear.weight": torch.randn(H, I, dtype=torch.float64) * M[0], "linear.bias": torch.randn(H, dtype=torch.float64),
         "out.weight": torch.randn(I, H, dtype=torch.float64) * M[1], "out.bias": torch.randn(I, dtype=torch.float64)}
    x = torch.tensor([[(v >> i) & 1 for i in range(I)] for v in range(1 << I)], dtype=torch.float64)
    total = torch.exp(-R.nll_rows(R.logits(P, x), x)).sum().item()
    assert abs(total - 1.0) <= 1e-12, total
    # the free-running sampler's conditionals are the teacher-forced ones of its own sample
    u = R.uniforms(16, I, 7)
    xs, ps = R.free_running(P, m_in, u)
    assert (ps - R.teacher_forced(P, xs)).abs().max().item() <= 1e-13
    bad = {k: v.clone() for k, v in P.items()}
    d = int(np.argmin(m_in))
    bad["out.weight"][d, 0] = 1.0                                  # the first pixel now sees something
    bad["linear.weight"][0, int(np.argsort(m_in)[0])] = 1.0
    assert abs(torch.exp(-R.nll_rows(R.logits(bad, x), x)).sum().item() - 1.0) > 1e-6


def test_loss_reference_and_general_loss_agree():
    a = torch.tensor([[-30.0, -1.0, 0.0, 2.5, 30.0]], dtype=torch.float64)
    x = torch.tensor([[1.0, 0.0, 1.0, 1.0, 0.0]], dtype=torch.float64)
    want = -(x * torch.log(torch.sigmoid(a)) + (1 - x) * torch.log(torch.sigmoid(-a))).sum(1)
    assert (R.nll_rows(a, x) - want).abs().max().item() <= 1e-12
    assert (gmade.nll_rows(a, x) - want).abs().max().item() <= 1e-12
    direct = (torch.clamp(a, min=0) + torch.log1p(torch.exp(-a.abs())) - x * a).sum(1)     # the contract's formula
    assert (R.nll_rows(a, x) - direct).abs().max().item() <= 1e-12
    _, _, da = R.loss_and_grads({"linear.weight": torch.zeros(3, 5), "linear.bias": torch.zeros(3),
                                 "out.weight": torch.zeros(5, 3), "out.bias": a[0].clone()},
                                x, (torch.ones(3, 5, dtype=torch.float64), torch.ones(5, 3, dtype=torch.float64)))
    assert (da - (torch.sigmoid(a) - x)).abs().max().item() <= 1e-15        # d loss / d a = (sigmoid(a) - x) / b


def test_uniform_rule_known_answers():
    seed = 0x0123456789ABCDEF
    u = gmade.uniforms_reference(3, 10, seed)                    # I = 10: a partial third Philox word group
    assert u.dtype == np.float32 and u.shape == (3, 10) and np.array_equal(u, R.uniforms(3, 10, seed))
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    for r in range(3):
        for d in range(10):
            w = gdvae.philox4x32_10(np.array([d >> 2, 0, r, 0x4D414453], np.uint64), key)
            assert u[r, d] == np.float32((2 * (int(w[d & 3]) >> 9) + 1) * 2.0 ** -24)
    assert gmade.TAG_MS == 0x4D414453 == int.from_bytes(b"MADS", "big")
    assert 0.0 < u.min() and u.max() < 1.0
    # the Philox known answer the other counter streams' tests pin (Random123's kat_vectors: counter 0, key 0)
    z4 = gdvae.philox4x32_10(np.zeros(4, np.uint64), np.zeros(2, np.uint64))
    assert [int(v) for v in z4] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    a = gmade.uniforms_reference(4, 8, 1)
    assert np.array_equal(a[2:], gmade.uniforms_reference(2, 8, 1, row0=2))         # rows are counters
    assert np.array_equal(a[:, :5], gmade.uniforms_reference(4, 5, 1))              # so are pixels
    assert not np.array_equal(a, gmade.uniforms_reference(4, 8, 2))
    big = gmade.uniforms_reference(64, 784, 3)
    assert abs(big.mean() - 0.5) <= 5 / (12 * big.size) ** 0.5
    from generative_models_amd import ddpm as gddpm
    from generative_models_amd import iwae as giwae
    tags = {gmade.TAG_MS, gddpm.TAG_T, gddpm.TAG_E, gddpm.TAG_V, gddpm.TAG_VE, gddpm.TAG_S, gdvae.CTR_TAG,
            giwae.TAG_TRAIN, giwae.TAG_EVAL, 0}
    assert len(tags) == 10                                       # distinct streams


@pytest.mark.parametrize("bad", [dict(image_size=1), dict(image_size=8193), dict(image_size=16.0), dict(image_size=True),
                                 dict(hidden_dim=0), dict(hidden_dim=1025), dict(hidden_dim="8"), dict(order="reverse"),
                                 dict(order=None), dict(order_seed=-1), dict(order_seed=1 << 32), dict(order_seed=0.5)])
def test_bad_model_arguments_raise(bad):
    kw = dict(dict(image_size=16, hidden_dim=8), **bad)
    with pytest.raises(ValueError) as ei:
        made.MADE(**kw)
    assert isinstance(ei.value, _lib.GMError) and isinstance(ei.value, made.MADEError)


def test_limits_are_accepted():
    assert made.MADE(2, 1).m_h.tolist() == [1]
    assert gmade.check_shape(8192, 1024) == (8192, 1024)


def test_bad_seed_n_and_n_known_raise_before_anything_runs():
    tr = _trainer(made.MADE(16, 8))
    for kw in (dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(seed=None), dict(seed=False), dict(n=0),
               dict(n=2.5), dict(n=True)):
        with pytest.raises(ValueError) as ei:
            tr.sample(**dict(dict(n=4), **kw))
        assert isinstance(ei.value, _lib.GMError), kw
    for kw in (dict(n_known=-1), dict(n_known=17), dict(n_known=1.0), dict(n_known=True), dict(seed=-1)):
        with pytest.raises(ValueError) as ei:
            tr.complete(torch.zeros(2, 16), **dict(dict(n_known=3), **kw))
        assert isinstance(ei.value, _lib.GMError), kw
    with pytest.raises(ValueError):
        tr.complete(torch.zeros(2, 15), 3)                       # another image size
    assert gmade.check_seed((1 << 64) - 1) == (1 << 64) - 1 and gmade.check_known(np.int64(16), 16) == 16
    with pytest.raises(ValueError):
        gmade.inverse_order(np.array([1, 1, 3]))


def _ptr(a):
    return ctypes.pointer(a)


def test_new_symbols_declared_bound_and_reject_bad_arguments():
    lib = _lib.load()
    assert (_lib.MADE_TAG_S, _lib.MADE_MIN_I, _lib.MADE_MAX_I, _lib.MADE_MAX_H) == (0x4D414453, 2, 8192, 1024)
    E_, p = _lib.GM_EINVAL, 64                                  # p: a non-null placeholder, never dereferenced here
    # gm_made_bce(stream, logits, lda, x, ldx, dA, ldd, part, scale, B, I)
    ok = [p, 16, 2 * p, 16, 3 * p, 16, 4 * p, 0.25, 4, 16]
    for i, v in ((0, None), (2, None), (6, None), (1, 15), (3, 15), (5, 15), (4, 2 * p), (8, 0), (9, 0), (9, 8193),
                 (7, float("nan")), (7, float("inf")), (7, -1.0)):
        bad = list(ok)
        bad[i] = v
        assert lib.gm_made_bce(None, *bad) == E_, (i, v)
    assert b"bad argument" in lib.gm_last_error()

    # gm_made_mask(stream, args)
    def mask(**kw):
        a = ops_fused.MadeMaskArgs()
        a.W1, a.m1, a.v1, a.W2, a.m2, a.v2, a.m_in, a.m_h, a.I, a.H = p, 2 * p, 3 * p, 4 * p, 5 * p, 6 * p, 7 * p, 8 * p, 16, 8
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gm_made_mask(None, _ptr(a))
    for kw in (dict(W1=None), dict(W2=None), dict(m_in=None), dict(m_h=None), dict(I=1), dict(I=8193), dict(H=0),
               dict(H=1025), dict(m1=None), dict(v1=None), dict(m2=None), dict(v2=None), dict(W2=p)):
        assert mask(**kw) == E_, kw
    assert lib.gm_made_mask(None, None) == E_

    # gm_made_sample(stream, args)
    def samp(**kw):
        a = ops_fused.MadeSampleArgs()
        a.W2, a.b2, a.W1T, a.b1, a.m_h, a.inv_order, a.x, a.ldx = p, 2 * p, 3 * p, 4 * p, 5 * p, 6 * p, 7 * p, 16
        a.seed, a.n, a.I, a.H, a.n_known = 1, 4, 16, 8, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.gm_made_sample(None, _ptr(a))
    for kw in (dict(W2=None), dict(b2=None), dict(W1T=None), dict(b1=None), dict(m_h=None), dict(inv_order=None),
               dict(x=None), dict(ldx=15), dict(n=0), dict(n=(1 << 32) + 1), dict(I=1), dict(I=8193), dict(H=0),
               dict(H=1025), dict(n_known=-1), dict(n_known=17), dict(n_known=3), dict(n_known=3, given=8 * p, ldg=15),
               dict(n_known=3, given=7 * p, ldg=16), dict(p=8 * p, ldp=15), dict(p=7 * p, ldp=16),
               dict(n_known=16, given=8 * p, ldg=16, p=8 * p, ldp=16)):
        assert samp(**kw) == E_, kw
    assert lib.gm_made_sample(None, None) == E_
    # gm_made_uniform(stream, u, ldu, seed, row0, rows, I)
    ok = [p, 16, 1, 0, 4, 16]
    for i, v in ((0, None), (1, 15), (3, -1), (4, 0), (4, 1 << 31), (5, 0), (5, 8193), (3, (1 << 32) - 3)):
        bad = list(ok)
        bad[i] = v
        assert lib.gm_made_uniform(None, *bad) == E_, (i, v)


def test_fused_and_general_path_selection():
    mk = lambda: made.MADE(16, 8)
    assert _trainer(mk())._stock()
    assert _trainer(made.MADE(15, 7, "random", 2))._stock()      # odd widths stay on the fused path (element paths)

    class Mine(made.MADETrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    assert not _trainer(mk(), Mine)._stock()
    tr = _trainer(mk())
    tr.evaluate = lambda it: 0.0                               # an instance attribute overrides a hook too
    assert not tr._stock()

    class MyMADE(made.MADE):
        pass
    assert not _trainer(MyMADE(16, 8))._stock()                # a subclassed model
    m = mk()
    m.extra = nn.Linear(2, 2)                                  # an edited network
    assert not _trainer(m)._stock()
    m = mk()
    m.out = nn.Linear(8, 15)                                   # a layer of another shape
    assert not _trainer(m)._stock()
    m = mk()
    m.m_h = m.m_h.long()                                       # degree buffers of another type
    assert not _trainer(m)._stock()
    assert _trainer(mk())._engine_class() is gmade.MADEEngine
    with pytest.raises(_lib.GMError):
        gmade.MADEEngine(MyMADE(16, 8), "cpu")                 # the engine itself refuses an edited model


def test_data_parallelism_is_refused():
    tr = _trainer(made.MADE(16, 8))
    with pytest.raises(_lib.GMError):
        gmade.MADEEngine(tr.model, "cpu", world_size=2, rank=0)
    with pytest.raises(_lib.GMError):
        gmade.MADEEngine(tr.model, "cpu", force_dp=True)
    tr.force_dp = True
    tr._engine = None
    with pytest.raises(_lib.GMError):
        tr.train(1)
    with pytest.raises(_lib.GMError):
        tr.reconstruct_images(torch.zeros(2, 16), 0)


@pytest.mark.parametrize("case", list(R.SAMPLER_CASES))
def test_sampler_cases_stay_inside_the_undecided_cap(case):
    """What tests/test_gpu_made.py relies on, with the reference alone: under each case's weights and seed the fp64
    free-running sample has at most 0.1 % undecided pixels (|u - p64| <= 1e-5), at least 90 % of its rows have none, and
    every logit stays within +-8."""
    n, I, H, order, seed = R.SAMPLER_CASES[case]
    sd, P, m_in = R.case_weights(I, H, order)
    assert np.array_equal(sd["m_in"].numpy(), gmade.degrees(I, H, order, R.ORDER_SEED)[0])
    M1, M2 = R.masks(m_in, sd["m_h"].numpy())
    assert torch.all(P["linear.weight"][M1 == 0] == 0) and torch.all(P["out.weight"][M2 == 0] == 0)
    u = R.uniforms(n, I, seed)
    x, p = R.free_running(P, m_in, u)
    a = torch.log(p) - torch.log1p(-p)
    assert a.abs().max().item() <= 8.0, a.abs().max().item()
    und = R.undecided(u, p.numpy())
    print(case, "undecided pixels", int(und.sum()), "of", und.size, "rows without", int((~und.any(1)).sum()), "of", n)
    assert und.sum() <= R.UNDECIDED_CAP * und.size
    assert (~und.any(1)).sum() >= 0.9 * n
    assert 0.02 < x.mean().item() < 0.98                        # neither all dark nor all lit: the decisions matter
