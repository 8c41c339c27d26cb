"""Denoising VAE without a GPU: module surface and state_dict round trip with the VAE, the numpy Philox / corruption
rule the GPU tests use as their reference, argument validation, the C-ABI of the new kernels and its refusals, fused /
general path selection and the data-parallel refusal."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import dvae  # noqa: E402
import vae  # noqa: E402
from generative_models_amd import _lib, ops_fused  # noqa: E402
from generative_models_amd import dvae as gdvae  # noqa: E402

# (the riding forms are the gather block of gm_linear_fwd_ex: gm_gather_args.corrupt / out_c)
M32 = 0xFFFFFFFF


def _loaders(n=40, batch=8, side=4):
    x = torch.bernoulli(torch.full((n, 1, side, side), 0.5))
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, **noise):
    tr = object.__new__(cls or dvae.DVAETrainer)      # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.noise, tr.level, tr.seed = gdvae.check_noise(noise.get("noise", "salt_pepper"), noise.get("level", 0.25),
                                                    noise.get("seed", 0))
    return tr


def test_module_surface_and_state_dict_round_trip_with_the_vae():
    torch.manual_seed(3)
    d = dvae.DVAE(16, 12, 4)
    torch.manual_seed(3)
    v = vae.VAE(16, 12, 4)
    assert [n for n, _ in d.named_modules()] == [n for n, _ in v.named_modules()]
    assert list(d.state_dict()) == list(v.state_dict())
    for k in v.state_dict():                                   # same construction order: same initial weights
        assert torch.equal(d.state_dict()[k], v.state_dict()[k]), k
    assert isinstance(d, vae.VAE) and dvae.Encoder is vae.Encoder and dvae.Decoder is vae.Decoder
    v2 = vae.VAE(16, 12, 4)
    v2.load_state_dict(d.state_dict())
    d2 = dvae.DVAE(16, 12, 4)
    d2.load_state_dict(v2.state_dict())
    for k, t in d2.state_dict().items():
        assert torch.equal(t, d.state_dict()[k]), k
    assert (d.image_size, d.hidden_dim, d.z_dim, d.shape) == (16, 12, 4, 4)
    for name in ("sample", "parzen", "denoise", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(dvae.DVAETrainer, name))
    assert dvae.DVAETrainer.sample is vae.VAETrainer.sample and dvae.DVAETrainer.parzen is vae.VAETrainer.parzen


def test_numpy_philox_known_answers():
    ph = lambda c, k: [int(v) for v in gdvae.philox4x32_10(np.array(c, np.uint64), np.array(k, np.uint64))]
    assert ph([0] * 4, [0] * 2) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert ph([M32] * 4, [M32] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert ph([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # vectorised: a batch of counters gives the same words as one call each
    ctr = np.array([[0, 0, 0, 0], [M32] * 4, [1, 2, 3, 4]], np.uint64)
    key = np.array([[0, 0], [M32, M32], [5, 6]], np.uint64)
    got = gdvae.philox4x32_10(ctr, key)
    for i in range(3):
        assert [int(v) for v in got[i]] == ph(list(ctr[i]), list(key[i]))


def test_corruption_words_follow_the_counter_layout():
    seed, step, row0 = (7 << 32) | 11, 5, 3
    w = gdvae.corruption_words(2, 10, seed, step, row0)
    assert w.shape == (2, 10) and w.dtype == np.uint32
    for r in range(2):
        for e in range(10):
            ref = gdvae.philox4x32_10(np.array([e >> 2, step, row0 + r, 0x44564145], np.uint64),
                                      np.array([11, 7], np.uint64))
            assert int(w[r, e]) == int(ref[e & 3]), (r, e)


def test_salt_pepper_thresholds():
    assert gdvae.sp_threshold(0.0) == 0
    assert gdvae.sp_threshold(0.5) == 1 << 30
    assert gdvae.sp_threshold(1.0) == 1 << 31
    assert gdvae.sp_threshold(0.25) == 1 << 29
    x = np.full((64, 100), 0.5, np.float32)
    words = gdvae.corruption_words(64, 100, 9, 2).astype(np.uint64)
    for p in (0.5, 1.0):
        y = gdvae.corrupt_reference(x, "salt_pepper", p, 9, 2)
        T = gdvae.sp_threshold(p)
        assert np.array_equal(y == 0.0, words < T)
        assert np.array_equal(y == 1.0, (words >= T) & (words < 2 * T))
        assert np.array_equal(y == 0.5, words >= 2 * T)
    y = gdvae.corrupt_reference(x, "salt_pepper", 1.0, 9, 2)
    assert set(np.unique(y)) <= {0.0, 1.0}                      # p = 1 replaces every pixel, by a fair coin
    y = gdvae.corrupt_reference(x, "salt_pepper", 0.5, 9, 2)
    assert abs((y != 0.5).mean() - 0.5) < 0.05


def test_level_zero_is_the_identity_and_gaussian_moves_every_pixel():
    x = np.random.RandomState(0).rand(5, 13).astype(np.float32)
    x[0, 0] = -0.0
    for noise in ("salt_pepper", "gaussian"):
        y = gdvae.corrupt_reference(x, noise, 0.0, 3, 4)
        assert y.tobytes() == x.tobytes()
    y = gdvae.corrupt_reference(x, "gaussian", 0.3, 3, 4)
    assert np.all(y != x) and abs(float((y - x).std()) - 0.3) < 0.15
    # different seeds / steps / rows give different words
    w = gdvae.corruption_words(3, 8, 1, 0)
    assert not np.array_equal(w, gdvae.corruption_words(3, 8, 2, 0))
    assert not np.array_equal(w, gdvae.corruption_words(3, 8, 1, 1))
    assert not np.array_equal(w[1:], gdvae.corruption_words(2, 8, 1, 0, row0=0))
    assert np.array_equal(w[1:], gdvae.corruption_words(2, 8, 1, 0, row0=1))


@pytest.mark.parametrize("bad", [dict(noise="pepper"), dict(noise=None), dict(level=float("nan")),
                                 dict(level=float("inf")), dict(level=-0.1), dict(level=1.5), dict(level="x"),
                                 dict(noise="gaussian", level=-1.0), dict(noise="gaussian", level=float("inf")),
                                 dict(noise="gaussian", level=1e39), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5),
                                 dict(seed=True), dict(level=True)])
def test_bad_noise_settings_raise_before_anything_runs(bad):
    kw = dict(noise="salt_pepper", level=0.25, seed=0)
    kw.update(bad)
    with pytest.raises(ValueError) as e:
        dvae.DVAETrainer(None, None, None, None, **kw)           # raises before touching the model or the loaders
    assert isinstance(e.value, _lib.GMError)
    with pytest.raises(ValueError):
        dvae.corrupt(torch.zeros(2, 4), **kw)
    gdvae.check_noise("gaussian", 7.5, (1 << 64) - 1)
    gdvae.check_noise("salt_pepper", 1, 0)


def test_noise_settings_are_keyword_only():
    import inspect
    sig = inspect.signature(dvae.DVAETrainer.__init__).parameters
    assert list(sig)[1:] == ["model", "train_iter", "val_iter", "test_iter", "viz", "noise", "level", "seed"]
    for k in ("noise", "level", "seed"):
        assert sig[k].kind == inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(dvae.corrupt).parameters
    assert list(sig) == ["images", "noise", "level", "seed", "step", "row0"]


def test_new_symbols_declared_bound_and_reject_bad_arguments():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("libgm_hip.so not built")
    lib = _lib.load()
    E = _lib.GM_EINVAL
    p = 64                                                      # a non-null placeholder; never dereferenced here
    ok = ops_fused.corrupt_args("salt_pepper", 0.5, 1)

    def args(**kw):
        a = ops_fused.corrupt_args("salt_pepper", 0.5, 1)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    bad_args = [None, args(kind=3), args(kind=-1), args(level=float("nan")), args(level=-0.5), args(level=1.5),
                args(kind=2, level=float("inf")), args(kind=2, level=1e39), args(row0=-1)]
    by = lambda a: a if a is None else _ptr(a)
    for a in bad_args:
        assert lib.gm_dvae_corrupt(None, by(a), p, 8, 2 * p, 8, 4, 8) == E
        assert lib.gm_gather_rows_corrupt(None, by(a), p, 16, p, _lib.NO_SLOT, 2 * p, 3 * p, 8, 4, 8) == E
    c = _ptr(ok)
    for bad in ((None, 8, 2 * p, 8, 4, 8), (p, 8, None, 8, 4, 8), (p, 8, 2 * p, 8, -1, 8), (p, 4, 2 * p, 8, 4, 8),
                (p, 8, 2 * p, 4, 4, 8), (p, 8, 2 * p, 8, 4, 0), (p, 8, p, 12, 4, 8)):
        assert lib.gm_dvae_corrupt(None, c, *bad) == E, bad
    assert lib.gm_dvae_corrupt(None, c, p, 8, 2 * p, 8, 0, 8) == 0          # no rows: nothing to launch
    S = _lib.NO_SLOT
    for bad in ((None, 16, p, S, 2 * p, 3 * p, 8, 4, 8), (p, 16, None, S, 2 * p, 3 * p, 8, 4, 8),
                (p, 16, p, S, None, 3 * p, 8, 4, 8), (p, 16, p, S, 2 * p, None, 8, 4, 8),
                (p, 16, p, S, 2 * p, 2 * p, 8, 4, 8), (p, 16, p, S, 2 * p, 3 * p, 4, 4, 8),
                (p, 16, p, S, 2 * p, 3 * p, 8, 0, 8), (p, 0, p, S, 2 * p, 3 * p, 8, 4, 8),
                (p, 16, p, S, 2 * p, p, 8, 4, 8)):
        assert lib.gm_gather_rows_corrupt(None, c, *bad) == E, bad
    for bad in ((None, 1, 16, p, S, 2 * p, 3 * p, 8, 4, 8), (p, 1, 16, p, S, 2 * p, None, 8, 4, 8),
                (p, 0, 16, p, S, 2 * p, 3 * p, 40, 4, 40), (p, 1, 16, p, S, 2 * p, 3 * p, 4, 4, 8),
                (p, 1, 16, p, S, 2 * p, 2 * p, 8, 4, 8)):
        assert lib.gm_gather_rows_bits_corrupt(None, c, *bad) == E, bad
    assert lib.gm_gather_rows_bits_corrupt(None, None, p, 1, 16, p, S, 2 * p, 3 * p, 8, 4, 8) == E
    # the riding forms: the gather's refusals, and out_c may not be an operand or the output of the GEMM
    X, W, Y = 5 * p, 6 * p, 7 * p
    def ride(out_c, corrupt, bits=False, ld_out=8):
        g = _lib.GatherArgs(n_rows=16, idx=p, idx_slot=S, out=2 * p, ld_out=ld_out, B=4, row_elems=8, out_c=out_c)
        if bits:
            g.bits, g.words_per_row = p, 1
        else:
            g.data = p
        if corrupt is not None:
            g.corrupt = corrupt
        a = _lib.FwdArgs(X=X, ldx=8, x_slot=S, W=W, Y=Y, ldy=8, M=4, K=8, N=8, act=1, gather=_ptr(g))
        return lib.gm_linear_fwd_ex(None, _ptr(a))
    for out_c in (None, X, Y, 2 * p):
        assert ride(out_c, c) == E, out_c
        assert ride(out_c, c, bits=True) == E
    assert ride(3 * p, None) == E
    assert ride(3 * p, _ptr(args(kind=9))) == E
    assert ride(3 * p, c, ld_out=4) == E   # ld < row


def _ptr(a):
    import ctypes
    return ctypes.pointer(a)


def test_fused_and_general_path_selection():
    mk = lambda: dvae.DVAE(16, 8, 4)
    assert _trainer(mk())._stock()
    assert _trainer(mk(), noise="gaussian", level=0.0)._stock()

    class Mine(dvae.DVAETrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    assert not _trainer(mk(), Mine)._stock()
    tr = _trainer(mk())
    tr.compute_batch = lambda batch: None                      # an instance attribute overrides a hook too
    assert not tr._stock()

    class MyEnc(dvae.Encoder):
        pass
    m = mk()
    m.encoder = MyEnc(16, 8, 4)                                # a subclassed module
    assert not _trainer(m)._stock()
    m = mk()
    m.decoder.extra = nn.Linear(2, 2)                          # an edited network
    assert not _trainer(m)._stock()

    class MyDVAE(dvae.DVAE):
        pass
    assert not _trainer(MyDVAE(16, 8, 4))._stock()
    from generative_models_amd.engine import DVAEEngine
    tr = _trainer(mk())
    assert tr._engine_class() is DVAEEngine and tr._engine_kwargs() == {"trainer": tr}


def test_data_parallelism_is_refused():
    from generative_models_amd.engine import DVAEEngine
    with pytest.raises(_lib.GMError):
        DVAEEngine(dvae.DVAE(16, 8, 4), "cpu", world_size=2, rank=0)
    with pytest.raises(_lib.GMError):
        DVAEEngine(dvae.DVAE(16, 8, 4), "cpu", force_dp=True)
    tr = _trainer(dvae.DVAE(16, 8, 4))
    tr.force_dp = True
    tr._engine = None
    with pytest.raises(_lib.GMError):
        tr.train(1)
    assert tr._engine is None
