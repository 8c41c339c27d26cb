"""The VQ-VAE without a GPU: module surface, signatures, defaults and state_dict keys, vae.py's Decoder reused, the
refusals (constructor, beta, codes, bits, prior sizes, data parallel, iwae.log_likelihood), the fp64 reference's closed
forms (dml, dE) against autograd on the stop-gradient loss, code_bits / bits_code, the C-ABI of the three new kernels and
its refusals, struct and limit mirrors, the checkpoint config and fused / general path selection."""
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

import vae  # noqa: E402
import vq_vae  # noqa: E402
import vqvae_reference as R  # noqa: E402
from generative_models_amd import _lib, metrics, ops_fused  # noqa: E402
from generative_models_amd import iwae as giwae  # noqa: E402
from generative_models_amd import vqvae as gvq  # noqa: E402



def _loaders(n=40, batch=8, side=4):
    x = torch.bernoulli(torch.full((n, 1, side, side), 0.5))
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, beta=0.25):
    tr = object.__new__(cls or vq_vae.VQVAETrainer)      # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.k, tr.seed, tr.beta, tr.noise_steps, tr.prior, tr._engine = 1, 0, beta, 0, None, None
    return tr


def test_module_surface_and_state_dict_keys():
    m = vq_vae.VQVAE(16, 12, 3, 4, 8)
    assert list(m.state_dict()) == list(R.KEYS)
    assert tuple(m.encoder.embed.weight.shape) == (12, 12) and tuple(m.codebook.weight.shape) == (8, 4)
    assert tuple(m.decoder.linear.weight.shape) == (12, 12) and m.z_dim == 12
    assert type(m.decoder) is vae.Decoder and vq_vae.Decoder is vae.Decoder              # vae.py's Decoder reused
    assert vq_vae.Encoder is gvq.Encoder and vq_vae.Encoder is not vae.Encoder
    cb = m.codebook.weight.detach()
    assert float(cb.abs().max()) <= 1.0 / 8 and float(cb.std()) > 0.0
    sig = inspect.signature(vq_vae.VQVAE.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [
        ("image_size", 784), ("hidden_dim", 400), ("num_vars", 16), ("code_dim", 16), ("num_codes", 128)]
    sig = inspect.signature(vq_vae.VQVAETrainer.__init__).parameters
    assert list(sig)[1:] == ["model", "train_iter", "val_iter", "test_iter", "viz", "beta"]
    assert sig["beta"].default == 0.25 and sig["beta"].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(vq_vae.VQVAETrainer.train).parameters
    assert (sig["lr"].default, sig["weight_decay"].default) == (1e-3, 1e-5)
    sig = inspect.signature(vq_vae.VQVAETrainer.fit_prior).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [
        ("num_epochs", 5), ("hidden_dim", 400), ("lr", 1e-3), ("batch_size", 512), ("order", "natural")]
    for name in ("codes", "decode", "reconstruct", "code_usage", "fit_prior", "sample", "parzen", "log_likelihood",
                 "save_checkpoint", "load_checkpoint", "compute_batch", "evaluate"):
        assert callable(getattr(vq_vae.VQVAETrainer, name)), name
    for name in ("Encoder", "Decoder", "VQVAE", "VQVAETrainer", "VQVAEError", "code_bits", "bits_code", "get_data",
                 "to_cuda"):
        assert hasattr(vq_vae, name), name
    assert issubclass(gvq.VQVAEError, _lib.GMError) and issubclass(gvq.VQVAEError, ValueError)
    import generative_models_amd as pkg
    from generative_models_amd.engine import IWAEEngine, VQVAEEngine
    assert pkg.VQVAE is gvq.VQVAE and pkg.VQVAETrainer is gvq.VQVAETrainer and pkg.VQVAEEngine is VQVAEEngine
    assert issubclass(VQVAEEngine, IWAEEngine) and issubclass(gvq.VQVAETrainer, giwae.IWAETrainer)
    for f in ("_head", "_extra_params", "_sample", "_reduce", "_second_sum", "_settings"):
        assert f in VQVAEEngine.__dict__, f
    assert gvq.__doc__ and "argmin" in gvq.__doc__ and "2 (n_k E_k - s_k)" in gvq.__doc__
    assert metrics.VQResult._fields == ("ll_mean", "ll_stderr", "recon_mean", "prior_mean", "n")
    assert vq_vae.VQVAETrainer._series == (("losses", "recon"), ("vq_loss", "kl"))


@pytest.mark.parametrize("kw", [dict(num_vars=0), dict(num_vars=2.0), dict(num_vars=True), dict(code_dim=0),
                                dict(code_dim="4"), dict(num_codes=1), dict(num_codes=8.0), dict(num_codes=None)])
def test_bad_sizes_are_refused(kw):
    with pytest.raises(gvq.VQVAEError):
        vq_vae.VQVAE(16, 12, **dict(dict(num_vars=3, code_dim=4, num_codes=8), **kw))
    with pytest.raises(ValueError):
        vq_vae.VQVAE(16, 12, **dict(dict(num_vars=3, code_dim=4, num_codes=8), **kw))


@pytest.mark.parametrize("beta", [-0.1, float("nan"), float("inf"), "x", None])
def test_bad_beta_is_refused(beta):
    with pytest.raises(gvq.VQVAEError):
        vq_vae.VQVAETrainer(vq_vae.VQVAE(16, 12, 3, 4, 8), *_loaders(), beta=beta)
    tr = _trainer(vq_vae.VQVAE(16, 12, 3, 4, 8), beta=beta)
    with pytest.raises(gvq.VQVAEError):
        tr.train(1)                                      # a beta changed after construction is checked again
    assert gvq.check_beta(0) == 0.0 and gvq.check_beta(np.float32(0.5)) == 0.5


@pytest.mark.parametrize("K", [2, 4, 128, 1024])
def test_code_bits_round_trip(K):
    L = K.bit_length() - 1
    gen = torch.Generator().manual_seed(K)
    c = torch.randint(0, K, (37, 5), generator=gen)
    c[0], c[1] = 0, K - 1
    b = vq_vae.code_bits(c, K)
    assert b.shape == (37, 5 * L) and b.dtype == torch.float32 and set(b.unique().tolist()) <= {0.0, 1.0}
    assert torch.equal(vq_vae.bits_code(b, K), c) and vq_vae.bits_code(b, K).dtype == torch.int64
    assert torch.equal(vq_vae.bits_code(b.to(torch.int32), K), c)
    # most significant first, variable n in bits n L .. n L + L - 1
    v = int(c[5, 3])
    assert b[5, 3 * L:4 * L].tolist() == [float((v >> (L - 1 - i)) & 1) for i in range(L)]
    assert torch.all(b[0] == 0.0) and torch.all(b[1] == 1.0)
    # every bit pattern is a valid code
    pat = (torch.rand(50, 5 * L, generator=gen) < 0.5).float()
    cc = vq_vae.bits_code(pat, K)
    assert int(cc.min()) >= 0 and int(cc.max()) < K and torch.equal(vq_vae.code_bits(cc, K), pat)


def test_bits_refusals():
    ok = torch.zeros(4, 3, dtype=torch.int64)
    for K in (5, 1, 0, 6.0, True):
        with pytest.raises(gvq.VQVAEError):
            vq_vae.code_bits(ok, K)
        with pytest.raises(gvq.VQVAEError):
            vq_vae.bits_code(torch.zeros(4, 6), K)
    for bad in (ok.float(), ok - 1, ok + 8, ok == 0, ok[0]):
        with pytest.raises(gvq.VQVAEError):
            vq_vae.code_bits(bad, 8)
    for bad in (torch.zeros(4, 7), torch.full((4, 6), 0.5), torch.full((4, 6), 2), torch.zeros(6)):
        with pytest.raises(gvq.VQVAEError):
            vq_vae.bits_code(bad, 8)


def test_prior_sizes_are_checked_before_anything_runs():
    with pytest.raises(gvq.VQVAEError, match="power of two"):
        _trainer(vq_vae.VQVAE(16, 12, 3, 4, 5)).fit_prior(1)
    with pytest.raises(gvq.VQVAEError, match="MADE"):
        _trainer(vq_vae.VQVAE(16, 12, 1, 4, 2)).fit_prior(1)                 # 1 bit: below MADE's smallest image
    with pytest.raises(gvq.VQVAEError, match="MADE"):
        _trainer(vq_vae.VQVAE(16, 12, 1024, 4, 512)).fit_prior(1)            # 9216 bits: above its largest
    tr = _trainer(vq_vae.VQVAE(16, 12, 3, 4, 8))
    with pytest.raises(_lib.GMError, match="fit_prior"):
        tr.log_likelihood(torch.zeros(2, 16))
    assert tr.prior_state is None


@pytest.mark.parametrize("N,D,K,B", [(1, 4, 2, 7), (3, 4, 5, 7), (7, 8, 33, 33), (16, 16, 128, 40)])
def test_closed_forms_equal_autograd_on_the_stop_gradient_loss(N, D, K, B):
    gen = torch.Generator().manual_seed(1000 * N + 10 * D + K)
    ze = torch.randn(B, N * D, generator=gen, dtype=torch.float64)
    E = torch.randn(K, D, generator=gen, dtype=torch.float64)
    dz = torch.randn(B, N * D, generator=gen, dtype=torch.float64)
    for beta in (0.0, 0.25, 2.0):
        r = R.rows_reference(ze, E, N, beta, dzdec=dz)
        gz, gE = R.stopgrad_gradients(ze, E, N, beta, dz)
        scale = lambda a: max(1.0, np.abs(a).max())
        assert np.abs(r["dml"] - gz).max() <= 1e-12 * scale(gz)
        assert np.abs(r["dE"] - gE).max() <= 1e-12 * scale(gE)
        assert r["n_k"].sum() == B * N and r["codes"].min() >= 0 and r["codes"].max() < K
        assert np.allclose(r["lp"], -(1 + beta) * r["qerr"], rtol=1e-15, atol=0)
        assert (r["gap"] >= 0).all()
        # the arg min is the arg min: no other code is closer
        d = R.distances(ze, E, N).numpy()
        assert np.allclose(np.take_along_axis(d, r["codes"][..., None], -1)[..., 0].sum(1), r["qerr"], rtol=1e-12)
        assert (d.min(-1) == np.take_along_axis(d, r["codes"][..., None], -1)[..., 0]).all()
    # on given codes the closed forms follow those codes
    other = (r["codes"] + 1) % K
    r2 = R.rows_reference(ze, E, N, 0.25, dzdec=dz, codes=other)
    gz, gE = R.stopgrad_gradients(ze, E, N, 0.25, dz, codes=other)
    assert (r2["codes"] == other).all() and np.abs(r2["dml"] - gz).max() <= 1e-12 * max(1.0, np.abs(gz).max())
    assert np.abs(r2["dE"] - gE).max() <= 1e-12 * max(1.0, np.abs(gE).max())
    # a tie takes the lowest index
    E2 = E.clone()
    E2[K - 1] = E2[0]
    c = R.rows_reference(ze, E2, N, 0.25)["codes"]
    assert (c != K - 1).all()


def test_model_reference_gradients_match_the_closed_forms():
    """autograd through the whole model gives, at the encoder's output, dzdec + 2 beta (z_e - E_c), and at the codebook
    the codebook term alone."""
    I, H, N, D, K, B, beta = 20, 12, 3, 4, 6, 9, 0.25
    torch.manual_seed(3)
    m = vq_vae.VQVAE(I, H, N, D, K)
    with torch.no_grad():
        m.codebook.weight.mul_(K)
    P = {n: v.detach().double().numpy() for n, v in m.state_dict().items()}
    x = torch.bernoulli(torch.full((B, I), 0.4)).double().numpy()
    r = R.model_reference(P, x, N, beta)
    Pt = {n: R.as_t(P[n]) for n in R.KEYS}
    ze = R._encode(Pt, R.as_t(x))
    rows = R.rows_reference(ze, Pt["codebook.weight"], N, beta)
    assert (rows["codes"] == r["codes"]).all() and len(np.unique(r["codes"])) > 1
    assert np.abs(r["grads"]["codebook.weight"] - rows["dE"]).max() <= 1e-12 * max(1.0, np.abs(rows["dE"]).max())
    assert abs(r["vq"] - rows["qerr"].sum()) <= 1e-12 * max(1.0, r["vq"])
    recon = ((R.as_t(x) - R._decode(Pt, R.as_t(rows["zq"]))) ** 2).sum().item()
    assert abs(r["loss"] - (recon + (1 + beta) * rows["qerr"].sum())) <= 1e-12 * r["loss"]


def test_new_symbols_are_declared_and_bound():
    assert (_lib.VQ_MIN_D, _lib.VQ_MAX_D, _lib.VQ_MAX_ND) == (4, 64, 1024)
    assert (_lib.VQ_MIN_K, _lib.VQ_MAX_K, _lib.VQ_MAX_KD) == (2, 1024, 16384)
    from generative_models_amd import _build
    assert "gm_vq.hip" in _build.SOURCES
    # the default sizes and every GPU test shape lie inside the limits
    for N, D, K in ((16, 16, 128), (1, 4, 2), (3, 4, 5), (7, 8, 33), (8, 64, 256), (49, 4, 16), (16, 16, 1024), (6, 4, 8),
                    (8, 4, 16)):
        assert ops_fused.vq_fused_sizes(N, D, K), (N, D, K)
    for N, D, K in ((3, 2, 8), (3, 6, 8), (3, 68, 8), (257, 4, 8), (3, 4, 1), (3, 4, 1025), (3, 32, 1024), (0, 4, 8)):
        assert not ops_fused.vq_fused_sizes(N, D, K), (N, D, K)


def test_kernels_reject_null_out_of_range_and_aliased_arguments():
    """Host arrays stand in for device ones: every call below must return before it launches anything."""
    lib = _lib.load()
    a = [np.zeros(4096, dtype=np.float32) for _ in range(12)]
    p = lambda i: a[i].ctypes.data
    B, N, D, K = 4, 3, 4, 5
    W = N * D
    names = [n for n, _ in ops_fused.VqArgs._fields_]

    def args(**kw):
        v = dict(ze=p(0), ldz=W, E=p(1), lde=D, codes=p(2), ldc=N, beta=0.25, B=B, N=N, D=D, K=K, zq=p(3), ldq=W,
                 qerr=p(4), lp=p(5), dzdec=p(6), lddz=W, wn=p(7), dml=p(8), lddml=W)
        v.update(kw)
        return ops_fused.VqArgs(*[v[n] for n in names])
    shape = [dict(B=0), dict(N=0), dict(D=0), dict(D=2), dict(D=6), dict(D=68), dict(N=257, ldz=1028, ldq=1028), dict(K=1),
             dict(K=1025), dict(K=1024, D=32, ldz=96, ldq=96, lddz=96, lddml=96, lde=32), dict(ze=None), dict(E=None),
             dict(codes=None), dict(ldz=W - 1), dict(lde=D - 1), dict(ldc=N - 1), dict(beta=-1.0),
             dict(beta=float("nan")), dict(beta=float("inf"))]
    quant = shape + [dict(zq=None), dict(qerr=None), dict(lp=None), dict(ldq=W - 1), dict(zq=p(0)), dict(zq=p(1)),
                     dict(qerr=p(0)), dict(lp=p(4)), dict(lp=p(3)), dict(codes=p(3)), dict(codes=p(0))]
    assert lib.gm_vq_quantise(None, None) == _lib.GM_EINVAL
    for kw in quant:
        assert lib.gm_vq_quantise(None, ctypes.byref(args(**kw))) == _lib.GM_EINVAL, kw
        assert b"bad argument" in lib.gm_last_error()
    red = shape + [dict(dzdec=None), dict(wn=None), dict(dml=None), dict(lddz=W - 1), dict(lddml=W - 1), dict(dml=p(0)),
                   dict(dml=p(1)), dict(dml=p(2)), dict(dml=p(7))]
    assert lib.gm_vq_reduce(None, None) == _lib.GM_EINVAL
    for kw in red:
        assert lib.gm_vq_reduce(None, ctypes.byref(args(**kw))) == _lib.GM_EINVAL, kw
        assert b"bad argument" in lib.gm_last_error()
    snames = [n for n, _ in ops_fused.VqStepArgs._fields_]

    def sargs(**kw):
        v = dict(ze=p(0), ldz=W, codes=p(2), ldc=N, E=p(1), m=p(3), v=p(4), grad=p(5), nk=p(6), usage=p(7), sched=p(8),
                 sched_slot=_lib.NO_SLOT, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, B=B, N=N, D=D, K=K)
        v.update(kw)
        return ops_fused.VqStepArgs(*[v[n] for n in snames])
    step = [dict(B=0), dict(N=0), dict(D=2), dict(D=68), dict(K=1), dict(K=1025), dict(K=1024, D=32, ldz=96),
            dict(ze=None), dict(codes=None), dict(E=None), dict(m=None), dict(v=None), dict(ldz=W - 1), dict(ldc=N - 1),
            dict(grad=p(1)), dict(m=p(1)), dict(v=p(3)), dict(nk=p(7)), dict(grad=p(0)),
            dict(sched=None, grad=None, nk=None, usage=None)]
    assert lib.gm_vq_step(None, None) == _lib.GM_EINVAL
    for kw in step:
        assert lib.gm_vq_step(None, ctypes.byref(sargs(**kw))) == _lib.GM_EINVAL, kw
        assert b"bad argument" in lib.gm_last_error()
    for t in a:
        assert not t.any()                                               # nothing was written
    with pytest.raises(_lib.GMError):
        _lib.call("gm_vq_quantise", None, None)


class _Mine(vq_vae.VQVAETrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_path_selection():
    assert _trainer(vq_vae.VQVAE(16, 12, 3, 4, 8))._stock()
    assert _trainer(vq_vae.VQVAE(16, 12, 16, 64, 256))._stock() and _trainer(vq_vae.VQVAE(16, 12, 256, 4, 2))._stock()
    assert _trainer(vq_vae.VQVAE(16, 12, 16, 16, 1024))._stock()
    assert not _trainer(vq_vae.VQVAE(16, 12, 3, 2, 8))._stock()                    # D below the limit
    assert not _trainer(vq_vae.VQVAE(16, 12, 3, 6, 8))._stock()                    # D no multiple of 4
    assert not _trainer(vq_vae.VQVAE(16, 12, 3, 32, 1024))._stock()                # K D above the limit
    assert not _trainer(vq_vae.VQVAE(16, 12, 257, 4, 8))._stock()                  # N D above the limit
    assert not _trainer(vq_vae.VQVAE(16, 12, 3, 4, 8), cls=_Mine)._stock()         # an overridden hook
    m = vq_vae.VQVAE(16, 12, 3, 4, 8)
    m.encoder.extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock()                                                # an edited encoder
    m = vq_vae.VQVAE(16, 12, 3, 4, 8)
    m.codebook = torch.nn.Embedding(9, 4)
    assert not _trainer(m)._stock()                                                # a codebook of another size
    m = vq_vae.VQVAE(16, 12, 3, 4, 8)
    m.encoder = vae.Encoder(16, 12, 12)
    assert not _trainer(m)._stock()                                                # another encoder

    class Sub(vq_vae.VQVAE):
        pass
    assert not _trainer(Sub(16, 12, 3, 4, 8))._stock()                             # a subclassed model


def test_data_parallel_is_refused_and_the_checkpoint_config():
    from generative_models_amd.engine import VQVAEEngine
    m = vq_vae.VQVAE(16, 12, 3, 4, 8)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            VQVAEEngine(m, "cpu", trainer=_trainer(m), **kw)
    tr = _trainer(m)
    tr.force_dp = True
    with pytest.raises(_lib.GMError, match="one GPU"):
        tr.train(1)
    with pytest.raises(_lib.GMError, match="general path"):
        VQVAEEngine(vq_vae.VQVAE(16, 12, 3, 32, 1024), "cpu", trainer=_trainer(m))   # outside the limits: no launch
    eng = object.__new__(VQVAEEngine)
    eng.N, eng.D, eng.K, eng.trainer = 3, 4, 8, _trainer(m, beta=0.5)
    assert eng._settings() == {"num_vars": 3, "code_dim": 4, "num_codes": 8, "beta": 0.5}
    assert "prior_state" in vq_vae.VQVAETrainer._history and eng._noise(0, True) is None


def test_bad_codes_are_refused():
    tr = _trainer(vq_vae.VQVAE(16, 12, 3, 4, 8))
    ok = torch.zeros(4, 3, dtype=torch.int64)
    for bad in (ok[:, :2], ok.float(), ok - 1, ok + 8, ok == 0, ok[0]):
        with pytest.raises(ValueError):
            tr.decode(bad)


def test_iwae_log_likelihood_refuses_the_model():
    tr = _trainer(vq_vae.VQVAE(16, 12, 3, 4, 8))
    with pytest.raises(_lib.GMError, match="Encoder"):
        giwae.log_likelihood(tr, torch.zeros(2, 16), 3, 0)
    assert "vq_quantise" in inspect.getsource(vq_vae.VQVAETrainer._quantise)
