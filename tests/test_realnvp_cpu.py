"""The RealNVP coupling flow without a GPU: module surface and state_dict keys, the constructor's refusals at every limit,
the split rule, the fp64 reference's own invertibility and its log-determinant against the Jacobian's slogdet, the
identity flow of a fresh model, known answers of the noise rules, the C-ABI of the new kernels and its refusals,
fused / general path selection, the data-parallel refusal, the checkpoint config's strict check, and the
reference's own training on the learning test's data."""
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

import real_nvp  # noqa: E402
import realnvp_reference as R  # noqa: E402
from generative_models_amd import _lib, metrics, ops_fused  # noqa: E402
from generative_models_amd import realnvp as gnvp  # noqa: E402
from generative_models_amd.dvae import philox4x32_10  # noqa: E402

NEW = ("gm_nvp_pre", "gm_nvp_couple", "gm_nvp_loss", "gm_nvp_couple_bwd", "gm_nvp_post")


def _loaders(n=40, batch=8, side=4):
    x = torch.rand(n, 1, side, side)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None):
    tr = object.__new__(cls or real_nvp.RealNVPTrainer)  # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.seed, tr.noise_steps, tr._engine = 0, 0, None
    return tr


def test_module_surface_and_state_dict_keys():
    m = real_nvp.RealNVP(7, 5, 3)
    assert list(m.state_dict()) == R.keys(3)
    shapes = [tuple(v.shape) for v in m.state_dict().values()]
    assert shapes == [(5, 4), (5,), (6, 5), (6,), (5, 3), (5,), (8, 5), (8,), (5, 4), (5,), (6, 5), (6,)]
    assert (m.image_size, m.hidden_dim, m.num_couplings, m.mask, m.alpha, m.levels, m.s_cap, m.Da, m.Db) == \
        (7, 5, 3, "checker", 0.05, 256, 2.0, 4, 3)
    assert type(m.couplings) is torch.nn.ModuleList and all(type(c) is real_nvp.Coupling for c in m.couplings)
    sig = inspect.signature(real_nvp.RealNVP.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [
        ("image_size", 784), ("hidden_dim", 400), ("num_couplings", 4), ("mask", "checker"), ("alpha", 0.05),
        ("levels", 256), ("s_cap", 2.0)]
    T = real_nvp.RealNVPTrainer
    sig = inspect.signature(T.train).parameters
    assert [(n, p.default) for n, p in list(sig.items())[2:4]] == [("lr", 1e-3), ("weight_decay", 0.0)]
    assert T._hook_names == ("compute_batch", "evaluate")
    sig = inspect.signature(T.log_likelihood).parameters
    assert (sig["images"].default, sig["seed"].default) == (None, 1)
    sig = inspect.signature(T.sample).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("n", inspect.Parameter.empty), ("seed", 0),
                                                                  ("temperature", 1.0)]
    assert inspect.signature(T.encode).parameters["seed"].default == 0
    assert list(inspect.signature(T.interpolate).parameters)[1:4] == ["a", "b", "steps"]
    for name in ("sample", "encode", "decode", "interpolate", "parzen", "log_likelihood", "bits_per_dim", "sample_images",
                 "generate_images", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(T, name)), name
    assert issubclass(gnvp.RealNVPError, _lib.GMError) and issubclass(gnvp.RealNVPError, ValueError)
    import generative_models_amd as pkg
    from generative_models_amd import viz
    from generative_models_amd.engine import VAEEngine
    assert pkg.RealNVP is gnvp.RealNVP and pkg.RealNVPTrainer is T and pkg.RealNVPEngine is gnvp.RealNVPEngine
    assert issubclass(gnvp.RealNVPEngine, VAEEngine) and gnvp.RealNVPEngine.has_eps is False
    for f in ("_buffers", "_issue", "configure"):    # _alloc, the guard around _buffers, is the shared base's
        assert f in gnvp.RealNVPEngine.__dict__, f
    assert callable(viz.realnvp_sample_images)
    assert gnvp.__doc__ and "The contract" in gnvp.__doc__ and "NVPD" in gnvp.__doc__
    assert metrics.NLLResult._fields == ("ll_mean", "ll_stderr", "n")
    tr = _trainer(m)
    assert abs(tr.bits_per_dim(metrics.NLLResult(-7 * math.log(2.0) * 3.5, 0.0, 1)) - 3.5) < 1e-12
    tags = {gnvp.TAG_TRAIN, gnvp.TAG_EVAL, gnvp.TAG_S, _lib.MADE_TAG_S, _lib.CAT_TAG_TRAIN, _lib.CAT_TAG_EVAL,
            _lib.DDPM_TAG_T, _lib.DDPM_TAG_E, _lib.DDPM_TAG_V, _lib.DDPM_TAG_VE, _lib.DDPM_TAG_S}
    assert len(tags) == 11                                                # tags of its own
    assert (gnvp.TAG_TRAIN, gnvp.TAG_EVAL, gnvp.TAG_S) == tuple(int.from_bytes(t, "big") for t in (b"NVPD", b"NVPV", b"NVPS"))
    assert (R.TAG_TRAIN, R.TAG_EVAL, R.TAG_S) == (gnvp.TAG_TRAIN, gnvp.TAG_EVAL, gnvp.TAG_S)


@pytest.mark.parametrize("kw", [
    dict(image_size=1), dict(image_size=8193), dict(image_size=16.0), dict(image_size=True),
    dict(hidden_dim=0), dict(hidden_dim=1025), dict(hidden_dim=None),
    dict(num_couplings=0), dict(num_couplings=17), dict(num_couplings=2.0),
    dict(mask="stripes"), dict(mask=0), dict(alpha=-1e-3), dict(alpha=0.5), dict(alpha=float("nan")), dict(alpha="x"),
    dict(levels=1), dict(levels=65537), dict(levels=256.0), dict(s_cap=0.0), dict(s_cap=8.5), dict(s_cap=-1.0),
    dict(s_cap=float("inf"))])
def test_constructor_refusals(kw):
    args = dict(image_size=16, hidden_dim=8, num_couplings=2)
    args.update(kw)
    with pytest.raises(gnvp.RealNVPError):
        real_nvp.RealNVP(**args)
    with pytest.raises(ValueError):
        real_nvp.RealNVP(**args)


def test_constructor_accepts_every_limit():
    for kw in (dict(image_size=2, hidden_dim=1, num_couplings=1), dict(image_size=16, hidden_dim=4, num_couplings=16),
               dict(image_size=16, hidden_dim=4, alpha=0.0, levels=2, s_cap=8), dict(image_size=16, hidden_dim=4,
                                                                                    alpha=0.4999, levels=65536)):
        real_nvp.RealNVP(**kw)
    m = real_nvp.RealNVP(8192, 1, 1)
    assert tuple(m.couplings[0].out.weight.shape) == (8192, 1)


@pytest.mark.parametrize("mask", ["checker", "half"])
@pytest.mark.parametrize("D", [7, 10, 784])
def test_split_rule(D, mask):
    a, b = gnvp.split_indices(D, mask)
    Da, Db = (D + 1) // 2, D // 2
    assert a.size == Da and b.size == Db
    assert np.array_equal(np.sort(np.concatenate([a, b])), np.arange(D))            # a partition of 0 .. D - 1
    if mask == "checker":
        assert np.all(a % 2 == 0) and np.all(b % 2 == 1)
    else:
        assert np.array_equal(a, np.arange(Da)) and np.array_equal(b, np.arange(Da, D))
    ra, rb = R.split_idx(D, mask)
    assert np.array_equal(a, ra) and np.array_equal(b, rb)
    m = real_nvp.RealNVP(D, 3, 2, mask)
    y = torch.arange(2 * D, dtype=torch.float32).view(2, D)
    ya, yb = m.split(y)
    assert torch.equal(ya, y[:, a]) and torch.equal(yb, y[:, b]) and torch.equal(m.merge(ya, yb), y)
    assert torch.equal(R.merge(*R.split(y.double(), mask), mask), y.double())
    assert (m.Da, m.Db) == (Da, Db)
    dims = [(tuple(c.linear.weight.shape)[1], tuple(c.out.weight.shape)[0]) for c in m.couplings]
    assert dims == [(Da, 2 * Db), (Db, 2 * Da)]                                     # even k transforms B, odd k A


CFG = dict(K=3, s_cap=2.0, mask="checker", alpha=0.05, levels=256)


@pytest.mark.parametrize("mask", ["checker", "half"])
@pytest.mark.parametrize("D,H,K", [(6, 5, 3), (7, 4, 4), (16, 8, 1)])
def test_reference_inverse_of_forward(D, H, K, mask):
    P = R.f64(R.random_weights(D, H, K, seed=D, out_scale=2.0))
    y = torch.randn(9, D, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 3
    z, _ = R.forward(P, y, K, 2.0, mask)
    assert (z - y).abs().max() > 0.1
    assert (R.inverse(P, z, K, 2.0, mask) - y).abs().max().item() <= 1e-12
    assert (R.forward(P, R.inverse(P, y, K, 2.0, mask), K, 2.0, mask)[0] - y).abs().max().item() <= 1e-12


@pytest.mark.parametrize("mask", ["checker", "half"])
def test_reference_logdet_is_the_jacobians(mask):
    """D = 6, H = 5, K = 3, random non-zero weights: the log-determinant the reference accumulates (preprocessing +
    couplings) equals slogdet of the autograd Jacobian of the whole map, dequantised pixel -> z, to 1e-10."""
    D, H, K = 6, 5, 3
    cfg = dict(CFG, mask=mask)
    P = R.f64(R.random_weights(D, H, K, seed=2, out_scale=2.0))
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        v = torch.rand(D, dtype=torch.float64, generator=g) * 0.98 + 0.01          # the dequantised pixel (q + u) / levels

        def whole(v):
            w = cfg["alpha"] + (1.0 - 2.0 * cfg["alpha"]) * v
            y = torch.log(w) - torch.log1p(-w)
            return R.forward(P, y[None], K, cfg["s_cap"], mask)[0][0]
        J = torch.autograd.functional.jacobian(whole, v)
        sign, logabs = torch.linalg.slogdet(J)
        # the same through pre(): x on the grid and u chosen so that (q + u) / levels = v
        q = torch.floor(v * cfg["levels"])
        u = v * cfg["levels"] - q
        y, ld0 = R.pre((q / (cfg["levels"] - 1))[None], u[None], cfg["alpha"], cfg["levels"])
        _, ld = R.forward(P, y, K, cfg["s_cap"], mask)
        assert sign.item() > 0
        assert abs((ld0 + ld).item() - logabs.item()) <= 1e-10, ((ld0 + ld).item(), logabs.item())


def test_fresh_model_is_the_identity_flow():
    m = real_nvp.RealNVP(10, 6, 4)
    for c in m.couplings:
        assert not c.out.weight.any() and not c.out.bias.any() and c.linear.weight.abs().max() > 0
    P = R.f64(m.state_dict())
    y = torch.randn(5, 10, dtype=torch.float64)
    z, ld = R.forward(P, y, 4, m.s_cap, m.mask)
    assert torch.equal(z, y) and not ld.any()
    assert torch.equal(R.inverse(P, y, 4, m.s_cap, m.mask), y)


def test_noise_rules_known_answers():
    """u and z by hand from dvae.philox4x32_10: counter (e >> 2, step, row, TAG), key (seed mod 2^32, seed >> 32), word
    e & 3; ph_unit; the Box-Muller pairing (0, 1), (2, 3)."""
    seed, step, row0, n, D = (7 << 32) | 5, 11, 3, 4, 10
    key = np.array([5, 7], dtype=np.uint64)
    u = gnvp.uniforms_reference(n, D, seed, step, gnvp.TAG_EVAL, row0)
    z = gnvp.normals_reference(n, D, seed, row0)
    assert u.dtype == np.float32 and u.shape == (n, D) and z.shape == (n, D)
    for r in range(n):
        for e in (0, 1, 5, 9):
            w = philox4x32_10(np.array([e >> 2, step, row0 + r, gnvp.TAG_EVAL], dtype=np.uint64), key)
            want = np.float32((2 * (int(w[e & 3]) >> 9) + 1) * 2.0 ** -24)
            assert u[r, e] == want and 0.0 < want < 1.0
            w = philox4x32_10(np.array([e >> 2, 0, row0 + r, gnvp.TAG_S], dtype=np.uint64), key)
            pair = (e & 3) // 2 * 2
            ua, ub = ((2 * (int(w[pair + j]) >> 9) + 1) * 2.0 ** -24 for j in (0, 1))
            rad, phi = math.sqrt(-2.0 * math.log(ua)), 2.0 * math.pi * ub
            assert abs(z[r, e] - (rad * math.cos(phi) if e % 2 == 0 else rad * math.sin(phi))) <= 1e-12
    # indexed by row and element: a prefix of a wider or longer draw
    assert np.array_equal(gnvp.uniforms_reference(2, 7, seed, step, gnvp.TAG_EVAL, row0), u[:2, :7])
    assert np.array_equal(gnvp.normals_reference(2, 7, seed, row0), z[:2, :7])
    assert not np.array_equal(gnvp.uniforms_reference(n, D, seed, step, gnvp.TAG_TRAIN, row0), u)
    assert u.min() >= 2.0 ** -24 and u.max() <= 1.0 - 2.0 ** -24
    # the fp32 preprocessing stays finite at alpha = 0 on the extreme words, where v rounds to 1
    ext = torch.tensor([[2.0 ** -24, 1.0 - 2.0 ** -24]], dtype=torch.float32)
    for x in (0.0, 1.0):
        y, ld = gnvp.preprocess(torch.full((1, 2), x), ext, 0.0, 256)
        ry, rld = R.pre(torch.full((1, 2), x), ext, 0.0, 256)
        assert torch.isfinite(y).all() and torch.isfinite(ld).all()
        assert ((y.double() - ry).abs() / ry.abs().clamp(min=1.0)).max() <= 1e-6 and abs(ld.item() - rld.item()) <= 1e-4


def test_torch_restatement_agrees_with_the_reference():
    """realnvp.preprocess / RealNVP.split / postprocess in fp64 against tests/realnvp_reference.py."""
    g = torch.Generator().manual_seed(0)
    x = torch.floor(torch.rand(6, 10, generator=g, dtype=torch.float64) * 256) / 255
    u = torch.from_numpy(gnvp.uniforms_reference(6, 10, 3, 0).astype(np.float64))
    y, ld = gnvp.preprocess(x, u, 0.05, 256)
    ry, rld = R.pre(x, u, 0.05, 256)
    assert (y - ry).abs().max() <= 1e-12 and (ld - rld).abs().max() <= 1e-11
    assert (gnvp.postprocess(y, 0.05) - R.post(ry, 0.05)).abs().max() <= 1e-15
    assert torch.equal(torch.floor(R.post(ry, 0.05) * 256), R.quantise(x, 256))         # the round trip requantises
    assert abs(gnvp.nll_constant(10, 256) - R.nll_const(10, 256)) < 1e-12


def test_new_symbols_are_declared_and_bound():
    assert (_lib.NVP_MIN_D, _lib.NVP_MAX_D, _lib.NVP_MAX_H, _lib.NVP_MAX_K, _lib.NVP_MAX_LEVELS, _lib.NVP_MAX_S_CAP) == \
        (2, 8192, 1024, 16, 65536, 8)
    from generative_models_amd import _build
    assert "gm_nvp.hip" in _build.SOURCES
    assert os.path.isfile(os.path.join(_build.CSRC, "gm_nvp.h"))


def _mk(ct, base, **kw):
    v = dict(base)
    v.update(kw)
    return ct(*[v[n] for n, _ in ct._fields_])


def test_kernels_reject_null_and_out_of_limit_arguments():
    """Host arrays stand in for device ones: every call below must return before it launches anything."""
    lib = _lib.load()
    a = [np.zeros(1 << 15, dtype=np.float32) for _ in range(8)]
    p = lambda i: a[i].ctypes.data
    B, D, Da, Db = 4, 10, 5, 5
    for name in NEW:
        assert getattr(lib, name)(None, None) == _lib.GM_EINVAL, name
        assert b"bad argument" in lib.gm_last_error()

    def refused(name, ct, base, cases):
        for kw in cases:
            assert getattr(lib, name)(None, ctypes.byref(_mk(ct, base, **kw))) == _lib.GM_EINVAL, (name, kw)
            assert b"bad argument" in lib.gm_last_error()

    pre = dict(x=p(0), ldx=D, ya=p(1), lda=Da, yb=p(2), ldb=Db, logdet=p(3), u=None, ldu=0, seed=0, step_ctr=None,
               step_base=None, step_add=0, row0=0, tag=gnvp.TAG_TRAIN, alpha=0.05, levels=256, mask=0, mode=_lib.NVP_PRE,
               B=B, D=D)
    refused("gm_nvp_pre", ops_fused.NvpPreArgs, pre, [
        dict(B=0), dict(D=1), dict(D=8193), dict(mode=2), dict(mode=-1), dict(row0=-1), dict(row0=(1 << 32) - 3),
        dict(x=None), dict(ya=None), dict(yb=None), dict(logdet=None), dict(ldx=D - 1), dict(lda=Da - 1), dict(ldb=Db - 1),
        dict(mask=2), dict(mask=-1), dict(alpha=-0.01), dict(alpha=0.5), dict(alpha=float("nan")), dict(levels=1),
        dict(levels=65537), dict(ya=p(0)), dict(yb=p(0)), dict(yb=p(1)), dict(logdet=p(1)), dict(logdet=p(0)),
        dict(mode=_lib.NVP_NOISE), dict(mode=_lib.NVP_NOISE, u=p(4), ldu=D - 1)])
    cpl = dict(st=p(0), ldst=2 * Db, inp=p(1), ldin=Db, out=p(2), ldout=Db, logdet=p(3), s_cap=2.0, inverse=0, B=B, Dt=Db)
    refused("gm_nvp_couple", ops_fused.NvpCoupleArgs, cpl, [
        dict(B=0), dict(Dt=0), dict(Dt=4097), dict(s_cap=0.0), dict(s_cap=8.5), dict(s_cap=float("nan")), dict(st=None),
        dict(inp=None), dict(out=None), dict(logdet=None), dict(ldst=2 * Db - 1), dict(ldin=Db - 1), dict(ldout=Db - 1),
        dict(out=p(0)), dict(out=p(1)), dict(logdet=p(2)), dict(inverse=2), dict(inverse=-1)])
    loss = dict(za=p(0), ldza=Da, zb=p(1), ldzb=Db, logdet=p(2), part=p(3), dza=p(4), lddza=Da, dzb=p(5), lddzb=Db,
                cst=1.0, scale=0.25, B=B, Da=Da, Db=Db)
    refused("gm_nvp_loss", ops_fused.NvpLossArgs, loss, [
        dict(B=0), dict(Da=0), dict(Db=0), dict(Da=4097, Db=4096), dict(Da=5, Db=3), dict(Da=4, Db=5), dict(za=None),
        dict(zb=None), dict(logdet=None), dict(part=None), dict(ldza=Da - 1), dict(ldzb=Db - 1), dict(dza=None),
        dict(dzb=None), dict(lddza=Da - 1), dict(lddzb=Db - 1), dict(dza=p(5)), dict(dza=p(0)), dict(dzb=p(1)),
        dict(part=p(0)), dict(part=p(2)), dict(cst=float("nan")), dict(scale=float("inf")), dict(scale=-1.0)])
    bwd = dict(st=p(0), ldst=2 * Db, x=p(1), ldx=Db, g0=p(2), ldg0=Db, g1=p(3), ldg1=Db, dst=p(4), lddst=2 * Db, dx=p(5),
               lddx=Db, c=-0.25, s_cap=2.0, B=B, Dt=Db)
    refused("gm_nvp_couple_bwd", ops_fused.NvpCoupleBwdArgs, bwd, [
        dict(B=0), dict(Dt=0), dict(Dt=4097), dict(s_cap=0.0), dict(s_cap=9.0), dict(c=float("nan")), dict(st=None),
        dict(x=None), dict(g0=None), dict(dst=None), dict(ldst=2 * Db - 1), dict(ldx=Db - 1), dict(ldg0=Db - 1),
        dict(ldg1=Db - 1), dict(lddst=2 * Db - 1), dict(lddx=Db - 1), dict(dx=p(4)), dict(dst=p(0)), dict(dst=p(2)),
        dict(dx=p(1)), dict(dx=p(3))])
    post = dict(ya=p(0), lda=Da, yb=p(1), ldb=Db, x=p(2), ldx=D, seed=0, row0=0, alpha=0.05, temperature=1.0, mask=0,
                mode=_lib.NVP_POST, B=B, D=D)
    refused("gm_nvp_post", ops_fused.NvpPostArgs, post, [
        dict(B=0), dict(D=1), dict(D=8193), dict(mask=3), dict(mode=2), dict(ya=None), dict(yb=None), dict(yb=p(0)),
        dict(lda=Da - 1), dict(ldb=Db - 1), dict(x=None), dict(ldx=D - 1), dict(x=p(0)), dict(x=p(1)), dict(alpha=0.5),
        dict(alpha=-0.1), dict(mode=_lib.NVP_PRIOR, row0=-1), dict(mode=_lib.NVP_PRIOR, temperature=-1.0),
        dict(mode=_lib.NVP_PRIOR, temperature=float("nan")), dict(mode=_lib.NVP_PRIOR, row0=(1 << 32) - 3)])
    for t in a:
        assert not t.any()                                                # nothing was written
    with pytest.raises(_lib.GMError):
        _lib.call("gm_nvp_loss", None, None)


class _Mine(real_nvp.RealNVPTrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_path_selection():
    assert _trainer(real_nvp.RealNVP(16, 8, 3))._stock()
    assert _trainer(real_nvp.RealNVP(7, 1, 1, "half", 0.0, 2, 8))._stock()
    assert _trainer(real_nvp.RealNVP(16, 8, 16))._stock()
    assert not _trainer(real_nvp.RealNVP(16, 8, 3), cls=_Mine)._stock()            # an overridden hook
    m = real_nvp.RealNVP(16, 8, 3)
    m.couplings[1].extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock()                                                # an edited coupling
    m = real_nvp.RealNVP(16, 8, 3)
    m.couplings[2].out = torch.nn.Linear(8, 12)
    assert not _trainer(m)._stock()                                                # an out layer of another width
    m = real_nvp.RealNVP(16, 8, 3)
    m.couplings.append(real_nvp.Coupling(8, 8, 8))
    assert not _trainer(m)._stock()                                                # a coupling more than num_couplings
    m = real_nvp.RealNVP(16, 8, 3)
    m.norm = torch.nn.BatchNorm1d(16)
    assert not _trainer(m)._stock()                                                # another layer
    m = real_nvp.RealNVP(16, 8, 3)
    m.s_cap = 9.0
    assert not _trainer(m)._stock()                                                # a setting outside the kernels' limits

    class Sub(real_nvp.RealNVP):
        pass
    assert not _trainer(Sub(16, 8, 3))._stock()                                    # a subclassed model


def test_data_parallel_is_refused():
    m = real_nvp.RealNVP(16, 8, 3)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            gnvp.RealNVPEngine(m, "cpu", trainer=_trainer(m), **kw)
    tr = _trainer(m)
    tr.force_dp = True
    with pytest.raises(_lib.GMError, match="one GPU"):
        tr.train(1)
    m.couplings[0].extra = torch.nn.Linear(2, 2)
    with pytest.raises(_lib.GMError, match="general path"):
        gnvp.RealNVPEngine(m, "cpu", trainer=_trainer(m))


def test_checkpoint_config_is_checked_under_strict():
    """The settings a checkpoint carries -- mask, alpha, levels, s_cap, seed -- are compared by configure() before
    anything is allocated on a device or launched: a differing one is refused unless the load was lenient."""
    m = real_nvp.RealNVP(16, 8, 2, "half", 0.1, 64, 3.0)
    tr = _trainer(m)
    tr.seed = 9
    eng = gnvp.RealNVPEngine(m, "cpu", trainer=tr)
    now = eng._settings()
    assert now == {"mask": "half", "alpha": 0.1, "levels": 64, "s_cap": 3.0, "seed": 9}
    n = eng.fp.m.numel()
    for key, other in (("mask", "checker"), ("alpha", 0.05), ("levels", 256), ("s_cap", 2.0), ("seed", 0)):
        saved = dict(now, B=8, lr=1e-3, weight_decay=0.0)
        saved[key] = other
        resume = {"m": torch.zeros(n), "v": torch.zeros(n), "step": 5, "config": saved}
        with pytest.raises(_lib.GMError, match="different settings") as ei:
            eng.configure(8, 5, 1e-3, 0.0, resume=resume)
        assert key in str(ei.value)
    src = inspect.getsource(real_nvp.RealNVPTrainer.save_checkpoint)
    assert "noise_steps" in src and "losses" in src


def test_reference_training_clears_the_learning_tests_bound():
    """The GPU learning test's premise, checked on its reference: 150 Adam batches of 16 on the 4-pattern data take the
    fp64 reference's validation NLL below the identity flow's on the same validation stream."""
    D, H, K, b = 16, 8, 4, 16
    cfg = dict(K=K, s_cap=2.0, mask="checker", alpha=0.05, levels=256)
    x = R.pattern_data(64, D)
    torch.manual_seed(1234)
    m = real_nvp.RealNVP(D, H, K)
    noise = lambda tag, step, n: torch.from_numpy(gnvp.uniforms_reference(n, D, 5, step, tag).astype(np.float64))
    ident = np.mean([(R.nll_rows(R.f64(m.state_dict()), x[i:i + b].double(), noise(R.TAG_EVAL, i // b, b), cfg).mean()).item()
                     for i in range(0, 64, b)])
    P = {n: torch.nn.Parameter(v) for n, v in R.f64(m.state_dict()).items()}
    opt = torch.optim.Adam(list(P.values()), lr=1e-3)
    g = torch.Generator().manual_seed(0)
    for step in range(150):
        xb = x[torch.randperm(64, generator=g)[:b]].double()
        opt.zero_grad()
        (R.nll_rows(P, xb, noise(R.TAG_TRAIN, step, b), cfg).sum() / b).backward()
        opt.step()
    with torch.no_grad():
        val = np.mean([(R.nll_rows(P, x[i:i + b].double(), noise(R.TAG_EVAL, i // b, b), cfg).mean()).item()
                       for i in range(0, 64, b)])
    print("identity", ident, "trained", val)
    assert val < ident
