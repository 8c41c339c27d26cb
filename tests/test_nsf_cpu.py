"""The neural spline flow without a GPU: module surface and state_dict keys, the constructor's refusals and limits, the
reference's own invertibility, its log-determinant against autograd's Jacobian, the identity flow of a fresh model,
monotonicity and C1 continuity at the knots, the linear tails, the package's torch restatement against the reference, the
C-ABI of the two new kernels and its refusals, the kernels' resource rows, the wide conditioner GEMMs' launch plans, path
selection, the data-parallel refusal, the checkpoint config's strict check, the share of pixels the GPU test's gradient
comparisons leave out, and the reference's own training on the learning test's data."""
import ctypes
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))
sys.path.insert(0, HERE)

import linear_path_cases as lp  # noqa: E402
import nsf_reference as N  # noqa: E402
import spline_flow  # noqa: E402
from generative_models_amd import _abi, _build, _lib, nsf, ops, ops_fused  # noqa: E402
from generative_models_amd import realnvp as gnvp  # noqa: E402

NEW = ("gm_nsf_couple", "gm_nsf_couple_bwd")
BINS = (4, 8, 16)


def _loaders(n=40, batch=8, side=4):
    x = torch.rand(n, 1, side, side)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None):
    tr = object.__new__(cls or spline_flow.SplineFlowTrainer)  # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.seed, tr.noise_steps, tr._engine = 0, 0, None
    return tr


def cfg_of(K, bins, tail=3.0, mask="checker"):
    return dict(K=K, bins=bins, tail=tail, mask=mask, alpha=0.05, levels=256)


def test_module_surface_and_state_dict_keys():
    m = spline_flow.SplineFlow(7, 5, 3, 4)
    assert list(m.state_dict()) == N.keys(3)
    shapes = [tuple(v.shape) for v in m.state_dict().values()]
    assert shapes == [(5, 4), (5,), (33, 5), (33,), (5, 3), (5,), (44, 5), (44,), (5, 4), (5,), (33, 5), (33,)]
    assert (m.image_size, m.hidden_dim, m.num_couplings, m.num_bins, m.tail_bound, m.mask, m.alpha, m.levels, m.Da,
            m.Db) == (7, 5, 3, 4, 3.0, "checker", 0.05, 256, 4, 3)
    assert not hasattr(m, "s_cap")
    assert all(type(c) is spline_flow.SplineCoupling for c in m.couplings)
    sig = inspect.signature(spline_flow.SplineFlow.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [
        ("image_size", 784), ("hidden_dim", 400), ("num_couplings", 4), ("num_bins", 8), ("tail_bound", 3.0),
        ("mask", "checker"), ("alpha", 0.05), ("levels", 256)]
    T = spline_flow.SplineFlowTrainer
    assert issubclass(T, gnvp.DequantFlowTrainer) and T._hook_names == ("compute_batch", "evaluate")
    sig = inspect.signature(T.train).parameters
    assert [(n, p.default) for n, p in list(sig.items())[2:4]] == [("lr", 1e-3), ("weight_decay", 0.0)]
    for name in ("sample", "encode", "decode", "parzen", "log_likelihood", "bits_per_dim", "sample_images",
                 "generate_images", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(T, name)), name
    for name in ("sample", "encode", "decode", "log_likelihood", "_forward_rows", "_inverse_rows", "_prior"):
        assert getattr(T, name) is getattr(gnvp.RealNVPTrainer, name), name       # RealNVP's protocol, defined once
    assert issubclass(nsf.SplineFlowError, _lib.GMError) and issubclass(nsf.SplineFlowError, ValueError)
    assert T._error is nsf.SplineFlowError and spline_flow.SplineFlowError is nsf.SplineFlowError
    import generative_models_amd as pkg
    assert pkg.SplineFlow is nsf.SplineFlow and pkg.SplineFlowTrainer is T and pkg.SplineFlowEngine is nsf.SplineFlowEngine
    assert issubclass(nsf.SplineFlowEngine, gnvp.RealNVPEngine)
    for f in ("_issue", "_buffers", "configure", "_chain"):                       # RealNVP's batch, not a copy of it
        assert f not in nsf.SplineFlowEngine.__dict__, f
    assert nsf.__doc__ and "The contract" in nsf.__doc__ and "NVPD" in nsf.__doc__
    assert (T._tag_train, T._tag_eval) == (gnvp.TAG_TRAIN, gnvp.TAG_EVAL)
    assert nsf.MIN_BIN == N.MIN_BIN == 1e-3 and nsf.SLOPE_SHIFT == N.SLOPE_SHIFT
    hdr = open(os.path.join(_build.CSRC, "gm_nsf.h")).read()
    assert "#define NSF_MIN_BIN 1e-3f" in hdr
    assert np.float32(float(hdr.split("#define NSF_SLOPE_SHIFT ")[1].split("f")[0])) == np.float32(N.SLOPE_SHIFT)


@pytest.mark.parametrize("kw", [
    dict(image_size=1), dict(image_size=8193), dict(image_size=16.0), dict(image_size=True),
    dict(hidden_dim=0), dict(hidden_dim=1025), dict(hidden_dim=None),
    dict(num_couplings=0), dict(num_couplings=17), dict(num_couplings=2.0),
    dict(num_bins=0), dict(num_bins=2), dict(num_bins=6), dict(num_bins=32), dict(num_bins=8.0), dict(num_bins=True),
    dict(tail_bound=0.0), dict(tail_bound=-3.0), dict(tail_bound=64.5), dict(tail_bound=1e-60),
    dict(tail_bound=float("inf")), dict(tail_bound=float("nan")), dict(tail_bound="3"),
    dict(mask="stripes"), dict(mask=0), dict(alpha=-1e-3), dict(alpha=0.5), dict(alpha=float("nan")), dict(alpha="x"),
    dict(levels=1), dict(levels=65537), dict(levels=256.0), dict(s_cap=2.0)])
def test_constructor_refusals(kw):
    args = dict(image_size=16, hidden_dim=8, num_couplings=2)
    args.update(kw)
    with pytest.raises((nsf.SplineFlowError, TypeError) if "s_cap" in kw else nsf.SplineFlowError):
        spline_flow.SplineFlow(**args)
    if "s_cap" not in kw:
        with pytest.raises(ValueError):
            spline_flow.SplineFlow(**args)


def test_constructor_accepts_every_limit():
    for kw in (dict(image_size=2, hidden_dim=1, num_couplings=1), dict(image_size=16, hidden_dim=4, num_couplings=16),
               dict(image_size=16, hidden_dim=4, num_bins=4, tail_bound=64, alpha=0.0, levels=2),
               dict(image_size=16, hidden_dim=4, num_bins=16, tail_bound=1e-6, alpha=0.4999, levels=65536, mask="half")):
        spline_flow.SplineFlow(**kw)
    m = spline_flow.SplineFlow(8192, 1, 1, 16)
    assert tuple(m.couplings[0].out.weight.shape) == (47 * 4096, 1)


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("tail", [3.0, 0.75])
def test_reference_inverse_of_forward_and_its_jacobian(bins, tail):
    """fp64: inverse(forward(x)) = x per pixel, forward(inverse(y)) = y, and the log-derivative the reference reports is
    the log of autograd's dy/dx (the coupling's Jacobian is diagonal)."""
    st, x, _, _ = N.kernel_inputs(16, 64, bins, tail, seed=bins, scale=1.0)
    st, x = st.double(), x.double().requires_grad_(True)
    y, ld, inside, k, xi = N.couple(st, x, bins, tail, detail=True)
    assert inside.any() and (~inside).any() and len(set(k[inside].tolist())) == bins
    (dy,) = torch.autograd.grad(y.sum(), x)
    assert (dy > 0).all() and (torch.log(dy) - ld.detach()).abs().max().item() <= 1e-11
    # an error of y comes back as one of x divided by the slope: the round trip per pixel in units of 1 / (dy/dx)
    assert ((N.couple_inv(st, y.detach(), bins, tail) - x.detach()).abs() * dy).max().item() <= 1e-12
    xs = N.couple_inv(st, x.detach(), bins, tail)
    assert (N.couple(st, xs, bins, tail)[0] - x.detach()).abs().max().item() <= 1e-12
    assert torch.equal(N.couple(st, x.detach(), bins, tail)[1], ld.detach().sum(1))


@pytest.mark.parametrize("mask", ["checker", "half"])
def test_reference_model_logdet_is_the_jacobians(mask):
    D, H, K, bins = 6, 5, 3, 4
    cfg = cfg_of(K, bins, mask=mask)
    P = N.f64(N.random_weights(D, H, K, bins, seed=2, out_scale=1.0))
    g = torch.Generator().manual_seed(4)
    for _ in range(3):
        y = torch.randn(D, dtype=torch.float64, generator=g) * 1.5
        J = torch.autograd.functional.jacobian(lambda v: N.forward(P, v[None], cfg)[0][0], y)
        sign, logabs = torch.linalg.slogdet(J)
        z, ld = N.forward(P, y[None], cfg)
        assert sign.item() > 0 and abs(ld.item() - logabs.item()) <= 1e-10
        assert (N.inverse(P, z, cfg)[0] - y).abs().max().item() <= 1e-12


def test_fresh_model_is_the_identity_flow():
    m = spline_flow.SplineFlow(10, 6, 4, 8)
    for c in m.couplings:
        assert not c.out.weight.any() and not c.out.bias.any() and c.linear.weight.abs().max() > 0
    P, cfg = N.f64(m.state_dict()), cfg_of(4, 8)
    y = torch.randn(5, 10, dtype=torch.float64) * 2
    z, ld = N.forward(P, y, cfg)
    assert (z - y).abs().max().item() <= 1e-14 and ld.abs().max().item() <= 1e-13
    assert (N.inverse(P, y, cfg) - y).abs().max().item() <= 1e-14
    z32, ld32 = N.forward({n: v.float() for n, v in P.items()}, y.float(), cfg)    # "to rounding" in fp32
    assert (z32 - y.float()).abs().max().item() <= 2e-6 and ld32.abs().max().item() <= 1e-5


@pytest.mark.parametrize("bins", BINS)
def test_monotone_and_c1_at_the_knots(bins):
    """Across every interior knot the value and the slope agree from both sides, the slope there is the knot's d_i, the
    ends meet the tails with slope 1, and the map ascends on a fine grid."""
    tail = 3.0
    st = N.kernel_inputs(1, 1, bins, tail, seed=7, scale=1.0)[0].double()
    w, h, d, xs, ys = N.spline_params(st, 1, bins, tail)
    f = lambda v: N.couple(st, torch.tensor([[v]], dtype=torch.float64), bins, tail, detail=True)
    for i in range(bins + 1):
        kx = xs[0, 0, i].item()
        lo, hi = f(np.nextafter(kx, -np.inf)), f(kx if i < bins else np.nextafter(kx, np.inf))
        assert abs(lo[0].item() - ys[0, 0, i].item()) <= 1e-14 and abs(hi[0].item() - ys[0, 0, i].item()) <= 1e-14
        for side in (lo, hi):
            inside = side[2].item()
            assert abs(side[1].item() - (np.log(d[0, 0, i].item()) if inside else 0.0)) <= 1e-12
    assert d[0, 0, 0] == 1 and d[0, 0, bins] == 1 and xs[0, 0, 0] == -tail and xs[0, 0, bins] == tail
    grid = torch.linspace(-tail - 1, tail + 1, 20001, dtype=torch.float64)[:, None]
    y = N.couple(st.expand(20001, -1), grid, bins, tail)[0][:, 0]
    assert (y[1:] > y[:-1]).all()


def test_tails_are_the_identity_with_zero_gradients():
    bins, tail = 8, 0.75
    st, x, g, _ = N.kernel_inputs(4, 50, bins, tail, seed=3)
    x[0, :4] = torch.tensor([-tail, tail, -tail - 1e-3, 30.0])
    y, ld, inside, _, _ = N.couple(st.double(), x.double(), bins, tail, detail=True)
    assert not inside[0, :4].any() and 0.3 < inside.double().mean() < 0.7
    assert torch.equal(y[~inside], x.double()[~inside]) and not ld[~inside].any()
    dst, dx = N.couple_bwd(st.double(), x.double(), g.double(), -0.25, bins, tail)
    out = (~inside)[:, None, :].expand(4, N.n_params(bins), 50)
    assert not dst.view(4, -1, 50)[out].any() and torch.equal(dx[~inside], g.double()[~inside])
    assert dst.view(4, -1, 50)[~out].abs().min() >= 0 and dst.abs().max() > 0


@pytest.mark.parametrize("bins", BINS)
def test_package_restatement_agrees_with_the_reference(bins):
    """nsf.spline / spline_inverse (the general path's torch ops) in fp64 against tests/nsf_reference.py, gradients too."""
    st, x, g, _ = N.kernel_inputs(5, 33, bins, 3.0, seed=bins)
    st, x, g = st.double(), x.double(), g.double()
    ry, rld = N.couple(st, x, bins, 3.0)
    a, b = st.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y, ld = nsf.spline(a, b, bins, 3.0)
    assert (y - ry).abs().max().item() <= 1e-13 and (ld - rld).abs().max().item() <= 1e-12
    ((g * y).sum() - 0.2 * ld.sum()).backward()
    rdst, rdx = N.couple_bwd(st, x, g, -0.2, bins, 3.0)
    assert (a.grad - rdst).abs().max().item() <= 1e-12 and (b.grad - rdx).abs().max().item() <= 1e-12
    assert (nsf.spline_inverse(st, ry, bins, 3.0) - x).abs().max().item() <= 1e-12


def test_new_symbols_are_declared_bound_and_built():
    assert (_lib.NSF_MIN_BINS, _lib.NSF_MAX_BINS, _lib.NSF_MAX_TAIL) == (4, 16, 64)
    assert nsf.BINS == BINS
    for name in NEW:
        assert name in _abi._SIGNATURES
    assert _abi.STRUCTS["gm_nsf_couple_args"] is ops_fused.NsfCoupleArgs
    assert _abi.STRUCTS["gm_nsf_couple_bwd_args"] is ops_fused.NsfCoupleBwdArgs
    i = _build.SOURCES.index("gm_nsf.hip")
    assert 0 < i < len(_build.SOURCES) - 1
    assert os.path.isfile(os.path.join(_build.CSRC, "gm_nsf.h")) and os.path.isfile(os.path.join(_build.CSRC, "gm_nsf.hip"))
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name).argtypes[1] is ctypes.POINTER(_abi.STRUCTS[name + "_args"])
    assert callable(ops_fused.nsf_couple) and callable(ops_fused.nsf_couple_bwd)


def _mk(ct, base, **kw):
    v = dict(base)
    v.update(kw)
    return ct(*[v[n] for n, _ in ct._fields_])


def test_kernels_reject_null_and_out_of_limit_arguments():
    """Host arrays stand in for device ones: every call below must return before it launches anything."""
    lib = _lib.load()
    a = [np.zeros(1 << 15, dtype=np.float32) for _ in range(6)]
    p = lambda i: a[i].ctypes.data
    B, Dt, bins = 4, 5, 8
    W = 23 * Dt
    for name in NEW:
        assert getattr(lib, name)(None, None) == _lib.GM_EINVAL, name
        assert b"bad argument" in lib.gm_last_error()

    def refused(name, ct, base, cases):
        for kw in cases:
            assert getattr(lib, name)(None, ctypes.byref(_mk(ct, base, **kw))) == _lib.GM_EINVAL, (name, kw)
            assert b"bad argument" in lib.gm_last_error()

    cpl = dict(st=p(0), ldst=W, inp=p(1), ldin=Dt, out=p(2), ldout=Dt, logdet=p(3), tail_bound=3.0, inverse=0, B=B, Dt=Dt,
               bins=bins)
    refused("gm_nsf_couple", ops_fused.NsfCoupleArgs, cpl, [
        dict(B=0), dict(Dt=0), dict(Dt=4097), dict(bins=0), dict(bins=2), dict(bins=6), dict(bins=12), dict(bins=32),
        dict(bins=-8), dict(tail_bound=0.0), dict(tail_bound=-1.0), dict(tail_bound=64.5), dict(tail_bound=float("nan")),
        dict(tail_bound=float("inf")), dict(st=None), dict(inp=None), dict(out=None), dict(logdet=None), dict(ldst=W - 1),
        dict(bins=16, ldst=47 * Dt - 1), dict(ldin=Dt - 1), dict(ldout=Dt - 1), dict(out=p(0)), dict(out=p(1)),
        dict(logdet=p(2)), dict(logdet=p(0)), dict(logdet=p(1)), dict(inverse=2), dict(inverse=-1),
        dict(inverse=1, out=p(1)), dict(inverse=1, ldst=W - 1)])
    bwd = dict(st=p(0), ldst=W, x=p(1), ldx=Dt, g0=p(2), ldg0=Dt, g1=p(3), ldg1=Dt, dst=p(4), lddst=W, dx=p(5), lddx=Dt,
               c=-0.25, tail_bound=3.0, B=B, Dt=Dt, bins=bins)
    refused("gm_nsf_couple_bwd", ops_fused.NsfCoupleBwdArgs, bwd, [
        dict(B=0), dict(Dt=0), dict(Dt=4097), dict(bins=5), dict(bins=0), dict(bins=64), dict(tail_bound=0.0),
        dict(tail_bound=65.0), dict(tail_bound=float("nan")), dict(c=float("nan")), dict(c=float("inf")), dict(st=None),
        dict(x=None), dict(g0=None), dict(dst=None), dict(ldst=W - 1), dict(ldx=Dt - 1), dict(ldg0=Dt - 1),
        dict(ldg1=Dt - 1), dict(lddst=W - 1), dict(bins=16, lddst=47 * Dt - 1, ldst=47 * Dt), dict(lddx=Dt - 1),
        dict(dx=p(4)), dict(dst=p(0)), dict(dst=p(1)), dict(dst=p(2)), dict(dst=p(3)), dict(dx=p(0)), dict(dx=p(1)),
        dict(dx=p(2)), dict(dx=p(3))])
    for t in a:
        assert not t.any()                                                # nothing was written
    with pytest.raises(_lib.GMError):
        _lib.call("gm_nsf_couple", None, None)


def test_resource_table_lists_the_six_kernels_without_scratch_or_spills():
    table = json.load(open(os.path.join(os.path.dirname(HERE), "profiles", "kernel_resources.json")))
    for kernel in ("nsf_couple_kernel", "nsf_couple_bwd_kernel"):
        rows = {k: v for k, v in table.items() if k.startswith(kernel + "<")}
        assert sorted(rows) == sorted("%s<%d>" % (kernel, n) for n in BINS), rows.keys()
        for k, r in rows.items():
            assert r["scratch"] == 0 and r["spills"] == 0, (k, r)
            assert r["vgpr"] + r["agpr"] <= 512, (k, r)               # one 256-thread workgroup per CU at the least


@pytest.mark.parametrize("N_", [9016, 18424])
def test_the_wide_conditioner_gemms_have_a_launch_plan(N_):
    """out is H -> P Dt: 9016 columns at 8 bins and 18 424 at 16 for 784-pixel images, wider than anything else in the
    package.  The library's own dispatch, run dry, plans every GEMM of the batch at that width, mirrored too."""
    for M, K, Nn in ((512, 400, N_), (512, N_, 400), (16, 8, N_)):
        for mode, on in (("fwd", ("X", "W", "Y")), ("dx", ("dA", "W", "dX")), ("dw", ("dA", "X", "dW"))):
            c = lp.Case("", mode, M, K, Nn, on, {}, {}, None)
            m, d = lp.descriptor(c, lp.placeholder_pointers(c))
            plan = ops.linear_plan(m, d)
            assert plan["launches"] == 1 and plan["family"] in ("lds", "k32", "split"), (mode, M, K, Nn, plan)
            assert 1 <= plan["grid_x"] <= 65535 * 32 and 1 <= plan["grid_y"] <= 65535, plan


class _Mine(spline_flow.SplineFlowTrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_path_selection():
    assert _trainer(spline_flow.SplineFlow(16, 8, 3))._stock()
    assert _trainer(spline_flow.SplineFlow(7, 1, 1, 4, 64.0, "half", 0.0, 2))._stock()
    assert _trainer(spline_flow.SplineFlow(16, 8, 16, 16))._stock()
    assert not _trainer(spline_flow.SplineFlow(16, 8, 3), cls=_Mine)._stock()      # an overridden hook
    m = spline_flow.SplineFlow(16, 8, 3)
    m.couplings[1].extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock()                                                # an edited coupling
    m = spline_flow.SplineFlow(16, 8, 3)
    m.couplings[2].out = torch.nn.Linear(8, 16)
    assert not _trainer(m)._stock()                                                # RealNVP's width is not the spline's
    m = spline_flow.SplineFlow(16, 8, 3)
    m.num_bins = 4
    assert not _trainer(m)._stock()                                                # out layers of another bin count
    m = spline_flow.SplineFlow(16, 8, 3)
    m.couplings.append(spline_flow.SplineCoupling(8, 8, 8, 8))
    assert not _trainer(m)._stock()
    m = spline_flow.SplineFlow(16, 8, 3)
    m.tail_bound = 65.0
    assert not _trainer(m)._stock()                                                # a setting outside the kernels' limits
    assert not gnvp.realnvp_fused_ok(spline_flow.SplineFlow(16, 8, 3))
    assert not nsf.spline_fused_ok(gnvp.RealNVP(16, 8, 3))

    class Sub(spline_flow.SplineFlow):
        pass
    assert not _trainer(Sub(16, 8, 3))._stock()                                    # a subclassed model


def test_data_parallel_is_refused():
    m = spline_flow.SplineFlow(16, 8, 3)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            nsf.SplineFlowEngine(m, "cpu", trainer=_trainer(m), **kw)
    tr = _trainer(m)
    tr.force_dp = True
    with pytest.raises(_lib.GMError, match="one GPU"):
        tr.train(1)
    m.couplings[0].extra = torch.nn.Linear(2, 2)
    with pytest.raises(_lib.GMError, match="general path"):
        nsf.SplineFlowEngine(m, "cpu", trainer=_trainer(m))
    with pytest.raises(_lib.GMError, match="general path"):
        nsf.SplineFlowEngine(gnvp.RealNVP(16, 8, 3), "cpu", trainer=_trainer(m))


def test_checkpoint_config_is_checked_under_strict():
    m = spline_flow.SplineFlow(16, 8, 2, 4, 2.5, "half", 0.1, 64)
    tr = _trainer(m)
    tr.seed = 9
    eng = nsf.SplineFlowEngine(m, "cpu", trainer=tr)
    now = eng._settings()
    assert now == {"mask": "half", "alpha": 0.1, "levels": 64, "num_bins": 4, "tail_bound": 2.5, "seed": 9}
    n = eng.fp.m.numel()
    for key, other in (("mask", "checker"), ("alpha", 0.05), ("levels", 256), ("num_bins", 8), ("tail_bound", 3.0),
                       ("seed", 0)):
        saved = dict(now, B=8, lr=1e-3, weight_decay=0.0)
        saved[key] = other
        resume = {"m": torch.zeros(n), "v": torch.zeros(n), "step": 5, "config": saved}
        with pytest.raises(_lib.GMError, match="different settings") as ei:
            eng.configure(8, 5, 1e-3, 0.0, resume=resume)
        assert key in str(ei.value)


def test_the_gradient_comparisons_leave_out_at_most_a_thousandth_of_the_pixels():
    """The GPU test's kernel cases, by the reference alone: pixels whose fp64 xi lies within 1e-5 of a knot (where the
    log-determinant's gradient jumps) are at most 0.1 % of the in-range pixels, summed over the cases of a (bins, tail)
    pair and in the largest case alone."""
    for bins in BINS:
        for tail in (3.0, 0.75):
            ex = ins = 0
            for b, dt, bn, tl, seed in N.KERNEL_CASES:
                if (bn, tl) != (bins, tail):
                    continue
                st, x, _, _ = N.kernel_inputs(b, dt, bins, tail, seed)
                e, i = N.near_knot(st, x, bins, tail)
                ex, ins = ex + int(e.sum()), ins + int(i.sum())
                if dt == 392:
                    assert int(e.sum()) <= N.KNOT_SHARE * int(i.sum()), (bins, tail, int(e.sum()), int(i.sum()))
            print("bins", bins, "tail", tail, "excluded", ex, "of", ins)
            assert ex <= N.KNOT_SHARE * ins


def test_reference_training_clears_the_learning_tests_bound():
    """The GPU learning test's premise, checked on its reference: 152 Adam batches of 16 on RealNVP's 4-pattern data take
    the fp64 reference's validation NLL below the identity flow's on the same validation stream."""
    D, H, K, b, bins = 16, 8, 4, 16, 8
    cfg = cfg_of(K, bins)
    x = N.pattern_data(64, D)
    torch.manual_seed(1234)
    m = spline_flow.SplineFlow(D, H, K, bins)
    noise = lambda tag, step, n: torch.from_numpy(gnvp.uniforms_reference(n, D, 5, step, tag).astype(np.float64))
    ident = np.mean([(N.nll_rows(N.f64(m.state_dict()), x[i:i + b].double(), noise(N.TAG_EVAL, i // b, b), cfg).mean()).item()
                     for i in range(0, 64, b)])
    P = {n: torch.nn.Parameter(v) for n, v in N.f64(m.state_dict()).items()}
    opt = torch.optim.Adam(list(P.values()), lr=1e-3)
    g = torch.Generator().manual_seed(0)
    for step in range(152):
        xb = x[torch.randperm(64, generator=g)[:b]].double()
        opt.zero_grad()
        (N.nll_rows(P, xb, noise(N.TAG_TRAIN, step, b), cfg).sum() / b).backward()
        opt.step()
    with torch.no_grad():
        val = np.mean([(N.nll_rows(P, x[i:i + b].double(), noise(N.TAG_EVAL, i // b, b), cfg).mean()).item()
                       for i in range(0, 64, b)])
    print("identity", ident, "trained", val)
    assert val < ident
