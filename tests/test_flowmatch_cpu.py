"""Flow matching without a GPU: the trace identity behind the exact divergence against autograd's Jacobian, the
reference validated on a field with a closed form (an all-lit, affine field: the divergence is a constant trace and the
log-likelihood converges to the analytic one at each solver's order), ode_table, the tables, the numpy noise rule, the
refusals, the C-ABI of the new kernels and its refusals, the resource table's new rows, path selection and the
drop-in module's exports."""
import ctypes
import inspect
import json
import math
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

import flow_matching  # noqa: E402
import flowmatch_reference as R  # noqa: E402
from generative_models_amd import _lib, ops_fused, philox  # noqa: E402
from generative_models_amd import flowmatch as gfm  # noqa: E402

KERNELS = ("fm_qsample_kernel", "fm_gather_qsample_kernel", "fm_div_kernel", "fm_div_finish_kernel", "fm_stage_kernel")


def _random_params(I, H, E, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(zip(R.NAMES, (r(H, I + E), r(H), r(H, H), r(H), r(I, H), r(I))))


@pytest.mark.parametrize("I,H,E", [(6, 5, 4), (13, 7, 4)])
def test_trace_identity_against_autograds_jacobian(I, H, E):
    P = _random_params(I, H, E, seed=I)
    g = torch.Generator().manual_seed(100 + I)
    xin = torch.randn(9, I + E, generator=g, dtype=torch.float64)
    div = R.divergence(P, xin, I)
    seen = set()
    for b in range(xin.shape[0]):
        tr = R.jacobian_trace(P, xin[b], I)
        assert abs(float(div[b] - tr)) <= 1e-12 * max(1.0, abs(float(tr))), (b, float(div[b]), float(tr))
        a1, a2 = R.pre_activations(P, xin[b:b + 1])
        seen.add((tuple((a1 > 0).flatten().tolist()), tuple((a2 > 0).flatten().tolist())))
    assert len(seen) > 1                                                    # the rows differ in their ReLU patterns
    # relu'(0) = 0: a unit whose pre-activation is exactly 0.0 or -0.0 is not lit -- in the reference's own divergence()
    assert R.patterns(torch.tensor([0.0, -0.0, 5e-324, -1.0, 2.0], dtype=torch.float64)).tolist() == [0, 0, 1, 0, 1]
    P0 = {k: v.clone() for k, v in P.items()}
    P0[R.NAMES[1]][0], P0[R.NAMES[1]][1] = 0.0, -0.0                        # at the input row 0 units 0 and 1 of the first
    x0 = torch.zeros(1, I + E, dtype=torch.float64)                         # layer sit at exactly zero, weights and all
    a1, a2 = R.pre_activations(P0, x0)
    assert a1[0, 0] == 0 and a1[0, 1] == 0 and (a1[0, 2:] != 0).all()
    Q0 = R.divergence_matrix(P0, I)
    m1, m2 = (a1 > 0).double(), (a2 > 0).double()
    assert m2.sum() > 0
    m1z = m1.clone()
    m1z[0, :2] = 1.0                                                        # what lighting the two units would add
    div0 = R.divergence(P0, x0, I)
    assert torch.equal(div0, R.divergence_of_patterns(Q0, m1, m2))
    assert not torch.equal(div0, R.divergence_of_patterns(Q0, m1z, m2))
    tr = R.jacobian_trace(P0, x0[0], I)                                     # autograd's relu'(0) is 0 as well
    assert abs(float(div0[0] - tr)) <= 1e-12 * max(1.0, abs(float(tr)))


def test_the_end_to_end_case_meets_its_cap_on_marked_rows_for_the_reference_alone():
    """flowmatch_reference.e2e_measure on this CPU: at most 5 % of the rows come near a ReLU switch (the condition of the
    GPU test's end-to-end case, met by the reference alone), and twice the fp32 run's deviations stay within the bound
    derived from the recorded figures."""
    got = R.e2e_measure()
    print(got)
    assert got["marked"] <= R.E2E_MAX_MARKED
    assert set(R.E2E_FP32_DEV) == {"nll", "z", "x"}
    for k in R.E2E_FP32_DEV:
        assert 2 * got[k] <= R.E2E_TOL, (k, got[k])
    assert R.E2E_TOL == max(R.LOSS_TOL, 2 * max(R.E2E_FP32_DEV.values()))


# The closed-form case: reference.affine_model(I = 6, H = 5, E = 4, seed 0, weights 0.3 N(0, 1), biases 20) on rows
# y1 = 1.5 N(0, 1) (seed 1), T = 64, steps 4 -> 8 -> 16, the tableau's coefficients unrounded (the device's fp32 table
# puts a floor of about 1e-5 under rk4's error here).  The fp64 reference gives the log-likelihood's error ratios
#   euler 1.78, 1.90;  heun 4.06, 4.03;  rk4 16.88, 16.45,   each within a factor 1.5 of 2, 4 and 16.
AFFINE = dict(I=6, H=5, E=4, T=64, steps=(4, 8, 16))
ORDER = {"euler": 2.0, "heun": 4.0, "rk4": 16.0}


def _affine_case():
    c = AFFINE
    P = R.affine_model(c["I"], c["H"], c["E"])
    g = torch.Generator().manual_seed(1)
    y1 = 1.5 * torch.randn(16, c["I"], generator=g, dtype=torch.float64)
    return c, P, y1


def test_all_lit_field_has_a_constant_divergence():
    c, P, y1 = _affine_case()
    A, _ = R.affine_form(P, c["I"])
    temb = torch.from_numpy(gfm.tables(c["T"], c["E"])["temb"])
    for j in (0, 17, c["T"]):
        xin = torch.cat([y1, temb[j].expand(y1.shape[0], c["E"])], dim=1)
        a1, a2 = R.pre_activations(P, xin)
        assert a1.min() > 1.0 and a2.min() > 1.0                            # every ReLU lit, with room
        div = R.divergence(P, xin, c["I"])
        assert (div - A.diagonal().sum()).abs().max() <= 1e-13
        v = R.forward(P, xin)
        Aa, cc = R.affine_form(P, c["I"])
        assert (v - (y1 @ Aa.T + cc)).abs().max() <= 1e-12                  # the field is A y + c there


@pytest.mark.parametrize("solver", ["euler", "heun", "rk4"])
def test_reference_converges_to_the_closed_form_at_the_solvers_order(solver):
    c, P, y1 = _affine_case()
    z_ex, l_ex = R.affine_solution(P, y1, c["I"])
    ll_ex = -R.nll_rows(z_ex, torch.zeros(16, dtype=torch.float64), l_ex, c["I"], 256)
    errs = []
    for steps in c["steps"]:
        z, l, marked = R.solve(P, y1, c["T"], c["E"], steps, solver, -1, fp32_table=False)
        assert not marked.any()
        assert (l - l_ex).abs().max() <= 1e-7                               # a constant integrand: exact up to the table's fp32 h b
        ll = -R.nll_rows(z, torch.zeros(16, dtype=torch.float64), l, c["I"], 256)
        errs.append(float((ll - ll_ex).abs().max()))
    ratios = [errs[i] / errs[i + 1] for i in range(len(errs) - 1)]
    print(solver, "errors", errs, "ratios", ratios)
    for r in ratios:
        assert ORDER[solver] / 1.5 <= r <= ORDER[solver] * 1.5, (solver, errs, ratios)
    # and forward again: decode(encode) returns the start to the solver's accuracy
    z, _, _ = R.solve(P, y1, c["T"], c["E"], c["steps"][-1], "rk4", -1)
    back, l2, _ = R.solve(P, z, c["T"], c["E"], c["steps"][-1], "rk4", 1)
    assert (back - y1).abs().max() <= 1e-6 and (l2 + l_ex).abs().max() <= 1e-7


@pytest.mark.parametrize("solver", ["euler", "heun", "rk4"])
@pytest.mark.parametrize("direction", [1, -1])
def test_ode_table(solver, direction):
    T = 48
    a, b, cc = gfm.TABLEAUS[solver]
    ns = len(b)
    assert abs(sum(b) - 1.0) <= 1e-15 and len(a) == ns - 1 and len(cc) == ns
    for steps in (1, 2, 6, 24):
        tab = gfm.ode_table(T, steps, solver, direction)
        assert tab.shape == (steps * ns, 8) and tab.dtype == np.float64
        h = direction / steps
        for n in range(steps):
            rows = tab[n * ns:(n + 1) * ns]
            assert abs(rows[:, 1].sum() - h) <= 1e-15                       # the b of a step sum to h
            assert list(rows[:, 2]) == [1.0] + [0.0] * (ns - 1) and list(rows[:, 3]) == [0.0] * (ns - 1) + [1.0]
            assert rows[-1, 0] == 0.0
            j0 = n * (T // steps) if direction == 1 else T - n * (T // steps)
            for i in range(ns):
                assert rows[i, 5] == j0 + direction * cc[i] * (T // steps)
                if i < ns - 1:
                    assert abs(rows[i, 0] - h * a[i]) <= 1e-15
        j = tab[:, 5]
        assert np.all(j == np.round(j)) and j.min() >= 0 and j.max() <= T  # every evaluation on the grid
        assert np.array_equal(tab[:-1, 4], tab[1:, 5]) and tab[-1, 4] == -1.0
        assert j[0] == (0 if direction == 1 else T) and np.all(tab[:, 6:] == 0)
    ok = {"euler": 5, "heun": 5, "rk4": 4}[solver]
    gfm.ode_table(40, ok, solver, direction)
    for T_, steps in ((48, 5), (48, 0), (48, -2), (50, 7)) + (((50, 50), (48, 16)) if solver == "rk4" else ()):
        if solver == "rk4" and (T_, steps) == (48, 16):
            continue
        with pytest.raises(gfm.FlowMatchError):
            gfm.ode_table(T_, steps, solver, direction)
    for bad in (dict(solver="midpoint"), dict(solver=None), dict(direction=0), dict(direction=2), dict(steps=2.0),
                dict(steps=True)):
        with pytest.raises(gfm.FlowMatchError):
            gfm.ode_table(**dict(dict(T=48, steps=2, solver=solver, direction=direction), **bad))
    with pytest.raises(gfm.FlowMatchError):
        gfm.ode_table(50, 50, "rk4", 1)                                     # 2 steps must divide T
    assert gfm.ode_table(50, 25, "rk4", 1).shape == (100, 8)


def test_tables_and_the_noise_rule():
    T, E = 50, 8
    tab = gfm.tables(T, E)
    assert tab["tt"].shape == tab["tc"].shape == (T + 1,) and tab["temb"].shape == (T + 1, E)
    assert tab["tt"][0] == 0 and tab["tt"][T] == 1 and tab["tc"][0] == 1 and tab["tc"][T] == 0
    assert np.allclose(tab["tt"] + tab["tc"], 1.0, atol=1e-16)
    f = np.exp(-math.log(1e4) * np.arange(E // 2) / (E // 2))
    assert np.allclose(tab["temb"][7], np.concatenate([np.sin(1000.0 * 7 / T * f), np.cos(1000.0 * 7 / T * f)]), atol=1e-12)
    m = flow_matching.FlowMatching(16, 12, E, T)
    assert {n for n, _ in m.named_buffers()} == {"tt", "tc", "temb"} and all(b.dtype == torch.float32 for b in m.buffers())
    assert torch.equal(m.temb, torch.from_numpy(tab["temb"].astype(np.float32)))
    # j: mulhi of word 0, in [0, T], every grid point reached
    for seed, step, row0 in ((0, 0, 0), (2 ** 40 + 5, 7, 3)):
        j = gfm.grid_index_reference(4000, T, seed, step, gfm.TAG_T, row0)
        w = philox.words(4000, 1, seed, step, gfm.TAG_T, row0)[:, 0].astype(np.uint64)
        assert np.array_equal(j, (w * np.uint64(T + 1)) >> np.uint64(32)) and j.min() == 0 and j.max() == T
        assert len(np.unique(j)) == T + 1
    assert [t.to_bytes(4, "big") for t in (gfm.TAG_D, gfm.TAG_T, gfm.TAG_N, gfm.TAG_VD, gfm.TAG_VT, gfm.TAG_VN)] == \
        [b"FMTD", b"FMTT", b"FMTN", b"FMVD", b"FMVT", b"FMVN"]
    # the path in numpy: j = 0 gives y0, j = T gives y1, exactly
    g = np.random.default_rng(0)
    y1, y0 = g.standard_normal((3, 5)).astype(np.float32), g.standard_normal((3, 5)).astype(np.float32)
    yt, u = gfm.path_reference(y1, y0, np.array([0, T, 13]), T)
    assert np.array_equal(yt[0], y0[0]) and np.array_equal(yt[1], y1[1]) and np.array_equal(u, y1 - y0)
    assert np.allclose(yt[2], 13 / T * y1[2] + (T - 13) / T * y0[2], atol=1e-6)


def test_module_surface_and_exports():
    for n in ("VelocityField", "FlowMatching", "FlowMatchingTrainer", "FlowMatchError"):
        assert hasattr(flow_matching, n), n
    assert flow_matching.FlowMatchingTrainer is gfm.FlowMatchTrainer
    import generative_models_amd as pkg
    assert pkg.FlowMatching is gfm.FlowMatching and pkg.FlowMatchTrainer is gfm.FlowMatchTrainer
    assert pkg.FlowMatchEngine is gfm.FlowMatchEngine
    m = flow_matching.FlowMatching(16, 12, 8, 50)
    assert list(m.state_dict()) == list(R.NAMES) and type(m.field) is flow_matching.VelocityField
    assert not m.field.out.weight.any() and not m.field.out.bias.any()      # a fresh model is the identity flow
    assert (tuple(m.field.linear.weight.shape), tuple(m.field.hidden.weight.shape), tuple(m.field.out.weight.shape)) == \
        ((12, 24), (12, 12), (16, 12))
    sig = inspect.signature(flow_matching.FlowMatching.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[1:]] == [("image_size", 784), ("hidden_dim", 400),
                                                                  ("time_dim", 32), ("T", 1000)]
    T = gfm.FlowMatchTrainer
    sig = inspect.signature(T.__init__).parameters
    assert [(n, p.default) for n, p in list(sig.items())[5:]] == [("seed", 0), ("alpha", 0.05), ("levels", 256),
                                                                  ("viz", False)]
    p = inspect.signature(T.sample).parameters
    assert [(n, q.default) for n, q in list(p.items())[1:]] == [("n", inspect.Parameter.empty), ("seed", 0),
                                                                ("temperature", 1.0), ("steps", 50), ("solver", "heun"),
                                                                ("return_trajectory", False)]
    p = inspect.signature(T.encode).parameters
    assert (p["seed"].default, p["batch"].default, p["steps"].default, p["solver"].default) == (0, 1024, 100, "rk4")
    from generative_models_amd import engine, realnvp
    assert issubclass(T, realnvp.DequantFlowTrainer) and T._series == (("losses", "recon"),)
    assert issubclass(gfm.FlowMatchEngine, engine.VAEEngine) and "_gather_sample" in gfm.FlowMatchEngine.__dict__
    assert gfm.FlowMatchEngine._issue is engine.TimeRegressionEngine._issue        # the DDPM engine's step body
    for name in ("sample", "encode", "decode", "log_likelihood", "log_likelihood_rows", "bits_per_dim", "velocity",
                 "divergence", "parzen", "mmd", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(T, name)), name
    assert issubclass(gfm.FlowMatchError, _lib.GMError) and issubclass(gfm.FlowMatchError, ValueError)
    assert gfm.__doc__ and "The contract." in gfm.__doc__ and "not of the discrete map" in gfm.__doc__


def test_refusals():
    for args in ((0, 8, 8, 50), (8193, 8, 8, 50), (16, 0, 8, 50), (16, 1025, 8, 50), (16, 8, 6, 50), (16, 8, 0, 50),
                 (16, 8, 132, 50), (16, 8, 8, 1), (16, 8, 8, 4097), (16.0, 8, 8, 50), (16, 8, 8, True)):
        with pytest.raises(gfm.FlowMatchError) as ei:
            flow_matching.FlowMatching(*args)
        assert isinstance(ei.value, ValueError) and isinstance(ei.value, _lib.GMError)
    flow_matching.FlowMatching(1, 1, 4, 2), flow_matching.FlowMatching(64, 1024, 128, 4096)
    m = flow_matching.FlowMatching(16, 8, 8, 50)
    for kw in (dict(seed=-1), dict(seed=1.5), dict(alpha=0.5), dict(alpha=-0.1), dict(alpha=float("nan")),
               dict(levels=1), dict(levels=65537), dict(levels=2.0)):
        with pytest.raises(gfm.FlowMatchError):
            flow_matching.FlowMatchingTrainer(m, None, None, None, **kw)     # before anything is touched
    tr = object.__new__(gfm.FlowMatchTrainer)
    tr.model, tr.alpha, tr.levels, tr.seed = m, 0.05, 256, 0
    for kw in (dict(n=0), dict(n=2.0), dict(n=3, seed=-1), dict(n=3, temperature=-1.0), dict(n=3, steps=7),
               dict(n=3, steps=0), dict(n=3, solver="dopri5"), dict(n=3, steps=50, solver="rk4")):
        with pytest.raises(gfm.FlowMatchError):
            tr.sample(**kw)                                                 # refused before a device is looked for
    for fn in (tr.encode, tr.log_likelihood_rows, tr.decode):
        with pytest.raises(gfm.FlowMatchError):
            fn(torch.zeros(2, 16), steps=7)


def test_new_symbols_are_declared_and_bound():
    from generative_models_amd import _build
    assert _build.SOURCES[-1] == "gm_fm.hip" and "gm_gemm.hip" == _build.SOURCES[0]
    assert (_lib.FM_TAG_D, _lib.FM_MAX_H) == (0x464D5444, 1024)


def test_kernels_reject_null_and_out_of_limit_arguments():
    """Host arrays stand in for device ones: every call below must return before it launches anything."""
    lib = _lib.load()
    a = [np.zeros(1 << 12, dtype=np.float32) for _ in range(10)]
    p = lambda i: a[i].ctypes.data
    B, I, E, T, H = 5, 12, 8, 50, 7
    noise = lambda **kw: ctypes.byref(ops_fused.fm_noise(1, True, **kw))
    tabs = lambda **kw: ctypes.byref(ops_fused.FmTables(**dict(dict(tt=p(0), tc=p(1), temb=p(2), T=T, E=E), **kw)))

    def out(**kw):
        d = dict(xin=p(3), ldin=I + E, u=p(4), ldu=I, logdet=p(5), j=p(6), y1=None, ldy1=0, y0=None, ldy0=0,
                 alpha=0.05, levels=256)
        d.update(kw)
        return ctypes.byref(ops_fused.FmOut(**d))

    def qs(n=None, s=None, o=None, x=p(7), ldx=I, rows=B, I=I):
        return lib.gm_fm_qsample(None, n if n is not None else noise(), s if s is not None else tabs(),
                                 o if o is not None else out(), x, ldx, rows, I)

    idx = np.zeros(64, dtype=np.int64)

    def gq(o=None, data=p(7), n_rows=9, ix=idx.ctypes.data, dst=p(8), ld_out=I, B=B, I=I):
        return lib.gm_gather_rows_fm_qsample(None, noise(), tabs(), o if o is not None else out(), data, n_rows, ix,
                                             _lib.NO_SLOT, dst, ld_out, B, I)

    def gb(bits=p(7), wpr=1, n_rows=9, dst=p(8), ld_out=I, B=B, I=I):
        return lib.gm_gather_rows_bits_fm_qsample(None, noise(), tabs(), out(), bits, wpr, n_rows, idx.ctypes.data,
                                                  _lib.NO_SLOT, dst, ld_out, B, I)

    def div(**kw):
        d = dict(H1=p(0), ld1=H, H2=p(1), ld2=H, Q=p(2), ldq=H, part=p(3), part_floats=B, div=p(4), B=B, H=H)
        d.update(kw)
        return lib.gm_fm_div(None, ctypes.byref(ops_fused.FmDivArgs(**d)))

    def stage(**kw):
        d = dict(k=p(0), ldk=I, base=p(1), ldb=I, acc=p(2), lda=I, xin=p(3), ldin=I + E, L=p(4), div=p(5), div_stride=B,
                 div_parts=1, tab=p(6), slot=_lib.slot(0, 0, 0, 0, 8), temb=p(7), traj=None, traj_stride=0, tick=None,
                 done=None, rows=B, I=I, E=E, T=T, S=4, stages=2)
        d.update(kw)
        return lib.gm_fm_stage(None, ctypes.byref(ops_fused.FmStageArgs(**d)))

    null = lambda ct: ctypes.POINTER(ct)()
    cases = {
        qs: (dict(n=null(ops_fused.FmNoise)), dict(s=null(ops_fused.FmTables)), dict(o=null(ops_fused.FmOut)), dict(x=None), dict(ldx=I - 1), dict(rows=0), dict(I=0),
             dict(I=8193), dict(s=tabs(tt=None)), dict(s=tabs(tc=None)), dict(s=tabs(temb=None)), dict(s=tabs(E=6)),
             dict(s=tabs(E=0)), dict(s=tabs(E=132)), dict(s=tabs(T=1)), dict(s=tabs(T=4097)), dict(o=out(xin=None)),
             dict(o=out(u=None)), dict(o=out(logdet=None)), dict(o=out(ldin=I + E - 1)), dict(o=out(ldu=I - 1)),
             dict(o=out(y1=p(8), ldy1=I - 1)), dict(o=out(y0=p(8), ldy0=I - 1)), dict(o=out(alpha=0.5)),
             dict(o=out(alpha=-0.1)), dict(o=out(levels=1)), dict(o=out(levels=65537)), dict(o=out(u=p(3))),
             dict(x=p(3)), dict(n=noise(row0=-1)), dict(n=noise(row0=2 ** 32))),
        gq: (dict(data=None), dict(ix=None), dict(dst=None), dict(B=0), dict(I=0), dict(ld_out=I - 1), dict(n_rows=0),
             dict(o=out(xin=None)), dict(dst=p(3)), dict(dst=p(4)), dict(o=out(ldin=I + E - 1))),
        gb: (dict(bits=None), dict(dst=None), dict(B=0), dict(wpr=0), dict(ld_out=I - 1)),
        div: (dict(H1=None), dict(H2=None), dict(Q=None), dict(part=None), dict(B=0), dict(B=2 ** 30 + 1, part_floats=2 ** 40), dict(H=0), dict(H=1025),
              dict(ld1=H - 1), dict(ld2=H - 1), dict(ldq=H - 1), dict(part_floats=B - 1), dict(part=p(0)),
              dict(div=p(3)), dict(div=p(2))),
        stage: (dict(k=None), dict(base=None), dict(acc=None), dict(xin=None), dict(tab=None), dict(temb=None),
                dict(rows=0), dict(I=0), dict(I=8193), dict(E=6), dict(T=1), dict(S=0), dict(stages=0), dict(stages=5),
                dict(S=5), dict(ldk=I - 1), dict(ldb=I - 1), dict(lda=I - 1), dict(ldin=I + E - 1), dict(L=None),
                dict(div_parts=0), dict(div_parts=33), dict(div_parts=2, div_stride=B - 1),
                dict(slot=_lib.slot(0, 0, 0, 0, 4)), dict(base=p(0)), dict(acc=p(1)), dict(xin=p(2)),
                dict(traj=p(8), traj_stride=B * I - 1), dict(traj=p(3), traj_stride=B * I), dict(tick=p(9))),
    }
    for fn, kws in cases.items():
        for kw in kws:
            assert fn(**kw) == _lib.GM_EINVAL, (fn.__name__, kw)
            assert b"bad argument" in lib.gm_last_error()
    for t in a:
        assert not t.any()                                               # nothing was written
    assert not idx.any()


def test_resource_table_has_the_new_kernels_without_scratch_or_spills():
    table = json.load(open(os.path.join(ROOT, "profiles", "kernel_resources.json")))
    for k in KERNELS:
        rows = [v for n, v in table.items() if n.split("<")[0] == k]
        assert len(rows) == 1, k
        assert rows[0]["scratch"] == 0 and rows[0]["spills"] == 0, (k, rows[0])
    assert table["fm_div_kernel"]["lds"] == 0 and table["fm_div_kernel"]["agpr"] + table["fm_div_kernel"]["vgpr"] <= 128


# ---- path selection and the engine's host side ----------------------------------------------------------------------
def _loaders(n=40, batch=8, side=4):
    x = torch.rand(n, 1, side, side)
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, **kw):
    tr = object.__new__(cls or gfm.FlowMatchTrainer)         # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    tr.seed, tr.alpha, tr.levels, tr.noise_steps, tr._engine = 0, 0.05, 256, 0, None
    for n, v in kw.items():
        setattr(tr, n, v)
    return tr


class _Mine(gfm.FlowMatchTrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_path_selection():
    assert _trainer(flow_matching.FlowMatching(16, 8, 8, 50))._stock()
    assert not _trainer(flow_matching.FlowMatching(16, 8, 8, 50), cls=_Mine)._stock()       # an overridden hook
    assert not _trainer(flow_matching.FlowMatching(16, 8, 8, 50), alpha=0.7)._stock()       # settings the kernels refuse
    m = flow_matching.FlowMatching(16, 8, 8, 50)
    m.field.extra = torch.nn.Linear(2, 2)
    assert not _trainer(m)._stock() and not gfm.flowmatch_fused_ok(m)                       # an edited field

    class Sub(flow_matching.FlowMatching):
        pass
    assert not _trainer(Sub(16, 8, 8, 50))._stock()                                         # a subclassed model
    m = flow_matching.FlowMatching(16, 8, 8, 50)
    m.T = 60
    assert not gfm.flowmatch_fused_ok(m)                                                    # tables of another grid


def test_engine_refuses_data_parallelism_and_other_settings_on_resume():
    m = flow_matching.FlowMatching(16, 8, 8, 50)
    for kw in (dict(world_size=2), dict(force_dp=True)):
        with pytest.raises(_lib.GMError, match="one GPU"):
            gfm.FlowMatchEngine(m, "cpu", trainer=_trainer(m), **kw)
    bad = flow_matching.FlowMatching(16, 8, 8, 50)
    bad.field.extra = torch.nn.Linear(2, 2)
    with pytest.raises(_lib.GMError, match="general path"):
        gfm.FlowMatchEngine(bad, "cpu", trainer=_trainer(m))
    tr = _trainer(m, seed=9, alpha=0.1, levels=16)
    eng = gfm.FlowMatchEngine(m, "cpu", trainer=tr)
    now = eng._settings()
    assert now == {"T": 50, "time_dim": 8, "alpha": 0.1, "levels": 16, "seed": 9}
    n = eng.fp.m.numel()
    for key, other in (("T", 60), ("time_dim", 4), ("alpha", 0.05), ("levels", 256), ("seed", 0)):
        saved = dict(now, B=8, lr=1e-3, weight_decay=0.0)
        saved[key] = other
        resume = {"m": torch.zeros(n), "v": torch.zeros(n), "step": 5, "config": saved}
        with pytest.raises(_lib.GMError, match="different settings") as ei:
            eng.configure(8, 5, 1e-3, 0.0, resume=resume)
        assert key in str(ei.value)
