"""Every vector / element path of the non-GEMM kernels (tests/kernel_path_cases.py) on the GPU, inside the guarded buffers
of tests/guarded.py: the arms the project's own workload (I = 784, H = 400, Z = 20, fresh allocations: always the vector
arm, below every cap) never takes.

Each array of a call sits in a NaN-filled backing buffer (guards before and after, the pad columns of `ld > width`, the
other slots of a ring, the output rectangle itself).  After the call

1. every float outside the output rectangles is bit-identical to what it was, inputs entirely (int32 view);
2. no output element still holds the NaN pattern;
3. the values are compared with an fp64 evaluation of the same expression (kernel_path_cases.row_errors): by close64's
   rule -- HIP error <= 2 x the fp32 CPU evaluation's own error + 2^-23 of the scale -- for the reductions an fp32
   evaluation exists for (row norms, dot products, column sums, the finalised sums), by the tolerance the kernel's
   per-op test states elsewhere, never a looser one; per-row arrays (pen, n, share, s, the partials) row by row against
   each row's OWN scale.  Exact results (masks, copies, gathers, zero-norm rows) are compared bit for bit.

A NaN read from a pad or a guard that reaches the arithmetic fails step 3; the kernels' clamped loads stay inside the
row.  Every comparison prints e_hip, e_cpu, its bound and their ratio; the last test prints the worst ratio per kernel
as the rows of profiles/kernel_path_errors.md."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import kernel_path_cases as kp  # noqa: E402
from guarded import NAN_BITS, RING, Array, Placed  # noqa: E402
from generative_models_amd import ops, ops_fused as of  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda:0"
LAM = kp.LAM
STATS = {}                              # kernel -> comparisons, worst ratio and where
SHARED = {}                             # outputs that must be bit-identical across the placements of the same inputs


def params(kernel):
    cs = kp.cases(kernel)
    return pytest.mark.parametrize("c", cs, ids=[c.id for c in cs])


# ---- placement ----------------------------------------------------------------------------------------------------------
def arr(c, name, rows, width, role, ring=1):
    return Array(name, rows, width, width + c.ld.get(name, 0), 1 if name in c.off else 0, role, ring)


def mat(c, name, rows, width, role, values=None, ring=1):
    return Placed(arr(c, name, rows, width, role, ring), values, dev=DEV)


def vec(c, name, n, role, values=None, ring=1):
    return Placed(arr(c, name, 1, n, role, ring), values, vector=True, dev=DEV)


def ring_arg(p):
    """(tensor, slot) a wrapper reads the placed array through: slot 0's view and the ring slot, or the view itself."""
    if p.array.ring > 1:
        return p.first, ops.slot(0, 0, p.pick, p.array.ring, p.stride)
    return p.view, ops.NO_SLOT


def flat(p):
    return p.view.reshape(-1)


def slot1(p):
    """A one-float output addressed as element 1 of a three-float window: its neighbours are guards."""
    return p.buf[p.base - 1:p.base + 2], ops.slot(0, 0, 1, 0, 1)


def finish(c, placed):
    torch.cuda.synchronize()
    touched = [n for n, p in placed.items() if not p.untouched_outside()]
    assert not touched, "%s: floats outside the output rectangle changed in %s" % (c.id, touched)
    left = {n: p.unwritten() for n, p in placed.items() if p.array.role == "out" and p.unwritten()}
    assert not left, "%s: output elements never written: %s" % (c.id, left)


def stat(c):
    st = STATS.setdefault(c.kernel, dict(n=0, ratio=-1.0, at=None, e_hip=0.0, e_cpu=0.0, cases=set()))
    st["n"] += 1
    st["cases"].add(c.id)
    return st


def check(c, what, got, ref64, ref32=None, tol=None, rows=False, scale=None):
    ratio, e_hip, e_cpu, bound, r = kp.row_errors(got, ref64, ref32, tol, rows, scale)
    st = stat(c)
    if ratio > st["ratio"]:
        st.update(ratio=ratio, at="%s %s" % (c.id, what), e_hip=e_hip, e_cpu=e_cpu)
    print("%s %s: e_hip %.3e e_cpu %.3e bound %.3e (%s) ratio %.3f row %d" %
          (c.id, what, e_hip, e_cpu, bound, "tolerance" if tol is not None else "2 e_cpu + 2^-23", ratio, r))
    assert ratio <= 1.0, "%s %s: HIP err %.3e > bound %.3e (e_cpu %.3e) at row %d" % (c.id, what, e_hip, bound, e_cpu, r)


def exact(c, what, got, want):
    st = stat(c)
    st["ratio"] = max(st["ratio"], 0.0)
    st["at"] = st["at"] or "%s %s" % (c.id, what)
    got, want = got.detach().cpu().contiguous(), want.detach().cpu().contiguous()
    assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), \
        "%s: %s is not bit-identical" % (c.id, what)


def shared(c, key, what, got, group=None):
    """`got` is bit-identical across every placement of the same inputs (an elementwise result)."""
    st = stat(c)
    st["ratio"] = max(st["ratio"], 0.0)
    st["at"] = st["at"] or "%s %s" % (c.id, what)
    got = got.detach().cpu().contiguous().clone()
    first = SHARED.setdefault((group or c.kernel,) + key + (what,), (c.id, got))
    assert torch.equal(first[1].view(torch.int32), got.view(torch.int32)), \
        "%s: %s differs from the same inputs' result at %s" % (c.id, what, first[0])


def refs(fn, *a):
    return fn(*a, torch.float64), fn(*a, torch.float32)


# ---- 2. row kernels with a register-resident vector path and a width cap ---------------------------------------------
@params("gp_norm")
def test_gp_norm(c):
    """pen and gamma within test_wgangp_penalty_chain_vs_autograd's 5e-6, of each row's own scale; the all-zero row gives
    gamma exactly 0 and pen exactly k * k."""
    t, k, B, I = kp.row_inputs("gp_norm", c.B, c.W), c.flags["k"], c.B, c.W
    r64, r32 = refs(kp.ref_gp_norm, t, k)
    P = dict(g=mat(c, "g", B, I, "in", t["g"]), gamma=mat(c, "gamma", B, I, "out"), pen=vec(c, "pen", B, "out"))
    of.gp_norm(P["g"].view, P["gamma"].view, flat(P["pen"]), LAM, kp.inv_b(B), k=k)
    finish(c, P)
    check(c, "pen", flat(P["pen"]), r64["pen"], r32["pen"], tol=5e-6, rows=True)
    check(c, "gamma", P["gamma"].view, r64["gamma"], r32["gamma"], tol=5e-6, rows=True)
    if B > 1:
        assert float(P["gamma"].view[1].abs().max()) == 0.0 and float(flat(P["pen"])[1]) == float(np.float32(k) * np.float32(k))


@params("pdw_dir")
def test_pdw_dir(c):
    """pen and gamma within test_pdw_dir_vs_fp64's 2e-5, of each row's own scale; the x == xr row has d = 0."""
    t, B, I = kp.row_inputs("pdw_dir", c.B, c.W), c.B, c.W
    r64, r32 = refs(kp.ref_pdw, t)
    P = dict(g=mat(c, "g", B, I, "in", t["g"]), x=mat(c, "x", B, I, "in", t["x"]), xr=mat(c, "xr", B, I, "in", t["xr"]),
             n=vec(c, "n", B, "in", t["n"]), gamma=mat(c, "gamma", B, I, "out"), pen=vec(c, "pen", B, "out"))
    of.pdw_dir(P["g"].view, P["x"].view, P["xr"].view, flat(P["n"]), P["gamma"].view, flat(P["pen"]), LAM, kp.inv_b(B))
    finish(c, P)
    check(c, "pen", flat(P["pen"]), r64["pen"], r32["pen"], tol=2e-5, rows=True)
    check(c, "gamma", P["gamma"].view, r64["gamma"], r32["gamma"], tol=2e-5, rows=True)


@params("pdw_couple")
def test_pdw_couple(c):
    """n and share (row norms) by close64 per row; dA and xhat within test_pdw_couple_vs_fp64's 2e-5 of each row's scale;
    xcopy bit-equal to x, xhat bit-equal across placements; the x == xr row: n, share and dA exactly 0."""
    t, B, I = kp.row_inputs("pdw_couple", c.B, c.W), c.B, c.W
    r64, r32 = refs(kp.ref_pdw, t)
    has = lambda n: n not in c.absent
    P = dict(x=mat(c, "x", B, I, "in", t["x"]), xr=mat(c, "xr", B, I, "in", t["xr"]), share=vec(c, "share", B, "out"))
    if has("n"):
        P["n"] = vec(c, "n", B, "out")
    if has("t"):
        P["t"] = vec(c, "t", B, "in", t["t"], ring=RING if c.flags.get("ring") else 1)
    for name in ("dA", "xhat", "xcopy"):
        if has(name):
            P[name] = mat(c, name, B, I, "out")
    tt, t_slot = ring_arg(P["t"]) if has("t") else (None, ops.NO_SLOT)
    v = lambda n: P[n].view if n in P else None
    of.pdw_couple(P["x"].view, P["xr"].view, flat(P["share"]), B, inv_b=kp.inv_b(B), n=flat(P["n"]) if has("n") else None,
                  t=tt.reshape(-1) if tt is not None else None, t_slot=t_slot, dA=v("dA"), xhat=v("xhat"), xcopy=v("xcopy"))
    finish(c, P)
    check(c, "share", flat(P["share"]), r64["share"], r32["share"], rows=True)
    if has("n"):
        check(c, "n", flat(P["n"]), r64["n"], r32["n"], rows=True)
    if has("dA"):
        check(c, "dA", P["dA"].view, r64["dA"], r32["dA"], tol=2e-5, rows=True)
    if has("xhat"):
        check(c, "xhat", P["xhat"].view, r64["xhat"], r32["xhat"], tol=2e-5, rows=True)
        shared(c, (B, I), "xhat", P["xhat"].view)                    # it does not depend on the row norm
    if has("xcopy"):
        exact(c, "xcopy", P["xcopy"].view, t["x"])
    if B > 1:
        assert float(flat(P["share"])[1]) == 0.0
        assert not has("n") or float(flat(P["n"])[1]) == 0.0
        assert not has("dA") or float(P["dA"].view[1].abs().max()) == 0.0


@params("head_gp")
def test_head_gp(c):
    """s against fp64 by close64 per row; u bit-equal to w2 or to 0 by the mask [s > 0][h > 0] of the fp64 reference (no
    row is within rounding of the kink: tests/test_kernel_path_cases_cpu.py)."""
    t, B, H = kp.row_inputs("head_gp", c.B, c.W), c.B, c.W
    r64, r32 = refs(kp.ref_head_gp, t)
    assert r64["a2"].abs().min().item() > 1e-3                       # on the inputs: every mask is defined
    P = dict(h=mat(c, "h", B, H, "in", t["h"]), w2=vec(c, "w2", H, "in", t["w2"]), b2=vec(c, "b2", 1, "in", t["b2"]),
             s=vec(c, "s", B, "out"), u=mat(c, "u", B, H, "out"))
    of.head_gp(P["h"].view, P["w2"].view, flat(P["b2"]), flat(P["s"]), P["u"].view)
    finish(c, P)
    check(c, "s", flat(P["s"]), r64["s"], r32["s"], rows=True)
    mask = (r64["s"] > 0)[:, None] & (t["h"] > 0)
    exact(c, "u", P["u"].view, torch.where(mask, t["w2"][None, :].expand(B, H), torch.zeros(B, H)))
    dead = r64["s"] == 0
    assert float(flat(P["s"]).cpu()[dead].abs().sum()) == 0.0 and float(P["u"].view.cpu()[dead].abs().sum()) == 0.0


# ---- 3. column reductions --------------------------------------------------------------------------------------------
@params("gp_dw2")
def test_gp_dw2(c):
    """The column sums by close64 and within test_wgangp_penalty_chain_vs_autograd's 1e-5; h and t strided (ld = H + 3)."""
    t, B, H, store = kp.column_inputs("gp_dw2", c.B, c.W), c.B, c.W, c.flags["store"]
    r64, r32 = refs(kp.ref_gp_dw2, t, store)
    P = dict(s=vec(c, "s", B, "in", t["s"]), h=mat(c, "h", B, H, "in", t["h"]), t=mat(c, "t", B, H, "in", t["t"]),
             gw2=vec(c, "gw2", H, "out", None if store else t["gw2"]))
    (of.gp_dw2_store if store else of.gp_dw2)(flat(P["s"]), P["h"].view, P["t"].view, flat(P["gw2"]))
    finish(c, P)
    check(c, "gw2", flat(P["gw2"]), r64["gw2"], r32["gw2"])
    check(c, "gw2 (1e-5)", flat(P["gw2"]), r64["gw2"], r32["gw2"], tol=1e-5)


@params("dragan_head_bwd")
def test_dragan_head_bwd(c):
    """gw2 (column sums), gb2 (fp64 sum of da2) and dA1 (one product) by close64; gw2 and gb2 also within
    test_dragan_penalty_chain_vs_autograd's 2e-5; H, T and dA1 strided (ld = Hd + 3)."""
    t, B, H, store = kp.column_inputs("dragan_head_bwd", c.B, c.W), c.B, c.W, c.flags["store"]
    r64, r32 = refs(kp.ref_dragan_head_bwd, t, store)
    P = dict(H=mat(c, "H", B, H, "in", t["H"]), T=mat(c, "T", B, H, "in", t["T"]), da2=vec(c, "da2", B, "in", t["da2"]),
             w2=vec(c, "w2", H, "in", t["w2"]), gw2=vec(c, "gw2", H, "out", None if store else t["gw2"]),
             gb2=vec(c, "gb2", 1, "out", None if store else t["gb2"]), dA1=mat(c, "dA1", B, H, "out"))
    of.dragan_head_bwd(P["H"].view, P["T"].view, flat(P["da2"]), flat(P["w2"]), flat(P["gw2"]), flat(P["gb2"]),
                       P["dA1"].view, B, store=store)
    finish(c, P)
    for n in ("gw2", "gb2"):
        check(c, n, flat(P[n]), r64[n], r32[n])
        check(c, n + " (2e-5)", flat(P[n]), r64[n], r32[n], tol=2e-5)
    check(c, "dA1", P["dA1"].view, r64["dA1"], r32["dA1"])


# ---- 4. placement cases for the other dual-path kernels ----------------------------------------------------------------
@params("made_bce")
def test_made_bce(c):
    """tests/test_gpu_made.py::test_bce_kernel_against_fp64's inputs, reference and bounds; dA bit-identical across
    placements (elementwise)."""
    import made_reference as R
    B, I = c.B, c.W
    g = kp.gen("made_bce", B, I)
    a = (torch.rand(B, I, generator=g) * 2 - 1) * 30.0
    a[0, :4] = torch.tensor([30.0, -30.0, 0.0, -0.0])
    x = torch.bernoulli(torch.full((B, I), 0.4), generator=g)
    scale = kp.inv_b(B)
    P = dict(logits=mat(c, "logits", B, I, "in", a), x=mat(c, "x", B, I, "in", x), part=vec(c, "part", B, "out"))
    if "dA" not in c.absent:
        P["dA"] = mat(c, "dA", B, I, "out")
    of.made_bce(P["logits"].view, P["x"].view, flat(P["part"]), B, scale, dA=P["dA"].view if "dA" in P else None)
    finish(c, P)
    rows = R.nll_rows(a.double(), x.double())
    check(c, "part", flat(P["part"]), rows, tol=R.LOSS_TOL, rows=True, scale=rows.clamp(min=1.0))
    if "dA" in P:
        check(c, "dA", P["dA"].view, (torch.sigmoid(a.double()) - x.double()) * scale, tol=R.GRAD_TOL)
        shared(c, (B, I), "dA", P["dA"].view)


@params("iwae_weights")
def test_iwae_weights(c):
    """tests/test_gpu_iwae.py::test_weights_vs_reference_on_realistic_inputs' inputs, references and allowances."""
    import test_gpu_iwae as ti
    B, k, I = c.B, 5, c.W
    g = kp.gen("iwae_weights", B, I)
    x = torch.bernoulli(torch.full((B, I), 0.3), generator=g)
    sharp = torch.linspace(0.15, 0.45, k).repeat(B)[:, None]
    xr = (x.repeat_interleave(k, 0) * (1 - 2 * sharp) + sharp + 0.05 * (torch.rand(B * k, I, generator=g) - 0.5))
    xr = xr.clamp(1e-3, 1 - 1e-3)
    lp = -120.0 + 3.0 * torch.randn(B * k, generator=g)
    ref, f32 = ti._weights_reference(x, xr, lp, B, k), ti._weights_fp32_cpu(x, xr, lp, B, k)
    P = dict(x=mat(c, "x", B, I, "in", x), xr=mat(c, "xr", B * k, I, "in", xr), lp=vec(c, "lp", B * k, "in", lp),
             negL=vec(c, "negL", B, "out"), ess=vec(c, "ess", B, "out"), wn=vec(c, "wn", B * k, "out"))
    if "dA" not in c.absent:
        P["dA"] = mat(c, "dA", B * k, I, "out")
    of.iwae_weights(P["x"].view, P["xr"].view, flat(P["lp"]), flat(P["negL"]), flat(P["ess"]), flat(P["wn"]), B, k,
                    dA=P["dA"].view if "dA" in P else None)
    finish(c, P)
    got = {"L": -flat(P["negL"]), "ess": flat(P["ess"]), "wn": P["wn"].view.reshape(B, k)}
    if "dA" in P:
        got["dA"] = P["dA"].view
    for n, base in (("L", ti.T_LOSS), ("ess", ti.T_LOSS), ("wn", ti.T_GRAD), ("dA", ti.T_GRAD)):
        if n in got:
            check(c, n, got[n], torch.from_numpy(np.asarray(ref[n])), tol=ti.fp32_allowance(base, ref[n], f32, n))


@params("bir_mmd")
def test_bir_mmd(c):
    """tests/test_gpu_fused_ops.py::test_bir_mmd_matches_fp64_autograd's reference and bounds (the sum of the partials
    within 1e-4 of max(10, |mmd|), dz within 2e-5 of max(1, |dz|)); prior through a ring slot, one with an odd stride."""
    B, Z, lam = c.B, c.W, 1000.0
    g = kp.gen("bir_mmd", B, Z)
    z = torch.randn(B, Z, generator=g) * 0.7 + 0.2
    x = torch.randn(B, Z, generator=g)
    P = dict(z=mat(c, "z", B, Z, "in", z), partial=vec(c, "partial", B, "out"))
    if c.flags.get("odd_stride"):
        # a ring of three [B, Z] slots B * Z + 1 floats apart: the slot's stride alone costs the 16-byte loads
        stride = B * Z + 1
        ring = torch.full((3 * stride,), float("nan")).view(torch.int32).fill_(NAN_BITS).view(torch.float32)
        ring[stride:stride + B * Z] = x.reshape(-1)
        P["prior"] = vec(c, "prior", 3 * stride, "in", ring)
        prior, slot = flat(P["prior"]), ops.slot(0, 0, 1, 3, stride)
    else:
        P["prior"] = vec(c, "prior", B * Z, "in", x, ring=RING if c.flags.get("ring") else 1)
        prior, slot = ring_arg(P["prior"])
    if "dz" not in c.absent:
        P["dz"] = mat(c, "dz", B, Z, "out")
    of.bir_mmd(P["z"].view, prior.reshape(-1), flat(P["partial"]), P["dz"].view if "dz" in P else None, B, Z, lam,
               prior_slot=slot)
    finish(c, P)
    zd, xd = z.double().requires_grad_(True), x.double()
    kern = lambda a, b: torch.exp(-((a.unsqueeze(1) - b.unsqueeze(0)) ** 2).mean(2) / Z)
    mmd = lam * (kern(xd, xd).sum() + kern(zd, zd).sum() - 2 * kern(xd, zd).sum())
    mmd.backward()
    got = lam * flat(P["partial"]).double().sum().reshape(1)
    check(c, "mmd", got, mmd.detach().reshape(1), tol=1e-4, scale=max(10.0, abs(mmd.item())))
    if "dz" in P:
        check(c, "dz", P["dz"].view, zd.grad, tol=2e-5, scale=max(1.0, zd.grad.abs().max().item()))


def _dataset(kernel, I, packed):
    g = kp.gen("dataset", I, packed)
    N = 40
    x = torch.bernoulli(torch.full((N, I), 0.3), generator=g) if packed else torch.rand(N, I, generator=g)
    return x, torch.randint(0, N, (3, 16), generator=g)


@params("gather_rows")
def test_gather_rows(c):
    """out = data[idx], bit for bit, through an index ring slot."""
    B, I = c.B, c.W
    x, idx = _dataset("gather", I, False)
    P = dict(data=mat(c, "data", x.shape[0], I, "in", x), out=mat(c, "out", B, I, "out"))
    ops.gather_rows(P["data"].view, idx.to(DEV).view(-1), P["out"].view, idx_slot=ops.slot(0, 0, 1, 3, B))
    finish(c, P)
    exact(c, "out", P["out"].view, x[idx[1]])


@params("gather_bits")
def test_gather_bits(c):
    """The bit-packed gather to fp32 rows equals the fp32 gather (tests/test_gpu_ops.py), bit for bit."""
    B, I = c.B, c.W
    x, idx = _dataset("gather", I, True)
    P = dict(out=mat(c, "out", B, I, "out"))
    ops.gather_rows(ops.PackedData(x.to(DEV)), idx.to(DEV).view(-1), P["out"].view, idx_slot=ops.slot(0, 0, 1, 3, B))
    finish(c, P)
    exact(c, "out", P["out"].view, x[idx[1]])


def _corrupted(c, got, x, noise, level, seed, step, row0=0):
    """Against the numpy rule by tests/test_gpu_dvae.py's close_rule, and bit-identical across placements."""
    import test_gpu_dvae as td
    td.close_rule(got, x.numpy(), noise, level, seed, step, row0)
    shared(c, (tuple(x.shape), noise), "corrupted", got)


@params("dvae_corrupt")
def test_dvae_corrupt(c):
    B, I, noise = c.B, c.W, c.flags["noise"]
    g = kp.gen("dvae_corrupt", B, I)
    x = torch.rand(B, I, generator=g)
    x[:, ::3] = (x[:, ::3] > 0.5).float()
    P = dict(x=mat(c, "x", B, I, "in", x), out=mat(c, "out", B, I, "out"))
    of.dvae_corrupt(P["x"].view, of.corrupt_args(noise, 0.5, 4, step=6, row0=2), out=P["out"].view)
    finish(c, P)
    _corrupted(c, P["out"].view, x, noise, 0.5, 4, 6, 2)


def _gather_corrupt(c, packed):
    B, I, noise = c.B, c.W, c.flags["noise"]
    x, idx = _dataset("gather", I, packed)
    P = dict(out=mat(c, "out", B, I, "out"), out_c=mat(c, "out_c", B, I, "out"))
    if packed:
        data = ops.PackedData(x.to(DEV))
    else:
        P["data"] = mat(c, "data", x.shape[0], I, "in", x)
        data = P["data"].view
    of.gather_rows_corrupt(data, idx.to(DEV).view(-1), P["out"].view, P["out_c"].view,
                           of.corrupt_args(noise, 0.25, 77, step=105), idx_slot=ops.slot(0, 0, 1, 3, B))
    finish(c, P)
    exact(c, "out", P["out"].view, x[idx[1]])
    _corrupted(c, P["out_c"].view, x[idx[1]], noise, 0.25, 77, 105)


@params("gather_corrupt")
def test_gather_corrupt(c):
    _gather_corrupt(c, False)


@params("gather_bits_corrupt")
def test_gather_bits_corrupt(c):
    _gather_corrupt(c, True)


# ---- 5. flat kernels past their grid caps, and the short ends --------------------------------------------------------
@params("adam")
def test_adam(c):
    """tests/test_gpu_ops.py::test_adam_vs_torch's reference (torch.optim.Adam on the CPU), gradient magnitudes and
    bounds, with p, g, m, v in guarded buffers; one misaligned pointer: refused on the host, not one float changes."""
    n, steps, lr, scaled = c.W, c.flags["steps"], 2e-4, c.flags["scaled"]
    g_ = kp.gen("adam", n)
    p = torch.randn(n, generator=g_)
    ref_p = p.clone().requires_grad_()
    k = 0.5 if scaled else 1.0                                       # BEGAN's plateau factor: a power of two
    opt = torch.optim.Adam([ref_p], lr=lr * k)
    z = torch.zeros(n)
    P = dict(p=vec(c, "p", n, "out", p), g=vec(c, "g", n, "in", z), m=vec(c, "m", n, "out", z), v=vec(c, "v", n, "out", z))
    sched = torch.from_numpy(ops.adam_schedule(lr, steps)).to(DEV)
    lr_scale = torch.tensor([k], device=DEV) if scaled else None
    if c.flags.get("refused"):
        P["g"].view.copy_(torch.randn(n, generator=g_).reshape(1, n))
        before = {nm: q.buf.view(torch.int32).clone() for nm, q in P.items()}
        with pytest.raises(GMError):
            ops.adam(flat(P["p"]), flat(P["g"]), flat(P["m"]), flat(P["v"]), sched, ops.slot(0, 0, 0, 0, 1), lr_scale=lr_scale)
        torch.cuda.synchronize()
        assert all(torch.equal(q.buf.view(torch.int32), before[nm]) for nm, q in P.items()), c.id
        return
    for s in range(steps):
        g = torch.randn(n, generator=g_) * (10.0 ** (s - 3))
        ref_p.grad = g.clone()
        opt.step()
        gp = vec(c, "g", n, "in", g)                                  # a fresh guarded gradient per step
        ops.adam(flat(P["p"]), flat(gp), flat(P["m"]), flat(P["v"]), sched, ops.slot(0, 0, s, 0, 1), lr_scale=lr_scale)
        finish(c, dict(P, g=gp))
        check(c, "p step %d" % s, flat(P["p"]), ref_p.data, tol=2e-7, scale=max(1.0, ref_p.data.abs().max().item()))
    st = opt.state[ref_p]
    check(c, "exp_avg", flat(P["m"]), st["exp_avg"], tol=1e-6)
    check(c, "exp_avg_sq", flat(P["v"]), st["exp_avg_sq"], tol=1e-6)


@params("gp_u")
def test_gp_u(c):
    """u = [s > 0][h > 0] w2, bit for bit, past the grid cap of 2048 workgroups."""
    B, H = c.B, c.W
    g = kp.gen("gp_u", B, H)
    s, h, w2 = torch.randn(B, generator=g), torch.randn(B, H, generator=g), torch.randn(H, generator=g)
    s[1::3] = 0.0
    h = h * (torch.rand(B, H, generator=g) > 0.2)
    P = dict(s=vec(c, "s", B, "in", s), h=mat(c, "h", B, H, "in", h), w2=vec(c, "w2", H, "in", w2), u=mat(c, "u", B, H, "out"))
    of.gp_u(flat(P["s"]), P["h"].view, flat(P["w2"]), P["u"].view)
    finish(c, P)
    exact(c, "u", P["u"].view, torch.where((s > 0)[:, None] & (h > 0), w2[None, :].expand(B, H), torch.zeros(B, H)))


@params("bir_reparam")
def test_bir_reparam(c):
    """z = mu + eps: one rounded add, bit for bit, past the grid cap of 256 workgroups; eps through a ring slot."""
    B, Z = c.B, c.W
    g = kp.gen("bir_reparam", B, Z)
    mu, eps = torch.randn(B, Z, generator=g), torch.randn(B, Z, generator=g)
    P = dict(mu=mat(c, "mu", B, Z, "in", mu), eps=vec(c, "eps", B * Z, "in", eps, ring=RING), z=mat(c, "z", B, Z, "out"))
    e, slot = ring_arg(P["eps"])
    of.bir_reparam(P["mu"].view, e.reshape(-1), P["z"].view, B, Z, eps_slot=slot)
    finish(c, P)
    exact(c, "z", P["z"].view, mu + eps)


@params("act_bwd")
def test_act_bwd(c):
    """dA = act'(Y) dY past the grid cap of 2048 workgroups, by close64 (two products at the most)."""
    n, act = c.W, c.flags["act"]
    g = kp.gen("act_bwd", n)
    dY, Y = torch.randn(n, generator=g), torch.rand(n, generator=g) - (0.3 if act == "relu" else 0.0)
    P = dict(dY=vec(c, "dY", n, "in", dY), Y=vec(c, "Y", n, "in", Y), dA=vec(c, "dA", n, "out"))
    ops.act_bwd(flat(P["dY"]), flat(P["Y"]), flat(P["dA"]), act)
    finish(c, P)
    check(c, "dA", flat(P["dA"]), kp.act_bwd_ref(dY, Y, act, torch.float64), kp.act_bwd_ref(dY, Y, act, torch.float32))


@params("copy_slot")
def test_copy_slot(c):
    """Slot 1 of one ring into slot 2 of another, past the grid cap of 1024 workgroups: bit for bit, no other slot."""
    n = c.W
    src = torch.randn(n, generator=kp.gen("copy_slot", n))
    P = dict(src=vec(c, "src", n, "in", src, ring=RING))
    P["dst"] = Placed(arr(c, "dst", 1, n, "out", RING), None, vector=True, pick=2, dev=DEV)
    (s, s_slot), (d, d_slot) = ring_arg(P["src"]), ring_arg(P["dst"])
    ops.copy_slot(s.reshape(-1), d.reshape(-1), n, src_slot=s_slot, dst_slot=d_slot)
    finish(c, P)
    exact(c, "dst", flat(P["dst"]), src)


@params("sum_finalize")
def test_sum_finalize(c):
    """out[1] = scale * sum(partial[:n]) against an fp64 sum by close64 (the fp32 yardstick: torch's own sum); the float
    behind the last partial is the NaN pattern, which only an unclamped load would read; out[0] and out[2] are guards."""
    n, form, scale = c.W, c.flags["form"], 0.25
    vals = kp.sum_inputs(n)
    P = dict(partial=vec(c, "partial", n, "in", vals), out=vec(c, "out", 1, "out"))
    out, slot = slot1(P["out"])
    tick = torch.zeros(1, dtype=torch.int64, device=DEV)
    if form == "fin2":
        vb = kp.sum_inputs(kp.SUM_N[(kp.SUM_N.index(n) + 4) % len(kp.SUM_N)])
        P.update(pb=vec(c, "pb", vb.numel(), "in", vb), out_b=vec(c, "out_b", 1, "out"))
        ob, slot_b = slot1(P["out_b"])
        of.sum_finalize2(flat(P["partial"]), n, out, slot, flat(P["pb"]), vb.numel(), ob, slot_b, scale_a=scale,
                         scale_b=2.0, tick=tick)
    else:
        of.sum_finalize(flat(P["partial"]), n, out, scale=scale, out_slot=slot, tick=tick if form == "tick" else None)
    finish(c, P)
    assert int(tick) == (0 if form == "plain" else 1)
    check(c, "sum", flat(P["out"]), (vals.double().sum() * scale).reshape(1), (vals.sum() * scale).reshape(1))
    if form == "fin2":
        check(c, "sum b", flat(P["out_b"]), (vb.double().sum() * 2.0).reshape(1), (vb.sum() * 2.0).reshape(1))


# ---- 6. leading dimensions for the rest of gm_fused.hip --------------------------------------------------------------
def _ld_case(c):
    t = kp.ld_inputs(c.kernel, c.B, c.W)
    return t, kp.ref_ld(c.kernel, t, torch.float64), kp.ref_ld(c.kernel, t, torch.float32)


@params("interp")
def test_interp(c):
    """test_interp's 2e-6; every matrix with a leading dimension of its own, eps through ring slot 1."""
    (t, r64, r32), B, I = _ld_case(c), c.B, c.W
    P = dict(eps=vec(c, "eps", B, "in", t["eps"], ring=RING), x=mat(c, "x", B, I, "in", t["x"]),
             g=mat(c, "g", B, I, "in", t["g"]), out=mat(c, "out", B, I, "out"))
    e, slot = ring_arg(P["eps"])
    of.interp(e.reshape(-1), slot, P["x"].view, P["g"].view, P["out"].view)
    finish(c, P)
    check(c, "out", P["out"].view, r64["out"], r32["out"], tol=2e-6)


@params("sqerr_sigmoid_bwd")
def test_sqerr_sigmoid_bwd(c):
    """test_sqerr_sigmoid_backward's 5e-6 for dA and for the row partials, those per row."""
    (t, r64, r32), B, I = _ld_case(c), c.B, c.W
    P = dict(x=mat(c, "x", B, I, "in", t["x"]), xr=mat(c, "xr", B, I, "in", t["xr"]), dA=mat(c, "dA", B, I, "out"),
             partial=vec(c, "partial", B, "out"))
    of.sqerr_sigmoid_bwd(P["x"].view, P["xr"].view, P["dA"].view, flat(P["partial"]), B)
    finish(c, P)
    check(c, "dA", P["dA"].view, r64["dA"], r32["dA"], tol=5e-6)
    check(c, "partial", flat(P["partial"]), r64["partial"], r32["partial"], tol=5e-6, rows=True)


def _reparam(c, wide):
    (t, r64, r32), B, Z = _ld_case(c), c.B, c.W
    P = dict(ml=mat(c, "ml", B, 2 * Z, "in", t["ml"]), eps=vec(c, "eps", B * Z, "in", t["eps"], ring=RING),
             z=mat(c, "z", B, Z, "out"))
    e, slot = ring_arg(P["eps"])
    if wide:
        nb = (B * Z + 255) // 256
        P["kl"] = vec(c, "kl", nb, "out")
        assert of.vae_reparam_wide(P["ml"].view, e.reshape(-1), P["z"].view, flat(P["kl"]), B, Z, eps_slot=slot) == nb
    else:
        P["kl"] = vec(c, "kl", 1, "out")
        out, kl_slot = slot1(P["kl"])
        of.vae_reparam(P["ml"].view, e.reshape(-1), P["z"].view, out, B, Z, eps_slot=slot, kl_slot=kl_slot)
    finish(c, P)
    check(c, "z", P["z"].view, r64["z"], r32["z"], tol=2e-6)
    shared(c, (B, Z), "z", P["z"].view, group="vae_reparam*")        # the two forms: the same bits
    check(c, "kl", flat(P["kl"]).double().sum().reshape(1), r64["kl"], tol=1e-5, scale=max(1.0, abs(float(r64["kl"]))))


@params("vae_reparam")
def test_vae_reparam(c):
    """test_vae_reparam_forward_and_backward's bounds: z 2e-6, kl 1e-5 of max(1, |kl|); only its own kl slot."""
    _reparam(c, False)


@params("vae_reparam_wide")
def test_vae_reparam_wide(c):
    """The wide form: z bit-identical to vae_reparam's (test_vae_reparam_wide_and_dual_finalize), the partials add up to kl."""
    _reparam(c, True)


@params("vae_reparam_bwd")
def test_vae_reparam_bwd(c):
    """test_vae_reparam_forward_and_backward's 5e-6; ml, dz and dml each with a leading dimension of its own."""
    (t, r64, r32), B, Z = _ld_case(c), c.B, c.W
    P = dict(ml=mat(c, "ml", B, 2 * Z, "in", t["ml"]), eps=vec(c, "eps", B * Z, "in", t["eps"], ring=RING),
             dz=mat(c, "dz", B, Z, "in", t["dz"]), dml=mat(c, "dml", B, 2 * Z, "out"))
    e, slot = ring_arg(P["eps"])
    of.vae_reparam_bwd(P["ml"].view, e.reshape(-1), P["dz"].view, P["dml"].view, B, Z, eps_slot=slot)
    finish(c, P)
    check(c, "dml", P["dml"].view, r64["dml"], r32["dml"], tol=5e-6)


@params("l1_rows")
def test_l1_rows(c):
    """test_l1_rows_and_dx_add's 1e-6 for the row sums (per row) and the gradient; 2 B rows, the second half scaled by -K."""
    (t, r64, r32), B, I = _ld_case(c), c.B, c.W
    P = dict(Y=mat(c, "Y", 2 * B, I, "in", t["Y"]), X=mat(c, "X", 2 * B, I, "in", t["X"]), K=vec(c, "K", 1, "in", t["K"]),
             dY=mat(c, "dY", 2 * B, I, "out"), rowsum=vec(c, "rowsum", 2 * B, "out"))
    of.l1_rows(P["Y"].view, P["X"].view, 2 * B, B, flat(P["K"]), P["dY"].view, flat(P["rowsum"]))
    finish(c, P)
    check(c, "rowsum", flat(P["rowsum"]), r64["rowsum"], r32["rowsum"], tol=1e-6, rows=True)
    check(c, "dY", P["dY"].view, r64["dY"], r32["dY"], tol=1e-6)


@params("dragan_xhat")
def test_dragan_xhat(c):
    """test_dragan_xhat's 2e-6; delta and U through ring slot 1."""
    (t, r64, r32), B, I = _ld_case(c), c.B, c.W
    P = dict(x=mat(c, "x", B, I, "in", t["x"]), delta=vec(c, "delta", B, "in", t["delta"], ring=RING),
             U=vec(c, "U", B * I, "in", t["U"], ring=RING), std=vec(c, "std", 1, "in", t["std"]), out=mat(c, "out", B, I, "out"))
    (d, d_slot), (u, u_slot) = ring_arg(P["delta"]), ring_arg(P["U"])
    of.dragan_xhat(P["x"].view, d.reshape(-1), d_slot, u.reshape(-1), u_slot, flat(P["std"]), P["out"].view, B)
    finish(c, P)
    check(c, "out", P["out"].view, r64["out"], r32["out"], tol=2e-6)


@params("dragan_rows")
def test_dragan_rows(c):
    """pen within test_dragan_penalty_chain_vs_autograd's 1e-5, per row; dv and da2, which that test only sees through the
    GEMMs behind them, within the 2e-5 it holds those to, per row."""
    (t, r64, r32), B, I = _ld_case(c), c.B, c.W
    P = dict(s=vec(c, "s", B, "in", t["s"]), V=mat(c, "V", B, I, "in", t["V"]), dv=mat(c, "dv", B, I, "out"),
             da2=vec(c, "da2", B, "out"), pen=vec(c, "pen", B, "out"))
    of.dragan_rows(flat(P["s"]), P["V"].view, P["dv"].view, flat(P["da2"]), flat(P["pen"]), LAM, kp.inv_b(B), B)
    finish(c, P)
    check(c, "pen", flat(P["pen"]), r64["pen"], r32["pen"], tol=1e-5, rows=True)
    check(c, "dv", P["dv"].view, r64["dv"], r32["dv"], tol=2e-5, rows=True)
    check(c, "da2", flat(P["da2"]), r64["da2"], r32["da2"], tol=2e-5, rows=True)
    if B > 1:
        assert float(P["dv"].view[1].abs().max()) == 0.0 and float(flat(P["pen"])[1]) == 1.0   # the zero-norm row


# ---- the record ------------------------------------------------------------------------------------------------------------
def test_worst_ratio_per_kernel_report():
    """The rows of profiles/kernel_path_errors.md (run the whole module with -s): per kernel the cases run, the
    comparisons made and the largest e_hip / bound with the case it came from."""
    print()
    print("| kernel | cases | comparisons | worst e_hip / bound | e_hip | e_cpu | worst at |")
    print("|---|---|---|---|---|---|---|")
    for k in kp.KERNELS:
        st = STATS.get(k)
        if st:
            print("| %s | %d | %d | %.3f | %.3e | %.3e | %s |" % (k, len(st["cases"]), st["n"], st["ratio"], st["e_hip"],
                                                                st["e_cpu"], st["at"]))
    for k, st in STATS.items():
        assert st["ratio"] <= 1.0, (k, st)
