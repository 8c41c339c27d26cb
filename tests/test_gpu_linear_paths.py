"""Every launch path of the linear layers (tests/linear_path_cases.py) on the GPU, inside guarded buffers.

Each array of a call -- operands and outputs -- lives inside a larger backing buffer filled with one quiet-NaN bit
pattern: at least 64 rows' worth of floats (64 floats for vectors) before and after it, the pad columns of an `ld >
width` array, the other slots of a ring, and the output rectangle itself (an element the kernel does not write stays
NaN; with `accumulate`, and for Adam's parameters and moments, it holds the base values).  After the call

1. every float outside the output rectangles, of every array, must be bit-identical to what it was (int32 view);
2. the output is compared with an fp64 evaluation of the same expression by close64 (tests/test_gpu_ops.py: HIP error
   <= 2 x the fp32 CPU result's error against fp64 + 2^-23 of the output's scale), dW as test_dw_against_fp64 does; db,
   which ATen sums pairwise, keeps test_linear_bwd_dw's bound; the Adam epilogue's p / m / v keep test_adam_vs_torch's,
   from the gradient the launch itself wrote.

A value read from outside an operand's rectangle is NaN, so if it reaches the arithmetic the output fails step 2: the
kernels' clamped loads stay inside the rectangle and zero by select.  Before the call the case's plan is asked again
with the real pointers: the test runs the kernel its name says."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import guarded  # noqa: E402
import linear_path_cases as lp  # noqa: E402
from generative_models_amd import ops  # noqa: E402

DEV = "cuda:0"
NAN_BITS = guarded.NAN_BITS              # a quiet NaN no arithmetic produces
VECTORS = ("bias", "db", "pb", "mb", "vb", "sched")
WORST = {"ratio": 0.0, "case": None}     # the largest e_hip / bound of the session (printed with every case)


# ---- inputs and references: once per shape / expression, shared by the cases that differ in placement only ------------
@functools.lru_cache(maxsize=4)
def inputs(op, M, K, N):
    g = torch.Generator().manual_seed({"fwd": 1, "dx": 2, "dw": 3}[op] + 10 * N + 100003 * K + 1000000007 * M)
    r = lambda *s: torch.randn(*s, generator=g)
    if op == "fwd":
        return dict(X=r(M, K), W=r(N, K) / K ** 0.5, bias=r(N))
    if op == "dx":
        return dict(dA=r(M, N), W=r(N, K) / N ** 0.5, below=torch.rand(M, K, generator=g), add=r(M, K))
    return dict(dA=r(M, N), X=r(M, K), dW=r(N, K), db=r(N), pW=r(N, K) * 0.1, mW=r(N, K).abs() * 0.01,
                vW=r(N, K).abs() * 0.001, pb=r(N) * 0.1, mb=r(N).abs() * 0.01, vb=r(N).abs() * 0.001,
                sched=torch.from_numpy(ops.adam_schedule(lp.ADAM_LR, 2, lp.ADAM_BETAS)).reshape(-1))


def act(y, a):
    return F.relu(y) if a == "relu" else torch.sigmoid(y) if a == "sigmoid" else y


def evaluate(op, t, flags, f64):
    """The call's expression on the CPU, in fp64 or fp32."""
    c = (lambda x: x.double()) if f64 else (lambda x: x)
    if op == "fwd":
        return dict(Y=act(F.linear(c(t["X"]), c(t["W"]), c(t["bias"]) if flags.get("bias", True) else None),
                          flags.get("act", "relu")))
    if op == "dx":
        r = c(t["dA"]) @ c(t["W"])
        if flags.get("add"):
            r = r + lp.ADD_SCALE * c(t["add"])
        below = c(t["below"]) - (0.5 if flags.get("epi") == "relu" else 0.0)
        if flags.get("epi") == "relu":
            r = r * (below > 0)
        elif flags.get("epi") == "sigmoid":
            r = r * (below * (1 - below))
        return dict(dX=r)
    dW, db = c(t["dA"]).t() @ c(t["X"]), c(t["dA"]).sum(0)
    if flags.get("accumulate"):
        dW, db = c(t["dW"]) + dW, c(t["db"]) + db
    return dict(dW=dW, db=db)


@functools.lru_cache(maxsize=4)
def reference(op, M, K, N, flag_items):
    t, flags = inputs(op, M, K, N), dict(flag_items)
    return evaluate(op, t, flags, True), evaluate(op, t, flags, False)


def expression_flags(c):
    """The flags that change the values (placement, slots and the optimizer do not)."""
    return tuple(sorted((k, v) for k, v in c.flags.items() if k in ("bias", "act", "epi", "add", "accumulate")))


# ---- guarded placement (tests/guarded.py) ------------------------------------------------------------------------------
def Placed(a, values):
    return guarded.Placed(a, values, vector=a.name in VECTORS, pick=lp.RING_PICK, dev=DEV)


def cpu_below(c, t):
    return t["below"] - (0.5 if c.flags.get("epi") == "relu" else 0.0)


@pytest.mark.parametrize("c", lp.CASES, ids=[c.id for c in lp.CASES])
def test_linear_path(c):
    t = inputs(c.op, c.M, c.K, c.N)
    ref64, ref32 = reference(c.op, c.M, c.K, c.N, expression_flags(c))
    placed = {}
    for name, a in lp.arrays(c).items():
        if a.role == "in":
            values = cpu_below(c, t) if name == "below" else t[name]
        elif name in ("pW", "mW", "vW", "pb", "mb", "vb"):
            values = t[name]                                             # Adam's parameters and moments
        else:
            values = t[name] if c.flags.get("accumulate") else None      # the rectangle stays NaN
        placed[name] = Placed(a, values)
    mode, d = lp.descriptor(c, {n: p.ptr for n, p in placed.items()})
    plan = ops.linear_plan(mode, d)
    assert lp.plan_key(plan) == c.plan and plan["launches"] == 1, (c.id, plan)
    if mode == "fwd":
        ops._fwd_ex(d, None)
    elif mode == "dx":
        ops._dx_ex(d, None)
    else:
        ops._dw_ex(d, None, None, None)
    torch.cuda.synchronize()

    touched = [n for n, p in placed.items() if not p.untouched_outside()]
    assert not touched, "%s: floats outside the output rectangle changed in %s" % (c.id, touched)

    out = "Y" if mode == "fwd" else "dX" if mode == "dx" else "dW"
    got = placed[out].view
    e_hip, e_cpu, bound, scale = lp.errors64(got, ref64[out], ref32[out])
    if e_hip / bound > WORST["ratio"]:
        WORST.update(ratio=e_hip / bound, case=c.id)
    print("%s: e_hip %.3e e_cpu %.3e bound %.3e ratio %.3f (worst so far %.3f at %s)"
          % (c.id, e_hip, e_cpu, bound, e_hip / bound, WORST["ratio"], WORST["case"]))
    lp.close64(got, ref64[out], ref32[out], c.id + " " + out)
    if "db" in placed:
        lp.close(placed["db"].view.reshape(-1), ref64["db"], 2e-6 * max(1, c.M ** 0.5 / 4), c.id + " db")
    if c.flags.get("adam"):
        # the optimizer step of the epilogue, from the gradient it was given (torch's _single_tensor_adam in fp64)
        step_size, bc2_sqrt = (float(x) for x in t["sched"][2:4])
        b1, b2 = lp.ADAM_BETAS
        for g_, p_, m_, v_ in (("dW", "pW", "mW", "vW"), ("db", "pb", "mb", "vb")):
            g = placed[g_].view.cpu().double().reshape(t[p_].shape)
            m = t[m_].double() + (1 - b1) * (g - t[m_].double())
            v = t[v_].double() * b2 + (1 - b2) * g * g
            p = t[p_].double() - step_size * m / (v.sqrt() / bc2_sqrt + lp.ADAM_EPS)
            err = (placed[p_].view.cpu().double().reshape(p.shape) - p).abs().max().item()
            assert err <= 2e-7 * max(1.0, p.abs().max().item()), (c.id, p_, err)
            lp.close(placed[m_].view.reshape(m.shape), m, 1e-6, c.id + " " + m_)
            lp.close(placed[v_].view.reshape(v.shape), v, 1e-6, c.id + " " + v_)
