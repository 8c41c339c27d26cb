"""The linear layers' launch paths as a table of cases (tests/test_linear_plan_cpu.py pins the table against the
library's own dispatch, tests/test_gpu_linear_paths.py runs every case on the GPU inside guarded buffers).

The host dispatch of csrc/gm_gemm.hip picks one of some sixty kernel instantiations per call, from shape thresholds
(tile counts, reduction length, M >= 1024, K <= 32, 768 reduction rows), 16-byte alignment of every operand and the
leading dimensions.  A case names a layer shape, where each array sits relative to a 16-byte boundary, its leading
dimension, the flags of the call -- and the PLAN the call is meant to reach, as the string plan_key() makes of
ops.linear_plan's answer.  The shapes are the smallest that reach each path; the query is the authority: when a
threshold moves, a case moves, and the CPU test says which.

Layer shapes are (M, K, N): M rows, K inputs, N outputs, for all three ops (forward Y[M,N] = act(X[M,K] W[N,K]^T + b),
input gradient dX[M,K] = (dA[M,N] W + add) act'(below), weight gradient dW[N,K] = dA[M,N]^T X[M,K], db = colsum dA).
"""
from collections import OrderedDict, namedtuple

from generative_models_amd import _lib



# ---- the comparison criteria (shared with tests/test_gpu_ops.py) ------------------------------------------------------
def close(got, ref, tol=1e-5, what="", atol=0.0):
    got = got.detach().cpu().double()
    ref = ref.detach().cpu().double()
    scale = max(ref.abs().max().item(), 1e-30)
    err = max((got - ref).abs().max().item() - atol, 0.0) / scale
    assert err <= tol, "%s: max err %.3e (scaled) > %.1e; ref scale %.3e" % (what, err, tol, scale)


def errors64(got, ref64, ref32):
    """(e_hip, e_cpu, bound, scale) of close64."""
    got, ref32, ref64 = got.detach().cpu().double(), ref32.detach().cpu().double(), ref64.detach().cpu().double()
    scale = max(ref64.abs().max().item(), 1e-30)
    e_hip = (got - ref64).abs().max().item() / scale
    e_cpu = (ref32 - ref64).abs().max().item() / scale
    return e_hip, e_cpu, 2.0 * e_cpu + 2.0 ** -23, scale


def close64(got, ref64, ref32, what=""):
    """The HIP result against an fp64 evaluation of the same expression, bounded by TWICE the error the fp32 CPU
    result (MKL / ATen, its own summation order) has against that fp64 value, plus one fp32 ulp of the output's scale
    (exact cases: M = 1, identity operands).  An MKL-vs-HIP comparison with a sqrt(K) allowance cannot tell which of
    the two is off; this can."""
    e_hip, e_cpu, bound, scale = errors64(got, ref64, ref32)
    assert e_hip <= bound, "%s: HIP err %.3e (scaled) > 2 x CPU fp32 err %.3e + 1 ulp; scale %.3e" % (what, e_hip, e_cpu, scale)
    return e_hip, e_cpu, bound


Case = namedtuple("Case", "id op M K N off ld flags plan")
# off: the arrays that start one float past a 16-byte boundary; ld: array -> floats added to its width;
# flags: bias / act (fwd), epi / add (dx), db / accumulate / adam (dw), slot (ring slot on X: fwd, dw)
Array = namedtuple("Array", "name rows width ld off role ring")      # role: "in" | "out"; ring: slots of a ring (1: none)

RING, RING_PICK = 3, 1          # a ring slot on X: three slots, the call reads the second
# guards of every case, before and after each array: rows' worth of floats for a matrix (of its leading dimension), floats
# for a vector -- more than the tallest tile (64 rows) and the widest (64 columns), so an over-write by a whole tile shows
GUARD_ROWS, GUARD_FLOATS = 64, 64


def pad4(n):
    return (-n) % 4


# ---- plans as strings -------------------------------------------------------------------------------------------------
def lds(mode, cfg, ns, epi):
    return "%s lds cfg%d ns%d epi%d" % (mode, cfg, ns, epi)


def k32(epi, slot):
    return "fwd k32 epi%d slot%d" % (epi, slot)


def split(mode, tile, v, x, epi, dma=0, slot=0):
    return "%s split %s v%d x%d epi%d dma%d slot%d" % (mode, tile, v, x, epi, dma, slot)


def plan_key(p):
    """ops.linear_plan's dict as the string a case carries."""
    if p["family"] == "lds":
        return lds(p["mode"], p["lds_cfg"], p["lds_stages"], p["vec_epi"])
    if p["family"] == "k32":
        return k32(p["vec_epi"], p["slots"])
    if p["family"] == "split":
        return split(p["mode"], "%dx%d" % (16 * p["mi"], 16 * p["ni"]), p["vec"], p["xv"], p["vec_epi"], p["dma"], p["slots"])
    return "%s %s" % (p["mode"], p["family"])


# ---- where a case's arrays live ---------------------------------------------------------------------------------------
def arrays(c):
    """Every array of the call, in a fixed order."""
    f, M, K, N = c.flags, c.M, c.K, c.N

    def arr(name, rows, width, role, ring=1):
        return Array(name, rows, width, width + c.ld.get(name, 0), 1 if name in c.off else 0, role, ring)
    ring = RING if f.get("slot") else 1
    if c.op == "fwd":
        out = [arr("X", M, K, "in", ring), arr("W", N, K, "in")]
        if f.get("bias", True):
            out.append(arr("bias", 1, N, "in"))
        out.append(arr("Y", M, N, "out"))
    elif c.op == "dx":
        out = [arr("dA", M, N, "in"), arr("W", N, K, "in")]
        if f.get("epi", "id") != "id":
            out.append(arr("below", M, K, "in"))
        if f.get("add"):
            out.append(arr("add", M, K, "in"))
        out.append(arr("dX", M, K, "out"))
    else:
        out = [arr("dA", M, N, "in"), arr("X", M, K, "in", ring), arr("dW", N, K, "out")]
        if f.get("db", True):
            out.append(arr("db", 1, N, "out"))
        if f.get("adam"):
            out += [arr(n, N, K, "out") for n in ("pW", "mW", "vW")] + [arr(n, 1, N, "out") for n in ("pb", "mb", "vb")]
            out.append(arr("sched", 1, 4, "in"))
    for a in out:
        assert a.name in ("X", "Y", "dA", "dX", "below", "add") or a.ld == a.width, "%s has no leading dimension" % a.name
    return OrderedDict((a.name, a) for a in out)


def ring_stride(a):
    """Floats between two slots of X's ring: whole float4s, so that the slot alone never costs the 16-byte paths."""
    return a.rows * a.ld + pad4(a.rows * a.ld)


def descriptor(c, ptr):
    """(mode, descriptor) of the case's call; ptr: array name -> address of its first element (of the ring's first slot).
    The CPU test passes placeholders with the alignment of the real ones, the GPU test the real ones."""
    a, f = arrays(c), c.flags
    slot = _lib.slot(add=RING_PICK, ring=RING, stride=ring_stride(a["X"])) if f.get("slot") else _lib.NO_SLOT
    if c.op == "fwd":
        d = _lib.FwdArgs(X=ptr["X"], ldx=a["X"].ld, x_slot=slot, W=ptr["W"], bias=ptr.get("bias"), Y=ptr["Y"],
                         ldy=a["Y"].ld, M=c.M, K=c.K, N=c.N, act=_lib.ACT[f.get("act", "relu")])
    elif c.op == "dx":
        d = _lib.DxArgs(dA=ptr["dA"], lda=a["dA"].ld, W=ptr["W"], dX=ptr["dX"], ldx=a["dX"].ld, M=c.M, K=c.K, N=c.N,
                        epi=_lib.ACT[f.get("epi", "id")])
        if "below" in a:
            d.below, d.ld_below = ptr["below"], a["below"].ld
        if "add" in a:
            d.add, d.ldadd, d.add_scale = ptr["add"], a["add"].ld, ADD_SCALE
    else:
        d = _lib.DwAdamArgs(dA=ptr["dA"], lda=a["dA"].ld, X=ptr["X"], ldx=a["X"].ld, x_slot=slot, dW=ptr["dW"],
                            db=ptr.get("db"), M=c.M, K=c.K, N=c.N, accumulate=1 if f.get("accumulate") else 0)
        if f.get("adam"):
            for n in ("pW", "mW", "vW", "pb", "mb", "vb", "sched"):
                setattr(d, n, ptr[n])
            d.sched_slot = _lib.slot(add=1, stride=2)         # the schedule's second entry
            d.beta1, d.beta2, d.eps = ADAM_BETAS[0], ADAM_BETAS[1], ADAM_EPS
    return c.op, d


ADD_SCALE = 0.75
ADAM_BETAS, ADAM_EPS, ADAM_LR = (0.9, 0.999), 1e-8, 1e-3


def placeholder_pointers(c):
    """Distinct addresses with each array's offset from a 16-byte boundary."""
    return {n: (1 << 20) * (i + 1) + 4 * a.off for i, (n, a) in enumerate(arrays(c).items())}


# ---- the table --------------------------------------------------------------------------------------------------------
CASES = []


def add(op, M, K, N, plan, tag, off=(), ld=None, **flags):
    CASES.append(Case("%s-%dx%dx%d-%s" % (op, M, K, N, tag), op, M, K, N, tuple(off), dict(ld or {}), flags, plan))


def _fwd_split():
    # (tile, M, K, N, slot): 16x32 by <= 128 tiles; 32x32 by M <= 16 and by 129 .. 256 tiles; 32x64 / 64x32 by > 256
    # tiles over >= 497 of reduction; 48x32 where that covers a 64x32 launch in <= 256 workgroups
    bases = [("16x32", 33, 68, 35, (0, 1)), ("32x32", 7, 36, 45, (1,)), ("32x32", 160, 36, 900, (0,)),
             ("32x64", 497, 500, 590, (0, 1)), ("64x32", 1001, 500, 390, (0, 1)), ("48x32", 1001, 500, 300, (0, 1))]
    for tile, M, K, N, slots in bases:
        for s in slots:
            t = "-slot" if s else ""
            ypad = {"Y": pad4(N)}
            # 1. aligned, rows of Y in whole float4s
            add("fwd", M, K, N, split("fwd", tile, 1, 0, 1, 0, s), "aligned" + t, ld=ypad, slot=s)
            # ... and the float4 epilogue lost to Y alone: ragged rows (N % 4 != 0) or Y one float off
            if N % 4:
                add("fwd", M, K, N, split("fwd", tile, 1, 0, 0, 0, s), "yragged" + t, slot=s, act="sigmoid")
            else:
                add("fwd", M, K, N, split("fwd", tile, 1, 0, 0, 0, s), "yoff" + t, off=("Y",), slot=s, act="sigmoid")
            # 2. every array one float off
            add("fwd", M, K, N, split("fwd", tile, 0, 0, 0, 0, s), "alloff" + t, off=("X", "W", "bias", "Y"), ld=ypad, slot=s,
                act="id")
            # 3. K % 4 != 0 under an aligned, whole-float4 Y
            add("fwd", M, K + 1, N, split("fwd", tile, 0, 0, 1, 0, s), "kodd" + t, ld=ypad, slot=s, bias=(s == 0))
    # the scalar path over M >= 1024 rows, which the LDS kernel refuses
    add("fwd", 1025, 501, 300, split("fwd", "48x32", 0, 0, 1), "kodd-manyrows")
    # leading dimensions: + 4 keeps the 16-byte paths, + 3 drops them
    add("fwd", 33, 68, 36, split("fwd", "16x32", 1, 0, 1), "ld+4", ld={"X": 4, "Y": 4})
    add("fwd", 33, 68, 36, split("fwd", "16x32", 0, 0, 0), "ld+3", ld={"X": 3, "Y": 3})
    add("fwd", 497, 500, 592, split("fwd", "32x64", 1, 0, 1), "ld+4", ld={"X": 4, "Y": 4})
    add("fwd", 497, 500, 592, split("fwd", "32x64", 0, 0, 0), "ld+3", ld={"X": 3, "Y": 3})


def _fwd_k32():
    i = 0
    for K in (4, 20, 32):
        for M in (1, 37):
            for N in (1, 50, 65):
                s, e = i & 1, (i >> 1) & 1               # ring slot on X; whole-float4 rows of Y
                add("fwd", M, K, N, k32(e, s), "k32" + ("-slot" if s else "") + ("-ypad" if e else ""),
                    ld={"Y": pad4(N)} if e else None, slot=s, act=("id", "sigmoid", "relu")[i % 3])
                i += 1
    add("fwd", 37, 20, 52, k32(1, 0), "k32-ld+4", ld={"X": 4, "Y": 4})
    add("fwd", 37, 20, 52, split("fwd", "16x32", 0, 0, 0), "k32-ld+3", ld={"X": 3, "Y": 3})      # no 16-byte rows: not k32


# reduction lengths of the LDS kernel -> stages of its instantiation (0: the runtime loop).  64: two stages, the
# prologue's look-ahead loads all past the end; 96: no tail; 385 .. 416 -> 13 stages, 769 .. 800 -> 25, both ends each
LDS_RED = [(64, 0), (68, 0), (96, 0), (100, 0), (388, 13), (416, 13), (772, 25), (800, 25)]


def _fwd_lds():
    for cfg, N in ((2, 33), (1, 449)):                  # 32x64 tiles for the narrow output, 64x64 for the wide one
        for i, (K, ns) in enumerate(LDS_RED):
            e = (i + (i >> 2)) & 1                      # both epilogues on every instantiation
            add("fwd", 1025, K, N, lds("fwd", cfg, ns, e), "lds" + ("-ypad" if e else "-yragged"),
                ld={"Y": pad4(N)} if e else None, act=("relu", "sigmoid")[i & 1])
    add("fwd", 1025, 100, 64, lds("fwd", 2, 0, 1), "lds-n64")
    add("fwd", 1025, 100, 64, lds("fwd", 2, 0, 0), "lds-yoff", off=("Y",))
    add("fwd", 1025, 68, 452, lds("fwd", 1, 0, 0), "lds-biasoff", off=("bias",))
    add("fwd", 1025, 68, 452, lds("fwd", 1, 0, 1), "lds-ld+4", ld={"X": 4, "Y": 4})
    add("fwd", 1025, 68, 452, lds("fwd", 1, 0, 0), "lds-ldy+3", ld={"X": 4, "Y": 3})
    add("fwd", 1025, 68, 452, split("fwd", "32x32", 0, 0, 0), "lds-ld+3", ld={"X": 3, "Y": 3})     # ldx % 4: not LDS


def _dx_lds():
    for cfg, K in ((2, 36), (1, 452)):
        for i, (N, ns) in enumerate(LDS_RED):
            e = (i + (i >> 2)) & 1
            epi = ("id", "relu", "sigmoid")[i % 3]
            # the float4 epilogue lost to dX (one float off) or, with an activation gradient, to `below`
            off = () if e else (("below",) if epi != "id" and i & 1 else ("dX",))
            add("dx", 1025, K, N, lds("dx", cfg, ns, e), "lds-" + epi + ("" if e else "-" + off[0] + "off"), off=off,
                epi=epi, add=(i == 3 or i == 6))
    add("dx", 1025, 36, 68, lds("dx", 2, 0, 1), "lds-ld+4", ld={"dA": 4, "dX": 4, "below": 4, "add": 4}, epi="relu", add=True)
    add("dx", 1025, 36, 68, lds("dx", 2, 0, 0), "lds-ldx+3", ld={"dA": 4, "dX": 3, "below": 4, "add": 4}, epi="relu", add=True)
    add("dx", 1025, 36, 68, lds("dx", 2, 0, 0), "lds-ldbelow+3", ld={"below": 3}, epi="sigmoid")
    add("dx", 1025, 36, 68, lds("dx", 2, 0, 0), "lds-ldadd+3", ld={"add": 3}, add=True)
    add("dx", 1025, 36, 68, split("dx", "16x32", 0, 1, 1), "lds-lda+3", ld={"dA": 3}, epi="relu")   # lda % 4: not LDS


def _dx_split():
    # (tile, M, K, N): GEMM dims M x K over a reduction of N; no 48-wide tiles for the input gradient
    bases = [("16x32", 33, 68, 36), ("32x32", 7, 36, 44), ("32x64", 497, 592, 500), ("64x32", 1001, 300, 500)]
    for j, (tile, M, K, N) in enumerate(bases):
        for v in (1, 0):
            for x in (1, 0):
                for e in (1, 0):
                    i = 4 * v + 2 * x + e + j
                    epi = ("relu", "sigmoid", "id")[i % 3]
                    off = []
                    n, k, ld = N, K, {}
                    if not v:                           # dA: one float off, or rows of N % 4 != 0
                        if i & 1:
                            off.append("dA")
                        else:
                            n = N + 1
                    if not x:                           # W: one float off, or rows of K % 4 != 0 (dX padded to whole float4s)
                        if i & 2:
                            off.append("W")
                        else:
                            k = K + 1
                            ld = {"dX": pad4(k), "below": pad4(k), "add": pad4(k)}
                    if not e:
                        if k != K and i & 4:
                            ld = {}                     # ragged rows of dX
                        else:
                            off.append("below" if epi != "id" and i & 1 else "dX")
                    add("dx", M, k, n, split("dx", tile, v, x, e), "v%dx%de%d-%s" % (v, x, e, epi), off=off, ld=ld, epi=epi,
                        add=(i % 4 == 1))
    # >= 1024 rows on the scalar paths, which the LDS kernel refuses
    add("dx", 1025, 300, 501, split("dx", "64x32", 0, 1, 1), "nodd-manyrows", epi="relu")
    add("dx", 1025, 300, 500, split("dx", "64x32", 1, 0, 1), "woff-manyrows", off=("W",), epi="sigmoid")
    add("dx", 33, 68, 36, split("dx", "16x32", 1, 1, 1), "ld+4", ld={"dA": 4, "dX": 4, "below": 4, "add": 4}, epi="relu", add=True)
    add("dx", 33, 68, 36, split("dx", "16x32", 0, 1, 0), "ld+3", ld={"dA": 3, "dX": 3, "below": 3, "add": 3}, epi="relu", add=True)
    add("dx", 497, 592, 500, split("dx", "32x64", 1, 1, 1), "ld+4", ld={"dA": 4, "dX": 4, "below": 4}, epi="sigmoid")
    add("dx", 497, 592, 500, split("dx", "32x64", 0, 1, 0), "ld+3", ld={"dA": 3, "dX": 3, "below": 3}, epi="sigmoid")


def _dw():
    # (tile, rows M, K, N): GEMM dims N x (K + 1 with db) over a reduction of M rows
    bases = [("16x32", 17, 48, 36), ("32x32", 33, 44, 16), ("32x48", 17, 784, 400), ("48x32", 17, 400, 784),
             ("32x64", 497, 768, 544), ("64x32", 497, 544, 768)]
    for j, (tile, M, K, N) in enumerate(bases):
        for x in (1, 0):
            for e in (1, 0):
                for s in (0, 1):
                    i = 4 * x + 2 * e + s + j
                    off, k, ld = [], K, {}
                    if not x:
                        if e or i & 1:                  # K % 4 != 0 takes the float4 epilogue with it: misalign instead
                            off += ["dA", "X"] if i & 2 else ["X"]
                        else:
                            k = K - 1
                    if not e and k == K:
                        off.append("dW")
                    add("dw", M, k, N, split("dw", tile, 0, x, e, 0, s), "x%de%d%s" % (x, e, "-slot" if s else ""), off=off,
                        ld=ld, slot=s, db=(i % 3 != 2), accumulate=(i % 4 == 3))
    # LDS-DMA on both 48-wide tiles: 768 rows is the threshold (whole chunks); 777 and 1000 rows take the loop copy for a
    # ragged last chunk; 767 stays on the register path
    for tile, K, N in (("32x48", 784, 400), ("48x32", 400, 784)):
        add("dw", 768, K, N, split("dw", tile, 0, 1, 1, 1, 0), "dma")
        add("dw", 777, K, N, split("dw", tile, 0, 1, 1, 1, 1), "dma-ragged-slot", slot=1)
        add("dw", 1000, K, N, split("dw", tile, 0, 1, 0, 1, 0), "dma-ragged-dwoff", off=("dW",), db=False)
        add("dw", 777, K, N, split("dw", tile, 0, 1, 0, 1, 1), "dma-ragged-dwoff-slot", off=("dW",), slot=1, accumulate=True)
        add("dw", 767, K, N, split("dw", tile, 0, 1, 1, 0, 0), "below-dma")
        add("dw", 777, K, N, split("dw", tile, 0, 1, 1, 1, 0), "dma-ld+4", ld={"dA": 4, "X": 4})
        add("dw", 777, K, N, split("dw", tile, 0, 0, 1, 0, 0), "dma-ld+3", ld={"dA": 3, "X": 3})       # no 16-byte rows: no DMA
        add("dw", 777, K, N, split("dw", tile, 0, 1, 1, 1, 0), "dma-adam", adam=True)
    add("dw", 17, 48, 36, split("dw", "16x32", 0, 1, 1), "ld+4", ld={"dA": 4, "X": 4})
    add("dw", 17, 48, 36, split("dw", "16x32", 0, 0, 1), "ld+3", ld={"dA": 3, "X": 3})
    # the Adam epilogue: float4 and scalar
    add("dw", 33, 48, 36, split("dw", "16x32", 0, 1, 1), "adam", adam=True)
    add("dw", 33, 48, 36, split("dw", "16x32", 0, 1, 0), "adam-moff", off=("mW",), adam=True)
    add("dw", 33, 47, 36, split("dw", "16x32", 0, 0, 0), "adam-kodd", adam=True)
    add("dw", 17, 784, 400, split("dw", "32x48", 0, 1, 1), "adam", adam=True)


_fwd_split()
_fwd_k32()
_fwd_lds()
_dx_lds()
_dx_split()
_dw()
assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"
