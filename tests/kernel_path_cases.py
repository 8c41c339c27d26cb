"""The non-GEMM kernels' launch paths as tables of cases (tests/test_kernel_path_cases_cpu.py checks the tables' own
bookkeeping, tests/test_gpu_kernel_paths.py runs every case on the GPU inside the guarded buffers of tests/guarded.py).

Most kernels around the GEMMs decide on the host between a 16-byte (`vec`) and an element (`elem`) instantiation: from
the width, a width cap, every leading dimension and every pointer's alignment -- silently.  They have no plan query, so
a case carries the arm it is BUILT to reach and the one clause of the host predicate that sends it there; PREDICATES
quotes each predicate with file and line, `failed()` evaluates its clauses from the case's own placement, and the CPU
test holds the two against each other.  The flat kernels cap their grid and walk the rest in a stride loop, the column
reductions unroll over rows: their cases (arm `loop`) name the trip count they are built to reach in their tag.  The
fp64 / fp32 evaluations of every expression live here too (`dt` picks the precision): the expressions and tolerances
of tests/test_gpu_fused_ops.py, tests/test_gpu_ops.py and tests/test_gpu_pdwgan.py, lifted, not restated elsewhere.

Cases per kernel:
    gp_norm: 36
    pdw_dir: 30
    pdw_couple: 36
    head_gp: 25
    gp_dw2: 24
    dragan_head_bwd: 18
    made_bce: 15
    iwae_weights: 15
    bir_mmd: 20
    gather_rows: 6
    gather_bits: 5
    dvae_corrupt: 14
    gather_corrupt: 14
    gather_bits_corrupt: 12
    adam: 24
    gp_u: 2
    bir_reparam: 1
    act_bwd: 3
    copy_slot: 1
    sum_finalize: 27
    interp: 2
    sqerr_sigmoid_bwd: 2
    vae_reparam: 2
    vae_reparam_wide: 2
    vae_reparam_bwd: 2
    l1_rows: 2
    dragan_xhat: 2
    dragan_rows: 2
"""
import functools
import re
from collections import OrderedDict, namedtuple

import numpy as np
import torch

Case = namedtuple("Case", "id kernel B W arm clause off ld absent flags")
# B rows, W width (I / H / Z / n); arm: "vec" | "elem" | "loop"; clause: the predicate clause that fails (elem only);
# off: arrays one float past a 16-byte boundary; ld: array -> floats added to its width; absent: optional arrays left out

# ---- the host predicates ----------------------------------------------------------------------------------------------
# width: the name of the width in the source; cap: the register-resident paths' width cap; arrays: (name, its leading
# dimension's name in the source, or None for a vector / contiguous array) of every array the predicate names; extra:
# further clauses.  The vector arm needs every clause to hold.
PREDICATES = OrderedDict([
    # csrc/gm_fused.hip:112-113  vec4 = (I % 4 == 0) && I <= 1024 && (ldg % 4 == 0) && (ldm % 4 == 0) && ((g | gam) & 15) == 0
    ("gp_norm", dict(width="I", cap=1024, arrays=(("g", "ldg"), ("gamma", "ldm")))),
    # csrc/gm_pdw.hip:162-163  vec4 = (I % 4 == 0) && I <= 1024 && pdw_al16(g, ldg) && pdw_al16(x, ldx) && pdw_al16(xr, ldr)
    #                                 && pdw_al16(gamma, ldm);  pdw_al16(q, ld) (:94-96) = !q || (q & 15) == 0 && ld % 4 == 0
    ("pdw_dir", dict(width="I", cap=1024, arrays=(("g", "ldg"), ("x", "ldx"), ("xr", "ldr"), ("gamma", "ldm")))),
    # csrc/gm_pdw.hip:104-105  vec4 = (I % 4 == 0) && I <= 1024 && pdw_al16(x, ldx) && pdw_al16(xr, ldr) &&
    #                                 pdw_al16(dA, ldd) && pdw_al16(xhat, ldh) && pdw_al16(xcopy, ldc)
    ("pdw_couple", dict(width="I", cap=1024, arrays=(("x", "ldx"), ("xr", "ldr"), ("dA", "ldd"), ("xhat", "ldh"),
                                                      ("xcopy", "ldc")))),
    # csrc/gm_fused.hip:224-226  vec4 = (H % 4 == 0) && H <= 512 && (ldh % 4 == 0) && (ldu % 4 == 0) && ((h | w2 | u) & 15) == 0
    ("head_gp", dict(width="H", cap=512, arrays=(("h", "ldh"), ("w2", None), ("u", "ldu")))),
    # csrc/gm_made.hip:185-186  vec = I % 4 == 0 && lda % 4 == 0 && ldx % 4 == 0 && al16(logits) && al16(x) &&
    #                                 (!dA || (ldd % 4 == 0 && al16(dA)))
    ("made_bce", dict(width="I", cap=None, arrays=(("logits", "lda"), ("x", "ldx"), ("dA", "ldd")))),
    # csrc/gm_iwae.hip:235-236  vec = I % 4 == 0 && ldx % 4 == 0 && ldr % 4 == 0 && al16(x) && al16(xr) &&
    #                                 (!dA || (lda % 4 == 0 && al16(dA)))
    ("iwae_weights", dict(width="I", cap=None, arrays=(("x", "ldx"), ("xr", "ldr"), ("dA", "lda")))),
    # csrc/gm_fused.hip:380-382  al = (ldz % 4 == 0) && ((z | prior) & 15) == 0 && (prior_slot.stride % 4 == 0); the
    # compile-time-Z kernels take Z in {20, 8, 32} under `al`, the generic kernel everything else
    ("bir_mmd", dict(width=None, cap=None, arrays=(("z", "ldz"), ("prior", None)), extra=("prior_slot.stride % 4",))),
    # csrc/gm_gather.h:82-84  vec = (row_elems % 4 == 0) && (ld_out % 4 == 0) && (data & 15) == 0 && (out & 15) == 0
    ("gather_rows", dict(width="row_elems", cap=None, arrays=(("data", None), ("out", "ld_out")))),
    # csrc/gm_gather.h:97  vec = (row_elems % 4 == 0) && (ld_out % 4 == 0) && (out & 15) == 0
    ("gather_bits", dict(width="row_elems", cap=None, arrays=(("out", "ld_out"),))),
    # csrc/gm_dvae.hip:58  vec = row_elems % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && al16(x) && al16(out)
    ("dvae_corrupt", dict(width="row_elems", cap=None, arrays=(("x", "ldx"), ("out", "ldo")))),
    # csrc/gm_gather.h:82-84 and csrc/gm_dvae.h:109  vec = (the gather's) && (out_c & 15) == 0; out_c has out's ld
    ("gather_corrupt", dict(width="row_elems", cap=None, arrays=(("data", None), ("out", "ld_out"), ("out_c", None)))),
    # csrc/gm_gather.h:97 and csrc/gm_dvae.h:109
    ("gather_bits_corrupt", dict(width="row_elems", cap=None, arrays=(("out", "ld_out"), ("out_c", None)))),
])
# arrays that take the leading dimension of another one (the wrapper refuses anything else)
LD_FOLLOWS = {"gather_corrupt": {"out_c": "out"}, "gather_bits_corrupt": {"out_c": "out"}}


def clauses(kernel):
    """Every clause of the kernel's predicate, as the strings the cases carry."""
    p = PREDICATES[kernel]
    out = []
    if p["width"]:
        out.append("%s %% 4" % p["width"])
    if p["cap"]:
        out.append("%s > %d" % (p["width"], p["cap"]))
    out += ["%s %% 4" % ld for _, ld in p["arrays"] if ld]
    out += ["%s off 16 B" % n for n, _ in p["arrays"]]
    return out + list(p.get("extra", ()))


def failed(c):
    """The clauses of its kernel's predicate that the case's own shape and placement fail (absent arrays pass)."""
    p = PREDICATES[c.kernel]
    out = []
    if p["width"] and c.W % 4:
        out.append("%s %% 4" % p["width"])
    if p["cap"] and c.W > p["cap"]:
        out.append("%s > %d" % (p["width"], p["cap"]))
    for n, ld in p["arrays"]:
        if n in c.absent:
            continue
        if ld and (c.W + c.ld.get(n, 0)) % 4:
            out.append("%s %% 4" % ld)
        if n in c.off:
            out.append("%s off 16 B" % n)
    if c.flags.get("odd_stride"):
        out.append("prior_slot.stride % 4")
    return out


CASES = []


def add(kernel, tag, B, W, arm, clause=None, off=(), ld=None, absent=(), **flags):
    CASES.append(Case("%s-B%d-W%d-%s" % (kernel, B, W, tag), kernel, B, W, arm, clause, tuple(off), dict(ld or {}),
                      tuple(absent), flags))


def cases(kernel):
    return [c for c in CASES if c.kernel == kernel]


def placements(kernel, B, W, tag="", absent=(), one_at_a_time=True, **flags):
    """aligned; ld + 4 on every array (keeps the vector arm); then ld + 3 and off = 1 on ONE array at a time, over every
    array the predicate names: a predicate that forgets an operand shows only when that operand alone is off."""
    p = PREDICATES[kernel]
    names = [(n, ld) for n, ld in p["arrays"] if n not in absent]
    follows = LD_FOLLOWS.get(kernel, {})
    add(kernel, tag + "aligned", B, W, "vec", absent=absent, **flags)
    add(kernel, tag + "ld+4", B, W, "vec", ld={n: 4 for n, ld in names if ld or n in follows}, absent=absent, **flags)
    if not one_at_a_time:
        return
    for n, ld in names:
        if ld:
            lds = {n: 3}
            lds.update({f: 3 for f, src in follows.items() if src == n})
            add(kernel, tag + "%s+3" % ld, B, W, "elem", "%s %% 4" % ld, ld=lds, absent=absent, **flags)
    for n, _ in names:
        add(kernel, tag + "%s-off" % n, B, W, "elem", "%s off 16 B" % n, off=(n,), absent=absent, **flags)


def whole_rows(kernel, W, absent=()):
    """Leading dimensions that pad a ragged width to whole float4s: the width clause then fails ALONE."""
    follows = LD_FOLLOWS.get(kernel, {})
    return {n: (-W) % 4 for n, ld in PREDICATES[kernel]["arrays"] if (ld or n in follows) and n not in absent and W % 4}


def width_arm(kernel, W):
    p = PREDICATES[kernel]
    if W % 4:
        return "elem", "%s %% 4" % p["width"]
    if p["cap"] and W > p["cap"]:
        return "elem", "%s > %d" % (p["width"], p["cap"])
    return "vec", None


# ---- 2. row kernels with a register-resident vector path and a width cap ---------------------------------------------
# four float4 slots per lane under the cap of 1024 (two under 512 for head_gp): 4 = one float4 in lane 0, every other
# load clamped; 252 / 256 / 260 = slot 0 one short, exactly full, slot 1 in lane 0 only; 1020 / 1024 every slot (one
# short, full); 1028 vector-eligible but past the cap; 1, 3, 1023 ragged
ROW_WIDTHS = (1, 3, 4, 252, 256, 260, 1020, 1024, 1028, 1023)
HEAD_WIDTHS = (1, 3, 4, 256, 260, 508, 512, 516, 37)


def _rows():
    for W in ROW_WIDTHS:
        for B in (1, 5):
            arm, cl = width_arm("gp_norm", W)
            for k in ((1.0, 0.75) if B == 5 else (1.0,)):          # DRAGAN passes its own k
                add("gp_norm", "k%g" % k, B, W, arm, cl, ld=whole_rows("gp_norm", W), k=k)
            add("pdw_dir", "sweep", B, W, arm, cl, ld=whole_rows("pdw_dir", W))
            add("pdw_couple", "sweep", B, W, arm, cl, ld=whole_rows("pdw_couple", W), ring=(B == 5))   # t through a ring slot
    placements("gp_norm", 5, 256, k=1.0)
    placements("pdw_dir", 5, 256)
    placements("pdw_couple", 5, 256, ring=True)
    for ab in (("n",), ("dA",), ("xhat", "t"), ("xcopy",)):           # each optional array absent in turn
        add("pdw_couple", "no-" + ab[0], 5, 256, "vec", absent=ab, ring=True)
    for W in HEAD_WIDTHS:
        for B in (1, 5):
            arm, cl = width_arm("head_gp", W)
            add("head_gp", "sweep", B, W, arm, cl, ld=whole_rows("head_gp", W))
    placements("head_gp", 5, 260)


# ---- 3. column reductions --------------------------------------------------------------------------------------------
# gp_dw2_kernel (csrc/gm_fused.hip:126-158): 32 row-groups, `for (; b + 96 < B; b += 128)` four rows in flight, then the
# tail.  B = 97: the first B at which row-group 0 enters the unrolled loop; 129: an unrolled trip and a tail; 225: two.
DW2_B, DW2_H = (1, 31, 32, 33, 97, 128, 129, 225), (1, 31, 32, 33, 65)
# dragan_head_bwd_kernel (:1538-1581): HB_COLS = 16 columns x HB_RG = 64 row-groups; gb2 by workgroup 0, 1024 stride
HB_B, HB_H = (1, 63, 64, 65, 1025), (1, 15, 16, 17, 33)


def _columns():
    for store in (False, True):
        t = "store" if store else "acc"
        for B, H in [(B, 33) for B in DW2_B] + [(129, H) for H in DW2_H if H != 33]:
            add("gp_dw2", t, B, H, "loop", ld={"h": 3, "t": 3}, store=store)
        for B, H in [(B, 17) for B in HB_B] + [(65, H) for H in HB_H if H != 17]:
            add("dragan_head_bwd", t, B, H, "loop", ld={"H": 3, "T": 3, "dA1": 3}, store=store)


# ---- 4. placement cases for the other dual-path kernels (one small vector-eligible shape each, and one ragged width) ---
def _dual():
    for kernel, B, W in (("made_bce", 5, 64), ("iwae_weights", 3, 64)):
        placements(kernel, B, W)
        placements(kernel, B, W, tag="noda-", absent=("dA",))
        add(kernel, "ragged", B, 61, "elem", "I % 4", ld=whole_rows(kernel, 61))
    for Z in (20, 8):
        for dz in (True, False):
            t = "" if dz else "nodz-"
            ab = () if dz else ("dz",)
            add("bir_mmd", t + "aligned-ring", 37, Z, "vec", absent=ab, ring=True)
            add("bir_mmd", t + "ldz+3", 37, Z, "elem", "ldz % 4", ld={"z": 3}, absent=ab)
            add("bir_mmd", t + "z-off", 37, Z, "elem", "z off 16 B", off=("z",), absent=ab)
            add("bir_mmd", t + "prior-off", 37, Z, "elem", "prior off 16 B", off=("prior",), absent=ab, ring=True)
        add("bir_mmd", "lddz+3", 37, Z, "vec", ld={"dz": 3})          # dz is written by elements: not in the predicate
    add("bir_mmd", "odd-stride", 37, 20, "elem", "prior_slot.stride % 4", ring=True, odd_stride=True)
    add("bir_mmd", "nodz-odd-stride", 37, 20, "elem", "prior_slot.stride % 4", ring=True, odd_stride=True,
        absent=("dz",))
    placements("gather_rows", 16, 64)
    add("gather_rows", "ragged", 16, 61, "elem", "row_elems % 4", ld=whole_rows("gather_rows", 61))
    placements("gather_bits", 16, 64)
    add("gather_bits", "ragged", 16, 61, "elem", "row_elems % 4", ld=whole_rows("gather_bits", 61))
    for noise in ("salt_pepper", "gaussian"):
        placements("dvae_corrupt", 9, 64, tag=noise + "-", noise=noise)
        add("dvae_corrupt", noise + "-ragged", 9, 61, "elem", "row_elems % 4", ld=whole_rows("dvae_corrupt", 61), noise=noise)
        placements("gather_corrupt", 16, 64, tag=noise + "-", noise=noise)
        placements("gather_bits_corrupt", 16, 64, tag=noise + "-", noise=noise)
        for k in ("gather_corrupt", "gather_bits_corrupt"):
            add(k, noise + "-ragged", 16, 61, "elem", "row_elems % 4", ld=whole_rows(k, 61), noise=noise)


# ---- 5. flat kernels past their grid caps, and the short ends --------------------------------------------------------
# adam_kernel (csrc/gm_ops.hip:357-386): float4 loop over n / 4, at most 1024 workgroups of 256 -> the stride loop's
# second trip needs n > 1 048 576; then the tail of n % 4.  n < 4: no float4 at all.
ADAM_SMALL, ADAM_LARGE = (1, 2, 3, 4, 5, 1023), (1048576 + 7, 2 * 1048576 + 4 * 3 + 3)
# gm_strided_sum_1024 (csrc/gm_common.h:54-65): batches of 8 x 1024 clamped loads
SUM_N = (1, 7, 1023, 1024, 1025, 8191, 8192, 8193, 8192 + 3 * 1024 + 5)
ACTS = ("id", "relu", "sigmoid")


def _flat():
    for scaled in (False, True):
        t = "scaled" if scaled else "plain"
        for n in ADAM_SMALL:
            add("adam", t, 1, n, "loop", steps=3, scaled=scaled)
        for n in ADAM_LARGE:
            add("adam", t, 1, n, "loop", steps=2, scaled=scaled)
        for name in ("p", "g", "m", "v"):                            # refused on the host: nothing is launched
            add("adam", t + "-%s-off" % name, 1, 1023, "loop", off=(name,), steps=1, scaled=scaled, refused=True)
    add("gp_u", "capped", 1030, 512, "loop", ld={"h": 3, "u": 1})      # 527 360 elements > 2048 x 256
    add("gp_u", "one", 1, 1, "loop", ld={"h": 3, "u": 1})
    add("bir_reparam", "capped", 1100, 60, "loop", ld={"mu": 3, "z": 3})   # 66 000 > 256 x 256
    for a in ACTS:
        add("act_bwd", a, 1, 2048 * 256 + 5, "loop", act=a)
    add("copy_slot", "slots", 1, 1024 * 256 + 5, "loop")
    for form in ("plain", "tick", "fin2"):
        for n in SUM_N:
            add("sum_finalize", form, 1, n, "loop", form=form)


# ---- 6. leading dimensions for the rest of gm_fused.hip --------------------------------------------------------------
LD_KERNELS = OrderedDict([   # kernel -> (width, its matrices in argument order: each gets ld = width + 1, + 2, + 3, ...)
    ("interp", (37, ("x", "g", "out"))), ("sqerr_sigmoid_bwd", (37, ("x", "xr", "dA"))),
    ("vae_reparam", (6, ("ml", "z"))), ("vae_reparam_wide", (6, ("ml", "z"))), ("vae_reparam_bwd", (6, ("ml", "dz", "dml"))),
    ("l1_rows", (37, ("Y", "X", "dY"))), ("dragan_xhat", (37, ("x", "out"))), ("dragan_rows", (37, ("V", "dv")))])


def _lds():
    for kernel, (W, names) in LD_KERNELS.items():
        for B in (1, 5):
            add(kernel, "lds", B, W, "loop", ld={n: i + 1 for i, n in enumerate(names)}, ring=True)


_rows()
_columns()
_dual()
_flat()
_lds()
assert len({c.id for c in CASES}) == len(CASES), "case ids must be unique"
KERNELS = list(OrderedDict((c.kernel, 1) for c in CASES))


def docstring_counts():
    return {k: int(v) for k, v in re.findall(r"^    (\w+): (\d+)$", __doc__, flags=re.M)}


# ---- comparison ---------------------------------------------------------------------------------------------------------
ULP = 2.0 ** -23


def row_errors(got, ref64, ref32=None, tol=None, rows=False, scale=None):
    """(ratio, e_hip, e_cpu, bound, row): close64 (tests/linear_path_cases.py) with a scale per row.  rows: every row (of
    a per-row array: every element) is measured in units of its OWN largest reference magnitude -- a zero-norm row and a
    row of norm 30 sit in one launch; else the whole array in units of its largest magnitude.  e_hip / e_cpu: the largest
    such error of the HIP result / of the fp32 CPU evaluation against fp64, each over all rows, as close64 takes each
    over all elements (pairing them row by row would hang the verdict on how lucky the host's summation order was in
    that one row, which differs from host to host).  bound: `tol` where the kernel's per-op test states one, else twice
    e_cpu plus 2^-23.  A reference row that is exactly zero has to be matched exactly.  scale: the scale a stated
    tolerance is in units of where that is not the reference's largest magnitude (a float, or one per row).  row: where
    e_hip is."""
    d = lambda t: t.detach().cpu().double()
    got, ref64 = d(got), d(ref64)
    ref64 = ref64.reshape(got.shape) if ref64.numel() == got.numel() else ref64
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    shape = (got.shape[0], -1) if rows and got.dim() > 0 else (1, -1)
    got, ref64 = got.reshape(shape), ref64.reshape(shape)
    if scale is None:
        scale = ref64.abs().amax(1).clamp_min(1e-30)
    else:
        scale = torch.as_tensor(scale, dtype=torch.float64).reshape(-1).expand(got.shape[0])
    e_rows = (got - ref64).abs().amax(1) / scale
    e_rows = torch.where(torch.isnan(e_rows), torch.full_like(e_rows, float("inf")), e_rows)
    e_hip, r = float(e_rows.max()), int(e_rows.argmax())
    e_cpu = float(((d(ref32).reshape(shape) - ref64).abs().amax(1) / scale).max()) if ref32 is not None else 0.0
    bound = float(tol) if tol is not None else 2.0 * e_cpu + ULP
    return e_hip / bound, e_hip, e_cpu, bound, r


# ---- inputs and references: `dt` is torch.float64 (the reference) or torch.float32 (the CPU yardstick) ------------------
LAM = 10.0
NORMS = (3.0, 0.0, 30.0, 0.25, 2.0)       # the row norms of a B = 5 launch, away from k (pen = (n - k)^2 cancels near it)


def inv_b(B):
    return float(np.float32(1.0) / np.float32(B))


def gen(*key):
    return torch.Generator().manual_seed(int.from_bytes(repr(key).encode(), "little") % (2 ** 63 - 1))


def scaled_rows(t, norms):
    """Rows of t rescaled to the given norms (0: an all-zero row)."""
    n = t.double().norm(2, dim=1, keepdim=True).clamp_min(1e-30)
    return (t.double() / n * torch.tensor(norms[:t.shape[0]], dtype=torch.float64)[:, None]).float()


@functools.lru_cache(maxsize=8)
def row_inputs(kernel, B, W):
    g = gen(kernel, B, W)
    if kernel == "gp_norm":
        return dict(g=scaled_rows(torch.randn(B, W, generator=g), NORMS))
    if kernel in ("pdw_dir", "pdw_couple"):
        x = torch.rand(B, W, generator=g)
        xr = torch.sigmoid(torch.randn(B, W, generator=g))
        if B > 1:
            xr[1] = x[1]                                             # a row the reconstruction hits exactly: norm 0
        t = dict(x=x, xr=xr, t=torch.rand(B, generator=g), g=torch.randn(B, W, generator=g) / W ** 0.5)
        t["n"] = (x.double() - xr.double()).norm(2, dim=1).float()
        return t
    assert kernel == "head_gp"
    w2 = torch.randn(W, generator=g) / W ** 0.5
    base = torch.relu(torch.randn(B, W, generator=g) + 0.5)          # a hidden layer behind its ReLU: exact zeros
    alive = (torch.arange(B) % 2 == 0)[:, None]                      # rows 0, 2, 4 lean on w2 > 0, rows 1, 3 on w2 < 0
    lean = torch.where((w2[None, :] > 0) == alive, torch.tensor(1.0), torch.tensor(0.125))
    return dict(h=base * lean, w2=w2, b2=torch.tensor([0.05]))


def ref_gp_norm(t, k, dt):
    g = t["g"].to(dt)
    B = g.shape[0]
    n = g.norm(2, dim=1)
    dn = n - k
    coef = torch.where(n > 0, (LAM * (inv_b(B) * (2 * dn))) / n.clamp_min(1e-30), torch.zeros_like(n))
    return dict(pen=dn * dn, gamma=g * coef[:, None])


def ref_pdw(t, dt):
    x, xr, tt, g = (t[n].to(dt) for n in ("x", "xr", "t", "g"))
    B = x.shape[0]
    ib = inv_b(B)
    diff = x - xr
    n = diff.norm(2, dim=1)
    d = torch.where(n[:, None] > 0, diff / n[:, None].clamp_min(1e-30), torch.zeros_like(diff))
    out = dict(n=n, share=n * ib, dA=-(d * ib) * (xr * (1 - xr)), xhat=tt[:, None] * x + (1 - tt[:, None]) * xr)
    # pdw_dir is handed n as fp32 (tests/test_gpu_pdwgan.py::test_pdw_dir_vs_fp64): d from that n
    nd = t["n"].to(dt)
    dd = torch.where(nd[:, None] > 0, diff / nd[:, None].clamp_min(1e-30), torch.zeros_like(diff))
    e = g - dd
    out.update(pen=(e * e).sum(1), gamma=LAM * (ib * 2) * e)
    return out


def ref_head_gp(t, dt):
    h, w2, b2 = (t[n].to(dt) for n in ("h", "w2", "b2"))
    a2 = h @ w2 + b2
    return dict(a2=a2, s=torch.relu(a2))


@functools.lru_cache(maxsize=8)
def column_inputs(kernel, B, H):
    g = gen(kernel, B, H)
    r = lambda *s: torch.randn(*s, generator=g)
    holes = lambda *s: (torch.rand(*s, generator=g) > 0.2).float()   # exact zeros among both signs
    s = r(B)
    s[1::3] = 0.0
    s[0] = s[0].abs() + 0.1
    if kernel == "gp_dw2":
        return dict(s=s, h=r(B, H) * holes(B, H), t=r(B, H), gw2=r(H))
    return dict(H=r(B, H) * holes(B, H), T=r(B, H), da2=s / B, w2=r(H), gw2=r(H), gb2=r(1))


def ref_gp_dw2(t, store, dt):
    s, h, tt = (t[n].to(dt) for n in ("s", "h", "t"))
    v = (((s > 0)[:, None] & (h > 0)).to(dt) * tt).sum(0)
    return dict(gw2=v if store else t["gw2"].to(dt) + v)


def ref_dragan_head_bwd(t, store, dt):
    H, T, d, w = (t[n].to(dt) for n in ("H", "T", "da2", "w2"))
    on = H > 0
    gw2 = (torch.where(on, T, torch.zeros_like(T)) + d[:, None] * H).sum(0)
    gb2 = d.sum().reshape(1)
    if not store:
        gw2, gb2 = t["gw2"].to(dt) + gw2, t["gb2"].to(dt) + gb2
    return dict(gw2=gw2, gb2=gb2, dA1=torch.where(on, d[:, None] * w[None, :], torch.zeros_like(T)))


@functools.lru_cache(maxsize=4)
def sum_inputs(n):
    g = gen("sum", n)
    sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    return sign * 10.0 ** (torch.rand(n, generator=g) * 6 - 3)        # mixed signs, magnitudes 1e-3 .. 1e3


def act_bwd_ref(dY, Y, act, dt):
    g, s = dY.to(dt), Y.to(dt)
    return (g * (1 - s)) * s if act == "sigmoid" else torch.where(s > 0, g, torch.zeros_like(g)) if act == "relu" else g


@functools.lru_cache(maxsize=16)
def ld_inputs(kernel, B, W):
    g = gen(kernel, B, W)
    r = lambda *s: torch.randn(*s, generator=g)
    u = lambda *s: torch.rand(*s, generator=g)
    if kernel == "interp":
        return dict(eps=u(B), x=u(B, W), g=u(B, W))
    if kernel == "sqerr_sigmoid_bwd":
        return dict(x=(u(B, W) < 0.13).float(), xr=torch.sigmoid(r(B, W).double()).float())
    if kernel in ("vae_reparam", "vae_reparam_wide", "vae_reparam_bwd"):
        g = gen("vae_reparam*", B, W)                                # one set of inputs: the two forward forms agree bit for bit
        return dict(ml=r(B, 2 * W) * 0.5, eps=r(B, W), dz=r(B, W))
    if kernel == "l1_rows":
        return dict(Y=r(2 * B, W), X=r(2 * B, W), K=torch.tensor([0.37]))
    if kernel == "dragan_xhat":
        x = (u(B, W) < 0.13).float()
        return dict(x=x, delta=u(B), U=u(B, W), std=x.std().reshape(1) if x.numel() > 1 else torch.tensor([0.3]))
    assert kernel == "dragan_rows"
    s = torch.sigmoid(r(B))
    sp = ((1 - s) * s).double()
    V = scaled_rows(r(B, W), NORMS).double() / sp[:, None]           # ||s' v|| = NORMS: away from K = 1
    return dict(s=s, V=V.float())


def ref_ld(kernel, t, dt):
    """The expressions of tests/test_gpu_fused_ops.py (interp, sqerr, reparam, dragan) and tests/test_gpu_ops.py (l1)."""
    c = {n: v.to(dt) for n, v in t.items()}
    if kernel == "interp":
        return dict(out=c["eps"][:, None] * c["x"] + (1 - c["eps"][:, None]) * c["g"])
    if kernel == "sqerr_sigmoid_bwd":
        x, xr = c["x"], c["xr"]
        return dict(dA=(-(2 * (x - xr)) * (1 - xr)) * xr, partial=((x - xr) ** 2).sum(1))
    if kernel in ("vae_reparam", "vae_reparam_wide", "vae_reparam_bwd"):
        Z = c["eps"].shape[1]
        mu, lv, e, dz = c["ml"][:, :Z], c["ml"][:, Z:], c["eps"], c["dz"]
        return dict(z=mu + e * torch.exp(lv / 2), kl=torch.sum(0.5 * (mu ** 2 + torch.exp(lv) - lv - 1)).reshape(1),
                    dml=torch.cat([dz + mu, dz * e * 0.5 * torch.exp(lv / 2) + 0.5 * (torch.exp(lv) - 1)], 1))
    if kernel == "l1_rows":
        B = c["Y"].shape[0] // 2
        coef = torch.cat([torch.full((B, 1), 1.0 / B, dtype=dt), -c["K"].reshape(1, 1).expand(B, 1) / B])
        return dict(rowsum=(c["Y"] - c["X"]).abs().sum(1), dY=torch.sign(c["Y"] - c["X"]) * coef)
    if kernel == "dragan_xhat":
        d = c["delta"][:, None]
        return dict(out=d * c["x"] + (1 - d) * (c["x"] + c["std"] * c["U"]))
    assert kernel == "dragan_rows"
    s, V = c["s"], c["V"]
    B = s.shape[0]
    sp = (1 - s) * s
    gg = sp[:, None] * V
    n = gg.norm(2, dim=1)
    dn = n - 1.0
    coef = torch.where(n > 0, (LAM * (inv_b(B) * (2 * dn))) / n.clamp_min(1e-30), torch.zeros_like(n))
    gam = coef[:, None] * gg
    return dict(pen=dn * dn, dv=sp[:, None] * gam, da2=(gam * V).sum(1) * (sp * (1 - 2 * s)))
