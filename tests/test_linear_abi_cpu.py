"""The descriptor entry points of the linear layers (gm_linear_fwd_ex / gm_linear_bwd_dx_ex / gm_linear_bwd_dw_ex,
include/gm_hip.h) refuse on the host, before any launch: (1) every combination of optional blocks that no kernel
implements, (2) every bad value the argument checks of the launches they carry name.  No GPU: every call here returns
GM_EINVAL from the argument checks; the pointers are placeholders that are never dereferenced.  Each case starts from a
descriptor that passes every check, changes one thing, and expects gm_last_error to name that thing."""
import ctypes
import itertools
import os

import pytest

from generative_models_amd import _lib

pytestmark = pytest.mark.skipif(not os.path.isfile(_lib.LIB_PATH), reason="libgm_hip.so not built")

E = _lib.GM_EINVAL
X, W, Y, A, B_, C, D, G1, G2, G3, G4, H1, H2 = (4096 * i for i in range(1, 14))   # distinct, 16-byte aligned


def P(i):
    return 4096 * (20 + i)


def _err():
    return _lib.load().gm_last_error().decode()


def _set(obj, **kw):
    for k, v in kw.items():
        setattr(obj, k, v)
    return obj


# ---- descriptors that pass every check ------------------------------------------------------------------------------
def gather(**kw):
    return _set(_lib.GatherArgs(data=G1, n_rows=16, idx=G2, out=G3, ld_out=8, B=4, row_elems=8), **kw)


def gather_bits(**kw):
    return _set(_lib.GatherArgs(bits=G1, words_per_row=1, n_rows=16, idx=G2, out=G3, ld_out=8, B=4, row_elems=8), **kw)


def corrupt():
    return ctypes.pointer(_lib.CorruptArgs(kind=1, level=0.5, seed=1))


FWD_BLOCKS = {
    "interp": dict(ip_eps=A, ip_x=B_, ip_ldx=8, ip_out=C, ip_ldo=8, ip_rows=4),
    "head": dict(hd_w2=A, hd_b2=B_, hd_part=C, hd_ldp=4, hd_snap=D),
    "sqerr": dict(sq_target=A, sq_ldt=8, sq_dA=B_, sq_lda=8, sq_part=C, sq_ldp=1, act=2),
    "label": dict(lb_E=A, lb_C=3, lb=_lib.LabelSrc(B_, None, _lib.NO_SLOT)),
    "gather": dict(gather=ctypes.pointer(gather())),
}
XBITS = dict(xbits=G4, xbits_wpr=1, xbits_rows=32)


def fwd(*blocks, **kw):
    a = _lib.FwdArgs(X=X, ldx=8, W=W, Y=Y, ldy=8, M=32, K=8, N=8, act=1)
    for b in blocks:
        _set(a, **FWD_BLOCKS[b])
    return _set(a, **kw)


def head_args(**kw):
    return _set(_lib.HeadBwdArgs(H=H1, ldh=8, dS=P(1), w2=P(2), b2=P(3), rowloss=P(4), gw2=P(5), gb2=P(6),
                                 loss_out=P(7), inv_b=0.25, B=16, Hd=8), **kw)


def fold_args(**kw):
    return _set(_lib.HeadFoldArgs(part=P(8), ldp=4, nparts=1, snap=P(9), variant=0, out_act=2), **kw)


def dx(**kw):
    return _set(_lib.DxArgs(dA=A, lda=8, W=W, dX=X, ldx=8, M=32, K=8, N=8, epi=0), **kw)


DX_BLOCKS = {
    "add": lambda: dict(add=B_, ldadd=8, add_scale=1.0),
    "head": lambda: dict(head=ctypes.pointer(head_args())),
    "reparam": lambda: dict(rp_ml=B_, rp_ldml=16, rp_eps=C, rp_dml=D, rp_ldd=16),
    "gather": lambda: dict(gather=ctypes.pointer(gather())),
}


def dw(i=0, adam=True, **kw):
    b = 40 + 12 * i
    a = _lib.DwAdamArgs(dA=P(b), lda=8, X=P(b + 1), ldx=8, dW=P(b + 2), db=P(b + 3), M=32, K=8, N=8)
    if adam:
        _set(a, pW=P(b + 4), mW=P(b + 5), vW=P(b + 6), pb=P(b + 7), mb=P(b + 8), vb=P(b + 9), sched=P(b + 10),
             beta1=0.9, beta2=0.999, eps=1e-8)
    return _set(a, **kw)


def dw_head(**kw):          # the critic step's folded form: dA is the hidden layer H [2B, Hd]
    a = dw(**kw)
    h = head_args(H=a.dA)
    return a, h, fold_args()


def call_fwd(a):
    return _lib.load().gm_linear_fwd_ex(None, ctypes.byref(a))


def call_dx(a):
    return _lib.load().gm_linear_bwd_dx_ex(None, ctypes.byref(a))


def call_dw(a, b=None, t=None):
    return _lib.load().gm_linear_bwd_dw_ex(None, ctypes.byref(a), ctypes.byref(b) if b is not None else None,
                                          ctypes.byref(t) if t is not None else None)


def refused(rc, what):
    assert rc == E, (rc, what)
    assert what in _err(), (_err(), what)


# ---- a zeroed descriptor is the plain entry point's bad call ---------------------------------------------------------
def test_zeroed_and_null_descriptors_are_bad_arguments():
    lib = _lib.load()
    assert lib.gm_linear_fwd(None, None, 0, _lib.NO_SLOT, None, None, None, 0, 0, 0, 0, 0) == E
    plain = _err()
    assert plain.startswith("bad argument")
    refused(call_fwd(_lib.FwdArgs()), "bad argument")
    assert _err() == plain                                                   # the same check fires
    refused(call_dx(_lib.DxArgs()), "bad argument")
    refused(call_dw(_lib.DwAdamArgs()), "bad argument")
    for fn in (lib.gm_linear_fwd_ex, lib.gm_linear_bwd_dx_ex):
        assert fn(None, None) == E
    assert lib.gm_linear_bwd_dw_ex(None, None, None, None) == E


# ---- (1) combinations of optional blocks that no kernel implements ---------------------------------------------------
def test_forward_refuses_unreachable_block_combinations():
    for a, b in itertools.combinations(FWD_BLOCKS, 2):
        refused(call_fwd(fwd(a, b)), "at most one")
    refused(call_fwd(fwd(*FWD_BLOCKS)), "at most one")
    for blk in ("interp", "sqerr", "label", "gather"):
        refused(call_fwd(fwd(blk, **XBITS)), "xbits")
    refused(call_fwd(fwd(**XBITS)), "xbits")
    refused(call_fwd(fwd(gather=ctypes.pointer(gather(corrupt=corrupt())))), "!a.corrupt == !a.out_c")
    refused(call_fwd(fwd(gather=ctypes.pointer(gather(out_c=G4)))), "!a.corrupt == !a.out_c")
    for blk in ("sqerr", "label"):
        for s in (_lib.slot(ctr=G4), _lib.slot(add=1), _lib.slot(mul=1), _lib.slot(ring=2), _lib.slot(stride=4)):
            refused(call_fwd(fwd(blk, x_slot=s)), "no ring slot")
    refused(call_fwd(fwd("sqerr", act=1)), "GM_ACT_SIGMOID")      # the sqerr launch is the sigmoid output layer's


def test_input_gradient_refuses_unreachable_block_combinations():
    for a, b in itertools.combinations(DX_BLOCKS, 2):
        refused(call_dx(dx(**DX_BLOCKS[a](), **DX_BLOCKS[b]())), "at most one")
    refused(call_dx(dx(fold=ctypes.pointer(fold_args()))), "fold needs head")
    rp = DX_BLOCKS["reparam"]()
    refused(call_dx(dx(below=B_, ld_below=8, **rp)), "no activation gradient")
    refused(call_dx(dx(below=B_, ld_below=8, epi=1, **rp)), "no activation gradient")
    # the riding gather of an input gradient writes fp32 rows, uncorrupted
    refused(call_dx(dx(gather=ctypes.pointer(gather_bits(out=None, out_bits=G3)))), "bad argument")
    refused(call_dx(dx(gather=ctypes.pointer(gather(corrupt=corrupt(), out_c=G4)))), "!a.corrupt || forward")


def test_weight_gradient_refuses_unreachable_block_combinations():
    h, f = ctypes.pointer(head_args()), ctypes.pointer(fold_args())
    refused(call_dw(dw(0, head=h), dw(1)), "not in a pair")
    refused(call_dw(dw(0), dw(1, head=h)), "not in a pair")
    refused(call_dw(dw(ones_from=4)), "need head")
    refused(call_dw(dw(fold=f)), "need head")
    refused(call_dw(dw(0), dw(1, ones_from=4)), "need head")
    refused(call_dw(dw(head=h, **XBITS)), "xbits needs fold")
    refused(call_dw(dw(**XBITS)), "xbits needs fold")
    refused(call_dw(dw(accumulate=1)), "accumulate")                        # with sched
    refused(call_dw(dw(adam=False, accumulate=1, head=h)), "accumulate")
    refused(call_dw(dw(0, adam=False, accumulate=1), dw(1)), "accumulate")
    refused(call_dw(dw(0), dw(1, adam=False, accumulate=1)), "accumulate")
    l1 = dict(z=G1, ldz=8, H=G2, ldh=8, rows=4)
    fin = ctypes.pointer(_lib.Finalize2Args(pa=G1, na=4, out_a=G2, pb=G3, nb=4, out_b=G4, done=H2))
    refused(call_dw(dw(0), None, _lib.DwTail(**l1)), "gm_dw_tail")          # a tail without a pair
    refused(call_dw(dw(0), None, _lib.DwTail(fin=fin)), "gm_dw_tail")
    refused(call_dw(dw(0), dw(1), _lib.DwTail(fin=fin, **l1)), "gm_dw_tail")   # both riders
    refused(call_dw(dw(0), dw(1), _lib.DwTail()), "gm_dw_tail")             # neither


# ---- (2) the argument checks of the launches the descriptors carry --------------------------------------------------
def test_forward_checks_every_block():
    base = [dict(X=None), dict(W=None), dict(Y=None), dict(M=0), dict(K=0), dict(N=0), dict(ldx=4), dict(ldy=4),
            dict(act=-1), dict(act=3)]
    for blk in (None,) + tuple(FWD_BLOCKS):
        for bad in base:
            if blk == "sqerr" and "act" in bad:
                continue
            refused(call_fwd(fwd(*([blk] if blk else []), **bad)), "bad argument")
    for bad in (dict(ip_eps=None), dict(ip_x=None), dict(ip_out=None), dict(ip_rows=0), dict(ip_rows=33),
                dict(ip_ldx=4), dict(ip_ldo=4)):
        refused(call_fwd(fwd("interp", **bad)), "a.ip_eps && a.ip_x")
    for bad in (dict(hd_w2=None), dict(hd_b2=None), dict(hd_part=None), dict(hd_snap=None), dict(hd_ldp=0),
                dict(hd_ldp=6), dict(N=40, ldy=40, hd_ldp=1)):
        refused(call_fwd(fwd("head", **bad)), "a.hd_w2 && a.hd_b2")
    for bad in (dict(hd_part=Y), dict(hd_snap=Y), dict(hd_part=X), dict(hd_snap=X)):
        refused(call_fwd(fwd("head", **bad)), "a.hd_part != a.Y")
    for bad in (dict(xbits_rows=0), dict(xbits_rows=64), dict(xbits_rows=16), dict(xbits_wpr=0), dict(K=6)):
        refused(call_fwd(fwd("head", **dict(XBITS, **bad))), "a.xbits_rows > 0")
    for bad in (dict(xbits=Y), dict(xbits=C)):
        refused(call_fwd(fwd("head", **dict(XBITS, **bad))), "a.xbits != (const void*)a.Y")
    for bad in (dict(sq_target=None), dict(sq_dA=None), dict(sq_part=None), dict(sq_ldt=4), dict(sq_lda=4),
                dict(sq_ldp=0)):
        refused(call_fwd(fwd("sqerr", **bad)), "a.sq_target && a.sq_dA")
    for bad in (dict(sq_dA=Y), dict(sq_part=Y), dict(sq_part=B_), dict(sq_dA=X), dict(sq_part=X), dict(sq_target=Y),
                dict(sq_dA=A)):
        refused(call_fwd(fwd("sqerr", **bad)), "a.sq_dA != a.Y")
    for bad in (dict(lb_E=None), dict(lb=_lib.LabelSrc(None, None, _lib.NO_SLOT)), dict(lb_C=0), dict(lb_C=33)):
        refused(call_fwd(fwd("label", **bad)), "a.lb_E && a.lb.labels")


def test_gather_block_checks():
    def ride(g):
        return call_fwd(fwd(gather=ctypes.pointer(g)))
    refused(ride(gather(bits=G4)), "!a.data != !a.bits")
    refused(ride(gather(data=None)), "!a.data != !a.bits")
    refused(ride(gather(out_bits=G4)), "!a.out != !a.out_bits")
    refused(ride(gather(out=None)), "!a.out != !a.out_bits")
    refused(ride(gather(out=None, out_bits=G4)), "!a.out_bits ||")          # packed rows come from the packed dataset
    for bad in (dict(idx=None), dict(B=0), dict(row_elems=0), dict(ld_out=4), dict(n_rows=0)):
        refused(ride(gather(**bad)), "idx && out && B > 0")
        refused(ride(gather_bits(**bad)), "idx && out && B > 0")
    refused(ride(gather_bits(row_elems=40, ld_out=40)), "words_per_row * 32 >= row_elems")
    for bad in (dict(idx=None), dict(B=0), dict(words_per_row=0), dict(n_rows=0), dict(out_bits=G1)):
        refused(ride(gather_bits(**dict(dict(out=None, out_bits=G3), **bad))), "idx && out_bits && B > 0")
    for g in (gather, gather_bits):
        refused(ride(g(out=Y)), "gout != a.Y")
        refused(ride(g(out=X)), "gout != a.Y")
    refused(ride(gather_bits(out=None, out_bits=Y)), "gout != a.Y")
    refused(ride(gather_bits(out=None, out_bits=X)), "gout != a.Y")
    for oc in (Y, X):
        refused(ride(gather(corrupt=corrupt(), out_c=oc)), "c.out_c != a.Y")
    refused(ride(gather(corrupt=corrupt(), out_c=G3)), "out_c != g->out")
    refused(ride(gather_bits(out=None, out_bits=G3, corrupt=corrupt(), out_c=G4)), "!g->out_bits")
    # the input gradient's: the gathered rows are none of dA, W, dX, below
    for out in (None, A, W, X, B_):
        refused(call_dx(dx(below=B_, ld_below=8, epi=1, gather=ctypes.pointer(gather(out=out)))), "out && out != a.dA")
    refused(call_dx(dx(gather=ctypes.pointer(gather(ld_out=4)))), "idx && out && B > 0")


def test_input_gradient_checks_every_block():
    base = [dict(dA=None), dict(W=None), dict(dX=None), dict(M=0), dict(K=0), dict(N=0), dict(lda=4), dict(ldx=4)]
    for blk in (None, "add", "reparam", "gather"):
        for bad in base:
            refused(call_dx(dx(**dict(DX_BLOCKS[blk]() if blk else {}, **bad))), "bad argument: a.dA && a.W && a.dX")
    refused(call_dx(dx(epi=1)), "a.epi == GM_ACT_ID ||")
    refused(call_dx(dx(epi=1, below=B_, ld_below=4)), "a.epi == GM_ACT_ID ||")
    refused(call_dx(dx(add=B_, ldadd=4)), "a.ldadd >= a.K")
    for k in ("H", "dS", "rowloss", "dH"):
        refused(call_dx(dx(head=ctypes.pointer(head_args(**{k: X})))), "a.dX != a.head->H")
    refused(call_dx(dx(head=ctypes.pointer(head_args(gen_mode=1, H=None)))), "a.H && a.w2 && a.loss_out")
    refused(call_dx(dx(head=ctypes.pointer(head_args(gen_mode=1, dS=None)))), "fold || (a.dS && a.rowloss)")
    # folded: dA is the hidden layer the head reads, in generator mode
    ok = dict(gen_mode=1, H=A, B=32, Hd=8)
    f = ctypes.pointer(fold_args())
    for bad in (dict(gen_mode=0), dict(H=H1), dict(B=16), dict(Hd=4)):
        refused(call_dx(dx(head=ctypes.pointer(head_args(**dict(ok, **bad))), fold=f)), "a.head->gen_mode && a.head->H == a.dA")
    h = ctypes.pointer(head_args(**ok))
    refused(call_dx(dx(dX=A, head=h, fold=f)), "a.dX != a.dA")
    for k in ("S", "dS", "rowloss"):
        refused(call_dx(dx(head=h, fold=ctypes.pointer(fold_args(**{k: X})))), "a.dX != a.fold->S")
    refused(call_dx(dx(head=h, fold=ctypes.pointer(fold_args(ldp=5)))), "g.ldp % 4 == 0")
    rp = DX_BLOCKS["reparam"]()
    for bad in (dict(rp_ml=None), dict(rp_eps=None), dict(rp_dml=None), dict(rp_ldml=8), dict(rp_ldd=8), dict(rp_dml=X),
                dict(rp_dml=B_), dict(rp_dml=A)):
        refused(call_dx(dx(**dict(rp, **bad))), "a.rp_ml && a.rp_eps && a.rp_dml")


def test_weight_gradient_checks_every_rider():
    base = [dict(dA=None), dict(X=None), dict(dW=None), dict(M=0), dict(K=0), dict(N=0), dict(lda=4), dict(ldx=4)]
    for bad in base:
        refused(call_dw(dw(**bad)), "a.dA && a.X && a.dW")
        refused(call_dw(dw(0), dw(1, **bad)), "a.dA && a.X && a.dW")
    for k in ("db", "pW", "mW", "vW", "pb", "mb", "vb"):       # an optimizer step needs all of its arrays
        refused(call_dw(dw(**{k: None})), "a.db && a.pW && a.mW")
        refused(call_dw(dw(0), dw(1, **{k: None})), "a.db && a.pW && a.mW")
        refused(call_dw(dw(head=ctypes.pointer(head_args()), **{k: None})), "!a.sched ||")
    # the riding head
    a = dw()
    refused(call_dw(_set(a, head=ctypes.pointer(head_args(w2=a.pW)))), "a.head->w2 != a.pW")
    refused(call_dw(_set(a, head=ctypes.pointer(head_args(gw2=a.dW)))), "a.head->gw2 != a.dW")
    refused(call_dw(dw(head=ctypes.pointer(head_args(loss_out=None)))), "a.H && a.w2 && a.loss_out")
    for n in (-1, 33):
        refused(call_dw(dw(head=ctypes.pointer(head_args()), ones_from=n)), "a.ones_from >= 0 && a.ones_from <= a.M")
    refused(call_dw(dw(ones_from=-1)), "a.ones_from >= 0 && a.ones_from <= a.M")
    # the folded head
    for bad in (dict(gen_mode=1), dict(H=H2), dict(B=8), dict(Hd=4)):
        a, h, f = dw_head()
        refused(call_dw(_set(a, head=ctypes.pointer(_set(h, **bad)), fold=ctypes.pointer(f))), "!a.head->gen_mode && a.head->H == a.dA")
    a, h, f = dw_head()
    refused(call_dw(_set(a, dW=a.dA, head=ctypes.pointer(h), fold=ctypes.pointer(f))), "a.dW != a.dA")
    a, h, f = dw_head()
    refused(call_dw(_set(a, ones_from=4, head=ctypes.pointer(h), fold=ctypes.pointer(f))), "a.ones_from == 0")
    for k in ("w2", "b2"):
        a, h, f = dw_head()
        refused(call_dw(_set(a, head=ctypes.pointer(h), fold=ctypes.pointer(_set(f, snap=getattr(h, k))))), "a.fold->snap !=")
    for bad in (dict(xbits_rows=0), dict(xbits_rows=64), dict(xbits_rows=16), dict(xbits_wpr=0), dict(K=6)):
        a, h, f = dw_head(**dict(XBITS, **bad))
        refused(call_dw(_set(a, head=ctypes.pointer(h), fold=ctypes.pointer(f))), "a.xbits_rows > 0")
    for k in ("dW", "pW"):
        a, h, f = dw_head(**XBITS)
        refused(call_dw(_set(a, xbits=getattr(a, k), head=ctypes.pointer(h), fold=ctypes.pointer(f))), "a.xbits != (const void*)a.dW")
    a, h, f = dw_head()
    refused(call_dw(_set(a, head=ctypes.pointer(h), fold=ctypes.pointer(_set(f, nparts=2)))), "g.nparts == (a.Hd + 31) / 32")


def test_pair_checks():
    a, b = dw(0), dw(1)
    # neither GEMM may consume what the other produces or updates
    refused(call_dw(a, dw(1, dW=a.dW)), "a.dW != b.dW")
    refused(call_dw(a, dw(1, pW=a.pW)), "a.dW != b.dW")
    for k in ("dA", "X"):
        refused(call_dw(a, dw(1, **{k: a.pW})), "!a.pW ||")
        refused(call_dw(dw(0, **{k: b.pW}), b), "!b.pW ||")
        refused(call_dw(a, dw(1, **{k: a.dW})), "a.dW != b.dA")
        refused(call_dw(dw(0, **{k: b.dW}), b), "a.dW != b.dA")
    # the next iteration's first layer riding on the pair
    l1 = dict(z=G1, ldz=8, H=G2, ldh=8, rows=4)
    refused(call_dw(a, dw(1, adam=False), _lib.DwTail(**l1)), "b.sched && tail->z")
    for bad in (dict(z=None), dict(H=None), dict(rows=0), dict(ldz=4), dict(ldh=4)):
        refused(call_dw(a, b, _lib.DwTail(**dict(l1, **bad))), "b.sched && tail->z")
    for g in (a, b):
        for k in ("dA", "X", "dW", "db", "pW", "pb"):
            refused(call_dw(a, b, _lib.DwTail(**dict(l1, H=getattr(g, k)))), "q != (const void*)tail->H")
    refused(call_dw(a, b, _lib.DwTail(**dict(l1, H=G1))), "tail->z != (const void*)tail->H")
    # the two loss sums riding on the pair
    fin = dict(pa=G1, na=4, out_a=G2, pb=G3, nb=4, out_b=G4, done=H2)
    for bad in (dict(pa=None), dict(pb=None), dict(out_a=None), dict(out_b=None), dict(na=0), dict(nb=0),
                dict(done=None)):
        f = ctypes.pointer(_lib.Finalize2Args(**dict(fin, **bad)))
        refused(call_dw(a, b, _lib.DwTail(fin=f)), "fin->pa && fin->pb")
    # ... and a tail does not switch the pair's own checks off
    refused(call_dw(a, dw(1, dW=a.dW), _lib.DwTail(**l1)), "a.dW != b.dW")
    refused(call_dw(a, dw(1, dW=a.dW), _lib.DwTail(fin=ctypes.pointer(_lib.Finalize2Args(**fin)))), "a.dW != b.dW")
