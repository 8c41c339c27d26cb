"""Every loss variant on every kernel that evaluates `sample_terms` (csrc/gm_common.h) or the two-phase RaGAN / Fisher
prologue, against ONE reference (tests/loss_tail_reference.py: staged fp64 + fp32 torch CPU), on rows of two bands --
ordinary (|a2| <= 6) and saturated (a2 >= 20, -40 .. -20, <= -110; raw scores: 20 <= |a2| <= 30) -- and at the widths and
row counts where each kernel takes another path:

  a. ops.gan_loss (gan_loss_kernel, gm_ops.hip)                 -- scores given, exact edge values
  b. of.head_fwd_loss + of.head_bwd (gm_fused.hip, gm_head.h)   -- head_row<VEC4> widths 4 / 260 / 512, scalar 37 / 516
  c. folded critic step (fold_row in the weight-gradient launch) -- 1 / 2 / 16 partial dots, R = 528 tail loop
  d. two-phase folded critic step (fold_fill_lds_tp)            -- RaGAN, Fisher; second register lane, R = 2048 limit
  e. folded generator step (fold_row in the input-gradient launch)

Criterion: the project's close64 (tests/linear_path_cases.py) per output array -- HIP error against the staged fp64 value
<= 2 x the fp32-CPU error + 1 ulp of the array's scale -- applied SEPARATELY to the saturated and the ordinary rows of
the per-row arrays, so that a row of magnitude 1e13 cannot hide an error on a row of magnitude 1.  Scalars that are sums
with cancellation (the loss, gb2) are scaled by the sum of the magnitudes of their terms.  Device logf / expf / tanhf are
specified to a few ulps while the fp32 CPU error can be 0, so an error above the close64 bound but within 4 fp32 ulps of
the group's scale passes as `floor`; profiles/head_variant_errors.md records the measured errors per kernel, key and
band and names every group that needed the floor.  With GM_HEAD_VARIANT_LOG=<file> every comparison appends a line
there (kernel, key, mode, act, shape, output, band, e_hip, e_cpu, scale, verdict).

The inputs (loss_tail_reference.banded_case) make X W1^T + b1 and h . w2 + b2 exact in fp32 in any summation order, so
all three evaluations start the loss tail from the same pre-activation, bit for bit: what is compared is the tail."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import loss_tail_reference as ltr  # noqa: E402
from generative_models_amd import ops  # noqa: E402
from generative_models_amd import ops_fused as of  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402
from linear_path_cases import errors64  # noqa: E402

DEV = "cuda:0"
ULP = 2.0 ** -23
FLOOR = 4 * ULP
LOG = os.environ.get("GM_HEAD_VARIANT_LOG")
# the output activation(s) each loss runs on: the trainers' own pairing (sigmoid critic; WGAN-GP: relu) and the raw score
HEAD_ACTS = {"ns": ("sigmoid",), "mm": ("sigmoid",), "ra": ("sigmoid",), "fisher": ("sigmoid",),
             "w": ("sigmoid", "relu", "id"), "ls": ("sigmoid", "id")}
HEAD_ACTS.update({k: ("sigmoid", "id") for k in ltr.F_KEYS})
SEPARABLE = tuple(k for k in ltr.KEYS if k not in ltr.TWO_PHASE)
LR, SCHED_ROW = 2e-4, 2


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """A launch that faulted leaves the process without a usable device: end the session instead of launching more."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                                   # pragma: no cover
        pytest.exit("device fault: %s" % e, returncode=3)


class Judge:
    """close64 per group, every figure logged before anything is asserted; done() raises with all misses of the test."""

    def __init__(self, kernel, key, mode, act, shape):
        self.tag = (kernel, key, "G" if mode else "D", act, "x".join(str(s) for s in shape))
        self.fails = []

    def check(self, what, got, ref64, ref32, band="all", scale=None):
        got = torch.as_tensor(got).detach().cpu().double().reshape(-1)
        r64 = torch.as_tensor(ref64).detach().cpu().double().reshape(-1)
        r32 = torch.as_tensor(ref32).detach().cpu().double().reshape(-1)
        assert got.shape == r64.shape == r32.shape, what
        if not bool(torch.isfinite(got).all()):
            self.fails.append("%s [%s]: not finite" % (what, band))
            return
        e_hip, e_cpu, bound, own = errors64(got, r64, r32)
        if scale is not None:                                    # a sum with cancellation: scaled by sum |term|
            scale = max(float(scale), own)
            e_hip, e_cpu = e_hip * own / scale, e_cpu * own / scale
            bound = 2.0 * e_cpu + ULP
        else:
            scale = own
        verdict = "close64" if e_hip <= bound else "floor" if e_hip <= FLOOR else "FAIL"
        line = "\t".join(self.tag + (what, band, "%.3e" % e_hip, "%.3e" % e_cpu, "%.3e" % scale, verdict))
        if LOG:
            with open(LOG, "a") as f:
                f.write(line + "\n")
        else:
            print(line)
        if verdict == "FAIL":
            self.fails.append("%s [%s]: HIP err %.3e > 2 x CPU fp32 err %.3e + 1 ulp and > 4 ulp; scale %.3e"
                              % (what, band, e_hip, e_cpu, scale))

    def rows(self, what, got, ref64, ref32, sat):
        """A per-row array ([R] or [R, n]): the saturated and the ordinary rows as groups of their own."""
        got = got.detach().cpu()
        for band, m in (("saturated", sat), ("ordinary", ~sat)):
            if bool(m.any()):
                self.check(what, got[m], ref64[m], ref32[m], band)

    def exact_zeros(self, dS, r64, r32, out_act):
        """Where the fp32 score is exactly 0 or 1, a sigmoid's gradient is exactly zero; and wherever both references
        have no gradient at all (a rectified score of 0), neither has the kernel."""
        dS = dS.detach().cpu()
        dead = (r64["dS"] == 0) & (r32["dS"] == 0)
        if out_act == "sigmoid":
            flat = (r64["S"] == 0) | (r64["S"] == 1)
            assert bool((r64["dS"][flat] == 0).all())
            dead = dead | flat
        if not bool((dS[dead] == 0).all()):
            self.fails.append("dS is not exactly zero on %d rows without gradient" % int((dS[dead] != 0).sum()))

    def done(self):
        assert not self.fails, "%s:\n  %s" % (" ".join(self.tag), "\n  ".join(self.fails))


@functools.lru_cache(maxsize=None)
def case(B, I, Hd, out_act, gen_mode):
    return ltr.banded_case(B, I, Hd, out_act, gen_mode, 1000 * B + Hd + (7 if gen_mode else 0))


def dev(t):
    return t.to(DEV).contiguous()


def lam_of(key):
    return ltr.FISHER_LAMBDA if key == "fisher" else None


def fisher_aux():
    return torch.tensor([ltr.FISHER_LAMBDA, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0, 9.0], device=DEV)


# ---- a. ops.gan_loss --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 257, 2049])
@pytest.mark.parametrize("key", ltr.KEYS)
def test_gan_loss_on_exact_edge_scores(key, B):
    """One row, less than a wave, one past the workgroup's stride (256), many strides."""
    hyper = ltr.hyper_of(key)
    for out_act in ltr.ACTS[key]:
        for gen_mode in (False, True):
            R = B if gen_mode else 2 * B
            scores, sat = ltr.exact_scores(B, out_act, gen_mode, B + len(key))
            two_phase = key in ltr.TWO_PHASE and not gen_mode
            r64, r32 = ltr.tail(key, gen_mode, B, out_act, hyper, scores=scores, lam=lam_of(key))
            s = dev(scores)
            loss = torch.full((3,), 7.0, device=DEV)
            d = torch.full((R,), 7.0, device=DEV)
            db = torch.full((1,), 7.0, device=DEV)
            aux = fisher_aux() if key == "fisher" and not gen_mode else None
            ops.gan_loss(key, gen_mode, None if gen_mode else s[:B], s[B:] if not gen_mode else s, B, out_act, loss,
                         None if gen_mode else d[:B], d[B:] if not gen_mode else d, hyper=hyper,
                         loss_slot=ops.slot(0, 0, 1, 0, 1), aux=aux, db=db)
            torch.cuda.synchronize()
            j = Judge("gan_loss", key, gen_mode, out_act, (B,))
            assert loss[0].item() == 7.0 and loss[2].item() == 7.0
            j.check("loss", loss[1], r64["loss"], r32["loss"], scale=r64["loss_abs"])
            j.rows("dS", d, r64["dS"], r32["dS"], sat)
            j.exact_zeros(d, r64, r32, out_act)
            j.check("db", db, r64["gb2"], r32["gb2"], scale=r64["gb2_abs"])
            if two_phase and key == "fisher":
                j.check("moments", aux[1:5], r64["moments"], r32["moments"])
                j.check("lambda", aux[0], r64["lam_next"], r32["lam_next"])
                assert bool((aux[5:] == 9.0).all())
            j.done()


# ---- b. head_fwd_loss + head_bwd --------------------------------------------------------------------------------------
HEAD_SHAPES = [(3, 4), (24, 37), (40, 260), (33, 512), (17, 516)]
HEAD_I = 12


def run_head(key, gen_mode, out_act, B, Hd, c, j, pen=None, hyper=None, pad=0):
    """The pair against the reference; dH from head_fwd_loss (dH=) and from head_bwd must agree bit for bit.
    pad: H and dH are views of arrays that many columns wider."""
    R = B if gen_mode else 2 * B
    hyper = ltr.hyper_of(key) if hyper is None else hyper
    r64, r32 = ltr.tail(key, gen_mode, B, out_act, hyper, H=c["H"], w2=c["w2"], b2=c["b2"], pen=pen)
    assert torch.equal(r64["a2"], c["a2"]) and torch.equal(r32["a2"].double(), c["a2"])
    assert torch.equal(ltr.check_bands(r64["a2"], out_act, B, gen_mode), c["sat"])
    Hfull = torch.full((R, Hd + pad), -3.0, device=DEV)
    H = Hfull[:, :Hd]
    H.copy_(c["H"])
    w2, b2 = dev(c["w2"]), dev(c["b2"])
    S, dS, rl = (torch.full((R,), 7.0, device=DEV) for _ in range(3))
    dHfull = torch.full((R, Hd + pad), 7.0, device=DEV)
    dH = dHfull[:, :Hd]
    gw2, gb2 = torch.full((1, Hd), 7.0, device=DEV), torch.full((1,), 7.0, device=DEV)
    out = torch.full((1,), 7.0, device=DEV)
    pend = dev(pen) if pen is not None else None
    of.head_fwd_loss(key, gen_mode, H, w2, b2, out_act, B, hyper, 1.0 / B, pend, S, dS, rl, dH=dH)
    of.head_bwd(H, dS, w2, rl, None, None if gen_mode else gw2, None if gen_mode else gb2, out, ops.NO_SLOT, 1.0 / B,
                gen_mode, B)
    torch.cuda.synchronize()
    sat = c["sat"]
    j.rows("S", S, r64["S"], r32["S"], sat)
    j.rows("dS", dS, r64["dS"], r32["dS"], sat)
    j.rows("rowloss", rl, r64["rows"], r32["rows"], sat)
    j.rows("dH", dH, r64["dH"], r32["dH"], sat)
    j.exact_zeros(dS, r64, r32, out_act)
    j.check("loss", out, r64["loss"], r32["loss"], scale=r64["loss_abs"])
    if not gen_mode:
        j.check("gw2", gw2, r64["gw2"], r32["gw2"])
        j.check("gb2", gb2, r64["gb2"], r32["gb2"], scale=r64["gb2_abs"])
    if pad:
        assert bool((dHfull[:, Hd:] == 7.0).all()) and bool((Hfull[:, Hd:] == -3.0).all())
    S2, dS2, rl2 = (torch.full((R,), 5.0, device=DEV) for _ in range(3))
    dH2full = torch.full((R, Hd + pad), 5.0, device=DEV)
    dH2 = dH2full[:, :Hd]
    out2 = torch.full((1,), 5.0, device=DEV)
    of.head_fwd_loss(key, gen_mode, H, w2, b2, out_act, B, hyper, 1.0 / B, pend, S2, dS2, rl2)
    of.head_bwd(H, dS2, w2, rl2, dH2, None, None, out2, ops.NO_SLOT, 1.0 / B, gen_mode, B)
    torch.cuda.synchronize()
    for a, b, n in ((S, S2, "S"), (dS, dS2, "dS"), (rl, rl2, "rowloss"), (dH, dH2, "dH"), (out, out2, "loss")):
        assert torch.equal(a, b), "%s with and without dH=" % n
    if pad:
        assert bool((dH2full[:, Hd:] == 5.0).all())


@pytest.mark.parametrize("B,Hd", HEAD_SHAPES)
@pytest.mark.parametrize("key", ltr.KEYS)
def test_fused_head_pair_variants(key, B, Hd):
    """head_row<VEC4>: one float4 (4), second slot live in lane 0 only (260), last vector width (512); scalar path: 37
    and 516 (vector-eligible width past the vector path's limit)."""
    for out_act in HEAD_ACTS[key]:
        for gen_mode in ((True,) if key in ltr.TWO_PHASE else (False, True)):
            j = Judge("head_pair", key, gen_mode, out_act, (B, Hd))
            run_head(key, gen_mode, out_act, B, Hd, case(B, HEAD_I, Hd, out_act, gen_mode), j)
            j.done()


@pytest.mark.parametrize("key", ltr.TWO_PHASE)
def test_fused_head_refuses_the_two_phase_critic_losses(key):
    B, Hd = 3, 4
    c = case(B, HEAD_I, Hd, "sigmoid", False)
    S, dS, rl = (torch.full((2 * B,), 7.0, device=DEV) for _ in range(3))
    with pytest.raises(GMError):
        of.head_fwd_loss(key, False, dev(c["H"]), dev(c["w2"]), dev(c["b2"]), "sigmoid", B, ltr.hyper_of(key), 1.0 / B,
                         None, S, dS, rl)
    torch.cuda.synchronize()
    assert bool((S == 7.0).all()) and bool((dS == 7.0).all()) and bool((rl == 7.0).all())


@pytest.mark.parametrize("key,out_act,B,Hd", [("ns", "sigmoid", 24, 37), ("w", "relu", 40, 260)])
def test_fused_head_pair_with_penalty_rows(key, out_act, B, Hd):
    """hyper[7] * pen[r] on the x rows (DRAGAN on the NS loss, WGAN-GP on the rectified W loss)."""
    pen = torch.rand(B, generator=torch.Generator().manual_seed(B)) * 3.0
    hyper = tuple(ltr.hyper_of(key)) + (0.0,) * (7 - len(ltr.hyper_of(key))) + (10.0,)
    j = Judge("head_pair+pen", key, False, out_act, (B, Hd))
    run_head(key, False, out_act, B, Hd, case(B, HEAD_I, Hd, out_act, False), j, pen=pen, hyper=hyper)
    j.done()


@pytest.mark.parametrize("key,out_act,gen_mode,B,Hd,pad", [("mm", "sigmoid", False, 40, 260, 4),
                                                           ("f_hellinger", "id", True, 24, 37, 3),
                                                           ("f_jensen_shannon", "id", False, 33, 512, 8)])
def test_fused_head_pair_on_views_with_a_leading_dimension(key, out_act, gen_mode, B, Hd, pad):
    """H and dH as column slices of wider arrays: ld = Hd + 4 / + 8 keeps the vector path, + 3 takes the scalar one; the
    columns past Hd stay untouched."""
    j = Judge("head_pair+ld", key, gen_mode, out_act, (B, Hd))
    run_head(key, gen_mode, out_act, B, Hd, case(B, HEAD_I, Hd, out_act, gen_mode), j, pad=pad)
    j.done()


# ---- c / d. folded critic step ----------------------------------------------------------------------------------------
def critic_step(key, out_act, B, I, Hd, c, folded, aux=None, commit=False):
    """One critic step tail on the case's inputs: forward (+ partial dots), layer-1 weight gradient + Adam with the head
    riding (folded) or head_fwd_loss + the same launch reading dH (unfolded).  -> dict of device results + state before."""
    import torch.nn as nn
    from generative_models_amd.engine import FlatParams, _Linear
    net = nn.Sequential(nn.Linear(I, Hd), nn.Linear(Hd, 1))
    with torch.no_grad():
        net[0].weight.copy_(c["W1"]); net[0].bias.copy_(c["b1"]); net[1].weight.copy_(c["w2"]); net[1].bias.copy_(c["b2"])
    fp = FlatParams(net.parameters(), DEV)
    g = torch.Generator().manual_seed(11)
    fp.m.copy_(torch.randn(fp.n, generator=g) * 1e-3)
    fp.v.copy_(torch.rand(fp.n, generator=g) * 1e-4)
    before = dict(flat=fp.flat.clone(), m=fp.m.clone(), v=fp.v.clone())
    live = torch.zeros(fp.n, dtype=torch.bool)                 # the segments' padding belongs to no parameter
    for p, o in zip(fp.params, fp.offsets):
        live[o:o + p.numel()] = True
    L1, L2 = _Linear(fp, net[0]), _Linear(fp, net[1])
    X2 = dev(c["X"])
    H = torch.empty(2 * B, Hd, device=DEV)
    S, dS, rl = (torch.full((2 * B,), 7.0, device=DEV) for _ in range(3))
    loss = torch.full((1,), 7.0, device=DEV)
    sched = torch.from_numpy(ops.adam_schedule(LR, 4)).to(DEV)
    adam = dict(sched=sched, sched_slot=ops.slot(0, 0, SCHED_ROW, 0, 1), clamp=0.0)
    head = dict(H=H, lin=L2, loss_out=loss, loss_slot=ops.NO_SLOT, inv_b=1.0 / B, B=B, adam=adam)
    hyper = ltr.hyper_of(key)
    if folded:
        fold = ops.HeadFold(2 * B, Hd, DEV)
        ops.linear_fwd_headpart(X2, L1.W, L1.b, H, "relu", L2, fold)
        fa = fold.args(key, out_act, hyper, S=S, dS=dS, rowloss=rl, pen=aux)
        ops.linear_bwd_dw_adam_head_fold(H, X2, L1, adam, head, fa)
        aux_mid = aux.clone() if aux is not None else None
        if commit:
            of.fisher_commit(aux)
    else:
        aux_mid = None
        dH = torch.empty(2 * B, Hd, device=DEV)
        ops.linear_fwd(X2, L1.W, L1.b, H, "relu")
        of.head_fwd_loss(key, False, H, L2.W, L2.b, out_act, B, hyper, 1.0 / B, None, S, dS, rl, dH=dH)
        ops.linear_bwd_dw_adam_head(dH, X2, L1, adam, dict(head, dS=dS, rowloss=rl))
    torch.cuda.synchronize()
    return dict(flat=fp.flat.clone(), grad=fp.grad.clone(), m=fp.m.clone(), v=fp.v.clone(), loss=loss.clone(), S=S, dS=dS,
                rl=rl, H=H, views=[gv.clone() for gv in fp.gviews], before=before, live=live, sched=sched.cpu(), aux_mid=aux_mid,
                aux=aux.clone() if aux is not None else None)


def judge_critic_step(j, a, r64, r32, c, out_act, rows=True):
    sat = c["sat"]
    assert torch.equal(ltr.check_bands(r64["a2"], out_act, a["S"].numel() // 2, False), sat)
    assert torch.equal(a["H"].cpu(), c["H"]), "hidden layer: exact by construction"
    j.check("loss", a["loss"], r64["loss"], r32["loss"], scale=r64["loss_abs"])
    j.rows("S", a["S"], r64["S"], r32["S"], sat)
    j.rows("dS", a["dS"], r64["dS"], r32["dS"], sat)
    j.exact_zeros(a["dS"], r64, r32, out_act)
    if rows:
        j.rows("rowloss", a["rl"], r64["rows"], r32["rows"], sat)
    for got, n in zip(a["views"], ("gW1", "gb1", "gw2", "gb2")):
        j.check(n, got, r64[n], r32[n], scale=r64["gb2_abs"] if n == "gb2" else None)
    # Adam reads the gradient the launch stored: its own stage, from that fp32 gradient and the state before
    step, bc2 = float(a["sched"][SCHED_ROW, 0]), float(a["sched"][SCHED_ROW, 1])
    b, live = a["before"], a["live"]
    g = a["grad"].cpu()
    n64 = ltr.adam_step(b["flat"].cpu().double(), g, b["m"].cpu().double(), b["v"].cpu().double(), step, bc2)
    n32 = ltr.adam_step(b["flat"].cpu(), g, b["m"].cpu(), b["v"].cpu(), step, bc2)
    for k, x64, x32 in zip(("flat", "m", "v"), n64, n32):
        j.check("adam " + k, a[k].cpu()[live], x64[live], x32[live])
        assert torch.equal(a[k].cpu()[~live], b[k].cpu()[~live]), "padding of %s touched" % k


FOLD_KEYS = SEPARABLE
FOLD_SHAPES = [(24, 36, 20), (40, 36, 32), (100, 64, 48), (264, 36, 36), (24, 36, 512)]
STATE = ("grad", "flat", "m", "v", "loss", "S", "dS", "rl")


@pytest.mark.parametrize("B,I,Hd", FOLD_SHAPES)
@pytest.mark.parametrize("key", FOLD_KEYS)
def test_folded_critic_step_variants(key, B, I, Hd):
    """One partial dot per row (Hd <= 32), two with a ragged tile, R = 528 (the tail loop of head_bwd_body past 512 rows),
    sixteen partials: folded and unfolded against the reference, and the folded one bit for bit on a second run."""
    for out_act in HEAD_ACTS[key]:
        c = case(B, I, Hd, out_act, False)
        r64, r32 = ltr.tail(key, False, B, out_act, ltr.hyper_of(key), X=c["X"], W1=c["W1"], b1=c["b1"], w2=c["w2"],
                            b2=c["b2"])
        for folded in (True, False):
            a = critic_step(key, out_act, B, I, Hd, c, folded)
            j = Judge("fold_critic" if folded else "unfolded_critic", key, False, out_act, (B, I, Hd))
            judge_critic_step(j, a, r64, r32, c, out_act)
            j.done()
            if folded:
                a2 = critic_step(key, out_act, B, I, Hd, c, True)
                for k in STATE:
                    assert torch.equal(a[k], a2[k]), k + " on a second run"


TP_SHAPES = [(24, 36, 20), (264, 36, 36), (520, 36, 20), (1024, 36, 32)]


@pytest.mark.parametrize("B,I,Hd", TP_SHAPES)
@pytest.mark.parametrize("key", ltr.TWO_PHASE)
def test_two_phase_folded_critic_step(key, B, I, Hd):
    """fold_fill_lds_tp: R = 48; 528 (tail loop); 1040 (rows in the second register lane); 2048 (FOLD_MAX_ROWS)."""
    out_act = "sigmoid"
    c = case(B, I, Hd, out_act, False)
    lam = lam_of(key)
    r64, r32 = ltr.tail(key, False, B, out_act, ltr.hyper_of(key), X=c["X"], W1=c["W1"], b1=c["b1"], w2=c["w2"], b2=c["b2"],
                        lam=lam)
    fisher = key == "fisher"
    a = critic_step(key, out_act, B, I, Hd, c, True, aux=fisher_aux() if fisher else None, commit=fisher)
    j = Judge("fold_two_phase", key, False, out_act, (B, I, Hd))
    judge_critic_step(j, a, r64, r32, c, out_act, rows=False)
    assert bool((a["rl"] == 7.0).all()), "the two-phase launch writes no row losses"
    if fisher:
        mid, end = a["aux_mid"], a["aux"]
        assert mid[0].item() == fisher_aux()[0].item(), "lambda must not move before fisher_commit"
        j.check("moments", mid[1:5], r64["moments"], r32["moments"])
        j.check("lambda successor", mid[5], r64["lam_next"], r32["lam_next"])
        assert bool((mid[6:] == 9.0).all())
        assert end[0].item() == mid[5].item() and torch.equal(end[1:], mid[1:])
    # the one-workgroup loss kernel on the scores this launch stored: same formulas, other summation order
    S = a["S"]
    s64, s32 = ltr.tail(key, False, B, out_act, ltr.hyper_of(key), scores=S.cpu(), lam=lam)
    loss = torch.full((1,), 7.0, device=DEV)
    d = torch.full((2 * B,), 7.0, device=DEV)
    db = torch.full((1,), 7.0, device=DEV)
    aux = fisher_aux() if fisher else None
    ops.gan_loss(key, False, S[:B], S[B:], B, out_act, loss, d[:B], d[B:], hyper=ltr.hyper_of(key), aux=aux, db=db)
    torch.cuda.synchronize()
    for who, got in (("gan_loss", dict(loss=loss, dS=d, gb2=db)), ("two-phase", dict(loss=a["loss"], dS=a["dS"], gb2=a["views"][3]))):
        j.check(who + " loss on stored scores", got["loss"], s64["loss"], s32["loss"], scale=s64["loss_abs"])
        j.rows(who + " dS on stored scores", got["dS"], s64["dS"], s32["dS"], c["sat"])
        j.check(who + " gb2 on stored scores", got["gb2"], s64["gb2"], s32["gb2"], scale=s64["gb2_abs"])
    if fisher:
        j.check("gan_loss lambda on stored scores", aux[0], s64["lam_next"], s32["lam_next"])
        j.check("two-phase lambda on stored scores", a["aux_mid"][5], s64["lam_next"], s32["lam_next"])
    j.done()
    a2 = critic_step(key, out_act, B, I, Hd, c, True, aux=fisher_aux() if fisher else None, commit=fisher)
    for k in STATE:
        assert torch.equal(a[k], a2[k]), k + " on a second run"


@pytest.mark.parametrize("key", ltr.TWO_PHASE + ("ns",))
def test_folded_critic_step_refuses_more_rows_than_it_keeps(key):
    """2B = 2050 > FOLD_MAX_ROWS: GMError, and nothing is launched -- no output changes."""
    import torch.nn as nn
    from generative_models_amd.engine import FlatParams, _Linear
    B, I, Hd = 1025, 36, 20
    net = nn.Sequential(nn.Linear(I, Hd), nn.Linear(Hd, 1))
    fp = FlatParams(net.parameters(), DEV)
    L1, L2 = _Linear(fp, net[0]), _Linear(fp, net[1])
    X2 = torch.rand(2 * B, I, device=DEV)
    H = torch.empty(2 * B, Hd, device=DEV)
    S, dS, rl = (torch.full((2 * B,), 7.0, device=DEV) for _ in range(3))
    loss = torch.full((1,), 7.0, device=DEV)
    sched = torch.from_numpy(ops.adam_schedule(LR, 4)).to(DEV)
    adam = dict(sched=sched, sched_slot=ops.slot(0, 0, SCHED_ROW, 0, 1), clamp=0.0)
    head = dict(H=H, lin=L2, loss_out=loss, loss_slot=ops.NO_SLOT, inv_b=1.0 / B, B=B, adam=adam)
    fold = ops.HeadFold(2 * B, Hd, DEV)
    ops.linear_fwd_headpart(X2, L1.W, L1.b, H, "relu", L2, fold)
    aux = fisher_aux() if key == "fisher" else None
    fp.grad.fill_(7.0)
    torch.cuda.synchronize()
    state = [t.clone() for t in (fp.flat, fp.grad, fp.m, fp.v)]
    with pytest.raises(GMError):
        ops.linear_bwd_dw_adam_head_fold(H, X2, L1, adam, head,
                                         fold.args(key, "sigmoid", ltr.hyper_of(key), S=S, dS=dS, rowloss=rl, pen=aux))
    torch.cuda.synchronize()
    for t, t0 in zip((fp.flat, fp.grad, fp.m, fp.v), state):
        assert torch.equal(t, t0)
    assert loss.item() == 7.0 and all(bool((t == 7.0).all()) for t in (S, dS, rl))
    if aux is not None:
        assert torch.equal(aux, fisher_aux())


# ---- e. folded generator step -----------------------------------------------------------------------------------------
GEN_KEYS = ltr.KEYS
GEN_SHAPES = [(24, 36, 20), (33, 36, 36), (264, 36, 32)]


@pytest.mark.parametrize("B,I,Hd", GEN_SHAPES)
@pytest.mark.parametrize("key", GEN_KEYS)
def test_folded_generator_step_variants(key, B, I, Hd):
    """Forward + partial dots, then dX through layer 1 with the loss / tick workgroup riding: loss slot, one tick, dX
    (through the sigmoid gradient epilogue of the layer below), S, dS and the row losses."""
    from types import SimpleNamespace
    for out_act in HEAD_ACTS[key]:
        c = case(B, I, Hd, out_act, True)
        below = torch.rand(B, I, generator=torch.Generator().manual_seed(B + I))
        r64, r32 = ltr.tail(key, True, B, out_act, ltr.hyper_of(key), X=c["X"], W1=c["W1"], b1=c["b1"], w2=c["w2"],
                            b2=c["b2"], below=below)
        X, W1, b1 = dev(c["X"]), dev(c["W1"]), dev(c["b1"])
        L2 = SimpleNamespace(W=dev(c["w2"]), b=dev(c["b2"]))
        H = torch.empty(B, Hd, device=DEV)
        fold = ops.HeadFold(B, Hd, DEV)
        S, dS, rl = (torch.full((B,), 7.0, device=DEV) for _ in range(3))
        ctr = torch.ones(1, dtype=torch.int64, device=DEV)
        loss = torch.full((3,), 7.0, device=DEV)
        dX = torch.full((B, I), 7.0, device=DEV)
        ops.linear_fwd_headpart(X, W1, b1, H, "relu", L2, fold)
        ops.linear_bwd_dx_head_fold(H, W1, dX, dict(H=H, lin=L2, loss_out=loss, loss_slot=ops.slot(ctr.data_ptr(), 1, 0, 3, 1),
                                                    inv_b=1.0 / B, B=B, gen_mode=True, tick=ctr),
                                    fold.args(key, out_act, ltr.hyper_of(key), S=S, dS=dS, rowloss=rl), below=dev(below),
                                    epi="sigmoid")
        torch.cuda.synchronize()
        assert ctr.item() == 2, "one tick"
        assert loss[0].item() == 7.0 and loss[2].item() == 7.0
        assert torch.equal(H.cpu(), c["H"])
        j = Judge("fold_generator", key, True, out_act, (B, I, Hd))
        sat = c["sat"]
        assert torch.equal(ltr.check_bands(r64["a2"], out_act, B, True), sat)
        j.check("loss", loss[1], r64["loss"], r32["loss"], scale=r64["loss_abs"])
        j.rows("S", S, r64["S"], r32["S"], sat)
        j.rows("dS", dS, r64["dS"], r32["dS"], sat)
        j.rows("rowloss", rl, r64["rows"], r32["rows"], sat)
        j.rows("dX", dX, r64["dX"], r32["dX"], sat)
        j.exact_zeros(dS, r64, r32, out_act)
        j.done()
