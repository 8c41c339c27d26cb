"""The strided-set feed of the x-contiguous GEMM operands (csrc/gm_gemm.hip, raw_xs): bit for bit what the scalar operand
path computes.  The host picks the 16-byte operand paths by alignment, so the same operands one float off a 16-byte
boundary take the scalar path (XV = false), which the project documents as bit-identical."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from generative_models_amd import ops  # noqa: E402

DEV = "cuda"
ROWS = [1, 15, 16, 17, 33, 64]                     # partial chunk, one chunk per wave, waves with no chunk
LAYERS = [(4, 4), (16, 47), (33, 49), (48, 32), (100, 97)]     # [N, K]; every weight gradient carries the ones column (db)


def _off1(t):
    """The same values one float off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _lin(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return SimpleNamespace(W=r(n, k) * 0.1, b=r(n) * 0.1, gW=torch.zeros(n, k, device=DEV),
                           gb=torch.zeros(n, device=DEV), mW=r(n, k).abs() * 0.01, vW=r(n, k).abs() * 0.001,
                           mb=r(n).abs() * 0.01, vb=r(n).abs() * 0.001)


def _clone(lin):
    return SimpleNamespace(**{k: v.clone() for k, v in vars(lin).items()})


def _same(a, b, what):
    for k in vars(a):
        assert torch.equal(getattr(a, k), getattr(b, k)), (what, k)


def _adam():
    sched = torch.tensor([1e-3, 0.9, 2e-3, 0.8], device=DEV)
    return dict(sched=sched, sched_slot=ops.slot(0, 0, 1, 0, 1))     # the schedule's second entry


def _operands(R, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, N, generator=g).to(DEV), torch.randn(R, K, generator=g).to(DEV)


@pytest.mark.parametrize("N,K", LAYERS)
def test_dw_aligned_equals_misaligned(N, K):
    """ops.linear_bwd_dw and linear_bwd_dw_adam: dW, db and the stepped p / m / v."""
    adam = _adam()
    for R in ROWS:
        dA, X = _operands(R, N, K, 7 * R + N + K)
        lin = _lin(N, K, R + N)
        got = []
        for a, x in ((dA, X), (_off1(dA), _off1(X))):
            l0, l1 = _clone(lin), _clone(lin)
            ops.linear_bwd_dw(a, x, l0.gW, l0.gb)
            ops.linear_bwd_dw_adam(a, x, l1, adam)
            torch.cuda.synchronize()
            got.append((l0, l1))
        _same(got[0][0], got[1][0], ("dw", R, N, K))
        _same(got[0][1], got[1][1], ("dw_adam", R, N, K))
        assert not torch.equal(got[0][1].W, lin.W)


@pytest.mark.parametrize("N,K", LAYERS)
def test_dw_pair_aligned_equals_misaligned(N, K):
    """ops.linear_bwd_dw_adam_pair: this layer and a second one over the same rows."""
    adam = _adam()
    N2, K2 = 48, 32
    for R in ROWS:
        dA, X = _operands(R, N, K, 3 * R + N + K)
        dB, Y = _operands(R, N2, K2, 5 * R + N)
        la, lb = _lin(N, K, R + 1), _lin(N2, K2, R + 2)
        got = []
        for f in (lambda t: t, _off1):
            a, b = _clone(la), _clone(lb)
            ops.linear_bwd_dw_adam_pair(dict(dA=f(dA), X=f(X), lin=a, adam=adam), dict(dA=f(dB), X=f(Y), lin=b, adam=adam))
            torch.cuda.synchronize()
            got.append((a, b))
        _same(got[0][0], got[1][0], ("pair first", R, N, K))
        _same(got[0][1], got[1][1], ("pair second", R, N, K))


def test_dw_pair_with_layer1_rider():
    """[N, K] = (400, 20) at R = 256 behind a 784 x 400 layer: the pair kernel with its layer-1 rider, against the pair
    launch followed by the k32 forward, and against the pair on misaligned operands."""
    B, hid, Z, rows, I = 256, 400, 20, 512, 784
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    G2, G1 = _lin(I, hid, 1), _lin(hid, Z, 2)
    dXg, Hg2, dHg = r(B, I), torch.relu(r(B, hid)), r(B, hid)
    zring = r(3 * rows * Z)
    zbase = zring.view(-1, Z)
    ctr = torch.tensor([1], dtype=torch.int64, device=DEV)
    S = rows * Z
    x_slot = ops.slot(ctr.data_ptr(), 1, -1, 3, S)
    z_slot = ops.slot(ctr.data_ptr(), 1, 0, 3, S)
    adam = dict(sched=torch.tensor([1e-3, 0.9, 2e-3, 0.8], device=DEV), sched_slot=ops.slot(ctr.data_ptr(), 1, 0, 2, 1))
    out = {}
    for form in ("ref", "ride", "scalar"):
        g2, g1 = _clone(G2), _clone(G1)
        f = _off1 if form == "scalar" else (lambda t: t)
        first = dict(dA=f(dXg), X=f(Hg2), lin=g2, adam=adam, M=B)
        second = dict(dA=f(dHg), X=zbase, lin=g1, adam=adam, M=B, x_slot=x_slot)
        H = torch.full((rows, hid), -7.0, device=DEV)
        if form == "ride":
            ops.linear_bwd_dw_adam_pair_l1(first, second, zbase, H, rows, z_slot=z_slot)
        else:
            ops.linear_bwd_dw_adam_pair(first, second)
            ops.linear_fwd(zbase, g1.W, g1.b, H, "relu", M=rows, x_slot=z_slot)
        torch.cuda.synchronize()
        out[form] = (H, g2, g1)
    for form in ("ride", "scalar"):
        assert torch.equal(out["ref"][0], out[form][0]), form
        _same(out["ref"][1], out[form][1], form + " layer 2")
        _same(out["ref"][2], out[form][2], form + " layer 1")
    assert bool((out["ride"][0] != -7.0).all())


@pytest.mark.parametrize("epi", ["relu", "sigmoid"])
@pytest.mark.parametrize("N,K", LAYERS + [(400, 784)])
def test_dx_aligned_equals_misaligned(N, K, epi):
    """ops.linear_bwd_dx: W aligned (16-byte operand path) against W one float off (scalar path)."""
    for M in ([32] if N == 400 else ROWS):
        g = torch.Generator().manual_seed(M + N + K)
        dA = torch.randn(M, N, generator=g).to(DEV)
        W = torch.randn(N, K, generator=g).to(DEV)
        below = torch.rand(M, K, generator=g).to(DEV)
        a, b = torch.empty(M, K, device=DEV), torch.empty(M, K, device=DEV)
        ops.linear_bwd_dx(dA, W, a, below=below, epi=epi)
        ops.linear_bwd_dx(dA, _off1(W), b, below=below, epi=epi)
        torch.cuda.synchronize()
        assert torch.equal(a, b), (M, N, K, epi)
        assert bool(a.abs().sum() > 0)


def test_dx_gather_rider_equals_scalar_path():
    """The input gradient carrying the batch gather (16-byte path) against the plain launch on a misaligned W."""
    B, Hd, I = 64, 48, 36
    g = torch.Generator().manual_seed(5)
    dA = torch.randn(B, I, generator=g).to(DEV)
    W = torch.randn(I, Hd, generator=g).to(DEV)
    below = torch.relu(torch.randn(B, Hd, generator=g)).to(DEV)
    imgs = (torch.rand(200, I, generator=g) > 0.5).float().to(DEV)
    idx = torch.randint(0, 200, (B,), generator=g).to(DEV)
    out = torch.full((B, I), -1.0, device=DEV)
    dX, ref = torch.empty(B, Hd, device=DEV), torch.empty(B, Hd, device=DEV)
    ops.linear_bwd_dx_gather(dA, W, dX, imgs, idx, out, below=below, epi="relu")
    ops.linear_bwd_dx(dA, _off1(W), ref, below=below, epi="relu")
    torch.cuda.synchronize()
    assert torch.equal(dX, ref) and torch.equal(out, imgs[idx])


def _fold_setup(R, I, Hd, seed):
    import torch.nn as nn
    from generative_models_amd.engine import FlatParams, _Linear
    torch.manual_seed(seed)
    net = nn.Sequential(nn.Linear(I, Hd), nn.Linear(Hd, 1))
    fp = FlatParams(net.parameters(), DEV)
    fp.m.normal_().mul_(1e-3); fp.v.uniform_(0.0, 1e-4)
    return fp, _Linear(fp, net[0]), _Linear(fp, net[1])


def test_folded_dw_equals_unfolded_launch():
    """ops.linear_bwd_dw_adam_head_fold at R = 64, hidden 48, against the unfolded launch (linear_bwd_dw_adam_head) fed
    the dH the fold forms -- (h > 0) ? dS * w2 : 0 from the fold's own dS and w2 snapshot, one rounding per element --
    through the scalar operand path: layer 1's gradients, parameters and moments bit for bit."""
    B, I, Hd = 32, 36, 48
    hyper = [0.0, 1.0, 1.0]
    res = []
    torch.manual_seed(4)
    X2 = torch.bernoulli(torch.full((2 * B, I), 0.3)).to(DEV)
    for folded in (True, False):
        fp, L1, L2 = _fold_setup(2 * B, I, Hd, 3)
        H = torch.empty(2 * B, Hd, device=DEV)
        S = torch.zeros(2 * B, device=DEV); dS = torch.zeros_like(S); rl = torch.zeros_like(S)
        loss = torch.zeros(1, device=DEV)
        adam = dict(sched=torch.tensor([1e-3, 0.9, 2e-3, 0.8], device=DEV), sched_slot=ops.slot(0, 0, 1, 0, 1), clamp=0.0)
        head = dict(H=H, lin=L2, loss_out=loss, loss_slot=ops.NO_SLOT, inv_b=1.0 / B, B=B, adam=adam)
        fold = ops.HeadFold(2 * B, Hd, DEV)
        ops.linear_fwd_headpart(X2, L1.W, L1.b, H, "relu", L2, fold)
        w2 = L2.W.clone().view(-1)
        if folded:
            ops.linear_bwd_dw_adam_head_fold(H, X2, L1, adam, head, fold.args("ns", "sigmoid", hyper, S=S, dS=dS, rowloss=rl))
        else:
            dS, rl = res[0]["dS"], res[0]["rl"]
            dH = torch.where(H > 0, dS[:, None] * w2[None, :], torch.zeros((), device=DEV))
            ops.linear_bwd_dw_adam_head(_off1(dH), _off1(X2), L1, adam, dict(head, dS=dS, rowloss=rl))
        torch.cuda.synchronize()
        res.append(dict(dS=dS.clone(), rl=rl.clone(), W=L1.W.clone(), b=L1.b.clone(), gW=L1.gW.clone(),
                        gb=L1.gb.clone(), mW=L1.mW.clone(), vW=L1.vW.clone(), mb=L1.mb.clone(), vb=L1.vb.clone()))
    assert bool(res[0]["gW"].abs().sum() > 0)
    for k in ("W", "b", "gW", "gb", "mW", "vW", "mb", "vb"):
        assert torch.equal(res[0][k], res[1][k]), k


def test_folded_dx_equals_unfolded_launch():
    """ops.linear_bwd_dx_head_fold at R = 64, hidden 48, against ops.linear_bwd_dx on the dH the fold forms, W one float
    off (scalar path for the weight operand)."""
    B, I, Hd = 64, 36, 48
    hyper = [0.0, 1.0, 1.0]
    torch.manual_seed(9)
    Xg = torch.rand(B, I).to(DEV)
    W1 = (torch.randn(Hd, I) / I ** 0.5).to(DEV); b1 = (torch.randn(Hd) * 0.1).to(DEV)
    L2 = SimpleNamespace(W=(torch.randn(1, Hd) / Hd ** 0.5).to(DEV), b=torch.randn(1).to(DEV))
    below = torch.rand(B, I).to(DEV)
    H = torch.empty(B, Hd, device=DEV)
    fold = ops.HeadFold(B, Hd, DEV)
    S = torch.zeros(B, device=DEV); dS = torch.zeros(B, device=DEV); rl = torch.zeros(B, device=DEV)
    loss = torch.zeros(1, device=DEV); dX = torch.empty(B, I, device=DEV); ref = torch.empty(B, I, device=DEV)
    ops.linear_fwd_headpart(Xg, W1, b1, H, "relu", L2, fold)
    ops.linear_bwd_dx_head_fold(H, W1, dX, dict(H=H, lin=L2, loss_out=loss, loss_slot=ops.NO_SLOT, inv_b=1.0 / B, B=B,
                                                gen_mode=True),
                                fold.args("ns", "sigmoid", hyper, S=S, dS=dS, rowloss=rl), below=below, epi="sigmoid")
    dH = torch.where(H > 0, dS[:, None] * L2.W.view(-1)[None, :], torch.zeros((), device=DEV))
    ops.linear_bwd_dx(dH, _off1(W1), ref, below=below, epi="sigmoid")
    torch.cuda.synchronize()
    assert bool(dX.abs().sum() > 0)
    assert torch.equal(dX, ref)


def test_dw_against_fp64():
    """Independent of the operand paths: dW against dA.double().T @ X.double(), bounded by twice the error of the fp32
    CPU product against that value plus one fp32 ulp of the output's scale (tests/test_gpu_ops.py close64)."""
    for R, N, K in ((64, 48, 32), (256, 400, 20), (33, 100, 96)):
        dA, X = _operands(R, N, K, R + N)
        dW, db = torch.empty(N, K, device=DEV), torch.empty(N, device=DEV)
        ops.linear_bwd_dw(dA, X, dW, db)
        torch.cuda.synchronize()
        a, x = dA.cpu(), X.cpu()
        ref64, ref32 = a.double().t() @ x.double(), (a.t() @ x).double()
        scale = ref64.abs().max().item()
        e_hip = (dW.cpu().double() - ref64).abs().max().item() / scale
        e_cpu = (ref32 - ref64).abs().max().item() / scale
        print("R=%d N=%d K=%d: HIP err %.3e, CPU fp32 err %.3e" % (R, N, K, e_hip, e_cpu))
        assert e_hip <= 2.0 * e_cpu + 2.0 ** -23, (R, N, K, e_hip, e_cpu)
