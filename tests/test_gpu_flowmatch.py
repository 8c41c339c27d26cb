"""Flow matching on the MI355X: gm_fm_qsample against the numpy rule and gm_nvp_pre's bits, gm_fm_div exactly and
against fp64, gm_fm_stage against the fp64 stage rule, the engine against the fp64 oracle of flowmatch_reference.py,
reproducibility and resume, the fresh (identity) model, the all-lit affine model, the solver step by step and end to
end, and learning on the bands."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))
sys.path.insert(0, HERE)

import flow_matching  # noqa: E402
import flowmatch_reference as R  # noqa: E402
from generative_models_amd import ops, trainers  # noqa: E402
from generative_models_amd import flowmatch as gfm  # noqa: E402
from generative_models_amd import ops_fused as of_  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
ALPHA, LEVELS = 0.05, 256


def _tables(T, E):
    tab = gfm.tables(T, E)
    dev = {k: torch.from_numpy(tab[k].astype(np.float32)).to(DEV) for k in ("tt", "tc", "temb")}
    return of_.fm_tables(dev["tt"], dev["tc"], dev["temb"]), dev


def _data(packed, n, I, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.bernoulli(torch.full((n, I), 0.3), generator=g) if packed else torch.rand(n, I, generator=g)
    return x, (ops.PackedData(x.to(DEV)) if packed else x.to(DEV))


def _qs(x, noise, tab, alpha=ALPHA, levels=LEVELS):
    """(xin, u, logdet, j, y1, y0) of device rows x."""
    n, I = x.shape
    y1, y0 = torch.empty(n, I, device=DEV), torch.empty(n, I, device=DEV)
    return of_.fm_qsample(x, noise, tab, alpha, levels, y1=y1, y0=y0) + (y1, y0)


def _nvp_pre(x, seed, tag, step, row0, alpha=ALPHA, levels=LEVELS):
    n, I = x.shape
    y, ld = torch.empty(n, I, device=DEV), torch.empty(n, device=DEV)
    of_.nvp_pre(x, *of_.maf_halves(y, I), ld, n, seed, tag, alpha, levels, "half", step=step, row0=row0)
    return y, ld


# ---- the path sample ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b,I,E,T", [(37, 64, 8, 50), (5, 30, 4, 2), (64, 784, 32, 1000)],
                         ids=["37x64", "5x30-scalar-tails", "64x784"])
def test_qsample_against_the_rule(b, I, E, T):
    tab, _ = _tables(T, E)
    g = torch.Generator().manual_seed(b)
    x = torch.rand(b, I, generator=g)
    xd = x.to(DEV)
    for train in (True, False):
        for seed, step, row0 in [(0, 0, 0), ((1 << 64) - 1, 77, 3), (0x123456789ABCDEF, 1 << 20, 511)]:
            xin, u, ld, j, y1, y0 = _qs(xd, of_.fm_noise(seed, train, step=step, row0=row0), tab)
            py1, pld = _nvp_pre(xd, seed, gfm.TAG_D if train else gfm.TAG_VD, step, row0)
            assert torch.equal(y1, py1) and torch.equal(ld, pld)        # gm_nvp_pre's bits
            c = lambda t: t.cpu().numpy()
            R.close_rule(c(xin), c(u), c(ld), c(j), c(y1), c(y0), x.numpy(), T, E, seed, step, train, ALPHA, LEVELS, row0)
    nz = of_.fm_noise(9, True, step=3)
    a, b2 = _qs(xd, nz, tab), _qs(xd, nz, tab)
    assert all(torch.equal(p, q) for p, q in zip(a, b2))               # two calls: the same bits
    assert all(torch.equal(p, q) for p, q in zip(a, _qs(xd, of_.fm_noise(9, True, step=(1 << 32) + 3), tab)))
    if T == 2:                                                          # both ends are frequent: exactly y0 and y1
        seen = set()
        for step in range(8):
            o = _qs(xd, of_.fm_noise(9, True, step=step), tab)
            jj = o[3].long()
            seen |= set(jj.tolist())
            assert torch.equal(o[0][jj == 0][:, :I], o[5][jj == 0]) and torch.equal(o[0][jj == T][:, :I], o[4][jj == T])
        assert seen == {0, 1, 2}
    # other settings of the preprocessing reach the kernel
    o = _qs(xd, nz, tab, alpha=0.0, levels=16)
    py1, pld = _nvp_pre(xd, 9, gfm.TAG_D, 3, 0, alpha=0.0, levels=16)
    assert torch.equal(o[4], py1) and torch.equal(o[2], pld) and not torch.equal(o[4], a[4])
    # strided rows in and out with guard cells: nothing written past a row's floats, nor past row b
    big = torch.rand(b + 2, I + 9, generator=g).to(DEV)
    xs = big[:b, 3:3 + I]
    G = -7.0
    xin = torch.full((b + 2, I + E + 5), G, device=DEV)
    u, y1, y0 = (torch.full((b + 2, I + 3), G, device=DEV) for _ in range(3))
    ld = torch.full((b + 2,), G, device=DEV)
    j = torch.full((b + 2,), -7, dtype=torch.int32, device=DEV)
    of_.fm_qsample(xs, nz, tab, ALPHA, LEVELS, xin=xin[:b], u=u[:b], logdet=ld, j=j, y1=y1[:b], y0=y0[:b])
    want = _qs(xs.contiguous(), nz, tab)
    assert torch.equal(xin[:b, :I + E], want[0]) and torch.equal(u[:b, :I], want[1]) and torch.equal(ld[:b], want[2])
    assert torch.equal(j[:b], want[3]) and torch.equal(y1[:b, :I], want[4]) and torch.equal(y0[:b, :I], want[5])
    assert torch.all(xin[:, I + E:] == G) and all(torch.all(t[:, I:] == G) for t in (u, y1, y0))
    assert all(torch.all(t[b:] == G) for t in (xin, u, y1, y0, ld)) and torch.all(j[b:] == -7)
    # a device counter plus a device base equals the same step given as a value
    ctr = torch.tensor([40], dtype=torch.int64, device=DEV)
    base = torch.tensor([1000], dtype=torch.int64, device=DEV)
    via = _qs(xd, of_.fm_noise(11, True, step=2, step_ctr=ctr, step_base=base), tab)
    assert all(torch.equal(p, q) for p, q in zip(via, _qs(xd, of_.fm_noise(11, True, step=1042), tab)))
    assert not torch.equal(via[5], _qs(xd, of_.fm_noise(11, True, step=1041), tab)[5])


@pytest.mark.parametrize("packed", [True, False], ids=["bits", "fp32"])
@pytest.mark.parametrize("I,E,T", [(64, 8, 50), (30, 4, 2), (784, 32, 1000)])
def test_gathering_qsample_equals_gather_then_qsample(packed, I, E, T):
    tab, _ = _tables(T, E)
    x, data = _data(packed, 300, I)
    g = torch.Generator().manual_seed(I)
    B = 64
    idx = torch.randint(0, x.shape[0], (3, B), generator=g).to(DEV)
    ctr = torch.tensor([5], dtype=torch.int64, device=DEV)
    base = torch.tensor([100], dtype=torch.int64, device=DEV)
    ldin = (I + E + 3) // 4 * 4
    for b in (B, 37, 5):
        slot = ops.slot(ctr.data_ptr(), 1, 0, 3, B)              # idx slot: row ctr % 3 of the ring
        X, ref = torch.full((B, I), -1.0, device=DEV), torch.full((B, I), -1.0, device=DEV)
        xin, u = torch.full((B, ldin), -1.0, device=DEV), torch.full((B, I), -1.0, device=DEV)
        ld = torch.full((B,), -1.0, device=DEV)
        j = torch.full((B,), -1, dtype=torch.int32, device=DEV)
        for train in (True, False):
            of_.gather_rows_fm_qsample(data, idx.view(-1), X, xin, u, ld, j,
                                       of_.fm_noise(77, train, step_ctr=ctr, step_base=base), tab, ALPHA, LEVELS, B=b,
                                       idx_slot=slot)
            ops.gather_rows(data, idx.view(-1), ref, B=b, idx_slot=slot)
            assert torch.equal(X, ref)                          # the clean rows: exactly the plain gather's
            want = of_.fm_qsample(ref[:b].contiguous(), of_.fm_noise(77, train, step=105), tab, ALPHA, LEVELS)
            assert torch.equal(xin[:b, :I + E], want[0]) and torch.equal(u[:b], want[1])
            assert torch.equal(ld[:b], want[2]) and torch.equal(j[:b], want[3])
            assert torch.all(xin[b:] == -1.0) and torch.all(u[b:] == -1.0) and torch.all(j[b:] == -1)
            assert torch.all(ld[b:] == -1.0) and torch.all(xin[:, I + E:] == -1.0)


def test_qsample_statistics_over_a_million_draws():
    T, E, n, I = 50, 8, 1 << 20, 4                             # 2^20 grid indices, 2^22 normals
    tab, _ = _tables(T, E)
    x = torch.full((n, I), 0.5, device=DEV)
    y0 = torch.empty(n, I, device=DEV)
    _xin, _u, _ld, j = of_.fm_qsample(x, of_.fm_noise(123, True, step=9), tab, ALPHA, LEVELS, y0=y0)
    cnt = torch.bincount(j.long(), minlength=T + 1).double().cpu().numpy()
    p = 1.0 / (T + 1)
    assert cnt.sum() == n and len(cnt) == T + 1 and np.all(np.abs(cnt - n * p) <= 5 * (n * p * (1 - p)) ** 0.5), cnt
    e = y0.double()
    N = n * I
    m, v = e.mean().item(), e.var().item()
    assert abs(m) <= 5 / N ** 0.5 and abs(v - 1) <= 5 * (2 / N) ** 0.5, (m, v)
    ku = ((e - m) ** 4).mean().item() / v ** 2
    assert abs(ku - 3) <= 5 * (24 / N) ** 0.5, ku
    y0b = torch.empty(n, I, device=DEV)
    of_.fm_qsample(x, of_.fm_noise(123, True, step=10), tab, ALPHA, LEVELS, y0=y0b)
    assert abs((e * y0b.double()).mean().item()) <= 5 / N ** 0.5          # steps are uncorrelated
    assert abs((e[:, 0] * (j.double() - T / 2)).mean().item()) <= 5 * (((T + 1) ** 2 - 1) / 12 / n) ** 0.5   # j and y0 too


# ---- the divergence ---------------------------------------------------------------------------------------------------------
def _padded(t, pad, fill=3.0):
    """t's values in a wider array of another leading dimension (the padding holds `fill`)."""
    big = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    big[:, :t.shape[1]] = t
    return big.to(DEV)[:, :t.shape[1]]


def _signs(B, H, g):
    """Activations of random sign with exact zeros and -0.0 among them."""
    a = torch.randn(B, H, generator=g)
    r = torch.rand(B, H, generator=g)
    a[r < 0.1] = 0.0
    a[(r >= 0.1) & (r < 0.2)] = -0.0
    return a


_DIV_SHAPES = [(B, H) for B in (1, 15, 16, 17, 33, 512) for H in (1, 3, 4, 5, 17, 64, 400, 1024)]


@pytest.fixture(scope="module")
def div_exact_inputs():
    """The inputs of every exact case at the largest shape, made once: a case takes the leading rows and columns."""
    g = torch.Generator().manual_seed(5)
    return (torch.randint(-8, 9, (1024, 1024), generator=g).float(), _signs(512, 1024, g), _signs(512, 1024, g))


@pytest.mark.parametrize("B,H", _DIV_SHAPES, ids=["%dx%d" % s for s in _DIV_SHAPES])
def test_div_is_exact_on_integers(div_exact_inputs, B, H):
    """Q integer in [-8, 8] and 0 / 1 patterns: every partial sum is an integer below 8 H^2 <= 2^23, so any summation
    order is exact in fp32 and the device must equal the fp64 sum exactly."""
    Q, H1, H2 = (t[:n, :H].clone() for t, n in zip(div_exact_inputs, (H, B, B)))        # copies: the fixture is shared
    H2[0] = -1.0                                                 # a row with every ReLU dead: exactly 0
    if B > 1:
        H1[B - 1] = 0.0
    ref = R.divergence_of_patterns(Q.double(), (H1 > 0).double(), (H2 > 0).double())
    assert ref.abs().max() < 2 ** 24
    pad = 1 if H % 4 else 4                                       # keep (or break) the 16-byte path
    for pads in ((pad, pad, pad), (1, 3, 5), (0, 0, 0)):
        h1, h2, q = (_padded(t, p) for t, p in zip((H1, H2, Q), pads))
        tiles = of_.fm_div_tiles(H)
        div = torch.full((B + 2,), -7.0, device=DEV)
        part = torch.full((tiles * B + 2,), -7.0, device=DEV)
        got = of_.fm_div(h1, h2, q, part=part[1:tiles * B + 1], div=div[1:B + 1])
        assert torch.equal(got.cpu().double(), ref), (pads, (got.cpu().double() - ref).abs().max())
        assert div[0] == -7.0 and div[B + 1] == -7.0 and part[0] == -7.0 and part[-1] == -7.0     # the guard cells
        assert got[0] == 0.0 and (B == 1 or got[B - 1] == 0.0)
        # the partials alone (what gm_fm_stage adds up): the same sum, in tile order
        p2 = of_.fm_div(h1, h2, q, finish=False)
        assert tuple(p2.shape) == (tiles, B) and torch.equal(p2.double().sum(0).cpu(), ref)


@pytest.mark.parametrize("B,H", [(33, 48), (512, 400), (1000, 1024)])
def test_div_real_valued_against_fp64(B, H):
    g = torch.Generator().manual_seed(H)
    Q = torch.randn(H, H, generator=g)
    H1, H2 = _signs(B, H, g), _signs(B, H, g)
    m1, m2 = (H1 > 0), (H2 > 0)
    ref = R.divergence_of_patterns(Q.double(), m1.double(), m2.double()).numpy()
    f32 = ((m2.float().numpy() @ Q.numpy()) * m1.float().numpy()).sum(1, dtype=np.float32)      # numpy-float32's own sum
    lit = ((m2.double() @ Q.double().abs()) * m1.double()).sum(1).numpy()
    bound = 2 * np.abs(f32.astype(np.float64) - ref) + 2.0 ** -23 * lit
    h1, h2, q = _padded(H1, 4), _padded(H2, 8), _padded(Q, 4)
    a = of_.fm_div(h1, h2, q)
    err = np.abs(a.cpu().double().numpy() - ref)
    print("max err / bound", float((err / bound).max()), "max err", float(err.max()))
    assert np.all(err <= bound), float((err / bound).max())
    assert torch.equal(a, of_.fm_div(h1, h2, q))                  # two runs: the same bits
    assert torch.equal(a, of_.fm_div(H1.to(DEV), H2.to(DEV), Q.to(DEV)))     # nor do the leading dimensions matter


# ---- one solver stage -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,I,E,T", [(33, 64, 8, 48), (5, 30, 4, 4)])
def test_stage_against_fp64(n, I, E, T):
    _, dev = _tables(T, E)
    temb = dev["temb"]
    g = torch.Generator().manual_seed(n)
    ldin = (I + E + 3) // 4 * 4
    G = -7.0
    for solver in gfm.SOLVERS:
        ns = len(gfm.TABLEAUS[solver][1])
        for direction in (1, -1):
            steps = 2
            coef64 = gfm.ode_table(T, steps, solver, direction)
            coef = torch.from_numpy(coef64.astype(np.float32)).to(DEV)
            c32 = coef.cpu().double().numpy()
            S = coef.shape[0]
            for s in range(S):                                   # every stage of both steps: first, middle, last, final
                for with_div in (True, False):
                    k, base, acc = (1.5 * torch.randn(n, I, generator=g) for _ in range(3))
                    L, d = torch.randn(n, 2, generator=g), torch.randn(3, n, generator=g)
                    kd, bd, ad = (torch.full((n + 1, I + 3), G, device=DEV) for _ in range(3))
                    for t_, v in ((kd, k), (bd, base), (ad, acc)):
                        t_[:n, :I] = v.to(DEV)
                    xin = torch.full((n + 1, ldin + 4), G, device=DEV)
                    Ld = torch.full((n + 1, 2), G, device=DEV)
                    Ld[:n] = L.to(DEV)
                    of_.fm_stage(kd[:, :I], bd[:, :I], ad[:, :I], xin[:, :ldin], coef, temb, I, ns, L=Ld,
                                 div=d.to(DEV) if with_div else None, div_parts=3, step=s, rows=n)
                    first = c32[s, 2] != 0
                    y, rb, ra = R.stage_rule(k.double(), base.double(), acc.double() if not first else 0.0, c32[s])
                    scale = y.abs().max(1, keepdim=True).values.clamp(min=1.0)
                    assert ((xin[:n, :I].cpu().double() - y).abs() / scale).max() <= R.STEP_TOL, (solver, direction, s)
                    assert ((ad[:n, :I].cpu().double() - ra).abs() / scale).max() <= R.STEP_TOL
                    if c32[s, 3] != 0:
                        assert ((bd[:n, :I].cpu().double() - rb).abs() / scale).max() <= R.STEP_TOL
                        assert torch.equal(bd[:n, :I], xin[:n, :I])                  # y = Base on a step's last stage
                    else:
                        assert torch.equal(bd[:n, :I].cpu(), base)                  # Base moves on last stages only
                    if with_div:
                        dd = (d[0] + d[1]) + d[2]                                    # the partials in order, fp32
                        ly, lb, la = R.stage_rule(dd.double(), L[:, 0].double(), L[:, 1].double() if not first else 0.0,
                                                  c32[s])
                        ls = ly.abs().clamp(min=1.0)
                        assert ((Ld[:n, 1].cpu().double() - la).abs() / ls).max() <= R.STEP_TOL
                        want0 = lb if c32[s, 3] != 0 else L[:, 0].double()
                        assert ((Ld[:n, 0].cpu().double() - want0).abs() / ls).max() <= R.STEP_TOL
                    else:
                        assert torch.equal(Ld[:n].cpu(), L)                          # sampling: L is left alone
                    if s < S - 1:                                # the tail: temb[j_next], bit for bit
                        assert torch.equal(xin[:n, I:I + E], temb[int(coef64[s + 1, 5])].expand(n, E))
                    else:
                        assert torch.all(xin[:n, I:I + E] == G)                      # the final evaluation leaves it
                    assert torch.all(xin[n:] == G) and torch.all(xin[:, I + E:] == G) and torch.all(Ld[n:] == G)
                    assert all(torch.all(t_[n:] == G) and torch.all(t_[:, I:] == G) for t_ in (kd, bd, ad))
    # a slot over a device counter, the tick by the launch, the trajectory rows (heun: two stages per step)
    coef64 = gfm.ode_table(T, 2, "heun", 1)
    coef = torch.from_numpy(coef64.astype(np.float32)).to(DEV)
    ctr, done = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    k = torch.randn(n, I, generator=g).to(DEV)
    y = torch.randn(n, I, generator=g).to(DEV)
    st = []
    for _ in range(2):
        xin = torch.zeros(n, ldin, device=DEV)
        xin[:, :I] = y
        st.append(dict(xin=xin, base=y.clone(), acc=torch.zeros(n, I, device=DEV)))
    traj = torch.full((3, n, I), G, device=DEV)
    for s in range(4):
        a, b = st
        of_.fm_stage(k, a["base"], a["acc"], a["xin"], coef, temb, I, 2, slot=ops.slot(ctr.data_ptr(), 1, 0, 0, 8),
                     traj=traj, tick=ctr, done=done)
        of_.fm_stage(k, b["base"], b["acc"], b["xin"], coef, temb, I, 2, step=s)
        assert all(torch.equal(a[key], b[key]) for key in a) and ctr.item() == s + 1 and done.item() == 0
        if s % 2 == 1:
            assert torch.equal(traj[s // 2 + 1], a["xin"][:, :I])
        else:
            assert torch.all(traj[s // 2 + 1] == G)              # a step's first stage writes no trajectory row
    assert torch.all(traj[0] == G)
    # a constant field: two heun steps of h = 1/2 move y by k, to rounding
    assert (st[0]["base"] - (y + k)).abs().max().item() <= 1e-5


# ---- the engine against the fp64 oracle ------------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, side, seed=7, binary=True):
    """Image loaders; the data come from a private generator, the loaders shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, side * side), 0.3), generator=g) if binary else \
            torch.rand(n, side * side, generator=g)
        ds = torch.utils.data.TensorDataset(x.view(n, 1, side, side), torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


SMALL = dict(I=64, H=48, E=8, T=50, side=8, batch=32, n_train=200, n_val=48, n_test=48, epochs=2)
SMALL_FP32 = dict(SMALL, binary=False)
ODD = dict(SMALL, I=49, side=7, E=4)                        # I and I + E no multiples of 4: the scalar tails
FULL = dict(I=784, H=400, E=32, T=1000, side=28, batch=512, n_train=3 * 512 + 336, n_val=512, n_test=64, epochs=1)


def mk_loaders(cfg):
    return loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"], binary=cfg.get("binary", True))


def mk_model(cfg, fresh=False):
    """The model of a parity run: `out` random too (a fresh model's zero `out` leaves the two hidden layers without a
    gradient on the first batch, and their gradient tests without a scale)."""
    torch.manual_seed(1234)
    m = flow_matching.FlowMatching(cfg["I"], cfg["H"], cfg["E"], cfg["T"])
    if not fresh:
        with torch.no_grad():
            torch.nn.init.normal_(m.field.out.weight, std=0.5 / cfg["H"] ** 0.5)
            torch.nn.init.normal_(m.field.out.bias, std=0.1)
    return m


def product(cfg, its, epochs, seed=0, use_graph=True, trainer_cls=None, model=None):
    m = mk_model(cfg) if model is None else model
    tr = (trainer_cls or flow_matching.FlowMatchingTrainer)(m, *its, seed=seed)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs)
    torch.cuda.synchronize()
    return tr, m


def device_rows(cfg, seed):
    """The oracle's source of rows: the device's path sample of a batch, each row checked against the numpy rule."""
    tab, _ = _tables(cfg["T"], cfg["E"])
    I, E = cfg["I"], cfg["E"]

    def rows(x, step, train):
        xin, u, ld, j, y1, y0 = _qs(x.to(DEV), of_.fm_noise(seed, train, step=step), tab)
        c = lambda t: t.cpu().numpy()
        R.close_rule(c(xin), c(u), c(ld), c(j), c(y1), c(y0), x.numpy(), cfg["T"], E, seed, step, train, ALPHA, LEVELS)
        return xin[:, :I + E].cpu().double(), u.cpu().double()
    return rows


def lclose(got, ref, tol=R.LOSS_TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= tol, (err.max(), got[:4], ref[:4])


def parity(cfg, trainer_cls=None, seed=5):
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    init = mk_model(cfg)
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    losses, best, P = R.oracle_train(init.state_dict(), its, cfg["epochs"], device_rows(cfg, seed))
    o_rng = torch.get_rng_state()
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, cfg["epochs"], seed=seed, trainer_cls=trainer_cls, model=init)
    print("losses", tr.losses[:3], losses[:3], "best", tr.best_val_loss, best)
    lclose(tr.losses, losses)
    assert abs(tr.best_val_loss - best) <= R.LOSS_TOL * max(1, abs(best))
    assert torch.equal(torch.get_rng_state(), o_rng)           # the loaders' shuffles and nothing else
    assert tr.noise_steps == cfg["epochs"] * len(its[0]) and tr.num_epochs == cfg["epochs"]
    worst = {k: (v.cpu().double() - P[k]).abs().max().item() for k, v in m.state_dict().items()}
    print("max |w - oracle|", worst)
    assert max(worst.values()) <= R.PARAM_TOL, worst
    return tr


@pytest.mark.parametrize("cfg", [SMALL, SMALL_FP32, ODD, FULL], ids=["small-ragged", "small-fp32", "49-4-tails",
                                                                     "784-400-32-b512"])
def test_engine_vs_fp64_oracle(cfg):
    tr = parity(cfg)
    assert type(tr._engine).__name__ == "FlowMatchEngine"


@pytest.mark.parametrize("cfg", [SMALL, ODD, FULL], ids=["small", "49-4-tails", "784-400-32-b512"])
def test_teacher_forced_batch_gradients_vs_fp64(cfg):
    """One training batch through FlowMatchEngine from known weights: every gradient it leaves in the flat gradient
    buffer against fp64 autograd on the device's rows of that batch, within GRAD_TOL of each tensor's scale."""
    b = cfg["batch"]
    its = loaders(b, b, b, 16, cfg["side"])
    m = mk_model(cfg)
    init = R.f64(m.state_dict())
    tr = flow_matching.FlowMatchingTrainer(m, *its, seed=3)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    torch.cuda.synchronize()
    fp = tr._engine.fp
    got = {k: fp.gviews[[i for i, q in enumerate(fp.params) if q is p][0]].cpu().double()
           for k, p in m.named_parameters()}
    assert len(got) == 6
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    x = its[0].dataset.tensors[0][perm].reshape(b, -1)
    xin, u = device_rows(cfg, 3)(x, 0, True)
    loss, grads = R.loss_and_grads(init, xin, u)
    assert abs(tr.losses[0] - loss) <= R.LOSS_TOL * max(1.0, abs(loss))
    for k, gk in got.items():
        scale = grads[k].abs().max().item()
        assert scale > 0, k
        err = (gk - grads[k]).abs().max().item()
        assert err <= R.GRAD_TOL * scale, (k, err, scale)


def snapshot(tr, m):
    return (list(tr.losses), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state(), tr.noise_steps)


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
    assert torch.equal(a[3], b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_bitwise_reproducibility_and_resume(tmp_path):
    cfg = SMALL
    runs = []
    for use_graph in (True, True, False):                   # graph twice (same seed), then eager
        torch.manual_seed(99)
        runs.append(snapshot(*product(cfg, mk_loaders(cfg), 2, use_graph=use_graph)))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    torch.manual_seed(99)
    other = snapshot(*product(cfg, mk_loaders(cfg), 2, seed=6))
    assert other[0] != runs[0][0] and any(not torch.equal(other[2][k], runs[0][2][k]) for k in other[2])
    # train(1) + save + load into a fresh trainer + train(1) == train(2): the noise stream and Adam's steps continue
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 1)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    m2 = flow_matching.FlowMatching(cfg["I"], cfg["H"], cfg["E"], cfg["T"]).to(DEV)
    tr2 = flow_matching.FlowMatchingTrainer(m2, *its, seed=0)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == len(its[0])
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    same(snapshot(tr2, m2), runs[0])
    # a checkpoint of other settings is refused under strict=True, taken under strict=False
    mk = lambda T=cfg["T"], **kw: flow_matching.FlowMatchingTrainer(
        flow_matching.FlowMatching(cfg["I"], cfg["H"], cfg["E"], T).to(DEV), *its, **kw)
    for bad in (dict(seed=1), dict(T=100), dict(alpha=0.1), dict(levels=16)):
        t3 = mk(**bad)
        t3.load_checkpoint(path)
        with pytest.raises(GMError):
            t3.train(1)
    t3 = mk(seed=1)
    t3.load_checkpoint(path, strict=False)
    with contextlib.redirect_stdout(io.StringIO()):
        t3.train(1)


def test_general_path_agrees_with_the_fused_run():
    class Mine(flow_matching.FlowMatchingTrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    cfg = dict(SMALL, n_train=96)
    tr = parity(cfg, trainer_cls=Mine)
    assert tr._engine is None


# ---- the fresh model, the affine model ---------------------------------------------------------------------------------------
def test_fresh_model_is_the_identity_flow():
    cfg = SMALL
    its = mk_loaders(cfg)
    m = mk_model(cfg, fresh=True)
    tr = flow_matching.FlowMatchingTrainer(m, *its, seed=0)
    I = cfg["I"]
    st = torch.get_rng_state()
    z = torch.empty(300, I, device=DEV)
    of_.nvp_prior(*of_.maf_halves(z, I), 300, I, 7, "half")
    want = torch.empty(300, I, device=DEV)
    of_.nvp_post(*of_.maf_halves(z, I), want, 300, ALPHA, "half")
    zr = gfm.realnvp.normals_reference(300, I, 7)
    assert (np.abs(z.cpu().double().numpy() - zr) / np.maximum(1.0, np.abs(zr))).max() <= R.NORMAL_TOL
    for solver, steps in (("euler", 5), ("heun", 10), ("rk4", 5)):
        got = tr.sample(300, seed=7, steps=steps, solver=solver)
        assert torch.equal(got, want), solver                       # v = 0: gm_nvp_post of the prior's normals, bit for bit
        assert torch.equal(tr.sample(5, seed=7, steps=steps, solver=solver), got[:5])    # rows do not depend on n
    assert torch.equal(tr.sample(300, seed=7, temperature=0.5, steps=5), tr._post(0.5 * z))
    assert torch.equal(st, torch.get_rng_state())
    # the likelihood of the identity flow: the prior's density of y1 itself
    x = its[2].dataset.tensors[0].reshape(-1, I)
    ll = tr.log_likelihood_rows(x, seed=3, batch=32, steps=5, solver="heun")
    ref = []
    for i in range(0, x.shape[0], 32):
        y1, ld = _nvp_pre(x[i:i + 32].to(DEV), 3, gfm.TAG_VD, i // 32, 0)
        ref.append(-R.nll_rows(y1.cpu().double(), ld.cpu().double(), 0.0, I, LEVELS))
    ref = torch.cat(ref)
    assert ((ll - ref).abs() / ref.abs().clamp(min=1.0)).max() <= R.LOSS_TOL
    z2, lp = tr.encode(x[:40], seed=3, batch=16, steps=5, solver="euler")
    y1, ld = _nvp_pre(x[:16].to(DEV), 3, gfm.TAG_VD, 0, 0)
    assert torch.equal(z2[:16], y1) and tuple(lp.shape) == (40,)
    res = tr.log_likelihood(x, steps=5, solver="heun")
    assert res.n == x.shape[0] and np.isfinite(tr.bits_per_dim(res))


def _load(m, P):
    m.load_state_dict({k: v.float() for k, v in P.items()})
    return m.to(DEV)


def test_all_lit_affine_model_has_the_trace_as_divergence():
    I, H, E, T = 6, 5, 4, 64
    P = R.affine_model(I, H, E)
    m = _load(flow_matching.FlowMatching(I, H, E, T), P)
    tr = object.__new__(gfm.FlowMatchTrainer)
    tr.model = m
    g = torch.Generator().manual_seed(1)
    y = 1.5 * torch.randn(16, I, generator=g)
    P32 = R.f64(m.state_dict())                                    # the fp32 weights the device holds
    A, _ = R.affine_form(P32, I)
    trace = A.diagonal().sum().item()                              # tr(W3 W2 W1y): the divergence of every row
    Q = R.divergence_matrix(P32, I)
    qb = R.divergence_matrix_bound(P32, I)
    Qd = tr.divergence_matrix().cpu()                              # the device's own Q: fp32 products of a GEMM's outputs
    assert torch.all((Qd.double() - Q).abs() <= qb), ((Qd.double() - Q).abs() / qb).max()
    assert abs(Q.sum().item() - trace) <= 1e-12 * Q.abs().sum().item()           # every unit lit: the sum of all of Q
    f32 = float(Qd.numpy().sum(dtype=np.float32))
    # test_div_real_valued's bound on the sum (given the device's Q) plus what forming Q in fp32 may move its entries by
    # (flowmatch_reference.divergence_matrix_bound, the same rule one level down)
    bound = 2 * abs(f32 - Qd.double().sum().item()) + 2.0 ** -23 * Qd.double().abs().sum().item() + qb.sum().item()
    for j in (0, 17, T):
        d = tr.divergence(y, j).cpu().double()
        print("j", j, "max |div - trace|", (d - trace).abs().max().item(), "bound", bound)
        assert (d - trace).abs().max().item() <= bound, (j, d, trace, bound)
        v = tr.velocity(y, j).cpu().double()
        ref_v = R.forward(P32, torch.cat([y.double(), m.temb[j].cpu().double().expand(16, E)], 1))
        assert ((v - ref_v).abs() / ref_v.abs().clamp(min=1.0)).max() <= R.LOSS_TOL
    jj = torch.tensor([0, 17, T, 5] * 4)
    assert torch.equal(tr.divergence(y, jj), tr.divergence(y, jj))


# ---- the solver step by step and end to end ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained_small():
    cfg = SMALL
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 2)
    return cfg, tr, m


def _drive_every_evaluation(tr, P, y0, S, solver, direction, with_div):
    """The solver's launches one evaluation at a time, as FlowMatchTrainer._solve issues them launch by launch, each
    teacher-forced from the device's own state: the field of the device's input rows within the forward GEMMs' bound
    (LOSS_TOL of max(1, |v|), test_all_lit_affine_model's), the divergence given the device's own H1, H2 and Q within
    test_div_real_valued's bound, and the stage -- the next rows, Base, Acc and the log-determinant pair from the
    device's k, d, Base, Acc and pair -- within STEP_TOL of each row's scale.  Returns (Base, LBase) at the end."""
    m = tr.model
    I, E, T, H, n = m.image_size, m.time_dim, m.T, m.hidden_dim, y0.shape[0]
    coef64 = gfm.ode_table(T, S, solver, direction)
    coef = torch.from_numpy(coef64.astype(np.float32)).to(DEV)
    c32 = coef.cpu().double().numpy()
    ns = len(gfm.TABLEAUS[solver][1])
    w = tr._weights()
    Qd = tr.divergence_matrix()
    Q64 = Qd.cpu().double()
    z = lambda *s: torch.zeros(*s, device=DEV)
    xin_full, H1, H2, out = z(n, (I + E + 3) // 4 * 4), z(n, H), z(n, H), z(n, I)
    base, acc, L = y0.clone(), z(n, I), z(n, 2)
    xin_full[:, :I] = y0
    xin_full[:, I:I + E] = m.temb[int(coef64[0, 5])]
    xin = xin_full[:, :I + E]
    f = lambda t: t.cpu().double()
    for r in range(coef.shape[0]):
        row, first, last = c32[r], c32[r, 2] != 0, c32[r, 3] != 0
        assert torch.equal(xin[:, I:], m.temb[int(coef64[r, 5])].expand(n, E))       # this evaluation's time, bit for bit
        x0, b0, a0, L0 = f(xin), f(base), f(acc), f(L)
        ops.linear_fwd(xin, w[0], w[1], H1, "relu")
        ops.linear_fwd(H1, w[2], w[3], H2, "relu")
        ops.linear_fwd(H2, w[4], w[5], out, "id")
        k = f(out)
        v = R.forward(P, x0)
        assert ((k - v).abs() / v.abs().clamp(min=1.0)).max().item() <= R.LOSS_TOL, r
        part = None
        if with_div:
            part = of_.fm_div(H1, H2, Qd, finish=False)
            m1, m2 = (H1 > 0).cpu(), (H2 > 0).cpu()
            dref = R.divergence_of_patterns(Q64, m1.double(), m2.double()).numpy()
            f32 = ((m2.float().numpy() @ Qd.cpu().numpy()) * m1.float().numpy()).sum(1, dtype=np.float32)
            lit = ((m2.double() @ Q64.abs()) * m1.double()).sum(1).numpy()
            d32 = part[0].clone()
            for t_ in range(1, part.shape[0]):
                d32 += part[t_]                                  # the stage kernel's order: the tiles in turn, fp32
            d = f(d32)
            assert np.all(np.abs(d.numpy() - dref) <= 2 * np.abs(f32.astype(np.float64) - dref) + 2.0 ** -23 * lit), r
        of_.fm_stage(out, base, acc, xin_full, coef, m.temb, I, ns, L=L, div=part,
                     div_parts=of_.fm_div_tiles(H), step=r)
        y, rb, ra = R.stage_rule(k, b0, 0.0 if first else a0, row)
        scale = y.abs().max(1, keepdim=True).values.clamp(min=1.0)
        assert ((f(xin[:, :I]) - y).abs() / scale).max().item() <= R.STEP_TOL, (solver, direction, r)
        assert ((f(acc) - ra).abs() / scale).max().item() <= R.STEP_TOL and ((f(base) - rb).abs() / scale).max().item() \
            <= R.STEP_TOL, (solver, direction, r)
        if last:
            assert torch.equal(base, xin[:, :I])
        if with_div:
            ly, lb, la = R.stage_rule(d, L0[:, 0], 0.0 if first else L0[:, 1], row)
            ls = ly.abs().clamp(min=1.0)
            assert ((f(L[:, 1]) - la).abs() / ls).max().item() <= R.STEP_TOL, r
            assert ((f(L[:, 0]) - lb).abs() / ls).max().item() <= R.STEP_TOL, r
        else:
            assert not L.any()
    return base, L[:, 0].clone()


@pytest.mark.parametrize("solver,S", [("euler", 10), ("heun", 5), ("rk4", 5)])
def test_solver_step_by_step(trained_small, solver, S):
    cfg, tr, m = trained_small
    I, E, T, H, n = cfg["I"], cfg["E"], cfg["T"], cfg["H"], 33
    before = {k: v.clone() for k, v in m.state_dict().items()}
    st, mode = torch.get_rng_state(), m.training
    out, traj = tr.sample(n, seed=4, steps=S, solver=solver, return_trajectory=True)
    assert torch.equal(st, torch.get_rng_state()) and m.training == mode
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert tuple(out.shape) == (n, I) and tuple(traj.shape) == (S + 1, n, I)
    assert out.min().item() >= 0.0 and out.max().item() <= 1.0 and torch.equal(out, tr._post(traj[-1].contiguous()))
    z0 = gfm.realnvp.normals_reference(n, I, 4)
    assert (np.abs(traj[0].cpu().double().numpy() - z0) / np.maximum(1, np.abs(z0))).max() <= R.NORMAL_TOL
    P = R.f64(m.state_dict())
    for direction, with_div, y0 in ((1, False, traj[0]), (-1, True, traj[-1])):
        end, l = _drive_every_evaluation(tr, P, y0.contiguous(), S, solver, direction, with_div)
        got = tr._solve(y0.contiguous(), direction, S, solver, with_div=with_div)
        assert torch.equal(end, got[0]) and (not with_div or torch.equal(l, got[1]))   # the trainer's loop: the same bits
        if direction == 1:
            assert torch.equal(end, traj[-1])
    # graph replay == launch by launch, the cached graph == the first capture, another seed differs
    a = tr.sample(n, seed=4, steps=S, solver=solver)
    assert torch.equal(a, out) and torch.equal(tr.sample(n, seed=4, steps=S, solver=solver), out)
    tr.use_graph = False
    try:
        o2, t2 = tr.sample(n, seed=4, steps=S, solver=solver, return_trajectory=True)
        x = tr.test_iter.dataset.tensors[0].reshape(-1, I)[:20]
        ll_eager = tr.log_likelihood_rows(x, steps=S, solver=solver)
    finally:
        tr.use_graph = True
    assert torch.equal(o2, out) and torch.equal(t2, traj)
    assert torch.equal(tr.log_likelihood_rows(x, steps=S, solver=solver), ll_eager)     # the likelihood's graph too,
    assert torch.equal(tr.log_likelihood_rows(x, steps=S, solver=solver), ll_eager)     # and the kept one replayed
    assert not torch.equal(tr.sample(n, seed=5, steps=S, solver=solver), out)


def test_end_to_end_against_the_reference():
    c = R.E2E
    I, E, T, n = c["I"], c["E"], c["T"], c["n"]
    P = R.e2e_model()
    m = _load(flow_matching.FlowMatching(I, c["H"], E, T), P)
    x = R.e2e_rows()
    ds = torch.utils.data.TensorDataset(x.view(n, 1, 8, 8), torch.zeros(n, dtype=torch.int64))
    it = torch.utils.data.DataLoader(ds, batch_size=32, shuffle=True)
    tr = flow_matching.FlowMatchingTrainer(m, it, it, it, seed=0, alpha=c["alpha"], levels=c["levels"])
    P32 = R.f64(m.state_dict())
    u = torch.from_numpy(gfm.uniforms_reference(n, I, 1, 0, gfm.TAG_VD))
    for solver, steps in R.E2E_CASES:
        ll64, z64, marked = R.log_likelihood(P32, x, u, T, E, steps, solver, c["alpha"], c["levels"])
        assert marked.double().mean().item() <= R.E2E_MAX_MARKED
        keep = ~marked
        ll = tr.log_likelihood_rows(x, seed=1, batch=n, steps=steps, solver=solver)
        err = ((ll - ll64).abs() / ll64.abs().clamp(min=1.0))[keep].max().item()
        z, lp = tr.encode(x, seed=1, batch=n, steps=steps, solver=solver)
        zerr = ((z.cpu().double() - z64).abs() / z64.abs().clamp(min=1.0))[keep].max().item()
        print(solver, steps, "marked", int(marked.sum()), "ll err", err, "z err", zerr)
        assert err <= R.E2E_TOL and zerr <= R.E2E_TOL, (solver, steps, err, zerr)
        assert torch.equal(lp.cpu().double(), ll)
        # encode -> decode: the device's round trip from its own z against the reference's from its own, under the same
        # bound (flowmatch_reference.E2E_FP32_DEV["x"] is the fp32 CPU run's deviation of exactly this)
        back = tr.decode(z, batch=n, steps=steps, solver=solver)
        ref, mk2 = R.decode(P32, z64, T, E, steps, solver, c["alpha"])
        assert (marked | mk2).double().mean().item() <= R.E2E_MAX_MARKED
        xerr = (back.cpu().double() - ref).abs()[~(marked | mk2)].max().item()
        print(solver, steps, "x err", xerr)
        assert xerr <= R.E2E_TOL, (solver, steps, xerr)


def test_learning_on_bands():
    """The bands of flowmatch_reference.bands_data: the validation loss after the schedule is below the first epoch's and
    below the fp64 oracle's own after the same schedule plus 10 % (flowmatch_reference.BANDS_THRESHOLD); parzen() and
    mmd() run on the trained model."""
    cfg = R.BANDS
    torch.manual_seed(99)
    its = R.bands_loaders(cfg)
    tr = flow_matching.FlowMatchingTrainer(R.bands_model(cfg), *its, seed=cfg["seed"])
    vals = []
    for _ in range(cfg["epochs"]):
        with contextlib.redirect_stdout(io.StringIO()):
            tr.train(1, lr=cfg["lr"])
        vals.append(tr.best_val_loss)
    print("validation loss by epoch (best so far)", vals, "threshold", R.BANDS_THRESHOLD)
    assert vals[-1] < vals[0] and vals[-1] <= R.BANDS_THRESHOLD, vals
    st = torch.get_rng_state()
    res = tr.parzen(n_samples=64, n_val=32)
    assert np.isfinite([res.sigma, res.ll_mean, res.ll_stderr]).all()
    mm = tr.mmd(n_samples=64)
    assert np.isfinite(mm.mmd2) and mm.n_samples == 64
    assert torch.equal(st, torch.get_rng_state())
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        tr.viz_dir = d
        try:
            imgs = tr.generate_images(3, num_outputs=4)
        finally:
            tr.viz_dir = None
        assert imgs.shape == (4, 8, 8) and os.path.isfile(os.path.join(d, "FlowMatching", "sample_3.png"))
