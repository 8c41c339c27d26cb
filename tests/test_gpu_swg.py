"""The SWG on the MI355X: the sort-and-match kernel on given projections, the directions, SWGEngine batch by batch, the
general path, metrics.sliced_wasserstein and the trainers' swd().

A sort is discontinuous, so every comparison of ranks and coefficients hands swg_reference.py the device's own projection
bits, read back; only continuous quantities are compared across the GEMM.

Bounds: test_gpu_tcvae.py's rule as test_gpu_gmmn.py uses it -- an error, in units of the reference tensor's max-abs, may
be 4 x the deviation of a float32 CPU run from the fp64 reference, and at least the bases 1e-5 (loss sums), 1.5e-6
(gradients), 5e-5 (weights, absolute).  Every error is printed beside its allowance."""
import contextlib
import io
import math
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

import swg  # noqa: E402
import swg_reference as R  # noqa: E402
from generative_models_amd import swg as gswg  # noqa: E402
from generative_models_amd import metrics, ops, ops_fused, philox, trainers  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
T_LOSS, T_GRAD, T_PARAM = 1e-5, 1.5e-6, 5e-5              # test_gpu_tcvae.py's bases
# (P, N, M): one element; N != M both ways round the overlap walk; exactly a wave; one past a wave on one side; a ragged
# P; a length that is no power of two; the gradient limit
CASES = [(1, 1, 1), (3, 2, 3), (5, 64, 64), (4, 65, 63), (130, 257, 130), (2, 1000, 1000), (1, 2048, 2048)]
REGIMES = ("spread", "collapsed")


def quiet(fn, *a, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        out = fn(*a, **kw)
    torch.cuda.synchronize()
    return out


def scaled_err(got, ref):
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)


def check(tag, name, got, ref, f32, base=T_GRAD):
    """test_gpu_tcvae.py's check: max(base, 4 x the fp32 CPU run's deviation), in units of the tensor's max-abs."""
    tol, err = max(base, 4.0 * scaled_err(f32, ref)), scaled_err(got, ref)
    print("%s %s: err %.3g allowed %.3g (fp32 cpu %.3g)" % (tag, name, err, tol, scaled_err(f32, ref)))
    assert err <= tol, (tag, name, err, tol)
    return err


def projections(P, N, M, regime):
    g = torch.Generator().manual_seed(7919 * N + 31 * M + P)
    a, b = torch.randn(P, N, generator=g), torch.randn(P, M, generator=g)
    if regime == "collapsed":                                # every generated row on one point; ties across the halves
        c = torch.randn(P, 1, generator=g)
        a = c.expand(P, N).clone()
        b[:, 2::3] = c                                       # exact duplicates of a
        b[:, 0] = 0.0
        if M > 1:
            b[:, 1] = -0.0
    return a.contiguous(), b.contiguous()


def run_sort(a, b, grad=True, pads=(3, 5)):
    """gm_sw_sort + gm_sw_finalize on a | b at leading dimensions of their own between sentinels."""
    P, N, M = a.shape[0], a.shape[1], b.shape[1]
    Pr = torch.full((P, N + M + pads[0]), 7.0, device=DEV)
    Pr[:, :N], Pr[:, N:N + M] = a.to(DEV), b.to(DEV)
    Ct = torch.full((P, N + pads[1]), 9.0, device=DEV) if grad else None
    wsb = torch.full((P + 1,), -3.0, dtype=torch.float64, device=DEV)
    stats = torch.zeros(3, dtype=torch.float64, device=DEV)
    stats[2] = -5.0
    loss = torch.zeros(1, device=DEV)
    ops_fused.sw_sort(Pr[:, :N + M], N, M, wsb[:P], Ct=Ct[:, :N] if grad else None)
    ops_fused.sw_finalize(P, N, M, wsb[:P], stats, loss_out=loss)
    torch.cuda.synchronize()
    assert bool((Pr[:, N + M:] == 7.0).all()) and float(wsb[P]) == -3.0 and float(stats[2]) == -5.0
    assert torch.equal(Pr[:, :N].cpu(), a) and torch.equal(Pr[:, N:N + M].cpu(), b)
    if grad:
        assert bool((Ct[:, N:] == 9.0).all())
    st = stats.cpu().numpy()
    return {"ws": wsb[:P].cpu().numpy(), "swd2": st[0], "swd": st[1], "loss32": float(loss.item()),
            "Ct": Ct[:, :N].cpu().numpy() if grad else None}


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("P,N,M", CASES)
def test_sw_sort_on_given_projections(P, N, M, regime):
    """gm_sw_sort on given projections against the fp64 reference on the same bits: the ranks recovered from Ct (the rank
    r whose B_r = sum_j w_rj b_(j) is nearest to M a_i - Ct_i / scale) equal numpy's stable argsort; ws, swd2 and Ct are
    within the rule's bounds; the call without Ct and a second run give the same bits.  In the spread regime every rank is
    recovered exactly.  The collapsed regime (every a equal: the index alone decides the order) is exempt from exact
    recovery, because its b's hold exact duplicates: equal b's give equal B_r, so the rank cannot be read off a
    coefficient there, and two ranks count as one where their B_r differ by less than the coefficient's two fp32
    roundings.  What pins the tie order there instead: each coefficient, at its row's original position, equals the
    reference's to the fp32 rounding of one subtraction and one multiply.  Measured on an MI355X (worst over the cases, in units of max-abs; DESIGN.md section
    36): spread -- ws 6.8e-8 of 1e-5, Ct 6.6e-8 of 1.5e-6, every rank recovered exactly; collapsed -- ws 1.4e-8, Ct 1.0e-7,
    the coefficients at most 0.95 of their two-rounding bound, about a third of the ranks recovered only up to equal
    b's."""
    a, b = projections(P, N, M, regime)
    a64, b64 = a.double().numpy(), b.double().numpy()
    ref, f32 = R.sw_reference(a64, b64), R.sw_reference(a.numpy(), b.numpy(), np.float32)
    ref.update(R.sw_diagnostics(ref))
    tag = "%s %s" % ((P, N, M), regime)
    got = run_sort(a, b)
    for v in (got["ws"], got["Ct"]):
        assert np.all(np.isfinite(v)), tag
    scale = 2.0 / (float(P) * N * M)
    target = M * a64 - got["Ct"].astype(np.float64) / scale               # [P, N]: the B_r the device paired row i with
    # what an fp32 coefficient resolves of B_r: its two roundings, in B's units (and the reference's own fp64 sums)
    res = 2.0 ** -23 * (ref["Ct_abs"] + np.abs(ref["Ct"])) / scale + \
        1e-10 * np.maximum(1.0, np.abs(ref["B"]).max(1, keepdims=True))
    exact = 0
    for p in range(P):
        Bp, rank = ref["B"][p], ref["rank_a"][p]
        rec = np.abs(target[p][:, None] - Bp[None, :]).argmin(1)
        exact += int((rec == rank).sum())
        if regime == "spread":
            assert np.array_equal(rec, rank), (tag, p)                        # the stable argsort, exactly
        else:       # duplicates among the b's: the rank, or one whose B_r an fp32 coefficient cannot tell from it
            assert np.all((rec == rank) | (np.abs(Bp[rec] - Bp[rank]) <= res[p])), (tag, p)
    print("%s ranks recovered exactly: %d of %d" % (tag, exact, P * N))
    assert regime == "collapsed" or exact == P * N
    if regime == "collapsed":
        assert np.array_equal(ref["rank_a"], np.broadcast_to(np.arange(N), (P, N)))   # ties: the index order
        bound = 2.0 ** -24 * (ref["Ct_abs"] + np.abs(ref["Ct"])) * (1 + 1e-6) + 1e-45
        worst = (np.abs(got["Ct"] - ref["Ct"]) / bound).max()
        print("%s Ct against its two roundings: worst %.3g of the bound" % (tag, worst))
        assert worst <= 1.0, (tag, worst)
    check(tag, "ws", got["ws"], ref["ws"], f32["ws"], T_LOSS)
    check(tag, "swd2", got["swd2"], ref["swd2"], f32["swd2"], T_LOSS)
    check(tag, "Ct", got["Ct"], ref["Ct"], f32["Ct"])
    assert got["swd"] == math.sqrt(got["swd2"]) and got["loss32"] == float(np.float32(got["swd2"]))
    keys = run_sort(a, b, grad=False)
    assert np.array_equal(keys["ws"], got["ws"]) and keys["swd2"] == got["swd2"]      # values only: the same bits
    again = run_sort(a, b, pads=(0, 1))
    assert np.array_equal(again["ws"], got["ws"]) and np.array_equal(again["Ct"], got["Ct"])


def test_sw_sort_keys_only_at_the_row_limit():
    """(2, 16384, 10000) without Ct: 128 KiB of values in LDS, N != M.  Measured on an MI355X: ws 1.6e-10 of 1.9e-5."""
    P, N, M = 2, 16384, 10000
    a, b = projections(P, N, M, "spread")
    b = (0.8 * b + 0.3).contiguous()
    ref = R.sw_reference(a.double().numpy(), b.double().numpy())
    f32 = R.sw_reference(a.numpy(), b.numpy(), np.float32)
    got = run_sort(a, b, grad=False)
    check("keys only", "ws", got["ws"], ref["ws"], f32["ws"], T_LOSS)
    check("keys only", "swd2", got["swd2"], ref["swd2"], f32["swd2"], T_LOSS)
    assert np.array_equal(run_sort(a, b, grad=False, pads=(1, 0))["ws"], got["ws"])
    with pytest.raises(GMError):
        run_sort(a, b, grad=True)                                         # a gradient holds 2048 rows a side


# ---- the directions -------------------------------------------------------------------------------------------------
def normals_f32(P, I, seed, step, tag, row0=0):
    """Box-Muller in float32 on the CPU (the rule's yardstick): uniforms, log, sqrt, the angle and cos / sin in fp32."""
    w = philox.words(P, 4 * ((I + 3) // 4), seed, step, tag, row0)
    u = philox.unit_uniforms(w).reshape(P, -1, 2)
    r = np.sqrt(np.float32(-2.0) * np.log(u[..., 0]))
    phi = np.float32(2.0 * np.pi) * u[..., 1]
    return np.stack([r * np.cos(phi), r * np.sin(phi)], -1).reshape(P, -1)[:, :I].astype(np.float32)


@pytest.mark.parametrize("P,I", [(1, 1), (5, 7), (130, 784), (3, 8192), (2, 130)])
def test_directions_vs_reference(P, I):
    """Unit norm to 1e-6; equal to the fp64 reference within 4 fp32 ulps of the row's max-abs (the deviation of an fp32
    CPU Box-Muller is printed beside it for the record); row p depends on (seed, step, p, tag) alone.  Measured on an
    MI355X: at most 2.6 ulps (the fp32 CPU Box-Muller up to 6.0): the 4-ulp bound holds as stated."""
    for seed, step, tag, row0 in ((0, 0, gswg.TAG_DT, 0), (2 ** 40 + 5, 7, gswg.TAG_DV, 0), (9, 0, gswg.TAG_DM, 256)):
        buf = torch.full((P, I + 3), 7.0, device=DEV)
        th = ops_fused.sw_directions(buf[:, :I], ops_fused.sw_noise(seed, tag, step=step, row0=row0))
        torch.cuda.synchronize()
        assert bool((buf[:, I:] == 7.0).all())
        got = th.cpu().double().numpy()
        want = gswg.directions_reference(P, I, seed, step, tag, row0)
        assert np.abs(np.sqrt((got * got).sum(1)) - 1.0).max() <= 1e-6
        n32 = normals_f32(P, I, seed, step, tag, row0).astype(np.float64)
        cpu32 = (n32 / np.sqrt((n32 * n32).sum(1, keepdims=True))).astype(np.float32)
        rowmax = np.abs(want).max(1, keepdims=True)
        ulp = 2.0 ** (np.floor(np.log2(rowmax)) - 23)
        err, dev32 = (np.abs(got - want) / ulp).max(), (np.abs(cpu32 - want) / ulp).max()
        print("directions %s: %.3g ulps of the row's max-abs (fp32 cpu Box-Muller %.3g)" % ((P, I, tag), err, dev32))
        assert err <= 4.0, (P, I, tag, err)
        # a row-offset call and another P: the same rows
        if P > 1:
            part = torch.empty(P - 1, I, device=DEV)
            ops_fused.sw_directions(part, ops_fused.sw_noise(seed, tag, step=step, row0=row0 + 1))
            assert torch.equal(part, th[1:])
            head = torch.empty(1, I, device=DEV)
            ops_fused.sw_directions(head, ops_fused.sw_noise(seed, tag, step=step, row0=row0))
            assert torch.equal(head, th[:1])
    ctr = torch.tensor([3], dtype=torch.int64, device=DEV)               # the step as device words: ctr + base + add
    base = torch.tensor([40], dtype=torch.int64, device=DEV)
    x, y = torch.empty(P, I, device=DEV), torch.empty(P, I, device=DEV)
    ops_fused.sw_directions(x, ops_fused.sw_noise(1, gswg.TAG_DT, step=2, step_ctr=ctr, step_base=base))
    ops_fused.sw_directions(y, ops_fused.sw_noise(1, gswg.TAG_DT, step=45))
    assert torch.equal(x, y)


# ---- the engine, batch by batch -------------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, I, seed=7, binary=True):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g) if binary else torch.rand(n, I, generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


def make_model(I, H, Z, seed=1234):
    torch.manual_seed(seed)
    m = swg.SWG(I, H, Z)
    return m, {n: v.detach().clone().double().numpy() for n, v in m.state_dict().items()}


def engine_views(eng, model, what):
    fp = eng.fp
    out = {}
    for n, p in model.named_parameters():
        i = [j for j, q in enumerate(fp.params) if q is p][0]
        o = fp.offsets[i]
        out[n] = getattr(fp, what)[o:o + p.numel()].view(p.shape).cpu().clone()
    return out


@pytest.fixture
def spy(monkeypatch):
    """Every training batch of an eager SWGEngine run, read back: the weights before it, and Theta, Pr, R, Ct, dX, dA,
    the flat gradient and the loss after it."""
    snaps = []
    orig = gswg.SWGEngine._issue

    def issue(self, st, t, b, train, pos=0, of=1):
        assert not self.use_graph
        if train:
            torch.cuda.synchronize()
            before = {n: v.detach().cpu().clone().double().numpy() for n, v in self.model.state_dict().items()}
        orig(self, st, t, b, train, pos=pos, of=of)
        if train:
            torch.cuda.synchronize()
            c = lambda x: x.detach().cpu().clone().double().numpy()
            snaps.append({"b": b, "W": before, "Theta": c(self.Theta), "Pr": c(self.Pr[:, :2 * b]), "R": c(self.Rb[:2 * b]),
                          "Ct": c(self.Ct[:, :b]), "dX": c(self.dX[:b]), "dA": c(self.dA[:b]),
                          "Pr32": self.Pr[:, :2 * b].cpu().clone().numpy(), "loss": float(self.lossf.item()),
                          "grad": {n: v.double().numpy() for n, v in engine_views(self, self.model, "grad").items()}})
    monkeypatch.setattr(gswg.SWGEngine, "_issue", issue)
    return snaps


@pytest.mark.parametrize("I,H,Z,b,P", [(784, 400, 20, 65, 130), (13, 10, 3, 7, 5)])
def test_one_fused_batch_at_lr_0(spy, I, H, Z, b, P):
    """One batch with Adam's lr = 0: the parameters stay bit for bit; Theta and Pr are read back; Pr against Theta R^T in
    fp64 within the gradient bound; Ct and the loss against the reference ON THE DEVICE'S Pr; dX, dA and the flat weight
    gradients against fp64 from the device's Ct.  Measured on an MI355X at (784, 400, 20, 65, 130), in units of max-abs:
    Pr 1.3e-7 of 1.7e-6, Ct 6.0e-8, loss 1.3e-8 of 1e-5, dX 1.4e-7, dA 1.8e-7, weight gradients at most 1.6e-7 of 1.5e-6
    (DESIGN.md section 36)."""
    its = loaders(b, b, b, 16, I, binary=I == 784)
    m, W = make_model(I, H, Z)
    tr = swg.SWGTrainer(m, *its, num_projections=P, seed=3)
    tr.use_graph = False
    st = torch.get_rng_state()
    quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
    torch.set_rng_state(st)                                               # the epoch's shuffle, again
    assert type(tr._engine).__name__ == "SWGEngine" and len(spy) == 1 and len(tr.losses) == 1 and tr.noise_steps == 1
    for n, v in m.state_dict().items():
        assert np.array_equal(v.cpu().double().numpy(), W[n]), n          # lr = 0: nothing moved
    s = spy[0]
    tag = "batch %s" % ((I, H, Z, b, P),)
    th64 = gswg.directions_reference(P, I, 3, 0, gswg.TAG_DT)
    assert np.abs(s["Theta"] - th64).max() <= 1e-6 and np.abs((s["Theta"] ** 2).sum(1) - 1).max() <= 1e-6
    z = gswg.uniforms_reference(b, Z, 3, 0, gswg.TAG_T).astype(np.float64)
    X64 = R.generator(W, z)[1].numpy()
    X32 = R.generator(W, z, torch.float32)[1].numpy()
    check(tag, "X", s["R"][:b], X64, X32)
    Y = its[0].dataset.tensors[0][trainers._epoch_order(its[0])].double().numpy()
    assert np.array_equal(s["R"][b:], Y)
    check(tag, "Pr", s["Pr"], s["Theta"] @ s["R"].T, (s["Theta"].astype(np.float32) @ s["R"].astype(np.float32).T))
    ref = R.sw_reference(s["Pr"][:, :b], s["Pr"][:, b:])                  # the device's own projection bits
    f32 = R.sw_reference(s["Pr32"][:, :b], s["Pr32"][:, b:], np.float32)
    check(tag, "Ct", s["Ct"], ref["Ct"], f32["Ct"])
    check(tag, "loss", tr.losses[0], ref["swd2"], f32["swd2"], T_LOSS)
    assert tr.losses[0] == s["loss"]
    back, b32 = R.backward(W, z, s["Ct"], s["Theta"]), R.backward(W, z, s["Ct"], s["Theta"], torch.float32)
    check(tag, "dX", s["dX"], back["dX"], b32["dX"])
    check(tag, "dA", s["dA"], back["dA"], b32["dA"])
    assert sorted(s["grad"]) == sorted(R.KEYS)
    for n in R.KEYS:
        check(tag, n, s["grad"][n], back["grads"][n], b32["grads"][n])
    # the loss is continuous across the GEMM: the fp64 projections give it within the loss bound
    ref_c = R.sw_reference(th64 @ X64.T, th64 @ Y.T)
    f32_c = R.sw_reference((th64.astype(np.float32) @ X32.T), (th64.astype(np.float32) @ Y.astype(np.float32).T), np.float32)
    check(tag, "loss across the GEMM", tr.losses[0], ref_c["swd2"], f32_c["swd2"], T_LOSS)


def test_lockstep_over_three_training_batches(spy):
    """Three training batches at lr = 1e-3: before each step the device's weights go into the fp64 reference, whose
    gradient comes from the device's Ct of that batch; after the step the weights are within the weight bound.  Measured
    on an MI355X: at most 3.5e-8 of 5e-5."""
    I, H, Z, b, P = 64, 48, 8, 32, 40
    its = loaders(b, 3 * b, b, 16, I, binary=False)
    m, W0 = make_model(I, H, Z)
    tr = swg.SWGTrainer(m, *its, num_projections=P, seed=5)
    tr.use_graph = False
    quiet(tr.train, 1, lr=1e-3, weight_decay=1e-5)
    assert len(spy) == 3 and tr.noise_steps == 3
    final = {n: v.detach().cpu().double().numpy() for n, v in m.state_dict().items()}
    mom = {dt: ({k: 0.0 for k in R.KEYS}, {k: 0.0 for k in R.KEYS}) for dt in (torch.float64, torch.float32)}
    for t, s in enumerate(spy):
        z = gswg.uniforms_reference(b, Z, 5, t, gswg.TAG_T).astype(np.float64)
        after = spy[t + 1]["W"] if t + 1 < len(spy) else final
        step = {}
        for dt in (torch.float64, torch.float32):
            g = R.backward(s["W"], z, s["Ct"], s["Theta"], dt)["grads"]
            step[dt] = R.adam_step(s["W"], g, mom[dt][0], mom[dt][1], t, 1e-3, 1e-5, dt)
        for n in R.KEYS:
            err = np.abs(after[n] - step[torch.float64][n]).max()
            tol = max(T_PARAM, 4 * np.abs(step[torch.float32][n] - step[torch.float64][n]).max())
            print("lockstep step %d %s: err %.3g allowed %.3g" % (t, n, err, tol))
            assert err <= tol, (t, n, err, tol)
            assert np.abs(after[n] - s["W"][n]).max() > 1e-5              # and it moved
    assert np.array_equal(spy[0]["W"]["G.linear.weight"], W0["G.linear.weight"])


# ---- determinism ----------------------------------------------------------------------------------------------------
def _trained_small(epochs=1, cls=None, use_graph=True, n_train=96, I=64, H=48, Z=8, batch=32, its=None, **kw):
    its = its or loaders(batch, n_train, 48, 48, I)
    m, _ = make_model(I, H, Z)
    kw.setdefault("num_projections", 50)
    tr = (cls or swg.SWGTrainer)(m, *its, **kw)
    tr.use_graph = use_graph
    quiet(tr.train, epochs)
    return tr, m, its


def snapshot(tr, m):
    return (list(tr.losses), tr.best_val_loss, {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state())


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1]
    assert torch.equal(a[3], b[3])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_bitwise_reproducibility_graph_eager_and_resume(tmp_path):
    cfg = dict(n_train=300, batch=64)                       # 300 rows, bs 64: four full batches and one of 44
    runs = []
    for use_graph in (True, True, False):                   # graph twice, then eager
        torch.manual_seed(99)
        tr, m, _ = _trained_small(epochs=2, use_graph=use_graph, **cfg)
        runs.append(snapshot(tr, m))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    assert len(runs[0][0]) == 10 and all(math.isfinite(v) for v in runs[0][0])
    # 1 epoch + checkpoint + a fresh trainer's resumed epoch == 2 epochs
    torch.manual_seed(99)
    tr, m, its = _trained_small(epochs=1, **cfg)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    conf = ck["optim"]["config"]
    assert conf["num_projections"] == 50 and conf["seed"] == 0
    assert ck["history"]["noise_steps"] == 5 and len(ck["history"]["losses"]) == 5
    m2 = swg.SWG(64, 48, 8).to(DEV)
    tr2 = swg.SWGTrainer(m2, *its, num_projections=50)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == 5 and tr2.losses == runs[0][0][:5]
    quiet(tr2.train, 1)
    same(snapshot(tr2, m2), runs[0])
    # other settings: refused under strict, taken otherwise
    for kw in (dict(num_projections=51), dict(num_projections=50, seed=1)):
        t3 = swg.SWGTrainer(swg.SWG(64, 48, 8).to(DEV), *its, **kw)
        t3.load_checkpoint(path)
        with pytest.raises(GMError, match="different settings"):
            t3.train(1)
    t3 = swg.SWGTrainer(swg.SWG(64, 48, 8).to(DEV), *its, num_projections=51)
    t3.load_checkpoint(path, strict=False)
    quiet(t3.train, 1)


# ---- paths ----------------------------------------------------------------------------------------------------------
class Mine(swg.SWGTrainer):
    def compute_batch(self, batch):
        return super().compute_batch(batch)


def test_general_path_gradients_agree_with_the_fused_run(spy):
    """One batch of 67 rows at lr = 0 on both paths, on the same noise: autograd's .grad against the engine's flat
    gradient within the gradient bound (1.5e-6 of max-abs, or 4 x the fp32 CPU deviation), the two losses within the loss
    bound.  Measured on an MI355X: both paths within 1.4e-7 of the fp64 gradients, and bit for bit equal to each other."""
    I, H, Z, b, P = 130, 24, 6, 67, 33
    grads, losses = {}, {}
    for cls in (swg.SWGTrainer, Mine):
        its = loaders(b, b, b, 16, I, binary=False)
        m, W = make_model(I, H, Z)
        tr = cls(m, *its, num_projections=P, seed=3)
        tr.use_graph = False
        torch.manual_seed(99)
        quiet(tr.train, 1, lr=0.0, weight_decay=0.0)
        assert (tr._engine is None) == (cls is Mine) and len(tr.losses) == 1
        if cls is Mine:
            grads[cls] = {n: p.grad.detach().cpu().double().numpy() for n, p in m.named_parameters()}
        else:
            grads[cls] = spy[0]["grad"]
        losses[cls] = tr.losses[0]
    s = spy[0]
    z = gswg.uniforms_reference(b, Z, 3, 0, gswg.TAG_T).astype(np.float64)
    back, b32 = R.backward(W, z, s["Ct"], s["Theta"]), R.backward(W, z, s["Ct"], s["Theta"], torch.float32)
    ref = R.sw_reference(s["Pr"][:, :b], s["Pr"][:, b:])
    f32 = R.sw_reference(s["Pr32"][:, :b], s["Pr32"][:, b:], np.float32)
    for cls, nm in ((swg.SWGTrainer, "fused"), (Mine, "general")):
        check("paths", nm + " loss", losses[cls], ref["swd2"], f32["swd2"], T_LOSS)
        for n in R.KEYS:
            check("paths", "%s %s" % (nm, n), grads[cls][n], back["grads"][n], b32["grads"][n])
    for n in R.KEYS:                                        # the two paths against each other, the same allowance
        check("paths", "general vs fused " + n, grads[Mine][n], grads[swg.SWGTrainer][n],
              grads[swg.SWGTrainer][n] + (b32["grads"][n] - back["grads"][n]))


def test_sw_loss_function_gradient_and_refusals():
    N, M, I, P = 33, 31, 50, 17
    g = torch.Generator().manual_seed(4)
    X, Y = torch.rand(N, I, generator=g), torch.rand(M, I, generator=g)
    th = torch.empty(P, I, device=DEV)
    ops_fused.sw_directions(th, ops_fused.sw_noise(2, gswg.TAG_DT))
    xs = X.to(DEV).requires_grad_(True)
    loss = ops_fused.sw_loss(xs, Y.to(DEV), th)
    (3.0 * loss).backward()
    Pr = torch.empty(P, N + M, device=DEV)
    ops.linear_fwd(th, torch.cat([X, Y]).to(DEV), None, Pr, "id")        # the same launch: the same bits
    pr = Pr.cpu().numpy()
    ref = R.sw_reference(pr[:, :N].astype(np.float64), pr[:, N:].astype(np.float64))
    f32 = R.sw_reference(pr[:, :N], pr[:, N:], np.float32)
    th64 = th.cpu().double().numpy()
    check("sw_loss", "loss", loss.item(), ref["swd2"], f32["swd2"], T_LOSS)
    check("sw_loss", "dX", xs.grad.cpu().numpy(), 3.0 * ref["Ct"].T @ th64,
          3.0 * (f32["Ct"].T @ th64.astype(np.float32)))
    with pytest.raises(GMError, match="samples only"):
        ops_fused.sw_loss(X.to(DEV), Y.to(DEV).requires_grad_(True), th)
    with pytest.raises(GMError):
        ops_fused.sw_loss(X, Y, th)                         # host tensors: no CPU fallback


# ---- sampling and the score -----------------------------------------------------------------------------------------
def test_sample_is_reproducible_and_independent_of_n():
    tr, m, _ = _trained_small()
    st, mode = torch.get_rng_state(), m.training
    a, b, c, d = tr.sample(40, seed=5), tr.sample(40, seed=5), tr.sample(17, seed=5), tr.sample(40, seed=6)
    assert torch.equal(torch.get_rng_state(), st) and m.training == mode  # the global generator is untouched
    assert a.shape == (40, 64) and torch.equal(a, b) and not torch.equal(a, d)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    assert torch.equal(a[:17], c)                           # row r depends on (seed, r) alone: whole blocks, whatever n
    e = tr.sample(1030, seed=5)                             # past one block
    assert e.shape == (1030, 64) and torch.equal(e[:40], a) and torch.equal(e[1024:], tr.sample(1100, seed=5)[1024:1030])
    z = tr.prior(40, 0, gswg.TAG_S, seed=5)
    assert np.array_equal(z.cpu().numpy(), gswg.uniforms_reference(40, 8, 5, 0, gswg.TAG_S))
    for bad in (0, -1, 1.5, True):
        with pytest.raises(swg.SWGError):
            tr.sample(bad)
    res = tr.swd(n_samples=40, n_projections=20, seed=5)
    assert type(res).__name__ == "SWDResult" and (res.n_projections, res.n_samples, res.n_data) == (20, 40, 48)
    assert math.isfinite(res.swd2) and res.swd == math.sqrt(res.swd2)
    assert type(tr.mmd(n_samples=40, seed=5)).__name__ == "MMDResult"
    with pytest.raises(GMError):
        tr.log_likelihood()


def test_metrics_sliced_wasserstein_vs_reference_and_ordering():
    N, M, I, P = 300, 170, 50, 300                          # two blocks of projections: 256 and 44
    g = torch.Generator().manual_seed(8)
    X, Y = (0.7 * torch.rand(N, I, generator=g) + 0.1).to(DEV), torch.rand(M, I, generator=g).to(DEV)
    res = metrics.sliced_wasserstein(X, Y, n_projections=P, seed=4)
    th = torch.empty(P, I, device=DEV)                      # the same launches again: the metric's own projection bits
    Pr = torch.empty(P, N + M, device=DEV)
    Rr = torch.cat([X, Y]).contiguous()
    for p0 in range(0, P, 256):
        k = min(256, P - p0)
        ops_fused.sw_directions(th[p0:p0 + k], ops_fused.sw_noise(4, gswg.TAG_DM, row0=p0))
        ops.linear_fwd(th[p0:p0 + k], Rr, None, Pr[p0:p0 + k], "id")
    whole = torch.empty(P, I, device=DEV)
    ops_fused.sw_directions(whole, ops_fused.sw_noise(4, gswg.TAG_DM))
    assert torch.equal(whole, th)                           # the blocks are rows of one stream
    pr = Pr.cpu().numpy()
    ref = R.sw_reference(pr[:, :N].astype(np.float64), pr[:, N:].astype(np.float64))
    f32 = R.sw_reference(pr[:, :N], pr[:, N:], np.float32)
    check("metrics.swd", "swd2", res.swd2, ref["swd2"], f32["swd2"], T_LOSS)
    assert (res.n_projections, res.n_samples, res.n_data) == (P, N, M) and res.swd == math.sqrt(res.swd2)
    assert res == metrics.sliced_wasserstein(X, Y, n_projections=P, seed=4)
    assert res.swd2 != metrics.sliced_wasserstein(X, Y, n_projections=P, seed=5).swd2
    zero = metrics.sliced_wasserstein(Y, Y, n_projections=64)
    assert zero.swd2 == 0.0 and zero.swd == 0.0             # samples is data: exactly 0
    g = torch.Generator().manual_seed(3)
    x = torch.rand(400, I, generator=g).to(DEV)
    near = metrics.sliced_wasserstein(x[:200], x[200:], n_projections=128)
    far = metrics.sliced_wasserstein(x[:200], (x[200:] * 0.9 + 0.1).contiguous(), n_projections=128)
    print("swd2 near %.3g far %.3g" % (near.swd2, far.swd2))
    assert 0.0 < near.swd2 < far.swd2
    for bad in (dict(n_projections=0), dict(n_projections=8193), dict(seed=-1)):
        with pytest.raises(GMError):
            metrics.sliced_wasserstein(x[:5], x[5:10], **bad)
    with pytest.raises(GMError, match="radix"):
        metrics.sliced_wasserstein(torch.zeros(16385, 2, device=DEV), x[:5, :2].contiguous())


def test_gan_trainer_swd_on_an_untrained_nsgan():
    import ns_gan
    its = loaders(16, 64, 48, 48, 64)
    torch.manual_seed(1)
    tr = ns_gan.NSGANTrainer(ns_gan.NSGAN(image_size=64, hidden_dim=48, z_dim=8), *its)
    res = tr.swd(n_samples=50, n_projections=40, seed=2)
    assert type(res).__name__ == "SWDResult" and (res.n_projections, res.n_samples, res.n_data) == (40, 50, 48)
    assert res.swd2 > 0 and res == tr.swd(n_samples=50, n_projections=40, seed=2)
    g = swg.SWG(64, 48, 8)                                  # the generator's weights load into an SWG
    missing = g.load_state_dict(tr.model.state_dict(), strict=False)
    assert not missing.missing_keys and all(k.startswith("D.") for k in missing.unexpected_keys)


# ---- learning check -------------------------------------------------------------------------------------------------
def test_learning_on_bands():
    """The 16 band patterns tests/test_gpu_gmmn.py learns on (16 x 16 images, two adjacent rows or columns lit): over 320
    batches of 64 with 256 directions the validation loss (evaluate() on the validation streams, taken after the first
    epoch and after every 5 more) falls below the first epoch's, and the swd2 of 2 000 samples against the held-out rows
    is below the untrained generator's.  Observed on an MI355X: training loss 0.2261 (first 10 batches) -> 0.0345 (last
    10); validation loss 0.1897 after the first epoch, then 0.0851, 0.0575, 0.0411, 0.0327 (a margin of 0.157 below the
    first epoch's, 5.8x); swd2 0.2286 untrained -> 0.0313 trained."""
    def bands(reps):
        x = torch.zeros(16 * reps, 1, 16, 16)
        for i in range(16 * reps):
            k = i % 16
            j = 2 * (k % 8)
            if k < 8:
                x[i, 0, j:j + 2, :] = 1.0
            else:
                x[i, 0, :, j:j + 2] = 1.0
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(16 * reps, dtype=torch.int64)),
                                           batch_size=64, shuffle=True)
    its = bands(64), bands(16), bands(16)
    torch.manual_seed(5)
    tr = swg.SWGTrainer(swg.SWG(256, 128, 8), *its, num_projections=256, seed=0)
    before = tr.swd(n_samples=2000, n_projections=256, seed=1)

    def val():
        tr.model.eval()
        return float(tr.evaluate(tr.val_iter))
    quiet(tr.train, 1)
    vals = [val()]
    for n in (4, 5, 5, 5):
        quiet(tr.train, n)
        vals.append(val())
    assert type(tr._engine).__name__ == "SWGEngine"
    assert len(tr.losses) == 320 and all(math.isfinite(v) for v in tr.losses)
    after = tr.swd(n_samples=2000, n_projections=256, seed=1)
    first, last = np.mean(tr.losses[:10]), np.mean(tr.losses[-10:])
    print("learning: training loss first 10 %.5f last 10 %.5f; validation loss after 1 / 5 / 10 / 15 / 20 epochs %s; swd2 "
          "untrained %.5f trained %.5f" % (first, last, " ".join("%.5f" % v for v in vals), before.swd2, after.swd2))
    assert last < first and vals[-1] < vals[0] and after.swd2 < before.swd2
