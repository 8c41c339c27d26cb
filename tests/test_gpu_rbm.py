"""The restricted Boltzmann machine on the MI355X: the uniform kernel against the numpy rule bit for bit, the one-launch
Gibbs chain against the fp64 reference and the fp32 pinned-order restatement, its independence of the work mapping, the
gradient, visible-bias and transpose kernels, one engine batch's gradients and whole runs against an fp64 oracle fed the
device's own chain states, bitwise reproducibility (graph, eager, resume, PCD chains), the general path, annealed
importance sampling against the exact partition function of small RBMs, and learning itself.
tests/rbm_reference.py is the reference of every comparison; the code under test never is."""
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

import rbm  # noqa: E402
import rbm_reference as R  # noqa: E402
from generative_models_amd import metrics, ops  # noqa: E402
from generative_models_amd import rbm as grbm  # noqa: E402
from generative_models_amd import ops_fused as of_  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- gm_rbm_uniform ------------------------------------------------------------------------------------------------------
def test_uniform_kernel_is_the_numpy_rule():
    for tag in (R.TAG_D, R.TAG_H, R.TAG_V):
        for n, w, seed, t, row0 in [(5, 49, 0, 0, 0), (37, 784, (1 << 64) - 1, 7, 3), (300, 10, 0x123456789ABCDEF, 1 << 31,
                                                                                    1 << 20), (3, 1024, 9, 2, 0), (4, 1, 1, 5, 1)]:
            u = of_.rbm_uniform(n, w, seed, tag, step=t, row0=row0, device=DEV).cpu().numpy()
            assert u.tobytes() == R.uniforms(n, w, seed, tag, t, row0).tobytes(), (tag, n, w)
    # the step is counter + base + addend, as a captured graph reads it
    ctr, base = torch.tensor([5], device=DEV), torch.tensor([100], device=DEV)
    u = of_.rbm_uniform(4, 9, 3, R.TAG_H, step=2, step_ctr=ctr, step_base=base, device=DEV).cpu().numpy()
    assert u.tobytes() == R.uniforms(4, 9, 3, R.TAG_H, 107).tobytes()


# ---- gm_rbm_chain --------------------------------------------------------------------------------------------------------
def device_chain(W, c, b, x, steps, seed, **kw):
    """The kernel's outputs as numpy arrays (v0, v, p, a), the rows beyond n and the columns beyond I untouched."""
    n, I = x.shape
    Wd = T(W)
    WT = of_.rbm_transpose(Wd, torch.empty(I, W.shape[0], device=DEV))
    outs = {k: torch.full((n + 1, I + 3), -7.0, device=DEV) for k in ("v0", "v", "p", "a")}
    of_.rbm_chain(Wd, WT, T(c), T(b), T(x), steps, seed, n=n, v0_out=outs["v0"][:, :I], v_out=outs["v"][:, 1:1 + I],
                  p_out=outs["p"][:, 2:2 + I], a_out=outs["a"][:, 3:3 + I], **kw)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in outs.items()}
    for k, off in (("v0", 0), ("v", 1), ("p", 2), ("a", 3)):
        pad = np.ones(I + 3, bool)
        pad[off:off + I] = False
        assert np.all(host[k][:, pad] == -7.0) and np.all(host[k][n] == -7.0), k       # nothing out of its rows
        host[k] = host[k][:n, off:off + I]
    return host


@pytest.fixture(scope="module")
def chain_refs():
    out = {}
    for case, (n, I, H, steps, seed) in R.CHAIN_CASES.items():
        W, c, b = R.case_weights(I, H, seed)
        x = R.case_input(n, I, seed)
        kw = dict(row0=3, dstep=5, g0=11)
        out[case] = (W, c, b, x, R.chain(W, c, b, x, steps, seed, **kw),
                     R.chain(W, c, b, x, steps, seed, dtype=np.float32, **kw))
    return out


@pytest.mark.parametrize("case", list(R.CHAIN_CASES))
def test_chain_against_fp64_and_the_pinned_fp32_restatement(case, chain_refs):
    """Every decided row: v0, v and the final h (implied by the logits: a_out is b plus the W rows of the lit hidden
    units, so equal logits to the restatement's mean equal h) are the fp64 reference's exactly; p_out within STEP_TOL of
    fp64.  Against the fp32 restatement with the pinned sum order a_out is EXACT: the logit of an untempered chain is a
    sum of fp32 adds in a pinned order and involves no expf, so the bound is 0 ulp (the restatement itself is within
    1e-4 of fp64 on these cases, tests/test_rbm_cpu.py::test_chain_cases_are_decided)."""
    n, I, H, steps, seed = R.CHAIN_CASES[case]
    W, c, b, x, r64, r32 = chain_refs[case]
    d = device_chain(W, c, b, x, steps, seed, row0=3, d_add=5, g_add=11)
    ok = ~(r64["und"] | r32["und"])
    print(case, "decided rows", int(ok.sum()), "of", n)
    assert (~ok).sum() <= R.UNDECIDED_SHARE.get(case, 0.0) * n
    assert np.array_equal(d["v0"], r64["v0"].astype(np.float32))                 # the binarisation: every row
    assert np.array_equal(d["v"][ok], r64["v"][ok].astype(np.float32))
    perr = np.abs(d["p"].astype(np.float64) - r64["p"])[ok].max()
    aerr = np.abs(d["a"].astype(np.float64) - r32["a"].astype(np.float64))[ok].max()
    print("p err vs fp64", perr, "a err vs fp32 restatement", aerr)
    assert perr <= R.STEP_TOL
    assert np.array_equal(d["a"][ok], r32["a"][ok])
    # the final h, recovered from the logits: a - b = W^T h in fp64 within the sum's rounding, solved row by row
    h64 = r64["h"][ok].astype(np.float64)
    assert np.abs((d["a"][ok].astype(np.float64) - b[None, :]) - h64 @ W.astype(np.float64)).max() <= 1e-4
    assert set(np.unique(d["v"])) <= {0.0, 1.0} and set(np.unique(d["v0"])) <= {0.0, 1.0}


@pytest.mark.parametrize("case", ["5x49x32", "9x70x70", "8x784x400"])
def test_chain_does_not_depend_on_the_work_mapping(case, chain_refs):
    """One k-step launch == k one-step launches with the Gibbs addend advanced (v fed back in: binarising 0 / 1 rows is
    the identity); rows are independent of n and row0; steps = 0 returns exactly the binarisation, and {0, 1} input."""
    n, I, H, steps, seed = R.CHAIN_CASES[case]
    W, c, b, x, r64, _ = chain_refs[case]
    whole = device_chain(W, c, b, x, steps, seed, row0=3, d_add=5, g_add=11)
    cur = device_chain(W, c, b, x, 0, seed, row0=3, d_add=5)["v"]
    assert np.array_equal(cur, whole["v0"]) and np.array_equal(cur, r64["v0"].astype(np.float32))
    for s in range(steps):
        one = device_chain(W, c, b, cur, 1, seed, row0=3, d_add=99, g_add=11 + s)
        assert np.array_equal(one["v0"], cur)                    # {0, 1} input passes the binarisation unchanged
        cur = one["v"]
    for k in ("v", "p", "a"):
        assert one[k].tobytes() == whole[k].tobytes(), k
    # the device counter and base do what the addends do, g_mul scaling the Gibbs part
    ctr, base = torch.tensor([2], device=DEV), torch.tensor([1], device=DEV)
    via = device_chain(W, c, b, x, steps, seed, row0=3, step_ctr=ctr, step_base=base, d_add=2, g_mul=3, g_add=2)
    for k in ("v0", "v", "p", "a"):
        assert via[k].tobytes() == whole[k].tobytes(), k
    # rows 2 .. alone, as chain rows 5 ..: the same bits as inside the whole launch
    part = device_chain(W, c, b, x[2:], steps, seed, row0=5, d_add=5, g_add=11)
    for k in ("v0", "v", "p", "a"):
        assert part[k].tobytes() == whole[k][2:].tobytes(), k
    # in place: v_out may be x itself
    xd = T(whole["v0"])
    Wd = T(W)
    WT = of_.rbm_transpose(Wd, torch.empty(I, H, device=DEV))
    of_.rbm_chain(Wd, WT, T(c), T(b), xd, steps, seed, v_out=xd, row0=3, d_add=5, g_add=11)
    assert np.array_equal(xd.cpu().numpy(), whole["v"])


# ---- the small kernels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,I,H", R.GRAD_CASES)
def test_grad_and_vbias_kernels_against_fp64(B, I, H):
    W, c, b = R.case_weights(I, H, B)
    g = np.random.RandomState(B)
    V = (g.random_sample((2 * B, I)) < 0.4).astype(np.float32)
    pre64 = V.astype(np.float64) @ W.astype(np.float64).T + c[None, :]
    pre = pre64.astype(np.float32)
    inv_b = float(np.float32(1.0 / B))
    dA, part = torch.full((2 * B + 1, H + 2), -7.0, device=DEV), torch.zeros(2 * B + 1, device=DEV)
    Vd = torch.zeros(2 * B, I + 1, device=DEV)
    Vd[:, :I] = T(V)
    of_.rbm_grad(T(pre), Vd[:, :I], T(b), dA[:, :H], part, B, inv_b)
    sign = np.where(np.arange(2 * B) < B, -1.0, 1.0)[:, None]
    ref = sign * R.sigmoid(pre.astype(np.float64)) * inv_b
    err = np.abs(dA[:2 * B, :H].cpu().numpy() - ref).max()
    print("dA err / scale", err / np.abs(ref).max())
    assert err <= R.GRAD_TOL * np.abs(ref).max()
    assert torch.all(dA[2 * B] == -7.0) and torch.all(dA[:, H:] == -7.0) and part[2 * B].item() == 0.0
    F = -(V.astype(np.float64) @ b) - R.softplus(pre.astype(np.float64)).sum(1)
    F[B:] *= -1.0
    rel = (np.abs(part[:2 * B].cpu().numpy() - F) / np.maximum(1.0, np.abs(F))).max()
    print("free-energy row err", rel)
    assert rel <= R.LOSS_TOL
    res = torch.zeros(1, device=DEV)
    of_.sum_finalize(part, 2 * B, res, scale=inv_b)
    gap = R.cd_grads(W, c, b, V[:B], V[B:])[0]
    # the partials were formed from the fp32 pre-activations: allow the gap their rounding, LOSS_TOL of the energies' scale
    assert abs(res.item() - gap) <= R.LOSS_TOL * max(1.0, np.abs(F).max())
    # the visible bias: the gradient alone, then with Adam's step in the launch against fp64 Adam
    gb = torch.zeros(I, device=DEV)
    of_.rbm_vbias(Vd[:, :I], B, I, inv_b, g=gb)
    ref_g = (V[B:].astype(np.float64) - V[:B]).sum(0) * inv_b
    assert np.abs(gb.cpu().numpy() - ref_g).max() <= R.GRAD_TOL * np.abs(ref_g).max()
    sched = T(ops.adam_schedule(1e-2, 3))
    p, m, v = T(b.copy()), torch.zeros(I, device=DEV), torch.zeros(I, device=DEV)
    P, M, Vv = {"b": b.astype(np.float64)}, {"b": np.zeros(I)}, {"b": np.zeros(I)}
    for step in (1, 2, 3):
        of_.rbm_vbias(Vd[:, :I], B, I, inv_b, adam=dict(p=p, m=m, v=v, sched=sched, sched_slot=ops.slot(add=step - 1)),
                      weight_decay=1e-3)
        R.adam_step(P, {"b": ref_g}, M, Vv, step, 1e-2, wd=1e-3)
    assert np.abs(p.cpu().numpy() - P["b"]).max() <= R.PARAM_TOL
    assert np.abs(m.cpu().numpy() - M["b"]).max() <= R.GRAD_TOL * np.abs(M["b"]).max()
    # and against the flat Adam kernel on the same gradient: the same bits
    p2, m2, v2 = T(b.copy()), torch.zeros(I, device=DEV), torch.zeros(I, device=DEV)
    for step in (1, 2, 3):
        ops.adam(p2, gb, m2, v2, sched, ops.slot(add=step - 1), weight_decay=1e-3)
    assert torch.equal(p, p2) and torch.equal(m, m2) and torch.equal(v, v2)


@pytest.mark.parametrize("I,H", R.TRANSPOSE_CASES)
def test_transpose_kernel_is_a_bit_copy(I, H):
    g = np.random.RandomState(I)
    W = g.standard_normal((H, I)).astype(np.float32)
    W.view(np.uint32)[0, :3] = [0x7FC00001, 0x80000000, 0x00000001]               # a NaN payload, -0, a denormal
    Wd = T(W)
    WT = of_.rbm_transpose(Wd, torch.empty(I, H, device=DEV))
    assert WT.cpu().numpy().view(np.uint32).tobytes() == np.ascontiguousarray(W.T).view(np.uint32).tobytes()
    big_w, big_t = torch.full((H + 1, I + 5), -7.0, device=DEV), torch.full((I + 1, H + 3), -7.0, device=DEV)
    big_w[:H, 2:2 + I] = Wd
    of_.rbm_transpose(big_w[:H, 2:2 + I], big_t[:I, 1:1 + H])
    got = big_t.cpu().numpy()
    assert got[:I, 1:1 + H].view(np.uint32).tobytes() == np.ascontiguousarray(W.T).view(np.uint32).tobytes()
    assert np.all(got[I] == -7.0) and np.all(got[:, 0] == -7.0) and np.all(got[:, 1 + H:] == -7.0)


# ---- loaders, models, runs ---------------------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, shape, seed=7, binary=True):
    g = torch.Generator().manual_seed(seed)
    I = shape[0] * shape[1]

    def mk(n):
        x = torch.bernoulli(torch.full((n, I), 0.3), generator=g) if binary else torch.rand(n, I, generator=g)
        ds = torch.utils.data.TensorDataset(x.view(n, 1, *shape), torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


SMALL = dict(I=49, H=32, shape=(7, 7), batch=16, n_train=5 * 16 + 7, n_val=40, n_test=24, binary=False)
FULL = dict(I=784, H=400, shape=(28, 28), batch=512, n_train=3 * 512 + 336, n_val=512 + 100, n_test=64, binary=True)


def mk_loaders(cfg):
    return loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["shape"], binary=cfg["binary"])


def mk_model(cfg):
    torch.manual_seed(1234)
    m = rbm.RBM(cfg["I"], cfg["H"])
    with torch.no_grad():
        m.vbias.normal_(0.0, 0.1)
    return m


def product(cfg, its, epochs, use_graph=True, trainer_cls=None, model=None, k=1, mode="cd", seed=3, **kw):
    m = mk_model(cfg) if model is None else model
    tr = (trainer_cls or rbm.RBMTrainer)(m, *its, seed=seed, k=k, mode=mode)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs, **kw)
    torch.cuda.synchronize()
    return tr, m


@contextlib.contextmanager
def recorded_batches():
    """The engine's batches, eager: after each one the stacked chain states (training) or the one-step logits and the
    binarised rows (validation), as the device left them -- the oracle's input, in the role device_rows plays for
    MADE."""
    log = {"train": [], "val": [], "x": []}
    orig = grbm.RBMEngine._issue

    def issue(self, st, t, b, train, pos=0, of=1):
        orig(self, st, t, b, train, pos=pos, of=of)
        torch.cuda.synchronize()
        if train:
            log["train"].append(self.V[:2 * b].cpu().double().numpy())
            log["x"].append(self.X[:b].cpu().numpy())
        else:
            log["val"].append((self.A[:b].cpu().double().numpy(), self.Vv[:b].cpu().double().numpy()))
    grbm.RBMEngine._issue = issue
    try:
        yield log
    finally:
        grbm.RBMEngine._issue = orig


def oracle(init, states, lr=1e-3, wd=0.0):
    """RBMTrainer's optimisation in fp64 on the recorded chain states: (losses, final weights)."""
    P = {k: init[k].double().numpy().copy() for k in ("linear.weight", "linear.bias", "vbias")}
    M, V = {k: np.zeros_like(v) for k, v in P.items()}, {k: np.zeros_like(v) for k, v in P.items()}
    losses = []
    for step, S in enumerate(states, 1):
        b = S.shape[0] // 2
        loss, dW, dc, db = R.cd_grads(P["linear.weight"], P["linear.bias"], P["vbias"], S[:b], S[b:])
        losses.append(loss)
        R.adam_step(P, {"linear.weight": dW, "linear.bias": dc, "vbias": db}, M, V, step, lr, wd)
    return losses, P


def lclose(got, ref, tol=R.LOSS_TOL):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    print("loss err", err.max())
    assert err.max() <= tol, (err.max(), got[:4], ref[:4])


@pytest.mark.parametrize("cfg", [dict(SMALL, n_train=16), dict(FULL, n_train=512)], ids=["16x49x32", "512x784x400"])
def test_teacher_forced_batch_gradients_vs_fp64(cfg):
    """One engine batch from known weights: the dW, dc and db it leaves in the flat gradient buffer against the fp64 CD
    gradient on the device's own v0 / vk, within 1.5e-6 of each tensor's scale."""
    its = mk_loaders(cfg)
    m = mk_model(cfg)
    init = {k: v.clone() for k, v in m.state_dict().items()}
    with recorded_batches() as log:
        tr, m = product(cfg, its, 1, use_graph=False, model=m)
    assert len(log["train"]) == 1 and len(tr.losses) == 1
    S = log["train"][0]
    b = cfg["batch"]
    assert set(np.unique(S)) <= {0.0, 1.0} and S.shape == (2 * b, cfg["I"])
    loss, dW, dc, db = R.cd_grads(init["linear.weight"].numpy(), init["linear.bias"].numpy(), init["vbias"].numpy(),
                                  S[:b], S[b:])
    fp = tr._engine.fp
    got = [g.cpu().double().numpy() for g in fp.gviews]
    print("gap", tr.losses[0], loss)
    assert abs(tr.losses[0] - loss) <= R.LOSS_TOL * max(1.0, abs(loss))
    for name, gk, ref in zip(("dW", "dc", "db"), got, (dW, dc, db)):
        scale = np.abs(ref).max()
        assert scale > 0, name
        err = np.abs(gk - ref).max()
        print(name, "grad err / scale", err / scale)
        assert err <= R.GRAD_TOL * scale, (name, err, scale)


@pytest.mark.parametrize("k,mode", [(1, "cd"), (3, "cd"), (1, "pcd")], ids=["cd1", "cd3", "pcd1"])
@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["49-32-b16-fp32", "784-400-b512-bits"])
def test_engine_vs_fp64_oracle(cfg, k, mode):
    """An epoch (the last batch ragged) against fp64 Adam on the device's own chain states: per-batch losses within
    LOSS_TOL, weights within 5e-5; the
    chain states themselves are the fp64 chain's under the weights of their batch for all but undecided rows."""
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    m = mk_model(cfg)
    init = {k_: v.clone() for k_, v in m.state_dict().items()}
    with recorded_batches() as log:
        tr, m = product(cfg, its, 1, use_graph=False, model=m, k=k, mode=mode)
    nb = len(its[0])
    assert len(log["train"]) == nb == len(tr.losses) and log["train"][-1].shape[0] == 2 * (cfg["n_train"] % cfg["batch"])
    losses, P = oracle(init, log["train"])
    print("losses", tr.losses[:3], losses[:3])
    lclose(tr.losses, losses)
    worst = {n: np.abs(m.state_dict()[n].cpu().double().numpy() - P[n]).max() for n in P}
    print("max |w - oracle|", worst)
    assert max(worst.values()) <= R.PARAM_TOL, worst
    # validation: the reported number is the Bernoulli cross-entropy of the recorded logits against the binarised rows
    ce = np.mean([(R.softplus(a) - v0 * a).sum(1).mean() for a, v0 in log["val"]])
    assert abs(tr.recon_loss[-1] - ce) <= R.LOSS_TOL * max(1.0, ce) and len(log["val"]) == len(its[1])
    # the first batch's chain: the fp64 chain under the initial weights from the rows the batch gathered
    b = cfg["batch"]
    x = log["x"][0]
    data = its[0].dataset.tensors[0].reshape(-1, cfg["I"]).numpy()
    assert all((data == row).all(1).any() for row in x[:4])     # rows of the training set
    W, c, bv = (init[n].numpy() for n in ("linear.weight", "linear.bias", "vbias"))
    S = log["train"][0]
    if mode == "cd":
        r = R.chain(W, c, bv, x, k, 3, dstep=0, g0=0)
        ok = ~r["und"]
        assert np.array_equal(S[:b], r["v0"].astype(np.float64)) and ok.mean() >= 0.9
        assert np.array_equal(S[b:][ok], r["v"][ok].astype(np.float64))
    else:
        v0 = R.chain(W, c, bv, x, 0, 3, dstep=0)["v0"]
        r = R.chain(W, c, bv, v0.astype(np.float32), k, 3, dstep=0, g0=0)
        ok = ~r["und"]
        assert np.array_equal(S[:b], v0.astype(np.float64)) and np.array_equal(S[b:][ok], r["v"][ok].astype(np.float64))
        # the chains persist: the second batch's negative rows are not its data's binarisation
        assert not np.array_equal(log["train"][1][b:], log["train"][1][:b])
    assert type(tr._engine).__name__ == "RBMEngine"
    assert type(tr._device_data(tr.train_iter)).__name__ == ("PackedData" if cfg["binary"] else "Tensor")


def snapshot(tr, m):
    eng = tr._engine
    return (list(tr.losses), list(tr.recon_loss), {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state(), eng.fp.m.cpu().clone(), eng.fp.v.cpu().clone(), eng.P.cpu().clone(), tr.noise_steps)


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[7] == b[7]
    for i in (3, 4, 5, 6):
        assert torch.equal(a[i], b[i]), i
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


@pytest.mark.parametrize("k,mode", [(2, "cd"), (1, "pcd")], ids=["cd2", "pcd1"])
def test_bitwise_reproducibility_and_resume(tmp_path, k, mode):
    cfg = SMALL
    runs = []
    for use_graph in (True, True, False):                   # graph twice, then eager
        torch.manual_seed(99)
        runs.append(snapshot(*product(cfg, mk_loaders(cfg), 2, use_graph=use_graph, k=k, mode=mode)))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    assert (runs[0][6].abs().sum().item() > 0) == (mode == "pcd")
    # train(1) + save + load into a fresh trainer + train(1) == train(2): Adam's steps, the shuffles, the noise steps
    # and the persistent chains continue
    for use_graph in (True, False):
        torch.manual_seed(99)
        its = mk_loaders(cfg)
        tr, m = product(cfg, its, 1, use_graph=use_graph, k=k, mode=mode)
        path = str(tmp_path / ("ck%d.pt" % use_graph))
        tr.save_checkpoint(path)
        m2 = rbm.RBM(cfg["I"], cfg["H"]).to(DEV)
        tr2 = rbm.RBMTrainer(m2, *its, seed=3, k=k, mode=mode)
        tr2.use_graph = use_graph
        tr2.load_checkpoint(path)
        with contextlib.redirect_stdout(io.StringIO()):
            tr2.train(1)
        torch.cuda.synchronize()
        same(snapshot(tr2, m2), runs[0])
    # a checkpoint of another k, mode or seed is refused under strict=True
    for kw in (dict(k=k + 1, mode=mode, seed=3), dict(k=k, mode="pcd" if mode == "cd" else "cd", seed=3),
               dict(k=k, mode=mode, seed=4)):
        t3 = rbm.RBMTrainer(rbm.RBM(cfg["I"], cfg["H"]).to(DEV), *its, **kw)
        t3.load_checkpoint(path)
        with pytest.raises(GMError):
            t3.train(1)


@pytest.mark.parametrize("k,mode", [(2, "cd"), (1, "pcd")], ids=["cd2", "pcd1"])
def test_general_path_agrees_with_the_fused_run(k, mode):
    """A trainer with an overridden hook trains on the general path -- autograd of the gap, the chain composed from
    torch operations on gm_rbm_uniform's uniforms: losses and weights agree with the fused run to the oracle's bounds."""
    cfg = SMALL

    class Mine(rbm.RBMTrainer):
        def compute_batch(self, batch, train=True):
            return super().compute_batch(batch, train)
    torch.manual_seed(99)
    fused, mf = product(cfg, mk_loaders(cfg), 1, k=k, mode=mode)
    torch.manual_seed(99)
    gen, mg = product(cfg, mk_loaders(cfg), 1, trainer_cls=Mine, k=k, mode=mode)
    assert gen._engine is None and type(fused._engine).__name__ == "RBMEngine"
    lclose(gen.losses, fused.losses)
    worst = {n: (mf.state_dict()[n] - mg.state_dict()[n]).abs().max().item() for n in mf.state_dict()}
    print("max |fused - general|", worst)
    assert max(worst.values()) <= R.PARAM_TOL
    assert abs(gen.recon_loss[-1] - fused.recon_loss[-1]) <= R.LOSS_TOL * max(1.0, fused.recon_loss[-1])
    # sampling through the general chain: the same bits as the one-launch kernel's on decided rows
    xs, ps = fused.sample(64, seed=5, steps=3, return_probs=True)
    xg, pg = gen.sample(64, seed=5, steps=3, return_probs=True)
    agree = (xs == xg).all(1).float().mean().item()
    print("rows sampled alike", agree)
    assert agree >= 0.9


# ---- annealed importance sampling ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(R.AIS_CASES))
def test_ais_against_the_fp64_restatement_and_the_exact_partition_function(name):
    W, c, b, b_A, seed = R.ais_case(name)
    H, I = W.shape
    n, betas = R.AIS_CHAINS, R.uniform_betas(R.AIS_BETAS)
    x = np.repeat((1.0 / (1.0 + np.exp(-b_A.astype(np.float64)))).astype(np.float32)[None], n, 0)
    Wd = T(W)
    WT = of_.rbm_transpose(Wd, torch.empty(I, H, device=DEV))
    logw = torch.zeros(n + 1, dtype=torch.float64, device=DEV)
    v = torch.empty(n, I, device=DEV)
    of_.rbm_chain(Wd, WT, T(c), T(b), T(x), R.AIS_BETAS - 1, seed, n=n, v_out=v, betas=T(betas), b_A=T(b_A), logw=logw)
    lw = logw.cpu().numpy()
    assert lw[n] == 0.0
    r64 = R.chain(W, c, b, x, R.AIS_BETAS - 1, seed, betas=betas, b_A=b_A)
    ok = ~r64["und"]
    dev = np.abs(lw[:n] - r64["logw"])[ok].max()
    print(name, "decided rows", int(ok.sum()), "log-weight deviation from fp64", dev, "allowed", R.AIS_LOGW_TOL)
    assert ok.sum() >= 0.5 * n and dev <= R.AIS_LOGW_TOL
    assert np.array_equal(v.cpu().numpy()[ok], r64["v"][ok].astype(np.float32))
    log_z, se = R.ais_log_z(lw[:n], b_A, H)
    exact = R.exact_log_z(W, c, b)
    print("log Z", log_z, "+-", se, "exact", exact)
    assert abs(log_z - exact) <= 3 * se
    # the trainer's estimate on the same model: log Z from its own base rate, ll = -F - log Z
    ds = torch.utils.data.TensorDataset(torch.bernoulli(torch.full((64, 1, 1, I), 0.4),
                                                        generator=torch.Generator().manual_seed(1)),
                                        torch.zeros(64, dtype=torch.int64))
    its = [torch.utils.data.DataLoader(ds, batch_size=16, shuffle=True) for _ in range(3)]
    m = rbm.RBM(I, H)
    with torch.no_grad():
        m.linear.weight.copy_(torch.from_numpy(W)), m.linear.bias.copy_(torch.from_numpy(c)), m.vbias.copy_(torch.from_numpy(b))
    tr = rbm.RBMTrainer(m, *its)
    res = tr.log_likelihood(chains=n, betas=R.AIS_BETAS, seed=seed)
    assert isinstance(res, metrics.AISResult) and (res.chains, res.n_betas, res.n) == (n, R.AIS_BETAS, 64)
    assert abs(res.log_z - exact) <= 3 * res.log_z_stderr
    xs = ds.tensors[0].reshape(64, I).numpy()
    assert abs(res.ll_mean - (-R.free_energy(W, c, b, xs) - res.log_z).mean()) <= 1e-4
    assert np.abs(tr.free_energy(ds.tensors[0]).cpu().numpy() - R.free_energy(W, c, b, xs)).max() <= 1e-4
    assert np.abs(tr.hidden(ds.tensors[0]).cpu().numpy() - R.sigmoid(xs.astype(np.float64) @ W.T + c)).max() <= R.STEP_TOL


def test_ais_at_the_real_shapes_runs():
    """16 chains x 50 betas at 784-400: shapes, finiteness and the result's type; no accuracy claim."""
    cfg = dict(FULL, n_train=512, n_val=512)
    tr, m = product(cfg, mk_loaders(cfg), 1)
    res = tr.log_likelihood(chains=16, betas=50, seed=2)
    assert isinstance(res, metrics.AISResult) and (res.chains, res.n_betas, res.n) == (16, 50, cfg["n_test"])
    assert all(np.isfinite(v) for v in res)
    lw, b_A = tr.ais(chains=16, betas=50, seed=2)
    assert lw.shape == (16,) and lw.dtype == torch.float64 and b_A.shape == (784,) and bool(torch.isfinite(lw).all())
    imgs = tr.test_iter.dataset.tensors[0]
    assert torch.equal(tr.gibbs(imgs, 0).cpu(), imgs.reshape(-1, 784))         # {0, 1} rows pass the binarisation
    g = tr.gibbs(imgs, 2, seed=1)
    assert g.shape == (cfg["n_test"], 784) and set(torch.unique(g).tolist()) <= {0.0, 1.0}


# ---- learning --------------------------------------------------------------------------------------------------------------
def test_learning_on_bands():
    """The 16 band patterns tests/test_gpu_made.py learns on (16 x 16 images, two adjacent rows or columns lit).  CD-1
    lowers the one-step reconstruction cross-entropy; after training most chain samples lie on a band image (within 8 of
    256 pixels -- a uniformly random image is about 128 away from every band); the training images' free energy is
    below uniform noise's."""
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
    its = bands(128), bands(16), bands(16)
    torch.manual_seed(5)
    tr = rbm.RBMTrainer(rbm.RBM(256, 128), *its, seed=1)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(10, lr=1e-2)
    print("validation recon CE by epoch", tr.recon_loss)
    assert tr.recon_loss[-1] < tr.recon_loss[0] and tr.recon_loss[-1] < 0.25 * 256 * np.log(2.0)
    pats = its[0].dataset.tensors[0][:16].reshape(16, 256).to(DEV)
    s = tr.sample(256, seed=2, steps=500)
    dist = (s[:, None, :] - pats[None, :, :]).abs().sum(2).min(1).values
    frac = (dist <= 8).float().mean().item()
    print("samples within 8 pixels of a band image", frac, "median distance", dist.median().item())
    assert frac >= 0.5
    noise = torch.bernoulli(torch.full((256, 256), 0.5), generator=torch.Generator().manual_seed(3))
    f_data, f_noise = tr.free_energy(pats).mean().item(), tr.free_energy(noise).mean().item()
    print("free energy: bands", f_data, "noise", f_noise)
    assert f_data < f_noise
