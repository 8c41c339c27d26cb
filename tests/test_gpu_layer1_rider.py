"""The generator's first layer riding in the previous iteration's weight-gradient pair (ops.linear_bwd_dw_adam_pair_l1)
and the batch gather riding in the dH launch (ops.linear_bwd_dx_gather): bit for bit what the separate launches
compute, at the op level and over whole training runs."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from generative_models_amd import ops  # noqa: E402
from generative_models_amd.engine import GANEngine  # noqa: E402

DEV = "cuda"


def _lin(n, k, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return SimpleNamespace(W=r(n, k) * 0.1, b=r(n) * 0.1, gW=torch.zeros(n, k, device=DEV),
                           gb=torch.zeros(n, device=DEV), mW=r(n, k).abs() * 0.01, vW=r(n, k).abs() * 0.001,
                           mb=r(n).abs() * 0.01, vb=r(n).abs() * 0.001)


def _clone(lin):
    return SimpleNamespace(**{k: v.clone() for k, v in vars(lin).items()})


def _case(B, hid, Z, rows, I=784, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    G2, G1 = _lin(I, hid, seed + 1), _lin(hid, Z, seed + 2)
    dXg, Hg2, dHg = r(B, I), torch.relu(r(B, hid)), r(B, hid)
    R = 3                                            # noise ring of 3 slots (slot 1 is the next one)
    zring = r(R * max(B, rows) * Z)
    sched = torch.tensor([1e-3, 0.9, 2e-3, 0.8], device=DEV)
    return G2, G1, dXg, Hg2, dHg, zring, sched, R


@pytest.mark.parametrize("hid", [400, 390, 33])
@pytest.mark.parametrize("Z", [4, 20, 32])
@pytest.mark.parametrize("B,rows", [(64, 128), (100, 100), (256, 512), (1024, 256)])
def test_pair_l1_equals_pair_then_forward(hid, Z, B, rows):
    """ops.linear_bwd_dw_adam_pair_l1 == ops.linear_bwd_dw_adam_pair, then gm_linear_fwd (the k32 kernel) on the next
    slot of the noise ring with the stepped W1, b1: H, both layers' parameters, gradients and Adam moments."""
    G2, G1, dXg, Hg2, dHg, zring, sched, R = _case(B, hid, Z, rows, seed=B + hid + Z)
    ctr = torch.tensor([1], dtype=torch.int64, device=DEV)
    zbase = zring.view(-1, Z)
    S = max(B, rows) * Z                                             # elements per ring slot
    x_slot = ops.slot(ctr.data_ptr(), 1, -1, R, S)                   # this iteration's rows (slot 0)
    z_slot = ops.slot(ctr.data_ptr(), 1, 0, R, S)                    # the next iteration's (slot 1)
    adam = dict(sched=sched, sched_slot=ops.slot(ctr.data_ptr(), 1, 0, 2, 1))
    out = {}
    for form in ("ref", "ride"):
        g2, g1 = _clone(G2), _clone(G1)
        first = dict(dA=dXg, X=Hg2, lin=g2, adam=adam, M=B)
        second = dict(dA=dHg, X=zbase, lin=g1, adam=adam, M=B, x_slot=x_slot)
        H = torch.full((rows, hid), -7.0, device=DEV)
        if form == "ref":
            ops.linear_bwd_dw_adam_pair(first, second)
            ops.linear_fwd(zbase, g1.W, g1.b, H, "relu", M=rows, x_slot=z_slot)
        else:
            ops.linear_bwd_dw_adam_pair_l1(first, second, zbase, H, rows, z_slot=z_slot)
        torch.cuda.synchronize()
        out[form] = (H, g2, g1)
    (Hr, r2, r1), (Hg, q2, q1) = out["ref"], out["ride"]
    assert torch.equal(Hr, Hg), (hid, Z, B, rows)
    assert bool((Hr != -7.0).all())
    for a, b in ((r2, q2), (r1, q1)):
        for k in vars(a):
            assert torch.equal(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize("B,Hd,I", [(256, 400, 784), (100, 390, 784), (64, 33, 36)])
@pytest.mark.parametrize("packed", [True, False])
def test_dx_with_gather_riding(B, Hd, I, packed):
    """ops.linear_bwd_dx_gather == gm_gather_rows(_bits) + gm_linear_bwd_dx, bit for bit."""
    g = torch.Generator().manual_seed(B + Hd)
    dA = torch.randn(B, I, generator=g).to(DEV)
    W = torch.randn(I, Hd, generator=g).to(DEV)
    below = torch.relu(torch.randn(B, Hd, generator=g)).to(DEV)
    n = 500
    imgs = (torch.rand(n, I, generator=g) > 0.5).float()
    data = ops.PackedData(imgs) if packed else imgs.to(DEV)
    idx = torch.randint(0, n, (2 * B,), generator=g).to(DEV)
    slot = ops.slot(0, 0, 1, 0, B)                   # the second row of the index ring
    out_ref, out = torch.zeros(B, I, device=DEV), torch.full((B, I), -1.0, device=DEV)
    dX_ref, dX = torch.empty(B, Hd, device=DEV), torch.empty(B, Hd, device=DEV)
    ops.gather_rows(data, idx, out_ref, idx_slot=slot)
    ops.linear_bwd_dx(dA, W, dX_ref, below=below, epi="relu")
    ops.linear_bwd_dx_gather(dA, W, dX, data, idx, out, below=below, epi="relu", idx_slot=slot)
    torch.cuda.synchronize()
    assert torch.equal(dX, dX_ref) and torch.equal(out, out_ref)
    assert torch.equal(out.cpu(), imgs[idx[B:].cpu()])


def _run(variant, rides, monkeypatch, use_graph=True, env=None):
    from test_gpu_trainers import SMALL, run_product
    if not rides:
        monkeypatch.setattr(GANEngine, "_l1_rides", lambda self: False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    seen = []
    orig = GANEngine._issue_iteration

    def spy(self, st, it, pos=0, count=1):
        seen.append(self._l1_rides())
        return orig(self, st, it, pos, count)
    monkeypatch.setattr(GANEngine, "_issue_iteration", spy)
    tr, model, rng = run_product(variant, SMALL, SMALL["batch"], dict(num_epochs=1), use_graph=use_graph,
                                 capped=2 * 128 + 3)
    monkeypatch.undo()
    return tr, model, rng, any(seen)


@pytest.mark.parametrize("variant", ["ns", "ls"])
@pytest.mark.parametrize("mode", ["g1", "g2", "g128", "eager", "ring5"])
def test_engine_rider_changes_nothing(variant, mode, monkeypatch):
    """Rider on against rider off over 2 x 128 + 3 iterations: graphs of 1, 2 and 128 iterations, eager launches, a ring
    of 5 slots that wraps -- losses, parameters and the RNG position bitwise equal."""
    env = {"g1": {"GM_GRAPH_ITERS": "1"}, "g2": {"GM_GRAPH_ITERS": "2"}, "g128": {"GM_GRAPH_ITERS": "128"},
           "eager": {}, "ring5": {"GM_RING": "5"}}[mode]
    use_graph = mode != "eager"
    ref, ref_model, ref_rng, ref_rode = _run(variant, False, monkeypatch, use_graph, env)
    got, got_model, got_rng, rode = _run(variant, True, monkeypatch, use_graph, env)
    assert rode and not ref_rode
    assert len(got.Glosses) == len(ref.Glosses) and got.Glosses == ref.Glosses and got.Dlosses == ref.Dlosses
    assert torch.equal(ref_rng, got_rng)
    for (k, a), (_, b) in zip(got_model.state_dict().items(), ref_model.state_dict().items()):
        assert torch.equal(a, b), k
