"""Primal-Dual Wasserstein GAN without a GPU: the fp64 oracle's hand-written second backward against autograd, the
module layout and training surface, the draw order of the host replay, fast-path selection and the refusals."""
import inspect
import os
import sys

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import pdw_gan  # noqa: E402
from generative_models_amd import _lib  # noqa: E402
from generative_models_amd import pdwgan as pkg  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402



def _loaders(n=40, batch=8, side=4):
    x = torch.bernoulli(torch.full((n, 1, side, side), 0.5))
    ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None):
    tr = object.__new__(cls or pdw_gan.PDWGANTrainer)   # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders()
    return tr


def test_oracle_second_backward_formulas_vs_autograd():
    """The penalty's hand-derived second backward (the launch list's formulas) against fp64 autograd through
    autograd.grad(create_graph=True) at 64-48-8, b = 6: gamma = (2 lambda / b)(g - d), dW1 += u^T gamma,
    t = gamma W1^T, gw2 += sum_b m2 m1 . t, and no share for b1 / b2.  The seed is chosen so that every hidden
    pre-activation and critic output is at least 1e-3 away from its ReLU kink (asserted)."""
    I, H, b, lam = 64, 48, 6, 10.0
    g = torch.Generator().manual_seed(4)
    W1 = (torch.rand(H, I, generator=g, dtype=torch.float64) * 2 - 1) / I ** 0.5
    b1 = (torch.rand(H, generator=g, dtype=torch.float64) * 2 - 1) / I ** 0.5
    w2 = (torch.rand(1, H, generator=g, dtype=torch.float64) * 2 - 1) / H ** 0.5
    b2 = torch.full((1,), 0.3, dtype=torch.float64)
    x = torch.bernoulli(torch.full((b, I), 0.3, dtype=torch.float64), generator=g)
    xr = torch.sigmoid(torch.randn(b, I, generator=g, dtype=torch.float64))
    xr[1] = x[1]                                              # a row with d = 0
    t = torch.rand(b, 1, generator=g, dtype=torch.float64)
    diff = x - xr
    n = diff.norm(dim=1, keepdim=True)
    d = torch.where(n > 0, diff / n.clamp_min(1e-300), torch.zeros_like(diff))
    P = [p.clone().requires_grad_() for p in (W1, b1, w2, b2)]
    xh = (t * x + (1 - t) * xr).requires_grad_()
    a1 = xh @ P[0].T + P[1]
    a2 = torch.relu(a1) @ P[2].T + P[3]
    assert a1.abs().min().item() >= 1e-3 and a2.abs().min().item() >= 1e-3
    assert bool((a2 > 0).any()) and bool((a1 > 0).any()) and bool((a1 < 0).any())
    gr = torch.autograd.grad(torch.relu(a2).sum(), xh, create_graph=True)[0]
    pen = lam * ((gr - d) ** 2).sum(1).mean()
    ref = torch.autograd.grad(pen, P, allow_unused=True)
    # by hand
    m1, m2 = (a1 > 0).double(), (a2 > 0).double()
    u = m2 * m1 * w2                                         # [b, H]: gm_head_gp's seed
    gh = u @ W1                                              # g = u W1
    assert torch.allclose(gh, gr.detach(), rtol=0, atol=1e-14)
    gamma = (2 * lam / b) * (gh - d)
    dW1 = u.T @ gamma
    tt = gamma @ W1.T
    gw2 = (m2 * m1 * tt).sum(0, keepdim=True)
    for got, r, nm in ((dW1, ref[0], "dW1"), (gw2, ref[2], "gw2")):
        assert (got - r).abs().max().item() <= 1e-12 * max(1.0, r.abs().max().item()), nm
    assert ref[1] is None or ref[1].abs().max().item() == 0          # no bias shares
    assert ref[3] is None or ref[3].abs().max().item() == 0
    assert torch.equal(gamma[1], (2 * lam / b) * gh[1])               # the d = 0 row


def test_module_names_build_order_and_state_dict_keys():
    m = pdw_gan.PDWGAN(image_size=16, hidden_dim=12, z_dim=4)
    assert list(m.state_dict()) == [
        "E.linear.weight", "E.linear.bias", "E.z.weight", "E.z.bias",
        "G.linear.weight", "G.linear.bias", "G.generate.weight", "G.generate.bias",
        "D.linear.weight", "D.linear.bias", "D.discriminate.weight", "D.discriminate.bias"]
    assert [n for n, _ in m.named_children()] == ["E", "G", "D"]
    assert type(m.E).__name__ == "Encoder" and type(m.G).__name__ == "Generator" and type(m.D).__name__ == "CriticReLU"
    assert m.D._out_act == "relu"
    assert m.E.z.weight.shape == (4, 12) and m.G.generate.weight.shape == (16, 12)
    assert m.D.discriminate.weight.shape == (1, 12)
    assert (m.image_size, m.hidden_dim, m.z_dim, m.shape) == (16, 12, 4, 4)
    d = pdw_gan.PDWGAN()
    assert (d.image_size, d.hidden_dim, d.z_dim) == (784, 400, 20)
    # the build order is the initialisation's draw order: E, then G, then D
    torch.manual_seed(3)
    a = pdw_gan.PDWGAN(16, 12, 4)
    torch.manual_seed(3)
    e = pkg.Encoder(16, 12, 4)
    assert torch.equal(a.E.linear.weight, e.linear.weight) and torch.equal(a.E.z.bias, e.z.bias)


def test_surface_and_defaults():
    T = pdw_gan.PDWGANTrainer
    for name in ("train", "evaluate", "sample", "reconstruct", "parzen", "generate_images", "viz_loss",
                 "save_checkpoint", "load_checkpoint", "compute_batch", "train_D", "train_G"):
        assert callable(getattr(T, name)), name
    sig = inspect.signature(T.train).parameters
    assert list(sig)[1:7] == ["num_epochs", "E_lr", "G_lr", "D_lr", "lambda_z", "lambda_gp"]
    assert sig["E_lr"].default == sig["G_lr"].default == sig["D_lr"].default == 1e-4
    assert sig["lambda_gp"].default == 10.0 and sig["lambda_z"].default == pkg.LAMBDA_Z == 10.0
    assert "D_steps" not in sig
    assert list(inspect.signature(T.__init__).parameters)[1:] == ["model", "train_iter", "val_iter", "test_iter", "viz"]
    assert T._hook_names == ("compute_batch", "train_D", "train_G", "evaluate")
    assert pkg.HISTORY == ("Elosses", "Dlosses", "Glosses", "num_epochs", "best_val_loss")
    assert {"m", "v", "step", "steps"} <= set(pkg.OPTIM_FIELDS)
    import generative_models_amd
    assert generative_models_amd.PDWGANTrainer is T and generative_models_amd.PDWGAN is pdw_gan.PDWGAN
    tr = object.__new__(T)
    tr._engine = None
    with pytest.raises(GMError):                       # nothing to save before a fused train() call
        tr.save_checkpoint("unused.pt")


@pytest.mark.parametrize("B,Z,sizes", [(32, 8, [32, 32, 32, 8]), (512, 20, [512, 512, 336]), (8, 4, [8, 8, 3])])
def test_draw_order_leaves_the_generator_where_the_contract_does(B, Z, sizes):
    """The engine's host draws (one epoch's permutation, then per batch p, t, z_c, z_g) against the same draws made
    through torch call by call: values and the CPU generator's end state."""
    train_iter = _loaders(n=sum(sizes), batch=B)[0]
    from generative_models_amd.trainers import _epoch_order
    dst = dict(prior=torch.zeros(len(sizes), B, Z), t=torch.zeros(len(sizes), B), zc=torch.zeros(len(sizes), B, Z),
               zg=torch.zeros(len(sizes), B, Z))
    torch.manual_seed(11)
    perm = _epoch_order(train_iter)
    pkg.host_draws(dst, sizes, B, Z)
    end = torch.get_rng_state()
    torch.manual_seed(11)
    it = iter(train_iter)                                # the loader's own draws: base seed, sampler seed
    first = next(it)[0]
    assert torch.equal(first, train_iter.dataset.tensors[0][perm[:B]])
    for k, b in enumerate(sizes):
        p, t, zc, zg = torch.randn(b, Z), torch.rand(b, 1), torch.randn(b, Z), torch.randn(b, Z)
        assert torch.equal(dst["prior"][k].view(-1)[:b * Z], p.view(-1)), k
        assert torch.equal(dst["t"][k][:b], t.view(-1)), k
        assert torch.equal(dst["zc"][k].view(-1)[:b * Z], zc.view(-1)), k
        assert torch.equal(dst["zg"][k].view(-1)[:b * Z], zg.view(-1)), k
    assert torch.equal(end, torch.get_rng_state())


def test_stock_selection():
    assert _trainer(pdw_gan.PDWGAN(16, 8, 4))._stock()

    class MineD(pdw_gan.PDWGANTrainer):
        def train_D(self, images):
            return super().train_D(images)

    class MineEval(pdw_gan.PDWGANTrainer):
        def evaluate(self, iterator):
            return super().evaluate(iterator)
    assert not _trainer(pdw_gan.PDWGAN(16, 8, 4), MineD)._stock()
    assert not _trainer(pdw_gan.PDWGAN(16, 8, 4), MineEval)._stock()
    for hook in ("compute_batch", "train_G"):
        tr = _trainer(pdw_gan.PDWGAN(16, 8, 4))
        setattr(tr, hook, lambda *a: None)             # an instance attribute overrides a hook too
        assert not tr._stock()

    class MyG(pdw_gan.Generator):
        pass
    m = pdw_gan.PDWGAN(16, 8, 4)
    m.G = MyG(16, 8, 4)                                # a subclassed module
    assert not _trainer(m)._stock()
    m = pdw_gan.PDWGAN(16, 8, 4)
    m.E.extra = nn.Linear(2, 2)                        # an edited network
    assert not _trainer(m)._stock()

    class MyModel(pdw_gan.PDWGAN):
        pass
    assert not _trainer(MyModel(16, 8, 4))._stock()
    # outside the fused limits: Z > 32, Z % 4 != 0, H > 512, unequal hidden widths
    assert not _trainer(pdw_gan.PDWGAN(16, 8, 40))._stock()
    assert not _trainer(pdw_gan.PDWGAN(16, 8, 6))._stock()
    assert not _trainer(pdw_gan.PDWGAN(16, 520, 4))._stock()
    m = pdw_gan.PDWGAN(16, 8, 4)
    m.D = pdw_gan.Discriminator(16, 12, 1)
    assert not _trainer(m)._stock()
    assert _trainer(pdw_gan.PDWGAN(16, 512, 32))._stock()
    assert pkg.pdw_fused_ok(pdw_gan.PDWGAN()) and not pkg.pdw_fused_ok(pdw_gan.PDWGAN(16, 8, 6))


def test_world_size_above_one_is_refused():
    with pytest.raises(GMError):
        pkg.PDWGANEngine(pdw_gan.PDWGAN(16, 8, 4), "cpu", world_size=2)
    with pytest.raises(GMError):
        pkg.PDWGANEngine(pdw_gan.PDWGAN(16, 8, 4), "cpu", force_dp=True)
    with pytest.raises(GMError):                       # and a shape the fused batch does not take
        pkg.PDWGANEngine(pdw_gan.PDWGAN(16, 8, 6), "cpu")


def test_train_refuses_data_parallel_runs(monkeypatch):
    """PDWGANTrainer.train's own refusal (the one a user under torchrun reaches), before any path is chosen."""
    from generative_models_amd import dp
    monkeypatch.setattr(dp, "current", lambda: (2, 0, None))
    tr = _trainer(pdw_gan.PDWGAN(16, 8, 4))
    with pytest.raises(GMError, match="one GPU"):
        tr.train(1)


def test_new_symbols_declared_bound_and_reject_bad_arguments():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("libgm_hip.so not built")
    lib = _lib.load()
    E, p, S = _lib.GM_EINVAL, 16, _lib.NO_SLOT         # p: a non-null placeholder, never dereferenced on these paths

    def couple(**kw):
        a = dict(x=p, ldx=8, xr=p, ldr=8, t=p, n=p, share=p, dA=p, ldd=8, xhat=p, ldh=8, xcopy=p, ldc=8, B=4, I=8)
        a.update(kw)
        return lib.gm_pdw_couple(None, a["x"], a["ldx"], a["xr"], a["ldr"], a["t"], S, a["n"], a["share"], a["dA"],
                                 a["ldd"], a["xhat"], a["ldh"], a["xcopy"], a["ldc"], 0.25, a["B"], a["I"])
    for bad in (dict(x=None), dict(xr=None), dict(share=None), dict(B=0), dict(I=0), dict(ldx=7), dict(ldr=7),
                dict(ldd=7), dict(ldh=7), dict(ldc=7), dict(t=None)):
        assert couple(**bad) == E, bad                 # (the last: an interpolate without its t)

    def direction(**kw):
        a = dict(g=p, ldg=8, x=p, ldx=8, xr=p, ldr=8, n=p, gamma=p, ldm=8, pen=p, B=4, I=8)
        a.update(kw)
        return lib.gm_pdw_dir(None, a["g"], a["ldg"], a["x"], a["ldx"], a["xr"], a["ldr"], a["n"], a["gamma"],
                              a["ldm"], a["pen"], 10.0, 0.25, a["B"], a["I"])
    for bad in (dict(g=None), dict(x=None), dict(xr=None), dict(n=None), dict(gamma=None), dict(pen=None), dict(B=0),
                dict(I=0), dict(ldg=7), dict(ldx=7), dict(ldr=7), dict(ldm=7)):
        assert direction(**bad) == E, bad
