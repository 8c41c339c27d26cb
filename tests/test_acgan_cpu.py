"""Auxiliary-classifier GAN without a GPU: module layout, fast-path selection, the C-ABI of the new kernels, label and
sampling-argument refusals, the training defaults."""
import ctypes
import inspect
import os
import sys

import pytest
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import ac_gan  # noqa: E402
from generative_models_amd import _lib, acgan as pkg, ops_fused  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402



def _loaders(n=40, batch=8, side=4, classes=3, labels=None):
    x = torch.bernoulli(torch.full((n, 1, side, side), 0.5))
    y = torch.arange(n) % classes if labels is None else labels
    ds = torch.utils.data.TensorDataset(x, y)
    dl = lambda: torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return dl(), dl(), dl()


def _trainer(model, cls=None, **kw):
    tr = object.__new__(cls or ac_gan.ACGANTrainer)     # selection runs before anything touches a GPU
    tr.model, tr.train_iter, tr.val_iter, tr.test_iter = model, *_loaders(**kw)
    tr._engine = None
    return tr


def test_module_surface_and_state_dict_keys():
    m = ac_gan.ACGAN(image_size=16, hidden_dim=12, z_dim=4, num_classes=3)
    assert list(m.state_dict()) == [
        "G.linear.weight", "G.linear.bias", "G.label.weight", "G.generate.weight", "G.generate.bias",
        "D.linear.weight", "D.linear.bias", "D.discriminate.weight", "D.discriminate.bias",
        "D.classify.weight", "D.classify.bias"]
    assert m.G.label.bias is None and m.G.label.weight.shape == (12, 3)
    assert m.D.classify.weight.shape == (3, 12) and m.D.discriminate.weight.shape == (1, 12)
    assert (m.image_size, m.hidden_dim, m.z_dim, m.num_classes, m.shape) == (16, 12, 4, 3, 4)
    d = ac_gan.ACGAN()
    assert (d.image_size, d.hidden_dim, d.z_dim, d.num_classes) == (784, 400, 20, 10)
    assert issubclass(ac_gan.ACGANTrainer, pkg.GANTrainer)
    for name in ("sample", "generate_images", "parzen", "accuracy", "save_checkpoint", "load_checkpoint"):
        assert callable(getattr(ac_gan.ACGANTrainer, name))
    assert "labels" in inspect.signature(ac_gan.ACGANTrainer.sample).parameters
    assert "labels" in inspect.signature(ac_gan.ACGANTrainer.generate_images).parameters
    with pytest.raises(GMError):                        # no CPU execution path
        m.G(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int64))


def test_fused_ok_limits_and_stock_selection():
    ok = lambda **kw: _trainer(ac_gan.ACGAN(**dict(dict(image_size=16, hidden_dim=8, z_dim=4, num_classes=3), **kw)))._stock()
    assert ok()
    assert ok(num_classes=1) and ok(num_classes=32) and not ok(num_classes=33) and not ok(num_classes=40)
    assert ok(hidden_dim=1024) and not ok(hidden_dim=1028) and not ok(hidden_dim=10)
    assert pkg.acgan_fused_ok(ac_gan.ACGAN(16, 8, 4, 3)) and not pkg.acgan_fused_ok(ac_gan.ACGAN(16, 6, 4, 3))
    m = ac_gan.ACGAN(16, 8, 4, 3)
    m.G = ac_gan.Generator(16, 12, 4, 3)               # unequal hidden widths
    assert not _trainer(m)._stock()

    class MineD(ac_gan.ACGANTrainer):
        def train_D(self, images, labels):
            return super().train_D(images, labels)
    assert not _trainer(ac_gan.ACGAN(16, 8, 4, 3), MineD)._stock()
    tr = _trainer(ac_gan.ACGAN(16, 8, 4, 3))
    tr.compute_noise = lambda b, z: None               # an instance attribute overrides a hook too
    assert not tr._stock()

    class MyG(ac_gan.Generator):
        pass
    m = ac_gan.ACGAN(16, 8, 4, 3)
    m.G = MyG(16, 8, 4, 3)
    assert not _trainer(m)._stock()
    m = ac_gan.ACGAN(16, 8, 4, 3)
    m.D.extra = nn.Linear(2, 2)
    assert not _trainer(m)._stock()
    m = ac_gan.ACGAN(16, 8, 4, 3)
    m.G.label = nn.Linear(3, 8)                         # a label layer with a bias is not the split form
    assert not _trainer(m)._stock()

    class MyModel(ac_gan.ACGAN):
        pass
    assert not _trainer(MyModel(16, 8, 4, 3))._stock()
    with pytest.raises(GMError):
        pkg.ACGANEngine(ac_gan.ACGAN(16, 8, 4, 3), None, None, 8, "cpu", world_size=2)
    with pytest.raises(GMError):
        pkg.ACGANEngine(ac_gan.ACGAN(16, 8, 4, 40), None, None, 8, "cpu")


def test_new_symbols_declared_bound_and_reject_bad_arguments():
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("libgm_hip.so not built")
    lib = _lib.load()
    E = _lib.GM_EINVAL
    ws = lib.gm_acgan_heads_workspace_bytes
    # header + 3 floats per row + one partial of (C + 1)(Hd + 1) floats per 8 rows
    assert ws(512, 400, 10) == 4 * (4 + 3 * 512 + 64 * (11 * 401 + 1))
    for rows, Hd, C in ((0, 8, 3), (8, 8, 0), (8, 8, 33), (8, 6, 3), (8, 1028, 3), (8, 0, 3)):
        assert ws(rows, Hd, C) == -1
    p = 16                                             # a non-null, aligned placeholder; never dereferenced here
    labels = _lib.LabelSrc(p, None, _lib.NO_SLOT)

    def args(**kw):
        a = ops_fused.ACGANHeadsArgs()
        a.H, a.ldh, a.rows, a.B, a.Hd, a.C, a.gen_mode = p, 8, 16, 8, 8, 3, 0
        a.w2, a.b2, a.Wc, a.bc, a.lab = p, p, p, p, labels
        a.da2, a.dq, a.lddq = p, p, 3
        a.dPre, a.ldp = 2 * p, 8
        a.gw2, a.gb2, a.gWc, a.gbc = p, p, p, p
        a.ws, a.ws_bytes = p, ws(16, 8, 3)
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)
    common = (dict(H=None), dict(w2=None), dict(b2=None), dict(Wc=None), dict(bc=None), dict(da2=None), dict(dq=None),
              dict(ws=None), dict(C=0), dict(C=33), dict(Hd=6, ldh=8), dict(Hd=1028, ldh=1028), dict(rows=0),
              dict(rows=-4), dict(rows=15), dict(B=0), dict(ldh=4), dict(ldh=10), dict(lddq=2), dict(H=p + 4),
              dict(ws_bytes=ws(16, 8, 3) - 4), dict(gen_mode=1))       # (the last: rows != B in generator mode)
    for fn in (lib.gm_acgan_heads_fwd, lib.gm_acgan_heads_bwd):
        assert fn(None, None) == E
        for bad in common:
            assert fn(None, args(**bad)) == E, (fn.__name__, bad)
    fwd_only = (dict(lab=_lib.LabelSrc(None, None, _lib.NO_SLOT)), dict(ce_out=p), dict(acc_out=p))
    for bad in fwd_only:
        assert lib.gm_acgan_heads_fwd(None, args(**bad)) == E, bad
    bwd_only = (dict(dPre=None), dict(ldp=4), dict(dPre=p), dict(gw2=None), dict(gbc=None),
                dict(gw2=None, gb2=None, gWc=None, gbc=None),          # neither gradients nor Adam
                dict(sched=p),                                          # Adam without its moments
                dict(gen_mode=1, rows=8),                               # gradients in generator mode
                dict(gen_mode=1, rows=8, gw2=None, gb2=None, gWc=None, gbc=None, sched=p))
    for bad in bwd_only:
        assert lib.gm_acgan_heads_bwd(None, args(**bad)) == E, bad


def test_wrappers_refuse_shapes_outside_the_limits():
    with pytest.raises(GMError):
        ops_fused.acgan_heads_workspace(8, 8, 33, "cpu")
    with pytest.raises(GMError):
        ops_fused.acgan_heads_workspace(8, 1028, 3, "cpu")
    with pytest.raises(GMError):
        ops_fused.acgan_heads_workspace(0, 8, 3, "cpu")
    z = torch.zeros
    with pytest.raises(GMError):                        # Hd % 4 != 0
        ops_fused.acgan_heads_bwd(z(16, 6), z(1, 6), z(1), z(3, 6), z(3), 8, False, z(16), z(16, 3), z(16, 6), z(64))


def test_labels_outside_the_classes_raise_before_any_launch():
    for bad in (torch.arange(40) % 4, torch.arange(40) % 3 - 1):
        tr = _trainer(ac_gan.ACGAN(16, 8, 4, 3), labels=bad)
        tr.class_losses, tr.Glosses, tr.Dlosses, tr.viz, tr.num_epochs, tr.use_graph = [], [], [], False, 0, True
        assert tr._stock()
        with pytest.raises(GMError, match="class labels"):
            tr.train(1)
        assert tr._engine is None
    tr = _trainer(ac_gan.ACGAN(16, 8, 4, 3), labels=(torch.arange(40) % 3).float() + 0.5)
    with pytest.raises(GMError, match="integers"):
        tr._device_labels(tr.train_iter)


def test_sample_argument_checking():
    tr = _trainer(ac_gan.ACGAN(16, 8, 4, 3))
    st = torch.get_rng_state()
    for bad in (3, -1, [0, 1], [0, 1, 2, 3], True, [0.5, 1, 2], "ab"):
        with pytest.raises(ac_gan.LabelError):
            tr.sample(3, seed=0, labels=bad)
    assert torch.equal(st, torch.get_rng_state())       # refused before anything is drawn
    assert issubclass(ac_gan.LabelError, ValueError) and issubclass(ac_gan.LabelError, GMError)
    from generative_models_amd.cvae import _labels_arg
    assert _labels_arg(None, 5, 3).tolist() == [0, 1, 2, 0, 1] and _labels_arg(2, 3, 3).tolist() == [2, 2, 2]


def test_defaults_world_size_and_checkpoint_fields(monkeypatch):
    sig = inspect.signature(ac_gan.ACGANTrainer.train).parameters
    assert list(sig)[1:] == ["num_epochs", "G_lr", "D_lr", "D_steps", "class_weight"]
    assert (sig["G_lr"].default, sig["D_lr"].default, sig["D_steps"].default, sig["class_weight"].default) == \
        (2e-4, 2e-4, 1, 1.0)
    assert pkg.HISTORY == ("Glosses", "Dlosses", "class_losses", "num_epochs")
    assert pkg.ACGANEngine.launches_per_iteration(1) == 20
    tr = _trainer(ac_gan.ACGAN(16, 8, 4, 3))
    with pytest.raises(GMError):                        # nothing to save before a fused train() call
        tr.save_checkpoint("unused.pt")
    from generative_models_amd import dp
    monkeypatch.setattr(dp, "current", lambda: (2, 0, None))
    with pytest.raises(GMError, match="one GPU"):
        tr.train(1)
