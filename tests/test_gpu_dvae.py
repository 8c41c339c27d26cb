"""Denoising VAE on the MI355X: the device corruption against the numpy rule, the corrupting gathers against the plain
gather + corrupt(), the fused engine against a plain-torch CPU loop that replays VAETrainer's RNG protocol and corrupts
with the numpy rule, gradients against fp64, level 0 against the VAE, determinism and resume, the general path and
denoising itself."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "generative_models_amd", "src"))

import dvae  # noqa: E402
import vae  # noqa: E402
from generative_models_amd import ops, ops_fused, trainers  # noqa: E402
from generative_models_amd import dvae as gdvae  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402

DEV = "cuda"
LEVELS = {"salt_pepper": (0.0, 0.1, 0.5, 1.0), "gaussian": (0.0, 0.05, 1.0, 3.0)}


def close_rule(got, x, noise, level, seed, step, row0=0):
    """got (device rows) against corrupt_reference: salt-and-pepper bit for bit, gaussian within 4e-6 of the normal's
    scale (the bgan normals' tolerance)."""
    got = got.cpu().numpy()
    ref = gdvae.corrupt_reference(x, noise, level, seed, step, row0)
    if noise == "salt_pepper" or level == 0.0:
        assert got.tobytes() == ref.tobytes(), (noise, level, seed, step, row0)
        return
    n, I = x.shape
    nrm = gdvae.box_muller_normals(gdvae.corruption_words(n, 4 * ((I + 3) // 4), seed, step, row0))[:, :I]
    tol = 4e-6 * (np.maximum(1.0, np.abs(ref)) + np.float32(level) * np.maximum(1.0, np.abs(nrm)))
    err = np.abs(got.astype(np.float64) - ref)
    assert np.all(err <= tol), (noise, level, seed, step, float(err.max()))


@pytest.mark.parametrize("noise", ["salt_pepper", "gaussian"])
def test_corrupt_vs_numpy_rule(noise):
    g = torch.Generator().manual_seed(1)
    for n, I in [(1, 1), (3, 7), (5, 4), (17, 784), (64, 130)]:
        x = torch.rand(n, I, generator=g)
        x[:, ::3] = (x[:, ::3] > 0.5).float()
        for level in LEVELS[noise]:
            for seed, step, row0 in [(0, 0, 0), (1, 77, 0), ((1 << 64) - 1, 5, 3), (0x123456789ABCDEF, 1 << 20, 511)]:
                got = dvae.corrupt(x, noise, level, seed, step=step, row0=row0)
                close_rule(got, x.numpy(), noise, level, seed, step, row0)
    # the step is taken mod 2^32
    x = torch.rand(4, 33, generator=g)
    assert torch.equal(dvae.corrupt(x, noise, 0.5, 9, step=(1 << 32) + 3), dvae.corrupt(x, noise, 0.5, 9, step=3))
    # strided rows in and out, and in place
    big = torch.rand(9, 50, generator=g).to(DEV)
    xs = big[:, 3:44]
    out = torch.full((9, 60), -7.0, device=DEV)
    a = ops_fused.corrupt_args(noise, 0.5, 4, step=6, row0=2)
    ops_fused.dvae_corrupt(xs, a, out=out[:, :41])
    close_rule(out[:, :41], xs.cpu().numpy(), noise, 0.5, 4, 6, 2)
    assert torch.all(out[:, 41:] == -7.0)                      # nothing written past the row
    want = ops_fused.dvae_corrupt(xs.contiguous(), a)
    ip = xs.clone()
    ops_fused.dvae_corrupt(ip, a, out=ip)
    assert torch.equal(ip, want)
    # a device counter plus a device base equals the same step given as a value
    ctr = torch.tensor([40], dtype=torch.int64, device=DEV)
    base = torch.tensor([1000], dtype=torch.int64, device=DEV)
    x = torch.rand(8, 100, generator=g).to(DEV)
    via = ops_fused.dvae_corrupt(x, ops_fused.corrupt_args(noise, 0.3, 11, step=2, step_ctr=ctr, step_base=base))
    assert torch.equal(via, dvae.corrupt(x, noise, 0.3, 11, step=1042))
    assert not torch.equal(via, dvae.corrupt(x, noise, 0.3, 11, step=1041))


def test_corruption_statistics_over_4m_pixels():
    n, I = 4096, 1024                                          # 2^22 pixels
    x = torch.full((n, I), 0.5, device=DEV)
    y = dvae.corrupt(x, "salt_pepper", 0.5, 123, step=9)
    N = n * I
    replaced = (y != 0.5).double().sum().item()
    assert abs(replaced - 0.5 * N) <= 5 * (N * 0.25) ** 0.5, replaced
    ones = (y == 1.0).double().sum().item()
    assert abs(ones - 0.5 * replaced) <= 5 * (replaced * 0.25) ** 0.5, (ones, replaced)   # a fair coin
    z = torch.zeros(n, I, device=DEV)
    e = dvae.corrupt(z, "gaussian", 2.0, 123, step=9).double() / 2.0
    m, v = e.mean().item(), e.var().item()
    sk, ku = ((e - m) ** 3).mean().item() / v ** 1.5, ((e - m) ** 4).mean().item() / v ** 2
    assert abs(m) <= 5 / N ** 0.5 and abs(v - 1) <= 5 * (2 / N) ** 0.5, (m, v)
    assert abs(sk) <= 5 * (6 / N) ** 0.5 and abs(ku - 3) <= 5 * (24 / N) ** 0.5, (sk, ku)
    # neighbouring words are uncorrelated (pixels 4q + j, rows, steps)
    assert abs((e[:, :-1] * e[:, 1:]).mean().item()) <= 5 / N ** 0.5
    e2 = dvae.corrupt(z, "gaussian", 2.0, 123, step=10).double() / 2.0
    assert abs((e * e2).mean().item()) <= 5 / N ** 0.5


def _data(packed, n=300, I=784, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.bernoulli(torch.full((n, I), 0.3), generator=g) if packed else torch.rand(n, I, generator=g)
    return x, (ops.PackedData(x.to(DEV)) if packed else x.to(DEV))


@pytest.mark.parametrize("packed", [True, False], ids=["bits", "fp32"])
@pytest.mark.parametrize("noise", ["salt_pepper", "gaussian"])
def test_corrupting_gathers(packed, noise):
    for I in (784, 130):
        x, data = _data(packed, I=I)
        g = torch.Generator().manual_seed(I)
        B = 512
        idx = torch.randint(0, x.shape[0], (3, B), generator=g).to(DEV)
        ctr = torch.tensor([5], dtype=torch.int64, device=DEV)
        base = torch.tensor([100], dtype=torch.int64, device=DEV)
        for b in (B, 336, 17):
            # standalone: the batch's own rows at step ctr + base (idx slot: row ctr % 3 of the ring)
            slot = ops.slot(ctr.data_ptr(), 1, 0, 3, B)
            X, Xc, ref = (torch.full((B, I), -1.0, device=DEV) for _ in range(3))
            ops_fused.gather_rows_corrupt(data, idx.view(-1), X, Xc,
                                          ops_fused.corrupt_args(noise, 0.25, 77, step_ctr=ctr, step_base=base), B=b,
                                          idx_slot=slot)
            ops.gather_rows(data, idx.view(-1), ref, B=b, idx_slot=slot)
            assert torch.equal(X, ref)
            assert torch.equal(Xc[:b], dvae.corrupt(ref[:b], noise, 0.25, 77, step=105))
            assert torch.all(Xc[b:] == -1.0)
            # riding in a forward: the NEXT batch's rows (slot ctr + 1) at the next step
            for M, K, N in [(b, 400, 40), (b, 20, 400), (2048, 784, 400)]:
                h = torch.randn(M, K, generator=g).to(DEV)
                W, bias = torch.randn(N, K, generator=g).to(DEV), torch.randn(N, generator=g).to(DEV)
                y, y_ref = torch.empty(M, N, device=DEV), torch.empty(M, N, device=DEV)
                X.fill_(-1.0); Xc.fill_(-1.0); ref.fill_(-1.0)
                nslot = ops.slot(ctr.data_ptr(), 1, 1, 3, B)
                ops_fused.linear_fwd_gather_corrupt(
                    h, W, bias, y, "relu", data, idx.view(-1), X, Xc,
                    ops_fused.corrupt_args(noise, 0.25, 77, step=1, step_ctr=ctr, step_base=base), M=M, B=b,
                    idx_slot=nslot)
                ops.linear_fwd(h, W, bias, y_ref, "relu", M=M)
                ops.gather_rows(data, idx.view(-1), ref, B=b, idx_slot=nslot)
                assert torch.equal(y, y_ref), (M, K, N)
                assert torch.equal(X, ref), (M, K, N)
                assert torch.equal(Xc[:b], dvae.corrupt(ref[:b], noise, 0.25, 77, step=106)), (M, K, N)
                assert torch.all(Xc[b:] == -1.0)


# ---- the engine against an oracle ------------------------------------------------------------------------------------
def loaders(batch, n_train, n_val, n_test, side, seed=7, binary=True):
    """Image loaders; the data come from a private generator, the loaders shuffle on the global one."""
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        if binary:
            x = torch.bernoulli(torch.full((n, 1, side, side), 0.3), generator=g)
        else:
            x = torch.rand(n, 1, side, side, generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(n_val), mk(n_test)


class Oracle(nn.Module):
    """vae.VAE in plain torch on the CPU, in fp64 (eps drawn in fp32 as the protocol draws it); the encoder reads
    whatever rows it is given.  (An fp32 CPU oracle is the less accurate party at 784-400-20 with gaussian noise: one
    first-step Adam update of encoder.linear.weight lands 2e-3 off the fp64 one while the engine stays within 6e-8.)"""

    def __init__(self, m):
        super().__init__()
        cp = lambda lin: nn.Linear(lin.in_features, lin.out_features).requires_grad_(False)
        self.e1, self.mu, self.lv = cp(m.encoder.linear), cp(m.encoder.mu), cp(m.encoder.log_var)
        self.d1, self.rc = cp(m.decoder.linear), cp(m.decoder.recon)
        for o, s in ((self.e1, m.encoder.linear), (self.mu, m.encoder.mu), (self.lv, m.encoder.log_var),
                     (self.d1, m.decoder.linear), (self.rc, m.decoder.recon)):
            o.weight = nn.Parameter(s.weight.detach().cpu().clone())
            o.bias = nn.Parameter(s.bias.detach().cpu().clone())
        self.double()

    def forward(self, x_enc):
        h = F.relu(self.e1(x_enc.double()))
        mu, lv = self.mu(h), self.lv(h)
        z = mu + torch.randn(mu.shape) * torch.exp(lv / 2)
        return torch.sigmoid(self.rc(F.relu(self.d1(z)))), mu, lv

    def state(self):
        return {"encoder.linear.weight": self.e1.weight, "encoder.linear.bias": self.e1.bias,
                "encoder.mu.weight": self.mu.weight, "encoder.mu.bias": self.mu.bias,
                "encoder.log_var.weight": self.lv.weight, "encoder.log_var.bias": self.lv.bias,
                "decoder.linear.weight": self.d1.weight, "decoder.linear.bias": self.d1.bias,
                "decoder.recon.weight": self.rc.weight, "decoder.recon.bias": self.rc.bias}


def kl_sum(mu, lv):
    return torch.sum(0.5 * (mu ** 2 + torch.exp(lv) - lv - 1))


def oracle_train(o, its, epochs, noise, level, seed, lr=1e-3, wd=1e-5):
    """VAETrainer's protocol on the oracle (next(iter(test)) first, then per epoch a training and a validation pass),
    the encoder fed the numpy rule's corruption of each training batch; validation on clean images.

    Gaussian noise: the rule's fp64 normals and the device's fp32 ones differ in the last bits, and Adam's first step
    (m / sqrt(v) = sign(g)) turns a last-bit change of a near-zero gradient into a whole lr step of that weight.  So the
    oracle takes the device's rows for gaussian noise after checking every one of them against the numpy rule
    (close_rule: 4e-6 of the normal's scale); salt-and-pepper rows are the rule's own (bit-identical anyway)."""
    next(iter(its[2]))
    opt = torch.optim.Adam(o.parameters(), lr=lr, weight_decay=wd)
    recon, kl, best, step = [], [], 1e10, 0
    for _ in range(epochs):
        for x, _ in its[0]:
            x = x.view(x.shape[0], -1)
            x64 = x.double()
            if noise == "gaussian":
                dev = dvae.corrupt(x, noise, level, seed, step=step)
                close_rule(dev, x.numpy(), noise, level, seed, step)
                xt = dev.cpu()
            else:
                xt = torch.from_numpy(gdvae.corrupt_reference(x.numpy(), noise, level, seed, step))
            step += 1
            opt.zero_grad()
            out, mu, lv = o(xt)
            r, k = torch.sum((x64 - out) ** 2), kl_sum(mu, lv)
            (r + k).backward()
            opt.step()
            recon.append(r.item()); kl.append(k.item())
        vals = []
        with torch.no_grad():
            for x, _ in its[1]:
                x = x.view(x.shape[0], -1)
                out, mu, lv = o(x)
                vals.append((torch.sum((x.double() - out) ** 2) + kl_sum(mu, lv)).item())
        best = min(best, float(np.mean(vals)))
    return recon, kl, best


def product(cfg, its, epochs, noise, level, seed=0, use_graph=True, trainer_cls=None):
    torch.manual_seed(1234)
    m = dvae.DVAE(cfg["I"], cfg["H"], cfg["Z"])
    tr = (trainer_cls or dvae.DVAETrainer)(m, *its, noise=noise, level=level, seed=seed)
    tr.use_graph = use_graph
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(epochs)
    torch.cuda.synchronize()
    return tr, m


def lclose(got, ref, tol=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    assert err.max() <= tol, (err.max(), got[:4], ref[:4])


SMALL = dict(I=64, H=48, Z=8, side=8, batch=32, n_train=200, n_val=48, n_test=48, epochs=2)
SMALL_FP32 = dict(SMALL, binary=False)
FULL = dict(I=784, H=400, Z=20, side=28, batch=512, n_train=3 * 512 + 336, n_val=512, n_test=64, epochs=1)
# outside the VAE's fused launches: Z % 4 != 0, and Z > 32 with a hidden width > 512
ODD_Z = dict(I=64, H=48, Z=6, side=8, batch=32, n_train=200, n_val=48, n_test=48, epochs=2)
WIDE = dict(I=64, H=520, Z=40, side=8, batch=32, n_train=80, n_val=32, n_test=32, epochs=1)
LEVEL = {"salt_pepper": 0.25, "gaussian": 0.3}


def mk_loaders(cfg):
    return loaders(cfg["batch"], cfg["n_train"], cfg["n_val"], cfg["n_test"], cfg["side"],
                   binary=cfg.get("binary", True))


def parity(cfg, noise, trainer_cls=None, tol_w=5e-5, seed=5):
    level = LEVEL[noise]
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    torch.manual_seed(1234)
    init = dvae.DVAE(cfg["I"], cfg["H"], cfg["Z"])
    with torch.random.fork_rng(devices=[]):                # (the oracle's placeholder layers draw)
        o = Oracle(init)
    recon, kl, best = oracle_train(o, its, cfg["epochs"], noise, level, seed)
    o_rng = torch.get_rng_state()
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, cfg["epochs"], noise, level, seed=seed, trainer_cls=trainer_cls)
    lclose(np.array(tr.recon_loss) / 100, np.array(recon) / 100)
    lclose(tr.kl_loss, kl)
    assert abs(tr.best_val_loss - best) <= 1e-5 * max(1, abs(best))
    assert torch.equal(torch.get_rng_state(), o_rng)
    assert tr.noise_steps == cfg["epochs"] * len(its[0])
    ref = o.state()
    for k, v in m.state_dict().items():
        assert (v.cpu() - ref[k].detach()).abs().max().item() <= tol_w, k
    return tr


@pytest.mark.parametrize("noise", ["salt_pepper", "gaussian"])
@pytest.mark.parametrize("cfg", [SMALL, SMALL_FP32, FULL, ODD_Z, WIDE],
                         ids=["small-ragged", "small-fp32", "784-400-20-b512", "z6-fallback", "z40-h520-fallback"])
def test_dvae_engine_vs_oracle(cfg, noise):
    tr = parity(cfg, noise)
    assert type(tr._engine).__name__ == "DVAEEngine"


@pytest.mark.parametrize("noise", ["salt_pepper", "gaussian"])
@pytest.mark.parametrize("cfg", [SMALL, FULL, ODD_Z, WIDE], ids=["small", "784-400-20-b512", "z6", "z40-h520"])
def test_teacher_forced_step_gradients_vs_fp64(cfg, noise):
    """One training batch through DVAEEngine from known weights: every gradient it leaves in the flat gradient buffer
    against fp64 autograd on the same clean x, corrupted x~ (the device's, corrupt() at step 0) and eps, within 1.5e-6
    of each tensor's scale."""
    b = cfg["batch"]
    its = loaders(b, b, b, 16, cfg["side"])
    torch.manual_seed(1234)
    m = dvae.DVAE(cfg["I"], cfg["H"], cfg["Z"])
    init = {k: v.detach().clone().double() for k, v in m.state_dict().items()}
    tr = dvae.DVAETrainer(m, *its, noise=noise, level=LEVEL[noise], seed=3)
    st = torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    torch.cuda.synchronize()
    fp = tr._engine.fp
    got = {k: fp.gviews[[i for i, q in enumerate(fp.params) if q is p][0]].cpu().double()
           for k, p in m.named_parameters()}
    assert len(got) == 10
    torch.set_rng_state(st)
    perm = trainers._epoch_order(its[0])
    eps = torch.randn(b, cfg["Z"]).double()
    x32 = its[0].dataset.tensors[0][perm].reshape(b, -1)
    xt = dvae.corrupt(x32, noise, LEVEL[noise], 3, step=0).cpu().double()
    x = x32.double()
    assert not torch.equal(xt, x)
    P = {k: v.clone().requires_grad_() for k, v in init.items()}
    h = F.relu(xt @ P["encoder.linear.weight"].T + P["encoder.linear.bias"])
    mu = h @ P["encoder.mu.weight"].T + P["encoder.mu.bias"]
    lv = h @ P["encoder.log_var.weight"].T + P["encoder.log_var.bias"]
    z = mu + eps * torch.exp(lv / 2)
    hd = F.relu(z @ P["decoder.linear.weight"].T + P["decoder.linear.bias"])
    out = torch.sigmoid(hd @ P["decoder.recon.weight"].T + P["decoder.recon.bias"])
    loss = torch.sum((x - out) ** 2) + kl_sum(mu, lv)
    loss.backward()
    for k, g in got.items():
        ref = P[k].grad
        scale = ref.abs().max().item()
        assert scale > 0, k
        err = (g - ref).abs().max().item()
        assert err <= 1.5e-6 * scale, (k, err, scale)


def snapshot(tr, m):
    return (list(tr.recon_loss), list(tr.kl_loss), tr.best_val_loss,
            {k: v.cpu().clone() for k, v in m.state_dict().items()}, torch.get_rng_state())


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]
    assert torch.equal(a[4], b[4])
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("noise", ["salt_pepper", "gaussian"])
@pytest.mark.parametrize("cfg", [SMALL, FULL], ids=["small", "784-400-20-b512"])
def test_level_zero_equals_the_vae_bit_for_bit(cfg, noise):
    torch.manual_seed(99)
    tr, m = product(cfg, mk_loaders(cfg), cfg["epochs"], noise, 0.0)
    got = snapshot(tr, m)
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    torch.manual_seed(1234)
    mv = vae.VAE(cfg["I"], cfg["H"], cfg["Z"])
    tv = vae.VAETrainer(mv, *its)
    with contextlib.redirect_stdout(io.StringIO()):
        tv.train(cfg["epochs"])
    torch.cuda.synchronize()
    same(got, snapshot(tv, mv))


@pytest.mark.parametrize("noise", ["salt_pepper", "gaussian"])
def test_bitwise_reproducibility_and_resume(noise, tmp_path):
    cfg, level = SMALL, LEVEL[noise]
    runs = []
    for use_graph in (True, True, False):                   # graph twice (same seed), then eager
        torch.manual_seed(99)
        tr, m = product(cfg, mk_loaders(cfg), 2, noise, level, use_graph=use_graph)
        runs.append(snapshot(tr, m))
    same(runs[1], runs[0])
    same(runs[2], runs[0])
    torch.manual_seed(99)
    tr, m = product(cfg, mk_loaders(cfg), 2, noise, level, seed=6)
    other = snapshot(tr, m)
    assert any(not torch.equal(other[3][k], runs[0][3][k]) for k in other[3])
    # train(1) + save + load into a fresh trainer + train(1) == train(2): the noise stream continues
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 1, noise, level)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    m2 = dvae.DVAE(cfg["I"], cfg["H"], cfg["Z"]).to(DEV)
    tr2 = dvae.DVAETrainer(m2, *its, noise=noise, level=level, seed=0)
    tr2.load_checkpoint(path)
    assert tr2.noise_steps == len(its[0])
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1)
    torch.cuda.synchronize()
    same(snapshot(tr2, m2), runs[0])
    # a checkpoint of other noise settings is refused under strict=True, taken under strict=False
    for bad in (dict(noise=noise, level=level, seed=1), dict(noise=noise, level=level / 2, seed=0),
                dict(noise="gaussian" if noise == "salt_pepper" else "salt_pepper", level=0.1, seed=0)):
        t3 = dvae.DVAETrainer(dvae.DVAE(cfg["I"], cfg["H"], cfg["Z"]).to(DEV), *its, **bad)
        t3.load_checkpoint(path)
        with pytest.raises(GMError):
            t3.train(1)
    t3 = dvae.DVAETrainer(dvae.DVAE(cfg["I"], cfg["H"], cfg["Z"]).to(DEV), *its, noise=noise, level=level, seed=1)
    t3.load_checkpoint(path, strict=False)
    with contextlib.redirect_stdout(io.StringIO()):
        t3.train(1)
    # train(1); train(1): each call builds a new optimizer (vae.py:127-142), the noise stream runs on.  The second
    # call equals a fresh trainer from the first call's weights and RNG state whose noise_steps say where it is.
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 1, noise, level)
    w1, rng1 = {k: v.clone() for k, v in m.state_dict().items()}, torch.get_rng_state()
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    torch.cuda.synchronize()
    assert tr.noise_steps == 2 * len(its[0])
    two = snapshot(tr, m)
    for steps, equal in ((len(its[0]), True), (0, False)):
        m4 = dvae.DVAE(cfg["I"], cfg["H"], cfg["Z"]).to(DEV)
        t4 = dvae.DVAETrainer(m4, *its, noise=noise, level=level, seed=0)
        m4.load_state_dict(w1)
        t4.noise_steps = steps
        torch.set_rng_state(rng1)
        with contextlib.redirect_stdout(io.StringIO()):
            t4.train(1)
        torch.cuda.synchronize()
        assert t4.recon_loss == two[0][len(its[0]):] if equal else t4.recon_loss != two[0][len(its[0]):]
        if equal:
            for k, v in m4.state_dict().items():
                assert torch.equal(v.cpu(), two[3][k]), k


@pytest.mark.parametrize("noise", ["salt_pepper", "gaussian"])
def test_general_path_agrees_with_the_fused_run(noise):
    class Mine(dvae.DVAETrainer):
        def compute_batch(self, batch):
            return super().compute_batch(batch)
    cfg = dict(SMALL, n_train=96, epochs=2)
    tr = parity(cfg, noise, trainer_cls=Mine)
    assert tr._engine is None


def test_denoising():
    """Bands on 16 x 16 images (two adjacent rows or two adjacent columns lit: 16 patterns), salt-and-pepper p = 0.25:
    after training, the decoding of a corrupted test image is closer to its clean image than the corrupted image is."""
    g = torch.Generator().manual_seed(0)

    def bands(n):
        x = torch.zeros(n, 1, 16, 16)
        k = torch.randint(0, 16, (n,), generator=g)
        for i in range(n):
            j = 2 * (int(k[i]) % 8)
            if k[i] < 8:
                x[i, 0, j:j + 2, :] = 1.0
            else:
                x[i, 0, :, j:j + 2] = 1.0
        return torch.utils.data.DataLoader(torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64)),
                                           batch_size=64, shuffle=True)
    its = bands(2048), bands(256), bands(256)
    torch.manual_seed(5)
    m = dvae.DVAE(256, 128, 8)
    tr = dvae.DVAETrainer(m, *its, noise="salt_pepper", level=0.25, seed=2)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(20, lr=3e-3)
    clean = its[2].dataset.tensors[0].reshape(256, -1).to(DEV)
    st = torch.get_rng_state()
    noisy, recon = tr.denoise(clean)
    assert torch.equal(st, torch.get_rng_state())
    assert torch.equal(noisy, dvae.corrupt(clean, "salt_pepper", 0.25, 2, step=0))
    e_noisy = ((noisy - clean) ** 2).mean().item()
    e_recon = ((recon - clean) ** 2).mean().item()
    wrong = ((recon > 0.5).float() != clean).float().mean().item()
    print("denoise: mse(noisy, clean) %.5f, mse(recon, clean) %.5f, wrong pixels after rounding %.5f"
          % (e_noisy, e_recon, wrong))
    # measured on an MI355X: mse(noisy) 0.12506, mse(recon) 0.00134, 0.128 % of the rounded pixels wrong
    assert e_recon < 0.1 * e_noisy and wrong < 0.02, (e_recon, e_noisy, wrong)


def test_validation_is_clean():
    """best_val_loss is the clean validation loss: evaluate() with the trained model in eval mode corrupts nothing."""
    cfg = SMALL
    torch.manual_seed(99)
    its = mk_loaders(cfg)
    tr, m = product(cfg, its, 1, "salt_pepper", 1.0)
    m.eval()
    n0 = tr.noise_steps
    with torch.no_grad():
        r, k = tr.compute_batch(next(iter(its[1])))
    assert tr.noise_steps == n0                               # eval mode: no corruption, no step taken
    m.train()
    with torch.no_grad():
        tr.compute_batch(next(iter(its[1])))
    assert tr.noise_steps == n0 + 1
