"""Bayesian GAN on the MI355X: the Philox generator against Random123's known answers and a pure-Python reference,
gm_sghmc_step and gm_bgan_head against fp64, whole iterations against an fp64 oracle of the contract, fused vs general
path, bitwise determinism and resume, the global generator's cursor, sampling."""
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

import bayes_gan  # noqa: E402
import ns_gan  # noqa: E402
from generative_models_amd import ops_fused  # noqa: E402
from generative_models_amd._lib import GMError  # noqa: E402
from generative_models_amd.engine import draw_sampler_indices  # noqa: E402
from generative_models_amd.ops_fused import bgan_stream_latent as LAT, bgan_stream_param as PAR  # noqa: E402

DEV = "cuda"
EPS = 1e-8
M32 = 0xFFFFFFFF
SEED = 0x1234_5678_9ABC


def philox(ctr, key):
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k[1]) & M32, p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return c


def py_normals(seed, stream, t, n):
    """The contract's Normal(stream, t) in Python with an fp64 Box-Muller."""
    out = []
    u = lambda x: (2 * (x >> 9) + 1) * 2.0 ** -24
    for q in range((n + 3) // 4):
        x = philox([q, t & M32, stream, 0], [seed & M32, (seed >> 32) & M32])
        for a, b in ((x[0], x[1]), (x[2], x[3])):
            r = math.sqrt(-2.0 * math.log(u(a)))
            out += [r * math.cos(2 * math.pi * u(b)), r * math.sin(2 * math.pi * u(b))]
    return np.array(out[:n])


def normals(stream, t, n, seed=SEED):
    return ops_fused.philox_normal(seed, stream, t, n, device=DEV).view(-1)


# ---- 1, 2: the generator --------------------------------------------------------------------------------------------
def test_philox_raw_known_answers():
    ctr = [[0] * 4, [M32] * 4, [0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344]]
    key = [[0, 0], [M32, M32], [0xa4093822, 0x299f31d0]]
    want = [[0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd],
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]]
    i32 = lambda rows: torch.tensor(np.array(rows, dtype=np.uint32).view(np.int32), device=DEV)
    got = ops_fused.philox_raw(i32(ctr), i32(key)).cpu().numpy().view(np.uint32)
    assert got.tolist() == want


@pytest.mark.parametrize("n,t,stream", [(1, 0, PAR(0, 0, 0)), (7, 3, LAT(1, 2)), (13, 2 ** 31 + 7, PAR(1, 15, 3)),
                                        (1002, 123456789, LAT(0, 5)), (4096, M32, PAR(0, 3, 1))])
def test_normals_vs_python_reference(n, t, stream):
    got = normals(stream, t, n).double().cpu().numpy()
    want = py_normals(SEED, stream, t, n)
    assert np.all(np.abs(got - want) <= 4e-6 * np.maximum(1.0, np.abs(want)))
    longer = normals(stream, t, n + 13)
    assert torch.equal(longer[:n], normals(stream, t, n))            # a draw is a prefix of a longer one
    # several streams in one launch equal the single-stream draws
    multi = ops_fused.philox_normal(SEED, stream, t, n, nstreams=3, stream_stride=16, device=DEV)
    for j in range(3):
        assert torch.equal(multi[j], normals(stream + 16 * j, t, n))
    # the step can come from a device counter
    ctr = torch.tensor([t - 3], dtype=torch.int64, device=DEV)
    assert torch.equal(ops_fused.philox_normal(SEED, stream, 3, n, step=ctr, device=DEV).view(-1),
                       normals(stream, t, n))


def test_normal_moments():
    x = normals(LAT(0, 1), 17, 1 << 22).double()
    assert abs(x.mean().item()) < 2e-3 and abs(x.var().item() - 1.0) < 2e-3
    assert torch.isfinite(x).all()


# ---- 3: SGHMC ---------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 5, 401, 313600)


def _sghmc_case(gen, offsets_shift=0):
    segs, o = [], 0
    for i, n in enumerate(SIZES):
        o += offsets_shift * (i % 2)                    # odd segments start off the 4-element grid
        segs.append((o, n, PAR(i % 2, i, i % 4)))
        o += n
    N = o + 3
    r = lambda s: torch.randn(N, generator=gen) * s
    return segs, N, r(0.05), r(1.0), r(0.01)


@pytest.mark.parametrize("shift", [0, 1])
def test_sghmc_step_vs_fp64(shift):
    gen = torch.Generator().manual_seed(3)
    segs, N, th0, g0, v0 = _sghmc_case(gen, shift)
    th, g, v = (x.to(DEV) for x in (th0, g0, v0))
    lr, alpha, prior, noise, t = 2e-3, 0.1, 1.0 / 5000, 2 * 0.1 / 5000, 77
    ops_fused.sghmc_step(th, g, v, segs, torch.tensor([lr], device=DEV), alpha, prior, noise, SEED, t=t)
    wth, wv = th0.double().clone(), v0.double().clone()
    for o, n, s in segs:
        xi = normals(s, t, n).double().cpu()
        xi64 = torch.from_numpy(py_normals(SEED, s, t, min(n, 64)))
        assert torch.allclose(xi[:64], xi64, atol=4e-6 * 6, rtol=0)     # xi is the normals op's draw
        sl = slice(o, o + n)
        f32 = lambda x: float(np.float32(x))
        gg = g0[sl].double() + th0[sl].double() * f32(prior)
        wv[sl] = (1 - f32(alpha)) * v0[sl].double() - f32(lr) * gg + math.sqrt(f32(noise) * f32(lr)) * xi
        wth[sl] = th0[sl].double() + wv[sl]
    got_th, got_v = th.cpu().double(), v.cpu().double()
    assert (got_v - wv).abs().max() <= 1e-6 * wv.abs().max()
    assert (got_th - wth).abs().max() <= 1e-6 * wth.abs().max()
    mask = torch.ones(N, dtype=torch.bool)
    for o, n, _ in segs:
        mask[o:o + n] = False
    assert torch.equal(th.cpu()[mask], th0[mask]) and torch.equal(v.cpu()[mask], v0[mask])   # gaps untouched
    # two runs: the same bits
    th2, v2 = th0.to(DEV), v0.to(DEV)
    ops_fused.sghmc_step(th2, g, v2, segs, torch.tensor([lr], device=DEV), alpha, prior, noise, SEED, t=t)
    assert torch.equal(th2, th) and torch.equal(v2, v)
    # the step from a device counter
    th3, v3 = th0.to(DEV), v0.to(DEV)
    ctr = torch.tensor([70], dtype=torch.int64, device=DEV)
    ops_fused.sghmc_step(th3, g, v3, segs, torch.tensor([lr], device=DEV), alpha, prior, noise, SEED, t=7, step=ctr)
    assert torch.equal(th3, th)


def test_sghmc_full_friction_without_noise_is_sgd():
    gen = torch.Generator().manual_seed(4)
    segs, N, th0, g0, v0 = _sghmc_case(gen)
    th, g, v = th0.to(DEV), g0.to(DEV), v0.to(DEV)
    lr = 1e-2
    ops_fused.sghmc_step(th, g, v, segs, torch.tensor([lr], device=DEV), 1.0, 0.0, 0.0, SEED, t=5)
    want = th0.clone()
    for o, n, _ in segs:
        want[o:o + n] = th0[o:o + n] - torch.tensor(lr, dtype=torch.float32) * g0[o:o + n]
    assert torch.equal(th.cpu(), want)


# ---- 4: the ensemble head ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Jd", [1, 2, 3])
@pytest.mark.parametrize("Jg", [1, 2, 4])
@pytest.mark.parametrize("mode", [0, 1])
def test_head_vs_fp64(mode, Jg, Jd):
    B, H = 37, 44
    R = (1 + Jg) * B if mode == 0 else Jg * B
    gen = torch.Generator().manual_seed(10 * Jg + Jd + mode)
    h0 = torch.relu(torch.randn(R, Jd * H, generator=gen))
    w2 = torch.randn(Jd, H, generator=gen) * 0.2
    b2 = torch.randn(Jd, generator=gen) * 0.1
    h = h0.to(DEV)
    ws = ops_fused.bgan_head_workspace(mode, B, Jg, Jd, H, DEV)
    gw2, gb2 = torch.zeros(Jd, H, device=DEV), torch.zeros(Jd, device=DEV)
    loss = torch.zeros(Jd if mode == 0 else Jg, device=DEV)
    ops_fused.bgan_head(h, w2.to(DEV), b2.to(DEV), mode, B, Jg, Jd, ws, gw2=gw2 if mode == 0 else None,
                        gb2=gb2 if mode == 0 else None, loss_out=loss)
    H64 = h0.double().requires_grad_()
    W, bb = w2.double().requires_grad_(), b2.double().requires_grad_()
    s = torch.stack([torch.sigmoid(H64[:, k * H:(k + 1) * H] @ W[k] + bb[k]) for k in range(Jd)])   # [Jd, R]
    if mode == 0:
        L = torch.stack([-(torch.log(s[k, :B] + EPS).mean()
                           + sum(torch.log(1 - s[k, B + j * B:B + (j + 1) * B] + EPS).mean() for j in range(Jg)) / Jg)
                         for k in range(Jd)])
    else:
        L = torch.stack([-sum(torch.log(s[k, j * B:(j + 1) * B] + EPS).mean() for k in range(Jd)) / Jd
                         for j in range(Jg)])
    L.sum().backward()
    # dH w.r.t. the pre-activation hidden rows: d L / d h . [h > 0]
    dH = H64.grad * (h0.double() > 0)
    close = lambda a, b: (a.double().cpu() - b).abs().max().item() <= 1e-5 * max(1e-3, b.abs().max().item())
    assert close(loss, L.detach())
    assert close(h, dH)
    if mode == 0:
        assert close(gw2, W.grad) and close(gb2, bb.grad)


# ---- 5: whole iterations vs an fp64 oracle of the contract -------------------------------------------------------------
SMALL = dict(I=64, H=32, Z=8)
FULL = dict(I=784, H=400, Z=20)


def loaders(batch, n_train, side, seed=7):
    g = torch.Generator().manual_seed(seed)

    def mk(n):
        x = torch.bernoulli(torch.full((n, 1, side, side), 0.3), generator=g)
        ds = torch.utils.data.TensorDataset(x, torch.zeros(n, dtype=torch.int64))
        return torch.utils.data.DataLoader(ds, batch_size=batch, shuffle=True)
    return mk(n_train), mk(64), mk(64)


def product(cfg, Jg, Jd, its, seed=11, cls=None):
    torch.manual_seed(seed)
    m = bayes_gan.BayesGAN(cfg["I"], cfg["H"], cfg["Z"], Jg, Jd).to(DEV)
    return (cls or bayes_gan.BayesGANTrainer)(m, *its, seed=SEED), m


class Oracle:
    """The contract in fp64 torch on the CPU: batch rows from a replay of the global generator, z and xi from the
    normals op (itself checked against the Python reference above)."""

    def __init__(self, m, data, B, N, lr_G, lr_D, alpha, sigma, rng_state, D_steps):
        self.p = {k: v.detach().cpu().double().clone() for k, v in m.state_dict().items()}
        self.v = {k: torch.zeros_like(v) for k, v in self.p.items()}
        self.data, self.B, self.N, self.D_steps = data.reshape(data.shape[0], -1).double(), B, N, D_steps
        self.Jg, self.Jd, self.Z = len(m.G), len(m.D), m.z_dim
        self.lr, self.alpha, self.sigma = {"G": lr_G, "D": lr_D}, alpha, sigma
        self.rng, self.tD, self.tG = rng_state, 0, 0
        self.Dlosses, self.Glosses = [], []

    def _net(self, side, k, x, p):
        sec = "generate" if side == "G" else "discriminate"
        h = torch.relu(x @ p["%s.%d.linear.weight" % (side, k)].T + p["%s.%d.linear.bias" % (side, k)])
        return torch.sigmoid(h @ p["%s.%d.%s.weight" % (side, k, sec)].T + p["%s.%d.%s.bias" % (side, k, sec)])

    def _batch(self):
        with torch.random.fork_rng(devices=[]):
            torch.set_rng_state(self.rng)
            idx = np.empty(self.B, dtype=np.int64)
            draw_sampler_indices(self.data.shape[0], self.B, idx)
            torch.randn(self.B, self.Z)
            self.rng = torch.get_rng_state()
        return self.data[torch.from_numpy(idx)]

    def _z(self, phase, j, t):
        return normals(LAT(phase, j), t, self.B * self.Z).double().cpu().view(self.B, self.Z)

    def _sghmc(self, side, count, grads, t):
        f32 = lambda x: float(np.float32(x))
        lr, a = f32(self.lr[side]), f32(self.alpha)
        prior, noise = f32(1.0 / (self.sigma ** 2 * self.N)), f32(2 * self.alpha / self.N)
        sec = "generate" if side == "G" else "discriminate"
        for k in range(count):
            for ti, name in enumerate(("linear.weight", "linear.bias", sec + ".weight", sec + ".bias")):
                key = "%s.%d.%s" % (side, k, name)
                th = self.p[key]
                xi = normals(PAR(0 if side == "D" else 1, k, ti), t, th.numel()).double().cpu().view(th.shape)
                self.v[key] = (1 - a) * self.v[key] - lr * (grads[key] + th * prior) + math.sqrt(noise * lr) * xi
                self.p[key] = th + self.v[key]

    def iteration(self):
        step = []
        for _ in range(self.D_steps):
            x = self._batch()
            fakes = [self._net("G", j, self._z(0, j, self.tD), self.p) for j in range(self.Jg)]
            q = {k: v.clone().requires_grad_() for k, v in self.p.items() if k.startswith("D.")}
            L = torch.stack([-(torch.log(self._net("D", k, x, q) + EPS).mean()
                               + sum(torch.log(1 - self._net("D", k, f, q) + EPS).mean() for f in fakes) / self.Jg)
                             for k in range(self.Jd)])
            L.sum().backward()
            self._sghmc("D", self.Jd, {k: v.grad for k, v in q.items()}, self.tD)
            self.tD += 1
            step.append(L.mean().item())
        self.Dlosses.append(float(np.mean(step)))
        with torch.random.fork_rng(devices=[]):
            torch.set_rng_state(self.rng)
            torch.randn(self.B, self.Z)
            self.rng = torch.get_rng_state()
        q = {k: v.clone().requires_grad_() for k, v in self.p.items() if k.startswith("G.")}
        L = torch.stack([-sum(torch.log(self._net("D", k, self._net("G", j, self._z(1, j, self.tG), q), self.p) + EPS)
                              .mean() for k in range(self.Jd)) / self.Jd for j in range(self.Jg)])
        L.sum().backward()
        self._sghmc("G", self.Jg, {k: v.grad for k, v in q.items()}, self.tG)
        self.tG += 1
        self.Glosses.append(L.mean().item())


def _run(cfg, Jg, Jd, D_steps, iters, batch=32, cls=None, **kw):
    """A product run of exactly `iters` iterations (one epoch) and the oracle over the same iterations."""
    side = int(cfg["I"] ** 0.5)
    its = loaders(batch, batch * D_steps * iters, side)
    tr, m = product(cfg, Jg, Jd, its, cls=cls)
    N = len(its[0].dataset)
    o = Oracle(m, its[0].dataset.tensors[0], batch, N, kw.get("G_lr", 1e-3), kw.get("D_lr", 1e-3),
               kw.get("friction", 0.1), kw.get("prior_std", 1.0), torch.get_rng_state(), D_steps)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1, D_steps=D_steps, **kw)
    torch.cuda.synchronize()
    for _ in range(iters):
        o.iteration()
    return tr, m, o


def _check(tr, m, o, tol):
    assert len(tr.Dlosses) == len(o.Dlosses) and len(tr.Glosses) == len(o.Glosses)
    for a, b in zip(tr.Dlosses + tr.Glosses, o.Dlosses + o.Glosses):
        assert abs(a - b) <= tol * abs(b), (a, b)
    for k, v in m.state_dict().items():
        want = o.p[k]
        err = (v.detach().cpu().double() - want).abs().max().item()
        assert err <= tol * want.abs().max().item(), (k, err)


@pytest.mark.parametrize("shape", ["small", "full"])
@pytest.mark.parametrize("J", [(1, 1), (4, 2), (3, 3)])
@pytest.mark.parametrize("D_steps", [1, 2])
def test_one_iteration_vs_fp64_oracle(shape, J, D_steps):
    cfg = SMALL if shape == "small" else FULL
    tr, m, o = _run(cfg, J[0], J[1], D_steps, 1)
    assert tr._engine is not None and tr.t_D == D_steps and tr.t_G == 1
    _check(tr, m, o, 1e-5)


@pytest.mark.parametrize("shape", ["small", "full"])
def test_free_running_iterations_vs_fp64_oracle(shape):
    # 12 iterations.  Each update moves a parameter by about lr |g| + sqrt(2 alpha lr / N) ~ 1e-3 of scale ~0.05; its
    # fp32 error is ~1e-6 of that, and storing theta in fp32 adds 6e-8 of the scale per step.  Nothing in 12 steps
    # amplifies those (the parameters move by ~2 % in total), so 12 x (1e-5 one-step bound) / 4 = 3e-5 is generous.
    cfg = SMALL if shape == "small" else FULL
    tr, m, o = _run(cfg, 4, 2, 1, 12)
    _check(tr, m, o, 3e-5)


# ---- 6: fused vs general path --------------------------------------------------------------------------------------------
class SameFormulas(bayes_gan.BayesGANTrainer):
    """Hooks overridden with the contract's own formulas: the general path."""

    def train_D(self, images):
        m = self.model
        b = images.shape[0]
        with torch.no_grad():
            fakes = [g(self.latent(0, j, b)) for j, g in enumerate(m.G)]
        return torch.stack([-(torch.mean(torch.log(d(images) + EPS))
                              + sum(torch.mean(torch.log(1 - d(x) + EPS)) for x in fakes) / len(fakes)) for d in m.D])

    def train_G(self, images):
        m = self.model
        b = images.shape[0]
        xs = [g(self.latent(1, j, b)) for j, g in enumerate(m.G)]
        return torch.stack([-sum(torch.mean(torch.log(d(x) + EPS)) for d in m.D) / len(m.D) for x in xs])


def test_fused_vs_general_path():
    its = loaders(32, 32 * 5, 8)
    tr_f, m_f = product(SMALL, 3, 2, its)
    with contextlib.redirect_stdout(io.StringIO()):
        tr_f.train(1)
    rng_f = torch.get_rng_state()
    tr_g, m_g = product(SMALL, 3, 2, its, cls=SameFormulas)
    with contextlib.redirect_stdout(io.StringIO()):
        tr_g.train(1)
    assert tr_f._engine is not None and tr_g._engine is None
    assert torch.equal(rng_f, torch.get_rng_state())
    assert (tr_f.t_D, tr_f.t_G) == (tr_g.t_D, tr_g.t_G) == (5, 5)
    for a, b in zip(tr_f.Dlosses + tr_f.Glosses, tr_g.Dlosses + tr_g.Glosses):
        assert abs(a - b) <= 1e-5 * abs(b)
    sg = m_g.state_dict()
    for k, v in m_f.state_dict().items():
        assert (v - sg[k]).abs().max().item() <= 1e-5 * sg[k].abs().max().item(), k


# ---- 7: bitwise determinism and resume -----------------------------------------------------------------------------------
def _snap(tr, m):
    return (list(tr.Dlosses), list(tr.Glosses), {k: v.cpu().clone() for k, v in m.state_dict().items()},
            torch.get_rng_state(), (tr.t_D, tr.t_G))


def _same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(a[3], b[3]) and a[4] == b[4]
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k


def test_bitwise_graph_eager_sizes_runs_and_resume(tmp_path):
    its = loaders(32, 32 * 10, 8)                     # 10 steps per epoch at D_steps=1, 5 at D_steps=2
    runs = []
    for use_graph, K in ((True, 4), (True, 4), (True, 1), (False, 4), (True, 16)):
        tr, m = product(SMALL, 4, 2, its)
        tr.use_graph = use_graph
        tr._get_engine().graph_iters = K
        with contextlib.redirect_stdout(io.StringIO()):
            tr.train(2, D_steps=2)
        torch.cuda.synchronize()
        runs.append(_snap(tr, m))
    for r in runs[1:]:
        _same(r, runs[0])
    # train(1) + save_checkpoint + load_checkpoint into a fresh trainer + train(1) == train(2)
    tr, m = product(SMALL, 4, 2, its)
    tr._get_engine().graph_iters = 4
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1, D_steps=2)
    path = str(tmp_path / "ck.pt")
    tr.save_checkpoint(path)
    ck = torch.load(path, weights_only=True)
    assert ck["optim"]["t_D"] == 10 and ck["optim"]["t_G"] == 5 and ck["optim"]["seed"] == SEED
    assert len(ck["optim"]["vD"]) == 8 and len(ck["optim"]["vG"]) == 16
    assert any(v.abs().max() > 0 for v in ck["optim"]["vG"])
    state = torch.get_rng_state()
    torch.manual_seed(0)
    m2 = bayes_gan.BayesGAN(SMALL["I"], SMALL["H"], SMALL["Z"], 4, 2).to(DEV)
    tr2 = bayes_gan.BayesGANTrainer(m2, *its, seed=1)
    tr2.load_checkpoint(path)
    assert torch.equal(torch.get_rng_state(), state) and tr2.seed == SEED and (tr2.t_D, tr2.t_G) == (10, 5)
    with contextlib.redirect_stdout(io.StringIO()):
        tr2.train(1, D_steps=2)
    torch.cuda.synchronize()
    _same(_snap(tr2, m2), runs[0])
    # a new train() call without a checkpoint starts from zero momentum: not the resumed trajectory
    tr3, m3 = product(SMALL, 4, 2, its)
    with contextlib.redirect_stdout(io.StringIO()):
        tr3.train(1, D_steps=2)
        tr3.train(1, D_steps=2)
    assert tr3.Glosses[:5] == runs[0][1][:5] and tr3.Glosses[5:] != runs[0][1][5:]


# ---- 8: the global generator's cursor -----------------------------------------------------------------------------------
@pytest.mark.parametrize("D_steps", [1, 2])
def test_global_rng_state_matches_nsgan(D_steps):
    its = loaders(32, 32 * 6 + 7, 8)
    nm = ns_gan.NSGAN(64, 32, 8).to(DEV)
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        ns_gan.NSGANTrainer(nm, *its).train(2, D_steps=D_steps)
    want = torch.get_rng_state()
    tr, m = product(SMALL, 2, 2, its, seed=21)
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(2, D_steps=D_steps)
    assert tr._engine is not None
    assert torch.equal(torch.get_rng_state(), want)
    tr, m = product(SMALL, 2, 2, its, seed=21, cls=SameFormulas)
    torch.manual_seed(21)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(2, D_steps=D_steps)
    assert tr._engine is None
    assert torch.equal(torch.get_rng_state(), want)


# ---- 9: sampling, Parzen, refusals ------------------------------------------------------------------------------------------
def test_sample_mixture_parzen_and_data_parallel_refusal(monkeypatch):
    its = loaders(32, 128, 8)
    tr, m = product(SMALL, 3, 2, its)
    with contextlib.redirect_stdout(io.StringIO()):
        tr.train(1)
    st = torch.get_rng_state()
    s = tr.sample(20, seed=3)
    assert s.shape == (20, 64) and torch.equal(s, tr.sample(20, seed=3))
    assert torch.equal(st, torch.get_rng_state())
    z = torch.randn(20, 8, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        for i in range(20):
            assert torch.allclose(s[i], m.G[i % 3](z[i:i + 1])[0], atol=1e-6)
    r = tr.parzen(n_samples=200, n_val=32)
    assert all(math.isfinite(v) for v in (r.sigma, r.ll_mean, r.ll_stderr))
    imgs = tr.generate_images(1, num_outputs=16, save=False)
    assert imgs.shape == (16, 8, 8)
    from generative_models_amd import dp
    monkeypatch.setattr(dp, "current", lambda: (2, 0, None))
    with pytest.raises(GMError):
        tr.train(1)
