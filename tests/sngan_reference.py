"""sngan.py's contract restated in plain torch (any dtype, CPU): the critic's forward with its power-iteration step, the
two losses, the closed-form weight gradients, a whole training loop that replays the RNG protocol, and the fp32-vs-fp64
allowance the GPU tests hold their bounds against.  Imported by tests/test_sngan_cpu.py and tests/test_gpu_sngan.py."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-12
# the project's bounds (tests/test_gpu_aae.py)
KERNEL_TOL, LOSS_TOL, PARAM_TOL, LOCKSTEP_TOL = 2e-5, 1e-5, 5e-5, 1.5e-6


def power_step(W, u, training=True):
    """(u', v): v = normalize(W^T u); u' = normalize(W v) in training mode, the stored u otherwise."""
    v = F.normalize(W.t() @ u, dim=0, eps=EPS)
    return (F.normalize(W @ v, dim=0, eps=EPS) if training else u), v


def critic(x, W, b, w2, b2, u, training=True):
    """s(x) and the forward's pieces; u' and v are constants of the backward."""
    with torch.no_grad():
        u1, v = power_step(W.detach(), u, training)
    sigma = u1 @ (W @ v)
    Wbar = W / sigma
    w2bar = w2.reshape(-1) / torch.linalg.vector_norm(w2)
    h = torch.relu(x @ Wbar.t() + b)
    s = h @ w2bar + b2.reshape(())
    return s, dict(u=u1, v=v, sigma=sigma, Wbar=Wbar, w2bar=w2bar, h=h)


def d_loss(s, B):
    return torch.mean(torch.relu(1 - s[:B])) + torch.mean(torch.relu(1 + s[B:]))


def g_loss(s):
    return -torch.mean(s)


def closed_gW(G, Wbar, u, v, sigma):
    return (G - (G * Wbar).sum() * torch.outer(u, v)) / sigma


def closed_gw2(g, w2bar, nw2):
    return (g - (g @ w2bar) * w2bar) / nw2


def kink_distance(s, B):
    """The smallest |1 - s| over real rows and |1 + s| over fake rows."""
    return min((1 - s[:B]).abs().min().item(), (1 + s[B:]).abs().min().item())


def critic_step_case(B, I, H, seed, dtype=torch.float64):
    """A critic step's inputs at ns_gan.py's initialisation scale: binary x rows, G(z)-like rows in (0, 1), nn.Linear's
    uniform weights (every hinge term is active there, as at the start of training)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.cat([torch.bernoulli(torch.full((B, I), 0.3), generator=g), torch.rand(B, I, generator=g)])
    W = (torch.rand(H, I, generator=g) * 2 - 1) / I ** 0.5
    b = (torch.rand(H, generator=g) * 2 - 1) / I ** 0.5
    w2 = (torch.rand(1, H, generator=g) * 2 - 1) / H ** 0.5
    b2 = (torch.rand(1, generator=g) * 2 - 1) / H ** 0.5
    u = F.normalize(torch.randn(H, generator=g), dim=0, eps=EPS)
    return [t.to(dtype) for t in (x, W, b, w2, b2, u)]


def critic_step(x, W, b, w2, b2, u, B):
    """loss, gW, gb, gw2, u', v, sigma, s of one critic step by autograd (gb2 is a sum of +-1 / B: exact, left out)."""
    W, b, w2, b2 = (t.clone().requires_grad_() for t in (W, b, w2, b2))
    s, f = critic(x, W, b, w2, b2, u)
    loss = d_loss(s, B)
    gW, gb, gw2 = torch.autograd.grad(loss, (W, b, w2))
    return dict(loss=loss.detach().reshape(1), gW=gW, gb=gb, gw2=gw2, u=f["u"], v=f["v"],
                sigma=f["sigma"].detach().reshape(1), s=s.detach())


ALLOWANCE_SHAPES = [(4, 16, 8), (8, 20, 12), (5, 36, 24), (16, 784, 400)]
_ALLOWANCE = {}


def fp32_allowance(shapes=ALLOWANCE_SHAPES):
    """The worst |fp32 - fp64| / max|fp64| of a plain-torch critic step on the CPU over `shapes`, per quantity: what
    fp32 arithmetic alone costs (computed once per process).  The GPU tests assert that it is inside their bounds."""
    key = tuple(shapes)
    if key not in _ALLOWANCE:
        worst = {}
        for B, I, H in shapes:
            case = critic_step_case(B, I, H, 100 * H + B)
            r64 = critic_step(*case, B)
            r32 = critic_step(*[t.float() for t in case], B)
            for k, r in r64.items():
                e = (r32[k].double() - r).abs().max().item() / max(r.abs().max().item(), 1e-300)
                worst[k] = max(worst.get(k, 0.0), e)
        _ALLOWANCE[key] = worst
    return _ALLOWANCE[key]


class Oracle:
    """The SN-GAN as plain tensors on the CPU, initialised from the product model's state_dict."""
    G_KEYS = ("G.linear.weight", "G.linear.bias", "G.generate.weight", "G.generate.bias")
    D_KEYS = ("D.linear.weight", "D.linear.bias", "D.discriminate.weight", "D.discriminate.bias")

    def __init__(self, model, dtype=torch.float32, freeze_u=False):
        sd = {k: v.detach().cpu().clone().to(dtype) for k, v in model.state_dict().items()}
        self.p = {k: sd[k].requires_grad_() for k in self.G_KEYS + self.D_KEYS}
        self.u = sd["D.u"]
        self.dtype, self.freeze_u = dtype, freeze_u
        self.min_kink = float("inf")

    def gparams(self):
        return [self.p[k] for k in self.G_KEYS]

    def dparams(self):
        return [self.p[k] for k in self.D_KEYS]

    def G(self, z):
        p = self.p
        h = torch.relu(z @ p["G.linear.weight"].t() + p["G.linear.bias"])
        return torch.sigmoid(h @ p["G.generate.weight"].t() + p["G.generate.bias"])

    def D(self, x):
        p = self.p
        s, f = critic(x, p["D.linear.weight"], p["D.linear.bias"], p["D.discriminate.weight"],
                      p["D.discriminate.bias"], self.u, training=not self.freeze_u)
        self.u = f["u"]
        return s

    def d_loss(self, x, z):
        B = x.shape[0]
        s = self.D(torch.cat([x, self.G(z).detach()]))
        self.min_kink = min(self.min_kink, kink_distance(s.detach(), B))
        return d_loss(s, B)

    def g_loss(self, z):
        return g_loss(self.D(self.G(z)))

    def state(self):
        return dict({k: v.detach() for k, v in self.p.items()}, **{"D.u": self.u})


def oracle_train(o, train_iter, epochs, G_lr=1e-4, D_lr=4e-4, D_steps=1, betas=(0.0, 0.9)):
    """ns_gan.py:94-170 with sngan.py's losses and optimizers; every draw comes from the global CPU generator in fp32."""
    Z = o.p["G.linear.weight"].shape[1]
    G_opt = torch.optim.Adam(o.gparams(), lr=G_lr, betas=betas)
    D_opt = torch.optim.Adam(o.dparams(), lr=D_lr, betas=betas)
    steps = int(np.ceil(len(train_iter) / D_steps))
    Gl, Dl = [], []
    for _ in range(epochs):
        for _ in range(steps):
            step = []
            for _ in range(D_steps):
                x, _ = next(iter(train_iter))
                x = x.view(x.shape[0], -1).to(o.dtype)
                D_opt.zero_grad()
                d = o.d_loss(x, torch.randn(x.shape[0], Z).to(o.dtype))
                d.backward()
                D_opt.step()
                step.append(d.item())
            Dl.append(np.mean(step))
            G_opt.zero_grad()
            g = o.g_loss(torch.randn(x.shape[0], Z).to(o.dtype))
            g.backward()
            G_opt.step()
            Gl.append(g.item())
    return Gl, Dl
