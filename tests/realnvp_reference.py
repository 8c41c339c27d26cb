"""The RealNVP contract (generative_models_amd/realnvp.py's docstring) restated in torch fp64: preprocessing, split,
forward, inverse, loss, gradients by autograd, and the trainer's protocol as a CPU loop.  It takes the noise u and the
normals z as inputs, so every comparison runs on the device's own noise.  The reference of the tests; never the code
under test."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# the project's bounds (DESIGN.md sections 20 / 21), each relative to the tensor's scale
GRAD_TOL, LOSS_TOL, PARAM_TOL = 1.5e-6, 1e-5, 5e-5

TAG_TRAIN, TAG_EVAL, TAG_S = 0x4E565044, 0x4E565056, 0x4E565053      # "NVPD", "NVPV", "NVPS"


def keys(K):
    return ["couplings.%d.%s.%s" % (k, l, p) for k in range(K) for l in ("linear", "out") for p in ("weight", "bias")]


def f64(sd):
    return {n: v.detach().cpu().double().clone() for n, v in sd.items()}


def split_idx(D, mask):
    e = np.arange(D)
    if mask == "checker":
        return e[e % 2 == 0], e[e % 2 == 1]
    Da = -(-D // 2)
    return e[e < Da], e[e >= Da]


def split(y, mask):
    ia, ib = split_idx(y.shape[1], mask)
    return y[:, ia], y[:, ib]


def merge(a, b, mask):
    D = a.shape[1] + b.shape[1]
    ia, ib = split_idx(D, mask)
    y = torch.zeros(a.shape[0], D, dtype=a.dtype)
    y[:, ia] = a
    y[:, ib] = b
    return y


def pre(x, u, alpha, levels, dtype=torch.float64):
    """(y [n, D], logdet [n]) by the contract's formulas, fp64 (dtype=torch.float32: the fp32 restatement)."""
    x, u = torch.as_tensor(x).to(dtype), torch.as_tensor(u).to(dtype)
    q = torch.floor(x * (levels - 1) + 0.5)
    v = (q + u) / levels
    w = alpha + (1.0 - 2.0 * alpha) * v
    return torch.log(w) - torch.log1p(-w), (math.log(1.0 - 2.0 * alpha) - torch.log(w) - torch.log1p(-w)).sum(1)


def quantise(x, levels):
    return torch.floor(torch.as_tensor(x).double() * (levels - 1) + 0.5)


def post(y, alpha):
    return torch.clamp((torch.sigmoid(y) - alpha) / (1.0 - 2.0 * alpha), 0.0, 1.0)


def st_of(P, k, xc):
    h = F.relu(xc @ P["couplings.%d.linear.weight" % k].t() + P["couplings.%d.linear.bias" % k])
    return h @ P["couplings.%d.out.weight" % k].t() + P["couplings.%d.out.bias" % k]


def couple(st, x, cap):
    """(y, sum s) of one coupling on its transformed half."""
    dt = x.shape[1]
    s = cap * torch.tanh(st[:, :dt])
    return x * torch.exp(s) + st[:, dt:], s.sum(1)


def couple_inv(st, y, cap):
    dt = y.shape[1]
    return (y - st[:, dt:]) * torch.exp(-cap * torch.tanh(st[:, :dt]))


def couple_bwd(st, x, g, c, cap):
    """(dst, dx) by the contract's closed form."""
    dt = x.shape[1]
    e = torch.exp(cap * torch.tanh(st[:, :dt]))
    q = torch.exp(-2.0 * st[:, :dt].abs())
    sech2 = 4.0 * q / ((1.0 + q) * (1.0 + q))        # 1 - tanh^2 without the cancellation of a saturated tanh
    return torch.cat([(g * x * e + c) * cap * sech2, g], 1), g * e


def forward(P, y, K, cap, mask):
    """(z, logdet) of logit-space rows y."""
    h = list(split(y, mask))
    logdet = torch.zeros(y.shape[0], dtype=y.dtype)
    for k in range(K):
        t = 1 - (k & 1)
        h[t], s = couple(st_of(P, k, h[1 - t]), h[t], cap)
        logdet = logdet + s
    return merge(h[0], h[1], mask), logdet


def inverse(P, z, K, cap, mask):
    h = list(split(z, mask))
    for k in reversed(range(K)):
        t = 1 - (k & 1)
        h[t] = couple_inv(st_of(P, k, h[1 - t]), h[t], cap)
    return merge(h[0], h[1], mask)


def nll_const(D, levels):
    return 0.5 * D * math.log(2.0 * math.pi) + D * math.log(levels)


def nll_rows(P, x, u, cfg):
    """nll_r of pixel rows x under the noise u; cfg: dict(K, s_cap, mask, alpha, levels)."""
    y, ld0 = pre(x, u, cfg["alpha"], cfg["levels"], next(iter(P.values())).dtype)
    z, ld = forward(P, y, cfg["K"], cfg["s_cap"], cfg["mask"])
    return 0.5 * (z * z).sum(1) + nll_const(x.shape[1], cfg["levels"]) - ld0 - ld


def encode(P, x, u, cfg):
    y, ld0 = pre(x, u, cfg["alpha"], cfg["levels"])
    z, ld = forward(P, y, cfg["K"], cfg["s_cap"], cfg["mask"])
    return z, -(0.5 * (z * z).sum(1) + nll_const(x.shape[1], cfg["levels"]) - ld0 - ld)


def decode(P, z, cfg):
    return post(inverse(P, z, cfg["K"], cfg["s_cap"], cfg["mask"]), cfg["alpha"])


def loss_and_grads(P, x, u, cfg):
    P = {n: v.clone().requires_grad_(True) for n, v in P.items()}
    loss = nll_rows(P, x, u, cfg).sum() / x.shape[0]
    loss.backward()
    return loss.item(), {n: v.grad for n, v in P.items()}


def oracle_train(P, cfg, its, epochs, rows, noise, lr=1e-3, wd=0.0, steps0=0, dtype=torch.float64):
    """RealNVPTrainer's protocol in fp64 on the CPU: next(iter(test)) first, then per epoch a training pass (Adam on the
    mean NLL; batch i of the run under noise(TAG_TRAIN, steps0 + i, b)) and a validation pass (batch i under
    noise(TAG_EVAL, i, b)).  rows(x) -> the batch's rows as the device gathered them; noise(tag, step, b) -> u [b, D].
    Returns (losses, validation losses per epoch, parameters, Adam's state).  dtype=torch.float32: the same arithmetic in
    fp32, the yardstick of an allowance (4 x its deviation from the fp64 run)."""
    P = {n: torch.nn.Parameter(v.to(dtype)) for n, v in f64(P).items()}
    rows_, noise_ = rows, noise
    rows, noise = (lambda x: rows_(x).to(dtype)), (lambda tag, step, b: noise_(tag, step, b).to(dtype))
    next(iter(its[2]))
    opt = torch.optim.Adam(list(P.values()), lr=lr, weight_decay=wd)
    losses, vals, step = [], [], steps0
    for _ in range(epochs):
        for x, _y in its[0]:
            x = rows(x.view(x.shape[0], -1))
            opt.zero_grad()
            loss = nll_rows(P, x, noise(TAG_TRAIN, step, x.shape[0]), cfg).sum() / x.shape[0]
            loss.backward()
            opt.step()
            losses.append(loss.item())
            step += 1
        v = []
        with torch.no_grad():
            for i, (x, _y) in enumerate(its[1]):
                x = rows(x.view(x.shape[0], -1))
                v.append((nll_rows(P, x, noise(TAG_EVAL, i, x.shape[0]), cfg).sum() / x.shape[0]).item())
        vals.append(float(np.mean(v)))
    state = {n: opt.state[v] for n, v in P.items()}
    return losses, vals, {n: v.detach() for n, v in P.items()}, state


def random_weights(D, H, K, seed=0, out_scale=0.5):
    """A state_dict (float32) with non-zero out layers: the flow is not the identity."""
    g = torch.Generator().manual_seed(seed)
    Da, Db = -(-D // 2), D // 2
    sd = {}
    for k in range(K):
        dc, dt = (Da, Db) if k % 2 == 0 else (Db, Da)
        r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
        sd["couplings.%d.linear.weight" % k] = r(H, dc) * (2.0 / dc ** 0.5)
        sd["couplings.%d.linear.bias" % k] = r(H) * 0.5
        sd["couplings.%d.out.weight" % k] = r(2 * dt, H) * (out_scale / H ** 0.5)
        sd["couplings.%d.out.bias" % k] = r(2 * dt) * 0.1
    return sd


# ---- the learning test's data: 64 rows at D = 16 made of 4 fixed grey-level patterns ------------------------------------
def pattern_data(n=64, D=16, seed=3):
    g = torch.Generator().manual_seed(seed)
    pats = torch.floor(torch.rand(4, D, generator=g) * 256.0) / 255.0
    return pats[torch.arange(n) % 4].clamp(0.0, 1.0)
