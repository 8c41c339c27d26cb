"""The MAF contract (generative_models_amd/maf.py's docstring) restated in torch fp64: degrees, masks, the layer map, the
sequential inverse, the loss, gradients by autograd, and the trainer's protocol as a CPU loop with Adam.  It takes the
noise u and the normals z as inputs, so every comparison runs on the device's own noise.  The preprocessing, the
post-processing and the loss constant are RealNVP's and come from tests/realnvp_reference.py.  The reference of the tests;
never the code under test."""
import numpy as np
import torch
import torch.nn.functional as F

import realnvp_reference as NR
from realnvp_reference import nll_const, pattern_data, post, pre, quantise  # noqa: F401

# the project's bounds (DESIGN.md sections 20 / 24), each relative to the tensor's scale
GRAD_TOL, LOSS_TOL, PARAM_TOL = NR.GRAD_TOL, NR.LOSS_TOL, NR.PARAM_TOL

TAG_TRAIN, TAG_EVAL, TAG_S = 0x4D414644, 0x4D414656, NR.TAG_S      # "MAFD", "MAFV", RealNVP's "NVPS"


def keys(K, buffers=False):
    names = ("m_in", "m_h") if buffers else ()
    return ["layers.%d.%s" % (k, n) for k in range(K)
            for n in names + ("linear.weight", "linear.bias", "out.weight", "out.bias")]


def degrees(D, H, K, order="natural", order_seed=0):
    """([m_in of layer 0 .. K - 1], m_h) as int64 arrays, by the contract's rules."""
    if order == "natural":
        m_in = np.arange(1, D + 1)
    else:
        m_in = 1 + np.random.RandomState(order_seed).permutation(D)
    ins = [m_in.astype(np.int64)]
    for _ in range(1, K):
        ins.append(D + 1 - ins[-1])
    m_h = np.array([1 + (j * (D - 1)) // H for j in range(H)], dtype=np.int64)
    return ins, m_h


def masks(m_in, m_h):
    """(M1 [H, D], M2 [2 D, H]) as float64 tensors."""
    m_in, m_h = torch.as_tensor(np.asarray(m_in)).long(), torch.as_tensor(np.asarray(m_h)).long()
    M1 = (m_h[:, None] >= m_in[None, :]).double()
    M2 = (m_in[:, None] > m_h[None, :]).double()
    return M1, torch.cat([M2, M2])


def inv_order(m_in):
    m = np.asarray(m_in).astype(np.int64)
    inv = np.empty(m.size, dtype=np.int64)
    inv[m - 1] = np.arange(m.size)
    return inv


def f64(sd):
    """Floating tensors as float64 CPU copies; the degree buffers stay integers."""
    return {n: (v.detach().cpu().double().clone() if v.is_floating_point() else v.detach().cpu().long().clone())
            for n, v in sd.items()}


def to_dtype(P, dtype):
    return {n: (v.to(dtype) if v.is_floating_point() else v) for n, v in P.items()}


def layer_masks(P, k, dtype=torch.float64):
    M1, M2 = masks(P["layers.%d.m_in" % k].numpy(), P["layers.%d.m_h" % k].numpy())
    return M1.to(dtype), M2.to(dtype)


def ma_of(P, k, y):
    """[m | a] of layer k on rows y; the weights enter as weight * mask."""
    M1, M2 = layer_masks(P, k, y.dtype)
    h = F.relu(y @ (P["layers.%d.linear.weight" % k] * M1).t() + P["layers.%d.linear.bias" % k])
    return h @ (P["layers.%d.out.weight" % k] * M2).t() + P["layers.%d.out.bias" % k]


def couple(ma, y, cap):
    """(u, sum s) of one layer from its [m | a]."""
    D = y.shape[1]
    s = cap * torch.tanh(ma[:, D:])
    return (y - ma[:, :D]) * torch.exp(-s), s.sum(1)


def couple_bwd(ma, u, g, c, cap):
    """(dout [n, 2 D], dy) by the contract's closed form."""
    D = u.shape[1]
    a = ma[:, D:]
    e = torch.exp(-cap * torch.tanh(a))
    q = torch.exp(-2.0 * a.abs())
    sech2 = 4.0 * q / ((1.0 + q) * (1.0 + q))        # 1 - tanh^2 without the cancellation of a saturated tanh
    return torch.cat([-g * e, (-(g * u) - c) * cap * sech2], 1), g * e


def forward(P, y, K, cap):
    """(z, logdet) of logit-space rows y."""
    logdet = torch.zeros(y.shape[0], dtype=y.dtype)
    for k in range(K):
        y, s = couple(ma_of(P, k, y), y, cap)
        logdet = logdet - s
    return y, logdet


def invert_layer(P, k, u, cap):
    """(y, s) with layer k(y) = u: pixel by pixel in order of degree, each step a full pass."""
    D = u.shape[1]
    y, s = torch.zeros_like(u), torch.zeros_like(u)
    for d in inv_order(P["layers.%d.m_in" % k].numpy()):
        ma = ma_of(P, k, y)
        s[:, d] = cap * torch.tanh(ma[:, D + d])
        y[:, d] = u[:, d] * torch.exp(s[:, d]) + ma[:, d]
    return y, s


def inverse(P, z, K, cap):
    for k in reversed(range(K)):
        z = invert_layer(P, k, z, cap)[0]
    return z


def nll_rows(P, x, u, cfg):
    """nll_r of pixel rows x under the noise u; cfg: dict(K, s_cap, alpha, levels)."""
    dtype = P["layers.0.linear.weight"].dtype
    y, ld0 = pre(x, u, cfg["alpha"], cfg["levels"], dtype)
    z, ld = forward(P, y, cfg["K"], cfg["s_cap"])
    return 0.5 * (z * z).sum(1) + nll_const(x.shape[1], cfg["levels"]) - ld0 - ld


def encode(P, x, u, cfg):
    y, ld0 = pre(x, u, cfg["alpha"], cfg["levels"])
    z, ld = forward(P, y, cfg["K"], cfg["s_cap"])
    return z, -(0.5 * (z * z).sum(1) + nll_const(x.shape[1], cfg["levels"]) - ld0 - ld)


def decode(P, z, cfg):
    return post(inverse(P, z, cfg["K"], cfg["s_cap"]), cfg["alpha"])


def params(P, dtype=torch.float64):
    return {n: (torch.nn.Parameter(v.to(dtype)) if v.is_floating_point() else v) for n, v in P.items()}


def loss_and_grads(P, x, u, cfg):
    P = params(f64(P))
    loss = nll_rows(P, x, u, cfg).sum() / x.shape[0]
    loss.backward()
    return loss.item(), {n: v.grad for n, v in P.items() if v.is_floating_point()}


def oracle_train(P, cfg, its, epochs, rows, noise, lr=1e-3, wd=0.0, steps0=0, dtype=torch.float64):
    """MAFTrainer's protocol in fp64 on the CPU: next(iter(test)) first, then per epoch a training pass (Adam on the mean
    NLL; batch i of the run under noise(TAG_TRAIN, steps0 + i, b)) and a validation pass (batch i under noise(TAG_EVAL,
    i, b)).  rows(x) -> the batch's rows as the device gathered them; noise(tag, step, b) -> u [b, D].  The weights enter
    as weight * mask, so masked gradients, moments and entries stay zero.  Returns (losses, validation losses per epoch,
    parameters, Adam's state).  dtype=torch.float32: the same arithmetic in fp32, the yardstick of an allowance (4 x its
    deviation from the fp64 run)."""
    P = params(f64(P), dtype)
    for k in range(cfg["K"]):                        # training starts from masked weights, whatever was passed
        M1, M2 = layer_masks(P, k, dtype)
        with torch.no_grad():
            P["layers.%d.linear.weight" % k].mul_(M1)
            P["layers.%d.out.weight" % k].mul_(M2)
    rows_, noise_ = rows, noise
    rows, noise = (lambda x: rows_(x).to(dtype)), (lambda tag, step, b: noise_(tag, step, b).to(dtype))
    next(iter(its[2]))
    train = [v for v in P.values() if v.is_floating_point()]
    opt = torch.optim.Adam(train, lr=lr, weight_decay=wd)
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
    state = {n: opt.state[v] for n, v in P.items() if v.is_floating_point()}
    return losses, vals, {n: v.detach() for n, v in P.items()}, state


def random_weights(D, H, K, order="natural", order_seed=0, seed=0, out_scale=0.5):
    """A state_dict (float32 weights, int32 degree buffers) with non-zero, masked out layers: the flow is not the
    identity."""
    g = torch.Generator().manual_seed(seed)
    ins, m_h = degrees(D, H, K, order, order_seed)
    sd = {}
    r = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    for k in range(K):
        M1, M2 = masks(ins[k], m_h)
        sd["layers.%d.m_in" % k] = torch.from_numpy(ins[k].astype(np.int32))
        sd["layers.%d.m_h" % k] = torch.from_numpy(m_h.astype(np.int32))
        sd["layers.%d.linear.weight" % k] = r(H, D) * (2.0 / D ** 0.5) * M1.float()
        sd["layers.%d.linear.bias" % k] = r(H) * 0.5
        sd["layers.%d.out.weight" % k] = r(2 * D, H) * (out_scale / H ** 0.5) * M2.float()
        sd["layers.%d.out.bias" % k] = r(2 * D) * 0.1
    return sd
