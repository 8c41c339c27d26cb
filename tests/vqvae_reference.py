"""The VQ-VAE's contract (generative_models_amd/vqvae.py's docstring) restated in torch: float64 by default, a dtype argument
for the float32 yardstick.  Written from the contract and the paper (van den Oord, Vinyals & Kavukcuoglu, arXiv
1711.00937), not from the kernels: autograd on the stop-gradient loss gives the model's gradients, the closed forms (dml,
dE) are stated separately in `rows_reference` and tests/test_vqvae_cpu.py checks one against the other.  Every function
takes `codes=` to be evaluated on given choices (the device's own) instead of its own arg min."""
import math

import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("encoder.linear.weight", "encoder.linear.bias", "encoder.embed.weight", "encoder.embed.bias", "codebook.weight",
        "decoder.linear.weight", "decoder.linear.bias", "decoder.recon.weight", "decoder.recon.bias")


def as_t(a, dtype=torch.float64, grad=False):
    t = torch.as_tensor(np.asarray(a, dtype=np.float64)).to(dtype)
    return t.requires_grad_(True) if grad else t


def _np(v):
    if torch.is_tensor(v):
        v = v.detach()
        return v.double().numpy() if v.is_floating_point() else v.numpy()
    return v


def distances(ze, E, N):
    """[rows, N, K]: the direct squared distances sum_d (z_e,n,d - E_k,d)^2."""
    z = ze.view(ze.shape[0], N, 1, -1)
    return ((z - E[None, None]) ** 2).sum(-1)


def choose(ze, E, N, codes=None):
    """(codes [rows, N] int64 -- the arg min, the lowest index on a tie, or the given ones -- and gap [rows, N], the
    difference between the second-smallest and the smallest squared distance)."""
    d = distances(ze.detach(), E.detach(), N)
    two = torch.topk(d, 2, -1, largest=False).values
    arg = d.argmin(-1)                                             # torch returns the first minimum on the CPU
    if codes is not None:
        arg = torch.as_tensor(np.asarray(codes)).long().view(arg.shape)
    return arg, two[..., 1] - two[..., 0]


def rows_reference(ze, E, N, beta, dtype=torch.float64, dzdec=None, wn=None, codes=None):
    """The row-level contract.  ze [B, N D]; E [K, D].  Returns codes, gap [B, N], zq [B, N D], qerr, lp [B], n_k [K]
    (int64), s_k [K, D], dE [K, D] = 2 (n_k E_k - s_k) and, with dzdec [B, N D] (wn [B], default 1), dml [B, N D] = dzdec
    + 2 beta wn (ze - E_c)."""
    ze, E = as_t(ze, dtype), as_t(E, dtype)
    B, (K, D) = ze.shape[0], E.shape
    c, gap = choose(ze, E, N, codes)
    zq = E[c].reshape(B, N * D)
    qerr = ((ze - zq) ** 2).view(B, N, D).sum(-1).sum(-1)
    nk = torch.bincount(c.reshape(-1), minlength=K)
    sk = torch.zeros(K, D, dtype=dtype).index_add_(0, c.reshape(-1), ze.view(B * N, D))
    out = {"codes": c, "gap": gap, "zq": zq, "qerr": qerr, "lp": -(1.0 + beta) * qerr, "n_k": nk, "s_k": sk,
           "dE": 2.0 * (nk.to(dtype)[:, None] * E - sk)}
    if dzdec is not None:
        w = torch.ones(B, dtype=dtype) if wn is None else as_t(wn, dtype).reshape(-1)
        out["dml"] = as_t(dzdec, dtype) + 2.0 * beta * w[:, None] * (ze - zq)
    return {n: _np(v) for n, v in out.items()}


def stopgrad_gradients(ze, E, N, beta, dzdec, dtype=torch.float64, codes=None):
    """(d / d ze, d / d E) by autograd of sum(dzdec * (ze + sg[zq - ze])) + ||sg[ze] - E_c||^2 + beta ||ze - sg[E_c]||^2:
    the loss's dependence on ze and E with the decoder's input gradient given."""
    ze, E = as_t(ze, dtype, True), as_t(E, dtype, True)
    B, D = ze.shape[0], E.shape[1]
    c, _ = choose(ze, E, N, codes)
    zq = E[c].reshape(B, N * D)
    zin = ze + (zq - ze).detach()
    ((as_t(dzdec, dtype) * zin).sum() + ((ze.detach() - zq) ** 2).sum() + beta * ((ze - zq.detach()) ** 2).sum()).backward()
    return _np(ze.grad), _np(E.grad)


# ---- the model ---------------------------------------------------------------------------------------------------------
def _encode(P, x):
    h = F.relu(x @ P["encoder.linear.weight"].T + P["encoder.linear.bias"])
    return h @ P["encoder.embed.weight"].T + P["encoder.embed.bias"]


def _decode(P, z):
    hd = F.relu(z @ P["decoder.linear.weight"].T + P["decoder.linear.bias"])
    return torch.sigmoid(hd @ P["decoder.recon.weight"].T + P["decoder.recon.bias"])


def model_reference(P, x, N, beta, dtype=torch.float64, codes=None, grads=True):
    """One batch.  P: the 9 tensors by state_dict name; x [B, I].  Returns loss (= sum_b -log w = sum_b ||x - decoder(
    z_q)||^2 + (1 + beta) qerr), vq (= sum_b qerr), codes, min_gap, gap [B, N] and `grads` by autograd through the
    straight-through estimator and the two stop-gradient terms."""
    P = {n: as_t(P[n], dtype, grads) for n in KEYS}
    x = as_t(x, dtype)
    B = x.shape[0]
    ze, E = _encode(P, x), P["codebook.weight"]
    D = E.shape[1]
    c, gap = choose(ze, E, N, codes)
    zq = E[c].reshape(B, N * D)
    cb, cm = ((ze.detach() - zq) ** 2).sum(), ((ze - zq.detach()) ** 2).sum()
    loss = ((x - _decode(P, ze + (zq - ze).detach())) ** 2).sum() + cb + beta * cm
    out = {"loss": loss.item(), "vq": cb.item(), "codes": c.numpy(), "gap": gap.numpy(), "min_gap": float(gap.min())}
    if grads:
        loss.backward()
        out["grads"] = {n: v.grad.double().numpy() for n, v in P.items()}
    return out


def adam_reference(P, G, M, V, step, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8):
    """One torch.optim.Adam step (L2 weight decay folded into the gradient) in float64: (P', M', V')."""
    out = ({}, {}, {})
    for n in P:
        g = np.asarray(G[n], np.float64) + weight_decay * np.asarray(P[n], np.float64)
        m = betas[0] * np.asarray(M[n], np.float64) + (1 - betas[0]) * g
        v = betas[1] * np.asarray(V[n], np.float64) + (1 - betas[1]) * g * g
        den = np.sqrt(v) / math.sqrt(1 - betas[1] ** step) + eps
        out[0][n] = np.asarray(P[n], np.float64) - lr / (1 - betas[0] ** step) * m / den
        out[1][n], out[2][n] = m, v
    return out


def train_reference(P, batches, N, beta, lr, weight_decay, dtype=torch.float64, codes=None):
    """Training from P over `batches` (a list of x [b, I]) with Adam; codes: None or a list of the choices to evaluate each
    batch on.  Returns (P after every batch -- a list --, losses, vq sums, the smallest gap met).  With dtype float32 the
    parameters and moments are rounded to float32 after every step, as a float32 trainer keeps them."""
    P = {n: np.asarray(as_t(P[n], torch.float64).numpy()) for n in KEYS}
    M = {n: np.zeros_like(v) for n, v in P.items()}
    V = {n: np.zeros_like(v) for n, v in P.items()}
    trail, losses, vqs, gap = [], [], [], math.inf
    for t, x in enumerate(batches):
        r = model_reference(P, x, N, beta, dtype, codes=None if codes is None else codes[t])
        losses.append(r["loss"])
        vqs.append(r["vq"])
        gap = min(gap, r["min_gap"])
        P, M, V = adam_reference(P, r["grads"], M, V, t + 1, lr, weight_decay)
        if dtype == torch.float32:
            P, M, V = ({n: v.astype(np.float32).astype(np.float64) for n, v in d.items()} for d in (P, M, V))
        trail.append(dict(P))
    return trail, losses, vqs, gap
