"""The beta-TCVAE's contract (generative_models_amd/tcvae.py's docstring) restated in plain torch on the CPU: the oracle
of tests/test_tcvae_cpu.py and tests/test_gpu_tcvae.py in float64, and -- the same code in float32 -- the yardstick of
their allowances.  Nothing here imports the package's TCVAE code; gradients come from autograd."""
import math

import numpy as np
import torch
import torch.nn.functional as F

KEYS = ("encoder.linear.weight", "encoder.linear.bias", "encoder.mu.weight", "encoder.mu.bias",
        "encoder.log_var.weight", "encoder.log_var.bias", "decoder.linear.weight", "decoder.linear.bias",
        "decoder.recon.weight", "decoder.recon.bias")
LOG_2PI = math.log(2.0 * math.pi)


def as_t(a, dtype, grad=False):
    t = torch.as_tensor(np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a), dtype=dtype).clone()
    return t.requires_grad_() if grad else t


def pair_l(z, mu, lv):
    """l [M, M, Z]: l[i, j, d] = log N(z_id; mu_jd, exp(lv_jd))."""
    d = z[:, None, :] - mu[None, :, :]
    return -0.5 * (LOG_2PI + lv[None] + d * d * torch.exp(-lv)[None])


def terms_from_l(l, z, log_nm):
    """(mi, tc, dwkl) [M] each from the pair densities l [M, M, Z] and the samples z."""
    M = l.shape[0]
    idx = torch.arange(M)
    lqzx = l[idx, idx].sum(1)
    lpz = (-0.5 * (LOG_2PI + z * z)).sum(1)
    lqz = torch.logsumexp(l.sum(2), 1) - log_nm
    lprod = (torch.logsumexp(l, 1) - log_nm).sum(1)
    return lqzx - lqz, lqz - lprod, lprod - lpz


def analytic_coefficients(l, alpha, beta, gamma):
    """The issue's closed form: the coefficient of l(i, j, d) in -lp_i."""
    a = torch.softmax(l.sum(2), 1)
    c = torch.softmax(l, 1)
    return (beta - alpha) * a[:, :, None] + (gamma - beta) * c + alpha * torch.eye(l.shape[0], dtype=l.dtype)[:, :, None]


def autograd_coefficients(z, mu, lv, alpha, beta, gamma, log_nm):
    """The same coefficients as d sum_i (-lp_i) / d l with l a leaf (row i of l enters lp_i alone)."""
    l = pair_l(z, mu, lv).detach().requires_grad_()
    mi, tc, dw = terms_from_l(l, z, log_nm)
    (alpha * mi + beta * tc + gamma * dw).sum().backward()
    return l.grad


def rows_reference(ml, eps, coef, log_nm, dtype=torch.float64, wn=None, dzdec=None):
    """The two row kernels' contract.  ml [B, 2Z], eps [B, Z], coef = (alpha, beta, gamma).  Returns z [B, Z], lp [B],
    terms [B, 3] = (mi, tc, dwkl), the records lse_joint [B] and lse_dim [B, Z] (without the -1/2 log 2 pi of every l),
    amax (the mean over rows of max_j a_ij); with wn [B] and dzdec [B, Z] also dml [B, 2Z], the gradient of
    sum_i (dzdec_i . z_i - wn_i lp_i): what the backward kernel sees."""
    alpha, beta, gamma = coef
    ml = as_t(ml, dtype, True)
    B, Z = ml.shape[0], ml.shape[1] // 2
    e = as_t(eps, dtype).view(B, Z)
    mu, lv = ml[:, :Z], ml[:, Z:]
    z = mu + e * torch.exp(lv / 2)
    l = pair_l(z, mu, lv)
    mi, tc, dw = terms_from_l(l, z, log_nm)
    lp = -(alpha * mi + beta * tc + gamma * dw)
    lprime = l + 0.5 * LOG_2PI
    out = {"z": z, "lp": lp, "terms": torch.stack([mi, tc, dw], 1), "lse_joint": torch.logsumexp(lprime.sum(2), 1),
           "lse_dim": torch.logsumexp(lprime, 1), "amax": torch.softmax(l.sum(2), 1).max(1).values.mean()}
    if wn is not None:
        ((as_t(dzdec, dtype) * z).sum() - (as_t(wn, dtype).reshape(-1) * lp).sum()).backward()
        out["dml"] = ml.grad
    return {n: v.detach().double().numpy() for n, v in out.items()}


def model_reference(P, x, eps, coef, N, dtype=torch.float64):
    """The whole contract on one batch of a dataset of N.  P: the ten tensors by state_dict name; x [B, I]; eps [B, Z].
    Returns loss, tc (the batch's mean), terms [B, 3], recon [B], z, lp and `grads`: d loss / d every tensor, by name."""
    alpha, beta, gamma = coef
    P = {n: as_t(P[n], dtype, True) for n in KEYS}
    x = as_t(x, dtype)
    B = x.shape[0]
    h = F.relu(x @ P["encoder.linear.weight"].T + P["encoder.linear.bias"])
    mu = h @ P["encoder.mu.weight"].T + P["encoder.mu.bias"]
    lv = h @ P["encoder.log_var.weight"].T + P["encoder.log_var.bias"]
    z = mu + as_t(eps, dtype).view(B, -1) * torch.exp(lv / 2)
    hd = F.relu(z @ P["decoder.linear.weight"].T + P["decoder.linear.bias"])
    xr = torch.sigmoid(hd @ P["decoder.recon.weight"].T + P["decoder.recon.bias"])
    mi, tc, dw = terms_from_l(pair_l(z, mu, lv), z, math.log(N * B))
    lp = -(alpha * mi + beta * tc + gamma * dw)
    recon = ((x - xr) ** 2).sum(1)
    loss = (recon - lp).sum()
    loss.backward()
    out = {"loss": loss, "tc": tc.mean(), "terms": torch.stack([mi, tc, dw], 1), "recon": recon, "z": z, "lp": lp}
    out = {n: v.detach().double().numpy() for n, v in out.items()}
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


def train_reference(P, batches, eps_of, coef, N, lr, weight_decay, dtype=torch.float64):
    """Training from P over `batches` (a list of x [b, I]) of a dataset of N; eps_of(t, b) -> eps [b, Z] of batch t.
    Returns (P after, losses, tc means, the first batch's gradients).  With dtype float32 the parameters and moments are
    rounded to float32 after every step, as a float32 trainer keeps them."""
    P = {n: np.asarray(as_t(P[n], torch.float64).numpy()) for n in KEYS}
    M = {n: np.zeros_like(v) for n, v in P.items()}
    V = {n: np.zeros_like(v) for n, v in P.items()}
    losses, tcs, g0 = [], [], None
    for t, x in enumerate(batches):
        r = model_reference(P, x, eps_of(t, x.shape[0]), coef, N, dtype)
        losses.append(float(r["loss"]))
        tcs.append(float(r["tc"]))
        g0 = r["grads"] if g0 is None else g0
        P, M, V = adam_reference(P, r["grads"], M, V, t + 1, lr, weight_decay)
        if dtype == torch.float32:
            P, M, V = ({n: v.astype(np.float32).astype(np.float64) for n, v in d.items()} for d in (P, M, V))
    return P, losses, tcs, g0
