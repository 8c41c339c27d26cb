"""ddpm.py's contract restated in numpy / plain torch fp64 (CPU): the denoiser's forward, L_simple and its gradients, one
sampler step, Ho et al.'s posterior in its own parametrisation, the bound a device row is held to against the numpy
rule, and a whole training loop that replays the trainer's RNG protocol.  Imported by tests/test_ddpm_cpu.py and
tests/test_gpu_ddpm.py."""
import numpy as np
import torch
import torch.nn.functional as F

from generative_models_amd import ddpm as gddpm

# the project's bounds: device normals (tests/test_gpu_dvae.py close_rule), gradients, losses, weights, one sampler step
NORMAL_TOL, GRAD_TOL, LOSS_TOL, PARAM_TOL, STEP_TOL = 4e-6, 1.5e-6, 1e-5, 5e-5, 1e-5
NAMES = ("denoiser.linear.weight", "denoiser.linear.bias", "denoiser.hidden.weight", "denoiser.hidden.bias",
         "denoiser.out.weight", "denoiser.out.bias")


def f64(P):
    return {n: (v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(v)).double().clone() for n, v in P.items()}


def forward(P, xin):
    """eps_theta of the input rows xin = [x_t | temb[t]] (fp64 tensors)."""
    h1 = F.relu(xin @ P[NAMES[0]].T + P[NAMES[1]])
    h2 = F.relu(h1 @ P[NAMES[2]].T + P[NAMES[3]])
    return h2 @ P[NAMES[4]].T + P[NAMES[5]]


def l_simple(out, eps):
    """sum (eps - out)^2 / (b I)."""
    return torch.sum((eps - out) ** 2) / (out.shape[0] * out.shape[1])


def loss_and_grads(P, xin, eps):
    """(loss, d loss / d every tensor, d loss / d out) by fp64 autograd."""
    P = {n: v.clone().requires_grad_() for n, v in f64(P).items()}
    out = forward(P, xin.double())
    out.retain_grad()
    loss = l_simple(out, eps.double())
    loss.backward()
    return loss.item(), {n: v.grad for n, v in P.items()}, out.grad


def reverse_step(xt, eps, z, row, clip):
    """One sampler step in fp64 numpy with the coefficient row (s1_t, sa_t, sa_prev, dir, sigma, ...)."""
    s1, sa, sap, dr, sig = (float(v) for v in row[:5])
    x0 = (xt - s1 * eps) / sa
    if clip:
        x0 = np.clip(x0, -1.0, 1.0)
    ep = (xt - sa * x0) / s1
    return sap * x0 + dr * ep + sig * z


def posterior(T, t):
    """Ho et al. eq. 6 and 7 at timestep t >= 1: (coefficient of x0, coefficient of x_t, variance beta~_t)."""
    tab = gddpm.tables(T, 4)
    beta, ab = tab["beta"], tab["ab"]
    abp = ab[t - 1]
    return (np.sqrt(abp) * beta[t] / (1 - ab[t]), np.sqrt(1 - beta[t]) * (1 - abp) / (1 - ab[t]),
            (1 - abp) / (1 - ab[t]) * beta[t])


def close_rule(xin, eps, t, x, T, E, seed, step, train=True, row0=0):
    """A q-sample's device rows (numpy: xin [n, >= I + E], eps [n, I], t [n]) against the numpy rule: t and the temb
    tail bit for bit, eps within 4e-6 of the normal's scale, x_t within 4e-6 of its own scale plus s1_t times the
    normal's (the DVAE's gaussian bound with sigma = s1_t)."""
    n, I = x.shape
    rt, reps, rxt, rtemb = gddpm.qsample_reference(x, T, E, seed, step, train, row0)
    assert np.array_equal(np.asarray(t, np.int64), rt), (seed, step, train)
    assert xin[:, I:I + E].astype(np.float32).tobytes() == rtemb.tobytes()
    nscale = np.maximum(1.0, np.abs(reps))
    err = np.abs(eps.astype(np.float64) - reps)
    assert np.all(err <= NORMAL_TOL * nscale), float((err / nscale).max())
    s1 = gddpm.tables(T, E)["s1"].astype(np.float32).astype(np.float64)[rt][:, None]
    tol = NORMAL_TOL * (np.maximum(1.0, np.abs(rxt)) + s1 * nscale)
    err = np.abs(xin[:, :I].astype(np.float64) - rxt)
    assert np.all(err <= tol), float((err / tol).max())


def oracle_train(P, its, epochs, device_rows, lr=2e-4, wd=0.0):
    """DDPMTrainer's protocol in fp64 on the CPU: next(iter(test)) first, then per epoch a training pass (Adam on
    L_simple) and a validation pass.  device_rows(x, step, train) -> (xin, eps) float64 CPU tensors: the device's
    q-sample of the batch, which the caller has checked against the numpy rule (close_rule).  The oracle takes the
    device's rows because the rule's fp64 normals and the device's fp32 ones differ in the last bits, and Adam's first
    step (m / sqrt(v) = sign(g)) turns a last-bit change of a near-zero gradient into a whole lr step of that weight.
    Returns (losses, best_val_loss, parameters)."""
    P = {n: torch.nn.Parameter(v) for n, v in f64(P).items()}
    next(iter(its[2]))
    opt = torch.optim.Adam(list(P.values()), lr=lr, weight_decay=wd)
    losses, best, step = [], 1e10, 0
    for _ in range(epochs):
        for x, _y in its[0]:
            xin, eps = device_rows(x.view(x.shape[0], -1), step, True)
            step += 1
            opt.zero_grad()
            loss = l_simple(forward(P, xin), eps)
            loss.backward()
            opt.step()
            losses.append(loss.item())
        vals = []
        with torch.no_grad():
            for i, (x, _y) in enumerate(its[1]):
                xin, eps = device_rows(x.view(x.shape[0], -1), i, False)
                vals.append(l_simple(forward(P, xin), eps).item())
        best = min(best, float(np.mean(vals)))
    return losses, best, {n: v.detach() for n, v in P.items()}
