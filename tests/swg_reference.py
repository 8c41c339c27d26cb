"""The sliced Wasserstein loss of generative_models_amd/swg.py in numpy / torch, for the tests: the contract's overlap
form over given projection arrays (`sw_reference`), the replicate-and-sort form it is checked against (`sw_loops`), fp64
autograd (`autograd_dX`), the directions through philox.normals, and the generator's backward from given coefficients.

A sort is discontinuous: every comparison of ranks and coefficients with the device is made on the device's own
projection bits, handed to `sw_reference` as they were read back."""
import numpy as np
import torch

from generative_models_amd import philox

KEYS = ("G.linear.weight", "G.linear.bias", "G.generate.weight", "G.generate.bias")


def segments(N, M):
    """The overlaps of the masses [i M, (i + 1) M) and [j N, (j + 1) N) of N M: (i, j, w_ij) of every pair with
    w_ij > 0, in ascending order (at most N + M - 1 of them)."""
    cuts = np.unique(np.concatenate([np.arange(N + 1, dtype=np.int64) * M, np.arange(M + 1, dtype=np.int64) * N]))
    lo = cuts[:-1]
    return lo // M, lo // N, np.diff(cuts)


def _by_rank(i, terms, N):
    """[P, N]: per projection, the sum of terms [P, n_segments] over the segments of each rank i, in ascending j and in
    the terms' own dtype."""
    out = np.zeros((terms.shape[0], N), terms.dtype)
    for p in range(terms.shape[0]):
        np.add.at(out[p], i, terms[p])
    return out


def sw_reference(a, b, dtype=np.float64):
    """a [P, N], b [P, M] (the projections, as given) -> the stable-order ranks, W_p, and the loss's gradient with
    respect to a at the rows' original positions.  dtype float32: the differences, products and sums in float32."""
    a, b = np.atleast_2d(np.asarray(a)), np.atleast_2d(np.asarray(b))
    P, N, M = a.shape[0], a.shape[1], b.shape[1]
    oa, ob = np.argsort(a, axis=1, kind="stable"), np.argsort(b, axis=1, kind="stable")
    sa = np.take_along_axis(a, oa, 1).astype(dtype)
    sb = np.take_along_axis(b, ob, 1).astype(dtype)
    i, j, w = segments(N, M)
    w = w.astype(dtype)
    d = sa[:, i] - sb[:, j]
    ws = (w * (d * d)).sum(1, dtype=dtype)
    Ct = np.zeros((P, N), dtype)
    np.put_along_axis(Ct, oa, (dtype(2.0) / dtype(P * N * M)) * _by_rank(i, w * d, N), 1)
    rank = np.empty_like(oa)
    np.put_along_axis(rank, oa, np.broadcast_to(np.arange(N), oa.shape), 1)
    return {"order_a": oa, "order_b": ob, "rank_a": rank, "sorted_a": sa, "sorted_b": sb, "ws": ws, "Ct": Ct,
            "W": ws / dtype(N * M), "swd2": float(ws.astype(np.float64).sum() / (float(P) * N * M))}


def sw_diagnostics(ref):
    """What a test needs beside the reference `ref` (an fp64 sw_reference result) to read a device's Ct: `B` [P, N],
    B_r = sum_j w_rj b_(j), so that M a_i - B_r is rank r's coefficient for row i before the scale; and `Ct_abs`, the
    coefficient with |a_(i) - b_(j)| for the differences, at the rows' original positions: the scale of the fp32
    rounding of its subtractions."""
    sa, sb, oa = ref["sorted_a"], ref["sorted_b"], ref["order_a"]
    P, N, M = sa.shape[0], sa.shape[1], sb.shape[1]
    i, j, w = segments(N, M)
    w = w.astype(np.float64)
    Ca = np.zeros((P, N))
    np.put_along_axis(Ca, oa, 2.0 / (float(P) * N * M) * _by_rank(i, w * np.abs(sa[:, i] - sb[:, j]), N), 1)
    return {"B": _by_rank(i, w * sb[:, j], N), "Ct_abs": Ca}


def sw_loops(a, b):
    """W of two samples on the line by sorting both replicated to N M points (a to M copies of each, b to N)."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    ra, rb = np.sort(np.repeat(a, len(b))), np.sort(np.repeat(b, len(a)))
    return float(np.mean((ra - rb) ** 2))


def sw_torch(X, Y, Theta):
    """swd2 of rows X, Y over directions Theta as a differentiable torch scalar (the overlap form; sort's backward)."""
    N, M, P = X.shape[0], Y.shape[0], Theta.shape[0]
    i, j, w = segments(N, M)
    sa, sb = torch.sort(Theta @ X.T, dim=1)[0], torch.sort(Theta @ Y.T, dim=1)[0]
    d = sa[:, torch.as_tensor(i)] - sb[:, torch.as_tensor(j)]
    return (torch.as_tensor(w, dtype=X.dtype) * d * d).sum() / (float(P) * N * M)


def autograd_dX(X, Y, Theta):
    """(swd2, d swd2 / d X) by fp64 autograd."""
    X = torch.as_tensor(np.asarray(X), dtype=torch.float64).clone().requires_grad_(True)
    Y, Theta = (torch.as_tensor(np.asarray(v), dtype=torch.float64) for v in (Y, Theta))
    loss = sw_torch(X, Y, Theta)
    loss.backward()
    return float(loss.detach()), X.grad.numpy()


def directions_reference(P, I, seed, step, tag, row0=0, dtype=np.float64):
    """The unit directions [P, I]: philox.normals over the row's 2-norm (float32: the normals and the scaling rounded
    to float32, the norm's sum in fp64 as on the device)."""
    n = philox.normals(P, I, seed, step, tag, row0).astype(dtype)
    norm = np.sqrt((n.astype(np.float64) ** 2).sum(1, keepdims=True))
    safe = np.where(norm > 0, norm, 1.0)
    if dtype == np.float64:
        return np.where(norm > 0, n / safe, 0.0)
    return n * np.where(norm > 0, 1.0 / safe, 0.0).astype(dtype)


def _t(x, dtype):
    return torch.as_tensor(np.asarray(x)).to(dtype)


def generator(W, z, dtype=torch.float64):
    """(H, X) of the two-layer generator with weights W (state-dict names -> arrays) on the prior rows z."""
    w = {k: _t(W[k], dtype) for k in KEYS}
    z = _t(z, dtype)
    H = torch.relu(z @ w["G.linear.weight"].T + w["G.linear.bias"])
    return H, torch.sigmoid(H @ w["G.generate.weight"].T + w["G.generate.bias"])


def backward(W, z, Ct, Theta, dtype=torch.float64):
    """dX = Ct^T Theta, dA = dX x (1 - x) and the four weight gradients of the generator at weights W from given
    coefficients Ct [P, N]."""
    w = {k: _t(W[k], dtype) for k in KEYS}
    z = _t(z, dtype)
    H, X = generator(W, z, dtype)
    dX = _t(Ct, dtype).T @ _t(Theta, dtype)
    dA = dX * X * (1 - X)
    dH = (dA @ w["G.generate.weight"]) * (H > 0).to(dtype)
    grads = {"G.generate.weight": dA.T @ H, "G.generate.bias": dA.sum(0), "G.linear.weight": dH.T @ z,
             "G.linear.bias": dH.sum(0)}
    return {"X": X.numpy(), "dX": dX.numpy(), "dA": dA.numpy(), "grads": {k: v.numpy() for k, v in grads.items()}}


def adam_step(W, grads, m, v, t, lr, weight_decay=0.0, dtype=torch.float64):
    """One Adam step (torch's defaults, L2 weight decay) at 0-based step t; m and v are updated in place."""
    out = {}
    for k in KEYS:
        p = _t(W[k], dtype)
        g = _t(grads[k], dtype) + weight_decay * p
        m[k] = 0.9 * m[k] + 0.1 * g
        v[k] = 0.999 * v[k] + 0.001 * g * g
        mh, vh = m[k] / (1 - 0.9 ** (t + 1)), v[k] / (1 - 0.999 ** (t + 1))
        out[k] = (p - lr * mh / (vh.sqrt() + 1e-8)).double().numpy()
    return out
