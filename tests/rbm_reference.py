"""rbm.py's contract restated in numpy (CPU), independently of the code under test: the noise rule through
dvae.philox4x32_10, the Gibbs chain in fp64 and in fp32 with the pinned sum order, the free energy, the CD gradient,
annealed importance sampling and the exact partition function of a small RBM.  Imported by tests/test_rbm_cpu.py and
tests/test_gpu_rbm.py; it is the reference of every comparison there.

Conventions (made_reference's): a draw is undecided when |u - p64| <= UNDECIDED; a chain row is undecided from its first
such draw on, and nothing is asserted about it afterwards."""
import numpy as np

from generative_models_amd.dvae import philox4x32_10
from made_reference import GRAD_TOL, LOSS_TOL, PARAM_TOL, STEP_TOL, UNDECIDED  # noqa: F401

TAG_D, TAG_H, TAG_V = 0x52424D44, 0x52424D48, 0x52424D56      # "RBMD", "RBMH", "RBMV"
_M32 = 0xFFFFFFFF
F32 = np.float32

# Tolerance of a device AIS log-weight against the fp64 restatement on the same uniforms (decided rows): four times
# the largest deviation of `chain(..., dtype=float32)` (this file's fp32 restatement with the pinned sum order) from
# `chain(..., dtype=float64)` over the decided rows of both AIS_CASES, measured by tests/test_rbm_cpu.py
# ::test_fp32_ais_restatement_deviation, which prints the figures (9.4e-6 at 12x5, 2.24e-5 at 20x8) and asserts they have not grown.
AIS_RESTATEMENT_DEV = 2.3e-5
AIS_LOGW_TOL = 4 * AIS_RESTATEMENT_DEV


def uniforms(n, width, seed, tag, t=0, row0=0):
    """u [n, width] float32 by the contract's rule, one Philox call per (row, unit)."""
    key = np.array([seed & _M32, (seed >> 32) & _M32], dtype=np.uint64)
    e = np.arange(width, dtype=np.uint64)
    ctr = np.zeros((n, width, 4), dtype=np.uint64)
    ctr[..., 0] = (e >> np.uint64(2))[None, :]
    ctr[..., 1] = np.uint64(t & _M32)
    ctr[..., 2] = ((np.arange(n, dtype=np.uint64) + np.uint64(row0)) & np.uint64(_M32))[:, None]
    ctr[..., 3] = np.uint64(tag)
    w = philox4x32_10(ctr, key)
    word = np.take_along_axis(w, (e & np.uint64(3)).astype(np.int64)[None, :, None].repeat(n, 0), axis=2)[..., 0]
    v = 2 * (word.astype(np.uint64) >> np.uint64(9)) + 1        # < 2^24: exact in fp32
    return v.astype(np.float32) * np.float32(2.0 ** -24)


def softplus(a):
    """max(a, 0) + log1p(exp(-|a|)) in a's own precision."""
    return np.maximum(a, 0) + np.log1p(np.exp(-np.abs(a)))


def sigmoid(a):
    """1 / (1 + exp(-a)) in a's own precision (the pinned form)."""
    one = a.dtype.type(1)
    with np.errstate(over="ignore"):
        return one / (one + np.exp(-a))


def _pinned_sum(bias, M, lit, dtype):
    """bias + the rows of M selected by lit [n, rows] (bool), added in ascending row order, one accumulator per unit."""
    acc = np.repeat(bias[None, :].astype(dtype), lit.shape[0], 0)
    for i in range(M.shape[0]):
        sel = lit[:, i]
        if sel.any():
            acc[sel] = acc[sel] + M[i].astype(dtype)[None, :]
    return acc


def chain(W, c, b, x, steps, seed, row0=0, dstep=0, g0=0, betas=None, b_A=None, dtype=np.float64):
    """The chain of the contract on the rule's uniforms.  W [H, I], c [H], b [I] float32; x [n, I] float32 in [0, 1].
    dtype float64: the reference;  float32: the restatement with the pinned sum order and the pinned rounding of every
    tempered term.  Returns a dict: v0, v, h (bool), p, a (the last visible draw's conditionals and logits, dtype),
    logw (float64 [n], tempered chains), und (bool [n]: rows with an undecided draw, judged on THIS run's
    probabilities in fp64)."""
    n, I = x.shape
    H = W.shape[0]
    T = dtype
    WT = np.ascontiguousarray(W.T)
    v = uniforms(n, I, seed, TAG_D, dstep, row0) < x.astype(np.float32)
    out = dict(v0=v.copy(), und=np.zeros(n, bool), logw=np.zeros(n, np.float64), p=None, a=None,
               h=np.zeros((n, H), bool))
    bd = (b.astype(T) - b_A.astype(T)) if betas is not None else None
    for s in range(steps):
        t = g0 + s
        pre_h = _pinned_sum(c, WT, v, T)
        if betas is not None:
            bp, bc = T(betas[s]), T(betas[s + 1])
            bv = np.where(v, bd[None, :], T(0)).astype(T).sum(1, dtype=T)
            sps = (softplus((bc * pre_h).astype(T)) - softplus((bp * pre_h).astype(T))).astype(T).sum(1, dtype=T)
            out["logw"] += (((bc - bp) * bv).astype(T) + sps).astype(np.float64)
            a_h = (bc * pre_h).astype(T)
        else:
            a_h = pre_h
        p_h = sigmoid(a_h)
        u = uniforms(n, H, seed, TAG_H, t, row0)
        out["und"] |= (np.abs(u.astype(np.float64) - p_h.astype(np.float64)) <= UNDECIDED).any(1)
        h = u < p_h.astype(np.float32) if T is np.float32 else u.astype(np.float64) < p_h
        pre_v = _pinned_sum(b, W, h, T)
        if betas is not None:
            a_v = ((bc * pre_v).astype(T) + ((T(1) - bc) * b_A.astype(T)[None, :]).astype(T)).astype(T)
        else:
            a_v = pre_v
        p_v = sigmoid(a_v)
        u = uniforms(n, I, seed, TAG_V, t, row0)
        out["und"] |= (np.abs(u.astype(np.float64) - p_v.astype(np.float64)) <= UNDECIDED).any(1)
        v = u < p_v.astype(np.float32) if T is np.float32 else u.astype(np.float64) < p_v
        out.update(h=h, p=p_v, a=a_v)
    out["v"] = v
    return out


def free_energy(W, c, b, v):
    """F(v) = -b.v - sum_j softplus(c_j + W_j.v), fp64 [n]."""
    W, c, b, v = (np.asarray(t, np.float64) for t in (W, c, b, v))
    return -(v @ b) - softplus(v @ W.T + c[None, :]).sum(1)


def cd_grads(W, c, b, v0, vk):
    """(loss, dW, dc, db) of loss = mean_b [F(v0_b) - F(vk_b)] in fp64, v0 and vk constant: the CD / PCD update."""
    W, c, b, v0, vk = (np.asarray(t, np.float64) for t in (W, c, b, v0, vk))
    B = v0.shape[0]
    p0, pk = sigmoid(v0 @ W.T + c[None, :]), sigmoid(vk @ W.T + c[None, :])
    loss = (free_energy(W, c, b, v0) - free_energy(W, c, b, vk)).mean()
    return loss, (pk.T @ vk - p0.T @ v0) / B, (pk - p0).sum(0) / B, (vk - v0).sum(0) / B


def adam_step(P, G, M, V, step, lr, wd=0.0, b1=0.9, b2=0.999, eps=1e-8):
    """One Adam step in fp64 on dicts of arrays, in place (torch's _single_tensor_adam)."""
    for n in P:
        g = G[n] + wd * P[n]
        M[n] += (1 - b1) * (g - M[n])
        V[n] = V[n] * b2 + (1 - b2) * g * g
        denom = np.sqrt(V[n]) / np.sqrt(1 - b2 ** step) + eps
        P[n] += -(lr / (1 - b1 ** step)) * M[n] / denom


def base_rate(pixel_means_or_data, n=None):
    """b_A = logit of the Laplace-smoothed pixel means: (sum + 1) / (n + 2) of the binarised training rows."""
    x = np.asarray(pixel_means_or_data, np.float64)
    m = (x.sum(0) + 1.0) / (x.shape[0] + 2.0)
    return np.log(m) - np.log1p(-m)


def log_z_base(b_A, H):
    return H * np.log(2.0) + softplus(np.asarray(b_A, np.float64)).sum()


def log_mean_exp(lw):
    lw = np.asarray(lw, np.float64)
    m = lw.max()
    return m + np.log(np.mean(np.exp(lw - m)))


def ais_log_z(logw, b_A, H):
    """(log Z, its standard error by the delta method) from the chains' log-weights."""
    lw = np.asarray(logw, np.float64)
    w = np.exp(lw - lw.max())
    se = w.std() / (w.mean() * np.sqrt(lw.size))
    return log_mean_exp(lw) + log_z_base(b_A, H), se


def exact_log_z(W, c, b):
    """log Z by enumerating the 2^H hidden states: log sum_h exp(c.h + sum_i softplus(b_i + (W^T h)_i))."""
    W, c, b = (np.asarray(t, np.float64) for t in (W, c, b))
    H = W.shape[0]
    hs = ((np.arange(1 << H)[:, None] >> np.arange(H)[None, :]) & 1).astype(np.float64)
    t = hs @ c + softplus(hs @ W + b[None, :]).sum(1)
    m = t.max()
    return m + np.log(np.exp(t - m).sum())


def uniform_betas(n):
    return np.linspace(0.0, 1.0, n).astype(np.float32)


def case_weights(I, H, seed, scale=None):
    """Random float32 weights: W ~ scale N(0, 1) (default 4 / sqrt(max(I, H)): logits of a few units), c, b ~ 0.5 N."""
    g = np.random.RandomState(seed)
    scale = 4.0 / np.sqrt(max(I, H)) if scale is None else scale
    W = (g.standard_normal((H, I)) * scale).astype(np.float32)
    return W, (g.standard_normal(H) * 0.5).astype(np.float32), (g.standard_normal(I) * 0.5).astype(np.float32)


def case_input(n, I, seed):
    """Grey levels in [0, 1] with exact zeros and ones among them."""
    g = np.random.RandomState(seed + 1000)
    x = g.random_sample((n, I)).astype(np.float32)
    x[g.random_sample((n, I)) < 0.2] = 0.0
    x[g.random_sample((n, I)) < 0.2] = 1.0
    return x


# (n, I, H, steps, seed): the seeds are chosen so that the small cases have no undecided row in the fp64 reference
# (tests/test_rbm_cpu.py::test_chain_cases_are_decided asserts it); at 784-400 at most UNDECIDED_SHARE of the rows.
CHAIN_CASES = {"5x49x32": (5, 49, 32, 3, 26), "9x70x70": (9, 70, 70, 3, 22), "8x784x400": (8, 784, 400, 2, 23),
               "3x1024x1024": (3, 1024, 1024, 1, 24), "4x1x1": (4, 1, 1, 2, 25)}
UNDECIDED_SHARE = {"8x784x400": 0.05}
GRAD_CASES = [(5, 49, 32), (64, 784, 400)]
TRANSPOSE_CASES = [(49, 32), (70, 70), (784, 400)]
# (I, H, weight seed, chain seed): random weights of scale about 1, 256 chains, 500 betas
AIS_CASES = {"12x5": (12, 5, 31, 43), "20x8": (20, 8, 32, 43)}
AIS_CHAINS, AIS_BETAS = 256, 500


def ais_case(name):
    I, H, wseed, seed = AIS_CASES[name]
    W, c, b = case_weights(I, H, wseed, scale=1.0)
    g = np.random.RandomState(wseed + 7)
    data = (g.random_sample((200, I)) < g.random_sample(I)[None, :]).astype(np.float32)
    b_A = base_rate(data).astype(np.float32)
    return W, c, b, b_A, seed
