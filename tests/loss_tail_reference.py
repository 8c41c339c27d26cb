"""One staged fp64 reference for the critic tail (test infrastructure; no GPU).

The tail is  h -> a2 = h . w2 + b2 -> s = act(a2) -> loss(s) , with its backward down to (gw2, gb2, dH) and, for the
folded steps, through the hidden layer (gW1, gb1, dX).  csrc/gm_common.h (`sample_terms`), gm_ops.hip (`gan_loss_kernel`),
gm_fused.hip (`head_fwd_loss_kernel`) and gm_head.h (`fold_row`, `fold_fill_lds_tp`, `head_bwd_body`) each evaluate it.

A plain fp64 autograd run is NOT a reference for it once scores saturate: fp64 keeps 1 - s ~ 2e-9 where fp32 has exactly
0, so log(1 - s + eps) and its derivative differ by 1e-3 / 17 % from what the reference project computes.  The
specification is the reference project's fp32 arithmetic, in which every stage reads the fp32-ROUNDED result of the stage
before it.  So the reference is staged, and each stage is fp64 arithmetic on fp32-rounded inputs:

  1. a2 = h . w2 + b2 in fp64 (for the folded steps h = fl32(relu(X W1^T + b1)) first), s = fl32(act(a2));
  2. per-row loss term and dL/ds in fp64 at that s, in the expression order of oracle/port.py's loss lines
     (d_loss, g_loss, f_div_D, f_div_G): the operations fp32 does EXACTLY but with a rounding that matters --
     (1 - s), (s + eps), (sg - 1), mean(sg) of RaGAN, Fisher's moments -- are rounded to fp32 (`_r`), eps = float32(1e-8);
  3. dS = dL/ds * act'(s) with torch's backward formulas at the rounded s (sigmoid: grad * (1 - y) * y; relu: y > 0);
  4. dH = dS (x) w2 . [h > 0], gw2 = dS^T h, gb2 = fl32(sum over x rows) + fl32(sum over g rows), and through layer 1.

`tail()` returns that staged result AND the fp32 torch-CPU autograd result of the same tail (what the older op tests
compare with), so that the `close64` criterion of tests/linear_path_cases.py applies: HIP error against the staged value
<= 2 x fp32-CPU error + 1 ulp.  tests/test_loss_tail_cpu.py pins the loss expressions against oracle/port.py's own."""
import numpy as np
import torch

EPS32 = float(np.float32(1e-8))               # torch adds the Python scalar 1e-8 to an fp32 tensor as float32(1e-8)
F_KEYS = ("f_total_variation", "f_forward_kl", "f_reverse_kl", "f_pearson", "f_hellinger", "f_jensen_shannon")
KEYS = ("ns", "mm", "w", "ls", "ra", "fisher") + F_KEYS
TWO_PHASE = ("ra", "fisher")                   # critic losses that are not a mean of per-row terms
# output activations a loss is run with: the log losses need scores in (0, 1); everything else also runs on the raw
# (WGAN-GP: rectified) pre-activation
ACTS = {"ns": ("sigmoid",), "mm": ("sigmoid",), "ra": ("sigmoid",), "fisher": ("sigmoid", "relu", "id"),
        "w": ("sigmoid", "relu", "id"), "ls": ("sigmoid", "relu", "id")}
ACTS.update({k: ("sigmoid", "id") for k in F_KEYS})
LS_HYPER = (0.0, 1.0, 1.0)                     # (a, b, c) of ls_gan.py:192-193,213
FISHER_RHO, FISHER_LAMBDA = 0.05, 0.3


def hyper_of(key):
    return LS_HYPER if key == "ls" else (FISHER_RHO,) if key == "fisher" else ()


def _r(x):
    """fl32(x) on an fp64 tensor, straight through for autograd; the identity on fp32 tensors (already rounded)."""
    if x.dtype == torch.float32:
        return x
    return x + (x.float().double() - x).detach()


def _act(a2, out_act):
    return torch.sigmoid(a2) if out_act == "sigmoid" else torch.relu(a2) if out_act == "relu" else a2


def _act_bwd(g, s, out_act):
    """torch's SigmoidBackward / ReluBackward on the OUTPUT s."""
    if out_act == "sigmoid":
        return (g * (1 - s)) * s
    if out_act == "relu":
        return torch.where(s > 0, g, torch.zeros_like(g))
    return g


def loss_terms(key, gen_mode, s, B, hyper=(), lam=None, pen=None):
    """The loss lines of oracle/port.py on scores s ([2B] x rows then g rows; generator mode: [B]), in the dtype of s.
    -> dict(loss, lx, lg, aux): lx / lg the per-row terms (loss = mean(lx) + mean(lg); None for the two critic losses
    that are no mean of row terms), aux: Fisher's (m1x, m1g, m2x, m2g, omega)."""
    eps = EPS32
    hy = [float(np.float32(h)) for h in hyper] + [0.0] * (8 - len(hyper))
    D = not gen_mode
    sx, sg = (s[:B], s[B:]) if D else (None, s)
    lx = aux = None
    if key in ("ns", "mm") and D:                                   # ns_gan.py:191-192, mm_gan.py
        lx = -torch.log(_r(sx + eps))
        lg = -torch.log(_r(_r(1 - sg) + eps))
    elif key in ("ns", "ra") and not D:                             # ns_gan.py:214, ra_gan.py:227
        lg = -torch.log(_r(sg + eps))
    elif key == "mm":                                               # mm_gan.py:235
        lg = torch.log(_r(_r(1 - sg) + eps))
    elif key == "w" or (key == "fisher" and not D):                 # w_gan.py:208,227, fisher_gan.py:246
        if D:
            lx = -sx
        lg = sg if D else -sg
    elif key == "ls":                                               # ls_gan.py:192-193,213
        a, b, c = hy[0], hy[1], hy[2]
        if D:
            lx = 0.5 * (sx - b) ** 2
            lg = 0.5 * (sg - a) ** 2
        else:
            lg = 0.5 * (sg - c) ** 2
    elif key == "ra":                                               # ra_gan.py:204-205
        mg = _r(sg.mean())
        u = torch.sigmoid(_r(sx - mg))
        v = torch.sigmoid(_r(1 - sg))
        loss = -torch.mean(torch.log(u + eps) + torch.log(v + eps)) / 2
        return dict(loss=loss, lx=None, lg=None, aux=None)
    elif key == "fisher":                                           # fisher_gan.py:214-223
        m1x, m1g = _r(sx.mean()), _r(sg.mean())
        m2x, m2g = _r((sx ** 2).mean()), _r((sg ** 2).mean())
        omega = 1 - (0.5 * m2x + 0.5 * m2g)
        rho = hy[0]
        loss = -((m1x - m1g) + lam * omega - (rho / 2) * (omega ** 2))
        return dict(loss=loss, lx=None, lg=None, aux=(m1x, m1g, m2x, m2g, omega))
    elif key == "f_total_variation":                                # f_gan.py:99-142
        if D:
            lx = -(0.5 * torch.tanh(sx))
        lg = 0.5 * torch.tanh(sg) if D else -(0.5 * torch.tanh(sg))
    elif key == "f_forward_kl":
        e = torch.exp(_r(sg - 1))
        if D:
            lx = -sx
        lg = e if D else -e
    elif key == "f_reverse_kl":
        if D:
            lx = torch.exp(sx)
        lg = (-1 - sg) if D else -(-1 - sg)
    elif key == "f_pearson":
        q = 0.25 * sg ** 2 + sg
        if D:
            lx = -sx
        lg = q if D else -q
    elif key == "f_hellinger":
        h = (1 - torch.exp(sg)) / torch.exp(sg)
        if D:
            lx = -(1 - torch.exp(sx))
        lg = h if D else -h
    elif key == "f_jensen_shannon":
        if D:
            lx = -(2 - (1 + torch.exp(-sx)))
        lg = -(2 - torch.exp(sg)) if D else (2 - torch.exp(sg))
    else:
        raise AssertionError(key)
    if D and pen is not None:                                       # gradient-penalty rows ride on the x rows
        lx = lx + hy[7] * pen.to(lx.dtype)
    loss = lg.mean() if lx is None else lx.mean() + lg.mean()
    return dict(loss=loss, lx=lx, lg=lg, aux=aux)


def _rows(t):
    return None if t["lg"] is None else (t["lg"] if t["lx"] is None else torch.cat([t["lx"], t["lg"]])).detach()


def _finish(out, t, B, gen_mode, lam, rho):
    """loss scale and Fisher's state from the terms t."""
    rows = _rows(t)
    out["loss"] = t["loss"].detach().reshape(())
    out["rows"] = rows
    # a mean of row terms cancels (W, total variation on symmetric rows): its rounding error scales with sum |term|
    out["loss_abs"] = float(rows.double().abs().sum()) / B if rows is not None else abs(float(out["loss"]))
    if t["aux"] is not None:
        m1x, m1g, m2x, m2g, omega = [x.detach() for x in t["aux"]]
        out["moments"] = torch.stack([m1x, m1g, m2x, m2g]).reshape(4)
        out["lam_next"] = (lam.detach() + rho * lam.grad).reshape(())      # lambda += rho * lambda.grad (:155-156)
        out["loss_abs"] = float(m1x.abs() + m1g.abs() + (lam.detach() * omega).abs().sum() + (rho / 2) * omega ** 2)


def tail(key, gen_mode, B, out_act, hyper=(), H=None, w2=None, b2=None, X=None, W1=None, b1=None, scores=None,
         pen=None, lam=None, below=None):
    """-> (ref64, ref32): the staged fp64 result and the fp32 torch-CPU autograd result, dicts of detached CPU tensors:
    a2, S, rows (per-row loss terms or None), loss, loss_abs (float: inv_b * sum |term|), dS, gb2, gb2_abs (float:
    sum |dS|), and where there is a head (H or X given): h, dH, gw2; with layer 1 (X, W1, b1): gW1, gb1, dX (times below * (1 - below) if `below`,
    the sigmoid gradient epilogue of the generator's output layer); Fisher critic: moments [m1x, m1g, m2x, m2g], lam_next.

    Inputs are fp32 CPU tensors.  scores: the tail starts at given SCORES (ops.gan_loss; dS is then the gradient by the
    pre-activation through act' at that score)."""
    D = not gen_mode
    R = 2 * B if D else B
    rho = float(np.float32(hyper[0])) if key == "fisher" and hyper else 0.0
    two_phase_fisher = key == "fisher" and D
    out = []
    for dt in (torch.float64, torch.float32):
        o = {}
        c = lambda t: None if t is None else t.detach().to(dt)
        lam_t = torch.tensor([float(np.float32(lam))], dtype=dt, requires_grad=True) if two_phase_fisher else None
        staged = dt == torch.float64
        h = None
        if scores is not None:
            s = c(scores).reshape(R).requires_grad_(True)
            leaves = None
        else:
            w2_, b2_ = c(w2).reshape(-1), c(b2).reshape(())
            if X is not None:
                X_, W1_, b1_ = c(X), c(W1), c(b1)
                if staged:
                    h = _r(torch.relu(X_ @ W1_.t() + b1_)).detach()
                else:
                    X_.requires_grad_(True); W1_.requires_grad_(True); b1_.requires_grad_(True)
                    h = torch.relu(X_ @ W1_.t() + b1_)
                    h.retain_grad()
            else:
                h = c(H)
                if not staged:
                    h.requires_grad_(True)
            if staged:
                a2 = (h @ w2_ + b2_).detach()
                s = _r(_act(a2, out_act)).detach().requires_grad_(True)
            else:
                w2_.requires_grad_(True); b2_.requires_grad_(True)
                a2 = h @ w2_ + b2_
                a2.retain_grad()
                s = _act(a2, out_act)
                s.retain_grad()
            o["a2"] = a2.detach()
        t = loss_terms(key, gen_mode, s, B, hyper, lam_t, c(pen))
        t["loss"].backward()
        _finish(o, t, B, gen_mode, lam_t, rho)
        o["S"] = s.detach()
        if staged or scores is not None:
            dS = _act_bwd(s.grad, s.detach(), out_act)
        else:
            dS = a2.grad
        o["dS"] = dS.detach()
        o["gb2_abs"] = float(dS.double().abs().sum())
        if staged or scores is not None:                            # the two halves summed separately, as autograd does
            o["gb2"] = ((_r(dS[:B].sum()) + _r(dS[B:].sum())) if D else dS.sum()).detach().reshape(())
        if h is not None:
            hd = h.detach()
            o["h"] = hd
            mask = (hd > 0).to(dt)
            if staged:
                dH = (dS[:, None] * w2_[None, :]) * mask
                o["gw2"] = dS @ hd
                if X is not None:
                    o["gW1"], o["gb1"], dX = dH.t() @ X_, dH.sum(0), dH @ W1_
            else:
                dH = h.grad * mask                                   # ReluBackward of the hidden layer folded in
                o["gw2"], o["gb2"] = w2_.grad, b2_.grad.reshape(())
                if X is not None:
                    o["gW1"], o["gb1"], dX = W1_.grad, b1_.grad, X_.grad
            o["dH"] = dH.detach()
            if X is not None:
                if below is not None:
                    bl = c(below)
                    dX = dX * (bl * (1 - bl))
                o["dX"] = dX.detach()
        out.append(o)
    return out[0], out[1]


def adam_step(p, g, m, v, step_size, bc2_sqrt, betas=(0.9, 0.999), eps=1e-8):
    """torch's _single_tensor_adam (no weight decay) in the dtype of p: -> (p, m, v)."""
    dt = p.dtype
    # the constants as the kernels and torch's fp32 ops hold them: rounded to fp32 once
    omb1, b2, omb2, eps = (float(np.float32(x)) for x in (1.0 - betas[0], betas[1], 1.0 - betas[1], eps))
    g = g.to(dt)
    m = m + omb1 * (g - m)
    v = v * b2 + (omb2 * g) * g
    denom = v.sqrt() / float(bc2_sqrt) + eps
    p = p + ((-float(step_size)) * m) / denom
    return p, m, v


# ---- banded inputs ----------------------------------------------------------------------------------------------------
# Every row's fp64 pre-activation lies in one of two bands: ordinary |a2| <= 6, or saturated -- a2 >= 20, -40 <= a2 <= -20,
# a2 <= -110 (sigmoid scores: fp32 sigmoid is exactly 1 from 17 and exactly 0 below about -104), 20 <= |a2| <= 30 where
# the score is the pre-activation itself, so that every exp stays finite in fp32.  Between 6 and 20 the term 1 - s is a
# few fp32 ulps wide and the comparison is ill-conditioned, between -104 and -87 the score is denormal: no row is BUILT
# there.  All inputs sit on dyadic grids chosen so that every product and every partial sum of X W1^T + b1 and of
# h . w2 + b2 is exact in fp32 in ANY summation order: the HIP kernels, the fp32 CPU run and the fp64 reference then
# start the loss tail from the same a2 bit for bit, and what is compared is the tail's arithmetic (sigmoid, log, exp,
# the divisions, act') alone -- a summation-order difference of one ulp of a2 = -30 would otherwise move the score by
# 3e-6 of itself, far more than the tail's own rounding.
def row_kinds(n):
    """Kind of row i of a half: odd rows ordinary (0); even rows saturated, cycling +, -, far - (1, 2, 3)."""
    i = np.arange(n)
    return np.where(i % 2 == 1, 0, 1 + (i // 2) % 3)


def _targets(kinds, out_act, rng):
    sig = out_act == "sigmoid"
    lo = {0: -5.0, 1: 21.0, 2: -38.0 if sig else -28.5, 3: -140.0 if sig else 21.0}
    hi = {0: 5.0, 1: 55.0 if sig else 28.5, 2: -22.0, 3: -112.0 if sig else 28.5}
    return np.array([rng.uniform(lo[k], hi[k]) for k in kinds])


def in_ordinary(a2):
    return a2.abs() <= 6.0


def in_saturated(a2, out_act):
    if out_act == "sigmoid":
        return (a2 >= 20.0) | ((a2 >= -40.0) & (a2 <= -20.0)) | (a2 <= -110.0)
    return (a2.abs() >= 20.0) & (a2.abs() <= 30.0)


def check_bands(a2, out_act, B, gen_mode):
    """Asserts the input rule on the reference's fp64 pre-activations; -> the saturated rows (bool [R])."""
    a2 = a2.double()
    sat, ordi = in_saturated(a2, out_act), in_ordinary(a2)
    assert int((~(sat | ordi)).sum()) == 0, "rows outside both bands: %s" % a2[~(sat | ordi)].tolist()
    halves = [slice(0, B)] if gen_mode else [slice(0, B), slice(B, 2 * B)]
    for hf in halves:
        assert 4 * int(sat[hf].sum()) >= B, "fewer than a quarter of the rows saturated"
        if B >= 3:
            assert bool((a2[hf][sat[hf]] > 0).any()) and bool((a2[hf][sat[hf]] < 0).any()), "one sign only"
    return sat


def banded_case(B, I, Hd, out_act, gen_mode, seed):
    """A critic tail whose rows land in the bands: dict(X [R, I], W1 [Hd, I], b1, w2 [1, Hd], b2 [1], H = relu(X W1^T + b1)
    (exact in fp32), a2 (fp64), sat); fp32 CPU tensors.  Layer 1 is fixed; w2 takes the sign of W1 u for one direction u of
    the input space, so that a row k u + noise excites only hidden units of positive w2 and -k u + noise only those of
    negative w2: a2 is monotone in k, and k is found by bisection for the row's target."""
    rng = np.random.RandomState(seed)
    R = B if gen_mode else 2 * B
    u = rng.choice([-1.0, 1.0], size=I)
    W1 = rng.randint(-8, 9, size=(Hd, I)) / 8.0
    sgn = np.where(np.arange(Hd) % 2 == 0, 1.0, -1.0)
    d = W1 @ u
    W1 *= np.where(d * sgn < 0, -1.0, 1.0)[:, None]
    W1 += (np.abs(W1 @ u) < 0.125)[:, None] * sgn[:, None] * u[None, :] / 8.0
    assert bool(((W1 @ u) * sgn > 0).all())
    mmax = max(2, int(round(512.0 / Hd)))
    w2 = sgn * rng.randint(1, mmax + 1, size=Hd) / 128.0
    b1 = rng.randint(-8, 9, size=Hd) / 128.0
    b2 = rng.randint(-32, 33) / 128.0
    noise = rng.randint(-4, 5, size=(R, I)) * (rng.rand(R, I) < 0.5) / 16.0
    kinds = np.concatenate([row_kinds(B)] * (1 if gen_mode else 2))
    t = _targets(kinds, out_act, rng)
    sigma = np.sign(t)

    def rows_of(k):
        return (sigma * k)[:, None] * u[None, :] / 16.0 + noise

    def a2_of(k):
        return np.maximum(rows_of(k) @ W1.T + b1, 0.0) @ w2 + b2

    hi = np.ones(R)
    for _ in range(20):                                   # sigma * a2 is nondecreasing in k: bracket, then bisect
        short = sigma * a2_of(hi) < sigma * t
        if not short.any():
            break
        hi = np.where(short, hi * 2, hi)
    assert not (sigma * a2_of(hi) < sigma * t).any()
    lo = np.zeros(R)
    while (hi - lo > 1).any():
        mid = np.floor((lo + hi) / 2)
        ok = sigma * a2_of(mid) >= sigma * t
        hi, lo = np.where(ok, mid, hi), np.where(ok, lo, mid)
    k = np.where(sigma * a2_of(lo) >= sigma * t, lo, hi)
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    X = rows_of(k)
    pre = X @ W1.T + b1
    # exactness budget: every partial sum on its grid within 24 bits (layer 1: grid 2^-7; head: grid 2^-14)
    assert (np.abs(X) @ np.abs(W1.T)).max() + 1 < 2.0 ** 16 and (np.maximum(pre, 0) @ np.abs(w2)).max() + 1 < 2.0 ** 9
    c = dict(X=f32(X), W1=f32(W1), b1=f32(b1), w2=f32(w2).reshape(1, Hd), b2=f32(np.array([b2])))
    for n, a in (("X", X), ("W1", W1), ("b1", b1), ("w2", w2)):
        assert np.array_equal(c[n].double().numpy().reshape(a.shape), a), n
    c["H"] = f32(np.maximum(pre, 0.0))
    assert np.array_equal(c["H"].double().numpy(), np.maximum(pre, 0.0))
    c["a2"] = torch.from_numpy(a2_of(k))
    c["sat"] = check_bands(c["a2"], out_act, B, gen_mode)
    return c


def exact_scores(B, out_act, gen_mode, seed):
    """Scores for ops.gan_loss, whose inputs are scores: the exactly representable edge values 0, 1, 2^-24, 1 - 2^-24 and
    0.5 on every other row (the `saturated` group), ordinary scores between.  Raw pre-activation scores (id / relu) also
    take +-24 and +-30.  -> (scores [R] fp32, saturated [R] bool)."""
    rng = np.random.RandomState(seed)
    R = B if gen_mode else 2 * B
    edge = [1.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24, 0.5]
    if out_act != "sigmoid":
        edge += [24.0, -24.0, 30.0, -30.0]
        if out_act == "relu":
            edge = [max(e, 0.0) for e in edge]
    s = rng.randn(R)
    if out_act == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-s))
    elif out_act == "relu":
        s = np.maximum(s, 0.0)
    i = np.arange(R) % (B if B > 0 else 1)
    sat = i % 2 == 0
    s[sat] = np.array(edge)[(i[sat] // 2) % len(edge)]
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(sat)
