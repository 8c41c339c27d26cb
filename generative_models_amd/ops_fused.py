"""Tensor-level wrappers for the variant-specific fused kernels (csrc/gm_fused.hip)."""
import ctypes

import torch

from . import _lib
from ._abi import (NO_SLOT, SN_MAX_H, SN_MAX_I, SN_NR, SN_NT, SN_NW2, SN_SIGMA, STD_WS_BYTES,  # noqa: F401
                   ACGANHeadsArgs, CatArgs, DdpmNoise, DdpmOut, DdpmReverseArgs, DdpmTables, FlowParams, FlowStepArgs,
                   FmDivArgs, FmNoise, FmOut, FmStageArgs, FmTables, IafParams, IafStepArgs, IwaeNoise, MadeMaskArgs,
                   MadeSampleArgs, MafCoupleArgs, MafCoupleBwdArgs, MafInvertArgs, MafMaskArgs, NsfCoupleArgs,
                   NsfCoupleBwdArgs, NvpCoupleArgs, NvpCoupleBwdArgs, NvpLossArgs, NvpPostArgs, NvpPreArgs, RbmChainArgs,
                   RbmVbiasArgs, SNGradArgs, SNHeadArgs, SNPowerArgs, VqArgs, VqStepArgs)
from .ops import _ld, stream_ptr


def interp(eps, eps_slot, x, g, out, stream=None):
    """x_hat = eps*x + (1-eps)*g   (w_gp_gan.py:197-201)."""
    B, I = out.shape
    _lib.call("gm_interp", stream or stream_ptr(), eps.data_ptr(), eps_slot, x.data_ptr(), _ld(x),
              g.data_ptr(), _ld(g), out.data_ptr(), _ld(out), B, I)


def gp_u(s, h, w2, u, stream=None):
    B, H = u.shape
    _lib.call("gm_gp_u", stream or stream_ptr(), s.data_ptr(), h.data_ptr(), _ld(h), w2.data_ptr(),
              u.data_ptr(), _ld(u), B, H)


def gp_norm(g, gamma, pen, lam, inv_b, k=1.0, stream=None):
    B, I = g.shape
    _lib.call("gm_gp_norm", stream or stream_ptr(), g.data_ptr(), _ld(g), gamma.data_ptr(),
              _ld(gamma), pen.data_ptr(), lam, inv_b, k, B, I)


def gp_dw2(s, h, t, gw2, stream=None):
    B, H = h.shape
    _lib.call("gm_gp_dw2", stream or stream_ptr(), s.data_ptr(), h.data_ptr(), _ld(h), t.data_ptr(),
              _ld(t), gw2.data_ptr(), B, H)


def gp_dw2_store(s, h, t, out, stream=None):
    """out[n] = sum_b [s_b>0][h[b,n]>0] t[b,n] (gp_dw2 without the accumulation)."""
    B, H = h.shape
    _lib.call("gm_gp_dw2_store", stream or stream_ptr(), s.data_ptr(), h.data_ptr(), _ld(h), t.data_ptr(),
              _ld(t), out.data_ptr(), B, H)


def head_gp(h, w2, b2, s, u, stream=None):
    """D(x_hat)'s N = 1 layer + the seed of the input gradient in one launch (w_gp_gan.py:202-212)."""
    B, H = u.shape
    _lib.call("gm_head_gp", stream or stream_ptr(), h.data_ptr(), _ld(h), w2.data_ptr(), b2.data_ptr(),
              s.data_ptr(), u.data_ptr(), _ld(u), B, H)


def bir_reparam(mu, eps, z, B, Z, eps_slot=NO_SLOT, stream=None):
    """z = mu + eps (bir_vae.py:86-97; eps drawn on the host from numpy's global RNG)."""
    _lib.call("gm_bir_reparam", stream or stream_ptr(), mu.data_ptr(), _ld(mu), eps.data_ptr(), eps_slot,
              z.data_ptr(), _ld(z), B, Z)


def bir_mmd(z, prior, partial, dz, B, Z, lam, prior_slot=NO_SLOT, stream=None):
    """Row shares of the Gaussian-kernel MMD (bir_vae.py:201-221) and d(lam*mmd)/dz (dz may be None)."""
    _lib.call("gm_bir_mmd", stream or stream_ptr(), z.data_ptr(), _ld(z), prior.data_ptr(), prior_slot,
              partial.data_ptr(), dz.data_ptr() if dz is not None else None,
              _ld(dz) if dz is not None else 0, B, Z, lam)


def vae_reparam(ml, eps, z, kl_out, B, Z, eps_slot=NO_SLOT, kl_slot=NO_SLOT, stream=None):
    _lib.call("gm_vae_reparam", stream or stream_ptr(), ml.data_ptr(), _ld(ml), eps.data_ptr(),
              eps_slot, z.data_ptr(), _ld(z), kl_out.data_ptr(), kl_slot, B, Z)


def vae_reparam_wide(ml, eps, z, kl_part, B, Z, eps_slot=NO_SLOT, stream=None):
    """z = mu + eps*exp(lv/2); KL left as per-workgroup partial sums in kl_part (see sum_finalize2)."""
    _lib.call("gm_vae_reparam_wide", stream or stream_ptr(), ml.data_ptr(), _ld(ml), eps.data_ptr(),
              eps_slot, z.data_ptr(), _ld(z), kl_part.data_ptr(), kl_part.numel(), B, Z)
    return (B * Z + 255) // 256


def vae_bwd_mid(dHdec, Wd1, ml, eps, dml, Wml, He, dHe, B, eps_slot=NO_SLOT, stream=None):
    """dz = dHdec W_d1, d loss / d [mu | log_var] (-> dml), dHe = (dml W_ml) . [He > 0] as ONE launch (gm_vae_bwd_mid)."""
    Hd, Z = Wd1.shape
    if Hd > 512 or Wml.shape[1] != Hd or He.shape[1] < Hd:
        raise ValueError("vae_bwd_mid: one hidden width <= 512 for decoder and encoder (got %d / %d); use "
                         "linear_bwd_dx_reparam + linear_bwd_dx" % (Hd, Wml.shape[1]))
    _lib.call("gm_vae_bwd_mid", stream or stream_ptr(), dHdec.data_ptr(), _ld(dHdec), Wd1.data_ptr(), ml.data_ptr(),
              _ld(ml), eps.data_ptr(), eps_slot, dml.data_ptr(), _ld(dml), Wml.data_ptr(), He.data_ptr(), _ld(He),
              dHe.data_ptr(), _ld(dHe), B, Hd, Z)


def vae_reparam_fwd(ml, eps, z, kl_part, B, Z, W, bias, H, act, eps_slot=NO_SLOT, stream=None):
    """vae_reparam_wide + the decoder's first layer H = act(z W^T + bias) as ONE launch (gm_vae_reparam_fwd)."""
    from .ops import ACT
    _lib.call("gm_vae_reparam_fwd", stream or stream_ptr(), ml.data_ptr(), _ld(ml), eps.data_ptr(), eps_slot,
              z.data_ptr(), _ld(z), kl_part.data_ptr(), kl_part.numel(), B, Z, W.data_ptr(),
              bias.data_ptr() if bias is not None else None, H.data_ptr(), _ld(H), W.shape[0], ACT[act])
    return (B * Z + 255) // 256


def vae_reparam_fwd_label(ml, eps, z, kl_part, B, Z, W, bias, H, act, E, lab, eps_slot=NO_SLOT, stream=None):
    """vae_reparam_fwd whose decoder layer adds E[:, y_m] before the activation (gm_vae_reparam_fwd_label; the
    class-conditional decoder of cvae.py).  lab: ops.label_src."""
    from .ops import ACT, _check_labels
    if E.dim() != 2 or E.shape[0] != W.shape[0] or not 1 <= E.shape[1] <= 32 or not E.is_contiguous():
        raise _lib.GMError("label weight E must be [N=%d, C] with 1 <= C <= 32, got %s" % (W.shape[0], tuple(E.shape)))
    _check_labels(lab, B)
    _lib.call("gm_vae_reparam_fwd_label", stream or stream_ptr(), ml.data_ptr(), _ld(ml), eps.data_ptr(), eps_slot,
              z.data_ptr(), _ld(z), kl_part.data_ptr(), kl_part.numel(), B, Z, W.data_ptr(),
              bias.data_ptr() if bias is not None else None, H.data_ptr(), _ld(H), W.shape[0], ACT[act],
              E.data_ptr(), E.shape[1], lab)
    return (B * Z + 255) // 256


def sum_finalize2(pa, na, out_a, slot_a, pb, nb, out_b, slot_b, scale_a=1.0, scale_b=1.0, tick=None, stream=None):
    """Two fixed-order fp64 sums in one launch; tick: device step counter to advance (last launch of a step)."""
    _lib.call("gm_sum_finalize2_tick", stream or stream_ptr(), pa.data_ptr(), na, scale_a, out_a.data_ptr(),
              slot_a, pb.data_ptr(), nb, scale_b, out_b.data_ptr(), slot_b,
              tick.data_ptr() if tick is not None else None)


def vae_reparam_bwd(ml, eps, dz, dml, B, Z, eps_slot=NO_SLOT, stream=None):
    _lib.call("gm_vae_reparam_bwd", stream or stream_ptr(), ml.data_ptr(), _ld(ml), eps.data_ptr(),
              eps_slot, dz.data_ptr(), _ld(dz), dml.data_ptr(), _ld(dml), B, Z)


def sqerr_sigmoid_bwd(x, xr, dA, partial, B, stream=None):
    I = x.shape[1]
    _lib.call("gm_sqerr_sigmoid_bwd", stream or stream_ptr(), x.data_ptr(), _ld(x), xr.data_ptr(),
              _ld(xr), dA.data_ptr(), _ld(dA), partial.data_ptr(), B, I)


def sum_finalize(partial, n, out, scale=1.0, out_slot=NO_SLOT, tick=None, stream=None):
    """out[slot] = scale * sum(partial[:n]) (fp64, fixed order).  tick: device step counter to advance
    (this is then the last launch of the step)."""
    if tick is not None:
        _lib.call("gm_sum_finalize_tick", stream or stream_ptr(), partial.data_ptr(), n, scale,
                  out.data_ptr(), out_slot, tick.data_ptr())
        return
    _lib.call("gm_sum_finalize", stream or stream_ptr(), partial.data_ptr(), n, scale,
              out.data_ptr(), out_slot)


def head_fwd_loss(variant, gen_mode, H, w2, b2, out_act, B, hyper, inv_b, pen, S, dS, rowloss,
                  dH=None, final=None, stream=None):
    """Fused critic head forward + per-row loss + d loss/d pre-activation (separable variants).
    dH: also write the hidden-layer gradient.  final = dict(loss_out, loss_slot, done, tick=None):
    the last workgroup also writes the loss scalar (and ticks) -- no head_bwd needed for scalars."""
    import ctypes
    from ._lib import ACT, LOSS
    h = (ctypes.c_float * 8)(*([float(x) for x in hyper] + [0.0] * (8 - len(hyper))))
    args = [stream or stream_ptr(), LOSS[variant], 1 if gen_mode else 0,
            H.data_ptr(), _ld(H), w2.data_ptr(), b2.data_ptr(), ACT[out_act], B, H.shape[1], h,
            len(hyper), inv_b, pen.data_ptr() if pen is not None else None, S.data_ptr(),
            dS.data_ptr(), rowloss.data_ptr(), dH.data_ptr() if dH is not None else None,
            _ld(dH) if dH is not None else 0]
    if final is None:
        _lib.call("gm_head_fwd_loss", *args)
        return
    done, tick = final["done"], final.get("tick")
    assert done.dtype == torch.int32 and done.numel() >= 1
    _lib.call("gm_head_fwd_loss_final", *args, final["loss_out"].data_ptr(), final["loss_slot"],
              done.data_ptr(), tick.data_ptr() if tick is not None else None)


def head_bwd(H, dS, w2, rowloss, dH, gw2, gb2, loss_out, loss_slot, inv_b, gen_mode, B, lin=None,
             adam=None, tick=None, betas=(0.9, 0.999), eps=1e-8, stream=None):
    """dH = dS (x) w2 masked by H>0; gw2 = dS^T H; gb2; loss scalar (see gm_hip.h).
    adam (dict(sched, sched_slot, clamp)) + lin (engine._Linear of the head): also apply Adam to
    (w2, b2) here.  tick: device int64 counter to advance once the loss slot is written."""
    g = lambda t: t.data_ptr() if t is not None else None
    ldd = _ld(dH) if dH is not None else 0      # dH=None: head_fwd_loss already wrote it
    if adam is None and tick is None:
        _lib.call("gm_head_bwd", stream or stream_ptr(), H.data_ptr(), _ld(H), dS.data_ptr(),
                  w2.data_ptr(), rowloss.data_ptr(), g(dH), ldd, g(gw2), g(gb2),
                  loss_out.data_ptr(), loss_slot, inv_b, 1 if gen_mode else 0, B, H.shape[1])
        return
    with_adam = adam is not None
    _lib.call("gm_head_bwd_fused", stream or stream_ptr(), H.data_ptr(), _ld(H), dS.data_ptr(),
              w2.data_ptr(), lin.b.data_ptr() if with_adam else None, rowloss.data_ptr(),
              g(dH), ldd, g(gw2), g(gb2), loss_out.data_ptr(), loss_slot, inv_b,
              1 if gen_mode else 0, B, H.shape[1], 1 if with_adam else 0,
              lin.mW.data_ptr() if with_adam else None, lin.vW.data_ptr() if with_adam else None,
              lin.mb.data_ptr() if with_adam else None, lin.vb.data_ptr() if with_adam else None,
              adam["sched"].data_ptr() if with_adam else None,
              adam["sched_slot"] if with_adam else NO_SLOT, betas[0], betas[1], eps, 0.0,
              adam.get("clamp", 0.0) if with_adam else 0.0, g(tick))


def info_q_loss(q, noise, noise_slot, B, z_dim, disc_dim, cont_dim, dq, loss_out, loss_slot,
                lam=1.0, B_global=None, stream=None):
    """InfoGAN train_Q loss (info_gan.py:295-302) + d loss / d q."""
    _lib.call("gm_info_q_loss_dp", stream or stream_ptr(), q.data_ptr(), _ld(q), noise.data_ptr(),
              noise_slot, z_dim + disc_dim + cont_dim, B, B if B_global is None else B_global, z_dim,
              disc_dim, cont_dim, lam, dq.data_ptr(), _ld(dq), loss_out.data_ptr(), loss_slot)


def l1_rows(Y, X, R, B, K_dev, dY, rowsum, B_global=None, stream=None):
    """Per-row L1 error + gradient (BEGAN, be_gan.py:225-236,256).  B_global: the mean's
    denominator when this rank holds B of B_global rows."""
    _lib.call("gm_l1_rows_dp", stream or stream_ptr(), Y.data_ptr(), _ld(Y), X.data_ptr(), _ld(X), R,
              Y.shape[1], B, B if B_global is None else B_global,
              K_dev.data_ptr() if K_dev is not None else None, dY.data_ptr(), _ld(dY), rowsum.data_ptr())


def began_dloss(rows, B, state, loss_out, loss_slot, B_global=None, stream=None):
    _lib.call("gm_began_dloss_dp", stream or stream_ptr(), rows.data_ptr(), B,
              B if B_global is None else B_global, state.data_ptr(), loss_out.data_ptr(), loss_slot)


def began_update(state, dstate, istate, gamma, lam, patience, tick, stream=None):
    _lib.call("gm_began_update", stream or stream_ptr(), state.data_ptr(), dstate.data_ptr(),
              istate.data_ptr(), gamma, lam, patience, tick.data_ptr() if tick is not None else None)


def std_workspace(device):
    """Zeroed workspace of the multi-workgroup std kernels (allocate once, outside graph capture)."""
    import torch
    return torch.zeros(STD_WS_BYTES // 8, dtype=torch.float64, device=device)


def std_sums(X, R, out2, ws=None, stream=None):
    ws = std_workspace(X.device) if ws is None else ws
    _lib.call("gm_std_sums", stream or stream_ptr(), X.data_ptr(), _ld(X), R, X.shape[1], out2.data_ptr(),
              ws.data_ptr())


def std_from_sums(sums2, n_total, out, stream=None):
    _lib.call("gm_std_from_sums", stream or stream_ptr(), sums2.data_ptr(), n_total, out.data_ptr())


def std_all(X, R, out, ws=None, stream=None):
    ws = std_workspace(X.device) if ws is None else ws
    _lib.call("gm_std_all", stream or stream_ptr(), X.data_ptr(), _ld(X), R, X.shape[1], out.data_ptr(),
              ws.data_ptr())


def dragan_xhat(x, delta, delta_slot, U, u_slot, std_dev, out, B, C=1.0, stream=None):
    _lib.call("gm_dragan_xhat", stream or stream_ptr(), x.data_ptr(), _ld(x), delta.data_ptr(),
              delta_slot, U.data_ptr(), u_slot, std_dev.data_ptr(), C, out.data_ptr(), _ld(out), B,
              out.shape[1])


def dragan_rows(s, V, dv, da2, pen, lam, inv_b, B, K=1.0, stream=None):
    _lib.call("gm_dragan_rows", stream or stream_ptr(), s.data_ptr(), V.data_ptr(), _ld(V),
              dv.data_ptr(), _ld(dv), da2.data_ptr(), pen.data_ptr(), lam, inv_b, K, B, V.shape[1])


def fisher_commit(aux, stream=None):
    """aux[0] = aux[5]: lambda's successor, computed by the folded Fisher critic step, becomes lambda."""
    _lib.call("gm_fisher_commit", stream or stream_ptr(), aux.data_ptr())


def dragan_head_bwd(H, T, da2, w2, gw2, gb2, dA1, B, store=False, stream=None):
    """store: gw2 / gb2 receive the penalty's share alone (for the head backward's gw2_add / gb2_add)."""
    _lib.call("gm_dragan_head_bwd_store" if store else "gm_dragan_head_bwd", stream or stream_ptr(), H.data_ptr(), _ld(H), T.data_ptr(), _ld(T),
              da2.data_ptr(), w2.data_ptr(), gw2.data_ptr(), gb2.data_ptr(), dA1.data_ptr(), _ld(dA1),
              B, H.shape[1])


def _aae_shape(B, Z, H):
    if not (B > 0 and 0 < Z <= 32 and Z % 4 == 0 and 0 < H <= 512):
        raise _lib.GMError("the AAE kernels take 1 <= Z <= 32 with Z %% 4 == 0 and 1 <= H <= 512 (got B=%d, Z=%d, "
                           "H=%d); other shapes train on the general path" % (B, Z, H))


def aae_critic_workspace(B, Z, H, device):
    """A workspace for aae_critic_step at this shape (float32 device tensor)."""
    _aae_shape(B, Z, H)
    n = _lib.load().gm_aae_critic_workspace_bytes(B, Z, H)
    return torch.zeros((n + 3) // 4, device=device)


def aae_critic_step(z_real, z_fake, B, W1, b1, w2, b2, ws, grads=None, adam=None, moments=None, loss_out=None,
                    real_slot=NO_SLOT, loss_slot=NO_SLOT, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, stream=None):
    """The AAE's discriminator phase (gm_aae_critic_step): D = (W1 [H, Z], b1, w2 [1, H] or [H], b2) on B prior rows
    (z_real + real_slot) and B encoder rows z_fake; grads = (gW1, gb1, gw2, gb2) receive the gradient of
    -mean(log(D(z_real) + 1e-8) + log(1 - D(z_fake) + 1e-8)); with adam = dict(sched, sched_slot) and moments =
    (mW1, vW1, mb1, vb1, mw2, vw2, mb2, vb2) Adam steps D in the same launches; loss_out[loss_slot] = the loss."""
    from ._lib import AAECriticArgs
    H, Z = W1.shape
    _aae_shape(B, Z, H)
    if w2.numel() != H or b1.numel() != H or b2.numel() != 1 or z_fake.shape[0] < B or z_fake.shape[1] != Z:
        raise _lib.GMError("aae_critic_step: D must be [H, Z], [H], [1, H], [1] and z_fake [>= B, Z]")
    if ws.numel() * 4 < _lib.load().gm_aae_critic_workspace_bytes(B, Z, H):
        raise _lib.GMError("aae_critic_step: workspace too small (use aae_critic_workspace)")
    p = lambda t: t.data_ptr() if t is not None else None
    a = AAECriticArgs()
    a.z_real, a.real_slot, a.z_fake, a.ld_fake = p(z_real), real_slot, p(z_fake), _ld(z_fake)
    a.B, a.Z, a.H = B, Z, H
    a.W1, a.b1, a.w2, a.b2 = p(W1), p(b1), p(w2), p(b2)
    if grads is not None:
        a.gW1, a.gb1, a.gw2, a.gb2 = (p(g) for g in grads)
    if adam is not None:
        a.mW1, a.vW1, a.mb1, a.vb1, a.mw2, a.vw2, a.mb2, a.vb2 = (p(m) for m in moments)
        a.sched, a.sched_slot = p(adam["sched"]), adam["sched_slot"]
    a.beta1, a.beta2, a.eps, a.weight_decay = betas[0], betas[1], eps, weight_decay
    a.loss_out, a.loss_slot = p(loss_out), loss_slot
    a.ws, a.ws_bytes = p(ws), ws.numel() * 4
    import ctypes
    _lib.call("gm_aae_critic_step", stream or stream_ptr(), ctypes.byref(a))


def aae_gen_mid(z, He, W1, b1, w2, b2, Wz, dz, dHe, loss_part, B, stream=None):
    """The AAE's generator-phase middle launch (gm_aae_gen_mid): D (W1, b1, w2, b2) on the encoder rows z, the row terms
    -log(D(z) + 1e-8) into loss_part[:B], dz = d G_loss / d z and dHe = (dz Wz) . [He > 0]."""
    from ._lib import AAEGenArgs
    H, Z = W1.shape
    _aae_shape(B, Z, H)
    if tuple(Wz.shape) != (Z, H) or He.shape[1] != H or z.shape[1] != Z or loss_part.numel() < B:
        raise _lib.GMError("aae_gen_mid: Wz must be [Z, H], He [B, H], z [B, Z] and loss_part >= B floats")
    a = AAEGenArgs()
    a.z, a.ldz, a.He, a.ldhe = z.data_ptr(), _ld(z), He.data_ptr(), _ld(He)
    a.W1, a.b1, a.w2, a.b2, a.Wz = W1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), Wz.data_ptr()
    a.dz, a.lddz, a.dHe, a.lddhe = dz.data_ptr(), _ld(dz), dHe.data_ptr(), _ld(dHe)
    a.loss_part, a.B, a.Z, a.H = loss_part.data_ptr(), B, Z, H
    import ctypes
    _lib.call("gm_aae_gen_mid", stream or stream_ptr(), ctypes.byref(a))


# ---- auxiliary-classifier GAN (csrc/gm_acgan.hip; acgan.py) ---------------------------------------------------------
def _acgan_shape(rows, Hd, C):
    if not (rows >= 1 and 1 <= C <= 32 and 4 <= Hd <= 1024 and Hd % 4 == 0):
        raise _lib.GMError("the AC-GAN head kernels take 1 <= C <= 32 and 4 <= Hd <= 1024 with Hd %% 4 == 0 (got "
                           "rows=%d, Hd=%d, C=%d); other shapes train on the general path" % (rows, Hd, C))


def acgan_heads_workspace(rows, Hd, C, device):
    """A zeroed workspace for acgan_heads_fwd / acgan_heads_bwd at this shape (float32 device tensor)."""
    _acgan_shape(rows, Hd, C)
    n = _lib.load().gm_acgan_heads_workspace_bytes(rows, Hd, C)
    return torch.zeros((n + 3) // 4, device=device)


def _acgan_args(H, w2, b2, Wc, bc, B, gen_mode, class_weight, da2, dq, ws, rows):
    C, Hd = Wc.shape
    rows = (B if gen_mode else 2 * B) if rows is None else rows
    _acgan_shape(rows, Hd, C)
    if (H.dim() != 2 or H.shape[0] < rows or H.shape[1] != Hd or w2.numel() != Hd or b2.numel() != 1
            or bc.numel() != C or da2.numel() < rows or dq.dim() != 2 or dq.shape[0] < rows or dq.shape[1] != C
            or not Wc.is_contiguous()):
        raise _lib.GMError("acgan heads: H must be [>= rows, Hd], w2 [1, Hd], b2 [1], Wc [C, Hd] contiguous, bc [C], "
                           "da2 [>= rows] and dq [>= rows, C]")
    if ws.numel() * 4 < _lib.load().gm_acgan_heads_workspace_bytes(rows, Hd, C):
        raise _lib.GMError("acgan heads: workspace too small (use acgan_heads_workspace)")
    a = ACGANHeadsArgs()
    a.H, a.ldh, a.rows, a.B, a.Hd, a.C, a.gen_mode = H.data_ptr(), _ld(H), rows, B, Hd, C, 1 if gen_mode else 0
    a.w2, a.b2, a.Wc, a.bc = w2.data_ptr(), b2.data_ptr(), Wc.data_ptr(), bc.data_ptr()
    a.class_weight = float(class_weight)
    a.da2, a.dq, a.lddq = da2.data_ptr(), dq.data_ptr(), _ld(dq)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    return a


def acgan_heads_fwd(H, w2, b2, Wc, bc, lab, B, gen_mode, class_weight, da2, dq, ws, loss_out=None, loss_slot=NO_SLOT,
                    ce_out=None, ce_slot=NO_SLOT, acc_out=None, acc_slot=NO_SLOT, rows=None, stream=None):
    """Both AC-GAN critic heads on the hidden rows H (gm_acgan_heads_fwd): critic mode on 2B stacked rows [x; G(z, y)],
    generator mode on B generated rows; row m (and fake row B + m) has class lab[m] (ops.label_src).  Writes da2
    [rows] and dq [rows, C]; loss_out[loss_slot] = the total loss, ce_out[ce_slot] = CE of rows [0, B), acc_out[acc_slot]
    = the number of correctly classified real rows (critic mode)."""
    import ctypes
    from .ops import _check_labels
    a = _acgan_args(H, w2, b2, Wc, bc, B, gen_mode, class_weight, da2, dq, ws, rows)
    _check_labels(lab, B)
    a.lab = lab
    p = lambda t: t.data_ptr() if t is not None else None
    a.loss_out, a.loss_slot, a.ce_out, a.ce_slot = p(loss_out), loss_slot, p(ce_out), ce_slot
    a.acc_out, a.acc_slot = p(acc_out), acc_slot
    _lib.call("gm_acgan_heads_fwd", stream or stream_ptr(), ctypes.byref(a))


def acgan_heads_bwd(H, w2, b2, Wc, bc, B, gen_mode, da2, dq, dPre, ws, grads=None, adam=None, moments=None, rows=None,
                    betas=(0.9, 0.999), eps=1e-8, stream=None):
    """Both heads' backward (gm_acgan_heads_bwd): dPre = (da2 w2 + dq Wc) . [H > 0]; critic mode: grads = (gw2, gb2,
    gWc, gbc) receive the heads' gradients, and with adam = dict(sched, sched_slot) and moments = (mw2, vw2, mb2, vb2,
    mWc, vWc, mbc, vbc) Adam steps the four tensors in the same call."""
    import ctypes
    a = _acgan_args(H, w2, b2, Wc, bc, B, gen_mode, 0.0, da2, dq, ws, rows)
    if dPre.dim() != 2 or dPre.shape[0] < a.rows or dPre.shape[1] != a.Hd:
        raise _lib.GMError("acgan_heads_bwd: dPre must be [>= rows, Hd]")
    a.dPre, a.ldp = dPre.data_ptr(), _ld(dPre)
    if grads is not None:
        for g, ref in zip(grads, (w2, b2, Wc, bc)):
            if g.numel() != ref.numel() or not g.is_contiguous():
                raise _lib.GMError("acgan_heads_bwd: a gradient output does not match its parameter")
        a.gw2, a.gb2, a.gWc, a.gbc = (g.data_ptr() for g in grads)
    if adam is not None:
        a.mw2, a.vw2, a.mb2, a.vb2, a.mWc, a.vWc, a.mbc, a.vbc = (m.data_ptr() for m in moments)
        a.sched, a.sched_slot = adam["sched"].data_ptr(), adam["sched_slot"]
    a.beta1, a.beta2, a.eps = betas[0], betas[1], eps
    _lib.call("gm_acgan_heads_bwd", stream or stream_ptr(), ctypes.byref(a))


# ---- spectrally normalised hinge GAN (csrc/gm_sn.hip; sngan.py) -----------------------------------------------------
def _sn_w_shape(H, I):
    if not (4 <= H <= SN_MAX_H and H % 4 == 0 and 1 <= I <= SN_MAX_I):
        raise _lib.GMError("the spectral-norm kernels take 4 <= H <= 1024 with H %% 4 == 0 and 1 <= I <= 8192 (got "
                           "H=%d, I=%d); other shapes train on the general path" % (H, I))


def _sn_ws(nbytes, device):
    return torch.zeros((nbytes + 3) // 4, device=device)


def sn_power_workspace(H, I, device):
    _sn_w_shape(H, I)
    return _sn_ws(_lib.load().gm_sn_power_workspace_bytes(H, I), device)


def sn_head_workspace(rows, Hd, device):
    """A zeroed workspace for sn_head_fwd / sn_head_bwd at this shape (float32 device tensor)."""
    _sn_w_shape(Hd, 1)
    if rows < 1:
        raise _lib.GMError("sn head: rows must be >= 1")
    return _sn_ws(_lib.load().gm_sn_head_workspace_bytes(rows, Hd), device)


def sn_grad_workspace(H, device):
    _sn_w_shape(H, 1)
    return _sn_ws(_lib.load().gm_sn_grad_workspace_bytes(H), device)


def sn_power_iter(W, u, v, Wbar, w2, w2bar, stats, ws, update_u=True, stream=None):
    """One power-iteration step on W [H, I] (gm_sn_power_iter, three launches): v = normalize(W^T u), u' = normalize(W v),
    sigma = u'^T W v; writes v [I], Wbar = W / sigma, w2bar = w2 / ||w2||, stats [4] = (sigma, ||w2||, ||W^T u||,
    ||W v||) and, with update_u, u' over u.  update_u=False (eval mode): sigma = u^T W v with the stored u."""
    H, I = W.shape
    _sn_w_shape(H, I)
    if (not (W.is_contiguous() and Wbar.is_contiguous()) or tuple(Wbar.shape) != (H, I) or u.numel() != H
            or v.numel() != I or w2.numel() != H or w2bar.numel() != H or stats.numel() < 4):
        raise _lib.GMError("sn_power_iter: W and Wbar must be contiguous [H, I], u, w2, w2bar [H], v [I], stats [4]")
    a = SNPowerArgs()
    a.W, a.H, a.I, a.u, a.v, a.Wbar = W.data_ptr(), H, I, u.data_ptr(), v.data_ptr(), Wbar.data_ptr()
    a.w2, a.w2bar, a.stats, a.update_u = w2.data_ptr(), w2bar.data_ptr(), stats.data_ptr(), 1 if update_u else 0
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    _lib.call("gm_sn_power_iter", stream or stream_ptr(), ctypes.byref(a))


def _sn_head_args(H, w2bar, B, gen_mode, ds, ws, rows):
    Hd = w2bar.numel()
    rows = (B if gen_mode else 2 * B) if rows is None else rows
    _sn_w_shape(Hd, 1)
    if H.dim() != 2 or H.shape[0] < rows or H.shape[1] != Hd or ds.numel() < rows or rows < 1:
        raise _lib.GMError("sn head: H must be [>= rows, Hd], w2bar [Hd] and ds [>= rows]")
    a = SNHeadArgs()
    a.H, a.ldh, a.rows, a.B, a.Hd, a.gen_mode = H.data_ptr(), _ld(H), rows, B, Hd, 1 if gen_mode else 0
    a.w2bar, a.ds = w2bar.data_ptr(), ds.data_ptr()
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 4
    return a


def sn_head_fwd(H, w2bar, b2, B, gen_mode, s, ds, ws, loss_out=None, loss_slot=NO_SLOT, rows=None, stream=None):
    """The hinge head on the hidden rows H (gm_sn_head_fwd): s = H w2bar + b2, ds = d loss / d s, and loss_out[loss_slot]
    = mean relu(1 - s_real) + mean relu(1 + s_fake) on 2B stacked rows (critic mode) or -mean s on B rows."""
    a = _sn_head_args(H, w2bar, B, gen_mode, ds, ws, rows)
    if s.numel() < a.rows or b2.numel() != 1:
        raise _lib.GMError("sn_head_fwd: s must be [>= rows] and b2 [1]")
    a.b2, a.s = b2.data_ptr(), s.data_ptr()
    if loss_out is not None:
        a.loss_out, a.loss_slot = loss_out.data_ptr(), loss_slot
    _lib.call("gm_sn_head_fwd", stream or stream_ptr(), ctypes.byref(a))


def sn_head_bwd(H, w2bar, B, gen_mode, ds, dPre, ws, stats=None, grads=None, rows=None, stream=None):
    """The head's backward (gm_sn_head_bwd): dPre = ds w2bar . [H > 0]; critic mode: grads = (gw2, gb2) receive d loss / d
    w2 = (g - <g, w2bar> w2bar) / ||w2|| with g = sum ds h, and d loss / d b2 (stats: sn_power_iter's)."""
    a = _sn_head_args(H, w2bar, B, gen_mode, ds, ws, rows)
    if dPre.dim() != 2 or dPre.shape[0] < a.rows or dPre.shape[1] != a.Hd:
        raise _lib.GMError("sn_head_bwd: dPre must be [>= rows, Hd]")
    a.dPre, a.ldp = dPre.data_ptr(), _ld(dPre)
    if grads is not None:
        gw2, gb2 = grads
        if gw2.numel() != a.Hd or gb2.numel() != 1 or not gw2.is_contiguous() or stats is None:
            raise _lib.GMError("sn_head_bwd: grads must be (gw2 [Hd], gb2 [1]) with the power stage's stats")
        a.gw2, a.gb2, a.stats = gw2.data_ptr(), gb2.data_ptr(), stats.data_ptr()
    _lib.call("gm_sn_head_bwd", stream or stream_ptr(), ctypes.byref(a))


def sn_grad(G, Wbar, u, v, stats, gW, ws, stream=None):
    """gW = (G - <G, Wbar> u v^T) / sigma (gm_sn_grad, two launches): G = d loss / d Wbar, u / v / stats the forward's."""
    H, I = Wbar.shape
    _sn_w_shape(H, I)
    if (tuple(G.shape) != (H, I) or gW.numel() != H * I or u.numel() != H or v.numel() != I
            or not (G.is_contiguous() and Wbar.is_contiguous() and gW.is_contiguous())):
        raise _lib.GMError("sn_grad: G, Wbar and gW must be contiguous [H, I], u [H], v [I]")
    a = SNGradArgs()
    a.G, a.Wbar, a.H, a.I, a.u, a.v = G.data_ptr(), Wbar.data_ptr(), H, I, u.data_ptr(), v.data_ptr()
    a.stats, a.gW, a.ws, a.ws_bytes = stats.data_ptr(), gW.data_ptr(), ws.data_ptr(), ws.numel() * 4
    _lib.call("gm_sn_grad", stream or stream_ptr(), ctypes.byref(a))


# ---- Bayesian GAN (csrc/gm_bgan.hip; bgan.py) ----------------------------------------------------------------------
def bgan_stream_param(side, k, tensor):
    """The noise stream word of tensor `tensor` (0 linear.weight, 1 linear.bias, 2 second weight, 3 second bias) of
    sample k on `side` (0 critics, 1 generators)."""
    return 0x10000 | (side << 12) | (k << 4) | tensor


def bgan_stream_latent(phase, j):
    """The stream word of generator j's latent draw in phase 0 (critic update) or 1 (generator update)."""
    return 0x20000 | (phase << 12) | (j << 4)


def _u32(t, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()):
        raise _lib.GMError("%s must be a contiguous int32 device tensor" % name)
    return t


def philox_raw(ctr, key, stream=None):
    """Philox4x32-10 words for n (counter, key) pairs: ctr int32 [n, 4], key int32 [n, 2] (bit patterns) ->
    int32 [n, 4]."""
    n = ctr.shape[0]
    if ctr.shape != (n, 4) or key.shape != (n, 2):
        raise _lib.GMError("philox_raw: ctr must be [n, 4] and key [n, 2]")
    out = torch.empty(n, 4, dtype=torch.int32, device=ctr.device)
    _lib.call("gm_philox_raw", stream or stream_ptr(), _u32(ctr, "ctr").data_ptr(), _u32(key, "key").data_ptr(),
              out.data_ptr(), n)
    return out


def philox_normal(seed, stream_word, t, n, out=None, nstreams=1, stream_stride=0, step=None, device=None,
                  stream=None):
    """nstreams draws of n normals (gm_philox_normal): out[j, e] = Normal(seed, stream_word + j stream_stride,
    step) element e, with step = (*step if step is a device int64 tensor else 0) + t."""
    if out is None:
        out = torch.empty(nstreams, n, device=device or "cuda")
    if not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= nstreams * n):
        raise _lib.GMError("philox_normal: out must be a contiguous float32 device tensor of >= %d elements"
                           % (nstreams * n))
    if step is not None and not (step.is_cuda and step.dtype == torch.int64):
        raise _lib.GMError("philox_normal: step must be an int64 device tensor")
    _lib.call("gm_philox_normal", stream or stream_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, stream_word & 0xFFFFFFFF,
              stream_stride & 0xFFFFFFFF, nstreams, step.data_ptr() if step is not None else None, int(t),
              out.data_ptr(), n)
    return out


def sghmc_segments(segs):
    """A host segment table from (offset, numel, stream word) triples."""
    arr = (_lib.SghmcSeg * len(segs))()
    for a, (o, n, s) in zip(arr, segs):
        a.offset, a.numel, a.stream = int(o), int(n), int(s) & 0xFFFFFFFF
    return arr


def sghmc_step(theta, grad, mom, segs, lr, friction, prior, noise, seed, t=0, step=None, stream=None):
    """One SGHMC step (gm_sghmc_step) over the flat fp32 buffers theta / grad / mom: segs is a table of
    sghmc_segments, lr a device float32 tensor (eta in lr[0]), step a device int64 counter (or None) added to t."""
    for x, nm in ((theta, "theta"), (grad, "grad"), (mom, "mom")):
        if not (x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.numel() == theta.numel()):
            raise _lib.GMError("sghmc_step: %s must be a contiguous float32 device tensor like theta" % nm)
    if not (lr.is_cuda and lr.dtype == torch.float32):
        raise _lib.GMError("sghmc_step: lr must be a float32 device tensor")
    if step is not None and not (step.is_cuda and step.dtype == torch.int64):
        raise _lib.GMError("sghmc_step: step must be an int64 device tensor")
    if not isinstance(segs, ctypes.Array):
        segs = sghmc_segments(segs)
    a = _lib.SghmcArgs(theta.data_ptr(), grad.data_ptr(), mom.data_ptr(), theta.numel(), segs, len(segs),
                       step.data_ptr() if step is not None else None, int(t), lr.data_ptr(), friction, prior, noise,
                       int(seed) & 0xFFFFFFFFFFFFFFFF)
    _lib.call("gm_sghmc_step", stream or stream_ptr(), ctypes.byref(a))


def bgan_head_workspace(mode, B, Jg, Jd, H, device):
    n = _lib.load().gm_bgan_head_workspace_bytes(mode, B, Jg, Jd, H)
    if n < 0:
        raise _lib.GMError("bgan_head: shape (B=%d, Jg=%d, Jd=%d, H=%d) outside the kernel's limits" % (B, Jg, Jd, H))
    return torch.empty((n + 3) // 4, device=device)


def bgan_head(h, w2, b2, mode, B, Jg, Jd, ws, gw2=None, gb2=None, loss_out=None, loss_slot=NO_SLOT, stream=None):
    """The critic ensemble's head (gm_bgan_head) over h [R, Jd H] (dH written over it): mode 0 = critic update,
    mode 1 = generator update."""
    H = w2.numel() // Jd
    R = (1 + Jg) * B if mode == 0 else Jg * B
    if h.dim() != 2 or h.shape[0] < R or h.shape[1] != Jd * H or h.stride(1) != 1 or w2.numel() != Jd * H \
            or b2.numel() != Jd:
        raise _lib.GMError("bgan_head: h must be [>= %d, %d], w2 [%d, H], b2 [%d]" % (R, Jd * H, Jd, Jd))
    ptr = lambda x: x.data_ptr() if x is not None else None
    a = _lib.BganHeadArgs(h.data_ptr(), h.stride(0), w2.data_ptr(), b2.data_ptr(), ptr(gw2), ptr(gb2), ptr(loss_out),
                          loss_slot, ws.data_ptr(), ws.numel() * 4, mode, B, Jg, Jd, H)
    _lib.call("gm_bgan_head", stream or stream_ptr(), ctypes.byref(a))


# ---- The device noise clock and seed (csrc/gm_philox.h) --------------------------------------
def _clock(who, step, step_ctr, step_base):
    """(step_ctr's pointer, step_base's pointer, int(step)) of a noise block whose step is *step_ctr + *step_base +
    step: each tensor an int64 device tensor, or None for 0.  Checked before anything is launched: a tensor of another
    dtype or on the host would be read as raw memory."""
    for t, nm in ((step_ctr, "step_ctr"), (step_base, "step_base")):
        if t is not None and not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.int64):
            raise _lib.GMError("%s: %s must be an int64 device tensor or None" % (who, nm))
    ptr = lambda t: t.data_ptr() if t is not None else None
    return ptr(step_ctr), ptr(step_base), int(step)


def _seed64(who, seed):
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise _lib.GMError("%s: seed must lie in [0, 2^64)" % who)
    return seed


# ---- Denoising VAE (csrc/gm_dvae.hip, gm_dvae.h; dvae.py) ---------------------------------------------------------
def corrupt_args(noise, level, seed, step=0, step_ctr=None, step_base=None, row0=0):
    """A gm_corrupt_args block: noise "salt_pepper" / "gaussian" (or a GM_NOISE_* int), its level, the seed
    (0 <= seed < 2^64) and the training-batch step = *step_ctr + *step_base + step (int64 device tensors, or None for
    0).  The tensors must outlive every launch (and every captured graph) that reads them."""
    kind = _lib.NOISE[noise] if isinstance(noise, str) else int(noise)
    return _lib.CorruptArgs(kind, float(level), _seed64("corrupt_args", seed),
                            *_clock("corrupt_args", step, step_ctr, step_base), int(row0))


def _rows2d(x, name):
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1):
        raise _lib.GMError("%s must be a 2-D float32 device tensor with contiguous rows" % name)
    return x


def dvae_corrupt(x, args, out=None, stream=None):
    """out[r] = the corruption of row r of x (gm_dvae_corrupt; row r is batch position args.row0 + r).  out=None: a
    new tensor; out may be x itself."""
    _rows2d(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _rows2d(out, "out")
    if tuple(out.shape) != tuple(x.shape):
        raise _lib.GMError("dvae_corrupt: out %s does not match x %s" % (tuple(out.shape), tuple(x.shape)))
    _lib.call("gm_dvae_corrupt", stream or stream_ptr(), ctypes.byref(args), x.data_ptr(), x.stride(0),
              out.data_ptr(), out.stride(0), x.shape[0], x.shape[1])
    return out


def _corrupt_out(out, out_c):
    _rows2d(out_c, "out_c")
    if _ld(out_c) != _ld(out) or out_c.shape[1] != out.shape[1]:
        raise _lib.GMError("the corrupted rows must have the clean rows' shape and row stride")


def gather_rows_corrupt(data, idx, out, out_c, args, B=None, idx_slot=NO_SLOT, stream=None):
    """ops.gather_rows(data, idx, out) that also writes the corrupted rows to out_c (gm_gather_rows[_bits]_corrupt)."""
    from .ops import PackedData
    n_rows, row = data.shape
    B = out.shape[0] if B is None else B
    if not (idx.dtype == torch.int64 and idx.is_cuda):
        raise _lib.GMError("gather_rows_corrupt: idx must be an int64 device tensor")
    _rows2d(out, "out")
    _corrupt_out(out, out_c)
    if isinstance(data, PackedData):
        _lib.call("gm_gather_rows_bits_corrupt", stream or stream_ptr(), ctypes.byref(args), data.data_ptr(), data.wpr,
                  n_rows, idx.data_ptr(), idx_slot, out.data_ptr(), out_c.data_ptr(), _ld(out), B, row)
    else:
        _lib.call("gm_gather_rows_corrupt", stream or stream_ptr(), ctypes.byref(args), _rows2d(data, "data").data_ptr(),
                  n_rows, idx.data_ptr(), idx_slot, out.data_ptr(), out_c.data_ptr(), _ld(out), B, row)
    return out


def linear_fwd_gather_corrupt(x, W, b, y, act, data, idx, out, out_c, args, M=None, B=None, x_slot=NO_SLOT,
                              idx_slot=NO_SLOT, stream=None):
    """ops.linear_fwd_gather with the corrupting gather riding in the GEMM's grid (gm_gather_args.corrupt / out_c):
    out gets the clean rows, out_c their corruption; neither may be an operand of this GEMM."""
    from .ops import PackedData, _fwd_args, _fwd_ex, _gather_args
    _rows2d(out, "out")
    _corrupt_out(out, out_c)
    if not isinstance(data, PackedData):
        _rows2d(data, "data")
    a = _fwd_args(x, W, b, y, act, M, x_slot)
    g = _gather_args(data, idx, out, B, idx_slot)
    g.corrupt, g.out_c = ctypes.pointer(args), out_c.data_ptr()
    a.gather = ctypes.pointer(g)
    _fwd_ex(a, stream)
    return y


# ---- Primal-Dual Wasserstein GAN (csrc/gm_pdw.hip; pdwgan.py) -----------------------------------------------------
def pdw_couple(x, xr, share, B, inv_b=None, n=None, t=None, t_slot=NO_SLOT, dA=None, xhat=None, xcopy=None,
               stream=None):
    """The primal coupling of B image rows x with their reconstructions xr (gm_pdw_couple): share[b] = ||x_b - xr_b||
    * inv_b (inv_b: 1 / B by default), n[b] the norm itself, dA = d share / d (pre-sigmoid xr), xhat = t x + (1 - t)
    xr with t the t_slot row of the uniform ring, xcopy = x.  n, dA, xhat (with t) and xcopy are optional."""
    I = x.shape[1]
    for a, nm in ((x, "x"), (xr, "xr"), (dA, "dA"), (xhat, "xhat"), (xcopy, "xcopy")):
        if a is not None and (_rows2d(a, nm).shape[0] < B or a.shape[1] != I):
            raise _lib.GMError("pdw_couple: %s must be [>= %d, %d], got %s" % (nm, B, I, tuple(a.shape)))
    if share.numel() < B or (n is not None and n.numel() < B) or (xhat is not None and t is None):
        raise _lib.GMError("pdw_couple: share / n hold one float per row, and xhat needs t")
    if inv_b is None:
        import numpy as np
        inv_b = float(np.float32(1.0) / np.float32(B))
    p = lambda a: a.data_ptr() if a is not None else None
    ld = lambda a: _ld(a) if a is not None else 0
    _lib.call("gm_pdw_couple", stream or stream_ptr(), x.data_ptr(), _ld(x), xr.data_ptr(), _ld(xr), p(t), t_slot,
              p(n), share.data_ptr(), p(dA), ld(dA), p(xhat), ld(xhat), p(xcopy), ld(xcopy), inv_b, B, I)


def pdw_dir(g, x, xr, n, gamma, pen, lam, inv_b, stream=None):
    """PD-WGAN's direction penalty in gp_norm's place (gm_pdw_dir): pen[b] = ||g_b - d_b||^2 and gamma_b = lam * inv_b
    * 2 (g_b - d_b) with d_b = (x_b - xr_b) / n_b (0 where n_b == 0); the row count is g's."""
    B, I = g.shape
    for a, nm in ((g, "g"), (x, "x"), (xr, "xr"), (gamma, "gamma")):
        if _rows2d(a, nm).shape[0] < B or a.shape[1] != I:
            raise _lib.GMError("pdw_dir: %s must be [>= %d, %d], got %s" % (nm, B, I, tuple(a.shape)))
    if n.numel() < B or pen.numel() < B:
        raise _lib.GMError("pdw_dir: n and pen hold one float per row")
    _lib.call("gm_pdw_dir", stream or stream_ptr(), g.data_ptr(), _ld(g), x.data_ptr(), _ld(x), xr.data_ptr(), _ld(xr),
              n.data_ptr(), gamma.data_ptr(), _ld(gamma), pen.data_ptr(), lam, inv_b, B, I)


# ---- Importance-weighted autoencoder (csrc/gm_iwae.hip; iwae.py) ---------------------------------------------------
def iwae_noise(seed, tag, k_total, j0=0, step=0, step_ctr=None, step_base=None, q0=0):
    """A gm_iwae_noise block: the stream (seed, tag) at step = *step_ctr + *step_base + step (int64 device tensors, or
    None for 0); the call's sample j of image b draws noise row b * k_total + j0 + j.  The tensors must outlive every
    launch (and every captured graph) that reads them."""
    return IwaeNoise(_seed64("iwae_noise", seed), int(tag) & 0xFFFFFFFF,
                     *_clock("iwae_noise", step, step_ctr, step_base), int(k_total), int(j0), int(q0))


def iwae_sample(ml, z, lp, noise, B, k, Z, stream=None):
    """z [B k, Z] and lp [B k] of the k samples of each of B images from ml [B, 2Z] (gm_iwae_sample)."""
    if _rows2d(ml, "ml").shape[0] < B or ml.shape[1] < 2 * Z or _rows2d(z, "z").shape[0] < B * k or z.shape[1] < Z \
            or lp.numel() < B * k or not lp.is_contiguous():
        raise _lib.GMError("iwae_sample: ml %s / z %s / lp %s do not fit B=%d, k=%d, Z=%d"
                           % (tuple(ml.shape), tuple(z.shape), tuple(lp.shape), B, k, Z))
    _lib.call("gm_iwae_sample", stream or stream_ptr(), ctypes.byref(noise), ml.data_ptr(), _ld(ml), z.data_ptr(),
              _ld(z), lp.data_ptr(), B, k, Z)


def iwae_weights(x, xr, lp, negL, ess, wn, B, k, dA=None, ms=None, stream=None):
    """Per image: -L_k, ess, the normalised weights wn [B k] and, with dA [B k, I], the weighted gradient at the
    decoder's pre-sigmoid output; ms [B, 2] takes (max, sum) of exp(log w - max) (gm_iwae_weights)."""
    I = x.shape[1]
    if _rows2d(x, "x").shape[0] < B or _rows2d(xr, "xr").shape[0] < B * k or xr.shape[1] != I \
            or min(lp.numel(), wn.numel()) < B * k or min(negL.numel(), ess.numel()) < B \
            or (dA is not None and (_rows2d(dA, "dA").shape[0] < B * k or dA.shape[1] != I)) \
            or (ms is not None and (ms.numel() < 2 * B or not ms.is_contiguous())):
        raise _lib.GMError("iwae_weights: the arrays do not fit B=%d, k=%d, I=%d" % (B, k, I))
    for t in (lp, negL, ess, wn):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.GMError("iwae_weights: lp, negL, ess and wn must be contiguous float32 device tensors")
    _lib.call("gm_iwae_weights", stream or stream_ptr(), x.data_ptr(), _ld(x), xr.data_ptr(), _ld(xr), lp.data_ptr(),
              negL.data_ptr(), ess.data_ptr(), wn.data_ptr(), dA.data_ptr() if dA is not None else None,
              _ld(dA) if dA is not None else 0, ms.data_ptr() if ms is not None else None, B, k, I)


def iwae_reduce(ml, wn, dzdec, dml, noise, B, k, Z, dZ=None, stream=None):
    """d loss / d [mu | lv] -> dml [B, 2Z] from dzdec [B k, Z] = dHdec Wd1 and the weights (gm_iwae_reduce); dZ [B k, Z]
    takes d loss / d z when given."""
    if _rows2d(ml, "ml").shape[0] < B or ml.shape[1] < 2 * Z or _rows2d(dzdec, "dzdec").shape[0] < B * k \
            or dzdec.shape[1] < Z or _rows2d(dml, "dml").shape[0] < B or dml.shape[1] < 2 * Z or wn.numel() < B * k \
            or (dZ is not None and (_rows2d(dZ, "dZ").shape[0] < B * k or dZ.shape[1] < Z)):
        raise _lib.GMError("iwae_reduce: the arrays do not fit B=%d, k=%d, Z=%d" % (B, k, Z))
    _lib.call("gm_iwae_reduce", stream or stream_ptr(), ctypes.byref(noise), ml.data_ptr(), _ld(ml), wn.data_ptr(),
              dzdec.data_ptr(), _ld(dzdec), dml.data_ptr(), _ld(dml), dZ.data_ptr() if dZ is not None else None,
              _ld(dZ) if dZ is not None else 0, B, k, Z)


def iwae_normals(n_images, k, Z, seed, step, tag, device="cuda"):
    """eps [n_images k, Z]: the normals gm_iwae_sample draws for (seed, step, tag), through gm_iwae_sample itself
    on mu = 0, log_var = 0 (z = 0 + eps * exp(0) = eps, bit for bit).  k or Z above the fused limits go in pieces of 64
    samples by 32 latents.  What the general path's compute_batch feeds its reparameterisation."""
    MK, MZ = _lib.IWAE_MAX_K, _lib.IWAE_MAX_Z
    ml = torch.zeros(n_images, 2 * min(Z, MZ), device=device)
    out = torch.empty(n_images, k, Z, device=device)
    for j0 in range(0, k, MK):
        kc = min(MK, k - j0)
        for c0 in range(0, Z, MZ):
            zc = min(MZ, Z - c0)
            z = torch.empty(n_images * kc, zc, device=device)
            lp = torch.empty(n_images * kc, device=device)
            iwae_sample(ml[:, :2 * zc], z, lp, iwae_noise(seed, tag, k, j0=j0, step=step, q0=c0 // 4), n_images, kc, zc)
            out[:, j0:j0 + kc, c0:c0 + zc] = z.view(n_images, kc, zc)
    return out.view(n_images * k, Z)


# ---- beta-TCVAE (csrc/gm_tc.hip; tcvae.py) -------------------------------------------------------------------------
def _tc_vec(t, n, who, name):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            and t.numel() >= n):
        raise _lib.GMError("%s: %s must be a contiguous float32 device tensor of at least %d values" % (who, name, n))
    return t


def tc_records(B, Z, device="cuda"):
    """(lse_joint [B], lse_dim [B, Z], tc [B]): what tc_sample leaves for tc_reduce and for the batch's second sum."""
    z = lambda *s: torch.zeros(*s, device=device)
    return z(B), z(B, Z), z(B)


def tc_sample(ml, z, lp, lse_joint, lse_dim, tc, noise, alpha, beta, gamma, log_nm, B, Z, terms=None, stream=None):
    """z [B, Z], lp [B], the two logsumexp records, the tc row and (given) terms [B, 3] = (mi, tc, dwkl) of B images at
    k = 1 from ml [B, 2Z] (gm_tc_sample); noise: an iwae_noise block with k_total = 1; log_nm = log(N B)."""
    if _rows2d(ml, "ml").shape[0] < B or ml.shape[1] < 2 * Z or _rows2d(z, "z").shape[0] < B or z.shape[1] < Z \
            or _rows2d(lse_dim, "lse_dim").shape[0] < B or lse_dim.shape[1] < Z:
        raise _lib.GMError("tc_sample: ml %s / z %s / lse_dim %s do not fit B=%d, Z=%d"
                           % (tuple(ml.shape), tuple(z.shape), tuple(lse_dim.shape), B, Z))
    for t, nm in ((lp, "lp"), (lse_joint, "lse_joint"), (tc, "tc")):
        _tc_vec(t, B, "tc_sample", nm)
    if terms is not None:
        _tc_vec(terms, 3 * B, "tc_sample", "terms")
    _lib.call("gm_tc_sample", stream or stream_ptr(), ctypes.byref(noise), ml.data_ptr(), _ld(ml), z.data_ptr(), _ld(z),
              lp.data_ptr(), lse_joint.data_ptr(), lse_dim.data_ptr(), _ld(lse_dim), tc.data_ptr(),
              terms.data_ptr() if terms is not None else None, float(alpha), float(beta), float(gamma), float(log_nm),
              B, 1, Z)


def tc_reduce(ml, z, lse_joint, lse_dim, wn, dzdec, dml, noise, alpha, beta, gamma, B, Z, stream=None):
    """d loss / d [mu | lv] -> dml [B, 2Z] from tc_sample's z and records, the weights wn [B] and dzdec [B, Z] = dHdec
    Wd1 (gm_tc_reduce); noise: tc_sample's block."""
    for t, w, nm in ((ml, 2 * Z, "ml"), (z, Z, "z"), (lse_dim, Z, "lse_dim"), (dzdec, Z, "dzdec"), (dml, 2 * Z, "dml")):
        if _rows2d(t, nm).shape[0] < B or t.shape[1] < w:
            raise _lib.GMError("tc_reduce: %s %s does not fit B=%d, Z=%d" % (nm, tuple(t.shape), B, Z))
    for t, nm in ((lse_joint, "lse_joint"), (wn, "wn")):
        _tc_vec(t, B, "tc_reduce", nm)
    _lib.call("gm_tc_reduce", stream or stream_ptr(), ctypes.byref(noise), ml.data_ptr(), _ld(ml), z.data_ptr(), _ld(z),
              lse_joint.data_ptr(), lse_dim.data_ptr(), _ld(lse_dim), wn.data_ptr(), dzdec.data_ptr(), _ld(dzdec),
              dml.data_ptr(), _ld(dml), float(alpha), float(beta), float(gamma), B, 1, Z)


# ---- Planar-flow posterior of the normalizing-flow VAE (csrc/gm_flow.hip; nfvae.py) --------------------------------
def flow_params(u, w, b):
    """A gm_flow_params block over u [K, Z], w [K, Z], b [K] (contiguous float32 device tensors that outlive every
    launch and captured graph reading them)."""
    K, Z = u.shape
    for t, nm, shp in ((u, "u", (K, Z)), (w, "w", (K, Z)), (b, "b", (K,))):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == shp):
            raise _lib.GMError("flow_params: %s must be a contiguous float32 device tensor of shape %s, got %s"
                               % (nm, shp, tuple(t.shape)))
    return FlowParams(u.data_ptr(), w.data_ptr(), b.data_ptr(), K)


def flow_parts(B, K, device="cuda"):
    """The partial-gradient buffer flow_reduce fills and flow_step sums: ceil(B / 8) blocks of [K, 68] floats."""
    return torch.zeros((B + 7) // 8, K, _lib.FLOW_PART_STRIDE, device=device)


def flow_sample(ml, z, lp, noise, flow, B, k, Z, stream=None):
    """z_K [B k, Z] and lp [B k] of the k samples of each of B images from ml [B, 2Z] through the planar chain
    `flow` (a flow_params block) (gm_flow_sample)."""
    if _rows2d(ml, "ml").shape[0] < B or ml.shape[1] < 2 * Z or _rows2d(z, "z").shape[0] < B * k or z.shape[1] < Z \
            or lp.numel() < B * k or not lp.is_contiguous():
        raise _lib.GMError("flow_sample: ml %s / z %s / lp %s do not fit B=%d, k=%d, Z=%d"
                           % (tuple(ml.shape), tuple(z.shape), tuple(lp.shape), B, k, Z))
    _lib.call("gm_flow_sample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(flow), ml.data_ptr(), _ld(ml),
              z.data_ptr(), _ld(z), lp.data_ptr(), B, k, Z)


def flow_reduce(ml, wn, dzdec, dml, part, noise, flow, B, k, Z, stream=None):
    """d loss / d [mu | lv] -> dml [B, 2Z] and the flow parameters' partial gradient blocks -> part (flow_parts) from
    dzdec [B k, Z] = dHdec Wd1 and the weights wn [B k] (gm_flow_reduce)."""
    if _rows2d(ml, "ml").shape[0] < B or ml.shape[1] < 2 * Z or _rows2d(dzdec, "dzdec").shape[0] < B * k \
            or dzdec.shape[1] < Z or _rows2d(dml, "dml").shape[0] < B or dml.shape[1] < 2 * Z or wn.numel() < B * k \
            or not part.is_contiguous() or part.numel() < (B + 7) // 8 * flow.K * _lib.FLOW_PART_STRIDE:
        raise _lib.GMError("flow_reduce: the arrays do not fit B=%d, k=%d, Z=%d, K=%d" % (B, k, Z, flow.K))
    _lib.call("gm_flow_reduce", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(flow), ml.data_ptr(), _ld(ml),
              wn.data_ptr(), dzdec.data_ptr(), _ld(dzdec), dml.data_ptr(), _ld(dml), part.data_ptr(), B, k, Z)


def flow_step(part, B, u, w, b, moments, sched, sched_slot=NO_SLOT, grads=None, betas=(0.9, 0.999), eps=1e-8,
              weight_decay=0.0, stream=None):
    """The flow's optimiser step (gm_flow_step): flow_reduce's blocks for a batch of B images summed, the gradients of
    u, w, b formed (and written to grads = (gu, gw, gb) when given) and one Adam step taken at the schedule's slot;
    moments = (mu, vu, mw, vw, mb, vb), laid out like their parameters."""
    K, Z = u.shape
    nparts = (B + 7) // 8
    if len(moments) != 6 or part.numel() < nparts * K * _lib.FLOW_PART_STRIDE or not part.is_contiguous():
        raise _lib.GMError("flow_step: six moment tensors and %d partial blocks are needed" % nparts)
    n = [K * Z, K * Z, K]
    ts = [u, w, b] + list(moments) + (list(grads) if grads is not None else [])
    for t, cnt in zip(ts, n + [K * Z] * 4 + [K, K] + n):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == cnt):
            raise _lib.GMError("flow_step: every tensor must be a contiguous float32 device tensor sized like its "
                               "parameter (K=%d, Z=%d)" % (K, Z))
    g = [t.data_ptr() for t in grads] if grads is not None else [None, None, None]
    a = FlowStepArgs(part.data_ptr(), nparts, u.data_ptr(), w.data_ptr(), b.data_ptr(), g[0], g[1], g[2],
                     *[t.data_ptr() for t in moments], sched.data_ptr(), sched_slot, betas[0], betas[1], eps,
                     weight_decay, K, Z)
    _lib.call("gm_flow_step", stream or stream_ptr(), ctypes.byref(a))


# ---- Inverse-autoregressive-flow posterior of the IAF-VAE (csrc/gm_iaf.hip; iafvae.py) -----------------------------
def _iaf_f32(t, shape, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise _lib.GMError("%s must be a contiguous float32 device tensor of shape %s, got %s"
                           % (what, tuple(shape), tuple(t.shape)))


def iaf_shapes(K, Z, F, C):
    """The shapes of (W1, U, b1, W2, b2); U's is None when C == 0."""
    return (K, F, Z), ((K, F, C) if C else None), (K, F), (K, 2 * Z, F), (K, 2 * Z)


def iaf_params(W1, U, b1, W2, b2):
    """A gm_iaf_params block over the flow's stacked tensors (contiguous float32 device tensors that outlive every launch
    and captured graph reading them); U is None when the flow has no context.  The block carries .Z beside K, F, C."""
    K, F, Z = W1.shape
    C = 0 if U is None else U.shape[2]
    for t, shp, nm in zip((W1, U, b1, W2, b2), iaf_shapes(K, Z, F, C), ("W1", "U", "b1", "W2", "b2")):
        if shp is not None:
            _iaf_f32(t, shp, "iaf_params: " + nm)
    blk = IafParams(W1.data_ptr(), U.data_ptr() if C else None, b1.data_ptr(), W2.data_ptr(), b2.data_ptr(), K, F, C)
    blk.Z = Z
    return blk


def iaf_part_stride(Z, F, C):
    """Floats per layer of a partial block (GM_IAF_PART_STRIDE): [dW1 | dU | db1 | dW2 | db2]."""
    return F * Z + F * C + F + 2 * Z * F + 2 * Z


def iaf_nparts(B, k):
    """Partial blocks of a batch of B images of k samples (GM_IAF_PARTS): a workgroup owns max(1, 64 // k) images."""
    ipw = max(1, _lib.IAF_PART_ROWS // k)
    return (B + ipw - 1) // ipw


def iaf_parts(B, k, K, Z, F, C, device="cuda"):
    """The partial-gradient buffer iaf_reduce fills and iaf_step sums: [iaf_nparts(B, k), K, iaf_part_stride(Z, F, C)]."""
    return torch.zeros(iaf_nparts(B, k), K, iaf_part_stride(Z, F, C), device=device)


def iaf_sample(ml, z, lp, noise, flow, B, k, Z, stream=None):
    """z_K [B k, Z] and lp [B k] of the k samples of each of B images from ml [B, 2Z + C] = [mu | lv | h] through the
    chain `flow` (an iaf_params block) (gm_iaf_sample)."""
    if _rows2d(ml, "ml").shape[0] < B or ml.shape[1] < 2 * Z + flow.C or _rows2d(z, "z").shape[0] < B * k \
            or z.shape[1] < Z or lp.numel() < B * k or not lp.is_contiguous() or flow.Z != Z:
        raise _lib.GMError("iaf_sample: ml %s / z %s / lp %s do not fit B=%d, k=%d, Z=%d, C=%d"
                           % (tuple(ml.shape), tuple(z.shape), tuple(lp.shape), B, k, Z, flow.C))
    _lib.call("gm_iaf_sample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(flow), ml.data_ptr(), _ld(ml),
              z.data_ptr(), _ld(z), lp.data_ptr(), B, k, Z)


def iaf_reduce(ml, wn, dzdec, dml, part, noise, flow, B, k, Z, stream=None):
    """d loss / d [mu | lv | h] -> dml [B, 2Z + C] and the flow parameters' partial gradient blocks -> part (iaf_parts)
    from dzdec [B k, Z] = dHdec Wd1 and the weights wn [B k] (gm_iaf_reduce)."""
    W = 2 * Z + flow.C
    if _rows2d(ml, "ml").shape[0] < B or ml.shape[1] < W or _rows2d(dzdec, "dzdec").shape[0] < B * k \
            or dzdec.shape[1] < Z or _rows2d(dml, "dml").shape[0] < B or dml.shape[1] < W or wn.numel() < B * k \
            or not wn.is_contiguous() or not part.is_contiguous() or flow.Z != Z \
            or part.numel() < iaf_nparts(B, k) * flow.K * iaf_part_stride(Z, flow.F, flow.C):
        raise _lib.GMError("iaf_reduce: the arrays do not fit B=%d, k=%d, Z=%d, K=%d, F=%d, C=%d"
                           % (B, k, Z, flow.K, flow.F, flow.C))
    _lib.call("gm_iaf_reduce", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(flow), ml.data_ptr(), _ld(ml),
              wn.data_ptr(), dzdec.data_ptr(), _ld(dzdec), dml.data_ptr(), _ld(dml), part.data_ptr(), B, k, Z)


def iaf_step(part, B, k, params, m_in, moments, sched, sched_slot=NO_SLOT, grads=None, betas=(0.9, 0.999), eps=1e-8,
             weight_decay=0.0, stream=None):
    """The flow's optimiser step (gm_iaf_step): iaf_reduce's blocks for a batch of B images of k samples summed, masked
    entries left alone, the gradients written to grads when given, and one Adam step taken at the schedule's slot.
    params = (W1, U, b1, W2, b2) with U None when C == 0; moments = ((m, v) per parameter, in that order, None for a
    missing U); grads likewise; m_in [K, Z] int32 on the device."""
    W1, U = params[0], params[1]
    K, F, Z = W1.shape
    C = 0 if U is None else U.shape[2]
    shapes = iaf_shapes(K, Z, F, C)
    nparts = iaf_nparts(B, k)
    if part.numel() < nparts * K * iaf_part_stride(Z, F, C) or not part.is_contiguous():
        raise _lib.GMError("iaf_step: %d partial blocks are needed" % nparts)
    if not (m_in.is_cuda and m_in.dtype == torch.int32 and m_in.is_contiguous() and tuple(m_in.shape) == (K, Z)):
        raise _lib.GMError("iaf_step: m_in must be a contiguous int32 device tensor of shape %s" % ((K, Z),))
    arr = lambda: (ctypes.c_void_p * 5)()
    ap, ag, am, av = arr(), arr(), arr(), arr()
    for t, shp in enumerate(shapes):
        if shp is None:
            continue
        n = params[t].numel()
        _iaf_f32(params[t], shp, "iaf_step: a parameter")
        ap[t] = params[t].data_ptr()
        for dst, src in ((am, moments[t][0]), (av, moments[t][1])) + (((ag, grads[t]),) if grads is not None else ()):
            if not (src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and src.numel() == n):
                raise _lib.GMError("iaf_step: every moment and gradient must be a contiguous float32 device tensor "
                                   "sized like its parameter")
            dst[t] = src.data_ptr()
    a = IafStepArgs(part.data_ptr(), nparts, ap, ag, am, av, m_in.data_ptr(), sched.data_ptr(), sched_slot, betas[0],
                    betas[1], eps, weight_decay, K, Z, F, C)
    _lib.call("gm_iaf_step", stream or stream_ptr(), ctypes.byref(a))


# ---- Gumbel-Softmax posterior of the categorical VAE (csrc/gm_cat.hip; catvae.py) ----------------------------------
def _cat_f32(t, name):
    if not (t.is_cuda and t.dtype == torch.float32):
        raise _lib.GMError("%s must be a float32 device tensor (got %s on %s)" % (name, t.dtype, t.device))
    return t


def _cat_tau(a, tau, tau_tab, tau_slot):
    if tau_tab is not None:
        if not (tau_tab.is_cuda and tau_tab.dtype == torch.float32 and tau_tab.is_contiguous()):
            raise _lib.GMError("the temperature table must be a contiguous float32 device tensor")
        a.tau_tab, a.tau_slot = tau_tab.data_ptr(), tau_slot
    elif tau is not None:
        a.tau = float(tau)


def cat_sample(logits, y, lp, noise, B, k, N, C, mode, tau=None, tau_tab=None, tau_slot=NO_SLOT, kl=None, codes=None,
               stream=None):
    """The decoder's input y [B k, N C], lp [B k] and (kl [B], codes [B k, N] int32) of the k samples of each of B
    images from logits [B, N C] (gm_cat_sample).  mode: _lib.CAT_RELAXED (reads tau, a float, or tau_tab at tau_slot),
    CAT_ST, CAT_DISCRETE (needs codes) or CAT_NOISE (y = the Gumbel noise; logits and lp may be None)."""
    W = N * C
    a = CatArgs()
    if _rows2d(_cat_f32(y, "y"), "y").shape[0] < B * k or y.shape[1] < W:
        raise _lib.GMError("cat_sample: y %s does not fit B=%d, k=%d, N=%d, C=%d" % (tuple(y.shape), B, k, N, C))
    if mode != _lib.CAT_NOISE:
        if logits is None or lp is None or _rows2d(_cat_f32(logits, "logits"), "logits").shape[0] < B \
                or logits.shape[1] < W or _cat_f32(lp, "lp").numel() < B * k or not lp.is_contiguous():
            raise _lib.GMError("cat_sample: logits / lp do not fit B=%d, k=%d, N=%d, C=%d" % (B, k, N, C))
        a.logits, a.ldl, a.lp = logits.data_ptr(), _ld(logits), lp.data_ptr()
        if kl is not None:
            if _cat_f32(kl, "kl").numel() < B or not kl.is_contiguous():
                raise _lib.GMError("cat_sample: kl holds one float per image")
            a.kl = kl.data_ptr()
    if codes is not None:
        if not (codes.is_cuda and codes.dtype == torch.int32 and codes.is_contiguous() and codes.numel() >= B * k * N):
            raise _lib.GMError("cat_sample: codes must be a contiguous int32 device tensor of B k N elements")
        a.codes = codes.data_ptr()
    a.y, a.ldy = y.data_ptr(), _ld(y)
    a.B, a.k, a.N, a.C, a.mode = B, k, N, C, int(mode)
    _cat_tau(a, tau, tau_tab, tau_slot)
    _lib.call("gm_cat_sample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(a))


def cat_reduce(logits, dzdec, wn, dlogits, noise, B, N, C, tau=None, tau_tab=None, tau_slot=NO_SLOT, stream=None):
    """d loss / d logits -> dlogits [B, N C] from dzdec [B, N C] = d loss / d (decoder input) and wn [B], the Gumbel
    noise regenerated (gm_cat_reduce; the backward of CAT_RELAXED and of CAT_ST alike, k = 1)."""
    W = N * C
    for t, nm in ((logits, "logits"), (dzdec, "dzdec"), (dlogits, "dlogits")):
        if _rows2d(_cat_f32(t, nm), nm).shape[0] < B or t.shape[1] < W:
            raise _lib.GMError("cat_reduce: %s %s does not fit B=%d, N=%d, C=%d" % (nm, tuple(t.shape), B, N, C))
    if _cat_f32(wn, "wn").numel() < B or not wn.is_contiguous():
        raise _lib.GMError("cat_reduce: wn holds one float per image")
    a = CatArgs()
    a.logits, a.ldl = logits.data_ptr(), _ld(logits)
    a.dzdec, a.lddz, a.wn = dzdec.data_ptr(), _ld(dzdec), wn.data_ptr()
    a.dlogits, a.lddl = dlogits.data_ptr(), _ld(dlogits)
    a.B, a.k, a.N, a.C, a.mode = B, 1, N, C, _lib.CAT_RELAXED
    _cat_tau(a, tau, tau_tab, tau_slot)
    _lib.call("gm_cat_reduce", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(a))


def catvae_gumbels(n_images, k, N, C, seed, step, tag, device="cuda"):
    """g [n_images k, N C]: the Gumbel noise gm_cat_sample draws for (seed, step, tag), through gm_cat_sample's NOISE
    mode, bit for bit.  The noise of a row depends on the element's index alone, so any N, C and k go in pieces of 64
    samples by 1024 elements (each piece a launch over 256 "variables" of 4 "classes").  What the tests and the general
    path's compute_batch feed the relaxation."""
    W, MK, MW = N * C, _lib.IWAE_MAX_K, _lib.CAT_MAX_NC
    out = torch.empty(n_images, k, W, device=device)
    for j0 in range(0, k, MK):
        kc = min(MK, k - j0)
        for e0 in range(0, W, MW):
            nq = (min(MW, W - e0) + 3) // 4
            g = torch.empty(n_images * kc, 4 * nq, device=device)
            cat_sample(None, g, None, iwae_noise(seed, tag, k, j0=j0, step=step, q0=e0 // 4), n_images, kc, nq, 4,
                       _lib.CAT_NOISE)
            w = min(MW, W - e0)
            out[:, j0:j0 + kc, e0:e0 + w] = g.view(n_images, kc, 4 * nq)[:, :, :w]
    return out.view(n_images * k, W)


# ---- Vector quantisation of the VQ-VAE (csrc/gm_vq.hip; vqvae.py) --------------------------------------------------
def vq_fused_sizes(N, D, K):
    """True iff (num_vars, code_dim, num_codes) fit the quantisation kernels (the GM_VQ_* limits)."""
    return (N >= 1 and _lib.VQ_MIN_D <= D <= _lib.VQ_MAX_D and D % 4 == 0 and N * D <= _lib.VQ_MAX_ND
            and _lib.VQ_MIN_K <= K <= _lib.VQ_MAX_K and K * D <= _lib.VQ_MAX_KD)


def _vq_rows(t, name, rows, width, dtype=torch.float32):
    if not (t.is_cuda and t.dtype == dtype and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= rows
            and t.shape[1] >= width):
        raise _lib.GMError("%s must be a %s device tensor of at least [%d, %d] with unit column stride (got %s %s on %s)"
                           % (name, dtype, rows, width, t.dtype, tuple(t.shape), t.device))
    return t


def _vq_vec(t, name, n, dtype=torch.float32):
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous() and t.numel() >= n):
        raise _lib.GMError("%s must be a contiguous %s device tensor of at least %d elements" % (name, dtype, n))
    return t


def _vq_common(ze, E, codes, beta, B, N, D):
    K = E.shape[0]
    a = VqArgs()
    _vq_rows(ze, "ze", B, N * D), _vq_rows(E, "E", K, D), _vq_rows(codes, "codes", B, N, torch.int32)
    a.ze, a.ldz, a.E, a.lde, a.codes, a.ldc = ze.data_ptr(), _ld(ze), E.data_ptr(), _ld(E), codes.data_ptr(), _ld(codes)
    a.beta, a.B, a.N, a.D, a.K = float(beta), B, N, D, K
    return a


def vq_quantise(ze, E, zq, codes, qerr, lp, beta, B, N, D, stream=None):
    """z_q [B, N D] = E[codes], codes [B, N] int32 (the nearest code of each variable, the lowest index on a tie), qerr
    [B] and lp [B] = -(1 + beta) qerr from ze [B, N D] and the codebook E [K, D] (gm_vq_quantise)."""
    a = _vq_common(ze, E, codes, beta, B, N, D)
    _vq_rows(zq, "zq", B, N * D), _vq_vec(qerr, "qerr", B), _vq_vec(lp, "lp", B)
    a.zq, a.ldq, a.qerr, a.lp = zq.data_ptr(), _ld(zq), qerr.data_ptr(), lp.data_ptr()
    _lib.call("gm_vq_quantise", stream or stream_ptr(), ctypes.byref(a))


def vq_reduce(ze, E, codes, dzdec, wn, dml, beta, B, N, D, stream=None):
    """dml [B, N D] = dzdec + 2 beta wn (ze - E[codes]) (gm_vq_reduce): the decoder's input gradient straight through
    plus the commitment term."""
    a = _vq_common(ze, E, codes, beta, B, N, D)
    _vq_rows(dzdec, "dzdec", B, N * D), _vq_rows(dml, "dml", B, N * D), _vq_vec(wn, "wn", B)
    a.dzdec, a.lddz, a.wn, a.dml, a.lddml = dzdec.data_ptr(), _ld(dzdec), wn.data_ptr(), dml.data_ptr(), _ld(dml)
    _lib.call("gm_vq_reduce", stream or stream_ptr(), ctypes.byref(a))


def vq_step(ze, codes, E, B, N, D, moments=None, sched=None, sched_slot=NO_SLOT, grad=None, nk=None, usage=None,
            betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, stream=None):
    """The codebook's step (gm_vq_step): n_k and s_k of the batch's codes [B, N] and ze [B, N D] in a fixed order, the
    gradient 2 (n_k E_k - s_k) (-> grad [K, D] when given), n_k (-> nk [K] int32; added to usage [K] int32) and, with
    sched and moments = (m, v), one Adam step on E [K, D] at the schedule's slot.  E, the moments and grad are
    contiguous."""
    K = E.shape[0]
    _vq_rows(ze, "ze", B, N * D), _vq_rows(codes, "codes", B, N, torch.int32)
    a = VqStepArgs()
    a.ze, a.ldz, a.codes, a.ldc = ze.data_ptr(), _ld(ze), codes.data_ptr(), _ld(codes)
    if tuple(E.shape) != (K, D):
        raise _lib.GMError("vq_step: E must be [K, %d], got %s" % (D, tuple(E.shape)))
    a.E = _vq_vec(E, "E", K * D).data_ptr()
    if sched is not None:
        if moments is None or len(moments) != 2:
            raise _lib.GMError("vq_step: an Adam step needs moments = (m, v)")
        a.m, a.v = (_vq_vec(t, "moment", K * D).data_ptr() for t in moments)
        a.sched, a.sched_slot = _vq_vec(sched, "sched", 2).data_ptr(), sched_slot
    if grad is not None:
        a.grad = _vq_vec(grad, "grad", K * D).data_ptr()
    if nk is not None:
        a.nk = _vq_vec(nk, "nk", K, torch.int32).data_ptr()
    if usage is not None:
        a.usage = _vq_vec(usage, "usage", K, torch.int32).data_ptr()
    a.beta1, a.beta2, a.eps, a.weight_decay = betas[0], betas[1], eps, weight_decay
    a.B, a.N, a.D, a.K = B, N, D, K
    _lib.call("gm_vq_step", stream or stream_ptr(), ctypes.byref(a))


# ---- Denoising diffusion (csrc/gm_ddpm.hip, gm_ddpm.h; ddpm.py) ----------------------------------------------------
def ddpm_noise(seed, train=True, step=0, step_ctr=None, step_base=None, row0=0):
    """A gm_ddpm_noise block: the training stream (tags DDPT / DDPM) or the validation one (DDPV / DDPW) at step =
    *step_ctr + *step_base + step (int64 device tensors, or None for 0).  The tensors must outlive every launch (and
    every captured graph) that reads them."""
    tags = (_lib.DDPM_TAG_T, _lib.DDPM_TAG_E) if train else (_lib.DDPM_TAG_V, _lib.DDPM_TAG_VE)
    return DdpmNoise(_seed64("ddpm_noise", seed), tags[0], tags[1], *_clock("ddpm_noise", step, step_ctr, step_base),
                     int(row0))


def ddpm_tables(sa, s1, temb):
    """A gm_ddpm_tables block over the model's fp32 device buffers sa [T], s1 [T], temb [T, E]."""
    for t, nm in ((sa, "sa"), (s1, "s1"), (temb, "temb")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.GMError("ddpm_tables: %s must be a contiguous float32 device tensor" % nm)
    T, E = temb.shape
    if sa.numel() != T or s1.numel() != T:
        raise _lib.GMError("ddpm_tables: sa and s1 hold one float per timestep")
    tab = DdpmTables(sa.data_ptr(), s1.data_ptr(), temb.data_ptr(), T, E)
    tab.keep = (sa, s1, temb)
    return tab


def _ddpm_out(xin, eps, t, rows, I, E):
    if _rows2d(xin, "xin").shape[0] < rows or xin.shape[1] < I + E or _rows2d(eps, "eps").shape[0] < rows \
            or eps.shape[1] < I or (t is not None and not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
                                                           and t.numel() >= rows)):
        raise _lib.GMError("ddpm q-sample: xin %s / eps %s / t do not fit %d rows of %d + %d"
                           % (tuple(xin.shape), tuple(eps.shape), rows, I, E))
    return DdpmOut(xin.data_ptr(), _ld(xin), eps.data_ptr(), _ld(eps), t.data_ptr() if t is not None else None)


def ddpm_qsample(x, noise, tables, xin=None, eps=None, t=None, stream=None):
    """(xin, eps, t) of the image rows x [n, I] in [0, 1] (gm_ddpm_qsample): xin [n, I + E] = [x_t | temb[t]], eps
    [n, I] the noise, t [n] int32.  Missing outputs are allocated."""
    n, I = _rows2d(x, "x").shape
    E = tables.E
    xin = torch.empty(n, I + E, device=x.device) if xin is None else xin
    eps = torch.empty(n, I, device=x.device) if eps is None else eps
    t = torch.empty(n, dtype=torch.int32, device=x.device) if t is None else t
    if n:
        o = _ddpm_out(xin, eps, t, n, I, E)
        _lib.call("gm_ddpm_qsample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(tables), ctypes.byref(o),
                  x.data_ptr(), x.stride(0), n, I)
    return xin, eps, t


def gather_rows_qsample(data, idx, out, xin, eps, t, noise, tables, B=None, idx_slot=NO_SLOT, stream=None):
    """ops.gather_rows(data, idx, out) and the q-sample of every gathered row in one launch
    (gm_gather_rows[_bits]_qsample)."""
    from .ops import PackedData
    n_rows, row = data.shape
    B = out.shape[0] if B is None else B
    if not (idx.dtype == torch.int64 and idx.is_cuda):
        raise _lib.GMError("gather_rows_qsample: idx must be an int64 device tensor")
    if _rows2d(out, "out").shape[0] < B or out.shape[1] < row:
        raise _lib.GMError("gather_rows_qsample: out %s does not fit %d rows of %d" % (tuple(out.shape), B, row))
    o = _ddpm_out(xin, eps, t, B, row, tables.E)
    if isinstance(data, PackedData):
        _lib.call("gm_gather_rows_bits_qsample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(tables),
                  ctypes.byref(o), data.data_ptr(), data.wpr, n_rows, idx.data_ptr(), idx_slot, out.data_ptr(),
                  _ld(out), B, row)
    else:
        _lib.call("gm_gather_rows_qsample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(tables),
                  ctypes.byref(o), _rows2d(data, "data").data_ptr(), n_rows, idx.data_ptr(), idx_slot, out.data_ptr(),
                  _ld(out), B, row)
    return out


def ddpm_loss(out, eps, part, B, scale, dA=None, stream=None):
    """part[b] = sum_e (out - eps)^2 of row b and, with dA, dA = 2 scale (out - eps) (gm_ddpm_loss)."""
    I = out.shape[1]
    if _rows2d(out, "out").shape[0] < B or _rows2d(eps, "eps").shape[0] < B or eps.shape[1] < I or part.numel() < B \
            or not part.is_contiguous() or (dA is not None and (_rows2d(dA, "dA").shape[0] < B or dA.shape[1] != I)):
        raise _lib.GMError("ddpm_loss: the arrays do not fit B=%d, I=%d" % (B, I))
    _lib.call("gm_ddpm_loss", stream or stream_ptr(), out.data_ptr(), _ld(out), eps.data_ptr(), _ld(eps),
              dA.data_ptr() if dA is not None else None, _ld(dA) if dA is not None else 0, part.data_ptr(), scale, B, I)


def ddpm_reverse(xin, eps, coef, temb, I, seed, clip=True, slot=None, step=0, traj=None, tick=None, done=None,
                 rows=None, stream=None):
    """One sampler step in place on xin [n, >= I + E] with the denoiser's output eps [n, I] (gm_ddpm_reverse): the
    coefficients are row `slot` (a gm_slot of stride 8 over a device counter) or row `step` of coef [S, 8]; traj
    [S + 1, n, I] takes x_prev at index step + 1; tick (with done, one zeroed int32) is advanced by the launch."""
    T, E = temb.shape
    S = coef.shape[0]
    rows = xin.shape[0] if rows is None else rows
    if _rows2d(xin, "xin").shape[0] < rows or xin.shape[1] < I + E or _rows2d(eps, "eps").shape[0] < rows \
            or eps.shape[1] < I or tuple(coef.shape) != (S, 8) or not coef.is_contiguous() or not temb.is_contiguous():
        raise _lib.GMError("ddpm_reverse: xin %s / eps %s / coef %s do not fit %d rows of %d + %d"
                           % (tuple(xin.shape), tuple(eps.shape), tuple(coef.shape), rows, I, E))
    if traj is not None and not (traj.is_contiguous() and tuple(traj.shape) == (S + 1, rows, I)):
        raise _lib.GMError("ddpm_reverse: traj must be a contiguous [%d, %d, %d] tensor" % (S + 1, rows, I))
    if done is not None and not (done.dtype == torch.int32 and done.is_cuda):
        raise _lib.GMError("ddpm_reverse: done must be an int32 device tensor")
    a = DdpmReverseArgs()
    a.xin, a.ldin, a.eps, a.lde = xin.data_ptr(), _ld(xin), eps.data_ptr(), _ld(eps)
    a.coef, a.slot, a.temb = coef.data_ptr(), (slot if slot is not None else _lib.slot(0, 0, int(step), 0, 8)), \
        temb.data_ptr()
    if traj is not None:
        a.traj, a.traj_stride = traj.data_ptr(), rows * I
    a.seed = int(seed)
    a.tick = tick.data_ptr() if tick is not None else None
    a.done = done.data_ptr() if done is not None else None
    a.rows, a.I, a.E, a.T, a.S, a.clip = rows, I, E, T, S, 1 if clip else 0
    _lib.call("gm_ddpm_reverse", stream or stream_ptr(), ctypes.byref(a))


def ddpm_prior(xin, temb, I, seed, step, t, traj=None, rows=None, stream=None):
    """xin[:, :I] = the sampler's starting normals (counter step `step`), tails temb[t] (gm_ddpm_prior); traj [n, I]
    takes the same rows."""
    T, E = temb.shape
    rows = xin.shape[0] if rows is None else rows
    if _rows2d(xin, "xin").shape[0] < rows or xin.shape[1] < I + E or not temb.is_contiguous() \
            or (traj is not None and not (traj.is_contiguous() and traj.numel() >= rows * I)):
        raise _lib.GMError("ddpm_prior: xin %s does not fit %d rows of %d + %d" % (tuple(xin.shape), rows, I, E))
    _lib.call("gm_ddpm_prior", stream or stream_ptr(), xin.data_ptr(), _ld(xin), temb.data_ptr(), int(seed), int(step),
              int(t), traj.data_ptr() if traj is not None else None, rows, I, E, T)


# ---- Masked autoregressive model (csrc/gm_made.hip, gm_made.h; made.py) ----------------------------------------------
def _made_f32(t, shape, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == tuple(shape)):
        raise _lib.GMError("%s must be a contiguous float32 device tensor of shape %s" % (name, tuple(shape)))
    return t


def _made_i32(t, n, name):
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() == n):
        raise _lib.GMError("%s must be a contiguous int32 device tensor of %d elements" % (name, n))
    return t


def made_bce(logits, x, part, B, scale, dA=None, stream=None):
    """part[b] = sum_d softplus(a) - x a of row b and, with dA, dA = (sigmoid(a) - x) scale (gm_made_bce)."""
    I = logits.shape[1]
    if _rows2d(logits, "logits").shape[0] < B or _rows2d(x, "x").shape[0] < B or x.shape[1] < I or part.numel() < B \
            or not part.is_contiguous() or (dA is not None and (_rows2d(dA, "dA").shape[0] < B or dA.shape[1] != I)):
        raise _lib.GMError("made_bce: the arrays do not fit B=%d, I=%d" % (B, I))
    _lib.call("gm_made_bce", stream or stream_ptr(), logits.data_ptr(), _ld(logits), x.data_ptr(), _ld(x),
              dA.data_ptr() if dA is not None else None, _ld(dA) if dA is not None else 0, part.data_ptr(), scale, B, I)


def made_mask(W1, W2, m_in, m_h, moments1=None, moments2=None, stream=None):
    """Zeroes the masked entries of linear.weight W1 [H, I] and out.weight W2 [I, H] and -- moments = (m, v) flat views
    -- of their Adam moments (gm_made_mask); every other entry stays as it is."""
    H, I = W1.shape
    _made_f32(W1, (H, I), "W1"), _made_f32(W2, (I, H), "W2")
    a = MadeMaskArgs()
    a.W1, a.W2 = W1.data_ptr(), W2.data_ptr()
    a.m_in, a.m_h = _made_i32(m_in, I, "m_in").data_ptr(), _made_i32(m_h, H, "m_h").data_ptr()
    for mv, names in ((moments1, ("m1", "v1")), (moments2, ("m2", "v2"))):
        if mv is not None:
            for t, nm in zip(mv, names):
                setattr(a, nm, _made_f32(t.view(-1), (I * H,), nm).data_ptr())
    a.I, a.H = I, H
    _lib.call("gm_made_mask", stream or stream_ptr(), ctypes.byref(a))


def made_sample(W2, b2, W1T, b1, m_h, inv_order, n, seed, x=None, p=None, given=None, n_known=0, stream=None):
    """x [n, I] in {0, 1} drawn pixel by pixel in order of degree in ONE launch (gm_made_sample); p (a [n, I] tensor)
    receives the conditionals; the first n_known positions of the order are copied from given [n, I]."""
    I, H = W2.shape
    _made_f32(W2, (I, H), "W2"), _made_f32(W1T, (I, H), "W1T"), _made_f32(b2, (I,), "b2"), _made_f32(b1, (H,), "b1")
    x = torch.empty(n, I, device=W2.device) if x is None else x
    for t, nm in ((x, "x"), (p, "p"), (given, "given")):
        if t is not None and (_rows2d(t, nm).shape[0] < n or t.shape[1] < I):
            raise _lib.GMError("made_sample: %s %s does not fit %d rows of %d" % (nm, tuple(t.shape), n, I))
    a = MadeSampleArgs()
    a.W2, a.b2, a.W1T, a.b1 = W2.data_ptr(), b2.data_ptr(), W1T.data_ptr(), b1.data_ptr()
    a.m_h, a.inv_order = _made_i32(m_h, H, "m_h").data_ptr(), _made_i32(inv_order, I, "inv_order").data_ptr()
    a.x, a.ldx = x.data_ptr(), _ld(x)
    if p is not None:
        a.p, a.ldp = p.data_ptr(), _ld(p)
    if given is not None:
        a.given, a.ldg = given.data_ptr(), _ld(given)
    a.seed, a.n, a.I, a.H, a.n_known = int(seed), int(n), I, H, int(n_known)
    _lib.call("gm_made_sample", stream or stream_ptr(), ctypes.byref(a))
    return x


def made_uniform(n, I, seed, row0=0, device="cuda", stream=None):
    """u [n, I]: the sampler's uniforms of sample rows row0 .. row0 + n - 1 (gm_made_uniform)."""
    u = torch.empty(n, I, device=device)
    _lib.call("gm_made_uniform", stream or stream_ptr(), u.data_ptr(), _ld(u), int(seed), int(row0), int(n), int(I))
    return u


# ---- Restricted Boltzmann machine (csrc/gm_rbm.hip, gm_rbm.h; rbm.py) --------------------------------------------------
def rbm_chain(W, WT, c, b, x, steps, seed, n=None, v0_out=None, v_out=None, p_out=None, a_out=None, row0=0,
              step_ctr=None, step_base=None, d_add=0, g_mul=1, g_add=0, betas=None, b_A=None, logw=None, stream=None):
    """n Gibbs chains of `steps` steps from the binarisation of x [n, >= I], in ONE launch (gm_rbm_chain).  Outputs, each
    optional: v0_out (the binarisation), v_out (the last visible state; may be x), p_out / a_out (the conditionals of
    the last visible draw and their logits).  betas (float32 [steps + 1] on the device), b_A [I] and logw (float64 [n])
    together run the tempered chain of annealed importance sampling."""
    H, I = W.shape
    a = RbmChainArgs()
    a.step_ctr, a.step_base, _ = _clock("rbm_chain", 0, step_ctr, step_base)
    _made_f32(W, (H, I), "W"), _made_f32(WT, (I, H), "WT"), _made_f32(c, (H,), "c"), _made_f32(b, (I,), "b")
    n = x.shape[0] if n is None else int(n)
    for t, nm in ((x, "x"), (v0_out, "v0_out"), (v_out, "v_out"), (p_out, "p_out"), (a_out, "a_out")):
        if t is not None and (_rows2d(t, nm).shape[0] < n or t.shape[1] < I):
            raise _lib.GMError("rbm_chain: %s %s does not fit %d rows of %d" % (nm, tuple(t.shape), n, I))
    a.W, a.WT, a.c, a.b = W.data_ptr(), WT.data_ptr(), c.data_ptr(), b.data_ptr()
    a.x, a.ldx = x.data_ptr(), _ld(x)
    for t, nm, ld in ((v0_out, "v0_out", "ldv0"), (v_out, "v_out", "ldv"), (p_out, "p_out", "ldp"),
                      (a_out, "a_out", "lda")):
        if t is not None:
            setattr(a, nm, t.data_ptr())
            setattr(a, ld, _ld(t))
    if betas is not None or b_A is not None or logw is not None:
        if betas is None or b_A is None or logw is None:
            raise _lib.GMError("rbm_chain: betas, b_A and logw come together")
        _made_f32(betas, (int(steps) + 1,), "betas"), _made_f32(b_A, (I,), "b_A")
        if not (logw.is_cuda and logw.dtype == torch.float64 and logw.is_contiguous() and logw.numel() >= n):
            raise _lib.GMError("rbm_chain: logw must be a contiguous float64 device tensor of >= %d elements" % n)
        a.betas, a.b_A, a.logw = betas.data_ptr(), b_A.data_ptr(), logw.data_ptr()
    a.seed, a.row0, a.n, a.I, a.H, a.steps = int(seed), int(row0), n, I, H, int(steps)
    a.d_add, a.g_mul, a.g_add = int(d_add), int(g_mul), int(g_add)
    _lib.call("gm_rbm_chain", stream or stream_ptr(), ctypes.byref(a))


def rbm_grad(pre, V, b, dA, part, B, inv_b, stream=None):
    """From pre [2B, H] of the stacked V = [v0; vk]: dA = [-p0; +pk] inv_b and part [2B] = the signed free energies
    (gm_rbm_grad)."""
    H, I = pre.shape[1], b.numel()
    if _rows2d(pre, "pre").shape[0] < 2 * B or _rows2d(V, "V").shape[0] < 2 * B or V.shape[1] < I or \
            _rows2d(dA, "dA").shape[0] < 2 * B or dA.shape[1] != H or part.numel() < 2 * B or not part.is_contiguous():
        raise _lib.GMError("rbm_grad: the arrays do not fit B=%d, I=%d, H=%d" % (B, I, H))
    _lib.call("gm_rbm_grad", stream or stream_ptr(), pre.data_ptr(), _ld(pre), V.data_ptr(), _ld(V),
              _made_f32(b, (I,), "b").data_ptr(), dA.data_ptr(), _ld(dA), part.data_ptr(), inv_b, B, I, H)


def rbm_vbias(V, B, I, inv_b, g=None, adam=None, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, stream=None):
    """g [I] = inv_b sum_r (V[B + r] - V[r]) and, with adam = dict(p, m, v, sched, sched_slot), the Adam step of the
    visible bias in the same launch (gm_rbm_vbias)."""
    if _rows2d(V, "V").shape[0] < 2 * B or V.shape[1] < I:
        raise _lib.GMError("rbm_vbias: V %s does not fit 2 x %d rows of %d" % (tuple(V.shape), B, I))
    a = RbmVbiasArgs()
    a.V, a.ldv, a.inv_b, a.B, a.I = V.data_ptr(), _ld(V), inv_b, B, I
    if g is not None:
        a.g = _made_f32(g, (I,), "g").data_ptr()
    if adam is not None:
        a.pb, a.mb, a.vb = (_made_f32(adam[k], (I,), k).data_ptr() for k in ("p", "m", "v"))
        a.sched, a.sched_slot = adam["sched"].data_ptr(), adam.get("sched_slot", NO_SLOT)
    a.beta1, a.beta2, a.eps, a.weight_decay = betas[0], betas[1], eps, weight_decay
    _lib.call("gm_rbm_vbias", stream or stream_ptr(), ctypes.byref(a))


def rbm_transpose(W, WT, stream=None):
    """WT [cols, rows] = W [rows, cols] transposed, bit for bit (gm_rbm_transpose); either may be a row-strided view."""
    rows, cols = _rows2d(W, "W").shape
    if tuple(_rows2d(WT, "WT").shape) != (cols, rows):
        raise _lib.GMError("rbm_transpose: WT %s is not the transpose of W %s" % (tuple(WT.shape), tuple(W.shape)))
    _lib.call("gm_rbm_transpose", stream or stream_ptr(), W.data_ptr(), _ld(W), WT.data_ptr(), _ld(WT), rows, cols)
    return WT


def rbm_uniform(n, width, seed, tag, step=0, row0=0, step_ctr=None, step_base=None, device="cuda", stream=None):
    """u [n, width]: the RBM noise rule's uniforms of chain rows row0 .. under `tag` at step (gm_rbm_uniform)."""
    clock = _clock("rbm_uniform", step, step_ctr, step_base)
    u = torch.empty(n, width, device=device)
    _lib.call("gm_rbm_uniform", stream or stream_ptr(), u.data_ptr(), _ld(u), int(seed), int(tag), *clock, int(row0),
              int(n), int(width))
    return u


# ---- RealNVP coupling flow (csrc/gm_nvp.hip, gm_nvp.h; realnvp.py) ---------------------------------------------------
NVP_MASKS = {"checker": _lib.NVP_CHECKER, "half": _lib.NVP_HALF}


def _nvp_rows(t, B, W, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.stride(1) == 1 and t.shape[0] >= B
            and t.shape[1] >= W):
        raise _lib.GMError("%s must be a float32 device tensor of at least [%d, %d] with contiguous rows" % (name, B, W))
    return t


def _nvp_vec(t, B, name):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= B):
        raise _lib.GMError("%s must be a contiguous float32 device tensor of %d elements" % (name, B))
    return t


def _nvp_mask(mask):
    return NVP_MASKS[mask] if isinstance(mask, str) else int(mask)


def _nvp_noise(a, seed, tag, step, step_ctr, step_base, row0):
    a.seed, a.tag, a.row0 = _seed64("nvp_pre", seed), int(tag), int(row0)
    a.step_ctr, a.step_base, a.step_add = _clock("nvp_pre", step, step_ctr, step_base)


def nvp_pre(x, ya, yb, logdet, B, seed, tag, alpha, levels, mask, step=0, step_ctr=None, step_base=None, row0=0,
            stream=None):
    """Dequantise + logit + split of rows x [B, D] into ya [B, Da], yb [B, Db] and the rows' preprocessing
    log-determinant (gm_nvp_pre); the noise step is *step_ctr + *step_base + step."""
    D = x.shape[1]
    a = NvpPreArgs()
    _nvp_rows(x, B, D, "x"), _nvp_rows(ya, B, (D + 1) // 2, "ya"), _nvp_rows(yb, B, D // 2, "yb")
    a.x, a.ldx, a.ya, a.lda, a.yb, a.ldb = x.data_ptr(), _ld(x), ya.data_ptr(), _ld(ya), yb.data_ptr(), _ld(yb)
    a.logdet = _nvp_vec(logdet, B, "logdet").data_ptr()
    _nvp_noise(a, seed, tag, step, step_ctr, step_base, row0)
    a.alpha, a.levels, a.mask, a.mode, a.B, a.D = float(alpha), int(levels), _nvp_mask(mask), _lib.NVP_PRE, B, D
    _lib.call("gm_nvp_pre", stream or stream_ptr(), ctypes.byref(a))


def nvp_uniforms(n, D, seed, tag, step=0, row0=0, device="cuda", stream=None):
    """u [n, D]: the dequantisation noise gm_nvp_pre draws for (seed, tag, step) on rows row0 .., through its NOISE
    mode, bit for bit: what the general path and the tests feed the preprocessing."""
    a = NvpPreArgs()
    _nvp_noise(a, seed, tag, step, None, None, row0)
    u = torch.empty(n, D, device=device)
    a.u, a.ldu, a.mode, a.B, a.D = u.data_ptr(), _ld(u), _lib.NVP_NOISE, n, D
    _lib.call("gm_nvp_pre", stream or stream_ptr(), ctypes.byref(a))
    return u


def nvp_couple(st, inp, out, B, Dt, s_cap, logdet=None, inverse=False, stream=None):
    """out = inp exp(s) + t and logdet += sum s, or (inverse) out = (inp - t) exp(-s), with s = s_cap tanh(st[:, :Dt]),
    t = st[:, Dt:] (gm_nvp_couple)."""
    a = NvpCoupleArgs()
    _nvp_rows(st, B, 2 * Dt, "st"), _nvp_rows(inp, B, Dt, "inp"), _nvp_rows(out, B, Dt, "out")
    a.st, a.ldst, a.inp, a.ldin, a.out, a.ldout = st.data_ptr(), _ld(st), inp.data_ptr(), _ld(inp), out.data_ptr(), _ld(out)
    if not inverse:
        a.logdet = _nvp_vec(logdet, B, "logdet").data_ptr()
    a.s_cap, a.inverse, a.B, a.Dt = float(s_cap), 1 if inverse else 0, B, Dt
    _lib.call("gm_nvp_couple", stream or stream_ptr(), ctypes.byref(a))


def nvp_loss(za, zb, logdet, part, B, cst, scale=1.0, dza=None, dzb=None, stream=None):
    """part[r] = 0.5 sum z^2 - logdet[r] + cst and, with dza / dzb, dz = z scale (gm_nvp_loss)."""
    Da, Db = za.shape[1], zb.shape[1]
    a = NvpLossArgs()
    _nvp_rows(za, B, Da, "za"), _nvp_rows(zb, B, Db, "zb")
    a.za, a.ldza, a.zb, a.ldzb = za.data_ptr(), _ld(za), zb.data_ptr(), _ld(zb)
    a.logdet, a.part = _nvp_vec(logdet, B, "logdet").data_ptr(), _nvp_vec(part, B, "part").data_ptr()
    if dza is not None or dzb is not None:
        _nvp_rows(dza, B, Da, "dza"), _nvp_rows(dzb, B, Db, "dzb")
        a.dza, a.lddza, a.dzb, a.lddzb = dza.data_ptr(), _ld(dza), dzb.data_ptr(), _ld(dzb)
    a.cst, a.scale, a.B, a.Da, a.Db = float(cst), float(scale), B, Da, Db
    _lib.call("gm_nvp_loss", stream or stream_ptr(), ctypes.byref(a))


def nvp_couple_bwd(st, x, g0, dst, B, Dt, s_cap, c, g1=None, dx=None, stream=None):
    """dst[:, :Dt] = (g x exp(s) + c) s_cap (1 - tanh^2), dst[:, Dt:] = g, dx = g exp(s), with g = g0 (+ g1)
    (gm_nvp_couple_bwd)."""
    a = NvpCoupleBwdArgs()
    _nvp_rows(st, B, 2 * Dt, "st"), _nvp_rows(x, B, Dt, "x"), _nvp_rows(g0, B, Dt, "g0"), _nvp_rows(dst, B, 2 * Dt, "dst")
    a.st, a.ldst, a.x, a.ldx, a.g0, a.ldg0 = st.data_ptr(), _ld(st), x.data_ptr(), _ld(x), g0.data_ptr(), _ld(g0)
    a.dst, a.lddst = dst.data_ptr(), _ld(dst)
    if g1 is not None:
        a.g1, a.ldg1 = _nvp_rows(g1, B, Dt, "g1").data_ptr(), _ld(g1)
    if dx is not None:
        a.dx, a.lddx = _nvp_rows(dx, B, Dt, "dx").data_ptr(), _ld(dx)
    a.c, a.s_cap, a.B, a.Dt = float(c), float(s_cap), B, Dt
    _lib.call("gm_nvp_couple_bwd", stream or stream_ptr(), ctypes.byref(a))


def nvp_post(ya, yb, x, B, alpha, mask, stream=None):
    """x [B, D] = clamp((sigmoid(y) - alpha) / (1 - 2 alpha), 0, 1) from the halves (gm_nvp_post)."""
    D = x.shape[1]
    a = NvpPostArgs()
    _nvp_rows(ya, B, (D + 1) // 2, "ya"), _nvp_rows(yb, B, D // 2, "yb"), _nvp_rows(x, B, D, "x")
    a.ya, a.lda, a.yb, a.ldb, a.x, a.ldx = ya.data_ptr(), _ld(ya), yb.data_ptr(), _ld(yb), x.data_ptr(), _ld(x)
    a.alpha, a.mask, a.mode, a.B, a.D = float(alpha), _nvp_mask(mask), _lib.NVP_POST, B, D
    _lib.call("gm_nvp_post", stream or stream_ptr(), ctypes.byref(a))


def nvp_prior(za, zb, B, D, seed, mask, temperature=1.0, row0=0, stream=None):
    """The sampler's starting normals of rows row0 .. as halves za [B, Da], zb [B, Db], scaled by the temperature
    (gm_nvp_post's PRIOR mode)."""
    a = NvpPostArgs()
    _nvp_rows(za, B, (D + 1) // 2, "za"), _nvp_rows(zb, B, D // 2, "zb")
    a.ya, a.lda, a.yb, a.ldb = za.data_ptr(), _ld(za), zb.data_ptr(), _ld(zb)
    a.seed, a.row0, a.temperature = _seed64("nvp_prior", seed), int(row0), float(temperature)
    a.mask, a.mode, a.B, a.D = _nvp_mask(mask), _lib.NVP_PRIOR, B, D
    _lib.call("gm_nvp_post", stream or stream_ptr(), ctypes.byref(a))


# ---- Neural spline flow (csrc/gm_nsf.hip, gm_nsf.h; nsf.py) ----------------------------------------------------------
def nsf_couple(st, inp, out, B, Dt, bins, tail_bound, logdet=None, inverse=False, stream=None):
    """out = the rational-quadratic spline of inp under the parameter-major rows st [B, (3 bins - 1) Dt] and logdet +=
    the rows' sum of log dy/dx, or (inverse) out = the spline's inverse of inp (gm_nsf_couple)."""
    a = NsfCoupleArgs()
    _nvp_rows(st, B, (3 * bins - 1) * Dt, "st"), _nvp_rows(inp, B, Dt, "inp"), _nvp_rows(out, B, Dt, "out")
    a.st, a.ldst, a.inp, a.ldin, a.out, a.ldout = st.data_ptr(), _ld(st), inp.data_ptr(), _ld(inp), out.data_ptr(), _ld(out)
    if not inverse:
        a.logdet = _nvp_vec(logdet, B, "logdet").data_ptr()
    a.tail_bound, a.inverse, a.B, a.Dt, a.bins = float(tail_bound), 1 if inverse else 0, B, Dt, int(bins)
    _lib.call("gm_nsf_couple", stream or stream_ptr(), ctypes.byref(a))


def nsf_couple_bwd(st, x, g0, dst, B, Dt, bins, tail_bound, c, g1=None, dx=None, stream=None):
    """dst = d(g . y + c sum log dy/dx) / d st, every column written, and dx the same with respect to x, with g = g0
    (+ g1) (gm_nsf_couple_bwd)."""
    W = (3 * bins - 1) * Dt
    a = NsfCoupleBwdArgs()
    _nvp_rows(st, B, W, "st"), _nvp_rows(x, B, Dt, "x"), _nvp_rows(g0, B, Dt, "g0"), _nvp_rows(dst, B, W, "dst")
    a.st, a.ldst, a.x, a.ldx, a.g0, a.ldg0 = st.data_ptr(), _ld(st), x.data_ptr(), _ld(x), g0.data_ptr(), _ld(g0)
    a.dst, a.lddst = dst.data_ptr(), _ld(dst)
    if g1 is not None:
        a.g1, a.ldg1 = _nvp_rows(g1, B, Dt, "g1").data_ptr(), _ld(g1)
    if dx is not None:
        a.dx, a.lddx = _nvp_rows(dx, B, Dt, "dx").data_ptr(), _ld(dx)
    a.c, a.tail_bound, a.B, a.Dt, a.bins = float(c), float(tail_bound), B, Dt, int(bins)
    _lib.call("gm_nsf_couple_bwd", stream or stream_ptr(), ctypes.byref(a))


# ---- Masked autoregressive flow (csrc/gm_maf.hip, gm_maf.h; maf.py) --------------------------------------------------
def maf_halves(t, D):
    """The GM_NVP_HALF view of rows t [B, >= D]: (the first ceil(D / 2) columns, the rest), both inside t -- what
    gm_nvp_pre / gm_nvp_loss / gm_nvp_post take for an unsplit MAF row array."""
    Da = (D + 1) // 2
    return t[:, :Da], t[:, Da:D]


def maf_couple(y, ma, u, logdet, B, D, s_cap, stream=None):
    """u = (y - m) exp(-s) and logdet -= sum s, with [m | a] = ma and s = s_cap tanh(a) (gm_maf_couple)."""
    a = MafCoupleArgs()
    _nvp_rows(y, B, D, "y"), _nvp_rows(ma, B, 2 * D, "ma"), _nvp_rows(u, B, D, "u")
    a.y, a.ldy, a.ma, a.ldma, a.u, a.ldu = y.data_ptr(), _ld(y), ma.data_ptr(), _ld(ma), u.data_ptr(), _ld(u)
    a.logdet = _nvp_vec(logdet, B, "logdet").data_ptr()
    a.s_cap, a.B, a.D = float(s_cap), B, D
    _lib.call("gm_maf_couple", stream or stream_ptr(), ctypes.byref(a))


def maf_couple_bwd(ma, u, g, dout, B, D, s_cap, c, dy=None, stream=None):
    """dout[:, :D] = -g exp(-s), dout[:, D:] = (-(g u) - c) s_cap (1 - tanh^2(a)) and, with dy, dy = g exp(-s)
    (gm_maf_couple_bwd)."""
    a = MafCoupleBwdArgs()
    _nvp_rows(ma, B, 2 * D, "ma"), _nvp_rows(u, B, D, "u"), _nvp_rows(g, B, D, "g"), _nvp_rows(dout, B, 2 * D, "dout")
    a.ma, a.ldma, a.u, a.ldu, a.g, a.ldg = ma.data_ptr(), _ld(ma), u.data_ptr(), _ld(u), g.data_ptr(), _ld(g)
    a.dout, a.lddout = dout.data_ptr(), _ld(dout)
    if dy is not None:
        a.dy, a.lddy = _nvp_rows(dy, B, D, "dy").data_ptr(), _ld(dy)
    a.c, a.s_cap, a.B, a.D = float(c), float(s_cap), B, D
    _lib.call("gm_maf_couple_bwd", stream or stream_ptr(), ctypes.byref(a))


def maf_mask(W1, W2, m_in, m_h, moments1=None, moments2=None, stream=None):
    """Zeroes the masked entries of one layer's linear.weight W1 [H, D] and out.weight W2 [2 D, H] and -- moments =
    (m, v) flat views -- of their Adam moments (gm_maf_mask); every other entry stays as it is."""
    H, D = W1.shape
    _made_f32(W1, (H, D), "W1"), _made_f32(W2, (2 * D, H), "W2")
    a = MafMaskArgs()
    a.W1, a.W2 = W1.data_ptr(), W2.data_ptr()
    a.m_in, a.m_h = _made_i32(m_in, D, "m_in").data_ptr(), _made_i32(m_h, H, "m_h").data_ptr()
    for mv, names, n in ((moments1, ("m1", "v1"), D * H), (moments2, ("m2", "v2"), 2 * D * H)):
        if mv is not None:
            for t, nm in zip(mv, names):
                setattr(a, nm, _made_f32(t.view(-1), (n,), nm).data_ptr())
    a.D, a.H = D, H
    _lib.call("gm_maf_mask", stream or stream_ptr(), ctypes.byref(a))


def maf_invert(u, W2, b2, W1T, b1, m_h, inv_order, s_cap, n=None, y=None, s=None, stream=None):
    """y [n, D] with layer(y) = u, solved pixel by pixel in order of degree in ONE launch (gm_maf_invert); s (a [n, D]
    tensor) receives the log-scales."""
    D, H = W1T.shape
    _made_f32(W2, (2 * D, H), "W2"), _made_f32(W1T, (D, H), "W1T"), _made_f32(b2, (2 * D,), "b2"), _made_f32(b1, (H,), "b1")
    n = u.shape[0] if n is None else int(n)
    y = torch.empty(n, D, device=u.device) if y is None else y
    for t, nm in ((u, "u"), (y, "y"), (s, "s")):
        if t is not None:
            _nvp_rows(t, n, D, nm)
    a = MafInvertArgs()
    a.u, a.ldu, a.y, a.ldy = u.data_ptr(), _ld(u), y.data_ptr(), _ld(y)
    if s is not None:
        a.s, a.lds = s.data_ptr(), _ld(s)
    a.W2, a.b2, a.W1T, a.b1 = W2.data_ptr(), b2.data_ptr(), W1T.data_ptr(), b1.data_ptr()
    a.m_h, a.inv_order = _made_i32(m_h, H, "m_h").data_ptr(), _made_i32(inv_order, D, "inv_order").data_ptr()
    a.s_cap, a.n, a.D, a.H = float(s_cap), n, D, H
    _lib.call("gm_maf_invert", stream or stream_ptr(), ctypes.byref(a))
    return y


# ---- Generative moment matching network / kernel MMD (csrc/gm_gmmn.hip; gmmn.py, metrics.mmd) ----------------------
def gmmn_noise(seed, tag, step=0, step_ctr=None, step_base=None, row0=0):
    """The prior's noise block (a gm_iwae_noise at k = 1): stream (seed, tag) at step = *step_ctr + *step_base + step,
    the call's row b draws noise row row0 + b."""
    return iwae_noise(seed, tag, 1, j0=row0, step=step, step_ctr=step_ctr, step_base=step_base)


def gmmn_prior(z, noise, B=None, Z=None, stream=None):
    """z [B, Z] = 2 u - 1, u the uniforms of the noise block's rows (gm_gmmn_prior)."""
    B = z.shape[0] if B is None else int(B)
    Z = z.shape[1] if Z is None else int(Z)
    if _rows2d(z, "z").shape[0] < B or z.shape[1] < Z:
        raise _lib.GMError("gmmn_prior: z %s does not fit B=%d, Z=%d" % (tuple(z.shape), B, Z))
    _lib.call("gm_gmmn_prior", stream or stream_ptr(), ctypes.byref(noise), z.data_ptr(), _ld(z), B, Z)
    return z


def mmd_sigmas(sigmas, device="cuda", who="mmd", error=None):
    """The bandwidths as a float32 device vector: 1 to GM_MMD_MAX_SIGMAS finite values > 0, else `error` (GMError)."""
    import numpy as np
    error = error or _lib.GMError
    try:
        s = np.asarray(sigmas, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise error("%s: sigmas must be numbers, got %r" % (who, sigmas))
    if not 1 <= s.size <= _lib.MMD_MAX_SIGMAS:
        raise error("%s: 1 to %d bandwidths, got %d" % (who, _lib.MMD_MAX_SIGMAS, s.size))
    if not (np.all(np.isfinite(s)) and np.all(s > 0)):
        raise error("%s: every sigma must be finite and > 0, got %s" % (who, s.tolist()))
    return torch.from_numpy(s.astype(np.float32)).to(device) if device is not None else s


def mmd_workspace(N, M, grad, device="cuda"):
    """The device workspace of mmd_pairs / mmd_finalize for N generated and M data rows (gm_mmd_workspace_bytes)."""
    n = _lib.load().gm_mmd_workspace_bytes(int(N), int(M), 1 if grad else 0)
    if n < 0:
        _lib.check(int(n), "gm_mmd_workspace_bytes")
    return torch.empty(int(n) // 8 + 1, dtype=torch.float64, device=device)


def mmd_pairs(X, Y, sig, ws, C=None, Rc=None, N=None, M=None, stream=None):
    """Every tile's pairs of X [N, I] and Y [M, I] under the bandwidths sig (gm_mmd_pairs): the block sums (and, with C
    [N, >= N + M], the coefficients and the shares of r) are left in ws for mmd_finalize; Rc (contiguous, >= N + M rows of
    I; None: a new tensor) takes the rows less X's first row, what the distances and the product C (R - mu) are formed
    from."""
    N = X.shape[0] if N is None else int(N)
    M = Y.shape[0] if M is None else int(M)
    I = X.shape[1]
    if _rows2d(X, "X").shape[0] < N or _rows2d(Y, "Y").shape[0] < M or Y.shape[1] != I:
        raise _lib.GMError("mmd_pairs: X %s / Y %s do not fit N=%d, M=%d" % (tuple(X.shape), tuple(Y.shape), N, M))
    if C is not None and (_rows2d(C, "C").shape[0] < N or C.shape[1] < N + M):
        raise _lib.GMError("mmd_pairs: C %s does not fit [%d, %d]" % (tuple(C.shape), N, N + M))
    if Rc is None:
        Rc = torch.empty(N + M, I, device=X.device)
    if not (_rows2d(Rc, "Rc").is_contiguous() and Rc.shape[0] >= N + M and Rc.shape[1] == I):
        raise _lib.GMError("mmd_pairs: Rc %s must be contiguous [>= %d, %d]" % (tuple(Rc.shape), N + M, I))
    _tc_vec(sig, 1, "mmd_pairs", "sig")
    _lib.call("gm_mmd_pairs", stream or stream_ptr(), X.data_ptr(), _ld(X), N, Y.data_ptr(), _ld(Y), M, I,
              sig.data_ptr(), sig.numel(), C.data_ptr() if C is not None else None, _ld(C) if C is not None else 0,
              Rc.data_ptr(), ws.data_ptr(), ws.numel() * ws.element_size())


def mmd_finalize(N, M, n_sigma, sqrt_loss, ws, stats, r=None, loss_out=None, stream=None):
    """stats [10] float64 (mmd2, loss, 1 / (2 loss), the block sums; include/gm_hip.h) and, given r [N], the row sums
    of C, from the workspace mmd_pairs filled (gm_mmd_finalize).  loss_out: a float32 tensor taking the loss."""
    if not (stats.is_cuda and stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() >= 10):
        raise _lib.GMError("mmd_finalize: stats must be a contiguous float64 device tensor of 10 values")
    if r is not None:
        _tc_vec(r, N, "mmd_finalize", "r")
    if loss_out is not None:
        _tc_vec(loss_out, 1, "mmd_finalize", "loss_out")
    _lib.call("gm_mmd_finalize", stream or stream_ptr(), int(N), int(M), int(n_sigma), 1 if sqrt_loss else 0,
              1 if r is not None else 0, ws.data_ptr(), ws.numel() * ws.element_size(), stats.data_ptr(),
              r.data_ptr() if r is not None else None, loss_out.data_ptr() if loss_out is not None else None)


def mmd_grad(X, P, r, stats, dA, N=None, sigmoid=True, gscale=1.0, mu=None, stream=None):
    """dA [N, I] = gscale stats[2] (r_i (x - mu) - P) (sigmoid: times x (1 - x)) with P = C (R - mu) (gm_mmd_grad); mu: a
    row of I values (mmd_pairs' Rc is centred on X[0]), None: 0."""
    N = X.shape[0] if N is None else int(N)
    I = X.shape[1]
    for t, nm in ((X, "X"), (P, "P"), (dA, "dA")):
        if _rows2d(t, nm).shape[0] < N or t.shape[1] != I:
            raise _lib.GMError("mmd_grad: %s %s does not fit [%d, %d]" % (nm, tuple(t.shape), N, I))
    _tc_vec(r, N, "mmd_grad", "r")
    if mu is not None:
        _tc_vec(mu[0] if mu.dim() == 2 else mu, I, "mmd_grad", "mu")
    _lib.call("gm_mmd_grad", stream or stream_ptr(), X.data_ptr(), _ld(X), mu.data_ptr() if mu is not None else None,
              P.data_ptr(), _ld(P), r.data_ptr(),
              stats.data_ptr(), float(gscale), 1 if sigmoid else 0, dA.data_ptr(), _ld(dA), N, I)


def mmd_stats(samples, data, sig, sqrt_loss=False):
    """stats [10] (float64, device) of the rows `samples` against `data`: pairs without C, then finalize."""
    N, M = samples.shape[0], data.shape[0]
    ws = mmd_workspace(N, M, False, samples.device)
    stats = torch.zeros(10, dtype=torch.float64, device=samples.device)
    mmd_pairs(samples, data, sig, ws)
    mmd_finalize(N, M, sig.numel(), sqrt_loss, ws, stats)
    return stats


class _MMDLoss(torch.autograd.Function):
    """mmd_loss below: pairs + finalize forward; C (R - mu) through the GEMM kernels and gm_mmd_grad backward."""

    @staticmethod
    def forward(ctx, samples, data, sig, sqrt_loss):
        N, M, I = samples.shape[0], data.shape[0], samples.shape[1]
        grad = ctx.needs_input_grad[0]
        dev = samples.device
        R = torch.cat([samples.detach(), data.detach()], 0).contiguous()
        ws = mmd_workspace(N, M, grad, dev)
        stats = torch.zeros(10, dtype=torch.float64, device=dev)
        C = torch.empty(N, (N + M + 3) // 4 * 4, device=dev) if grad else None
        r = torch.empty(N, device=dev) if grad else None
        loss = torch.empty(1, device=dev)
        Rc = torch.empty_like(R)
        mmd_pairs(R[:N], R[N:], sig, ws, C=C, Rc=Rc)
        mmd_finalize(N, M, sig.numel(), sqrt_loss, ws, stats, r=r, loss_out=loss)
        if grad:
            ctx.save_for_backward(R, Rc, C, r, stats)
        ctx.shape = (N, M, I)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        from . import ops
        R, Rc, C, r, stats = ctx.saved_tensors
        N, M, I = ctx.shape
        P = torch.empty(N, I, device=R.device)
        dX = torch.empty(N, I, device=R.device)
        ops.linear_bwd_dx(C[:, :N + M], Rc, P, M=N)
        mmd_grad(R[:N], P, r, stats, dX, sigmoid=False, mu=R[:1])
        return dX * g, None, None, None


def mmd_loss(samples, data, sigmas, sqrt_loss=True):
    """The kernel MMD of gmmn.py's contract between samples [N, I] and data [M, I] (float32 device rows) as a
    differentiable scalar: sqrt(mmd2 + 1e-8) (sqrt_loss) or mmd2, the biased statistic.  The gradient is with respect
    to `samples` only: data.requires_grad raises.  sigmas: numbers, or the float32 device vector of mmd_sigmas."""
    if data.requires_grad:
        raise _lib.GMError("mmd_loss differentiates with respect to samples only: data.requires_grad is set")
    for t, nm in ((samples, "samples"), (data, "data")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
            raise _lib.GMError("mmd_loss: %s must be a 2-D float32 tensor on the MI355X; there is no CPU fallback" % nm)
    if samples.shape[1] != data.shape[1] or not 1 <= samples.shape[1] <= _lib.MMD_MAX_I:
        raise _lib.GMError("mmd_loss: rows of %d and %d values (1 to %d, equal)"
                           % (samples.shape[1], data.shape[1], _lib.MMD_MAX_I))
    if samples.shape[0] < 1 or data.shape[0] < 1 or samples.shape[0] > 65535:
        raise _lib.GMError("mmd_loss: 1 to 65535 sample rows and at least one data row")
    sig = sigmas if isinstance(sigmas, torch.Tensor) else mmd_sigmas(sigmas, samples.device, "mmd_loss")
    return _MMDLoss.apply(samples.contiguous(), data.contiguous(), sig, bool(sqrt_loss))


# ---- Sliced Wasserstein distance (csrc/gm_sw.hip; swg.py, metrics.sliced_wasserstein) ------------------------------
def sw_noise(seed, tag, step=0, step_ctr=None, step_base=None, row0=0):
    """The noise block of the SWG's prior or directions (a gm_iwae_noise at k = 1): stream (seed, tag) at step =
    *step_ctr + *step_base + step, the call's row p draws noise row row0 + p."""
    return iwae_noise(seed, tag, 1, j0=row0, step=step, step_ctr=step_ctr, step_base=step_base)


def sw_directions(theta, noise, P=None, I=None, stream=None):
    """theta [P, I]: the noise block's rows of normals, each scaled to unit 2-norm (gm_sw_directions)."""
    P = theta.shape[0] if P is None else int(P)
    I = theta.shape[1] if I is None else int(I)
    if _rows2d(theta, "theta").shape[0] < P or theta.shape[1] < I:
        raise _lib.GMError("sw_directions: theta %s does not fit P=%d, I=%d" % (tuple(theta.shape), P, I))
    _lib.call("gm_sw_directions", stream or stream_ptr(), ctypes.byref(noise), theta.data_ptr(), _ld(theta), P, I)
    return theta


def sw_workspace(P, device="cuda"):
    """The device workspace of sw_sort / sw_finalize for P projections: the column sums (gm_sw_workspace_bytes)."""
    n = _lib.load().gm_sw_workspace_bytes(int(P))
    if n < 0:
        _lib.check(int(n), "gm_sw_workspace_bytes")
    return torch.empty(int(n) // 8, dtype=torch.float64, device=device)


def _sw_ws(ws, P, who):
    if not (isinstance(ws, torch.Tensor) and ws.is_cuda and ws.dtype == torch.float64 and ws.is_contiguous()
            and ws.numel() >= P):
        raise _lib.GMError("%s: ws must be a contiguous float64 device tensor of at least %d values" % (who, P))
    return ws


def sw_sort(Pr, N, M, ws, Ct=None, P=None, stream=None):
    """Every projection's two columns sorted and matched by rank (gm_sw_sort): Pr [P, >= N + M] holds a_p in columns
    [0, N) and b_p in [N, N + M); ws[p] = W_p N M; Ct [P, >= N] (None: no gradient, up to SW_MAX_ROWS rows a side) takes
    d swd2 / d a at the rows' original positions."""
    P = Pr.shape[0] if P is None else int(P)
    N, M = int(N), int(M)
    if _rows2d(Pr, "Pr").shape[0] < P or Pr.shape[1] < N + M:
        raise _lib.GMError("sw_sort: Pr %s does not fit P=%d, N + M=%d" % (tuple(Pr.shape), P, N + M))
    if Ct is not None and (_rows2d(Ct, "Ct").shape[0] < P or Ct.shape[1] < N):
        raise _lib.GMError("sw_sort: Ct %s does not fit [%d, %d]" % (tuple(Ct.shape), P, N))
    _sw_ws(ws, P, "sw_sort")
    _lib.call("gm_sw_sort", stream or stream_ptr(), Pr.data_ptr(), _ld(Pr), P, N, M,
              Ct.data_ptr() if Ct is not None else None, _ld(Ct) if Ct is not None else 0, ws.data_ptr(), 8 * ws.numel())


def sw_finalize(P, N, M, ws, stats, loss_out=None, stream=None):
    """stats [2] float64 = (swd2, sqrt(swd2)) from the column sums sw_sort left in ws (gm_sw_finalize).  loss_out: a
    float32 tensor taking swd2."""
    if not (stats.is_cuda and stats.dtype == torch.float64 and stats.is_contiguous() and stats.numel() >= 2):
        raise _lib.GMError("sw_finalize: stats must be a contiguous float64 device tensor of 2 values")
    if loss_out is not None:
        _tc_vec(loss_out, 1, "sw_finalize", "loss_out")
    _sw_ws(ws, int(P), "sw_finalize")
    _lib.call("gm_sw_finalize", stream or stream_ptr(), int(P), int(N), int(M), ws.data_ptr(), 8 * ws.numel(),
              stats.data_ptr(), loss_out.data_ptr() if loss_out is not None else None)


class _SWLoss(torch.autograd.Function):
    """sw_loss below: the projection GEMM, sort and finalize forward; Ct^T Theta through the GEMM kernels backward."""

    @staticmethod
    def forward(ctx, samples, data, theta):
        from . import ops
        N, M, P = samples.shape[0], data.shape[0], theta.shape[0]
        grad = ctx.needs_input_grad[0]
        dev = samples.device
        R = torch.cat([samples.detach(), data.detach()], 0).contiguous()
        Pr = torch.empty(P, N + M, device=dev)
        ops.linear_fwd(theta, R, None, Pr, "id")                  # [P, N + M]: a projection's values are contiguous
        ws = sw_workspace(P, dev)
        stats = torch.zeros(2, dtype=torch.float64, device=dev)
        Ct = torch.empty(P, N, device=dev) if grad else None
        loss = torch.empty(1, device=dev)
        sw_sort(Pr, N, M, ws, Ct=Ct)
        sw_finalize(P, N, M, ws, stats, loss_out=loss)
        if grad:
            ctx.save_for_backward(Ct, theta)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        from . import ops
        Ct, theta = ctx.saved_tensors
        dX = torch.empty(Ct.shape[1], theta.shape[1], device=Ct.device)
        ops.linear_bwd_dw(Ct, theta, dX, None)                    # dX [N, I] = Ct^T Theta
        return dX * g, None, None


def sw_loss(samples, data, theta):
    """swd2 of swg.py's contract between samples [N, I] and data [M, I] (float32 device rows, at most SW_MAX_B each) over
    the unit directions theta [P, I], as a differentiable scalar.  The gradient is with respect to `samples` only."""
    if data.requires_grad or theta.requires_grad:
        raise _lib.GMError("sw_loss differentiates with respect to samples only: data or theta requires grad")
    for t, nm in ((samples, "samples"), (data, "data"), (theta, "theta")):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2):
            raise _lib.GMError("sw_loss: %s must be a 2-D float32 tensor on the MI355X; there is no CPU fallback" % nm)
    I = samples.shape[1]
    if data.shape[1] != I or theta.shape[1] != I or not 1 <= I <= _lib.MMD_MAX_I:
        raise _lib.GMError("sw_loss: rows of %d, %d and %d values (1 to %d, equal)"
                           % (I, data.shape[1], theta.shape[1], _lib.MMD_MAX_I))
    if not (1 <= samples.shape[0] <= _lib.SW_MAX_B and 1 <= data.shape[0] <= _lib.SW_MAX_B):
        raise _lib.GMError("sw_loss: 1 to %d sample rows and data rows" % _lib.SW_MAX_B)
    if not 1 <= theta.shape[0] <= _lib.SW_MAX_P:
        raise _lib.GMError("sw_loss: 1 to %d directions" % _lib.SW_MAX_P)
    return _SWLoss.apply(samples.contiguous(), data.contiguous(), theta.contiguous())


# ---- Flow matching (csrc/gm_fm.hip, gm_fm.h; flowmatch.py) ------------------------------------------------------------
def fm_noise(seed, train=True, step=0, step_ctr=None, step_base=None, row0=0):
    """A gm_fm_noise block: the training stream (tags FMTD / FMTT / FMTN) or the validation one (FMVD / FMVT / FMVN) at
    step = *step_ctr + *step_base + step (int64 device tensors, or None for 0).  The tensors must outlive every launch
    (and every captured graph) that reads them."""
    tags = (_lib.FM_TAG_D, _lib.FM_TAG_T, _lib.FM_TAG_N) if train else (_lib.FM_TAG_VD, _lib.FM_TAG_VT, _lib.FM_TAG_VN)
    return FmNoise(_seed64("fm_noise", seed), *tags, *_clock("fm_noise", step, step_ctr, step_base), int(row0))


def fm_tables(tt, tc, temb):
    """A gm_fm_tables block over the model's fp32 device buffers tt [T + 1], tc [T + 1], temb [T + 1, E]."""
    for t, nm in ((tt, "tt"), (tc, "tc"), (temb, "temb")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise _lib.GMError("fm_tables: %s must be a contiguous float32 device tensor" % nm)
    T1, E = temb.shape
    if tt.numel() != T1 or tc.numel() != T1:
        raise _lib.GMError("fm_tables: tt and tc hold one float per grid point")
    tab = FmTables(tt.data_ptr(), tc.data_ptr(), temb.data_ptr(), T1 - 1, E)
    tab.keep = (tt, tc, temb)
    return tab


def _fm_out(xin, u, logdet, j, rows, I, E, alpha, levels, y1=None, y0=None):
    _nvp_rows(xin, rows, I + E, "xin"), _nvp_rows(u, rows, I, "u"), _nvp_vec(logdet, rows, "logdet")
    if j is not None and not (j.is_cuda and j.dtype == torch.int32 and j.is_contiguous() and j.numel() >= rows):
        raise _lib.GMError("fm q-sample: j must be a contiguous int32 device tensor of %d elements" % rows)
    o = FmOut(xin.data_ptr(), _ld(xin), u.data_ptr(), _ld(u), logdet.data_ptr(), j.data_ptr() if j is not None else None)
    if y1 is not None:
        o.y1, o.ldy1 = _nvp_rows(y1, rows, I, "y1").data_ptr(), _ld(y1)
    if y0 is not None:
        o.y0, o.ldy0 = _nvp_rows(y0, rows, I, "y0").data_ptr(), _ld(y0)
    o.alpha, o.levels = float(alpha), int(levels)
    return o


def fm_qsample(x, noise, tables, alpha, levels, xin=None, u=None, logdet=None, j=None, y1=None, y0=None, stream=None):
    """(xin, u, logdet, j) of the image rows x [n, I] in [0, 1] (gm_fm_qsample): xin [n, I + E] = [y_t | temb[j]], u
    [n, I] = y1 - y0, logdet [n] the preprocessing log-determinant, j [n] int32 the grid index; y1 / y0 [n, I]
    (optional) take the preprocessed rows and the normals.  Missing outputs are allocated."""
    n, I = _rows2d(x, "x").shape
    E = tables.E
    xin = torch.empty(n, I + E, device=x.device) if xin is None else xin
    u = torch.empty(n, I, device=x.device) if u is None else u
    logdet = torch.empty(n, device=x.device) if logdet is None else logdet
    j = torch.empty(n, dtype=torch.int32, device=x.device) if j is None else j
    if n:
        o = _fm_out(xin, u, logdet, j, n, I, E, alpha, levels, y1, y0)
        _lib.call("gm_fm_qsample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(tables), ctypes.byref(o),
                  x.data_ptr(), x.stride(0), n, I)
    return xin, u, logdet, j


def gather_rows_fm_qsample(data, idx, out, xin, u, logdet, j, noise, tables, alpha, levels, B=None, idx_slot=NO_SLOT,
                           y1=None, y0=None, stream=None):
    """ops.gather_rows(data, idx, out) and the path sample of every gathered row in one launch
    (gm_gather_rows[_bits]_fm_qsample)."""
    from .ops import PackedData
    n_rows, row = data.shape
    B = out.shape[0] if B is None else B
    if not (idx.dtype == torch.int64 and idx.is_cuda):
        raise _lib.GMError("gather_rows_fm_qsample: idx must be an int64 device tensor")
    _nvp_rows(out, B, row, "out")
    o = _fm_out(xin, u, logdet, j, B, row, tables.E, alpha, levels, y1, y0)
    if isinstance(data, PackedData):
        _lib.call("gm_gather_rows_bits_fm_qsample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(tables),
                  ctypes.byref(o), data.data_ptr(), data.wpr, n_rows, idx.data_ptr(), idx_slot, out.data_ptr(),
                  _ld(out), B, row)
    else:
        _lib.call("gm_gather_rows_fm_qsample", stream or stream_ptr(), ctypes.byref(noise), ctypes.byref(tables),
                  ctypes.byref(o), _rows2d(data, "data").data_ptr(), n_rows, idx.data_ptr(), idx_slot, out.data_ptr(),
                  _ld(out), B, row)
    return out


def fm_div_tiles(H):
    """The number of partials per row gm_fm_div writes: one per 32 hidden units."""
    return (int(H) + 31) // 32


def fm_div(H1, H2, Q, B=None, part=None, div=None, finish=True, stream=None):
    """div [B] = sum_{i, j} [H2[b, i] > 0] Q[i, j] [H1[b, j] > 0] (gm_fm_div).  part [tiles, B] takes the tiles'
    partials; finish=False leaves them for gm_fm_stage to add and returns part."""
    H = Q.shape[0]
    B = H1.shape[0] if B is None else B
    if Q.dim() != 2 or Q.shape[1] != H or not 1 <= H <= _lib.FM_MAX_H:
        raise _lib.GMError("fm_div: Q must be [H, H] with 1 <= H <= %d, got %s" % (_lib.FM_MAX_H, tuple(Q.shape)))
    _nvp_rows(H1, B, H, "H1"), _nvp_rows(H2, B, H, "H2"), _nvp_rows(Q, H, H, "Q")
    tiles = fm_div_tiles(H)
    part = torch.empty(tiles, B, device=H1.device) if part is None else part
    if not (part.is_cuda and part.dtype == torch.float32 and part.is_contiguous() and part.numel() >= tiles * B):
        raise _lib.GMError("fm_div: part must be a contiguous float32 device tensor of %d elements" % (tiles * B))
    a = FmDivArgs(H1.data_ptr(), _ld(H1), H2.data_ptr(), _ld(H2), Q.data_ptr(), _ld(Q), part.data_ptr(), part.numel())
    if finish:
        div = torch.empty(B, device=H1.device) if div is None else div
        a.div = _nvp_vec(div, B, "div").data_ptr()
    a.B, a.H = B, H
    _lib.call("gm_fm_div", stream or stream_ptr(), ctypes.byref(a))
    return div if finish else part


def fm_stage(k, base, acc, xin, tab, temb, I, stages, L=None, div=None, div_parts=1, slot=None, step=0, traj=None,
             tick=None, done=None, rows=None, stream=None):
    """One solver stage in place (gm_fm_stage): the coefficients are row `slot` (a gm_slot of stride 8 over a device
    counter) or row `step` of tab [S, 8]; div [div_parts, rows] the divergence's partials (None: sampling, L is left
    alone); traj [S / stages + 1, rows, I] takes a step's result at index step + 1; tick (with done, one zeroed int32)
    is advanced by the launch."""
    T1, E = temb.shape
    S = tab.shape[0]
    rows = xin.shape[0] if rows is None else rows
    _nvp_rows(k, rows, I, "k"), _nvp_rows(base, rows, I, "base"), _nvp_rows(acc, rows, I, "acc")
    _nvp_rows(xin, rows, I + E, "xin")
    if tuple(tab.shape) != (S, 8) or not (tab.is_cuda and tab.dtype == torch.float32 and tab.is_contiguous()) \
            or not temb.is_contiguous():
        raise _lib.GMError("fm_stage: tab must be a contiguous float32 device tensor [S, 8]")
    if traj is not None and not (traj.is_contiguous() and tuple(traj.shape) == (S // stages + 1, rows, I)):
        raise _lib.GMError("fm_stage: traj must be a contiguous [%d, %d, %d] tensor" % (S // stages + 1, rows, I))
    if done is not None and not (done.dtype == torch.int32 and done.is_cuda):
        raise _lib.GMError("fm_stage: done must be an int32 device tensor")
    a = FmStageArgs()
    a.k, a.ldk, a.base, a.ldb, a.acc, a.lda = k.data_ptr(), _ld(k), base.data_ptr(), _ld(base), acc.data_ptr(), _ld(acc)
    a.xin, a.ldin = xin.data_ptr(), _ld(xin)
    if div is not None:
        if L is None or not (L.is_cuda and L.dtype == torch.float32 and L.is_contiguous() and L.numel() >= 2 * rows):
            raise _lib.GMError("fm_stage: the divergence needs L, a contiguous float32 device tensor [rows, 2]")
        if not (div.is_cuda and div.dtype == torch.float32 and div.is_contiguous() and div.numel() >= div_parts * rows):
            raise _lib.GMError("fm_stage: div must be a contiguous float32 device tensor [div_parts, rows]")
        a.L, a.div, a.div_stride, a.div_parts = L.data_ptr(), div.data_ptr(), rows, int(div_parts)
    a.tab, a.slot, a.temb = tab.data_ptr(), (slot if slot is not None else _lib.slot(0, 0, int(step), 0, 8)), \
        temb.data_ptr()
    if traj is not None:
        a.traj, a.traj_stride = traj.data_ptr(), rows * I
    a.tick = tick.data_ptr() if tick is not None else None
    a.done = done.data_ptr() if done is not None else None
    a.rows, a.I, a.E, a.T, a.S, a.stages = rows, I, E, T1 - 1, S, int(stages)
    _lib.call("gm_fm_stage", stream or stream_ptr(), ctypes.byref(a))
