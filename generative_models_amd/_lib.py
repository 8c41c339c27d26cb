"""ctypes binding of libgm_hip.so (C-ABI declared in include/gm_hip.h).

There is NO fallback: if the HIP library is missing or a call fails, this raises.  The product
path never routes through torch eager kernels or the CPU oracle for the ops bound here."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GM_LIB_PATH") or os.path.join(HERE, "libgm_hip.so")

GM_EINVAL = -10001
ACT_ID, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ACT = {"id": ACT_ID, None: ACT_ID, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID}
LOSS = {"ns": 0, "mm": 1, "w": 2, "ls": 3, "ra": 4, "fisher": 5, "f_total_variation": 6,
        "f_forward_kl": 7, "f_reverse_kl": 8, "f_pearson": 9, "f_hellinger": 10,
        "f_jensen_shannon": 11}


class Slot(ctypes.Structure):
    """gm_slot: ((ctr ? *ctr : 0) * mul + add) % ring * stride."""
    _fields_ = [("ctr", c_void_p), ("mul", c_int32), ("add", c_int32), ("ring", c_int32),
                ("stride", c_int64)]


def slot(ctr=0, mul=0, add=0, ring=0, stride=0):
    return Slot(ctr or None, mul, add, ring, stride)


NO_SLOT = Slot(None, 0, 0, 0, 0)


class HeadBwdArgs(ctypes.Structure):
    """gm_head_bwd_args (include/gm_hip.h): gm_head_bwd_fused's arguments as one block."""
    _fields_ = [("H", c_void_p), ("ldh", c_int64), ("dS", c_void_p), ("w2", c_void_p),
                ("b2", c_void_p), ("rowloss", c_void_p), ("dH", c_void_p), ("lddh", c_int64),
                ("gw2", c_void_p), ("gb2", c_void_p), ("loss_out", c_void_p), ("loss_slot", Slot),
                ("inv_b", c_float), ("gen_mode", c_int), ("B", c_int), ("Hd", c_int),
                ("with_adam", c_int), ("mW", c_void_p), ("vW", c_void_p), ("mb", c_void_p),
                ("vb", c_void_p), ("sched", c_void_p), ("sched_slot", Slot),
                ("beta1", ctypes.c_double), ("beta2", ctypes.c_double), ("eps", ctypes.c_double),
                ("weight_decay", ctypes.c_double), ("clamp", c_float), ("tick", c_void_p),
                ("gw2_add", c_void_p), ("pen_s", c_void_p), ("pen_h", c_void_p), ("pen_ldh", c_int64),
                ("pen_t", c_void_p), ("pen_ldt", c_int64), ("pen_rows", c_int), ("gb2_add", c_void_p)]



class HeadFoldArgs(ctypes.Structure):
    """gm_head_fold_args (include/gm_hip.h): the folded critic head's partial dots + loss settings."""
    _fields_ = [("part", c_void_p), ("ldp", c_int64), ("nparts", c_int), ("snap", c_void_p),
                ("variant", c_int), ("out_act", c_int), ("hyper", c_float * 8), ("n_hyper", c_int),
                ("pen", c_void_p), ("S", c_void_p), ("dS", c_void_p), ("rowloss", c_void_p)]


class LabelSrc(ctypes.Structure):
    """gm_label_src (include/gm_hip.h): row m's class is labels[idx ? idx_row[m] : m] (int32 labels, int64 idx)."""
    _fields_ = [("labels", c_void_p), ("idx", c_void_p), ("idx_slot", Slot)]


class LabelGradArgs(ctypes.Structure):
    """gm_label_grad_args (include/gm_hip.h): one conditioned layer of gm_label_grad_adam."""
    _fields_ = [("dPre", c_void_p), ("ld", c_int64), ("N", c_int), ("gE", c_void_p), ("E", c_void_p),
                ("mE", c_void_p), ("vE", c_void_p)]


class DwAdamArgs(ctypes.Structure):
    """gm_dw_adam_args (include/gm_hip.h): one weight gradient of gm_linear_bwd_dw_ex (+ Adam, + the riding head)."""
    _fields_ = [("dA", c_void_p), ("lda", c_int64), ("X", c_void_p), ("ldx", c_int64),
                ("x_slot", Slot), ("dW", c_void_p), ("db", c_void_p), ("M", c_int), ("K", c_int),
                ("N", c_int), ("pW", c_void_p), ("mW", c_void_p), ("vW", c_void_p),
                ("pb", c_void_p), ("mb", c_void_p), ("vb", c_void_p), ("sched", c_void_p),
                ("sched_slot", Slot), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("clamp", c_float),
                ("accumulate", c_int), ("ones_from", c_int), ("head", POINTER(HeadBwdArgs)),
                ("fold", POINTER(HeadFoldArgs)), ("xbits", c_void_p), ("xbits_wpr", c_int), ("xbits_rows", c_int)]


class AAECriticArgs(ctypes.Structure):
    """gm_aae_critic_args (include/gm_hip.h): the adversarial autoencoder's critic step."""
    _fields_ = [("z_real", c_void_p), ("real_slot", Slot), ("z_fake", c_void_p), ("ld_fake", c_int64),
                ("B", c_int), ("Z", c_int), ("H", c_int),
                ("W1", c_void_p), ("b1", c_void_p), ("w2", c_void_p), ("b2", c_void_p),
                ("gW1", c_void_p), ("gb1", c_void_p), ("gw2", c_void_p), ("gb2", c_void_p),
                ("mW1", c_void_p), ("vW1", c_void_p), ("mb1", c_void_p), ("vb1", c_void_p),
                ("mw2", c_void_p), ("vw2", c_void_p), ("mb2", c_void_p), ("vb2", c_void_p),
                ("sched", c_void_p), ("sched_slot", Slot), ("beta1", ctypes.c_double), ("beta2", ctypes.c_double),
                ("eps", ctypes.c_double), ("weight_decay", ctypes.c_double), ("loss_out", c_void_p),
                ("loss_slot", Slot), ("ws", c_void_p), ("ws_bytes", c_int64)]


class AAEGenArgs(ctypes.Structure):
    """gm_aae_gen_args (include/gm_hip.h): the adversarial autoencoder's generator-phase middle launch."""
    _fields_ = [("z", c_void_p), ("ldz", c_int64), ("He", c_void_p), ("ldhe", c_int64),
                ("W1", c_void_p), ("b1", c_void_p), ("w2", c_void_p), ("b2", c_void_p), ("Wz", c_void_p),
                ("dz", c_void_p), ("lddz", c_int64), ("dHe", c_void_p), ("lddhe", c_int64),
                ("loss_part", c_void_p), ("B", c_int), ("Z", c_int), ("H", c_int)]


class SghmcSeg(ctypes.Structure):
    """gm_sghmc_seg (include/gm_hip.h): one tensor of an SGHMC launch."""
    _fields_ = [("offset", c_int64), ("numel", c_int64), ("stream", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class SghmcArgs(ctypes.Structure):
    """gm_sghmc_args (include/gm_hip.h): one SGHMC step over a segment table."""
    _fields_ = [("theta", c_void_p), ("grad", c_void_p), ("mom", c_void_p), ("n_flat", c_int64),
                ("segs", POINTER(SghmcSeg)), ("nseg", c_int), ("step", c_void_p), ("step_add", c_int64),
                ("lr", c_void_p), ("friction", c_float), ("prior", c_float), ("noise", c_float),
                ("seed", ctypes.c_uint64)]


class BganHeadArgs(ctypes.Structure):
    """gm_bgan_head_args (include/gm_hip.h): the Bayesian GAN's critic-ensemble head."""
    _fields_ = [("h", c_void_p), ("ldh", c_int64), ("w2", c_void_p), ("b2", c_void_p), ("gw2", c_void_p),
                ("gb2", c_void_p), ("loss_out", c_void_p), ("loss_slot", Slot), ("ws", c_void_p),
                ("ws_bytes", c_int64), ("mode", c_int), ("B", c_int), ("Jg", c_int), ("Jd", c_int), ("H", c_int)]


class CorruptArgs(ctypes.Structure):
    """gm_corrupt_args (include/gm_hip.h): the denoising VAE's corruption rule, seed, step and first row."""
    _fields_ = [("kind", c_int), ("level", ctypes.c_double), ("seed", ctypes.c_uint64), ("step_ctr", c_void_p),
                ("step_base", c_void_p), ("step_add", c_int64), ("row0", c_int64)]


IWAE_TAG_TRAIN, IWAE_TAG_EVAL = 0x49574145, 0x49574556      # GM_IWAE_TAG_TRAIN / GM_IWAE_TAG_EVAL
IWAE_MAX_K, IWAE_MAX_Z = 64, 32                             # GM_IWAE_MAX_K / GM_IWAE_MAX_Z
FLOW_MAX_K, FLOW_PART_STRIDE = 32, 68                       # GM_FLOW_MAX_K / GM_FLOW_PART_STRIDE
IAF_MIN_Z, IAF_MAX_Z, IAF_MAX_K, IAF_MIN_F, IAF_MAX_F, IAF_MAX_C = 2, 32, 8, 4, 64, 32     # GM_IAF_* (include/gm_hip.h)
IAF_PART_ROWS = 64                                          # GM_IAF_PART_ROWS
# (gm_iaf_params / gm_iaf_step_args travel by pointer; their ctypes forms live in ops_fused)
CAT_TAG_TRAIN, CAT_TAG_EVAL = 0x43415454, 0x43415445        # GM_CAT_TAG_TRAIN / GM_CAT_TAG_EVAL
CAT_MIN_C, CAT_MAX_C, CAT_MAX_NC = 2, 64, 1024              # GM_CAT_MIN_C / GM_CAT_MAX_C / GM_CAT_MAX_NC
CAT_RELAXED, CAT_ST, CAT_DISCRETE, CAT_NOISE = 0, 1, 2, 3   # GM_CAT_RELAXED / _ST / _DISCRETE / _NOISE
# (gm_cat_args travels by pointer too: CatArgs in ops_fused)
# (gm_iwae_noise, gm_flow_params, gm_flow_step_args, gm_acgan_heads_args and the gm_sn_*_args travel by pointer; their
# ctypes forms, IwaeNoise, FlowParams, FlowStepArgs, ACGANHeadsArgs and SNPowerArgs / SNHeadArgs / SNGradArgs, live in
# ops_fused beside their wrappers)

DDPM_TAG_T, DDPM_TAG_E, DDPM_TAG_V, DDPM_TAG_VE, DDPM_TAG_S = 0x44445054, 0x4444504D, 0x44445056, 0x44445057, 0x44445053
DDPM_MAX_I, DDPM_MIN_E, DDPM_MAX_E, DDPM_MAX_T = 8192, 4, 128, 4096      # GM_DDPM_* (include/gm_hip.h)
GMMN_TAG_T, GMMN_TAG_V, GMMN_TAG_S = 0x474D4D54, 0x474D4D56, 0x474D4D53    # GM_GMMN_TAG_* ("GMMT", "GMMV", "GMMS")
MMD_MAX_SIGMAS, MMD_MAX_I, MMD_CHUNK, GMMN_MAX_Z, GMMN_MAX_B = 16, 8192, 128, 8192, 2048    # GM_MMD_* / GM_GMMN_*
SWG_TAG_T, SWG_TAG_V, SWG_TAG_S = 0x53574754, 0x53574756, 0x53574753         # GM_SWG_TAG_* ("SWGT", "SWGV", "SWGS")
SWG_TAG_DT, SWG_TAG_DV, SWG_TAG_DM = 0x53574454, 0x53574456, 0x5357444D      # the directions ("SWDT", "SWDV", "SWDM")
SW_MAX_P, SW_MAX_B, SW_MAX_ROWS = 8192, 2048, 16384                          # GM_SW_* (include/gm_hip.h)
# (gm_ddpm_noise / _tables / _out / _reverse_args travel by pointer; their ctypes forms live in ops_fused)
# GM_FM_TAG_* ("FMTD", "FMTT", "FMTN": training dequantisation / time / normals; "FMVD", "FMVT", "FMVN": validation)
FM_TAG_D, FM_TAG_T, FM_TAG_N, FM_TAG_VD, FM_TAG_VT, FM_TAG_VN = (0x464D5444, 0x464D5454, 0x464D544E, 0x464D5644,
                                                                 0x464D5654, 0x464D564E)
FM_MAX_H = 1024                                                          # GM_FM_MAX_H

MADE_TAG_S = 0x4D414453                                     # GM_MADE_TAG_S ("MADS")
MADE_MIN_I, MADE_MAX_I, MADE_MAX_H = 2, 8192, 1024          # GM_MADE_* (include/gm_hip.h)
# (gm_made_mask_args / gm_made_sample_args travel by pointer; their ctypes forms live in ops_fused)

NVP_TAG_TRAIN, NVP_TAG_EVAL, NVP_TAG_S = 0x4E565044, 0x4E565056, 0x4E565053     # GM_NVP_TAG_* ("NVPD", "NVPV", "NVPS")
NVP_MIN_D, NVP_MAX_D, NVP_MAX_H, NVP_MAX_K = 2, 8192, 1024, 16              # GM_NVP_* (include/gm_hip.h)
NVP_MAX_LEVELS, NVP_MAX_S_CAP = 65536, 8
NVP_CHECKER, NVP_HALF = 0, 1                                # GM_NVP_CHECKER / GM_NVP_HALF
NVP_PRE, NVP_NOISE, NVP_POST, NVP_PRIOR = 0, 1, 0, 1        # gm_nvp_pre's and gm_nvp_post's modes
# (the gm_nvp_*_args travel by pointer; their ctypes forms live in ops_fused)

MAF_TAG_TRAIN, MAF_TAG_EVAL = 0x4D414644, 0x4D414656          # GM_MAF_TAG_TRAIN / GM_MAF_TAG_EVAL ("MAFD", "MAFV")
MAF_MIN_D, MAF_MAX_D, MAF_MAX_H, MAF_MAX_K = 2, 8192, 1024, 16              # GM_MAF_* (include/gm_hip.h)
# (the gm_maf_*_args travel by pointer; their ctypes forms live in ops_fused)

RBM_TAG_D, RBM_TAG_H, RBM_TAG_V = 0x52424D44, 0x52424D48, 0x52424D56      # GM_RBM_TAG_* ("RBMD", "RBMH", "RBMV")
RBM_MAX_DIM, RBM_MAX_STEPS = 1024, 1 << 24                  # GM_RBM_MAX_DIM / GM_RBM_MAX_STEPS
# (gm_rbm_chain_args / gm_rbm_vbias_args travel by pointer; their ctypes forms live in ops_fused)

VQ_MIN_D, VQ_MAX_D, VQ_MAX_ND = 4, 64, 1024                 # GM_VQ_MIN_D / GM_VQ_MAX_D / GM_VQ_MAX_ND
VQ_MIN_K, VQ_MAX_K, VQ_MAX_KD = 2, 1024, 16384              # GM_VQ_MIN_K / GM_VQ_MAX_K / GM_VQ_MAX_KD
# (gm_vq_args / gm_vq_step_args travel by pointer; their ctypes forms live in ops_fused)

NOISE = {"salt_pepper": 1, "gaussian": 2}       # GM_NOISE_SALT_PEPPER, GM_NOISE_GAUSSIAN (GM_NOISE_NONE = 0)


class Finalize2Args(ctypes.Structure):
    """gm_finalize2_args (include/gm_hip.h): the two loss sums + counter tick that ride in a VAE batch's last launch."""
    _fields_ = [("pa", c_void_p), ("na", c_int), ("scale_a", c_float), ("out_a", c_void_p), ("slot_a", Slot),
                ("pb", c_void_p), ("nb", c_int), ("scale_b", c_float), ("out_b", c_void_p), ("slot_b", Slot),
                ("tick", c_void_p), ("done", c_void_p)]


class DwTail(ctypes.Structure):
    """gm_dw_tail (include/gm_hip.h): what a pair of weight gradients carries -- the next first layer, or the sums."""
    _fields_ = [("z", c_void_p), ("ldz", c_int64), ("z_slot", Slot), ("H", c_void_p), ("ldh", c_int64),
                ("rows", c_int), ("fin", POINTER(Finalize2Args))]


class GatherArgs(ctypes.Structure):
    """gm_gather_args (include/gm_hip.h): one batch gather riding in a forward / input-gradient launch."""
    _fields_ = [("data", c_void_p), ("bits", c_void_p), ("words_per_row", c_int), ("n_rows", c_int64),
                ("idx", c_void_p), ("idx_slot", Slot), ("out", c_void_p), ("ld_out", c_int64),
                ("out_bits", c_void_p), ("B", c_int), ("row_elems", c_int), ("corrupt", POINTER(CorruptArgs)),
                ("out_c", c_void_p)]


class FwdArgs(ctypes.Structure):
    """gm_fwd_args (include/gm_hip.h): gm_linear_fwd_ex -- the base GEMM and at most one optional block."""
    _fields_ = [("X", c_void_p), ("ldx", c_int64), ("x_slot", Slot), ("W", c_void_p), ("bias", c_void_p),
                ("Y", c_void_p), ("ldy", c_int64), ("M", c_int), ("K", c_int), ("N", c_int), ("act", c_int),
                ("ip_eps", c_void_p), ("ip_slot", Slot), ("ip_x", c_void_p), ("ip_ldx", c_int64),
                ("ip_out", c_void_p), ("ip_ldo", c_int64), ("ip_rows", c_int),
                ("hd_w2", c_void_p), ("hd_b2", c_void_p), ("hd_part", c_void_p), ("hd_ldp", c_int64),
                ("hd_snap", c_void_p), ("xbits", c_void_p), ("xbits_wpr", c_int), ("xbits_rows", c_int),
                ("sq_target", c_void_p), ("sq_ldt", c_int64), ("sq_dA", c_void_p), ("sq_lda", c_int64),
                ("sq_part", c_void_p), ("sq_ldp", c_int64),
                ("lb_E", c_void_p), ("lb_C", c_int), ("lb", LabelSrc), ("gather", POINTER(GatherArgs))]


class DxArgs(ctypes.Structure):
    """gm_dx_args (include/gm_hip.h): gm_linear_bwd_dx_ex -- the base GEMM and at most one optional block."""
    _fields_ = [("dA", c_void_p), ("lda", c_int64), ("W", c_void_p), ("dX", c_void_p), ("ldx", c_int64),
                ("below", c_void_p), ("ld_below", c_int64), ("M", c_int), ("K", c_int), ("N", c_int), ("epi", c_int),
                ("add", c_void_p), ("ldadd", c_int64), ("add_scale", c_float),
                ("head", POINTER(HeadBwdArgs)), ("fold", POINTER(HeadFoldArgs)),
                ("rp_ml", c_void_p), ("rp_ldml", c_int64), ("rp_eps", c_void_p), ("rp_slot", Slot),
                ("rp_dml", c_void_p), ("rp_ldd", c_int64), ("gather", POINTER(GatherArgs))]


class DrawOp(ctypes.Structure):
    """gm_draw_op (include/gm_hip.h): one draw of the per-iteration host RNG program."""
    _fields_ = [("kind", c_int32), ("n", c_int32), ("a", c_int64), ("b", c_int32), ("c", c_int32),
                ("dst", c_void_p), ("iter_stride", c_int64), ("e0", c_int64), ("e1", c_int64)]


class StageSeg(ctypes.Structure):
    """gm_stage_seg (include/gm_hip.h)."""
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("bytes_per_iter", c_int64),
                ("blocks", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("src_block_stride", c_int64), ("dst_block_stride", c_int64)]


# gm_linear_plan (include/gm_hip.h): modes, kernel families, and the plan's fields in GM_PLAN_F_* order
PLAN_MODE = {"fwd": 0, "dx": 1, "dw": 2}
PLAN_FAMILY = {1: "lds", 2: "k32", 3: "split", 4: "riding"}
PLAN_FIELDS = ("family", "mode", "mi", "ni", "lds_cfg", "lds_stages", "vec", "xv", "vec_epi", "dma", "slots", "launches",
               "grid_x", "grid_y", "block")
PLAN_INTS = 16                                              # GM_PLAN_FIELDS

DRAW_SAMPLER, DRAW_NORMAL, DRAW_UNIFORM, DRAW_INFO = 0, 1, 2, 3
GM_EUNSUPPORTED = -10002

_P = c_void_p      # device pointers travel as integers (tensor.data_ptr())

_SIGNATURES = {
    "gm_version": (c_int, []),
    "gm_arch": (c_char_p, []),
    "gm_last_error": (c_char_p, []),
    "gm_tick": (c_int, [_P, _P, c_int64]),
    "gm_copy_slot_f32": (c_int, [_P, _P, Slot, _P, Slot, c_int64]),
    "gm_gather_rows": (c_int, [_P, _P, c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_linear_fwd": (c_int, [_P, _P, c_int64, Slot, _P, _P, _P, c_int64, c_int, c_int, c_int,
                              c_int]),
    "gm_linear_bwd_dx": (c_int, [_P, _P, c_int64, _P, _P, c_int64, _P, c_int64, c_int, c_int,
                                 c_int, c_int]),
    "gm_linear_bwd_dw": (c_int, [_P, _P, c_int64, _P, c_int64, Slot, _P, _P, c_int, c_int, c_int,
                                 c_int]),
    "gm_linear_fwd_ex": (c_int, [_P, POINTER(FwdArgs)]),
    "gm_linear_bwd_dx_ex": (c_int, [_P, POINTER(DxArgs)]),
    "gm_linear_bwd_dw_ex": (c_int, [_P, POINTER(DwAdamArgs), POINTER(DwAdamArgs), POINTER(DwTail)]),
    "gm_linear_plan": (c_int, [c_int, _P, POINTER(c_int32)]),
    "gm_gan_loss": (c_int, [_P, c_int, c_int, _P, _P, c_int, c_int, POINTER(c_float), c_int,
                            c_float, _P, Slot, _P, _P, _P, _P]),
    "gm_gan_loss_phase": (c_int, [_P, c_int, c_int, _P, _P, c_int, c_int, POINTER(c_float), c_int,
                                  c_float, _P, Slot, _P, _P, _P, _P, c_int, _P, c_float]),
    "gm_l1_rows_dp": (c_int, [_P, _P, c_int64, _P, c_int64, c_int, c_int, c_int, c_int, _P, _P, c_int64, _P]),
    "gm_began_dloss_dp": (c_int, [_P, _P, c_int, c_int, _P, _P, Slot]),
    "gm_std_sums": (c_int, [_P, _P, c_int64, c_int, c_int, _P, _P]),
    "gm_std_from_sums": (c_int, [_P, _P, c_int64, _P]),
    "gm_adam": (c_int, [_P, _P, _P, _P, _P, c_int64, _P, Slot, ctypes.c_double, ctypes.c_double,
                        ctypes.c_double, ctypes.c_double, c_float]),
    "gm_interp": (c_int, [_P, _P, Slot, _P, c_int64, _P, c_int64, _P, c_int64, c_int, c_int]),
    "gm_gp_u": (c_int, [_P, _P, _P, c_int64, _P, _P, c_int64, c_int, c_int]),
    "gm_gp_norm": (c_int, [_P, _P, c_int64, _P, c_int64, _P, c_float, c_float, c_float, c_int,
                           c_int]),
    "gm_gp_dw2": (c_int, [_P, _P, _P, c_int64, _P, c_int64, _P, c_int, c_int]),
    "gm_bir_reparam": (c_int, [_P, _P, c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_bir_mmd": (c_int, [_P, _P, c_int64, _P, Slot, _P, _P, c_int64, c_int, c_int, c_float]),
    "gm_vae_reparam": (c_int, [_P, _P, c_int64, _P, Slot, _P, c_int64, _P, Slot, c_int, c_int]),
    "gm_vae_reparam_bwd": (c_int, [_P, _P, c_int64, _P, Slot, _P, c_int64, _P, c_int64, c_int,
                                   c_int]),
    "gm_sqerr_sigmoid_bwd": (c_int, [_P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_int, c_int]),
    "gm_sum_finalize": (c_int, [_P, _P, c_int, c_float, _P, Slot]),
    "gm_sum_finalize_tick": (c_int, [_P, _P, c_int, c_float, _P, Slot, _P]),
    "gm_sum_finalize2_tick": (c_int, [_P, _P, c_int, c_float, _P, Slot, _P, c_int, c_float, _P, Slot, _P]),
    "gm_vae_reparam_wide": (c_int, [_P, _P, c_int64, _P, Slot, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_vae_bwd_mid": (c_int, [_P, _P, c_int64, _P, _P, c_int64, _P, Slot, _P, c_int64, _P, _P, c_int64, _P, c_int64,
                               c_int, c_int, c_int]),
    "gm_vae_reparam_fwd": (c_int, [_P, _P, c_int64, _P, Slot, _P, c_int64, _P, c_int, c_int, c_int, _P, _P, _P,
                                   c_int64, c_int, c_int]),
    "gm_gather_rows_bits": (c_int, [_P, _P, c_int, c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_gather_rows_bits_packed": (c_int, [_P, _P, c_int, c_int64, _P, Slot, _P, c_int]),
    "gm_gp_dw2_store": (c_int, [_P, _P, _P, c_int64, _P, c_int64, _P, c_int, c_int]),
    "gm_head_gp": (c_int, [_P, _P, c_int64, _P, _P, _P, _P, c_int64, c_int, c_int]),
    "gm_head_bwd_fused": (c_int, [_P, _P, c_int64, _P, _P, _P, _P, _P, c_int64, _P, _P, _P, Slot,
                                  c_float, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, Slot,
                                  ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                  ctypes.c_double, c_float, _P]),
    "gm_head_fwd_loss": (c_int, [_P, c_int, c_int, _P, c_int64, _P, _P, c_int, c_int, c_int,
                                 POINTER(c_float), c_int, c_float, _P, _P, _P, _P, _P, c_int64]),
    "gm_head_fwd_loss_final": (c_int, [_P, c_int, c_int, _P, c_int64, _P, _P, c_int, c_int, c_int,
                                       POINTER(c_float), c_int, c_float, _P, _P, _P, _P, _P, c_int64,
                                       _P, Slot, _P, _P]),
    "gm_head_bwd": (c_int, [_P, _P, c_int64, _P, _P, _P, _P, c_int64, _P, _P, _P, Slot, c_float,
                            c_int, c_int, c_int]),
    "gm_clock_probe": (c_int, [_P, c_int, _P, _P]),
    "gm_stream_create": (c_int, [POINTER(c_void_p)]),
    "gm_stream_destroy": (c_int, [_P]),
    "gm_stream_wait_event": (c_int, [_P, _P]),
    "gm_l1_rows": (c_int, [_P, _P, c_int64, _P, c_int64, c_int, c_int, c_int, _P, _P, c_int64, _P]),
    "gm_began_dloss": (c_int, [_P, _P, c_int, _P, _P, Slot]),
    "gm_began_update": (c_int, [_P, _P, _P, _P, c_float, c_float, c_int64, _P]),
    "gm_adam_scaled": (c_int, [_P, _P, _P, _P, _P, c_int64, _P, Slot, ctypes.c_double, ctypes.c_double,
                               ctypes.c_double, ctypes.c_double, c_float, _P]),
    "gm_std_all": (c_int, [_P, _P, c_int64, c_int, c_int, _P, _P]),
    "gm_dragan_xhat": (c_int, [_P, _P, c_int64, _P, Slot, _P, Slot, _P, c_float, _P, c_int64, c_int,
                               c_int]),
    "gm_dragan_rows": (c_int, [_P, _P, _P, c_int64, _P, c_int64, _P, _P, c_float, c_float, c_float,
                               c_int, c_int]),
    "gm_dragan_head_bwd": (c_int, [_P, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int64, c_int,
                                   c_int]),
    "gm_fisher_commit": (c_int, [_P, _P]),
    "gm_dragan_head_bwd_store": (c_int, [_P, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int64, c_int,
                                   c_int]),
    "gm_info_q_loss": (c_int, [_P, _P, c_int64, _P, Slot, c_int64, c_int, c_int, c_int, c_int, c_float,
                               _P, c_int64, _P, Slot]),
    "gm_info_q_loss_dp": (c_int, [_P, _P, c_int64, _P, Slot, c_int64, c_int, c_int, c_int, c_int, c_int, c_float,
                                  _P, c_int64, _P, Slot]),
    "gm_act_bwd": (c_int, [_P, _P, _P, _P, c_int64, c_int]),
    "gm_randperm_prefix": (c_int, [ctypes.c_uint64, c_int64, c_int, _P]),
    "gm_mt19937_skip": (c_int, [_P, c_int64, ctypes.c_uint64]),
    "gm_comm_create": (c_int, [c_int, c_int, c_int64, POINTER(c_void_p), _P]),
    "gm_comm_connect": (c_int, [_P, _P]),
    "gm_comm_destroy": (c_int, [_P]),
    "gm_comm_error": (c_int, [_P, POINTER(c_int)]),
    "gm_comm_info": (c_int, [_P, POINTER(c_int)]),
    "gm_rccl_available": (c_int, []),
    "gm_rccl_unique_id": (c_int, [_P]),
    "gm_rccl_comm_create": (c_int, [c_int, c_int, _P, POINTER(c_void_p)]),
    "gm_rccl_allreduce_f32": (c_int, [_P, _P, _P, c_int64]),
    "gm_rccl_comm_destroy": (c_int, [_P]),
    "gm_comm_set_exchange": (c_int, [_P, c_int]),
    "gm_comm_set_max_blocks": (c_int, [_P, c_int]),
    "gm_comm_set_wait_seconds": (c_int, [_P, ctypes.c_double]),
    "gm_comm_buffer": (c_int, [_P, POINTER(c_void_p), POINTER(c_int64)]),
    "gm_allreduce_f32": (c_int, [_P, _P, _P, c_int64]),
    "gm_allreduce_adam_f32": (c_int, [_P, _P, _P, c_int64, _P, _P, _P, _P, Slot, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_double, ctypes.c_double, c_float, _P]),
    "gm_allreduce_scalars": (c_int, [_P, _P, _P, c_int]),
    "gm_stage_in": (c_int, [_P, POINTER(StageSeg), c_int, Slot, c_int]),
    "gm_stage_in_gated": (c_int, [_P, POINTER(StageSeg), c_int, Slot, c_int, _P, Slot, ctypes.c_double, _P,
                                  c_int]),
    "gm_host_device_ptr": (c_int, [_P, POINTER(c_void_p)]),
    "gm_host_replay": (c_int, [_P, c_int64, POINTER(DrawOp), c_int, c_int]),
    "gm_host_replay_threads": (c_int, [c_int]),
    "gm_numpy_legacy_normal_f32": (c_int, [_P, _P, _P, _P, ctypes.c_double, ctypes.c_double, c_int64, _P, c_int]),
    "gm_fill_submit": (c_int64, [_P, c_int64, POINTER(DrawOp), c_int, c_int, _P, c_int64]),
    "gm_fill_wait": (c_int, [c_int64]),
    "gm_fill_completed": (c_int64, []),
    "gm_fill_reset": (c_int, []),
    "gm_host_replay_flavour": (c_int, [c_int]),
    "gm_graph_begin": (c_int, [_P]),
    "gm_graph_end": (c_int, [_P, POINTER(c_void_p)]),
    "gm_graph_launch": (c_int, [_P, _P]),
    "gm_graph_destroy": (c_int, [_P]),
    "gm_event_create": (c_int, [POINTER(c_void_p)]),
    "gm_event_record": (c_int, [_P, _P]),
    "gm_event_sync": (c_int, [_P]),
    "gm_event_elapsed_ms": (c_int, [_P, _P, POINTER(c_float)]),
    "gm_event_destroy": (c_int, [_P]),
    "gm_vae_reparam_fwd_label": (c_int, [_P, _P, c_int64, _P, Slot, _P, c_int64, _P, c_int, c_int, c_int, _P, _P, _P,
                                         c_int64, c_int, c_int, _P, c_int, LabelSrc]),
    "gm_label_grad_adam": (c_int, [_P, POINTER(LabelGradArgs), c_int, LabelSrc, c_int, c_int, _P, Slot,
                                   ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "gm_parzen_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "gm_aae_critic_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "gm_aae_critic_step": (c_int, [_P, POINTER(AAECriticArgs)]),
    "gm_aae_gen_mid": (c_int, [_P, POINTER(AAEGenArgs)]),
    "gm_acgan_heads_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "gm_acgan_heads_fwd": (c_int, [_P, _P]),
    "gm_acgan_heads_bwd": (c_int, [_P, _P]),
    "gm_sn_power_workspace_bytes": (c_int64, [c_int, c_int]),
    "gm_sn_power_iter": (c_int, [_P, _P]),
    "gm_sn_head_workspace_bytes": (c_int64, [c_int, c_int]),
    "gm_sn_head_fwd": (c_int, [_P, _P]),
    "gm_sn_head_bwd": (c_int, [_P, _P]),
    "gm_sn_grad_workspace_bytes": (c_int64, [c_int]),
    "gm_sn_grad": (c_int, [_P, _P]),
    "gm_philox_raw": (c_int, [_P, _P, _P, _P, c_int64]),
    "gm_philox_normal": (c_int, [_P, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, c_int, _P, c_int64, _P,
                                 c_int64]),
    "gm_sghmc_step": (c_int, [_P, POINTER(SghmcArgs)]),
    "gm_bgan_head_workspace_bytes": (c_int64, [c_int, c_int, c_int, c_int, c_int]),
    "gm_bgan_head": (c_int, [_P, POINTER(BganHeadArgs)]),
    "gm_parzen_ll": (c_int, [_P, _P, c_int64, c_int, _P, c_int64, c_int, c_int, _P, c_int, _P, c_int64, _P,
                             c_int64]),
    "gm_dvae_corrupt": (c_int, [_P, POINTER(CorruptArgs), _P, c_int64, _P, c_int64, c_int64, c_int]),
    "gm_gather_rows_corrupt": (c_int, [_P, POINTER(CorruptArgs), _P, c_int64, _P, Slot, _P, _P, c_int64, c_int,
                                       c_int]),
    "gm_gather_rows_bits_corrupt": (c_int, [_P, POINTER(CorruptArgs), _P, c_int, c_int64, _P, Slot, _P, _P, c_int64,
                                            c_int, c_int]),
    "gm_pdw_couple": (c_int, [_P, _P, c_int64, _P, c_int64, _P, Slot, _P, _P, _P, c_int64, _P, c_int64, _P, c_int64,
                              c_float, c_int, c_int]),
    "gm_pdw_dir": (c_int, [_P, _P, c_int64, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_float, c_float, c_int,
                           c_int]),
    "gm_iwae_sample": (c_int, [_P, _P, _P, c_int64, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_iwae_weights": (c_int, [_P, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_iwae_reduce": (c_int, [_P, _P, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, c_int,
                               c_int, c_int]),
    "gm_flow_sample": (c_int, [_P, _P, _P, _P, c_int64, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_flow_reduce": (c_int, [_P, _P, _P, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_flow_step": (c_int, [_P, _P]),
    "gm_iaf_sample": (c_int, [_P, _P, _P, _P, c_int64, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_iaf_reduce": (c_int, [_P, _P, _P, _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_iaf_step": (c_int, [_P, _P]),
    "gm_tc_sample": (c_int, [_P, _P, _P, c_int64, _P, c_int64, _P, _P, _P, c_int64, _P, _P, c_float, c_float, c_float,
                             c_float, c_int, c_int, c_int]),
    "gm_tc_reduce": (c_int, [_P, _P, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P, _P, c_int64, _P, c_int64, c_float,
                             c_float, c_float, c_int, c_int, c_int]),
    "gm_mmd_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "gm_gmmn_prior": (c_int, [_P, _P, _P, c_int64, c_int, c_int]),
    "gm_mmd_pairs": (c_int, [_P, _P, c_int64, c_int, _P, c_int64, c_int, c_int, _P, c_int, _P, c_int64, _P, _P, c_int64]),
    "gm_mmd_finalize": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, c_int64, _P, _P, _P]),
    "gm_mmd_grad": (c_int, [_P, _P, c_int64, _P, _P, c_int64, _P, _P, c_float, c_int, _P, c_int64, c_int, c_int]),
    "gm_sw_workspace_bytes": (c_int64, [c_int]),
    "gm_sw_directions": (c_int, [_P, _P, _P, c_int64, c_int, c_int]),
    "gm_sw_sort": (c_int, [_P, _P, c_int64, c_int, c_int, c_int, _P, c_int64, _P, c_int64]),
    "gm_sw_finalize": (c_int, [_P, c_int, c_int, c_int, _P, c_int64, _P, _P]),
    "gm_cat_sample": (c_int, [_P, _P, _P]),
    "gm_cat_reduce": (c_int, [_P, _P, _P]),
    "gm_vq_quantise": (c_int, [_P, _P]),
    "gm_vq_reduce": (c_int, [_P, _P]),
    "gm_vq_step": (c_int, [_P, _P]),
    "gm_ddpm_qsample": (c_int, [_P, _P, _P, _P, _P, c_int64, c_int64, c_int]),
    "gm_gather_rows_qsample": (c_int, [_P, _P, _P, _P, _P, c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_gather_rows_bits_qsample": (c_int, [_P, _P, _P, _P, _P, c_int, c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_ddpm_loss": (c_int, [_P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_float, c_int, c_int]),
    "gm_ddpm_reverse": (c_int, [_P, _P]),
    "gm_ddpm_prior": (c_int, [_P, _P, c_int64, _P, ctypes.c_uint64, c_int64, c_int, _P, c_int, c_int, c_int, c_int]),
    "gm_fm_qsample": (c_int, [_P, _P, _P, _P, _P, c_int64, c_int64, c_int]),
    "gm_gather_rows_fm_qsample": (c_int, [_P, _P, _P, _P, _P, c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_gather_rows_bits_fm_qsample": (c_int, [_P, _P, _P, _P, _P, c_int, c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_fm_div": (c_int, [_P, _P]),
    "gm_fm_stage": (c_int, [_P, _P]),
    "gm_made_bce": (c_int, [_P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_float, c_int, c_int]),
    "gm_made_mask": (c_int, [_P, _P]),
    "gm_made_sample": (c_int, [_P, _P]),
    "gm_made_uniform": (c_int, [_P, _P, c_int64, ctypes.c_uint64, c_int64, c_int64, c_int]),
    "gm_nvp_pre": (c_int, [_P, _P]),
    "gm_nvp_couple": (c_int, [_P, _P]),
    "gm_nvp_loss": (c_int, [_P, _P]),
    "gm_nvp_couple_bwd": (c_int, [_P, _P]),
    "gm_nvp_post": (c_int, [_P, _P]),
    "gm_maf_couple": (c_int, [_P, _P]),
    "gm_maf_couple_bwd": (c_int, [_P, _P]),
    "gm_maf_mask": (c_int, [_P, _P]),
    "gm_maf_invert": (c_int, [_P, _P]),
    "gm_rbm_chain": (c_int, [_P, _P]),
    "gm_rbm_grad": (c_int, [_P, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_float, c_int, c_int, c_int]),
    "gm_rbm_vbias": (c_int, [_P, _P]),
    "gm_rbm_transpose": (c_int, [_P, _P, c_int64, _P, c_int64, c_int, c_int]),
    "gm_rbm_uniform": (c_int, [_P, _P, c_int64, ctypes.c_uint64, ctypes.c_uint32, _P, _P, c_int64, c_int64, c_int64,
                               c_int]),
}

_lib = None


class GMError(RuntimeError):
    pass


def check_int(v, name, error=GMError):
    """int(v) of an integer (Python's or numpy's, no bool); else `error`: the models' argument validator, raised as
    the calling module's own error class."""
    import numpy as np
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise error("%s must be an integer, got %r" % (name, v))
    return int(v)


def check_real(v, name, error=GMError):
    """float(v) of a finite number (Python's or numpy's, no bool); else `error`."""
    import math
    import numpy as np
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise error("%s must be a number, got %r" % (name, v))
    v = float(v)
    if not math.isfinite(v):
        raise error("%s must be finite, got %r" % (name, v))
    return v


def check_seed(seed, name="seed", error=GMError):
    """A counter-generator seed: an integer in [0, 2^64); else `error`."""
    seed = check_int(seed, name, error)
    if not 0 <= seed < 1 << 64:
        raise error("%s must lie in [0, 2^64), got %d" % (name, seed))
    return seed


def load():
    """Load libgm_hip.so; raise loudly if it is not there (build with __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise GMError("HIP extension %s is missing -- run `python __graft_entry__.py build` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().gm_last_error()
        raise GMError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else "?"))


def call(name, *args):
    check(getattr(load(), name)(*args), name)


def declared_symbols():
    """Every function declared in include/gm_hip.h (parsed), for the export test."""
    import re
    hdr = os.path.join(os.path.dirname(HERE), "include", "gm_hip.h")
    text = open(hdr).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gm_[a-z0-9_]+)\s*\(", text)))
