"""The C-ABI of libgm_hip.so as ctypes declarations: every struct, constant and prototype of include/gm_hip.h, once.

Nothing is loaded here (that is _lib's job) and nothing but ctypes is imported.  tests/test_abi_cpu.py compares all of it
with the header: layouts and field names, parameter lists and return types, and every #define and enum value.  A model
that adds to the header adds its structs, constants and signatures here, and no test of its own for them."""
import ctypes
from ctypes import (POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p)

_P = c_void_p      # device pointers, streams and handles travel as integers (tensor.data_ptr())

# ---- constants (#define GM_<NAME> and the enums; the header's comments say what each one bounds) ---------------------
GM_EINVAL, GM_EUNSUPPORTED = -10001, -10002
ACT_ID, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ACT = {"id": ACT_ID, None: ACT_ID, "relu": ACT_RELU, "sigmoid": ACT_SIGMOID}
LOSS = {"ns": 0, "mm": 1, "w": 2, "ls": 3, "ra": 4, "fisher": 5, "f_total_variation": 6,
        "f_forward_kl": 7, "f_reverse_kl": 8, "f_pearson": 9, "f_hellinger": 10,
        "f_jensen_shannon": 11}
DRAW_SAMPLER, DRAW_NORMAL, DRAW_UNIFORM, DRAW_INFO = 0, 1, 2, 3
NOISE = {"salt_pepper": 1, "gaussian": 2}       # GM_NOISE_SALT_PEPPER, GM_NOISE_GAUSSIAN (GM_NOISE_NONE = 0)
STD_WS_BYTES = 1088

# gm_linear_plan: modes, kernel families, and the plan's fields in GM_PLAN_F_* order
PLAN_MODE = {"fwd": 0, "dx": 1, "dw": 2}
PLAN_FAMILY = {1: "lds", 2: "k32", 3: "split", 4: "riding"}
PLAN_FIELDS = ("family", "mode", "mi", "ni", "lds_cfg", "lds_stages", "vec", "xv", "vec_epi", "dma", "slots", "launches",
               "grid_x", "grid_y", "block")
PLAN_INTS = 16                                              # GM_PLAN_FIELDS

SN_MAX_H, SN_MAX_I = 1024, 8192
SN_SIGMA, SN_NW2, SN_NT, SN_NR = 0, 1, 2, 3                 # GM_SN_STAT_*
IWAE_TAG_TRAIN, IWAE_TAG_EVAL = 0x49574145, 0x49574556      # "IWAE", "IWEV"
IWAE_MAX_K, IWAE_MAX_Z = 64, 32
FLOW_MAX_K, FLOW_PART_STRIDE = 32, 68
IAF_MIN_Z, IAF_MAX_Z, IAF_MAX_K, IAF_MIN_F, IAF_MAX_F, IAF_MAX_C = 2, 32, 8, 4, 64, 32
IAF_PART_ROWS = 64
CAT_TAG_TRAIN, CAT_TAG_EVAL = 0x43415454, 0x43415445        # "CATT", "CATE"
CAT_MIN_C, CAT_MAX_C, CAT_MAX_NC = 2, 64, 1024
CAT_RELAXED, CAT_ST, CAT_DISCRETE, CAT_NOISE = 0, 1, 2, 3
DDPM_TAG_T, DDPM_TAG_E, DDPM_TAG_V, DDPM_TAG_VE, DDPM_TAG_S = 0x44445054, 0x4444504D, 0x44445056, 0x44445057, 0x44445053
DDPM_MAX_I, DDPM_MIN_E, DDPM_MAX_E, DDPM_MAX_T = 8192, 4, 128, 4096
GMMN_TAG_T, GMMN_TAG_V, GMMN_TAG_S = 0x474D4D54, 0x474D4D56, 0x474D4D53    # "GMMT", "GMMV", "GMMS"
MMD_MAX_SIGMAS, MMD_MAX_I, MMD_CHUNK, GMMN_MAX_Z, GMMN_MAX_B = 16, 8192, 128, 8192, 2048
SWG_TAG_T, SWG_TAG_V, SWG_TAG_S = 0x53574754, 0x53574756, 0x53574753         # "SWGT", "SWGV", "SWGS"
SWG_TAG_DT, SWG_TAG_DV, SWG_TAG_DM = 0x53574454, 0x53574456, 0x5357444D      # the directions: "SWDT", "SWDV", "SWDM"
SW_MAX_P, SW_MAX_B, SW_MAX_ROWS = 8192, 2048, 16384
# "FMTD", "FMTT", "FMTN": training dequantisation / time / normals; "FMVD", "FMVT", "FMVN": validation
FM_TAG_D, FM_TAG_T, FM_TAG_N, FM_TAG_VD, FM_TAG_VT, FM_TAG_VN = (0x464D5444, 0x464D5454, 0x464D544E, 0x464D5644,
                                                                 0x464D5654, 0x464D564E)
FM_MAX_H = 1024
MADE_TAG_S = 0x4D414453                                     # "MADS"
MADE_MIN_I, MADE_MAX_I, MADE_MAX_H = 2, 8192, 1024
NVP_TAG_TRAIN, NVP_TAG_EVAL, NVP_TAG_S = 0x4E565044, 0x4E565056, 0x4E565053     # "NVPD", "NVPV", "NVPS"
NVP_MIN_D, NVP_MAX_D, NVP_MAX_H, NVP_MAX_K = 2, 8192, 1024, 16
NVP_MAX_LEVELS, NVP_MAX_S_CAP = 65536, 8
NVP_CHECKER, NVP_HALF = 0, 1
NVP_PRE, NVP_NOISE, NVP_POST, NVP_PRIOR = 0, 1, 0, 1        # gm_nvp_pre's and gm_nvp_post's modes
NSF_MIN_BINS, NSF_MAX_BINS, NSF_MAX_TAIL = 4, 16, 64
MAF_TAG_TRAIN, MAF_TAG_EVAL = 0x4D414644, 0x4D414656        # "MAFD", "MAFV"
MAF_MIN_D, MAF_MAX_D, MAF_MAX_H, MAF_MAX_K = 2, 8192, 1024, 16
RBM_TAG_D, RBM_TAG_H, RBM_TAG_V = 0x52424D44, 0x52424D48, 0x52424D56      # "RBMD", "RBMH", "RBMV"
RBM_MAX_DIM, RBM_MAX_STEPS = 1024, 1 << 24
VQ_MIN_D, VQ_MAX_D, VQ_MAX_ND = 4, 64, 1024
VQ_MIN_K, VQ_MAX_K, VQ_MAX_KD = 2, 1024, 16384


# ---- structs, in the header's order -----------------------------------------------------------------------------------
class Slot(ctypes.Structure):
    """((ctr ? *ctr : 0) * mul + add) % ring * stride."""
    c_name = "gm_slot"
    _fields_ = [("ctr", _P), ("mul", c_int32), ("add", c_int32), ("ring", c_int32), ("stride", c_int64)]


def slot(ctr=0, mul=0, add=0, ring=0, stride=0):
    return Slot(ctr or None, mul, add, ring, stride)


NO_SLOT = Slot(None, 0, 0, 0, 0)


class HeadBwdArgs(ctypes.Structure):
    """gm_head_bwd_fused's arguments as one block."""
    c_name = "gm_head_bwd_args"
    _fields_ = [("H", _P), ("ldh", c_int64), ("dS", _P), ("w2", _P), ("b2", _P), ("rowloss", _P), ("dH", _P),
                ("lddh", c_int64), ("gw2", _P), ("gb2", _P), ("loss_out", _P), ("loss_slot", Slot),
                ("inv_b", c_float), ("gen_mode", c_int), ("B", c_int), ("Hd", c_int), ("with_adam", c_int),
                ("mW", _P), ("vW", _P), ("mb", _P), ("vb", _P), ("sched", _P), ("sched_slot", Slot),
                ("beta1", c_double), ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double),
                ("clamp", c_float), ("tick", _P), ("gw2_add", _P), ("pen_s", _P), ("pen_h", _P), ("pen_ldh", c_int64),
                ("pen_t", _P), ("pen_ldt", c_int64), ("pen_rows", c_int), ("gb2_add", _P)]


class HeadFoldArgs(ctypes.Structure):
    """The folded critic head's partial dots + loss settings."""
    c_name = "gm_head_fold_args"
    _fields_ = [("part", _P), ("ldp", c_int64), ("nparts", c_int), ("snap", _P), ("variant", c_int),
                ("out_act", c_int), ("hyper", c_float * 8), ("n_hyper", c_int), ("pen", _P), ("S", _P), ("dS", _P),
                ("rowloss", _P)]


class StageSeg(ctypes.Structure):
    """One segment of a gm_stage_in copy."""
    c_name = "gm_stage_seg"
    _fields_ = [("src", _P), ("dst", _P), ("bytes_per_iter", c_int64), ("blocks", c_int32), ("reserved", c_int32),
                ("src_block_stride", c_int64), ("dst_block_stride", c_int64)]


class DrawOp(ctypes.Structure):
    """One draw of the per-iteration host RNG program."""
    c_name = "gm_draw_op"
    _fields_ = [("kind", c_int32), ("n", c_int32), ("a", c_int64), ("b", c_int32), ("c", c_int32), ("dst", _P),
                ("iter_stride", c_int64), ("e0", c_int64), ("e1", c_int64)]


class LabelSrc(ctypes.Structure):
    """Row m's class is labels[idx ? idx_row[m] : m] (int32 labels, int64 idx)."""
    c_name = "gm_label_src"
    _fields_ = [("labels", _P), ("idx", _P), ("idx_slot", Slot)]


class LabelGradArgs(ctypes.Structure):
    """One conditioned layer of gm_label_grad_adam."""
    c_name = "gm_label_grad_args"
    _fields_ = [("dPre", _P), ("ld", c_int64), ("N", c_int), ("gE", _P), ("E", _P), ("mE", _P), ("vE", _P)]


class AAECriticArgs(ctypes.Structure):
    """The adversarial autoencoder's critic step."""
    c_name = "gm_aae_critic_args"
    _fields_ = [("z_real", _P), ("real_slot", Slot), ("z_fake", _P), ("ld_fake", c_int64), ("B", c_int), ("Z", c_int),
                ("H", c_int), ("W1", _P), ("b1", _P), ("w2", _P), ("b2", _P), ("gW1", _P), ("gb1", _P), ("gw2", _P),
                ("gb2", _P), ("mW1", _P), ("vW1", _P), ("mb1", _P), ("vb1", _P), ("mw2", _P), ("vw2", _P),
                ("mb2", _P), ("vb2", _P), ("sched", _P), ("sched_slot", Slot), ("beta1", c_double),
                ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double), ("loss_out", _P),
                ("loss_slot", Slot), ("ws", _P), ("ws_bytes", c_int64)]


class AAEGenArgs(ctypes.Structure):
    """The adversarial autoencoder's generator-phase middle launch."""
    c_name = "gm_aae_gen_args"
    _fields_ = [("z", _P), ("ldz", c_int64), ("He", _P), ("ldhe", c_int64), ("W1", _P), ("b1", _P), ("w2", _P),
                ("b2", _P), ("Wz", _P), ("dz", _P), ("lddz", c_int64), ("dHe", _P), ("lddhe", c_int64),
                ("loss_part", _P), ("B", c_int), ("Z", c_int), ("H", c_int)]


class ACGANHeadsArgs(ctypes.Structure):
    """The AC-GAN critic's two heads, forward and backward."""
    c_name = "gm_acgan_heads_args"
    _fields_ = [("H", _P), ("ldh", c_int64), ("rows", c_int), ("B", c_int), ("Hd", c_int), ("C", c_int),
                ("gen_mode", c_int), ("w2", _P), ("b2", _P), ("Wc", _P), ("bc", _P), ("lab", LabelSrc),
                ("class_weight", c_float), ("da2", _P), ("dq", _P), ("lddq", c_int64), ("loss_out", _P),
                ("loss_slot", Slot), ("ce_out", _P), ("ce_slot", Slot), ("acc_out", _P), ("acc_slot", Slot),
                ("dPre", _P), ("ldp", c_int64), ("gw2", _P), ("gb2", _P), ("gWc", _P), ("gbc", _P), ("mw2", _P),
                ("vw2", _P), ("mb2", _P), ("vb2", _P), ("mWc", _P), ("vWc", _P), ("mbc", _P), ("vbc", _P),
                ("sched", _P), ("sched_slot", Slot), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("ws", _P), ("ws_bytes", c_int64)]


class SNPowerArgs(ctypes.Structure):
    """The power-iteration stage in front of a critic forward."""
    c_name = "gm_sn_power_args"
    _fields_ = [("W", _P), ("H", c_int), ("I", c_int), ("u", _P), ("v", _P), ("Wbar", _P), ("w2", _P), ("w2bar", _P),
                ("stats", _P), ("update_u", c_int), ("ws", _P), ("ws_bytes", c_int64)]


class SNHeadArgs(ctypes.Structure):
    """The hinge head on the normalised w2, forward and backward."""
    c_name = "gm_sn_head_args"
    _fields_ = [("H", _P), ("ldh", c_int64), ("rows", c_int), ("B", c_int), ("Hd", c_int), ("gen_mode", c_int),
                ("w2bar", _P), ("b2", _P), ("s", _P), ("ds", _P), ("loss_out", _P), ("loss_slot", Slot), ("dPre", _P),
                ("ldp", c_int64), ("stats", _P), ("gw2", _P), ("gb2", _P), ("ws", _P), ("ws_bytes", c_int64)]


class SNGradArgs(ctypes.Structure):
    """d loss / d Wbar carried back to W."""
    c_name = "gm_sn_grad_args"
    _fields_ = [("G", _P), ("Wbar", _P), ("H", c_int), ("I", c_int), ("u", _P), ("v", _P), ("stats", _P), ("gW", _P),
                ("ws", _P), ("ws_bytes", c_int64)]


class SghmcSeg(ctypes.Structure):
    """One tensor of an SGHMC launch."""
    c_name = "gm_sghmc_seg"
    _fields_ = [("offset", c_int64), ("numel", c_int64), ("stream", c_uint32), ("reserved", c_uint32)]


class SghmcArgs(ctypes.Structure):
    """One SGHMC step over a segment table."""
    c_name = "gm_sghmc_args"
    _fields_ = [("theta", _P), ("grad", _P), ("mom", _P), ("n_flat", c_int64), ("segs", POINTER(SghmcSeg)),
                ("nseg", c_int), ("step", _P), ("step_add", c_int64), ("lr", _P), ("friction", c_float),
                ("prior", c_float), ("noise", c_float), ("seed", c_uint64)]


class BganHeadArgs(ctypes.Structure):
    """The Bayesian GAN's critic-ensemble head."""
    c_name = "gm_bgan_head_args"
    _fields_ = [("h", _P), ("ldh", c_int64), ("w2", _P), ("b2", _P), ("gw2", _P), ("gb2", _P), ("loss_out", _P),
                ("loss_slot", Slot), ("ws", _P), ("ws_bytes", c_int64), ("mode", c_int), ("B", c_int), ("Jg", c_int),
                ("Jd", c_int), ("H", c_int)]


class CorruptArgs(ctypes.Structure):
    """The denoising VAE's corruption rule, seed, step and first row."""
    c_name = "gm_corrupt_args"
    _fields_ = [("kind", c_int), ("level", c_double), ("seed", c_uint64), ("step_ctr", _P), ("step_base", _P),
                ("step_add", c_int64), ("row0", c_int64)]


class GatherArgs(ctypes.Structure):
    """One batch gather riding in a forward / input-gradient launch."""
    c_name = "gm_gather_args"
    _fields_ = [("data", _P), ("bits", _P), ("words_per_row", c_int), ("n_rows", c_int64), ("idx", _P),
                ("idx_slot", Slot), ("out", _P), ("ld_out", c_int64), ("out_bits", _P), ("B", c_int),
                ("row_elems", c_int), ("corrupt", POINTER(CorruptArgs)), ("out_c", _P)]


class FwdArgs(ctypes.Structure):
    """gm_linear_fwd_ex: the base GEMM and at most one optional block."""
    c_name = "gm_fwd_args"
    _fields_ = [("X", _P), ("ldx", c_int64), ("x_slot", Slot), ("W", _P), ("bias", _P), ("Y", _P), ("ldy", c_int64),
                ("M", c_int), ("K", c_int), ("N", c_int), ("act", c_int),
                ("ip_eps", _P), ("ip_slot", Slot), ("ip_x", _P), ("ip_ldx", c_int64), ("ip_out", _P),
                ("ip_ldo", c_int64), ("ip_rows", c_int),
                ("hd_w2", _P), ("hd_b2", _P), ("hd_part", _P), ("hd_ldp", c_int64), ("hd_snap", _P),
                ("xbits", _P), ("xbits_wpr", c_int), ("xbits_rows", c_int),
                ("sq_target", _P), ("sq_ldt", c_int64), ("sq_dA", _P), ("sq_lda", c_int64), ("sq_part", _P),
                ("sq_ldp", c_int64),
                ("lb_E", _P), ("lb_C", c_int), ("lb", LabelSrc), ("gather", POINTER(GatherArgs))]


class DxArgs(ctypes.Structure):
    """gm_linear_bwd_dx_ex: the base GEMM and at most one optional block."""
    c_name = "gm_dx_args"
    _fields_ = [("dA", _P), ("lda", c_int64), ("W", _P), ("dX", _P), ("ldx", c_int64), ("below", _P),
                ("ld_below", c_int64), ("M", c_int), ("K", c_int), ("N", c_int), ("epi", c_int),
                ("add", _P), ("ldadd", c_int64), ("add_scale", c_float),
                ("head", POINTER(HeadBwdArgs)), ("fold", POINTER(HeadFoldArgs)),
                ("rp_ml", _P), ("rp_ldml", c_int64), ("rp_eps", _P), ("rp_slot", Slot), ("rp_dml", _P),
                ("rp_ldd", c_int64), ("gather", POINTER(GatherArgs))]


class DwAdamArgs(ctypes.Structure):
    """One weight gradient of gm_linear_bwd_dw_ex (+ Adam, + the riding head)."""
    c_name = "gm_dw_adam_args"
    _fields_ = [("dA", _P), ("lda", c_int64), ("X", _P), ("ldx", c_int64), ("x_slot", Slot), ("dW", _P), ("db", _P),
                ("M", c_int), ("K", c_int), ("N", c_int), ("pW", _P), ("mW", _P), ("vW", _P), ("pb", _P), ("mb", _P),
                ("vb", _P), ("sched", _P), ("sched_slot", Slot), ("beta1", c_double), ("beta2", c_double),
                ("eps", c_double), ("weight_decay", c_double), ("clamp", c_float), ("accumulate", c_int),
                ("ones_from", c_int), ("head", POINTER(HeadBwdArgs)), ("fold", POINTER(HeadFoldArgs)),
                ("xbits", _P), ("xbits_wpr", c_int), ("xbits_rows", c_int)]


class Finalize2Args(ctypes.Structure):
    """The two loss sums + counter tick that ride in a VAE batch's last launch."""
    c_name = "gm_finalize2_args"
    _fields_ = [("pa", _P), ("na", c_int), ("scale_a", c_float), ("out_a", _P), ("slot_a", Slot),
                ("pb", _P), ("nb", c_int), ("scale_b", c_float), ("out_b", _P), ("slot_b", Slot),
                ("tick", _P), ("done", _P)]


class DwTail(ctypes.Structure):
    """What a pair of weight gradients carries: the next first layer, or the sums."""
    c_name = "gm_dw_tail"
    _fields_ = [("z", _P), ("ldz", c_int64), ("z_slot", Slot), ("H", _P), ("ldh", c_int64), ("rows", c_int),
                ("fin", POINTER(Finalize2Args))]


class IwaeNoise(ctypes.Structure):
    """A noise stream: seed, tag, step and the sample rows of the call (the IWAE's, and every k = 1 prior's)."""
    c_name = "gm_iwae_noise"
    _fields_ = [("seed", c_uint64), ("tag", c_uint32), ("step_ctr", _P), ("step_base", _P), ("step_add", c_int64),
                ("k_total", c_int64), ("j0", c_int64), ("q0", c_int64)]


class FlowParams(ctypes.Structure):
    """The K planar layers' u [K, Z], w [K, Z], b [K]."""
    c_name = "gm_flow_params"
    _fields_ = [("u", _P), ("w", _P), ("b", _P), ("K", c_int)]


class FlowStepArgs(ctypes.Structure):
    """gm_flow_step's arguments as one block."""
    c_name = "gm_flow_step_args"
    _fields_ = [("part", _P), ("nparts", c_int), ("u", _P), ("w", _P), ("b", _P), ("gu", _P), ("gw", _P), ("gb", _P),
                ("mu", _P), ("vu", _P), ("mw", _P), ("vw", _P), ("mb", _P), ("vb", _P), ("sched", _P),
                ("sched_slot", Slot), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("weight_decay", c_double), ("K", c_int), ("Z", c_int)]


class IafParams(ctypes.Structure):
    """The K layers' W1 [K, F, Z], U [K, F, C], b1 [K, F], W2 [K, 2Z, F], b2 [K, 2Z]."""
    c_name = "gm_iaf_params"
    _fields_ = [("W1", _P), ("U", _P), ("b1", _P), ("W2", _P), ("b2", _P), ("K", c_int), ("F", c_int), ("C", c_int)]


class IafStepArgs(ctypes.Structure):
    """gm_iaf_step's arguments as one block."""
    c_name = "gm_iaf_step_args"
    _fields_ = [("part", _P), ("nparts", c_int), ("p", _P * 5), ("g", _P * 5), ("m", _P * 5), ("v", _P * 5),
                ("m_in", _P), ("sched", _P), ("sched_slot", Slot), ("beta1", c_double), ("beta2", c_double),
                ("eps", c_double), ("weight_decay", c_double), ("K", c_int), ("Z", c_int), ("F", c_int), ("C", c_int)]


class CatArgs(ctypes.Structure):
    """gm_cat_sample's and gm_cat_reduce's arguments as one block."""
    c_name = "gm_cat_args"
    _fields_ = [("logits", _P), ("ldl", c_int64), ("tau_tab", _P), ("tau_slot", Slot), ("tau", c_float), ("B", c_int),
                ("k", c_int), ("N", c_int), ("C", c_int), ("mode", c_int), ("y", _P), ("ldy", c_int64), ("lp", _P),
                ("kl", _P), ("codes", _P), ("dzdec", _P), ("lddz", c_int64), ("wn", _P), ("dlogits", _P),
                ("lddl", c_int64)]


class DdpmNoise(ctypes.Structure):
    """Seed, the two tags, the step and the first row's batch position."""
    c_name = "gm_ddpm_noise"
    _fields_ = [("seed", c_uint64), ("tag_t", c_uint32), ("tag_e", c_uint32), ("step_ctr", _P), ("step_base", _P),
                ("step_add", c_int64), ("row0", c_int64)]


class DdpmTables(ctypes.Structure):
    """The schedule and embedding tables on the device."""
    c_name = "gm_ddpm_tables"
    _fields_ = [("sa", _P), ("s1", _P), ("temb", _P), ("T", c_int), ("E", c_int)]


class DdpmOut(ctypes.Structure):
    """Where a q-sample writes."""
    c_name = "gm_ddpm_out"
    _fields_ = [("xin", _P), ("ldin", c_int64), ("eps", _P), ("lde", c_int64), ("t", _P)]


class DdpmReverseArgs(ctypes.Structure):
    """One sampler step."""
    c_name = "gm_ddpm_reverse_args"
    _fields_ = [("xin", _P), ("ldin", c_int64), ("eps", _P), ("lde", c_int64), ("coef", _P), ("slot", Slot),
                ("temb", _P), ("traj", _P), ("traj_stride", c_int64), ("seed", c_uint64), ("tick", _P), ("done", _P),
                ("rows", c_int), ("I", c_int), ("E", c_int), ("T", c_int), ("S", c_int), ("clip", c_int)]


class MadeMaskArgs(ctypes.Structure):
    """Both masked layers, their moments and the degree vectors."""
    c_name = "gm_made_mask_args"
    _fields_ = [("W1", _P), ("m1", _P), ("v1", _P), ("W2", _P), ("m2", _P), ("v2", _P), ("m_in", _P), ("m_h", _P),
                ("I", c_int), ("H", c_int)]


class MadeSampleArgs(ctypes.Structure):
    """The one-launch ancestral sampler."""
    c_name = "gm_made_sample_args"
    _fields_ = [("W2", _P), ("b2", _P), ("W1T", _P), ("b1", _P), ("m_h", _P), ("inv_order", _P), ("x", _P),
                ("ldx", c_int64), ("p", _P), ("ldp", c_int64), ("given", _P), ("ldg", c_int64), ("seed", c_uint64),
                ("n", c_int64), ("I", c_int), ("H", c_int), ("n_known", c_int)]


class NvpPreArgs(ctypes.Structure):
    """Dequantise + logit + split, or the noise alone."""
    c_name = "gm_nvp_pre_args"
    _fields_ = [("x", _P), ("ldx", c_int64), ("ya", _P), ("lda", c_int64), ("yb", _P), ("ldb", c_int64),
                ("logdet", _P), ("u", _P), ("ldu", c_int64), ("seed", c_uint64), ("step_ctr", _P), ("step_base", _P),
                ("step_add", c_int64), ("row0", c_int64), ("tag", c_uint32), ("alpha", c_float), ("levels", c_int),
                ("mask", c_int), ("mode", c_int), ("B", c_int), ("D", c_int)]


class NvpCoupleArgs(ctypes.Structure):
    """One affine coupling, forward or inverse."""
    c_name = "gm_nvp_couple_args"
    _fields_ = [("st", _P), ("ldst", c_int64), ("inp", _P), ("ldin", c_int64), ("out", _P), ("ldout", c_int64),
                ("logdet", _P), ("s_cap", c_float), ("inverse", c_int), ("B", c_int), ("Dt", c_int)]


class NvpLossArgs(ctypes.Structure):
    """The rows' negative log-likelihood and dz."""
    c_name = "gm_nvp_loss_args"
    _fields_ = [("za", _P), ("ldza", c_int64), ("zb", _P), ("ldzb", c_int64), ("logdet", _P), ("part", _P),
                ("dza", _P), ("lddza", c_int64), ("dzb", _P), ("lddzb", c_int64), ("cst", c_float), ("scale", c_float),
                ("B", c_int), ("Da", c_int), ("Db", c_int)]


class NvpCoupleBwdArgs(ctypes.Structure):
    """The coupling's backward."""
    c_name = "gm_nvp_couple_bwd_args"
    _fields_ = [("st", _P), ("ldst", c_int64), ("x", _P), ("ldx", c_int64), ("g0", _P), ("ldg0", c_int64),
                ("g1", _P), ("ldg1", c_int64), ("dst", _P), ("lddst", c_int64), ("dx", _P), ("lddx", c_int64),
                ("c", c_float), ("s_cap", c_float), ("B", c_int), ("Dt", c_int)]


class NvpPostArgs(ctypes.Structure):
    """Halves -> image, or the sampler's normals -> halves."""
    c_name = "gm_nvp_post_args"
    _fields_ = [("ya", _P), ("lda", c_int64), ("yb", _P), ("ldb", c_int64), ("x", _P), ("ldx", c_int64),
                ("seed", c_uint64), ("row0", c_int64), ("alpha", c_float), ("temperature", c_float), ("mask", c_int),
                ("mode", c_int), ("B", c_int), ("D", c_int)]


class NsfCoupleArgs(ctypes.Structure):
    """One rational-quadratic spline coupling, forward or inverse."""
    c_name = "gm_nsf_couple_args"
    _fields_ = [("st", _P), ("ldst", c_int64), ("inp", _P), ("ldin", c_int64), ("out", _P), ("ldout", c_int64),
                ("logdet", _P), ("tail_bound", c_float), ("inverse", c_int), ("B", c_int), ("Dt", c_int), ("bins", c_int)]


class NsfCoupleBwdArgs(ctypes.Structure):
    """The spline coupling's backward."""
    c_name = "gm_nsf_couple_bwd_args"
    _fields_ = [("st", _P), ("ldst", c_int64), ("x", _P), ("ldx", c_int64), ("g0", _P), ("ldg0", c_int64),
                ("g1", _P), ("ldg1", c_int64), ("dst", _P), ("lddst", c_int64), ("dx", _P), ("lddx", c_int64),
                ("c", c_float), ("tail_bound", c_float), ("B", c_int), ("Dt", c_int), ("bins", c_int)]


class MafCoupleArgs(ctypes.Structure):
    """One layer, data -> noise."""
    c_name = "gm_maf_couple_args"
    _fields_ = [("y", _P), ("ldy", c_int64), ("ma", _P), ("ldma", c_int64), ("u", _P), ("ldu", c_int64),
                ("logdet", _P), ("s_cap", c_float), ("B", c_int), ("D", c_int)]


class MafCoupleBwdArgs(ctypes.Structure):
    """The layer's backward."""
    c_name = "gm_maf_couple_bwd_args"
    _fields_ = [("ma", _P), ("ldma", c_int64), ("u", _P), ("ldu", c_int64), ("g", _P), ("ldg", c_int64),
                ("dout", _P), ("lddout", c_int64), ("dy", _P), ("lddy", c_int64), ("c", c_float), ("s_cap", c_float),
                ("B", c_int), ("D", c_int)]


class MafMaskArgs(ctypes.Structure):
    """One layer's masked weights, their moments and the degree vectors."""
    c_name = "gm_maf_mask_args"
    _fields_ = [("W1", _P), ("m1", _P), ("v1", _P), ("W2", _P), ("m2", _P), ("v2", _P), ("m_in", _P), ("m_h", _P),
                ("D", c_int), ("H", c_int)]


class MafInvertArgs(ctypes.Structure):
    """One layer's inverse in one launch."""
    c_name = "gm_maf_invert_args"
    _fields_ = [("u", _P), ("ldu", c_int64), ("y", _P), ("ldy", c_int64), ("s", _P), ("lds", c_int64), ("W2", _P),
                ("b2", _P), ("W1T", _P), ("b1", _P), ("m_h", _P), ("inv_order", _P), ("s_cap", c_float),
                ("n", c_int64), ("D", c_int), ("H", c_int)]


class RbmChainArgs(ctypes.Structure):
    """The one-launch Gibbs chain."""
    c_name = "gm_rbm_chain_args"
    _fields_ = [("W", _P), ("WT", _P), ("c", _P), ("b", _P), ("x", _P), ("ldx", c_int64), ("v0_out", _P),
                ("ldv0", c_int64), ("v_out", _P), ("ldv", c_int64), ("p_out", _P), ("ldp", c_int64), ("a_out", _P),
                ("lda", c_int64), ("seed", c_uint64), ("row0", c_int64), ("step_ctr", _P), ("step_base", _P),
                ("d_add", c_int64), ("g_mul", c_int64), ("g_add", c_int64), ("betas", _P), ("b_A", _P), ("logw", _P),
                ("n", c_int64), ("I", c_int), ("H", c_int), ("steps", c_int)]


class RbmVbiasArgs(ctypes.Structure):
    """The visible bias' gradient and its Adam step."""
    c_name = "gm_rbm_vbias_args"
    _fields_ = [("V", _P), ("ldv", c_int64), ("g", _P), ("pb", _P), ("mb", _P), ("vb", _P), ("sched", _P),
                ("sched_slot", Slot), ("beta1", c_double), ("beta2", c_double), ("eps", c_double),
                ("weight_decay", c_double), ("inv_b", c_float), ("B", c_int), ("I", c_int)]


class VqArgs(ctypes.Structure):
    """gm_vq_quantise's and gm_vq_reduce's arguments as one block."""
    c_name = "gm_vq_args"
    _fields_ = [("ze", _P), ("ldz", c_int64), ("E", _P), ("lde", c_int64), ("codes", _P), ("ldc", c_int64),
                ("beta", c_float), ("B", c_int), ("N", c_int), ("D", c_int), ("K", c_int), ("zq", _P), ("ldq", c_int64),
                ("qerr", _P), ("lp", _P), ("dzdec", _P), ("lddz", c_int64), ("wn", _P), ("dml", _P),
                ("lddml", c_int64)]


class VqStepArgs(ctypes.Structure):
    """gm_vq_step's arguments as one block."""
    c_name = "gm_vq_step_args"
    _fields_ = [("ze", _P), ("ldz", c_int64), ("codes", _P), ("ldc", c_int64), ("E", _P), ("m", _P), ("v", _P),
                ("grad", _P), ("nk", _P), ("usage", _P), ("sched", _P), ("sched_slot", Slot), ("beta1", c_double),
                ("beta2", c_double), ("eps", c_double), ("weight_decay", c_double), ("B", c_int), ("N", c_int),
                ("D", c_int), ("K", c_int)]


class FmNoise(ctypes.Structure):
    """Seed, the three tags, the step and the first row's batch position."""
    c_name = "gm_fm_noise"
    _fields_ = [("seed", c_uint64), ("tag_d", c_uint32), ("tag_t", c_uint32), ("tag_n", c_uint32), ("step_ctr", _P),
                ("step_base", _P), ("step_add", c_int64), ("row0", c_int64)]


class FmTables(ctypes.Structure):
    """The time grid's tables and the embedding table on the device."""
    c_name = "gm_fm_tables"
    _fields_ = [("tt", _P), ("tc", _P), ("temb", _P), ("T", c_int), ("E", c_int)]


class FmOut(ctypes.Structure):
    """Where a flow-matching q-sample writes."""
    c_name = "gm_fm_out"
    _fields_ = [("xin", _P), ("ldin", c_int64), ("u", _P), ("ldu", c_int64), ("logdet", _P), ("j", _P), ("y1", _P),
                ("ldy1", c_int64), ("y0", _P), ("ldy0", c_int64), ("alpha", c_float), ("levels", c_int)]


class FmDivArgs(ctypes.Structure):
    """The exact divergence of one field evaluation."""
    c_name = "gm_fm_div_args"
    _fields_ = [("H1", _P), ("ld1", c_int64), ("H2", _P), ("ld2", c_int64), ("Q", _P), ("ldq", c_int64), ("part", _P),
                ("part_floats", c_int64), ("div", _P), ("B", c_int), ("H", c_int)]


class FmStageArgs(ctypes.Structure):
    """One solver stage."""
    c_name = "gm_fm_stage_args"
    _fields_ = [("k", _P), ("ldk", c_int64), ("base", _P), ("ldb", c_int64), ("acc", _P), ("lda", c_int64),
                ("xin", _P), ("ldin", c_int64), ("L", _P), ("div", _P), ("div_stride", c_int64), ("div_parts", c_int),
                ("tab", _P), ("slot", Slot), ("temb", _P), ("traj", _P), ("traj_stride", c_int64), ("tick", _P),
                ("done", _P), ("rows", c_int), ("I", c_int), ("E", c_int), ("T", c_int), ("S", c_int),
                ("stages", c_int)]


STRUCTS = {ct.c_name: ct for ct in list(vars().values())
           if isinstance(ct, type) and issubclass(ct, ctypes.Structure) and ct is not ctypes.Structure}

# ---- prototypes: name -> (return type, parameter types).  A `const gm_x*` parameter is POINTER(its class), so a block of
# another struct in its place is refused before the library is entered; gm_linear_plan's descriptor alone is one of three
# structs by mode and stays a void pointer (ops.linear_plan casts).
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
    "gm_adam": (c_int, [_P, _P, _P, _P, _P, c_int64, _P, Slot, c_double, c_double, c_double, c_double, c_float]),
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
                                  c_double, c_double, c_double, c_double, c_float, _P]),
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
    "gm_adam_scaled": (c_int, [_P, _P, _P, _P, _P, c_int64, _P, Slot, c_double, c_double, c_double, c_double, c_float,
                               _P]),
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
    "gm_randperm_prefix": (c_int, [c_uint64, c_int64, c_int, _P]),
    "gm_mt19937_skip": (c_int, [_P, c_int64, c_uint64]),
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
    "gm_comm_set_wait_seconds": (c_int, [_P, c_double]),
    "gm_comm_buffer": (c_int, [_P, POINTER(c_void_p), POINTER(c_int64)]),
    "gm_allreduce_f32": (c_int, [_P, _P, _P, c_int64]),
    "gm_allreduce_adam_f32": (c_int, [_P, _P, _P, c_int64, _P, _P, _P, _P, Slot, c_double, c_double, c_double,
                                      c_double, c_float, _P]),
    "gm_allreduce_scalars": (c_int, [_P, _P, _P, c_int]),
    "gm_stage_in": (c_int, [_P, POINTER(StageSeg), c_int, Slot, c_int]),
    "gm_stage_in_gated": (c_int, [_P, POINTER(StageSeg), c_int, Slot, c_int, _P, Slot, c_double, _P, c_int]),
    "gm_host_device_ptr": (c_int, [_P, POINTER(c_void_p)]),
    "gm_host_replay": (c_int, [_P, c_int64, POINTER(DrawOp), c_int, c_int]),
    "gm_host_replay_threads": (c_int, [c_int]),
    "gm_numpy_legacy_normal_f32": (c_int, [_P, _P, _P, _P, c_double, c_double, c_int64, _P, c_int]),
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
                                   c_double, c_double, c_double, c_double]),
    "gm_parzen_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "gm_aae_critic_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "gm_aae_critic_step": (c_int, [_P, POINTER(AAECriticArgs)]),
    "gm_aae_gen_mid": (c_int, [_P, POINTER(AAEGenArgs)]),
    "gm_acgan_heads_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "gm_acgan_heads_fwd": (c_int, [_P, POINTER(ACGANHeadsArgs)]),
    "gm_acgan_heads_bwd": (c_int, [_P, POINTER(ACGANHeadsArgs)]),
    "gm_sn_power_workspace_bytes": (c_int64, [c_int, c_int]),
    "gm_sn_power_iter": (c_int, [_P, POINTER(SNPowerArgs)]),
    "gm_sn_head_workspace_bytes": (c_int64, [c_int, c_int]),
    "gm_sn_head_fwd": (c_int, [_P, POINTER(SNHeadArgs)]),
    "gm_sn_head_bwd": (c_int, [_P, POINTER(SNHeadArgs)]),
    "gm_sn_grad_workspace_bytes": (c_int64, [c_int]),
    "gm_sn_grad": (c_int, [_P, POINTER(SNGradArgs)]),
    "gm_philox_raw": (c_int, [_P, _P, _P, _P, c_int64]),
    "gm_philox_normal": (c_int, [_P, c_uint64, c_uint32, c_uint32, c_int, _P, c_int64, _P, c_int64]),
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
    "gm_iwae_sample": (c_int, [_P, POINTER(IwaeNoise), _P, c_int64, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_iwae_weights": (c_int, [_P, _P, c_int64, _P, c_int64, _P, _P, _P, _P, _P, c_int64, _P, c_int, c_int, c_int]),
    "gm_iwae_reduce": (c_int, [_P, POINTER(IwaeNoise), _P, c_int64, _P, _P, c_int64, _P, c_int64, _P, c_int64, c_int,
                               c_int, c_int]),
    "gm_flow_sample": (c_int, [_P, POINTER(IwaeNoise), POINTER(FlowParams), _P, c_int64, _P, c_int64, _P, c_int, c_int,
                               c_int]),
    "gm_flow_reduce": (c_int, [_P, POINTER(IwaeNoise), POINTER(FlowParams), _P, c_int64, _P, _P, c_int64, _P, c_int64,
                               _P, c_int, c_int, c_int]),
    "gm_flow_step": (c_int, [_P, POINTER(FlowStepArgs)]),
    "gm_iaf_sample": (c_int, [_P, POINTER(IwaeNoise), POINTER(IafParams), _P, c_int64, _P, c_int64, _P, c_int, c_int,
                              c_int]),
    "gm_iaf_reduce": (c_int, [_P, POINTER(IwaeNoise), POINTER(IafParams), _P, c_int64, _P, _P, c_int64, _P, c_int64,
                              _P, c_int, c_int, c_int]),
    "gm_iaf_step": (c_int, [_P, POINTER(IafStepArgs)]),
    "gm_tc_sample": (c_int, [_P, POINTER(IwaeNoise), _P, c_int64, _P, c_int64, _P, _P, _P, c_int64, _P, _P, c_float,
                             c_float, c_float, c_float, c_int, c_int, c_int]),
    "gm_tc_reduce": (c_int, [_P, POINTER(IwaeNoise), _P, c_int64, _P, c_int64, _P, _P, c_int64, _P, _P, c_int64, _P,
                             c_int64, c_float, c_float, c_float, c_int, c_int, c_int]),
    "gm_mmd_workspace_bytes": (c_int64, [c_int, c_int, c_int]),
    "gm_gmmn_prior": (c_int, [_P, POINTER(IwaeNoise), _P, c_int64, c_int, c_int]),
    "gm_mmd_pairs": (c_int, [_P, _P, c_int64, c_int, _P, c_int64, c_int, c_int, _P, c_int, _P, c_int64, _P, _P, c_int64]),
    "gm_mmd_finalize": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, c_int64, _P, _P, _P]),
    "gm_mmd_grad": (c_int, [_P, _P, c_int64, _P, _P, c_int64, _P, _P, c_float, c_int, _P, c_int64, c_int, c_int]),
    "gm_sw_workspace_bytes": (c_int64, [c_int]),
    "gm_sw_directions": (c_int, [_P, POINTER(IwaeNoise), _P, c_int64, c_int, c_int]),
    "gm_sw_sort": (c_int, [_P, _P, c_int64, c_int, c_int, c_int, _P, c_int64, _P, c_int64]),
    "gm_sw_finalize": (c_int, [_P, c_int, c_int, c_int, _P, c_int64, _P, _P]),
    "gm_cat_sample": (c_int, [_P, POINTER(IwaeNoise), POINTER(CatArgs)]),
    "gm_cat_reduce": (c_int, [_P, POINTER(IwaeNoise), POINTER(CatArgs)]),
    "gm_vq_quantise": (c_int, [_P, POINTER(VqArgs)]),
    "gm_vq_reduce": (c_int, [_P, POINTER(VqArgs)]),
    "gm_vq_step": (c_int, [_P, POINTER(VqStepArgs)]),
    "gm_ddpm_qsample": (c_int, [_P, POINTER(DdpmNoise), POINTER(DdpmTables), POINTER(DdpmOut), _P, c_int64, c_int64,
                                c_int]),
    "gm_gather_rows_qsample": (c_int, [_P, POINTER(DdpmNoise), POINTER(DdpmTables), POINTER(DdpmOut), _P, c_int64, _P,
                                       Slot, _P, c_int64, c_int, c_int]),
    "gm_gather_rows_bits_qsample": (c_int, [_P, POINTER(DdpmNoise), POINTER(DdpmTables), POINTER(DdpmOut), _P, c_int,
                                            c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_ddpm_loss": (c_int, [_P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_float, c_int, c_int]),
    "gm_ddpm_reverse": (c_int, [_P, POINTER(DdpmReverseArgs)]),
    "gm_ddpm_prior": (c_int, [_P, _P, c_int64, _P, c_uint64, c_int64, c_int, _P, c_int, c_int, c_int, c_int]),
    "gm_fm_qsample": (c_int, [_P, POINTER(FmNoise), POINTER(FmTables), POINTER(FmOut), _P, c_int64, c_int64, c_int]),
    "gm_gather_rows_fm_qsample": (c_int, [_P, POINTER(FmNoise), POINTER(FmTables), POINTER(FmOut), _P, c_int64, _P,
                                          Slot, _P, c_int64, c_int, c_int]),
    "gm_gather_rows_bits_fm_qsample": (c_int, [_P, POINTER(FmNoise), POINTER(FmTables), POINTER(FmOut), _P, c_int,
                                               c_int64, _P, Slot, _P, c_int64, c_int, c_int]),
    "gm_fm_div": (c_int, [_P, POINTER(FmDivArgs)]),
    "gm_fm_stage": (c_int, [_P, POINTER(FmStageArgs)]),
    "gm_made_bce": (c_int, [_P, _P, c_int64, _P, c_int64, _P, c_int64, _P, c_float, c_int, c_int]),
    "gm_made_mask": (c_int, [_P, POINTER(MadeMaskArgs)]),
    "gm_made_sample": (c_int, [_P, POINTER(MadeSampleArgs)]),
    "gm_made_uniform": (c_int, [_P, _P, c_int64, c_uint64, c_int64, c_int64, c_int]),
    "gm_nvp_pre": (c_int, [_P, POINTER(NvpPreArgs)]),
    "gm_nvp_couple": (c_int, [_P, POINTER(NvpCoupleArgs)]),
    "gm_nvp_loss": (c_int, [_P, POINTER(NvpLossArgs)]),
    "gm_nvp_couple_bwd": (c_int, [_P, POINTER(NvpCoupleBwdArgs)]),
    "gm_nvp_post": (c_int, [_P, POINTER(NvpPostArgs)]),
    "gm_nsf_couple": (c_int, [_P, POINTER(NsfCoupleArgs)]),
    "gm_nsf_couple_bwd": (c_int, [_P, POINTER(NsfCoupleBwdArgs)]),
    "gm_maf_couple": (c_int, [_P, POINTER(MafCoupleArgs)]),
    "gm_maf_couple_bwd": (c_int, [_P, POINTER(MafCoupleBwdArgs)]),
    "gm_maf_mask": (c_int, [_P, POINTER(MafMaskArgs)]),
    "gm_maf_invert": (c_int, [_P, POINTER(MafInvertArgs)]),
    "gm_rbm_chain": (c_int, [_P, POINTER(RbmChainArgs)]),
    "gm_rbm_grad": (c_int, [_P, _P, c_int64, _P, c_int64, _P, _P, c_int64, _P, c_float, c_int, c_int, c_int]),
    "gm_rbm_vbias": (c_int, [_P, POINTER(RbmVbiasArgs)]),
    "gm_rbm_transpose": (c_int, [_P, _P, c_int64, _P, c_int64, c_int, c_int]),
    "gm_rbm_uniform": (c_int, [_P, _P, c_int64, c_uint64, c_uint32, _P, _P, c_int64, c_int64, c_int64, c_int]),
}
