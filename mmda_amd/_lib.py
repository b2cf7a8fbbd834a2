"""ctypes binding of libmmda_hip.so (the C ABI declared in include/mmda_hip.h).

The product path has NO fallback: if the HIP library is missing or a call fails, this raises.  PyTorch is used by
callers only to own device memory and streams; every pointer handed over here is ``tensor.data_ptr()``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmmda_hip.so")

F32, BF16 = 0, 1
ACT = {"none": 0, "relu": 1, "sigmoid": 2, "leakyrelu": 3, "tanh": 4, "elu": 5, "hardtanh": 6, "hardshrink": 7, "prelu": 8, "rrelu": 9}

c_f32p = C.c_void_p      # device pointers travel as integers
c_stream = C.c_void_p


class GemmArgs(C.Structure):
    _fields_ = [("mode", C.c_int), ("transA", C.c_int), ("transB", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("batch", C.c_int),
                ("A", C.c_void_p), ("lda", C.c_int), ("strideA", C.c_int64),
                ("A2", C.c_void_p), ("gather", C.c_void_p),
                ("B", C.c_void_p), ("ldb", C.c_int), ("strideB", C.c_int64),
                ("C", C.c_void_p), ("ldc", C.c_int), ("strideC", C.c_int64),
                ("bias", C.c_void_p), ("bias2", C.c_void_p), ("strideBias", C.c_int64),
                ("accumulate", C.c_int), ("act", C.c_int),
                ("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("drop_site", C.c_int),
                ("gate", C.c_void_p), ("ldgate", C.c_int), ("gate_scale", C.c_float),
                ("alpha", C.c_float), ("bias_grad", C.c_void_p), ("bias_grad2", C.c_void_p)]


class GemmBf16Args(C.Structure):
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("A", C.c_void_p), ("lda", C.c_int), ("B", C.c_void_p), ("ldb", C.c_int),
                ("C", C.c_void_p), ("ldc", C.c_int), ("bias", C.c_void_p), ("bias2", C.c_void_p), ("bias_grad", C.c_void_p),
                ("bias_grad2", C.c_void_p), ("accumulate", C.c_int), ("alpha", C.c_float), ("perm_n_H", C.c_int), ("perm_m_H", C.c_int),
                ("tn", C.c_int)]


class GemmBf16PlanRow(C.Structure):
    """mmda_gemm_bf16_plan_row: what the launch plan of a call does with one problem"""
    _fields_ = [("cls", C.c_int), ("mixed", C.c_int), ("tx", C.c_int), ("ty", C.c_int), ("sk", C.c_int), ("per", C.c_int),
                ("last", C.c_int), ("launch", C.c_int)]


class GemmPlanRow(C.Structure):
    """mmda_gemm_plan_row: what mmda_gemm / mmda_gemm_grouped would do with one problem"""
    _fields_ = [("cls", C.c_int), ("mode", C.c_int), ("ta", C.c_int), ("tb", C.c_int), ("tx", C.c_int), ("ty", C.c_int), ("sk", C.c_int),
                ("per", C.c_int), ("last", C.c_int), ("ldn", C.c_int), ("blocks", C.c_int), ("launch", C.c_int),
                ("slab_off", C.c_int64), ("reduce", C.c_int)]


class ConvertJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("ld", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("gather", C.c_void_p),
                ("plain", C.c_void_p), ("ldp", C.c_int), ("transposed", C.c_void_p), ("ldt", C.c_int), ("row_perm_H", C.c_int),
                ("src_bf16", C.c_int)]


class SkinnyArgs(C.Structure):
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("transB", C.c_int),
                ("A", C.c_void_p), ("A2", C.c_void_p), ("lda", C.c_int), ("B", C.c_void_p), ("ldb", C.c_int),
                ("K2", C.c_int), ("A_2nd", C.c_void_p), ("lda_2nd", C.c_int), ("B_2nd", C.c_void_p), ("ldb_2nd", C.c_int),
                ("C", C.c_void_p), ("ldc", C.c_int), ("C2", C.c_void_p), ("ldc2", C.c_int), ("bias", C.c_void_p),
                ("accumulate", C.c_int), ("alpha", C.c_float), ("act", C.c_int),
                ("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("drop_site", C.c_int),
                ("gate", C.c_void_p), ("ldgate", C.c_int), ("gate_scale", C.c_float),
                ("dsig", C.c_void_p), ("dsig2", C.c_void_p), ("lddsig", C.c_int)]


class TransposeJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("rows", C.c_int), ("cols", C.c_int), ("ld", C.c_int), ("dst", C.c_void_p), ("ldd", C.c_int)]


class ActParams(C.Structure):
    _fields_ = [("slope", C.c_void_p), ("dslope", C.c_void_p), ("lo", C.c_float), ("hi", C.c_float), ("rand", C.c_int),
                ("seed", C.c_uint64), ("site", C.c_int)]


class LnArgs(C.Structure):
    _fields_ = [("rows", C.c_int), ("n", C.c_int), ("x", C.c_void_p), ("res", C.c_void_p), ("gamma", C.c_void_p),
                ("beta", C.c_void_p), ("y", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p), ("act", C.c_int),
                ("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("drop_site", C.c_int),
                ("permute_S", C.c_int), ("permute_B", C.c_int), ("eps", C.c_float), ("actp", ActParams),
                ("y_bf16", C.c_void_p), ("ld_bf16", C.c_int)]


class LnBwdArgs(C.Structure):
    _fields_ = [("rows", C.c_int), ("n", C.c_int), ("dy", C.c_void_p), ("x", C.c_void_p), ("res", C.c_void_p),
                ("gamma", C.c_void_p), ("mean", C.c_void_p), ("rstd", C.c_void_p),
                ("d_x", C.c_void_p), ("accumulate_dx", C.c_int), ("d_res", C.c_void_p),
                ("dgamma", C.c_void_p), ("dbeta", C.c_void_p),
                ("act", C.c_int), ("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("drop_site", C.c_int),
                ("permute_S", C.c_int), ("permute_B", C.c_int), ("actp", ActParams)]


class LstmDesc(C.Structure):
    _fields_ = [("H", C.c_int), ("gates", C.c_void_p), ("cstash", C.c_void_p), ("hseq", C.c_void_p),
                ("wpack", C.c_void_p * 2), ("wpack_c", C.c_void_p * 2), ("utt", C.c_void_p), ("layer", C.c_int), ("d_hseq", C.c_void_p),
                ("xchg", C.c_void_p), ("epoch_base", C.c_uint32), ("gate_minor", C.c_int), ("forward_only", C.c_int),
                ("cell", C.c_int), ("dg_bf16", C.c_void_p), ("dg_bf16_only", C.c_int)]


class LstmPlan(C.Structure):
    """mmda_lstm_plan: what the resident launch plan of an mmda_lstm_fwd / mmda_lstm_bwd call decides"""
    _fields_ = [("ok", C.c_int), ("form", C.c_int), ("wpb", C.c_int), ("groups", C.c_int), ("groups_per_launch", C.c_int),
                ("launches", C.c_int), ("wg_per_group", C.c_int), ("wg_per_desc", C.c_int * 4), ("gru", C.c_int),
                ("gate_minor", C.c_int), ("no_stash", C.c_int), ("dhseq", C.c_int), ("pair", C.c_int),
                ("kernel", C.c_int)]


class MisaStepRequest(C.Structure):
    """mmda_misa_step_request: what one forward pass is asked to be"""
    _fields_ = [("fused", C.c_int), ("has_labels", C.c_int), ("has_opt_step", C.c_int), ("enc_cached", C.c_int)]


STEP_PLAN_FIELDS = ("fused", "inf", "enc_cut", "enc_nostash", "enc_cached", "bfg", "gm", "kdg", "tn_wgrad", "want_b", "want_c", "want_wT",
                    "wT_merge", "skinny", "row_fuse", "ffn_fuse_fwd", "ffn_fuse_bwd", "seed_recon", "seed_cls", "fj_on", "fj_fwd",
                    "fj_device", "zg_here", "rec_hoisted", "sort_early", "embed_update", "embed_deferred", "embed_bg", "embed_bg_late",
                    "embed_bg_wgs", "embed_bg_lds")
# the step's switches in the order mmda_misa_plan_describe takes them (MMDA_MISA_STEP_SWITCHES of them), with their defaults
STEP_SWITCHES = {"MMDA_GEMM_TN": 1, "MMDA_WT_MERGE": 1, "MMDA_ROW_FUSE": 1, "MMDA_FFN_FUSE": 1, "MMDA_LOSS_SEEDS": 1, "MMDA_FLAG_JOIN": 1,
                 "MMDA_ZERO_GRAD_SIDE": -1, "MMDA_FUSED_SPLIT": 1, "MMDA_SORT_EARLY": 1, "MMDA_EMBED_BG": 1, "MMDA_EMBED_BG_WGS": 0,
                 "MMDA_EMBED_BG_LATE": 0, "MMDA_EMBED_BG_LDS": 1024}


class MisaStepPlan(C.Structure):
    """mmda_misa_step_plan: every choice of a form of the training step, one int per StepPlan field"""
    _fields_ = [(k, C.c_int) for k in STEP_PLAN_FIELDS]


class LossForms(C.Structure):
    """mmda_loss_forms: which kernel form the loss entry points pick for a shape"""
    _fields_ = [("diff_form", C.c_int), ("diff_products", C.c_int), ("diff_loss_sum", C.c_int), ("diff_combine_blocks", C.c_int),
                ("cmd_form", C.c_int), ("cmd_grid", C.c_int), ("recon_blocks", C.c_int), ("misc_recon_blocks", C.c_int)]


class RankPlan(C.Structure):
    """mmda_rank_plan: the launch mmda_rank_counts gives a shape"""
    _fields_ = [("rows_per_wg", C.c_int), ("tile", C.c_int), ("tiles", C.c_int), ("splits", C.c_int), ("tiles_per_split", C.c_int),
                ("grid_x", C.c_int), ("grid_y", C.c_int), ("grid_z", C.c_int), ("counts_bytes", C.c_int64)]


class GruPadJob(C.Structure):
    _fields_ = [("H", C.c_int), ("D", C.c_int), ("w_ih", C.c_void_p * 2), ("w_hh", C.c_void_p * 2), ("b_ih", C.c_void_p * 2),
                ("b_hh", C.c_void_p * 2), ("pw_ih", C.c_void_p), ("pw_hh", C.c_void_p * 2), ("pb_ih", C.c_void_p), ("pb_hh", C.c_void_p)]


class MisaConfig(C.Structure):
    _fields_ = [("vocab", C.c_int), ("d_t", C.c_int), ("d_v", C.c_int), ("d_a", C.c_int), ("hidden", C.c_int), ("ncls", C.c_int),
                ("act", C.c_int), ("use_cmd_sim", C.c_int), ("use_confidNet", C.c_int),
                ("dropout", C.c_float), ("fusion_dropout", C.c_float), ("threshold", C.c_float),
                ("reverse_grad_weight", C.c_float),
                ("diff_weight", C.c_float), ("sim_weight", C.c_float), ("recon_weight", C.c_float), ("conf_weight", C.c_float),
                ("mode", C.c_int), ("rnncell", C.c_int)]


class Mx8QuantJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("ld", C.c_int), ("rows", C.c_int), ("K", C.c_int), ("q", C.c_void_p), ("s", C.c_void_p)]


class Mx8Args(C.Structure):
    _fields_ = [("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("Aq", C.c_void_p), ("As", C.c_void_p), ("Bq", C.c_void_p),
                ("Bs", C.c_void_p), ("C", C.c_void_p), ("ldc", C.c_int), ("bias", C.c_void_p), ("act", C.c_int),
                ("drop_p", C.c_float), ("drop_seed", C.c_uint64), ("drop_site", C.c_int)]


class Run(C.Structure):
    """mmda_run: a trainable range of a flat bucket (frozen parameters)"""
    _fields_ = [("begin", C.c_int64), ("len", C.c_int64), ("first", C.c_int64)]


class AdamOpts(C.Structure):
    """mmda_adam_opts: Adam's settings beyond lr (scale_dev: one device float that multiplies grad_scale, or None)"""
    _fields_ = [("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float), ("decoupled", C.c_int),
                ("scale_dev", C.c_void_p)]


class ClsOpts(C.Structure):
    """mmda_cls_opts: the classification criterion beyond plain BCE (n_weights: 0, or the number of classes)"""
    _fields_ = [("focal_gamma", C.c_float), ("n_weights", C.c_int), ("pos_weight", C.c_float * 16)]


def cls_opts(pos_weight, focal_gamma):
    """``byref(ClsOpts)`` of a setting ``step_rules.cls_setting`` returned, or None (a NULL pointer) for the plain criterion."""
    if pos_weight is None and focal_gamma == 0.0:
        return None
    w = tuple(pos_weight or ())
    return C.byref(ClsOpts(focal_gamma=focal_gamma, n_weights=len(w), pos_weight=(C.c_float * 16)(*w)))


class InferSrc(C.Structure):
    """mmda_infer_src: what a forward left in the workspace, B columns"""
    _fields_ = [("scores", C.c_void_p), ("labels", C.c_void_p), ("tcp", C.c_void_p), ("hfused", C.c_void_p), ("x6", C.c_void_p),
                ("probs", C.c_void_p), ("ncls", C.c_int), ("hs", C.c_int), ("nhead", C.c_int)]


class InferOut(C.Structure):
    """mmda_infer_out: the result tables of an inference pass, one row per sample (None = not collected)"""
    _fields_ = [("scores", C.c_void_p), ("labels", C.c_void_p), ("tcp", C.c_void_p), ("hidden", C.c_void_p), ("utterance", C.c_void_p),
                ("attention", C.c_void_p)]


class EncodedBatch(C.Structure):
    """mmda_encoded_batch: B rows of the encoder cache's tables (tab_emo may be None where no labels are gathered)"""
    _fields_ = [("tab_t", C.c_void_p), ("tab_v", C.c_void_p), ("tab_a", C.c_void_p), ("tab_emo", C.c_void_p), ("rows", C.c_void_p),
                ("B", C.c_int)]


class ModalityP(C.Structure):
    """mmda_modality_p: the drop rates of text, visual, acoustic (passed by value)"""
    _fields_ = [("p", C.c_float * 3)]


class McOut(C.Structure):
    """mmda_mc_out: the per-sample tables of an MC-dropout reduction (None = not written); float64 but for ``draws`` (fp32)"""
    _fields_ = [("mean", C.c_void_p), ("var", C.c_void_p), ("entropy", C.c_void_p), ("expected_entropy", C.c_void_p),
                ("mutual_info", C.c_void_p), ("vote", C.c_void_p), ("draws", C.c_void_p)]


class BootPlan(C.Structure):
    """mmda_boot_plan: the form mmda_boot_counts gives a shape, and the limits of the bootstrap entry points"""
    _fields_ = [("form", C.c_int), ("threads", C.c_int), ("wgs_per_replicate", C.c_int), ("lds_bytes", C.c_int),
                ("state_words", C.c_int), ("lds_rows", C.c_int), ("rank_lds_bytes", C.c_int), ("max_replicates", C.c_int)]


class KnnPlan(C.Structure):
    """mmda_knn_plan: the launches mmda_knn_sets gives a shape, and the work buffer it is to be handed"""
    _fields_ = [("tile_q", C.c_int), ("tile_b", C.c_int), ("slab_rows", C.c_int), ("slabs", C.c_int), ("merge", C.c_int),
                ("launches", C.c_int), ("grid_x", C.c_int), ("grid_y", C.c_int), ("threads", C.c_int), ("lds_bytes", C.c_int),
                ("vector_loads", C.c_int), ("max_slabs", C.c_int), ("work_bytes", C.c_int64)]


KNN_MAX_D, KNN_MAX_SETS, KNN_MAX_K, TRUST_MAX_CLASSES = 1024, 16, 16, 8      # the limits of csrc/knn.hip
MC_MAX_PASSES, MC_MAX_WIDTH = 256, 64          # the K and W one mmda_mc_reduce launch takes


CELL = {"lstm": 0, "gru": 1}
TASK = {"emotion": 0, "sentiment": 1}            # MMDA_TASK_*
SENTI_LOSS = {"l1": 0, "mse": 1}                 # MMDA_SENTI_*
SENTI_STATE_WORDS, SENTI_FIGURES = 24, 9         # MMDA_SENTI_STATE_WORDS, MMDA_SENTI_FIGURES
SCALING_HOW = {"temperature": 0, "platt": 1}     # MMDA_SCALING_*
RELIAB_FIGURES, RELIAB_GRID_CAP, SCALING_MAX_ITER = 8, 32, 256   # MMDA_RELIAB_FIGURES, MMDA_RELIAB_GRID_CAP, MMDA_SCALING_MAX_ITER

# name -> (restype, argtypes).  Every symbol include/mmda_hip.h declares appears here (tests/test_abi.py checks it).
_P, _I, _I64, _F, _U64 = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_uint64
SIGNATURES = {
    "mmda_last_error": (C.c_char_p, []),
    "mmda_abi_version": (_I, []),
    "mmda_scratch_release": (_I, []),
    "mmda_debug_gemm_dma_mode": (_I, [_I]),
    "mmda_gemm": (_I, [C.POINTER(GemmArgs), _P]),
    "mmda_gemm_grouped": (_I, [C.POINTER(GemmArgs), _I, _P]),
    "mmda_gemm_plan_describe": (_I, [C.POINTER(GemmArgs), _I, _I, C.POINTER(GemmPlanRow), _I]),
    "mmda_gemm_bf16_grouped": (_I, [C.POINTER(GemmBf16Args), _I, _P]),
    "mmda_gemm_bf16_plan_describe": (_I, [C.POINTER(GemmBf16Args), _I, C.POINTER(C.c_int), C.POINTER(GemmBf16PlanRow), _I]),
    "mmda_convert_bf16": (_I, [C.POINTER(ConvertJob), _I, _P]),
    "mmda_gemm_skinny": (_I, [C.POINTER(SkinnyArgs), _I, _P]),
    "mmda_mx8_quant_bytes": (_I64, [_I, _I]),
    "mmda_mx8_quant": (_I, [C.POINTER(Mx8QuantJob), _I, _P]),
    "mmda_gemm_mx8": (_I, [C.POINTER(Mx8Args), _P]),
    "mmda_transpose_f32": (_I, [C.POINTER(TransposeJob), _I, _P]),
    "mmda_colsum": (_I, [_P, _I, _I, _I, _P, _P, _P]),
    "mmda_embed_gather": (_I, [_P, _P, _I, _I, _P, _P]),
    "mmda_embed_scatter_add": (_I, [_P, _P, _I, _I, _P, _P]),
    "mmda_embed_segment_sum_work_bytes": (_I64, [_I, _I]),
    "mmda_embed_segment_sum": (_I, [_P, _P, _I, _I, _P, _P, _I64, _P]),
    "mmda_allreduce": (_I, [_P, C.c_size_t, _P, _P]),
    "mmda_layernorm_fwd": (_I, [C.POINTER(LnArgs), _P]),
    "mmda_layernorm_bwd": (_I, [C.POINTER(LnBwdArgs), _P]),
    "mmda_layernorm_fwd_multi": (_I, [C.POINTER(LnArgs), _I, _P]),
    "mmda_layernorm_bwd_multi": (_I, [C.POINTER(LnBwdArgs), _I, _P]),
    "mmda_layernorm_param_grads": (_I, [C.POINTER(LnBwdArgs), _I, _P]),
    "mmda_lstm_packed_bytes": (_I64, [_I, _I, _I]),
    "mmda_lstm_xchg_bytes": (_I64, [_I, _I]),
    "mmda_lstm_resident_applicable": (_I, [_I, _I, C.POINTER(LstmDesc), _I, _I, _I]),
    "mmda_lstm_bwd_emits_dg_bf16": (_I, [_I, _I, C.POINTER(LstmDesc), _I, _I]),
    "mmda_lstm_plan_describe": (_I, [_I, C.POINTER(LstmDesc), _I, _I, _I, C.POINTER(C.c_int), C.POINTER(LstmPlan)]),
    "mmda_lstm_kernel_name": (C.c_char_p, [_I]),
    "mmda_debug_set_lstm_stamps": (_I, [_P]),
    "mmda_lstm_pack_whh": (_I, [_I, _I, _P, _P, _P, _P]),
    "mmda_lstm_pack_whh_multi": (_I, [_I, _I, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _P]),
    "mmda_lstm_pack_whh_cluster": (_I, [_I, _P, _P, _P]),
    "mmda_lstm_pack_whh_and_convert": (_I, [_I, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                            C.POINTER(C.c_void_p), C.POINTER(ConvertJob), _I, _P]),
    "mmda_lstm_pack_convert_transpose": (_I, [_I, C.POINTER(C.c_int), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_void_p), C.POINTER(ConvertJob), _I, C.POINTER(TransposeJob), _I, _P]),
    "mmda_lstm_fwd": (_I, [_I, _I, C.POINTER(LstmDesc), _I, _I, _P, _P]),
    "mmda_lstm_bwd": (_I, [_I, _I, C.POINTER(LstmDesc), _I, _I, _P, _P]),
    "mmda_gru_pad_params": (_I, [C.POINTER(GruPadJob), _I, _P]),
    "mmda_gru_unpad_grads": (_I, [C.POINTER(GruPadJob), _I, _P]),
    "mmda_attn_fwd": (_I, [_P, _I, _I, _I, _I, _P, _P, _F, _U64, _I, _P]),
    "mmda_attn_bwd": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _F, _U64, _I, _P]),
    "mmda_add": (_I, [_P, _P, _P, _I64, _P]),
    "mmda_sigmoid_bwd_inplace": (_I, [_P, _P, _I64, _P]),
    "mmda_act_dropout_fwd": (_I, [_P, _P, _I64, _I, _F, _U64, _I, _P]),
    "mmda_act_dropout_bwd": (_I, [_P, _P, _P, _I64, _I, _F, _U64, _I, _P]),
    "mmda_act_dropout_fwd_p": (_I, [_P, _P, _I64, _I, C.POINTER(ActParams), _F, _U64, _I, _P]),
    "mmda_act_dropout_bwd_p": (_I, [_P, _P, _P, _I64, _I, C.POINTER(ActParams), _F, _U64, _I, _P]),
    "mmda_heads_fwd": (_I, [_P, _I, _I, _F, _P, _P, _P, _F, _U64, _I, _P]),
    "mmda_heads_bwd": (_I, [_P, _P, _P, _P, _I, _I, _P, _F, _U64, _I, _P]),
    "mmda_heads_fwd_task": (_I, [_P, _I, _I, _F, _P, _P, _P, _F, _U64, _I, _I, _P]),
    "mmda_heads_bwd_task": (_I, [_P, _P, _P, _P, _I, _I, _P, _F, _U64, _I, _I, _P]),
    "mmda_loss_reg": (_I, [_P, _P, _I, _I, _I, _F, _P, _P, _P]),
    "mmda_senti_accumulate": (_I, [_P, _P, _I64, _P, _P]),
    "mmda_senti_finish": (_I, [_P, _P, _P]),
    "mmda_reliab_accumulate": (_I, [_P, _P, _I64, _I, _I, _P, _P]),
    "mmda_reliab_finish": (_I, [_P, _I, _I, _P, _P, _P]),
    "mmda_scaling_work_bytes": (_I64, [_I64, _I]),
    "mmda_scaling_fit": (_I, [_P, _P, _I64, _I, _I, _I, _I, _P, _I64, _P, _P, _P, _P, _P]),
    "mmda_scaling_apply": (_I, [_P, _P, _P, _I64, _I, _P, _P]),
    "mmda_misa_set_task": (_I, [_P, _I, _I]),
    "mmda_loss_cls": (_I, [_P, _P, _I, _I, _F, _P, _P, _P]),
    "mmda_loss_cls_opts": (_I, [_P, _P, _I, _I, _F, _P, _P, C.POINTER(ClsOpts), _P]),
    "mmda_loss_misc_opts": (_I, [_P, _P, _P, _I, _I, _P, _P, _I, _I, _F, _P, _P, _I64, _F, _P, _P, _P, _F, _F, _F, _F, _I,
                                 C.POINTER(ClsOpts), _P]),
    "mmda_label_counts": (_I, [_P, _I64, _I, _P, _P]),
    "mmda_misa_set_cls_loss": (_I, [_P, C.POINTER(ClsOpts)]),
    "mmda_loss_conf": (_I, [_P, _P, _P, _I, _I, _F, _P, _P, _P, _P]),
    "mmda_loss_diff": (_I, [_P, _I64, _I, _I, _F, _P, _P, _P, _P]),
    "mmda_loss_diff_work_floats": (_I64, [_I, _I]),
    "mmda_loss_diff_pairs": (_I, [_P, _I64, _I, _I, C.POINTER(C.c_int), _I, _I, _F, _P, _P, _P, _P]),
    "mmda_loss_cmd_pairs": (_I, [_P, _I64, _I, _I, C.POINTER(C.c_int), _I, _I, _I, _F, _F, _P, _P, _P]),
    "mmda_loss_cmd": (_I, [_P, _I64, _I, _I, _F, _P, _P, _P]),
    "mmda_loss_recon": (_I, [_P, _P, _I64, _I, _I, _F, _P, _P, _P, _P]),
    "mmda_loss_misc": (_I, [_P, _P, _P, _I, _I, _P, _P, _I, _I, _F, _P, _P, _I64, _F, _P, _P, _P, _F, _F, _F, _F, _I, _P]),
    "mmda_eval_accumulate": (_I, [_P, _P, _I, _I, _P, _P]),
    "mmda_calib_accumulate": (_I, [_P, _P, _I64, _I, _P, _I, _P, _P, _P]),
    "mmda_calib_select": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, _P, _P, _P]),
    "mmda_eval_accumulate_thr": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "mmda_rank_plan_describe": (_I, [_I64, _I, C.POINTER(RankPlan)]),
    "mmda_rank_counts": (_I, [_P, _P, _I64, _I, _P, _P]),
    "mmda_rank_finish": (_I, [_P, _P, _I64, _I, C.c_double, _P, _P]),
    "mmda_rank_rows_accumulate": (_I, [_P, _P, _I64, _I, _P, _P]),
    "mmda_loss_domain": (_I, [_P, _I, _F, _P, _P, _P]),
    "mmda_loss_forms_describe": (_I, [_I, _I, _I, _I, _I, _I64, C.POINTER(LossForms)]),
    "mmda_clamp_adam": (_I, [_P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mmda_clamp_adam_rows": (_I, [_P, _P, _P, _P, _I, _I, _P, _I, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mmda_embed_rows_sparse_adam": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _I, _I, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mmda_mark_rows": (_I, [_P, _I, _P, _I, _P]),
    "mmda_embed_deferred_scalar_floats": (_I64, [_I]),
    "mmda_embed_deferred_reset": (_I, [_P, _I, _P]),
    "mmda_embed_rows_dense_adam": (_I, [_P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _I, _I, _F, _F, _F, _F, _F, _F, _I, _I, _P]),
    "mmda_embed_rows_catch_up": (_I, [_P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _I, _I, _F, _F, _F, _I, _P]),
    "mmda_embed_rows_flush": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _I, _P]),
    "mmda_clamp": (_I, [_P, _I64, _F, _P]),
    "mmda_clamp_rmsprop": (_I, [_P, _P, _P, _I64, _F, _F, _F, _F, _F, _P]),
    "mmda_grad_accumulate": (_I, [_P, _P, _I64, _I, _P]),
    "mmda_clamp_adam_sum": (_I, [_P, _P, _P, _P, _P, _I64, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mmda_embed_rows_append": (_I, [_P, _P, _I64, _I64, _P, _P, _I, _I, _P, _I, _P]),
    "mmda_runs_build": (_I64, [C.POINTER(_I64), C.POINTER(_I64), _I, _I64, C.POINTER(Run), C.POINTER(_I)]),
    "mmda_clamp_adam_runs": (_I, [_P, _P, _P, _P, _P, _I, _I64, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mmda_clamp_adam_sum_runs": (_I, [_P, _P, _P, _P, _P, _P, _I, _I64, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mmda_clamp_rmsprop_runs": (_I, [_P, _P, _P, _P, _I, _I64, _F, _F, _F, _F, _F, _P]),
    "mmda_clamp_adam_opts": (_I, [_P, _P, _P, _P, _P, _I64, _P, _I, _I64, _F, _F, _F, _I, C.POINTER(AdamOpts), _P]),
    "mmda_clamp_adam_rows_opts": (_I, [_P, _P, _P, _P, _I, _I, _P, _I, _F, _F, _F, _I, C.POINTER(AdamOpts), _P]),
    "mmda_grad_norm_partials": (_I64, [_I64]),
    "mmda_grad_norm": (_I, [_P, _P, _I64, _P, _I, _I64, _F, _F, _P, _I64, _P, _P]),
    "mmda_grad_scale": (_I, [_P, _I64, _P, _I, _I64, _P, _P]),
    "mmda_misa_set_adam": (_I, [_P, C.POINTER(AdamOpts), _F]),
    "mmda_misa_create": (_I, [C.POINTER(MisaConfig), C.POINTER(C.c_void_p)]),
    "mmda_misa_destroy": (None, [_P]),
    "mmda_misa_num_params": (_I, [_P]),
    "mmda_misa_param_info": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_I64), C.POINTER(_I), C.POINTER(_I)]),
    "mmda_misa_flat_floats": (_I64, [_P]),
    "mmda_misa_dense_floats": (_I64, [_P]),
    "mmda_misa_bind": (_I, [_P, _P, _P, _P, _P]),
    "mmda_misa_workspace_floats": (_I64, [_P, _I, _I]),
    "mmda_misa_plan_describe": (_I, [_P, _I, _I, C.POINTER(MisaStepRequest), C.POINTER(C.c_int), _I, C.POINTER(MisaStepPlan)]),
    "mmda_misa_set_workspace": (_I, [_P, _P, _I64, _I, _I]),
    "mmda_misa_set_workspace_async": (_I, [_P, _P, _I64, _I, _I, _P]),
    "mmda_misa_tensor_offset": (_I64, [_P, C.c_char_p]),
    "mmda_misa_set_mode": (_I, [_P, _I]),
    "mmda_misa_set_overlap": (_I, [_P, _I]),
    "mmda_misa_set_recurrence": (_I, [_P, _I]),
    "mmda_misa_set_gemm_operands": (_I, [_P, _I]),
    "mmda_misa_early_grad_floats": (_I64, [_P]),
    "mmda_misa_wait_early_grads": (_I, [_P, _P]),
    "mmda_misa_set_inference": (_I, [_P, _I]),
    "mmda_misa_set_fusion_fp8": (_I, [_P, _I]),
    "mmda_misa_set_embed_update": (_I, [_P, _I]),
    "mmda_misa_set_trainable": (_I, [_P, C.c_char_p, _I]),
    "mmda_misa_trainable_info": (_I, [_P, C.POINTER(Run), _I, C.POINTER(_I), C.POINTER(_I64), C.POINTER(_I)]),
    "mmda_misa_set_cut_forward": (_I, [_P, _I]),
    "mmda_misa_set_embed_deferred": (_I, [_P, _P, _P, _I, _P]),
    "mmda_misa_embed_deferred_step": (_I, [_P, _F, _F, _F, _F, _F, _F, _I, _P]),
    "mmda_misa_embed_flush": (_I, [_P, _P]),
    "mmda_misa_set_embed_background": (_I, [_P, _I, _I]),
    "mmda_misa_embed_background_active": (_I, [_P]),
    "mmda_misa_cluster_status": (_I, [_P, C.POINTER(_I)]),
    "mmda_misa_forward": (_I, [_P, _P, _P, _P, _P, _I, _U64, _P]),
    "mmda_misa_losses": (_I, [_P, _P, _I, _P]),
    "mmda_misa_set_external_batch_losses": (_I, [_P, _I]),
    "mmda_misa_backward": (_I, [_P, _P, _P, _P, _P, _P]),
    "mmda_misa_zero_grad": (_I, [_P, _P]),
    "mmda_misa_zero_act_grads": (_I, [_P, _P]),
    "mmda_misa_adam_step": (_I, [_P, _F, _F, _F, _I, _P]),
    "mmda_misa_grad_accumulate": (_I, [_P, _P, _I, _P, _P, _I64, _I64, _P]),
    "mmda_misa_adam_step_accumulated": (_I, [_P, _P, _P, _P, _I64, _I64, _F, _F, _F, _I, _P]),
    "mmda_misa_timing_stride": (_I, [_P, _I]),
    "mmda_misa_timing_rotate": (_I, [_P, _I]),
    "mmda_misa_timing_begin": (_I, [_P, _I]),
    "mmda_misa_timing_collect": (_I, [_P, C.POINTER(C.c_float * 4), C.POINTER(_I)]),
    "mmda_misa_timing_end": (_I, [_P]),
    "mmda_misa_train_step": (_I, [_P, _P, _P, _P, _P, _P, _I, _U64, _I, _F, _F, _I, _P]),
    "mmda_collate_gather": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "mmda_infer_collect": (_I, [C.POINTER(InferSrc), C.POINTER(InferOut), _P, _I64, _I, _P]),
    "mmda_misa_infer_collect": (_I, [_P, C.POINTER(InferOut), _P, _I64, _P]),
    "mmda_encoded_collect": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P, _P, _I64, _I, _P]),
    "mmda_encoded_gather": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P]),
    "mmda_misa_encoded_collect": (_I, [_P, _P, _P, _P, _P, _I64, _P]),
    "mmda_misa_forward_encoded": (_I, [_P, C.POINTER(EncodedBatch), _I, _U64, _P]),
    "mmda_misa_train_step_encoded": (_I, [_P, C.POINTER(EncodedBatch), _P, _I, _U64, _I, _F, _F, _I, _P]),
    "mmda_collate_gather_masked": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, ModalityP, _U64, _I, _P, _P, _P, _P, _P, _P, _P]),
    "mmda_modality_mask": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "mmda_modality_attrib": (_I, [_P, _I64, _I, _P, _P, _P, _P, _P]),
    "mmda_mc_reduce": (_I, [_P, _I, _I, _I, _P, _I, C.POINTER(McOut), _P, _I64, _P]),
    "mmda_misa_mc_reduce": (_I, [_P, _I, _I, _P, C.POINTER(McOut), _P, _I64, _P]),
    "mmda_boot_plan_describe": (_I, [_I64, _I, _I, C.POINTER(BootPlan)]),
    "mmda_boot_pack": (_I, [_P, _P, _I64, _I, _P, _P]),
    "mmda_boot_counts": (_I, [_P, _I64, _I, _I, _U64, _I, _P, _P]),
    "mmda_boot_figures": (_I, [_P, _I, _I, _P, _P]),
    "mmda_boot_rank": (_I, [_P, _P, _P, _P, _I64, _I, _I, _U64, C.c_double, _P, _P]),
    "mmda_boot_summary": (_I, [_P, _P, _I, _I, C.c_double, C.c_double, _I, _P, _P]),
    "mmda_knn_plan_describe": (_I, [_I64, _I64, _I, _I, _I, C.POINTER(KnnPlan)]),
    "mmda_knn_sets": (_I, [_P, _P, _P, _I64, _I64, _I, _I, _I, _I, _P, _P, _P, _I64, _P]),
    "mmda_trust_score": (_I, [_P, _P, _P, _I64, _I, _I, _P, _P, _P, _P, _P, _P]),
}

_lib = None


class MMDAError(RuntimeError):
    pass


def load():
    """Load the library once.  Raises (never falls back) if it is missing: build it with
    ``python -c 'import __graft_entry__ as g; g.build()'`` or ``make -C mmda_amd/csrc``."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MMDAError(f"{LIB_PATH} not found: the HIP hot-path library is not built (make -C mmda_amd/csrc); "
                        "there is no CPU/PyTorch fallback")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/binding drift
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        lib = load()
        msg = lib.mmda_last_error()
        raise MMDAError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else t.data_ptr()


def stream_ptr():
    import torch
    return torch.cuda.current_stream().cuda_stream


def device_tables(a, b, who, names=None, dims="(N, C)"):
    """The two tables an evaluation report of ``who`` is given, detached, fp32 and contiguous: ``MMDAError`` unless both are device
    tensors; with ``names`` (how the message calls them, such as "scores and truth") ``ValueError`` unless both are 2-D of one
    shape."""
    import torch
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.is_cuda and b.is_cuda):
        raise MMDAError(f"{who} needs device tensors (the HIP path has no CPU fallback)")
    if names is not None and (a.dim() != 2 or b.shape != a.shape):
        raise ValueError(f"{names} must both be {dims}, not {tuple(a.shape)} and {tuple(b.shape)}")
    return a.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()
