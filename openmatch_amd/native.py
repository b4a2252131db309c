"""ctypes binding of libopenmatch_hip.so (C ABI declared in include/openmatch_hip.h).

The product path has NO fallback: if the shared library is missing, was built for another
ABI version, or a tensor does not live on an MI355X device, the call raises.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libopenmatch_hip.so")

OM_F32, OM_BF16, OM_F16 = 0, 1, 2
ACT_NONE, ACT_GELU_ERF, ACT_RELU, ACT_GELU_TANH = 0, 1, 2, 3
ACT_SILU = 5
ACT_MUL_RESID = 0x100
ACT_GELU_ERF_GRAD, ACT_PRE_GRAD = 4, 0x200      # training epilogues (csrc/kernels.h; include/openmatch_hip.h), om_debug_gemm_ex only
ARCH_BERT, ARCH_T5, ARCH_MODERNBERT, ARCH_CAUSAL, ARCH_NOMICBERT, ARCH_GEMMA3 = 0, 1, 2, 3, 4, 5
POOL_NONE, POOL_FIRST, POOL_MEAN, POOL_LAST = 0, 1, 2, 3
# om_debug_option switches used from Python (include/openmatch_hip.h: OM_OPT_*)
OPT_TRAIN_WGRAD_BATCH, OPT_GEMM_MAX_GRID, OPT_GEMM_CONT = 14, 15, 16
OPT_WGRAD_DEBUG = 5              # bit 3: the register-staged weight-gradient kernel for everything; value >> 4: workgroups aimed at / 64
OPT_GEMM_GROUP_M, OPT_GEMM_VARIANT, OPT_GEMM_SKINNY_M = 6, 12, 19
# om_debug_gemm_last codes (include/openmatch_hip.h: OM_GEMM_FAMILY_*)
GEMM_FAMILY = {"v1": 1, "v2": 2, "v6": 6, "g7": 7, "g7_one_tile": 70, "7c16": 71, "7r16": 72, "skinny": 9}
# om_debug_attention_last codes (include/openmatch_hip.h: OM_ATTN_FAMILY_*); the call returns family | key tiles << 8
ATTN_FAMILY = {"generic": 1, "fwd16": 2, "fwd16_kmax4": 3, "fwd16c": 4, "long": 5, "d32": 6, "band16": 7, "band32": 8}
# om_debug_attention_gqa_plan codes (OM_ATTN_GQA_FAMILY_*): out[0] of the call
GQA_FAMILY = {"causal64": 1, "causal128": 2, "full256": 3, "band256": 4}
# om_debug_attention_bwd_last codes (OM_ATTN_BWD_FAMILY_*), packed the same way
ATTN_BWD_FAMILY = {"bwd16": 1, "generic": 2, "long": 3, "d32": 4}
# om_debug_encoder_plan codes (OM_ENC_PATH_*); the call returns path | few_rows << 8 | two << 9 | lo8 << 10
ENC_PATH = {"bert_fused": 1, "bert_pending_ln": 2, "bert_few32": 3, "bert_plain": 4, "modernbert": 5, "t5_fused": 6, "t5_plain": 7}
# om_debug_scan_plan / om_sim_topk_info[5] codes (OM_SCAN_FAMILY_*); 0: the search never left the dense path
SCAN_FAMILY = {"dense": 0, "generic": 1, "wide": 2, "stream32": 3, "stream16": 4}
SCAN_FAMILY_NAME = {v: k for k, v in SCAN_FAMILY.items()}
# om_debug_scan_round / om_sim_topk_info[6] codes (OM_SCAN_KERNEL_*): the main launch of the last filtered round
SCAN_KERNEL = {"dense": 0, "tile2": 1, "tile6": 2, "wide7": 3, "wide7c": 4, "stream": 5}
SCAN_KERNEL_NAME = {v: k for k, v in SCAN_KERNEL.items()}
OPT_SCAN_GEN7 = 3
OPT_ATTENTION_FAST = 2
SEARCH_F32, SEARCH_F16_RESCORE, SEARCH_F16_ONLY = 0, 1, 2
DEBUG_LISTS = {"radix": 0, "sort": 1, "drop": 2, "append": 3, "emit": 4}      # OM_DEBUG_LISTS_*: the op of om_debug_select_lists
ABI_VERSION = 6

c_void_p, c_int, c_int64, c_float, c_size_t = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t


class OmLayerWeights(C.Structure):
    _fields_ = [(n, c_void_p) for n in (
        "qkv_w", "qkv_b", "o_w", "o_b", "ln1_g", "ln1_b", "ffn1_w", "ffn1_b", "ffn1g_w",
        "ffn2_w", "ffn2_b", "ln2_g", "ln2_b")]


class OmEncoderConfig(C.Structure):
    _fields_ = [("arch", c_int), ("dtype", c_int), ("hidden", c_int), ("n_layers", c_int),
                ("n_heads", c_int), ("head_dim", c_int), ("ffn", c_int), ("vocab", c_int),
                ("max_pos", c_int), ("type_vocab", c_int), ("act", c_int), ("ln_eps", c_float),
                ("rel_buckets", c_int), ("rel_max_dist", c_int), ("pooling", c_int),
                ("head_in", c_int), ("head_out", c_int), ("normalize", c_int),
                # ABI v6 (ModernBERT; NomicBERT: rope_theta_global; zero for BERT / T5)
                ("rope_theta_global", c_float), ("rope_theta_local", c_float), ("half_window", c_int),
                ("sliding_layers", C.c_uint64)]


class OmCausalConfig(C.Structure):
    """Llama / Qwen2 (om_causal_encoder_forward): the encoder's config, untouched, followed by what a grouped-query rotary stack adds."""
    _fields_ = [("base", OmEncoderConfig), ("n_kv_heads", c_int), ("rope_attention_scaling", c_float), ("inv_freq", c_float * 32)]


class OmCausalConfig2(C.Structure):
    """Qwen3 (om_causal2_encoder_forward): OmCausalConfig, untouched, followed by the q / k norm flag and the 64 frequencies of head_dim 128."""
    _fields_ = [("base", OmCausalConfig), ("qk_norm", c_int), ("reserved", c_int), ("inv_freq", c_float * 64)]


class OmCausalQkNorm(C.Structure):
    """One layer's q_norm.weight / k_norm.weight: device pointers to [head_dim] f32."""
    _fields_ = [("q_norm_g", c_void_p), ("k_norm_g", c_void_p)]


class OmGemma3Config(C.Structure):
    """EmbeddingGemma (om_gemma3_encoder_forward): OmCausalConfig, untouched, followed by the score scale, the band, the per-layer-type
    rotary tables and the two switches the entry refuses by name."""
    _fields_ = [("base", OmCausalConfig), ("attn_scale", c_float), ("half_window", c_int), ("sliding_layers", C.c_uint64),
                ("full_scaling", c_float), ("sliding_scaling", c_float), ("attn_logit_softcapping", c_float), ("bidirectional", c_int),
                ("full_inv_freq", c_float * 128), ("sliding_inv_freq", c_float * 128)]


class OmGemma3Norms(C.Structure):
    """One layer's q_norm / k_norm / post_attention_layernorm / post_feedforward_layernorm as g = 1 + weight: device pointers, f32."""
    _fields_ = [(n, c_void_p) for n in ("q_norm_g", "k_norm_g", "post_attention_norm_g", "post_feedforward_norm_g")]


class OmEncoderWeights(C.Structure):
    _fields_ = [("word_emb", c_void_p), ("pos_emb", c_void_p), ("type_emb", c_void_p),
                ("emb_ln_g", c_void_p), ("emb_ln_b", c_void_p),
                ("layers_host", C.POINTER(OmLayerWeights)), ("final_ln_g", c_void_p),
                ("rel_bias", c_void_p), ("head_w", c_void_p), ("folded", c_void_p), ("final_ln_b", c_void_p)]


class OmTnProblem(C.Structure):
    """One weight-gradient contraction of an om_gemm_tn_acc_batch launch (include/openmatch_hip.h)."""
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p), ("bias", c_void_p),
                ("lda", c_int64), ("ldb", c_int64), ("ldc", c_int64), ("N", c_int64), ("K", c_int64)]


class OmT5DecoderLayer(C.Structure):
    _fields_ = [(n, c_void_p) for n in (
        "sa_v_w", "sa_o_w", "sa_ln_g", "ca_q_w", "ca_kv_w", "ca_o_w", "ca_ln_g", "ffn1_w", "ffn1g_w", "ffn2_w", "ffn_ln_g")]


class OmT5DecoderWeights(C.Structure):
    _fields_ = [("start_emb", c_void_p), ("final_ln_g", c_void_p),
                ("layers_host", C.POINTER(OmT5DecoderLayer)), ("n_layers", c_int)]


class OmT5DecoderLayerGrads(C.Structure):
    _fields_ = [(n, c_void_p) for n in (
        "sa_v_w", "sa_o_w", "sa_ln_g", "ca_q_w", "ca_kv_w", "ca_o_w", "ca_ln_g", "ffn1_w", "ffn1g_w", "ffn2_w", "ffn_ln_g")]


class OmT5DecoderGrads(C.Structure):
    _fields_ = [("start_emb", c_void_p), ("final_ln_g", c_void_p), ("layers_host", C.POINTER(OmT5DecoderLayerGrads))]


class OmAdamTensor(C.Structure):
    """One parameter of an om_adamw_step launch (include/openmatch_hip.h)."""
    _fields_ = [("p", c_void_p), ("g", c_void_p), ("m", c_void_p), ("v", c_void_p), ("shadow0", c_void_p), ("shadow1", c_void_p),
                ("n", c_int64), ("weight_decay", c_float), ("shadow0_dtype", c_int), ("shadow1_dtype", c_int), ("reserved", c_int)]


class OmDebugGemmEpilogue(C.Structure):
    """Every field of the internal GemmEpilogue but its trace pointer (om_debug_gemm_ex / om_debug_gemm_plan_ex)."""
    _fields_ = [("bias", c_void_p), ("resid", c_void_p), ("ldr", c_int64), ("act", c_int),
                ("pre_act", c_void_p), ("ldp", c_int64), ("drop_p", c_float), ("seed", C.c_uint64), ("drop_rows", c_void_p),
                ("ln_stats", c_void_p), ("ln_colsum", c_void_p), ("rln_stats", c_void_p), ("rln_g", c_void_p), ("rln_b", c_void_p),
                ("stats_out", c_void_p), ("resid_lo", c_void_p), ("out_lo", c_void_p), ("resid32", c_void_p), ("out32", c_void_p),
                ("a_ln32", c_void_p), ("a_ln_g", c_void_p), ("a_ln_b", c_void_p), ("a_ln_stats_out", c_void_p), ("rln32", c_void_p),
                ("rln32_stats", c_void_p), ("lo8", c_int), ("ln_inv_h", c_float), ("ln_eps", c_float), ("ln_rms", c_int),
                ("reverse", c_int), ("rows_dev", c_void_p)]


class OmLnSite(C.Structure):
    """One LayerNorm site of om_debug_ln_param_reduce (include/openmatch_hip.h)."""
    _fields_ = [("partial", c_void_p), ("dg", c_void_p), ("db", c_void_p), ("blocks", c_int)]


# om_debug_row_kernel_last (include/openmatch_hip.h: OM_ROW_*)
ROW_KERNEL = {"fwd_generic": 1, "fwd_x8": 2, "ln_bwd": 3}
OPT_TRAIN_WGRAD_STREAM = 8
ADAM_CHUNK = 16384


class OmLayerGrads(C.Structure):
    _fields_ = [(n, c_void_p) for n in (
        "qkv_w", "qkv_b", "o_w", "o_b", "ln1_g", "ln1_b", "ffn1_w", "ffn1_b", "ffn2_w", "ffn2_b",
        "ln2_g", "ln2_b", "ffn1g_w")]


class OmEncoderGrads(C.Structure):
    _fields_ = [("word_emb", c_void_p), ("pos_emb", c_void_p), ("type_emb", c_void_p),
                ("emb_ln_g", c_void_p), ("emb_ln_b", c_void_p),
                ("layers_host", C.POINTER(OmLayerGrads)), ("head_w", c_void_p),
                ("final_ln_g", c_void_p), ("rel_bias", c_void_p)]


_SIGNATURES = {
    "om_last_error": (C.c_char_p, []),
    "om_abi_version": (c_int, []),
    "om_device_count": (c_int, []),
    "om_debug_gemm_trace": (None, [c_void_p]),
    "om_debug_gemm_gen": (None, [c_int]),
    "om_debug_option": (c_int, [c_int, c_int]),
    "om_debug_option_value": (c_int, [c_int]),
    "om_debug_gemm_last": (c_int, []),
    "om_debug_gemm_plan": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64,
                                   c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int]),
    "om_debug_gemm_ex": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64,
                                 c_int64, c_int64, c_int64, C.POINTER(OmDebugGemmEpilogue), c_void_p]),
    "om_debug_gemm_plan_ex": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64,
                                      c_int64, c_int64, c_int64, C.POINTER(OmDebugGemmEpilogue)]),
    "om_debug_gemm_splitk": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p]),
    "om_debug_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "om_debug_attention_ex": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_float,
                                      C.c_uint64, c_void_p, c_int, c_void_p, c_void_p, c_int]),
    "om_debug_rope": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_float, c_void_p]),
    "om_debug_rope_rows": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_float, c_void_p, c_void_p]),
    "om_debug_swiglu_rows": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "om_debug_embed": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int,
                               c_int, c_int, c_float, c_void_p]),
    "om_debug_attention_causal": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_void_p]),
    "om_debug_rope_gqa": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_int, C.POINTER(c_float), c_float, c_void_p]),
    "om_debug_attention_causal_packed": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_void_p]),
    "om_debug_rope_gqa_rows": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_int, C.POINTER(c_float), c_float, c_void_p, c_void_p]),
    "om_debug_attention_causal_hd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "om_debug_attention_causal_hd_packed": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_float,
                                                    c_void_p]),
    "om_debug_qknorm_rope": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, C.POINTER(c_float),
                                     c_float, c_void_p]),
    "om_debug_qknorm_rope_rows": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, C.POINTER(c_float),
                                          c_float, c_void_p, c_void_p]),
    "om_debug_attention_gqa_d256": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_int, c_void_p]),
    "om_debug_qknorm_rope_d256": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_float, C.POINTER(c_float), c_float,
                                          c_void_p]),
    "om_debug_attention_gqa_d256_packed": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, c_int,
                                                   c_void_p]),
    "om_debug_qknorm_rope_d256_rows": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_float, C.POINTER(c_float),
                                               c_float, c_void_p, c_void_p]),
    "om_debug_rmsnorm_add": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "om_debug_mask_extent": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "om_debug_pack_rows": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "om_debug_attention_last": (c_int, []),
    "om_debug_attention_plan": (c_int, [c_int, c_int64, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int]),
    "om_debug_attention_gqa_plan": (c_int, [c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_int64)]),
    "om_debug_attention_bwd_last": (c_int, []),
    "om_debug_attention_bwd_plan": (c_int, [c_int, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "om_debug_attention_bwd_ex": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                                          c_int, c_int, c_float, c_float, C.c_uint64, c_void_p, c_int, c_void_p]),
    "om_debug_attention_bwd_stats_bytes": (c_size_t, [c_int64, c_int]),
    "om_debug_encoder_plan": (c_int, [C.POINTER(OmEncoderConfig), c_int, c_int, c_int64, c_int64, c_int64, c_int]),
    "om_debug_train_plan": (c_int, [C.POINTER(OmEncoderConfig), c_int64, c_int64, c_int64, c_int, c_int, c_int, c_int]),
    "om_debug_encoder_skip_pad": (c_int, [C.POINTER(OmEncoderConfig), c_int, c_int, c_int64, c_int64, c_int]),
    "om_debug_encoder_cls_tail": (c_int, [C.POINTER(OmEncoderConfig), c_int, c_int, c_int64, c_int64, c_int64, c_int]),
    "om_debug_encoder_lanes": (c_int, [C.POINTER(OmEncoderConfig), c_int, c_int, c_int64, c_int64, c_int64, c_int, C.POINTER(c_int64)]),
    "om_debug_encoder_lane_ranges": (c_int, [C.POINTER(OmEncoderConfig), c_int, c_int, c_int64, c_int64, c_int, C.POINTER(c_int64), c_int]),
    "om_debug_encoder_lane_forks": (c_int64, []),
    "om_debug_gather_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                     c_int64, c_int, c_void_p]),
    "om_debug_attn_drop_keep": (c_int, [C.c_uint64, c_int64, c_int, c_int, c_int, c_int, c_int, c_float]),
    "om_debug_wave_sum_check": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "om_debug_row_kernel_last": (c_int, []),
    "om_debug_row_fwd_plan": (c_int, [c_int, c_int, c_int64, c_int, c_int64, c_int64, c_int, c_int, c_int, c_int]),
    "om_debug_row_bwd_plan": (c_int, [c_int, c_int, c_int64, c_int, c_int, c_int, c_int, c_int, C.POINTER(c_int64)]),
    "om_debug_layernorm": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_float, c_int, c_void_p,
                                   c_int, c_void_p]),
    "om_debug_layernorm_f32out": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_float, c_int,
                                          c_void_p, c_void_p, c_int, c_void_p]),
    "om_debug_layernorm_from_f32": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_float, c_int,
                                            c_void_p]),
    "om_debug_layernorm_dual": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_float,
                                        c_void_p]),
    "om_debug_norm_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_int, c_void_p,
                                  c_void_p]),
    "om_debug_ln_bwd_drop": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, C.c_uint64, c_void_p, c_void_p, c_int64,
                                     c_int, c_float, c_void_p, c_void_p, c_void_p, C.POINTER(c_int), c_void_p, c_void_p]),
    "om_debug_ln_param_reduce": (c_int, [C.POINTER(OmLnSite), c_int, c_int, c_void_p]),
    "om_debug_embed_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "om_debug_pool": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "om_debug_pool_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p]),
    "om_debug_l2norm": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "om_debug_l2norm_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "om_debug_colsum": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "om_debug_dropout": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_float, C.c_uint64, c_void_p, c_int, c_void_p]),
    "om_debug_ln_fold": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "om_debug_ln_stats_reduce": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "om_encoder_fold_bytes": (c_size_t, [C.POINTER(OmEncoderConfig)]),
    "om_encoder_fold_weights": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p, c_size_t, c_void_p]),
    "om_kernel_timing_enable": (c_int, [c_int]),
    "om_kernel_timing_read": (c_int, [c_int, C.POINTER(C.c_double), C.POINTER(c_int64), C.POINTER(C.c_double)]),
    "om_gemm_nt": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64,
                           c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "om_gemm_tn_acc": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                               c_int64, c_int64, c_int64, c_void_p]),
    "om_gemm_tn_acc_batch": (c_int, [c_int, C.POINTER(OmTnProblem), c_int, c_int64, c_void_p]),
    "om_debug_gemm_tn_last": (c_int, [C.POINTER(c_int64)]),
    "om_debug_gemm_tn_plan": (c_int, [c_int, c_int64, c_int64, c_int64, c_int64, c_int64, c_int, C.POINTER(c_int64)]),
    "om_debug_transpose": (c_int, [c_int, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64, c_int64, c_int, c_void_p]),
    "om_debug_transpose_batch": (c_int, [c_int, C.POINTER(c_void_p), C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_int), c_int, c_void_p]),
    "om_debug_zero_rows_from": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "om_debug_t5_act_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "om_debug_t5_act_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "om_debug_t5_embed_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "om_debug_t5_bias": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "om_debug_t5_bias_bwd": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "om_debug_dec_cross": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_float, C.c_uint64, c_void_p]),
    "om_debug_dec_cross_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int,
                                       c_float, C.c_uint64, c_void_p]),
    "om_debug_dec_final": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p]),
    "om_debug_dec_head_drop": (c_int, [c_int, c_void_p, c_int64, c_int, c_float, C.c_uint64, c_void_p]),
    "om_debug_dec_start": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "om_debug_dec_cast": (c_int, [c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "om_debug_dec_site": (C.c_uint64, [C.c_uint64, c_int, c_int]),
    "om_encoder_workspace_bytes": (c_size_t, [C.POINTER(OmEncoderConfig), c_int64, c_int64]),
    "om_t5_decoder_workspace_bytes": (c_size_t, [C.POINTER(OmEncoderConfig), c_int64, c_int64]),
    "om_t5_decoder_step": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmT5DecoderWeights), c_void_p, c_void_p,
                                   c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_t5_relative_bucket": (c_int, [c_int, c_int, c_int]),
    "om_encoder_forward": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p,
                                   c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                   c_void_p, c_size_t, c_void_p]),
    "om_causal_encoder_workspace_bytes": (c_size_t, [C.POINTER(OmCausalConfig), c_int64, c_int64]),
    "om_causal_encoder_forward": (c_int, [C.POINTER(OmCausalConfig), C.POINTER(OmEncoderWeights), c_void_p, c_void_p, c_int64, c_int64,
                                          c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_causal_encoder_packed_supported": (c_int, [C.POINTER(OmCausalConfig), c_int64, c_int64, c_int64]),
    "om_causal_encoder_workspace_bytes_packed": (c_size_t, [C.POINTER(OmCausalConfig), c_int64, c_int64, c_int64]),
    "om_causal_encoder_forward_packed": (c_int, [C.POINTER(OmCausalConfig), C.POINTER(OmEncoderWeights), c_void_p, c_void_p, c_int64, c_int64,
                                                 c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_causal2_encoder_workspace_bytes": (c_size_t, [C.POINTER(OmCausalConfig2), c_int64, c_int64]),
    "om_causal2_encoder_forward": (c_int, [C.POINTER(OmCausalConfig2), C.POINTER(OmEncoderWeights), C.POINTER(OmCausalQkNorm), c_void_p, c_void_p,
                                           c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_causal2_encoder_packed_supported": (c_int, [C.POINTER(OmCausalConfig2), c_int64, c_int64, c_int64]),
    "om_causal2_encoder_workspace_bytes_packed": (c_size_t, [C.POINTER(OmCausalConfig2), c_int64, c_int64, c_int64]),
    "om_causal2_encoder_forward_packed": (c_int, [C.POINTER(OmCausalConfig2), C.POINTER(OmEncoderWeights), C.POINTER(OmCausalQkNorm), c_void_p,
                                                  c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_gemma3_encoder_workspace_bytes": (c_size_t, [C.POINTER(OmGemma3Config), c_int64, c_int64]),
    "om_gemma3_encoder_forward": (c_int, [C.POINTER(OmGemma3Config), C.POINTER(OmEncoderWeights), C.POINTER(OmGemma3Norms), c_void_p, c_void_p,
                                          c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_gemma3_encoder_packed_supported": (c_int, [C.POINTER(OmGemma3Config), c_int64, c_int64, c_int64]),
    "om_gemma3_encoder_workspace_bytes_packed": (c_size_t, [C.POINTER(OmGemma3Config), c_int64, c_int64, c_int64]),
    "om_gemma3_encoder_forward_packed": (c_int, [C.POINTER(OmGemma3Config), C.POINTER(OmEncoderWeights), C.POINTER(OmGemma3Norms), c_void_p,
                                                 c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_encoder_packed_supported": (c_int, [C.POINTER(OmEncoderConfig), c_int, c_int64, c_int64, c_int64]),
    "om_encoder_workspace_bytes_packed": (c_size_t, [C.POINTER(OmEncoderConfig), c_int64, c_int64, c_int64]),
    "om_encoder_forward_packed": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p,
                                          c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                          c_void_p, c_size_t, c_void_p]),
    "om_encoder_tape_bytes": (c_size_t, [C.POINTER(OmEncoderConfig), c_int64, c_int64]),
    "om_encoder_train_workspace_bytes": (c_size_t, [C.POINTER(OmEncoderConfig), c_int64, c_int64]),
    "om_encoder_train_forward": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p,
                                         c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, C.c_uint64,
                                         c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_encoder_train_backward": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p,
                                          c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, C.c_uint64,
                                          c_void_p, c_void_p, C.POINTER(OmEncoderGrads), c_void_p, c_size_t,
                                          c_void_p]),
    "om_encoder_train_packed_supported": (c_int, [C.POINTER(OmEncoderConfig), c_int64, c_int64, c_int64]),
    "om_encoder_tape_bytes_packed": (c_size_t, [C.POINTER(OmEncoderConfig), c_int64, c_int64, c_int64]),
    "om_encoder_train_workspace_bytes_packed": (c_size_t, [C.POINTER(OmEncoderConfig), c_int64, c_int64, c_int64]),
    "om_encoder_train_forward_packed": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p,
                                                c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float, c_float, C.c_uint64,
                                                c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_encoder_train_backward_packed": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p,
                                                 c_void_p, c_void_p, c_int64, c_int64, c_int64, c_float, c_float, C.c_uint64,
                                                 c_void_p, c_void_p, C.POINTER(OmEncoderGrads), c_void_p, c_size_t,
                                                 c_void_p]),
    "om_encoder_train_forward_hidden": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p,
                                                c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, C.c_uint64,
                                                c_void_p, c_size_t, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_encoder_train_backward_hidden": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmEncoderWeights), c_void_p,
                                                 c_void_p, c_void_p, c_int64, c_int64, c_float, c_float, C.c_uint64,
                                                 c_void_p, c_void_p, C.POINTER(OmEncoderGrads), c_void_p, c_size_t,
                                                 c_void_p]),
    "om_t5_decoder_tape_bytes": (c_size_t, [C.POINTER(OmEncoderConfig), c_int, c_int64, c_int64]),
    "om_t5_decoder_train_workspace_bytes": (c_size_t, [C.POINTER(OmEncoderConfig), c_int, c_int64, c_int64]),
    "om_t5_decoder_train_forward": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmT5DecoderWeights), c_void_p, c_void_p,
                                            c_int64, c_int64, c_float, C.c_uint64, c_void_p, c_size_t, c_void_p,
                                            c_void_p, c_size_t, c_void_p]),
    "om_t5_decoder_train_backward": (c_int, [C.POINTER(OmEncoderConfig), C.POINTER(OmT5DecoderWeights), c_void_p, c_void_p,
                                             c_int64, c_int64, c_float, C.c_uint64, c_void_p, c_void_p,
                                             C.POINTER(OmT5DecoderGrads), c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_linear_f32_backward": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "om_index_to_f16": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "om_index_add_f16": (c_int, [c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "om_debug_rescore_rows": (c_int, [c_int, c_int, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_size_t,
                                      c_void_p]),
    "om_debug_select_lists": (c_int, [c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_void_p, C.c_uint32,
                                      c_void_p, c_int64, c_int, C.c_uint32, C.c_uint32, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_debug_query_prep": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "om_sim_topk_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "om_sim_topk": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                            c_int, c_int64, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_sim_topk_async_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "om_sim_topk_async": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int,
                                  c_int, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_debug_search_schedule": (c_int, [c_int, c_int64, c_int64, c_int, C.POINTER(c_int64), c_int, C.POINTER(c_int)]),
    "om_sim_topk_filtered_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "om_sim_topk_filtered": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_int64,
                                     c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_sim_topk_filtered_multi_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int64]),
    "om_sim_topk_filtered_multi": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_int64,
                                           c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_sim_topk_excluding_workspace_bytes": (c_size_t, [c_int64, c_int, c_int, c_int64]),
    "om_sim_topk_excluding": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_int64,
                                      c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_debug_search_exclude_schedule": (c_int, [c_int, c_int64, c_int64, c_int, c_int64, C.POINTER(c_int64), c_int, C.POINTER(c_int),
                                                 C.POINTER(c_int64)]),
    "om_debug_drop_lists_excluding": (c_int, [c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_int64, C.c_uint32, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_sim_topk_candidates_workspace_bytes": (c_size_t, [c_int64, c_int, c_int]),
    "om_sim_topk_candidates": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_int64, c_void_p, c_int64, c_void_p,
                                       c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_debug_drop_lists_multi": (c_int, [c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, C.c_uint32, c_int64, c_int64, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "om_debug_search_schedule_filtered": (c_int, [c_int, c_int64, c_int64, c_int, c_int64, C.POINTER(c_int64), c_int, C.POINTER(c_int),
                                                  C.POINTER(c_int64)]),
    "om_debug_search_filter_estimate": (c_int, [c_int, c_int64, c_int, c_int64, C.POINTER(c_int64), C.POINTER(c_int64)]),
    "om_sim_topk_info": (None, [C.POINTER(c_int64)]),
    "om_debug_scan_plan": (c_int, [c_int, c_int64, c_int, C.POINTER(c_int)]),
    "om_debug_scan_round": (c_int, [c_int, c_int64, c_int, c_int64, c_int, C.POINTER(c_int64)]),
    "om_debug_sim_stream": (c_int, [c_void_p, c_int64, C.c_uint32, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "om_debug_scan_kernel": (c_int, [c_int, c_int, c_void_p, c_int64, C.c_uint32, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                     c_int64, c_int, c_void_p]),
    "om_topk_merge": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_int, c_void_p, c_void_p,
                              c_void_p]),
    "om_contrastive_fwd_bwd": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                       c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "om_encoder_train_set_layer_events": (c_int, [c_void_p, c_int]),
    "om_comm_unique_id": (c_int, [c_void_p]),
    "om_comm_init": (c_int, [c_void_p, c_int, c_int, C.POINTER(c_void_p)]),
    "om_comm_destroy": (c_int, [c_void_p]),
    "om_comm_count": (c_int, [c_void_p, C.POINTER(c_int)]),
    "om_allgather_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p]),
    "om_allreduce_grads": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p]),
    "om_exchange_topk": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "om_grad_sqnorm": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "om_adamw_step": (c_int, [c_void_p, c_void_p, c_int, c_float, c_float, c_float, c_float, c_int64, c_void_p, c_float, c_float,
                              c_int, c_void_p, c_void_p]),
    "om_loss_scale_update": (c_int, [c_void_p, c_void_p, c_int, c_void_p]),
    "om_contrastive_fwd_bwd_ex": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p,
                                          c_float, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p]),
}

_lib = None


class NativeError(RuntimeError):
    pass


def lib():
    """The loaded library (loads on first use; raises if it is not there)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NativeError(
                f"{LIB_PATH} is missing: build the HIP library first "
                "(python -m openmatch_amd._build, or __graft_entry__.build()). "
                "openmatch_amd has no CPU / eager fallback.")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:
                raise NativeError(f"{LIB_PATH} does not export {name}; rebuild it") from e
            fn.restype, fn.argtypes = res, args
        if handle.om_abi_version() != ABI_VERSION:
            raise NativeError("libopenmatch_hip.so ABI version mismatch; rebuild it")
        _lib = handle
    return _lib


def exported_symbols():
    return list(_SIGNATURES)


def check(rc):
    if rc != 0:
        raise NativeError(lib().om_last_error().decode("utf-8", "replace"))


def require_device(*tensors):
    """Every tensor must be a contiguous ROCm device tensor; no silent host path."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise NativeError(
                "openmatch_amd runs on MI355X only: got a CPU tensor. Move the model and the batch "
                "to the GPU (model.to('cuda')); there is no CPU / eager fallback.")
        if not t.is_contiguous():
            raise NativeError("non-contiguous tensor passed to the HIP boundary")


def ptr(t):
    return c_void_p(t.data_ptr()) if t is not None else c_void_p(0)


def stream_ptr(device=None):
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Workspace:
    """Grow-only device scratch buffer (256-byte aligned), one per (device, tag)."""
    _pool = {}

    @classmethod
    def get(cls, device, nbytes, tag="default"):
        key = (str(device), tag)
        buf = cls._pool.get(key)
        # the caller gets data_ptr() + off with off up to 255: a buffer is only reused when nbytes fit BEHIND that offset
        if buf is None or buf.numel() - ((-buf.data_ptr()) % 256) < nbytes:
            buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
            cls._pool[key] = buf
        off = (-buf.data_ptr()) % 256
        return buf, buf.data_ptr() + off
