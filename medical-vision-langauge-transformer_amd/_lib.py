"""ctypes binding of the C-ABI in include/mvlt_hip.h (libmvlt_hip.so).

The HIP library is the product: if it is missing this module raises -- there
is no eager/CPU fallback anywhere in the package.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmvlt_hip.so")

F32, BF16 = 0, 1
OK = 0
ABI_VERSION = 17         # == MVLT_ABI_VERSION of the include/mvlt_hip.h these mirrors were written against
ERRORS = {-1: "MVLT_ERR_ARG", -2: "MVLT_ERR_LAUNCH", -3: "MVLT_ERR_UNSUPPORTED"}

EPI_BIAS, EPI_GELU, EPI_SAVE_PRE, EPI_DROPOUT = 1, 2, 4, 8
EPI_ROWSCALE, EPI_RESIDUAL, EPI_ROWMAP, EPI_MUL_GELU_GRAD = 16, 32, 64, 128
EPI_OUT_F32, EPI_ACCUM, EPI_TAIL = 256, 512, 1024
ATTN_SWIN, ATTN_BIDIR, ATTN_SEQ2SEQ = 0, 1, 2
ATTNMAP_HEAD_MEAN, ATTNMAP_RENORM = 1, 2
IMGXF_F32_CHW, IMGXF_U8_HWC = 0, 1
# enum MvltAttnRoute (mvlt_attn_route)
ATTN_ROUTES = ("UNSUPPORTED", "SWIN_FWD", "BERT_FWD_KT5", "BERT_FWD_KT9", "BERT_FWD_KT13", "SWIN_BWD_KS0", "SWIN_BWD_KS3",
               "SWIN_BWD_KS6", "SWIN_BWD_KS12", "SWIN_BWD", "BERT_BWD2_NW5", "BERT_BWD2_NW6", "BERT_BWD_SPLIT_KT5",
               "BERT_BWD_SPLIT_KT9", "BERT_BWD_SPLIT_KT13", "BERT_BWD_KT5", "BERT_BWD_KT9")
# enum MvltGemmRoute (mvlt_gemm_route / mvlt_gemm_group_route): the low 8 bits of the answer, the k-slice count above them
GEMM_ROUTES = ("", "SKINNY") + tuple(f"ROWSTREAM_{i}" for i in range(9)) + (
    "G8_22_NARROW", "G8_22_WIDE", "G8_12_NARROW", "G8_12_WIDE", "GLDS", "REG", "GROUP_GLDS_128x128", "GROUP_GLDS_64x128_S3",
    "GROUP_GLDS_64x128_S2", "GROUP_REG_128x128", "GROUP_REG_64x128", "GROUP_REG_64x96", "GROUP_ATOMIC", "GROUP_G8_22",
    "GROUP_G8_12", "GROUP_G8_11")


def gemm_route_name(r):
    """(name, k-slices) of a non-negative mvlt_gemm_route / mvlt_gemm_group_route answer; a negative one raises."""
    if r < 0:
        raise RuntimeError(f"mvlt_gemm_route: {ERRORS.get(r, r)}")
    return GEMM_ROUTES[r & 255], r >> 8


vp, i32, i64, u64, u32, f32, sz = C.c_void_p, C.c_int, C.c_int64, C.c_uint64, C.c_uint32, C.c_float, C.c_size_t


class MvltGemm(C.Structure):
    _fields_ = [("dtype", i32), ("M", i32), ("N", i32), ("K", i32),
                ("A", vp), ("lda", i64), ("a_kmajor", i32),
                ("B", vp), ("ldb", i64), ("b_kmajor", i32),
                ("C", vp), ("ldc", i64), ("epilogue", i32),
                ("bias", vp), ("pre", vp), ("residual", vp), ("ldr", i64), ("aux", vp),
                ("rowscale", vp), ("rows_per_scale", i32), ("rowmap", vp),
                ("dropout_p", f32), ("seed", u64), ("tag", u32),
                ("split_k", i32), ("workspace", vp), ("workspace_bytes", sz), ("a_colsum", vp), ("event_after_main", vp), ("m_dev", vp),
                ("prefetch", vp), ("prefetch_bytes", i64)]


class MvltLayerNorm(C.Structure):
    _fields_ = [("dtype", i32), ("rows", i32), ("C", i32), ("eps", f32),
                ("x", vp), ("gamma", vp), ("beta", vp),
                ("y", vp), ("y_pre", vp), ("mean", vp), ("rstd", vp),
                ("out_rowmap", vp), ("merge_H", i32), ("merge_W", i32), ("gelu", i32), ("rows_dev", vp)]


class MvltLayerNormBwd(C.Structure):
    _fields_ = [("dtype", i32), ("rows", i32), ("C", i32),
                ("dy", vp), ("dy_rowmap", vp),
                ("x", vp), ("mean", vp), ("rstd", vp), ("gamma", vp),
                ("y_pre", vp), ("gelu", i32),
                ("dres", vp), ("dx", vp),
                ("merge_H", i32), ("merge_W", i32),
                ("dgamma", vp), ("dbeta", vp), ("accumulate", i32),
                ("workspace", vp),
                ("dz", vp), ("dz_rowmap", vp), ("dz_rowscale", vp), ("dz_rows_per_scale", i32),
                ("dz_dropout_p", f32), ("seed", u64), ("tag", u32), ("defer_param_reduce", i32), ("rows_dev", vp),
                ("dy_parts", i32), ("dy_part_stride", i64)]


class MvltLnReduceItem(C.Structure):
    _fields_ = [("workspace", vp), ("nparts", i32), ("C", i32), ("dgamma", vp), ("dbeta", vp)]


class MvltAttn(C.Structure):
    _fields_ = [("dtype", i32), ("mode", i32),
                ("nseq", i32), ("L", i32), ("nH", i32), ("hd", i32),
                ("qkv", vp), ("out", vp), ("lse", vp), ("scale", f32),
                ("bias_table", vp), ("nW", i32), ("win_res", i32), ("shift", i32),
                ("text_ids", vp), ("T", i32), ("image_mask", vp), ("obj_end", i32),
                ("dropout_p", f32), ("seed", u64), ("tag", u32),
                ("dout", vp), ("dqkv", vp), ("dbias_table", vp), ("delta_ws", vp),
                ("row_start", vp), ("seq_len", vp), ("dout_weight", vp), ("prefetch", vp), ("prefetch_bytes", i64)]


class MvltSwinWmsa(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("res", i32), ("C", i32), ("nH", i32), ("shift", i32),
                ("x", vp), ("y", vp), ("w2n", vp),
                ("ln_gamma", vp), ("ln_beta", vp), ("ln_eps", f32),
                ("wqkv", vp), ("bqkv", vp), ("wproj", vp), ("bproj", vp),
                ("bias_table", vp), ("scale", f32), ("rowscale", vp),
                ("xn_win", vp), ("attn_out", vp), ("lse", vp), ("mean", vp), ("rstd", vp),
                ("dy_win", vp), ("dqkv", vp), ("dxn_win", vp), ("qkv_win", vp), ("head_split", i32), ("dbias_ws", vp)]


class MvltSwinDbiasItem(C.Structure):
    _fields_ = [("ws", vp), ("nwg", i32), ("nH", i32), ("dbias_table", vp)]


class MvltEmbed(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("n_img", i32), ("T", i32), ("H", i32),
                ("text_ids", vp), ("image_feature", vp),
                ("word_emb", vp), ("pos_emb", vp), ("type_emb", vp),
                ("cls_id", i32), ("sep_id", i32), ("pos_offset", i32), ("type_override", i32),
                ("out", vp),
                ("dout", vp), ("dimage", vp), ("dword", vp), ("dpos", vp), ("dtype_emb", vp),
                ("row_start", vp), ("seq_len", vp), ("pos_offset_dev", vp), ("pos_rows", i32), ("type_rows", i32)]


class MvltAttnCached(C.Structure):
    _fields_ = [("dtype", i32), ("B", i32), ("nH", i32), ("hd", i32), ("past", i32), ("n_new", i32),
                ("cache_cap", i32),
                ("qkv_new", vp), ("k_cache", vp), ("v_cache", vp), ("out", vp), ("scale", f32), ("past_dev", vp)]


class MvltRange(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("bytes", C.c_int64)]


class MvltZeroItem(C.Structure):
    _fields_ = [("ptr", vp), ("n", i64)]


class MvltMlmMask(C.Structure):
    _fields_ = [("B", i32), ("T", i32), ("vocab_size", i32), ("mask_id", i32),
                ("ids_in", vp), ("full_len", vp), ("itm_label", vp), ("ids_out", vp), ("labels", vp), ("seed", u64)]


class MvltGreedyState(C.Structure):
    _fields_ = [("unfinished", vp), ("eos_id", i64), ("pad_id", i64), ("has_eos", i32),
                ("col", vp), ("past", vp), ("ids", vp), ("ld_ids", i64), ("scores", vp), ("ld_scores", i64),
                ("alive", vp), ("new_ids", vp), ("ld_new", i64), ("ticket", vp)]


class MvltSampleState(C.Structure):
    _fields_ = MvltGreedyState._fields_ + [("seed", vp), ("tag0", u32), ("inv_temperature", f32)]


class MvltSampleFilter(C.Structure):
    _fields_ = [("top_k", i32), ("top_p", f32), ("x", vp), ("ldx", i64), ("row0", u32)]


class MvltBeamCand(C.Structure):
    _fields_ = [("num_beams", i32), ("n_cand", i32), ("beam_scores", vp), ("x", vp), ("ldx", i64),
                ("cand_score", vp), ("cand_beam", vp), ("cand_tok", vp), ("lse", vp)]


class MvltLogitRules(C.Structure):
    _fields_ = [("seen", vp), ("banned", vp), ("ld_words", i64), ("penalty", f32), ("ids", vp), ("ld_ids", i64), ("col", vp),
                ("ngram", i32), ("min_length", i32), ("eos_id", i64), ("has_eos", i32)]


class MvltAttnCachedBeam(C.Structure):
    _fields_ = MvltAttnCached._fields_[:1] + [("rows", i32)] + MvltAttnCached._fields_[2:] + [
        ("num_beams", i32), ("prefix", i32), ("slot", vp), ("ld_slot", i64)]


class MvltBeamStep(C.Structure):
    _fields_ = [("G", i32), ("num_beams", i32), ("n_cand", i32), ("src_beams", i32), ("max_length", i32), ("has_eos", i32),
                ("eos_id", i64), ("pad_id", i64), ("mask_id", i64),
                ("cand_score", vp), ("cand_beam", vp), ("cand_tok", vp), ("hyp_score", vp), ("hyp_len", vp), ("hyp_tokens", vp),
                ("n_hyp", vp), ("worst", vp), ("done", vp), ("seq", vp), ("slot", vp), ("ld_slot", i64),
                ("col", vp), ("past", vp), ("ticket", vp), ("alive", vp), ("beam_scores", vp), ("new_ids", vp), ("beam_idx", vp),
                ("cand_log", vp)]


class MvltHeadCE(C.Structure):
    _fields_ = [("labels", vp), ("lse", vp), ("x_label", vp), ("acc", vp), ("workspace", vp), ("workspace_bytes", sz)]


class MvltRetrievalHead(C.Structure):
    _fields_ = [("dtype", i32), ("P", i32), ("H", i32), ("hidden", vp), ("ld_hidden", i64), ("row_start", vp), ("p_dev", vp),
                ("w_pool", vp), ("b_pool", vp), ("w_tr", vp), ("b_tr", vp), ("ln_gamma", vp), ("ln_beta", vp), ("ln_eps", f32),
                ("w_out", vp), ("b_out", vp), ("out_index", vp), ("scores", vp), ("pooled", vp), ("t1", vp), ("logits", vp)]


# every symbol include/mvlt_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mvlt_version": (i32, []),
    "mvlt_arch": (C.c_char_p, []),
    "mvlt_sizeof": (sz, [i32]),
    "mvlt_gemm": (i32, [C.POINTER(MvltGemm), vp]),
    "mvlt_gemm_workspace_bytes": (sz, [C.POINTER(MvltGemm)]),
    "mvlt_gemm_plan": (i32, [C.POINTER(MvltGemm), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
    "mvlt_gemm_route": (i32, [C.POINTER(MvltGemm)]),
    "mvlt_gemm_group_route": (i32, [C.POINTER(MvltGemm), i32]),
    "mvlt_gemm_group": (i32, [C.POINTER(MvltGemm), i32, vp]),
    "mvlt_gemm_group_workspace_bytes": (sz, [C.POINTER(MvltGemm), i32]),
    "mvlt_gemm_argmax": (i32, [C.POINTER(MvltGemm), vp, vp, vp, vp, vp]),
    "mvlt_gemm_argmax_greedy": (i32, [C.POINTER(MvltGemm), vp, vp, C.POINTER(MvltGreedyState), vp]),
    "mvlt_gemm_sample": (i32, [C.POINTER(MvltGemm), vp, vp, vp, vp, u64, u32, f32, vp]),
    "mvlt_gemm_sample_step": (i32, [C.POINTER(MvltGemm), vp, vp, C.POINTER(MvltSampleState), vp]),
    "mvlt_gemm_sample_filtered": (i32, [C.POINTER(MvltGemm), vp, vp, C.POINTER(MvltSampleFilter), vp, vp, u64, u32, f32, vp]),
    "mvlt_gemm_sample_filtered_step": (i32, [C.POINTER(MvltGemm), vp, vp, C.POINTER(MvltSampleFilter), C.POINTER(MvltSampleState), vp]),
    "mvlt_decode_rules_plan": (i32, [C.POINTER(MvltLogitRules), i32, i32, vp]),
    "mvlt_gemm_argmax_rules": (i32, [C.POINTER(MvltGemm), vp, vp, vp, vp, C.POINTER(MvltLogitRules), vp]),
    "mvlt_gemm_argmax_greedy_rules": (i32, [C.POINTER(MvltGemm), vp, vp, C.POINTER(MvltGreedyState), C.POINTER(MvltLogitRules), vp]),
    "mvlt_gemm_pick_rows": (i32, [C.POINTER(MvltGemm), vp, vp, vp, vp, vp, vp, u64, u32, vp]),
    "mvlt_gemm_pick_rows_rules": (i32, [C.POINTER(MvltGemm), vp, vp, vp, vp, vp, vp, u64, u32, C.POINTER(MvltLogitRules), vp]),
    "mvlt_gemm_pick_rows_step": (i32, [C.POINTER(MvltGemm), vp, vp, vp, vp, C.POINTER(MvltSampleState), vp]),
    "mvlt_gemm_pick_rows_step_rules": (i32, [C.POINTER(MvltGemm), vp, vp, vp, vp, C.POINTER(MvltSampleState), C.POINTER(MvltLogitRules), vp]),
    "mvlt_gemm_sample_rules": (i32, [C.POINTER(MvltGemm), vp, vp, vp, vp, u64, u32, f32, C.POINTER(MvltLogitRules), vp]),
    "mvlt_gemm_sample_step_rules": (i32, [C.POINTER(MvltGemm), vp, vp, C.POINTER(MvltSampleState), C.POINTER(MvltLogitRules), vp]),
    "mvlt_gemm_sample_filtered_rules": (i32, [C.POINTER(MvltGemm), vp, vp, C.POINTER(MvltSampleFilter), vp, vp, u64, u32, f32,
                                            C.POINTER(MvltLogitRules), vp]),
    "mvlt_gemm_sample_filtered_step_rules": (i32, [C.POINTER(MvltGemm), vp, vp, C.POINTER(MvltSampleFilter), C.POINTER(MvltSampleState),
                                                 C.POINTER(MvltLogitRules), vp]),
    "mvlt_gemm_beam_candidates": (i32, [C.POINTER(MvltGemm), C.POINTER(MvltBeamCand), vp]),
    "mvlt_beam_rules_plan": (i32, [C.POINTER(MvltLogitRules), vp, i64, i32, i32, vp]),
    "mvlt_gemm_beam_candidates_rules": (i32, [C.POINTER(MvltGemm), C.POINTER(MvltBeamCand), C.POINTER(MvltLogitRules), vp]),
    "mvlt_mlm_head_ce": (i32, [C.POINTER(MvltGemm), C.POINTER(MvltHeadCE), vp]),
    "mvlt_mlm_head_ce_workspace_bytes": (sz, [i32, i32]),
    "mvlt_retrieval_head_supported": (i32, [i32, i32]),
    "mvlt_retrieval_head": (i32, [C.POINTER(MvltRetrievalHead), vp]),
    "mvlt_recall_ranks": (i32, [vp, i64, i32, i32, vp, vp, vp, vp, vp]),
    "mvlt_recall_counts": (i32, [vp, i32, C.POINTER(i32), i32, vp, vp]),
    "mvlt_report_ngram_keys": (i32, [vp, i64, i32, i32, vp, i32, C.POINTER(i64), i32, vp, vp, vp]),
    "mvlt_report_stats": (i32, [vp, i64, i32, i32, vp, i64, i32, i32, vp, vp, i32, C.POINTER(i64), i32, vp, vp, i32, vp, vp, vp]),
    "mvlt_gemm_skinny_accum": (i32, [C.POINTER(MvltGemm), vp, i32, vp]),
    "mvlt_layernorm_acc_fwd": (i32, [i32, vp, i32, vp, vp, vp, vp, f32, i32, i32, vp, vp]),
    "mvlt_colsum": (i32, [i32, vp, i64, i32, i32, vp, i32, vp, vp]),
    "mvlt_colsum_workspace_rows": (i32, [i32]),
    "mvlt_layernorm_fwd": (i32, [C.POINTER(MvltLayerNorm), vp]),
    "mvlt_layernorm_bwd": (i32, [C.POINTER(MvltLayerNormBwd), vp]),
    "mvlt_layernorm_bwd_workspace_rows": (i32, []),
    "mvlt_layernorm_bwd_nparts": (i32, [i32, i32]),
    "mvlt_layernorm_param_reduce_batch": (i32, [C.POINTER(MvltLnReduceItem), i32, vp]),
    "mvlt_attn_fwd": (i32, [C.POINTER(MvltAttn), vp]),
    "mvlt_attn_bwd": (i32, [C.POINTER(MvltAttn), vp]),
    "mvlt_attn_bwd_ev": (i32, [C.POINTER(MvltAttn), vp, vp]),
    "mvlt_attn_route": (i32, [C.POINTER(MvltAttn), i32]),
    "mvlt_swin_bwd_proj_supported": (i32, [i32, i32, i32, i32, i32]),
    "mvlt_attn_probs": (i32, [C.POINTER(MvltAttn), i32, i32, i32, i32, i32, vp, vp]),
    "mvlt_swin_wmsa_supported": (i32, [i32, i32, i32]),
    "mvlt_swin_wmsa_fwd": (i32, [C.POINTER(MvltSwinWmsa), vp]),
    "mvlt_swin_wmsa2_supported": (i32, [i32, i32, i32, i32, i32]),
    "mvlt_swin_wmsa2_sync_words": (i32, [i32, i32]),
    "mvlt_swin_wmsa2_fwd": (i32, [C.POINTER(MvltSwinWmsa), vp, vp]),
    "mvlt_swin_wmsa2_bwd_parts": (i32, [i32, i32, i32, i32, i32]),
    "mvlt_swin_wmsa2_bwd_workgroups": (i32, [i32, i32, i32, i32, i32]),
    "mvlt_swin_wmsa2_bwd_dbias": (i32, [C.POINTER(MvltSwinDbiasItem), i32, vp]),
    "mvlt_swin_wmsa2_bwd": (i32, [C.POINTER(MvltSwinWmsa), vp]),
    "mvlt_swin_wmsa2_bwd_ev": (i32, [C.POINTER(MvltSwinWmsa), vp, vp]),
    "mvlt_swin_wmsa2_set_timeout_ms": (i32, [i32]),
    "mvlt_debug_hold_cus": (i32, [i32, i32, i32, vp]),
    "mvlt_debug_stream_copy": (i32, [vp, vp, i64, i32, i32, vp]),
    "mvlt_im2col_patch": (i32, [i32, vp, vp, i32, i32, i32, i32, vp]),
    "mvlt_pack_plan": (i32, [vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]),
    "mvlt_label_plan": (i32, [vp, vp, i32, vp, vp, vp, vp]),
    "mvlt_rows_scatter": (i32, [i32, vp, vp, i32, i32, vp, vp, vp]),
    "mvlt_embed_fwd": (i32, [C.POINTER(MvltEmbed), vp]),
    "mvlt_embed_fwd_rows": (i32, [C.POINTER(MvltEmbed), vp, vp]),
    "mvlt_embed_bwd": (i32, [C.POINTER(MvltEmbed), vp]),
    "mvlt_rows_transform": (i32, [i32, vp, vp, i32, i32, vp, vp, i32, f32, u64, u32, vp]),
    "mvlt_cast": (i32, [i32, vp, i32, vp, i64, vp]),
    "mvlt_gelu_fwd": (i32, [i32, vp, vp, i64, vp]),
    "mvlt_tanh_fwd": (i32, [i32, vp, vp, i64, vp]),
    "mvlt_tanh_bwd": (i32, [i32, vp, vp, vp, i64, vp]),
    "mvlt_dropout_mask": (i32, [vp, i64, f32, u64, u32, vp]),
    "mvlt_gumbel_noise": (i32, [u64, u32, i32, i32, vp, vp]),
    "mvlt_droppath_scale": (i32, [vp, i32, f32, u64, u32, vp]),
    "mvlt_droppath_scales": (i32, [vp, vp, i32, i32, u64, u32, vp]),
    "mvlt_droppath_plan": (i32, [vp, i32, i32, vp, i32, i32, i64, vp, vp, vp, vp]),
    "mvlt_ce_fwd": (i32, [i32, vp, i64, i32, i32, vp, vp, vp, vp, vp]),
    "mvlt_ce_bwd": (i32, [i32, vp, i64, i32, i32, vp, vp, vp, f32, vp, vp, vp]),
    "mvlt_ce_fwd_ragged": (i32, [i32, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp]),
    "mvlt_ce_bwd_ragged": (i32, [i32, vp, i64, i32, i32, vp, vp, vp, f32, vp, vp, vp, vp]),
    "mvlt_seq_loss_plan": (i32, [vp, i64, i32, i32, i64, vp, i64, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp]),
    "mvlt_seq_loss_fwd": (i32, [vp, vp, vp, i32, vp, vp, vp]),
    "mvlt_ce_bwd_weighted": (i32, [i32, vp, i64, i32, i32, vp, vp, vp, vp, f32, vp, vp, vp, vp]),
    "mvlt_gelu_bwd": (i32, [i32, vp, vp, vp, i64, vp]),
    "mvlt_softmax_rows": (i32, [i32, vp, i64, i32, i32, vp, vp]),
    "mvlt_adamw": (i32, [vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, f32, vp]),
    "mvlt_adamw_guarded": (i32, [vp, vp, vp, vp, vp, i64, f32, f32, f32, f32, f32, i32, f32, vp, vp, vp]),
    "mvlt_adamw_groups_block": (i32, []),
    "mvlt_adamw_groups": (i32, [vp, vp, vp, vp, vp, i64, vp, vp, vp, i32, f32, f32, f32, f32, i32, f32, vp, vp, vp]),
    "mvlt_grad_sumsq_parts": (i32, []),
    "mvlt_grad_sumsq": (i32, [vp, i64, vp, i32, vp]),
    "mvlt_grad_norm_finish": (i32, [vp, i32, f32, f32, i32, vp, vp, vp]),
    "mvlt_attn_cached": (i32, [C.POINTER(MvltAttnCached), vp]),
    "mvlt_attn_cached_rows": (i32, [C.POINTER(MvltAttnCached), vp, vp]),
    "mvlt_attn_cached_beam": (i32, [C.POINTER(MvltAttnCachedBeam), vp]),
    "mvlt_beam_step": (i32, [C.POINTER(MvltBeamStep), vp]),
    "mvlt_argmax": (i32, [i32, vp, i64, i32, i32, vp, vp]),
    "mvlt_zero_batch": (i32, [C.POINTER(MvltZeroItem), i32, vp]),
    "mvlt_prefetch": (i32, [C.POINTER(MvltRange), i32, vp]),
    "mvlt_image_normalize": (i32, [vp, vp, i32, i32, i32, vp]),
    "mvlt_mlm_mask": (i32, [C.POINTER(MvltMlmMask), vp]),
    "mvlt_image_transform": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp]),
}

# ctypes mirror of every struct, in the order of the MVLT_STRUCT_* ids of the header
STRUCTS = [MvltGemm, MvltLayerNorm, MvltLayerNormBwd, MvltLnReduceItem, MvltAttn, MvltSwinWmsa, MvltEmbed,
           MvltAttnCached, MvltZeroItem, MvltRange, MvltMlmMask, MvltGreedyState, MvltSwinDbiasItem,
           MvltSampleState, MvltSampleFilter, MvltBeamCand, MvltAttnCachedBeam, MvltHeadCE, MvltRetrievalHead, MvltBeamStep,
           MvltLogitRules]

_lib = None


def lib():
    """Load libmvlt_hip.so (built by __graft_entry__.build() / csrc/Makefile)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP kernels first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C medical-vision-langauge-transformer_amd/csrc). There is no fallback path.")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        if L.mvlt_version() != ABI_VERSION or L.mvlt_arch() != b"gfx950":
            raise RuntimeError(f"libmvlt_hip.so reports ABI {L.mvlt_version()} / arch {L.mvlt_arch()!r}; this binding "
                               f"was written for ABI {ABI_VERSION} / gfx950: rebuild (make -C .../csrc)")
        for sid, st in enumerate(STRUCTS):
            if L.mvlt_sizeof(sid) != C.sizeof(st):
                raise RuntimeError(f"{st.__name__}: the library was compiled with {L.mvlt_sizeof(sid)} bytes, the "
                                   f"ctypes mirror has {C.sizeof(st)}: stale libmvlt_hip.so or stale _lib.py")
        _lib = L
    return _lib


def check(rc, what):
    if rc != OK:
        raise RuntimeError(f"{what} failed: {ERRORS.get(rc, rc)}")
