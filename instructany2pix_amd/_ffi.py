"""ctypes binding of libia2p_hip.so (C ABI declared in include/ia2p.h; test hooks and the profile interface in include/ia2p_debug.h).

The product path has no CPU fallback: if the library is missing this module raises at import of the
symbols, and every compute entry point needs device pointers on an MI355X.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libia2p_hip.so")

IA2P_OK = 0
_STATUS_NAMES = {1: "INVALID", 2: "SHAPE", 3: "KEY", 4: "STATE", 5: "NOMEM", 6: "HIP", 7: "ARCH"}
MAX_BLOCKS = 4


class UNetConfigC(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int), ("out_channels", C.c_int), ("n_blocks", C.c_int),
        ("block_out_channels", C.c_int * MAX_BLOCKS), ("transformer_layers_per_block", C.c_int * MAX_BLOCKS),
        ("num_heads", C.c_int * MAX_BLOCKS), ("layers_per_block", C.c_int), ("cross_attention_dim", C.c_int),
        ("norm_num_groups", C.c_int), ("norm_eps", C.c_float), ("addition_time_embed_dim", C.c_int),
        ("projection_class_embeddings_input_dim", C.c_int), ("time_embed_dim", C.c_int), ("time_proj_dim", C.c_int),
        ("mid_transformer_layers", C.c_int), ("num_time_ids", C.c_int),
    ]


class ControlNetConfigC(C.Structure):
    """ia2p_controlnet_config (include/ia2p.h): the UNet config plus the condition embedding's widths"""
    _fields_ = [("unet", UNetConfigC), ("conditioning_channels", C.c_int), ("conditioning_embedding_out_channels", C.c_int * 4)]


class LnFoldC(C.Structure):
    _fields_ = [("stats", C.c_void_p), ("slots", C.c_int), ("colsum", C.c_void_p), ("fbias", C.c_void_p), ("eps", C.c_float)]


class CLIPConfigC(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int), ("intermediate_size", C.c_int),
                ("max_positions", C.c_int), ("projection_dim", C.c_int), ("hidden_act", C.c_int), ("eos_token_id", C.c_int), ("layer_norm_eps", C.c_float)]


class ViTConfigC(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int), ("intermediate_size", C.c_int), ("in_channels", C.c_int),
                ("image_h", C.c_int), ("image_w", C.c_int), ("patch_size", C.c_int), ("patch_stride", C.c_int), ("pre_ln", C.c_int), ("stem_ln", C.c_int),
                ("bias_kv", C.c_int), ("out_dim", C.c_int), ("layer_norm_eps", C.c_float)]


class SAMConfigC(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int), ("mlp_dim", C.c_int), ("image_size", C.c_int), ("patch_size", C.c_int),
                ("window_size", C.c_int), ("num_global", C.c_int), ("global_attn_indexes", C.c_int * 8), ("output_channels", C.c_int), ("dec_hidden", C.c_int),
                ("dec_layers", C.c_int), ("dec_heads", C.c_int), ("dec_mlp_dim", C.c_int), ("dec_downsample_rate", C.c_int), ("layer_norm_eps", C.c_float)]


class LLMConfigC(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("hidden_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int), ("num_kv_heads", C.c_int),
                ("intermediate_size", C.c_int), ("rms_norm_eps", C.c_float), ("rope_theta", C.c_float)]


class VAEConfigC(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("latent_channels", C.c_int), ("n_blocks", C.c_int),
                ("block_out_channels", C.c_int * MAX_BLOCKS), ("layers_per_block", C.c_int), ("norm_num_groups", C.c_int),
                ("norm_eps", C.c_float), ("stream_scale", C.c_float)]


class ConvGnC(C.Structure):
    """ia2p_conv_gn (include/ia2p.h): a 3x3 convolution with the GroupNorm + SiLU in front of it applied inside the kernel"""
    _fields_ = [("x0", C.c_void_p), ("C0", C.c_int), ("st0", C.c_void_p), ("rows0", C.c_int),
                ("x1", C.c_void_p), ("C1", C.c_int), ("st1", C.c_void_p), ("rows1", C.c_int),
                ("gamma", C.c_void_p), ("beta", C.c_void_p), ("groups", C.c_int), ("eps", C.c_float),
                ("Wp", C.c_void_p), ("bias", C.c_void_p), ("rowvec", C.c_void_p), ("residual", C.c_void_p), ("y", C.c_void_p),
                ("B", C.c_int), ("H", C.c_int), ("W", C.c_int), ("Co", C.c_int),
                ("xa", C.c_void_p), ("Ca", C.c_int), ("splitk", C.c_int), ("partial", C.c_void_p), ("gn_out", C.c_void_p)]


_P, _I, _F, _SZ, _I64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_int64


class GemmFormC(C.Structure):
    """ia2p_gemm_form (include/ia2p.h): a GEMM launch with every option of its descriptor (strides, row map, activation, epilogue scales, folded LayerNorm)"""
    _fields_ = [("A", _P), ("lda", _I), ("W", _P), ("ldw", _I), ("bias", _P), ("residual", _P), ("ldr", _I), ("C", _P), ("ldc", _I), ("M", _I), ("N", _I), ("K", _I),
                ("rpb", _I), ("bstride", _I), ("roff", _I), ("act", _I), ("acc_scale", _F), ("bias_scale", _F),
                ("rowvec", _P), ("rowvec_ld", _I), ("rows_per_batch", _I), ("ln", _P), ("stats_out", _P), ("stats_slots", _P), ("splitk", _I), ("partial", _P)]


class ConvFormC(C.Structure):
    """ia2p_conv_form (include/ia2p.h): ia2p_conv3x3 plus pad_lo, the epilogue scales and the K split"""
    _fields_ = [("x", _P), ("Wp", _P), ("bias", _P), ("rowvec", _P), ("residual", _P), ("y", _P),
                ("B", _I), ("Hs", _I), ("Ws", _I), ("Cin", _I), ("Co", _I), ("stride", _I), ("up", _I), ("pad_lo", _I),
                ("acc_scale", _F), ("bias_scale", _F), ("splitk", _I), ("partial", _P)]


class UNetCallC(C.Structure):
    """ia2p_unet_call (include/ia2p.h): one UNet evaluation as a record; which fields may meet is the table there"""
    _fields_ = [("struct_size", C.c_uint32), ("B", _I), ("h", _I), ("w", _I), ("L", _I), ("G", _I), ("n_down", _I), ("timestep", _F),
                ("sample", _P), ("context", _P), ("kv", _P), ("text_embeds", _P), ("time_ids", _P), ("out", _P), ("timesteps", _P), ("ip_scales", _P),
                ("region_masks", _P), ("down_residuals", C.POINTER(_P)), ("mid_residual", _P)]


# every symbol include/ia2p.h and include/ia2p_debug.h declare: name -> (restype, argtypes)
SIGNATURES = {
    "ia2p_create": (_I, [C.POINTER(UNetConfigC), C.POINTER(_P)]),
    "ia2p_destroy": (None, [_P]),
    "ia2p_last_error": (C.c_char_p, [_P]),
    "ia2p_device_is_gfx950": (_I, []),
    "ia2p_arena_bytes": (_SZ, [_P]),
    "ia2p_bind_arena": (_I, [_P, _P, _SZ]),
    "ia2p_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _P]),
    "ia2p_read_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _P]),
    "ia2p_finalize_weights": (_I, [_P]),
    "ia2p_adopt_arena": (_I, [_P, _I]),
    "ia2p_adopt_arena_on": (_I, [_P, _I, _P]),
    "ia2p_arena_raw_bytes": (_SZ, [_P]),
    "ia2p_bcast_arena": (_I, [_P, _P, _I, _I, _P]),
    "ia2p_rccl_available": (_I, []),
    "ia2p_set_ip_adapter": (_I, [_P, _I, _I, _F]),
    "ia2p_workspace_bytes_x": (_SZ, [_P, C.POINTER(UNetCallC)]),
    "ia2p_unet_forward_x": (_I, [_P, _P, C.POINTER(UNetCallC), _P, _SZ]),
    "ia2p_workspace_bytes": (_SZ, [_P, _I, _I, _I, _I]),
    "ia2p_unet_forward": (_I, [_P, _P, _P, _F, _P, _I, _P, _P, _P, _I, _I, _I, _P, _SZ]),
    "ia2p_unet_forward_v": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _P, _SZ]),
    "ia2p_workspace_bytes_r": (_SZ, [_P, _I, _I, _I, _I, _I]),
    "ia2p_unet_forward_r": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _P, _SZ, _P, _I]),
    "ia2p_workspace_bytes_c": (_SZ, [_P, _I, _I, _I, _I]),
    "ia2p_unet_num_skips": (_I, [_P]),
    "ia2p_unet_forward_c": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _I, _I, _I, _P, _SZ, C.POINTER(_P), _I, _P, _P, _I]),
    "ia2p_controlnet_create": (_I, [C.POINTER(ControlNetConfigC), C.POINTER(_P)]),
    "ia2p_controlnet_destroy": (None, [_P]),
    "ia2p_controlnet_last_error": (C.c_char_p, [_P]),
    "ia2p_controlnet_arena_bytes": (_SZ, [_P]),
    "ia2p_controlnet_bind_arena": (_I, [_P, _P, _SZ]),
    "ia2p_controlnet_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _P]),
    "ia2p_controlnet_finalize_weights": (_I, [_P]),
    "ia2p_controlnet_set_image_tokens": (_I, [_P, _I]),
    "ia2p_controlnet_check_unet": (_I, [_P, _P]),
    "ia2p_controlnet_num_residuals": (_I, [_P]),
    "ia2p_controlnet_residual_layout": (_SZ, [_P, _I, _I, _I, C.POINTER(_I64), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "ia2p_controlnet_embed_bytes": (_SZ, [_P, _I, _I, _I]),
    "ia2p_controlnet_embed_workspace_bytes": (_SZ, [_P, _I, _I, _I]),
    "ia2p_controlnet_embed": (_I, [_P, _P, _P, _I, _I, _I, _P, _SZ, _P, _SZ]),
    "ia2p_controlnet_workspace_bytes": (_SZ, [_P, _I, _I, _I, _I]),
    "ia2p_controlnet_context_kv_bytes": (_SZ, [_P, _I, _I]),
    "ia2p_controlnet_project_context": (_I, [_P, _P, _P, _I, _I, _P, _SZ, _P, _SZ]),
    "ia2p_controlnet_forward": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _SZ, _I, _I, _I, _P, _SZ]),
    "ia2p_conv_in_act": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I]),
    "ia2p_conv3x3_narrow": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I]),
    "ia2p_gemm_rowscale": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_residual_add_gnstats": (_I, [_P, _P, _P, _P, _I, _I, _I, _P]),
    "ia2p_context_kv_bytes": (_SZ, [_P, _I, _I]),
    "ia2p_project_context": (_I, [_P, _P, _P, _I, _I, _P, _SZ, _P, _SZ]),
    "ia2p_unet_forward_kv": (_I, [_P, _P, _P, _F, _P, _I, _P, _P, _P, _I, _I, _I, _P, _SZ]),
    "ia2p_autotune": (_I, [_P, _P, _P, _F, _P, _I, _P, _P, _P, _I, _I, _I, _P, _SZ, _I, _P]),
    "ia2p_plan_export": (_SZ, [_P, _SZ]),
    "ia2p_plan_import": (_I, [C.c_char_p]),
    "ia2p_plan_clear": (None, []),
    "ia2p_plan_generation": (C.c_ulonglong, []),
    "ia2p_ddim_step": (_I, [_P, _P, _P, _P, _F, _F, _F, _P, _P, _I64]),
    "ia2p_ddim_step_v": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I64]),
    "ia2p_mask_blend": (_I, [_P, _P, _P, _P, _P, _F, _F, _P, _P, _I, _I, _I64]),
    "ia2p_mask_blend_v": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I64]),
    "ia2p_known_blend_v": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I64, _I]),
    "ia2p_mask_to_latent": (_I, [_P, _P, _P, _I, _I, _I, _I]),
    "ia2p_mask_feather_u8": (_I, [_P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_image_composite_u8": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_randn_seeded": (_I, [_P, _P, _I, _I, _I64, _I64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "ia2p_lcm_step_v": (_I, [_P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int64), _P, _P, _I, _I64]),
    "ia2p_posterior_sample_seeded": (_I, [_P, _P, _P, _I, _I, _I64, _F, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "ia2p_polar_mix_v": (_I, [_P, _P, _P, C.POINTER(_F), _P, _I, _I64]),
    "ia2p_eps_contrast_map": (_I, [_P, _P, _P, _P, _I, _I, _I, _I64]),
    "ia2p_contrast_mask": (_I, [_P, _P, C.POINTER(_F), C.POINTER(C.c_int), _P, _P, _I, _I, _I]),
    "ia2p_groupnorm_silu": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _P]),
    "ia2p_layernorm": (_I, [_P, _P, _P, _P, _P, _I, _I, _F]),
    "ia2p_gemm": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_gemm_splitk": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P]),
    "ia2p_ffn": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P]),
    "ia2p_fold_layernorm": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I]),
    "ia2p_gemm_ex": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "ia2p_gemm_form": (_I, [_P, C.POINTER(GemmFormC)]),
    "ia2p_conv3x3_form": (_I, [_P, C.POINTER(ConvFormC)]),
    "ia2p_debug_set_gemm_splitk": (None, [_I]),
    "ia2p_conv3x3": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I]),
    "ia2p_conv3x3_splitk": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "ia2p_pack_conv3x3": (_I, [_P, _P, _P, _I, _I]),
    "ia2p_pack_conv_out": (_I, [_P, _P, _P, _I, _I]),
    "ia2p_conv3x3_cat": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I]),
    "ia2p_pack_geglu": (_I, [_P, _P, _P, _I, _I]),
    "ia2p_conv_in": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_conv_out": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_attention": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _F, _P, _P, _I, _I, _F]),
    "ia2p_attention_regions": (_I, [_P, _P, _I, _P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _F, _P, _P, _I, _I, _F, _P, _I, _P]),
    "ia2p_region_levels": (_I, [_P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_qkv_self_attention": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_qkv_self_attention_ctx": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _I, _I, _P]),
    "ia2p_qproj_attention": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I, _I, _F, _P, _P, _I, _I, _F]),
    "ia2p_linear_small": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_ip_attn_map": (_I, [_P, _P, _I, _P, _I, _P, _I, _I, _I, _I]),
    "ia2p_debug_set_gemm_tile": (None, [_I]),
    "ia2p_debug_gemm_tile_info": (_I, [_I, _P]),
    "ia2p_debug_set_xattn_min_tiles": (None, [_I]),
    "ia2p_debug_set_attn_fold": (None, [_I]),
    "ia2p_debug_set_splitk_inkernel": (None, [C.c_longlong]),
    "ia2p_debug_invalidate_splitk_counters": (None, []),
    "ia2p_debug_fill_splitk_counters": (_I, [_P, _I]),
    "ia2p_debug_gemm_plan": (None, [_I, _I, _I, _I, _I, _P, _P]),
    "ia2p_clip_create": (_I, [C.POINTER(CLIPConfigC), C.POINTER(_P)]),
    "ia2p_clip_destroy": (None, [_P]),
    "ia2p_clip_last_error": (C.c_char_p, [_P]),
    "ia2p_clip_arena_bytes": (_SZ, [_P]),
    "ia2p_clip_bind_arena": (_I, [_P, _P, _SZ]),
    "ia2p_clip_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I, _P]),
    "ia2p_clip_finalize_weights": (_I, [_P]),
    "ia2p_clip_workspace_bytes": (_SZ, [_P, _I, _I]),
    "ia2p_clip_encode": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P, _SZ]),
    "ia2p_clip_encode_embeds": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _SZ]),
    "ia2p_vit_create": (_I, [C.POINTER(ViTConfigC), C.POINTER(_P)]),
    "ia2p_vit_destroy": (None, [_P]),
    "ia2p_vit_last_error": (C.c_char_p, [_P]),
    "ia2p_vit_arena_bytes": (_SZ, [_P]),
    "ia2p_vit_tokens": (_I, [_P]),
    "ia2p_vit_bind_arena": (_I, [_P, _P, _SZ]),
    "ia2p_vit_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I, _P]),
    "ia2p_vit_finalize_weights": (_I, [_P]),
    "ia2p_vit_workspace_bytes": (_SZ, [_P, _I]),
    "ia2p_vit_encode": (_I, [_P, _P, _P, _I, _P, _P, _P, _SZ]),
    "ia2p_attention_full": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_sam_create": (_I, [C.POINTER(SAMConfigC), C.POINTER(_P)]),
    "ia2p_sam_destroy": (None, [_P]),
    "ia2p_sam_last_error": (C.c_char_p, [_P]),
    "ia2p_sam_arena_bytes": (_SZ, [_P]),
    "ia2p_sam_bind_arena": (_I, [_P, _P, _SZ]),
    "ia2p_sam_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I, _P]),
    "ia2p_sam_finalize_weights": (_I, [_P]),
    "ia2p_sam_workspace_bytes": (_SZ, [_P, _I, _I]),
    "ia2p_sam_encode_image": (_I, [_P, _P, _P, _I, _P, _P, _SZ]),
    "ia2p_sam_predict_boxes": (_I, [_P, _P, _P, C.POINTER(_F), _I, _P, _P, _P, _SZ]),
    "ia2p_attention_window_relpos": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I]),
    "ia2p_attention_global_relpos": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_attention_small_head": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_mask_upsample_threshold": (_I, [_P, _P, _I, _I, _I, _I, _I64, _I, _I, _F, _P, _P]),
    "ia2p_mask_morph": (_I, [_P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_prior_step": (_I, [_P, _P, _P, _P, _P, _F, _F, _F, _F, _F, _F, _P, _I64]),
    "ia2p_llm_create": (_I, [C.POINTER(LLMConfigC), C.POINTER(_P)]),
    "ia2p_llm_destroy": (None, [_P]),
    "ia2p_llm_last_error": (C.c_char_p, [_P]),
    "ia2p_llm_arena_bytes": (_SZ, [_P]),
    "ia2p_llm_bind_arena": (_I, [_P, _P, _SZ]),
    "ia2p_llm_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _I, _P]),
    "ia2p_llm_finalize_weights": (_I, [_P]),
    "ia2p_llm_kv_bytes": (_SZ, [_P, _I]),
    "ia2p_llm_bind_kv": (_I, [_P, _P, _SZ, _I]),
    "ia2p_llm_workspace_bytes": (_SZ, [_P, _I]),
    "ia2p_llm_reset": (_I, [_P]),
    "ia2p_llm_position": (_I, [_P]),
    "ia2p_llm_embed": (_I, [_P, _P, _P, _I, _P]),
    "ia2p_llm_prefill": (_I, [_P, _P, _P, _I, _P, _P, _P, _SZ]),
    "ia2p_llm_decode": (_I, [_P, _P, _I, _P, _P, _P, _SZ]),
    "ia2p_llm_gemv": (_I, [_P, _P, _P, _P, _I, _I]),
    "ia2p_llm_set_weight_format": (_I, [_P, _I, C.POINTER(_F)]),
    "ia2p_llm_weight_bits": (_I, [_P]),
    "ia2p_llm_q4_packed_bytes": (_SZ, [_I64, _I64]),
    "ia2p_llm_quantize_q4": (_I, [_P, _P, _I64, _I64, C.POINTER(_F), _P, _P]),
    "ia2p_llm_dequantize_q4": (_I, [_P, _P, _P, _I64, _I64, C.POINTER(_F), _P]),
    "ia2p_llm_gemv_q4": (_I, [_P, _P, _P, C.POINTER(_F), _P, _P, _I, _I]),
    "ia2p_llm_kv_slots_bytes": (_SZ, [_P, _I, _I]),
    "ia2p_llm_bind_kv_slots": (_I, [_P, _P, _SZ, _I, _I]),
    "ia2p_llm_slots": (_I, [_P]),
    "ia2p_llm_reset_slot": (_I, [_P, _I]),
    "ia2p_llm_slot_position": (_I, [_P, _I]),
    "ia2p_llm_prefill_slot": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _SZ]),
    "ia2p_llm_decode_batch": (_I, [_P, _P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _I, _P, _P, _P, _SZ]),
    "ia2p_llm_decode_batch_dev": (_I, [_P, _P, C.POINTER(C.c_int32), _P, C.POINTER(C.c_int32), _I, _P, _P, _P, _SZ]),
    "ia2p_sample_tokens": (_I, [_P, _P, _I64, _I, _I, _F, _I, _I, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), _P, _P, _P]),
    "ia2p_sample_tokens_p": (_I, [_P, _P, _I64, _I, _I, _F, _I, _F, _I, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), _P, _P, _P]),
    "ia2p_llm_batch_workspace_bytes": (_SZ, [_P, _I, _I]),
    "ia2p_llm_gemv_rows": (_I, [_P, _P, _P, _P, _I, _I, _I]),
    "ia2p_llm_gemv_q4_rows": (_I, [_P, _P, _P, C.POINTER(_F), _P, _P, _I, _I, _I]),
    "ia2p_llm_gemv_epi": (_I, [_P, _P, _P, C.POINTER(_F), _P, _P, _F, _I, _P, _P, _I, _I, _I]),
    "ia2p_llm_gemv_qkv": (_I, [_P, _P, _P, C.POINTER(_F), _P, _P, _F, _P, C.POINTER(C.c_int32), _P, C.POINTER(_P), C.POINTER(_P), _I, _I, _I]),
    "ia2p_llm_attention_rows": (_I, [_P, _P, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32), _P, _I, _I, _I]),
    "ia2p_llm_attention_prefill": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_llm_rmsnorm_rows": (_I, [_P, _P, _P, _F, _P, _I, _I]),
    "ia2p_llm_rope_cache_rows": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I]),
    "ia2p_llm_silu_mul_rows": (_I, [_P, _P, _P, _I, _I]),
    "ia2p_llm_rope_inv_freq": (_I, [_F, C.POINTER(_F)]),
    "ia2p_gelu": (_I, [_P, _P, _I64]),
    "ia2p_clip_embed": (_I, [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I]),
    "ia2p_causal_attention_small": (_I, [_P, _P, _P, _I, _I, _I, _I]),
    "ia2p_clip_pool": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _F]),
    "ia2p_softmax_rows": (_I, [_P, _P, _I64, _I, _I, _F]),
    "ia2p_conv1x1_nchw": (_I, [_P, _P, _P, _P, _P, _I, _I, _I, _I64]),
    "ia2p_patch_gather": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I]),
    "ia2p_vit_embed": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F]),
    "ia2p_vit_project": (_I, [_P, _P, _P, _P, _I, _I, _I]),
    "ia2p_embed": (_I, [_P, _F, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_concat": (_I, [_P, _P, _I, _I, _P, _I, _I, _P, _I64]),
    "ia2p_cat_rows": (_I, [_P, _P, _I, _P, _I, _P, _P, _P, _P, _I]),
    "ia2p_pixel_shuffle2": (_I, [_P, _P, _P, _I, _I, _I, _I]),
    "ia2p_hyper_dot": (_I, [_P, _P, _I64, _P, _P, _I, _I, _I]),
    "ia2p_sam_act": (_I, [_P, _P, _I64, _I]),
    "ia2p_sam_add_rows": (_I, [_P, _P, _P, _P, _I64, _I64]),
    "ia2p_sam_take_col": (_I, [_P, _P, _I64, _P, _I]),
    "ia2p_lora_merge": (_I, [_P, _P, _P, _I, _I64, _I, C.POINTER(_P), C.POINTER(_P), C.POINTER(_I), C.POINTER(_F)]),
    "ia2p_vae_create": (_I, [C.POINTER(VAEConfigC), C.POINTER(_P)]),
    "ia2p_vae_destroy": (None, [_P]),
    "ia2p_vae_last_error": (C.c_char_p, [_P]),
    "ia2p_vae_arena_bytes": (_SZ, [_P]),
    "ia2p_vae_bind_arena": (_I, [_P, _P, _SZ]),
    "ia2p_vae_load_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(_I64), _I, _P]),
    "ia2p_vae_finalize_weights": (_I, [_P]),
    "ia2p_vae_workspace_bytes": (_SZ, [_P, _I, _I, _I, _I]),
    "ia2p_vae_decode": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _SZ]),
    "ia2p_vae_encode": (_I, [_P, _P, _P, _P, _I, _I, _I, _P, _SZ]),
    "ia2p_image_from_u8": (_I, [_P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_image_to_u8": (_I, [_P, _P, _P, _I, _I, _I, _I]),
    "ia2p_image_to_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I]),
    "ia2p_image_requantize": (_I, [_P, _P, _P, _I64]),
    "ia2p_image_grey_u8": (_I, [_P, _P, _P, _I, _I, _I]),
    "ia2p_image_gauss_workspace_bytes": (_SZ, [_I, _I, _I, _I]),
    "ia2p_image_gauss_u8": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, C.POINTER(C.c_uint16), _I]),
    "ia2p_canny_workspace_bytes": (_SZ, [_I, _I, _I]),
    "ia2p_canny_max_rounds": (_I64, [_I, _I, _I]),
    "ia2p_canny_u8": (_I, [_P, _P, _P, _P, _SZ, _I, _I, _I, _F, _F, _I, C.POINTER(_I)]),
    "ia2p_canny_hysteresis_u8": (_I, [_P, _P, _P, _P, _SZ, _I, _I, _I, C.POINTER(_I)]),
    "ia2p_condition_from_u8": (_I, [_P, _P, _P, _I, _I, _I, _I]),
    "ia2p_profile_enable": (_I, [_P, _I]),
    "ia2p_profile_classes": (_I, []),
    "ia2p_profile_read_region": (_I, [_P, _I, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ia2p_profile_read_prefetch": (_I, [_P, _I, _P]),
    "ia2p_set_gn_fuse": (_I, [_P, _I]),
    "ia2p_debug_set_gn_plan": (None, [_I]),
    "ia2p_gn_colstats": (_I, [_P, _P, _I, _I, _I, _P]),
    "ia2p_gn_apply_stats": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _I, _I, _I, _F, _I]),
    "ia2p_conv3x3_gn": (_I, [_P, C.POINTER(ConvGnC), _P]),
    "ia2p_gemm_gnstats": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P, _I, _P, _P]),
    "ia2p_profile_roles": (_I, []),
    "ia2p_profile_read_role_class": (_I, [_P, _I, _I, C.POINTER(_I64), C.POINTER(C.c_double)]),
    "ia2p_profile_read_role": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "ia2p_profile_read": (_I, [_P, _I, C.c_char_p, _I, C.POINTER(_I64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
}

_lib = None


class IA2PError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load the HIP library. Fails loudly when it has not been built (no fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise IA2PError(f"{LIB_PATH} is missing: build it with `python -m instructany2pix_amd.build` "
                            f"(the denoise path has no non-HIP fallback)")
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7). It MUST be in the
        # process before this library is dlopen'ed so both bind to the SAME runtime instance; loaded the other way
        # round, a second runtime comes up and one of the two sees "No HIP GPUs" (observed on the MI355X boxes).
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)           # AttributeError if the .so does not export a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


FAMILIES = ("", "vae", "clip", "vit", "sam", "llm")      # the executors behind `ia2p_<family>_*`; "" is the UNet's unprefixed `ia2p_*`
UNET_KIND_FAMILIES = ("controlnet",)                     # ... and those whose handle is an ia2p_ctx of the UNet's kind under a prefix of its own (same lifecycle names)


def _family_fn(l, family: str, name: str):
    return getattr(l, f"ia2p_{family}_{name}" if family else f"ia2p_{name}")


def check(status: int, ctx=None, family: str = "", **spelled):
    """Map ia2p_status to the exception types the reference raises at the same conditions
    (ValueError from check_inputs/_get_add_time_ids, reference pnp_pipeline.py:49-66). The text is `ia2p_<family>_last_error(ctx)`;
    `vae=True` and the other family names as keywords are spellings of `family="vae"`."""
    if status == IA2P_OK:
        return
    family = next((f for f, on in spelled.items() if on), family)
    if family not in FAMILIES + UNET_KIND_FAMILIES:
        raise TypeError(f"check: no executor family '{family}'")
    msg = _family_fn(lib(), family, "last_error")(ctx)
    msg = msg.decode() if msg else ""
    text = f"ia2p {_STATUS_NAMES.get(status, status)}: {msg}"
    if status in (1, 2):
        raise ValueError(text)
    if status == 3:
        raise KeyError(text)
    if status == 5:
        raise MemoryError(text)
    raise IA2PError(text)


def addr(t):
    """Device address of a torch tensor as an integer, for a pointer field of a record (None -> NULL). Tensors must be contiguous CUDA tensors."""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous(), "ia2p needs contiguous device tensors"
    return t.data_ptr()


def ptr(t):
    """... as a pointer argument"""
    return None if t is None else C.c_void_p(addr(t))


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(method):
    """A method of an `Executor` that hands the library a stream: runs with the executor's device current (see `Executor`)."""
    @functools.wraps(method)
    def run(self, *a, **kw):
        with self._on_device():
            return method(self, *a, **kw)
    return run


class Executor:
    """One handle behind `ia2p_<family>_*` and the device memory it runs in; the six model classes derive from it. The lifecycle they share
    (DESIGN.md §13): create -> arena_bytes -> allocate and bind the arena -> load_tensor per parameter -> finalize -> workspace -> the
    model's own pass entry points -> destroy. The arena (`arena`) and the workspace (`_ws`) are torch tensors this object owns; the
    library borrows them and allocates nothing itself.

    Device rule: whatever hands the library a stream runs with `self.device` current. `current_stream()` is the CURRENT device's stream,
    and the pointers next to it live on `self.device`: without the guard a process whose current device is another GPU would pair a
    stream of one GPU with memory of another. The guard is scoped (`torch.cuda.device`); it leaves the process's current device alone."""

    _h = None            # class-level defaults: an object whose constructor raised (or never ran: a test stand-in) still destroys cleanly
    _ws = None
    def __init__(self, family: str, config_c, device, prepare=None):
        """`config_c`: the family's config struct; `prepare()`: what must happen between create and the sizing of the arena."""
        import torch
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise IA2PError(f"{type(self).__name__} runs only on an MI355X device (no CPU path exists)")
        self._family, self._lib = family, lib()
        with self._on_device():
            if not self._lib.ia2p_device_is_gfx950():
                raise IA2PError("libia2p_hip.so is compiled for gfx950 only")
            h = C.c_void_p()
            check(self._fn("create")(C.byref(config_c), C.byref(h)), None, family)
            self._h = h
            if prepare is not None:
                prepare()
            n = self._fn("arena_bytes")(h)
            self.arena = torch.zeros(n, dtype=torch.uint8, device=self.device)     # the ONE flat weight buffer
            self.check(self._fn("bind_arena")(h, ptr(self.arena), n))

    def _fn(self, name: str):
        return _family_fn(self._lib, self._family, name)

    def _on_device(self):
        import torch
        if self.device.type != "cuda":     # only a stand-in that skipped the constructor (the tests drive the LLM's host bookkeeping through one on the CPU)
            return contextlib.nullcontext()
        return torch.cuda.device(self.device)

    def check(self, status: int):
        check(status, self._h, self._family)

    def __del__(self):
        try:
            h, self._h = self._h, None
            if h:
                self._fn("destroy")(h)
        except Exception:
            pass

    # torch.nn.Module look-alikes the pipelines call
    def to(self, *a, **kw):
        return self

    def eval(self):
        return self

    @on_device
    def load_tensor(self, key: str, tensor):
        import torch
        t = tensor.detach().to(device=self.device, dtype=torch.float16).contiguous()
        shape = (C.c_int64 * t.ndim)(*t.shape)
        self.check(self._fn("load_tensor")(self._h, key.encode(), ptr(t), shape, t.ndim, current_stream()))
        # the copy into the arena is only enqueued, and `t` is a temporary whenever the caller's tensor was not fp16, contiguous and on
        # this device already: wait for the copy before the temporary can die
        torch.cuda.current_stream().synchronize()

    @on_device
    def finalize(self):
        self.check(self._fn("finalize_weights")(self._h))

    @on_device
    def workspace(self, nbytes: int):
        """The workspace tensor for a pass that needs `nbytes` (the answer of a `*_workspace_bytes` query; 0 is that query's refusal, raised
        with the handle's message). One buffer, which grows only when it is too small."""
        import torch
        if nbytes == 0:
            self.check(2)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def _context_kv(self, topology, kv_bytes, project, ctx_in, ctx, B, L, ws):
        """K/V projections of `ctx` (an executor of the UNet's kind, which keeps `_kv` and `_weights_gen`; `kv_bytes` / `project`: its `*_context_kv_bytes` /
        `*_project_context`), cached in `_kv` = (context tensor, its _version, topology, weight generation, (B, L), kv buffer) while the same
        unmodified tensor object `ctx_in` arrives with the same weights and `topology` (how the context's rows split into text and image tokens). The source tensor
        is kept alive so its address cannot be handed to another tensor."""
        import torch
        k = self._kv
        if k is not None and k[0] is ctx_in and k[1] == ctx_in._version and k[2] == topology and k[3] == self._weights_gen and k[4] == (B, L):
            return k[5]
        n = kv_bytes(self._h, B, L)
        if n == 0:
            self.check(2)
        buf = k[5] if (k is not None and k[5].numel() == n) else torch.empty(n, dtype=torch.uint8, device=self.device)
        self._kv = None
        self.check(project(self._h, current_stream(), ptr(ctx), L, B, ptr(buf), n, ptr(ws), ws.numel()))
        self._kv = (ctx_in, ctx_in._version, topology, self._weights_gen, (B, L), buf)
        return buf


def make_config(cfg) -> UNetConfigC:
    c = UNetConfigC()
    c.in_channels, c.out_channels = cfg.in_channels, cfg.out_channels
    c.n_blocks = len(cfg.block_out_channels)
    if c.n_blocks > MAX_BLOCKS:
        raise ValueError(f"at most {MAX_BLOCKS} resolution levels are supported")
    for i in range(c.n_blocks):
        c.block_out_channels[i] = cfg.block_out_channels[i]
        c.transformer_layers_per_block[i] = cfg.transformer_layers_per_block[i]
        c.num_heads[i] = cfg.attention_head_dim[i]
    c.layers_per_block = cfg.layers_per_block
    c.cross_attention_dim = cfg.cross_attention_dim
    c.norm_num_groups, c.norm_eps = cfg.norm_num_groups, cfg.norm_eps
    c.addition_time_embed_dim = cfg.addition_time_embed_dim
    c.projection_class_embeddings_input_dim = cfg.projection_class_embeddings_input_dim
    c.time_embed_dim, c.time_proj_dim = cfg.time_embed_dim, cfg.time_proj_dim
    c.mid_transformer_layers, c.num_time_ids = cfg.mid_block_transformer_layers, cfg.num_time_ids
    return c


def make_controlnet_config(cfg) -> ControlNetConfigC:
    c = ControlNetConfigC()
    c.unet = make_config(cfg)
    c.conditioning_channels = cfg.conditioning_channels
    if len(cfg.conditioning_embedding_out_channels) != 4:
        raise ValueError("conditioning_embedding_out_channels must name four widths")
    for i, v in enumerate(cfg.conditioning_embedding_out_channels):
        c.conditioning_embedding_out_channels[i] = int(v)
    return c


def make_clip_config(cfg) -> CLIPConfigC:
    c = CLIPConfigC()
    c.vocab_size, c.hidden_size, c.num_layers, c.num_heads = cfg.vocab_size, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads
    c.intermediate_size, c.max_positions, c.projection_dim = cfg.intermediate_size, cfg.max_position_embeddings, cfg.projection_dim
    c.hidden_act = {"gelu": 1, "quick_gelu": 2, "gelu_new": 3}[cfg.hidden_act]
    c.eos_token_id, c.layer_norm_eps = cfg.eos_token_id, cfg.layer_norm_eps
    return c


def make_vit_config(cfg) -> ViTConfigC:
    c = ViTConfigC()
    for name, _ in ViTConfigC._fields_:
        setattr(c, name, getattr(cfg, name))
    return c


def make_sam_config(cfg) -> SAMConfigC:
    c = SAMConfigC()
    if len(cfg.global_attn_indexes) > 8:
        raise ValueError("at most 8 global-attention blocks are supported")
    for name, _ in SAMConfigC._fields_:
        if name == "num_global":
            c.num_global = len(cfg.global_attn_indexes)
        elif name == "global_attn_indexes":
            for i, v in enumerate(cfg.global_attn_indexes):
                c.global_attn_indexes[i] = int(v)
        else:
            setattr(c, name, getattr(cfg, name))
    return c


def make_llm_config(cfg) -> LLMConfigC:
    c = LLMConfigC()
    c.vocab_size, c.hidden_size, c.num_layers, c.num_heads = cfg.vocab_size, cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads
    c.num_kv_heads, c.intermediate_size = cfg.num_key_value_heads, cfg.intermediate_size
    c.rms_norm_eps, c.rope_theta = cfg.rms_norm_eps, cfg.rope_theta
    return c


def make_vae_config(cfg) -> VAEConfigC:
    c = VAEConfigC()
    c.in_channels, c.out_channels, c.latent_channels = cfg.in_channels, cfg.out_channels, cfg.latent_channels
    c.n_blocks = len(cfg.block_out_channels)
    if c.n_blocks > MAX_BLOCKS:
        raise ValueError(f"at most {MAX_BLOCKS} resolution levels are supported")
    for i in range(c.n_blocks):
        c.block_out_channels[i] = cfg.block_out_channels[i]
    c.layers_per_block, c.norm_num_groups, c.norm_eps = cfg.layers_per_block, cfg.norm_num_groups, cfg.norm_eps
    c.stream_scale = float(getattr(cfg, "stream_scale", 1.0))
    return c
