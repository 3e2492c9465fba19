"""ctypes binding of libdm_engine.so (C ABI: include/dm_engine.h) — PyTorch-ROCm is used only for
device memory, streams and `torch.distributed`; every FLOP of the U-Net runs in the HIP library.

There is NO fallback path: if the library is missing or no GPU is present, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdm_engine.so")
_lib = None
_CHECK_DEVICE_SLOTS = os.environ.get("DM_CHECK_SLOTS", "0") not in ("", "0")     # debug: validate prompt slots that live on the GPU

_vp, _cp, _i32, _i64, _f32, _f64, _sz = C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_size_t
_pvp, _pi32, _pi64, _pf32, _pf64, _psz = (C.POINTER(t) for t in (_vp, _i32, _i64, _f32, _f64, _sz))
_WEIGHT = [_vp, _cp, _vp, _i32, _pi64, _i32]        # (handle, name, host_ptr, dtype, shape, ndim) of every *_load_*weight
_PROF = [_vp, _pf64, _pf64, _pi64, _pf64, _pf64, _pi64]

# The C signature of every symbol include/dm_engine.h declares, in the header's order: name -> (restype, argtypes).  This is the one
# place a signature is written down; load_library() applies it and tests/test_abi.py checks it against the header argument by argument.
SIGNATURES = {
    "dm_version": (_cp, []),
    "dm_scheduler_alphas_cumprod": (_i32, [_i32, _f32, _f32, _pf32]),
    "dm_timestep_sinusoid": (_i32, [_i32, _i32, _pf32]),
    "dm_engine_create": (_i32, [_i32, _pvp]),
    "dm_engine_destroy": (None, [_vp]),
    "dm_last_error": (_cp, [_vp]),
    "dm_engine_load_weight": (_i32, _WEIGHT),
    "dm_engine_finalize": (_i32, [_vp]),
    "dm_engine_set_prompts": (_i32, [_vp, _vp, _i32, _vp]),
    "dm_score": (_i32, [_vp] * 6 + [_i32] * 5 + [_vp, _vp]),
    "dm_score_conds": (_i32, [_vp] * 5 + [_i32] * 6 + [_vp, _vp]),
    "dm_score_conds_slots": (_i32, [_vp] * 6 + [_i32] * 6 + [_vp, _vp]),
    "dm_unet_forward": (_i32, [_vp] * 4 + [_i32, _i32, _i32, _vp, _vp]),
    "dm_dift": (_i32, [_vp] * 4 + [_i32] * 4 + [_vp, _vp, _i32, _vp]),
    "dm_dift_shape": (_i32, [_i32, _i32, _i32, _pi32, _pi32, _pi32]),
    "dm_reduce_typicality": (_i32, [_vp, _vp] + [_i32] * 5 + [_vp, _vp, _vp]),
    "dm_reduce_typicality_batched": (_i32, [_vp, _vp] + [_i32] * 7 + [_vp, _vp, _vp]),
    "dm_typicality_image": (_i32, [_vp, _vp] + [_i32] * 9 + [_vp, _vp, _vp]),
    "dm_normalize_map": (_i32, [_vp, _vp, _i64, _i32] + [_vp] * 4),
    "dm_resize_lanczos": (_i32, [_vp, _vp, _vp] + [_i32] * 4 + [_vp, _vp, _vp]),
    "dm_typicality_image_batched": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "dm_mine_patches": (_i32, [_vp] * 4 + [_i32] * 5 + [_vp] * 4),
    "dm_mine_parallel": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp] + [_i32] * 4 + [_vp] * 7),
    "dm_clipmine_workspace_bytes": (_sz, [_i32, _i64, _i64]),
    "dm_clipmine_rank": (_i32, [_vp, _vp, _vp, _i32, _vp, _i32, _vp] + [_i32] * 4 + [_vp, _sz] + [_vp] * 5),
    "dm_kmeans_workspace_bytes": (_i32, [_i32, _i32, _i32, _psz]),
    "dm_kmeans_fit": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _f32, _vp, _sz] + [_vp] * 5),
    "dm_cluster_rank": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _sz] + [_vp] * 5),
    "dm_umap_workspace_bytes": (_i32, [_i32] * 4 + [_psz]),
    "dm_umap_knn": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp, _vp]),
    "dm_umap_graph": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz] + [_vp] * 7),
    "dm_umap_layout": (_i32, [_vp] * 4 + [_i32] * 3 + [_f32, _f32] + [_i32] * 4 + [_vp, _vp, _sz]),
    "dm_umap_spectral_workspace_bytes": (_i32, [_i32, _i32, _psz]),
    "dm_umap_spectral": (_i32, [_vp] * 4 + [_i32] * 3 + [_vp] * 3 + [_sz] + [_vp] * 4),
    "dm_umap_sparse_workspace_bytes": (_i32, [_i32] * 4 + [_psz]),
    "dm_umap_sparse_knn": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp, _vp]),
    "dm_umap_sparse_graph": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz] + [_vp] * 6),
    "dm_umap_sparse_layout": (_i32, [_vp] * 4 + [_i32] * 3 + [_f32, _f32] + [_i32] * 4 + [_vp, _vp, _sz]),
    "dm_umap_sparse_spectral_workspace_bytes": (_i32, [_i32, _i32, _psz]),
    "dm_umap_sparse_spectral": (_i32, [_vp] * 4 + [_i32] * 3 + [_vp] * 3 + [_sz] + [_vp] * 4),
    "dm_umap_components_workspace_bytes": (_i32, [_i32, _psz]),
    "dm_umap_components": (_i32, [_vp] * 5 + [_i32] * 3 + [_vp, _sz] + [_vp] * 9),
    "dm_umap_multi_workspace_bytes": (_i32, [_i32, _i32, _psz]),
    "dm_umap_multi_init": (_i32, [_vp] * 11 + [_i32] * 5 + [_vp] * 5 + [_sz] + [_vp] * 5),
    "dm_xray_eval_workspace_bytes": (_sz, [_i32, _i32, _i64]),
    "dm_xray_eval": (_i32, [_vp, _vp, _i32, _vp, _i32] + [_vp] * 6),
    "dm_overlay_workspace_bytes": (_sz, [_i32, _i64, _i32, _i32]),
    "dm_gaussian_filter_maps": (_i32, [_vp, _vp, _i32, _f64, _vp, _i32, _i32, _vp, _sz, _vp, _vp, _vp]),
    "dm_overlay_blend": (_i32, [_vp, _i64, _vp, _i64, _vp, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp]),
    "dm_dense_search_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "dm_dense_search_winners": (_i32, [_vp] * 4 + [_i32] * 6 + [_vp, _sz, _vp, _vp]),
    "dm_dense_search_topk": (_i32, [_vp] * 3 + [_i32] * 5 + [_vp] * 4),
    "dm_dense_search_gather": (_i32, [_vp, _vp] + [_i32] * 3 + [_vp, _i32, _vp]),
    "dm_dense_wide_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "dm_dense_wide_winners": (_i32, [_vp] * 4 + [_i32] * 6 + [_vp, _sz, _vp, _vp]),
    "dm_dense_wide_topk": (_i32, [_vp] * 3 + [_i32] * 5 + [_vp] * 8),
    "dm_detector_rank_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "dm_detector_rank": (_i32, [_vp] * 6 + [_i32] * 5 + [_vp, _sz, _vp, _vp]),
    "dm_hoglab_bin_table": (_i32, [_vp]),
    "dm_hoglab_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "dm_hoglab_cells": (_i32, [_vp, _vp] + [_i32] * 3 + [_vp] * 3),
    "dm_hoglab_features": (_i32, [_vp, _vp] + [_i32] * 3 + [_vp] * 4 + [_sz]),
    "dm_svm_workspace_bytes": (_sz, [_i32, _i32]),
    "dm_svm_fit": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _f64, _f64, _i32, _vp, _sz] + [_vp] * 5),
    "dm_svm_hard_negatives": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32] + [_vp] * 3 + [_i32, _vp, _vp, _vp, _sz] + [_vp] * 3),
    "dm_prof_enable": (_i32, [_vp, _i32]),
    "dm_measure_mfma_rate": (_i32, [_vp, _i32, _i32, _pf64, _pf64]),
    "dm_prof_read": (_i32, _PROF),
    "dm_prof_read_folded": (_i32, [_vp, _pf64]),
    "dm_engine_load_vae_weight": (_i32, _WEIGHT),
    "dm_engine_finalize_vae": (_i32, [_vp]),
    "dm_vae_encode": (_i32, [_vp, _vp, _vp] + [_i32] * 4 + [_f32] + [_vp] * 4),
    "dm_engine_load_vae_decoder_weight": (_i32, _WEIGHT),
    "dm_engine_finalize_vae_decoder": (_i32, [_vp]),
    "dm_vae_decode": (_i32, [_vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "dm_sample_run": (_i32, [_vp] * 5 + [_i32] * 4 + [_f32, _vp]),
    "dm_engine_load_clip_weight": (_i32, _WEIGHT),
    "dm_engine_finalize_clip": (_i32, [_vp]),
    "dm_clip_encode": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _vp]),
    "dm_patch_embed": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp]),
    "dm_engine_memory": (_i32, [_vp, _psz, _psz]),
    "dm_engine_reserve": (_i32, [_vp] + [_i32] * 5 + [_vp]),
    "dm_engine_stats": (_i32, [_vp, _pi64, _pi64, _pi64]),
    "dm_op_igemm": (_i32, [_vp] * 8 + [_i32] * 11),
    "dm_set_option": (_i32, [_cp, _i32]),
    "dm_get_option": (_i32, [_cp, _pi32]),
    "dm_op_igemm_tile": (_i32, [_i32] * 4),
    "dm_op_igemm_head_rows": (_i32, [_i32] * 5),
    "dm_op_igemm_pers_max_source_channels": (_i32, []),
    "dm_op_attention": (_i32, [_vp] * 5 + [_i32] * 4 + [_i64] * 4 + [_vp] + [_i32] * 5 + [_f32]),
    "dm_op_attention_slots": (_i32, [_vp] * 5 + [_i32] * 4 + [_i64] * 4 + [_vp] + [_i32] * 8 + [_f32]),
    "dm_op_attention_route": (_i32, [_i32] * 6),
    "dm_op_ln_stats": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp]),
    "dm_op_igemm_ln": (_i32, [_vp] * 7 + [_i32] * 4),
    "dm_op_igemm_splitk": (_i32, [_vp] * 8 + [_i32] * 11 + [_vp]),
    "dm_op_attention512": (_i32, [_vp] * 5 + [_i32] * 4 + [_f32]),
    "dm_op_groupnorm": (_i32, [_vp, _vp, _vp] + [_i32] * 5 + [_f32, _vp, _vp, _i32, _vp]),
    "dm_op_layernorm": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _f32, _vp]),
    "dm_op_conv_out": (_i32, [_vp] * 5 + [_i32] * 4 + [_vp, _vp]),
    "dm_op_conv_temb_gn_blocks": (_i32, [_vp] * 6 + [_i32] * 6 + [_vp, _pi32]),
    "dm_op_gn_blocks": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "dm_op_groupnorm_blocks": (_i32, [_vp, _vp, _vp] + [_i32] * 4 + [_f32, _vp, _vp, _i32, _vp]),
    "dm_op_igemm_shortcut": (_i32, [_vp] * 8 + [_i32] * 8),
    "dm_op_fold_upconv_weights": (_i32, [_vp, _i32, _i32, _vp]),
    "dm_op_upconv_folded": (_i32, [_vp] * 5 + [_i32] * 5),
    "dm_op_groupnorm_conv1x1": (_i32, [_vp, _vp] + [_i32] * 4 + [_f32] + [_vp] * 4 + [_i32, _vp]),
    "dm_op_time_gather": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "dm_op_silu": (_i32, [_vp, _vp, _vp, _i64]),
    "dm_op_im2col_in": (_i32, [_vp] * 7 + [_i32] * 4 + [_vp]),
    "dm_op_nhwc_to_nchw": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "dm_op_ensemble_mean": (_i32, [_vp, _vp] + [_i32] * 4 + [_vp]),
    "dm_op_im2col_rgb": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "dm_op_posterior": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "dm_op_clip_embed": (_i32, [_vp] * 4 + [_i32] * 4 + [_vp]),
    "dm_op_clip_attention": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "dm_op_quick_gelu": (_i32, [_vp, _vp, _i64]),
    "dm_op_f16_to_f32": (_i32, [_vp, _vp, _vp, _i64]),
    "dm_op_cfg_ddim_step": (_i32, [_vp] * 4 + [_f32, _i64, _vp]),
    "dm_op_latent_prologue": (_i32, [_vp] * 4 + [_i32, _i32, _f32, _vp, _i32]),
    "dm_op_decoder_tail_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "dm_op_decoder_tail": (_i32, [_vp] * 6 + [_i32] * 3 + [_f32, _vp, _sz, _vp, _vp]),
    "dm_f32_create": (_i32, [_i32, _pvp]),
    "dm_f32_destroy": (None, [_vp]),
    "dm_f32_last_error": (_cp, [_vp]),
    "dm_f32_load_weight": (_i32, _WEIGHT),
    "dm_f32_finalize": (_i32, [_vp]),
    "dm_f32_set_prompts": (_i32, [_vp, _vp, _i32, _vp]),
    "dm_f32_unet_forward": (_i32, [_vp] * 4 + [_i32, _i32, _i32, _vp, _vp]),
    "dm_f32_dift": (_i32, [_vp] * 4 + [_i32] * 4 + [_vp, _vp, _i32, _vp]),
    "dm_f32_score": (_i32, [_vp] * 6 + [_i32] * 4 + [_vp, _vp]),
    "dm_f32_load_vae_weight": (_i32, _WEIGHT),
    "dm_f32_finalize_vae": (_i32, [_vp]),
    "dm_f32_vae_encode": (_i32, [_vp, _vp, _vp] + [_i32] * 4 + [_f32, _vp, _vp, _vp]),
    "dm_f32_load_vae_decoder_weight": (_i32, _WEIGHT),
    "dm_f32_finalize_vae_decoder": (_i32, [_vp]),
    "dm_f32_vae_decode": (_i32, [_vp, _vp, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _vp]),
    "dm_f32_unet_forward_inject": (_i32, [_vp] * 4 + [_i32] * 5 + [_vp, _vp]),
    "dm_f32_ddim_run": (_i32, [_vp] * 7 + [_i32] * 4 + [_vp]),
    "dm_f32_pnp_run": (_i32, [_vp] * 7 + [_i32, _i32, _vp] + [_i32] * 4 + [_f32, _vp]),
    "dm_f32_load_clip_weight": (_i32, _WEIGHT),
    "dm_f32_finalize_clip": (_i32, [_vp]),
    "dm_f32_clip_encode": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "dm_f32_load_clip_vision_weight": (_i32, _WEIGHT),
    "dm_f32_finalize_clip_vision": (_i32, [_vp]),
    "dm_f32_clip_preprocess": (_i32, [_vp] * 4 + [_i32, _vp, _vp]),
    "dm_f32_clip_image_features": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "dm_f32_clip_vision_hidden": (_i32, [_vp, _vp, _i32, _vp, _vp]),
    "dm_f32_clip_patch_features": (_i32, [_vp] * 4 + [_i32, _i32, _vp, _vp]),
    "dm_f32_clip_text_embeds": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "dm_f32_load_clip_tower_weight": (_i32, _WEIGHT),
    "dm_f32_finalize_clip_tower": (_i32, [_vp, _vp]),
    "dm_f32_clip_tower_preprocess": (_i32, [_vp] * 4 + [_i32, _i32, _vp, _vp]),
    "dm_f32_clip_tower_tokens": (_i32, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "dm_f32_clip_tower_image_tokens": (_i32, [_vp] * 4 + [_i32, _vp, _vp]),
    "dm_f32_prof_enable": (_i32, [_vp, _i32]),
    "dm_f32_prof_read": (_i32, _PROF),
    "dm_f32_memory": (_i32, [_vp, _psz, _psz]),
    "dm_f32_op_gemm": (_i32, [_vp] * 8 + [_i32] * 10),
    "dm_f32_op_attention": (_i32, [_vp] * 5 + [_i32] * 4 + [_i64] * 4 + [_vp] + [_i32] * 6 + [_f32]),
    "dm_f32_op_groupnorm": (_i32, [_vp, _vp, _vp] + [_i32] * 5 + [_f32, _vp, _vp, _i32, _vp, _vp]),
    "dm_f32_op_layernorm": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _f32, _vp]),
    "dm_f32_op_clip_patch_ln": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _f32, _vp]),
    "dm_f32_op_ddim_step": (_i32, [_vp] * 4 + [_i64, _vp]),
    "dm_f32_op_ddim_step_cfg": (_i32, [_vp] * 4 + [_f32, _vp, _i64, _vp]),
    "dm_f32_op_bcast_add": (_i32, [_vp, _vp, _vp, _i32, _i64, _vp]),
    "dm_f32_op_decoder_tail": (_i32, [_vp] * 7 + [_i32] * 5 + [_vp, _vp]),
    "dm_f32_op_conv_out": (_i32, [_vp] * 4 + [_i32] * 5 + [_vp]),
    "dm_f32_op_clip_embed": (_i32, [_vp] * 4 + [_i32] * 4 + [_vp]),
    "dm_f32_op_clip_attention": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "dm_f32_op_quick_gelu": (_i32, [_vp, _vp, _i64]),
    "dm_f32_op_silu": (_i32, [_vp, _vp, _vp, _i64]),
    "dm_f32_op_timestep_embed": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "dm_f32_op_conv_in": (_i32, [_vp] * 4 + [_i32] * 5 + [_vp]),
    "dm_f32_op_add_noise": (_i32, [_vp] * 7 + [_i32, _i64, _vp]),
    "dm_f32_op_sqerr": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "dm_f32_op_nhwc_to_nchw": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "dm_f32_op_ensemble_mean": (_i32, [_vp, _vp] + [_i32] * 4 + [_vp]),
    "dm_f32_op_posterior": (_i32, [_vp] * 5 + [_i32] * 3 + [_f32, _vp, _vp]),
    "dm_f32_op_gemm_wgrad_workspace": (_sz, [_i32] * 8),
    "dm_f32_op_gemm_wgrad": (_i32, [_vp] * 6 + [_sz] + [_i32] * 10),
    "dm_f32_op_colsum": (_i32, [_vp, _vp] + [_i32] * 4 + [_vp]),
    "dm_f32_op_groupnorm_bwd": (_i32, [_vp] * 4 + [_i32] * 5 + [_vp, _vp, _vp, _i32, _vp, _sz] + [_vp] * 4),
    "dm_f32_op_silu_bwd": (_i32, [_vp] * 4 + [_i64]),
    "dm_f32_op_zero_insert2": (_i32, [_vp, _vp] + [_i32] * 4 + [_vp]),
    "dm_f32_op_nearest_bwd": (_i32, [_vp, _vp] + [_i32] * 6 + [_vp]),
    "dm_f32_op_attention_bwd_workspace": (_sz, [_i32] * 5),
    "dm_f32_op_attention_bwd_slabs": (_i32, [_i32, _i32]),
    "dm_f32_op_attention_bwd": (_i32, [_vp] * 12 + [_i32] * 5 + [_f32, _vp, _sz]),
    "dm_f32_op_attention_bwd_phases": (_i32, [_vp] * 12 + [_i32] * 5 + [_f32, _vp, _sz, _i32]),
    "dm_f32_op_layernorm_bwd_workspace": (_sz, [_i32, _i32]),
    "dm_f32_op_layernorm_bwd": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _f32, _vp, _sz, _vp, _vp, _vp]),
    "dm_f32_op_geglu": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "dm_f32_op_geglu_bwd": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp]),
}
SYMBOLS = list(SIGNATURES)

# dm_mine_desc of include/dm_engine.h (48 bytes) and the compile-time cap of k_per_image
MINE_DESC_DTYPE = np.dtype([("grid_offset", "<i8"), ("work_offset", "<i8"), ("map_offset", "<i8"), ("n_draws", "<i4"), ("n_cond", "<i4"),
                            ("h", "<i4"), ("w", "<i4"), ("H", "<i4"), ("W", "<i4")])
MINE_MAX_K = 64
MINE_MAX_SETS = 16          # DM_MINE_MAX_SETS: the set counts median_maps_kernel is instantiated for
CLIP_TOWER_CHUNK = 64       # CT_CHUNK (f32_impl.h): images per run of the configurable CLIP image tower


def get_options(names=("ln_fold", "gn_fold", "ff_fold", "sc_fold", "up_fold", "tap_reuse", "ln_inkernel", "igemm_splitk", "q_once", "gn_epi", "conv_out_rows", "gn_skip", "attn_pipe", "graph")) -> dict:
    """Current values of the library's runtime switches (dm_get_option); {} with a library that predates the getter."""
    lib = load_library()
    out = {}
    if not hasattr(lib, "dm_get_option"):
        return out
    for n in names:
        v = C.c_int32()
        if lib.dm_get_option(n.encode(), C.byref(v)) == 0:
            out[n] = v.value
    return out


class EngineError(RuntimeError):
    pass


def load_library(path: Optional[str] = None) -> C.CDLL:
    """Load libdm_engine.so; raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("DM_ENGINE_LIB") or LIB_PATH   # DM_ENGINE_LIB: kernel A/B experiments
    if not os.path.exists(p):
        raise EngineError(
            f"{p} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
            "The typicality engine has no CPU / PyTorch fallback.")
    # PyTorch-ROCm ships its own libamdhip64; importing torch first makes this library bind to that
    # same HIP runtime (two runtimes in one process cannot see each other's device context).
    import torch  # noqa: F401
    lib = C.CDLL(p)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name, None)          # a symbol is absent only from older A/B libraries loaded through DM_ENGINE_LIB
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = lib
    return lib


def _p(t):
    """A tensor's address as a pointer argument; None stays NULL."""
    return None if t is None else C.c_void_p(t.data_ptr())


def scheduler_alphas_cumprod(n: int = 1000, beta_start: float = 0.00085, beta_end: float = 0.012) -> np.ndarray:
    """Host-only: the engine's own ᾱ table (no GPU needed)."""
    lib = load_library()
    out = np.empty(n, dtype=np.float32)
    if lib.dm_scheduler_alphas_cumprod(n, beta_start, beta_end, out.ctypes.data_as(C.POINTER(C.c_float))):
        raise EngineError("dm_scheduler_alphas_cumprod failed")
    return out


def timestep_sinusoid(t: int, dim: int = 320) -> np.ndarray:
    lib = load_library()
    out = np.empty(dim, dtype=np.float32)
    if lib.dm_timestep_sinusoid(int(t), dim, out.ctypes.data_as(C.POINTER(C.c_float))):
        raise EngineError("dm_timestep_sinusoid failed")
    return out


def dift_shape(h: int, w: int, up_ft_index: int = 1) -> Tuple[int, int, int]:
    lib = load_library()
    c, oh, ow = C.c_int(), C.c_int(), C.c_int()
    if lib.dm_dift_shape(h, w, up_ft_index, C.byref(c), C.byref(oh), C.byref(ow)):
        raise EngineError("dm_dift_shape failed")
    return c.value, oh.value, ow.value


# -- the dm_mine_desc table of the batched mining calls ---------------------------------------------------------------------------
def _mine_desc(shapes, kx: int, ky: int):
    """dm_mine_desc rows (map_offset, H, W) for pooled maps [OH, OW] of window kx x ky packed back to back -> (table, floats in all)."""
    desc = np.zeros(len(shapes), dtype=MINE_DESC_DTYPE)
    sizes = [int(s[0]) * int(s[1]) for s in shapes]
    desc["H"], desc["W"] = [s[0] + kx - 1 for s in shapes], [s[1] + ky - 1 for s in shapes]
    desc["map_offset"] = np.cumsum([0] + sizes[:-1])
    return desc, sum(sizes)


def _check_mine_args(what: str, k_per_image, priority, n: int, of: str) -> int:
    if priority is not None and len(priority) != n:
        raise ValueError(f"{n} {of} but {len(priority)} priority maps")
    k_per_image = int(k_per_image)
    if k_per_image < 1 or k_per_image > MINE_MAX_K:
        raise EngineError(f"{what}: k_per_image {k_per_image} outside [1, {MINE_MAX_K}]")
    return k_per_image


def _pack_priority(torch, device, priority, shapes, whose: str):
    """The optional sort-key maps, one per entry of `shapes` and shaped like it, as one fp32 buffer on `device` (None stays None)."""
    if priority is None:
        return None
    for b, (t, s) in enumerate(zip(priority, shapes)):
        if tuple(t.shape) != tuple(s):
            raise ValueError(f"priority map {b} is {tuple(t.shape)}, the {whose} {tuple(s)}")
    return torch.cat([torch.as_tensor(t).to(device, torch.float32).reshape(-1) for t in priority])


def _views(buffer, desc, kx: int, ky: int):
    """The maps [H-kx+1, W-ky+1] of a descriptor table as views of the packed buffer they lie in."""
    out = []
    for d in desc:
        at, oh, ow = int(d["map_offset"]), int(d["H"]) - kx + 1, int(d["W"]) - ky + 1
        out.append(buffer[at:at + oh * ow].view(oh, ow))
    return out


class _EngineBase:
    """What the fp16 and the fp32 engine share: the handle, the weight loader, the prompt slots, and the calls that differ only in
    the C prefix and the tensor type.  A subclass names those; one engine per GPU (the reference is one process per GPU,
    compute.py:215).  No fallback: raises without the library or a GPU."""
    _OBJ = _RUN = None      # C prefixes: _OBJ of create / destroy / load_*_weight / finalize_* / set_prompts / memory, _RUN of every other call
    _DTYPE = None           # torch's name of the element type of the tensors at the boundary

    def __init__(self, device: int = 0):
        import torch
        self._torch = torch
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise EngineError("no GPU visible: the MI355X typicality engine has no CPU fallback")
        self.dtype = getattr(torch, self._DTYPE)
        # resolved once: `unet` and `dift` run once per U-Net batch
        self._unet_fn, self._dift_fn = getattr(self.lib, self._RUN + "unet_forward"), getattr(self.lib, self._RUN + "dift")
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        h = C.c_void_p()
        if getattr(self.lib, self._OBJ + "create")(self.device_index, C.byref(h)):
            raise EngineError(f"{self._OBJ}create: " + getattr(self.lib, self._RUN + "last_error")(None).decode())
        self._h = h
        self.n_prompts = 0
        self.prompt_generation = 0          # bumped by every set_prompts: callers that cache slots compare it
        self._finalized = False

    # -- plumbing --------------------------------------------------------------------------------
    def _check(self, rc: int, what: str):
        if rc:
            raise EngineError(f"{what}: {getattr(self.lib, self._RUN + 'last_error')(self._h).decode()}")

    def _call(self, prefix: str, name: str, *args):
        """A call on the handle that is not in the hot path: <prefix><name>(handle, *args), checked."""
        self._check(getattr(self.lib, prefix + name)(self._h, *args), self._RUN[3:] + name)

    def _stream(self):
        return C.c_void_p(self._torch.cuda.current_stream(self.device).cuda_stream)

    def kmeans_fit(self, X, k: int = 32, seed: int = 10, max_iter: int = 300, tol: float = 1e-4, init_index=None, work=None):
        """scikit-learn's `KMeans(n_clusters=k, random_state=seed).fit(X)` on this engine's device and current stream
        (dm_kmeans_fit; see `clustering.kmeans_fit`)."""
        from . import clustering
        with self._torch.cuda.device(self.device):
            return clustering.kmeans_fit(X, k, seed, max_iter, tol, init_index, work)

    def cluster_rank(self, X, labels, centers, D, aggregate: str = "median", order_by: str = "centroid", rank_features=None, work=None):
        """The tail of the reference's `cluster()` on the device (dm_cluster_rank; see `clustering.rank_clusters`)."""
        from . import clustering
        with self._torch.cuda.device(self.device):
            return clustering.rank_clusters(X, labels, centers, D, aggregate, order_by, rank_features, work)

    def umap_fit(self, X, n_components: int, n_neighbors: int = 15, seed: int = 42, n_epochs=None, work=None, init_solver: str = "host",
                 route: str = "auto", disconnected: str = "random"):
        """The UMAP projection of the clustering stage on this engine's device and current stream (dm_umap_knn / dm_umap_graph /
        dm_umap_layout, and dm_umap_spectral with init_solver='device', or their dm_umap_sparse_ forms by `route`; see `umapfit.umap_fit`;
        parity with umap-learn unpinned)."""
        from . import umapfit
        with self._torch.cuda.device(self.device):
            return umapfit.umap_fit(X, n_components, n_neighbors, seed, n_epochs, work, init_solver=init_solver, route=route,
                                    disconnected=disconnected)

    def xray_eval(self, maps, boxes, thresholds=None, work=None):
        """The counts of the X-ray application's AUC-PR and the box sums for a batch of heat-maps on this engine's device and
        current stream (dm_xray_eval; see `xray.xray_eval`)."""
        from . import xray
        with self._torch.cuda.device(self.device):
            return xray.xray_eval(maps, boxes, thresholds, work)

    def gaussian_filter(self, maps, sigma, post_op: str = "none", work=None, return_max: bool = False):
        """scipy's `gaussian_filter(a, sigma)` on a list of fp32 maps of mixed sizes, bit for bit, on this engine's device and current
        stream (dm_gaussian_filter_maps; see `overlay.gaussian_filter`)."""
        from . import overlay
        with self._torch.cuda.device(self.device):
            return overlay.gaussian_filter(maps, sigma, post_op, work, return_max)

    def overlay_rows(self, images, maps, rows, variant: str = "image", sigma=10, want_alpha: bool = False):
        """The reference's three alpha-blend variants and `filter_patch` for a table of boxes on this engine's device and current
        stream (dm_gaussian_filter_maps + dm_overlay_blend; see `overlay.overlay_rows`)."""
        from . import overlay
        with self._torch.cuda.device(self.device):
            return overlay.overlay_rows(images, maps, rows, variant, sigma, want_alpha)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self.lib, self._OBJ + "destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights ---------------------------------------------------------------------------------
    def _load(self, what: str, sd, *finalize_args):
        """Every tensor of a state dict (numpy or torch; fp16 and fp32 as they are, anything else widened to fp32) to
        <_OBJ>load<what>_weight, then <_OBJ>finalize<what>(handle, *finalize_args); what = "" (the U-Net), "_vae", "_clip",
        "_clip_vision", "_clip_tower"."""
        torch = self._torch
        fn = getattr(self.lib, f"{self._OBJ}load{what}_weight")
        for name, t in sd.items():
            if hasattr(t, "detach"):
                t = t.detach().to("cpu")
                t = t.to(torch.float32).numpy() if t.dtype not in (torch.float16, torch.float32) else t.numpy()
            a = np.ascontiguousarray(t)
            if a.dtype == np.float16:
                dt = 0
            elif a.dtype == np.float32:
                dt = 1
            else:
                a = a.astype(np.float32)
                dt = 1
            shape = (C.c_int64 * a.ndim)(*a.shape)
            self._check(fn(self._h, name.encode(), a.ctypes.data_as(C.c_void_p), dt, shape, a.ndim),
                        f"{self._RUN[3:]}load{what}_weight({name})")
        self._call(self._OBJ, f"finalize{what}", *finalize_args)

    def load_state_dict(self, sd: Dict[str, "np.ndarray"]):
        """sd: diffusers-named U-Net state dict (numpy or torch tensors, fp16/fp32/bf16; the fp32 engine keeps fp32 as it is and
        widens fp16 / bf16 exactly)."""
        self._load("", sd)
        self._finalized = True

    def load_vae_state_dict(self, sd: Dict[str, "np.ndarray"]):
        """sd: `AutoencoderKL.state_dict()` (`pipe.vae`, compute.py:73); only `encoder.*` and
        `quant_conv.*` are used, the decoder half is ignored.  Optional: scoring needs only the U-Net."""
        self._load("_vae", sd)
        self._vae_ready = True

    def load_clip_state_dict(self, sd: Dict[str, "np.ndarray"]):
        """sd: `CLIPTextModel.state_dict()` (`pipe.text_encoder`, compute.py:68; the featuriser's pipeline keeps it in fp32,
        dift.py:197-199).  Optional.  The fp32 net also takes `CLIPTextModelWithProjection.state_dict()`: its 197th tensor
        `text_projection.weight` enables `UNetEngineF32.clip_text_embeds`."""
        self._load("_clip", sd)
        self._clip_ready = True

    # -- prompts ---------------------------------------------------------------------------------
    def set_prompts(self, ctx):
        """ctx [P,77,768] (`prompt_embeds`, dift.py:222-227): distinct prompt embeddings, kept in the engine's element type;
        precomputes cross-attention K/V for them."""
        ctx = ctx.to(self.device, self.dtype).contiguous()
        assert ctx.dim() == 3 and ctx.shape[1] == 77 and ctx.shape[2] == 768, ctx.shape
        self._call(self._OBJ, "set_prompts", _p(ctx), ctx.shape[0], self._stream())
        self._ctx_keepalive = ctx
        self.n_prompts = ctx.shape[0]
        self.prompt_generation += 1

    def _slots(self, slots, batch):
        """Prompt slots of a batch -> int32 on the device.  Host-side inputs (lists, CPU tensors) are range-checked against
        the registered prompts here (a slot beyond them would read another prompt set's stale K/V rows); a tensor that
        already lives on the device is not pulled back for the check — that would be two blocking syncs in the hot path
        (`TypicalityScorer.compute_loss` passes `torch.unique`'s inverse, in range by construction) — the kernels clamp
        device-side slots to the registered range instead (memory-safe, never another engine's rows)."""
        torch = self._torch
        s = torch.as_tensor(slots)
        assert s.shape == (batch,), (s.shape, batch)
        if s.numel() and (not s.is_cuda or _CHECK_DEVICE_SLOTS):      # DM_CHECK_SLOTS=1: also range-check device tensors (two syncs)
            lo, hi = int(s.min()), int(s.max())
            if lo < 0 or hi >= self.n_prompts:
                raise EngineError(f"prompt slot {lo if lo < 0 else hi} outside the {self.n_prompts} prompts registered "
                                  "by set_prompts")
        return s.to(self.device, torch.int32).contiguous()

    def _timesteps(self, t, batch):
        """t (a number, a list or a tensor; one value is broadcast) -> int64 [batch] on the device."""
        torch = self._torch
        t = torch.as_tensor(t, device=self.device).to(torch.int64).reshape(-1)
        if t.numel() == 1:
            t = t.expand(batch)
        assert t.shape == (batch,), (t.shape, batch)
        return t.contiguous()

    def _x_index(self, x_index, n_x, batch):
        """The row of x each sample reads -> int32 [batch] on the device, or None for the identity; one x serves every sample."""
        torch = self._torch
        if x_index is not None:
            xi = torch.as_tensor(x_index, device=self.device).to(torch.int32).contiguous()
            assert xi.shape == (batch,)
            return xi
        if n_x == batch:
            return None
        assert n_x == 1, "x must have 1 or B rows when x_index is not given"
        return torch.zeros(batch, dtype=torch.int32, device=self.device)

    # -- the U-Net -------------------------------------------------------------------------------
    def unet(self, sample, t, slots):
        """`unet(sample, t, ctx).sample` (compute.py:100) -> [B,4,h,w] in the engine's element type."""
        torch = self._torch
        sample = sample.to(self.device, self.dtype).contiguous()
        B, _, h, w = sample.shape
        t = self._timesteps(t, B)
        s = self._slots(slots, B)
        out = torch.empty(B, 4, h, w, dtype=self.dtype, device=self.device)
        self._check(self._unet_fn(self._h, _p(sample), _p(t), _p(s), B, h, w, _p(out), self._stream()), self._unet_fn.__name__)
        return out

    def dift(self, noisy, t, slots, up_ft_index: int = 1, ensemble: Optional[int] = None):
        """MyUNet2DConditionModel.forward tap (dift.py:24-169).  Returns (features [B,C,h',w'] in the engine's element type,
        ensemble mean fp32 [B/ens,C,h',w'] or None)."""
        torch = self._torch
        noisy = noisy.to(self.device, self.dtype).contiguous()
        B, _, h, w = noisy.shape
        t = self._timesteps(t, B)
        s = self._slots(slots, B)
        c, oh, ow = dift_shape(h, w, up_ft_index)
        feat = torch.empty(B, c, oh, ow, dtype=self.dtype, device=self.device)
        mean = torch.empty(B // ensemble, c, oh, ow, dtype=torch.float32, device=self.device) if ensemble else None
        self._check(self._dift_fn(self._h, _p(noisy), _p(t), _p(s), B, h, w, up_ft_index, _p(feat), _p(mean), int(ensemble or 1),
                                  self._stream()), self._dift_fn.__name__)
        return feat, mean

    # -- measurement -----------------------------------------------------------------------------
    def prof_enable(self, on: bool = True):
        self._call(self._RUN, "prof_enable", 1 if on else 0)

    def prof_read(self) -> dict:
        a, b, c2 = C.c_double(), C.c_double(), C.c_int64()
        d, e, f = C.c_double(), C.c_double(), C.c_int64()
        self._call(self._RUN, "prof_read", C.byref(a), C.byref(b), C.byref(c2), C.byref(d), C.byref(e), C.byref(f))
        return {"igemm_ms": a.value, "igemm_flops": b.value, "igemm_launches": c2.value,
                "attn_ms": d.value, "attn_flops": e.value, "attn_launches": f.value}

    def memory(self) -> dict:
        a, b = C.c_size_t(), C.c_size_t()
        self._call(self._OBJ, "memory", C.byref(a), C.byref(b))
        return {"weights_bytes": a.value, "arena_bytes": b.value}


class UNetEngine(_EngineBase):
    """The fp16 engine of the typicality path (C ABI: dm_engine_* / dm_*): fp16 weights and activations, fp32 accumulation — the
    arithmetic of the reference's autocast run (compute.py:98)."""
    _OBJ, _RUN, _DTYPE = "dm_engine_", "dm_", "float16"

    def clip_encode(self, input_ids, out_dtype=None):
        """`self.clip(tokens)[0]` (compute.py:51): input_ids [n, 77] (tokenizer output, padding="max_length")
        -> last_hidden_state [n, 77, 768] on the GPU (`out_dtype` fp32 default like `.float()`, or fp16)."""
        torch = self._torch
        out_dtype = out_dtype or torch.float32
        ids = torch.as_tensor(input_ids).to(self.device, torch.int32).contiguous()
        assert ids.dim() == 2 and ids.shape[1] == 77, ids.shape
        out = torch.empty(ids.shape[0], 77, 768, dtype=out_dtype, device=self.device)
        p16 = _p(out) if out_dtype == torch.float16 else None
        p32 = _p(out) if out_dtype == torch.float32 else None
        assert p16 or p32
        self._check(self.lib.dm_clip_encode(self._h, _p(ids), ids.shape[0], 77, p16, p32, self._stream()),
                    "dm_clip_encode")
        return out

    def load_vae_safetensors(self, path: str):
        """`vae/diffusion_pytorch_model.safetensors` of a diffusers pipeline directory."""
        from safetensors.numpy import load_file
        self.load_vae_state_dict(load_file(path))

    def vae_encode(self, image, noise=None, scaling_factor: float = 0.18215, out_dtype=None, return_moments=False,
                   draws_per_image: int = 1):
        """`vae.encode(image).latent_dist.sample() * scaling_factor` (compute.py:91-93) with the N(0,1) draw
        injected (`noise` [B*D,4,H/8,W/8], D = draws_per_image; None -> posterior mode).  image [B,3,H,W] in
        [-1,1].  Returns latents [B*D,4,H/8,W/8] (`out_dtype` fp16 default, or fp32; sample b*D+d belongs to
        image b) [, moments fp32 [B,8,H/8,W/8]].  The encoder runs once per image whatever D is."""
        torch = self._torch
        out_dtype = out_dtype or torch.float16
        image = image.to(self.device, torch.float16).contiguous()
        B, c, H, W = image.shape
        assert c == 3 and H >= 8 and W >= 8, image.shape
        h, w = H // 8, W // 8
        if noise is not None:
            noise = noise.to(self.device, torch.float16).contiguous()
            assert noise.shape == (B * draws_per_image, 4, h, w), noise.shape
        lat = torch.empty(B * draws_per_image, 4, h, w, dtype=out_dtype, device=self.device)
        mom = torch.empty(B, 8, h, w, dtype=torch.float32, device=self.device) if return_moments else None
        p16 = _p(lat) if out_dtype == torch.float16 else None
        p32 = _p(lat) if out_dtype == torch.float32 else None
        assert p16 or p32, "out_dtype must be torch.float16 or torch.float32"
        self._check(self.lib.dm_vae_encode(self._h, _p(image),
                                           _p(noise), B,
                                           int(draws_per_image), H, W, float(scaling_factor), p16, p32,
                                           _p(mom), self._stream()),
                    "dm_vae_encode")
        return (lat, mom) if return_moments else lat

    # -- text-to-image sampling (finetuning/cars.py:235-255; see diff_mining_amd.sample) ---------------------------------------------
    def load_vae_decoder_state_dict(self, sd: Dict[str, "np.ndarray"]):
        """sd: `AutoencoderKL.state_dict()`; only `post_quant_conv.*` and `decoder.*` are used (140 tensors, 49,490,199 parameters), the
        encoder half is ignored.  A weight set of its own, beside `load_vae_state_dict`.  An incomplete set is refused here, by name,
        before anything is staged."""
        from .vae_spec import canonical_vae_decoder_name, vae_decoder_tensor_spec
        have = {canonical_vae_decoder_name(k) for k in sd}
        missing = [n for n, _ in vae_decoder_tensor_spec() if n not in have]
        if missing:
            raise EngineError(f"load_vae_decoder_state_dict: {len(missing)} of the 140 decoder tensors are missing (first: {missing[0]})")
        self._load("_vae_decoder", sd)
        self._vae_decoder_ready = True

    def load_vae_decoder_safetensors(self, path: str):
        """`vae/diffusion_pytorch_model.safetensors` of a diffusers pipeline directory: its decoder half."""
        from safetensors.numpy import load_file
        self.load_vae_decoder_state_dict(load_file(path))

    def vae_decode(self, latent, raw: bool = False, want: str = "u8", scaling_factor: float = 0.18215):
        """`vae.decode(latent / scaling_factor).sample` of the pipeline under autocast.  latent [B,4,h,w] (taken as fp32).  want "u8":
        [B,8h,8w,3] uint8 = `VaeImageProcessor.postprocess` ((x / 2 + 0.5).clamp(0, 1) in fp16, * 255, rounded half to even); "f16":
        [B,3,8h,8w] fp16, the sample itself; raw=True: the pair (sample, image).  On the device."""
        torch = self._torch
        assert want in ("u8", "f16"), want
        latent = latent.to(self.device, torch.float32).contiguous()
        B, c, h, w = latent.shape
        assert c == 4, latent.shape
        f = torch.empty(B, 3, 8 * h, 8 * w, dtype=torch.float16, device=self.device) if (raw or want == "f16") else None
        u = torch.empty(B, 8 * h, 8 * w, 3, dtype=torch.uint8, device=self.device) if (raw or want == "u8") else None
        self._check(self.lib.dm_vae_decode(self._h, _p(latent), B, h, w, float(np.float32(scaling_factor)), _p(f), _p(u), self._stream()),
                    "dm_vae_decode")
        return (f, u) if raw else (u if want == "u8" else f)

    def sample_run(self, x, timesteps, coef, slots, guidance_scale: float = 7.5):
        """`len(timesteps)` guided DDIM updates of x [B,4,h,w] fp32 on the device queue (dm_sample_run): per step eps = unet(cat([x, x]), t_i,
        slots) at batch 2B, then the guided update with row i of `coef` (`sample.sample_coefficients`).  slots [2B]: the B unconditional
        prompts, then the B conditional ones.  Returns the new x (fp32, a new tensor)."""
        torch = self._torch
        x = x.to(self.device, torch.float32).contiguous().clone()
        B, c, h, w = x.shape
        assert c == 4, x.shape
        t = np.ascontiguousarray(np.asarray(timesteps, dtype=np.int64).reshape(-1))
        cf = np.ascontiguousarray(np.asarray(coef, dtype=np.float32).reshape(-1, 4))
        if cf.shape[0] != t.shape[0]:
            raise ValueError(f"{t.shape[0]} timesteps but {cf.shape[0]} coefficient rows")
        s = self._slots(slots, 2 * B)
        self._check(self.lib.dm_sample_run(self._h, _p(x), t.ctypes.data_as(C.c_void_p), cf.ctypes.data_as(C.c_void_p), _p(s), B, h, w,
                                           int(t.shape[0]), float(guidance_scale), self._stream()), "dm_sample_run")
        return x

    def resize_lanczos(self, images, out_w: int, out_h: int, resample: bool = True):
        """`PIL.Image.resize((out_w, out_h), LANCZOS)` + `to_tensor(x) * 2 - 1` (D.rescale + D.load_image, compute.py:126-132,
        165-180) of uint8 HWC RGB arrays of any sizes in ONE launch of dm_resize_lanczos -> [n,3,out_h,out_w] fp32 on the
        device, bit-equal to `load_image(img.resize(..., LANCZOS))`.  The coefficient tables are PIL's, built on the host
        (resample.lanczos_axis).  resample=False: the images already have the size; only the normalisation runs."""
        torch = self._torch
        from . import resample as RS
        imgs = [np.ascontiguousarray(a) for a in images]
        for a in imgs:
            assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3, (a.dtype, a.shape)
            assert resample or a.shape[:2] == (out_h, out_w), (a.shape, out_h, out_w)
        n = len(imgs)
        assert n >= 1 and out_w >= 1 and out_h >= 1
        desc, tables, tmp_rows = RS.resize_plan([(a.shape[1], a.shape[0]) for a in imgs], out_w, out_h)
        src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(self.device)
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(self.device)
        out = torch.empty(n, 3, out_h, out_w, dtype=torch.float32, device=self.device)
        tab_d = tmp = None
        if resample:
            tab_d = torch.from_numpy(tables).to(self.device)
            tmp = torch.empty(n * 3 * tmp_rows * out_w, dtype=torch.uint8, device=self.device)
        rc = self.lib.dm_resize_lanczos(_p(src), _p(desc_d),
                                        _p(tab_d), n, out_w, out_h, tmp_rows if resample else 0,
                                        _p(tmp), _p(out), self._stream())
        if rc:
            raise EngineError(f"dm_resize_lanczos: {'bad argument' if rc == 1 else 'HIP launch failed'} (rc {rc})")
        return out

    def load_safetensors(self, path: str, check_config: bool = True):
        """`unet/diffusion_pytorch_model.safetensors` of a diffusers pipeline directory (the format
        the reference's `--export-only` writes, finetuning/base.py:245-250).  The `config.json` next to it (the file
        `from_pretrained` builds the U-Net from, compute.py:65-70) is read first: an architecture other than SDv1.5's
        is rejected by key name (`unet_spec.check_unet_config`) instead of by a tensor-shape message later."""
        from safetensors.numpy import load_file
        cfg = os.path.join(os.path.dirname(os.path.abspath(path)), "config.json")
        if check_config and os.path.isfile(cfg):
            from .unet_spec import check_unet_config_file
            try:
                check_unet_config_file(cfg)
            except ValueError as e:
                raise EngineError(f"{cfg}: {e}") from None
        self.load_state_dict(load_file(path))

    def load_pipeline_dir(self, model_path: str, vae: bool = True, text_encoder: bool = True, vae_decoder: bool = False):
        """`StableDiffusionPipeline.from_pretrained(model_path)` as far as the path needs it (compute.py:65-73): the
        U-Net (config.json checked), and when present the VAE encoder and the CLIP text tower of the directory; with
        `vae_decoder=True` also the VAE's decoder half (`sample.sample`)."""
        unet = os.path.join(model_path, "unet", "diffusion_pytorch_model.safetensors")
        if not os.path.isfile(unet):
            raise EngineError(f"{unet} not found (a diffusers pipeline directory with safetensors weights is expected)")
        self.load_safetensors(unet)
        v = os.path.join(model_path, "vae", "diffusion_pytorch_model.safetensors")
        if vae and os.path.isfile(v):
            self.load_vae_safetensors(v)
        if vae_decoder and os.path.isfile(v):
            self.load_vae_decoder_safetensors(v)
        c = os.path.join(model_path, "text_encoder", "model.safetensors")
        if text_encoder and os.path.isfile(c):
            from safetensors.numpy import load_file
            self.load_clip_state_dict(load_file(c))

    def _latents(self, x, eps, latent_dtype):
        """x / eps in the element type the engine's add_noise and MSE run in: fp32 (the reference's flow, also
        the default for anything that is not fp16 already) or fp16 (both must then be fp16-valued)."""
        torch = self._torch
        if latent_dtype is None:
            latent_dtype = torch.float16 if (x.dtype == torch.float16 and eps.dtype == torch.float16) else torch.float32
        assert latent_dtype in (torch.float16, torch.float32), latent_dtype
        return (x.to(self.device, latent_dtype).contiguous(), eps.to(self.device, latent_dtype).contiguous(),
                1 if latent_dtype == torch.float32 else 0)

    # -- hot path --------------------------------------------------------------------------------
    def score(self, x, eps, t, slots, x_index=None, latent_dtype=None):
        """SD.compute_loss (compute.py:95-102) fused: returns loss [B,4,h,w] fp32 on the GPU.
        latent_dtype: torch.float32 (add_noise and the eps of the MSE in fp32, as the reference's autocast run) or
        torch.float16 (fp16 scheduler arithmetic); default: fp16 only if both x and eps already are fp16."""
        torch = self._torch
        x, eps, ld = self._latents(x, eps, latent_dtype)
        B, _, h, w = eps.shape
        t = t.to(self.device, torch.int64).contiguous()
        assert t.shape == (B,)
        s = self._slots(slots, B)
        xi = self._x_index(x_index, x.shape[0], B)
        out = torch.empty(B, 4, h, w, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_score(self._h, _p(x), _p(xi), _p(eps), _p(t), _p(s), B, x.shape[0], h, w, ld, _p(out),
                                      self._stream()), "dm_score")
        return out

    def score_conds(self, x, eps, t, n_cond: int, x_index=None, latent_dtype=None, slot_table=None):
        """D.compute_losses' inner call pattern: each of the U draws (x, eps, t) under n_cond prompts.
        Returns loss [n_cond*U,4,h,w] fp32, cond-major (row k*U+i).  Bit-identical to `score` on the tiled
        batch; the prompt-independent head of the U-Net runs once per draw.  latent_dtype as in `score`.
        slot_table [n_cond, U] int32 (optional): the registered prompt of draw i in its k-th condition — draws of images
        with different categories in one call (the reference's work list, compute.py:284-290); default: prompt k for every draw."""
        torch = self._torch
        x, eps, ld = self._latents(x, eps, latent_dtype)
        U, _, h, w = eps.shape
        t = t.to(self.device, torch.int64).contiguous()
        assert t.shape == (U,) and n_cond >= 2
        st = None
        if slot_table is not None:
            st = self._slots(torch.as_tensor(slot_table).reshape(-1), n_cond * U)
        else:
            assert n_cond <= self.n_prompts
        xi = self._x_index(x_index, x.shape[0], U)
        out = torch.empty(n_cond * U, 4, h, w, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_score_conds_slots(self._h, _p(x), _p(xi), _p(eps), _p(t), _p(st), n_cond, U, x.shape[0], h, w, ld,
                                                  _p(out), self._stream()), "dm_score_conds")
        return out

    def reduce_typicality(self, grid):
        """grid [N,n_cond,4,h,w] (fp32 or fp16, on the GPU) -> (map [h,w] fp32, scalar [1] fp32)."""
        torch = self._torch
        grid = grid.to(self.device).contiguous()
        assert grid.dim() == 5 and grid.shape[2] == 4
        assert grid.dtype in (torch.float16, torch.float32)
        N, nc, _, h, w = grid.shape
        m = torch.empty(h, w, dtype=torch.float32, device=self.device)
        sc = torch.empty(1, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_reduce_typicality(self._h, _p(grid),
                                                  1 if grid.dtype == torch.float16 else 0, N, nc, h, w,
                                                  _p(m), _p(sc), self._stream()),
                    "dm_reduce_typicality")
        return m, sc

    def reduce_typicality_batched(self, loss, n_images: int, n_draws: int, n_cond: int, cond_major: bool = False):
        """All images of a batch in one launch.  loss: [n_images, n_draws, n_cond, 4, h, w] (reference grids), or —
        cond_major — the [n_cond * n_images * n_draws, 4, h, w] rows `score_conds` returns for image-major draws.
        Returns (maps [n_images,h,w] fp32, scalars [n_images] fp32) on the GPU."""
        torch = self._torch
        loss = loss.to(self.device).contiguous()
        assert loss.dtype in (torch.float16, torch.float32)
        h, w = loss.shape[-2:]
        assert loss.shape[-3] == 4 and loss.numel() == n_images * n_draws * n_cond * 4 * h * w, loss.shape
        maps = torch.empty(n_images, h, w, dtype=torch.float32, device=self.device)
        sc = torch.empty(n_images, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_reduce_typicality_batched(self._h, _p(loss),
                                                          1 if loss.dtype == torch.float16 else 0, n_images, n_draws,
                                                          n_cond, h, w, 1 if cond_major else 0,
                                                          _p(maps), _p(sc),
                                                          self._stream()), "dm_reduce_typicality_batched")
        return maps, sc

    def typicality_image(self, grid, image_size, kx: int = 1, ky: int = 1):
        """`Cluster.load_typicality` (cluster.py:125-137) on the GPU: grid [N,n_cond,4,h,w] ->
        [H-kx+1, W-ky+1] fp32 = mean_N(pool(interp(mean_C L_null)) - pool(interp(mean_C L_c)));
        image_size = (H, W).  kx = ky = 1 is the X-ray per-pixel map (xray/compute.py:210-218)."""
        torch = self._torch
        grid = grid.to(self.device).contiguous()
        assert grid.dim() == 5 and grid.shape[2] == 4 and grid.dtype in (torch.float16, torch.float32)
        N, nc, _, h, w = grid.shape
        H, W = int(image_size[0]), int(image_size[1])
        work = torch.empty(h * w + H * W, dtype=torch.float32, device=self.device)
        out = torch.empty(H - kx + 1, W - ky + 1, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_typicality_image(self._h, _p(grid),
                                                 1 if grid.dtype == torch.float16 else 0, N, nc, h, w, H, W, kx, ky,
                                                 _p(work), _p(out), self._stream()),
                    "dm_typicality_image")
        return out

    def typicality_image_batched(self, grids, image_sizes, kx: int = 1, ky: int = 1):
        """`typicality_image` for a list of images in ONE call (dm_typicality_image_batched): grids[b] [N_b, n_cond_b, 4, h_b, w_b]
        (fp16 or fp32; every size may differ per image), image_sizes[b] = (H_b, W_b) -> list of maps [H_b-kx+1, W_b-ky+1] fp32 on the
        GPU, views of one packed buffer, each bit-equal to `typicality_image(grids[b], image_sizes[b], kx, ky)`.  The grids are packed
        into one buffer of one type: fp16 when all are fp16, else fp32 (the widening is exact and is what the kernel does anyway).
        The descriptor table is built with numpy and uploaded once."""
        torch = self._torch
        if len(grids) != len(image_sizes) or len(grids) < 1:
            raise ValueError(f"{len(grids)} grids but {len(image_sizes)} image sizes")
        grids = [torch.as_tensor(g) for g in grids]
        for g in grids:
            if g.dim() != 5 or g.shape[2] != 4 or g.dtype not in (torch.float16, torch.float32):
                raise ValueError(f"grid must be [N, n_cond, 4, h, w] fp16 / fp32, got {tuple(g.shape)} {g.dtype}")
        dt = torch.float16 if all(g.dtype == torch.float16 for g in grids) else torch.float32
        desc = np.zeros(len(grids), dtype=MINE_DESC_DTYPE)
        g_at = w_at = m_at = 0
        for b, (g, (H, W)) in enumerate(zip(grids, image_sizes)):
            N, nc, _, h, w = g.shape
            H, W = int(H), int(W)
            if kx < 1 or ky < 1 or kx > H or ky > W:
                raise EngineError(f"typicality_image_batched: bad window {kx}x{ky} for {H}x{W} (image {b})")
            desc[b] = (g_at, w_at, m_at, N, nc, h, w, H, W)
            g_at += g.numel()
            w_at += h * w + H * (W - ky + 1)
            m_at += (H - kx + 1) * (W - ky + 1)
        loss = torch.cat([g.to(self.device, dt).reshape(-1) for g in grids])
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(self.device)
        work = torch.empty(w_at, dtype=torch.float32, device=self.device)
        maps = torch.empty(m_at, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_typicality_image_batched(self._h, _p(loss), 1 if dt == torch.float16 else 0, _p(desc_d), len(grids),
                                                         int(kx), int(ky), _p(work), _p(maps), self._stream()),
                    "dm_typicality_image_batched")
        return _views(maps, desc, kx, ky)

    def mine_patches(self, maps, kx: int, ky: int, k_per_image: int = 5, ascending: bool = False, priority=None):
        """`sort` + `get_non_overlapping` (utils.py:82-102) on the candidate frame of `Cluster.df_D` (cluster.py:194-201), for a list
        of pooled maps [OH_b, OW_b] fp32 (`typicality_image_batched`'s output, window kx x ky) in ONE launch, one workgroup per image:
        k_per_image rounds of "take the best remaining candidate (i, j), drop every candidate with |i-i*| <= kx and |j-j*| <= ky".
        Returns (boxes [n, k, 4] int32 = (x_start, y_start, x_end, y_end) = (i, j, i+kx, j+ky) with x = rows, D [n, k] fp32,
        count [n] int32) on the GPU; slots past count[b] hold -1 / NaN (the map ran out).  ascending=True is `compute_least`'s
        order.  Ties go to the lowest row-major index; NaN keys are never chosen.  priority: optional list of maps of the same
        shapes that supply the sort key instead (D is still read from `maps`) — the ranks of a permutation give the reference's
        shuffled arm."""
        torch = self._torch
        n = len(maps)
        if n < 1:
            raise ValueError("no maps")
        k_per_image = _check_mine_args("mine_patches", k_per_image, priority, n, "maps")
        maps = [torch.as_tensor(m) for m in maps]
        for b, m in enumerate(maps):
            if m.dim() != 2 or m.numel() < 1:
                raise ValueError(f"map {b} must be [OH, OW], got {tuple(m.shape)}")
        shapes = [m.shape for m in maps]
        desc, _ = _mine_desc(shapes, kx, ky)
        packed = torch.cat([m.to(self.device, torch.float32).reshape(-1) for m in maps])
        prio = _pack_priority(torch, self.device, priority, shapes, "map")
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(self.device)
        boxes = torch.empty(n, k_per_image, 4, dtype=torch.int32, device=self.device)
        dvals = torch.empty(n, k_per_image, dtype=torch.float32, device=self.device)
        count = torch.empty(n, dtype=torch.int32, device=self.device)
        self._check(self.lib.dm_mine_patches(self._h, _p(packed), _p(prio), _p(desc_d), n, int(kx), int(ky), k_per_image,
                                             1 if ascending else 0, _p(boxes), _p(dvals), _p(count), self._stream()), "dm_mine_patches")
        return boxes, dvals, count

    @staticmethod
    def _place_maps(torch, maps, device):
        """fp32 maps for a call that addresses them as base pointer + element offsets: contiguous views of ONE buffer on
        `device` (`typicality_image_batched`'s output) stay where they lie, anything else is packed into a new buffer.
        Returns (base tensor, offsets from its first element, copied)."""
        stores = {m.untyped_storage().data_ptr() for m in maps}
        if len(stores) == 1 and all(m.dtype == torch.float32 and m.device == torch.device(device) and m.is_contiguous() for m in maps):
            lo = min(m.storage_offset() for m in maps)
            hi = max(m.storage_offset() + m.numel() for m in maps)
            base = maps[0].as_strided((hi - lo,), (1,), lo)
            return base, [m.storage_offset() - lo for m in maps], False
        base = torch.cat([m.to(device, torch.float32).reshape(-1) for m in maps])
        return base, [int(v) for v in np.cumsum([0] + [m.numel() for m in maps[:-1]])], True

    def mine_parallel(self, maps_by_group, kx: int, ky: int, k_per_image: int = 5, ascending: bool = False, priority=None):
        """`Cluster.df_PD.compute` (parallel-dataset/cluster.py:229-241) for a list of parallel groups in ONE call
        (dm_mine_parallel).  maps_by_group[g]: the n_sets pooled maps [OH_g, OW_g] fp32 of group g, one per set (country), all of
        one size; n_sets is the same for every group, 1..MINE_MAX_SETS.  Views of `typicality_image_batched`'s packed buffer are
        read in place.  Per group: the per-candidate median across the sets (`np.median(np.stack(...), axis=0)`; NaN where any
        set is NaN), `mine_patches`' selection on that median map, and every set's own value at the winners.
        Returns (boxes [G, k, 4] int32, D [G, k] fp32 = the median at the winner, set_D [G, k, n_sets] fp32, count [G] int32,
        medians: list of G maps [OH_g, OW_g] fp32), all on the GPU; slots past count[g] hold -1 / NaN.  priority: optional list
        of G maps shaped like the medians that supply the sort key (the shuffled arm), as in `mine_patches`."""
        torch = self._torch
        G = len(maps_by_group)
        if G < 1:
            raise ValueError("no groups")
        n_sets = len(maps_by_group[0])
        if n_sets < 1 or n_sets > MINE_MAX_SETS:
            raise EngineError(f"mine_parallel: n_sets {n_sets} outside [1, {MINE_MAX_SETS}]")
        if any(len(g) != n_sets for g in maps_by_group):
            raise ValueError(f"every group must hold {n_sets} maps, got {[len(g) for g in maps_by_group]}")
        k_per_image = _check_mine_args("mine_parallel", k_per_image, priority, G, "groups")
        flat = [torch.as_tensor(m) for g in maps_by_group for m in g]
        for b, m in enumerate(flat):
            if m.dim() != 2 or m.numel() < 1:
                raise ValueError(f"map {b % n_sets} of group {b // n_sets} must be [OH, OW], got {tuple(m.shape)}")
        shapes = [flat[g * n_sets].shape for g in range(G)]
        for b, m in enumerate(flat):
            if m.shape != shapes[b // n_sets]:
                raise EngineError(f"mine_parallel: set {b % n_sets} of group {b // n_sets} is {tuple(m.shape)}, "
                                  f"the group {tuple(shapes[b // n_sets])}")
        desc, _ = _mine_desc([m.shape for m in flat], kx, ky)
        gdesc, n_med = _mine_desc(shapes, kx, ky)
        packed, offsets, _ = self._place_maps(torch, flat, self.device)
        desc["map_offset"] = offsets
        prio = _pack_priority(torch, self.device, priority, shapes, "group's maps")
        up = torch.from_numpy(np.concatenate([desc, gdesc]).view(np.uint8)).to(self.device)          # both tables in one upload
        desc_d, gdesc_d = up[:desc.nbytes], up[desc.nbytes:]
        med = torch.empty(n_med, dtype=torch.float32, device=self.device)
        boxes = torch.empty(G, k_per_image, 4, dtype=torch.int32, device=self.device)
        dvals = torch.empty(G, k_per_image, dtype=torch.float32, device=self.device)
        set_d = torch.empty(G, k_per_image, n_sets, dtype=torch.float32, device=self.device)
        count = torch.empty(G, dtype=torch.int32, device=self.device)
        self._check(self.lib.dm_mine_parallel(self._h, _p(packed), _p(desc_d), G, n_sets, _p(gdesc_d), int(kx), int(ky), k_per_image,
                                              1 if ascending else 0, _p(prio), _p(med), _p(boxes), _p(dvals), _p(set_d), _p(count),
                                              self._stream()), "dm_mine_parallel")
        return boxes, dvals, set_d, count, _views(med, gdesc, kx, ky)

    NORM_MODES = {"signed": 1, "maxabs": 2, "positive": 3, "split": 4}

    def normalize_map(self, dm, mode: str = "signed"):
        """The consumers' normalisations of an image-space map (fp32, on the GPU, numpy's fp32 arithmetic): "signed" =
        `normalize(dm)` of cluster.py:32-47 as `load_typicality_norm` calls it (cluster.py:112-123); "maxabs" = `dm /
        np.max(np.abs(dm))` (`d_compute`, utils.py:130; utils.py:14-20); "positive" = positive_only=True; "split" =
        positive_only='split' (returns the pair)."""
        torch = self._torch
        dm = dm.to(self.device, torch.float32).contiguous()
        out = torch.empty_like(dm)
        neg = torch.empty_like(dm) if mode == "split" else None
        work = torch.empty(2, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_normalize_map(self._h, _p(dm), dm.numel(), self.NORM_MODES[mode],
                                              _p(work), _p(out),
                                              _p(neg), self._stream()),
                    "dm_normalize_map")
        return (out, neg) if mode == "split" else out

    def patch_embed(self, feat, boxes):
        """DIFT patch descriptors (cluster.py:291-299): feat [C,h,w] or [1,C,h,w] fp32 (the ensemble mean of
        `dift`), boxes [P,4] int = (r0, r1, c0, c1) feature cells -> [P,C] fp32, window mean then L2-normalised."""
        torch = self._torch
        feat = feat.to(self.device, torch.float32).contiguous()
        if feat.dim() == 4:
            assert feat.shape[0] == 1
            feat = feat[0]
        Cc, h, w = feat.shape
        b = torch.as_tensor(boxes, device=self.device).to(torch.int32).contiguous()
        assert b.dim() == 2 and b.shape[1] == 4, b.shape
        out = torch.empty(b.shape[0], Cc, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_patch_embed(self._h, _p(feat), Cc, h, w, _p(b),
                                            b.shape[0], _p(out), self._stream()), "dm_patch_embed")
        return out

    # -- measurement -----------------------------------------------------------------------------
    def measure_mfma_rate(self, steps: int = 20000, zero_operands: bool = False) -> dict:
        """Measurement only: TFLOP/s and shader clock the matrix cores sustain on the igemm tile's MFMA stream alone (dm_measure_mfma_rate;
        ~10 us per 100 steps).  bench.py quotes the kernel family against it beside the nominal peak."""
        tf, ghz = C.c_double(), C.c_double()
        self._check(self.lib.dm_measure_mfma_rate(self._stream(), int(steps), 1 if zero_operands else 0, C.byref(tf), C.byref(ghz)), "measure_mfma_rate")
        return {"tflops": tf.value, "sclk_ghz": ghz.value}

    def prof_read(self) -> dict:
        out = super().prof_read()
        out["igemm_flops_folded"] = 0.0
        if hasattr(self.lib, "dm_prof_read_folded"):       # (absent only from older A/B libraries loaded through DM_ENGINE_LIB)
            g = C.c_double()
            self._call("dm_", "prof_read_folded", C.byref(g))
            out["igemm_flops_folded"] = g.value
        return out

    def reserve(self, max_batch: int = 0, h: int = 0, w: int = 0, n_cond: int = 1, max_prompts: int = 0):
        """Pre-size the workspace arena for U-Net batches of up to `max_batch` samples of h x w latents (n_cond > 1: the
        `score_conds` schedule) and the K/V cache for `max_prompts` prompts: no call within those bounds allocates
        afterwards (dm_engine_reserve)."""
        self._check(self.lib.dm_engine_reserve(self._h, int(max_batch), int(h), int(w), int(n_cond), int(max_prompts),
                                               self._stream()), "dm_engine_reserve")

    def stats(self) -> dict:
        a, b, g = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.dm_engine_stats(self._h, C.byref(a), C.byref(b), C.byref(g)), "dm_engine_stats")
        return {"device_allocs": a.value, "schedule_dry_runs": b.value, "graph_launches": g.value}


class UNetEngineF32(_EngineBase):
    """The SDv1.5 U-Net in plain fp32 on the fp32 matrix cores (C ABI: dm_f32_*) — the arithmetic of the reference's DIFT
    featuriser, which loads its pipeline without torch_dtype and runs without autocast (dift.py:191,197-199).  Same
    diffusers-named state dict and prompt-slot mechanism as `UNetEngine`; every tensor at this boundary is fp32."""
    _OBJ, _RUN, _DTYPE = "dm_f32_", "dm_f32_", "float32"

    def load_safetensors(self, path: str):
        from safetensors.numpy import load_file
        self.load_state_dict(load_file(path))

    def clip_encode(self, input_ids, out_dtype=None):
        """`text_encoder(input_ids)[0]` in fp32 — `pipe.encode_prompt(prompt)[0]` of the reference's featuriser (dift.py:222-226):
        input_ids [n, 77] (tokenizer output, padding="max_length") -> last_hidden_state [n, 77, 768] fp32 on the GPU."""
        torch = self._torch
        if out_dtype not in (None, torch.float32):
            raise ValueError("the fp32 net's text tower returns fp32 hidden states")
        ids = torch.as_tensor(input_ids).to(self.device, torch.int32).contiguous()
        if ids.dim() != 2 or ids.shape[1] != 77:
            raise ValueError(f"input_ids must be [n, 77], got {tuple(ids.shape)}")
        out = torch.empty(ids.shape[0], 77, 768, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_clip_encode(self._h, _p(ids), ids.shape[0], 77, _p(out),
                                                self._stream()), "dm_f32_clip_encode")
        return out

    # -- CLIP ViT-B/32 image tower: the CLIP branch of Cluster.compute_embeddings (cluster.py:224-231, 243-310) ----------------------
    def load_clip_vision_state_dict(self, sd: Dict[str, "np.ndarray"]):
        """sd: `CLIPVisionModelWithProjection.state_dict()` or a full `CLIPModel.state_dict()` (`openai/clip-vit-base-patch32`; the text
        half, `logit_scale` and `position_ids` are skipped).  Checked against clip_spec.clip_vision_tensor_spec; kept in fp32."""
        from .clip_spec import map_clip_vision_state_dict
        try:
            canon = map_clip_vision_state_dict(sd)
        except ValueError as e:
            raise EngineError(f"CLIP vision state dict: {e}") from None
        names = {k: (k if k == "visual_projection.weight" else "vision_model." + k) for k in canon}
        self._load("_clip_vision", {names[k]: v for k, v in canon.items()})
        self._clip_vision_ready = True

    def load_clip_vision_dir(self, path: str):
        """A local `openai/clip-vit-base-patch32` (CLIPModel) or CLIPVisionModelWithProjection directory: `config.json` is checked
        (clip_spec.check_clip_vision_config), then `model.safetensors` or `pytorch_model.bin` is loaded."""
        import json
        from .clip_spec import check_clip_vision_config
        cfg = os.path.join(path, "config.json")
        if not os.path.isfile(cfg):
            raise EngineError(f"{cfg} not found")
        try:
            with open(cfg) as f:
                check_clip_vision_config(json.load(f))
        except ValueError as e:
            raise EngineError(f"{cfg}: {e}") from None
        st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
        if os.path.isfile(st):
            from safetensors.numpy import load_file
            sd = load_file(st)
        elif os.path.isfile(pt):
            sd = self._torch.load(pt, map_location="cpu", weights_only=True)
        else:
            raise EngineError(f"{path}: neither model.safetensors nor pytorch_model.bin")
        self.load_clip_vision_state_dict(sd)

    def _clip_batch(self, images, boxes):
        """Checked uint8 images on the device + the launch's descriptors and tables (resample.clip_plan)."""
        torch = self._torch
        from . import resample as RS
        if isinstance(images, np.ndarray) or hasattr(images, "convert"):
            raise TypeError("images must be a list of uint8 HWC arrays / PIL images")
        imgs = [RS.check_clip_image(a) for a in images]
        if boxes is None:
            boxes = [None] * len(imgs)
        desc, tables, owner = RS.clip_plan(imgs, boxes)
        if len(desc) == 0:
            raise ValueError("no patches")
        src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(self.device)
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(self.device)
        tab_d = torch.from_numpy(tables).to(self.device)
        return src, desc_d, tab_d, len(desc)

    def clip_preprocess(self, images, boxes=None):
        """`CLIPImageProcessor(images=[image.crop((y0, x0, y1, x1))])["pixel_values"]` (cluster.py:227) for every box of every image,
        bit-equal to it, on the device.  images: list of uint8 HWC RGB arrays or PIL images (`Cluster.load_image`'s output); boxes:
        per image a list of boxes (x_start, y_start, x_end, y_end; x = rows) or None for the whole image (None: every image whole).
        Returns pixel_values [P, 3, 224, 224] fp32 on the GPU in box order."""
        torch = self._torch
        src, desc_d, tab_d, P = self._clip_batch(images, boxes)
        out = torch.empty(P, 3, 224, 224, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_clip_preprocess(self._h, _p(src), _p(desc_d),
                                                    _p(tab_d), P, _p(out), self._stream()),
                    "dm_f32_clip_preprocess")
        return out

    def _pixel_values(self, pixel_values):
        torch = self._torch
        pv = torch.as_tensor(pixel_values).to(self.device, torch.float32).contiguous()
        if pv.dim() != 4 or tuple(pv.shape[1:]) != (3, 224, 224) or pv.shape[0] < 1:
            raise ValueError(f"pixel_values must be [n, 3, 224, 224], got {tuple(pv.shape)}")
        return pv

    def clip_image_features(self, pixel_values, normalize: bool = True):
        """`CLIPModel.get_image_features(pixel_values)` in fp32 -> [n, 512] on the GPU; normalize=True divides by the L2 norm as
        `Cluster.embed` does (cluster.py:229-230)."""
        torch = self._torch
        pv = self._pixel_values(pixel_values)
        out = torch.empty(pv.shape[0], 512, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_clip_image_features(self._h, _p(pv), pv.shape[0], int(bool(normalize)),
                                                        _p(out), self._stream()), "dm_f32_clip_image_features")
        return out

    def clip_vision_hidden(self, pixel_values):
        """The vision transformer's last_hidden_state [n, 50, 768] fp32 (before post_layernorm), for parity checks."""
        torch = self._torch
        pv = self._pixel_values(pixel_values)
        out = torch.empty(pv.shape[0], 50, 768, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_clip_vision_hidden(self._h, _p(pv), pv.shape[0], _p(out),
                                                       self._stream()), "dm_f32_clip_vision_hidden")
        return out

    def clip_patch_features(self, images, boxes, normalize: bool = True):
        """`embed(image.convert('RGB').crop(box))` (cluster.py:224-231, 308) for every box of every image in one call: preprocessing and
        tower fused (bit-equal to clip_image_features(clip_preprocess(images, boxes))) -> [P, 512] fp32 on the GPU in box order."""
        torch = self._torch
        src, desc_d, tab_d, P = self._clip_batch(images, boxes)
        out = torch.empty(P, 512, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_clip_patch_features(self._h, _p(src), _p(desc_d),
                                                        _p(tab_d), P, int(bool(normalize)), _p(out),
                                                        self._stream()), "dm_f32_clip_patch_features")
        return out


    # -- the CLIP baseline from pixels (clipmining/ranking.py:58-70): text embeddings + the configurable image tower ---------------
    def clip_text_embeds(self, input_ids, normalize: bool = True):
        """`CLIPTextModelWithProjection(input_ids).text_embeds` in fp32 -> [n, 768] on the GPU; normalize=True divides each row by
        its L2 norm (ranking.py:63).  input_ids [n, 77]: the reference tokenises with padding=True (the longest prompt), the engine
        takes 77 ids — the text tower is causal, so the pooled row (the first position of the largest id = the EOS token) does not
        see the padding behind it.  Needs `text_projection.weight` in the state dict given to load_clip_state_dict."""
        torch = self._torch
        ids = torch.as_tensor(input_ids).to(self.device, torch.int32).contiguous()
        if ids.dim() != 2 or ids.shape[1] != 77 or ids.shape[0] < 1:
            raise ValueError(f"input_ids must be [n, 77], got {tuple(ids.shape)}")
        out = torch.empty(ids.shape[0], 768, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_clip_text_embeds(self._h, _p(ids), ids.shape[0], 77, int(bool(normalize)), _p(out),
                                                     self._stream()), "dm_f32_clip_text_embeds")
        return out

    def load_clip_tower_state_dict(self, sd: Dict[str, "np.ndarray"], cfg=None):
        """The configurable image tower (default clip_spec.CLIP_L14_336_VISION = StreetCLIP's): sd = a full `CLIPModel.state_dict()`
        or `CLIPVisionModelWithProjection.state_dict()` (the text half, `logit_scale` and `position_ids` are skipped).  Checked against
        clip_spec.clip_vision_tensor_spec(cfg); kept in fp32.  A second weight set beside the ViT-B/32 tower's."""
        from .clip_spec import CLIP_L14_336_VISION, check_clip_tower_geometry, map_clip_vision_state_dict
        cfg = cfg or CLIP_L14_336_VISION
        try:
            check_clip_tower_geometry(cfg)
            canon = map_clip_vision_state_dict(sd, cfg)
        except ValueError as e:
            raise EngineError(f"CLIP tower state dict: {e}") from None
        c = (C.c_int32 * 7)(cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads, cfg.image_size,
                            cfg.patch_size, cfg.projection_dim)             # dm_clip_tower_config
        names = {k: (k if k == "visual_projection.weight" else "vision_model." + k) for k in canon}
        self._load("_clip_tower", {names[k]: v for k, v in canon.items()}, C.cast(c, C.c_void_p))
        self._clip_tower_cfg = cfg

    def load_clip_tower_dir(self, path: str, cfg=None):
        """A local `geolocal/StreetCLIP` (CLIPModel) or CLIPVisionModelWithProjection directory: `config.json` is checked against cfg
        (clip_spec.check_clip_tower_config names the offending key), then `model.safetensors` or `pytorch_model.bin` is loaded."""
        import json
        from .clip_spec import CLIP_L14_336_VISION, check_clip_tower_config
        cfg = cfg or CLIP_L14_336_VISION
        cj = os.path.join(path, "config.json")
        if not os.path.isfile(cj):
            raise EngineError(f"{cj} not found")
        try:
            with open(cj) as f:
                check_clip_tower_config(json.load(f), cfg)
        except ValueError as e:
            raise EngineError(f"{cj}: {e}") from None
        st, pt = os.path.join(path, "model.safetensors"), os.path.join(path, "pytorch_model.bin")
        if os.path.isfile(st):
            from safetensors.numpy import load_file
            sd = load_file(st)
        elif os.path.isfile(pt):
            sd = self._torch.load(pt, map_location="cpu", weights_only=True)
        else:
            raise EngineError(f"{path}: neither model.safetensors nor pytorch_model.bin")
        self.load_clip_tower_state_dict(sd, cfg)

    def _tower_cfg(self, what: str):
        cfg = getattr(self, "_clip_tower_cfg", None)
        if cfg is None:
            raise EngineError(f"{what}: CLIP tower weights not loaded (load_clip_tower_state_dict)")
        return cfg

    def _tower_batch(self, images, cfg):
        """Checked square uint8 images on the device + the call's descriptors and tables (resample.clip_tower_plan)."""
        torch = self._torch
        from . import resample as RS
        if isinstance(images, np.ndarray) or hasattr(images, "convert"):
            raise TypeError("images must be a list of uint8 HWC arrays / PIL images")
        imgs = [RS.check_clip_tower_image(a) for a in images]
        if not imgs:
            raise ValueError("no images")
        desc, tables = RS.clip_tower_plan(imgs, cfg.image_size)
        src = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(self.device)
        desc_d = torch.from_numpy(desc.view(np.uint8)).to(self.device)
        tab_d = torch.from_numpy(tables).to(self.device)
        return src, desc_d, tab_d, len(imgs)

    def clip_tower_preprocess(self, images):
        """`CLIPImageProcessor(size={"shortest_edge": S}, do_center_crop=False)(images=image)["pixel_values"]` (ranking.py:66) for a
        list of SQUARE uint8 HWC RGB arrays / PIL images (the reference center-crops to 512 x 512 first: clipmine.center_crop), bit-equal
        to it, on the device -> [n, 3, S, S] fp32.  Anything non-square raises ValueError."""
        torch = self._torch
        cfg = self._tower_cfg("clip_tower_preprocess")
        src, desc_d, tab_d, n = self._tower_batch(images, cfg)
        out = torch.empty(n, 3, cfg.image_size, cfg.image_size, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_clip_tower_preprocess(self._h, _p(src), _p(desc_d), _p(tab_d), n, 0, _p(out), self._stream()),
                    "dm_f32_clip_tower_preprocess")
        return out

    def clip_patch_tokens(self, pixel_values, return_hidden: bool = False):
        """`visual_projection(post_layernorm(vision_model(pixel_values).last_hidden_state[:, 1:, :]))` (ranking.py:66-70) in fp32:
        pixel_values [n, 3, S, S] -> tokens [n, G^2, projection_dim] on the GPU (every patch token, CLS dropped); return_hidden adds
        last_hidden_state [n, G^2 + 1, hidden]."""
        torch = self._torch
        cfg = self._tower_cfg("clip_patch_tokens")
        S, g2 = cfg.image_size, (cfg.image_size // cfg.patch_size) ** 2
        pv = torch.as_tensor(pixel_values).to(self.device, torch.float32).contiguous()
        if pv.dim() != 4 or tuple(pv.shape[1:]) != (3, S, S) or pv.shape[0] < 1:
            raise ValueError(f"pixel_values must be [n, 3, {S}, {S}], got {tuple(pv.shape)}")
        tok = torch.empty(pv.shape[0], g2, cfg.projection_dim, dtype=torch.float32, device=self.device)
        hid = torch.empty(pv.shape[0], g2 + 1, cfg.hidden_size, dtype=torch.float32, device=self.device) if return_hidden else None
        self._check(self.lib.dm_f32_clip_tower_tokens(self._h, _p(pv), pv.shape[0], _p(tok), _p(hid), self._stream()),
                    "dm_f32_clip_tower_tokens")
        return (tok, hid) if return_hidden else tok

    def clip_image_tokens(self, images):
        """clip_patch_tokens(clip_tower_preprocess(images)) fused — the preprocessing writes the patch rows of the embedding GEMM —
        and bit-equal to it: square uint8 images -> [n, G^2, projection_dim] fp32 on the GPU."""
        torch = self._torch
        cfg = self._tower_cfg("clip_image_tokens")
        src, desc_d, tab_d, n = self._tower_batch(images, cfg)
        tok = torch.empty(n, (cfg.image_size // cfg.patch_size) ** 2, cfg.projection_dim, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_clip_tower_image_tokens(self._h, _p(src), _p(desc_d), _p(tab_d), n, _p(tok), self._stream()),
                    "dm_f32_clip_tower_image_tokens")
        return tok

    def vae_encode(self, image, noise=None, scaling_factor: float = 0.18215, return_moments=False, draws_per_image: int = 1):
        """`vae.encode(image).latent_dist.sample() * scaling_factor` in fp32 (dift.py:187) with the N(0,1) draw injected (`noise`
        [B*D,4,H/8,W/8]; None -> posterior mode).  image [B,3,H,W] in [-1,1].  Returns latents [B*D,4,H/8,W/8] fp32 [, moments
        fp32 [B,8,H/8,W/8]]; the encoder runs once per image whatever D is."""
        torch = self._torch
        image = image.to(self.device, torch.float32).contiguous()
        B, c, H, W = image.shape
        assert c == 3 and H >= 8 and W >= 8, image.shape
        h, w = H // 8, W // 8
        if noise is not None:
            noise = noise.to(self.device, torch.float32).contiguous()
            assert noise.shape == (B * draws_per_image, 4, h, w), noise.shape
        lat = torch.empty(B * draws_per_image, 4, h, w, dtype=torch.float32, device=self.device)
        mom = torch.empty(B, 8, h, w, dtype=torch.float32, device=self.device) if return_moments else None
        self._check(self.lib.dm_f32_vae_encode(self._h, _p(image), _p(noise),
                                               B, int(draws_per_image), H, W, float(scaling_factor), _p(lat),
                                               _p(mom), self._stream()), "dm_f32_vae_encode")
        return (lat, mom) if return_moments else lat

    # -- the parallel-dataset generator (applications/parallel-dataset/pnp.py; see diff_mining_amd.pnp) ------------------------------
    def load_vae_decoder_state_dict(self, sd: Dict[str, "np.ndarray"]):
        """sd: `AutoencoderKL.state_dict()`; only `post_quant_conv.*` and `decoder.*` are used (140 tensors), the encoder half is
        ignored.  A weight set of its own, beside `load_vae_state_dict`."""
        self._load("_vae_decoder", sd)
        self._vae_decoder_ready = True

    def vae_decode(self, latent, raw: bool = False, want: str = "f32", latent_scale=None):
        """`vae.decode(1 / 0.18215 * latent).sample` in fp32 (pnp.py:137-142, :531-536).  latent [B,4,h,w].  want "f32": [B,3,8h,8w]
        fp32, the sample if `raw`, else `(sample / 2 + 0.5).clamp(0, 1)`; "u8": [B,8h,8w,3] uint8 = that image * 255 truncated
        (`pilify`, pnp.py:590-591); "both": the pair."""
        torch = self._torch
        assert want in ("f32", "u8", "both"), want
        latent = latent.to(self.device, torch.float32).contiguous()
        B, c, h, w = latent.shape
        assert c == 4, latent.shape
        scale = np.float32(1 / 0.18215) if latent_scale is None else np.float32(latent_scale)      # fp32 tensor * Python scalar
        f = torch.empty(B, 3, 8 * h, 8 * w, dtype=torch.float32, device=self.device) if want != "u8" else None
        u = torch.empty(B, 8 * h, 8 * w, 3, dtype=torch.uint8, device=self.device) if want != "f32" else None
        self._check(self.lib.dm_f32_vae_decode(self._h, _p(latent), B, h, w, float(scale), int(bool(raw)), _p(f), _p(u), self._stream()),
                    "dm_f32_vae_decode")
        return f if want == "f32" else u if want == "u8" else (f, u)

    def unet_inject(self, sample, t, slots, conv_mask: int = 0, attn_mask: int = 0):
        """One U-Net forward with Plug-and-Play's injection (pnp.py:345-350, :424-432): sample [1 + n,4,h,w], row 0 the source.  Masks as
        `pnp.injection_plan` gives them; masks of 0 = `unet`."""
        torch = self._torch
        sample = sample.to(self.device, torch.float32).contiguous()
        B, _, h, w = sample.shape
        t = self._timesteps(t, B)
        s = self._slots(slots, B)
        out = torch.empty(B, 4, h, w, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_unet_forward_inject(self._h, _p(sample), _p(t), _p(s), B, h, w, int(conv_mask), int(attn_mask), _p(out),
                                                        self._stream()), "dm_f32_unet_forward_inject")
        return out

    @staticmethod
    def _loop_tables(timesteps, coef):
        t = np.ascontiguousarray(np.asarray(timesteps, dtype=np.int64).reshape(-1))
        c = np.ascontiguousarray(np.asarray(coef, dtype=np.float32).reshape(-1, 4))
        if c.shape[0] != t.shape[0]:
            raise ValueError(f"{t.shape[0]} timesteps but {c.shape[0]} coefficient rows")
        return t, c

    def ddim_run(self, x, timesteps, coef, slots, save_rows=None, n_rows: int = 0):
        """`len(timesteps)` DDIM updates of x [B,4,h,w] on the device queue (pnp.py:156-203): eps = unet(x, t_i, slots), then
        x = c0 * ((x - c1 * eps) / c2) + c3 * eps with row i of `coef` (`pnp.ddim_coefficients`).  save_rows [n] (-1: not kept) names the
        row of the returned trajectory [n_rows,B,4,h,w] that keeps the x after step i.  Returns (x, trajectory or None); x is a new
        tensor."""
        torch = self._torch
        x = x.to(self.device, torch.float32).contiguous().clone()
        B, _, h, w = x.shape
        t, c = self._loop_tables(timesteps, coef)
        s = self._slots(slots, B)
        save = traj = None
        if save_rows is not None:
            save = np.ascontiguousarray(np.asarray(save_rows, dtype=np.int32).reshape(-1))
            if save.shape[0] != t.shape[0] or (save.size and int(save.max()) >= n_rows):
                raise ValueError("save_rows must hold one row index below n_rows (or -1) per step")
            traj = torch.zeros(max(n_rows, 1), B, 4, h, w, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_ddim_run(self._h, _p(x), t.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), _p(s),
                                             save.ctypes.data_as(C.c_void_p) if save is not None else None, _p(traj), B, h, w, int(t.shape[0]),
                                             self._stream()), "dm_f32_ddim_run")
        return x, traj

    def pnp_run(self, x, source, timesteps, coef, conv_on, attn_on, conv_mask: int, attn_mask: int, slots, guidance_scale: float = 7.5):
        """Plug-and-Play sampling (pnp.py:538-577) of B targets x [B,4,h,w] of one source: source [n,4,h,w] = its latent at
        timesteps[i]; slots [1 + 2B] = (source, B unconditional, B conditional prompts).  Returns the new x."""
        torch = self._torch
        x = x.to(self.device, torch.float32).contiguous().clone()
        B, _, h, w = x.shape
        t, c = self._loop_tables(timesteps, coef)
        n = int(t.shape[0])
        source = source.to(self.device, torch.float32).contiguous()
        assert source.shape == (n, 4, h, w), (source.shape, (n, 4, h, w))
        on_c = np.ascontiguousarray(np.asarray(conv_on, dtype=np.uint8).reshape(-1))
        on_a = np.ascontiguousarray(np.asarray(attn_on, dtype=np.uint8).reshape(-1))
        assert on_c.shape == (n,) and on_a.shape == (n,), (on_c.shape, on_a.shape, n)
        s = self._slots(slots, 1 + 2 * B)
        self._check(self.lib.dm_f32_pnp_run(self._h, _p(x), _p(source), t.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                                            on_c.ctypes.data_as(C.c_void_p), on_a.ctypes.data_as(C.c_void_p), int(conv_mask), int(attn_mask), _p(s),
                                            B, h, w, n, float(guidance_scale), self._stream()), "dm_f32_pnp_run")
        return x

    def score(self, x, eps, t, slots, x_index=None):
        """SD.compute_loss (compute.py:95-102) with no autocast: fp32 add_noise, fp32 U-Net, fp32 squared error -> [B,4,h,w] fp32.
        The exact-arithmetic yardstick of `UNetEngine.score`."""
        torch = self._torch
        x = x.to(self.device, torch.float32).contiguous()
        eps = eps.to(self.device, torch.float32).contiguous()
        B, _, h, w = eps.shape
        t = self._timesteps(t, B)
        s = self._slots(slots, B)
        xi = self._x_index(x_index, x.shape[0], B)
        out = torch.empty(B, 4, h, w, dtype=torch.float32, device=self.device)
        self._check(self.lib.dm_f32_score(self._h, _p(x), _p(xi), _p(eps), _p(t), _p(s), B, x.shape[0], h, w, _p(out), self._stream()),
                    "dm_f32_score")
        return out

    def score_conds(self, x, eps, t, n_cond: int, x_index=None, latent_dtype=None, slot_table=None):
        """Each of the U draws (x, eps, t) under n_cond prompts -> loss [n_cond*U,4,h,w] fp32, cond-major (row k*U+i), like
        `UNetEngine.score_conds` — the same keywords, so `TypicalityScorer.compute_losses_batch` / `compute_submission` run on either
        engine: `slot_table` [n_cond, U] = the registered prompt of draw i in its k-th condition (default: prompt k for
        every draw); `latent_dtype` must be None or float32 (this net has one dtype flow: everything fp32)."""
        torch = self._torch
        if latent_dtype not in (None, torch.float32):
            raise ValueError("UNetEngineF32.score_conds: the fp32 net has no fp16 latent flow (latent_dtype must be None or torch.float32)")
        U = eps.shape[0]
        t = torch.as_tensor(t).reshape(-1)
        xi = None if x_index is None else torch.as_tensor(x_index).reshape(-1).repeat(n_cond)
        xx = x if (x.shape[0] == 1 or x_index is not None) else x.repeat(n_cond, 1, 1, 1)
        if slot_table is not None:
            slots = torch.as_tensor(slot_table).to(torch.int32).reshape(-1)
            if slots.numel() != n_cond * U:
                raise ValueError(f"slot_table must hold n_cond * U = {n_cond * U} entries, got {slots.numel()}")
        else:
            slots = torch.arange(n_cond, dtype=torch.int32).repeat_interleave(U)
        return self.score(xx, eps.repeat(n_cond, 1, 1, 1), t.repeat(n_cond), slots, x_index=xi)
