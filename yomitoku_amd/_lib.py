"""ctypes binding of libymk_hip.so (the C ABI declared in include/ymk.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C yomitoku_amd/csrc``.
There is no CPU fallback: if the shared object is missing or a call fails, this module raises.
"""

from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libymk_hip.so")

# name -> (restype, argtypes); kept in one table so tests can check every symbol of ymk.h exists
SIGNATURES = {
    "ymk_version": (c_int, []),
    "ymk_last_error": (c_char_p, []),
    "ymk_device_count": (c_int, []),
    "ymk_model_create": (c_void_p, [c_char_p, c_int]),
    "ymk_model_destroy": (None, [c_void_p]),
    "ymk_model_set_param": (c_int, [c_void_p, c_char_p, c_double]),
    "ymk_model_set_tensor": (c_int, [c_void_p, c_char_p, c_void_p, c_int, POINTER(c_int64)]),
    "ymk_model_finalize": (c_int, [c_void_p]),
    "ymk_model_reserve": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p]),
    "ymk_op_plan_workspace": (c_int, [c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
    "ymk_model_weight_bytes": (c_int64, [c_void_p]),
    "ymk_model_workspace_bytes": (c_int64, [c_void_p]),
    "ymk_dbnet_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_parseq_dims": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int)]),
    "ymk_parseq_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, POINTER(c_int), POINTER(c_int), c_void_p]),
    "ymk_parseq_forward_groups": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_int), POINTER(c_int), c_int, c_void_p, POINTER(c_int),
                                          POINTER(c_int), c_void_p]),
    "ymk_parseq_token_stats": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ymk_rtdetr_forward": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ymk_det_preprocess": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_pil_resize_to_chw": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p,
         c_void_p],
    ),
    "ymk_pil_resize_batch_to_chw": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_pil_batch_record_words": (c_int, []),
    "ymk_crop_batch": (
        c_int,
        [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p],
    ),
    "ymk_crop_batch_levels": (
        c_int,
        [c_void_p, POINTER(c_int), POINTER(c_int), c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int,
         c_void_p],
    ),
    "ymk_halve_u8c3": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "ymk_crop_desc_size": (c_int, []),
    "ymk_draw_overlay": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int64, c_void_p]),
    "ymk_heatmap_blend": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ymk_overlay_tile": (c_int, []),
    "ymk_overlay_chunk": (c_int, []),
    "ymk_overlay_layout": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p]),
    "ymk_draw_overlay_pages": (c_int, [c_void_p, c_int64, c_void_p, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "ymk_overlay_cull_pass": (c_int, []),
    "ymk_jpeg_page_words": (c_int, []),
    "ymk_jpeg_quant_tables": (c_int, [c_int, POINTER(c_int)]),
    "ymk_jpeg_header": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int]),
    "ymk_jpeg_scratch_bytes": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, POINTER(c_int64)]),
    "ymk_jpeg_coefficients": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_int64, c_void_p]),
    "ymk_jpeg_entropy": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "ymk_jpeg_compact": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                 c_void_p]),
    "ymk_jpeg_encode_pages": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                      c_void_p, c_int64, c_void_p, c_void_p]),
    "ymk_jpeg_header_opt": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_int, POINTER(c_int)]),
    "ymk_jpeg_scratch_bytes_opt": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, POINTER(c_int64)]),
    "ymk_jpeg_histogram": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "ymk_jpeg_optimal_tables": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ymk_jpeg_entropy_opt": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                     c_void_p]),
    "ymk_jpeg_compact_opt": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                                     c_int64, c_void_p, c_void_p]),
    "ymk_jpeg_encode_pages_opt": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "ymk_jpeg_header_mode": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int]),
    "ymk_jpeg_header_opt_mode": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, POINTER(c_int)]),
    "ymk_jpeg_scratch_bytes_mode": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, POINTER(c_int64)]),
    "ymk_jpeg_scratch_bytes_opt_mode": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int,
                                                POINTER(c_int64)]),
    "ymk_jpeg_pages_grey": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p]),
    "ymk_g4_page_words": (c_int, []),
    "ymk_g4_slot_words": (c_int, [c_int]),
    "ymk_g4_file_capacity": (c_int64, [c_int, c_int]),
    "ymk_g4_scratch_bytes": (c_int, [POINTER(c_int), POINTER(c_int), c_int, POINTER(c_int64)]),
    "ymk_g4_test_pack": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "ymk_g4_code_rows": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "ymk_g4_scan": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "ymk_g4_concat": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                              c_void_p]),
    "ymk_g4_encode_pages": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                                    c_int64, c_int64, c_void_p, c_void_p]),
    "ymk_flate_page_words": (c_int, []),
    "ymk_flate_file_capacity": (c_int64, [c_int, c_int, c_int]),
    "ymk_flate_scratch_bytes": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, POINTER(c_int64)]),
    "ymk_flate_rows": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "ymk_flate_tables": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "ymk_flate_code": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "ymk_flate_scan": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p]),
    "ymk_flate_gather": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int64, c_void_p]),
    "ymk_flate_encode_pages": (c_int, [c_void_p, c_int64, c_int, c_int, c_int64, c_int64, c_int64, c_int64, c_int, c_int, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_int64, c_void_p, c_void_p]),
    "ymk_bin_scratch_bytes": (c_int, [POINTER(c_int), POINTER(c_int), c_int, POINTER(c_int64)]),
    "ymk_bin_test_hist": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "ymk_bin_otsu": (c_int, [c_int, c_void_p, c_void_p, c_void_p]),
    "ymk_bin_otsu_pack": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "ymk_bin_adaptive_pack": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "ymk_dsk_page_words": (c_int, []),
    "ymk_dsk_check_angles": (c_int, [POINTER(c_int), c_int, POINTER(c_int)]),
    "ymk_dsk_scratch_bytes": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, c_int, c_int, POINTER(c_int64), POINTER(c_int)]),
    "ymk_dsk_luma": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "ymk_dsk_scores": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ymk_dsk_choose": (c_int, [c_void_p, c_int64, c_int, c_int64, c_int64, c_int64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_dsk_rotate": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p, c_int, c_void_p, c_void_p]),
    "ymk_dsk_pages": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                              c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "ymk_mrc_page_words": (c_int, []),
    "ymk_mrc_scratch_bytes": (c_int, [POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, c_int, c_int, POINTER(c_int64), POINTER(c_int64)]),
    "ymk_mrc_cells": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64, c_void_p]),
    "ymk_mrc_pull": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int64, c_void_p, c_int64, c_int64, c_void_p]),
    "ymk_mrc_push": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                             c_void_p]),
    "ymk_mrc_pages": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                              c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "ymk_cc_tile_w": (c_int, []),
    "ymk_cc_tile_h": (c_int, []),
    "ymk_cc_scratch_bytes": (c_int, [POINTER(c_int), POINTER(c_int), c_int, POINTER(c_int64)]),
    "ymk_cc_despeckle_pages": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int,
                                       c_int, c_void_p, c_void_p]),
    "ymk_cc_stage": (c_int, [c_int, c_int, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int,
                             c_void_p, c_void_p]),
    "ymk_cc_filter_scratch_bytes": (c_int, [POINTER(c_int), POINTER(c_int), c_int, POINTER(c_int64)]),
    "ymk_cc_filter_pages": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                    c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_cc_filter_stage": (c_int, [c_int, c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                                    c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "ymk_pil_resize_u8_record_words": (c_int, []),
    "ymk_pil_resize_u8": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_void_p]),
    "ymk_crop_u8_record_words": (c_int, []),
    "ymk_crop_u8": (c_int, [c_void_p, c_int64, c_int, c_int64, c_void_p]),
    "ymk_db_postprocess": (
        c_int,
        [c_void_p, c_int, c_int, c_float, c_float, c_int, c_int, c_float, c_int, c_int, c_void_p, c_void_p, c_int,
         POINTER(c_int)],
    ),
    "ymk_table_hole_rects": (c_int, [c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, POINTER(c_int)]),
    "ymk_debug_option": (c_int, [c_char_p, c_int]),
    "ymk_stat": (c_int, [c_char_p, POINTER(c_int64)]),
    "ymk_op_vit_mlp": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, POINTER(c_float), c_void_p],
    ),
    "ymk_amax_check_counters": (c_int, [POINTER(c_int64)]),
    "ymk_prof_begin": (c_int, []),
    "ymk_prof_end": (c_int, [POINTER(c_double), POINTER(c_double), POINTER(c_int64)]),
    "ymk_prof_bytes": (c_int, [POINTER(c_double)]),
    "ymk_prof_launch_table": (c_int, [POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int64, POINTER(c_int64)]),
    "ymk_op_conv2d": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p,
         c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    ),
    "ymk_op_conv2d_view": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
         c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p],
    ),
    "ymk_op_conv_planes_pair": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_int, c_void_p]
        + [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p] * 2
        + [c_void_p, c_void_p, c_void_p, POINTER(c_int), POINTER(c_float), POINTER(c_float), c_void_p],
    ),
    "ymk_op_conv1x1_astat": (
        c_int,
        [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int,
         POINTER(c_float), c_void_p],
    ),
    "ymk_op_layernorm": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_void_p]),
    "ymk_op_attention": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_int,
         c_void_p],
    ),
    "ymk_op_nar_cross_attention": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p, c_void_p],
    ),
    "ymk_op_layernorm_view": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_float, c_void_p, c_int, c_void_p]),
    "ymk_op_attention_view": (
        c_int,
        [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, c_int, c_int,
         c_int64, c_int64, c_int64, c_int64, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
         c_void_p, c_void_p, c_void_p],
    ),
    "ymk_op_maxpool3x3s2": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_op_upsample_bilinear": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p],
    ),
    "ymk_op_topk_tokens": (c_int, [c_void_p, c_int, POINTER(c_int), c_int, c_int, c_void_p, c_void_p]),
    "ymk_op_gather_queries": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int, POINTER(c_int), c_int, c_int, c_void_p, c_void_p, c_void_p],
    ),
    "ymk_op_refine_boxes": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "ymk_op_mask_rows": (c_int, [c_void_p, c_void_p, c_int, POINTER(c_int), c_int, c_void_p, c_void_p]),
    "ymk_op_deform_sample": (
        c_int,
        [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, POINTER(c_int), c_int, c_void_p, c_void_p],
    ),
    "ymk_op_avgpool2x2_ceil": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_op_upsample_nearest2x": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_op_maxpool3x3s2_view": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "ymk_op_avgpool2x2_ceil_view": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "ymk_op_upsample_nearest2x_view": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "ymk_op_upsample_bilinear_view": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p],
    ),
    "ymk_op_nchw3_to_nhwc4": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_op_add_bcast": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "ymk_op_absmax": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "ymk_op_amax_merge": (c_int, [c_void_p, c_void_p, c_void_p]),
    "ymk_op_deconv2x2": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p],
    ),
    "ymk_op_deconv2x2_to1_sigmoid": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_float, c_void_p, c_void_p]),
    "ymk_op_dbnet_asf": (
        c_int,
        [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_float, c_void_p, c_void_p, c_void_p],
    ),
    "ymk_op_parseq_dec_step": (
        c_int,
        [c_int, c_int, c_int] + [c_void_p] * 12 + [POINTER(c_void_p), c_void_p, c_int, c_void_p, c_void_p]
        + [c_void_p] * 8 + [c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    ),
    "ymk_op_greedy_step": (
        c_int,
        [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
         c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p],
    ),
    "ymk_op_greedy_step_retire": (
        c_int,
        [c_void_p, c_int64, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p,
         c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p],
    ),
    "ymk_op_parseq_dec_step_state": (
        c_int,
        [c_int, c_int, c_int] + [c_void_p] * 12 + [POINTER(c_void_p), c_void_p, c_int, c_void_p, c_void_p]
        + [c_void_p] * 8 + [c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p],
    ),
    "ymk_op_rowmax_head": (
        c_int,
        [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p],
    ),
    "ymk_op_refine_prep": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "ymk_op_rep_cut": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "ymk_op_row_argmax": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "ymk_op_ctx_embed_ln": (
        c_int,
        [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_int, c_int, c_int, c_void_p],
    ),
    "ymk_op_init_decode": (c_int, [c_void_p, c_int, c_void_p, c_int, c_int, c_int, c_void_p]),
    "ymk_op_tile_rows": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p]),
    "ymk_op_add_pos_embed": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
}

_lib = None


class YmkError(RuntimeError):
    pass


def load():
    """Load libymk_hip.so once; raises YmkError when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise YmkError(
            f"{LIB_PATH} not found - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C yomitoku_amd/csrc` (there is no CPU fallback)"
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    # evaluation switches for a whole process (include/ymk.h: ymk_debug_option): YMK_CONV_SPLIT=2 is short for
    # YMK_DEBUG_OPTIONS="conv_split=2"; several options are comma separated
    spec = os.environ.get("YMK_DEBUG_OPTIONS", "")
    if os.environ.get("YMK_CONV_SPLIT"):
        spec += ",conv_split=" + os.environ["YMK_CONV_SPLIT"]
    if os.environ.get("YMK_WORKSPACE_REUSE"):  # planned workspaces for every model that does not say otherwise itself
        spec += ",workspace_reuse=" + os.environ["YMK_WORKSPACE_REUSE"]
    for item in filter(None, (x.strip() for x in spec.split(","))):
        key, _, value = item.partition("=")
        if lib.ymk_debug_option(key.strip().encode(), int(value)) != 0:
            raise YmkError(f"YMK_DEBUG_OPTIONS ({item}): " + lib.ymk_last_error().decode("utf-8", "replace"))
    return lib


def check(status: int, what: str = "ymk call"):
    if status != 0:
        msg = load().ymk_last_error()
        raise YmkError(f"{what} failed: {msg.decode('utf-8', 'replace') if msg else status}")


CONV_FAST_DEFAULT = 27  # ymk_debug_option("conv_fast"): the library's default bits (include/ymk.h)


def stat(key: str) -> int:
    """A launch counter of the library (include/ymk.h: ymk_stat)."""
    v = c_int64()
    check(load().ymk_stat(key.encode(), ctypes.byref(v)), f"ymk_stat({key})")
    return int(v.value)


def debug_option(key: str, value: int):
    """Test / measurement knob of the library (include/ymk.h: ymk_debug_option)."""
    check(load().ymk_debug_option(key.encode(), int(value)), f"ymk_debug_option({key})")


def plan_workspace(sizes, release_pos):
    """(offsets, peak, live_bound) of the workspace planner on a trace (include/ymk.h: ymk_op_plan_workspace; host only)."""
    n = len(sizes)
    arr = c_int64 * max(1, n)
    off, peak, live = arr(), c_int64(), c_int64()
    check(load().ymk_op_plan_workspace(n, arr(*[int(v) for v in sizes]), arr(*[int(v) for v in release_pos]), off,
                                       ctypes.byref(peak), ctypes.byref(live)), "ymk_op_plan_workspace")
    return [int(off[i]) for i in range(n)], int(peak.value), int(live.value)


def amax_check_counters():
    """(launches checked, records below the true max|x|, records > 2^8 above it, largest exponent distance) of the
    ymk_debug_option("amax_check", 1) self-check (include/ymk.h)."""
    import ctypes

    out = (ctypes.c_int64 * 4)()
    check(load().ymk_amax_check_counters(out), "ymk_amax_check_counters")
    return tuple(int(v) for v in out)


def prof_launch_table():
    """[(ms, flop, bytes, mfma_products)] of the launches between the last ymk_prof_begin / ymk_prof_end (include/ymk.h)."""
    import ctypes

    lib, n = load(), ctypes.c_int64()
    check(lib.ymk_prof_launch_table(None, None, None, None, 0, ctypes.byref(n)), "ymk_prof_launch_table")
    cols = [(ctypes.c_double * max(1, n.value))() for _ in range(4)]
    check(lib.ymk_prof_launch_table(*cols, n.value, ctypes.byref(n)), "ymk_prof_launch_table")
    return [tuple(float(c[i]) for c in cols) for i in range(n.value)]


def ptr(t):
    """Device/host address of a torch tensor (must be contiguous) or None."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return t.data_ptr()


def current_stream_ptr():
    import torch

    return torch.cuda.current_stream().cuda_stream


def dims_array(shape):
    arr = (c_int64 * max(1, len(shape)))(*[int(s) for s in shape])
    return arr
