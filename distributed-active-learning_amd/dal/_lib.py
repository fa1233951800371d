"""ctypes binding of libdal.so (the C ABI declared in include/dal.h).

The library is built in-tree (``make -C distributed-active-learning_amd/csrc``
or ``__graft_entry__.build()``) and loaded from this directory.  There is no
fallback: if the library is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_double, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdal.so")

# constants mirrored from include/dal.h
DAL_OK = 0
DAL_FLAG_ZERO_NORM = 1
DAL_FLAG_CAND_OVERFLOW = 2
DAL_FLAG_RF_SPLITS = 4
DAL_FLAG_SAMPLE_MISS = 8
DAL_FLAG_NONFINITE = 16
DAL_ROW_CANDIDATE = 1
DAL_ROW_EXCLUDED = 2
DAL_DENSITY_NONE = 0
DAL_DENSITY_FIXED = 1
DAL_DENSITY_EXACT = 2
DAL_ASCENDING = 0
DAL_DESCENDING = 1
DAL_KEY_NAN = 0xFFFFFFFFFFFFFFFE
DAL_KEY_NONE = 0xFFFFFFFFFFFFFFFF
DAL_FIXED_SCALE = 4294967296.0
DAL_ROW_GRANULE = 512
DAL_CANON_CHUNK = 256
DAL_DOWNDATE_MAX_ROWS = 1024
DAL_DOWNDATE_TILE = 64
DAL_MAX_TREE_DEPTH = 16
DAL_SORT_CAP = 8192
DAL_SORT_CAP_PAYLOAD = 4096
DAL_STEP_RESET_STATUS = 1
DAL_STEP_WS_CLEAN = 2
DAL_STEP_KEEP_GROUPS = 4
DAL_STEP_SELECT_ONLY = 8
DAL_RF_MAX_SPLITS = 255
DAL_RF_MAX_SPLIT_SAMPLE = 16384
DAL_RF_MAX_DEPTH = 10
DAL_RF_SPLIT_LDS_BYTES = 163840
DAL_MC_MAX_CLASSES = 32
DAL_MC_MAX_TREES = 255
DAL_MC_LEAST_CONFIDENCE = 0
DAL_MC_MARGIN = 1
DAL_MC_ENTROPY = 2
DAL_REG_MAX_DEPTH = 10
DAL_X_F32 = 0
DAL_X_F64 = 1
DAL_LAL_MAX_TREES = 4095
DAL_RF_REG_MAX_LIMBS = 8
DAL_RF_MAX_SPLIT_SAMPLE_F64 = 8192
DAL_RF_JOB_BYTES = 512
DAL_RF_SPAN_I32 = 0
DAL_RF_SPAN_I64 = 1
DAL_ROW_PICKED = 4
DAL_KCENTER_JOB_BYTES = 512
DAL_SOFT_MAX_DEPTH = 16
DAL_SOFT_MAX_CLASSES = 32
DAL_SOFT_MAX_TREES = 255
DAL_SOFT_ONE = 1 << 31
DAL_SOFT_LEAST_CONFIDENCE = 0
DAL_SOFT_MARGIN = 1
DAL_SOFT_ENTROPY = 2
DAL_SOFT_ENTROPY_SHIFT = 29


def kcenter_record_bytes(d: int) -> int:
    """DAL_KCENTER_RECORD_BYTES(d): key, index, value, one reserved word, d bf16 values."""
    return 32 + 2 * int(d)


# name -> (restype, argtypes); every symbol of include/dal.h
SIGNATURES = {
    "dal_status_string": (ctypes.c_char_p, [c_int]),
    "dal_abi_version": (c_int, []),
    "dal_pad_rows": (c_int64, [c_int64]),
    "dal_pad_features": (c_int64, [c_int64]),
    "dal_density_error_bound": (c_double, [c_int64]),
    "dal_normalize_rows": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                   c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_mark_rows_count": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "dal_mark_rows": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "dal_canon_colsum_partials": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                          c_void_p, c_void_p]),
    "dal_canon_colsum_reduce": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "dal_canon_colsum_partials_chunks": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                                 c_void_p, c_int64, c_void_p, c_void_p]),
    "dal_density_downdate_error_bound": (c_double, [c_int64, c_int64]),
    "dal_density_downdate": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_int, c_void_p]),
    "dal_gram_rowsum": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                c_int, c_void_p]),
    "dal_split_f16_halves": (c_int64, [c_int64, c_int64]),
    "dal_split_f16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "dal_prep_split": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_prep_split_fp4_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "dal_prep_split_fp4": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int64,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_size_t, c_void_p, c_void_p]),
    "dal_gram_sym_residual_fp4_pre": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_size_t, c_void_p]),
    "dal_density_error_bound_sym": (c_double, [c_int64]),
    "dal_density_error_bound_sym_d": (c_double, [c_int64, c_int64]),
    "dal_gram_rowsum_sym": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                    c_int64, c_int64, c_void_p, c_int, c_void_p]),
    "dal_gram_rowsum_sym_skip": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                         c_int64, c_int64, c_int64, c_int64, c_void_p, c_int, c_void_p]),
    "dal_gram_sym_residual_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "dal_gram_sym_residual": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                      c_size_t, c_void_p]),
    "dal_quant_i8": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "dal_gram_rowsum_sym_i8_skip": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                            c_int64, c_int64, c_int64, c_int64, c_void_p, c_int, c_void_p]),
    "dal_gram_sym_residual_i8": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                         c_size_t, c_void_p]),
    "dal_quant_fp4": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "dal_gram_rowsum_sym_fp4_skip": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64,
                                             c_int64, c_int64, c_int64, c_int64, c_void_p, c_int, c_void_p]),
    "dal_gram_sym_residual_fp4": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                          c_size_t, c_void_p]),
    "dal_forest_score": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int32,
                                 c_int32, c_void_p, c_void_p, c_int, c_double, c_void_p, c_double,
                                 c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_forest_blocked_rows": (c_int, [c_int64, c_int32, c_int32]),
    "dal_pool_blocked_floats": (c_int64, [c_int64, c_int64]),
    "dal_pool_blocked": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "dal_forest_prep_bytes": (c_size_t, [c_int64, c_int32, c_int32]),
    "dal_forest_prepare": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int64, c_void_p, c_size_t, c_void_p]),
    "dal_forest_score_blocked": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                         c_int32,
                                         c_int32, c_void_p, c_void_p, c_int, c_double, c_void_p, c_double,
                                         c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_forest_multiclass_max_classes": (c_int, []),
    "dal_forest_score_multiclass": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int32,
                                            c_int32, c_int32, c_void_p, c_int, c_void_p, c_int, c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_forest_score_multiclass_dw": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int32,
                                               c_int32, c_int32, c_void_p, c_void_p, c_int, c_double, c_void_p,
                                               c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                               c_void_p, c_void_p, c_void_p]),
    "dal_forest_multiclass_blocked_rows": (c_int, [c_int64, c_int32, c_int32, c_int32]),
    "dal_forest_score_multiclass_blocked": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                                    c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int,
                                                    c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                                    c_void_p]),
    "dal_forest_score_multiclass_dw_blocked": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                                                       c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p,
                                                       c_void_p, c_int, c_double, c_void_p, c_double, c_void_p,
                                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                                       c_void_p]),
    "dal_forest_soft_max_depth": (c_int, []),
    "dal_forest_score_soft": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                      c_int32, c_int32, c_int32, c_int, c_void_p, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "dal_forest_score_soft_dw": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                         c_int32, c_int32, c_int32, c_void_p, c_int, c_double, c_void_p, c_double,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "dal_forest_score_soft_bald": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                           c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_int, c_void_p,
                                           c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_dw_step_soft": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                 c_int32, c_int32, c_int32, c_void_p, c_double, c_void_p, c_double, c_int64,
                                 c_void_p, c_void_p, c_int64, c_int64, c_int32, ctypes.c_uint32, c_void_p, c_size_t,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_density_separable": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_void_p]),
    "dal_topk_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "dal_topk": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p,
                         c_void_p]),
    "dal_dw_select_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "dal_dw_select": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64,
                              c_void_p, c_double, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                              c_int64, c_int32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                              c_void_p, c_void_p]),
    "dal_dw_step_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "dal_dw_step": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                            c_void_p, c_double, c_void_p, c_double, c_int64, c_void_p, c_void_p, c_int64, c_int64,
                            c_int32, ctypes.c_uint32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_dw_step_multiclass": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                       c_int32, c_int32, c_int32, c_void_p, c_void_p, c_double, c_void_p, c_double,
                                       c_int64, c_void_p, c_void_p, c_int64, c_int64, c_int32, ctypes.c_uint32,
                                       c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p]),
    "dal_dw_step_multiclass_form": (c_int, [c_int64, c_int64, c_int32, c_int32, c_int32, c_int64, c_int64, c_int32,
                                            c_int]),
    "dal_dw_plan_create_multiclass": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p,
                                              c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_double,
                                              c_void_p, c_void_p, c_double, c_int64, c_void_p, c_void_p, c_int64,
                                              c_int64, c_int32, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                              c_void_p, c_void_p]),
    "dal_dw_plan_create": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int32, c_int32,
                                   c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_double, c_int64, c_void_p,
                                   c_void_p, c_int64, c_int64, c_int32, c_void_p, c_size_t, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_dw_plan_run": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_dw_plan_launch": (c_int, [c_void_p, c_void_p, c_int64, c_void_p]),
    "dal_dw_plan_destroy": (None, [c_void_p]),
    "dal_maxcos_label_rows_granule": (c_int64, [c_int64]),
    "dal_maxcos_error_bound": (c_double, [c_int64]),
    "dal_inv_norms_bf16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                   c_void_p]),
    "dal_canon_unit_rows_bf16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p]),
    "dal_max_cosine": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_unit_rows_f16": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p]),
    "dal_maxcos_unit_error_bound": (c_double, [c_int64]),
    "dal_max_cosine_unit": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "dal_text_shape": (c_int, [c_void_p, c_size_t, c_int64, c_void_p, c_void_p]),
    "dal_parse_labeled_text": (c_int, [c_void_p, c_size_t, c_int64, c_int64, c_int, c_void_p, c_void_p, c_int]),
    "dal_maxcos_argmax_resolve": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_void_p,
                                          c_void_p]),
    "dal_interval_keys_f32": (c_int, [c_void_p, c_int64, c_double, c_void_p, c_int, c_void_p,
                                      c_void_p, c_void_p]),
    "dal_maxcos_select_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "dal_maxcos_select": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64,
                                  c_int64, c_void_p, c_int64, c_int64, c_int32, c_void_p, c_size_t, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_topk_merge_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "dal_topk_merge": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p]),
    "dal_sort_pairs": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "dal_gram_entries": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p]),
    "dal_cosine_pairs_error_bound": (c_double, [c_int64]),
    "dal_cosine_pairs": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64,
                                 c_void_p, c_double, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_cosine_pairs_resolve": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_int64,
                                         c_void_p, c_void_p]),
    "dal_rf_find_splits": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int32, c_void_p,
                                   c_void_p, c_void_p, c_void_p]),
    "dal_rf_train_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32, c_int32]),
    "dal_rf_train": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32,
                             c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_double, c_void_p,
                             c_void_p, c_void_p, c_size_t, c_void_p]),
    "dal_rf_train_multiclass_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int32, c_int32, c_int32, c_int32,
                                                           c_int32]),
    "dal_rf_train_multiclass": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32,
                                        c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_double, c_int32,
                                        c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dal_forest_regress_chunk_trees": (c_int, [c_int32]),
    "dal_forest_regress": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_int32, c_int32, c_void_p, c_void_p]),
    "dal_rf_find_splits_f64": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_int64, c_int32,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_rf_bin_rows": (c_int, [c_void_p, c_int, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "dal_rf_train_regressor_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32, c_int32, c_int32, c_int32,
                                                          c_int32]),
    "dal_rf_train_regressor": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_void_p,
                                       c_void_p, c_int32, c_int32, c_int32, c_int32, c_double, c_int32, c_int32,
                                       c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                       c_void_p]),
    "dal_rf_train_begin": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                   c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_double,
                                   c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dal_rf_train_level_stats": (c_int, [c_void_p, c_int32, c_void_p]),
    "dal_rf_train_level_split": (c_int, [c_void_p, c_int32, c_void_p]),
    "dal_rf_train_finish": (c_int, [c_void_p, c_void_p]),
    "dal_rf_train_level_span": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "dal_rf_train_multiclass_begin": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                              c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                              c_int32, c_double, c_int32, c_void_p, c_void_p, c_void_p, c_size_t,
                                              c_void_p]),
    "dal_rf_train_multiclass_level_stats": (c_int, [c_void_p, c_int32, c_void_p]),
    "dal_rf_train_multiclass_level_split": (c_int, [c_void_p, c_int32, c_void_p]),
    "dal_rf_train_multiclass_finish": (c_int, [c_void_p, c_void_p]),
    "dal_rf_train_multiclass_level_span": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "dal_rf_train_regressor_begin": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                             c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32,
                                             c_double, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_size_t, c_void_p]),
    "dal_rf_train_regressor_level_stats": (c_int, [c_void_p, c_int32, c_void_p]),
    "dal_rf_train_regressor_level_split": (c_int, [c_void_p, c_int32, c_void_p]),
    "dal_rf_train_regressor_finish": (c_int, [c_void_p, c_void_p]),
    "dal_rf_train_regressor_level_span": (c_int, [c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "dal_vote_histogram": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_void_p, c_void_p]),
    "dal_lal_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_double, c_double, c_void_p, c_void_p]),
    "dal_votes_rescore": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "dal_scaler_rows_per_block": (c_int64, [c_int64, c_int64]),
    "dal_scaler_limbs": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_scaler_format": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_scaler_accumulate": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_int32, c_int32, c_void_p,
                                      c_void_p]),
    "dal_scaler_transform": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int,
                                     c_int64, c_void_p]),
    "dal_forest_evaluate_cells": (c_int, [c_int32, c_int32]),
    "dal_forest_evaluate_blocked_rows": (c_int, [c_int64, c_int32, c_int32, c_int32]),
    "dal_forest_evaluate": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p,
                                    c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_sq_error_format": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_sq_error_accumulate": (c_int, [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p]),
    "dal_kcenter_error_bound": (c_double, [c_int64]),
    "dal_kcenter_workspace_bytes": (c_size_t, [c_int64, c_int64, c_int64, c_int64]),
    "dal_kcenter_begin": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_kcenter_propose": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "dal_kcenter_commit": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "dal_kcenter_select": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int64, c_int64, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "dal_kcenter_ranked_workspace_bytes": (c_size_t, [c_int64]),
    "dal_kcenter_ranked_error_bound": (c_double, [c_int64, c_double]),
    "dal_kcenter_ranked_attach": (c_int, [c_void_p, c_void_p, c_double, c_void_p, c_size_t, c_void_p, c_void_p]),
    "dal_kcenter_run": (c_int, [c_void_p, c_void_p]),
}

_lib = None


class DalError(RuntimeError):
    pass


def load():
    """Load libdal.so (raises if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DalError(
            f"{LIB_PATH} not found: build the HIP library first "
            "(python -c 'import __graft_entry__ as g; g.build()')")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str):
    if rc != DAL_OK:
        msg = load().dal_status_string(rc).decode()
        raise DalError(f"{what} failed: {msg} (status {rc})")


def call(name: str, *args):
    """Call a status-returning entry point and raise on failure."""
    rc = getattr(load(), name)(*args)
    check(rc, name)
