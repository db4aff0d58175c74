"""ctypes binding of liblmi_hip.so (the C ABI in include/lmi_hip.h).

There is no CPU fallback: if the HIP library is missing or fails, this module raises.
torch is imported first so that the HIP runtime (libamdhip64.so.7) already loaded by PyTorch-ROCm
is the one the library binds to; torch device pointers and streams are then valid inside it.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LMI_LIB") or os.path.join(_HERE, "liblmi_hip.so")  # LMI_LIB: A/B builds (tools/)
K_PER_BUCKET = 10
KNN_MAX_K = 1024   # LMI_KNN_MAX_K: the largest k of `knn` (lmi_knn); `knn_ip` (lmi_knn_ip) stays at K_PER_BUCKET
T_INFERENCE, T_ROUTE, T_SCAN, T_MERGE, T_TOTAL, T_PF_SAMPLE, T_PF_EMIT, T_RESCORE, T_FALLBACK, T_CLOCK_MHZ, T_COUNT = (
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12)   # (T_CLOCK_MHZ is not a time: the shader clock held under pass 2, from in-kernel counters)

#: the LMI_PLAN_* words of include/lmi_hip.h, in their order (lmi_debug_last_plan / lmi_debug_plan)
PLAN_FIELDS = ("fast", "low_d", "ps_wide", "tile_cb", "sample_max", "qbound", "primary_nb", "use_front", "streamed", "G", "use_tail",
               "tail_merges", "KG16", "dp", "route_nb_template", "pack_gs", "pack_cp", "pack_vec", "route_sort_global", "merge_kind",
               "rescore_small_waves", "overflow_sorted")
#: the LMI_MLP_PLAN_* words, in their order (lmi_debug_last_mlp_plan / lmi_debug_mlp_plan)
MLP_PLAN_FIELDS = ("num_cus", "fm_ok", "logits_lds", "lds_bytes", "fused", "mode", "fused_blocks", "nq_head", "layers_queries",
                   "cbw0", "cbw1", "cbw2", "cbw3", "cbw4", "cbw5", "cbw6", "cbw7", "rank_kernel", "softmax_kernel", "vec_in", "in_chunks")
#: the LMI_KNN_PLAN_* words, in their order (lmi_debug_knn_plan)
KNN_PLAN_FIELDS = ("PIECES", "PIECE_ROWS", "SPLITS", "QUERY_GROUPS", "QUERY_ROWS", "VEC_XQ", "VEC_XB", "WORKSPACE_BYTES", "LIST_ROWS")
KNN_METRICS = {"ip": 0, "l2": 1}   # LMI_METRIC_IP, LMI_METRIC_L2
#: the LMI_KNN_RANGE_PLAN_* words, in their order (lmi_debug_knn_range_plan)
KNN_RANGE_PLAN_FIELDS = ("PIECES", "PIECE_ROWS", "SPLITS", "QUERY_GROUPS", "QUERY_ROWS", "RESULTS", "CHUNK_BYTES", "WORKSPACE_BYTES")
UNION_MAX_K = 1024   # LMI_UNION_MAX_K: the largest k of the union scan (`Index.scan_union`, `search_union`, `search_tree_union`)
#: the LMI_UNION_PLAN_* words, in their order (lmi_debug_union_plan)
UNION_PLAN_FIELDS = ("GROUPS", "QUERY_ROWS", "WAVES", "SLAB_BYTES", "LIST_ROWS", "LISTS_PER_QUERY", "WORKSPACE_BYTES", "VEC_ROWS")
UNION_PART_PLANES = 5   # LMI_UNION_PART_PLANES: a part of the union scan is int32 [5, nq, k] -- the LMI_UPART_* planes, in their order:
UPART_SCORE, UPART_DIST, UPART_ID, UPART_RANK, UPART_ROW = range(5)
FILTER_KEEP, FILTER_DROP = 0, 1   # LMI_FILTER_KEEP, LMI_FILTER_DROP: the list names the allowed / the disallowed ids
FILTER_MAX = 1024                 # LMI_FILTER_MAX: filters of one set (`Filter`)
#: the LMI_FILTER_PLAN_* words, in their order (lmi_debug_filter_plan)
FILTER_PLAN_FIELDS = ("FILTERS", "MASK_BYTES", "SLOTS", "SKIPPED")
#: the LMI_RANGE_PLAN_* words, in their order (lmi_debug_range_plan)
RANGE_PLAN_FIELDS = ("GROUPS", "QUERY_ROWS", "WAVES", "SLAB_BYTES", "RESULTS", "CHUNK_BYTES", "WORKSPACE_BYTES")
#: the LMI_RANGE_JOIN_* words, in their order (lmi_debug_range_join_plan)
RANGE_JOIN_FIELDS = ("PARTS", "RUNS", "PIECES", "RESULTS", "LARGEST_PART")
#: the LMI_RANGE_SORT_PLAN_* words, in their order (lmi_debug_range_sort_plan)
RANGE_SORT_PLAN_FIELDS = ("GROUPS", "WAVE_SEGMENTS", "TILE_SEGMENTS", "LONG_SEGMENTS", "SKIPPED_SEGMENTS", "TILE_ROWS", "WAVE_ROWS",
                          "MERGE_ROWS", "MAX_PASSES", "SCRATCH_BYTES", "RESULTS")
RANGE_SORT_MIN_TILE_ROWS, RANGE_SORT_MAX_TILE_ROWS = 64, 8192   # what lmi_range_sort_set_geometry takes for tile_rows (a power of two)
#: the LMI_REGROUP_PLAN_* words, in their order (lmi_debug_regroup_plan)
REGROUP_PLAN_FIELDS = ("ROWS", "TILE_ROWS", "TILES", "MERGE_ROWS", "PASSES", "MAP_BYTES", "NAMED")
REGROUP_MIN_TILE_ROWS, REGROUP_MAX_TILE_ROWS = 64, 8192   # what lmi_regroup_set_geometry takes (a power of two)
REGROUP_MAX_LABELS = 1 << 20                              # lmi_regroup: L_new stays below it
CONCAT_MAX_PARTS = 64   # LMI_CONCAT_MAX_PARTS: parts of one `Index.concat`, the receiver included
#: the LMI_CONCAT_PLAN_* words, in their order (lmi_debug_concat_plan)
CONCAT_PLAN_FIELDS = ("PARTS", "ROWS", "SLAB_ROWS", "MAP_BYTES", "RESCALED_PARTS")
#: the LMI_FETCH_PLAN_* words, in their order (lmi_debug_fetch_plan)
FETCH_PLAN_FIELDS = ("REQUESTS", "UNIQUE", "PIECES", "PIECE_ROWS", "FOUND", "FORM", "WORKSPACE_BYTES")
FETCH_MAX_PIECE_ROWS = 1 << 24   # what lmi_fetch_set_geometry takes at most
#: the words of `cover_last_plan` (LMI_COVER_PLAN_* of include/lmi_hip.h, in the enum's order)
COVER_PLAN_FIELDS = ("GROUPS", "QUERY_ROWS", "BUCKETS", "ADMITTED", "MAX_PER_QUERY", "NB_USED", "WORKSPACE_BYTES")
COVER_MAX_QUERY_ROWS = 1 << 20   # what lmi_cover_set_geometry takes at most

_lib = None

_f32p = ctypes.POINTER(ctypes.c_float)
_i32p = ctypes.POINTER(ctypes.c_int32)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u32p = ctypes.POINTER(ctypes.c_uint32)
_u8p = ctypes.POINTER(ctypes.c_uint8)
_vp = ctypes.c_void_p

#: every symbol include/lmi_hip.h declares: name -> (restype, argtypes)
SIGNATURES = {
    "lmi_abi_version": (ctypes.c_int, []),
    "lmi_last_error": (ctypes.c_char_p, []),
    "lmi_build_info": (ctypes.c_char_p, []),
    "lmi_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_vp)]),
    "lmi_destroy": (ctypes.c_int, [_vp]),
    "lmi_set_stream": (ctypes.c_int, [_vp, _vp]),
    "lmi_set_mlp": (ctypes.c_int, [_vp, ctypes.c_int, _i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "lmi_set_fused_mlp": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmi_set_stop_mass": (ctypes.c_int, [_vp, ctypes.c_float]),
    "lmi_set_path_mass": (ctypes.c_int, [_vp, ctypes.c_float]),
    "lmi_set_stop_rows": (ctypes.c_int, [_vp, ctypes.c_int64]),
    "lmi_set_metric": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmi_set_storage": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmi_index_bytes": (ctypes.c_int, [_vp, _i64p]),
    "lmi_nav_set_model": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "lmi_nav_set_tree": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp]),
    "lmi_nav_order": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int]),
    "lmi_search_tree": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "lmi_buckets_begin": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    "lmi_buckets_add_rows": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "lmi_buckets_add_owned_rows": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int]),
    "lmi_buckets_end": (ctypes.c_int, [_vp]),
    "lmi_buckets_insert": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, _i64p]),
    "lmi_buckets_delete": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _i64p]),
    "lmi_subset": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(_vp), _i64p]),
    "lmi_regroup": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, _vp, ctypes.c_int, ctypes.POINTER(_vp), _i64p]),
    "lmi_regroup_set_geometry": (ctypes.c_int, [ctypes.c_int64]),
    "lmi_debug_regroup_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    "lmi_concat": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, ctypes.POINTER(_vp), _i64p]),
    "lmi_debug_concat_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    "lmi_bucket_sizes": (ctypes.c_int, [_vp, _vp]),
    "lmi_mlp_topk": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int]),
    "lmi_mlp_proba": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int]),
    "lmi_scan_topk": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
                                     ctypes.c_int]),
    "lmi_search": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp,
                                  ctypes.c_int]),
    "lmi_merge_gathered": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int64, ctypes.c_int,
                                          ctypes.c_int, _vp, _vp, ctypes.c_int]),
    "lmi_comm_unique_id": (ctypes.c_int, [_vp]),
    "lmi_comm_init": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "lmi_comm_destroy": (ctypes.c_int, [_vp]),
    "lmi_allgather_merge": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int,
                                           _vp, _vp]),
    "lmi_bucket_read": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    "lmi_copy_out": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64]),
    "lmi_copy_out_many": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp, _vp]),
    "lmi_pipeline_submit": (ctypes.c_int, [_vp] * 7 + [_vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "lmi_knn_ip": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int,
                                  ctypes.c_int, _vp, _vp]),
    "lmi_knn": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                               _vp, _vp, ctypes.c_int]),
    "lmi_knn_f16": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   _vp, _vp, ctypes.c_int]),
    "lmi_knn_set_geometry": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64]),
    "lmi_debug_knn_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    "lmi_knn_range": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int64,
                                     ctypes.POINTER(_vp), ctypes.c_int]),
    "lmi_knn_range_f16": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, _vp,
                                         ctypes.c_int64, ctypes.POINTER(_vp), ctypes.c_int]),
    "lmi_debug_knn_range_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    "lmi_scan_union": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int]),
    "lmi_search_union": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "lmi_search_tree_union": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "lmi_union_set_geometry": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "lmi_debug_union_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    "lmi_scan_union_part": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int]),
    "lmi_merge_union_parts": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int]),
    "lmi_allgather_merge_union": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp]),
    # filter sets and the filtered union scan: the parent call's arguments, then (filter, filter_of on the host)
    "lmi_filter_create": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.POINTER(_vp)]),
    "lmi_filter_destroy": (ctypes.c_int, [_vp]),
    "lmi_filter_counts": (ctypes.c_int, [_vp, _vp]),
    "lmi_filter_bucket_mask": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    "lmi_scan_union_filtered": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int, _vp, _vp]),
    "lmi_search_union_filtered": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, ctypes.c_int,
                                                 _vp, _vp]),
    "lmi_search_tree_union_filtered": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp,
                                                      ctypes.c_int, _vp, _vp]),
    "lmi_debug_filter_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    # the range search: (.., radius on the host, filter, filter_of on the host, max_total, &result, [order outputs,] on_device)
    "lmi_scan_range": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int64, ctypes.POINTER(_vp),
                                      ctypes.c_int]),
    "lmi_search_range": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int64, ctypes.POINTER(_vp),
                                        _vp, ctypes.c_int]),
    "lmi_search_tree_range": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int64,
                                             ctypes.POINTER(_vp), _vp, _vp, ctypes.c_int]),
    "lmi_range_result_total": (ctypes.c_int, [_vp, _i64p]),
    "lmi_range_result_lims": (ctypes.c_int, [_vp, _vp]),
    "lmi_range_result_read": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int]),
    "lmi_range_result_destroy": (ctypes.c_int, [_vp]),
    "lmi_debug_range_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    # the range search across ranks: a result's per-(query, rank) counts, the join of the ranks' parts, its exchange through RCCL
    "lmi_range_result_pair_counts": (ctypes.c_int, [_vp, _i32p, _vp]),
    "lmi_join_range_parts": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                            ctypes.c_int64, ctypes.POINTER(_vp), ctypes.c_int]),
    "lmi_allgather_join_range": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int64, ctypes.POINTER(_vp)]),
    "lmi_range_join_set_geometry": (ctypes.c_int, [ctypes.c_int64]),
    "lmi_debug_range_join_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    # a range result sorted by distance on the device
    "lmi_range_result_sort": (ctypes.c_int, [_vp, _vp]),
    "lmi_range_result_sorted": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "lmi_range_sort_set_geometry": (ctypes.c_int, [ctypes.c_int64, ctypes.c_int64]),
    "lmi_debug_range_sort_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    "lmi_kmeans": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp,
                                  ctypes.c_int]),
    "lmi_train": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int, _i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                 ctypes.POINTER(_vp), _i64p, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, ctypes.c_int]),
    # the index build on binary16 rows (arguments as the namesakes')
    "lmi_kmeans_f16": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp,
                                      ctypes.c_int]),
    "lmi_train_f16": (ctypes.c_int, [ctypes.c_int, _vp, ctypes.c_int64, _vp, ctypes.c_int, _i32p, ctypes.POINTER(_vp), ctypes.POINTER(_vp),
                                     ctypes.POINTER(_vp), _i64p, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, _vp, ctypes.c_int]),
    "lmi_mlp_topk_f16": (ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, ctypes.c_int]),
    "lmi_timings": (ctypes.c_int, [_vp, _vp]),
    "lmi_timings_reset": (ctypes.c_int, [_vp]),
    "lmi_set_timing": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmi_timings_mean": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_int)]),
    "lmi_scan_stats": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_double), _i64p, _i64p]),
    "lmi_set_chunk_rows": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmi_workspace_bytes": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _i64p]),
    "lmi_set_prefilter": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmi_debug_peek": (ctypes.c_int, [_vp, ctypes.c_char_p, _vp, ctypes.c_int64]),
    "lmi_clone_view": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "lmi_prefilter_stats": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), _i64p, _i64p]),
    "lmi_debug_emit_all": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lmi_debug_read_candidates": (ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_int, _vp, _vp,
                                                 ctypes.POINTER(ctypes.c_int), _f32p, _f32p, _f32p]),
    "lmi_debug_layout": (ctypes.c_int, [_vp, _vp, _vp, _i64p, _i64p, _vp]),
    "lmi_debug_last_plan": (ctypes.c_int, [_vp, _i32p, ctypes.c_int]),
    "lmi_debug_plan": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int]),
    "lmi_debug_last_mlp_plan": (ctypes.c_int, [_vp, _i32p, ctypes.c_int]),
    "lmi_debug_mlp_plan": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _i32p, ctypes.c_int]),
    # binary16 rows and queries as they are distributed (uint16 bit patterns; arguments as the namesakes')
    "lmi_buckets_add_rows_f16": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int]),
    "lmi_buckets_add_owned_rows_f16": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int64, ctypes.c_int]),
    "lmi_buckets_insert_f16": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_int64, ctypes.c_int, _i64p]),
    "lmi_bucket_read_f16": (ctypes.c_int, [_vp, ctypes.c_int, _vp, _vp]),
    # stored objects by id: (handle, ids, n, rows, bucket, row, on_device)
    "lmi_rows_fetch": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int]),
    "lmi_rows_fetch_f16": (ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp, _vp, _vp, ctypes.c_int]),
    "lmi_fetch_set_geometry": (ctypes.c_int, [ctypes.c_int64]),
    "lmi_debug_fetch_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    # the bucket cover and the exact range search: (handle, cover, queries, nq, radius on the host, ..)
    "lmi_cover_create": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "lmi_cover_destroy": (ctypes.c_int, [_vp]),
    "lmi_cover_read": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "lmi_cover_order": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, ctypes.c_int]),
    "lmi_search_range_exact": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp, _vp, _vp, ctypes.c_int64, ctypes.POINTER(_vp), _i32p, _vp,
                                              ctypes.c_int]),
    "lmi_cover_set_geometry": (ctypes.c_int, [ctypes.c_int64]),
    "lmi_debug_cover_plan": (ctypes.c_int, [_i64p, ctypes.c_int]),
    "lmi_scan_topk_f16": (ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp,
                                         ctypes.c_int]),
    "lmi_search_f16": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp,
                                      ctypes.c_int]),
    "lmi_search_tree_f16": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp, _vp, _vp, _vp, _vp,
                                           ctypes.c_int]),
}


class LmiError(RuntimeError):
    """Raised when a C-ABI call returns non-zero (message from lmi_last_error)."""


def lib() -> ctypes.CDLL:
    """Loads liblmi_hip.so (after torch, so one HIP runtime serves both) and declares prototypes."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise LmiError(
                f"{LIB_PATH} is missing: build it with learnedmetricindex_amd/csrc/build.sh "
                "(or __graft_entry__.build()); there is no CPU fallback")
        import torch  # noqa: F401  (loads PyTorch-ROCm's libamdhip64 first)

        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lmi_abi_version() != 1:
            raise LmiError("liblmi_hip.so ABI version mismatch")
        _lib = L
    return _lib


def _check(rc: int) -> None:
    if rc != 0:
        raise LmiError(lib().lmi_last_error().decode("utf-8", "replace"))


def _ptr(a) -> int:
    """Raw address of a numpy array or torch tensor (None -> NULL)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()  # torch.Tensor


def _np(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=dtype)


def _is_f16(a) -> bool:
    """A numpy float16 array or a torch.float16 tensor: data the `_f16` entry points take as it is."""
    if isinstance(a, np.ndarray):
        return a.dtype == np.float16
    return getattr(a, "dtype", None) is not None and str(a.dtype) == "torch.float16"


def _rows_arg(rows):
    """(rows, on_device, f16) of an ingest call: numpy -> C-contiguous float16 (kept) or float32 (anything else is
    converted, as before); a CUDA torch tensor -> as it is, float16 or a 4-byte float."""
    f16 = _is_f16(rows)
    if isinstance(rows, np.ndarray):
        return _np(rows, np.float16 if f16 else np.float32), 0, f16
    assert rows.is_cuda and rows.is_contiguous() and rows.dtype.is_floating_point and rows.element_size() == (2 if f16 else 4)
    return rows, 1, f16


def _device_f16(qn_t, qs_t) -> bool:
    """Whether a device search call takes its `_f16` form: both query tensors are torch.float16 (contiguous).  A half tensor
    beside a float one is an error: nothing is converted on the device on the caller's behalf."""
    f16 = _is_f16(qn_t), _is_f16(qs_t)
    assert f16[0] == f16[1], "device query tensors must both be float16 or both float32"
    assert not f16[0] or (qn_t.is_contiguous() and qs_t.is_contiguous())
    return f16[0]


def _nbytes(a) -> int:
    return int(a.nbytes) if isinstance(a, np.ndarray) else int(a.numel() * a.element_size())


def _queries(queries_nav, queries_search):
    """(qn, qs, f16) of a search call: both arrays float16 -> kept as halves for the `_f16` call; otherwise float32 (a
    half array beside a float one is widened on the host).  `qs is qn` where the caller passed one array twice."""
    same = queries_search is queries_nav
    f16 = _is_f16(queries_nav) and (same or _is_f16(queries_search))
    dt = np.float16 if f16 else np.float32
    qn = _np(queries_nav, dt)
    return qn, (qn if same else _np(queries_search, dt)), f16


def _array_arg(who: str, name: str, a, dtype: Optional[str] = None, rank: Optional[str] = None, kind: bool = True) -> bool:
    """Whether `a` is a numpy array.  Checks, each only if asked for and in this order: `kind`: numpy or a torch tensor on the device;
    `dtype`; `rank` "2d": two-dimensional, "nd": [n,d] with n, d >= 1."""
    is_np = isinstance(a, np.ndarray)
    if kind and not is_np and not (hasattr(a, "data_ptr") and hasattr(a, "is_cuda")):
        raise ValueError(f"{who}: {name} must be a numpy array or a torch tensor on the device")
    if dtype is not None and str(a.dtype).replace("torch.", "") != dtype:
        raise ValueError(f"{who}: {name} must be {dtype}, not {a.dtype}")
    if rank is not None and (a.ndim != 2 or (rank == "nd" and min(a.shape) < 1)):
        want = "[n,d] with n, d >= 1" if rank == "nd" else "two-dimensional"
        raise ValueError(f"{who}: {name} must be {want}, not {tuple(a.shape)}")
    return is_np


def _sync_device(t) -> int:
    """The tensor's device index, after a synchronise: these calls run on the NULL stream; whatever produced `t` may not have."""
    import torch

    torch.cuda.synchronize(t.device)
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def f16_admissible(x):
    """(ok, reason): whether `storage="f16"` (LMI_STORAGE_F16) would accept the scan vectors `x` -- the library's rule
    (include/lmi_hip.h, decided there on the device) in numpy, for callers who want to know before they upload.  Every value
    must be finite and exactly representable in binary16, and so must the value times the index scale: the power of two `s`
    with max|x| * s in [0.5, 1)."""
    x = np.asarray(x, dtype=np.float32)
    if x.size == 0:
        return True, "admissible"
    if not np.isfinite(x).all():
        return False, "a value is not finite (inf or NaN)"
    with np.errstate(over="ignore"):
        if not np.array_equal(x.astype(np.float16).astype(np.float32), x):
            return False, "a value is not exactly representable in binary16"
    m = float(np.abs(x).max())
    s = np.float32(1.0) if m == 0.0 else np.float32(np.ldexp(1.0, -int(np.frexp(m)[1])))
    xs = x * s   # a power of two: exact in binary32
    if not np.array_equal(xs.astype(np.float16).astype(np.float32), xs):
        return False, f"a value times the index scale {float(s):g} is not exactly representable in binary16"
    return True, "admissible"


class Index:
    """One device-resident index: thin, typed wrapper over an `lmi_index*`."""

    METRICS = {"ip": 0, "l2": 1}
    STORAGES = {"f32": 0, "f16": 1}

    def __init__(self, device: int = 0, chunk_rows: Optional[int] = None, prefilter: Optional[bool] = None,
                 metric: str = "ip", storage: str = "f32"):
        self._h = _vp()
        _check(lib().lmi_create(int(device), ctypes.byref(self._h)))
        try:
            self._configure(device, chunk_rows, prefilter, metric, storage)
        except BaseException:
            self.close()   # a refused setting leaves no handle behind
            raise

    def _configure(self, device, chunk_rows, prefilter, metric, storage) -> None:
        self.device = int(device)
        self.n_classes = None
        self.d_nav = None
        self.d = None
        self.L = None
        self.stop_mass = 0.0
        self.path_mass = 0.0
        self.stop_rows = 0
        self.bytes_in = 0   # bytes handed to add_rows / add_owned_rows / insert since the last buckets_begin (counted here, not in the library)
        if chunk_rows is not None:
            _check(lib().lmi_set_chunk_rows(self._h, int(chunk_rows)))
        if prefilter is None and os.environ.get("LMI_PREFILTER") is not None:
            prefilter = os.environ["LMI_PREFILTER"] not in ("0", "off", "false")
        if prefilter is not None:
            self.set_prefilter(prefilter)
        if metric != "ip":  # "l2": squared Euclidean distances instead of 1 - inner product
            _check(lib().lmi_set_metric(self._h, self.METRICS[metric]))
        self.metric = metric
        self.storage = "f32"
        if storage != "f32":  # "f16": the fp16 fragments only, for binary16-exact vectors (lmi_set_storage)
            self.set_storage(storage)

    def set_storage(self, storage: str) -> None:
        """"f32" (default) or "f16" (`lmi_set_storage`): how the next `buckets_begin` stores the scan vectors.  "f16" keeps the
        prefilter's fp16 fragments only -- a third of the memory, same results bit for bit -- and `buckets_end` refuses data
        that is not binary16-exact (`f16_admissible`).  Not with metric "l2", `prefilter=False`, `insert` or `delete`."""
        if storage not in self.STORAGES:
            raise ValueError(f"storage must be one of {sorted(self.STORAGES)}, not {storage!r}")
        _check(lib().lmi_set_storage(self._h, self.STORAGES[storage]))
        self.storage = storage

    def index_bytes(self) -> int:
        """Device bytes of the index images held right now: vector images, ids, per-bucket tables (`lmi_index_bytes`; valid from
        `buckets_begin` on)."""
        out = ctypes.c_int64(0)
        _check(lib().lmi_index_bytes(self._h, ctypes.byref(out)))
        return out.value

    def close(self) -> None:
        for c in getattr(self, "_views", []):   # clones borrow this handle's memory: they go first
            c.close()
        self._views = []
        if getattr(self, "_h", None) is not None and self._h:
            lib().lmi_destroy(self._h)
            self._h = None

    def clone_view(self) -> "Index":
        """A second handle on the same index (`lmi_clone_view`): shares the weights and the bucket slabs, has its own
        workspaces, stream and timings.  Closed with (before) this one."""
        v = self._derived()
        _check(lib().lmi_clone_view(self._h, ctypes.byref(v._h)))
        v.N = getattr(self, "N", None)
        v._parent = self
        self.__dict__.setdefault("_views", []).append(v)
        return v

    def _derived(self) -> "Index":
        """An `Index` without a handle yet that describes this one's models and index (`clone_view`, `subset`)."""
        v = Index.__new__(Index)
        v._h, v._views = _vp(), []
        for a in ("device", "n_classes", "d_nav", "d", "L", "metric", "storage", "stop_mass", "path_mass", "stop_rows"):
            setattr(v, a, getattr(self, a, None))
        return v

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def set_prefilter(self, on) -> None:
        """fp16 prefilter + exact re-rank (default) or f32 MFMA for every similarity; same results."""
        _check(lib().lmi_set_prefilter(self._h, int(on)))

    def debug_peek(self, name: str, nbytes: int) -> np.ndarray:
        """Developer aid: the first `nbytes` of a named internal device buffer as uint8."""
        out = np.empty(nbytes, np.uint8)
        _check(lib().lmi_debug_peek(self._h, name.encode(), out.ctypes.data_as(_vp), nbytes))
        return out

    def prefilter_stats(self):
        """(active, survivors re-scored exactly, slots that fell back to exact brute force)."""
        a = ctypes.c_int(0)
        sv = ctypes.c_int64(0)
        fb = ctypes.c_int64(0)
        _check(lib().lmi_prefilter_stats(self._h, ctypes.byref(a), ctypes.byref(sv), ctypes.byref(fb)))
        return bool(a.value), sv.value, fb.value

    def debug_emit_all(self, on: bool) -> None:
        """Test hook: pass 2 emits every row of a visited bucket (see include/lmi_hip.h)."""
        _check(lib().lmi_debug_emit_all(self._h, 1 if on else 0))

    def debug_read_candidates(self, slot: int, cap: int = 1024):
        """Test hook: (rows u32[n], shat f32[n], emitted count, 2*eps', qscale, xscale) of slot q*nb+r."""
        rows = np.empty(cap, dtype=np.uint32)
        shat = np.empty(cap, dtype=np.float32)
        cnt = ctypes.c_int(0)
        e2, qs, xs = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0)
        _check(lib().lmi_debug_read_candidates(self._h, int(slot), int(cap), _ptr(rows), _ptr(shat), ctypes.byref(cnt),
                                               ctypes.byref(e2), ctypes.byref(qs), ctypes.byref(xs)))
        n = max(0, min(cnt.value, cap))
        return rows[:n], shat[:n], cnt.value, e2.value, qs.value, xs.value

    def debug_layout(self) -> dict:
        """Test hook (`lmi_debug_layout`, host tables only): rb_start i32[L+1], cap_rb i32[L], n_rb_total, alloc_rb and
        counters i64[4] = (slack fills, relocations, growth re-packs, hole re-packs) of this handle's inserts."""
        rb_start = np.empty(self.L + 1, dtype=np.int32)
        cap_rb = np.empty(self.L, dtype=np.int32)
        counters = np.empty(4, dtype=np.int64)
        n_rb, alloc = ctypes.c_int64(0), ctypes.c_int64(0)
        _check(lib().lmi_debug_layout(self._h, _ptr(rb_start), _ptr(cap_rb), ctypes.byref(n_rb), ctypes.byref(alloc),
                                      _ptr(counters)))
        return dict(rb_start=rb_start, cap_rb=cap_rb, n_rb_total=n_rb.value, alloc_rb=alloc.value, counters=counters)

    def debug_last_plan(self) -> dict:
        """Test hook (`lmi_debug_last_plan`): the kernel forms the last scan on this handle took, as recorded while it ran --
        `PLAN_FIELDS` -> int.  The plan's fields, then the launch sites' template choices (-1: that launch was not part of the call)."""
        w = (ctypes.c_int32 * len(PLAN_FIELDS))()
        _check(lib().lmi_debug_last_plan(self._h, w, len(PLAN_FIELDS)))
        return dict(zip(PLAN_FIELDS, (int(v) for v in w)))

    def debug_plan(self, nq: int, nb: int, k: int = 10) -> dict:
        """Test hook (`lmi_debug_plan`): the forms a scan of nq queries x nb buckets with this k would take on this handle; the
        argument checks of `scan_topk`, nothing is launched.  `overflow_sorted` depends on the handle's history: -1 here."""
        w = (ctypes.c_int32 * len(PLAN_FIELDS))()
        _check(lib().lmi_debug_plan(self._h, int(nq), int(nb), int(k), w, len(PLAN_FIELDS)))
        return dict(zip(PLAN_FIELDS, (int(v) for v in w)))

    def debug_last_mlp_plan(self) -> dict:
        """Test hook (`lmi_debug_last_mlp_plan`): the form the last MLP forward on this handle took (`mlp_topk`, `mlp_proba`, the
        MLP step of `search`), as recorded while it ran -- `MLP_PLAN_FIELDS` -> int; all zero before the first one."""
        w = (ctypes.c_int32 * len(MLP_PLAN_FIELDS))()
        _check(lib().lmi_debug_last_mlp_plan(self._h, w, len(MLP_PLAN_FIELDS)))
        return dict(zip(MLP_PLAN_FIELDS, (int(v) for v in w)))

    def debug_mlp_plan(self, nq: int, nb: int = 1, want_proba: bool = False, want_logits: bool = False) -> dict:
        """Test hook (`lmi_debug_mlp_plan`): the form `mlp_topk(q[nq], nb, want_logits)` -- or, with `want_proba`, `mlp_proba(q[nq])` --
        would take on this handle; the calls' argument checks, nothing is launched."""
        w = (ctypes.c_int32 * len(MLP_PLAN_FIELDS))()
        _check(lib().lmi_debug_mlp_plan(self._h, int(nq), int(nb), int(bool(want_proba)), int(bool(want_logits)), w, len(MLP_PLAN_FIELDS)))
        return dict(zip(MLP_PLAN_FIELDS, (int(v) for v in w)))

    def set_stream(self, stream_ptr: int) -> None:
        _check(lib().lmi_set_stream(self._h, _vp(stream_ptr)))

    # ---- MLP -------------------------------------------------------------------------------
    def set_mlp(self, layers: Sequence) -> None:
        """layers = [(W [out,in], b [out]), ...] in torch.nn.Linear layout."""
        Ws, bs, n, dims_c, Wp, bp = self._pack_layers(layers)
        _check(lib().lmi_set_mlp(self._h, n, dims_c, Wp, bp))
        self.d_nav, self.n_classes = dims_c[0], dims_c[n]

    def set_fused_mlp(self, mode: int) -> None:
        """2: always the one-launch MLP kernel, 0: always the per-layer kernels, 1 (default): by batch size; identical outputs."""
        _check(lib().lmi_set_fused_mlp(self._h, int(mode)))

    def set_stop_mass(self, mass: float) -> None:
        """Probability-mass stop of the 1-level navigation (`lmi_set_stop_mass`): 0 = off (default); 0 < mass <= 1: a
        query's bucket order keeps rank t >= 1 only while the probabilities of the ranks before it sum to less than
        `mass` (binary32, in rank order); the ranks cut are -1 = unvisited.  Anything else raises and changes nothing.
        `self.stop_mass` holds the value in force (a clone view starts with its parent's)."""
        _check(lib().lmi_set_stop_mass(self._h, ctypes.c_float(mass)))
        self.stop_mass = float(np.float32(mass))

    def set_path_mass(self, mass: float) -> None:
        """Probability-mass stop of the multi-level walk (`lmi_set_path_mass`; `nav_order`, `search_tree`): 0 = off
        (default); 0 < mass <= 1: a query's walk ends once the path probabilities (the product of the local probabilities
        along a bucket's path) of the buckets it has recorded sum to `mass` or more (binary32, in recording order); the
        slots behind the stop are -1 = unvisited.  The walk's order does not change.  Anything else raises and changes
        nothing.  `self.path_mass` holds the value in force (a clone view starts with its parent's); the 1-level calls
        ignore it, as the walk ignores `stop_mass`."""
        _check(lib().lmi_set_path_mass(self._h, ctypes.c_float(mass)))
        self.path_mass = float(np.float32(mass))

    def set_stop_rows(self, rows: int) -> None:
        """Row-budget stop (`lmi_set_stop_rows`): 0 = off (default); rows > 0: a query visits buckets in the model's order --
        the 1-level bucket order (`mlp_topk`, `search`) and the multi-level walk (`nav_order`, `search_tree`) alike -- until
        the buckets it has visited hold `rows` objects or more, counted by the index's sizes at the time of the call
        (`bucket_sizes`); the bucket that crosses the budget is scanned whole, the ranks behind it are -1 = unvisited.  With
        `stop_mass` (1-level) or `path_mass` (walk) set as well a query goes on only while both allow it.  A negative value
        raises and changes nothing.  `self.stop_rows` holds the value in force (a clone view and a subset start with it)."""
        _check(lib().lmi_set_stop_rows(self._h, ctypes.c_int64(int(rows))))
        self.stop_rows = int(rows)

    @staticmethod
    def _pack_layers(layers):
        """(W arrays, b arrays -- kept alive by the caller --, n, dims, W pointers, b pointers) as lmi_set_mlp / lmi_nav_set_model take them."""
        Ws = [_np(W, np.float32) for W, _ in layers]
        bs = [_np(b, np.float32) for _, b in layers]
        dims = [Ws[0].shape[1]] + [W.shape[0] for W in Ws]
        for i, (W, b) in enumerate(zip(Ws, bs)):
            assert W.shape == (dims[i + 1], dims[i]) and b.shape == (dims[i + 1],)
        n = len(Ws)
        return Ws, bs, n, (ctypes.c_int32 * (n + 1))(*dims), (_vp * n)(*[W.ctypes.data for W in Ws]), (_vp * n)(*[b.ctypes.data for b in bs])

    # ---- multi-level navigation ---------------------------------------------------------------
    def nav_set_model(self, model_id: int, layers: Sequence) -> None:
        """Model of an internal node (model_id >= 1; the root is set_mlp)."""
        Ws, bs, n, dims_c, Wp, bp = self._pack_layers(layers)
        _check(lib().lmi_nav_set_model(self._h, int(model_id), n, dims_c, Wp, bp))

    def nav_set_tree(self, child_offset, child_model, child_bucket) -> None:
        co, cm, cbk = _np(child_offset, np.int32), _np(child_model, np.int32), _np(child_bucket, np.int32)
        assert cm.shape == cbk.shape == (int(co[-1]),)
        _check(lib().lmi_nav_set_tree(self._h, co.shape[0] - 1, _ptr(co), _ptr(cm), _ptr(cbk)))

    def nav_order(self, queries_nav, nb: int):
        """(slab bucket ids i32[nq,nb], flat child indices i32[nq,nb]) of the multi-level walk."""
        q = _np(queries_nav, np.float32)
        slab = np.empty((q.shape[0], nb), dtype=np.int32)
        ent = np.empty((q.shape[0], nb), dtype=np.int32)
        _check(lib().lmi_nav_order(self._h, _ptr(q), q.shape[0], int(nb), _ptr(slab), _ptr(ent), 0))
        return slab, ent

    def search_tree(self, queries_nav, queries_search, nb: int, k: int = 10, want_keys: bool = False, want_order: bool = False):
        """The multi-level walk + the scan of its buckets in one call (lmi_search_tree): (dists f32[nq,kout], ids u32[nq,kout]
        [, keys] [, slab bucket ids i32[nq,nb], flat child indices i32[nq,nb]])."""
        qn, qs, f16 = _queries(queries_nav, queries_search)   # both float16: uploaded as halves (lmi_search_tree_f16)
        nq = qn.shape[0]
        ko = self.kout(nb, k)
        d = np.empty((nq, ko), dtype=np.float32)
        i = np.empty((nq, ko), dtype=np.uint32)
        keys = np.empty((nq, ko), dtype=np.uint32) if want_keys else None
        slab = np.empty((nq, nb), dtype=np.int32) if want_order else None
        ent = np.empty((nq, nb), dtype=np.int32) if want_order else None
        fn = lib().lmi_search_tree_f16 if f16 else lib().lmi_search_tree
        _check(fn(self._h, _ptr(qn), _ptr(qs), nq, int(nb), int(k), _ptr(d), _ptr(i), _ptr(keys), _ptr(slab), _ptr(ent), 0))
        out = (d, i) + ((keys,) if want_keys else ()) + ((slab, ent) if want_order else ())
        return out

    def search_tree_device(self, qn_t, qs_t, nb: int, k: int, d_t, i_t, keys_t=None, slab_t=None, ent_t=None) -> None:
        """Device tensors; both query tensors torch.float16 -> `lmi_search_tree_f16` (any 2-byte-aligned address)."""
        fn = lib().lmi_search_tree_f16 if _device_f16(qn_t, qs_t) else lib().lmi_search_tree
        _check(fn(self._h, _ptr(qn_t), _ptr(qs_t), int(qn_t.shape[0]), int(nb), int(k), _ptr(d_t), _ptr(i_t),
                                     _ptr(keys_t), _ptr(slab_t), _ptr(ent_t), 1))

    # ---- buckets ---------------------------------------------------------------------------
    def buckets_begin(self, labels, d: int, L: int, ids=None, owned=None) -> None:
        labels = _np(labels, np.int64).reshape(-1)
        ids_a = None if ids is None else _np(ids, np.uint32).reshape(-1)
        owned_a = None if owned is None else _np(owned, np.uint8).reshape(-1)
        assert ids_a is None or ids_a.shape == labels.shape
        assert owned_a is None or owned_a.shape == (L,)
        _check(lib().lmi_buckets_begin(self._h, labels.shape[0], int(d), int(L), _ptr(labels), _ptr(ids_a),
                                       _ptr(owned_a)))
        self.N, self.d, self.L = labels.shape[0], int(d), int(L)
        self.bytes_in = 0

    def add_rows(self, rows, row0: int) -> None:
        """rows: numpy [n,d] (host) or a CUDA torch tensor (device), float32 or float16.  Halves go to
        `lmi_buckets_add_rows_f16` as they are -- no host widening, half the bytes; the index is the one their widened
        values build.  Pieces of either type may be mixed within a build."""
        rows, on_device, f16 = _rows_arg(rows)
        assert rows.shape[1] == self.d
        fn = lib().lmi_buckets_add_rows_f16 if f16 else lib().lmi_buckets_add_rows
        _check(fn(self._h, _ptr(rows), int(row0), int(rows.shape[0]), on_device))
        self.bytes_in += _nbytes(rows)

    def add_owned_rows(self, rows, index) -> None:
        """Owned-only ingest: rows[i] is object index[i] (int64 original row numbers); both numpy or both CUDA tensors.
        float32 or float16 rows, as `add_rows`."""
        rows, on_device, f16 = _rows_arg(rows)
        if on_device:
            assert index.is_cuda and index.is_contiguous() and index.element_size() == 8
        else:
            index = _np(index, np.int64).reshape(-1)
        assert rows.shape[1] == self.d and index.shape[0] == rows.shape[0]
        fn = lib().lmi_buckets_add_owned_rows_f16 if f16 else lib().lmi_buckets_add_owned_rows
        _check(fn(self._h, _ptr(rows), _ptr(index), int(rows.shape[0]), on_device))
        self.bytes_in += _nbytes(rows)

    def buckets_end(self) -> None:
        _check(lib().lmi_buckets_end(self._h))

    def set_buckets(self, data, labels, L: int, ids=None, owned=None, piece: int = 1 << 18) -> None:
        data = data if not isinstance(data, np.ndarray) or data.dtype == np.float16 else _np(data, np.float32)   # halves stay halves
        self.buckets_begin(labels, data.shape[1], L, ids, owned)
        for r0 in range(0, data.shape[0], piece):
            self.add_rows(data[r0: r0 + piece], r0)
        self.buckets_end()

    def insert(self, rows, labels, ids) -> int:
        """Adds objects to the built index (`lmi_buckets_insert`): rows numpy [n,d] (host) or a CUDA torch tensor, float32
        or float16 (`lmi_buckets_insert_f16`: the halves as they are), labels int64 [n] bucket ids, ids uint32 [n].  Each goes
        after the last object of its bucket.  Returns how many were stored (objects of buckets this handle does not own are
        skipped)."""
        labels = _np(labels, np.int64).reshape(-1)
        ids_a = _np(ids, np.uint32).reshape(-1)
        rows, on_device, f16 = _rows_arg(rows)
        if not on_device:
            rows = rows.reshape(-1, self.d)
        assert rows.shape[1] == self.d and labels.shape[0] == ids_a.shape[0] == rows.shape[0]
        out = ctypes.c_int64(0)
        fn = lib().lmi_buckets_insert_f16 if f16 else lib().lmi_buckets_insert
        _check(fn(self._h, _ptr(rows), _ptr(labels), _ptr(ids_a), int(rows.shape[0]), on_device, ctypes.byref(out)))
        self.bytes_in += _nbytes(rows)
        self.N = getattr(self, "N", 0) + int(rows.shape[0])
        return out.value

    def delete(self, ids) -> int:
        """Removes every object whose id is in `ids` (`lmi_buckets_delete`); the others keep their order.  Returns how
        many were removed (ids not present are not an error)."""
        ids_a = _np(ids, np.uint32).reshape(-1)
        out = ctypes.c_int64(0)
        _check(lib().lmi_buckets_delete(self._h, _ptr(ids_a), int(ids_a.shape[0]), ctypes.byref(out)))
        self.N = getattr(self, "N", 0) - out.value
        return out.value

    def subset(self, ids, drop: bool = False) -> "Index":
        """A new, independent `Index` that holds only some of this one's objects, derived on the device (`lmi_subset`): those
        whose id is in `ids` (default) or, with `drop=True`, all but those; ids not present and duplicates are ignored
        (`drop=True` with no ids is the full copy).  It owns its models and images -- it is no clone view, this index may be
        closed, mutated or rebuilt without it noticing -- carries this one's settings, and holds exactly what a fresh build of
        the kept objects (every bucket's, in the order held here) would: same search results bit for bit, same layout.  Works on
        a `storage="f16"` index, which `delete` refuses, while clone views live, and on a clone view.  `N` is the kept count.
        Ids that are not integers or lie outside uint32 raise ValueError before the library is called."""
        a = np.asarray(ids).reshape(-1)
        if a.size and a.dtype.kind not in "iu":   # (an empty list is float64 and has nothing to truncate)
            raise ValueError(f"subset: ids must be integers, not {a.dtype}")
        if a.size and (a.min() < 0 or a.max() >= 2 ** 32):
            raise ValueError("subset: ids must fit uint32")
        ids_a = _np(a, np.uint32)
        v = self._derived()
        kept = ctypes.c_int64(0)
        _check(lib().lmi_subset(self._h, _ptr(ids_a), int(ids_a.shape[0]), 1 if drop else 0, ctypes.byref(v._h), ctypes.byref(kept)))
        v.N, v.bytes_in = kept.value, 0
        return v

    def regroup(self, ids, labels, L_new: int, bucket_map=None) -> "Index":
        """A new, independent `Index` that holds this one's objects under new bucket labels, derived on the device (`lmi_regroup`).
        An object whose id is `ids[i]` goes to bucket `labels[i]`; every other object goes to `bucket_map[its bucket]` (int [L];
        None: it keeps its bucket, which needs `L_new >= L`; an entry of -1: "this bucket must be emptied by the list").  Two objects
        that share an id both move; ids that no object carries are ignored; an id listed twice raises.  The result holds exactly what
        a fresh build of "this index's objects in the order held here (bucket ascending, then row), each with its new label" would:
        a new bucket's objects are ordered by (old bucket, old row), whatever the order of the list -- same search results bit for
        bit, same layout.  It owns its images and copies of the models, carries this one's settings, but NOT the tree tables (they
        name this index's buckets): call `set_mlp` / `nav_set_model` / `nav_set_tree` for what changed; `search` refuses a root model
        whose class count is not `L_new`, the explicit-order scans work at once.  `.n_named` on the result is the number of objects
        (not list entries) that took their label from the list.  This index is only read; works on every storage, while clone views
        live, and on one.  Bad arguments raise ValueError before the library is called (`regroup_args`)."""
        ids_a, lab_a, map_a, L_new = regroup_args(ids, labels, L_new, bucket_map, self.L)
        v = self._derived()
        named = ctypes.c_int64(0)
        _check(lib().lmi_regroup(self._h, _ptr(ids_a), _ptr(lab_a), int(ids_a.shape[0]), _ptr(map_a), L_new, ctypes.byref(v._h),
                                 ctypes.byref(named)))
        v.L, v.N, v.bytes_in, v.n_named = L_new, getattr(self, "N", None), 0, named.value
        return v

    def concat(self, *others: "Index") -> "Index":
        """A new, independent `Index` that holds this one's objects and then every one of `others`', derived on the device
        (`lmi_concat`).  All parts are built indexes over the same partition (same d, L, metric, storage, prefilter and `owned`
        mask, on one device; the library refuses anything else by name).  Bucket b of the result is this index's bucket b followed
        by `others[0]`'s bucket b and so on -- exactly what a fresh build of "this index's objects in the order held here, then
        `others[0]`'s, ..." would hold: same search results bit for bit, same layout.  It owns its images and copies of THIS
        index's models and tree (the others' models are ignored) and carries this one's settings.  How a `storage="f16"` index,
        which `insert` refuses, grows: build the new objects as a small index, concatenate, close the small one; the library
        refuses (`LmiError`) if the larger scale of the result would push a stored half below the binary16 subnormals, as a fresh
        build of the same rows would.  Without `others` the result is this index's compaction (`subset([], drop=True)`).  A part
        may be passed twice.  The parts are only read: works while clone views live, and on them.  `N` is the stored objects.
        Arguments that are no open `Index`, or more than `CONCAT_MAX_PARTS` parts, raise ValueError before the library is called."""
        parts = concat_args(self, others)
        v = self._derived()
        total = ctypes.c_int64(0)
        handles = (_vp * len(parts))(*[p._h.value if isinstance(p._h, _vp) else p._h for p in parts])
        _check(lib().lmi_concat(handles, len(parts), ctypes.byref(v._h), ctypes.byref(total)))
        v.N, v.bytes_in = total.value, 0
        return v

    def bucket_sizes(self) -> np.ndarray:
        out = np.zeros(self.L, dtype=np.int64)
        _check(lib().lmi_bucket_sizes(self._h, _ptr(out)))
        return out

    # ---- query path, host arrays ------------------------------------------------------------
    def mlp_topk(self, queries_nav, nb: int, want_logits: bool = False):
        f16 = _is_f16(queries_nav)   # float16 queries are uploaded as halves (lmi_mlp_topk_f16) and widened on the device
        q = _np(queries_nav, np.float16 if f16 else np.float32)
        order = np.empty((q.shape[0], nb), dtype=np.int32)
        logits = np.empty((q.shape[0], self.n_classes), dtype=np.float32) if want_logits else None
        fn = lib().lmi_mlp_topk_f16 if f16 else lib().lmi_mlp_topk
        _check(fn(self._h, _ptr(q), q.shape[0], int(nb), _ptr(order), _ptr(logits), 0))
        return (order, logits) if want_logits else order

    def mlp_proba(self, queries_nav):
        """(probs f32[n,L] descending, classes i32[n,L]) -- NeuralNetwork.predict_proba."""
        q = _np(queries_nav, np.float32)
        probs = np.empty((q.shape[0], self.n_classes), dtype=np.float32)
        classes = np.empty((q.shape[0], self.n_classes), dtype=np.int32)
        _check(lib().lmi_mlp_proba(self._h, _ptr(q), q.shape[0], _ptr(probs), _ptr(classes), 0))
        return probs, classes

    @staticmethod
    def kout(nb: int, k: int) -> int:
        return K_PER_BUCKET if nb == 1 else k

    def scan_topk(self, queries_search, bucket_order, k: int = 10, want_keys: bool = False):
        f16 = _is_f16(queries_search)   # float16 queries are uploaded as halves (lmi_scan_topk_f16) and widened on the device
        q = _np(queries_search, np.float16 if f16 else np.float32)
        bo = _np(bucket_order, np.int32).reshape(q.shape[0], -1)
        nb = bo.shape[1]
        ko = self.kout(nb, k)
        d = np.empty((q.shape[0], ko), dtype=np.float32)
        i = np.empty((q.shape[0], ko), dtype=np.uint32)
        keys = np.empty((q.shape[0], ko), dtype=np.uint32) if want_keys else None
        fn = lib().lmi_scan_topk_f16 if f16 else lib().lmi_scan_topk
        _check(fn(self._h, _ptr(q), q.shape[0], _ptr(bo), nb, int(k), _ptr(d), _ptr(i), _ptr(keys), 0))
        return (d, i, keys) if want_keys else (d, i)

    def search(self, queries_nav, queries_search, nb: int, k: int = 10, want_keys: bool = False):
        qn, qs, f16 = _queries(queries_nav, queries_search)   # both float16: uploaded as halves (lmi_search_f16)
        nq = qn.shape[0]
        ko = self.kout(nb, k)
        d = np.empty((nq, ko), dtype=np.float32)
        i = np.empty((nq, ko), dtype=np.uint32)
        bo = np.empty((nq, nb), dtype=np.int32)
        keys = np.empty((nq, ko), dtype=np.uint32) if want_keys else None
        fn = lib().lmi_search_f16 if f16 else lib().lmi_search
        _check(fn(self._h, _ptr(qn), _ptr(qs), nq, int(nb), int(k), _ptr(d), _ptr(i), _ptr(keys), _ptr(bo), 0))
        return (d, i, bo, keys) if want_keys else (d, i, bo)

    # ---- the union scan: the k best objects of the union of a query's visited buckets, k <= UNION_MAX_K (include/lmi_hip.h) ----
    @staticmethod
    def _union_args(who: str, k: int, nb: int, **arrays) -> None:
        """Argument errors of the union calls, raised before the library loads."""
        if not isinstance(k, (int, np.integer)) or k < 1 or k > UNION_MAX_K:
            raise ValueError(f"{who}: k {k!r} outside [1, {UNION_MAX_K}]")
        if not isinstance(nb, (int, np.integer)) or nb < 1 or nb > 1024:
            raise ValueError(f"{who}: n_buckets {nb!r} outside [1, 1024]")
        for name, a in arrays.items():
            if a is None or not hasattr(a, "shape") or len(a.shape) != 2:
                raise ValueError(f"{who}: {name} must be a two-dimensional array")
        rows = {int(a.shape[0]) for a in arrays.values()}
        if len(rows) > 1:
            raise ValueError(f"{who}: the arrays disagree about the number of queries ({sorted(rows)})")

    @staticmethod
    def _filter_args(who: str, filter, filter_of, nq: int):
        """(filter handle, filter_of i32[nq] or None) of a filtered union call; argument errors are raised before the library loads.
        `filter_of` stays on the host also for the `_device` forms."""
        if filter is None:
            if filter_of is not None:
                raise ValueError(f"{who}: filter_of without a filter")
            return None, None
        if not isinstance(filter, Filter):
            raise ValueError(f"{who}: filter must be a _capi.Filter, not {type(filter).__name__}")
        if getattr(filter, "_f", None) is None:
            raise ValueError(f"{who}: the filter is closed")
        if filter_of is None:
            return filter._f, None
        fo = np.asarray(filter_of.cpu().numpy() if hasattr(filter_of, "cpu") else filter_of)
        if fo.ndim != 1 or fo.shape[0] != nq or fo.dtype.kind not in "iu":
            raise ValueError(f"{who}: filter_of must be one integer per query ([{nq}]), not {fo.dtype}{tuple(fo.shape)}")
        if fo.size and (fo.min() < -1 or fo.max() >= filter.nf):
            raise ValueError(f"{who}: filter_of holds a value outside [-1, {filter.nf})")
        return filter._f, _np(fo, np.int32)

    def _union_call(self, name: str, args: tuple, f, fo) -> None:
        """`name(handle, *args)`, or with a filter `name_filtered(handle, *args, filter, filter_of)`."""
        if f is None:
            _check(getattr(lib(), name)(self._h, *args))
        else:
            _check(getattr(lib(), name + "_filtered")(self._h, *args, f, _ptr(fo)))

    #: the three forms of a union or range call: what the library's name begins with, what its two arrays are called, its order outputs
    _FORMS = {"scan": ("lmi_scan", ("queries_search", "bucket_order"), 0),
              "search": ("lmi_search", ("queries_nav", "queries_search"), 1),
              "search_tree": ("lmi_search_tree", ("queries_nav", "queries_search"), 2)}

    @staticmethod
    def _form_inputs(form: str, first, second, nb: int, orders):
        """(head, orders, nq, keep) of a union or range call whose argument checks have passed.  `first`, `second`: the form's two arrays
        (`_FORMS`).  `orders` None: host arrays -- float32 queries (one array where the caller passed one twice), an int32 bucket order, and
        the form's order outputs i32[nq,nb] are made here; otherwise device tensors, taken as they are, with the caller's order outputs.
        `head`: the library's arguments up to n_buckets; `keep`: the arrays `head` points into."""
        if orders is None:
            same = second is first
            first = _np(first, np.float32)
            second = _np(second, np.int32) if form == "scan" else first if same else _np(second, np.float32)
            orders = tuple(np.empty((first.shape[0], nb), dtype=np.int32) for _ in range(Index._FORMS[form][2]))
        nq = int(first.shape[0])
        head = (_ptr(first), nq, _ptr(second), int(nb)) if form == "scan" else (_ptr(first), _ptr(second), nq, int(nb))
        return head, orders, nq, (first, second)

    def _union(self, form: str, first, second, nb: int, k: int, filter, filter_of, outs=None, orders=None):
        """A union call of one form: on host arrays (`outs` None) the outputs are made here and returned with the form's orders."""
        host = outs is None
        who = f"{form}_union" if host else f"{form}_union_device"
        self._union_args(who, k, nb, **dict(zip(self._FORMS[form][1], (first, second))))
        head, orders, nq, _keep = self._form_inputs(form, first, second, nb, None if host else orders)   # (_keep: alive until the call returns)
        if host:
            outs = (np.empty((nq, k), dtype=np.float32), np.empty((nq, k), dtype=np.uint32), np.empty((nq,), dtype=np.int32))
        f, fo = self._filter_args(who, filter, filter_of, nq)
        self._union_call(self._FORMS[form][0] + "_union", head + (int(k),) + tuple(_ptr(x) for x in outs + orders) + (0 if host else 1,), f, fo)
        return outs + orders if host else None

    def scan_union(self, queries_search, bucket_order, k: int = 10, filter=None, filter_of=None):
        """(dists f32[nq,k], ids u32[nq,k], counts i32[nq]) of `lmi_scan_union`: per query the k best objects of the union of the
        buckets `bucket_order[q]` lists (-1: none); behind `counts[q]` real results dist = +inf, id = 0.
        `filter` (a `Filter` made on this index) restricts every query's candidates to the rows its filter allows
        (`lmi_scan_union_filtered`): query q uses filter `filter_of[q]` (int, -1 = unfiltered; None = all use filter 0).  The same two
        keywords on `search_union`, `search_tree_union` and the `_device` forms, where `filter_of` stays a host array."""
        if not hasattr(bucket_order, "shape") or len(bucket_order.shape) != 2:
            raise ValueError("scan_union: bucket_order must be a two-dimensional array")
        return self._union("scan", queries_search, bucket_order, int(bucket_order.shape[1]), k, filter, filter_of)

    def search_union(self, queries_nav, queries_search, nb: int, k: int = 10, filter=None, filter_of=None):
        """`lmi_search_union`: (dists, ids, counts, bucket order i32[nq,nb]).  `filter`, `filter_of`: as in `scan_union`."""
        return self._union("search", queries_nav, queries_search, nb, k, filter, filter_of)

    def search_tree_union(self, queries_nav, queries_search, nb: int, k: int = 10, filter=None, filter_of=None):
        """`lmi_search_tree_union`: (dists, ids, counts, slab bucket ids i32[nq,nb], flat child indices i32[nq,nb]).  `filter`,
        `filter_of`: as in `scan_union`."""
        return self._union("search_tree", queries_nav, queries_search, nb, k, filter, filter_of)

    def scan_union_device(self, qs_t, bo_t, nb: int, k: int, d_t, i_t, counts_t=None, filter=None, filter_of=None) -> None:
        """Device tensors (float32 queries, int32 order, float32 / uint32-sized / int32 outputs); returns when they have landed."""
        self._union("scan", qs_t, bo_t, nb, k, filter, filter_of, (d_t, i_t, counts_t), ())

    def search_union_device(self, qn_t, qs_t, nb: int, k: int, d_t, i_t, counts_t=None, bo_t=None, filter=None, filter_of=None) -> None:
        self._union("search", qn_t, qs_t, nb, k, filter, filter_of, (d_t, i_t, counts_t), (bo_t,))

    def search_tree_union_device(self, qn_t, qs_t, nb: int, k: int, d_t, i_t, counts_t=None, slab_t=None, ent_t=None, filter=None,
                                 filter_of=None) -> None:
        self._union("search_tree", qn_t, qs_t, nb, k, filter, filter_of, (d_t, i_t, counts_t), (slab_t, ent_t))

    # ---- the range search: every object of the visited buckets within a radius, in ordinal order (include/lmi_hip.h, lmi_scan_range) ----
    @staticmethod
    def _range_args(who: str, nb: int, radius, max_total, **arrays) -> np.ndarray:
        """radius f32[nq] of a range call (a scalar serves every query); argument errors are raised before the library loads."""
        Index._union_args(who, 1, nb, **arrays)
        nq = int(next(iter(arrays.values())).shape[0])
        if radius is None:
            raise ValueError(f"{who}: radius is None")
        r = np.asarray(radius.cpu().numpy() if hasattr(radius, "cpu") else radius)
        if r.dtype.kind not in "fiu" or r.ndim > 1 or (r.ndim == 1 and r.shape[0] != nq):
            raise ValueError(f"{who}: radius must be a number or one number per query ([{nq}]), not {r.dtype}{tuple(r.shape)}")
        if isinstance(max_total, bool) or not isinstance(max_total, (int, np.integer)) or max_total < 0:
            raise ValueError(f"{who}: max_total {max_total!r} must be an integer >= 0 (0: no limit)")
        return np.ascontiguousarray(np.broadcast_to(r.astype(np.float32), (nq,)))

    #: the range calls take `sort=True`: every query's results come back nearest first, sorted on the device (`lmi_range_result_sort`)
    range_sort = True

    def _range_call(self, name: str, head: tuple, radius, f, fo, max_total: int, tail: tuple, sort: bool = False) -> "RangeResult":
        res = _vp()
        _check(getattr(lib(), name)(self._h, *head, _ptr(radius), f, _ptr(fo), int(max_total), ctypes.byref(res), *tail))
        out = RangeResult(res, int(radius.shape[0]))
        if sort:
            try:
                out.sort(self)
            except Exception:
                out.close()
                raise
        return out

    def _range(self, form: str, first, second, nb: int, radius, filter, filter_of, max_total, sort, orders=None):
        """A range call of one form: on host arrays (`orders` None) the result is read, closed and returned with the form's orders; on
        device tensors the `RangeResult` is returned."""
        host = orders is None
        who = f"{form}_range" if host else f"{form}_range_device"
        r = self._range_args(who, nb, radius, max_total, **dict(zip(self._FORMS[form][1], (first, second))))
        head, orders, nq, _keep = self._form_inputs(form, first, second, nb, orders)
        f, fo = self._filter_args(who, filter, filter_of, nq)
        res = self._range_call(self._FORMS[form][0] + "_range", head, r, f, fo, max_total, tuple(_ptr(x) for x in orders) + (0 if host else 1,), sort)
        if not host:
            return res
        with res:
            return (res.lims,) + res.read() + orders

    def scan_range(self, queries_search, bucket_order, radius, filter=None, filter_of=None, max_total: int = 0, sort: bool = False):
        """(lims i64[nq + 1], dists f32[total], ids u32[total]) of `lmi_scan_range`: per query every object of the buckets
        `bucket_order[q]` lists (-1: none) whose distance is <= `radius` (a number, or one per query), in (rank, row) order; query q owns
        [lims[q], lims[q + 1]).  `filter`, `filter_of`: as in `scan_union`.  `max_total` > 0: the call fails (LmiError) once more results
        than that have been counted.  `sort=True` (all six range calls): every query's results stably sorted by distance on the device
        (`RangeResult.sort`) before they are read or returned."""
        if not hasattr(bucket_order, "shape") or len(bucket_order.shape) != 2:
            raise ValueError("scan_range: bucket_order must be a two-dimensional array")
        return self._range("scan", queries_search, bucket_order, int(bucket_order.shape[1]), radius, filter, filter_of, max_total, sort)

    def search_range(self, queries_nav, queries_search, nb: int, radius, filter=None, filter_of=None, max_total: int = 0,
                     sort: bool = False):
        """`lmi_search_range`: (lims, dists, ids, bucket order i32[nq,nb])."""
        return self._range("search", queries_nav, queries_search, nb, radius, filter, filter_of, max_total, sort)

    def search_tree_range(self, queries_nav, queries_search, nb: int, radius, filter=None, filter_of=None, max_total: int = 0,
                          sort: bool = False):
        """`lmi_search_tree_range`: (lims, dists, ids, slab bucket ids i32[nq,nb], flat child indices i32[nq,nb])."""
        return self._range("search_tree", queries_nav, queries_search, nb, radius, filter, filter_of, max_total, sort)

    def scan_range_device(self, qs_t, bo_t, nb: int, radius, filter=None, filter_of=None, max_total: int = 0,
                          sort: bool = False) -> "RangeResult":
        """Device tensors (float32 queries, int32 order); `radius` and `filter_of` stay on the host.  Returns the `RangeResult`, whose
        arrays stay on the device until `read()` / `read_into()`."""
        return self._range("scan", qs_t, bo_t, nb, radius, filter, filter_of, max_total, sort, ())

    def search_range_device(self, qn_t, qs_t, nb: int, radius, bo_t=None, filter=None, filter_of=None, max_total: int = 0,
                            sort: bool = False) -> "RangeResult":
        return self._range("search", qn_t, qs_t, nb, radius, filter, filter_of, max_total, sort, (bo_t,))

    def search_tree_range_device(self, qn_t, qs_t, nb: int, radius, slab_t=None, ent_t=None, filter=None, filter_of=None,
                                 max_total: int = 0, sort: bool = False) -> "RangeResult":
        return self._range("search_tree", qn_t, qs_t, nb, radius, filter, filter_of, max_total, sort, (slab_t, ent_t))

    # ---- the exact range search: buckets pruned by covering balls (include/lmi_hip.h, lmi_cover_create / lmi_search_range_exact) ----
    def _cover_args(self, who: str, queries, radius, cover, device: bool) -> np.ndarray:
        """radius f32[nq] of a call that takes a cover; argument errors are raised before the library loads."""
        if getattr(self, "_h", None) is None or not self._h:
            raise ValueError(f"{who}: the index is closed")
        if not isinstance(cover, Cover):
            raise ValueError(f"{who}: cover must be a _capi.Cover, not {type(cover).__name__}")
        if getattr(cover, "_c", None) is None:
            raise ValueError(f"{who}: the cover is closed")
        if queries is None or not hasattr(queries, "shape") or len(queries.shape) != 2:
            raise ValueError(f"{who}: queries_search must be a two-dimensional array")
        if device:
            if not (hasattr(queries, "is_cuda") and queries.is_cuda and queries.is_contiguous() and str(queries.dtype) == "torch.float32"):
                raise ValueError(f"{who}: queries_search must be a contiguous float32 tensor on the device")
        elif hasattr(queries, "is_cuda"):
            raise ValueError(f"{who}: queries_search must be a numpy array (device tensors go to {who}_device)")
        if self.d is not None and int(queries.shape[1]) != int(self.d):
            raise ValueError(f"{who}: queries_search has {int(queries.shape[1])} columns, the index {int(self.d)}")
        return self._range_args(who, 1, radius, 0, queries_search=queries)

    @staticmethod
    def _cover_nb(who: str, nb):
        if nb is None:
            return None
        if isinstance(nb, bool) or not isinstance(nb, (int, np.integer)) or nb < 1:
            raise ValueError(f"{who}: nb {nb!r} must be an integer >= 1, or None to size the order by the counts")
        return int(nb)

    def cover_order(self, queries_search, radius, cover: "Cover", nb: Optional[int] = None):
        """(order i32[nq, nb], counts i32[nq]) of `lmi_cover_order`: per query the buckets that may hold an object within `radius` (a
        number, or one per query), in ascending bucket id, then -1.  `nb=None` counts first and sizes the order by the largest count
        (at least 1); a given `nb` that some query exceeds is refused (LmiError) and nothing is returned."""
        nb = self._cover_nb("cover_order", nb)
        r = self._cover_args("cover_order", queries_search, radius, cover, False)
        q = _np(queries_search, np.float32)
        nq = int(q.shape[0])
        counts = np.zeros(nq, dtype=np.int32)
        if nb is None:
            _check(lib().lmi_cover_order(self._h, cover._c, _ptr(q), nq, _ptr(r), 0, None, _ptr(counts), 0))
            nb = max(1, int(counts.max()) if nq else 1)
        order = np.full((nq, nb), -1, dtype=np.int32)
        _check(lib().lmi_cover_order(self._h, cover._c, _ptr(q), nq, _ptr(r), nb, _ptr(order), _ptr(counts), 0))
        return order, counts

    def cover_order_device(self, qs_t, radius, cover: "Cover", nb: int, order_t=None, counts_t=None) -> None:
        """Device tensors: float32 queries, `order_t` int32 [nq, nb] and `counts_t` int32 [nq] (each may be None); `radius` stays on the
        host.  Returns when they have landed."""
        nb = self._cover_nb("cover_order_device", nb if order_t is not None else (nb or 1))
        r = self._cover_args("cover_order_device", qs_t, radius, cover, True)
        nq = int(qs_t.shape[0])
        for name, t, shape in (("order_t", order_t, (nq, nb)), ("counts_t", counts_t, (nq,))):
            if t is not None and not (hasattr(t, "is_cuda") and t.is_cuda and t.is_contiguous() and str(t.dtype) == "torch.int32"
                                      and tuple(t.shape) == shape):
                raise ValueError(f"cover_order_device: {name} must be a contiguous int32 device tensor of shape {shape}")
        _check(lib().lmi_cover_order(self._h, cover._c, _ptr(qs_t), nq, _ptr(r), nb, _ptr(order_t), _ptr(counts_t), 1))

    def _range_exact(self, who: str, queries, radius, cover, filter, filter_of, max_total, sort, counts, on_device: int) -> "RangeResult":
        r = self._cover_args(who, queries, radius, cover, bool(on_device))
        if isinstance(max_total, bool) or not isinstance(max_total, (int, np.integer)) or max_total < 0:
            raise ValueError(f"{who}: max_total {max_total!r} must be an integer >= 0 (0: no limit)")
        nq = int(queries.shape[0])
        f, fo = self._filter_args(who, filter, filter_of, nq)
        res, nb_used = _vp(), ctypes.c_int32(0)
        _check(lib().lmi_search_range_exact(self._h, cover._c, _ptr(queries), nq, _ptr(r), f, _ptr(fo), int(max_total), ctypes.byref(res),
                                            ctypes.byref(nb_used), _ptr(counts), on_device))
        out = RangeResult(res, nq)
        out.nb_used = int(nb_used.value)
        if sort:
            try:
                out.sort(self)
            except Exception:
                out.close()
                raise
        return out

    def search_range_exact(self, queries_search, radius, cover: "Cover", filter=None, filter_of=None, max_total: int = 0,
                           sort: bool = False):
        """(lims i64[nq + 1], dists f32[total], ids u32[total]) of `lmi_search_range_exact`: per query EVERY object this handle stores
        whose distance is <= `radius` (a number, or one per query), in (bucket, row) order -- as sets what `range_knn` gives over all
        stored objects -- while only the buckets whose covering ball the query's ball may meet are scanned.  `cover`: a `Cover` made on
        this index (or on the index this one is a clone view of).  `filter`, `filter_of`, `max_total`, `sort`: as in `scan_range`."""
        q = queries_search
        self._cover_args("search_range_exact", q, radius, cover, False)
        q = _np(q, np.float32)
        with self._range_exact("search_range_exact", q, radius, cover, filter, filter_of, max_total, sort, None, 0) as res:
            return (res.lims,) + res.read()

    def search_range_exact_device(self, qs_t, radius, cover: "Cover", filter=None, filter_of=None, max_total: int = 0, sort: bool = False,
                                  counts_t=None) -> "RangeResult":
        """Device tensors (float32 queries; `counts_t` int32 [nq] or None <- the buckets admitted per query); `radius` and `filter_of`
        stay on the host.  Returns the `RangeResult` (its `nb_used`: the buckets per query of the scan), whose arrays stay on the device
        until `read()` / `read_into()`."""
        if counts_t is not None and not (hasattr(counts_t, "is_cuda") and counts_t.is_cuda and counts_t.is_contiguous()
                                         and str(counts_t.dtype) == "torch.int32" and hasattr(qs_t, "shape")
                                         and tuple(counts_t.shape) == (int(qs_t.shape[0]),)):
            raise ValueError("search_range_exact_device: counts_t must be a contiguous int32 device tensor of shape (nq,)")
        return self._range_exact("search_range_exact_device", qs_t, radius, cover, filter, filter_of, max_total, sort, counts_t, 1)

    # ---- the range search across ranks: the join of the ranks' parts (include/lmi_hip.h, lmi_join_range_parts) ----
    @staticmethod
    def _range_join_args(who: str, counts, dists, ids, max_total):
        """(counts i32[world, nq, nb] contiguous, on_device) of a join; argument errors are raised before the library loads."""
        if not isinstance(counts, np.ndarray) or counts.ndim != 3 or counts.dtype.kind not in "iu":
            raise ValueError(f"{who}: counts must be an integer numpy array [world, nq, nb] on the host")
        world, nq, nb = (int(x) for x in counts.shape)
        if world < 1 or world > 64:
            raise ValueError(f"{who}: world {world} outside [1, 64]")
        if nb < 1 or nb > 1024:
            raise ValueError(f"{who}: nb {nb} outside [1, 1024]")
        if nq * nb >= 1 << 31:
            raise ValueError(f"{who}: nq * nb = {nq * nb} is too large")
        if isinstance(max_total, bool) or not isinstance(max_total, (int, np.integer)) or max_total < 0:
            raise ValueError(f"{who}: max_total {max_total!r} must be an integer >= 0 (0: no limit)")
        for name, arrs in (("dists", dists), ("ids", ids)):
            if not isinstance(arrs, (list, tuple)) or len(arrs) != world:
                raise ValueError(f"{who}: {name} must be a list of {world} arrays, one per part (None for a part without results)")
        present = [a for a in list(dists) + list(ids) if a is not None]
        host = [isinstance(a, np.ndarray) for a in present]
        if any(host) and not all(host):
            raise ValueError(f"{who}: the parts must be all numpy arrays or all tensors on the device")
        totals = counts.astype(np.int64).reshape(world, -1).sum(axis=1)
        for r in range(world):
            for name, a in (("dists", dists[r]), ("ids", ids[r])):
                if a is None:
                    if totals[r] > 0:
                        raise ValueError(f"{who}: part {r} holds {int(totals[r])} results and its {name} is None")
                    continue
                if not isinstance(a, np.ndarray) and not (hasattr(a, "is_cuda") and a.is_cuda and a.is_contiguous() and a.element_size() == 4):
                    raise ValueError(f"{who}: {name}[{r}] must be a numpy array or a contiguous tensor of 4-byte elements on the device")
                if len(a.shape) != 1 or int(a.shape[0]) < totals[r]:
                    raise ValueError(f"{who}: {name}[{r}] must be one-dimensional with >= {int(totals[r])} elements, not {tuple(a.shape)}")
        return np.ascontiguousarray(counts, dtype=np.int32), (0 if all(host) else 1)

    def join_range_parts(self, counts, dists, ids, max_total: int = 0) -> "RangeResult":
        """`lmi_join_range_parts`: counts i32[world, nq, nb] (host), `dists` / `ids` lists of the parts' arrays (all numpy: host pointers;
        all tensors: device pointers; None for a part without results) -> the `RangeResult` one handle holding every bucket returns."""
        c, on_device = self._range_join_args("join_range_parts", counts, dists, ids, max_total)
        world, nq, nb = c.shape
        if on_device == 0:
            dists = [None if a is None else _np(a, np.float32) for a in dists]
            ids = [None if a is None else _np(a, np.uint32) for a in ids]
        pd = (_vp * world)(*[_ptr(a) for a in dists])
        pi = (_vp * world)(*[_ptr(a) for a in ids])
        res = _vp()
        _check(lib().lmi_join_range_parts(self._h, world, nq, nb, _ptr(c), pd, pi, int(max_total), ctypes.byref(res), on_device))
        return RangeResult(res, nq)

    def allgather_join_range(self, comm, rank: int, world: int, part: "RangeResult", max_total: int = 0) -> "RangeResult":
        """This rank's `RangeResult` (of `scan_range_device` on its owned buckets) -> the joined result on every rank
        (`lmi_allgather_join_range`: two ncclAllGather calls and one stream synchronisation between them)."""
        who = "allgather_join_range"
        if not isinstance(world, (int, np.integer)) or world < 1 or world > 64:
            raise ValueError(f"{who}: world {world!r} outside [1, 64]")
        if not isinstance(rank, (int, np.integer)) or rank < 0 or rank >= world:
            raise ValueError(f"{who}: rank {rank!r} of {world}")
        if comm is None or not isinstance(part, RangeResult):
            raise ValueError(f"{who}: comm must not be None and part must be a RangeResult")
        if isinstance(max_total, bool) or not isinstance(max_total, (int, np.integer)) or max_total < 0:
            raise ValueError(f"{who}: max_total {max_total!r} must be an integer >= 0 (0: no limit)")
        res = _vp()
        _check(lib().lmi_allgather_join_range(self._h, comm, int(rank), int(world), part._open(), int(max_total), ctypes.byref(res)))
        return RangeResult(res, part.nq)

    @staticmethod
    def set_range_join_geometry(piece_rows: int = 0) -> None:
        """Test hook (`lmi_range_join_set_geometry`): the most results of one copy piece of the joins on this thread; 0 = the default.
        Never changes a result."""
        if isinstance(piece_rows, bool) or not isinstance(piece_rows, (int, np.integer)) or piece_rows < 0 or piece_rows > 1 << 30:
            raise ValueError(f"set_range_join_geometry: piece_rows {piece_rows!r} outside [0, 2^30]")
        _check(lib().lmi_range_join_set_geometry(int(piece_rows)))

    # ---- the union scan across ranks: a rank's part and the merge of the parts (include/lmi_hip.h, lmi_scan_union_part) ----
    @staticmethod
    def _union_merge_args(who: str, world, nq, k) -> None:
        """Argument errors of the merges of union parts, raised before the library loads."""
        if not isinstance(world, (int, np.integer)) or world < 1 or world > 64:
            raise ValueError(f"{who}: world {world!r} outside [1, 64]")
        if not isinstance(k, (int, np.integer)) or k < 1 or k > UNION_MAX_K:
            raise ValueError(f"{who}: k {k!r} outside [1, {UNION_MAX_K}]")
        if not isinstance(nq, (int, np.integer)) or nq < 0:
            raise ValueError(f"{who}: nq {nq!r} is negative")

    def scan_union_part(self, queries_search, bucket_order, k: int = 10):
        """(part i32[5, nq, k], counts i32[nq]) of `lmi_scan_union_part`: this handle's part of the union scan -- score bits, dist bits,
        ids, ranks and rows per result (the `UPART_*` planes), padding behind `counts[q]` real results."""
        if not hasattr(bucket_order, "shape") or len(bucket_order.shape) != 2:
            raise ValueError("scan_union_part: bucket_order must be a two-dimensional array")
        nb = int(bucket_order.shape[1])
        self._union_args("scan_union_part", k, nb, queries_search=queries_search, bucket_order=bucket_order)
        q = _np(queries_search, np.float32)
        bo = _np(bucket_order, np.int32)
        nq = q.shape[0]
        part = np.empty((UNION_PART_PLANES, nq, k), dtype=np.int32)
        c = np.empty((nq,), dtype=np.int32)
        _check(lib().lmi_scan_union_part(self._h, _ptr(q), nq, _ptr(bo), nb, int(k), _ptr(part), _ptr(c), 0))
        return part, c

    def scan_union_part_device(self, qs_t, bo_t, nb: int, k: int, part_t, counts_t=None) -> None:
        """Device tensors (float32 queries, int32 order, a contiguous int32 [5, nq, k] part); returns when they have landed."""
        self._union_args("scan_union_part_device", k, nb, queries_search=qs_t, bucket_order=bo_t)
        if part_t is None or tuple(part_t.shape) != (UNION_PART_PLANES, int(qs_t.shape[0]), int(k)):
            raise ValueError(f"scan_union_part_device: part must be [{UNION_PART_PLANES}, nq, k]")
        _check(lib().lmi_scan_union_part(self._h, _ptr(qs_t), int(qs_t.shape[0]), _ptr(bo_t), int(nb), int(k), _ptr(part_t), _ptr(counts_t), 1))

    def merge_union_parts(self, parts, world: int, nq: int, k: int, out_d, out_i, counts=None) -> None:
        """`lmi_merge_union_parts`: parts [world, 5, nq, k] int32, dense (numpy: host pointers, the call returns with the result;
        torch: device pointers, asynchronous on the handle's stream) -> out_d f32[nq, k], out_i u32[nq, k], counts i32[nq]."""
        self._union_merge_args("merge_union_parts", world, nq, k)
        if parts is None or out_d is None or out_i is None:
            raise ValueError("merge_union_parts: parts, out_d and out_i must not be None")
        if int(np.prod(tuple(parts.shape))) != world * UNION_PART_PLANES * nq * k:
            raise ValueError(f"merge_union_parts: parts must hold [world, {UNION_PART_PLANES}, nq, k] words, not {tuple(parts.shape)}")
        on_device = 0 if isinstance(parts, np.ndarray) else 1
        if on_device == 0:
            parts = _np(parts, np.int32)
        _check(lib().lmi_merge_union_parts(self._h, _ptr(parts), int(world), int(nq), int(k), _ptr(out_d), _ptr(out_i), _ptr(counts), on_device))

    def allgather_merge_union(self, comm, rank: int, world: int, part_t, out_d_t, out_i_t, counts_t=None) -> None:
        """This rank's [5, nq, k] device part -> merged (dists, ids, counts) on every rank (`lmi_allgather_merge_union`)."""
        if part_t is None or len(part_t.shape) != 3 or int(part_t.shape[0]) != UNION_PART_PLANES:
            raise ValueError(f"allgather_merge_union: part must be [{UNION_PART_PLANES}, nq, k]")
        nq, k = int(part_t.shape[1]), int(part_t.shape[2])
        self._union_merge_args("allgather_merge_union", world, nq, k)
        if not isinstance(rank, (int, np.integer)) or rank < 0 or rank >= world:
            raise ValueError(f"allgather_merge_union: rank {rank!r} of {world}")
        if comm is None or out_d_t is None or out_i_t is None:
            raise ValueError("allgather_merge_union: comm, out_d and out_i must not be None")
        _check(lib().lmi_allgather_merge_union(self._h, comm, int(rank), int(world), _ptr(part_t), nq, k, _ptr(out_d_t), _ptr(out_i_t),
                                               _ptr(counts_t)))

    # ---- query path, device tensors (torch), asynchronous on the handle's stream --------------
    def search_device(self, qn_t, qs_t, nb: int, k: int, d_t, i_t, keys_t=None, bo_t=None) -> None:
        """Device tensors; both query tensors torch.float16 -> `lmi_search_f16`: they are widened into the handle's buffers."""
        fn = lib().lmi_search_f16 if _device_f16(qn_t, qs_t) else lib().lmi_search
        _check(fn(self._h, _ptr(qn_t), _ptr(qs_t), int(qn_t.shape[0]), int(nb), int(k), _ptr(d_t),
                                _ptr(i_t), _ptr(keys_t), _ptr(bo_t), 1))

    def mlp_topk_device(self, qn_t, nb: int, bo_t, logits_t=None) -> None:
        """A contiguous torch.float16 query tensor -> `lmi_mlp_topk_f16` (any 2-byte-aligned address)."""
        fn = lib().lmi_mlp_topk_f16 if _device_f16(qn_t, qn_t) else lib().lmi_mlp_topk
        _check(fn(self._h, _ptr(qn_t), int(qn_t.shape[0]), int(nb), _ptr(bo_t), _ptr(logits_t), 1))

    def scan_topk_device(self, qs_t, bo_t, nb: int, k: int, d_t, i_t, keys_t=None) -> None:
        fn = lib().lmi_scan_topk_f16 if _device_f16(qs_t, qs_t) else lib().lmi_scan_topk
        _check(fn(self._h, _ptr(qs_t), int(qs_t.shape[0]), _ptr(bo_t), int(nb), int(k), _ptr(d_t),
                                   _ptr(i_t), _ptr(keys_t), 1))

    def merge_gathered(self, gd, gi, gk, world: int, nq: int, kout: int, out_d, out_i, world_stride: int = 0) -> None:
        on_device = 0 if isinstance(gd, np.ndarray) else 1
        _check(lib().lmi_merge_gathered(self._h, _ptr(gd), _ptr(gi), _ptr(gk), int(world), int(world_stride),
                                        int(nq), int(kout), _ptr(out_d), _ptr(out_i), on_device))

    def copy_out(self, dst_pinned_t, src_dev_t) -> None:
        """src (device tensor) -> dst (pinned host tensor of the same byte size) by a kernel on the handle's stream."""
        nbytes = src_dev_t.numel() * src_dev_t.element_size()
        assert dst_pinned_t.is_pinned() and dst_pinned_t.numel() * dst_pinned_t.element_size() == nbytes
        assert src_dev_t.is_contiguous() and dst_pinned_t.is_contiguous()
        _check(lib().lmi_copy_out(self._h, _ptr(dst_pinned_t), _ptr(src_dev_t), nbytes))

    def copy_out_many(self, pairs) -> None:
        """[(dst pinned host tensor, src device tensor), ..] (up to 4) by ONE kernel on the handle's stream."""
        n = len(pairs)
        dst = (ctypes.c_void_p * n)()
        src = (ctypes.c_void_p * n)()
        nby = (ctypes.c_int64 * n)()
        for i, (d_t, s_t) in enumerate(pairs):
            nbytes = s_t.numel() * s_t.element_size()
            assert d_t.is_pinned() and d_t.numel() * d_t.element_size() == nbytes and s_t.is_contiguous() and d_t.is_contiguous()
            dst[i], src[i], nby[i] = d_t.data_ptr(), s_t.data_ptr(), nbytes
        _check(lib().lmi_copy_out_many(self._h, n, dst, src, nby))

    def pipeline_submit(self, s_in, s_nav, s_run, ev_in, ev_nav, ev_out, qn_h, qs_h, qn_d, qs_d, nb: int, k: int, d_out, i_out, bo_d, bo_h,
                        overlap_nav: bool) -> None:
        """One batch of a host-in -> host-out pipeline as ONE C call (lmi_pipeline_submit): raw stream / event handles, torch tensors."""
        _check(lib().lmi_pipeline_submit(self._h, s_in, s_nav, s_run, ev_in, ev_nav, ev_out, _ptr(qn_h), _ptr(qs_h), _ptr(qn_d), _ptr(qs_d),
                                         int(qn_d.shape[0]), int(nb), int(k), _ptr(d_out), _ptr(i_out), _ptr(bo_d), _ptr(bo_h), 1 if overlap_nav else 0))

    # ---- RCCL inside the library (the sharded exchange without torch.distributed) ----------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        _check(lib().lmi_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        """ncclComm_t (opaque pointer) over `world` ranks; collective: every rank calls it with rank 0's id."""
        comm = _vp()
        _check(lib().lmi_comm_init(self._h, int(rank), int(world), ctypes.c_char_p(unique_id), ctypes.byref(comm)))
        return comm

    @staticmethod
    def comm_destroy(comm) -> None:
        _check(lib().lmi_comm_destroy(comm))

    def allgather_merge(self, comm, rank: int, world: int, d_t, i_t, k_t, out_d_t, out_i_t) -> None:
        """This rank's [nq, kout] device tensors (dists, ids, keys) -> merged (dists, ids) on every rank."""
        nq, kout = int(d_t.shape[0]), int(d_t.shape[1])
        _check(lib().lmi_allgather_merge(self._h, comm, int(rank), int(world), _ptr(d_t), _ptr(i_t), _ptr(k_t), nq, kout,
                                         _ptr(out_d_t), _ptr(out_i_t)))

    def read_bucket(self, b: int, rows_out=None, ids_out=None, dtype=np.float32):
        """(rows [n_b,d], ids u32[n_b]) of bucket b, in bucket order; `rows_out` / `ids_out`: C-contiguous
        numpy arrays of exactly that shape to fill instead of fresh ones (e.g. slices of one host slab).
        `dtype`: np.float32 (default) or np.float16 (`lmi_bucket_read_f16`): the rows as halves -- the stored halves of a
        `storage="f16"` index; an f32 index narrows on the device and raises `LmiError` when a value of the bucket is not
        exactly representable in binary16 (nothing approximate is returned)."""
        dtype = np.dtype(dtype)
        assert dtype in (np.dtype(np.float32), np.dtype(np.float16)), "read_bucket: dtype is np.float32 or np.float16"
        n = int(self.bucket_sizes()[b])
        rows = np.empty((n, self.d), dtype=dtype) if rows_out is None else rows_out
        ids = np.empty(n, dtype=np.uint32) if ids_out is None else ids_out
        assert rows.shape == (n, self.d) and rows.dtype == dtype and rows.flags.c_contiguous
        assert ids.shape == (n,) and ids.dtype == np.uint32 and ids.flags.c_contiguous
        fn = lib().lmi_bucket_read_f16 if dtype == np.float16 else lib().lmi_bucket_read
        _check(fn(self._h, int(b), _ptr(rows), _ptr(ids)))
        return rows, ids

    def fetch(self, ids, dtype=np.float32, rows_out=None, where: bool = False):
        """The stored vectors of the objects with these ids (`lmi_rows_fetch`; np.float16: `lmi_rows_fetch_f16`): rows [n, d], exactly
        what `read_bucket` returns for them, in the order asked for.  `ids`: any integer array-like with values in [0, 2^32), in any
        order, repeats allowed (ValueError otherwise, before the library is called).  An id no stored object carries gets a row of
        zeros; `where=True` returns (rows, bucket int32 [n], row int32 [n]) -- the object's bucket and its row in `read_bucket`'s
        order, (-1, -1) for an absent id, and for an id several objects carry the first one by (bucket, row).  `rows_out`: a
        C-contiguous array [n, d] of `dtype` to fill.  np.float16 on an f32 index narrows on the device and raises `LmiError` when
        a fetched value is not exactly representable in binary16 (`rows_out` is then untouched)."""
        ids_a, dtype = fetch_args("fetch", self, ids, dtype)
        n = int(ids_a.shape[0])
        rows = np.empty((n, self.d), dtype=dtype) if rows_out is None else rows_out
        if not (isinstance(rows, np.ndarray) and rows.shape == (n, self.d) and rows.dtype == dtype and rows.flags.c_contiguous):
            raise ValueError(f"fetch: rows_out must be a C-contiguous {dtype} array of shape {(n, self.d)}")
        bucket = np.empty(n, np.int32) if where else None
        row = np.empty(n, np.int32) if where else None
        fn = lib().lmi_rows_fetch_f16 if dtype == np.float16 else lib().lmi_rows_fetch
        _check(fn(self._h, _ptr(ids_a), n, _ptr(rows), _ptr(bucket), _ptr(row), 0))
        return (rows, bucket, row) if where else rows

    def locate(self, ids):
        """(bucket int32 [n], row int32 [n]) of the objects with these ids, as `fetch(.., where=True)` reports them, without reading
        a vector (`lmi_rows_fetch` with no rows)."""
        ids_a, _ = fetch_args("locate", self, ids, np.float32)
        n = int(ids_a.shape[0])
        bucket, row = np.empty(n, np.int32), np.empty(n, np.int32)
        _check(lib().lmi_rows_fetch(self._h, _ptr(ids_a), n, None, _ptr(bucket), _ptr(row), 0))
        return bucket, row

    def fetch_device(self, ids_t, rows_t=None, bucket_t=None, row_t=None) -> None:
        """`fetch` on contiguous device tensors: ids_t [n] holding uint32 bit patterns (torch.uint32 or torch.int32) -> rows_t [n, d]
        (torch.float32: `lmi_rows_fetch`; torch.float16: `lmi_rows_fetch_f16`), bucket_t / row_t int32 [n]; each output may be
        None, not all.  The vectors never leave the device (the ids are copied to the host to be sorted: 4n bytes)."""
        n = fetch_device_args(self, ids_t, rows_t, bucket_t, row_t)
        if n == 0:   # (an empty tensor has no address: nothing to ask the library for)
            return
        fn = lib().lmi_rows_fetch_f16 if rows_t is not None and _is_f16(rows_t) else lib().lmi_rows_fetch
        _check(fn(self._h, _ptr(ids_t), n, _ptr(rows_t), _ptr(bucket_t), _ptr(row_t), 1))

    def workspace_bytes(self, nq: int, nb: int) -> int:
        """Device bytes the per-call workspaces of a search of nq queries x nb buckets need (lmi_workspace_bytes)."""
        out = ctypes.c_int64(0)
        _check(lib().lmi_workspace_bytes(self._h, int(nq), int(nb), ctypes.byref(out)))
        return out.value

    def timings(self) -> np.ndarray:
        ms = np.zeros(T_COUNT, dtype=np.float32)
        _check(lib().lmi_timings(self._h, _ptr(ms)))
        return ms

    def set_timing(self, level: int) -> None:
        """2 (default): every phase from device-side clock stamps (no bubbles); 3: every phase from hipEvents (each a ~5 us bubble);
        1: hipEvents around the whole call only; 0: nothing."""
        _check(lib().lmi_set_timing(self._h, int(level)))

    def timings_reset(self) -> None:
        _check(lib().lmi_timings_reset(self._h))

    def timings_mean(self):
        """(mean ms per slot, calls averaged) since timings_reset -- one stream sync for the whole loop."""
        ms = np.zeros(T_COUNT, dtype=np.float32)
        n = ctypes.c_int(0)
        _check(lib().lmi_timings_mean(self._h, _ptr(ms), ctypes.byref(n)))
        return ms, n.value

    def scan_stats(self):
        fl = ctypes.c_double(0)
        pairs = ctypes.c_int64(0)
        items = ctypes.c_int64(0)
        _check(lib().lmi_scan_stats(self._h, ctypes.byref(fl), ctypes.byref(pairs), ctypes.byref(items)))
        return fl.value, pairs.value, items.value


def knn_ip(xq, xb, k: int = 10, device: int = 0):
    """faiss.knn(xq, xb, k, metric=faiss.METRIC_INNER_PRODUCT) on the GPU (LearnedIndex.py:360-365)."""
    xq = _np(xq, np.float32)
    xb = _np(xb, np.float32)
    assert xq.ndim == 2 and xb.ndim == 2 and xq.shape[1] == xb.shape[1]
    D = np.empty((xq.shape[0], k), dtype=np.float32)
    I = np.empty((xq.shape[0], k), dtype=np.int64)
    _check(lib().lmi_knn_ip(int(device), _ptr(xq), xq.shape[0], _ptr(xb), xb.shape[0], xq.shape[1], int(k),
                            _ptr(D), _ptr(I)))
    return D, I


def _knn_inputs(who: str, xq, xb):
    """(is numpy, is float16) of the two arrays of `knn` / `range_knn`: both float32 or both float16 (then the `_f16` entry point takes
    them as they are: nothing is widened on the host), both numpy or both torch.  Anything else -- one float16 array beside a float32
    one included -- is a ValueError."""
    f16 = _is_f16(xq) and _is_f16(xb)
    dtype = "float16" if f16 else "float32"   # a mixed pair: the float16 array is told that it must be float32
    is_np = _array_arg(who, "xq", xq, dtype, "2d"), _array_arg(who, "xb", xb, dtype, "2d")
    if is_np[0] != is_np[1]:
        raise ValueError(f"{who}: xq and xb must both be numpy arrays or both be torch tensors on the device")
    return is_np[0], f16


def knn(xq, xb, k: int = 10, metric: str = "ip", device: int = 0):
    """Exact brute-force k-NN on the device for k up to KNN_MAX_K (`lmi_knn`): (D f32[nq,k], I i64[nq,k]).  metric "ip": the k
    largest inner products, descending; "l2": the k smallest squared Euclidean distances, ascending; ties go to the lower row; fewer
    than k rows pad with I = -1 and D = -FLT_MAX (l2: FLT_MAX).  The same input gives the same result bit for bit
    (include/lmi_hip.h states the arithmetic; oracle.knn_ip / oracle.knn_l2 restate it).  `xq`, `xb`: float32 numpy arrays -- `xb`
    is uploaded in pieces and never resident as a whole -- or contiguous float32 torch tensors on the device, both of one kind; D and
    I then come back as tensors on that device and the inputs are only read.  Both float16 (numpy, or contiguous torch.float16 tensors
    on one device): `lmi_knn_f16` takes the halves as they are -- half the upload, no widened copy anywhere -- and returns bit for bit
    what the call on the arrays widened to float32 returns.  One float16 array beside a float32 one is refused.  Argument errors raise
    ValueError before the library is loaded."""
    is_np, f16 = _knn_inputs("knn", xq, xb)
    if metric not in KNN_METRICS:
        raise ValueError(f"knn: metric {metric!r} unknown ('ip' or 'l2')")
    nq, d, nb, k = int(xq.shape[0]), int(xq.shape[1]), int(xb.shape[0]), int(k)
    if int(xb.shape[1]) != d:
        raise ValueError(f"knn: xq has {d} columns, xb {int(xb.shape[1])}")
    if d < 1 or d > 4096:
        raise ValueError(f"knn: d {d} outside [1, 4096]")
    if k < 1 or k > KNN_MAX_K:
        raise ValueError(f"knn: k {k} outside [1, {KNN_MAX_K}]")
    if is_np:
        xq, xb = np.ascontiguousarray(xq), np.ascontiguousarray(xb)
        D = np.empty((nq, k), dtype=np.float32)
        I = np.empty((nq, k), dtype=np.int64)
        call = lib().lmi_knn_f16 if f16 else lib().lmi_knn
        _check(call(int(device), _ptr(xq), nq, _ptr(xb), nb, d, k, KNN_METRICS[metric], _ptr(D), _ptr(I), 0))
        return D, I
    if not (xq.is_cuda and xb.is_cuda and xq.is_contiguous() and xb.is_contiguous()) or xq.device != xb.device:
        raise ValueError("knn: torch xq and xb must be contiguous tensors on one device")
    import torch

    D = torch.empty((nq, k), dtype=torch.float32, device=xq.device)
    I = torch.empty((nq, k), dtype=torch.int64, device=xq.device)
    call = lib().lmi_knn_f16 if f16 else lib().lmi_knn
    _check(call(_sync_device(xq), _ptr(xq), nq, _ptr(xb), nb, d, k, KNN_METRICS[metric], _ptr(D), _ptr(I), 1))
    return D, I


def knn_set_geometry(piece_rows: int = 0, splits: int = 0, query_rows: int = 0) -> None:
    """Tuning / test hook (`lmi_knn_set_geometry`): rows of `xb` per piece, splits per piece, queries per group of the `knn` calls
    of this thread; 0 = chosen by the library.  Never changes a result."""
    _check(lib().lmi_knn_set_geometry(int(piece_rows), int(splits), int(query_rows)))


def knn_last_plan() -> dict:
    """What the last `knn` on this thread did, float32 or float16 (`lmi_debug_knn_plan`): `KNN_PLAN_FIELDS` -> int."""
    w = (ctypes.c_int64 * len(KNN_PLAN_FIELDS))()
    _check(lib().lmi_debug_knn_plan(w, len(KNN_PLAN_FIELDS)))
    return dict(zip(KNN_PLAN_FIELDS, (int(v) for v in w)))


class Filter:
    """A filter set over one built `Index` (`lmi_filter_create`): `lists[j]` holds filter j's ids, `modes[j]` is "keep" / FILTER_KEEP
    (a stored row is allowed iff its id is listed; the default) or "drop" / FILTER_DROP (iff it is not).  Duplicates and ids the
    index does not hold are ignored; an empty keep list allows nothing, an empty drop list everything.  Passed as `filter=` to
    `Index.scan_union`, `search_union`, `search_tree_union` and their `_device` forms, on the index it was made on or a clone
    view of it; after `insert` / `delete`, and on a `subset`, the library refuses it as stale and it has to be made again.
    Argument errors raise ValueError before the library loads."""

    MODES = {"keep": FILTER_KEEP, "drop": FILTER_DROP, FILTER_KEEP: FILTER_KEEP, FILTER_DROP: FILTER_DROP}

    def __init__(self, index: "Index", lists, modes=None):
        self._f = None   # (closed until the library has made it)
        ids, offsets, modes_a = self.pack(lists, modes)
        self.nf = int(modes_a.shape[0])
        f = _vp()
        _check(lib().lmi_filter_create(index._h, _ptr(ids), _ptr(offsets), self.nf, _ptr(modes_a), ctypes.byref(f)))
        self._f = f
        self.L = int(index.L)
        self._sizes = index.bucket_sizes()

    @classmethod
    def pack(cls, lists, modes=None):
        """(ids u32[total], offsets i64[nf + 1], modes i32[nf]): the arguments of `lmi_filter_create`."""
        if isinstance(lists, np.ndarray) and lists.ndim == 1:
            raise ValueError("Filter: lists must be a sequence of id lists (one per filter), not one flat array")
        lists = [np.asarray(a).reshape(-1) for a in lists]
        nf = len(lists)
        if nf < 1 or nf > FILTER_MAX:
            raise ValueError(f"Filter: {nf} filters outside [1, {FILTER_MAX}]")
        modes = ["keep"] * nf if modes is None else list(modes)
        if len(modes) != nf:
            raise ValueError(f"Filter: {len(modes)} modes for {nf} lists")
        for m in modes:
            if isinstance(m, (bool, float)) or m not in cls.MODES:
                raise ValueError(f"Filter: mode {m!r} is neither 'keep' / FILTER_KEEP nor 'drop' / FILTER_DROP")
        for j, a in enumerate(lists):
            if a.size and a.dtype.kind not in "iu":   # (an empty list is float64 and has nothing to truncate)
                raise ValueError(f"Filter: the ids of filter {j} must be integers, not {a.dtype}")
            if a.size and (a.min() < 0 or a.max() >= 2 ** 32):
                raise ValueError(f"Filter: the ids of filter {j} must fit uint32")
        offsets = np.zeros(nf + 1, dtype=np.int64)
        np.cumsum([a.size for a in lists], out=offsets[1:])
        if offsets[-1] >= 2 ** 31:
            raise ValueError("Filter: 2^31 ids or more in all")
        ids = _np(np.concatenate(lists), np.uint32) if offsets[-1] else np.zeros(0, dtype=np.uint32)
        return ids, offsets, np.asarray([cls.MODES[m] for m in modes], dtype=np.int32)

    def counts(self) -> np.ndarray:
        """i64[nf, L]: the allowed rows per (filter, bucket) (`lmi_filter_counts`)."""
        out = np.zeros((self.nf, self.L), dtype=np.int64)
        _check(lib().lmi_filter_counts(self._f, _ptr(out)))
        return out

    def bucket_mask(self, j: int, bucket: int) -> np.ndarray:
        """u8[n_b]: 1 where filter j allows the row, in `read_bucket`'s order (`lmi_filter_bucket_mask`)."""
        if not 0 <= int(j) < self.nf or not 0 <= int(bucket) < self.L:
            raise ValueError(f"bucket_mask: (filter {j}, bucket {bucket}) outside ({self.nf}, {self.L})")
        out = np.zeros(int(self._sizes[bucket]), dtype=np.uint8)
        _check(lib().lmi_filter_bucket_mask(self._f, int(j), int(bucket), _ptr(out)))
        return out

    def close(self) -> None:
        if getattr(self, "_f", None) is not None:
            f, self._f = self._f, None
            lib().lmi_filter_destroy(f)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Cover:
    """The covering balls of a built `Index` (`lmi_cover_create`): per bucket a centre, a covering radius and the live row count,
    computed on the device from the stored rows.  Passed as `cover=` to `Index.cover_order`, `Index.search_range_exact` and their
    `_device` forms, on the index it was made on or a clone view of it; after `insert` / `delete`, and on a `subset`, `regroup` or
    `concat` result, the library refuses it as stale and it has to be made again.  It does not refer to the `Index` and may outlive
    it.  A context manager: leaving the block closes it."""

    def __init__(self, index: "Index"):
        self._c = None   # (closed until the library has made it)
        if not isinstance(index, Index) or getattr(index, "_h", None) is None or not index._h:
            raise ValueError("Cover: index must be an open Index")
        c = _vp()
        _check(lib().lmi_cover_create(index._h, ctypes.byref(c)))
        self._c = c
        self.L, self.d = int(index.L), int(index.d)

    def read(self):
        """(centres f32[L, d], radius f32[L], counts i64[L]) on the host (`lmi_cover_read`)."""
        if getattr(self, "_c", None) is None:
            raise ValueError("Cover: the cover is closed")
        centres = np.zeros((self.L, self.d), dtype=np.float32)
        radius = np.zeros(self.L, dtype=np.float32)
        counts = np.zeros(self.L, dtype=np.int64)
        _check(lib().lmi_cover_read(self._c, _ptr(centres), _ptr(radius), _ptr(counts)))
        return centres, radius, counts

    def close(self) -> None:
        if getattr(self, "_c", None) is not None:
            c, self._c = self._c, None
            lib().lmi_cover_destroy(c)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cover_set_geometry(query_rows: int = 0) -> None:
    """Test hook (`lmi_cover_set_geometry`): queries per group of the pruning pass on this thread, an integer in [0, 2^20]; 0 = the
    default.  Never changes a result."""
    if isinstance(query_rows, bool) or not isinstance(query_rows, (int, np.integer)) or not 0 <= query_rows <= COVER_MAX_QUERY_ROWS:
        raise ValueError(f"cover_set_geometry: query_rows {query_rows!r} must be an integer in [0, {COVER_MAX_QUERY_ROWS}] (0: the default)")
    _check(lib().lmi_cover_set_geometry(int(query_rows)))


def cover_last_plan() -> dict:
    """What the last `cover_order` / `search_range_exact` on this thread did (`lmi_debug_cover_plan`): `COVER_PLAN_FIELDS` -> int."""
    w = (ctypes.c_int64 * len(COVER_PLAN_FIELDS))()
    _check(lib().lmi_debug_cover_plan(w, len(COVER_PLAN_FIELDS)))
    return dict(zip(COVER_PLAN_FIELDS, (int(v) for v in w)))


def filter_last_plan() -> dict:
    """What the last filtered union call on this thread did (`lmi_debug_filter_plan`): `FILTER_PLAN_FIELDS` -> int."""
    w = (ctypes.c_int64 * len(FILTER_PLAN_FIELDS))()
    _check(lib().lmi_debug_filter_plan(w, len(FILTER_PLAN_FIELDS)))
    return dict(zip(FILTER_PLAN_FIELDS, (int(v) for v in w)))


class RangeResult:
    """The results of one range call (`lmi_range_result`): `lims` i64[nq + 1] and `total` = lims[nq] on the host, the distances and ids
    on the device until they are read.  It does not refer to the `Index` it came from and may outlive it.  A context manager: leaving
    the block closes it."""

    def __init__(self, handle, nq: int):
        self._r = handle
        self.nq = int(nq)
        self.lims = np.zeros(self.nq + 1, dtype=np.int64)
        _check(lib().lmi_range_result_lims(self._r, _ptr(self.lims)))
        self.total = int(self.lims[-1])

    def _open(self):
        if getattr(self, "_r", None) is None:
            raise ValueError("RangeResult: the result is closed")
        return self._r

    def read(self):
        """(dists f32[total], ids u32[total]) on the host."""
        d = np.empty(self.total, dtype=np.float32)
        i = np.empty(self.total, dtype=np.uint32)
        _check(lib().lmi_range_result_read(self._open(), _ptr(d), _ptr(i), 0))
        return d, i

    def pair_counts(self) -> np.ndarray:
        """i32[nq, nb]: the results of every (query, rank t of the bucket in the query's order) (`lmi_range_result_pair_counts`); row q
        sums to lims[q + 1] - lims[q].  What a rank hands on beside its arrays for `Index.join_range_parts`."""
        nb = ctypes.c_int32(0)
        _check(lib().lmi_range_result_pair_counts(self._open(), ctypes.byref(nb), None))
        c = np.zeros((self.nq, int(nb.value)), dtype=np.int32)
        if self.nq > 0:
            _check(lib().lmi_range_result_pair_counts(self._r, None, _ptr(c)))
        return c

    def sort(self, index) -> "RangeResult":
        """Every query's results stably sorted by distance, on the device and in place (`lmi_range_result_sort`): what
        `np.argsort(dists[a:b], kind="stable")` makes of each segment, -0 == +0 and NaNs last.  `index` is any open `Index` on the
        result's device (it provides the stream; it needs no built index).  `lims` and `pair_counts()` stay as they are.  Returns self."""
        if not isinstance(index, Index) or getattr(index, "_h", None) is None:
            raise ValueError("RangeResult.sort: index must be an open Index")
        r = self._open()
        _check(lib().lmi_range_result_sort(index._h, r))
        return self

    @property
    def sorted(self) -> bool:
        """True once `sort` has run on this result (`lmi_range_result_sorted`): its segments are no longer in (rank, row) order."""
        r, flag = self._open(), ctypes.c_int(0)
        _check(lib().lmi_range_result_sorted(r, ctypes.byref(flag)))
        return bool(flag.value)

    def read_into(self, d_t, i_t) -> None:
        """Device tensors of at least `total` 4-byte elements each (float32; int32 or uint32-sized) <- the distances and the ids."""
        for name, t in (("d_t", d_t), ("i_t", i_t)):
            if not (hasattr(t, "is_cuda") and t.is_cuda and t.is_contiguous() and t.element_size() == 4 and t.numel() >= self.total):
                raise ValueError(f"RangeResult.read_into: {name} must be a contiguous device tensor of >= {self.total} 4-byte elements")
        _check(lib().lmi_range_result_read(self._open(), _ptr(d_t), _ptr(i_t), 1))

    def close(self) -> None:
        if getattr(self, "_r", None) is not None:
            r, self._r = self._r, None
            lib().lmi_range_result_destroy(r)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def range_last_plan() -> dict:
    """What the last range call on this thread did (`lmi_debug_range_plan`): `RANGE_PLAN_FIELDS` -> int."""
    w = (ctypes.c_int64 * len(RANGE_PLAN_FIELDS))()
    _check(lib().lmi_debug_range_plan(w, len(RANGE_PLAN_FIELDS)))
    return dict(zip(RANGE_PLAN_FIELDS, (int(v) for v in w)))


def range_knn(xq, xb, radius, metric: str = "ip", max_total: int = 0, device: int = 0) -> "RangeResult":
    """Exact brute-force range query on the device (`lmi_knn_range`): the `RangeResult` of, per query, every row of `xb` within
    distance `radius` (a number, or one per query) -- metric "ip": 1 - the inner product, "l2": the squared Euclidean distance, as
    `knn` computes them -- in ascending row order; `ids` are row numbers in `xb`.  A NaN or -inf radius admits nothing.  `xq`, `xb`:
    float32 numpy arrays or contiguous float32 torch tensors on the device, both of one kind, as `knn` takes them -- or both float16,
    which `lmi_knn_range_f16` takes as they are, with the result of the call on the widened arrays bit for bit; `radius` stays on the
    host.  `max_total` > 0: the call fails (LmiError) once more results than that have been counted.  The same input gives the
    same result bit for bit.  Argument errors raise ValueError before the library is loaded."""
    is_np, f16 = _knn_inputs("range_knn", xq, xb)
    if metric not in KNN_METRICS:
        raise ValueError(f"range_knn: metric {metric!r} unknown ('ip' or 'l2')")
    nq, d, nb = int(xq.shape[0]), int(xq.shape[1]), int(xb.shape[0])
    if int(xb.shape[1]) != d:
        raise ValueError(f"range_knn: xq has {d} columns, xb {int(xb.shape[1])}")
    if d < 1 or d > 4096:
        raise ValueError(f"range_knn: d {d} outside [1, 4096]")
    if radius is None:
        raise ValueError("range_knn: radius is None")
    r = np.asarray(radius.cpu().numpy() if hasattr(radius, "cpu") else radius)
    if r.dtype.kind not in "fiu" or r.ndim > 1 or (r.ndim == 1 and r.shape[0] != nq):
        raise ValueError(f"range_knn: radius must be a number or one number per query ([{nq}]), not {r.dtype}{tuple(r.shape)}")
    if isinstance(max_total, bool) or not isinstance(max_total, (int, np.integer)) or max_total < 0:
        raise ValueError(f"range_knn: max_total {max_total!r} must be an integer >= 0 (0: no limit)")
    r = np.ascontiguousarray(np.broadcast_to(r.astype(np.float32), (nq,)))
    if is_np:
        xq, xb, on_device = np.ascontiguousarray(xq), np.ascontiguousarray(xb), 0
    else:
        if not (xq.is_cuda and xb.is_cuda and xq.is_contiguous() and xb.is_contiguous()) or xq.device != xb.device:
            raise ValueError("range_knn: torch xq and xb must be contiguous tensors on one device")
        device, on_device = _sync_device(xq), 1
    res = _vp()
    call = lib().lmi_knn_range_f16 if f16 else lib().lmi_knn_range
    _check(call(int(device), _ptr(xq), nq, _ptr(xb), nb, d, KNN_METRICS[metric], _ptr(r), int(max_total), ctypes.byref(res), on_device))
    return RangeResult(res, nq)


def knn_range_last_plan() -> dict:
    """What the last `range_knn` on this thread did (`lmi_debug_knn_range_plan`): `KNN_RANGE_PLAN_FIELDS` -> int."""
    w = (ctypes.c_int64 * len(KNN_RANGE_PLAN_FIELDS))()
    _check(lib().lmi_debug_knn_range_plan(w, len(KNN_RANGE_PLAN_FIELDS)))
    return dict(zip(KNN_RANGE_PLAN_FIELDS, (int(v) for v in w)))


def range_join_last_plan() -> dict:
    """What the last join of range parts on this thread did (`lmi_debug_range_join_plan`): `RANGE_JOIN_FIELDS` -> int."""
    w = (ctypes.c_int64 * len(RANGE_JOIN_FIELDS))()
    _check(lib().lmi_debug_range_join_plan(w, len(RANGE_JOIN_FIELDS)))
    return dict(zip(RANGE_JOIN_FIELDS, (int(v) for v in w)))


def range_sort_set_geometry(tile_rows: int = 0, scratch_bytes: int = 0) -> None:
    """Test hook (`lmi_range_sort_set_geometry`): the tile length (a power of two in [64, 8192]) and the groups' scratch budget in bytes
    (at most 2^40) of `RangeResult.sort` on this thread; 0 = the default.  Never changes a result."""
    for name, v in (("tile_rows", tile_rows), ("scratch_bytes", scratch_bytes)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
            raise ValueError(f"range_sort_set_geometry: {name} {v!r} must be an integer >= 0 (0: the default)")
    if tile_rows and (tile_rows & (tile_rows - 1) or not RANGE_SORT_MIN_TILE_ROWS <= tile_rows <= RANGE_SORT_MAX_TILE_ROWS):
        raise ValueError(f"range_sort_set_geometry: tile_rows {tile_rows} is not a power of two in "
                         f"[{RANGE_SORT_MIN_TILE_ROWS}, {RANGE_SORT_MAX_TILE_ROWS}]")
    if scratch_bytes > 1 << 40:
        raise ValueError(f"range_sort_set_geometry: scratch_bytes {scratch_bytes} above 2^40")
    _check(lib().lmi_range_sort_set_geometry(int(tile_rows), int(scratch_bytes)))


def range_sort_last_plan() -> dict:
    """What the last `RangeResult.sort` on this thread did (`lmi_debug_range_sort_plan`): `RANGE_SORT_PLAN_FIELDS` (lower case) -> int."""
    w = (ctypes.c_int64 * len(RANGE_SORT_PLAN_FIELDS))()
    _check(lib().lmi_debug_range_sort_plan(w, len(RANGE_SORT_PLAN_FIELDS)))
    return dict(zip((n.lower() for n in RANGE_SORT_PLAN_FIELDS), (int(v) for v in w)))


def regroup_args(ids, labels, L_new, bucket_map, L):
    """`Index.regroup`'s arguments as the library takes them -- (ids uint32 [n], labels int64 [n], bucket_map int32 [L] or None, L_new)
    -- or ValueError; needs no library.  What it cannot see (which objects the index holds) the library checks."""
    if isinstance(L_new, bool) or not isinstance(L_new, (int, np.integer)) or not 1 <= L_new < REGROUP_MAX_LABELS:
        raise ValueError(f"regroup: L_new {L_new!r} must be an integer in [1, {REGROUP_MAX_LABELS})")
    a, lab = np.asarray(ids).reshape(-1), np.asarray(labels).reshape(-1)
    if a.shape[0] != lab.shape[0]:
        raise ValueError(f"regroup: {a.shape[0]} ids but {lab.shape[0]} labels")
    for name, x in (("ids", a), ("labels", lab)):
        if x.size and x.dtype.kind not in "iu":   # (an empty list is float64 and has nothing to truncate)
            raise ValueError(f"regroup: {name} must be integers, not {x.dtype}")
    if a.size and (a.min() < 0 or a.max() >= 2 ** 32):
        raise ValueError("regroup: ids must fit uint32")
    if lab.size and (lab.min() < 0 or lab.max() >= L_new):
        bad = int(np.flatnonzero((lab < 0) | (lab >= L_new))[0])
        raise ValueError(f"regroup: labels[{bad}] = {int(lab[bad])} outside [0, {L_new})")
    ids_a = _np(a, np.uint32)
    if ids_a.size > 1:
        srt = np.sort(ids_a)
        dup = np.flatnonzero(srt[1:] == srt[:-1])
        if dup.size:
            raise ValueError(f"regroup: id {int(srt[dup[0]])} is listed twice")
    map_a = None
    if bucket_map is None:
        if L_new < L:
            raise ValueError(f"regroup: without a bucket_map every unnamed object keeps its bucket, which needs L_new >= L ({L_new} < {L})")
    else:
        m = np.asarray(bucket_map).reshape(-1)
        if m.shape[0] != L or (m.size and m.dtype.kind not in "iu"):
            raise ValueError(f"regroup: bucket_map must be {L} integers (one per bucket of this index)")
        if m.size and (m.min() < -1 or m.max() >= L_new):
            bad = int(np.flatnonzero((m < -1) | (m >= L_new))[0])
            raise ValueError(f"regroup: bucket_map[{bad}] = {int(m[bad])} outside [-1, {L_new})")
        map_a = _np(m, np.int32)
    return ids_a, _np(lab, np.int64), map_a, int(L_new)


def regroup_set_geometry(tile_rows: int = 0) -> None:
    """Test hook (`lmi_regroup_set_geometry`): the tile length (a power of two in [64, 8192]; 0 = the default) of the sort inside
    `Index.regroup` on this thread.  Never changes a result."""
    if isinstance(tile_rows, bool) or not isinstance(tile_rows, (int, np.integer)) or tile_rows < 0:
        raise ValueError(f"regroup_set_geometry: tile_rows {tile_rows!r} must be an integer >= 0 (0: the default)")
    if tile_rows and (tile_rows & (tile_rows - 1) or not REGROUP_MIN_TILE_ROWS <= tile_rows <= REGROUP_MAX_TILE_ROWS):
        raise ValueError(f"regroup_set_geometry: tile_rows {tile_rows} is not a power of two in "
                         f"[{REGROUP_MIN_TILE_ROWS}, {REGROUP_MAX_TILE_ROWS}]")
    _check(lib().lmi_regroup_set_geometry(int(tile_rows)))


def regroup_last_plan() -> dict:
    """What the last `Index.regroup` on this thread did (`lmi_debug_regroup_plan`): `REGROUP_PLAN_FIELDS` (lower case) -> int."""
    w = (ctypes.c_int64 * len(REGROUP_PLAN_FIELDS))()
    _check(lib().lmi_debug_regroup_plan(w, len(REGROUP_PLAN_FIELDS)))
    return dict(zip((n.lower() for n in REGROUP_PLAN_FIELDS), (int(v) for v in w)))


def concat_args(first, others):
    """`Index.concat`'s parts as the library takes them -- the list [first, *others] of open `Index` objects -- or ValueError,
    before the library is touched.  What the parts must agree in (d, L, metric, storage, prefilter, `owned` mask, device) is the
    library's to check: it knows all of it, this module only part."""
    parts = [first] + list(others)
    if len(parts) > CONCAT_MAX_PARTS:
        raise ValueError(f"concat: {len(parts)} parts (this index and {len(others)} others), at most {CONCAT_MAX_PARTS}")
    for t, p in enumerate(parts):
        if not isinstance(p, Index):
            raise ValueError(f"concat: part {t} must be an Index, not {type(p).__name__}")
        if getattr(p, "_h", None) is None or not p._h:
            raise ValueError(f"concat: part {t} is closed")
    return parts


def concat_last_plan() -> dict:
    """What the last `Index.concat` on this thread did (`lmi_debug_concat_plan`): `CONCAT_PLAN_FIELDS` (lower case) -> int."""
    w = (ctypes.c_int64 * len(CONCAT_PLAN_FIELDS))()
    _check(lib().lmi_debug_concat_plan(w, len(CONCAT_PLAN_FIELDS)))
    return dict(zip((n.lower() for n in CONCAT_PLAN_FIELDS), (int(v) for v in w)))


def fetch_args(who: str, index, ids, dtype):
    """(ids uint32 [n], dtype) of `Index.fetch` / `Index.locate`, or ValueError; needs no library."""
    if getattr(index, "_h", None) is None or not index._h:
        raise ValueError(f"{who}: the index is closed")
    try:
        dtype = np.dtype(dtype)
    except TypeError:
        raise ValueError(f"{who}: dtype must be np.float32 or np.float16, not {dtype!r}") from None
    if dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise ValueError(f"{who}: dtype must be np.float32 or np.float16, not {dtype}")
    a = np.asarray(ids).reshape(-1)
    if a.size and a.dtype.kind not in "iu":   # (an empty list is float64 and has nothing to truncate)
        raise ValueError(f"{who}: ids must be integers, not {a.dtype}")
    if a.size and (a.min() < 0 or a.max() >= 2 ** 32):
        raise ValueError(f"{who}: ids must lie in [0, 2^32)")
    if a.size >= 2 ** 31:
        raise ValueError(f"{who}: {a.size} ids, at most 2^31 - 1")
    return _np(a, np.uint32), dtype


def fetch_device_args(index, ids_t, rows_t, bucket_t, row_t) -> int:
    """n of `Index.fetch_device`, or ValueError; needs no library."""
    who = "fetch_device"
    if getattr(index, "_h", None) is None or not index._h:
        raise ValueError(f"{who}: the index is closed")
    def dev(name, t, dtypes, shape):
        if not (hasattr(t, "data_ptr") and getattr(t, "is_cuda", False) and t.is_contiguous()):
            raise ValueError(f"{who}: {name} must be a contiguous torch tensor on the device")
        if str(t.dtype).replace("torch.", "") not in dtypes:
            raise ValueError(f"{who}: {name} must be {' or '.join(dtypes)}, not {t.dtype}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{who}: {name} must have shape {shape}, not {tuple(t.shape)}")
    if not hasattr(ids_t, "shape") or len(ids_t.shape) != 1:
        raise ValueError(f"{who}: ids_t must be one-dimensional")
    n = int(ids_t.shape[0])
    dev("ids_t", ids_t, ("uint32", "int32"), (n,))
    if rows_t is None and bucket_t is None and row_t is None:
        raise ValueError(f"{who}: rows_t, bucket_t and row_t are all None: nothing was asked for")
    if rows_t is not None:
        dev("rows_t", rows_t, ("float32", "float16"), (n, index.d))
    for name, t in (("bucket_t", bucket_t), ("row_t", row_t)):
        if t is not None:
            dev(name, t, ("int32",), (n,))
    return n


def fetch_set_geometry(piece_rows: int = 0) -> None:
    """Test hook (`lmi_fetch_set_geometry`): requests per piece of `Index.fetch` / `locate` / `fetch_device` on this thread, an integer
    in [0, 2^24]; 0 = the default (host outputs: what a 64-MiB stage holds; device outputs: 2^24).  Never changes a result."""
    if isinstance(piece_rows, bool) or not isinstance(piece_rows, (int, np.integer)) or not 0 <= piece_rows <= FETCH_MAX_PIECE_ROWS:
        raise ValueError(f"fetch_set_geometry: piece_rows {piece_rows!r} must be an integer in [0, {FETCH_MAX_PIECE_ROWS}] (0: the default)")
    _check(lib().lmi_fetch_set_geometry(int(piece_rows)))


def fetch_last_plan() -> dict:
    """What the last fetch on this thread did (`lmi_debug_fetch_plan`): `FETCH_PLAN_FIELDS` -> int."""
    w = (ctypes.c_int64 * len(FETCH_PLAN_FIELDS))()
    _check(lib().lmi_debug_fetch_plan(w, len(FETCH_PLAN_FIELDS)))
    return dict(zip(FETCH_PLAN_FIELDS, (int(v) for v in w)))


def union_set_geometry(query_rows: int = 0, slab_bytes: int = 0) -> None:
    """Tuning / test hook (`lmi_union_set_geometry`): queries per group and bytes of a wave's score slab of the union calls on this
    thread; 0 = the library's choice.  Never changes a result."""
    _check(lib().lmi_union_set_geometry(int(query_rows), int(slab_bytes)))


def union_last_plan() -> dict:
    """What the last union call on this thread did (`lmi_debug_union_plan`): `UNION_PLAN_FIELDS` -> int."""
    w = (ctypes.c_int64 * len(UNION_PLAN_FIELDS))()
    _check(lib().lmi_debug_union_plan(w, len(UNION_PLAN_FIELDS)))
    return dict(zip(UNION_PLAN_FIELDS, (int(v) for v in w)))


def kmeans(x, k: int, niter: int = 20, init=None, seed: int = 2023, device: int = 0):
    """Lloyd's k-means on the device (`lmi_kmeans`): (centroids f32[k,d], labels i32[n], counts i64[k], changed i64[niter+1]).
    The same input gives the same result bit for bit (include/lmi_hip.h states the arithmetic; tests/kmeans_ref.py restates it).
    `x`: a float32 numpy array [n,d], or a contiguous float32 torch tensor on the device -- then `centroids` and `labels` come back
    as tensors on that device and `x` is only read.  A float16 `x` (numpy, or a contiguous torch.float16 tensor on the device) goes to
    `lmi_kmeans_f16` as it is -- half the upload, resident as halves, no widened copy anywhere -- and the result is bit for bit that of
    the call on `x` widened to float32; the centroids are float32 either way.  `init`: f32 [k,d] initial centroids; None: the rows
    `np.random.RandomState(seed).choice(n, k, replace=False)` of `x`, widened to float32.  `changed[it]`: rows whose label moved in
    pass `it` (zeros behind a fixed point).  Argument errors raise ValueError before the library is loaded."""
    f16 = _is_f16(x)
    is_np = _array_arg("kmeans", "x", x, "float16" if f16 else "float32", "nd")
    n, d = int(x.shape[0]), int(x.shape[1])
    k, niter = int(k), int(niter)
    if k < 1 or k > n:
        raise ValueError(f"kmeans: k {k} outside [1, n = {n}]")
    if niter < 0:
        raise ValueError(f"kmeans: niter {niter} < 0")
    if init is not None:
        init = np.asarray(init.detach().cpu().numpy() if hasattr(init, "detach") else init)
        if init.dtype != np.float32 or init.shape != (k, d):
            raise ValueError(f"kmeans: init must be float32 [{k},{d}], not {init.dtype} {tuple(init.shape)}")
    counts = np.zeros(k, dtype=np.int64)
    changed = np.zeros(niter + 1, dtype=np.int64)
    if is_np:
        x = np.ascontiguousarray(x)
        cent = np.array(x[np.random.RandomState(seed).choice(n, k, replace=False)] if init is None else init, dtype=np.float32, order="C")
        labels = np.empty(n, dtype=np.int32)
        call = lib().lmi_kmeans_f16 if f16 else lib().lmi_kmeans
        _check(call(int(device), _ptr(x), n, d, k, niter, _ptr(cent), _ptr(labels), _ptr(counts), _ptr(changed), 0))
        return cent, labels, counts, changed
    if not x.is_cuda or not x.is_contiguous():
        raise ValueError("kmeans: a torch x must be a contiguous tensor on the device")
    import torch

    if init is None:
        rows = torch.from_numpy(np.random.RandomState(seed).choice(n, k, replace=False)).to(x.device)
        cent = x[rows].to(torch.float32)   # a copy either way: indexing gathers
    else:
        cent = torch.from_numpy(np.array(init, dtype=np.float32, order="C")).to(x.device)
    labels = torch.empty(n, dtype=torch.int32, device=x.device)
    call = lib().lmi_kmeans_f16 if f16 else lib().lmi_kmeans
    _check(call(_sync_device(x), _ptr(x), n, d, k, niter, _ptr(cent), _ptr(labels), _ptr(counts), _ptr(changed), 1))
    return cent, labels, counts, changed


def train(x, labels, layers, batch_rows, lr: float, state=None, device: int = 0):
    """Adam steps on a Linear/ReLU stack on the device (`lmi_train`): returns `(layers, state, losses)`.
    `x` f32 [n,d] and `labels` int32 [n]: numpy arrays, or contiguous torch tensors on the device (both; they are only read).
    `layers` = [(W [out,in], b [out]), ...] the initial parameters (copied, not changed); `batch_rows` int64 [n_steps, bsz]: the rows
    step s trains on; `state` = (adam, t) as returned by an earlier call -- adam = [m(W_0), v(W_0), m(b_0), v(b_0), m(W_1), ...], t the
    Adam steps taken so far -- or None: zeros.  `losses` f32 [n_steps].  The same input gives the same parameters and moments bit for bit
    (include/lmi_hip.h states the arithmetic; tests/train_ref.py restates it).  A float16 `x` (numpy, or a contiguous torch.float16
    tensor on the device) goes to `lmi_train_f16` as it is -- the named rows are uploaded as halves and widened on the device -- and
    everything returned, losses included, is bit for bit that of the call on `x` widened to float32.  Argument errors raise ValueError
    before the library is loaded."""
    is_np = _array_arg("train", "x", x)
    if isinstance(labels, np.ndarray) != is_np:
        raise ValueError("train: x and labels must both be numpy arrays or both be tensors on the device")
    f16 = _is_f16(x)
    _array_arg("train", "x", x, "float16" if f16 else "float32")
    _array_arg("train", "labels", labels, "int32", kind=False)
    _array_arg("train", "x", x, rank="nd")
    n, d = int(x.shape[0]), int(x.shape[1])
    if tuple(labels.shape) != (n,):
        raise ValueError(f"train: labels must be [{n}], not {tuple(labels.shape)}")
    Ws = [np.array(W, dtype=np.float32, order="C") for W, _ in layers]
    bs = [np.array(b, dtype=np.float32, order="C") for _, b in layers]
    nl = len(Ws)
    if nl < 1:
        raise ValueError("train: no layers")
    dims = [d] + [int(W.shape[0]) for W in Ws]
    for i, (W, b) in enumerate(zip(Ws, bs)):
        if W.shape != (dims[i + 1], dims[i]) or b.shape != (dims[i + 1],):
            raise ValueError(f"train: layer {i} must be W [{dims[i + 1]},{dims[i]}] and b [{dims[i + 1]}], not {W.shape} and {b.shape}")
    rows = np.ascontiguousarray(batch_rows, dtype=np.int64)
    if rows.ndim != 2 or rows.shape[1] < 1:
        raise ValueError(f"train: batch_rows must be [n_steps,bsz] with bsz >= 1, not {rows.shape}")
    n_steps, bsz = int(rows.shape[0]), int(rows.shape[1])
    if not (np.isfinite(lr) and lr > 0):
        raise ValueError(f"train: lr {lr} is not a finite positive number")
    shapes = [s for W, b in zip(Ws, bs) for s in (W.shape, W.shape, b.shape, b.shape)]
    if state is None:
        adam, t0 = [np.zeros(s, dtype=np.float32) for s in shapes], 0
    else:
        adam, t0 = [np.array(a, dtype=np.float32, order="C") for a in state[0]], int(state[1])
        if [a.shape for a in adam] != shapes:
            raise ValueError("train: state[0] must hold m(W), v(W), m(b), v(b) of every layer, in the layers' shapes")
        if t0 < 0:
            raise ValueError(f"train: state t {t0} < 0")
    if is_np:
        x, labels, on_device = np.ascontiguousarray(x), np.ascontiguousarray(labels), 0
    else:
        if not (x.is_cuda and x.is_contiguous() and labels.is_cuda and labels.is_contiguous()):
            raise ValueError("train: torch x and labels must be contiguous tensors on the device")
        device, on_device = _sync_device(x), 1
    losses = np.zeros(n_steps, dtype=np.float32)
    t = ctypes.c_int64(t0)
    dims_c = (ctypes.c_int32 * (nl + 1))(*dims)
    Wp = (_vp * nl)(*[W.ctypes.data for W in Ws])
    bp = (_vp * nl)(*[b.ctypes.data for b in bs])
    ap = (_vp * (4 * nl))(*[a.ctypes.data for a in adam])
    call = lib().lmi_train_f16 if f16 else lib().lmi_train
    _check(call(int(device), _ptr(x), n, _ptr(labels), nl, dims_c, Wp, bp, ap, ctypes.byref(t), _ptr(rows), n_steps, bsz,
                float(lr), _ptr(losses), on_device))
    return list(zip(Ws, bs)), (adam, int(t.value)), losses
