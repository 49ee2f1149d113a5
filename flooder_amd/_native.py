"""ctypes binding of ``libflooder_hip.so`` (C ABI declared in ``include/flooder_hip.h``).

There is no CPU fallback: if the shared library is missing or cannot be loaded, every GPU
entry point raises ``ImportError`` telling the user to build it (``python -m flooder_amd.build``).
"""

from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_uint32, c_void_p

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# FLOODER_HIP_LIB: another build of the library (the diagnostic variants of tools/gpu_session.sh are built beside
# the product library and selected here - the product file is never overwritten)
LIB_PATH = os.environ.get("FLOODER_HIP_LIB") or os.path.join(_PKG_DIR, "libflooder_hip.so")



class _Block(ctypes.Structure):
    """A parameter block of include/flooder_hip.h: ``size`` and ``abi`` are filled in, fields are set by NAME (a
    keyword that is not a field of the struct is a TypeError), tensors are passed as their ``data_ptr()``."""

    ABI = 1

    def __init__(self, **fields):
        super().__init__()
        self.size = ctypes.sizeof(self)
        self.abi = self.ABI
        known = {name for name, _ in self._fields_}
        for key, value in fields.items():
            if key not in known:
                raise TypeError(f"{type(self).__name__} has no field {key!r}")
            if value is not None and not isinstance(value, (int, float)):
                value = ptr(value)
            setattr(self, key, value)


def _fields(spec: str):
    """``"p pts_sorted; i64 n_pts; i32 dim"`` -> ctypes fields (p: pointer, i64 / i32 / u32 / f32)."""
    kinds = {"p": c_void_p, "i64": c_int64, "i32": c_int32, "u32": c_uint32, "f32": c_float}
    out = []
    for item in spec.replace("\n", " ").split(";"):
        item = item.strip()
        if item:
            kind, name = item.split()
            out.append((name, kinds[kind]))
    return out


class FusedSweep(_Block):
    """``flooder_fused_sweep_t``: the buffers the three launches of the fused 2-D / 3-D sweep share."""

    _fields_ = _fields("""u32 size; u32 abi; p pts_sorted; i64 n_pts; i32 dim; i32 k1; p nodes; p density_grid; p cloud_box;
        p verts; p weights; i32 R; i32 n_faces; i64 n_simplices; p memb; f32 alpha; i32 n_coarse; p coarse_rows; p parents;
        p face_bits; p face_slot; p d2_scratch; p flag_list; p flag_count; p flag_key; p flag_hist; p flag_sorted; p top;
        p top_list; p top_count; p simplex_weight; p plane_scratch; p wit_queue; p wit_item_list; p wit_stats;
        p cell_queue; p defer_list; p defer_c; p defer_ctl; p light_list; p heavy_list; p cell_stats; p finish_ctl;
        p hard_scratch; i32 hard_cap; i32 probed; p finish_stats; p wit_runs; i32 wit_run_len; i32 wit_n_runs;
        i32 planes_ready; i32 reserved; p face_owner; p min_face; p chunk_faces; p tile_faces""")


class SortedSweep(_Block):
    """``flooder_sorted_sweep_t``: the sorted-sample sweep above three dimensions."""

    _fields_ = _fields("""u32 size; u32 abi; p pts_sorted; i64 n_pts; i32 dim; i32 k1; p nodes; p verts; p weights; i32 R;
        i32 n_faces; i64 n_simplices; p sample_order; p queue; p memb; p face_bits; p face_slot; p stats; p out_d2;
        i32 shard_rank; i32 shard_world""")


class FpsBatched(_Block):
    """``flooder_fps_batched_t``: the batched landmark selection."""

    _fields_ = _fields("""u32 size; u32 abi; p pts; i64 n_pts; i32 dim; i32 ld; p pts_sorted; p order; i64 start; i32 n_lms;
        i32 reserved; p out_idx; p minsq; p bucket_box; p bucket_keys; p bucket_coord; p work_best; p work_rec; p work_ctr;
        p launches_out""")


class WitnessSearch(_Block):
    """``flooder_witness_search_t``: the exact witness point of every distinct face (flooder_amd.grad)."""

    _fields_ = _fields("""u32 size; u32 abi; p pts_sorted; i64 n_pts; i32 dim; i32 k1; p nodes; p order; p verts; p weights;
        i32 R; i32 reserved; i64 n_simplices; i64 n_queries; p q_simplex; p q_row; p q_d2; p out_point; p not_found""")


class KnnSweep(_Block):
    """``flooder_knn_sweep_t``: the tree sweep that keeps the k nearest points of every sample (robust filtration)."""

    _fields_ = _fields("""u32 size; u32 abi; p pts_sorted; i64 n_pts; i32 dim; i32 k1; p nodes; p verts; p weights; i32 R;
        i32 k; i64 n_simplices; i32 stat; i32 reserved; p queue; p out_bits; p stats""")


class KnnSorted(_Block):
    """``flooder_knn_sorted_t``, ``flooder_knn_sweep_t`` and a tail: the k-nearest sweep over tiles of 64 consecutive
    entries of a sample order (the robust dimension pass above 3-D; ``neighbor_distance`` in its query form k1 = R = 1)."""

    _fields_ = KnnSweep._fields_ + _fields("p sample_order")


class KnnIds(_Block):
    """``flooder_knn_ids_t``, ``flooder_knn_sorted_t`` and a tail (the library serves the three blocks as one, the longest):
    the sweep over sorted tiles keeping (d2 word, original id) keys - which points the k nearest of every sample are
    (``nearest_neighbors``, the backward of ``neighbor_distance``)."""

    _fields_ = KnnSorted._fields_ + _fields("p order; p out_ids; p out_d2")


KNN_COLS_MAX = 64  # FLOODER_KNN_COLS_MAX: every (k, stat) pair with k <= 32 and two statistics


class KnnProfile(_Block):
    """``flooder_knn_profile_t``: one k-nearest sweep at the largest k that writes a plane per (k, stat) column.
    ``columns``: the (k, stat index) pairs in the caller's order (fills ``n_cols``, ``col_k`` and ``col_stat``)."""

    _fields_ = _fields("""u32 size; u32 abi; p pts_sorted; i64 n_pts; i32 dim; i32 k1; p nodes; p verts; p weights; i32 R;
        i32 n_cols; i64 n_simplices; p queue; p out_bits; p stats""") + [("col_k", c_int32 * KNN_COLS_MAX),
                                                                        ("col_stat", c_int32 * KNN_COLS_MAX)]

    def __init__(self, columns=(), **fields):
        super().__init__(**fields)
        columns = list(columns)
        if columns:
            if len(columns) > KNN_COLS_MAX:
                raise ValueError(f"KnnProfile holds at most {KNN_COLS_MAX} columns, got {len(columns)}")
            self.n_cols = len(columns)
            for c, (k, stat) in enumerate(columns):
                self.col_k[c] = int(k)
                self.col_stat[c] = int(stat)


class WitnessKnn(_Block):
    """``flooder_witness_knn_t``: the k points that realise a robust value (flooder_amd.grad, neighbors > 1)."""

    _fields_ = _fields("""u32 size; u32 abi; p pts_sorted; i64 n_pts; i32 dim; i32 k1; p nodes; p order; p verts; p weights;
        i32 R; i32 k; i64 n_simplices; i64 n_queries; p q_simplex; p q_row; p q_stat; p out_ids; p out_d2; p not_found;
        i32 stat; i32 reserved""")


class KnnMerge(_Block):
    """``flooder_knn_merge_t``: the exact k-best merge of the point shards' lists (robust filtration, ``mode="points"``)."""

    _fields_ = _fields("""u32 size; u32 abi; p lists; i64 n_cells; i32 n_lists; i32 k; i32 stat; i32 reserved;
        p out_bits""")


class KnnWide(_Block):
    """``flooder_knn_wide_t``: the k nearest points of every cell for k up to 1024, one wave per cell, the list in LDS
    (``flood_complex(neighbor_mass=m)``, ``distance_to_measure``)."""

    _fields_ = _fields("""u32 size; u32 abi; p pts_sorted; i64 n_pts; i32 dim; i32 k1; p nodes; p verts; p weights; i32 R;
        i32 k; i64 n_simplices; i32 stat; i32 reserved; p order; p sample_order; p out_bits; p out_ids; p out_d2""")


POWER_COLS_MAX = 8  # FLOODER_POWER_COLS_MAX: weight columns of one power-profile sweep


def column_arrays(columns):
    """(k, stat index) pairs -> (n_cols, col_k, col_stat): the host int32 arrays ``flooder_knn_wide_profile_f32`` reads
    before its launch (at most ``KNN_COLS_MAX`` columns)."""
    columns = list(columns)
    if len(columns) > KNN_COLS_MAX:
        raise ValueError(f"flooder_knn_wide_profile_f32 takes at most {KNN_COLS_MAX} columns, got {len(columns)}")
    n = len(columns)
    return n, (c_int32 * max(n, 1))(*[int(k) for k, _ in columns]), (c_int32 * max(n, 1))(*[int(s) for _, s in columns])


# The control words of the fused sweep (include/flooder_hip.h, FLOODER_<name>: int32 word offsets into finish_ctl,
# defer_ctl and the queue areas); tests/test_host.py compiles the header and compares
QUEUE_WORDS = 512
FINISH_CTL_PASS_HEADS, FINISH_CTL_TOP_COUNT = 0, 3
FINISH_CTL_TOP_HARD_HEAD, FINISH_CTL_TOP_HARD_LEN, FINISH_CTL_REST_HARD_HEAD, FINISH_CTL_REST_HARD_LEN = 4, 5, 6, 7
FINISH_CTL_SINGLE_LEFT, FINISH_CTL_QUEUES, FINISH_CTL_WORDS = 8, 24, 24 + 3 * QUEUE_WORDS
FLAG_HIST_WORDS = 8192
DEFER_CTL_COUNT, DEFER_CTL_QUEUE, DEFER_CTL_LIGHT, DEFER_CTL_HEAVY, DEFER_CTL_SPLIT_DONE = 0, 1, 2, 3, 4
DEFER_CTL_TILE_COUNT, DEFER_CTL_WORDS = 6, 8
CELL_QUEUE_RUNS, CELL_QUEUE_CHUNKS, CELL_QUEUE_TILES, CELL_QUEUE_WORDS = 0, QUEUE_WORDS, 2 * QUEUE_WORDS, 3 * QUEUE_WORDS
WIT_QUEUE_ITEM_COUNT = QUEUE_WORDS - 1

_lib = None
_load_error: Exception | None = None
_load_missing = False  # the last failure was "file not found" (worth another look after a build)

# name -> (restype, argtypes); the single source the symbol test checks against the header
SIGNATURES = {
    "flooder_abi_version": (c_int, []),
    "flooder_last_error": (c_char_p, []),
    "flooder_device_arch": (c_int, [c_int, c_char_p, c_int]),
    "flooder_set_option": (c_int, [c_char_p, c_int]),
    "flooder_get_option": (c_int, [c_char_p, ctypes.POINTER(c_int)]),
    "flooder_padded_dim": (c_int, [c_int]),
    "flooder_ball_count_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_int64, c_void_p, c_void_p]),
    "flooder_ball_fill_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                      c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_sweep_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int, c_int,
                                  c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_face_max_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_void_p,
                                     c_void_p, c_void_p]),
    "flooder_bbox_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "flooder_bbox_chunk_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_int, c_void_p]),
    "flooder_bbox_reduce_f32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_void_p]),
    "flooder_morton_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "flooder_morton_zero_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "flooder_curve_key_bits": (c_int, [c_int]),
    "flooder_index_sort_bytes": (c_int64, [c_int64]),
    "flooder_index_sort": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "flooder_index_sort_state_words": (c_int64, [c_int64, c_int]),
    "flooder_index_sort_zeroed": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p,
                                          c_void_p]),
    "flooder_kd_order_bytes": (c_int64, [c_int64]),
    "flooder_kd_order_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "flooder_select_grid_bytes": (c_int64, [c_int]),
    "flooder_box_select_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                       c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_gather_rows_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "flooder_bvh_node_count": (c_int64, [c_int64]),
    "flooder_bvh_build_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "flooder_index_rows_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                       c_void_p, c_void_p]),
    "flooder_sweep_bvh_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                      c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_sample_key_bits": (c_int, [c_int]),
    "flooder_sorted_tile_samples": (c_int, []),
    "flooder_sample_keys_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "flooder_sample_keys_late_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p]),
    "flooder_sweep_bvh_items_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                            c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                            c_void_p, c_void_p, c_void_p]),
    "flooder_sweep_cell_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                       c_int64, c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p]),
    "flooder_density_grid_words": (c_int64, [c_int]),
    "flooder_density_grid_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "flooder_cloud_kind": (c_int, [c_void_p, c_int, c_void_p]),
    "flooder_wit_max_rows": (c_int, []),
    "flooder_wit_max_coarse": (c_int, []),
    "flooder_finish_single_tiles": (c_int, []),
    "flooder_finish_single_batches": (c_int, []),
    "flooder_face_values_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "flooder_face_closure_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "flooder_simplex_weight_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p]),
    "flooder_simplex_planes_forget": (None, []),
    "flooder_simplex_prepare_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                            c_int64, c_void_p]),
    "flooder_selftest": (c_int, [c_void_p, c_void_p, c_void_p]),
    "flooder_wit_probe_f32": (c_int, [c_void_p, c_int, c_int64, c_float, c_void_p, c_void_p, c_int64, c_void_p, c_int, c_void_p,
                                      c_void_p, c_void_p]),
    "flooder_fill_u32": (c_int, [c_void_p, c_int64, c_uint32, c_void_p]),
    "flooder_gather_rows_f64": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    "flooder_sweep_bvh_f64": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64,
                                      c_void_p, c_void_p, c_void_p]),
    "flooder_face_max_f64": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "flooder_fps_bucket_count": (c_int64, [c_int64]),
    "flooder_fps_indexed_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_int64, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_fps_batched_max_points": (c_int64, []),
    "flooder_fps_batched_rec_words": (c_int64, [c_int64, c_int, c_int]),
    "flooder_fps_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_int, c_int64, c_void_p, c_void_p,
                                c_void_p, c_void_p]),
    # the parameter-block forms of the long entry points (what the default path calls)
    "flooder_fused_witness": (c_int, [ctypes.POINTER(FusedSweep), c_void_p]),
    "flooder_fused_cell": (c_int, [ctypes.POINTER(FusedSweep), c_void_p]),
    "flooder_fused_finish": (c_int, [ctypes.POINTER(FusedSweep), c_void_p]),
    "flooder_sorted_faces": (c_int, [ctypes.POINTER(SortedSweep), c_void_p]),
    "flooder_sorted_minima": (c_int, [ctypes.POINTER(SortedSweep), c_void_p]),
    "flooder_fps_batched": (c_int, [ctypes.POINTER(FpsBatched), c_void_p]),
    # witnesses of the filtration values and the scatter of their gradients (flooder_amd.grad)
    "flooder_face_argmax_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                        c_void_p]),
    "flooder_witness_search": (c_int, [ctypes.POINTER(WitnessSearch), c_void_p]),
    "flooder_segment_sum_f32": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    # the k nearest points of every sample (flood_complex(neighbors=k))
    "flooder_sweep_knn_f32": (c_int, [ctypes.POINTER(KnnSweep), c_void_p]),
    # ... the same sweep over tiles of the sorted sample order (above 3-D; neighbor_distance)
    "flooder_sweep_knn_sorted_f32": (c_int, [ctypes.POINTER(KnnSorted), c_void_p]),
    # ... keeping (d2 word, original id) keys: the neighbours themselves (nearest_neighbors, neighbor_distance's backward)
    "flooder_knn_ids_sorted_f32": (c_int, [ctypes.POINTER(KnnIds), c_void_p]),
    # ... every (k, stat) column of a list from one sweep at the largest k (flood_profile)
    "flooder_sweep_knn_profile_f32": (c_int, [ctypes.POINTER(KnnProfile), c_void_p]),
    # ... and which k points realise the statistic of a witness sample (flood_filtration(neighbors=k))
    "flooder_witness_knn": (c_int, [ctypes.POINTER(WitnessKnn), c_void_p]),
    # ... and the k best of the union of the point shards' k best (flood_complex(neighbor_reduce_hook=...))
    "flooder_knn_merge_f32": (c_int, [ctypes.POINTER(KnnMerge), c_void_p]),
    # ... and the k nearest for k up to 1024, one wave per cell (flood_complex(neighbor_mass=m), distance_to_measure)
    "flooder_knn_wide_f32": (c_int, [ctypes.POINTER(KnnWide), c_void_p]),
    # ... and every (k, stat) column of that list from one walk at the largest k: the same block, then n_cols, the
    # host arrays col_k and col_stat (int32) and plane_stride (distance_to_measure_profile)
    "flooder_knn_wide_profile_f32": (c_int, [ctypes.POINTER(KnnWide), c_int, c_void_p, c_void_p, c_int64, c_void_p]),
    # ... and the nearest sites of a weighted measure up to a cumulative mass: the same block (its k is the list
    # capacity), then masses, target (a device float64), ld_out and out_count (distance_to_weighted_measure)
    "flooder_knn_mass_f32": (c_int, [ctypes.POINTER(KnnWide), c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    # ... and every (target, stat) column of that list from one walk at the largest target: the same block, then masses,
    # n_cols, targets (a device float64 array), the host array col_stat (int32), plane_stride and the planes of counts
    # (distance_to_weighted_measure_profile)
    "flooder_knn_mass_profile_f32": (c_int, [ctypes.POINTER(KnnWide), c_void_p, c_int, c_void_p, c_void_p, c_int64,
                                             c_void_p, c_void_p]),
    # the weighted filtration (flood_complex(point_weights=w)): the minimum of a value per tree row over every node, and
    # the power-distance sweep on the block of the sorted k-nearest sweep (k = 1) plus the weights and their node minima
    "flooder_node_min_f32": (c_int, [c_void_p, c_int64, c_void_p, c_void_p]),
    "flooder_sweep_power_f32": (c_int, [ctypes.POINTER(KnnSorted), c_void_p, c_void_p, c_void_p]),
    # ... for up to 8 interleaved weight columns in one walk of the tree: the same block, then n_cols, w_cols and
    # node_w_cols (power_profile, dtm_profile)
    "flooder_node_min_cols_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p]),
    "flooder_sweep_power_profile_f32": (c_int, [ctypes.POINTER(KnnSorted), c_int, c_void_p, c_void_p, c_void_p]),
    # ... and which point attains a power word: the witness search's block plus the same two pointers (power_filtration)
    "flooder_witness_power": (c_int, [ctypes.POINTER(WitnessSearch), c_void_p, c_void_p, c_void_p]),
    # the backward of the distance to a measure (distance_to_measure(differentiable=True)): per query the sum over its
    # listed neighbours, and its transpose over the entries sorted by target
    "flooder_dtm_grad_queries_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int,
                                             c_void_p, c_void_p, c_void_p]),
    "flooder_dtm_grad_points_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int64, c_void_p, c_void_p]),
    # ... and of the distance to a WEIGHTED measure (distance_to_weighted_measure(differentiable=True)) over the rows and
    # counts of flooder_knn_mass_f32: sites are (n, dim + 1) rows (coordinates, then the mass), qrow the (Q, 4) crossing
    # rows (coefficient in; rho, crossing id, dstar2 out); then the two transposes, into the sites and into the masses
    "flooder_mass_grad_queries_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p,
                                              c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_mass_grad_points_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_int64, c_void_p, c_void_p]),
    "flooder_mass_grad_masses_f32": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_int64, c_void_p, c_void_p]),
}

# The positional forms of the five entry points above: still exported by the library (same symbols as before round 6),
# typed here so that the symbol test covers them and tests can call them, but nothing in flooder_amd does.
POSITIONAL_SIGNATURES = {
    "flooder_sweep_bvh_sorted_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                             c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_sweep_bvh_sorted_shard_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                                   c_int64, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p,
                                                   c_void_p]),
    "flooder_sweep_cell_faces_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                             c_int64, c_float, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_sweep_witness_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64,
                                          c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "flooder_finish_faces_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int64,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                         c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "flooder_sweep_bvh_sorted_faces_f32": (c_int, [c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                                   c_int64, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                                   c_void_p, c_void_p]),
    "flooder_fps_batched_f32": (c_int, [c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p, c_int, c_int64, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
}


def load():
    """Load the library once (after torch, so both share one HIP runtime) and type its symbols."""
    global _lib, _load_error, _load_missing
    if _lib is not None:
        return _lib
    if _load_error is not None:
        # (a library that was missing may have been built since - __graft_entry__.build() imports the package
        # before it compiles: look again; any other failure stays cached)
        if not (_load_missing and os.path.exists(LIB_PATH)):
            raise ImportError(str(_load_error)) from _load_error
        _load_error = None
    try:
        import torch  # noqa: F401  (loads libamdhip64.so.7 first; our DT_NEEDED resolves to it)

        _load_missing = not os.path.exists(LIB_PATH)
        if _load_missing:
            raise OSError(f"{LIB_PATH} not found")
        lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        for name, (res, args) in {**SIGNATURES, **POSITIONAL_SIGNATURES}.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        from .build import ROOT  # noqa: F401

        if lib.flooder_abi_version() != 1:
            raise OSError(f"ABI version mismatch: library reports {lib.flooder_abi_version()}, binding expects 1")
        _lib = lib
        return lib
    except Exception as exc:  # noqa: BLE001
        _load_error = ImportError(
            f"flooder_amd: the HIP kernel library could not be loaded ({exc}). "
            "Build it with `python -m flooder_amd.build` (needs hipcc, --offload-arch=gfx950). "
            "There is no CPU fallback for CUDA/ROCm tensors."
        )
        raise _load_error from exc


def available() -> bool:
    try:
        load()
        return True
    except ImportError:
        return False


def check(rc: int, what: str) -> None:
    if rc != 0:
        lib = load()
        msg = lib.flooder_last_error()
        raise RuntimeError(f"{what} failed (code {rc}): {msg.decode() if msg else '?'}")


def ptr(t) -> int:
    """Raw device (or host) address of a contiguous torch tensor; None -> NULL."""
    if t is None:
        return 0
    if not t.is_contiguous():
        raise ValueError("tensor passed to the native library must be contiguous")
    return t.data_ptr()


def current_stream_ptr(device) -> int:
    import torch

    return torch.cuda.current_stream(device).cuda_stream
