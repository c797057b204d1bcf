"""ctypes binding of include/hsearch.h.  No compute here; everything runs in libhsearch_amd.so."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

HS_OK, HS_ERR_INVALID, HS_ERR_NO_DEVICE, HS_ERR_HIP, HS_ERR_CAPACITY, HS_ERR_STATE, \
    HS_ERR_KEY_COLLISION, HS_ERR_NOMEM, HS_ERR_IO, HS_ERR_PEER = range(10)
_STATUS = ["HS_OK", "HS_ERR_INVALID", "HS_ERR_NO_DEVICE", "HS_ERR_HIP", "HS_ERR_CAPACITY",
           "HS_ERR_STATE", "HS_ERR_KEY_COLLISION", "HS_ERR_NOMEM", "HS_ERR_IO", "HS_ERR_PEER"]

# Row order of the embedding table (include/hs_tables.h HS_CODE_TO_LETTER): BLOSUM order.
_ALPHABET = "ARNDCQEGHILKMFPSTWYV"

EXPORTS = ["hs_create", "hs_destroy", "hs_last_error", "hs_get_profile", "hs_get_params", "hs_version",
           "hs_set_verify_mode", "hs_set_hash_mode", "hs_set_option", "hs_set_bucket_partition", "hs_set_multiprobe", "hs_probe_buckets", "hs_wait_event", "hs_set_planes", "hs_self_join", "hs_self_join_range", "hs_clustering",
           "hs_clustering_begin", "hs_clustering_table_edges", "hs_clustering_table_apply",
           "hs_clustering_end",
           "hs_embed_codes", "hs_hash_codes", "hs_hash_points", "hs_key_string", "hs_key_fingerprint",
           "hs_key_strings_equal", "hs_index_build", "hs_index_build_subset", "hs_index_build_windows", "hs_index_shard_begin", "hs_index_shard_hash_dev", "hs_index_shard_group_dev",
           "hs_index_shard_tuples_dev", "hs_index_shard_finish_dev", "hs_index_shard_end", "hs_index_save", "hs_index_load", "hs_index_file_check", "hs_klsh_draw_planes", "hs_klsh_codes",
           "hs_index_info_get", "hs_query", "hs_query_dev", "hs_query_codes", "hs_query_codes_dev", "hs_bruteforce",
           "hs_bruteforce_topk", "hs_merge_first_table_dev", "hs_query_radii", "hs_query_radii_dev",
           "hs_bruteforce_radii", "hs_annotate", "hs_annotate_dev", "hs_merge_best", "hs_components", "hs_components_dev",
           "hs_components_range", "hs_components_range_dev", "hs_components_merge", "hs_degrees", "hs_degrees_dev",
           "hs_degrees_range", "hs_degrees_range_dev", "hs_dbscan", "hs_dbscan_dev", "hs_dbscan_edges",
           "hs_cluster_profile", "hs_cluster_profile_dev", "hs_cluster_radii", "hs_cluster_radii_dev",
           "hs_cluster_summary_codes", "hs_msf", "hs_msf_dev", "hs_msf_edges", "hs_msf_cut", "hs_core_distance",
           "hs_core_distance_dev", "hs_density_tree", "hs_density_tree_dev", "hs_density_tree_edges",
           "hs_density_tree_cut", "hs_query_topk", "hs_query_topk_dev", "hs_self_knn", "hs_self_knn_range",
           "hs_self_knn_dev", "hs_self_knn_range_dev", "hs_topk_merge", "hs_seq_match", "hs_seq_match_dev",
           "hs_window_id_start", "hs_seq_match_hits", "hs_seq_match_merge", "hs_join6_tables", "hs_join6_thresholds",
           "hs_join6_selftest", "hs_join6_tile_offset", "hs_index_append", "hs_index_append_dev", "hs_index_append_windows",
           "hs_index_table_append", "hs_index_remove", "hs_index_remove_dev", "hs_index_remove_ranges",
           "hs_index_table_remove", "hs_pssm_scan", "hs_pssm_scan_dev", "hs_pssm_tables",
           "hs_pssm_topk", "hs_pssm_topk_dev", "hs_pssm_topk_hits", "hs_pssm_seq_scan", "hs_pssm_seq_scan_dev",
           "hs_pssm_seq_hits", "hs_pssm_hit_counts", "hs_pssm_hit_counts_dev", "hs_pssm_refine", "hs_pssm_count_hits",
           "hs_pssm_rank", "hs_pssm_rank_dev", "hs_pssm_rank_scores", "hs_pssm_rank_plan", "hs_pssm_refine_rank",
           "hs_pssm_log_odds", "hs_pssm_background", "hs_pssm_pvalue", "hs_pssm_pvalue_dev",
           "hs_pssm_pvalue_threshold", "hs_pssm_pvalue_threshold_dev", "hs_pssm_null_tables", "hs_pssm_pvalue_host",
           "hs_pssm_threshold_host", "hs_pssm_weighted_counts", "hs_pssm_weighted_counts_dev",
           "hs_pssm_refine_weighted", "hs_pssm_weight_hits", "hs_pssm_log_odds_weighted", "hs_pssm_weight_u",
           "hs_cluster_weighted_profile", "hs_cluster_weighted_profile_dev", "hs_cluster_pssm_cover",
           "hs_cluster_pssm_cover_dev", "hs_cluster_weights_codes", "hs_cluster_cover_codes",
           "hs_pssm_compare", "hs_pssm_compare_dev", "hs_pssm_compare_host", "hs_pssm_compare_tables",
           "hs_pssm_compare_pass", "hs_pssm_compare_columns", "hs_pssm_family_scan", "hs_pssm_family_scan_dev",
           "hs_pssm_family_hits", "hs_pssm_family_layout", "hs_pssm_family_chain", "hs_pssm_family_chain_dev",
           "hs_pssm_family_chain_hits"]

TOPK_MAX = 64        # HS_TOPK_MAX: the widest row of query_topk / self_knn / topk_merge
NO_ID = 0xffffffff   # the id and table of an unused entry of such a row (its distance is +inf)
NOISE = 0xffffffff   # HS_NOISE: the label of a k-mer that is neither core nor border (hs_dbscan)


class HsError(RuntimeError):
    def __init__(self, status, message):
        self.status = status
        name = _STATUS[status] if 0 <= status < len(_STATUS) else str(status)
        super().__init__("%s: %s" % (name, message))


class _Params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("K", C.c_uint32), ("L", C.c_uint32), ("W", C.c_double),
                ("device", C.c_int32), ("alphabet", C.c_uint32)]


class _Profile(C.Structure):
    _fields_ = [("ms_hash", C.c_double), ("ms_sort", C.c_double), ("ms_gather", C.c_double),
                ("ms_probe", C.c_double), ("ms_verify", C.c_double), ("ms_finalize", C.c_double),
                ("ms_total", C.c_double), ("candidates", C.c_uint64), ("provisional", C.c_uint64),
                ("hits", C.c_uint64), ("verify_launches", C.c_uint64), ("join_batches", C.c_uint64),
                ("ms_join", C.c_double), ("join_items", C.c_uint64), ("join_pairs", C.c_uint64),
                ("join_pairs_issued", C.c_uint64), ("join_i8_batches", C.c_uint64),
                ("hash_values", C.c_uint64), ("hash_flagged", C.c_uint64),
                ("join_row_bytes", C.c_uint32), ("join_wide", C.c_uint32), ("join_items_resident", C.c_uint64),
                ("join_async_retries", C.c_uint64), ("queries_recognised", C.c_uint64),
                ("join_f6_batches", C.c_uint64), ("join_f6_wide_items", C.c_uint64),
                ("append_rebuilds", C.c_uint64),
                ("append_new_buckets", C.c_uint64), ("remove_rebuilds", C.c_uint64),
                ("remove_dead_buckets", C.c_uint64), ("remove_retupled", C.c_uint64),
                ("pssm_pairs", C.c_uint64), ("pssm_survivors", C.c_uint64), ("pssm_dead", C.c_uint64),
                ("pssm_mfma_steps", C.c_uint64), ("pssm_seq_rows", C.c_uint64), ("pssm_fam_rows", C.c_uint64),
                ("pssm_fam_kept", C.c_uint64), ("pssm_chain_segs", C.c_uint64), ("pssm_chain_kept", C.c_uint64),
                ("pssm_count_sites", C.c_uint64),
                ("pssm_count_items", C.c_uint64), ("pssm_weight_sites", C.c_uint64),
                ("pssm_weight_items", C.c_uint64), ("pssm_null_bins", C.c_uint64),
                ("pssm_null_profiles", C.c_uint64), ("summary_weight_rows", C.c_uint64),
                ("summary_weight_items", C.c_uint64), ("pssm_cmp_pairs", C.c_uint64),
                ("pssm_cmp_survivors", C.c_uint64), ("pssm_cmp_steps", C.c_uint64), ("pssm_rank_sample", C.c_uint64),
                ("pssm_rank_retries", C.c_uint64), ("pssm_topk_sample", C.c_uint64),
                ("pssm_topk_raised", C.c_uint64)]


class _IndexInfo(C.Structure):
    _fields_ = [("n", C.c_uint64), ("device_bytes", C.c_uint64), ("n_buckets", C.c_uint64 * 32),
                ("max_bucket", C.c_uint64 * 32), ("key_seed", C.c_uint32)]


class _DbscanCounts(C.Structure):
    _fields_ = [("n_clusters", C.c_uint64), ("n_core", C.c_uint64), ("n_border", C.c_uint64),
                ("n_noise", C.c_uint64), ("n_edges", C.c_uint64)]


class _MsfInfo(C.Structure):
    _fields_ = [("n_tree_edges", C.c_uint64), ("n_components", C.c_uint64), ("n_graph_edges", C.c_uint64),
                ("rounds", C.c_uint32), ("resident", C.c_uint32)]


class _DensityInfo(C.Structure):
    _fields_ = [("n_tree_edges", C.c_uint64), ("n_clusters", C.c_uint64), ("n_core", C.c_uint64),
                ("n_graph_edges", C.c_uint64), ("rounds", C.c_uint32), ("resident", C.c_uint32),
                ("self_joins", C.c_uint32)]


profile_fields = [f[0] for f in _Profile._fields_]

_libs = {}


def lib_path(hooks=False):
    # HSEARCH_AMD_LIB: another build of the same library (A/B runs of two kernel versions on one box)
    if hooks:
        return os.path.join(_HERE, "libhsearch_amd_hooks.so")
    return os.environ.get("HSEARCH_AMD_LIB") or os.path.join(_HERE, "libhsearch_amd.so")


def load(hooks=False):
    """Load libhsearch_amd.so.  Raises (never falls back) when it has not been built.
    hooks=True: the TEST build of the same library (libhsearch_amd_hooks.so: the same kernel objects
    under a C-ABI layer compiled with -DHS_TEST_HOOKS = fault injection), for the tests that need it."""
    if hooks not in _libs:
        # One ROCm runtime per process: PyTorch ships its own libamdhip64 / libhsa-runtime64 / librccl.
        # If this library (linked against /opt/rocm's) is loaded BEFORE torch, the process ends up with
        # /opt/rocm's HIP + HSA and, once torch is imported, torch's RCCL, whose dlopen of
        # "libhsa-runtime64.so" then maps a second, uninitialised HSA copy (ncclCommInitAll: "no
        # ROCm-capable device").  Importing torch first makes every later load resolve to its copies.
        # (The C++ programs under hsearch_amd/host have no torch and use /opt/rocm's throughout.)
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        path = lib_path(hooks)
        if not os.path.exists(path):
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; "
                              "g.build()'` (or make -C hsearch_amd/csrc)" % path)
        lib = C.CDLL(path)
        lib.hs_version.restype = C.c_char_p
        lib.hs_last_error.restype = C.c_char_p
        lib.hs_last_error.argtypes = [C.c_void_p]
        lib.hs_destroy.restype = None
        lib.hs_destroy.argtypes = [C.c_void_p]
        lib.hs_key_string.restype = C.c_uint32
        lib.hs_key_fingerprint.restype = C.c_uint64
        lib.hs_key_strings_equal.restype = C.c_int
        # per-query radii: (h, centers, qcodes, nq, radii, hit_q, hit_id, hit_table, hit_dist, cap, n_hits, cand)
        # (HSEARCH_AMD_LIB may name an older build without them: its calls then fail by name, not here)
        if hasattr(lib, "hs_query_radii"):
            for fn in (lib.hs_query_radii, lib.hs_query_radii_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
            lib.hs_bruteforce_radii.restype = C.c_int
            lib.hs_bruteforce_radii.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        # annotation: (h, centers, qcodes, nq, R, radii, out_id, out_q, out_table, out_dist, cap, n_out)
        if hasattr(lib, "hs_annotate"):
            for fn in (lib.hs_annotate, lib.hs_annotate_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
            lib.hs_merge_best.restype = C.c_int
            lib.hs_merge_best.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        # components: (h, [first, count,] R, sqrt_test, label, n_components, n_edges); merge: (labels, m, n, out, n_out)
        if hasattr(lib, "hs_components"):
            for fn in (lib.hs_components, lib.hs_components_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64)]
            for fn in (lib.hs_components_range, lib.hs_components_range_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_int, C.c_void_p,
                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            lib.hs_components_merge.restype = C.c_int
            lib.hs_components_merge.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]
        # degrees: (h, [first, count,] R, sqrt_test, degree, n_edges); dbscan: (h, R, sqrt_test, min_pts, label,
        # degree, counts); dbscan_edges: (ei, ej, n_edges, n, min_pts, label, degree, counts)
        if hasattr(lib, "hs_dbscan"):
            for fn in (lib.hs_degrees, lib.hs_degrees_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_uint64)]
            for fn in (lib.hs_degrees_range, lib.hs_degrees_range_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_int, C.c_void_p,
                               C.POINTER(C.c_uint64)]
            for fn in (lib.hs_dbscan, lib.hs_dbscan_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                               C.POINTER(_DbscanCounts)]
            lib.hs_dbscan_edges.restype = C.c_int
            lib.hs_dbscan_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_void_p,
                                            C.c_void_p, C.POINTER(_DbscanCounts)]
        # cluster summaries: profile (h, label, min_size, out_label, out_size, counts, centroid, cap, n_out); radii
        # (h, label, min_size, centers, n_rows, max_d2, radius, medoid); summary_codes: see include/hsearch.h
        if hasattr(lib, "hs_cluster_profile"):
            for fn in (lib.hs_cluster_profile, lib.hs_cluster_profile_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.POINTER(C.c_uint64)]
            for fn in (lib.hs_cluster_radii, lib.hs_cluster_radii_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                               C.c_void_p]
            lib.hs_cluster_summary_codes.restype = C.c_int
            lib.hs_cluster_summary_codes.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32,
                                                     C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p,
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        # spanning forest: msf (h, R, sqrt_test, lo, hi, dist, cap, label, info); msf_edges (ei, ej, dist, n_edges, n,
        # out_lo, out_hi, out_dist, cap, label, info); msf_cut (lo, hi, dist, m, n, r, label, n_components)
        if hasattr(lib, "hs_msf"):
            for fn in (lib.hs_msf, lib.hs_msf_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                               C.c_void_p, C.POINTER(_MsfInfo)]
            lib.hs_msf_edges.restype = C.c_int
            lib.hs_msf_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(_MsfInfo)]
            lib.hs_msf_cut.restype = C.c_int
            lib.hs_msf_cut.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_double,
                                       C.c_void_p, C.POINTER(C.c_uint64)]
        # density tree: core_distance (h, R, sqrt_test, min_pts, core, n_core, n_edges); density_tree (h, R, sqrt_test,
        # min_pts, lo, hi, w, cap, label, core, info); density_tree_edges (ei, ej, dist, n_edges, n, min_pts, out_lo,
        # out_hi, out_w, cap, label, core, info); density_tree_cut (lo, hi, w, m, core, n, r, label, n_clusters)
        if hasattr(lib, "hs_density_tree"):
            for fn in (lib.hs_core_distance, lib.hs_core_distance_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint64),
                               C.POINTER(C.c_uint64)]
            for fn in (lib.hs_density_tree, lib.hs_density_tree_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(_DensityInfo)]
            lib.hs_density_tree_edges.restype = C.c_int
            lib.hs_density_tree_edges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                  C.POINTER(_DensityInfo)]
            lib.hs_density_tree_cut.restype = C.c_int
            lib.hs_density_tree_cut.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                C.c_double, C.c_void_p, C.POINTER(C.c_uint64)]
        # top-k: query_topk (h, centers, qcodes, nq, R, radii, topk, nn_id, nn_table, nn_dist, nn_count, n_hits);
        # self_knn (h, [first, count,] R, sqrt_test, topk, nn_id, nn_table, nn_dist, nn_count, n_edges); topk_merge
        # (q, id, table, dist, n_tuples, nq, topk, nn_id, nn_table, nn_dist, nn_count)
        if hasattr(lib, "hs_query_topk"):
            for fn in (lib.hs_query_topk, lib.hs_query_topk_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_uint32,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
            for fn in (lib.hs_self_knn, lib.hs_self_knn_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.POINTER(C.c_uint64)]
            for fn in (lib.hs_self_knn_range, lib.hs_self_knn_range_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_double, C.c_int, C.c_uint32, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
            lib.hs_topk_merge.restype = C.c_int
            lib.hs_topk_merge.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                          C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        # seq_match (h, centers, qcodes, nq, R, radii, q_group, n_groups, q_off, id_start, n_seq, the nine row arrays, cap,
        # n_out, n_hits); seq_match_hits (q, id, dist, n_tuples, nq, q_group, n_groups, q_off, id_start, n_seq, rows, cap,
        # n_out); seq_match_merge (the nine arrays in, n_rows, the nine out, cap, n_out)
        if hasattr(lib, "hs_seq_match"):
            rows = [C.c_void_p] * 9
            for fn in (lib.hs_seq_match, lib.hs_seq_match_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64] + rows + [
                                   C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
            lib.hs_window_id_start.restype = C.c_int
            lib.hs_window_id_start.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
            lib.hs_seq_match_hits.restype = C.c_int
            lib.hs_seq_match_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                              C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64] + rows + [
                                                  C.c_uint64, C.POINTER(C.c_uint64)]
            lib.hs_seq_match_merge.restype = C.c_int
            lib.hs_seq_match_merge.argtypes = rows + [C.c_uint64] + rows + [C.c_uint64, C.POINTER(C.c_uint64)]
        # index append: (h, codes, m); windows as hs_index_build_windows; table_append: see include/hsearch.h
        if hasattr(lib, "hs_index_append"):
            for fn in (lib.hs_index_append, lib.hs_index_append_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
            lib.hs_index_append_windows.restype = C.c_int
            lib.hs_index_append_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                    C.POINTER(C.c_uint64), C.c_void_p]
            lib.hs_index_table_append.restype = C.c_int
            lib.hs_index_table_append.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                                  C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint32)]
        # index remove: (h, ids, m, new_id); ranges: (h, first, count, n_ranges, new_id); table_remove: include/hsearch.h
        if hasattr(lib, "hs_index_remove"):
            for fn in (lib.hs_index_remove, lib.hs_index_remove_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
            lib.hs_index_remove_ranges.restype = C.c_int
            lib.hs_index_remove_ranges.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
            lib.hs_index_table_remove.restype = C.c_int
            lib.hs_index_table_remove.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                                  C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64)]
        # PSSM scan: (h, S, t, nm, hit_m, hit_id, hit_score, cap, &n_hits, cnt); tables: include/hsearch.h
        if hasattr(lib, "hs_pssm_scan"):
            for fn in (lib.hs_pssm_scan, lib.hs_pssm_scan_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
            lib.hs_pssm_tables.restype = C.c_int
            lib.hs_pssm_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        # profile against profile: (h, X, nx, Y, ny, t, v, hit_x, hit_y, hit_d, hit_score, cap, &n_hits, cnt); the host
        # rule takes (X, nx, Y, ny, k, alphabet, t, v, ...) instead; tables, pass, columns: include/hsearch.h
        if hasattr(lib, "hs_pssm_compare"):
            for fn in (lib.hs_pssm_compare, lib.hs_pssm_compare_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                               C.c_void_p]
            lib.hs_pssm_compare_host.restype = C.c_int
            lib.hs_pssm_compare_host.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32,
                                                 C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p]
            lib.hs_pssm_compare_tables.restype = C.c_int
            lib.hs_pssm_compare_tables.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p]
            lib.hs_pssm_compare_pass.restype = C.c_int
            lib.hs_pssm_compare_pass.argtypes = [C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double,
                                                 C.c_uint32, C.c_uint32, C.c_double]
            lib.hs_pssm_compare_columns.restype = C.c_int
            lib.hs_pssm_compare_columns.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p]
        # PSSM top-N: (h, S, t_floor, nm, topk, top_id, top_score, top_count, t_used); hits: include/hsearch.h
        if hasattr(lib, "hs_pssm_topk"):
            for fn in (lib.hs_pssm_topk, lib.hs_pssm_topk_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]
            lib.hs_pssm_topk_hits.restype = C.c_int
            lib.hs_pssm_topk_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
        # PSSM hits per sequence: (h, S, t, nm, id_start, n_seq, 7 row arrays, cap, &n_out, &n_hits, cnt, seq_cnt);
        # hits: (m, id, score, n_tuples, nm, id_start, n_seq, 7 row arrays, cap, &n_out)
        if hasattr(lib, "hs_pssm_seq_scan"):
            rows7 = [C.c_void_p] * 7
            for fn in (lib.hs_pssm_seq_scan, lib.hs_pssm_seq_scan_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + rows7 + [
                    C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
            lib.hs_pssm_seq_hits.restype = C.c_int
            lib.hs_pssm_seq_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                             C.c_uint64] + rows7 + [C.c_uint64, C.POINTER(C.c_uint64)]
        # PSSM families: (h, S, t, nm, m_group, n_groups, m_off, id_start, n_seq, min_count, t_group, 10 row arrays,
        # cap, &n_out, &n_hits, cnt, grp_rows); hits: (m, id, score, n_tuples, nm, m_group, ..., t_group, 10 row arrays,
        # cap, &n_out); layout: (x, y, d, n_hits, nm, group, off, order, &n_groups, &n_conflicts)
        if hasattr(lib, "hs_pssm_family_scan"):
            rows10 = [C.c_void_p] * 10
            fam = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]
            for fn in (lib.hs_pssm_family_scan, lib.hs_pssm_family_scan_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] + fam + rows10 + [
                    C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
            lib.hs_pssm_family_hits.restype = C.c_int
            lib.hs_pssm_family_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + fam + \
                rows10 + [C.c_uint64, C.POINTER(C.c_uint64)]
            lib.hs_pssm_family_layout.restype = C.c_int
            lib.hs_pssm_family_layout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                                  C.POINTER(C.c_uint64)]
        # PSSM family chains: the family scan's arguments with (max_shift, gap_open, gap_ext) in front of min_count;
        # hits: ..., 10 row arrays, cap, &n_out, path_start, path_m, path_id, path_cap, &n_path
        if hasattr(lib, "hs_pssm_family_chain"):
            rows10 = [C.c_void_p] * 10
            chain = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_double,
                     C.c_uint32, C.c_void_p]
            for fn in (lib.hs_pssm_family_chain, lib.hs_pssm_family_chain_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64] + chain + rows10 + [
                    C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
            lib.hs_pssm_family_chain_hits.restype = C.c_int
            lib.hs_pssm_family_chain_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64] + \
                chain + rows10 + [C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.POINTER(C.c_uint64)]
        # PSSM hit counts: (h, S, t, nm, id_start, n_seq, counts, cnt, used, &n_hits); refine, count_hits, log_odds,
        # background: include/hsearch.h
        if hasattr(lib, "hs_pssm_hit_counts"):
            for fn in (lib.hs_pssm_hit_counts, lib.hs_pssm_hit_counts_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
            lib.hs_pssm_refine.restype = C.c_int
            lib.hs_pssm_refine.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                           C.c_void_p, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
            lib.hs_pssm_count_hits.restype = C.c_int
            lib.hs_pssm_count_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p,
                                               C.c_void_p]
            lib.hs_pssm_log_odds.restype = C.c_int
            lib.hs_pssm_log_odds.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_double,
                                             C.c_void_p]
            lib.hs_pssm_background.restype = C.c_int
            lib.hs_pssm_background.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
        # PSSM rank: (h, S, rank, nm, t_rank, cnt_ge, cnt_gt, t_scan, rounds); scores, plan, refine_rank:
        # include/hsearch.h
        if hasattr(lib, "hs_pssm_rank"):
            for fn in (lib.hs_pssm_rank, lib.hs_pssm_rank_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_void_p]
            lib.hs_pssm_rank_scores.restype = C.c_int
            lib.hs_pssm_rank_scores.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.hs_pssm_rank_plan.restype = C.c_int
            lib.hs_pssm_rank_plan.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
            lib.hs_pssm_refine_rank.restype = C.c_int
            lib.hs_pssm_refine_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                C.c_void_p, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        # PSSM sequence weights: (h, S, t, nm, id_start, n_seq, counts, wcounts, wsum, distinct, cnt, used, &n_hits);
        # refine_weighted, weight_hits, log_odds_weighted, weight_u: include/hsearch.h
        if hasattr(lib, "hs_pssm_weighted_counts"):
            for fn in (lib.hs_pssm_weighted_counts, lib.hs_pssm_weighted_counts_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64] + [
                    C.c_void_p] * 6 + [C.POINTER(C.c_uint64)]
            lib.hs_pssm_refine_weighted.restype = C.c_int
            lib.hs_pssm_refine_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                                    C.c_void_p, C.c_uint64, C.c_void_p, C.c_double, C.c_uint32,
                                                    C.c_uint32] + [C.c_void_p] * 7 + [C.POINTER(C.c_uint32),
                                                                                     C.POINTER(C.c_uint32)]
            lib.hs_pssm_weight_hits.restype = C.c_int
            lib.hs_pssm_weight_hits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64] + [
                                                    C.c_void_p] * 5
            lib.hs_pssm_log_odds_weighted.restype = C.c_int
            lib.hs_pssm_log_odds_weighted.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32,
                                                      C.c_uint32, C.c_void_p, C.c_double, C.c_void_p]
            lib.hs_pssm_weight_u.restype = C.c_uint64
            lib.hs_pssm_weight_u.argtypes = [C.c_uint32, C.c_uint32]
        # clusters to profiles: weighted_profile (h, label, min_size, out_label, out_size, counts, wcounts, wsum,
        # distinct, cap, n_out); pssm_cover (h, label, min_size, S, n_rows, min_score, argmin); the host rules (codes, n,
        # k, alphabet, label, min_size, ...)
        if hasattr(lib, "hs_cluster_weighted_profile"):
            for fn in (lib.hs_cluster_weighted_profile, lib.hs_cluster_weighted_profile_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32] + [C.c_void_p] * 6 + [C.c_uint64,
                                                                                        C.POINTER(C.c_uint64)]
            for fn in (lib.hs_cluster_pssm_cover, lib.hs_cluster_pssm_cover_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
            head = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]
            lib.hs_cluster_weights_codes.restype = C.c_int
            lib.hs_cluster_weights_codes.argtypes = head + [C.c_void_p] * 6 + [C.c_uint64, C.POINTER(C.c_uint64)]
            lib.hs_cluster_cover_codes.restype = C.c_int
            lib.hs_cluster_cover_codes.argtypes = head + [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        # PSSM p-values: (h, S, bg, t_lo, nm, hit_m, hit_score, n, p_hi, p_lo); (h, S, bg, t_lo, p, nm, t_p, p_hi, p_lo,
        # flag); the host forms: include/hsearch.h
        if hasattr(lib, "hs_pssm_pvalue"):
            for fn in (lib.hs_pssm_pvalue, lib.hs_pssm_pvalue_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                               C.c_uint64, C.c_void_p, C.c_void_p]
            for fn in (lib.hs_pssm_pvalue_threshold, lib.hs_pssm_pvalue_threshold_dev):
                fn.restype = C.c_int
                fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p,
                               C.c_void_p, C.c_void_p, C.c_void_p]
            head = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
            lib.hs_pssm_null_tables.restype = C.c_int
            lib.hs_pssm_null_tables.argtypes = head + [C.c_void_p] * 6
            lib.hs_pssm_pvalue_host.restype = C.c_int
            lib.hs_pssm_pvalue_host.argtypes = head + [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
            lib.hs_pssm_threshold_host.restype = C.c_int
            lib.hs_pssm_threshold_host.argtypes = head + [C.c_void_p] * 5
        _libs[hooks] = lib
    return _libs[hooks]


def alphabet():
    return _ALPHABET


def codes_from_letters(seqs):
    """['ARND...', ...] (equal lengths, letters of the 20-letter alphabet) -> uint8 [n][k]."""
    lut = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(_ALPHABET):
        lut[ord(ch)] = i
    arr = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    codes = lut[arr].reshape(len(seqs), -1)
    if (codes == 255).any():
        raise ValueError("letter outside ARNDCQEGHILKMFPSTWYV")
    return codes


def key_string(buckets):
    b = np.ascontiguousarray(buckets, dtype=np.int32)
    buf = C.create_string_buffer(12 * len(b) + 1)
    load().hs_key_string(b.ctypes.data_as(C.c_void_p), C.c_uint32(len(b)), buf, C.c_uint32(len(buf)))
    return buf.value.decode()


def key_fingerprint(buckets, seed=0):
    b = np.ascontiguousarray(buckets, dtype=np.int32)
    return int(load().hs_key_fingerprint(b.ctypes.data_as(C.c_void_p), C.c_uint32(len(b)),
                                         C.c_uint32(seed)))


def key_strings_equal(x, y):
    x = np.ascontiguousarray(x, dtype=np.int32)
    y = np.ascontiguousarray(y, dtype=np.int32)
    assert len(x) == len(y)
    return bool(load().hs_key_strings_equal(x.ctypes.data_as(C.c_void_p),
                                            y.ctypes.data_as(C.c_void_p), C.c_uint32(len(x))))


def _vp(arr):
    return arr.ctypes.data_as(C.c_void_p)


def merge_best(id, q, table, dist, cap=None):
    """hs_merge_best (host only, no GPU): of n tuples in any order, per distinct id the one smallest under
    (dist, table, q), rows in ascending id -- the rule of Engine.annotate, for merging several annotations or
    reducing a raw hit list.  cap=None: as many rows as needed; a given cap that is too small raises
    HsError(HS_ERR_CAPACITY) with the required size in .needed."""
    id = np.ascontiguousarray(id, dtype=np.uint32)
    q = np.ascontiguousarray(q, dtype=np.uint32)
    table = np.ascontiguousarray(table, dtype=np.uint32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    n = len(id)
    assert id.shape == q.shape == table.shape == dist.shape == (n,)
    room = n if cap is None else int(cap)
    oid = np.empty(room, dtype=np.uint32)
    oq = np.empty(room, dtype=np.uint32)
    ot = np.empty(room, dtype=np.uint32)
    od = np.empty(room, dtype=np.float64)
    n_out = C.c_uint64(0)
    st = load().hs_merge_best(_vp(id), _vp(q), _vp(table), _vp(dist), n, _vp(oid), _vp(oq), _vp(ot), _vp(od), room,
                              C.byref(n_out))
    if st != HS_OK:
        e = HsError(st, "hs_merge_best")
        e.needed = int(n_out.value)
        raise e
    m = int(n_out.value)
    return dict(id=oid[:m], q=oq[:m], table=ot[:m], dist=od[:m])


def topk_merge(q, id, table, dist, nq, topk, out=None):
    """hs_topk_merge (host only, no GPU): of tuples (q, id, table, dist) in any order, per q the topk smallest under
    (dist, id) -- the rule of Engine.query_topk / Engine.self_knn, for reducing a raw hit list or merging the rows of
    the parts of a partition (flatten them: q = np.repeat(np.arange(nq), topk)).  Tuples with id == capi.NO_ID are
    skipped; a (q, id) given several times counts once with its smallest table.  dict(id, table, dist [nq][topk],
    count [nq]); count is the number of distinct ids given for q -- over rows already cut at topk only a lower bound of
    the hit count.  table=None: no tables are known, the rows' tables are all capi.NO_ID.  out: such a dict to write
    into (it stays untouched when the input is invalid)."""
    q = np.ascontiguousarray(q, dtype=np.uint32).ravel()
    id = np.ascontiguousarray(id, dtype=np.uint32).ravel()
    if table is not None:
        table = np.ascontiguousarray(table, dtype=np.uint32).ravel()
    dist = np.ascontiguousarray(dist, dtype=np.float64).ravel()
    n = len(q)
    assert id.shape == dist.shape == (n,) and (table is None or table.shape == (n,))
    nq, topk = int(nq), int(topk)
    rows = max(0, min(topk, TOPK_MAX))  # (an invalid topk is the library's to refuse)
    if out is None:
        out = dict(id=np.empty((nq, rows), dtype=np.uint32), table=np.empty((nq, rows), dtype=np.uint32),
                   dist=np.empty((nq, rows), dtype=np.float64), count=np.empty(nq, dtype=np.uint32))
    st = load().hs_topk_merge(_vp(q), _vp(id), None if table is None else _vp(table), _vp(dist), n, nq, topk, _vp(out["id"]), _vp(out["table"]),
                              _vp(out["dist"]), _vp(out["count"]))
    if st != HS_OK:
        raise HsError(st, "hs_topk_merge")
    return out


SEQ_MATCH_FIELDS = (("group", np.uint32), ("seq", np.uint32), ("diag", np.int32), ("count", np.uint32),
                    ("best_dist", np.float64), ("best_q", np.uint32), ("best_id", np.uint32), ("lo", np.uint32),
                    ("hi", np.uint32))


def _seq_rows(cap):
    return [np.empty(cap, dtype=t) for _, t in SEQ_MATCH_FIELDS]


def _seq_dict(arrs, m):
    return {name: a[:m] for (name, _), a in zip(SEQ_MATCH_FIELDS, arrs)}


def _seq_keys(nq, q_group, n_groups, q_off, id_start):
    """the three key arrays of seq_match as the library takes them, and (n_groups, n_seq)"""
    if q_group is not None:
        q_group = np.ascontiguousarray(q_group, dtype=np.uint32)
        assert q_group.shape == (nq,) and n_groups is not None, "q_group [nq] comes with n_groups"
    if q_off is not None:
        q_off = np.ascontiguousarray(q_off, dtype=np.uint32)
        assert q_off.shape == (nq,)
    id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
    assert id_start.ndim == 1 and len(id_start) >= 1
    return q_group, q_off, id_start, int(nq if n_groups is None else n_groups), len(id_start) - 1


def window_id_start(seq_start, k):
    """hs_window_id_start (host only): id_start [n_seq + 1] uint64 of an index built by Engine.index_build_windows over
    seq_start at k-mer length k -- sequence s owns the window ids [id_start[s], id_start[s + 1])."""
    seq_start = np.ascontiguousarray(seq_start, dtype=np.uint64)
    assert seq_start.ndim == 1 and len(seq_start) >= 1
    out = np.empty(len(seq_start), dtype=np.uint64)
    st = load().hs_window_id_start(_vp(seq_start), len(seq_start) - 1, int(k), _vp(out))
    if st != HS_OK:
        raise HsError(st, "hs_window_id_start")
    return out


def protein_queries(residues, seq_start, k):
    """Query proteins cut into windows on the host: residues uint8 codes, seq_start [n_prot + 1] ascending offsets ->
    dict(qcodes [nq][k] uint8, q_group [nq] = the protein, q_off [nq] = the window's offset in it), windows numbered
    protein-major as index_build_windows numbers a database's; proteins shorter than k contribute none.  What
    Engine.seq_match takes with codes=True, n_groups = n_prot."""
    residues = np.ascontiguousarray(residues, dtype=np.uint8)
    seq_start = np.ascontiguousarray(seq_start, dtype=np.int64)
    k = int(k)
    lens = np.diff(seq_start)
    nwin = np.maximum(lens - k + 1, 0)
    q_group = np.repeat(np.arange(len(nwin), dtype=np.uint32), nwin)
    first = np.concatenate([[0], np.cumsum(nwin)])[:-1]
    q_off = (np.arange(int(nwin.sum()), dtype=np.int64) - np.repeat(first, nwin)).astype(np.uint32)
    pos = np.repeat(seq_start[:-1], nwin) + q_off
    qcodes = residues[pos[:, None] + np.arange(k)[None, :]] if len(pos) else np.empty((0, k), dtype=np.uint8)
    return dict(qcodes=np.ascontiguousarray(qcodes, dtype=np.uint8), q_group=q_group, q_off=q_off)


def seq_match_hits(q, id, dist, nq, id_start, q_group=None, n_groups=None, q_off=None, cap=None, out=None):
    """hs_seq_match_hits (host only, no GPU): the rule of Engine.seq_match over ANY list of hits (q, id, dist) in any
    order -- one row per distinct (group, sequence, diagonal): dict(group, seq, diag, count, best_dist, best_q, best_id,
    lo, hi).  A (q, id) given twice counts once.  cap=None: as many rows as needed; a given cap that is too small
    raises HsError(HS_ERR_CAPACITY) with the required size in .needed.  out: a list of the nine arrays to write into."""
    q = np.ascontiguousarray(q, dtype=np.uint32).ravel()
    id = np.ascontiguousarray(id, dtype=np.uint32).ravel()
    dist = np.ascontiguousarray(dist, dtype=np.float64).ravel()
    n = len(q)
    assert id.shape == dist.shape == (n,)
    q_group, q_off, id_start, n_groups, n_seq = _seq_keys(int(nq), q_group, n_groups, q_off, id_start)
    room = n if cap is None else int(cap)
    arrs = _seq_rows(room) if out is None else out
    n_out = C.c_uint64(0)
    st = load().hs_seq_match_hits(_vp(q), _vp(id), _vp(dist), n, int(nq), None if q_group is None else _vp(q_group),
                                  n_groups, None if q_off is None else _vp(q_off), _vp(id_start), n_seq,
                                  *[_vp(a) for a in arrs], room, C.byref(n_out))
    if st != HS_OK:
        e = HsError(st, "hs_seq_match_hits")
        e.needed = int(n_out.value)
        raise e
    return _seq_dict(arrs, int(n_out.value))


def seq_match_merge(rows, cap=None, out=None):
    """hs_seq_match_merge (host only, no GPU): rows -- a dict as Engine.seq_match returns it, or a list of them that is
    concatenated -- with equal (group, seq, diag) combined: counts add, best is the min, lo the min, hi the max.  Only
    for parts whose hit lists are disjoint (query blocks, q and the groups made global first); parts that can report
    one (q, id) twice go through seq_match_hits."""
    if isinstance(rows, dict):
        rows = [rows]
    ins = [np.ascontiguousarray(np.concatenate([np.asarray(r[name], dtype=t) for r in rows]) if rows
                                else np.empty(0, dtype=t), dtype=t) for name, t in SEQ_MATCH_FIELDS]
    n = len(ins[0])
    assert all(a.shape == (n,) for a in ins)
    room = n if cap is None else int(cap)
    arrs = _seq_rows(room) if out is None else out
    n_out = C.c_uint64(0)
    st = load().hs_seq_match_merge(*[_vp(a) for a in ins], n, *[_vp(a) for a in arrs], room, C.byref(n_out))
    if st != HS_OK:
        e = HsError(st, "hs_seq_match_merge")
        e.needed = int(n_out.value)
        raise e
    return _seq_dict(arrs, int(n_out.value))


def components_merge(labels, out=None):
    """hs_components_merge (host only, no GPU): labels [m][n] uint32, m label arrays over the same n vertices as
    Engine.components returns them (one per range of a partition, in any order) -> dict(label, n_components) of the
    union of the m forests.  out: a uint32 [n] array to write into (it stays untouched when the input is invalid)."""
    labels = np.ascontiguousarray(labels, dtype=np.uint32)
    assert labels.ndim == 2
    m, n = labels.shape
    if out is None:
        out = np.empty(n, dtype=np.uint32)
    assert out.dtype == np.uint32 and out.shape == (n,) and out.flags["C_CONTIGUOUS"]
    nc = C.c_uint64(0)
    st = load().hs_components_merge(_vp(labels), m, n, _vp(out), C.byref(nc))
    if st != HS_OK:
        raise HsError(st, "hs_components_merge")
    return dict(label=out, n_components=int(nc.value))


def _counts_dict(c):
    return {f[0]: int(getattr(c, f[0])) for f in _DbscanCounts._fields_}


def dbscan_edges(ei, ej, n, min_pts, want_degree=False):
    """hs_dbscan_edges (host only, no GPU): the rule of Engine.dbscan applied to any list of pairs (ei[t], ej[t]) over
    n vertices -- either or both directions, repeated, in any order, self pairs ignored -> dict(label uint32 [n] with
    NOISE for noise, degree if asked, n_clusters, n_core, n_border, n_noise, n_edges = the sum of the degrees)."""
    ei = np.ascontiguousarray(ei, dtype=np.uint32)
    ej = np.ascontiguousarray(ej, dtype=np.uint32)
    assert ei.ndim == 1 and ei.shape == ej.shape
    n = int(n)
    label = np.empty(n, dtype=np.uint32)
    degree = np.empty(n, dtype=np.uint32) if want_degree else None
    c = _DbscanCounts()
    st = load().hs_dbscan_edges(_vp(ei), _vp(ej), len(ei), n, int(min_pts), _vp(label),
                                _vp(degree) if want_degree else None, C.byref(c))
    if st != HS_OK:
        raise HsError(st, "hs_dbscan_edges")
    res = dict(label=label, **_counts_dict(c))
    if want_degree:
        res["degree"] = degree
    return res


def _msf_dict(info, lo, hi, dist, label):
    m = int(info.n_tree_edges)
    res = dict(lo=lo[:m], hi=hi[:m], dist=dist[:m], **{f[0]: int(getattr(info, f[0])) for f in _MsfInfo._fields_})
    if label is not None:
        res["label"] = label
    return res


def msf_edges(ei, ej, dist, n, want_label=False, cap=None):
    """hs_msf_edges (host only, no GPU): the minimum spanning forest, under the order (dist, lo, hi), of any list of
    weighted pairs (ei[t], ej[t], dist[t]) over n vertices -- either or both directions, repeated, in any order, self
    pairs ignored -> dict(lo, hi, dist: the tree edges in ascending (dist, lo, hi) with lo < hi; label if asked;
    n_tree_edges, n_components, n_graph_edges = twice the distinct pairs, rounds = resident = 0).  The forest of the
    concatenation of several forests is the forest of the union of their graphs (the merge of ranks' results).
    cap=None: room for every result; a given cap that is too small raises HsError(HS_ERR_CAPACITY) with .needed."""
    ei = np.ascontiguousarray(ei, dtype=np.uint32)
    ej = np.ascontiguousarray(ej, dtype=np.uint32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    assert ei.ndim == 1 and ei.shape == ej.shape == dist.shape
    n = int(n)
    room = n if cap is None else int(cap)
    lo = np.empty(room, dtype=np.uint32)
    hi = np.empty(room, dtype=np.uint32)
    od = np.empty(room, dtype=np.float64)
    label = np.empty(n, dtype=np.uint32) if want_label else None
    info = _MsfInfo()
    st = load().hs_msf_edges(_vp(ei), _vp(ej), _vp(dist), len(ei), n, _vp(lo), _vp(hi), _vp(od), room,
                             _vp(label) if want_label else None, C.byref(info))
    if st != HS_OK:
        e = HsError(st, "hs_msf_edges")
        e.needed = int(info.n_tree_edges)
        raise e
    return _msf_dict(info, lo, hi, od, label)


def msf_cut(tree, r, n=None, out=None):
    """hs_msf_cut (host only, no GPU): tree = a dict with lo, hi, dist as Engine.msf / msf_edges return them (n from its
    label, or given) -> dict(label uint32 [n] = the smallest id per component of the forest of the tree edges with
    dist <= r, n_components).  out: a uint32 [n] array to write into (untouched when the input is invalid)."""
    lo = np.ascontiguousarray(tree["lo"], dtype=np.uint32)
    hi = np.ascontiguousarray(tree["hi"], dtype=np.uint32)
    dist = np.ascontiguousarray(tree["dist"], dtype=np.float64)
    assert lo.ndim == 1 and lo.shape == hi.shape == dist.shape
    n = len(tree["label"]) if n is None else int(n)
    if out is None:
        out = np.empty(n, dtype=np.uint32)
    assert out.dtype == np.uint32 and out.shape == (n,) and out.flags["C_CONTIGUOUS"]
    nc = C.c_uint64(0)
    st = load().hs_msf_cut(_vp(lo), _vp(hi), _vp(dist), len(lo), n, float(r), _vp(out), C.byref(nc))
    if st != HS_OK:
        raise HsError(st, "hs_msf_cut")
    return dict(label=out, n_components=int(nc.value))


def _density_dict(info, lo, hi, w, label, core):
    m = int(info.n_tree_edges)
    res = dict(lo=lo[:m], hi=hi[:m], w=w[:m], **{f[0]: int(getattr(info, f[0])) for f in _DensityInfo._fields_})
    if label is not None:
        res["label"] = label
    if core is not None:
        res["core"] = core
    return res


def density_tree_edges(ei, ej, dist, n, min_pts, want_label=True, cap=None):
    """hs_density_tree_edges (host only, no GPU): the density tree -- the minimum spanning forest under (w, lo, hi),
    w = max(core[a], core[b], dist) -- of any list of weighted pairs over n vertices, presented as msf_edges accepts
    them -> dict(lo, hi, w: the n_core - n_clusters tree edges in ascending (w, lo, hi); core float64 [n] (inf: fewer
    than min_pts - 1 neighbours); label if asked (NOISE where core is inf); n_tree_edges, n_clusters, n_core,
    n_graph_edges, rounds = resident = self_joins = 0).  cap as in msf_edges."""
    ei = np.ascontiguousarray(ei, dtype=np.uint32)
    ej = np.ascontiguousarray(ej, dtype=np.uint32)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    assert ei.ndim == 1 and ei.shape == ej.shape == dist.shape
    n = int(n)
    room = n if cap is None else int(cap)
    lo = np.empty(room, dtype=np.uint32)
    hi = np.empty(room, dtype=np.uint32)
    w = np.empty(room, dtype=np.float64)
    label = np.empty(n, dtype=np.uint32) if want_label else None
    core = np.empty(n, dtype=np.float64)
    info = _DensityInfo()
    st = load().hs_density_tree_edges(_vp(ei), _vp(ej), _vp(dist), len(ei), n, int(min_pts), _vp(lo), _vp(hi), _vp(w),
                                      room, _vp(label) if want_label else None, _vp(core), C.byref(info))
    if st != HS_OK:
        e = HsError(st, "hs_density_tree_edges")
        e.needed = int(info.n_tree_edges)
        raise e
    return _density_dict(info, lo, hi, w, label, core)


def density_tree_cut(tree, r, n=None, out=None):
    """hs_density_tree_cut (host only, no GPU): tree = a dict with lo, hi, w, core as Engine.density_tree /
    density_tree_edges return them -> dict(label uint32 [n]: NOISE where core > r or core is inf, else the smallest id per component
    of the tree edges with w <= r; n_clusters).  out: a uint32 [n] array to write into (untouched when the input is
    invalid)."""
    lo = np.ascontiguousarray(tree["lo"], dtype=np.uint32)
    hi = np.ascontiguousarray(tree["hi"], dtype=np.uint32)
    w = np.ascontiguousarray(tree["w"], dtype=np.float64)
    core = np.ascontiguousarray(tree["core"], dtype=np.float64)
    assert lo.ndim == 1 and lo.shape == hi.shape == w.shape and core.ndim == 1
    n = len(core) if n is None else int(n)
    assert len(core) == n
    if out is None:
        out = np.empty(n, dtype=np.uint32)
    assert out.dtype == np.uint32 and out.shape == (n,) and out.flags["C_CONTIGUOUS"]
    nc = C.c_uint64(0)
    st = load().hs_density_tree_cut(_vp(lo), _vp(hi), _vp(w), len(lo), _vp(core), n, float(r), _vp(out), C.byref(nc))
    if st != HS_OK:
        raise HsError(st, "hs_density_tree_cut")
    return dict(label=out, n_clusters=int(nc.value))


def cluster_summary_codes(codes, label, min_size=1, coords=None, centers=None, want_counts=False, want_radii=True,
                          cap=None):
    """hs_cluster_summary_codes (host only, no GPU): the rules of Engine.cluster_profile and Engine.cluster_radii for
    codes uint8 [n][k], label uint32 [n] (NOISE or a value < n) and coords [alphabet][8] (None: the default table)
    -> dict(label, size, centroid [rows][8k], counts [rows][k][alphabet] if asked, and with want_radii max_d2, radius,
    medoid -- against centers [rows][8k], or against the centroids when centers is None).  Rows: the clusters of at
    least min_size members in ascending label.  cap=None: as many rows as needed; a given cap that is too small
    raises HsError(HS_ERR_CAPACITY) with the required size in .needed."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    label = np.ascontiguousarray(label, dtype=np.uint32)
    assert codes.ndim == 2 and label.shape == (codes.shape[0],)
    n, k = codes.shape
    alpha = 20
    if coords is not None:
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        assert coords.ndim == 2 and coords.shape[1] == 8
        alpha = coords.shape[0]
    room = n // max(1, int(min_size)) if cap is None else int(cap)
    if centers is not None:
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        assert centers.ndim == 2 and centers.shape[1] == 8 * k
    ol = np.empty(room, dtype=np.uint32)
    osz = np.empty(room, dtype=np.uint32)
    cen = np.empty((room, 8 * k), dtype=np.float64)
    cnt = np.empty((room, k, alpha), dtype=np.uint32) if want_counts else None
    mx = np.empty(room, dtype=np.float64) if want_radii else None
    rad = np.empty(room, dtype=np.float64) if want_radii else None
    med = np.empty(room, dtype=np.uint32) if want_radii else None
    n_out = C.c_uint64(0)
    opt = lambda a: None if a is None else _vp(a)
    st = load().hs_cluster_summary_codes(_vp(codes), n, k, opt(coords), alpha if coords is not None else 0, _vp(label),
                                         int(min_size), opt(centers), 0 if centers is None else centers.shape[0],
                                         _vp(ol), _vp(osz), opt(cnt), _vp(cen), opt(mx), opt(rad), opt(med), room,
                                         C.byref(n_out))
    if st != HS_OK:
        e = HsError(st, "hs_cluster_summary_codes")
        e.needed = int(n_out.value)
        raise e
    m = int(n_out.value)
    res = dict(label=ol[:m], size=osz[:m], centroid=cen[:m])
    if want_counts:
        res["counts"] = cnt[:m]
    if want_radii:
        res.update(max_d2=mx[:m], radius=rad[:m], medoid=med[:m])
    return res


def join6_tables(coords):
    """The FP6 join filter's tables for a coordinate table ([alphabet][8] doubles), computed on the host (no GPU):
    dict(s, codes [alphabet][4] six-bit e2m3 codes, e [alphabet], r [alphabet], pair [1024][2] dwords)."""
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    A = coords.shape[0]
    s = C.c_double(0.0)
    codes = np.zeros((32, 4), dtype=np.uint8)
    e, r = np.zeros(32), np.zeros(32)
    pair = np.zeros((1024, 2), dtype=np.uint32)
    lib = load()
    st = lib.hs_join6_tables(_vp(coords), C.c_uint32(A), C.byref(s), _vp(codes), _vp(e), _vp(r), _vp(pair))
    if st:
        raise HsError(st, "hs_join6_tables")
    return dict(s=s.value, codes=codes[:A], e=e[:A], r=r[:A], pair=pair)


def join6_thresholds(coords, kmers, r2):
    """What the FP6 join carries for k-mers ([n][k] codes) at squared radii r2 [n], in units of 2^-6, on the host:
    dict(rho64 [n] a member's rho as its record encodes it, c64 [n] a query's C operand, rho0_64, rec [n][4])."""
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    kmers = np.ascontiguousarray(kmers, dtype=np.uint8)
    n, k = kmers.shape
    r2 = np.ascontiguousarray(np.broadcast_to(np.asarray(r2, dtype=np.float64), (n,)))
    rho64, c64 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    rho0 = C.c_int64(0)
    rec = np.zeros((n, 4), dtype=np.uint32)
    st = load().hs_join6_thresholds(_vp(coords), C.c_uint32(coords.shape[0]), _vp(kmers), C.c_uint64(n), C.c_uint32(k),
                                    _vp(r2), _vp(rho64), _vp(c64), C.byref(rho0), _vp(rec))
    if st:
        raise HsError(st, "hs_join6_thresholds")
    return dict(rho64=rho64, c64=c64, rho0_64=rho0.value, rec=rec)


def pssm_tables(S, t):
    """The PSSM scan filter's tables for profiles S [nm][k][alphabet] and thresholds t [nm], computed on the host (no
    GPU; hs_pssm_tables): dict(code uint8 [nm][k][alphabet] six-bit e2m3 codes, tau [nm] on the 1/8 grid (-inf: the
    profile passes every k-mer, +inf: dead), dead uint8 [nm]).  For every k-mer x whose rounded fp64 score reaches
    t[m], the sum over p of E2M3[code[m][p][x_p]] is >= tau[m]."""
    S = np.ascontiguousarray(S, dtype=np.float64)
    t = np.ascontiguousarray(t, dtype=np.float64)
    assert S.ndim == 3 and t.shape == (S.shape[0],), (S.shape, t.shape)
    nm, k, A = S.shape
    code = np.zeros((nm, k, A), dtype=np.uint8)
    tau = np.zeros(nm)
    dead = np.zeros(nm, dtype=np.uint8)
    st = load().hs_pssm_tables(_vp(S), _vp(t), C.c_uint64(nm), C.c_uint32(k), C.c_uint32(A), _vp(code), _vp(tau),
                               _vp(dead))
    if st:
        raise HsError(st, "hs_pssm_tables")
    return dict(code=code, tau=tau, dead=dead)


def _pssm_compare_args(X, t, Y):
    X = np.ascontiguousarray(X, dtype=np.float64)
    assert X.ndim == 3, X.shape
    nx, k, A = X.shape
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(t, dtype=np.float64), (nx,)))
    if Y is not None:
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        assert Y.ndim == 3 and Y.shape[1:] == (k, A), (X.shape, Y.shape)
    return X, t, Y, nx, (Y.shape[0] if Y is not None else 0), k, A


def _pssm_compare_call(call, nx, cap, want_counts):
    """The capacity retry of the comparing calls: call(hx, hy, hd, hs, cap, &n, cnt) -> status"""
    cap = int(cap) if cap is not None else max(1024, 16 * nx)
    cnt = np.zeros(nx, dtype=np.uint64) if want_counts else None
    while True:
        hx = np.empty(cap, dtype=np.uint32)
        hy = np.empty(cap, dtype=np.uint32)
        hd = np.empty(cap, dtype=np.int32)
        hs = np.empty(cap, dtype=np.float64)
        n = C.c_uint64(0)
        st = call(_vp(hx), _vp(hy), _vp(hd), _vp(hs), C.c_uint64(cap), C.byref(n), _vp(cnt) if want_counts else None)
        if st == HS_ERR_CAPACITY:
            cap = int(n.value)
            continue
        if st != HS_OK:
            return st, None
        n = int(n.value)
        res = dict(x=hx[:n], y=hy[:n], d=hd[:n], score=hs[:n])
        if want_counts:
            res["cnt"] = cnt
        return st, res


def pssm_compare_host(X, t, Y=None, min_overlap=1, cap=None, want_counts=True):
    """hs_pssm_compare_host: the rule of Engine.pssm_compare on one CPU thread (no GPU, no handle).  X [nx][k][alphabet],
    t a scalar or [nx], Y [ny][k][alphabet] or None (X against itself, pairs x < y).  dict(x, y, d, score[, cnt])."""
    X, t, Y, nx, ny, k, A = _pssm_compare_args(X, t, Y)
    lib = load()
    st, res = _pssm_compare_call(
        lambda hx, hy, hd, hs, c, n, cnt: lib.hs_pssm_compare_host(
            _vp(X), C.c_uint64(nx), _vp(Y) if Y is not None else None, C.c_uint64(ny), C.c_uint32(k), C.c_uint32(A),
            _vp(t), C.c_uint32(min_overlap), hx, hy, hd, hs, c, n, cnt), nx, cap, want_counts)
    if st != HS_OK:
        raise HsError(st, "hs_pssm_compare_host refused its arguments")
    return res


def pssm_compare_tables(X):
    """hs_pssm_compare_tables: the int8 filter's tables of the profiles X [nx][k][alphabet], the bits the device builds:
    dict(q [nx][k][alphabet] int8, s [nx], l1 [nx], amax [nx])."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    nx, k, A = X.shape
    q = np.zeros((nx, k, A), dtype=np.int8)
    s = np.zeros(nx, dtype=np.float64)
    l1 = np.zeros(nx, dtype=np.float64)
    amax = np.zeros(nx, dtype=np.float64)
    st = load().hs_pssm_compare_tables(_vp(X), C.c_uint64(nx), C.c_uint32(k), C.c_uint32(A), _vp(q), _vp(s), _vp(l1),
                                       _vp(amax))
    if st != HS_OK:
        raise HsError(st, "hs_pssm_compare_tables refused its arguments")
    return dict(q=q, s=s, l1=l1, amax=amax)


def pssm_compare_pass(I, s_x, l1_x, amax_x, s_y, l1_y, k, alphabet, t):
    """hs_pssm_compare_pass: the filter's test on one pair at the largest integer sum I over the allowed offsets."""
    return bool(load().hs_pssm_compare_pass(int(I), float(s_x), float(l1_x), float(amax_x), float(s_y), float(l1_y),
                                            int(k), int(alphabet), float(t)))


def pssm_compare_columns(X, mode="pearson"):
    """hs_pssm_compare_columns: the column transform applied before comparing.  mode "pearson" (0): every column
    centred on its mean and divided by its Euclidean norm; "cosine" (1): divided by the norm only."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    nm, k, A = X.shape
    mode = {"pearson": 0, "cosine": 1}.get(mode, mode)
    out = np.empty_like(X)
    st = load().hs_pssm_compare_columns(_vp(X), C.c_uint64(nm), C.c_uint32(k), C.c_uint32(A), C.c_int(int(mode)), _vp(out))
    if st != HS_OK:
        raise HsError(st, "hs_pssm_compare_columns refused its arguments")
    return out


def pssm_topk_hits(m, id, score, nm, topk):
    """hs_pssm_topk's rule on the host for any list of (m, id, score) tuples (hs_pssm_topk_hits; no GPU): dict(id
    uint32 [nm][topk] padded with NO_ID, score [nm][topk] padded with -inf, count uint32 [nm]).  Tuples with id == NO_ID
    are skipped; a repeated (m, id) counts once if its score bits agree, else HsError."""
    m = np.ascontiguousarray(m, dtype=np.uint32)
    id = np.ascontiguousarray(id, dtype=np.uint32)
    score = np.ascontiguousarray(score, dtype=np.float64)
    assert m.ndim == 1 and m.shape == id.shape == score.shape, (m.shape, id.shape, score.shape)
    rows = max(int(nm), 0) if 1 <= int(topk) <= TOPK_MAX else 0
    tid = np.empty((rows, max(int(topk), 1)), dtype=np.uint32)
    ts = np.empty((rows, max(int(topk), 1)), dtype=np.float64)
    tc = np.empty(max(rows, 1), dtype=np.uint32)
    st = load().hs_pssm_topk_hits(_vp(m), _vp(id), _vp(score), C.c_uint64(len(m)), C.c_uint64(int(nm)),
                                  C.c_uint32(int(topk)), _vp(tid), _vp(ts), _vp(tc))
    if st:
        raise HsError(st, "hs_pssm_topk_hits")
    return dict(id=tid, score=ts, count=tc[:rows])


PSSM_SEQ_FIELDS = (("m", np.uint32), ("seq", np.uint32), ("count", np.uint32), ("best_score", np.float64),
                   ("best_id", np.uint32), ("lo", np.uint32), ("hi", np.uint32))


def _pssm_seq_rows(cap):
    return [np.empty(cap, dtype=t) for _, t in PSSM_SEQ_FIELDS]


def _pssm_seq_dict(arrs, n):
    return {name: a[:n] for (name, _), a in zip(PSSM_SEQ_FIELDS, arrs)}


def pssm_seq_hits(m, id, score, nm, id_start, cap=None, out=None):
    """hs_pssm_seq_hits (host only, no GPU): the rule of Engine.pssm_seq_scan over ANY list of hits (m, id, score) in
    any order -- one row per distinct (profile, sequence): dict(m, seq, count, best_score, best_id, lo, hi).  A (m, id)
    given twice with one score counts once.  cap=None: as many rows as needed; a given cap that is too small raises
    HsError(HS_ERR_CAPACITY) with the required size in .needed.  out: a list of the seven arrays to write into."""
    m = np.ascontiguousarray(m, dtype=np.uint32).ravel()
    id = np.ascontiguousarray(id, dtype=np.uint32).ravel()
    score = np.ascontiguousarray(score, dtype=np.float64).ravel()
    n = len(m)
    assert id.shape == score.shape == (n,)
    if id_start is not None:
        id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
        assert id_start.ndim == 1 and len(id_start) >= 1
    room = n if cap is None else int(cap)
    arrs = _pssm_seq_rows(room) if out is None else out
    n_out = C.c_uint64(0)
    st = load().hs_pssm_seq_hits(_vp(m), _vp(id), _vp(score), n, int(nm), None if id_start is None else _vp(id_start),
                                 0 if id_start is None else len(id_start) - 1, *[_vp(a) for a in arrs], room,
                                 C.byref(n_out))
    if st != HS_OK:
        e = HsError(st, "hs_pssm_seq_hits")
        e.needed = int(n_out.value)
        raise e
    return _pssm_seq_dict(arrs, int(n_out.value))


PSSM_FAMILY_FIELDS = (("group", np.uint32), ("seq", np.uint32), ("diag", np.int32), ("count", np.uint32),
                      ("sum", np.float64), ("best_score", np.float64), ("best_m", np.uint32), ("best_id", np.uint32),
                      ("lo", np.uint32), ("hi", np.uint32))


def _pssm_family_rows(cap):
    return [np.empty(cap, dtype=t) for _, t in PSSM_FAMILY_FIELDS]


def _pssm_family_dict(arrs, n):
    return {name: a[:n] for (name, _), a in zip(PSSM_FAMILY_FIELDS, arrs)}


def _pssm_family_args(nm, m_group, n_groups, m_off, id_start, min_count, t_group):
    """the family arguments as contiguous arrays (None stays None) and their ctypes values, in the C order"""
    if m_group is not None:
        m_group = np.ascontiguousarray(m_group, dtype=np.uint32)
        assert m_group.shape == (nm,), m_group.shape
    if n_groups is None:
        n_groups = nm if m_group is None else (int(m_group.max()) + 1 if nm else 0)
    if m_off is not None:
        m_off = np.ascontiguousarray(m_off, dtype=np.uint32)
        assert m_off.shape == (nm,), m_off.shape
    if id_start is not None:
        id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
        assert id_start.ndim == 1 and len(id_start) >= 1
    if t_group is not None:
        t_group = np.ascontiguousarray(t_group, dtype=np.float64)
        assert t_group.shape == (int(n_groups),), t_group.shape
    keep = (m_group, m_off, id_start, t_group)
    vals = [None if m_group is None else _vp(m_group), int(n_groups), None if m_off is None else _vp(m_off),
            None if id_start is None else _vp(id_start), 0 if id_start is None else len(id_start) - 1,
            C.c_uint32(int(min_count)), None if t_group is None else _vp(t_group)]
    return keep, vals, int(n_groups)


def pssm_family_hits(m, id, score, nm, id_start, m_group=None, n_groups=None, m_off=None, min_count=1, t_group=None,
                     cap=None, out=None):
    """hs_pssm_family_hits (host only, no GPU): the rule of Engine.pssm_family_scan over ANY list of hits (m, id,
    score) in any order -- one row per distinct (family, sequence, diagonal) that passes the filters: dict(group, seq,
    diag, count, sum, best_score, best_m, best_id, lo, hi).  A (m, id) given twice with one score counts once.
    n_groups=None: nm without m_group, else its largest value + 1.  cap=None: as many rows as needed; a given cap that
    is too small raises HsError(HS_ERR_CAPACITY) with the required size in .needed.  out: a list of the ten arrays."""
    m = np.ascontiguousarray(m, dtype=np.uint32).ravel()
    id = np.ascontiguousarray(id, dtype=np.uint32).ravel()
    score = np.ascontiguousarray(score, dtype=np.float64).ravel()
    n = len(m)
    assert id.shape == score.shape == (n,)
    keep, vals, _ = _pssm_family_args(int(nm), m_group, n_groups, m_off, id_start, min_count, t_group)
    room = n if cap is None else int(cap)
    arrs = _pssm_family_rows(room) if out is None else out
    n_out = C.c_uint64(0)
    st = load().hs_pssm_family_hits(_vp(m), _vp(id), _vp(score), n, int(nm), *vals, *[_vp(a) for a in arrs], room,
                                    C.byref(n_out))
    if st != HS_OK:
        e = HsError(st, "hs_pssm_family_hits")
        e.needed = int(n_out.value)
        raise e
    return _pssm_family_dict(arrs, int(n_out.value))


PSSM_CHAIN_FIELDS = (("group", np.uint32), ("seq", np.uint32), ("count", np.uint32), ("gaps", np.uint32),
                     ("score", np.float64), ("first_m", np.uint32), ("first_id", np.uint32), ("last_m", np.uint32),
                     ("last_id", np.uint32), ("shift", np.int32))


def _pssm_chain_rows(cap):
    return [np.empty(cap, dtype=t) for _, t in PSSM_CHAIN_FIELDS]


def _pssm_chain_dict(arrs, n):
    return {name: a[:n] for (name, _), a in zip(PSSM_CHAIN_FIELDS, arrs)}


def _pssm_chain_vals(vals, max_shift, gap_open, gap_ext):
    """_pssm_family_args' values with the chain's three in front of min_count (the C order)"""
    return vals[:5] + [C.c_uint32(int(max_shift)), C.c_double(float(gap_open)), C.c_double(float(gap_ext))] + vals[5:]


def pssm_family_chain_hits(m, id, score, nm, id_start, m_group, m_off, max_shift, gap_open=0.0, gap_ext=0.0,
                           min_count=1, t_group=None, n_groups=None, cap=None, out=None, want_path=False,
                           path_cap=None):
    """hs_pssm_family_chain_hits (host only, no GPU): the rule of Engine.pssm_family_chain over ANY list of hits (m,
    id, score) in any order -- per (family, sequence) the best gapped chain that passes the filters: dict(group, seq,
    count, gaps, score, first_m, first_id, last_m, last_id, shift).  want_path: also path_start [rows + 1], path_m,
    path_id, the chains' hits from first to last.  cap / path_cap=None: as much room as can be needed; a given one that
    is too small raises HsError(HS_ERR_CAPACITY) with the required sizes in .needed and .needed_path."""
    m = np.ascontiguousarray(m, dtype=np.uint32).ravel()
    id = np.ascontiguousarray(id, dtype=np.uint32).ravel()
    score = np.ascontiguousarray(score, dtype=np.float64).ravel()
    n = len(m)
    assert id.shape == score.shape == (n,)
    keep, vals, _ = _pssm_family_args(int(nm), m_group, n_groups, m_off, id_start, min_count, t_group)
    vals = _pssm_chain_vals(vals, max_shift, gap_open, gap_ext)
    room = n if cap is None else int(cap)
    arrs = _pssm_chain_rows(room) if out is None else out
    n_out, n_path = C.c_uint64(0), C.c_uint64(0)
    proom = (n if path_cap is None else int(path_cap)) if want_path else 0
    pstart = np.empty(room + 1, dtype=np.uint64) if want_path else None
    pm, pid = (np.empty(max(proom, 1), dtype=np.uint32) for _ in range(2)) if want_path else (None, None)
    st = load().hs_pssm_family_chain_hits(_vp(m), _vp(id), _vp(score), n, int(nm), *vals, *[_vp(a) for a in arrs], room,
                                          C.byref(n_out), _vp(pstart) if want_path else None,
                                          _vp(pm) if want_path else None, _vp(pid) if want_path else None, proom,
                                          C.byref(n_path) if want_path else None)
    if st != HS_OK:
        e = HsError(st, "hs_pssm_family_chain_hits")
        e.needed, e.needed_path = int(n_out.value), int(n_path.value)
        raise e
    res = _pssm_chain_dict(arrs, int(n_out.value))
    if want_path:
        res["path_start"] = pstart[:int(n_out.value) + 1]
        res["path_m"], res["path_id"] = pm[:int(n_path.value)], pid[:int(n_path.value)]
    return res


def pssm_family_layout(hit_x, hit_y, hit_d, nm):
    """hs_pssm_family_layout (host only, no GPU): the hits (x, y, d) of Engine.pssm_compare's self mode, in their
    order, to families: dict(group uint32 [nm], off uint32 [nm], order uint32 [nm] -- the profiles sorted by (group,
    off, m), the order in which to pass them to pssm_family_scan --, n_groups, n_conflicts).  A hit says that profile y
    lies d columns to the right of profile x; one that disagrees with the positions fixed before it only counts."""
    x = np.ascontiguousarray(hit_x, dtype=np.uint32).ravel()
    y = np.ascontiguousarray(hit_y, dtype=np.uint32).ravel()
    d = np.ascontiguousarray(hit_d, dtype=np.int32).ravel()
    assert x.shape == y.shape == d.shape, (x.shape, y.shape, d.shape)
    nm = int(nm)
    group, off, order = (np.empty(max(nm, 1), dtype=np.uint32) for _ in range(3))
    ng, nc = C.c_uint64(0), C.c_uint64(0)
    st = load().hs_pssm_family_layout(_vp(x), _vp(y), _vp(d), len(x), nm, _vp(group), _vp(off), _vp(order),
                                      C.byref(ng), C.byref(nc))
    if st != HS_OK:
        raise HsError(st, "hs_pssm_family_layout refused its arguments")
    return dict(group=group[:nm], off=off[:nm], order=order[:nm], n_groups=int(ng.value), n_conflicts=int(nc.value))


def pssm_count_hits(codes, alphabet, m, id, score, nm, id_start=None):
    """hs_pssm_count_hits (host only, no GPU): the rule of Engine.pssm_hit_counts over ANY list of hits (m, id, score)
    in any order over codes [n][k]: dict(counts uint32 [nm][k][alphabet], used uint64 [nm]).  id_start=None: every
    distinct (m, id) is a site; else one site per (profile, sequence), the best hit of capi.pssm_seq_hits' rows."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    assert codes.ndim == 2
    n, k = codes.shape
    m = np.ascontiguousarray(m, dtype=np.uint32).ravel()
    id = np.ascontiguousarray(id, dtype=np.uint32).ravel()
    score = np.ascontiguousarray(score, dtype=np.float64).ravel()
    assert id.shape == score.shape == m.shape
    if id_start is not None:
        id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
        assert id_start.ndim == 1 and len(id_start) >= 1
    rows = max(int(nm), 0)
    counts = np.empty((rows, k, max(int(alphabet), 1)), dtype=np.uint32)
    used = np.empty(max(rows, 1), dtype=np.uint64)
    st = load().hs_pssm_count_hits(_vp(codes), n, k, int(alphabet), _vp(m), _vp(id), _vp(score), len(m), int(nm),
                                   None if id_start is None else _vp(id_start),
                                   0 if id_start is None else len(id_start) - 1, _vp(counts), _vp(used))
    if st:
        raise HsError(st, "hs_pssm_count_hits")
    return dict(counts=counts, used=used[:rows])


def cluster_weights_codes(codes, alphabet, label, min_size=1, want_counts=False, cap=None):
    """hs_cluster_weights_codes (host only, no GPU): the rule of Engine.cluster_weighted_profile for codes uint8 [n][k]
    over `alphabet` residues and label uint32 [n] (NOISE or a value < n) -> dict(label, size, wcounts uint64
    [rows][k][alphabet], wsum uint64 [rows], distinct uint32 [rows], counts uint32 [rows][k][alphabet] if asked).  Rows:
    the clusters of at least min_size members in ascending label.  cap=None: as many rows as needed; a given cap that
    is too small raises HsError(HS_ERR_CAPACITY) with the required size in .needed."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    label = np.ascontiguousarray(label, dtype=np.uint32)
    assert codes.ndim == 2 and label.shape == (codes.shape[0],)
    n, k = codes.shape
    A = max(int(alphabet), 1)
    room = n // max(1, int(min_size)) if cap is None else int(cap)
    ol, osz = np.empty(room, dtype=np.uint32), np.empty(room, dtype=np.uint32)
    wc = np.empty((room, k, A), dtype=np.uint64)
    ws, di = np.empty(room, dtype=np.uint64), np.empty(room, dtype=np.uint32)
    cnt = np.empty((room, k, A), dtype=np.uint32) if want_counts else None
    n_out = C.c_uint64(0)
    st = load().hs_cluster_weights_codes(_vp(codes), n, k, int(alphabet), _vp(label), int(min_size), _vp(ol), _vp(osz),
                                         None if cnt is None else _vp(cnt), _vp(wc), _vp(ws), _vp(di), room,
                                         C.byref(n_out))
    if st != HS_OK:
        e = HsError(st, "hs_cluster_weights_codes")
        e.needed = int(n_out.value)
        raise e
    m = int(n_out.value)
    res = dict(label=ol[:m], size=osz[:m], wcounts=wc[:m], wsum=ws[:m], distinct=di[:m])
    if want_counts:
        res["counts"] = cnt[:m]
    return res


def cluster_cover_codes(codes, alphabet, label, S, min_size=1):
    """hs_cluster_cover_codes (host only, no GPU): the rule of Engine.cluster_pssm_cover for codes uint8 [n][k], label
    uint32 [n] and profiles S [rows][k][alphabet], one per cluster of at least min_size members in ascending label ->
    dict(min_score float64 [rows], argmin uint32 [rows])."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    label = np.ascontiguousarray(label, dtype=np.uint32)
    S = np.ascontiguousarray(S, dtype=np.float64)
    assert codes.ndim == 2 and label.shape == (codes.shape[0],)
    n, k = codes.shape
    rows = S.shape[0]
    assert S.shape == (rows, k, int(alphabet)), S.shape
    ms, am = np.empty(rows, dtype=np.float64), np.empty(rows, dtype=np.uint32)
    st = load().hs_cluster_cover_codes(_vp(codes), n, k, int(alphabet), _vp(label), int(min_size), _vp(S), rows,
                                       _vp(ms), _vp(am))
    if st != HS_OK:
        raise HsError(st, "hs_cluster_cover_codes")
    return dict(min_score=ms, argmin=am)


def pssm_weight_hits(codes, alphabet, m, id, score, nm, id_start=None):
    """hs_pssm_weight_hits (host only, no GPU): the rule of Engine.pssm_weighted_counts over ANY list of hits (m, id,
    score) in any order over codes [n][k]: dict(counts uint32 [nm][k][alphabet], wcounts uint64 [nm][k][alphabet], wsum
    uint64 [nm], distinct uint32 [nm], used uint64 [nm]).  The sites are capi.pssm_count_hits'.  The merge of several
    GPUs' hit lists: weights do not merge from per-GPU wcounts."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    assert codes.ndim == 2
    n, k = codes.shape
    m = np.ascontiguousarray(m, dtype=np.uint32).ravel()
    id = np.ascontiguousarray(id, dtype=np.uint32).ravel()
    score = np.ascontiguousarray(score, dtype=np.float64).ravel()
    assert id.shape == score.shape == m.shape
    if id_start is not None:
        id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
        assert id_start.ndim == 1 and len(id_start) >= 1
    rows = max(int(nm), 0)
    shape = (rows, k, max(int(alphabet), 1))
    counts, wcounts = np.empty(shape, dtype=np.uint32), np.empty(shape, dtype=np.uint64)
    wsum, used = np.empty(max(rows, 1), dtype=np.uint64), np.empty(max(rows, 1), dtype=np.uint64)
    distinct = np.empty(max(rows, 1), dtype=np.uint32)
    st = load().hs_pssm_weight_hits(_vp(codes), n, k, int(alphabet), _vp(m), _vp(id), _vp(score), len(m), int(nm),
                                    None if id_start is None else _vp(id_start),
                                    0 if id_start is None else len(id_start) - 1, _vp(counts), _vp(wcounts),
                                    _vp(wsum), _vp(distinct), _vp(used))
    if st:
        raise HsError(st, "hs_pssm_weight_hits")
    return dict(counts=counts, wcounts=wcounts, wsum=wsum[:rows], distinct=distinct[:rows], used=used[:rows])


def pssm_weight_u(r, c):
    """hs_pssm_weight_u: floor(2^56 / (r * c)), 0 where r == 0 or c == 0."""
    return int(load().hs_pssm_weight_u(int(r), int(c)))


def pssm_log_odds_weighted(wcounts, wsum, n_eff, background, pseudo=1.0):
    """hs_pssm_log_odds_weighted (host only): S[m][p][a] = log2(((f * n_eff[m] + pseudo * bg[a]) / (n_eff[m] + pseudo))
    / bg[a]) with f = wcounts[m][p][a] / wsum[m] (0 where wsum[m] == 0), every operation rounded to fp64 -- the function
    Engine.pssm_refine_weighted applies, bit for bit."""
    wcounts = np.ascontiguousarray(wcounts, dtype=np.uint64)
    assert wcounts.ndim == 3
    nm, k, A = wcounts.shape
    wsum = np.ascontiguousarray(wsum, dtype=np.uint64)
    n_eff = np.ascontiguousarray(n_eff, dtype=np.float64)
    bg = np.ascontiguousarray(background, dtype=np.float64)
    assert wsum.shape == (nm,) and n_eff.shape == (nm,) and bg.shape == (A,), (wsum.shape, n_eff.shape, bg.shape)
    S = np.empty((nm, k, A), dtype=np.float64)
    st = load().hs_pssm_log_odds_weighted(_vp(wcounts), _vp(wsum), _vp(n_eff), nm, k, A, _vp(bg), float(pseudo), _vp(S))
    if st:
        raise HsError(st, "hs_pssm_log_odds_weighted")
    return S


def pssm_rank_scores(codes, alphabet, S, rank):
    """hs_pssm_rank_scores (host only, no GPU): the rule of Engine.pssm_rank over codes [n][k] -- every (profile, k-mer)
    pair scored under pssm_scan's contract, then dict(t [nm] the rank-th largest score of each profile, cnt_ge, cnt_gt
    uint64 [nm] the k-mers at or above and above it).  rank: a scalar or [nm]."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    assert codes.ndim == 2
    n, k = codes.shape
    S = np.ascontiguousarray(S, dtype=np.float64)
    nm = S.shape[0]
    assert S.ndim == 3 and S.shape[1] == k and (S.shape[2] == int(alphabet) or not 1 <= int(alphabet) <= 32), S.shape
    rank = np.ascontiguousarray(np.broadcast_to(np.asarray(rank, dtype=np.uint64), (nm,)))
    t = np.empty(max(nm, 1), dtype=np.float64)
    ge, gt = np.empty(max(nm, 1), dtype=np.uint64), np.empty(max(nm, 1), dtype=np.uint64)
    st = load().hs_pssm_rank_scores(_vp(codes), n, k, int(alphabet), _vp(S), nm, _vp(rank), _vp(t), _vp(ge), _vp(gt))
    if st:
        raise HsError(st, "hs_pssm_rank_scores")
    return dict(t=t[:nm], cnt_ge=ge[:nm], cnt_gt=gt[:nm])


def pssm_rank_plan(rank, n, n_s, round=0):
    """hs_pssm_rank_plan: the sample rank r_s that round `round` of Engine.pssm_rank takes its proposed threshold from,
    for the wanted rank among n k-mers and a sample of n_s; n_s + 1 means beyond the sample (the scan at -DBL_MAX)."""
    out = C.c_uint64(0)
    st = load().hs_pssm_rank_plan(int(rank), int(n), int(n_s), int(round), C.byref(out))
    if st:
        raise HsError(st, "hs_pssm_rank_plan")
    return int(out.value)


def _pssm_null_args(S, bg, t_lo):
    S = np.ascontiguousarray(S, dtype=np.float64)
    assert S.ndim == 3, S.shape
    nm, k, A = S.shape
    bg = np.ascontiguousarray(bg, dtype=np.float64)
    assert bg.shape == (A,), bg.shape
    if t_lo is not None:
        t_lo = np.ascontiguousarray(np.broadcast_to(np.asarray(t_lo, dtype=np.float64), (nm,)))
    return S, nm, k, A, bg, t_lo


def _opt(a):
    return None if a is None else _vp(a)


def pssm_null_tables(S, bg, t_lo=None, bins=4096, want_lower=True):
    """hs_pssm_null_tables (host only, no GPU): the tables Engine.pssm_pvalue builds on the device, bit for bit, for S
    [nm][k][alphabet] under the null bg [alphabet] on a grid of `bins` bins from t_lo (None: 0; a scalar or [nm]) to
    each profile's maximal score.  dict(q_dn, q_up uint16 [nm][k][alphabet], delta [nm], dead uint8 [nm], cdf_dn,
    cdf_up [nm][bins]); want_lower=False leaves cdf_up out."""
    S, nm, k, A, bg, t_lo = _pssm_null_args(S, bg, t_lo)
    B = int(bins)
    q_dn, q_up = np.empty((nm, k, A), np.uint16), np.empty((nm, k, A), np.uint16)
    delta, dead = np.empty(max(nm, 1), np.float64), np.empty(max(nm, 1), np.uint8)
    cdf_dn = np.empty((nm, max(B, 1)), np.float64)
    cdf_up = np.empty((nm, max(B, 1)), np.float64) if want_lower else None
    st = load().hs_pssm_null_tables(_vp(S), nm, k, A, _vp(bg), _opt(t_lo), B, _vp(q_dn), _vp(q_up), _vp(delta),
                                    _vp(dead), _vp(cdf_dn), _opt(cdf_up))
    if st:
        raise HsError(st, "hs_pssm_null_tables")
    res = dict(q_dn=q_dn, q_up=q_up, delta=delta[:nm], dead=dead[:nm], cdf_dn=cdf_dn)
    if want_lower:
        res["cdf_up"] = cdf_up
    return res


def pssm_pvalue_host(S, bg, hit_m, hit_score, t_lo=None, bins=4096, want_lower=True):
    """hs_pssm_pvalue_host (host only, no GPU): the rule of Engine.pssm_pvalue -- dict(p_hi [n][, p_lo [n]]), the
    bracket of P{score >= hit_score[i]} under the null bg for profile hit_m[i]."""
    S, nm, k, A, bg, t_lo = _pssm_null_args(S, bg, t_lo)
    hit_m = np.ascontiguousarray(hit_m, dtype=np.uint32)
    hit_score = np.ascontiguousarray(hit_score, dtype=np.float64)
    n = len(hit_m)
    assert hit_m.shape == hit_score.shape == (n,)
    p_hi = np.empty(max(n, 1), np.float64)
    p_lo = np.empty(max(n, 1), np.float64) if want_lower else None
    st = load().hs_pssm_pvalue_host(_vp(S), nm, k, A, _vp(bg), _opt(t_lo), int(bins), _vp(hit_m), _vp(hit_score), n,
                                    _vp(p_hi), _opt(p_lo))
    if st:
        raise HsError(st, "hs_pssm_pvalue_host")
    res = dict(p_hi=p_hi[:n])
    if want_lower:
        res["p_lo"] = p_lo[:n]
    return res


def pssm_threshold_host(S, bg, p, t_lo=None, bins=4096, want_lower=True):
    """hs_pssm_threshold_host (host only, no GPU): the rule of Engine.pssm_pvalue_threshold -- dict(t [nm] the
    threshold of the p-value p (a scalar or [nm], each in (0, 1]), p_hi [nm][, p_lo [nm]] the bracket at t, flag uint32
    [nm]: 0 exact on the grid, 1 clipped at t_lo, 2 nothing admissible (t = +DBL_MAX))."""
    S, nm, k, A, bg, t_lo = _pssm_null_args(S, bg, t_lo)
    p = np.ascontiguousarray(np.broadcast_to(np.asarray(p, dtype=np.float64), (nm,)))
    t = np.empty(max(nm, 1), np.float64)
    p_hi = np.empty(max(nm, 1), np.float64)
    p_lo = np.empty(max(nm, 1), np.float64) if want_lower else None
    flag = np.empty(max(nm, 1), np.uint32)
    st = load().hs_pssm_threshold_host(_vp(S), nm, k, A, _vp(bg), _opt(t_lo), int(bins), _vp(p), _vp(t), _vp(p_hi),
                                       _opt(p_lo), _vp(flag))
    if st:
        raise HsError(st, "hs_pssm_threshold_host")
    res = dict(t=t[:nm], p_hi=p_hi[:nm], flag=flag[:nm])
    if want_lower:
        res["p_lo"] = p_lo[:nm]
    return res


def pssm_log_odds_exact(counts, background, pseudo=1.0):
    """hs_pssm_log_odds (host only): S[m][p][a] = log2((((double)c + pseudo * bg[a]) / ((double)size + pseudo)) /
    bg[a]) for counts uint32 [nm][k][alphabet], every operation rounded to fp64 -- the function Engine.pssm_refine
    applies, bit for bit."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    assert counts.ndim == 3
    nm, k, A = counts.shape
    bg = np.ascontiguousarray(background, dtype=np.float64)
    assert bg.shape == (A,), bg.shape
    S = np.empty((nm, k, A), dtype=np.float64)
    st = load().hs_pssm_log_odds(_vp(counts), nm, k, A, _vp(bg), float(pseudo), _vp(S))
    if st:
        raise HsError(st, "hs_pssm_log_odds")
    return S


def pssm_background(counts_row):
    """hs_pssm_background (host only): the residue frequencies [alphabet] of one profile's counts [k][alphabet]; a
    residue that never occurs gets the smallest positive frequency, without renormalising."""
    counts_row = np.ascontiguousarray(counts_row, dtype=np.uint32)
    assert counts_row.ndim == 2
    k, A = counts_row.shape
    bg = np.empty(A, dtype=np.float64)
    st = load().hs_pssm_background(_vp(counts_row), k, A, _vp(bg))
    if st:
        raise HsError(st, "hs_pssm_background")
    return bg


def pssm_log_odds(counts, background=None, pseudo=1.0):
    """Log-odds profiles from position frequency matrices (hs_cluster_profile's counts [rows][k][alphabet]):
    S[r][p][a] = log2((count + pseudo * bg[a]) / (size + pseudo) / bg[a]), size = the row's members (the counts of a
    position sum to it).  background: [alphabet] frequencies; default: the residue frequencies of the counts themselves,
    summed over rows and positions (a residue that never occurs gets the smallest positive frequency seen, so that no
    entry is infinite).  Plain numpy: a convenience, not a bit-exact contract."""
    counts = np.asarray(counts, dtype=np.float64)
    assert counts.ndim == 3
    if background is None:
        bg = counts.sum(axis=(0, 1))
        if not bg.sum() > 0:
            bg = np.ones(counts.shape[2])
        bg = np.where(bg > 0, bg, bg[bg > 0].min())
        bg = bg / bg.sum()
    else:
        bg = np.asarray(background, dtype=np.float64)
        assert bg.shape == (counts.shape[2],) and (bg > 0).all()
    size = counts.sum(axis=2, keepdims=True)
    return np.log2((counts + pseudo * bg) / (size + pseudo) / bg)


def join6_tile_offset(nr, row, piece):
    """Byte offset of 16-byte piece `piece` (0..7) of row `row` inside a gathered query tile of nr <= 32 rows of the
    FP6 join (hs_join6_tile_offset; no GPU)."""
    f = load().hs_join6_tile_offset
    f.restype = C.c_uint32
    return int(f(C.c_uint32(nr), C.c_uint32(row), C.c_uint32(piece)))


def join6_selftest(device=0, variant=0):
    """GPU: the FP6 join kernel's tile product against int64 arithmetic on rows at the format's extremes.
    Returns (mismatches, first_bad) -- first_bad = (case, lane * 4 + register, float bits, expected in 64ths)."""
    n = C.c_uint64(0)
    bad = (C.c_uint32 * 4)()
    st = load().hs_join6_selftest(C.c_int(device), C.c_int(variant), C.byref(n), bad)
    if st:
        raise HsError(st, "hs_join6_selftest")
    return int(n.value), tuple(int(x) for x in bad)


def index_file_check(path):
    """Host-only check of an index file (hs_index_file_check): header, payload length + hash and the
    content rules hs_index_load enforces on the device.  Raises HsError(HS_ERR_IO) naming the fault."""
    err = C.create_string_buffer(512)
    st = load().hs_index_file_check(str(path).encode(), err, C.c_uint32(len(err)))
    if st != HS_OK:
        raise HsError(st, err.value.decode())


def index_table_append(ids, dir_key, dir_start, dir_tuple, block_ints, seed=0, out=None):
    """hs_index_table_append: one table (ids [n], dir_key [nb], dir_start [nb + 1], dir_tuple [nb][K], as hs_index_save
    writes them) merged on the host with the bucket ints block_ints [m][K] of m appended k-mers.  Returns (ids [n + m],
    dir_key, dir_start, dir_tuple) of the grown table, or None when a fingerprint is shared by two HashKey strings
    (collided: nothing written).  out: the four arrays to write into (tests: they must stay untouched on a
    collision); their directory capacity is len(out[1]).  An invalid table raises HsError(HS_ERR_INVALID)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    dir_key = np.ascontiguousarray(dir_key, dtype=np.uint64)
    dir_start = np.ascontiguousarray(dir_start, dtype=np.uint32)
    dir_tuple = np.ascontiguousarray(dir_tuple, dtype=np.int32)
    block_ints = np.ascontiguousarray(block_ints, dtype=np.int32)
    n, nb, m = len(ids), len(dir_key), block_ints.shape[0]
    K = block_ints.shape[1] if block_ints.ndim == 2 else dir_tuple.shape[1]
    assert len(dir_start) == nb + 1 and dir_tuple.size == nb * K and block_ints.size == m * K
    lib = load()
    nb_out, collided = C.c_uint64(0), C.c_uint32(0)

    def call(o_ids, o_key, o_start, o_tuple, cap):
        return lib.hs_index_table_append(_vp(ids), _vp(dir_key), _vp(dir_start), _vp(dir_tuple), C.c_uint64(n),
                                         C.c_uint64(nb), _vp(block_ints), C.c_uint64(m), C.c_uint32(K), C.c_uint32(seed),
                                         o_ids, o_key, o_start, o_tuple, C.c_uint64(cap), C.byref(nb_out),
                                         C.byref(collided))
    if out is None:
        st = call(None, None, None, None, 0)       # the two-call pattern: the count first
        if st == HS_OK and collided.value:
            return None
        if st not in (HS_OK, HS_ERR_CAPACITY):
            raise HsError(st, "hs_index_table_append")
        cap = int(nb_out.value)
        out = (np.empty(n + m, dtype=np.uint32), np.empty(cap, dtype=np.uint64), np.empty(cap + 1, dtype=np.uint32),
               np.empty((cap, K), dtype=np.int32))
    o_ids, o_key, o_start, o_tuple = out
    assert len(o_ids) >= n + m and len(o_start) >= len(o_key) + 1 and o_tuple.size >= len(o_key) * K
    st = call(_vp(o_ids), _vp(o_key), _vp(o_start), _vp(o_tuple), len(o_key))
    if st != HS_OK:
        raise HsError(st, "hs_index_table_append")
    if collided.value:
        return None
    nbo = int(nb_out.value)
    return o_ids[:n + m], o_key[:nbo], o_start[:nbo + 1], o_tuple.reshape(-1, K)[:nbo]


def index_table_remove(ids, dir_key, dir_start, dir_tuple, dead_ids, ints, seed=0, out=None):
    """hs_index_table_remove: one table (ids [n], dir_key [nb], dir_start [nb + 1], dir_tuple [nb][K], as hs_index_save
    writes them) without the ids `dead_ids` (any order, duplicates allowed), on the host.  ints [n][K]: bucket ints by
    OLD id (only the rows of k-mers that become a bucket's first member are read; None where there is none).  Returns
    (ids [n'], dir_key, dir_start, dir_tuple) of the shrunken table.  out: the four arrays to write into; their
    directory capacity is len(out[1]).  An id >= n or an invalid table raises HsError(HS_ERR_INVALID)."""
    ids = np.ascontiguousarray(ids, dtype=np.uint32)
    dir_key = np.ascontiguousarray(dir_key, dtype=np.uint64)
    dir_start = np.ascontiguousarray(dir_start, dtype=np.uint32)
    dir_tuple = np.ascontiguousarray(dir_tuple, dtype=np.int32)
    dead_ids = np.ascontiguousarray(dead_ids, dtype=np.uint32).reshape(-1)
    n, nb, m = len(ids), len(dir_key), len(dead_ids)
    if ints is not None:
        ints = np.ascontiguousarray(ints, dtype=np.int32)
        K = ints.shape[1]
        assert ints.shape[0] == n
    else:
        K = dir_tuple.shape[1]
    assert len(dir_start) == nb + 1 and dir_tuple.size == nb * K
    lib = load()
    n_out, nb_out = C.c_uint64(0), C.c_uint64(0)

    def call(o_ids, o_key, o_start, o_tuple, cap):
        return lib.hs_index_table_remove(_vp(ids), _vp(dir_key), _vp(dir_start), _vp(dir_tuple), C.c_uint64(n),
                                         C.c_uint64(nb), _vp(dead_ids), C.c_uint64(m),
                                         None if ints is None else _vp(ints), C.c_uint32(K), C.c_uint32(seed),
                                         o_ids, o_key, o_start, o_tuple, C.c_uint64(cap), C.byref(n_out),
                                         C.byref(nb_out))
    if out is None:
        st = call(None, None, None, None, 0)       # the two-call pattern: the counts first
        if st not in (HS_OK, HS_ERR_CAPACITY):
            raise HsError(st, "hs_index_table_remove")
        cap = int(nb_out.value)
        out = (np.empty(n, dtype=np.uint32), np.empty(cap, dtype=np.uint64), np.empty(cap + 1, dtype=np.uint32),
               np.empty((cap, K), dtype=np.int32))
    o_ids, o_key, o_start, o_tuple = out
    assert len(o_ids) >= n - min(m, n) and len(o_start) >= len(o_key) + 1 and o_tuple.size >= len(o_key) * K
    st = call(_vp(o_ids), _vp(o_key), _vp(o_start), _vp(o_tuple), len(o_key))
    if st != HS_OK:
        raise HsError(st, "hs_index_table_remove")
    n2, nbo = int(n_out.value), int(nb_out.value)
    return o_ids[:n2], o_key[:nbo], o_start[:nbo + 1], o_tuple.reshape(-1, K)[:nbo]


KLSH_NONE = 0xffffffffffffffff
_REDUCED_CLASS = {c: k for k, grp in enumerate(["AST", "RKEDQ", "NH", "C", "G", "IVLM", "FYW", "P"])
                  for c in grp}   # pcluster util.hpp:100-104 (include/hs_tables.h HS_REDUCED_CLASS)


def klsh_draw_planes(feat=512, bits=16, sigma=0.2):
    """The planes KLSH::KLSH draws from its default-seeded engine (lsh.cpp:17-38): (w, b, t)."""
    w = np.empty((bits, feat)); b = np.empty(bits); t = np.empty(bits)
    st = load().hs_klsh_draw_planes(C.c_uint32(feat), C.c_uint32(bits), C.c_double(sigma), _vp(w),
                                    _vp(b), _vp(t))
    if st != HS_OK:
        raise HsError(st, "hs_klsh_draw_planes")
    return w, b, t


def klsh_codes(classes, seq_start, w, b, t, device=0):
    """KLSH code of every sequence of a concatenated buffer of reduced-alphabet
    classes (pcluster.cpp:11-33 + lsh.cpp:40-49) on the GPU.  Returns (codes uint64 [n_seq] with
    KLSH_NONE for sequences shorter than 3, uncertain-bit masks uint64 [n_seq])."""
    classes = np.ascontiguousarray(classes, dtype=np.uint8)
    seq_start = np.ascontiguousarray(seq_start, dtype=np.uint64)
    w = np.ascontiguousarray(w, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    t = np.ascontiguousarray(t, dtype=np.float64)
    n_seq = len(seq_start) - 1
    codes = np.empty(n_seq, dtype=np.uint64); unc = np.empty(n_seq, dtype=np.uint64)
    err = C.create_string_buffer(256)
    st = load().hs_klsh_codes(C.c_int(device), _vp(classes), C.c_uint64(len(classes)), _vp(seq_start),
                              C.c_uint64(n_seq), _vp(w), _vp(b), _vp(t), C.c_uint32(w.shape[0]),
                              _vp(codes), _vp(unc), err, C.c_uint32(256))
    if st != HS_OK:
        raise HsError(st, err.value.decode())
    return codes, unc


class Engine:
    """One handle = one GPU + one index.  Mirrors the reference's operator surface:
    LSH(dim, K, W) x L  ->  Engine(k, K, L, W, a, b);  HashBucketIndex -> hash_points/hash_codes;
    Search() build loop -> index_build; Search() query loop -> query; noLSH Search() -> bruteforce.
    """

    def __init__(self, k, K, L, W, a, b, device=0, coords=None, hooks=False, options=None):
        self._lib = load(hooks)
        self.k, self.K, self.L, self.W = int(k), int(K), int(L), float(W)
        self.d = 8 * self.k
        self.T = 0  # hs_set_multiprobe
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert a.shape == (self.L, self.K, self.d), a.shape
        assert b.shape == (self.L, self.K), b.shape
        cptr = None
        if coords is not None:
            coords = np.ascontiguousarray(coords, dtype=np.float64)
            assert coords.ndim == 2 and coords.shape[1] == 8 and 1 <= coords.shape[0] <= 32
            cptr = _vp(coords)
        params = _Params(self.k, self.K, self.L, self.W, int(device),
                         0 if coords is None else coords.shape[0])
        self._h = C.c_void_p()
        st = self._lib.hs_create(C.byref(params), _vp(a), _vp(b), cptr, C.byref(self._h))
        if st != HS_OK:
            msg = self._lib.hs_last_error(self._h).decode() if self._h else ""
            if self._h:
                self._lib.hs_destroy(self._h)
                self._h = C.c_void_p()
            raise HsError(st, msg or "hs_create failed (is a gfx950 GPU visible?)")
        for name, value in (options or {}).items():      # hs_set_option, before any index exists
            self.set_option(name, value)

    # -- helpers
    def _check(self, st):
        if st != HS_OK:
            raise HsError(st, self._lib.hs_last_error(self._h).decode())

    def set_verify_mode(self, mode):
        """'auto' | 'stream' | 'join' -- which filter kernel runs in front of the exact decision."""
        self._check(self._lib.hs_set_verify_mode(self._h, {"auto": 0, "stream": 1, "join": 2, "join16": 3}[mode]))

    def set_hash_mode(self, mode, eps_scale=1.0):
        """'auto' | 'exact' | 'mfma' -- how the bucket ints are evaluated (identical results)."""
        self._check(self._lib.hs_set_hash_mode(self._h, {"auto": 0, "exact": 1, "mfma": 2}[mode],
                                               C.c_double(eps_scale)))

    OPTIONS = {"query_batch": 1, "seg_mode": 2, "join_resident": 3, "recognise_kmers": 4, "build_grouping": 5,
               "wide_rows": 6, "refine8": 7, "self_codes": 8, "sort_hits": 10, "sync_items": 11,
               "join_min_q": 12, "join_min_m": 13, "sort_from_bit": 14, "build_serial": 15,
               "join_xcd_run": 16, "probe_records": 17, "join_chunk": 18, "summary_chunk": 19, "summary_rows": 20,
               "msf_edge_budget": 21, "join_f6": 22, "pssm_filter": 23, "pssm_topk_sample": 24, "pssm_rank_sample": 26,
               "pssm_count_chunk": 25, "pssm_null_bins": 27, "join_f6_form": 28,
               "pssm_cmp_filter": 29}

    def set_option(self, name, value):
        """hs_set_option (include/hsearch.h hs_option): path selection / batch sizing; never changes a result."""
        self._check(self._lib.hs_set_option(self._h, C.c_int(self.OPTIONS[name]), C.c_int64(int(value))))

    def set_bucket_partition(self, part, n_parts):
        """hs_set_bucket_partition: the handle's searches probe only the buckets of `part` of `n_parts` (1: all)."""
        self._check(self._lib.hs_set_bucket_partition(self._h, C.c_uint32(part), C.c_uint32(n_parts)))

    def set_multiprobe(self, T):
        """hs_set_multiprobe: the handle's searches also probe the T neighbouring buckets per table (0: one probe)."""
        self._check(self._lib.hs_set_multiprobe(self._h, C.c_uint32(int(T))))
        self.T = int(T)

    def probe_buckets(self, centers):
        """hs_probe_buckets: (buckets int32 [nq][L][1+T][K], valid uint8 [nq][L][1+T]) under the handle's T."""
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        n = centers.shape[0]
        assert centers.shape == (n, self.d)
        P = self.T + 1
        buckets = np.empty((n, self.L, P, self.K), dtype=np.int32)
        valid = np.empty((n, self.L, P), dtype=np.uint8)
        self._check(self._lib.hs_probe_buckets(self._h, _vp(centers), C.c_uint64(n), _vp(buckets), _vp(valid)))
        return buckets, valid

    def wait_event(self, event_handle):
        """hs_wait_event: the library's stream waits for a hipEvent_t (int handle, e.g. torch.cuda.Event.cuda_event)."""
        self._check(self._lib.hs_wait_event(self._h, C.c_void_p(event_handle)))

    def set_planes(self, a, b):
        """A new hash family of the same shape for this handle (hs_set_planes); drops the index."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert a.shape == (self.L, self.K, self.d) and b.shape == (self.L, self.K)
        self._check(self._lib.hs_set_planes(self._h, _vp(a), _vp(b)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hs_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def profile(self):
        p = _Profile()
        self._check(self._lib.hs_get_profile(self._h, C.byref(p)))
        return {f: getattr(p, f) for f in profile_fields}

    def index_info(self):
        info = _IndexInfo()
        self._check(self._lib.hs_index_info_get(self._h, C.byref(info)))
        return dict(n=info.n, device_bytes=info.device_bytes,
                    n_buckets=list(info.n_buckets)[:self.L], max_bucket=list(info.max_bucket)[:self.L],
                    key_seed=info.key_seed)

    # -- a2 / a4 / a5
    def embed_codes(self, codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n = codes.shape[0]
        out = np.empty((n, self.d), dtype=np.float64)
        self._check(self._lib.hs_embed_codes(self._h, _vp(codes), C.c_uint64(n), _vp(out)))
        return out

    def hash_codes(self, codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n = codes.shape[0]
        assert codes.shape == (n, self.k)
        out = np.empty((n, self.L, self.K), dtype=np.int32)
        self._check(self._lib.hs_hash_codes(self._h, _vp(codes), C.c_uint64(n), _vp(out)))
        return out

    def hash_points(self, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        n = pts.shape[0]
        assert pts.shape == (n, self.d)
        out = np.empty((n, self.L, self.K), dtype=np.int32)
        self._check(self._lib.hs_hash_points(self._h, _vp(pts), C.c_uint64(n), _vp(out)))
        return out

    # -- a7
    def index_build(self, codes):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        n = codes.shape[0]
        assert codes.ndim == 2 and codes.shape[1] == self.k
        self._check(self._lib.hs_index_build(self._h, _vp(codes), C.c_uint64(n)))
        return self.index_info()

    def index_build_subset(self, codes_all, subset):
        """Index over rows `subset` (uint32, or None for all) of a code array kept on the device across
        calls (hs_index_build_subset); the array must stay alive and unchanged between calls."""
        assert codes_all.dtype == np.uint8 and codes_all.flags["C_CONTIGUOUS"] and codes_all.shape[1] == self.k
        n_all = codes_all.shape[0]
        sub = None if subset is None else np.ascontiguousarray(subset, dtype=np.uint32)
        n_sub = n_all if sub is None else len(sub)
        self._check(self._lib.hs_index_build_subset(self._h, _vp(codes_all), C.c_uint64(n_all),
                                                    _vp(sub) if sub is not None else C.c_void_p(0),
                                                    C.c_uint64(n_sub)))
        return self.index_info()

    # -- a7 with the hashing spread over ranks (hs_index_shard_*: pointers are device pointers, ints)
    def shard_begin(self, codes, rank, world):
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        assert codes.ndim == 2 and codes.shape[1] == self.k
        lo, cnt = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.hs_index_shard_begin(self._h, _vp(codes), C.c_uint64(codes.shape[0]), C.c_uint32(rank),
                                                   C.c_uint32(world), C.byref(lo), C.byref(cnt)))
        return lo.value, cnt.value

    def shard_hash(self, l, seed, d_fp_block):
        self._check(self._lib.hs_index_shard_hash_dev(self._h, C.c_uint32(l), C.c_uint32(seed), C.c_void_p(d_fp_block)))

    def shard_group(self, l, d_fp_all):
        nb = C.c_uint32(0)
        self._check(self._lib.hs_index_shard_group_dev(self._h, C.c_uint32(l), C.c_void_p(d_fp_all), C.byref(nb)))
        return nb.value

    def shard_tuples(self, l, d_tuples):
        self._check(self._lib.hs_index_shard_tuples_dev(self._h, C.c_uint32(l), C.c_void_p(d_tuples)))

    def shard_finish(self, l, d_tuples_all):
        col = C.c_uint32(0)
        self._check(self._lib.hs_index_shard_finish_dev(self._h, C.c_uint32(l), C.c_void_p(d_tuples_all), C.byref(col)))
        return col.value

    def shard_end(self, seed):
        self._check(self._lib.hs_index_shard_end(self._h, C.c_uint32(seed)))
        return self.index_info()

    def index_build_windows(self, residues, seq_start):
        """the DB = every length-k window of every sequence of a concatenated
        residue-code buffer (kmer_search.cpp:64-83 order).  residues: uint8 codes; seq_start:
        n_seq + 1 ascending offsets ending at len(residues).  Returns (index info, window start
        positions [n_windows] uint32); DB id i = window i."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        seq_start = np.ascontiguousarray(seq_start, dtype=np.uint64)
        n_seq = len(seq_start) - 1
        assert n_seq >= 0 and int(seq_start[-1]) == len(residues)
        lens = np.diff(seq_start.astype(np.int64))
        n_win = int(np.maximum(lens - self.k + 1, 0).sum())
        pos = np.empty(n_win, dtype=np.uint32)
        n = C.c_uint64(0)
        self._check(self._lib.hs_index_build_windows(self._h, _vp(residues), C.c_uint64(len(residues)),
                                                     _vp(seq_start), C.c_uint64(n_seq), C.byref(n),
                                                     _vp(pos)))
        assert int(n.value) == n_win
        return self.index_info(), pos

    def index_append(self, codes):
        """hs_index_append: the built index grown by the k-mers `codes` (ids n .. n + m - 1), on the device; the
        handle then equals one built over the concatenation, bit for bit.  Returns the index info."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        assert codes.ndim == 2 and codes.shape[1] == self.k
        self._check(self._lib.hs_index_append(self._h, _vp(codes), C.c_uint64(codes.shape[0])))
        return self.index_info()

    def index_append_dev(self, tensor):
        """hs_index_append_dev: the block as a uint8 tensor [m][k] on the handle's GPU (or (device pointer, m))."""
        if isinstance(tensor, tuple):
            ptr, m = int(tensor[0]), int(tensor[1])
        else:
            assert tensor.is_cuda and tensor.is_contiguous() and tensor.dim() == 2 and tensor.shape[1] == self.k
            assert tensor.element_size() == 1
            import torch
            torch.cuda.current_stream(tensor.device).synchronize()   # complete when it is handed over
            ptr, m = tensor.data_ptr(), tensor.shape[0]
        self._check(self._lib.hs_index_append_dev(self._h, C.c_void_p(ptr), C.c_uint64(m)))
        return self.index_info()

    def index_append_windows(self, residues, seq_start):
        """hs_index_append_windows: the windows of further sequences appended (index_build_windows' enumeration).
        Returns (index info, window start positions [m] uint32 of the APPENDED windows, in `residues`)."""
        residues = np.ascontiguousarray(residues, dtype=np.uint8)
        seq_start = np.ascontiguousarray(seq_start, dtype=np.uint64)
        n_seq = len(seq_start) - 1
        assert n_seq >= 0 and int(seq_start[-1]) == len(residues)
        lens = np.diff(seq_start.astype(np.int64))
        n_win = int(np.maximum(lens - self.k + 1, 0).sum())
        pos = np.empty(n_win, dtype=np.uint32)
        n = C.c_uint64(0)
        self._check(self._lib.hs_index_append_windows(self._h, _vp(residues), C.c_uint64(len(residues)),
                                                      _vp(seq_start), C.c_uint64(n_seq), C.byref(n), _vp(pos)))
        assert int(n.value) == n_win
        return self.index_info(), pos

    def index_remove(self, ids):
        """hs_index_remove: the built index without the k-mers `ids` (any order, duplicates allowed), on the device;
        the handle then equals one built over the surviving rows, bit for bit.  Returns new_id [old n] uint32: each
        old id's new id, 0xffffffff for a removed one."""
        ids = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        new_id = np.empty(self._n(), dtype=np.uint32)
        self._check(self._lib.hs_index_remove(self._h, _vp(ids), C.c_uint64(len(ids)), _vp(new_id)))
        return new_id

    def index_remove_dev(self, tensor, new_id=None):
        """hs_index_remove_dev: the ids as an int32 / uint32 tensor [m] on the handle's GPU (or (device pointer, m));
        new_id: an int32 tensor [old n] on the same GPU to receive the new ids (0xffffffff reads -1), or None."""
        if isinstance(tensor, tuple):
            ptr, m = int(tensor[0]), int(tensor[1])
        else:
            assert tensor.is_cuda and tensor.is_contiguous() and tensor.dim() == 1 and tensor.element_size() == 4
            import torch
            torch.cuda.current_stream(tensor.device).synchronize()   # complete when it is handed over
            ptr, m = tensor.data_ptr(), tensor.shape[0]
        out = None
        if new_id is not None:
            assert new_id.is_cuda and new_id.is_contiguous() and new_id.element_size() == 4
            assert new_id.numel() >= self._n()
            out = C.c_void_p(new_id.data_ptr())
        self._check(self._lib.hs_index_remove_dev(self._h, C.c_void_p(ptr), C.c_uint64(m), out))
        return self.index_info()

    def index_remove_ranges(self, first, count):
        """hs_index_remove_ranges: the ids [first[r], first[r] + count[r]) removed (ranges may overlap), marked on the
        device; for a windows index window_id_start gives a sequence's range.  Returns new_id as index_remove."""
        first = np.ascontiguousarray(first, dtype=np.uint64).reshape(-1)
        count = np.ascontiguousarray(count, dtype=np.uint64).reshape(-1)
        assert len(first) == len(count)
        new_id = np.empty(self._n(), dtype=np.uint32)
        self._check(self._lib.hs_index_remove_ranges(self._h, _vp(first), _vp(count), C.c_uint64(len(first)),
                                                     _vp(new_id)))
        return new_id

    def index_save(self, path):
        """write the built index (parameters, planes, table, codes, L tables)."""
        self._check(self._lib.hs_index_save(self._h, str(path).encode()))

    def index_load(self, path):
        """Restore an index written by index_save into a handle created with the same parameters,
        planes and coordinate table (HS_ERR_IO otherwise)."""
        self._check(self._lib.hs_index_load(self._h, str(path).encode()))
        return self.index_info()

    # -- a8..a10
    def query(self, centers, R, cap=None, want_cand=True):
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        nq = centers.shape[0]
        assert centers.shape == (nq, self.d)
        cap = int(cap) if cap is not None else max(1024, 64 * nq)
        while True:
            hq = np.empty(cap, dtype=np.uint32)
            hid = np.empty(cap, dtype=np.uint32)
            ht = np.empty(cap, dtype=np.uint32)
            hd = np.empty(cap, dtype=np.float64)
            cand = np.zeros((nq, self.L), dtype=np.uint64) if want_cand else None
            n = C.c_uint64(0)
            st = self._lib.hs_query(self._h, _vp(centers), C.c_uint64(nq), C.c_double(R), _vp(hq),
                                    _vp(hid), _vp(ht), _vp(hd), C.c_uint64(cap), C.byref(n),
                                    _vp(cand) if want_cand else None)
            if st == HS_ERR_CAPACITY:
                cap = int(n.value)
                continue
            self._check(st)
            n = int(n.value)
            return dict(q=hq[:n], id=hid[:n], table=ht[:n], dist=hd[:n], cand=cand)

    def query_codes(self, qcodes, R, cap=None, want_cand=True):
        """hs_query_codes: the queries are k-mers given as residue codes [nq][k] (uint8)."""
        qcodes = np.ascontiguousarray(qcodes, dtype=np.uint8)
        nq = qcodes.shape[0]
        assert qcodes.shape == (nq, self.k)
        cap = int(cap) if cap is not None else max(1024, 64 * nq)
        while True:
            hq = np.empty(cap, dtype=np.uint32)
            hid = np.empty(cap, dtype=np.uint32)
            ht = np.empty(cap, dtype=np.uint32)
            hd = np.empty(cap, dtype=np.float64)
            cand = np.zeros((nq, self.L), dtype=np.uint64) if want_cand else None
            n = C.c_uint64(0)
            st = self._lib.hs_query_codes(self._h, _vp(qcodes), C.c_uint64(nq), C.c_double(R), _vp(hq),
                                          _vp(hid), _vp(ht), _vp(hd), C.c_uint64(cap), C.byref(n),
                                          _vp(cand) if want_cand else None)
            if st == HS_ERR_CAPACITY:
                cap = int(n.value)
                continue
            self._check(st)
            n = int(n.value)
            return dict(q=hq[:n], id=hid[:n], table=ht[:n], dist=hd[:n], cand=cand)

    def query_into(self, queries, R, hq, hid, ht, hd, codes=False):
        """hs_query / hs_query_codes (HOST pointers, the PCIe-inclusive entry points) into caller-owned
        numpy arrays -- no allocation per call, for timing.  Returns the number of hits."""
        queries = np.ascontiguousarray(queries, dtype=np.uint8 if codes else np.float64)
        n = C.c_uint64(0)
        fn = self._lib.hs_query_codes if codes else self._lib.hs_query
        st = fn(self._h, _vp(queries), C.c_uint64(queries.shape[0]), C.c_double(R), _vp(hq), _vp(hid), _vp(ht),
                _vp(hd), C.c_uint64(len(hq)), C.byref(n), None)
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n.value)
            raise e
        self._check(st)
        return int(n.value)

    def query_dev(self, d_centers_ptr, nq, R, d_q, d_id, d_table, d_dist, cap, d_cand=None, codes=False):
        """Raw device-pointer call (ints from torch .data_ptr()).  Returns the number of hits; raises
        HsError(HS_ERR_CAPACITY) with the required size in .needed when cap is too small.
        codes=True: d_centers_ptr points at residue codes uint8 [nq][k] (hs_query_codes_dev)."""
        n = C.c_uint64(0)
        fn = self._lib.hs_query_codes_dev if codes else self._lib.hs_query_dev
        st = fn(self._h, C.c_void_p(d_centers_ptr), C.c_uint64(nq), C.c_double(R),
                                    C.c_void_p(d_q), C.c_void_p(d_id), C.c_void_p(d_table),
                                    C.c_void_p(d_dist), C.c_uint64(cap), C.byref(n),
                                    C.c_void_p(d_cand) if d_cand else None)
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n.value)
            raise e
        self._check(st)
        return int(n.value)

    def query_radii(self, queries, radii, codes=False, cap=None, want_cand=True):
        """hs_query_radii: query q searched at radii[q]; queries are points [nq][d], or with codes=True residue
        codes [nq][k].  The same result dict as query()."""
        queries = np.ascontiguousarray(queries, dtype=np.uint8 if codes else np.float64)
        radii = np.ascontiguousarray(radii, dtype=np.float64)
        nq = queries.shape[0]
        assert queries.shape == (nq, self.k if codes else self.d) and radii.shape == (nq,)
        cap = int(cap) if cap is not None else max(1024, 64 * nq)
        while True:
            hq = np.empty(cap, dtype=np.uint32)
            hid = np.empty(cap, dtype=np.uint32)
            ht = np.empty(cap, dtype=np.uint32)
            hd = np.empty(cap, dtype=np.float64)
            cand = np.zeros((nq, self.L), dtype=np.uint64) if want_cand else None
            n = C.c_uint64(0)
            st = self._lib.hs_query_radii(self._h, None if codes else _vp(queries), _vp(queries) if codes else None,
                                          nq, _vp(radii), _vp(hq), _vp(hid), _vp(ht), _vp(hd), cap, C.byref(n),
                                          _vp(cand) if want_cand else None)
            if st == HS_ERR_CAPACITY:
                cap = int(n.value)
                continue
            self._check(st)
            n = int(n.value)
            return dict(q=hq[:n], id=hid[:n], table=ht[:n], dist=hd[:n], cand=cand)

    def query_radii_dev(self, d_queries_ptr, nq, d_radii_ptr, d_q, d_id, d_table, d_dist, cap, d_cand=None,
                        codes=False):
        """hs_query_radii_dev (device pointers as ints); as query_dev, with float64 radii [nq] on the device."""
        n = C.c_uint64(0)
        st = self._lib.hs_query_radii_dev(self._h, None if codes else d_queries_ptr, d_queries_ptr if codes else None,
                                          nq, d_radii_ptr, d_q, d_id, d_table, d_dist, cap, C.byref(n),
                                          d_cand if d_cand else None)
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n.value)
            raise e
        self._check(st)
        return int(n.value)

    def annotate(self, queries, R=None, radii=None, codes=False, cap=None):
        """hs_annotate: per DB k-mer reached, the nearest centre -- of the hits query() / query_codes() (R) or
        query_radii() (radii) would return, per distinct id the one smallest under (dist, table, q), in ascending
        id.  queries are points [nq][d], or with codes=True residue codes [nq][k].  cap=None: sized by the index."""
        queries = np.ascontiguousarray(queries, dtype=np.uint8 if codes else np.float64)
        nq = queries.shape[0]
        assert queries.shape == (nq, self.k if codes else self.d)
        assert (R is None) != (radii is None), "exactly one of R and radii"
        if radii is not None:
            radii = np.ascontiguousarray(radii, dtype=np.float64)
            assert radii.shape == (nq,)
        if cap is None:  # the index's n always suffices
            info = _IndexInfo()
            cap = max(1024, int(info.n)) if self._lib.hs_index_info_get(self._h, C.byref(info)) == HS_OK else 1024
        cap = int(cap)
        while True:
            oid = np.empty(cap, dtype=np.uint32)
            oq = np.empty(cap, dtype=np.uint32)
            ot = np.empty(cap, dtype=np.uint32)
            od = np.empty(cap, dtype=np.float64)
            n = C.c_uint64(0)
            st = self._lib.hs_annotate(self._h, None if codes else _vp(queries), _vp(queries) if codes else None, nq,
                                       0.0 if R is None else float(R), None if radii is None else _vp(radii),
                                       _vp(oid), _vp(oq), _vp(ot), _vp(od), cap, C.byref(n))
            if st == HS_ERR_CAPACITY:
                cap = int(n.value)
                continue
            self._check(st)
            n = int(n.value)
            return dict(id=oid[:n], q=oq[:n], table=ot[:n], dist=od[:n])

    def annotate_dev(self, d_queries_ptr, nq, R, d_radii_ptr, d_id, d_q, d_table, d_dist, cap, codes=False):
        """hs_annotate_dev (device pointers as ints; d_radii_ptr None or 0: every query at R).  Returns the number
        of rows; raises HsError(HS_ERR_CAPACITY) with the required size in .needed when cap is too small."""
        n = C.c_uint64(0)
        st = self._lib.hs_annotate_dev(self._h, None if codes else d_queries_ptr, d_queries_ptr if codes else None,
                                       nq, float(R), d_radii_ptr if d_radii_ptr else None, d_id, d_q, d_table, d_dist,
                                       cap, C.byref(n))
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n.value)
            raise e
        self._check(st)
        return int(n.value)

    def query_topk(self, queries, topk, R=None, radii=None, codes=False):
        """hs_query_topk: per query the topk smallest, under (dist, id), of the hits query() / query_codes() (R) or
        query_radii() (radii) would return, selected on the device: dict(id, table, dist [nq][topk] -- unused entries
        capi.NO_ID, capi.NO_ID, inf --, count uint32 [nq] = the query's full hit count, n_hits = their sum).  queries are
        points [nq][d], or with codes=True residue codes [nq][k]."""
        queries = np.ascontiguousarray(queries, dtype=np.uint8 if codes else np.float64)
        nq = queries.shape[0]
        assert queries.shape == (nq, self.k if codes else self.d)
        assert (R is None) != (radii is None), "exactly one of R and radii"
        if radii is not None:
            radii = np.ascontiguousarray(radii, dtype=np.float64)
            assert radii.shape == (nq,)
        topk = int(topk)
        rows = max(0, min(topk, TOPK_MAX))
        nid = np.empty((nq, rows), dtype=np.uint32)
        nt = np.empty((nq, rows), dtype=np.uint32)
        nd = np.empty((nq, rows), dtype=np.float64)
        cnt = np.empty(nq, dtype=np.uint32)
        n = C.c_uint64(0)
        self._check(self._lib.hs_query_topk(self._h, None if codes else _vp(queries), _vp(queries) if codes else None,
                                            nq, 0.0 if R is None else float(R), None if radii is None else _vp(radii),
                                            topk, _vp(nid), _vp(nt), _vp(nd), _vp(cnt), C.byref(n)))
        return dict(id=nid, table=nt, dist=nd, count=cnt, n_hits=int(n.value))

    def query_topk_dev(self, d_queries_ptr, nq, topk, R, d_radii_ptr, d_id, d_table, d_dist, d_count, codes=False):
        """hs_query_topk_dev (device pointers as ints; d_radii_ptr None or 0: every query at R; d_table may be None):
        the rows into uint32 / uint32 / float64 [nq][topk] and the counts into uint32 [nq]; returns n_hits."""
        n = C.c_uint64(0)
        self._check(self._lib.hs_query_topk_dev(self._h, None if codes else d_queries_ptr,
                                                d_queries_ptr if codes else None, nq, float(R),
                                                d_radii_ptr if d_radii_ptr else None, int(topk), d_id,
                                                d_table if d_table else None, d_dist, d_count, C.byref(n)))
        return int(n.value)

    def seq_match(self, queries, id_start, R=None, radii=None, codes=False, q_group=None, n_groups=None, q_off=None):
        """hs_seq_match: the hits query() / query_codes() (R) or query_radii() (radii) would return, reduced on the
        device per (query group, database sequence, diagonal): dict(group, seq, diag, count, best_dist, best_q, best_id,
        lo, hi -- one row per distinct key, ascending --, n_hits).  id_start [n_seq + 1]: sequence s owns the ids
        [id_start[s], id_start[s + 1]) (capi.window_id_start for a windows index).  q_group [nq] with n_groups (None:
        every query its own group), q_off [nq] (None: no diagonals, diag = 0).  queries are points [nq][d], or with
        codes=True residue codes [nq][k] (capi.protein_queries cuts proteins into them).  Two calls: the row count,
        then the rows."""
        queries = np.ascontiguousarray(queries, dtype=np.uint8 if codes else np.float64)
        nq = queries.shape[0]
        assert queries.shape == (nq, self.k if codes else self.d)
        assert (R is None) != (radii is None), "exactly one of R and radii"
        if radii is not None:
            radii = np.ascontiguousarray(radii, dtype=np.float64)
            assert radii.shape == (nq,)
        q_group, q_off, id_start, n_groups, n_seq = _seq_keys(nq, q_group, n_groups, q_off, id_start)
        cap = 0
        while True:
            arrs = _seq_rows(cap)
            n, nh = C.c_uint64(0), C.c_uint64(0)
            st = self._lib.hs_seq_match(self._h, None if codes else _vp(queries), _vp(queries) if codes else None, nq,
                                        0.0 if R is None else float(R), None if radii is None else _vp(radii),
                                        None if q_group is None else _vp(q_group), n_groups,
                                        None if q_off is None else _vp(q_off), _vp(id_start), n_seq,
                                        *[_vp(a) if cap else None for a in arrs], cap, C.byref(n), C.byref(nh))
            if st == HS_ERR_CAPACITY and int(n.value) > cap:
                cap = int(n.value)
                continue
            self._check(st)
            res = _seq_dict(arrs, int(n.value))
            res["n_hits"] = int(nh.value)
            return res

    def seq_match_dev(self, d_queries_ptr, nq, R, d_radii_ptr, d_q_group, n_groups, d_q_off, d_id_start, n_seq, d_rows,
                      cap, codes=False):
        """hs_seq_match_dev (device pointers as ints; d_radii_ptr / d_q_group / d_q_off None or 0: absent; d_rows: the
        nine row arrays in the order of capi.SEQ_MATCH_FIELDS).  Returns (rows, n_hits); raises
        HsError(HS_ERR_CAPACITY) with the required size in .needed when cap is too small."""
        n, nh = C.c_uint64(0), C.c_uint64(0)
        st = self._lib.hs_seq_match_dev(self._h, None if codes else d_queries_ptr, d_queries_ptr if codes else None,
                                        nq, float(R), d_radii_ptr if d_radii_ptr else None,
                                        d_q_group if d_q_group else None, int(n_groups), d_q_off if d_q_off else None,
                                        d_id_start, int(n_seq), *[p if p else None for p in d_rows], cap, C.byref(n),
                                        C.byref(nh))
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n.value)
            raise e
        self._check(st)
        return int(n.value), int(nh.value)

    def merge_first_table_dev(self, d_q, d_id, d_table, d_dist, n):
        """hs_merge_first_table_dev (device pointers as ints; in place): the number of tuples kept."""
        n_out = C.c_uint64(0)
        self._check(self._lib.hs_merge_first_table_dev(self._h, C.c_void_p(d_q), C.c_void_p(d_id), C.c_void_p(d_table),
                                                       C.c_void_p(d_dist), C.c_uint64(n), C.byref(n_out)))
        return int(n_out.value)

    # -- a11
    def bruteforce(self, centers, R, cap=None):
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        nq = centers.shape[0]
        cap = int(cap) if cap is not None else max(1024, 64 * nq)
        while True:
            hq = np.empty(cap, dtype=np.uint32)
            hid = np.empty(cap, dtype=np.uint32)
            hd = np.empty(cap, dtype=np.float64)
            n = C.c_uint64(0)
            st = self._lib.hs_bruteforce(self._h, _vp(centers), C.c_uint64(nq), C.c_double(R),
                                         _vp(hq), _vp(hid), _vp(hd), C.c_uint64(cap), C.byref(n))
            if st == HS_ERR_CAPACITY:
                cap = int(n.value)
                continue
            self._check(st)
            n = int(n.value)
            return dict(q=hq[:n], id=hid[:n], dist=hd[:n])

    def _alphabet(self):
        p = _Params()
        self._check(self._lib.hs_get_params(self._h, C.byref(p)))
        return int(p.alphabet)

    def pssm_scan(self, S, t, cap=None, want_counts=True):
        """hs_pssm_scan: every indexed k-mer against the profiles S [nm][k][alphabet] at thresholds t [nm].
        dict(m, id, score[, cnt]): the hits (score >= t[m], the fp64 left-to-right sum) in (m, id) order."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        nm = S.shape[0]
        assert S.shape == (nm, self.k, self._alphabet()) and t.shape == (nm,), (S.shape, t.shape)
        cap = int(cap) if cap is not None else max(1024, 64 * nm)
        cnt = np.zeros(nm, dtype=np.uint64) if want_counts else None
        while True:
            hm = np.empty(cap, dtype=np.uint32)
            hid = np.empty(cap, dtype=np.uint32)
            hs = np.empty(cap, dtype=np.float64)
            n = C.c_uint64(0)
            st = self._lib.hs_pssm_scan(self._h, _vp(S), _vp(t), C.c_uint64(nm), _vp(hm), _vp(hid), _vp(hs),
                                        C.c_uint64(cap), C.byref(n), _vp(cnt) if want_counts else None)
            if st == HS_ERR_CAPACITY:
                cap = int(n.value)
                continue
            self._check(st)
            n = int(n.value)
            res = dict(m=hm[:n], id=hid[:n], score=hs[:n])
            if want_counts:
                res["cnt"] = cnt
            return res

    def pssm_scan_dev(self, d_S, d_t, nm, d_m, d_id, d_score, cap, d_cnt=None):
        """hs_pssm_scan_dev: device pointers (ints, e.g. tensor.data_ptr()); returns the hit count.  Raises HsError
        with status HS_ERR_CAPACITY (its required capacity in .n_hits) when the hits exceed cap."""
        n = C.c_uint64(0)
        st = self._lib.hs_pssm_scan_dev(self._h, C.c_void_p(d_S), C.c_void_p(d_t), C.c_uint64(nm), C.c_void_p(d_m),
                                        C.c_void_p(d_id), C.c_void_p(d_score), C.c_uint64(cap), C.byref(n),
                                        C.c_void_p(d_cnt) if d_cnt else None)
        if st != HS_OK:
            err = HsError(st, self._lib.hs_last_error(self._h).decode())
            err.n_hits = int(n.value)
            raise err
        return int(n.value)

    def pssm_compare(self, X, t, Y=None, min_overlap=1, cap=None, want_counts=True):
        """hs_pssm_compare: the profiles X [nx][k][alphabet] against Y [ny][k][alphabet] (None: X against itself, pairs
        x < y) at every offset with at least min_overlap columns in common; t a scalar or [nx].  No index is needed.
        dict(x, y, d, score[, cnt]): one hit per pair whose best offset scores >= t[x], in (x, y) order."""
        X, t, Y, nx, ny, k, A = _pssm_compare_args(X, t, Y)
        assert (k, A) == (self.k, self._alphabet()), X.shape
        st, res = _pssm_compare_call(
            lambda hx, hy, hd, hs, c, n, cnt: self._lib.hs_pssm_compare(
                self._h, _vp(X), C.c_uint64(nx), _vp(Y) if Y is not None else None, C.c_uint64(ny), _vp(t),
                C.c_uint32(min_overlap), hx, hy, hd, hs, c, n, cnt), nx, cap, want_counts)
        self._check(st)
        return res

    def pssm_compare_dev(self, d_X, nx, d_Y, ny, d_t, min_overlap, d_x, d_y, d_d, d_score, cap, d_cnt=None):
        """hs_pssm_compare_dev: device pointers (ints, e.g. tensor.data_ptr(); d_Y 0 / None: self mode); returns the hit
        count.  Raises HsError with status HS_ERR_CAPACITY (its required capacity in .n_hits) when the hits exceed cap."""
        n = C.c_uint64(0)
        st = self._lib.hs_pssm_compare_dev(self._h, C.c_void_p(d_X), C.c_uint64(nx), C.c_void_p(d_Y) if d_Y else None,
                                           C.c_uint64(ny), C.c_void_p(d_t), C.c_uint32(min_overlap), C.c_void_p(d_x),
                                           C.c_void_p(d_y), C.c_void_p(d_d), C.c_void_p(d_score), C.c_uint64(cap),
                                           C.byref(n), C.c_void_p(d_cnt) if d_cnt else None)
        if st != HS_OK:
            err = HsError(st, self._lib.hs_last_error(self._h).decode())
            err.n_hits = int(n.value)
            raise err
        return int(n.value)

    def pssm_topk(self, S, topk, t_floor=None, want_thresholds=False):
        """hs_pssm_topk: the topk best indexed k-mers of every profile S [nm][k][alphabet] under (score descending, id
        ascending), among those scoring >= t_floor[m] (None: no floor).  dict(id uint32 [nm][topk] padded with NO_ID,
        score [nm][topk] padded with -inf, count uint32 [nm][, t_used [nm]: the thresholds the profiles were scanned
        at -- the one output that depends on the "pssm_topk_sample" option])."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        nm = S.shape[0]
        assert S.shape == (nm, self.k, self._alphabet()), S.shape
        if t_floor is not None:
            t_floor = np.ascontiguousarray(t_floor, dtype=np.float64)
            assert t_floor.shape == (nm,), t_floor.shape
        cols = int(topk) if 1 <= int(topk) <= TOPK_MAX else 1
        tid = np.empty((nm, cols), dtype=np.uint32)
        ts = np.empty((nm, cols), dtype=np.float64)
        tc = np.empty(max(nm, 1), dtype=np.uint32)
        tu = np.empty(max(nm, 1), dtype=np.float64) if want_thresholds else None
        self._check(self._lib.hs_pssm_topk(self._h, _vp(S), _vp(t_floor) if t_floor is not None else None,
                                           C.c_uint64(nm), C.c_uint32(int(topk)), _vp(tid), _vp(ts), _vp(tc),
                                           _vp(tu) if want_thresholds else None))
        res = dict(id=tid, score=ts, count=tc[:nm])
        if want_thresholds:
            res["t_used"] = tu[:nm]
        return res

    def pssm_topk_dev(self, d_S, d_t_floor, nm, topk, d_id, d_score, d_count, d_t_used=None):
        """hs_pssm_topk_dev: device pointers (ints, e.g. tensor.data_ptr(); d_t_floor and d_t_used may be None)."""
        self._check(self._lib.hs_pssm_topk_dev(self._h, C.c_void_p(d_S), C.c_void_p(d_t_floor) if d_t_floor else None,
                                               C.c_uint64(nm), C.c_uint32(int(topk)), C.c_void_p(d_id),
                                               C.c_void_p(d_score), C.c_void_p(d_count),
                                               C.c_void_p(d_t_used) if d_t_used else None))

    def pssm_seq_scan(self, S, t, id_start, cap=None, want_counts=True):
        """hs_pssm_seq_scan: the hits of pssm_scan(S, t) reduced on the device per (profile, database sequence):
        dict(m, seq, count, best_score, best_id, lo, hi -- one row per distinct (m, seq), ascending --, n_hits[, cnt
        [nm] the hits and seq_cnt [nm] the rows per profile]).  id_start [n_seq + 1]: sequence s owns the ids
        [id_start[s], id_start[s + 1]) (capi.window_id_start for a windows index).  cap=None: two calls, the row count
        then the rows; a given cap that is too small raises HsError(HS_ERR_CAPACITY) with .needed, .n_hits and, with
        want_counts, .cnt and .seq_cnt."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        nm = S.shape[0]
        assert S.shape == (nm, self.k, self._alphabet()) and t.shape == (nm,), (S.shape, t.shape)
        if id_start is not None:
            id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
            assert id_start.ndim == 1 and len(id_start) >= 1
        n_seq = 0 if id_start is None else len(id_start) - 1
        cnt = np.zeros(nm, dtype=np.uint64) if want_counts else None
        seq_cnt = np.zeros(nm, dtype=np.uint64) if want_counts else None
        room = 0 if cap is None else int(cap)
        while True:
            arrs = _pssm_seq_rows(room)
            n, nh = C.c_uint64(0), C.c_uint64(0)
            st = self._lib.hs_pssm_seq_scan(self._h, _vp(S), _vp(t), nm, None if id_start is None else _vp(id_start),
                                            n_seq, *[_vp(a) if room else None for a in arrs], room, C.byref(n),
                                            C.byref(nh), _vp(cnt) if want_counts else None,
                                            _vp(seq_cnt) if want_counts else None)
            if st == HS_ERR_CAPACITY:
                if cap is None and int(n.value) > room:
                    room = int(n.value)
                    continue
                e = HsError(st, self._lib.hs_last_error(self._h).decode())
                e.needed, e.n_hits, e.cnt, e.seq_cnt = int(n.value), int(nh.value), cnt, seq_cnt
                raise e
            self._check(st)
            res = _pssm_seq_dict(arrs, int(n.value))
            res["n_hits"] = int(nh.value)
            if want_counts:
                res["cnt"], res["seq_cnt"] = cnt, seq_cnt
            return res

    def pssm_seq_scan_dev(self, d_S, d_t, nm, d_id_start, n_seq, d_rows, cap, d_cnt=None, d_seq_cnt=None):
        """hs_pssm_seq_scan_dev: device pointers (ints, e.g. tensor.data_ptr(); d_rows: the seven row arrays in the
        order of capi.PSSM_SEQ_FIELDS).  Returns (rows, n_hits); raises HsError(HS_ERR_CAPACITY) with the required size
        in .needed and the hit count in .n_hits when cap is too small."""
        n, nh = C.c_uint64(0), C.c_uint64(0)
        st = self._lib.hs_pssm_seq_scan_dev(self._h, d_S if d_S else None, d_t if d_t else None, int(nm),
                                            d_id_start if d_id_start else None, int(n_seq),
                                            *[p if p else None for p in d_rows], int(cap), C.byref(n), C.byref(nh),
                                            d_cnt if d_cnt else None, d_seq_cnt if d_seq_cnt else None)
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed, e.n_hits = int(n.value), int(nh.value)
            raise e
        self._check(st)
        return int(n.value), int(nh.value)

    def pssm_family_scan(self, S, t, id_start, m_group=None, m_off=None, min_count=1, t_group=None, cap=None,
                         want_counts=True, n_groups=None):
        """hs_pssm_family_scan: the hits of pssm_scan(S, t) reduced on the device per (family, database sequence,
        diagonal): dict(group, seq, diag, count, sum, best_score, best_m, best_id, lo, hi -- one row per distinct
        (group, seq, diag) that passes the filters, ascending --, n_hits[, cnt [nm] the hits per profile and grp_rows
        [n_groups] the reported rows per family]).  m_group [nm] non-decreasing (None: every profile its own family);
        m_off [nm]: a profile's offset inside its family, diag = (id - id_start[seq]) - m_off (None: no diagonals);
        a row is reported iff count >= min_count and sum >= t_group[group] (None: no sum filter).  cap=None: two
        calls, the row count then the rows; a given cap that is too small raises HsError(HS_ERR_CAPACITY) with
        .needed, .n_hits and, with want_counts, .cnt and .grp_rows."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        nm = S.shape[0]
        assert S.shape == (nm, self.k, self._alphabet()) and t.shape == (nm,), (S.shape, t.shape)
        keep, vals, n_groups = _pssm_family_args(nm, m_group, n_groups, m_off, id_start, min_count, t_group)
        cnt = np.zeros(nm, dtype=np.uint64) if want_counts else None
        grp_rows = np.zeros(n_groups, dtype=np.uint64) if want_counts else None
        room = 0 if cap is None else int(cap)
        while True:
            arrs = _pssm_family_rows(room)
            n, nh = C.c_uint64(0), C.c_uint64(0)
            st = self._lib.hs_pssm_family_scan(self._h, _vp(S), _vp(t), nm, *vals,
                                               *[_vp(a) if room else None for a in arrs], room, C.byref(n),
                                               C.byref(nh), _vp(cnt) if want_counts else None,
                                               _vp(grp_rows) if want_counts else None)
            if st == HS_ERR_CAPACITY:
                if cap is None and int(n.value) > room:
                    room = int(n.value)
                    continue
                e = HsError(st, self._lib.hs_last_error(self._h).decode())
                e.needed, e.n_hits, e.cnt, e.grp_rows = int(n.value), int(nh.value), cnt, grp_rows
                raise e
            self._check(st)
            res = _pssm_family_dict(arrs, int(n.value))
            res["n_hits"] = int(nh.value)
            if want_counts:
                res["cnt"], res["grp_rows"] = cnt, grp_rows
            return res

    def pssm_family_scan_dev(self, d_S, d_t, nm, d_m_group, n_groups, d_m_off, d_id_start, n_seq, min_count,
                             d_t_group, d_rows, cap, d_cnt=None, d_grp_rows=None):
        """hs_pssm_family_scan_dev: device pointers (ints, e.g. tensor.data_ptr(); d_m_group, d_m_off, d_t_group,
        d_cnt and d_grp_rows may be None; d_rows: the ten row arrays in the order of capi.PSSM_FAMILY_FIELDS).
        Returns (rows, n_hits); raises HsError(HS_ERR_CAPACITY) with the required size in .needed and the hit count
        in .n_hits when cap is too small."""
        n, nh = C.c_uint64(0), C.c_uint64(0)
        st = self._lib.hs_pssm_family_scan_dev(self._h, d_S if d_S else None, d_t if d_t else None, int(nm),
                                               d_m_group if d_m_group else None, int(n_groups),
                                               d_m_off if d_m_off else None, d_id_start if d_id_start else None,
                                               int(n_seq), C.c_uint32(int(min_count)),
                                               d_t_group if d_t_group else None, *[p if p else None for p in d_rows],
                                               int(cap), C.byref(n), C.byref(nh), d_cnt if d_cnt else None,
                                               d_grp_rows if d_grp_rows else None)
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed, e.n_hits = int(n.value), int(nh.value)
            raise e
        self._check(st)
        return int(n.value), int(nh.value)

    def pssm_family_chain(self, S, t, id_start, m_group, m_off, max_shift, gap_open=0.0, gap_ext=0.0, min_count=1,
                          t_group=None, cap=None, want_counts=True, n_groups=None):
        """hs_pssm_family_chain: the hits of pssm_scan(S, t) linked on the device into the best gapped chain per
        (family, database sequence): dict(group, seq, count, gaps, score, first_m, first_id, last_m, last_id, shift --
        at most one row per (group, seq), ascending --, n_hits[, cnt [nm] the hits per profile and grp_rows [n_groups]
        the reported rows per family]).  m_group [nm] non-decreasing (None: every profile its own family); m_off [nm],
        required, non-decreasing inside a family; hits of later profiles at later offsets link when their diagonals
        differ by d <= max_shift, at the cost gap_open + gap_ext * d for d >= 1; a chain is reported iff it holds
        min_count blocks and its score reaches t_group[group] (None: no score filter).  cap=None: two calls, the row
        count then the rows; a given cap that is too small raises HsError(HS_ERR_CAPACITY) with .needed, .n_hits and,
        with want_counts, .cnt and .grp_rows."""
        S = np.ascontiguousarray(S, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        nm = S.shape[0]
        assert S.shape == (nm, self.k, self._alphabet()) and t.shape == (nm,), (S.shape, t.shape)
        keep, vals, n_groups = _pssm_family_args(nm, m_group, n_groups, m_off, id_start, min_count, t_group)
        vals = _pssm_chain_vals(vals, max_shift, gap_open, gap_ext)
        cnt = np.zeros(nm, dtype=np.uint64) if want_counts else None
        grp_rows = np.zeros(n_groups, dtype=np.uint64) if want_counts else None
        room = 0 if cap is None else int(cap)
        while True:
            arrs = _pssm_chain_rows(room)
            n, nh = C.c_uint64(0), C.c_uint64(0)
            st = self._lib.hs_pssm_family_chain(self._h, _vp(S), _vp(t), nm, *vals,
                                                *[_vp(a) if room else None for a in arrs], room, C.byref(n),
                                                C.byref(nh), _vp(cnt) if want_counts else None,
                                                _vp(grp_rows) if want_counts else None)
            if st == HS_ERR_CAPACITY:
                if cap is None and int(n.value) > room:
                    room = int(n.value)
                    continue
                e = HsError(st, self._lib.hs_last_error(self._h).decode())
                e.needed, e.n_hits, e.cnt, e.grp_rows = int(n.value), int(nh.value), cnt, grp_rows
                raise e
            self._check(st)
            res = _pssm_chain_dict(arrs, int(n.value))
            res["n_hits"] = int(nh.value)
            if want_counts:
                res["cnt"], res["grp_rows"] = cnt, grp_rows
            return res

    def pssm_family_chain_dev(self, d_S, d_t, nm, d_m_group, n_groups, d_m_off, d_id_start, n_seq, max_shift, gap_open,
                              gap_ext, min_count, d_t_group, d_rows, cap, d_cnt=None, d_grp_rows=None):
        """hs_pssm_family_chain_dev: device pointers (ints, e.g. tensor.data_ptr(); d_m_group, d_t_group, d_cnt and
        d_grp_rows may be None; d_rows: the ten row arrays in the order of capi.PSSM_CHAIN_FIELDS).  Returns (rows,
        n_hits); raises HsError(HS_ERR_CAPACITY) with the required size in .needed and the hit count in .n_hits when
        cap is too small."""
        n, nh = C.c_uint64(0), C.c_uint64(0)
        st = self._lib.hs_pssm_family_chain_dev(self._h, d_S if d_S else None, d_t if d_t else None, int(nm),
                                                d_m_group if d_m_group else None, int(n_groups),
                                                d_m_off if d_m_off else None, d_id_start if d_id_start else None,
                                                int(n_seq), C.c_uint32(int(max_shift)), C.c_double(float(gap_open)),
                                                C.c_double(float(gap_ext)), C.c_uint32(int(min_count)),
                                                d_t_group if d_t_group else None, *[p if p else None for p in d_rows],
                                                int(cap), C.byref(n), C.byref(nh), d_cnt if d_cnt else None,
                                                d_grp_rows if d_grp_rows else None)
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed, e.n_hits = int(n.value), int(nh.value)
            raise e
        self._check(st)
        return int(n.value), int(nh.value)

    def _pssm_args(self, S, t, id_start):
        S = np.ascontiguousarray(S, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.float64)
        nm = S.shape[0]
        assert S.shape == (nm, self.k, self._alphabet()) and t.shape == (nm,), (S.shape, t.shape)
        if id_start is not None:
            id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
            assert id_start.ndim == 1 and len(id_start) >= 1
        return S, t, nm, id_start, 0 if id_start is None else len(id_start) - 1

    def pssm_hit_counts(self, S, t, id_start=None):
        """hs_pssm_hit_counts: the position frequency matrices of pssm_scan(S, t)'s hits, reduced on the device:
        dict(counts uint32 [nm][k][alphabet], cnt [nm] the hits and used [nm] the sites per profile, n_hits).
        id_start=None: every hit is a site; id_start [n_seq + 1]: one site per (profile, sequence), the best hit of
        pssm_seq_scan's rows."""
        S, t, nm, id_start, n_seq = self._pssm_args(S, t, id_start)
        counts = np.empty(S.shape, dtype=np.uint32)
        cnt, used = np.empty(max(nm, 1), dtype=np.uint64), np.empty(max(nm, 1), dtype=np.uint64)
        nh = C.c_uint64(0)
        self._check(self._lib.hs_pssm_hit_counts(self._h, _vp(S), _vp(t), nm, None if id_start is None else _vp(id_start),
                                                 n_seq, _vp(counts), _vp(cnt), _vp(used), C.byref(nh)))
        return dict(counts=counts, cnt=cnt[:nm], used=used[:nm], n_hits=int(nh.value))

    def pssm_hit_counts_dev(self, d_S, d_t, nm, d_counts, d_id_start=None, n_seq=0, d_cnt=None, d_used=None):
        """hs_pssm_hit_counts_dev: device pointers (ints, e.g. tensor.data_ptr(); d_id_start, d_cnt and d_used may be
        None).  Returns n_hits."""
        nh = C.c_uint64(0)
        self._check(self._lib.hs_pssm_hit_counts_dev(self._h, d_S if d_S else None, d_t if d_t else None, int(nm),
                                                     d_id_start if d_id_start else None, int(n_seq),
                                                     d_counts if d_counts else None, d_cnt if d_cnt else None,
                                                     d_used if d_used else None, C.byref(nh)))
        return int(nh.value)

    def pssm_refine(self, S, t, n_iter, id_start=None, background=None, pseudo=1.0):
        """hs_pssm_refine: scan, rebuild the profiles from the counts of their own hits (hs_pssm_log_odds), scan again
        -- until two scans count the same or n_iter scans have run.  dict(S [nm][k][alphabet] the last profiles
        computed, counts, used: of the last scan, iters, converged).  background=None: the residue composition of
        the index (one extra scan).  A profile without hits keeps its matrix."""
        S, t, nm, id_start, n_seq = self._pssm_args(S, t, id_start)
        bg = None
        if background is not None:
            bg = np.ascontiguousarray(background, dtype=np.float64)
            assert bg.shape == (self._alphabet(),), bg.shape
        S_out = np.empty(S.shape, dtype=np.float64)
        counts = np.empty(S.shape, dtype=np.uint32)
        used = np.empty(max(nm, 1), dtype=np.uint64)
        iters, conv = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.hs_pssm_refine(self._h, _vp(S), _vp(t), nm, None if id_start is None else _vp(id_start),
                                             n_seq, None if bg is None else _vp(bg), float(pseudo), int(n_iter),
                                             _vp(S_out), _vp(counts), _vp(used), C.byref(iters), C.byref(conv)))
        return dict(S=S_out, counts=counts, used=used[:nm], iters=int(iters.value), converged=bool(conv.value))

    def _pssm_rank_args(self, S, rank):
        S = np.ascontiguousarray(S, dtype=np.float64)
        nm = S.shape[0]
        assert S.shape == (nm, self.k, self._alphabet()), S.shape
        rank = np.ascontiguousarray(np.broadcast_to(np.asarray(rank, dtype=np.uint64), (nm,)))
        return S, rank, nm

    def pssm_rank(self, S, rank, want_diagnostics=False):
        """hs_pssm_rank: for every profile S [nm][k][alphabet] the exact score of its rank-th best indexed k-mer (rank:
        a scalar or [nm], each 1 .. n) -- the threshold at which pssm_scan returns the rank best k-mers and their
        ties.  dict(t [nm], cnt_ge [nm] the k-mers scoring >= t (what pssm_scan at t returns), cnt_gt [nm] those
        scoring > t[, t_scan [nm] and rounds [nm]: the threshold of the round that resolved the profile and the
        retries before it -- the outputs that depend on the "pssm_rank_sample" option])."""
        S, rank, nm = self._pssm_rank_args(S, rank)
        t = np.empty(max(nm, 1), dtype=np.float64)
        ge, gt = np.empty(max(nm, 1), dtype=np.uint64), np.empty(max(nm, 1), dtype=np.uint64)
        ts = np.empty(max(nm, 1), dtype=np.float64) if want_diagnostics else None
        ro = np.empty(max(nm, 1), dtype=np.uint32) if want_diagnostics else None
        self._check(self._lib.hs_pssm_rank(self._h, _vp(S), _vp(rank), C.c_uint64(nm), _vp(t), _vp(ge), _vp(gt),
                                           _vp(ts) if want_diagnostics else None,
                                           _vp(ro) if want_diagnostics else None))
        res = dict(t=t[:nm], cnt_ge=ge[:nm], cnt_gt=gt[:nm])
        if want_diagnostics:
            res["t_scan"], res["rounds"] = ts[:nm], ro[:nm]
        return res

    def pssm_rank_dev(self, d_S, d_rank, nm, d_t, d_cnt_ge, d_cnt_gt, d_t_scan=None, d_rounds=None):
        """hs_pssm_rank_dev: device pointers (ints, e.g. tensor.data_ptr(); d_t_scan and d_rounds may be None)."""
        self._check(self._lib.hs_pssm_rank_dev(self._h, d_S if d_S else None, d_rank if d_rank else None,
                                               C.c_uint64(int(nm)), d_t if d_t else None,
                                               d_cnt_ge if d_cnt_ge else None, d_cnt_gt if d_cnt_gt else None,
                                               d_t_scan if d_t_scan else None, d_rounds if d_rounds else None))

    def _pssm_null_in(self, S, bg, t_lo):
        S = np.ascontiguousarray(S, dtype=np.float64)
        nm = S.shape[0]
        assert S.shape == (nm, self.k, self._alphabet()), S.shape
        if bg is not None:
            bg = np.ascontiguousarray(bg, dtype=np.float64)
            assert bg.shape == (self._alphabet(),), bg.shape
        if t_lo is not None:
            t_lo = np.ascontiguousarray(np.broadcast_to(np.asarray(t_lo, dtype=np.float64), (nm,)))
        return S, nm, bg, t_lo

    def pssm_pvalue(self, S, hit_m, hit_score, bg=None, t_lo=None, want_lower=True):
        """hs_pssm_pvalue: for n hits (hit_m[i], hit_score[i]) of the profiles S [nm][k][alphabet] -- pssm_scan's, or
        any list, in any order -- the bracket p_lo <= P{a random k-mer scores >= hit_score[i]} <= p_hi under the null
        model bg [alphabet] (None: the index's residue composition, one extra scan) on a grid of "pssm_null_bins" bins
        from t_lo (None: 0; a scalar or [nm]) to each profile's maximal score.  dict(p_hi [n][, p_lo [n]]);
        want_lower=False runs the upper side alone, which halves the work."""
        S, nm, bg, t_lo = self._pssm_null_in(S, bg, t_lo)
        hit_m = np.ascontiguousarray(hit_m, dtype=np.uint32)
        hit_score = np.ascontiguousarray(hit_score, dtype=np.float64)
        n = len(hit_m)
        assert hit_m.shape == hit_score.shape == (n,)
        p_hi = np.empty(max(n, 1), np.float64)
        p_lo = np.empty(max(n, 1), np.float64) if want_lower else None
        self._check(self._lib.hs_pssm_pvalue(self._h, _vp(S), _opt(bg), _opt(t_lo), C.c_uint64(nm), _vp(hit_m),
                                             _vp(hit_score), C.c_uint64(n), _vp(p_hi), _opt(p_lo)))
        res = dict(p_hi=p_hi[:n])
        if want_lower:
            res["p_lo"] = p_lo[:n]
        return res

    def pssm_pvalue_dev(self, d_S, nm, d_hit_m, d_hit_score, n, d_p_hi, d_p_lo=None, d_bg=None, d_t_lo=None):
        """hs_pssm_pvalue_dev: device pointers (ints, e.g. tensor.data_ptr(); d_p_lo, d_bg and d_t_lo may be None) --
        the hit list pssm_scan_dev returns never crosses PCIe."""
        self._check(self._lib.hs_pssm_pvalue_dev(self._h, d_S if d_S else None, d_bg if d_bg else None,
                                                 d_t_lo if d_t_lo else None, C.c_uint64(int(nm)),
                                                 d_hit_m if d_hit_m else None, d_hit_score if d_hit_score else None,
                                                 C.c_uint64(int(n)), d_p_hi if d_p_hi else None,
                                                 d_p_lo if d_p_lo else None))

    def pssm_pvalue_threshold(self, S, p, bg=None, t_lo=None, want_lower=True):
        """hs_pssm_pvalue_threshold: per profile the threshold t of the p-value p (a scalar or [nm], each in (0, 1]) under
        the null model of pssm_pvalue: the smallest t whose p_hi is <= p on the grid -- a threshold every profile call
        accepts.  dict(t [nm], p_hi [nm][, p_lo [nm]] the bracket at t, flag uint32 [nm]: 0 exact on the grid, 1 clipped
        at t_lo (a lower t_lo might admit more), 2 nothing admissible: t = +DBL_MAX, which no k-mer reaches)."""
        S, nm, bg, t_lo = self._pssm_null_in(S, bg, t_lo)
        p = np.ascontiguousarray(np.broadcast_to(np.asarray(p, dtype=np.float64), (nm,)))
        t = np.empty(max(nm, 1), np.float64)
        p_hi = np.empty(max(nm, 1), np.float64)
        p_lo = np.empty(max(nm, 1), np.float64) if want_lower else None
        flag = np.empty(max(nm, 1), np.uint32)
        self._check(self._lib.hs_pssm_pvalue_threshold(self._h, _vp(S), _opt(bg), _opt(t_lo), _vp(p), C.c_uint64(nm),
                                                       _vp(t), _vp(p_hi), _opt(p_lo), _vp(flag)))
        res = dict(t=t[:nm], p_hi=p_hi[:nm], flag=flag[:nm])
        if want_lower:
            res["p_lo"] = p_lo[:nm]
        return res

    def pssm_pvalue_threshold_dev(self, d_S, d_p, nm, d_t, d_p_hi, d_flag, d_p_lo=None, d_bg=None, d_t_lo=None):
        """hs_pssm_pvalue_threshold_dev: device pointers (ints; d_p_lo, d_bg and d_t_lo may be None)."""
        self._check(self._lib.hs_pssm_pvalue_threshold_dev(self._h, d_S if d_S else None, d_bg if d_bg else None,
                                                           d_t_lo if d_t_lo else None, d_p if d_p else None,
                                                           C.c_uint64(int(nm)), d_t if d_t else None,
                                                           d_p_hi if d_p_hi else None, d_p_lo if d_p_lo else None,
                                                           d_flag if d_flag else None))

    def pssm_refine_rank(self, S, rank, n_iter, id_start=None, background=None, pseudo=1.0):
        """hs_pssm_refine_rank: pssm_refine with the threshold rule -- every iteration scans at the threshold that admits
        the rank best k-mers (and their ties) of the current matrix.  dict(S, t [nm] the threshold of the last scan,
        counts, used: of the last scan, iters, converged).  used may exceed rank (ties); with id_start the rank still
        counts k-mers, not proteins."""
        S, rank, nm = self._pssm_rank_args(S, rank)
        if id_start is not None:
            id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
            assert id_start.ndim == 1 and len(id_start) >= 1
        n_seq = 0 if id_start is None else len(id_start) - 1
        bg = None
        if background is not None:
            bg = np.ascontiguousarray(background, dtype=np.float64)
            assert bg.shape == (self._alphabet(),), bg.shape
        S_out = np.empty(S.shape, dtype=np.float64)
        t_out = np.empty(max(nm, 1), dtype=np.float64)
        counts = np.empty(S.shape, dtype=np.uint32)
        used = np.empty(max(nm, 1), dtype=np.uint64)
        iters, conv = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.hs_pssm_refine_rank(self._h, _vp(S), _vp(rank), nm,
                                                  None if id_start is None else _vp(id_start), n_seq,
                                                  None if bg is None else _vp(bg), float(pseudo), int(n_iter),
                                                  _vp(S_out), _vp(t_out), _vp(counts), _vp(used), C.byref(iters),
                                                  C.byref(conv)))
        return dict(S=S_out, t=t_out[:nm], counts=counts, used=used[:nm], iters=int(iters.value),
                    converged=bool(conv.value))

    def pssm_weighted_counts(self, S, t, id_start=None):
        """hs_pssm_weighted_counts: pssm_hit_counts with position-based sequence weights (Henikoff and Henikoff 1994)
        in integers, reduced on the device: dict(counts uint32 and wcounts uint64 [nm][k][alphabet], wsum uint64 [nm]
        (every column of wcounts[m] sums to it; at most k * 2^56), distinct uint32 [nm] (the residues that occur,
        summed over the positions), cnt, used, n_hits).  The sites are pssm_hit_counts'."""
        S, t, nm, id_start, n_seq = self._pssm_args(S, t, id_start)
        counts, wcounts = np.empty(S.shape, dtype=np.uint32), np.empty(S.shape, dtype=np.uint64)
        wsum, cnt, used = (np.empty(max(nm, 1), dtype=np.uint64) for _ in range(3))
        distinct = np.empty(max(nm, 1), dtype=np.uint32)
        nh = C.c_uint64(0)
        self._check(self._lib.hs_pssm_weighted_counts(self._h, _vp(S), _vp(t), nm,
                                                      None if id_start is None else _vp(id_start), n_seq, _vp(counts),
                                                      _vp(wcounts), _vp(wsum), _vp(distinct), _vp(cnt), _vp(used),
                                                      C.byref(nh)))
        return dict(counts=counts, wcounts=wcounts, wsum=wsum[:nm], distinct=distinct[:nm], cnt=cnt[:nm],
                    used=used[:nm], n_hits=int(nh.value))

    def pssm_weighted_counts_dev(self, d_S, d_t, nm, d_wcounts, d_id_start=None, n_seq=0, d_counts=None, d_wsum=None,
                                 d_distinct=None, d_cnt=None, d_used=None):
        """hs_pssm_weighted_counts_dev: device pointers (ints, e.g. tensor.data_ptr(); all but d_S, d_t and d_wcounts
        may be None).  Returns n_hits."""
        nh = C.c_uint64(0)
        self._check(self._lib.hs_pssm_weighted_counts_dev(
            self._h, d_S if d_S else None, d_t if d_t else None, int(nm), d_id_start if d_id_start else None,
            int(n_seq), d_counts if d_counts else None, d_wcounts if d_wcounts else None, d_wsum if d_wsum else None,
            d_distinct if d_distinct else None, d_cnt if d_cnt else None, d_used if d_used else None, C.byref(nh)))
        return int(nh.value)

    def pssm_refine_weighted(self, S, n_iter, t=None, rank=None, id_start=None, background=None, pseudo=1.0,
                             neff="sites"):
        """hs_pssm_refine_weighted: pssm_refine (t given) or pssm_refine_rank (rank given) -- exactly one of them --
        with every scan's sites weighted (pssm_weighted_counts) and the log-odds taken from the weighted frequencies
        at n_eff observations: neff="sites": used[m]; "columns": distinct[m] / k.  Converged when counts and wcounts
        both repeat.  dict(S, t (rank given), counts, wcounts, wsum, distinct, used: of the last scan, iters,
        converged)."""
        assert (t is None) != (rank is None), "exactly one of t and rank"
        rule = {"sites": 0, "columns": 1}[neff]
        if rank is None:
            S, v, nm = self._pssm_args(S, t, None)[:3]
        else:
            S, v, nm = self._pssm_rank_args(S, rank)
        if id_start is not None:
            id_start = np.ascontiguousarray(id_start, dtype=np.uint64)
            assert id_start.ndim == 1 and len(id_start) >= 1
        n_seq = 0 if id_start is None else len(id_start) - 1
        bg = None
        if background is not None:
            bg = np.ascontiguousarray(background, dtype=np.float64)
            assert bg.shape == (self._alphabet(),), bg.shape
        S_out = np.empty(S.shape, dtype=np.float64)
        t_out = np.empty(max(nm, 1), dtype=np.float64)
        counts, wcounts = np.empty(S.shape, dtype=np.uint32), np.empty(S.shape, dtype=np.uint64)
        wsum, used = np.empty(max(nm, 1), dtype=np.uint64), np.empty(max(nm, 1), dtype=np.uint64)
        distinct = np.empty(max(nm, 1), dtype=np.uint32)
        iters, conv = C.c_uint32(0), C.c_uint32(0)
        self._check(self._lib.hs_pssm_refine_weighted(
            self._h, _vp(S), None if rank is not None else _vp(v), None if rank is None else _vp(v), nm,
            None if id_start is None else _vp(id_start), n_seq, None if bg is None else _vp(bg), float(pseudo), rule,
            int(n_iter), _vp(S_out), _vp(t_out), _vp(counts), _vp(wcounts), _vp(wsum), _vp(distinct), _vp(used),
            C.byref(iters), C.byref(conv)))
        res = dict(S=S_out, counts=counts, wcounts=wcounts, wsum=wsum[:nm], distinct=distinct[:nm], used=used[:nm],
                   iters=int(iters.value), converged=bool(conv.value))
        if rank is not None:
            res["t"] = t_out[:nm]
        return res

    def bruteforce_radii(self, centers, radii, cap=None):
        """hs_bruteforce_radii: brute force with centre q searched at radii[q]."""
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        radii = np.ascontiguousarray(radii, dtype=np.float64)
        nq = centers.shape[0]
        assert centers.shape == (nq, self.d) and radii.shape == (nq,)
        cap = int(cap) if cap is not None else max(1024, 64 * nq)
        while True:
            hq = np.empty(cap, dtype=np.uint32)
            hid = np.empty(cap, dtype=np.uint32)
            hd = np.empty(cap, dtype=np.float64)
            n = C.c_uint64(0)
            st = self._lib.hs_bruteforce_radii(self._h, _vp(centers), nq, _vp(radii), _vp(hq), _vp(hid), _vp(hd),
                                               cap, C.byref(n))
            if st == HS_ERR_CAPACITY:
                cap = int(n.value)
                continue
            self._check(st)
            n = int(n.value)
            return dict(q=hq[:n], id=hid[:n], dist=hd[:n])

    def bruteforce_topk(self, centers, topk):
        """Exact k nearest DB k-mers per query: (ids [nq][topk], squared distances [nq][topk]),
        ordered by (d2, id); ground truth of recall@k."""
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        nq = centers.shape[0]
        nn = np.empty((nq, topk), dtype=np.uint32)
        d2 = np.empty((nq, topk), dtype=np.float64)
        self._check(self._lib.hs_bruteforce_topk(self._h, _vp(centers), C.c_uint64(nq),
                                                 C.c_uint32(topk), _vp(nn), _vp(d2)))
        return nn, d2

    # -- a12
    def self_join(self, R, sqrt_test=True, cap=None, first=0, count=None):
        """All ordered within-bucket pairs (i, j), i != j, within R: dict(i, j, table, dist);
        first/count restrict the i side to a block of the indexed k-mers (one rank's shard)."""
        cap = int(cap) if cap is not None else 1 << 16
        count = self.index_info()["n"] - first if count is None else count
        while True:
            ei = np.empty(cap, dtype=np.uint32)
            ej = np.empty(cap, dtype=np.uint32)
            et = np.empty(cap, dtype=np.uint32)
            ed = np.empty(cap, dtype=np.float64)
            n = C.c_uint64(0)
            st = self._lib.hs_self_join_range(self._h, C.c_uint64(first), C.c_uint64(count),
                                              C.c_double(R), C.c_int(1 if sqrt_test else 0),
                                              _vp(ei), _vp(ej), _vp(et), _vp(ed), C.c_uint64(cap),
                                              C.byref(n))
            if st == HS_ERR_CAPACITY:
                cap = int(n.value)
                continue
            self._check(st)
            n = int(n.value)
            return dict(i=ei[:n], j=ej[:n], table=et[:n], dist=ed[:n])

    def components(self, R, sqrt_test=True, first=0, count=None):
        """hs_components / hs_components_range: the connected components of the graph self_join(R, sqrt_test, first,
        count) returns, united on the device: dict(label uint32 [n] = the smallest id of every k-mer's component,
        n_components, n_edges = len(self_join(...)["i"]))."""
        info = _IndexInfo()
        n = int(info.n) if self._lib.hs_index_info_get(self._h, C.byref(info)) == HS_OK else 0
        count = n - first if count is None else count
        label = np.empty(n, dtype=np.uint32)
        nc, ne = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.hs_components_range(self._h, first, count, float(R), 1 if sqrt_test else 0, _vp(label),
                                                  C.byref(nc), C.byref(ne)))
        return dict(label=label, n_components=int(nc.value), n_edges=int(ne.value))

    def components_dev(self, d_label_ptr, R, sqrt_test=True):
        """hs_components_dev: the labels into uint32 [n] device memory (pointer as int); (n_components, n_edges)."""
        nc, ne = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.hs_components_dev(self._h, float(R), 1 if sqrt_test else 0, d_label_ptr, C.byref(nc),
                                                C.byref(ne)))
        return int(nc.value), int(ne.value)

    def _n(self):
        info = _IndexInfo()
        return int(info.n) if self._lib.hs_index_info_get(self._h, C.byref(info)) == HS_OK else 0

    def degrees(self, R, sqrt_test=True, first=0, count=None):
        """hs_degrees / hs_degrees_range: uint32 [n], the number of distinct neighbours of every k-mer in the graph
        self_join(R, sqrt_test, first, count) returns, counted on the device: np.bincount(self_join(...)["i"])."""
        n = self._n()
        count = n - first if count is None else count
        degree = np.empty(n, dtype=np.uint32)
        ne = C.c_uint64(0)
        self._check(self._lib.hs_degrees_range(self._h, first, count, float(R), 1 if sqrt_test else 0, _vp(degree),
                                               C.byref(ne)))
        return degree

    def degrees_dev(self, d_degree_ptr, R, sqrt_test=True, first=0, count=None):
        """hs_degrees_range_dev: the degrees into uint32 [n] device memory (pointer as int); returns n_edges."""
        count = self._n() - first if count is None else count
        ne = C.c_uint64(0)
        self._check(self._lib.hs_degrees_range_dev(self._h, first, count, float(R), 1 if sqrt_test else 0,
                                                   d_degree_ptr, C.byref(ne)))
        return int(ne.value)

    def dbscan(self, R, min_pts, sqrt_test=True, want_degree=False):
        """hs_dbscan: the density clusters of the graph self_join(R, sqrt_test) returns, reduced on the device:
        dict(label uint32 [n] -- the smallest core id of the cluster, capi.NOISE for noise --, degree if asked,
        n_clusters, n_core, n_border, n_noise, n_edges).  A k-mer is core with degree + 1 >= min_pts; a border
        k-mer takes the label of its core neighbour with the smallest id."""
        n = self._n()
        label = np.empty(n, dtype=np.uint32)
        degree = np.empty(n, dtype=np.uint32) if want_degree else None
        c = _DbscanCounts()
        self._check(self._lib.hs_dbscan(self._h, float(R), 1 if sqrt_test else 0, int(min_pts), _vp(label),
                                        _vp(degree) if want_degree else None, C.byref(c)))
        res = dict(label=label, **_counts_dict(c))
        if want_degree:
            res["degree"] = degree
        return res

    def dbscan_dev(self, d_label_ptr, R, min_pts, sqrt_test=True, d_degree_ptr=None):
        """hs_dbscan_dev: the labels (and, with d_degree_ptr, the degrees) into uint32 [n] device memory (pointers as
        ints); returns the dict of the five counts."""
        c = _DbscanCounts()
        self._check(self._lib.hs_dbscan_dev(self._h, float(R), 1 if sqrt_test else 0, int(min_pts), d_label_ptr,
                                            d_degree_ptr, C.byref(c)))
        return _counts_dict(c)

    def msf(self, R, sqrt_test=True, want_label=False):
        """hs_msf: the minimum spanning forest -- the single-linkage tree up to R -- of the graph self_join(R, sqrt_test)
        returns, found on the device: dict(lo, hi, dist: the n - n_components tree edges in ascending (dist, lo, hi)
        = the merge order, lo < hi; label (= components(R, sqrt_test)["label"]) if asked; n_tree_edges, n_components,
        n_graph_edges = len(self_join(...)["i"]), rounds, resident).  capi.msf_cut(tree, r) cuts it at a radius."""
        n = self._n()
        lo = np.empty(n, dtype=np.uint32)
        hi = np.empty(n, dtype=np.uint32)
        dist = np.empty(n, dtype=np.float64)
        label = np.empty(n, dtype=np.uint32) if want_label else None
        info = _MsfInfo()
        self._check(self._lib.hs_msf(self._h, float(R), 1 if sqrt_test else 0, _vp(lo), _vp(hi), _vp(dist), n,
                                     _vp(label) if want_label else None, C.byref(info)))
        return _msf_dict(info, lo, hi, dist, label)

    def msf_dev(self, d_lo_ptr, d_hi_ptr, d_dist_ptr, cap, R, sqrt_test=True, d_label_ptr=None):
        """hs_msf_dev: the tree edges into uint32 / uint32 / float64 [cap] device memory and, with d_label_ptr, the labels
        into uint32 [n] (pointers as ints); returns the dict of the counts (n_tree_edges, ...).  A cap that is too small
        raises HsError(HS_ERR_CAPACITY) with the required size in .needed; none of the arrays, the labels included, is
        written then."""
        info = _MsfInfo()
        st = self._lib.hs_msf_dev(self._h, float(R), 1 if sqrt_test else 0, d_lo_ptr, d_hi_ptr, d_dist_ptr, int(cap),
                                  d_label_ptr, C.byref(info))
        if st != HS_OK:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(info.n_tree_edges)
            raise e
        return {f[0]: int(getattr(info, f[0])) for f in _MsfInfo._fields_}

    def core_distance(self, R, min_pts, sqrt_test=True):
        """hs_core_distance: dict(core float64 [n] -- the (min_pts - 1)-th smallest neighbour distance of every k-mer in
        the graph self_join(R, sqrt_test) returns, with multiplicity; 0 for min_pts = 1, inf with fewer neighbours --,
        n_core = the finite ones, n_edges), settled on the device in one self-join."""
        n = self._n()
        core = np.empty(n, dtype=np.float64)
        nc, ne = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.hs_core_distance(self._h, float(R), 1 if sqrt_test else 0, int(min_pts), _vp(core),
                                               C.byref(nc), C.byref(ne)))
        return dict(core=core, n_core=int(nc.value), n_edges=int(ne.value))

    def core_distance_dev(self, d_core_ptr, R, min_pts, sqrt_test=True):
        """hs_core_distance_dev: the core distances into float64 [n] device memory (pointer as int); (n_core, n_edges)."""
        nc, ne = C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.hs_core_distance_dev(self._h, float(R), 1 if sqrt_test else 0, int(min_pts), d_core_ptr,
                                                   C.byref(nc), C.byref(ne)))
        return int(nc.value), int(ne.value)

    def self_knn(self, R, topk, sqrt_test=True, first=0, count=None):
        """hs_self_knn / hs_self_knn_range: the k-nearest-neighbour graph within R -- per k-mer first + t the topk
        smallest, under (dist, id), of its edges in self_join(R, sqrt_test, first, count), selected on the device:
        dict(id, table, dist [count][topk] -- unused entries capi.NO_ID, capi.NO_ID, inf --, count uint32 [count] = the
        k-mer's degree (degrees()), n_edges).  dist[:, m - 2] is core_distance(R, m)["core"] for 2 <= m <= topk + 1."""
        count = self._n() - first if count is None else count
        topk = int(topk)
        rows = max(0, min(topk, TOPK_MAX))
        nid = np.empty((count, rows), dtype=np.uint32)
        nt = np.empty((count, rows), dtype=np.uint32)
        nd = np.empty((count, rows), dtype=np.float64)
        cnt = np.empty(count, dtype=np.uint32)
        ne = C.c_uint64(0)
        self._check(self._lib.hs_self_knn_range(self._h, first, count, float(R), 1 if sqrt_test else 0, topk, _vp(nid),
                                                _vp(nt), _vp(nd), _vp(cnt), C.byref(ne)))
        return dict(id=nid, table=nt, dist=nd, count=cnt, n_edges=int(ne.value))

    def self_knn_dev(self, d_id, d_table, d_dist, d_count, R, topk, sqrt_test=True, first=0, count=None):
        """hs_self_knn_range_dev: the rows into uint32 / uint32 / float64 [count][topk] and the degrees into uint32 [count]
        device memory (pointers as ints; d_table may be None); returns n_edges."""
        count = self._n() - first if count is None else count
        ne = C.c_uint64(0)
        self._check(self._lib.hs_self_knn_range_dev(self._h, first, count, float(R), 1 if sqrt_test else 0, int(topk),
                                                    d_id, d_table if d_table else None, d_dist, d_count, C.byref(ne)))
        return int(ne.value)

    def density_tree(self, R, min_pts, sqrt_test=True, want_label=True):
        """hs_density_tree: DBSCAN* at every radius up to R -- the minimum spanning forest of the graph self_join(R,
        sqrt_test) under the mutual-reachability weight w = max(core[a], core[b], dist), found on the device:
        dict(lo, hi, w: the n_core - n_clusters tree edges in ascending (w, lo, hi); core float64 [n]; label if asked
        (= dbscan(R, min_pts)'s on its core k-mers, capi.NOISE elsewhere: border k-mers are noise); n_tree_edges,
        n_clusters, n_core, n_graph_edges, rounds, resident, self_joins).  capi.density_tree_cut(tree, r) cuts it."""
        n = self._n()
        lo = np.empty(n, dtype=np.uint32)
        hi = np.empty(n, dtype=np.uint32)
        w = np.empty(n, dtype=np.float64)
        core = np.empty(n, dtype=np.float64)
        label = np.empty(n, dtype=np.uint32) if want_label else None
        info = _DensityInfo()
        self._check(self._lib.hs_density_tree(self._h, float(R), 1 if sqrt_test else 0, int(min_pts), _vp(lo), _vp(hi),
                                              _vp(w), n, _vp(label) if want_label else None, _vp(core),
                                              C.byref(info)))
        return _density_dict(info, lo, hi, w, label, core)

    def density_tree_dev(self, d_lo_ptr, d_hi_ptr, d_w_ptr, cap, R, min_pts, sqrt_test=True, d_label_ptr=None,
                         d_core_ptr=None):
        """hs_density_tree_dev: the tree edges into uint32 / uint32 / float64 [cap] device memory and, where given, the
        labels into uint32 [n] and the core distances into float64 [n] (pointers as ints); returns the dict of the
        counts.  A cap that is too small raises HsError(HS_ERR_CAPACITY) with the required size in .needed; none of
        the arrays is written then."""
        info = _DensityInfo()
        st = self._lib.hs_density_tree_dev(self._h, float(R), 1 if sqrt_test else 0, int(min_pts), d_lo_ptr, d_hi_ptr,
                                           d_w_ptr, int(cap), d_label_ptr, d_core_ptr, C.byref(info))
        if st != HS_OK:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(info.n_tree_edges)
            raise e
        return {f[0]: int(getattr(info, f[0])) for f in _DensityInfo._fields_}

    def cluster_profile(self, label, min_size=1, want_counts=False, cap=None):
        """hs_cluster_profile: the clusters of label uint32 [n] (NOISE or a value < n: the labels of components(),
        dbscan() or clustering()'s owner) with at least min_size members, in ascending label, summarised on the
        device: dict(label, size, centroid float64 [rows][d], counts uint32 [rows][k][alphabet] if asked)."""
        label = np.ascontiguousarray(label, dtype=np.uint32)
        n = self._n()
        assert label.shape == (n,)
        p = _Params()
        self._check(self._lib.hs_get_params(self._h, C.byref(p)))
        cap = n // max(1, int(min_size)) if cap is None else int(cap)
        ol = np.empty(cap, dtype=np.uint32)
        osz = np.empty(cap, dtype=np.uint32)
        cen = np.empty((cap, self.d), dtype=np.float64)
        cnt = np.empty((cap, self.k, int(p.alphabet)), dtype=np.uint32) if want_counts else None
        n_out = C.c_uint64(0)
        st = self._lib.hs_cluster_profile(self._h, _vp(label), int(min_size), _vp(ol), _vp(osz),
                                          _vp(cnt) if want_counts else None, _vp(cen), cap, C.byref(n_out))
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n_out.value)
            raise e
        self._check(st)
        m = int(n_out.value)
        res = dict(label=ol[:m], size=osz[:m], centroid=cen[:m])
        if want_counts:
            res["counts"] = cnt[:m]
        return res

    def cluster_radii(self, label, centers, min_size=1):
        """hs_cluster_radii: per row of cluster_profile(label, min_size) and its centre centers[row] (any points
        [rows][d]): dict(max_d2 = the largest member d2, radius = the smallest double whose square covers it, medoid =
        the member smallest under (d2, id))."""
        label = np.ascontiguousarray(label, dtype=np.uint32)
        centers = np.ascontiguousarray(centers, dtype=np.float64)
        rows = centers.shape[0]
        assert label.shape == (self._n(),) and centers.shape == (rows, self.d)
        mx = np.empty(rows, dtype=np.float64)
        rad = np.empty(rows, dtype=np.float64)
        med = np.empty(rows, dtype=np.uint32)
        self._check(self._lib.hs_cluster_radii(self._h, _vp(label), int(min_size), _vp(centers), rows, _vp(mx),
                                               _vp(rad), _vp(med)))
        return dict(max_d2=mx, radius=rad, medoid=med)

    def cluster_summary(self, label, min_size=1, want_counts=False):
        """cluster_profile, then cluster_radii against its centroids, as one dict."""
        res = self.cluster_profile(label, min_size, want_counts=want_counts)
        res.update(self.cluster_radii(label, res["centroid"], min_size))
        return res

    def cluster_profile_dev(self, d_label_ptr, min_size, d_out_label, d_out_size, d_counts, d_centroid, cap):
        """hs_cluster_profile_dev (device pointers as ints; d_counts None or 0: no counts).  Returns the number of
        rows; raises HsError(HS_ERR_CAPACITY) with the required size in .needed when cap is too small."""
        n_out = C.c_uint64(0)
        st = self._lib.hs_cluster_profile_dev(self._h, d_label_ptr, int(min_size), d_out_label, d_out_size,
                                              d_counts if d_counts else None, d_centroid, cap, C.byref(n_out))
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n_out.value)
            raise e
        self._check(st)
        return int(n_out.value)

    def cluster_radii_dev(self, d_label_ptr, min_size, d_centers, n_rows, d_max_d2, d_radius, d_medoid):
        """hs_cluster_radii_dev (device pointers as ints)."""
        self._check(self._lib.hs_cluster_radii_dev(self._h, d_label_ptr, int(min_size), d_centers, int(n_rows),
                                                   d_max_d2, d_radius, d_medoid))

    def cluster_weighted_profile(self, label, min_size=1, want_counts=False, cap=None):
        """hs_cluster_weighted_profile: the rows of cluster_profile(label, min_size) with position-based sequence
        weights (the rule of pssm_weighted_counts, the sites of a row being its members), reduced on the device:
        dict(label, size, wcounts uint64 [rows][k][alphabet], wsum uint64 [rows] (every column of wcounts[row] sums to
        it), distinct uint32 [rows], counts uint32 [rows][k][alphabet] if asked)."""
        label = np.ascontiguousarray(label, dtype=np.uint32)
        n = self._n()
        assert label.shape == (n,)
        A = self._alphabet()
        cap = n // max(1, int(min_size)) if cap is None else int(cap)
        ol, osz = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
        wc = np.empty((cap, self.k, A), dtype=np.uint64)
        ws, di = np.empty(cap, dtype=np.uint64), np.empty(cap, dtype=np.uint32)
        cnt = np.empty((cap, self.k, A), dtype=np.uint32) if want_counts else None
        n_out = C.c_uint64(0)
        st = self._lib.hs_cluster_weighted_profile(self._h, _vp(label), int(min_size), _vp(ol), _vp(osz),
                                                   _vp(cnt) if want_counts else None, _vp(wc), _vp(ws), _vp(di), cap,
                                                   C.byref(n_out))
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n_out.value)
            raise e
        self._check(st)
        m = int(n_out.value)
        res = dict(label=ol[:m], size=osz[:m], wcounts=wc[:m], wsum=ws[:m], distinct=di[:m])
        if want_counts:
            res["counts"] = cnt[:m]
        return res

    def cluster_weighted_profile_dev(self, d_label_ptr, min_size, d_out_label, d_out_size, d_counts, d_wcounts, d_wsum,
                                     d_distinct, cap):
        """hs_cluster_weighted_profile_dev (device pointers as ints; d_counts, d_wsum, d_distinct None or 0: not
        wanted).  Returns the number of rows; raises HsError(HS_ERR_CAPACITY) with the required size in .needed when
        cap is too small."""
        n_out = C.c_uint64(0)
        st = self._lib.hs_cluster_weighted_profile_dev(self._h, d_label_ptr, int(min_size), d_out_label, d_out_size,
                                                       d_counts if d_counts else None, d_wcounts,
                                                       d_wsum if d_wsum else None, d_distinct if d_distinct else None,
                                                       cap, C.byref(n_out))
        if st == HS_ERR_CAPACITY:
            e = HsError(st, self._lib.hs_last_error(self._h).decode())
            e.needed = int(n_out.value)
            raise e
        self._check(st)
        return int(n_out.value)

    def cluster_pssm_cover(self, label, S, min_size=1):
        """hs_cluster_pssm_cover: per row of cluster_profile(label, min_size) and its profile S[row] ([rows][k][alphabet])
        dict(min_score = the smallest pssm_scan score of the row's members under S[row], argmin = the member attaining
        it, the smallest id among ties).  pssm_scan(S, min_score) returns every member of row r under profile r."""
        label = np.ascontiguousarray(label, dtype=np.uint32)
        S = np.ascontiguousarray(S, dtype=np.float64)
        rows = S.shape[0]
        assert label.shape == (self._n(),) and S.shape == (rows, self.k, self._alphabet()), S.shape
        ms, am = np.empty(rows, dtype=np.float64), np.empty(rows, dtype=np.uint32)
        self._check(self._lib.hs_cluster_pssm_cover(self._h, _vp(label), int(min_size), _vp(S), rows, _vp(ms), _vp(am)))
        return dict(min_score=ms, argmin=am)

    def cluster_pssm_cover_dev(self, d_label_ptr, min_size, d_S, n_rows, d_min_score, d_argmin):
        """hs_cluster_pssm_cover_dev (device pointers as ints)."""
        self._check(self._lib.hs_cluster_pssm_cover_dev(self._h, d_label_ptr, int(min_size), d_S, int(n_rows),
                                                        d_min_score, d_argmin))

    def index_composition(self):
        """The residue composition [alphabet] of the index as hs_pssm_refine takes it: the counts of one profile that
        hits every k-mer (one scan), through hs_pssm_background."""
        zero = np.zeros((1, self.k, self._alphabet()), dtype=np.float64)
        return pssm_background(self.pssm_hit_counts(zero, np.zeros(1))["counts"][0])

    def cluster_pssm(self, label, min_size=1, weights="sites", bg=None, pseudo=1.0, threshold="cover"):
        """From clusters to profiles pssm_scan can be given, in one call: the rows of cluster_profile(label, min_size)
        -> dict(label, size, counts, S float64 [rows][k][alphabet][, t [rows]][, wcounts, wsum, distinct]).
        weights: "none": S = hs_pssm_log_odds(counts); "sites" / "columns": S = hs_pssm_log_odds_weighted(wcounts, wsum,
        n_eff) of cluster_weighted_profile with n_eff = size / distinct / k.  bg [alphabet] (None: index_composition()),
        pseudo: the log-odds'.  threshold: "cover": t = cluster_pssm_cover's min_score (every member of a row is a hit
        of its profile at t); "rank": t = pssm_rank(S, rank = size); None: no t."""
        assert weights in ("none", "sites", "columns") and threshold in ("cover", "rank", None)
        if weights == "none":
            res = self.cluster_profile(label, min_size, want_counts=True)
            del res["centroid"]
        else:
            res = self.cluster_weighted_profile(label, min_size, want_counts=True)
        bg = self.index_composition() if bg is None else np.ascontiguousarray(bg, dtype=np.float64)
        if weights == "none":
            res["S"] = pssm_log_odds_exact(res["counts"], bg, pseudo)
        else:
            n_eff = (res["size"].astype(np.float64) if weights == "sites"
                     else res["distinct"].astype(np.float64) / np.float64(self.k))
            res["S"] = pssm_log_odds_weighted(res["wcounts"], res["wsum"], n_eff, bg, pseudo)
        rows = len(res["label"])
        if threshold == "cover":
            res["t"] = self.cluster_pssm_cover(label, res["S"], min_size)["min_score"]
        elif threshold == "rank":
            res["t"] = (self.pssm_rank(res["S"], res["size"].astype(np.uint64))["t"] if rows
                        else np.empty(0, dtype=np.float64))
        return res


def clustering(k, K, L, W, a, b, codes, R, device=0, coords=None):
    """Clustering() of hclust2.cpp:86-151 on the GPU path: (merged, owner, absorbed_table)."""
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    n = codes.shape[0]
    assert a.shape == (L, K, 8 * k) and b.shape == (L, K) and codes.shape == (n, k)
    cptr, alpha = None, 0
    if coords is not None:
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        cptr, alpha = _vp(coords), coords.shape[0]
    params = _Params(int(k), int(K), int(L), float(W), int(device), alpha)
    merged = np.empty(n, dtype=np.uint8)
    owner = np.empty(n, dtype=np.uint32)
    table = np.empty(n, dtype=np.uint32)
    err = C.create_string_buffer(512)
    st = lib.hs_clustering(C.byref(params), _vp(a), _vp(b), cptr, _vp(codes), C.c_uint64(n),
                           C.c_double(R), _vp(merged), _vp(owner), _vp(table), err, C.c_uint32(512))
    if st != HS_OK:
        raise HsError(st, err.value.decode())
    return merged, owner, table


class ClusterState:
    """Clustering() table by table (hs_clustering_begin/.../end): the form the multi-GPU driver
    (hsearch_amd.dist.clustering_sharded) uses; one GPU with world=1 equals clustering()."""

    def __init__(self, k, K, L, W, a, b, codes, R, device=0, coords=None):
        self._lib = load()
        self._a = np.ascontiguousarray(a, dtype=np.float64)
        self._b = np.ascontiguousarray(b, dtype=np.float64)
        self._codes = np.ascontiguousarray(codes, dtype=np.uint8)   # kept alive: the state borrows it
        self.n = self._codes.shape[0]
        self.L = int(L)
        assert self._a.shape == (L, K, 8 * k) and self._b.shape == (L, K) and self._codes.shape == (self.n, k)
        cptr, alpha = None, 0
        if coords is not None:
            coords = np.ascontiguousarray(coords, dtype=np.float64)
            cptr, alpha = _vp(coords), coords.shape[0]
        params = _Params(int(k), int(K), int(L), float(W), int(device), alpha)
        self._st = C.c_void_p()
        self._err = C.create_string_buffer(512)
        st = self._lib.hs_clustering_begin(C.byref(params), _vp(self._a), _vp(self._b), cptr,
                                           _vp(self._codes), C.c_uint64(self.n), C.c_double(R),
                                           C.byref(self._st), self._err, C.c_uint32(512))
        if st != HS_OK:
            raise HsError(st, self._err.value.decode())
        self._cap = 4 * self.n + 1024

    def table_edges(self, l, rank=0, world=1):
        """This rank's share of table l's within-bucket pairs within R: (i, j, dist), original ids."""
        while True:
            ei = np.empty(self._cap, dtype=np.uint32)
            ej = np.empty(self._cap, dtype=np.uint32)
            ed = np.empty(self._cap, dtype=np.float64)
            n = C.c_uint64(0)
            st = self._lib.hs_clustering_table_edges(self._st, C.c_uint32(l), C.c_uint32(rank),
                                                     C.c_uint32(world), _vp(ei), _vp(ej), _vp(ed),
                                                     C.c_uint64(self._cap), C.byref(n), self._err,
                                                     C.c_uint32(512))
            if st == HS_ERR_CAPACITY:
                self._cap = int(n.value)
                continue
            if st != HS_OK:
                raise HsError(st, self._err.value.decode())
            n = int(n.value)
            return ei[:n], ej[:n], ed[:n]

    def table_apply(self, l, edge_i, edge_j):
        """The greedy pass of table l over ALL ranks' edges (any order); host only."""
        edge_i = np.ascontiguousarray(edge_i, dtype=np.uint32)
        edge_j = np.ascontiguousarray(edge_j, dtype=np.uint32)
        assert edge_i.shape == edge_j.shape
        st = self._lib.hs_clustering_table_apply(self._st, C.c_uint32(l), _vp(edge_i), _vp(edge_j),
                                                 C.c_uint64(edge_i.shape[0]))
        if st != HS_OK:
            raise HsError(st, "hs_clustering_table_apply")

    def end(self):
        """(merged, owner, absorbed_table); frees the state."""
        merged = np.empty(self.n, dtype=np.uint8)
        owner = np.empty(self.n, dtype=np.uint32)
        table = np.empty(self.n, dtype=np.uint32)
        st, self._st = self._st, None
        rc = self._lib.hs_clustering_end(st, _vp(merged), _vp(owner), _vp(table))
        if rc != HS_OK:
            raise HsError(rc, "hs_clustering_end")
        return merged, owner, table

    def __del__(self):
        if getattr(self, "_st", None):
            self._lib.hs_clustering_end(self._st, None, None, None)
            self._st = None


def clusters_file_text(merged, owner, table, names=None):
    """The reference's clusters file (hclust2.cpp:137-150) from hs_clustering's outputs."""
    n = len(merged)
    members = {}
    order = np.lexsort((np.arange(n), table.astype(np.int64)))
    for i in order:
        if merged[i] == 2:
            members.setdefault(int(owner[i]), []).append(int(i))
    out, cid = [], 0
    for i in range(n):
        if merged[i] in (0, 1):
            ids = [i] + members.get(i, [])
            out.append("#clusterid:%d:size%d" % (cid, len(ids)))
            out.extend(str(j) if names is None else names[j] for j in ids)
            cid += 1
    return "\n".join(out) + "\n"
