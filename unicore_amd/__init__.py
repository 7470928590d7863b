"""unicore_amd — ctypes binding of libunicore_cluster.so (the MI355X-native `unicore cluster` engine).

The library is the product; this module only mirrors its C ABI (include/unicore_cluster.h) for Python
callers (tests, bench.py).  There is no Python or CPU
fallback: if the HIP library cannot be loaded, importing `lib()` raises, and on a machine without a
GPU every compute call returns UC_ERR_DEVICE.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libunicore_cluster.so")

UC_OK, UC_ERR_GENERIC, UC_ERR_ARGS, UC_ERR_IO, UC_ERR_DEVICE = 0, 1, 2, 3, 4
NSTAGE = 8
PHASES = ("prefilter", "exchange_lists_to_home", "merge_at_home", "exchange_pairs_to_owner", "install_owned", "gapped", "edge_gather", "rank0_serial_cover")
STAGES = ("load", "index", "kmer", "ungapped", "select", "gapped", "setcover", "output")


class UcOpts(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("threads", C.c_int32), ("verbosity", C.c_int32), ("device", C.c_int32),
                ("num_gpus", C.c_int32), ("cluster_options", C.c_char_p), ("data_dir", C.c_char_p)]


class UcStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "n_seqs", "n_residues", "n_index_entries", "n_sim_kmers", "n_kmer_hits", "n_candidates", "n_prefilter_hits",
        "n_gapped_alignments", "n_start_alignments", "n_pk_reruns", "n_edges", "n_clusters", "cells_fwd", "cells_rev", "cells_start")] + [
        ("algorithmic_bytes", C.c_uint64 * NSTAGE), ("stage_seconds", C.c_double * NSTAGE),
        ("sw_kernel_ms", C.c_double), ("sw_kernel_launches", C.c_uint64), ("sw_algorithmic_bytes", C.c_uint64),
        ("prefilter_kernel_ms", C.c_double), ("n_filtered_hits", C.c_uint64), ("n_sw_runs", C.c_uint64),
        ("cells_run", C.c_uint64), ("exchange_seconds", C.c_double), ("exchange_bytes", C.c_uint64),
        ("n_gpus", C.c_uint32), ("target_shards", C.c_uint32), ("phase_seconds", C.c_double * 8),
        ("nccl_ranks", C.c_uint32), ("reserved0", C.c_uint32), ("exchange2_seconds", C.c_double * 4), ("cells_tb", C.c_uint64)]

    def as_dict(self):
        d = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            d[name] = list(v) if hasattr(v, "__len__") else v
        return d


class UcTreeStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_groups", "n_rows", "n_pairs_scored", "n_rows_unaligned", "n_columns", "n_columns_kept", "n_groups_dropped")] + [
        ("seconds", C.c_double * 7)]


TREE_PHASES = ("read", "pair_scores", "centres", "centre_alignments", "layout_render_filter", "write", "total")
TREE_MAX_REFINE = 8      # == UC_TREE_MAX_REFINE


class UcTreeRefinedStats(C.Structure):
    _fields_ = [("tree", UcTreeStats)] + [(n, C.c_uint64) for n in ("n_rounds", "n_tasks", "n_cells", "n_rows_became_aligned", "n_rows_became_unaligned")] + [
        ("width_before", C.c_uint64 * TREE_MAX_REFINE), ("width_after", C.c_uint64 * TREE_MAX_REFINE), ("seconds", C.c_double * 3)]


TREE_REFINED_PHASES = ("profile_dp_walk", "layout_compaction", "total")


class UcMsaProgressiveStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_merges", "n_levels", "n_launches", "n_cells")]


class UcTreeProgressiveStats(C.Structure):
    _fields_ = [("tree", UcTreeStats)] + [(n, C.c_uint64) for n in ("n_groups_aligned", "n_merges", "n_levels", "n_launches", "n_cells", "width_before", "width_after")] + [
        ("seconds", C.c_double * 3)]


TREE_PROGRESSIVE_PHASES = ("guide", "merges", "total")
MSA_PROGRESSIVE_MAX_ROWS = 8192      # == MSA_PROG_MAX_ROWS


class UcNjStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "n_columns", "n_pairs_incomparable", "n_pairs_capped", "n_lengths_clamped")] + [("seconds", C.c_double * 5)]


NJ_PHASES = ("read", "counts", "transform", "join", "write")
NJ_MODELS = {"kimura": 0, "p": 1}
NJ_SUPPORT_MODES = {"fbp": 0, "tbe": 1}      # UC_NJ_SUPPORT_FBP / UC_NJ_SUPPORT_TBE
NJ_NO_NODE = 0xFFFFFFFF  # == UC_NJ_NO_NODE: the third root entry of a two-leaf tree


class UcNjBootStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_rows", "n_columns", "n_replicates", "n_batches", "support_min", "support_sum")] + [("seconds", C.c_double * 7)]


NJ_BOOT_PHASES = ("read", "main_tree", "counts", "transform", "join", "support", "write")


class UcT5Stats(C.Structure):
    _fields_ = [("n_seqs", C.c_uint64), ("n_tokens", C.c_uint64), ("flops", C.c_double), ("gpu_ms", C.c_double),
                ("n_replicas", C.c_uint32), ("reserved0", C.c_uint32), ("gpu_ms_sum", C.c_double),
                ("tokens_min_replica", C.c_uint64), ("tokens_max_replica", C.c_uint64)]


HIT_DTYPE = np.dtype([("target", "<u4"), ("score", "<i4"), ("diag", "<i4")])
ALN_DTYPE = np.dtype([(n, "<i4") for n in ("score", "score_rev", "corrected", "qstart", "qend", "tstart", "tend",
                                            "aln_len", "idents", "pass_evalue", "accepted", "gap_opens")])

# every symbol include/unicore_cluster.h declares (tests check the library exports all of them)
SYMBOLS = (
    "uc_cluster", "uc_createtsv", "uc_rmdb", "uc_search", "uc_convertalis", "uc_last_error", "uc_version", "uc_check_options",
    "uc_option_arity", "uc_release_scratch", "uc_createdb", "uc_t5_load", "uc_t5_free", "uc_t5_encode", "uc_t5_get_stats", "uc_comm_unique_id", "uc_comm_create", "uc_comm_destroy", "uc_comm_info", "uc_engine_cluster_step",
    "uc_engine_create", "uc_engine_destroy", "uc_engine_load_db", "uc_engine_set_db", "uc_engine_num_seqs",
    "uc_engine_prefilter", "uc_engine_prefilter_range", "uc_engine_hits_size", "uc_engine_hits_get", "uc_engine_hits_get_range", "uc_engine_hits_set", "uc_engine_hits_merge",
    "uc_engine_hits_export_dev", "uc_engine_hits_import_dev", "uc_engine_setcover",
    "uc_hits_merge", "uc_engine_align", "uc_engine_alns_get", "uc_engine_edges_size", "uc_engine_edges_get",
    "uc_engine_stats", "uc_engine_reset_stats", "uc_setcover", "uc_write_cluster_db",
    "uc_engine_ungapped_batch", "uc_engine_ungapped_select", "uc_engine_ungapped_all", "uc_engine_sw_batch", "uc_engine_sw_pass", "uc_engine_sw_pass2", "uc_engine_backtraces_size", "uc_engine_backtraces_get",
    "uc_backtrace_render", "uc_format_output_check", "uc_engine_tb_emit_pass", "uc_abi_version", "uc_stats_size", "uc_set_round_hook",
    "uc_t5_gemm_variant", "uc_t5_kernel_gemm", "uc_t5_kernel_rmsnorm", "uc_t5_kernel_attention", "uc_t5_kernel_cnn_head", "uc_t5_bias_table",
    "uc_cluster_graph", "uc_engine_cluster_graph", "uc_engine_reassign", "uc_engine_td_onchip", "uc_engine_sw_task_queries", "uc_engine_linclust_pairs",
    "uc_profile_count", "uc_profile_count_dev", "uc_profile",
    "uc_msa_center", "uc_msa_center_dev", "uc_msa_star", "uc_msa_star_dev", "uc_msa_filter", "uc_msa_filter_dev", "uc_tree",
    "uc_msa_profile_align", "uc_msa_profile_align_dev", "uc_msa_profile_layout", "uc_msa_profile_layout_dev", "uc_msa_profile_geometry", "uc_tree_refined",
    "uc_msa_self_scores", "uc_msa_guide", "uc_msa_guide_dev", "uc_msa_merge", "uc_msa_merge_dev", "uc_msa_progressive", "uc_msa_progressive_dev",
    "uc_msa_progressive_geometry", "uc_tree_progressive",
    "uc_nj_counts", "uc_nj_counts_dev", "uc_nj_distances", "uc_nj_join", "uc_nj_join_dev", "uc_nj_newick", "uc_nj_geometry", "uc_tree_infer",
    "uc_nj_boot_columns", "uc_nj_boot_counts", "uc_nj_boot_counts_dev", "uc_nj_join_batch", "uc_nj_join_batch_dev", "uc_nj_support", "uc_nj_newick_support",
    "uc_nj_boot_geometry", "uc_tree_infer_boot",
    "uc_nj_transfer", "uc_nj_transfer_dev", "uc_nj_newick_transfer", "uc_nj_transfer_geometry", "uc_tree_infer_support",
)
NO_GENE = 0xFFFFFFFF  # == UC_NO_GENE: a TSV row whose gene name is not in the map
ABI_VERSION = 9      # == UC_ABI_VERSION of include/unicore_cluster.h this binding mirrors
ROUND_HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_int32, C.c_uint32, C.POINTER(C.c_uint32), C.c_int32, C.c_void_p)

_lib = None


class UcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("unicore_cluster error %d: %s" % (code, msg))
        self.code = code


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing — run `make product` (or __graft_entry__.build()); there is no fallback path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    L.uc_last_error.restype = C.c_char_p
    L.uc_version.restype = C.c_char_p
    L.uc_check_options.argtypes = [C.c_char_p]
    L.uc_option_arity.argtypes = [C.c_char_p]
    L.uc_createdb.argtypes = [C.POINTER(C.c_char_p), C.c_int, C.c_char_p, C.c_char_p, C.POINTER(UcOpts), C.POINTER(UcT5Stats)]
    L.uc_t5_load.argtypes = [C.c_char_p, i32, C.POINTER(vp)]
    L.uc_t5_free.argtypes = [vp]
    L.uc_t5_free.restype = None
    L.uc_t5_encode.argtypes = [vp, u32, vp, C.c_char_p, vp, vp]
    L.uc_t5_get_stats.argtypes = [vp, C.POINTER(UcT5Stats)]
    L.uc_release_scratch.restype = None
    L.uc_comm_unique_id.argtypes = [vp]
    L.uc_comm_create.argtypes = [vp, i32, i32, i32, C.POINTER(vp)]
    L.uc_comm_destroy.argtypes = [vp]
    L.uc_comm_destroy.restype = None
    L.uc_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.uc_engine_cluster_step.argtypes = [vp, vp, i32, vp, C.POINTER(u64)]
    L.uc_cluster.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(UcOpts), C.POINTER(UcStats)]
    L.uc_createtsv.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(UcOpts)]
    L.uc_search.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(UcOpts), C.POINTER(UcStats)]
    L.uc_convertalis.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(UcOpts)]
    L.uc_engine_prefilter_range.argtypes = [vp, u32, u32, u32, u32]
    L.uc_rmdb.argtypes = [C.c_char_p]
    L.uc_engine_create.argtypes = [C.POINTER(UcOpts), C.POINTER(vp)]
    L.uc_engine_destroy.argtypes = [vp]
    L.uc_engine_destroy.restype = None
    L.uc_engine_load_db.argtypes = [vp, C.c_char_p]
    L.uc_engine_set_db.argtypes = [vp, u32, vp, vp, vp]
    L.uc_engine_num_seqs.argtypes = [vp]
    L.uc_engine_num_seqs.restype = u32
    L.uc_engine_prefilter.argtypes = [vp, u32, u32]
    L.uc_engine_hits_size.argtypes = [vp, C.POINTER(u64)]
    L.uc_engine_hits_get.argtypes = [vp, vp, vp]
    L.uc_engine_hits_get_range.argtypes = [vp, u32, u32, vp, vp]
    L.uc_engine_hits_set.argtypes = [vp, vp, vp]
    L.uc_engine_hits_merge.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp)]
    L.uc_engine_hits_export_dev.argtypes = [vp, vp, vp, vp, vp]
    L.uc_engine_setcover.argtypes = [vp, vp, u64, vp]
    L.uc_engine_hits_import_dev.argtypes = [vp, u64, vp, vp, vp, vp, u32, u32, C.POINTER(u64)]
    L.uc_hits_merge.argtypes = [u32, i32, C.c_int, C.POINTER(vp), C.POINTER(vp), vp, vp, u64, C.POINTER(u64)]
    L.uc_engine_align.argtypes = [vp, u32, u32]
    L.uc_engine_alns_get.argtypes = [vp, u32, u32, vp]
    L.uc_engine_edges_size.argtypes = [vp, C.POINTER(u64)]
    L.uc_engine_edges_get.argtypes = [vp, vp]
    L.uc_engine_stats.argtypes = [vp, C.POINTER(UcStats)]
    L.uc_engine_reset_stats.argtypes = [vp]
    L.uc_engine_reset_stats.restype = None
    L.uc_engine_td_onchip.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.uc_engine_sw_task_queries.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.uc_engine_linclust_pairs.argtypes = [vp, i32, i32, vp, u64, C.POINTER(u64)]
    L.uc_setcover.argtypes = [u32, vp, u64, vp]
    L.uc_cluster_graph.argtypes = [u32, vp, u64, vp, i32, vp]
    L.uc_engine_cluster_graph.argtypes = [vp, i32, vp, u64, vp]
    L.uc_engine_reassign.argtypes = [vp, vp, vp, vp, vp]
    L.uc_write_cluster_db.argtypes = [C.c_char_p, u32, vp]
    L.uc_profile_count.argtypes = [u64, vp, vp, u32, u32, vp, vp, u32, u32] + [vp] * 7
    L.uc_profile_count_dev.argtypes = [i32, u64, vp, vp, u32, u32, vp, vp, u32, u32] + [vp] * 7
    L.uc_profile.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32, C.POINTER(UcOpts)]
    L.uc_msa_center.argtypes = [u32, vp, vp, vp]
    L.uc_msa_center_dev.argtypes = [i32, u32, vp, vp, vp]
    L.uc_msa_star.argtypes = [u32, vp, vp, u32] + [vp] * 8 + [vp, vp, vp, u64, vp, vp, u64, vp]
    L.uc_msa_star_dev.argtypes = [i32] + L.uc_msa_star.argtypes
    L.uc_msa_filter.argtypes = [u32, vp, vp, vp, u32, vp, vp, vp]
    L.uc_msa_filter_dev.argtypes = [i32] + L.uc_msa_filter.argtypes
    L.uc_tree.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32, C.c_char_p, C.POINTER(UcOpts), C.POINTER(UcTreeStats)]
    L.uc_msa_profile_align.argtypes = [u32] + [vp] * 9 + [i32, i32] + [vp] * 8 + [u64, vp]
    L.uc_msa_profile_align_dev.argtypes = [i32] + L.uc_msa_profile_align.argtypes
    L.uc_msa_profile_align.argtypes = L.uc_msa_profile_align.argtypes + [u32]
    L.uc_msa_profile_layout.argtypes = [u32] + [vp] * 15 + [u64, vp]
    L.uc_msa_profile_layout_dev.argtypes = [i32] + L.uc_msa_profile_layout.argtypes
    L.uc_msa_profile_geometry.argtypes = [vp, vp, vp]
    L.uc_tree_refined.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32, C.c_char_p, u32, C.POINTER(UcOpts), C.POINTER(UcTreeRefinedStats)]
    L.uc_msa_self_scores.argtypes = [u64] + [vp] * 6
    L.uc_msa_guide.argtypes = [u32] + [vp] * 5
    L.uc_msa_guide_dev.argtypes = [i32] + L.uc_msa_guide.argtypes
    L.uc_msa_merge.argtypes = [u32] + [vp] * 10 + [i32, i32] + [vp] * 7 + [u64, vp, vp, vp, u64, vp]
    L.uc_msa_merge_dev.argtypes = [i32] + L.uc_msa_merge.argtypes
    L.uc_msa_merge.argtypes = L.uc_msa_merge.argtypes + [u32]
    L.uc_msa_progressive.argtypes = [u32] + [vp] * 7 + [i32, i32, vp, vp, vp, u64, vp, C.POINTER(UcMsaProgressiveStats)]
    L.uc_msa_progressive_dev.argtypes = [i32] + L.uc_msa_progressive.argtypes
    L.uc_msa_progressive.argtypes = L.uc_msa_progressive.argtypes + [u32]
    L.uc_msa_progressive_geometry.argtypes = [vp, vp, vp]
    L.uc_tree_progressive.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32, C.c_char_p, C.POINTER(UcOpts), C.POINTER(UcTreeProgressiveStats)]
    L.uc_nj_counts.argtypes = [u32, u64, vp, u32, vp, vp]
    L.uc_nj_counts_dev.argtypes = [i32] + L.uc_nj_counts.argtypes
    L.uc_nj_distances.argtypes = [vp, vp, u32, u32, vp]
    L.uc_nj_join.argtypes = [u32] + [vp] * 7
    L.uc_nj_join_dev.argtypes = [i32] + L.uc_nj_join.argtypes
    L.uc_nj_newick.argtypes = [C.POINTER(C.c_char_p), u32] + [vp] * 6 + [vp, u64, C.POINTER(u64)]
    L.uc_nj_geometry.argtypes = [C.POINTER(u32), C.POINTER(u32)]
    L.uc_tree_infer.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(UcOpts), C.POINTER(UcNjStats)]
    L.uc_nj_boot_columns.argtypes = [u64, u64, u32, vp]
    L.uc_nj_boot_counts.argtypes = [u32, u64, vp, u64, u32, u32, u32, vp, vp]
    L.uc_nj_boot_counts_dev.argtypes = [i32] + L.uc_nj_boot_counts.argtypes
    L.uc_nj_join_batch.argtypes = [u32, u32] + [vp] * 7
    L.uc_nj_join_batch_dev.argtypes = [i32] + L.uc_nj_join_batch.argtypes
    L.uc_nj_support.argtypes = [u32, vp, vp, u32, vp, vp, vp]
    L.uc_nj_newick_support.argtypes = [C.POINTER(C.c_char_p), u32] + [vp] * 6 + [vp, u32, vp, u64, C.POINTER(u64)]
    L.uc_nj_boot_geometry.argtypes = [C.POINTER(u32)]
    L.uc_tree_infer_boot.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32, u64, C.POINTER(UcOpts), C.POINTER(UcNjBootStats)]
    L.uc_nj_transfer.argtypes = [u32, vp, vp, u32, vp, vp, u32, vp, vp]
    L.uc_nj_transfer_dev.argtypes = [i32] + L.uc_nj_transfer.argtypes
    L.uc_nj_newick_transfer.argtypes = [C.POINTER(C.c_char_p), u32] + [vp] * 6 + [vp, vp, u32, vp, u64, C.POINTER(u64)]
    L.uc_nj_transfer_geometry.argtypes = [C.POINTER(u32), C.POINTER(u32), C.POINTER(u32)]
    L.uc_tree_infer_support.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, u32, u64, u32, C.POINTER(UcOpts), C.POINTER(UcNjBootStats)]
    L.uc_engine_ungapped_batch.argtypes = [vp, u64, vp, vp, vp, vp]
    L.uc_engine_ungapped_select.argtypes = [vp, u64, vp, vp, vp, C.c_int32, vp, vp, vp]
    L.uc_engine_ungapped_all.argtypes = [vp, u32, u32, u32, u32, u64, vp, vp]
    L.uc_engine_sw_batch.argtypes = [vp, C.c_int, u64, vp, vp, vp, vp, vp, vp, vp]
    L.uc_engine_sw_pass.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, u64, vp, vp, vp, vp] + [vp] * 8
    L.uc_engine_sw_pass2.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, u64, vp, vp, vp, vp] + [vp] * 10
    L.uc_engine_backtraces_size.argtypes = [vp, u32, u32, C.POINTER(u64)]
    L.uc_engine_backtraces_get.argtypes = [vp, u32, u32, vp, vp]
    L.uc_backtrace_render.argtypes = [vp, u64, C.c_char_p, u64, C.POINTER(u64)]
    L.uc_format_output_check.argtypes = [C.c_char_p, C.POINTER(u32)]
    L.uc_engine_tb_emit_pass.argtypes = [vp, C.c_int, C.c_int, u64, vp, vp, vp, vp] + [vp] * 6 + [vp, vp, u64, C.POINTER(u64)]
    L.uc_t5_gemm_variant.argtypes = [i32, i32, i32, C.POINTER(i32)]
    L.uc_t5_kernel_gemm.argtypes = [i32, i32, i32, i32, i32, i32, vp, vp, vp]
    L.uc_t5_kernel_rmsnorm.argtypes = [i32, i32, i32, C.c_float, vp, vp, vp]
    L.uc_t5_kernel_attention.argtypes = [i32, i32, i32, vp, i32, vp, vp, vp]
    L.uc_t5_kernel_cnn_head.argtypes = [i32, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.uc_t5_bias_table.argtypes = [i32, i32, i32, i32, vp, vp]
    L.uc_abi_version.restype = u32
    L.uc_stats_size.restype = C.c_size_t
    L.uc_set_round_hook.argtypes = [ROUND_HOOK, vp]
    L.uc_set_round_hook.restype = None
    # uc_stats carries no size field: a binding that disagrees with the library about its layout would be overrun silently
    if L.uc_abi_version() != ABI_VERSION or L.uc_stats_size() != C.sizeof(UcStats):
        raise ImportError("libunicore_cluster.so has ABI %d / uc_stats of %d bytes; this binding mirrors ABI %d / %d bytes — rebuild (`make product`)"
                          % (L.uc_abi_version(), L.uc_stats_size(), ABI_VERSION, C.sizeof(UcStats)))
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise UcError(rc, lib().uc_last_error().decode(errors="replace"))


def make_opts(cluster_options="", threads=1, verbosity=1, device=-1, data_dir=None, num_gpus=1):
    o = UcOpts()
    o.struct_size = C.sizeof(UcOpts)
    o.threads = threads
    o.verbosity = verbosity
    o.device = device
    o.num_gpus = num_gpus
    o.cluster_options = cluster_options.encode()
    o.data_dir = data_dir.encode() if data_dir else None
    return o


def version():
    return lib().uc_version().decode()


def check_options(s):
    return lib().uc_check_options(s.encode())


def cluster(db, out_cluster_db, tmp, cluster_options="-c 0.8", threads=1, verbosity=1, device=-1, num_gpus=1):
    """== `foldseek cluster` (cluster.rs:45-56).  Returns the stats dict.  num_gpus: 0 = all visible GPUs."""
    o, st = make_opts(cluster_options, threads, verbosity, device, num_gpus=num_gpus), UcStats()
    _check(lib().uc_cluster(db.encode(), out_cluster_db.encode(), tmp.encode(), C.byref(o), C.byref(st)))
    return st.as_dict()


def createtsv(db, cluster_db, out_tsv, verbosity=1):
    o = make_opts("", 1, verbosity)
    _check(lib().uc_createtsv(db.encode(), cluster_db.encode(), out_tsv.encode(), C.byref(o)))


def search(query_db, target_db, out_aln_db, tmp, search_options="-c 0.8", threads=1, verbosity=1, device=-1):
    """== `foldseek search` (search.rs:44-50).  Returns the stats dict."""
    o, st = make_opts(search_options, threads, verbosity, device), UcStats()
    _check(lib().uc_search(query_db.encode(), target_db.encode(), out_aln_db.encode(), tmp.encode(), C.byref(o), C.byref(st)))
    return st.as_dict()


def convertalis(query_db, target_db, aln_db, out_m8, verbosity=1, format_output=None):
    """== `foldseek convertalis` (search.rs:57-60); format_output: the LIST of --format-output (None = the 12 BLAST-tab columns)"""
    o = make_opts("--format-output %s" % format_output if format_output else "", 1, verbosity)
    _check(lib().uc_convertalis(query_db.encode(), target_db.encode(), aln_db.encode(), out_m8.encode(), C.byref(o)))


def render_backtrace(runs):
    """run words (length << 2 | op; 0 M, 1 I, 2 D) -> "35M2D110M" (uc_backtrace_render: the text of the alignment DB's 15th field)"""
    r = np.ascontiguousarray(runs, np.uint32)
    buf = C.create_string_buffer(12 * len(r) + 1)
    _check(lib().uc_backtrace_render(r.ctypes.data, len(r), buf, len(buf), None))
    return buf.value.decode()


def format_output_columns(names):
    """number of columns of a --format-output LIST; UcError for an unknown name"""
    k = C.c_uint32(0)
    _check(lib().uc_format_output_check(names.encode(), C.byref(k)))
    return k.value


def rmdb(prefix):
    _check(lib().uc_rmdb(prefix.encode()))


def setcover(n, edges):
    e = np.ascontiguousarray(edges, np.uint32).reshape(-1, 2)
    assign = np.zeros(n, np.uint32)
    _check(lib().uc_setcover(n, e.ctypes.data, len(e), assign.ctypes.data))
    return assign


def cluster_graph(n, edges, lens, mode):
    """E7 on the host by rule (uc_cluster_graph): mode 0 = greedy set cover, 2 = greedy incremental (--cluster-mode 2: longest sequence first,
    ties by ascending id; lens[n] = residue counts, may be None for mode 0).  Needs no device."""
    e = np.ascontiguousarray(edges, np.uint32).reshape(-1, 2)
    ln = np.ascontiguousarray(lens, np.uint32) if lens is not None else None
    if ln is not None and len(ln) != n:
        raise ValueError("lens has %d entries for %d nodes" % (len(ln), n))
    assign = np.zeros(n, np.uint32)
    _check(lib().uc_cluster_graph(n, e.ctypes.data, len(e), ln.ctypes.data if ln is not None else None, mode, assign.ctypes.data))
    return assign


def profile_count(group, gene, n_groups, sp_off, sp, n_species, threshold=80, device=None):
    """The counting core of `unicore profile` (rule UC-P; uc_profile_count / uc_profile_count_dev).  group[i] = dense group index of row i,
    gene[i] = gene id or NO_GENE, sp_off / sp = the gene -> species CSR (ascending ids).  device=None: the host counter (needs no GPU);
    an ordinal (-1 = the current device): the HIP kernels.  Returns a dict: single, multiple, core [n_groups], full [n_species],
    core_off [n_groups + 1], core_gene / core_species (the file lines of every core group, ascending species)."""
    gr, ge = np.ascontiguousarray(group, np.uint32), np.ascontiguousarray(gene, np.uint32)
    so, spv = np.ascontiguousarray(sp_off, np.uint64), np.ascontiguousarray(sp, np.uint32)
    if len(gr) != len(ge):
        raise ValueError("group has %d entries, gene %d" % (len(gr), len(ge)))
    if len(so) < 1:
        raise ValueError("sp_off needs n_genes + 1 entries")
    n_genes = len(so) - 1
    cnt = np.diff(so.astype(np.int64))
    ok = (ge != NO_GENE) & (ge < n_genes)
    cap = int(cnt[ge[ok]].sum()) if n_genes and len(ge) and (cnt >= 0).all() else 0
    ng, ns = max(int(n_groups), 0), max(int(n_species), 0)
    small = ng < (1 << 24) and ns < (1 << 24)      # beyond the limit the call refuses before it looks at an array
    single, multiple = (np.zeros(ng if small else 1, np.uint32) for _ in range(2))
    core, full = np.zeros(ng if small else 1, np.uint8), np.zeros(ns if small else 1, np.uint32)
    core_off = np.zeros((ng if small else 0) + 1, np.uint64)
    cg, cs = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
    args = [len(gr), gr.ctypes.data, ge.ctypes.data, n_groups, n_genes, so.ctypes.data, spv.ctypes.data, n_species, threshold,
            single.ctypes.data, multiple.ctypes.data, core.ctypes.data, core_off.ctypes.data, cg.ctypes.data, cs.ctypes.data, full.ctypes.data]
    _check(lib().uc_profile_count(*args) if device is None else lib().uc_profile_count_dev(device, *args))
    n = int(core_off[-1])
    return {"single": single, "multiple": multiple, "core": core, "full": full, "core_off": core_off, "core_gene": cg[:n].copy(), "core_species": cs[:n].copy()}


def profile(db, tsv, out_dir, threshold=80, verbosity=1, device=-1):
    """== `unicore profile -t threshold <db> <tsv> <out_dir>` (uc_profile): reads <db>.map and the TSV, writes one .txt per core group,
    copiness.tsv and profile.chk into out_dir.  verbosity is Unicore's 0..4 scale.  UC_PROFILE_HOST=1 in the environment selects the
    host counter."""
    o = make_opts("", 1, verbosity, device)
    _check(lib().uc_profile(db.encode(), tsv.encode(), out_dir.encode(), threshold, C.byref(o)))


def _ptr(a):
    return a.ctypes.data if a is not None and a.size else None


def msa_center(grp_off, scores, device=None):
    """UC-T/C (uc_msa_center / uc_msa_center_dev): grp_off [n_groups + 1] counts rows, scores holds every group's packed upper triangle of pair
    scores (row-major over i < j), groups back to back.  Returns centre [n_groups]: per group the row with the largest 64-bit row sum, the
    earliest among equals.  device=None: the host twin (needs no GPU); an ordinal (-1 = the current device): the HIP kernels."""
    go, sc = np.ascontiguousarray(grp_off, np.uint64), np.ascontiguousarray(scores, np.int32)
    ng = len(go) - 1
    if ng < 0:
        raise ValueError("grp_off needs n_groups + 1 entries")
    m = np.diff(go.astype(np.int64))
    if ng and (m >= 0).all() and len(sc) != int((m * (m - 1) // 2).sum()):
        raise ValueError("scores has %d entries, the triangles hold %d" % (len(sc), int((m * (m - 1) // 2).sum())))
    centre = np.zeros(max(ng, 1), np.uint32)
    args = [ng, go.ctypes.data, _ptr(sc), centre.ctypes.data]
    _check(lib().uc_msa_center(*args) if device is None else lib().uc_msa_center_dev(device, *args))
    return centre[:ng]


def msa_star(grp_off, centre, res_off, res, qs, ts, run_off, runs, aligned, device=None):
    """UC-T/L and the rows (uc_msa_star / uc_msa_star_dev).  res: one or two byte arrays (tracks) on the offsets res_off [n_rows + 1]; per row qs, ts,
    aligned and the backtrace runs[run_off[r]:run_off[r + 1]] (length << 2 | op; 0 M, 1 I, 2 D; centre as query).  Returns a dict: width [n_groups],
    col (the centre positions' columns, groups back to back), cnt (rows with a residue per column of track 0), cells (list, one flat uint8 array
    per track: group g holds m_g x width[g] bytes, row-major).  device as in msa_center."""
    go, ce = np.ascontiguousarray(grp_off, np.uint64), np.ascontiguousarray(centre, np.uint32)
    ro, uo = np.ascontiguousarray(res_off, np.uint64), np.ascontiguousarray(run_off, np.uint64)
    tracks = [np.ascontiguousarray(t, np.uint8) for t in (res if isinstance(res, (list, tuple)) else [res])]
    q, t, al = np.ascontiguousarray(qs, np.int32), np.ascontiguousarray(ts, np.int32), np.ascontiguousarray(aligned, np.uint8)
    ru = np.ascontiguousarray(runs, np.uint32)
    ng = len(go) - 1
    n_rows = int(go[-1]) if ng > 0 else 0
    if len(ce) != ng or any(len(x) != n_rows for x in (q, t, al)) or len(ro) != n_rows + 1 or len(uo) != n_rows + 1:
        raise ValueError("array lengths do not match grp_off")
    if n_rows and (int(uo[-1]) > len(ru) or any(int(ro[-1]) > len(x) for x in tracks) or len({len(x) for x in tracks}) != 1):
        raise ValueError("res_off / run_off reach beyond the arrays they index")
    # capacities from the bound the call itself uses: centre lengths + every D run, per group times its rows
    ln = np.diff(ro.astype(np.int64))
    dl = np.where((ru & 3) == 2, ru >> 2, 0).astype(np.int64)
    dcum = np.concatenate([[0], np.cumsum(dl)])
    cols = cells = ncol = 0
    for g in range(ng):
        b, e = int(go[g]), int(go[g + 1])
        if not (0 <= b <= e <= n_rows) or int(ce[g]) >= max(e - b, 1) or not (0 <= int(uo[b]) <= int(uo[e]) <= len(ru)):
            continue      # the call refuses these itself
        lc = max(int(ln[b + int(ce[g])]), 0)
        w = lc + int(dcum[int(uo[e])] - dcum[int(uo[b])])
        cols += w; cells += (e - b) * w; ncol += lc
    width, col, cnt = np.zeros(max(ng, 1), np.uint32), np.zeros(max(ncol, 1), np.uint32), np.zeros(max(cols, 1), np.uint32)
    out = [np.zeros(max(cells, 1), np.uint8) for _ in tracks]
    need = np.zeros(2, np.uint64)
    args = [ng, go.ctypes.data, _ptr(ce), len(tracks), ro.ctypes.data, _ptr(tracks[0]), _ptr(tracks[1]) if len(tracks) > 1 else None, _ptr(q), _ptr(t),
            uo.ctypes.data, _ptr(ru), _ptr(al), width.ctypes.data, col.ctypes.data, cnt.ctypes.data, cols, out[0].ctypes.data,
            out[1].ctypes.data if len(tracks) > 1 else None, cells, need.ctypes.data]
    _check(lib().uc_msa_star(*args) if device is None else lib().uc_msa_star_dev(device, *args))
    return {"width": width[:ng], "col": col[:ncol], "cnt": cnt[: int(need[0])].copy(), "cells": [o[: int(need[1])].copy() for o in out]}


def msa_filter(grp_off, width, cells, threshold, device=None):
    """UC-T/F (uc_msa_filter / uc_msa_filter_dev): cells is one track as msa_star lays it out; column c of group g is kept iff cnt * 100 >=
    threshold * m_g.  Returns a dict: keep (uint8 per column), fwidth [n_groups], fcells (flat: group g holds m_g x fwidth[g] bytes)."""
    go, w, ce = np.ascontiguousarray(grp_off, np.uint64), np.ascontiguousarray(width, np.uint32), np.ascontiguousarray(cells, np.uint8)
    ng = len(go) - 1
    if len(w) != ng:
        raise ValueError("width has %d entries for %d groups" % (len(w), ng))
    m = np.diff(go.astype(np.int64))
    ncols, ncells = int(w.astype(np.int64).sum()), int((m * w.astype(np.int64)).sum()) if ng else 0
    if len(ce) != max(ncells, 0) and ng and (m > 0).all():
        raise ValueError("cells has %d bytes, the groups hold %d" % (len(ce), ncells))
    keep, fwidth, fcells = np.zeros(max(ncols, 1), np.uint8), np.zeros(max(ng, 1), np.uint32), np.zeros(max(ncells, 1), np.uint8)
    args = [ng, go.ctypes.data, _ptr(w), _ptr(ce), threshold, keep.ctypes.data, fwidth.ctypes.data, fcells.ctypes.data]
    _check(lib().uc_msa_filter(*args) if device is None else lib().uc_msa_filter_dev(device, *args))
    nf = int((m * fwidth[:ng].astype(np.int64)).sum()) if ng else 0
    return {"keep": keep[:ncols], "fwidth": fwidth[:ng], "fcells": fcells[:nf].copy()}


def msa_profile_geometry():
    """The profile DP kernel's geometry (uc_msa_profile_geometry): {"chunk": columns of the MSA a wave holds at a time, "cap": the widest MSA the kernel
    serves (0: no cap, wider tasks run chunk after chunk), "task_bytes_per_cell": bytes of the decision buffer per DP cell}."""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().uc_msa_profile_geometry(C.byref(a), C.byref(b), C.byref(c)))
    return {"chunk": a.value, "cap": b.value, "task_bytes_per_cell": c.value}


def _profile_shape(grp_off, width, cells, res_off, res):
    go, w, ro = np.ascontiguousarray(grp_off, np.uint64), np.ascontiguousarray(width, np.uint32), np.ascontiguousarray(res_off, np.uint64)
    ce, tr = [np.ascontiguousarray(c, np.uint8) for c in cells], [np.ascontiguousarray(t, np.uint8) for t in res]
    ng = len(go) - 1
    if ng < 0 or len(w) != ng or len(ce) != 2 or len(tr) != 2:
        raise ValueError("grp_off needs n_groups + 1 entries, width n_groups, cells and res two tracks (amino acids, 3Di)")
    n_rows = int(go[-1]) if ng > 0 else 0
    m = np.diff(go.astype(np.int64))
    if len(ro) != n_rows + 1:
        raise ValueError("res_off needs n_rows + 1 entries")
    ok = ng == 0 or ((m > 0).all() and int(go[0]) == 0)      # the call refuses the rest itself
    if ok and (any(len(c) != int((m * w.astype(np.int64)).sum()) for c in ce) or (n_rows and any(len(t) < int(ro[-1]) for t in tr))):
        raise ValueError("cells / res do not hold what grp_off, width and res_off describe")
    return go, w, ro, ce, tr, ng, n_rows, m, ok


def msa_profile_align(grp_off, width, cells, res_off, res, S3, SA, gap_open, gap_ext, device=None, threads=1):
    """UC-T/P, the alignment (uc_msa_profile_align / _dev): every row of every group against the leave-one-out profile of the group's MSA.  cells and
    res: [amino acids, 3Di] as bytes (cells as msa_star lays them out), S3 / SA: 21 x 21 int8, [column letter][row letter].  Returns a dict: aligned,
    score, qs, ts, qe, te per row, run_off [n_rows + 1], runs (length << 2 | op; 0 M, 1 I = column only, 2 D = residue only).  device as in msa_center; threads: the host twin's."""
    go, w, ro, ce, tr, ng, n_rows, m, ok = _profile_shape(grp_off, width, cells, res_off, res)
    s3, sa = np.ascontiguousarray(S3, np.int8).reshape(-1), np.ascontiguousarray(SA, np.int8).reshape(-1)
    if len(s3) != 441 or len(sa) != 441:
        raise ValueError("S3 and SA are 21 x 21")
    cap = 0
    if ok and ng:
        ln = np.diff(ro.astype(np.int64))
        cap = int(np.maximum(ln, 0).sum() + (m * w.astype(np.int64)).sum())
    al = np.zeros(max(n_rows, 1), np.uint8)
    sc, qs, ts, qe, te = (np.zeros(max(n_rows, 1), np.int32) for _ in range(5))
    uo, runs, need = np.zeros(n_rows + 1, np.uint64), np.zeros(max(cap, 1), np.uint32), np.zeros(1, np.uint64)
    args = [ng, go.ctypes.data, _ptr(w), _ptr(ce[0]), _ptr(ce[1]), ro.ctypes.data, _ptr(tr[0]), _ptr(tr[1]), s3.ctypes.data, sa.ctypes.data, gap_open, gap_ext,
            al.ctypes.data, sc.ctypes.data, qs.ctypes.data, ts.ctypes.data, qe.ctypes.data, te.ctypes.data, uo.ctypes.data, runs.ctypes.data, cap, need.ctypes.data]
    _check(lib().uc_msa_profile_align(*args, threads) if device is None else lib().uc_msa_profile_align_dev(device, *args))
    return {"aligned": al[:n_rows], "score": sc[:n_rows], "qs": qs[:n_rows], "ts": ts[:n_rows], "qe": qe[:n_rows], "te": te[:n_rows], "run_off": uo,
            "runs": runs[: int(need[0])].copy()}


def msa_profile_layout(grp_off, width, cells, res_off, res, aligned, qs, ts, run_off, runs, device=None):
    """UC-T/P, layout and compaction (uc_msa_profile_layout / _dev): the new MSA from msa_profile_align's alignments, UC-T/L with a virtual centre of
    the old width, the columns without an amino acid dropped.  Returns a dict: width [n_groups], cells [amino acids, 3Di].  device as in msa_center."""
    go, w, ro, ce, tr, ng, n_rows, m, ok = _profile_shape(grp_off, width, cells, res_off, res)
    al, q, t = np.ascontiguousarray(aligned, np.uint8), np.ascontiguousarray(qs, np.int32), np.ascontiguousarray(ts, np.int32)
    uo, ru = np.ascontiguousarray(run_off, np.uint64), np.ascontiguousarray(runs, np.uint32)
    if any(len(x) != n_rows for x in (al, q, t)) or len(uo) != n_rows + 1 or (n_rows and int(uo[-1]) > len(ru)):
        raise ValueError("array lengths do not match grp_off")
    cap = 0
    if ok and ng:      # rows x (width + every D run) per group
        dl = np.where((ru & 3) == 2, ru >> 2, 0).astype(np.int64)
        dcum = np.concatenate([[0], np.cumsum(dl)])
        for g in range(ng):
            b, e = int(go[g]), int(go[g + 1])
            if 0 <= int(uo[b]) <= int(uo[e]) <= len(ru):
                cap += (e - b) * (int(w[g]) + int(dcum[int(uo[e])] - dcum[int(uo[b])]))
    nw, out, need = np.zeros(max(ng, 1), np.uint32), [np.zeros(max(cap, 1), np.uint8) for _ in range(2)], np.zeros(1, np.uint64)
    args = [ng, go.ctypes.data, _ptr(w), _ptr(ce[0]), _ptr(ce[1]), ro.ctypes.data, _ptr(tr[0]), _ptr(tr[1]), _ptr(al), _ptr(q), _ptr(t), uo.ctypes.data, _ptr(ru),
            nw.ctypes.data, out[0].ctypes.data, out[1].ctypes.data, cap, need.ctypes.data]
    _check(lib().uc_msa_profile_layout(*args) if device is None else lib().uc_msa_profile_layout_dev(device, *args))
    return {"width": nw[:ng], "cells": [o[: int(need[0])].copy() for o in out]}


def msa_progressive_geometry():
    """The progressive DP kernel's geometry (uc_msa_progressive_geometry): {"chunk": a's columns a wave holds at a time, "cap": the widest side the kernel
    serves (0: no cap), "task_bytes_per_cell": bytes of the score and decision buffers per DP cell}."""
    a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().uc_msa_progressive_geometry(C.byref(a), C.byref(b), C.byref(c)))
    return {"chunk": a.value, "cap": b.value, "task_bytes_per_cell": c.value}


def msa_self_scores(res_off, res, S3, SA):
    """uc_msa_self_scores (host only): per row the sum over its residues of SA[a][a] + S3[d][d], int64.  res: [amino acids, 3Di]."""
    ro, tr = np.ascontiguousarray(res_off, np.uint64), [np.ascontiguousarray(t, np.uint8) for t in res]
    s3, sa = np.ascontiguousarray(S3, np.int8).reshape(-1), np.ascontiguousarray(SA, np.int8).reshape(-1)
    if len(s3) != 441 or len(sa) != 441 or len(tr) != 2 or len(ro) < 1:
        raise ValueError("S3 and SA are 21 x 21, res two tracks, res_off n_rows + 1 entries")
    n = len(ro) - 1
    if n and any(len(t) < int(ro[-1]) for t in tr):
        raise ValueError("res_off reaches beyond res")
    out = np.zeros(max(n, 1), np.int64)
    _check(lib().uc_msa_self_scores(n, ro.ctypes.data, _ptr(tr[0]), _ptr(tr[1]), s3.ctypes.data, sa.ctypes.data, out.ctypes.data))
    return out[:n]


def msa_guide(grp_off, scores, self_scores, device=None):
    """UC-T/G/T (uc_msa_guide / uc_msa_guide_dev): the guide tree of every group from its packed triangle of pair scores (as msa_center takes it) and
    the rows' self scores.  Returns a dict: D (list, per group an m x m fp64 matrix), merges (list, per group an (m - 1) x 2 uint32 array of node
    pairs (a, b); merge k creates node m + k).  device as in msa_center."""
    go, sc, se = np.ascontiguousarray(grp_off, np.uint64), np.ascontiguousarray(scores, np.int32), np.ascontiguousarray(self_scores, np.int64)
    ng = len(go) - 1
    if ng < 0:
        raise ValueError("grp_off needs n_groups + 1 entries")
    m = np.diff(go.astype(np.int64))
    ok = ng == 0 or ((m > 0).all() and int(go[0]) == 0 and (m <= MSA_PROGRESSIVE_MAX_ROWS).all())      # the call refuses the rest itself
    n_rows = int(go[-1]) if ng > 0 and ok else 0
    if ok and ng and (len(sc) != int((m * (m - 1) // 2).sum()) or len(se) != n_rows):
        raise ValueError("scores holds the triangles and self_scores one entry per row")
    D = np.zeros(max(int((m * m).sum()) if ok and ng else 0, 1), np.float64)
    mg = np.zeros(max(2 * (n_rows - ng), 1), np.uint32)
    args = [ng, go.ctypes.data, _ptr(sc), _ptr(se), D.ctypes.data, mg.ctypes.data]
    _check(lib().uc_msa_guide(*args) if device is None else lib().uc_msa_guide_dev(device, *args))
    outD, outM, d0 = [], [], 0
    for g in range(ng):
        k, b = int(m[g]), int(go[g])
        outD.append(D[d0:d0 + k * k].reshape(k, k).copy()); d0 += k * k
        outM.append(mg[2 * (b - g):2 * (b - g) + 2 * (k - 1)].reshape(k - 1, 2).copy())
    return {"D": outD, "merges": outM}


def msa_merge(ma, mb, Wa, Wb, a, b, S3, SA, gap_open, gap_ext, device=None, threads=1):
    """UC-T/G/M (uc_msa_merge / uc_msa_merge_dev): a batch of independent profile-profile merges.  ma, mb, Wa, Wb per task; a and b: [amino acids, 3Di],
    each the sides' cells task after task (m x W bytes row-major, `-` or a letter).  Returns a dict: score, is, js, ie, je, width per task, run_off
    [n_tasks + 1], runs (length << 2 | op; 0 M, 1 I = a's column alone, 2 D = b's column alone), cell_off [n_tasks + 1], cells [amino acids, 3Di]
    (task k: (ma + mb) x width[k] bytes at cell_off[k]).  device as in msa_center; threads: the host twin's."""
    A_, B_, WA, WB = (np.ascontiguousarray(x, np.uint32) for x in (ma, mb, Wa, Wb))
    ca, cb = [np.ascontiguousarray(x, np.uint8) for x in a], [np.ascontiguousarray(x, np.uint8) for x in b]
    s3, sa = np.ascontiguousarray(S3, np.int8).reshape(-1), np.ascontiguousarray(SA, np.int8).reshape(-1)
    n = len(A_)
    if len(s3) != 441 or len(sa) != 441 or len(ca) != 2 or len(cb) != 2 or any(len(x) != n for x in (B_, WA, WB)):
        raise ValueError("S3 and SA are 21 x 21, a and b two tracks, ma, mb, Wa and Wb one entry per task")
    i64 = lambda x: x.astype(np.int64)
    if any(len(c) != int((i64(A_) * i64(WA)).sum()) for c in ca) or any(len(c) != int((i64(B_) * i64(WB)).sum()) for c in cb):
        raise ValueError("a / b do not hold what ma, mb, Wa and Wb describe")
    rcap, ccap = int((i64(WA) + i64(WB)).sum()), int(((i64(A_) + i64(B_)) * (i64(WA) + i64(WB))).sum())
    sc, i0, j0, ie, je = (np.zeros(max(n, 1), np.int32) for _ in range(5))
    uo, runs, width = np.zeros(n + 1, np.uint64), np.zeros(max(rcap, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
    out, need = [np.zeros(max(ccap, 1), np.uint8) for _ in range(2)], np.zeros(2, np.uint64)
    args = [n, _ptr(A_), _ptr(B_), _ptr(WA), _ptr(WB), _ptr(ca[0]), _ptr(ca[1]), _ptr(cb[0]), _ptr(cb[1]), s3.ctypes.data, sa.ctypes.data, gap_open, gap_ext,
            sc.ctypes.data, i0.ctypes.data, j0.ctypes.data, ie.ctypes.data, je.ctypes.data, uo.ctypes.data, runs.ctypes.data, rcap, width.ctypes.data,
            out[0].ctypes.data, out[1].ctypes.data, ccap, need.ctypes.data]
    _check(lib().uc_msa_merge(*args, threads) if device is None else lib().uc_msa_merge_dev(device, *args))
    co = np.concatenate([[0], np.cumsum((i64(A_) + i64(B_)) * i64(width[:n]))]).astype(np.uint64)
    return {"score": sc[:n], "is": i0[:n], "js": j0[:n], "ie": ie[:n], "je": je[:n], "width": width[:n], "run_off": uo, "runs": runs[: int(need[0])].copy(),
            "cell_off": co, "cells": [o[: int(need[1])].copy() for o in out]}


def msa_progressive(grp_off, res_off, res, merges, S3, SA, gap_open, gap_ext, device=None, threads=1):
    """UC-T/G (uc_msa_progressive / uc_msa_progressive_dev): the progressive MSA of every group along its merge list.  res: [amino acids, 3Di] on the
    offsets res_off; merges: per group an (m - 1) x 2 array of node pairs as msa_guide returns them (any tree over the group may be forced).  Returns a
    dict: width [n_groups], cells [amino acids, 3Di] (group g: m_g x width[g] bytes, rows in file order), stats.  device as in msa_center."""
    go, ro = np.ascontiguousarray(grp_off, np.uint64), np.ascontiguousarray(res_off, np.uint64)
    tr = [np.ascontiguousarray(t, np.uint8) for t in res]
    s3, sa = np.ascontiguousarray(S3, np.int8).reshape(-1), np.ascontiguousarray(SA, np.int8).reshape(-1)
    ng = len(go) - 1
    if ng < 0 or len(s3) != 441 or len(sa) != 441 or len(tr) != 2 or len(merges) != ng:
        raise ValueError("grp_off needs n_groups + 1 entries, S3 and SA are 21 x 21, res two tracks, merges one list per group")
    m = np.diff(go.astype(np.int64))
    ok = ng == 0 or ((m > 0).all() and int(go[0]) == 0)      # the call refuses the rest itself
    n_rows = int(go[-1]) if ng > 0 and ok else 0
    if len(ro) != n_rows + 1 and ok:
        raise ValueError("res_off needs n_rows + 1 entries")
    parts = [np.ascontiguousarray(x, np.uint32).reshape(-1) for x in merges]
    if ok and any(len(x) != 2 * (int(k) - 1) for x, k in zip(parts, m)):
        raise UcError(UC_ERR_ARGS, "progressive MSA: a group's merge list holds m - 1 pairs")
    mg = np.concatenate(parts + [np.zeros(1, np.uint32)])
    cap = 0
    if ok and ng and (np.diff(ro.astype(np.int64)) >= 0).all() and int(ro[0]) == 0:
        if any(len(t) < int(ro[-1]) for t in tr):
            raise ValueError("res_off reaches beyond res")
        cap = int(sum(int(m[g]) * (int(ro[int(go[g + 1])]) - int(ro[int(go[g])])) for g in range(ng)))
    width, out, need, st = np.zeros(max(ng, 1), np.uint32), [np.zeros(max(cap, 1), np.uint8) for _ in range(2)], np.zeros(1, np.uint64), UcMsaProgressiveStats()
    args = [ng, go.ctypes.data, ro.ctypes.data, _ptr(tr[0]), _ptr(tr[1]), mg.ctypes.data, s3.ctypes.data, sa.ctypes.data, gap_open, gap_ext, width.ctypes.data,
            out[0].ctypes.data, out[1].ctypes.data, cap, need.ctypes.data, C.byref(st)]
    _check(lib().uc_msa_progressive(*args, threads) if device is None else lib().uc_msa_progressive_dev(device, *args))
    return {"width": width[:ng], "cells": [o[: int(need[0])].copy() for o in out], "stats": {k: int(getattr(st, k)) for k, _ in UcMsaProgressiveStats._fields_}}


def tree(db, profile_dir, out_dir, threshold=50, aligner_options="", verbosity=1, device=-1, aligner="star", refine_iters=1):
    """== `unicore tree --no-inference -d threshold -o aligner_options <db> <profile_dir> <out_dir>` (uc_tree): a centre-star MSA of every gene
    file of a `profile` output on the engine's gapped stage, filtered and concatenated into out_dir/combined.fasta (+ .partitions, fasta/<gene>/*,
    tree.chk).  verbosity is Unicore's 0..4 scale.  UC_TREE_HOST=1 in the environment runs layout, rendering and filter through the host twins.
    Returns the stats dict (counts and seconds per phase).  aligner="profile" (uc_tree_refined, `-a profile --refine-iters refine_iters`): refine_iters
    (1 .. 8) rounds of profile refinement (UC-T/P) follow the star MSA; the dict then also holds "refine".  With aligner="star" refine_iters is not read."""
    if aligner not in ("star", "profile", "progressive"):
        raise ValueError("aligner is 'star', 'profile' or 'progressive'")
    o = make_opts("", 1, verbosity, device)
    if aligner == "progressive":      # uc_tree_progressive, `-a progressive` (UC-T/G): the dict then also holds "progressive"
        ps = UcTreeProgressiveStats()
        _check(lib().uc_tree_progressive(db.encode(), profile_dir.encode(), out_dir.encode(), threshold, (aligner_options or "").encode(), C.byref(o), C.byref(ps)))
        d = {k: int(getattr(ps.tree, k)) for k, _ in UcTreeStats._fields_ if k != "seconds"}
        d["seconds"] = dict(zip(TREE_PHASES, ps.tree.seconds))
        d["progressive"] = {k: int(getattr(ps, k)) for k, _ in UcTreeProgressiveStats._fields_ if k not in ("tree", "seconds")}
        d["progressive"]["seconds"] = dict(zip(TREE_PROGRESSIVE_PHASES, ps.seconds))
        return d
    if aligner == "profile":
        if not 1 <= int(refine_iters) <= TREE_MAX_REFINE:
            raise ValueError("refine_iters is 1 .. %d" % TREE_MAX_REFINE)
        rs = UcTreeRefinedStats()
        _check(lib().uc_tree_refined(db.encode(), profile_dir.encode(), out_dir.encode(), threshold, (aligner_options or "").encode(), int(refine_iters), C.byref(o), C.byref(rs)))
        st = rs.tree
    else:
        st = UcTreeStats()
        _check(lib().uc_tree(db.encode(), profile_dir.encode(), out_dir.encode(), threshold, (aligner_options or "").encode(), C.byref(o), C.byref(st)))
    d = {k: int(getattr(st, k)) for k, _ in UcTreeStats._fields_ if k != "seconds"}
    d["seconds"] = dict(zip(TREE_PHASES, st.seconds))
    if aligner == "profile":
        d["refine"] = {k: int(getattr(rs, k)) for k in ("n_rounds", "n_tasks", "n_cells", "n_rows_became_aligned", "n_rows_became_unaligned")}
        d["refine"].update(width_before=list(rs.width_before)[: int(rs.n_rounds)], width_after=list(rs.width_after)[: int(rs.n_rounds)],
                           seconds=dict(zip(TREE_REFINED_PHASES, rs.seconds)))
    return d


def nj_geometry():
    """The count kernel's geometry (uc_nj_geometry): {"tile": rows of a pair tile, "chunk": columns staged through LDS at a time}."""
    t, c = C.c_uint32(), C.c_uint32()
    _check(lib().uc_nj_geometry(C.byref(t), C.byref(c)))
    return {"tile": t.value, "chunk": c.value}


def nj_counts(cells, device=None, threads=1):
    """UC-N/D (uc_nj_counts / uc_nj_counts_dev): cells is n rows of w bytes (a 2-D uint8 array, or a list of equally long byte strings).  Returns
    (comp, diff), uint32 over the packed upper triangle (i < j at i n - i (i + 1) / 2 + (j - i - 1)): the columns where both cells are informative
    (an ASCII letter other than X / x) and those of them where the letters differ, case folded.  device as in msa_center; threads: the host twin's."""
    if isinstance(cells, (list, tuple)):
        if len({len(r) for r in cells}) > 1:
            raise ValueError("rows of unequal width")
        cells = np.frombuffer(b"".join(bytes(r) for r in cells), np.uint8).reshape(len(cells), -1) if cells else np.zeros((0, 0), np.uint8)
    ce = np.ascontiguousarray(cells, np.uint8)
    if ce.ndim != 2:
        raise ValueError("cells is n rows x w columns")
    n, w = ce.shape
    tri = max(n * (n - 1) // 2, 1)
    comp, diff = np.zeros(tri, np.uint32), np.zeros(tri, np.uint32)
    args = [n, w, _ptr(ce), threads, comp.ctypes.data, diff.ctypes.data]
    _check(lib().uc_nj_counts(*args) if device is None else lib().uc_nj_counts_dev(device, *args))
    return comp[: n * (n - 1) // 2], diff[: n * (n - 1) // 2]


def nj_distances(comp, diff, n, model="kimura"):
    """uc_nj_distances (host only): the n x n fp64 distance matrix of the counts under `model` ("kimura": min(5, -log(1 - p - 0.2 p p)), "p": p;
    5 where nothing compares).  An unknown model is UC_ERR_ARGS."""
    co, di = np.ascontiguousarray(comp, np.uint32), np.ascontiguousarray(diff, np.uint32)
    if len(co) != len(di) or (2 <= n <= 16384 and len(co) != n * (n - 1) // 2):
        raise ValueError("comp and diff hold n (n - 1) / 2 entries each")
    if model not in NJ_MODELS:
        raise UcError(UC_ERR_ARGS, "nj: unknown model '%s' (kimura, p)" % model)
    D = np.zeros((max(n, 1), max(n, 1)), np.float64)
    _check(lib().uc_nj_distances(_ptr(co), _ptr(di), n, NJ_MODELS[model], D.ctypes.data))
    return D


def nj_join(D, device=None):
    """UC-N/J (uc_nj_join / uc_nj_join_dev): neighbour joining on the symmetric n x n fp64 matrix D (not modified).  Returns a dict: join_a, join_b
    (uint32, n - 3: the nodes joined by every step; leaves are 0 .. n - 1, step s creates node n + s), len_a, len_b (fp64), root_node [3],
    root_len [3] (n == 2: two entries, the third NJ_NO_NODE / 0).  device as in msa_center."""
    d = np.ascontiguousarray(D, np.float64)
    if d.ndim != 2 or d.shape[0] != d.shape[1]:
        raise ValueError("D is n x n")
    n = d.shape[0]
    steps = max(n - 3, 0)
    ja, jb = np.zeros(max(steps, 1), np.uint32), np.zeros(max(steps, 1), np.uint32)
    la, lb = np.zeros(max(steps, 1), np.float64), np.zeros(max(steps, 1), np.float64)
    rn, rl = np.zeros(3, np.uint32), np.zeros(3, np.float64)
    args = [n, _ptr(d), ja.ctypes.data, jb.ctypes.data, la.ctypes.data, lb.ctypes.data, rn.ctypes.data, rl.ctypes.data]
    _check(lib().uc_nj_join(*args) if device is None else lib().uc_nj_join_dev(device, *args))
    return {"join_a": ja[:steps], "join_b": jb[:steps], "len_a": la[:steps], "len_b": lb[:steps], "root_node": rn, "root_len": rl}


def nj_newick(names, joins, support=None, n_rep=0, light=None, phi_sum=None):
    """uc_nj_newick / uc_nj_newick_support / uc_nj_newick_transfer (host only): the tree of nj_join's dict over the leaf names (str or bytes) as one
    Newick line with its newline (str).  With support (nj_support's array) and n_rep > 0 every internal node but the root carries its percentage,
    rounded half up.  With light and phi_sum (nj_transfer's light and the sum of its phi over the replicates) instead of support, the labels are
    UC-N/T's: the percentage of 1 - phi_sum / (n_rep (light - 1)), rounded half up."""
    nm = [x if isinstance(x, bytes) else x.encode() for x in names]
    arr = (C.c_char_p * max(len(nm), 1))(*nm)
    a = [np.ascontiguousarray(joins[k], t) for k, t in (("join_a", np.uint32), ("join_b", np.uint32), ("len_a", np.float64), ("len_b", np.float64),
                                                        ("root_node", np.uint32), ("root_len", np.float64))]
    need = C.c_uint64()
    ptrs = [_ptr(x) for x in a]
    if light is not None or phi_sum is not None:
        if support is not None:
            raise ValueError("support or (light, phi_sum), not both")
        li = None if light is None else np.ascontiguousarray(light, np.uint32)
        ps = None if phi_sum is None else np.ascontiguousarray(phi_sum, np.uint64)
        call = lambda buf, cap: lib().uc_nj_newick_transfer(arr, len(nm), *ptrs, None if li is None else _ptr(li), None if ps is None else _ptr(ps), n_rep, buf, cap, C.byref(need))
    elif support is None and not n_rep:
        call = lambda buf, cap: lib().uc_nj_newick(arr, len(nm), *ptrs, buf, cap, C.byref(need))
    else:
        su = None if support is None else np.ascontiguousarray(support, np.uint32)
        call = lambda buf, cap: lib().uc_nj_newick_support(arr, len(nm), *ptrs, None if su is None else _ptr(su), n_rep, buf, cap, C.byref(need))
    _check(call(None, 0))
    buf = C.create_string_buffer(need.value + 1)
    _check(call(C.cast(buf, C.c_void_p), need.value + 1))
    return buf.value.decode()


def nj_boot_geometry():
    """uc_nj_boot_geometry: {"lds_rows": the largest n whose batched join loop runs in LDS, one workgroup per replicate}."""
    r = C.c_uint32()
    _check(lib().uc_nj_boot_geometry(C.byref(r)))
    return {"lds_rows": r.value}


def nj_boot_columns(w, seed, rep):
    """UC-N/B (uc_nj_boot_columns, host only): the w source columns replicate `rep` draws under `seed`, uint32."""
    cols = np.zeros(max(min(w, 1 << 31), 1), np.uint32)
    _check(lib().uc_nj_boot_columns(w, seed & (2 ** 64 - 1), rep, cols.ctypes.data))
    return cols[:w]


def nj_boot_counts(rows, seed, rep0, n_rep, device=None, threads=1):
    """UC-N/B (uc_nj_boot_counts / uc_nj_boot_counts_dev): rows as nj_counts takes them.  Returns (comp, diff), uint32 [n_rep][n (n - 1) / 2]: the
    counts of replicates rep0 .. rep0 + n_rep - 1 over their drawn columns.  device as in msa_center; threads: the host twin's."""
    if isinstance(rows, (list, tuple)):
        if len({len(r) for r in rows}) > 1:
            raise ValueError("rows of unequal width")
        rows = np.frombuffer(b"".join(bytes(r) for r in rows), np.uint8).reshape(len(rows), -1) if rows else np.zeros((0, 0), np.uint8)
    ce = np.ascontiguousarray(rows, np.uint8)
    if ce.ndim != 2:
        raise ValueError("rows is n rows x w columns")
    n, w = ce.shape
    tri = n * (n - 1) // 2
    comp, diff = np.zeros((max(n_rep, 1), max(tri, 1)), np.uint32), np.zeros((max(n_rep, 1), max(tri, 1)), np.uint32)
    args = [n, w, _ptr(ce), seed & (2 ** 64 - 1), rep0, n_rep, threads, comp.ctypes.data, diff.ctypes.data]
    _check(lib().uc_nj_boot_counts(*args) if device is None else lib().uc_nj_boot_counts_dev(device, *args))
    return comp[:n_rep, :tri], diff[:n_rep, :tri]


def nj_join_batch(D, device=None):
    """UC-N/J on a batch (uc_nj_join_batch / uc_nj_join_batch_dev): D is [n_rep][n][n] fp64 (not modified).  Returns nj_join's dict with a leading
    replicate axis on every array; replicate b equals nj_join(D[b]) by bits.  device as in msa_center."""
    d = np.ascontiguousarray(D, np.float64)
    if d.ndim != 3 or d.shape[1] != d.shape[2]:
        raise ValueError("D is n_rep x n x n")
    B, n = d.shape[0], d.shape[1]
    steps = max(n - 3, 0)
    ja, jb = np.zeros((max(B, 1), max(steps, 1)), np.uint32), np.zeros((max(B, 1), max(steps, 1)), np.uint32)
    la, lb = np.zeros((max(B, 1), max(steps, 1)), np.float64), np.zeros((max(B, 1), max(steps, 1)), np.float64)
    rn, rl = np.zeros((max(B, 1), 3), np.uint32), np.zeros((max(B, 1), 3), np.float64)
    args = [n, B, _ptr(d), ja.ctypes.data, jb.ctypes.data, la.ctypes.data, lb.ctypes.data, rn.ctypes.data, rl.ctypes.data]
    _check(lib().uc_nj_join_batch(*args) if device is None else lib().uc_nj_join_batch_dev(device, *args))
    return {"join_a": ja[:B, :steps], "join_b": jb[:B, :steps], "len_a": la[:B, :steps], "len_b": lb[:B, :steps], "root_node": rn[:B], "root_len": rl[:B]}


def nj_support(n, joins, rep_join_a, rep_join_b):
    """UC-N/B (uc_nj_support, host only): joins is the main tree's nj_join dict over n leaves, rep_join_a / rep_join_b [n_rep][n - 3] the replicates'
    (nj_join_batch's arrays).  Returns uint32 [n - 3]: for the split of every join of the main tree, the replicates that hold the same split."""
    steps = max(n - 3, 0)
    ja, jb = np.ascontiguousarray(joins["join_a"], np.uint32), np.ascontiguousarray(joins["join_b"], np.uint32)
    ra, rb = np.ascontiguousarray(rep_join_a, np.uint32).reshape(-1, max(steps, 1)), np.ascontiguousarray(rep_join_b, np.uint32).reshape(-1, max(steps, 1))
    if len(ja) != steps or len(jb) != steps or ra.shape != rb.shape or (steps and ra.shape[1] != steps):
        raise ValueError("join arrays hold n - 3 entries per tree")
    B = ra.shape[0] if steps else 0
    out = np.zeros(max(steps, 1), np.uint32)
    _check(lib().uc_nj_support(n, _ptr(ja), _ptr(jb), B, _ptr(ra), _ptr(rb), out.ctypes.data))
    return out[:steps]


def nj_transfer_geometry():
    """The comparison kernel's geometry (uc_nj_transfer_geometry): {"tile": splits of a tile, "chunk": 32-bit words staged through LDS at a time,
    "host_leaves": the largest tree whose transfer phase tree_infer runs on the host twin also on a device run}."""
    t, c, h = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(lib().uc_nj_transfer_geometry(C.byref(t), C.byref(c), C.byref(h)))
    return {"tile": t.value, "chunk": c.value, "host_leaves": h.value}


def nj_transfer(n, joins, rep_join_a, rep_join_b, device=None, threads=1):
    """UC-N/T (uc_nj_transfer / uc_nj_transfer_dev): joins is the main tree's nj_join dict over n leaves, rep_join_a / rep_join_b [n_rep][n - 3] the
    replicates' (nj_join_batch's arrays).  Returns (phi, light): phi uint32 [n_rep][n - 3], the transfer index of every main-tree join in every
    replicate (0 exactly where the replicate holds the split), and light uint32 [n - 3], the smaller side of every main-tree split.  device as in
    msa_center; threads: the host twin's."""
    steps = max(n - 3, 0)
    ja, jb = np.ascontiguousarray(joins["join_a"], np.uint32), np.ascontiguousarray(joins["join_b"], np.uint32)
    ra, rb = np.ascontiguousarray(rep_join_a, np.uint32).reshape(-1, max(steps, 1)), np.ascontiguousarray(rep_join_b, np.uint32).reshape(-1, max(steps, 1))
    if len(ja) != steps or len(jb) != steps or ra.shape != rb.shape or (steps and ra.shape[1] != steps):
        raise ValueError("join arrays hold n - 3 entries per tree")
    B = ra.shape[0] if steps else 0
    phi, light = np.zeros((max(B, 1), max(steps, 1)), np.uint32), np.zeros(max(steps, 1), np.uint32)
    args = [n, _ptr(ja), _ptr(jb), B, _ptr(ra), _ptr(rb), threads, phi.ctypes.data, light.ctypes.data]
    _check(lib().uc_nj_transfer(*args) if device is None else lib().uc_nj_transfer_dev(device, *args))
    return phi[:B, :steps], light[:steps]


def tree_infer(fasta, out, model="kimura", verbosity=1, device=-1, threads=1, bootstrap=0, seed=1, support="fbp"):
    """== the inference step of `unicore tree -t nj` (uc_tree_infer): reads the aligned FASTA `fasta`, counts on the device, transforms under
    `model`, joins and writes the Newick line to `out`.  UC_TREE_HOST=1 in the environment runs the host twins (no GPU needed); UC_TREE_DUMP=1
    also writes <out>.dist.tsv.  Returns the stats dict (counts and seconds per phase).  bootstrap > 0 (uc_tree_infer_boot): `bootstrap`
    replicate trees drawn under `seed` label every internal branch of the same tree with its support; the stats dict is then the bootstrap's
    (replicates, batches, smallest and summed support, seconds per phase) and a dump also writes <out>.boot.tsv and <out>.boottrees.
    support: "fbp" (the share of replicates that hold the split) or "tbe" (uc_tree_infer_support: the transfer bootstrap expectation, UC-N/T);
    anything else is UC_ERR_ARGS, with or without replicates; without replicates it is unused."""
    if support not in NJ_SUPPORT_MODES:
        raise UcError(UC_ERR_ARGS, "nj: unknown support mode '%s' (fbp, tbe)" % (support,))
    if bootstrap:
        o, st = make_opts("", threads, verbosity, device), UcNjBootStats()
        if support == "fbp":
            _check(lib().uc_tree_infer_boot(fasta.encode(), out.encode(), None if model is None else model.encode(), bootstrap, seed & (2 ** 64 - 1), C.byref(o), C.byref(st)))
        else:
            _check(lib().uc_tree_infer_support(fasta.encode(), out.encode(), None if model is None else model.encode(), bootstrap, seed & (2 ** 64 - 1),
                                               NJ_SUPPORT_MODES[support], C.byref(o), C.byref(st)))
        d = {k: int(getattr(st, k)) for k, _ in UcNjBootStats._fields_ if k != "seconds"}
        d["seconds"] = dict(zip(NJ_BOOT_PHASES, st.seconds))
        return d
    o, st = make_opts("", threads, verbosity, device), UcNjStats()
    _check(lib().uc_tree_infer(fasta.encode(), out.encode(), None if model is None else model.encode(), C.byref(o), C.byref(st)))
    d = {k: int(getattr(st, k)) for k, _ in UcNjStats._fields_ if k != "seconds"}
    d["seconds"] = dict(zip(NJ_PHASES, st.seconds))
    return d


def hits_merge(n_seqs, max_seqs, parts):
    """parts: list of (counts u32[n_seqs], hits HIT_DTYPE[...]).  Host-only (no device needed)."""
    k = len(parts)
    cs = [np.ascontiguousarray(c, np.uint32) for c, _ in parts]
    hs = [np.ascontiguousarray(h, HIT_DTYPE) for _, h in parts]
    cp = (C.c_void_p * k)(*[c.ctypes.data for c in cs])
    hp = (C.c_void_p * k)(*[h.ctypes.data for h in hs])
    cap = int(sum(len(h) for h in hs))
    oc, oh, on = np.zeros(n_seqs, np.uint32), np.zeros(max(cap, 1), HIT_DTYPE), C.c_uint64()
    _check(lib().uc_hits_merge(n_seqs, max_seqs, k, cp, hp, oc.ctypes.data, oh.ctypes.data, cap, C.byref(on)))
    return oc, oh[: on.value].copy()


def createdb(fasta_paths, out_db, model, verbosity=1, device=-1, num_gpus=1):
    """== `foldseek createdb <fasta...> <db> --prostt5-model <model>` (createdb.rs:157-166): ProstT5 AA -> 3Di on the GPU(s);
    num_gpus: one encoder replica per GPU, sequences sharded over them (0 = all visible GPUs)"""
    if isinstance(fasta_paths, str):
        fasta_paths = [fasta_paths]
    arr = (C.c_char_p * len(fasta_paths))(*[p.encode() for p in fasta_paths])
    o, st = make_opts("", 1, verbosity, device, None, num_gpus), UcT5Stats()
    _check(lib().uc_createdb(arr, len(fasta_paths), out_db.encode(), model.encode(), C.byref(o), C.byref(st)))
    return {k: getattr(st, k) for k, _ in UcT5Stats._fields_}


_round_hook_keepalive = None


def set_round_hook(fn):
    """uc_set_round_hook: fn(round, ids, kmer_thr, view) is called once per workflow round of uc_cluster — after the round's gapped stage,
    before its set cover — with round = -1 for the linear-time pre-step, ids = database sequence number of every round-local index (a copy)
    and view = an Engine facade over the round's engine (hits_range / alns_range / stats; valid only during the call).  None unregisters."""
    global _round_hook_keepalive
    if fn is None:
        lib().uc_set_round_hook(ROUND_HOOK(), None)
        _round_hook_keepalive = None
        return

    def tramp(_user, rnd, m, ids, kthr, eng):
        view = Engine.__new__(Engine)
        view._h = C.c_void_p(eng)
        try:
            fn(int(rnd), np.ctypeslib.as_array(ids, shape=(int(m),)).copy(), int(kthr), view)
        finally:
            view._h = C.c_void_p()      # a view never destroys the engine it looked at
    cb = ROUND_HOOK(tramp)
    _round_hook_keepalive = cb
    lib().uc_set_round_hook(cb, None)


class T5Encoder:
    """the ProstT5 AA -> 3Di encoder (uc_t5_* of the C ABI)"""

    def __init__(self, model, device=-1):
        self._h = C.c_void_p()
        _check(lib().uc_t5_load(model.encode(), device, C.byref(self._h)))

    def close(self):
        if self._h:
            lib().uc_t5_free(self._h)
            self._h = C.c_void_p()

    def encode(self, seqs, logits=False):
        """seqs: list of residue strings -> list of uint8 arrays (3Di states 0..19) [, list of float32 [L, 20] logits]"""
        off = np.zeros(len(seqs) + 1, np.uint64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        aa = "".join(seqs).encode()
        codes = np.zeros(max(int(off[-1]), 1), np.uint8)
        lg = np.zeros((max(int(off[-1]), 1), 20), np.float32) if logits else None
        _check(lib().uc_t5_encode(self._h, len(seqs), off.ctypes.data, aa, codes.ctypes.data, lg.ctypes.data if logits else None))
        out = [codes[int(off[i]):int(off[i + 1])].copy() for i in range(len(seqs))]
        if logits:
            return out, [lg[int(off[i]):int(off[i + 1])].copy() for i in range(len(seqs))]
        return out

    def stats(self):
        st = UcT5Stats()
        _check(lib().uc_t5_get_stats(self._h, C.byref(st)))
        return {k: getattr(st, k) for k, _ in UcT5Stats._fields_}


# ---- kernel-level entry points of the ProstT5 encoder: numpy in, numpy out (f16 arrays cross the ABI as their uint16 bit patterns)
def _f16(a):
    return np.ascontiguousarray(a, np.float16).view(np.uint16)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def t5_gemm_variant(M, N, K):
    """the GEMM kernel the encoder picks for M x N x K: 0 = 128 x 128 tile, 1 = 256 x 256 tile, 2 = 256 x 256 persistent (host only)"""
    v = C.c_int32()
    _check(lib().uc_t5_gemm_variant(M, N, K, C.byref(v)))
    return v.value


def t5_kernel_gemm(A, W, epi, variant=-1, init=None, device=-1):
    """A [M, K], W [N, K] f16 -> A . W^T as f16 (epi 0), ReLU'd f16 (epi 1) or init + A . W^T in fp32 (epi 2, init [M, N] fp32)"""
    A, W = _f16(A), _f16(W)
    (M, K), N = A.shape, W.shape[0]
    if W.shape[1] != K:
        raise ValueError("A is [M, %d] but W is [N, %d]" % (K, W.shape[1]))
    if epi == 2:
        out = np.zeros((M, N), np.float32) if init is None else np.array(init, np.float32, order="C").reshape(M, N)
    else:
        out = np.zeros((M, N), np.uint16)
    _check(lib().uc_t5_kernel_gemm(device, variant, epi, M, N, K, A.ctypes.data, W.ctypes.data, out.ctypes.data))
    return out if epi == 2 else out.view(np.float16)


def t5_kernel_rmsnorm(x, w, eps, device=-1):
    """x [T, D] fp32, w [D] fp32 -> f16 [T, D]"""
    x, w = _f32(x), _f32(w)
    y = np.zeros(x.shape, np.uint16)
    _check(lib().uc_t5_kernel_rmsnorm(device, x.shape[0], x.shape[1], eps, x.ctypes.data, w.ctypes.data, y.ctypes.data))
    return y.view(np.float16)


def t5_kernel_attention(qkv, seq_len, bias, bias_span, n_heads, device=-1):
    """qkv [T, 3 * H * 128] f16 of the sequences packed in order, bias [H, 2 * bias_span - 1] fp32 -> f16 [T, H * 128]"""
    qkv, bias = _f16(qkv), _f32(bias)
    sl = np.ascontiguousarray(seq_len, np.int32)
    out = np.zeros((qkv.shape[0], n_heads * 128), np.uint16)
    _check(lib().uc_t5_kernel_attention(device, n_heads, len(sl), sl.ctypes.data, bias_span, bias.ctypes.data, qkv.ctypes.data, out.ctypes.data))
    return out.view(np.float16)


def t5_kernel_cnn_head(x, seq_len, w1, b1, w2, b2, eos_in_head, device=-1):
    """x [T, D] f16 (per sequence <AA2fold>, residues, </s>), w1 [C1, D, KW], b1 [C1], w2 [NO, C1, KW], b2 [NO] fp32
    -> (codes uint8 [T], logits fp32 [T, NO]) for every token"""
    x, w1, b1, w2, b2 = _f16(x), _f32(w1), _f32(b1), _f32(w2), _f32(b2)
    sl = np.ascontiguousarray(seq_len, np.int32)
    (C1, D, KW), NO, T = w1.shape, w2.shape[0], x.shape[0]
    codes, logits = np.zeros(T, np.uint8), np.zeros((T, NO), np.float32)
    _check(lib().uc_t5_kernel_cnn_head(device, len(sl), sl.ctypes.data, D, C1, KW, NO, int(eos_in_head), x.ctypes.data, w1.ctypes.data, b1.ctypes.data,
                                       w2.ctypes.data, b2.ctypes.data, codes.ctypes.data, logits.ctypes.data))
    return codes, logits


def t5_bias_table(rel_bias, max_dist, span):
    """rel_bias [H, buckets] fp32 -> the encoder's table [H, 2 * span - 1] over key - query in (-span, span) (host only)"""
    rb = _f32(rel_bias)
    out = np.zeros((rb.shape[0], 2 * span - 1), np.float32)
    _check(lib().uc_t5_bias_table(rb.shape[0], rb.shape[1], max_dist, span, rb.ctypes.data, out.ctypes.data))
    return out


class Comm:
    """RCCL communicator of the one-process-per-GPU layout (uc_comm_* of the C ABI).  Rank 0 calls Comm.unique_id()
    and ships the 128 bytes to the other ranks; creating the communicator is collective."""

    @staticmethod
    def unique_id():
        buf = (C.c_uint8 * 128)()
        _check(lib().uc_comm_unique_id(buf))
        return bytes(buf)

    def __init__(self, uid, rank, world, device=-1):
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _check(lib().uc_comm_create(buf, rank, world, device, C.byref(self._h)))

    def info(self):
        """(ranks, rank, device) as RCCL itself reports them (ncclCommCount / ncclCommUserRank / ncclCommCuDevice)"""
        n, r, d = C.c_int32(), C.c_int32(), C.c_int32()
        _check(lib().uc_comm_info(self._h, C.byref(n), C.byref(r), C.byref(d)))
        return n.value, r.value, d.value

    def close(self):
        if self._h:
            lib().uc_comm_destroy(self._h)
            self._h = C.c_void_p()


class Engine:
    """One engine = one HIP device with the sequence DB resident in HBM (uc_engine_* of the C ABI)."""

    def __init__(self, cluster_options="-c 0.8", threads=1, verbosity=1, device=-1, data_dir=None):
        self._h = C.c_void_p()
        o = make_opts(cluster_options, threads, verbosity, device, data_dir)
        _check(lib().uc_engine_create(C.byref(o), C.byref(self._h)))

    def close(self):
        if self._h:
            lib().uc_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_db(self, prefix):
        _check(lib().uc_engine_load_db(self._h, prefix.encode()))

    def set_db(self, off, s3, sa):
        off = np.ascontiguousarray(off, np.uint64)
        s3 = np.ascontiguousarray(s3, np.uint8)
        sa = np.ascontiguousarray(sa, np.uint8)
        _check(lib().uc_engine_set_db(self._h, len(off) - 1, off.ctypes.data, s3.ctypes.data, sa.ctypes.data))

    @property
    def n(self):
        return int(lib().uc_engine_num_seqs(self._h))

    def prefilter(self, tbegin=0, tend=None, qbegin=None, qend=None):
        tend = self.n if tend is None else tend
        if qbegin is None and qend is None:
            _check(lib().uc_engine_prefilter(self._h, tbegin, tend))
        else:
            _check(lib().uc_engine_prefilter_range(self._h, tbegin, tend, qbegin or 0, self.n if qend is None else qend))

    def hits_size(self):
        nh = C.c_uint64()
        _check(lib().uc_engine_hits_size(self._h, C.byref(nh)))
        return int(nh.value)

    def hits(self):
        nh = C.c_uint64()
        _check(lib().uc_engine_hits_size(self._h, C.byref(nh)))
        counts = np.zeros(self.n, np.uint32)
        hits = np.zeros(max(nh.value, 1), HIT_DTYPE)
        _check(lib().uc_engine_hits_get(self._h, counts.ctypes.data, hits.ctypes.data))
        return counts, hits[: nh.value]

    def hits_range(self, qbegin, qend):
        """(counts, hits) of the queries [qbegin, qend) only"""
        counts = np.zeros(max(qend - qbegin, 1), np.uint32)
        _check(lib().uc_engine_hits_get_range(self._h, qbegin, qend, counts.ctypes.data, None))
        counts = counts[: qend - qbegin]
        k = int(counts.sum())
        hits = np.zeros(max(k, 1), HIT_DTYPE)
        _check(lib().uc_engine_hits_get_range(self._h, qbegin, qend, None, hits.ctypes.data))
        return counts, hits[:k]

    def alns_range(self, qbegin, qend):
        """alignment records of the queries [qbegin, qend) only (one per hit, in hit order)"""
        counts, _ = np.zeros(max(qend - qbegin, 1), np.uint32), None
        _check(lib().uc_engine_hits_get_range(self._h, qbegin, qend, counts.ctypes.data, None))
        k = int(counts[: qend - qbegin].sum())
        out = np.zeros(max(k, 1), ALN_DTYPE)
        _check(lib().uc_engine_alns_get(self._h, qbegin, qend, out.ctypes.data))
        return out[:k]

    def set_hits(self, counts, hits):
        counts = np.ascontiguousarray(counts, np.uint32)
        hits = np.ascontiguousarray(hits, HIT_DTYPE)
        _check(lib().uc_engine_hits_set(self._h, counts.ctypes.data, hits.ctypes.data))

    def hits_export_dev(self, d_query, d_target, d_score, d_diag):
        """copy the device-resident hit lists into caller-owned DEVICE buffers (raw pointers, hits_size() x 4 B each)"""
        _check(lib().uc_engine_hits_export_dev(self._h, d_query, d_target, d_score, d_diag))

    def hits_import_dev(self, n, d_query, d_target, d_score, d_diag, rank=0, world=1):
        """install the merged union of shard lists given as DEVICE arrays; keeps the pairs owned by `rank`"""
        k = C.c_uint64()
        _check(lib().uc_engine_hits_import_dev(self._h, n, d_query, d_target, d_score, d_diag, rank, world, C.byref(k)))
        return int(k.value)

    def setcover(self, edges):
        """E7 with the graph built on this engine's GPU and the greedy cover on the host (same result as setcover())"""
        e = np.ascontiguousarray(edges, np.uint32).reshape(-1, 2)
        assign = np.zeros(self.n, np.uint32)
        _check(lib().uc_engine_setcover(self._h, e.ctypes.data, len(e), assign.ctypes.data))
        return assign

    def cluster_graph(self, edges, mode):
        """E7 on this engine's GPU by rule (uc_engine_cluster_graph): mode 0 = greedy set cover (== setcover()), 2 = greedy incremental with the
        lengths of the engine's database (same result as cluster_graph() of the module)"""
        e = np.ascontiguousarray(edges, np.uint32).reshape(-1, 2)
        assign = np.zeros(self.n, np.uint32)
        _check(lib().uc_engine_cluster_graph(self._h, mode, e.ctypes.data, len(e), assign.ctypes.data))
        return assign

    def reassign(self, assign):
        """Rule UC-1/R (--cluster-reassign, uc_engine_reassign) on the assignment `assign` of the engine's database under the engine's options.
        Returns (assign_out, rejected bool[n], counts dict: verified, rejected, research_accepted, clusters)."""
        a = np.ascontiguousarray(assign, np.uint32)
        if len(a) != self.n:
            raise ValueError("assign has %d entries for %d sequences" % (len(a), self.n))
        out, rej, cnt = np.zeros(self.n, np.uint32), np.zeros(max(self.n, 1), np.uint8), np.zeros(4, np.uint64)
        _check(lib().uc_engine_reassign(self._h, a.ctypes.data, out.ctypes.data, rej.ctypes.data, cnt.ctypes.data))
        return out, rej[: self.n].astype(bool), dict(zip(("verified", "rejected", "research_accepted", "clusters"), (int(x) for x in cnt)))

    def linclust_pairs(self, m=None, install=False):
        """E8a on the engine's database (uc_engine_linclust_pairs): the sorted unique (centre, member) pairs as uint32 [np, 2]; m=None takes the
        engine's --kmer-per-seq, otherwise m in [1, 1000].  install=True makes them the engine's hit lists (read them with hits()) and returns
        their number."""
        k = C.c_uint64()
        mm = 0 if m is None else int(m)
        if mm < 0 or (m is not None and mm == 0):
            raise UcError(UC_ERR_ARGS, "linclust_pairs: m must be None or in [1, 1000]")
        if install:
            _check(lib().uc_engine_linclust_pairs(self._h, mm, 1, None, 0, C.byref(k)))
            return int(k.value)
        cap = 1 << 16
        while True:
            out = np.zeros((cap, 2), np.uint32)
            _check(lib().uc_engine_linclust_pairs(self._h, mm, 0, out.ctypes.data, cap, C.byref(k)))
            if k.value <= cap:
                return out[: k.value].copy()
            cap = int(k.value)

    def align(self, qbegin=0, qend=None):
        _check(lib().uc_engine_align(self._h, qbegin, self.n if qend is None else qend))

    def cluster_step(self, comm=None, target_shards=0):
        """One pass of the (sharded) hot path inside the library: prefilter of this rank's grid cell -> RCCL hit all-gather +
        device merge -> E5/E6 -> edges to rank 0 -> set cover there.  Returns (assign or None, gapped alignments of this rank)."""
        rank0 = comm is None or comm.rank == 0
        assign = np.zeros(self.n, np.uint32) if rank0 else None
        k = C.c_uint64()
        _check(lib().uc_engine_cluster_step(self._h, comm._h if comm is not None else None, target_shards,
                                            assign.ctypes.data if rank0 else None, C.byref(k)))
        return assign, int(k.value)

    def alns(self, qbegin=0, qend=None):
        qend = self.n if qend is None else qend
        counts, _ = self.hits()
        n = int(counts[qbegin:qend].sum())
        out = np.zeros(max(n, 1), ALN_DTYPE)
        _check(lib().uc_engine_alns_get(self._h, qbegin, qend, out.ctypes.data))
        return out[:n]

    def edges(self):
        ne = C.c_uint64()
        _check(lib().uc_engine_edges_size(self._h, C.byref(ne)))
        e = np.zeros((max(ne.value, 1), 2), np.uint32)
        _check(lib().uc_engine_edges_get(self._h, e.ctypes.data))
        return e[: ne.value]

    def stats(self):
        st = UcStats()
        _check(lib().uc_engine_stats(self._h, C.byref(st)))
        d = st.as_dict()
        # what the prefilter's on-chip diagonal selection took since the last reset (uc_engine_td_onchip: not part of uc_stats)
        td = (C.c_uint64 * 4)()
        _check(lib().uc_engine_td_onchip(self._h, td))
        d["td_onchip_queries"], d["td_onchip_keys"] = int(td[0]), int(td[2])
        # class launches of the packed gapped kernel that served several tasks per workgroup, and their tasks (uc_engine_sw_task_queries)
        mq = (C.c_uint64 * 2)()
        _check(lib().uc_engine_sw_task_queries(self._h, mq))
        d["sw_multiquery_launches"], d["sw_multiquery_tasks"] = int(mq[0]), int(mq[1])
        return d

    def reset_stats(self):
        lib().uc_engine_reset_stats(self._h)

    def ungapped(self, q, t, diag):
        q = np.ascontiguousarray(q, np.uint32); t = np.ascontiguousarray(t, np.uint32)
        diag = np.ascontiguousarray(diag, np.int32)
        out = np.zeros(len(q), np.int32)
        _check(lib().uc_engine_ungapped_batch(self._h, len(q), q.ctypes.data, t.ctypes.data, diag.ctypes.data, out.ctypes.data))
        return out

    def ungapped_select(self, q, t, diag, min_score):
        """E3 and E4's key pass on explicit candidates (uc_engine_ungapped_select): (scores, overlap residues counted, candidates kept)"""
        q = np.ascontiguousarray(q, np.uint32); t = np.ascontiguousarray(t, np.uint32)
        diag = np.ascontiguousarray(diag, np.int32)
        out = np.zeros(len(q), np.int32)
        ovl, kept = C.c_uint64(0), C.c_uint64(0)
        _check(lib().uc_engine_ungapped_select(self._h, len(q), q.ctypes.data, t.ctypes.data, diag.ctypes.data, int(min_score), out.ctypes.data,
                                               C.byref(ovl), C.byref(kept)))
        return out, int(ovl.value), int(kept.value)

    def ungapped_all(self, qbegin=0, qend=None, tbegin=0, tend=None, tile_bytes=0):
        """Rule UC-1/X (--prefilter-mode 1) on queries [qbegin, qend) x targets [tbegin, tend): dense int32 arrays (score, diag) of that shape,
        the best ungapped score over all diagonals (capped at 255) and the smallest diagonal that reaches it.  tile_bytes: the tile budget (0 = default)."""
        qend = self.n if qend is None else qend
        tend = self.n if tend is None else tend
        score = np.zeros((max(qend - qbegin, 0), max(tend - tbegin, 0)), np.int32)
        diag = np.zeros_like(score)
        _check(lib().uc_engine_ungapped_all(self._h, qbegin, qend, tbegin, tend, tile_bytes, score.ctypes.data, diag.ctypes.data))
        return score, diag

    def sw(self, mode, q, t, qend=None, tend=None):
        q = np.ascontiguousarray(q, np.uint32); t = np.ascontiguousarray(t, np.uint32)
        n = len(q)
        qe = np.ascontiguousarray(qend, np.int32) if qend is not None else None
        te = np.ascontiguousarray(tend, np.int32) if tend is not None else None
        s, oq, ot = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        _check(lib().uc_engine_sw_batch(self._h, mode, n, q.ctypes.data, t.ctypes.data,
                                        qe.ctypes.data if qe is not None else None, te.ctypes.data if te is not None else None,
                                        s.ctypes.data, oq.ctypes.data, ot.ctypes.data))
        return s, oq, ot

    def backtraces(self, qbegin=0, qend=None):
        """(run_off, runs) of the hits of queries [qbegin, qend), aligned with alns_range: slice k = runs[run_off[k]:run_off[k + 1]],
        words length << 2 | op (0 M, 1 I, 2 D); needs -a in the engine's options (uc_engine_backtraces_get)"""
        qend = self.n if qend is None else qend
        k = C.c_uint64(0)
        _check(lib().uc_engine_backtraces_size(self._h, qbegin, qend, C.byref(k)))
        nh = C.c_uint64(0)
        _check(lib().uc_engine_hits_size(self._h, C.byref(nh)))
        off = np.zeros(nh.value + 2, np.uint64)       # at least one per hit of the range + 1
        runs = np.zeros(max(k.value, 1), np.uint32)
        _check(lib().uc_engine_backtraces_get(self._h, qbegin, qend, off.ctypes.data, runs.ctypes.data))
        return off, runs[: k.value]

    def tb_emit_pass(self, route, q, t, box, known=None, band=0):
        """ONE traceback pass with backtrace emission (uc_engine_tb_emit_pass): route 0 banded packed MODE 7 + walk, 1 whole box,
        2 stored int32 matrix, 3 long-query route.  Returns a dict: cls, aln_len, idents, gaps, miss, plain (int32) and cigar (list of str)."""
        q = np.ascontiguousarray(q, np.uint32); t = np.ascontiguousarray(t, np.uint32)
        n = len(q)
        bx = np.ascontiguousarray(box, np.int32).reshape(n, 4)
        kn = np.ascontiguousarray(known, np.int32) if known is not None else None
        out = {k: np.full(n, -1, np.int32) for k in ("cls", "aln_len", "idents", "gaps", "miss", "plain")}
        cap = int((bx[:, 1] - bx[:, 0] + 1).sum() + (bx[:, 3] - bx[:, 2] + 1).sum()) + 1     # a path has at most rows + columns steps
        off = np.zeros(n + 1, np.uint64)
        runs = np.zeros(cap, np.uint32)
        k = C.c_uint64(0)
        _check(lib().uc_engine_tb_emit_pass(self._h, route, band, n, q.ctypes.data, t.ctypes.data, bx.ctypes.data,
                                            kn.ctypes.data if kn is not None else None,
                                            *[out[x].ctypes.data for x in ("cls", "aln_len", "idents", "gaps", "miss", "plain")],
                                            off.ctypes.data, runs.ctypes.data, cap, C.byref(k)))
        out["cigar"] = [render_backtrace(runs[int(off[i]):int(off[i + 1])]) if off[i + 1] > off[i] else "" for i in range(n)]
        return out

    def sw_pass(self, table, mode, q, t, box=None, known=None, band=0, raw=False, second=False):
        """ONE gapped pass (class table, mode) on the pairs (q[i], t[i]), as Engine.align runs it (uc_engine_sw_pass):
        box [n, 4] = (qs, qe, ts, te), known [n] optimum scores.  Returns a dict of int32 arrays: score, qe, te, cls,
        aln_len, idents, gaps, miss.  second=True (modes 4 / 6, uc_engine_sw_pass2): also qe2, te2, the optimal cell in the
        first optimal row, then the first column - the answer of the pair (t, q) with the roles swapped; -2 where absent."""
        q = np.ascontiguousarray(q, np.uint32); t = np.ascontiguousarray(t, np.uint32)
        n = len(q)
        bx = np.ascontiguousarray(box, np.int32).reshape(n, 4) if box is not None else None
        kn = np.ascontiguousarray(known, np.int32) if known is not None else None
        names = ("score", "qe", "te", "cls", "aln_len", "idents", "gaps", "miss") + (("qe2", "te2") if second else ())
        out = {k: np.full(n, -1, np.int32) for k in names}
        fn = lib().uc_engine_sw_pass2 if second else lib().uc_engine_sw_pass
        _check(fn(self._h, table, mode, band, int(bool(raw)), n, q.ctypes.data, t.ctypes.data,
                  bx.ctypes.data if bx is not None else None, kn.ctypes.data if kn is not None else None,
                  *[out[k].ctypes.data for k in names]))
        return out
