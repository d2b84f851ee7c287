"""ctypes binding of libmyfm_hip.so (include/myfm_hip.h) -- used by the parity tests and bench.py
to reach the device path through the C ABI itself. The estimator layer goes through the pybind11
module ``myfm_amd._myfm`` (host C++), which links the same library.

There is no fallback: a missing library is an ImportError, a missing GPU is a RuntimeError.
"""
import ctypes as C
import os

import numpy as np
import scipy.sparse as sps

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmyfm_hip.so")

MFM_OK, MFM_ERR_INVALID, MFM_ERR_RUNTIME, MFM_ERR_DEVICE = 0, 1, 2, 3
TASK_REGRESSION, TASK_CLASSIFICATION, TASK_ORDERED = 0, 1, 2

# every symbol declared in include/myfm_hip.h (tests check the library exports all of them)
SYMBOLS = [
    "mfm_version", "mfm_device_count", "mfm_global_error", "mfm_create", "mfm_destroy", "mfm_last_error",
    "mfm_set_stream", "mfm_synchronize", "mfm_set_main", "mfm_add_block", "mfm_set_groups", "mfm_finalize",
    "mfm_peer_info", "mfm_peer_set", "mfm_peer_model_info", "mfm_peer_set_model", "mfm_peer_export", "mfm_peer_import", "mfm_peer_drop", "mfm_set_residual_policy", "mfm_dim_all", "mfm_plan_info", "mfm_plan_flags", "mfm_res_info", "mfm_cell_info", "mfm_chain_stream_info", "mfm_set_state", "mfm_get_state", "mfm_set_w0", "mfm_zero_w", "mfm_get_e",
    "mfm_get_q", "mfm_set_e", "mfm_reduce_e", "mfm_shift_e", "mfm_group_stats_w", "mfm_group_stats_V",
    "mfm_sweep_w", "mfm_sweep_V", "mfm_sweep_wV", "mfm_update_e_regression", "mfm_update_e_classification", "mfm_score_train",
    "mfm_oprobit_add_group", "mfm_oprobit_eval", "mfm_oprobit_sample_z", "mfm_hyper_stats", "mfm_timing_enable", "mfm_timing_select", "mfm_timing_reset",
    "mfm_timing_n_classes", "mfm_timing_class_name", "mfm_timing_get", "mfm_design_create", "mfm_design_add_block",
    "mfm_design_destroy", "mfm_design_last_error", "mfm_design_dim_all", "mfm_design_predict",
    "mfm_host_column_levels", "mfm_rng_prepare", "mfm_rng_seed_mt19937", "mfm_rng_set_program", "mfm_rng_prefetch", "mfm_rng_acquire",
    "mfm_rng_get_z", "mfm_design_score_ctx", "mfm_design_n_rows", "mfm_set_allreduce", "mfm_set_row_offset", "mfm_set_main_levels",
    "mfm_test_erfcx", "mfm_test_truncated_normal", "mfm_get_device", "mfm_set_shard", "mfm_comm_unique_id", "mfm_comm_init",
    "mfm_comm_stats", "mfm_comm_info", "mfm_store_create", "mfm_store_destroy", "mfm_store_last_error", "mfm_store_size", "mfm_store_push_ctx",
    "mfm_store_push_host", "mfm_store_get", "mfm_design_predict_store", "mfm_store_reserve", "mfm_cs_plan_selftest", "mfm_cs_plan_probe",
    "mfm_regression_iteration_ready", "mfm_regression_iteration",
    "mfm_update_e_classification_exact", "mfm_oprobit_sample_z_exact", "mfm_latent_stats", "mfm_rng_host_read", "mfm_rng_host_advance", "mfm_set_latent_order",
    "mfm_vb_create", "mfm_vb_add_block", "mfm_vb_finalize", "mfm_vb_destroy", "mfm_vb_last_error", "mfm_vb_plan_info", "mfm_vb_set_state", "mfm_vb_get_state",
    "mfm_vb_set_w0", "mfm_vb_update_e", "mfm_vb_shift_e", "mfm_vb_get_e", "mfm_vb_get_cache", "mfm_vb_zero_w", "mfm_vb_sweep_w",
    "mfm_vb_sweep_V", "mfm_vb_group_stats", "mfm_vb_synchronize", "mfm_vb_truncated_normal",
    "mfm_vb_set_stream", "mfm_vb_set_allreduce", "mfm_vb_set_shard", "mfm_vb_comm_init", "mfm_vb_comm_stats", "mfm_vb_set_levels",
    "mfm_vb_design_levels",
    "mfm_pairs_create", "mfm_pairs_destroy", "mfm_pairs_last_error", "mfm_pairs_set_exclude", "mfm_pairs_set_scratch_bound",
    "mfm_pairs_scores_store", "mfm_pairs_topk_store", "mfm_pairs_scores", "mfm_pairs_topk", "mfm_pairs_add_block",
    "mfm_pairs_set_cutpoints", "mfm_pairs_moments_store", "mfm_pairs_moments", "mfm_pairs_topk_ucb_store", "mfm_pairs_topk_ucb",
    "mfm_pairs_set_targets", "mfm_pairs_rank_store", "mfm_pairs_rank",
    "mfm_pairs_topk_samples_store", "mfm_pairs_topk_samples", "mfm_pairs_topk_prob_store", "mfm_pairs_topk_prob",
    "mfm_pairs_create_sim", "mfm_pairs_sim_store", "mfm_pairs_sim", "mfm_pairs_topk_sim_store", "mfm_pairs_topk_sim",
    "mfm_foldin_create", "mfm_foldin_destroy", "mfm_foldin_last_error", "mfm_foldin_set_scratch_bound", "mfm_foldin_max_rank",
    "mfm_foldin_solve_store", "mfm_foldin_solve", "mfm_foldin_gibbs_solve_store", "mfm_foldin_gibbs_solve",
    "mfm_design_summary_store", "mfm_design_summary", "mfm_design_summary_oprobit_store", "mfm_design_summary_oprobit",
    "mfm_design_logdens_store", "mfm_design_logdens", "mfm_logdens_value",
    "mfm_design_loo_store", "mfm_design_loo", "mfm_psis_row",
    "mfm_design_ess_store", "mfm_design_ess", "mfm_ess_row", "mfm_rank_z_table",
    "mfm_design_ess_chains_store", "mfm_design_ess_chains", "mfm_ess_row_chains", "mfm_ess_check_chains", "mfm_ess_max_chains",
    "mfm_design_crps_store", "mfm_design_crps", "mfm_crps_row",
    "mfm_design_loo_summary_store", "mfm_design_loo_summary", "mfm_design_loo_crps_store", "mfm_design_loo_crps",
    "mfm_loo_summary_row", "mfm_loo_crps_row",
    "mfm_design_contrib_store", "mfm_design_contrib", "mfm_contrib_row",
    "mfm_design_moments_vb", "mfm_pairs_moments_vb", "mfm_pairs_topk_bound_vb",
]

SIM_METRICS = {"cosine": 0, "dot": 1}  # (MFM_PAIRS_SIM_* of myfm_hip.h)
PAIRS_VOTE_MAX = 32768  # (MFM_PAIRS_VOTE_MAX of myfm_hip.h: samples * k of a topk_prob call)

# a record of mfm_chain_stream_info / mfm_cs_plan_probe (MFM_CHAIN_STREAM_INFO_FIELDS of include/myfm_hip.h)
CHAIN_STREAM_INFO = ("block", "n_cols", "n_steps", "Cg", "Lw", "NB", "RD", "n_slots", "max_hot_col", "max_enter", "max_exit", "max_cold_sr",
                     "max_enter_sr", "max_exit_sr", "n_cols_no_hot")
CHAIN_STREAM_INFO_TAIL = ("lds_bytes", "n_cold", "n_hot", "launches_w", "launches_V")
CHAIN_STREAM_INFO_FIELDS = len(CHAIN_STREAM_INFO) + 10 + len(CHAIN_STREAM_INFO_TAIL)


def chain_stream_record(rec):
    n = len(CHAIN_STREAM_INFO)
    d = dict(zip(CHAIN_STREAM_INFO, (int(v) for v in rec[:n])))
    d["hot_rounds"] = [int(v) for v in rec[n:n + 10]]
    d.update(zip(CHAIN_STREAM_INFO_TAIL, (int(v) for v in rec[n + 10:])))
    return d


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH
        )
    from ._build import preload_hip_runtime

    preload_hip_runtime()
    L = C.CDLL(LIB_PATH)
    vp, i64, i32, dbl, P = C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p
    u64 = C.c_uint64
    L.mfm_version.restype = C.c_char_p
    L.mfm_global_error.restype = C.c_char_p
    L.mfm_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.mfm_destroy.argtypes = [vp]
    L.mfm_destroy.restype = None
    L.mfm_last_error.restype = C.c_char_p
    L.mfm_last_error.argtypes = [vp]
    L.mfm_set_stream.argtypes = [vp, vp]
    L.mfm_synchronize.argtypes = [vp]
    L.mfm_set_main.argtypes = [vp, i64, i64, P, P, P, P]
    L.mfm_add_block.argtypes = [vp, i64, i64, P, P, P, P]
    L.mfm_set_groups.argtypes = [vp, P, i64, i32]
    L.mfm_finalize.argtypes = [vp, i32]
    L.mfm_peer_info.argtypes = [vp, P, P, P, P, P]
    L.mfm_peer_set.argtypes = [vp, i32, i32, P, P]
    L.mfm_peer_model_info.argtypes = [vp, P, P]
    L.mfm_peer_set_model.argtypes = [vp, i32, i32, P, P]
    L.mfm_peer_export.argtypes = [vp, P]
    L.mfm_peer_import.argtypes = [vp, i32, i32, P]
    L.mfm_peer_drop.argtypes = [vp]
    L.mfm_regression_iteration_ready.argtypes = [vp]
    L.mfm_regression_iteration.argtypes = [vp, P, P, P, P, P, P, P, P]
    L.mfm_set_residual_policy.argtypes = [vp, i32]
    L.mfm_dim_all.restype = i64
    L.mfm_dim_all.argtypes = [vp]
    L.mfm_plan_info.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.mfm_plan_flags.argtypes = [vp]
    L.mfm_res_info.argtypes = [vp, P, C.c_int, C.c_char_p, C.c_int]
    L.mfm_cell_info.argtypes = [vp, P, C.c_int, C.c_char_p, C.c_int]
    L.mfm_chain_stream_info.argtypes = [vp, P, C.c_int, C.POINTER(C.c_int)]
    L.mfm_cs_plan_probe.argtypes = [i64, i32, P, P, P, i32, i32, i32, i32, P, P, C.POINTER(i32), C.POINTER(dbl)]
    L.mfm_set_state.argtypes = [vp, dbl, P, P]
    L.mfm_get_state.argtypes = [vp, C.POINTER(dbl), P, P]
    L.mfm_set_w0.argtypes = [vp, dbl]
    L.mfm_zero_w.argtypes = [vp]
    L.mfm_get_e.argtypes = [vp, P]
    L.mfm_get_q.argtypes = [vp, P]
    L.mfm_set_e.argtypes = [vp, P]
    L.mfm_reduce_e.argtypes = [vp, C.POINTER(dbl), C.POINTER(dbl)]
    L.mfm_shift_e.argtypes = [vp, dbl]
    L.mfm_group_stats_w.argtypes = [vp, P, P, P]
    L.mfm_group_stats_V.argtypes = [vp, P, P, P]
    L.mfm_hyper_stats.argtypes = [vp, C.c_int32, P, P, P, P, P, P, P, P]
    L.mfm_sweep_w.argtypes = [vp, dbl, P, P, P]
    L.mfm_sweep_V.argtypes = [vp, i32, i32, dbl, P, P, P]
    L.mfm_sweep_wV.argtypes = [vp, dbl, dbl, P, P, P, i32, i32, P, P, P]
    L.mfm_update_e_regression.argtypes = [vp]
    L.mfm_update_e_classification.argtypes = [vp, u64, u64]
    L.mfm_score_train.argtypes = [vp]
    L.mfm_oprobit_add_group.argtypes = [vp, i32, P, i64, C.POINTER(i32)]
    L.mfm_oprobit_eval.argtypes = [vp, i32, P, C.POINTER(dbl), P, P]
    L.mfm_oprobit_sample_z.argtypes = [vp, i32, P, u64, u64]
    L.mfm_timing_enable.argtypes = [vp, C.c_int]
    L.mfm_timing_select.argtypes = [vp, C.c_int32]
    L.mfm_timing_reset.argtypes = [vp]
    L.mfm_timing_class_name.restype = C.c_char_p
    L.mfm_timing_class_name.argtypes = [C.c_int]
    L.mfm_timing_get.argtypes = [vp, C.c_int, C.POINTER(dbl), C.POINTER(i64), C.POINTER(dbl)]
    L.mfm_design_create.argtypes = [C.c_int, i64, i64, P, P, P, C.POINTER(vp)]
    L.mfm_design_add_block.argtypes = [vp, i64, i64, P, P, P, P]
    L.mfm_design_destroy.argtypes = [vp]
    L.mfm_design_destroy.restype = None
    L.mfm_design_last_error.restype = C.c_char_p
    L.mfm_design_last_error.argtypes = [vp]
    L.mfm_design_dim_all.restype = i64
    L.mfm_design_dim_all.argtypes = [vp]
    L.mfm_design_predict.argtypes = [vp, i32, i32, P, P, P, i32, i32, P, P]
    L.mfm_host_column_levels.argtypes = [i64, i64, P, P, P, C.POINTER(i32)]
    L.mfm_rng_prepare.argtypes = [i64, i32, i32]
    L.mfm_rng_seed_mt19937.argtypes = [vp, P, i32]
    L.mfm_rng_set_program.argtypes = [vp, P, i32]
    L.mfm_rng_prefetch.argtypes = [vp]
    L.mfm_rng_acquire.argtypes = [vp, P, i64]
    L.mfm_rng_get_z.argtypes = [vp, P, P]
    L.mfm_update_e_classification_exact.argtypes = [vp, C.POINTER(i32)]
    L.mfm_oprobit_sample_z_exact.argtypes = [vp, i32, P, C.POINTER(i32)]
    L.mfm_latent_stats.argtypes = [vp, P]
    L.mfm_set_latent_order.argtypes = [vp, P, i64]
    L.mfm_rng_host_read.argtypes = [vp, u64, i64, P]
    L.mfm_rng_host_advance.argtypes = [vp, u64]
    L.mfm_design_score_ctx.argtypes = [vp, vp, P]
    L.mfm_design_n_rows.restype = i64
    L.mfm_design_n_rows.argtypes = [vp]
    L.mfm_set_allreduce.argtypes = [vp, vp, vp]
    L.mfm_set_row_offset.argtypes = [vp, i64]
    L.mfm_set_main_levels.argtypes = [vp, P, i64]
    L.mfm_get_device.argtypes = [vp]
    L.mfm_set_shard.argtypes = [vp, i32, i32]
    L.mfm_comm_unique_id.argtypes = [P]
    L.mfm_comm_init.argtypes = [vp, P, i32, i32]
    L.mfm_comm_stats.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
    L.mfm_comm_info.argtypes = [vp, C.POINTER(i32), C.c_char_p, i64]
    L.mfm_store_create.argtypes = [C.c_int, i64, i32, C.POINTER(vp)]
    L.mfm_store_destroy.argtypes = [vp]
    L.mfm_store_destroy.restype = None
    L.mfm_store_last_error.restype = C.c_char_p
    L.mfm_store_last_error.argtypes = [vp]
    L.mfm_store_size.argtypes = [vp]
    L.mfm_store_reserve.argtypes = [vp, i32]
    L.mfm_store_push_ctx.argtypes = [vp, vp]
    L.mfm_store_push_host.argtypes = [vp, dbl, P, P]
    L.mfm_store_get.argtypes = [vp, i32, C.POINTER(dbl), P, P]
    L.mfm_design_predict_store.argtypes = [vp, vp, i32, i32, i32, i32, P, P]
    L.mfm_design_summary_store.argtypes = [vp, vp, i32, i32, i32, i32, P, P, P, i64, i32, P, P, P]
    L.mfm_design_summary.argtypes = [vp, i32, i32, P, P, P, i32, i32, P, P, P, i64, i32, P, P, P]
    L.mfm_design_summary_oprobit_store.argtypes = [vp, vp, i32, i32, i32, i32, P, i32, P, i64, i32, P, P, P]
    L.mfm_design_summary_oprobit.argtypes = [vp, i32, i32, P, P, P, i32, i32, P, i32, P, i64, i32, P, P, P]
    L.mfm_design_logdens_store.argtypes = [vp, vp, i32, i32, i32, P, P, i32, P, i64, i32, P, P, P, P, P]
    L.mfm_design_logdens.argtypes = [vp, i32, i32, P, P, P, i32, P, P, i32, P, i64, i32, P, P, P, P, P]
    L.mfm_logdens_value.argtypes = [i32, dbl, dbl, dbl, dbl, i32, P, P]
    L.mfm_design_loo_store.argtypes = [vp, vp, i32, i32, i32, P, P, i32, P, i64, i32, i32, P, P, P, P, P]
    L.mfm_design_loo.argtypes = [vp, i32, i32, P, P, P, i32, P, P, i32, P, i64, i32, i32, P, P, P, P, P]
    L.mfm_psis_row.argtypes = [i32, i32, P, P, P, P]
    L.mfm_design_ess_store.argtypes = [vp, vp, i32, i32, i32, i32, P, P, i32, P, i64, i32, P, P, P, P]
    L.mfm_design_ess.argtypes = [vp, i32, i32, P, P, P, i32, i32, P, P, i32, P, i64, i32, P, P, P, P]
    L.mfm_ess_row.argtypes = [i32, P, P, P]
    L.mfm_design_ess_chains_store.argtypes = [vp, vp, i32, i32, i32, i32, i32, P, P, i32, P, i64, i32, P, P, P, P]
    L.mfm_design_ess_chains.argtypes = [vp, i32, i32, P, P, P, i32, i32, i32, P, P, i32, P, i64, i32, P, P, P, P]
    L.mfm_ess_row_chains.argtypes = [i32, i32, P, P, P]
    L.mfm_ess_check_chains.argtypes = [i32, i32]
    L.mfm_ess_max_chains.argtypes = []
    L.mfm_rank_z_table.argtypes = [i32, P]
    L.mfm_design_crps_store.argtypes = [vp, vp, i32, i32, i32, P, P, i32, P, i64, i32, P, P, P]
    L.mfm_design_crps.argtypes = [vp, i32, i32, P, P, P, i32, P, P, i32, P, i64, i32, P, P, P]
    L.mfm_crps_row.argtypes = [i32, i32, dbl, P, P, i32, P, P]
    L.mfm_design_loo_summary_store.argtypes = [vp, vp, i32, i32, i32, P, P, i32, P, i64, i32, i32, i32, P, P, P, P, P, P, P]
    L.mfm_design_loo_summary.argtypes = [vp, i32, i32, P, P, P, i32, P, P, i32, P, i64, i32, i32, i32, P, P, P, P, P, P, P]
    L.mfm_design_contrib_store.argtypes = [vp, vp, i32, i32, i32, P, i64, i64, i32, P, P, P, P, P]
    L.mfm_design_contrib.argtypes = [vp, i32, i32, P, P, P, i32, P, i64, i64, i32, P, P, P, P, P]
    L.mfm_contrib_row.argtypes = [i32, P, P, i64, i32, i32, P, P, i32, P, i64, P, P]
    L.mfm_design_loo_crps_store.argtypes = [vp, vp, i32, i32, i32, P, P, i32, P, i64, i32, i32, P, P, P, P]
    L.mfm_design_loo_crps.argtypes = [vp, i32, i32, P, P, P, i32, P, P, i32, P, i64, i32, i32, P, P, P, P]
    L.mfm_loo_summary_row.argtypes = [i32, P, P, P, i32, P, P, P, P, P, P]
    L.mfm_loo_crps_row.argtypes = [i32, i32, dbl, P, P, P, i32, P, P]
    L.mfm_pairs_create.argtypes = [C.c_int, i64, i64, P, P, P, i64, P, P, P, C.POINTER(vp)]
    L.mfm_pairs_create_sim.argtypes = L.mfm_pairs_create.argtypes
    L.mfm_pairs_sim_store.argtypes = [vp, vp, i32, i32, i32, P, P]
    L.mfm_pairs_sim.argtypes = [vp, i32, i32, P, P, P, i32, P, P]
    L.mfm_pairs_topk_sim_store.argtypes = [vp, vp, i32, i32, i32, i32, C.c_double, P, P, P, P]
    L.mfm_pairs_topk_sim.argtypes = [vp, i32, i32, P, P, P, i32, i32, C.c_double, P, P, P, P]
    L.mfm_pairs_destroy.argtypes = [vp]
    L.mfm_pairs_destroy.restype = None
    L.mfm_pairs_last_error.restype = C.c_char_p
    L.mfm_pairs_last_error.argtypes = [vp]
    L.mfm_pairs_set_exclude.argtypes = [vp, P, P]
    L.mfm_pairs_set_scratch_bound.argtypes = [vp, i64]
    L.mfm_pairs_add_block.argtypes = [vp, i32, i64, i64, i64, P, P, P, P]
    L.mfm_pairs_set_cutpoints.argtypes = [vp, i32, i32, P]
    L.mfm_pairs_scores_store.argtypes = [vp, vp, i32, i32, i32, P]
    L.mfm_pairs_topk_store.argtypes = [vp, vp, i32, i32, i32, i32, P, P]
    L.mfm_pairs_scores.argtypes = [vp, i32, i32, P, P, P, i32, P]
    L.mfm_pairs_topk.argtypes = [vp, i32, i32, P, P, P, i32, i32, P, P]
    L.mfm_pairs_moments_store.argtypes = [vp, vp, i32, i32, i32, P, P]
    L.mfm_pairs_moments.argtypes = [vp, i32, i32, P, P, P, i32, P, P]
    L.mfm_pairs_topk_ucb_store.argtypes = [vp, vp, i32, i32, i32, i32, C.c_double, P, P, P, P]
    L.mfm_pairs_topk_ucb.argtypes = [vp, i32, i32, P, P, P, i32, i32, C.c_double, P, P, P, P]
    L.mfm_pairs_set_targets.argtypes = [vp, P, P]
    L.mfm_design_moments_vb.argtypes = [vp, i32, dbl, dbl, P, P, P, P, dbl, i32, i64, P, P, P]
    L.mfm_pairs_moments_vb.argtypes = [vp, i32, dbl, dbl, P, P, P, P, dbl, P, P]
    L.mfm_pairs_topk_bound_vb.argtypes = [vp, i32, dbl, dbl, P, P, P, P, dbl, i32, dbl, P, P, P, P]
    L.mfm_pairs_rank_store.argtypes = [vp, vp, i32, i32, i32, P, P]
    L.mfm_pairs_rank.argtypes = [vp, i32, i32, P, P, P, i32, P, P]
    L.mfm_pairs_topk_samples_store.argtypes = [vp, vp, i32, i32, i32, i32, P, P, P]
    L.mfm_pairs_topk_samples.argtypes = [vp, i32, i32, P, P, P, i32, i32, P, P, P]
    L.mfm_pairs_topk_prob_store.argtypes = [vp, vp, i32, i32, i32, i32, i32, P, P]
    L.mfm_pairs_topk_prob.argtypes = [vp, i32, i32, P, P, P, i32, i32, i32, P, P]
    L.mfm_foldin_create.argtypes = [C.c_int, i64, i64, P, P, P, P, i64, P, i32, C.POINTER(vp)]
    L.mfm_foldin_destroy.argtypes = [vp]
    L.mfm_foldin_destroy.restype = None
    L.mfm_foldin_last_error.restype = C.c_char_p
    L.mfm_foldin_last_error.argtypes = [vp]
    L.mfm_foldin_set_scratch_bound.argtypes = [vp, i64]
    L.mfm_foldin_max_rank.argtypes = []
    L.mfm_foldin_solve_store.argtypes = [vp, vp, i32, i32, P, P, P, i32, u64, P, P]
    L.mfm_foldin_solve.argtypes = [vp, i32, i32, P, P, P, P, P, P, i32, u64, P, P]
    L.mfm_foldin_gibbs_solve_store.argtypes = [vp, vp, i32, i32, i32, i32, P, P, P, i32, i32, i32, u64, P, P]
    L.mfm_foldin_gibbs_solve.argtypes = [vp, i32, i32, P, P, P, i32, i32, P, P, P, i32, i32, i32, u64, P, P]
    L.mfm_test_erfcx.argtypes = [C.c_int, P, i64, P]
    L.mfm_test_truncated_normal.argtypes = [C.c_int, i32, dbl, dbl, u64, u64, i64, P]
    _lib = L
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def csr_parts(X):
    X = sps.csr_matrix(X, dtype=np.float64)
    return (
        X,
        np.ascontiguousarray(X.indptr, dtype=np.int64),
        np.ascontiguousarray(X.indices, dtype=np.int32),
        np.ascontiguousarray(X.data, dtype=np.float64),
    )


def _raise(code, msg):
    msg = msg.decode() if isinstance(msg, bytes) else msg
    if code == MFM_ERR_INVALID:
        raise ValueError(msg)
    raise RuntimeError(msg)


def column_levels(X):
    """Host-only: level schedule of the columns of X (no GPU needed)."""
    X, ip, ix, _ = csr_parts(X)
    level = np.zeros(X.shape[1], dtype=np.int32)
    n = C.c_int32()
    rc = lib().mfm_host_column_levels(X.shape[0], X.shape[1], _p(ip), _p(ix), _p(level), C.byref(n))
    if rc:
        _raise(rc, lib().mfm_global_error())
    return level, n.value


def device_erfcx(x, device=0):
    """the device erfcx of mfm_oprobit_eval on x (test hook)"""
    x = _f64(x)
    out = np.empty_like(x)
    rc = lib().mfm_test_erfcx(device, _p(x), x.size, _p(out))
    if rc:
        _raise(rc, lib().mfm_global_error())
    return out


def device_truncated_normal(kind, lo, hi, n, seed=1, draw_index=0, device=0):
    """n draws of the device truncated-normal samplers (test hook): kind 'left' (z > lo), 'right' (z < hi), 'twoside'"""
    k = {"left": 0, "right": 1, "twoside": 2}[kind]
    out = np.empty(n)
    rc = lib().mfm_test_truncated_normal(device, k, float(lo), float(hi), seed, draw_index, n, _p(out))
    if rc:
        _raise(rc, lib().mfm_global_error())
    return out


class Context:
    """One training problem on one GPU: thin, explicit wrapper over the mfm_* entry points."""

    def __init__(self, X, y, blocks=(), rank=4, group_index=None, device=0):
        L = lib()
        h = C.c_void_p()
        rc = L.mfm_create(device, C.byref(h))
        if rc:
            _raise(rc, L.mfm_global_error())
        self.h = h
        X, ip, ix, dv = csr_parts(X)
        y = _f64(y)
        self.N, self.D0 = X.shape
        self._ck(L.mfm_set_main(h, X.shape[0], X.shape[1], _p(ip), _p(ix), _p(dv), _p(y)))
        D = X.shape[1]
        for mp, B in blocks:
            B, bp, bx, bv = csr_parts(B)
            mp = np.ascontiguousarray(mp, dtype=np.int64)
            self._ck(L.mfm_add_block(h, B.shape[0], B.shape[1], _p(bp), _p(bx), _p(bv), _p(mp)))
            D += B.shape[1]
        if group_index is None:
            group_index = np.zeros(D, dtype=np.int32)
        group_index = np.ascontiguousarray(group_index, dtype=np.int32)
        self.G = int(group_index.max()) + 1 if D else 1
        self._ck(L.mfm_set_groups(h, _p(group_index), group_index.shape[0], self.G))
        self._ck(L.mfm_finalize(h, rank))
        self.D, self.K = D, rank

    def _ck(self, rc):
        if rc:
            _raise(rc, lib().mfm_last_error(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib().mfm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- state; V crosses this wrapper in the (D, K) shape of the boundary
    def set_state(self, w0, w, V):
        w = _f64(w)
        Vt = _f64(np.asarray(V, dtype=np.float64).T)
        self._ck(lib().mfm_set_state(self.h, float(w0), _p(w), _p(Vt)))

    def get_state(self):
        w0 = C.c_double()
        w = np.empty(self.D)
        V = np.empty((self.K, self.D))
        self._ck(lib().mfm_get_state(self.h, C.byref(w0), _p(w), _p(V)))
        return w0.value, w, np.ascontiguousarray(V.T)

    def set_w0(self, w0):
        self._ck(lib().mfm_set_w0(self.h, float(w0)))

    def zero_w(self):
        self._ck(lib().mfm_zero_w(self.h))

    def get_e(self):
        e = np.empty(self.N)
        self._ck(lib().mfm_get_e(self.h, _p(e)))
        return e

    def get_q(self):
        q = np.empty(self.N)
        self._ck(lib().mfm_get_q(self.h, _p(q)))
        return q

    def set_e(self, e):
        e = _f64(e)
        self._ck(lib().mfm_set_e(self.h, _p(e)))

    # --- iteration pieces
    def reduce_e(self):
        a, b = C.c_double(), C.c_double()
        self._ck(lib().mfm_reduce_e(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def shift_e(self, delta):
        self._ck(lib().mfm_shift_e(self.h, float(delta)))

    def group_stats_w(self, mu_w):
        mu_w = _f64(mu_w)
        s, ss = np.empty(self.G), np.empty(self.G)
        self._ck(lib().mfm_group_stats_w(self.h, _p(mu_w), _p(s), _p(ss)))
        return s, ss

    def group_stats_V(self, mu_V):
        """mu_V: (G, K) -> (sum (G, K), ssd (G, K))"""
        mu = _f64(np.asarray(mu_V).T)
        s, ss = np.empty((self.K, self.G)), np.empty((self.K, self.G))
        self._ck(lib().mfm_group_stats_V(self.h, _p(mu), _p(s), _p(ss)))
        return s.T.copy(), ss.T.copy()

    def sweep_w(self, alpha, lambda_w, mu_w, z):
        lambda_w, mu_w = _f64(lambda_w), _f64(mu_w)
        if z is not None:
            z = _f64(z)
            assert z.shape[0] == self.D
        self._ck(lib().mfm_sweep_w(self.h, float(alpha), _p(lambda_w), _p(mu_w), _p(z)))

    def sweep_V(self, f_begin, f_end, alpha, lambda_V, mu_V, z):
        """lambda_V, mu_V: (G, K); z: ((f_end - f_begin), D)"""
        lam, mu = _f64(np.asarray(lambda_V).T), _f64(np.asarray(mu_V).T)
        if z is not None:
            z = _f64(z)
            assert z.size == (f_end - f_begin) * self.D
        self._ck(lib().mfm_sweep_V(self.h, f_begin, f_end, float(alpha), _p(lam), _p(mu), _p(z)))

    def sweep_wV(self, alpha, e_shift, lambda_w, mu_w, zw, f_begin, f_end, lambda_V, mu_V, zv):
        """update_w0's residual shift, update_w and update_V of factors [f_begin, f_end) as one call"""
        lambda_w, mu_w = _f64(lambda_w), _f64(mu_w)
        lam, mu = _f64(np.asarray(lambda_V).T), _f64(np.asarray(mu_V).T)
        if zw is not None:
            zw, zv = _f64(zw), _f64(zv)
            assert zw.shape[0] == self.D and zv.size == (f_end - f_begin) * self.D
        self._ck(lib().mfm_sweep_wV(self.h, float(alpha), float(e_shift), _p(lambda_w), _p(mu_w), _p(zw), f_begin, f_end,
                                    _p(lam), _p(mu), _p(zv)))

    def update_e_regression(self):
        self._ck(lib().mfm_update_e_regression(self.h))

    def update_e_classification(self, seed, draw_index):
        self._ck(lib().mfm_update_e_classification(self.h, seed, draw_index))

    def score_train(self):
        self._ck(lib().mfm_score_train(self.h))

    def oprobit_add_group(self, n_class, rows=None):
        g = C.c_int32()
        if rows is None:
            self._ck(lib().mfm_oprobit_add_group(self.h, n_class, None, 0, C.byref(g)))
        else:
            rows = np.ascontiguousarray(rows, dtype=np.int64)
            self._ck(lib().mfm_oprobit_add_group(self.h, n_class, _p(rows), rows.shape[0], C.byref(g)))
        return g.value

    def oprobit_eval(self, group, gamma, want_h=True):
        gamma = _f64(gamma)
        m = gamma.shape[0]
        ll = C.c_double()
        dg = np.empty(m)
        H = np.empty((m, m)) if want_h else None
        self._ck(lib().mfm_oprobit_eval(self.h, group, _p(gamma), C.byref(ll), _p(dg), _p(H)))
        return ll.value, dg, H

    def oprobit_sample_z(self, group, gamma, seed, draw_index):
        gamma = _f64(gamma)
        self._ck(lib().mfm_oprobit_sample_z(self.h, group, _p(gamma), seed, draw_index))

    def synchronize(self):
        self._ck(lib().mfm_synchronize(self.h))

    # --- device random stream
    RNG_OP = np.dtype([("kind", np.int32), ("dest", np.int32), ("count", np.int64), ("offset", np.int64), ("shape", np.float64)])

    def rng_seed_mt19937(self, state624, position):
        st = np.ascontiguousarray(state624, dtype=np.uint32)
        assert st.shape[0] == 624
        self._ck(lib().mfm_rng_seed_mt19937(self.h, _p(st), int(position)))

    def rng_set_program(self, ops):
        """ops: list of (kind, dest, count, offset, shape)"""
        arr = np.array([tuple(o) for o in ops], dtype=self.RNG_OP)
        self._n_hv = int(sum(o[2] for o in ops if o[1] == 0))
        self._ck(lib().mfm_rng_set_program(self.h, _p(arr), len(ops)))

    def rng_prefetch(self):
        self._ck(lib().mfm_rng_prefetch(self.h))

    def rng_acquire(self):
        hv = np.empty(max(self._n_hv, 1))
        self._ck(lib().mfm_rng_acquire(self.h, _p(hv), self._n_hv))
        return hv[: self._n_hv]

    def rng_get_z(self):
        zw, zv = np.empty(self.D), np.empty((max(self.K, 1), self.D))
        self._ck(lib().mfm_rng_get_z(self.h, _p(zw), _p(zv)))
        return zw, zv[: self.K]

    # --- the state-dependent draws on the same stream (latent mode "exact")
    def update_e_classification_exact(self):
        st = C.c_int32()
        self._ck(lib().mfm_update_e_classification_exact(self.h, C.byref(st)))
        return st.value

    def oprobit_sample_z_exact(self, group, gamma):
        gamma = _f64(gamma)
        st = C.c_int32()
        self._ck(lib().mfm_oprobit_sample_z_exact(self.h, group, _p(gamma), C.byref(st)))
        return st.value

    def latent_stats(self):
        out = np.zeros(8, dtype=np.int64)
        self._ck(lib().mfm_latent_stats(self.h, _p(out)))
        return dict(zip(("status", "chunks", "subs", "lq", "quads", "walkers", "attempts"), (int(v) for v in out)))

    def rng_host_read(self, offset, n):
        out = np.empty(max(int(n), 1), dtype=np.uint32)
        self._ck(lib().mfm_rng_host_read(self.h, int(offset), int(n), _p(out)))
        return out[: int(n)]

    def rng_host_advance(self, words):
        self._ck(lib().mfm_rng_host_advance(self.h, int(words)))

    def set_residual_policy(self, recomputable):
        self._ck(lib().mfm_set_residual_policy(self.h, 1 if recomputable else 0))

    def plan_flags(self):
        f = lib().mfm_plan_flags(self.h)
        return {"qfree": bool(f & 1), "unit": bool(f & 2), "ell": bool(f & 4), "sharded": bool(f & 8), "soa": bool(f & 16),
                "fused_next": bool(f & 32), "sharded_fused": bool(f & 64), "mf": bool(f & 128), "resident": bool(f & 256), "cell": bool(f & 512), "streamed_chain": bool(f & 1024), "resident_overflow": bool(f & 2048)}

    RES_INFO = ("ready", "G", "RV", "RL", "RX", "umax", "n_items", "item_bits", "n_runs", "max_wg_users", "max_slice_items",
                "e_where", "n_rows", "s2_in_sweep_b", "lds_bytes", "entry_bytes")
    E_WHERE = ("rows", "slots", "slots_with_sums", "cell", "dropped")

    def res_info(self):
        """the persistent sweep's layout (mfm_res_info): the RES_INFO fields as ints, `ready` as a bool, `e_where` as one of
        E_WHERE, and `why`, the planner's refusal text ('' when the layout was taken)"""
        out = np.zeros(len(self.RES_INFO), dtype=np.int64)
        why = C.create_string_buffer(256)
        self._ck(lib().mfm_res_info(self.h, _p(out), out.shape[0], why, len(why)))
        d = dict(zip(self.RES_INFO, (int(v) for v in out)))
        d["ready"] = bool(d["ready"])
        d["e_where"] = self.E_WHERE[d["e_where"]]
        d["why"] = why.value.decode()
        return d

    CELL_INFO = ("ready", "G", "umax", "item32", "n_streams", "n_fields", "N", "Npad", "max_steps", "chunk_max", "chunk_min",
                 "chunks_empty", "split_mask", "score_fb")
    CELL_STREAM_TYPE = ("U", "I", "C")
    CELL_MAX_STREAMS, CELL_MAX_FIELDS = 4, 16  # (csrc/mfm_cell.hpp; three entries each in mfm_cell_info's output)
    CELL_INFO_FIELDS = len(CELL_INFO) + 3 * CELL_MAX_STREAMS + 3 * CELL_MAX_FIELDS  # MFM_CELL_INFO_FIELDS of include/myfm_hip.h

    def cell_info(self):
        """the cell path's plan (mfm_cell_info): the CELL_INFO fields as ints (`ready`, `item32` as bools), `streams`: a list of
        (type 'U' | 'I' | 'C', record slot, cardinality), `fields`: a list of (stream, kind 0 main field | 1 block, n) in Gibbs
        order, and `why`, the planner's refusal text ('' when the plan was taken or the cell path was not tried)"""
        out = np.zeros(self.CELL_INFO_FIELDS, dtype=np.int64)
        why = C.create_string_buffer(256)
        self._ck(lib().mfm_cell_info(self.h, _p(out), out.shape[0], why, len(why)))
        n = len(self.CELL_INFO)
        nf = n + 3 * self.CELL_MAX_STREAMS  # where the fields' entries begin
        d = dict(zip(self.CELL_INFO, (int(v) for v in out[:n])))
        d["ready"], d["item32"] = bool(d["ready"]), bool(d["item32"])
        d["streams"] = [(self.CELL_STREAM_TYPE[int(out[n + 3 * s])], int(out[n + 3 * s + 1]), int(out[n + 3 * s + 2]))
                        for s in range(d["n_streams"])]
        d["fields"] = [tuple(int(x) for x in out[nf + 3 * k:nf + 3 * k + 3]) for k in range(d["n_fields"])]
        d["why"] = why.value.decode()
        return d

    def chain_stream_info(self):
        """the streamed chain runs of the relation blocks' plans (mfm_chain_stream_info): one dict per run with the
        CHAIN_STREAM_INFO fields as ints and `hot_rounds`, a list of ten counts (columns whose hot entries fill i wavefront
        rounds, the last entry: nine or more)"""
        n = C.c_int(0)
        self._ck(lib().mfm_chain_stream_info(self.h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), CHAIN_STREAM_INFO_FIELDS), dtype=np.int64)
        self._ck(lib().mfm_chain_stream_info(self.h, _p(out), n.value, C.byref(n)))
        return [chain_stream_record(out[i]) for i in range(n.value)]

    def plan_info(self):
        a, b = C.c_int64(), C.c_int64()
        lib().mfm_plan_info(self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    # --- timing
    def timing_enable(self, on=True):
        self._ck(lib().mfm_timing_enable(self.h, int(on)))

    def timing_reset(self):
        self._ck(lib().mfm_timing_reset(self.h))

    def timing(self):
        """{class name: (ms_total, launches, algorithmic_bytes_total)} for classes that ran."""
        L = lib()
        out = {}
        for c in range(L.mfm_timing_n_classes()):
            ms, n, by = C.c_double(), C.c_int64(), C.c_double()
            self._ck(L.mfm_timing_get(self.h, c, C.byref(ms), C.byref(n), C.byref(by)))
            if n.value:
                out[L.mfm_timing_class_name(c).decode()] = (ms.value, n.value, by.value)
        return out


class Design:
    """A prediction design (main CSR + relation blocks) resident on the GPU."""

    def __init__(self, X, blocks=(), device=0):
        L = lib()
        h = C.c_void_p()
        X, ip, ix, dv = csr_parts(X)
        rc = L.mfm_design_create(device, X.shape[0], X.shape[1], _p(ip), _p(ix), _p(dv), C.byref(h))
        if rc:
            _raise(rc, L.mfm_global_error())
        self.h = h
        self.N = X.shape[0]
        for mp, B in blocks:
            B, bp, bx, bv = csr_parts(B)
            mp = np.ascontiguousarray(mp, dtype=np.int64)
            if mp.shape[0] != self.N:
                self.close()
                raise ValueError("Relation blocks have inconsistent mapper size with case_size")
            rc = L.mfm_design_add_block(h, B.shape[0], B.shape[1], _p(bp), _p(bx), _p(bv), _p(mp))
            if rc:
                msg = L.mfm_design_last_error(h)
                self.close()
                _raise(rc, msg)
        self.D = L.mfm_design_dim_all(h)

    def close(self):
        if getattr(self, "h", None):
            lib().mfm_design_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def score_ctx(self, ctx):
        """FM::predict_score with the model state resident in training context `ctx`."""
        out = np.empty(self.N)
        self._ck(lib().mfm_design_score_ctx(self.h, ctx.h, _p(out)))
        return out

    def _ck(self, rc):
        if rc:
            _raise(rc, lib().mfm_design_last_error(self.h))

    def moments_vb(self, model, extra_var=0.0, want_prob=False, tile_rows=0):
        """(mean[N], std[N][, Phi(mean / sqrt(1 + var))[N]]) of the score under the mean-field posterior `model` = (w0, w0_var,
        w[D], w_var[D], V[D, K], V_var[D, K]) (mfm_design_moments_vb)"""
        K, head, keep = _pack_vb_model(model)
        mean, std, prob = np.empty(self.N), np.empty(self.N), np.empty(self.N if want_prob else 0)
        self._ck(lib().mfm_design_moments_vb(self.h, K, *head, float(extra_var), int(bool(want_prob)), int(tile_rows), _p(mean), _p(std),
                                             _p(prob) if want_prob else None))
        return (mean, std, prob) if want_prob else (mean, std)

    # each operation once, over a sample source (_host / _resident); Store's methods of the same names pass a resident range
    def _predict(self, src, mode, cutpoints):
        n_cut, cp = 0, None
        if mode == 2:
            cp = _f64(np.stack([np.asarray(c, dtype=np.float64) for c in cutpoints]))
            n_cut = cp.shape[1]
        out = np.empty((self.N, n_cut + 1) if mode == 2 else self.N)
        self._ck(src.call("mfm_design_predict", self.h, mode, n_cut, _p(cp), _p(out)))
        return out

    def _summary(self, src, mode, quantiles, precisions, tile_rows, chunk_samples):
        probs, prec, z, mean, std, q = _summary_args(self.N, quantiles, precisions)
        self._ck(src.call("mfm_design_summary", self.h, mode, len(probs), _p(probs), _p(prec), _p(z), int(tile_rows),
                          int(chunk_samples), _p(mean), _p(std), _p(q)))
        return mean, std, q

    def _summary_oprobit(self, src, cutpoints, expected, quantiles, tile_rows, chunk_samples):
        cp, n_cut, probs, mean, std, q = _summary_oprobit_args(self.N, cutpoints, expected, quantiles)
        self._ck(src.call("mfm_design_summary_oprobit", self.h, int(bool(expected)), n_cut, _p(cp), len(probs), _p(probs),
                          int(tile_rows), int(chunk_samples), _p(mean), _p(std), _p(q)))
        return mean, std, q

    def _log_density_args(self, y, precisions, cutpoints):
        """(y[N], precisions[S] or None, n_cut, cutpoints[S, n_cut] or None) as mfm_design_logdens* and mfm_design_loo* take them"""
        y = _f64(y).reshape(-1)
        if y.shape[0] != self.N:
            raise ValueError("y must hold one value per design row")
        prec = None if precisions is None else _f64(precisions).reshape(-1)
        cp, n_cut = None, 0
        if cutpoints is not None:
            cp = _f64(cutpoints)
            if cp.ndim != 2:
                raise ValueError("cutpoints must be a 2-D array, one row of n_cut cutpoints per sample")
            n_cut = cp.shape[1]
        return y, prec, n_cut, cp

    def _log_density(self, src, task, y, precisions, cutpoints, pointwise, tile_rows, chunk_samples):
        y, prec, n_cut, cp = self._log_density_args(y, precisions, cutpoints)
        lpd, mean, var = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        pit = np.empty(self.N) if task == TASK_REGRESSION else None
        ll = np.empty((src.S, self.N)) if pointwise else None
        self._ck(src.call("mfm_design_logdens", self.h, int(task), _p(y), _p(prec), n_cut, _p(cp), int(tile_rows), int(chunk_samples),
                          _p(lpd), _p(mean), _p(var), _p(pit), _p(ll)))
        return lpd, mean, var, pit, ll

    def log_density(self, samples, task, y, precisions=None, cutpoints=None, pointwise=False, tile_rows=0, chunk_samples=0):
        """samples as predict; task 0 regression (precisions[S]), 1 probit classification (y in {0, 1}), 2 ordered probit
        (cutpoints[S][n_cut], y the class labels). Returns (lpd[N], log_lik_mean[N], log_lik_var[N], pit[N] or None,
        log_lik[S, N] or None) of the observed y over the samples (mfm_design_logdens)."""
        return self._log_density(_host(samples), task, y, precisions, cutpoints, pointwise, tile_rows, chunk_samples)

    def _loo(self, src, task, y, precisions, cutpoints, log_weights, r_eff, tile_rows, chunk_samples):
        y, prec, n_cut, cp = self._log_density_args(y, precisions, cutpoints)
        elpd, k, lpd = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        pit = np.empty(self.N) if task == TASK_REGRESSION else None
        lw = np.empty((src.S, self.N)) if log_weights else None
        self._ck(src.call("mfm_design_loo", self.h, int(task), _p(y), _p(prec), n_cut, _p(cp), int(tile_rows), int(chunk_samples),
                          psis_tail_len(src.S, r_eff), _p(elpd), _p(k), _p(lpd), _p(pit), _p(lw)))
        return elpd, k, lpd, pit, lw

    def loo(self, samples, task, y, precisions=None, cutpoints=None, log_weights=False, r_eff=1.0, tile_rows=0, chunk_samples=0):
        """samples, task, y, precisions and cutpoints as log_density. Returns (elpd_loo[N], pareto_k[N], lpd[N], loo_pit[N] or
        None, log_weights[S, N] or None): Pareto-smoothed importance-sampling leave-one-out of the observed y over the samples,
        the tail of ceil(min(0.2 S, 3 sqrt(S / r_eff))) ratios smoothed (mfm_design_loo)."""
        return self._loo(_host(samples), task, y, precisions, cutpoints, log_weights, r_eff, tile_rows, chunk_samples)

    def _ess(self, src, kind, mode_or_task, y, precisions, cutpoints, tile_rows, chunk_samples, n_chains=1):
        if kind == 1:
            y, prec, n_cut, cp = self._log_density_args(y, precisions, cutpoints)
        else:  # (the value needs no targets; what it must not be given is the library's to refuse)
            _, prec, n_cut, cp = self._log_density_args(np.zeros(self.N), precisions, cutpoints)
            y = None
        out = [np.empty(self.N) for _ in range(4)]
        self._ck(src.call("mfm_design_ess_chains", self.h, int(n_chains), int(kind), int(mode_or_task), _p(y), _p(prec), n_cut, _p(cp),
                          int(tile_rows), int(chunk_samples), *[_p(o) for o in out]))
        return tuple(out)

    def ess(self, samples, kind, mode_or_task, y=None, precisions=None, cutpoints=None, tile_rows=0, chunk_samples=0, n_chains=1):
        """samples as predict. Chain diagnostics per row over the samples in their order, n_chains chains of equal length one after
        another (mfm_design_ess_chains; one chain: what mfm_design_ess gives, bit for bit). kind 0, the prediction
        value of mode 0 score, 1 Phi(score), 2 the expected class index under cutpoints[S][n_cut]: (rhat[N], ess_bulk[N],
        ess_mean[N], mcse_mean[N]). kind 1, the likelihood of y with task, precisions and cutpoints as log_density: (rhat[N],
        ess_bulk[N], r_eff[N], mcse_lpd[N])."""
        return self._ess(_host(samples), kind, mode_or_task, y, precisions, cutpoints, tile_rows, chunk_samples, n_chains)

    def _crps(self, src, task, y, precisions, cutpoints, tile_rows, chunk_samples):
        y, prec, n_cut, cp = self._log_density_args(y, precisions, cutpoints)
        crps, accuracy, spread = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        self._ck(src.call("mfm_design_crps", self.h, int(task), _p(y), _p(prec), n_cut, _p(cp), int(tile_rows), int(chunk_samples),
                          _p(crps), _p(accuracy), _p(spread)))
        return crps, accuracy, spread

    def crps(self, samples, task, y, precisions=None, cutpoints=None, tile_rows=0, chunk_samples=0):
        """samples, task, y, precisions and cutpoints as log_density (task 0: at most 1024 samples). Returns (crps[N], accuracy[N],
        spread[N]): the continuous ranked probability score E|Y - y| - E|Y - Y'| / 2 of the predictive distribution of y over the
        samples and its two terms; the Brier score for task 1, the ranked probability score for task 2 (mfm_design_crps)."""
        return self._crps(_host(samples), task, y, precisions, cutpoints, tile_rows, chunk_samples)

    def _loo_summary(self, src, task, y, precisions, cutpoints, quantiles, r_eff, tile_rows, chunk_samples):
        y, prec, n_cut, cp = self._log_density_args(y, precisions, cutpoints)
        probs = _f64(quantiles).reshape(-1)
        mean, std, ess, k = np.empty(self.N), np.empty(self.N), np.empty(self.N), np.empty(self.N)
        q = np.empty((len(probs), self.N))
        std_y = np.empty(self.N) if task == TASK_REGRESSION else None
        self._ck(src.call("mfm_design_loo_summary", self.h, int(task), _p(y), _p(prec), n_cut, _p(cp), int(tile_rows), int(chunk_samples),
                          psis_tail_len(src.S, r_eff), len(probs), _p(probs), _p(mean), _p(std), _p(q), _p(std_y), _p(ess), _p(k)))
        return mean, std, q, std_y, ess, k

    def loo_summary(self, samples, task, y, precisions=None, cutpoints=None, quantiles=(), r_eff=1.0, tile_rows=0, chunk_samples=0):
        """samples, task, y, precisions, cutpoints and r_eff as loo. Returns (mean[N], std[N], quantiles[Q, N], std_y[N] or None,
        ess[N], pareto_k[N]): the leave-one-out weighted summary of the value summary / summary_oprobit(expected) summarise
        (mfm_design_loo_summary)."""
        return self._loo_summary(_host(samples), task, y, precisions, cutpoints, quantiles, r_eff, tile_rows, chunk_samples)

    def _loo_crps(self, src, task, y, precisions, cutpoints, r_eff, tile_rows, chunk_samples):
        y, prec, n_cut, cp = self._log_density_args(y, precisions, cutpoints)
        crps, accuracy, spread, k = np.empty(self.N), np.empty(self.N), np.empty(self.N), np.empty(self.N)
        self._ck(src.call("mfm_design_loo_crps", self.h, int(task), _p(y), _p(prec), n_cut, _p(cp), int(tile_rows), int(chunk_samples),
                          psis_tail_len(src.S, r_eff), _p(crps), _p(accuracy), _p(spread), _p(k)))
        return crps, accuracy, spread, k

    def loo_crps(self, samples, task, y, precisions=None, cutpoints=None, r_eff=1.0, tile_rows=0, chunk_samples=0):
        """samples, task, y, precisions, cutpoints and r_eff as loo (task 0: at most 1024 samples). Returns (crps[N], accuracy[N],
        spread[N], pareto_k[N]): crps with the predictive distribution reweighted by the leave-one-out weights (mfm_design_loo_crps)."""
        return self._loo_crps(_host(samples), task, y, precisions, cutpoints, r_eff, tile_rows, chunk_samples)

    def _contributions(self, src, n_fields, field_of, tile_rows, chunk_samples):
        F = int(n_fields)
        fo = np.ascontiguousarray(np.asarray(field_of).reshape(-1), dtype=np.int32)
        Pn = max(F, 0) * (max(F, 0) + 1) // 2
        bias, lin, lin_std = np.empty(2), np.empty((max(F, 0), self.N)), np.empty((max(F, 0), self.N))
        inter, inter_std = np.empty((Pn, self.N)), np.empty((Pn, self.N))
        self._ck(src.call("mfm_design_contrib", self.h, F, _p(fo), fo.shape[0], int(tile_rows), int(chunk_samples), _p(bias), _p(lin),
                          _p(lin_std), _p(inter), _p(inter_std)))
        return bias[0], bias[1], lin, lin_std, inter, inter_std

    def contributions(self, samples, n_fields, field_of, tile_rows=0, chunk_samples=0):
        """samples as predict; field_of[D] in [0, n_fields), n_fields <= 16. Returns (bias, bias_std, linear[F, N], linear_std[F, N],
        interaction[P, N], interaction_std[P, N]): mean and population standard deviation over the samples of every field's linear
        term and every field pair's interaction, pair (g, h), g <= h, at g F - g (g - 1) / 2 + (h - g) (mfm_design_contrib)."""
        return self._contributions(_host(samples), n_fields, field_of, tile_rows, chunk_samples)

    def predict(self, samples, mode=0, cutpoints=None):
        """samples: list of (w0, w[D], V[D, K]); mode 0 mean score, 1 mean Phi(score), 2 ordered probit."""
        return self._predict(_host(samples), mode, cutpoints)

    def summary(self, samples, mode=0, quantiles=(), precisions=None, tile_rows=0, chunk_samples=0):
        """samples as predict; mode 0 score, 1 Phi(score). Returns (mean[N], std[N], quantiles[Q, N]) over the samples;
        precisions[S]: of the mixture mean_s N(score_s, 1 / precisions[s]) (mfm_design_summary)."""
        return self._summary(_host(samples), mode, quantiles, precisions, tile_rows, chunk_samples)

    def summary_oprobit(self, samples, cutpoints, expected=False, quantiles=(), tile_rows=0, chunk_samples=0):
        """samples as predict, cutpoints[S][n_cut]. Summaries of the class probabilities, (mean[N, C], std[N, C],
        quantiles[Q, N, C]) with C = n_cut + 1, or with `expected` of the expected class index, (mean[N], std[N],
        quantiles[Q, N]) (mfm_design_summary_oprobit)."""
        return self._summary_oprobit(_host(samples), cutpoints, expected, quantiles, tile_rows, chunk_samples)


def _summary_oprobit_args(N, cutpoints, expected, quantiles):
    """cutpoints [S][n_cut] (n_cut = 0 for none), n_cut, the probabilities and the three output arrays of an ordered-probit summary"""
    cp = _f64(cutpoints)
    if cp.ndim != 2:
        raise ValueError("cutpoints must be a 2-D array, one row of n_cut cutpoints per sample")
    n_cut = cp.shape[1]
    probs = _f64(quantiles).reshape(-1)
    tail = () if expected else (n_cut + 1,)
    return cp, n_cut, probs, np.empty((N,) + tail), np.empty((N,) + tail), np.empty((len(probs), N) + tail)


def _summary_args(N, quantiles, precisions):
    """probabilities, precisions, Phi^-1 of the probabilities (noise only) and the three output arrays of a summary call"""
    from statistics import NormalDist

    probs = _f64(quantiles).reshape(-1)
    prec = None if precisions is None else _f64(precisions).reshape(-1)
    z = None
    if prec is not None:
        z = _f64([NormalDist().inv_cdf(float(p)) if 0.0 < p < 1.0 else np.nan for p in probs])
    return probs, prec, z, np.empty(N), np.empty(N), np.empty((len(probs), N))


class Store:
    """posterior samples resident on the GPU (mfm_store_*)"""

    def __init__(self, D, K, device=0):
        h = C.c_void_p()
        rc = lib().mfm_store_create(device, D, K, C.byref(h))
        if rc:
            _raise(rc, lib().mfm_global_error())
        self.h, self.D, self.K = h, D, K

    def close(self):
        if getattr(self, "h", None):
            lib().mfm_store_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            _raise(rc, lib().mfm_store_last_error(self.h))

    def __len__(self):
        return lib().mfm_store_size(self.h)

    def push_ctx(self, ctx):
        self._ck(lib().mfm_store_push_ctx(self.h, ctx.h))

    def push(self, w0, w, V):
        w, Vt = _f64(w), _f64(np.asarray(V, dtype=np.float64).T)
        self._ck(lib().mfm_store_push_host(self.h, float(w0), _p(w), _p(Vt)))

    def get(self, idx):
        w0, w, V = C.c_double(), np.empty(self.D), np.empty((self.K, self.D))
        self._ck(lib().mfm_store_get(self.h, idx, C.byref(w0), _p(w), _p(V)))
        return w0.value, w, np.ascontiguousarray(V.T)

    def predict(self, design, mode=0, cutpoints=None, first=0, count=None):
        return design._predict(_resident(self, first, count), mode, cutpoints)

    def summary(self, design, mode=0, quantiles=(), precisions=None, first=0, count=None, tile_rows=0, chunk_samples=0):
        """Design.summary over the resident samples [first, first + count) (mfm_design_summary_store)"""
        return design._summary(_resident(self, first, count), mode, quantiles, precisions, tile_rows, chunk_samples)

    def summary_oprobit(self, design, cutpoints, expected=False, quantiles=(), first=0, count=None, tile_rows=0, chunk_samples=0):
        """Design.summary_oprobit over the resident samples [first, first + count) (mfm_design_summary_oprobit_store)"""
        return design._summary_oprobit(_resident(self, first, count), cutpoints, expected, quantiles, tile_rows, chunk_samples)

    def log_density(self, design, task, y, precisions=None, cutpoints=None, pointwise=False, first=0, count=None, tile_rows=0,
                    chunk_samples=0):
        """Design.log_density over the resident samples [first, first + count) (mfm_design_logdens_store)"""
        return design._log_density(_resident(self, first, count), task, y, precisions, cutpoints, pointwise, tile_rows, chunk_samples)

    def loo(self, design, task, y, precisions=None, cutpoints=None, log_weights=False, r_eff=1.0, first=0, count=None, tile_rows=0,
            chunk_samples=0):
        """Design.loo over the resident samples [first, first + count) (mfm_design_loo_store)"""
        return design._loo(_resident(self, first, count), task, y, precisions, cutpoints, log_weights, r_eff, tile_rows, chunk_samples)

    def ess(self, design, kind, mode_or_task, y=None, precisions=None, cutpoints=None, first=0, count=None, tile_rows=0, chunk_samples=0,
            n_chains=1):
        """Design.ess over the resident samples [first, first + count) (mfm_design_ess_chains_store)"""
        return design._ess(_resident(self, first, count), kind, mode_or_task, y, precisions, cutpoints, tile_rows, chunk_samples, n_chains)

    def crps(self, design, task, y, precisions=None, cutpoints=None, first=0, count=None, tile_rows=0, chunk_samples=0):
        """Design.crps over the resident samples [first, first + count) (mfm_design_crps_store)"""
        return design._crps(_resident(self, first, count), task, y, precisions, cutpoints, tile_rows, chunk_samples)

    def loo_summary(self, design, task, y, precisions=None, cutpoints=None, quantiles=(), r_eff=1.0, first=0, count=None, tile_rows=0,
                    chunk_samples=0):
        """Design.loo_summary over the resident samples [first, first + count) (mfm_design_loo_summary_store)"""
        return design._loo_summary(_resident(self, first, count), task, y, precisions, cutpoints, quantiles, r_eff, tile_rows, chunk_samples)

    def loo_crps(self, design, task, y, precisions=None, cutpoints=None, r_eff=1.0, first=0, count=None, tile_rows=0, chunk_samples=0):
        """Design.loo_crps over the resident samples [first, first + count) (mfm_design_loo_crps_store)"""
        return design._loo_crps(_resident(self, first, count), task, y, precisions, cutpoints, r_eff, tile_rows, chunk_samples)


    def contributions(self, design, n_fields, field_of, first=0, count=None, tile_rows=0, chunk_samples=0):
        """Design.contributions over the resident samples [first, first + count) (mfm_design_contrib_store)"""
        return design._contributions(_resident(self, first, count), n_fields, field_of, tile_rows, chunk_samples)


def contrib_row(idx, val, samples, n_fields, field_of):
    """(mean[F + P], std[F + P]) of one row's components on the host, by the functions the device runs and in its orders: the
    row's entries (idx, val) in the flat design, samples a list of (w0, w[D], V[D, K]) (mfm_contrib_row)"""
    K, S, _, ws, Vs = _pack_samples(samples)
    D = np.asarray(samples[0][1]).shape[0] if S else 0
    idx = np.ascontiguousarray(np.asarray(idx).reshape(-1), dtype=np.int32)
    val = _f64(val).reshape(-1)
    if idx.shape[0] != val.shape[0]:
        raise ValueError("idx and val hold one entry each per stored element of the row")
    fo = np.ascontiguousarray(np.asarray(field_of).reshape(-1), dtype=np.int32)
    F = int(n_fields)
    n_out = max(F, 0) + max(F, 0) * (max(F, 0) + 1) // 2
    mean, std = np.empty(n_out), np.empty(n_out)
    rc = lib().mfm_contrib_row(idx.shape[0], _p(idx), _p(val), D, K, S, _p(ws), _p(Vs), F, _p(fo), fo.shape[0], _p(mean), _p(std))
    if rc:
        _raise(rc, lib().mfm_global_error())
    return mean, std


def crps_row(task, y, scores, precisions=None, cutpoints=None):
    """(crps, accuracy, spread) of one row on the host, by the functions the device runs and in its summation orders: scores[S],
    precisions[S] (task 0), cutpoints[S, n_cut] (task 2) (mfm_crps_row)"""
    scores = _f64(scores).reshape(-1)
    prec = None if precisions is None else _f64(precisions).reshape(-1)
    cp, n_cut = None, 0
    if cutpoints is not None:
        cp = _f64(cutpoints)
        if cp.ndim != 2:
            raise ValueError("cutpoints must be a 2-D array, one row of n_cut cutpoints per sample")
        n_cut = cp.shape[1]
    if (prec is not None and prec.shape[0] != scores.shape[0]) or (cp is not None and cp.shape[0] != scores.shape[0]):
        raise ValueError("precisions and cutpoints hold one entry per score")
    out = np.empty(3)
    rc = lib().mfm_crps_row(int(task), scores.shape[0], float(y), _p(scores), _p(prec), n_cut, _p(cp), _p(out))
    if rc:
        _raise(rc, lib().mfm_global_error())
    return tuple(out)


def ess_row(x, n_chains=1):
    """(ess, rhat) of one sequence of draws on the host, n_chains chains of equal length one after another, by the scalar pieces the
    device runs (mfm_ess_row_chains)"""
    x = _f64(x).reshape(-1)
    ess, rhat = C.c_double(), C.c_double()
    rc = lib().mfm_ess_row_chains(x.shape[0], int(n_chains), _p(x), C.byref(ess), C.byref(rhat))
    if rc:
        _raise(rc, lib().mfm_global_error())
    return ess.value, rhat.value


def rank_z_table(S):
    """table[2S - 1] of the rank-normalised values by twice the average rank (mfm_rank_z_table)"""
    out = np.empty(max(2 * int(S) - 1, 0))
    rc = lib().mfm_rank_z_table(int(S), _p(out))
    if rc:
        _raise(rc, lib().mfm_global_error())
    return out


def psis_tail_len(S, r_eff=1.0):
    """the number of importance ratios PSIS smooths: ceil(min(0.2 S, 3 sqrt(S / r_eff)))"""
    r_eff = float(r_eff)
    if not (r_eff > 0.0) or not np.isfinite(r_eff):
        raise ValueError("r_eff must be one finite positive number")
    return 0 if S <= 1 else int(np.ceil(min(0.2 * S, 3.0 * np.sqrt(S / r_eff))))  # (below 5 nothing is smoothed; the library wants M < S)


def _pack_vb_model(model):
    """(w0, w0_var, w[D], w_var[D], V[D, K], V_var[D, K]) -> K, the six arguments of the mfm_*_vb entry points (V, V_var
    column-major), and the arrays they point into"""
    w0, w0_var, w, w_var, V, V_var = model
    V, V_var = np.asarray(V, dtype=np.float64), np.asarray(V_var, dtype=np.float64)
    keep = (_f64(w), _f64(w_var), _f64(V.T), _f64(V_var.T))
    return V.shape[1], (float(w0), float(w0_var)) + tuple(_p(a) for a in keep), keep


def _pack_samples(samples):
    """list of (w0, w[D], V[D, K]) -> K, S, w0s, ws, Vs in the layout of the host-sample entry points"""
    S = len(samples)
    K = np.asarray(samples[0][2]).shape[1] if S else 0
    w0s = _f64([s[0] for s in samples])
    ws = _f64(np.stack([np.asarray(s[1], dtype=np.float64) for s in samples])) if S else np.empty(0)
    Vs = _f64(np.stack([np.asarray(s[2], dtype=np.float64).T for s in samples])) if S else np.empty(0)
    return K, S, w0s, ws, Vs


class _Samples:
    """Where an operation reads the kept samples: S samples of rank K, the suffix of the C symbol that reads them and the head
    of its argument list after the handle. Every mfm_X_store(h, store, first, count, TAIL...) has a twin
    mfm_X(h, rank, n_samples, w0s, ws, Vs, TAIL...) with the same TAIL (include/myfm_hip.h)."""

    def __init__(self, S, K, suffix, head, keep):
        self.S, self.K, self.suffix, self.head, self.keep = S, K, suffix, head, keep  # (keep: what the head points into)

    def call(self, symbol, handle, *tail):
        return getattr(lib(), symbol + self.suffix)(handle, *self.head, *tail)


def _host(samples):
    """host samples, a list of (w0, w[D], V[D, K]), packed once"""
    K, S, w0s, ws, Vs = _pack_samples(samples)
    return _Samples(S, K, "", (K, S, _p(w0s), _p(ws), _p(Vs)), (w0s, ws, Vs))


def _resident(store, first, count):
    """the samples [first, first + count) of a Store (count None: up to its end), read in place"""
    count = len(store) - first if count is None else count
    return _Samples(count, store.K, "_store", (store.h, first, count), store)


def _sim_metric(metric):
    """"cosine" / "dot" -> the number the C ABI takes; an integer is passed on for the library to judge"""
    if isinstance(metric, str) and metric in SIM_METRICS:
        return SIM_METRICS[metric]
    if isinstance(metric, (bool, np.bool_)) or not isinstance(metric, (int, np.integer)):
        raise ValueError('metric must be "cosine" or "dot" (or the C ABI\'s number, 0 or 1), got %r' % (metric,))
    return int(metric)


class Pairs:
    """Query x candidate scoring (mfm_pairs_*): both sides (U, D) / (I, D) sparse in the model's feature space, no column in
    both. `exclude`: optional (U, I) sparse pattern of pairs the top-k leaves out. `scratch_bound`: bytes of query-side
    scratch per chunk of queries (default 256 MB; a small value makes a small table cross the chunking). `rel_query` /
    `rel_cand`: relation blocks of the sides, each entry (col_offset, o2b, csr): side row r additionally holds row o2b[r] of
    `csr` at columns [col_offset, col_offset + csr.shape[1]) of the same D columns (the main matrices keep the model's width
    and leave the blocks' columns empty); applied in list order. `cutpoints`: (S, n_cut) array, the samples' cutpoints for
    mode 2 (the mean over the samples of the expected class index of the ordered probit). `targets`: optional (U, I) sparse
    pattern of the pairs `rank` ranks, at most 64 per row and none of them excluded. `similarity`: a similarity handle
    (mfm_pairs_create_sim): the sides may share columns, and only sim / topk_sim run on it."""

    def __init__(self, X_query, X_cand, exclude=None, scratch_bound=None, device=0, rel_query=(), rel_cand=(), cutpoints=None,
                 targets=None, similarity=False):
        L = lib()
        h = C.c_void_p()
        Xq, qp, qx, qv = csr_parts(X_query)
        Xc, cp, cx, cv = csr_parts(X_cand)
        if Xq.shape[1] != Xc.shape[1]:
            raise ValueError("X_query and X_cand differ in width")
        create = L.mfm_pairs_create_sim if similarity else L.mfm_pairs_create
        rc = create(device, Xq.shape[1], Xq.shape[0], _p(qp), _p(qx), _p(qv), Xc.shape[0], _p(cp), _p(cx), _p(cv), C.byref(h))
        if rc:
            _raise(rc, L.mfm_pairs_last_error(None))
        self.h, self.U, self.I, self.D = h, Xq.shape[0], Xc.shape[0], Xq.shape[1]
        self.n_targets = 0
        if exclude is not None:
            E = sps.csr_matrix(exclude)
            if E.shape != (self.U, self.I):
                self.close()
                raise ValueError("exclude must have shape (n_queries, n_candidates)")
            ep = np.ascontiguousarray(E.indptr, dtype=np.int64)
            ex = np.ascontiguousarray(E.indices, dtype=np.int32)
            self._ck(L.mfm_pairs_set_exclude(h, _p(ep), _p(ex)))
        if scratch_bound is not None:
            self._ck(L.mfm_pairs_set_scratch_bound(h, int(scratch_bound)))
        try:
            for side, rels in ((0, rel_query), (1, rel_cand)):
                for off, o2b, B in rels:
                    B, bp, bx, bv = csr_parts(B)
                    o2b = np.ascontiguousarray(o2b, dtype=np.int64)
                    if o2b.shape != ((self.U, self.I)[side],):
                        raise ValueError("a block's o2b must have one entry per row of its side")
                    self._ck(L.mfm_pairs_add_block(h, side, int(off), B.shape[1], B.shape[0], _p(o2b), _p(bp), _p(bx), _p(bv)))
            if cutpoints is not None:
                cp = _f64(np.atleast_2d(np.asarray(cutpoints, dtype=np.float64)))
                self._ck(L.mfm_pairs_set_cutpoints(h, cp.shape[0], cp.shape[1], _p(cp)))
            if targets is not None:
                T = sps.csr_matrix(targets)
                if T.shape != (self.U, self.I):
                    raise ValueError("targets must have shape (n_queries, n_candidates)")
                if not T.has_sorted_indices:
                    T = T.sorted_indices()
                tp = np.ascontiguousarray(T.indptr, dtype=np.int64)
                tx = np.ascontiguousarray(T.indices, dtype=np.int32)
                self._ck(L.mfm_pairs_set_targets(h, _p(tp), _p(tx)))
                self.n_targets = int(tp[-1])
        except Exception:
            self.close()
            raise

    def _ck(self, rc):
        if rc:
            _raise(rc, lib().mfm_pairs_last_error(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib().mfm_pairs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # each operation once, over a sample source (_host / _resident)
    def _scores(self, src, mode):
        out = np.empty((self.U, self.I))
        self._ck(src.call("mfm_pairs_scores", self.h, mode, _p(out)))
        return out

    def _topk(self, src, k, mode):
        kk = max(int(k), 1)
        idx, val = np.empty((self.U, kk), dtype=np.int64), np.empty((self.U, kk))
        self._ck(src.call("mfm_pairs_topk", self.h, mode, int(k), _p(idx), _p(val)))
        return idx, val

    def _moments(self, src, mode):
        mean, std = np.empty((self.U, self.I)), np.empty((self.U, self.I))
        self._ck(src.call("mfm_pairs_moments", self.h, mode, _p(mean), _p(std)))
        return mean, std

    def _topk_ucb(self, src, k, beta, mode):
        kk = max(int(k), 1)
        idx, val, mean, std = np.empty((self.U, kk), dtype=np.int64), np.empty((self.U, kk)), np.empty((self.U, kk)), np.empty((self.U, kk))
        self._ck(src.call("mfm_pairs_topk_ucb", self.h, mode, int(k), float(beta), _p(idx), _p(val), _p(mean), _p(std)))
        return idx, val, mean, std

    def moments_vb(self, model, extra_var=0.0):
        """(mean (U, I), std (U, I)) of the score of every pair under the mean-field posterior `model` (Design.moments_vb)"""
        K, head, keep = _pack_vb_model(model)
        mean, std = np.empty((self.U, self.I)), np.empty((self.U, self.I))
        self._ck(lib().mfm_pairs_moments_vb(self.h, K, *head, float(extra_var), _p(mean), _p(std)))
        return mean, std

    def topk_bound_vb(self, model, k, beta, extra_var=0.0):
        """(indices, value, mean, std), each (U, k): the top k by value = mean + beta * std of the score under `model`"""
        K, head, keep = _pack_vb_model(model)
        kk = max(int(k), 1)
        idx, val, mean, std = np.empty((self.U, kk), dtype=np.int64), np.empty((self.U, kk)), np.empty((self.U, kk)), np.empty((self.U, kk))
        self._ck(lib().mfm_pairs_topk_bound_vb(self.h, K, *head, float(extra_var), int(k), float(beta), _p(idx), _p(val), _p(mean), _p(std)))
        return idx, val, mean, std

    def _rank(self, src, mode):
        rank, val = np.empty(self.n_targets, dtype=np.int64), np.empty(self.n_targets)
        self._ck(src.call("mfm_pairs_rank", self.h, mode, _p(rank), _p(val)))
        return rank, val

    def scores(self, samples, mode=0):
        """(U, I) mean score (mode 0), mean Phi(score) (mode 1) or mean expected class index (mode 2, with `cutpoints`);
        samples: list of (w0, w[D], V[D, K])"""
        return self._scores(_host(samples), mode)

    def topk(self, samples, k, mode=0):
        """(indices int64 (U, k), values (U, k)) ordered by (value descending, index ascending); tail -1 / -inf"""
        return self._topk(_host(samples), k, mode)

    def scores_store(self, store, mode=0, first=0, count=None):
        return self._scores(_resident(store, first, count), mode)

    def topk_store(self, store, k, mode=0, first=0, count=None):
        return self._topk(_resident(store, first, count), k, mode)

    # ---- the moments form: mean and population std over the samples of the per-sample value
    def moments(self, samples, mode=0):
        """(mean (U, I), std (U, I)) of the per-sample value of every pair"""
        return self._moments(_host(samples), mode)

    def moments_store(self, store, mode=0, first=0, count=None):
        return self._moments(_resident(store, first, count), mode)

    def topk_ucb(self, samples, k, beta=1.0, mode=0):
        """(indices int64 (U, k), value, mean, std (U, k)) ranked by value = mean + beta * std under (value descending, index
        ascending). mean and std are recomputed for the selected pairs in another association than the selecting kernel's:
        value equals mean + beta * std within rounding, not bit for bit. Tail: -1 / -inf / NaN / NaN."""
        return self._topk_ucb(_host(samples), k, beta, mode)

    def topk_ucb_store(self, store, k, beta=1.0, mode=0, first=0, count=None):
        return self._topk_ucb(_resident(store, first, count), k, beta, mode)

    # ---- the similarity forms: mean and population std over the samples of the per-sample cosine / inner product
    def _sim(self, src, metric):
        mean, std = np.empty((self.U, self.I)), np.empty((self.U, self.I))
        self._ck(src.call("mfm_pairs_sim", self.h, _sim_metric(metric), _p(mean), _p(std)))
        return mean, std

    def _topk_sim(self, src, k, metric, beta):
        kk = max(int(k), 1)
        idx, val, mean, std = np.empty((self.U, kk), dtype=np.int64), np.empty((self.U, kk)), np.empty((self.U, kk)), np.empty((self.U, kk))
        self._ck(src.call("mfm_pairs_topk_sim", self.h, _sim_metric(metric), int(k), float(beta), _p(idx), _p(val), _p(mean), _p(std)))
        return idx, val, mean, std

    def sim(self, samples, metric="cosine"):
        """(mean (U, I), std (U, I)) of the per-sample cosine ("cosine") or inner product ("dot") of the two rows' embeddings;
        metric: one of the two names or the C ABI's number. An empty row or an all-zero embedding gives 0 under both."""
        return self._sim(_host(samples), metric)

    def sim_store(self, store, metric="cosine", first=0, count=None):
        return self._sim(_resident(store, first, count), metric)

    def topk_sim(self, samples, k, metric="cosine", beta=0.0):
        """(indices int64 (U, k), value, mean, std (U, k)) ranked by value = mean + beta * std of the similarity, as topk_ucb ranks
        the score; the handle's exclusions are left out. Tail: -1 / -inf / NaN / NaN."""
        return self._topk_sim(_host(samples), k, metric, beta)

    def topk_sim_store(self, store, k, metric="cosine", beta=0.0, first=0, count=None):
        return self._topk_sim(_resident(store, first, count), k, metric, beta)

    # ---- the rank form
    def rank(self, samples, mode=0):
        """(rank int64 (nnz,), value (nnz,)) of the handle's `targets`, in the order of targets.indices after sort_indices():
        rank = the number of non-excluded candidates of the target's query that beat it under (value descending, index
        ascending), the target itself apart; value = the pair's value, bit for bit that of scores / topk"""
        return self._rank(_host(samples), mode)

    def rank_store(self, store, mode=0, first=0, count=None):
        return self._rank(_resident(store, first, count), mode)

    # ---- the per-sample selecting form and the vote
    def _topk_samples(self, src, k, mode, row_sample):
        kk = max(int(k), 1)
        if row_sample is None:
            shape, rs = (src.S, self.U, kk), None
        else:
            rs = np.ascontiguousarray(row_sample, dtype=np.int32)
            if rs.shape != (self.U,):
                raise ValueError("row_sample must have one entry per query row")
            shape = (self.U, kk)
        idx, val = np.empty(shape, dtype=np.int64), np.empty(shape)
        self._ck(src.call("mfm_pairs_topk_samples", self.h, mode, int(k), None if rs is None else _p(rs), _p(idx), _p(val)))
        return idx, val

    def _topk_prob(self, src, k, n_top, mode):
        nn = max(int(n_top), 1)
        idx, prob = np.empty((self.U, nn), dtype=np.int64), np.empty((self.U, nn))
        self._ck(src.call("mfm_pairs_topk_prob", self.h, mode, int(k), int(n_top), _p(idx), _p(prob)))
        return idx, prob

    def topk_samples(self, samples, k, mode=0, row_sample=None):
        """every sample's own top k under (value descending, index ascending): (indices int64 (S, U, k), values (S, U, k)); with
        row_sample (U,) ints in [0, S) only the list of row u under sample row_sample[u]: (U, k) each. Tail -1 / -inf."""
        return self._topk_samples(_host(samples), k, mode, row_sample)

    def topk_samples_store(self, store, k, mode=0, row_sample=None, first=0, count=None):
        return self._topk_samples(_resident(store, first, count), k, mode, row_sample)

    def topk_prob(self, samples, k, n_top=None, mode=0):
        """(indices int64 (U, n_top), probability (U, n_top)): the candidates that the most samples hold among their k best and
        the share of the samples that do, ordered by (count descending, index ascending); missing entries -1 / 0.0. S * k may
        not exceed PAIRS_VOTE_MAX."""
        return self._topk_prob(_host(samples), k, k if n_top is None else n_top, mode)

    def topk_prob_store(self, store, k, n_top=None, mode=0, first=0, count=None):
        return self._topk_prob(_resident(store, first, count), k, k if n_top is None else n_top, mode)


def group_by_entity(X, y, entity, n_entities):
    """the observations grouped by entity with a stable sort: (X rows in that order, y, offsets int64 (U + 1,))"""
    entity = np.ascontiguousarray(entity, dtype=np.int64)
    order = np.argsort(entity, kind="stable")
    offsets = np.zeros(int(n_entities) + 1, dtype=np.int64)
    np.cumsum(np.bincount(entity, minlength=int(n_entities)), out=offsets[1:])
    return sps.csr_matrix(X, dtype=np.float64)[order], _f64(y)[order], offsets


class FoldIn:
    """The observations of U new one-hot entities resident on the GPU (mfm_foldin_*): X (n, D) the context rows in the model's
    feature space, y (n,), entity (n,) in [0, U) in any order. `scratch_bound`: bytes of results per chunk of entities and
    samples (default 256 MB; a small value makes a small problem cross the chunking)."""

    def __init__(self, X, y, entity, n_entities, fit_linear=True, scratch_bound=None, device=0):
        L = lib()
        h = C.c_void_p()
        Xg, yg, off = group_by_entity(X, y, entity, n_entities)
        Xg, ip, ix, dv = csr_parts(Xg)
        rc = L.mfm_foldin_create(device, Xg.shape[1], Xg.shape[0], _p(ip), _p(ix), _p(dv), _p(yg), int(n_entities), _p(off),
                                 int(bool(fit_linear)), C.byref(h))
        if rc:
            _raise(rc, L.mfm_foldin_last_error(None))
        self.h, self.U, self.D = h, int(n_entities), Xg.shape[1]
        if scratch_bound is not None:
            self._ck(L.mfm_foldin_set_scratch_bound(h, int(scratch_bound)))

    def _ck(self, rc):
        if rc:
            _raise(rc, lib().mfm_foldin_last_error(self.h))

    def close(self):
        if getattr(self, "h", None):
            lib().mfm_foldin_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _hypers(S, K, alpha, mu, lam):
        alpha, mu, lam = _f64(alpha).reshape(-1), _f64(mu), _f64(lam)
        if alpha.shape != (S,) or mu.shape != (S, K + 1) or lam.shape != (S, K + 1):
            raise ValueError("alpha must have shape (S,), mu and lam (S, K + 1)")
        return alpha, mu, lam

    # each operation once, over a sample source (_host / _resident)
    def _solve(self, src, alpha, mu, lam, draw, seed):
        alpha, mu, lam = self._hypers(src.S, src.K, alpha, mu, lam)
        w_new, V_new = np.empty((src.S, self.U)), np.empty((src.S, self.U, src.K))
        self._ck(src.call("mfm_foldin_solve", self.h, _p(alpha), _p(mu), _p(lam), int(bool(draw)), int(seed), _p(w_new), _p(V_new)))
        return w_new, V_new

    def solve(self, samples, alpha, mu, lam, draw=False, seed=0):
        """(w_new (S, U), V_new (S, U, K)) under host samples, a list of (w0, w[D], V[D, K]); alpha (S,), mu / lam (S, K + 1)"""
        return self._solve(_host(samples), alpha, mu, lam, draw, seed)

    def solve_store(self, store, alpha, mu, lam, draw=False, seed=0, first=0, count=None):
        return self._solve(_resident(store, first, count), alpha, mu, lam, draw, seed)

    FOLDIN_TASKS = {"classifier": 0, "ordered": 1}

    def _solve_gibbs(self, src, mu, lam, task, cutpoints, n_burn, n_inner, draw, seed):
        _, mu, lam = self._hypers(src.S, src.K, np.ones(src.S), mu, lam)
        if task not in self.FOLDIN_TASKS:
            raise ValueError("task must be 'classifier' or 'ordered'")
        n_class, cut = 0, None
        if task == "ordered":
            cut = _f64(cutpoints)
            if cut.ndim != 2 or cut.shape[0] != src.S or cut.shape[1] < 1:
                raise ValueError("cutpoints must have shape (S, n_class - 1)")
            n_class = cut.shape[1] + 1
        w_new, V_new = np.empty((src.S, self.U)), np.empty((src.S, self.U, src.K))
        self._ck(src.call("mfm_foldin_gibbs_solve", self.h, self.FOLDIN_TASKS[task], n_class, _p(cut), _p(mu), _p(lam), int(n_burn),
                          int(n_inner), int(bool(draw)), int(seed), _p(w_new), _p(V_new)))
        return w_new, V_new

    def solve_gibbs(self, samples, mu, lam, task, cutpoints=None, n_burn=10, n_inner=40, draw=False, seed=0):
        """(w_new (S, U), V_new (S, U, K)) of a probit model under host samples by the inner chain (mfm_foldin_gibbs_solve): task
        'classifier' (the handle's y is +-1) or 'ordered' (class indices; cutpoints (S, n_class - 1)); mu / lam (S, K + 1)"""
        return self._solve_gibbs(_host(samples), mu, lam, task, cutpoints, n_burn, n_inner, draw, seed)

    def solve_gibbs_store(self, store, mu, lam, task, cutpoints=None, n_burn=10, n_inner=40, draw=False, seed=0, first=0, count=None):
        return self._solve_gibbs(_resident(store, first, count), mu, lam, task, cutpoints, n_burn, n_inner, draw, seed)
