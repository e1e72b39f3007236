"""ctypes bindings of include/tsgo.h.  Loading fails loudly: there is no Python/CPU fallback."""
import ctypes as C
import os

from . import build
from .graph import tsgo_graph

TSGO_MAX_TRACE = 256


class tsgo_config(C.Structure):
    _fields_ = [("device", C.c_int32), ("precision", C.c_int32), ("pcg_rel_tol", C.c_double),
                ("pcg_max_iters", C.c_int32), ("lanes_per_pose", C.c_int32), ("lanes_per_lm", C.c_int32),
                ("use_graphs", C.c_int32), ("rank", C.c_int32), ("world", C.c_int32), ("verbose", C.c_int32),
                ("preconditioner", C.c_int32), ("xcd_map", C.c_int32), ("warm_start", C.c_int32), ("rules", C.c_int32), ("lr", C.c_double), ("odom_jacobian", C.c_int32), ("reuse_structure", C.c_int32), ("cycle_level0", C.c_int32), ("cycle_storage", C.c_int32), ("warm_requests", C.c_int32),
                ("lm_lambda0", C.c_double), ("lm_chi2_rel_tol", C.c_double)]


class tsgo_stats(C.Structure):
    _fields_ = [("iterations_run", C.c_int32), ("stop_reason", C.c_int32), ("chi2", C.c_double * TSGO_MAX_TRACE),
                ("pcg_iters", C.c_int32 * TSGO_MAX_TRACE), ("last_delta_norm", C.c_double),
                ("ms_total", C.c_double), ("ms_linearize", C.c_double), ("ms_solve", C.c_double),
                ("ms_update", C.c_double), ("ms_setup", C.c_double), ("structure_reused", C.c_int32), ("cycle_storage_now", C.c_int32), ("lambda_last", C.c_double), ("n_pose", C.c_int64), ("n_lm", C.c_int64),
                ("n_odom_edges", C.c_int64), ("n_lm_edges", C.c_int64), ("pcg_iters_total", C.c_int64),
                ("pcg_fallbacks", C.c_int32), ("trace_len", C.c_int32), ("chi2_last", C.c_double), ("history_carried", C.c_int32), ("graph_replay", C.c_int32),
                ("steps_rejected", C.c_int32), ("lm_lambda", C.c_double * TSGO_MAX_TRACE), ("lm_gain", C.c_double * TSGO_MAX_TRACE),
                ("lm_pred", C.c_double * TSGO_MAX_TRACE), ("lm_chi2_trial", C.c_double * TSGO_MAX_TRACE)]


class tsgo_marginal_stats(C.Structure):
    _fields_ = [("columns", C.c_int32), ("batches", C.c_int32), ("batch_width", C.c_int32), ("pcg_iters_max", C.c_int32),
                ("pcg_iters_total", C.c_int64), ("preconditioner", C.c_int32), ("fallbacks", C.c_int32),
                ("ms_total", C.c_double), ("ms_solve", C.c_double)]


class tsgo_robust(C.Structure):
    _fields_ = [("kernel", C.c_int32 * 5), ("reserved", C.c_int32), ("delta", C.c_double * 5)]


TSGO_EDGE_ROBUST_MAX = 15


class tsgo_edge_robust_entry(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("reserved", C.c_int32), ("delta", C.c_double)]


class tsgo_edge_robust_stats(C.Structure):
    _fields_ = [("edges_by_entry", C.c_int64 * (TSGO_EDGE_ROBUST_MAX + 1)), ("overridden_by_class", C.c_int64 * 5), ("active", C.c_int32),
                ("reserved", C.c_int32), ("ms_total", C.c_double)]


class tsgo_dogleg_params(C.Structure):
    _fields_ = [("radius0", C.c_double), ("radius_min", C.c_double), ("radius_max", C.c_double), ("chi2_rel_tol", C.c_double)]


class tsgo_dogleg_trace(C.Structure):
    _fields_ = [("trials", C.c_int32), ("solves", C.c_int32), ("kind", C.c_int32 * TSGO_MAX_TRACE), ("solved", C.c_int32 * TSGO_MAX_TRACE)] + \
               [(n, C.c_double * TSGO_MAX_TRACE) for n in ("radius", "step_norm", "gg", "gHg", "gd", "dd")] + [("radius_last", C.c_double)]


class tsgo_edge_class_summary(C.Structure):
    _fields_ = [("edges", C.c_int64), ("downweighted", C.c_int64), ("s_sum", C.c_double), ("rho_sum", C.c_double), ("s_max", C.c_double),
                ("s_max_edge", C.c_int64)]


class tsgo_edge_report_stats(C.Structure):
    _fields_ = [("cls", tsgo_edge_class_summary * 5), ("chi2", C.c_double), ("ms_total", C.c_double)]


class tsgo_gate_stats(C.Structure):
    _fields_ = [("candidates", C.c_int32), ("vertices", C.c_int32), ("not_pd", C.c_int32), ("reserved", C.c_int32),
                ("solve", tsgo_marginal_stats), ("ms_total", C.c_double), ("ms_readout", C.c_double)]


class tsgo_sample_stats(C.Structure):
    _fields_ = [("samples", C.c_int32), ("reserved", C.c_int32), ("solve", tsgo_marginal_stats),
                ("ms_total", C.c_double), ("ms_noise", C.c_double), ("ms_readout", C.c_double)]


class tsgo_leverage_stats(C.Structure):
    _fields_ = [("samples", C.c_int32), ("reserved", C.c_int32), ("edges", C.c_int64 * 5), ("h_sum", C.c_double * 5), ("dof_sum", C.c_double * 5),
                ("h_gauge", C.c_double), ("trace", C.c_double), ("unknowns", C.c_int64), ("solve", tsgo_marginal_stats),
                ("ms_total", C.c_double), ("ms_noise", C.c_double), ("ms_readout", C.c_double)]


class tsgo_init_stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("poses_set", "landmarks_set", "roots_fixed", "roots_free", "edges_usable", "tree_edges", "landmarks_unobserved")] + \
               [("depth_max", C.c_int32), ("rounds", C.c_int32), ("ms_total", C.c_double), ("ms_tree", C.c_double), ("ms_device", C.c_double)]


INIT_POSES, INIT_LANDMARKS = 1, 2      # TSGO_INIT_*


class tsgo_edge_info_stats(C.Structure):
    _fields_ = [("edges_listed", C.c_int64), ("edges_by_class", C.c_int64 * 5), ("maps_built", C.c_int32), ("reserved", C.c_int32),
                ("ms_total", C.c_double), ("ms_host", C.c_double), ("ms_device", C.c_double)]


class tsgo_vertex_edit_stats(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("listed", "poses", "landmarks", "fixed_now", "released")] + [(n, C.c_double) for n in ("ms_total", "ms_host", "ms_device")]


TSGO_GNC_MAX_ROUNDS = 128
GNC_STOP = {0: "all_inliers", 1: "binary", 2: "rounds", 3: "solver_failed"}      # TSGO_GNC_*


class tsgo_gnc_params(C.Structure):
    _fields_ = [("barc2", C.c_double * 5), ("mu_step", C.c_double), ("rounds_max", C.c_int32), ("inner_iterations", C.c_int32),
                ("keep_weights", C.c_int32), ("reserved", C.c_int32)]


class tsgo_gnc_stats(C.Structure):
    _R = TSGO_GNC_MAX_ROUNDS
    _fields_ = [("rounds", C.c_int32), ("stop_reason", C.c_int32), ("q_max", C.c_double), ("mu", C.c_double * _R), ("cost", C.c_double * _R),
                ("chi2_inner", C.c_double * _R), ("inner_iterations_run", C.c_int32 * _R), ("inner_stop", C.c_int32 * _R),
                ("n_zero", C.c_int64 * _R), ("n_one", C.c_int64 * _R), ("n_between", C.c_int64 * _R), ("subject_by_class", C.c_int64 * 5),
                ("pcg_iters_total", C.c_int64), ("ms_total", C.c_double), ("ms_reweight", C.c_double), ("ms_inner", C.c_double)]


TSGO_MIX_MAX_ROUNDS = 128
TSGO_MIX_MAX_MEMBERS = 64
MIX_STOP = {0: "stable", 1: "rounds", 2: "solver"}      # TSGO_MIX_*


class tsgo_mixture_params(C.Structure):
    _fields_ = [("rounds_max", C.c_int32), ("inner_iterations", C.c_int32), ("keep_selection", C.c_int32), ("reserved", C.c_int32)]


class tsgo_mixture_stats(C.Structure):
    _R = TSGO_MIX_MAX_ROUNDS + 1
    _fields_ = [("rounds", C.c_int32), ("passes", C.c_int32), ("stop_reason", C.c_int32), ("reserved", C.c_int32),
                ("n_changed", C.c_int64 * _R), ("cost_sum", C.c_double * _R), ("chi2_inner", C.c_double * _R),
                ("inner_iterations_run", C.c_int32 * _R), ("inner_stop", C.c_int32 * _R), ("groups", C.c_int64), ("members", C.c_int64),
                ("members_by_class", C.c_int64 * 5), ("pcg_iters_total", C.c_int64), ("ms_total", C.c_double), ("ms_select", C.c_double),
                ("ms_inner", C.c_double)]


ROBUST_KERNELS = {"none": 0, "huber": 1, "cauchy": 2, "geman_mcclure": 3}      # TSGO_ROBUST_*
ROBUST_CLASSES = ("odom", "lm", "virtual", "pose_prior", "lm_prior")            # = tsgo_graph.e_type 0 .. 4


class tsgo_cycle_level(C.Structure):
    _fields_ = [("rows", C.c_int64), ("blocks", C.c_int64), ("sweeps_per_cycle", C.c_int32), ("lanes_per_row", C.c_int32),
                ("us_per_sweep", C.c_double), ("bytes_per_sweep", C.c_double)]


class tsgo_prof_entry(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("where", C.c_char * 32), ("launches_per_iteration", C.c_int32), ("reserved", C.c_int32),
                ("us", C.c_double), ("bytes", C.c_double)]


class tsgo_synth_config(C.Structure):
    _fields_ = [("n_poses", C.c_int64), ("lm_per_pose", C.c_int32), ("lm_obs_target", C.c_double),
                ("loop_closures", C.c_int32), ("seed", C.c_uint64)]


class tsgo_layout_info(C.Structure):
    _fields_ = [(n, C.c_int64) for n in ("n_pose", "n_lm_local", "n_lm_total", "n_lm_edges_local", "n_odom_slots",
                                         "rows_by_pose", "rows_by_lm", "rows_odom")] + \
               [("lanes_per_pose", C.c_int32), ("lanes_per_lm", C.c_int32)] + \
               [(n, C.c_int64) for n in ("lm_first", "lm_last", "pose_first", "pose_last")]


class tsgo_amg_info(C.Structure):
    _fields_ = [("n_levels", C.c_int32), ("rows", C.c_int64 * 8), ("blocks", C.c_int64 * 8), ("p_blocks", C.c_int64 * 8),
                ("schur_contribs", C.c_int64), ("ms_layout", C.c_double), ("ms_symbolic", C.c_double),
                ("agg_min", C.c_int32 * 8), ("agg_max", C.c_int32 * 8), ("checksum", C.c_uint64)]


class tsgo_testing_sym_out(C.Structure):
    _fields_ = [("cap_blocks", C.c_int64), ("cap_pairs", C.c_int64)] + [(n, C.c_void_p) for n in ("zptr", "zcol", "pl_ptr", "px", "py", "mirror", "upper", "n_upper")] + \
               [("nnz", C.c_int64), ("pairs", C.c_int64), ("upper_blocks", C.c_int64), ("declined", C.c_int32), ("not_symmetric", C.c_int32)]


class tsgo_testing_schur_out(C.Structure):
    _fields_ = [("cap_blocks", C.c_int64), ("cap_pairs", C.c_int64), ("cap_od", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("zptr", "zcol", "sc_ptr", "sc_optr", "slot_i", "slot_k", "os")] + \
               [("nnz", C.c_int64), ("pairs", C.c_int64), ("od", C.c_int64), ("declined", C.c_int32), ("reserved", C.c_int32)]


class tsgo_testing_warm_out(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("warmed", "n_prev", "n_tested", "n_max", "order", "done", "carried")] + \
               [("err", C.c_double * 6), ("scale", C.c_double), ("bdb", C.c_double), ("rdr", C.c_double)] + [(n, C.c_void_p) for n in ("hist", "b", "x0", "r0")]


HOST_SYMBOLS = ["tsgo_default_config", "tsgo_default_robust", "tsgo_default_gnc", "tsgo_default_mixture", "tsgo_default_dogleg", "tsgo_last_error", "tsgo_wire_decode", "tsgo_wire_new", "tsgo_wire_decode_into", "tsgo_wire_view", "tsgo_wire_free",
                "tsgo_wire_encode_response", "tsgo_wire_encode_request", "tsgo_synth_create", "tsgo_synth_view",
                "tsgo_synth_truth", "tsgo_synth_free", "tsgo_layout_probe", "tsgo_amg_probe", "tsgo_amg_probe_shard", "tsgo_init_tree", "tsgo_sample_noise"]
DEVICE_SYMBOLS = ["tsgo_device_count", "tsgo_create", "tsgo_destroy", "tsgo_set_graph", "tsgo_reset_history", "tsgo_optimize", "tsgo_get_vertices",
                  "tsgo_linearize", "tsgo_solve_step", "tsgo_comm_unique_id", "tsgo_comm_init", "tsgo_comm_selftest", "tsgo_comm_time_allreduce", "tsgo_time_kernel", "tsgo_cycle_probe", "tsgo_profile_iteration",
                  "tsgo_marginals", "tsgo_joint_marginals", "tsgo_set_robust", "tsgo_get_robust", "tsgo_edge_report", "tsgo_gate_edges", "tsgo_init_estimates",
                  "tsgo_set_edge_information", "tsgo_get_edge_information", "tsgo_gnc", "tsgo_sample_marginals", "tsgo_set_dogleg", "tsgo_get_dogleg", "tsgo_get_dogleg_trace",
                  "tsgo_set_edge_robust", "tsgo_get_edge_robust", "tsgo_set_fixed", "tsgo_get_fixed", "tsgo_set_estimates", "tsgo_edge_leverage", "tsgo_max_mixture"]
TESTING_SYMBOLS = ["tsgo_local_group_create", "tsgo_local_group_destroy", "tsgo_comm_init_local", "tsgo_testing_apply",
                   "tsgo_testing_sym_scan", "tsgo_testing_sym_product", "tsgo_testing_schur_pattern", "tsgo_testing_lane_sums", "tsgo_testing_warm_start"]      # include/tsgo_testing.h: libtsgo_hip_testing.so only


def _declare_host(L):
    vp, u8p = C.c_void_p, C.POINTER(C.c_uint8)
    L.tsgo_default_config.argtypes = [C.POINTER(tsgo_config)]; L.tsgo_default_config.restype = None
    L.tsgo_default_robust.argtypes = [C.POINTER(tsgo_robust)]; L.tsgo_default_robust.restype = None
    L.tsgo_default_gnc.argtypes = [C.POINTER(tsgo_gnc_params)]; L.tsgo_default_gnc.restype = None
    L.tsgo_default_dogleg.argtypes = [C.POINTER(tsgo_dogleg_params)]; L.tsgo_default_dogleg.restype = None
    L.tsgo_default_mixture.argtypes = [C.POINTER(tsgo_mixture_params)]; L.tsgo_default_mixture.restype = None
    L.tsgo_last_error.restype = C.c_char_p
    L.tsgo_wire_decode.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(vp)]
    L.tsgo_wire_new.argtypes = []; L.tsgo_wire_new.restype = vp
    L.tsgo_wire_decode_into.argtypes = [vp, C.c_char_p, C.c_size_t]
    L.tsgo_wire_view.argtypes = [vp, C.POINTER(tsgo_graph)]; L.tsgo_wire_view.restype = None
    L.tsgo_wire_free.argtypes = [vp]; L.tsgo_wire_free.restype = None
    L.tsgo_wire_encode_response.argtypes = [vp, vp, vp, C.c_size_t]; L.tsgo_wire_encode_response.restype = C.c_int64
    L.tsgo_wire_encode_request.argtypes = [C.POINTER(tsgo_graph), vp, C.c_size_t]; L.tsgo_wire_encode_request.restype = C.c_int64
    L.tsgo_synth_create.argtypes = [C.POINTER(tsgo_synth_config), C.POINTER(vp)]
    L.tsgo_synth_view.argtypes = [vp, C.POINTER(tsgo_graph)]; L.tsgo_synth_view.restype = None
    L.tsgo_synth_truth.argtypes = [vp]; L.tsgo_synth_truth.restype = C.POINTER(C.c_double)
    L.tsgo_synth_free.argtypes = [vp]; L.tsgo_synth_free.restype = None
    L.tsgo_layout_probe.argtypes = [C.POINTER(tsgo_graph), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                    C.POINTER(tsgo_layout_info)]
    L.tsgo_amg_probe.argtypes = [C.POINTER(tsgo_graph), C.POINTER(tsgo_amg_info)]
    L.tsgo_amg_probe_shard.argtypes = [C.POINTER(tsgo_graph), C.c_int32, C.c_int32, C.POINTER(tsgo_amg_info), C.POINTER(C.c_int64)]
    L.tsgo_init_tree.argtypes = [C.POINTER(tsgo_graph), vp, C.c_int64, vp, vp, vp, C.POINTER(tsgo_init_stats)]
    L.tsgo_sample_noise.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp]; L.tsgo_sample_noise.restype = None
    del u8p


def _declare_device(L):
    vp = C.c_void_p
    L.tsgo_create.argtypes = [C.POINTER(tsgo_config), C.POINTER(vp)]
    L.tsgo_destroy.argtypes = [vp]; L.tsgo_destroy.restype = None
    L.tsgo_set_graph.argtypes = [vp, C.POINTER(tsgo_graph)]
    L.tsgo_optimize.argtypes = [vp, C.c_int32, C.POINTER(tsgo_stats)]
    L.tsgo_reset_history.argtypes = [vp]; L.tsgo_reset_history.restype = None
    L.tsgo_get_vertices.argtypes = [vp, vp]
    L.tsgo_linearize.argtypes = [vp, vp, vp, C.POINTER(C.c_double)]
    L.tsgo_solve_step.argtypes = [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    L.tsgo_comm_unique_id.argtypes = [vp]
    L.tsgo_comm_init.argtypes = [vp, vp]
    L.tsgo_comm_selftest.argtypes = [vp, C.POINTER(C.c_int32)]
    L.tsgo_device_count.argtypes = []
    L.tsgo_comm_time_allreduce.argtypes = [vp, C.c_int64, C.c_int32, C.POINTER(C.c_double)]
    L.tsgo_time_kernel.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.tsgo_cycle_probe.argtypes = [vp, C.c_int32, C.POINTER(tsgo_cycle_level), C.c_int32]
    L.tsgo_profile_iteration.argtypes = [vp, C.c_int32, C.POINTER(tsgo_prof_entry), C.c_int32]
    L.tsgo_marginals.argtypes = [vp, vp, C.c_int32, C.c_double, vp, C.POINTER(tsgo_marginal_stats)]
    L.tsgo_joint_marginals.argtypes = [vp, vp, C.c_int32, C.c_double, vp, C.c_int64, C.POINTER(C.c_int32), C.POINTER(tsgo_marginal_stats)]
    L.tsgo_sample_marginals.argtypes = [vp, C.c_int32, C.c_uint64, C.c_double, vp, C.c_int64, vp, C.c_int64, C.POINTER(tsgo_sample_stats)]
    L.tsgo_edge_leverage.argtypes = [vp, C.c_int32, C.c_uint64, C.c_double, vp, C.c_int64, C.POINTER(tsgo_leverage_stats)]
    L.tsgo_set_robust.argtypes = [vp, C.POINTER(tsgo_robust)]
    L.tsgo_get_robust.argtypes = [vp, C.POINTER(tsgo_robust)]
    L.tsgo_set_edge_robust.argtypes = [vp, C.c_int32, vp, vp, C.c_int64, C.POINTER(tsgo_edge_robust_stats)]
    L.tsgo_get_edge_robust.argtypes = [vp, C.POINTER(C.c_int32), vp, vp, C.c_int64]
    L.tsgo_set_dogleg.argtypes = [vp, C.POINTER(tsgo_dogleg_params)]
    L.tsgo_get_dogleg.argtypes = [vp, C.POINTER(tsgo_dogleg_params)]
    L.tsgo_get_dogleg_trace.argtypes = [vp, C.POINTER(tsgo_dogleg_trace)]
    L.tsgo_edge_report.argtypes = [vp, vp, C.c_int64, C.POINTER(tsgo_edge_report_stats)]
    L.tsgo_gate_edges.argtypes = [vp, C.c_int32, vp, vp, vp, vp, C.c_double, vp, vp, C.POINTER(tsgo_gate_stats)]
    L.tsgo_init_estimates.argtypes = [vp, C.c_int32, vp, C.c_int64, C.POINTER(tsgo_init_stats)]
    L.tsgo_set_edge_information.argtypes = [vp, C.c_int64, vp, vp, C.POINTER(tsgo_edge_info_stats)]
    L.tsgo_get_edge_information.argtypes = [vp, vp, C.c_int64]
    L.tsgo_gnc.argtypes = [vp, C.POINTER(tsgo_gnc_params), vp, C.c_int64, vp, C.c_int64, C.POINTER(tsgo_gnc_stats)]
    L.tsgo_max_mixture.argtypes = [vp, C.POINTER(tsgo_mixture_params), C.c_int64, vp, vp, vp, vp, C.c_int64, vp, C.c_int64, C.POINTER(tsgo_mixture_stats)]
    L.tsgo_set_fixed.argtypes = [vp, C.c_int64, vp, vp, C.POINTER(tsgo_vertex_edit_stats)]
    L.tsgo_get_fixed.argtypes = [vp, vp, C.c_int64]
    L.tsgo_set_estimates.argtypes = [vp, C.c_int64, vp, vp, C.POINTER(tsgo_vertex_edit_stats)]


def _declare_testing(L):
    vp = C.c_void_p
    L.tsgo_local_group_create.argtypes = [C.c_int32, C.POINTER(vp)]
    L.tsgo_local_group_destroy.argtypes = [vp]; L.tsgo_local_group_destroy.restype = None
    L.tsgo_comm_init_local.argtypes = [vp, vp]
    L.tsgo_testing_apply.argtypes = [vp, C.c_int32, vp, vp, C.c_int32]
    L.tsgo_testing_sym_scan.argtypes = [C.c_int32, vp, vp]
    L.tsgo_testing_sym_product.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, C.c_int32, C.c_int32, vp, vp, C.POINTER(tsgo_testing_sym_out)]
    L.tsgo_testing_schur_pattern.argtypes = [C.c_int32, C.c_int32, C.c_int32] + [vp] * 9 + [C.c_int32, C.POINTER(tsgo_testing_schur_out)]
    L.tsgo_testing_lane_sums.argtypes = [vp, vp, vp, vp]
    L.tsgo_testing_warm_start.argtypes = [vp, C.c_int32, vp, C.c_int32, C.POINTER(tsgo_testing_warm_out)]


_host = None
_hip = None
_hip_testing = None


def host_lib():
    """libtsgo_host.so: codec, synthetic graphs, layout probe.  No GPU needed."""
    global _host
    if _host is None:
        # TSGO_HOST_SO: an instrumented build of the same sources (tools/sanitize_host.sh: ASan + UBSan, CPU only)
        path = os.environ.get("TSGO_HOST_SO") or (build.HOST_SO if os.path.exists(build.HOST_SO) else build.build_host())
        _host = C.CDLL(path)
        _declare_host(_host)
    return _host


def hip_lib():
    """libtsgo_hip.so: the device path.  Raises if the library is missing or cannot be loaded."""
    global _hip
    if _hip is None:
        if not os.path.exists(build.HIP_SO):
            raise RuntimeError("toyslam_amd: %s is missing — run __graft_entry__.build() (hipcc, gfx950). "
                               "There is no CPU fallback." % build.HIP_SO)
        _hip = C.CDLL(build.HIP_SO)
        _declare_host(_hip)
        _declare_device(_hip)
    return _hip


def hip_testing_lib():
    """libtsgo_hip_testing.so: the same sources built with -DTSGO_TESTING — test hooks, research variables and the in-process
    all-reduce group (include/tsgo_testing.h).  Loaded by the tests that need one of those; never by the product path."""
    global _hip_testing
    if _hip_testing is None:
        if not os.path.exists(build.HIP_TESTING_SO):
            raise RuntimeError("toyslam_amd: %s is missing — run __graft_entry__.build()" % build.HIP_TESTING_SO)
        _hip_testing = C.CDLL(build.HIP_TESTING_SO)
        _declare_host(_hip_testing)
        _declare_device(_hip_testing)
        _declare_testing(_hip_testing)
    return _hip_testing


def check(lib, rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, lib.tsgo_last_error().decode()))
