"""ctypes binding of libmiosqp_hip.so (the C ABI declared in include/miosqp_amd.h).

The product path has no CPU fallback: if the shared library is missing or cannot be loaded this
module raises, and `OSQP.setup` raises when no gfx950 device is visible.
"""
import ctypes as C
import os

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "libmiosqp_hip.so")

dp = C.POINTER(C.c_double)
dpp = C.POINTER(dp)
ip = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)


class Settings(C.Structure):
    _fields_ = [(k, C.c_double) for k in
                ("rho", "sigma", "alpha", "eps_abs", "eps_rel", "eps_prim_inf", "eps_dual_inf")] + \
               [(k, C.c_int32) for k in ("max_iter", "scaling", "check_termination", "warm_start",
                                         "device", "max_batch", "fold", "resident", "setup_on_device", "coop", "pers", "batch_pers",
                                         "rho_auto")]


class Info(C.Structure):
    _fields_ = [("status_val", C.c_int32), ("iter", C.c_int32), ("run_time", C.c_double),
                ("obj_val", C.c_double), ("pri_res", C.c_double), ("dua_res", C.c_double),
                ("device_time", C.c_double), ("lower", C.c_double),
                ("int_inf", C.c_int32), ("nextvar", C.c_int32), ("heur_viol", C.c_double),
                ("heur_obj", C.c_double)]


class TreeInfo(C.Structure):
    _fields_ = [("nodes", C.c_int32), ("osqp_iter", C.c_int32), ("leaves_left", C.c_int32), ("overflow", C.c_int32),
                ("max_leaves", C.c_int32), ("found", C.c_int32), ("upper_glob", C.c_double), ("lower_glob", C.c_double),
                ("device_time", C.c_double), ("run_time", C.c_double)]


class TreeRfInfo(C.Structure):
    _fields_ = [("calls", C.c_int32), ("candidates", C.c_int32), ("feasible", C.c_int32), ("improved", C.c_int32),
                ("osqp_iter", C.c_int32), ("form", C.c_int32), ("pad0", C.c_int32), ("pad1", C.c_int32)]


class TreeSbInfo(C.Structure):
    _fields_ = [("calls", C.c_int32), ("children", C.c_int32), ("osqp_iter", C.c_int32), ("form", C.c_int32),
                ("pad0", C.c_int32), ("pad1", C.c_int32), ("pad2", C.c_int32), ("pad3", C.c_int32)]


class ModelsStats(C.Structure):
    _fields_ = [("launches", C.c_int32), ("models_wave", C.c_int32), ("models_group", C.c_int32), ("pad", C.c_int32),
                ("lds_bytes", C.c_int64), ("device_time", C.c_double), ("run_time", C.c_double)]


class PolishModelsStats(C.Structure):
    _fields_ = [("launches", C.c_int32), ("models", C.c_int32), ("lds_bytes", C.c_int64), ("arena_bytes", C.c_int64),
                ("device_time", C.c_double), ("run_time", C.c_double), ("upload_time", C.c_double),
                ("launch_time", C.c_double), ("download_time", C.c_double)]


class PolishModelsLargeStats(C.Structure):
    _fields_ = [("launches", C.c_int32), ("models", C.c_int32), ("workgroups", C.c_int32), ("pad", C.c_int32),
                ("slab_bytes", C.c_int64), ("arena_bytes", C.c_int64), ("device_time", C.c_double),
                ("run_time", C.c_double), ("upload_time", C.c_double), ("launch_time", C.c_double),
                ("download_time", C.c_double)]


class SetupModel(C.Structure):
    _fields_ = [("n", C.c_int32), ("M", C.c_int32), ("Pp", ip), ("Pi", ip), ("Px", dp), ("Ap", ip), ("Ai", ip), ("Ax", dp),
                ("q", dp), ("l", dp), ("u", dp), ("settings", C.POINTER(Settings)), ("n_int", C.c_int32), ("m_orig", C.c_int32),
                ("i_idx", ip), ("l_root", dp), ("u_root", dp), ("eps_int_feas", C.c_double), ("eps_lin", C.c_double)]


class SetupModelsStats(C.Structure):
    _fields_ = [("models", C.c_int32), ("launches", C.c_int32), ("device_mallocs", C.c_int32), ("host_mallocs", C.c_int32),
                ("streams", C.c_int32), ("reserved", C.c_int32), ("arena_bytes", C.c_int64), ("pinned_bytes", C.c_int64),
                ("lds_bytes", C.c_int64), ("device_time", C.c_double), ("run_time", C.c_double)]


class LockstepStats(C.Structure):
    _fields_ = [("waves", C.c_int32), ("max_width", C.c_int32), ("grown", C.c_int32), ("wave_cap", C.c_int32),
                ("nodes", C.c_int64), ("iters_slowest", C.c_int64), ("iters_all", C.c_int64), ("device_time", C.c_double),
                ("run_time", C.c_double), ("host_time", C.c_double), ("wave_width", ip), ("wave_iter_max", ip), ("wave_iter_mean", dp),
                ("finished_at", ip), ("node_hviol", dp), ("node_cap", C.c_int32), ("reserved", C.c_int32)]


class LockstepRfStats(C.Structure):
    _fields_ = [("batches", C.c_int32), ("reserved", C.c_int32), ("columns", C.c_int64), ("iters_slowest", C.c_int64),
                ("device_time", C.c_double), ("calls", ip), ("candidates", ip), ("feasible", ip), ("improved", ip),
                ("iters", i64p), ("cand_status", ip), ("cand_iter", ip), ("cand_obj", dp), ("cand_viol", dp)]


class LockstepSbStats(C.Structure):
    _fields_ = [("batches", C.c_int32), ("reserved", C.c_int32), ("columns", C.c_int64), ("iters_slowest", C.c_int64),
                ("device_time", C.c_double), ("calls", ip), ("children", ip), ("iters", i64p), ("first_k", ip),
                ("first_chosen", ip), ("first_cand", ip), ("first_status", ip), ("first_iter", ip), ("first_lower", dp)]


class LockstepAheadStats(C.Structure):
    _fields_ = [("waves", C.c_int32), ("wave_cap", C.c_int32), ("columns", C.c_int64), ("sent", C.c_int64),
                ("hits", C.c_int64), ("discarded", C.c_int64), ("called_off", C.c_int64), ("hit_iters", C.c_int64),
                ("discarded_iters", C.c_int64), ("called_off_iters", C.c_int64), ("free_slots", C.c_int32),
                ("slot_cap", C.c_int32), ("wave_width", ip), ("wave_iter_mandatory", ip), ("wave_chunks", ip)]


class RefillStats(C.Structure):
    _fields_ = [("chunks", C.c_int32), ("columns", C.c_int32), ("grown", C.c_int32), ("chunk_cap", C.c_int32),
                ("nodes", C.c_int64), ("iters_all", C.c_int64), ("col_chunks_busy", C.c_int64),
                ("col_chunks_total", C.c_int64), ("device_time", C.c_double), ("run_time", C.c_double),
                ("host_time", C.c_double), ("chunk_time", C.c_double), ("nodes_max_iter", C.c_int64),
                ("iters_max_iter", C.c_int64), ("chunk_busy", ip), ("finished_at", ip)]


class SearchInfo(C.Structure):
    _fields_ = [("nodes", C.c_int64), ("osqp_iter", C.c_int64), ("open_leaves", C.c_int32), ("free_slots", C.c_int32),
                ("improved", C.c_int32), ("reserved", C.c_int32), ("upper_glob", C.c_double), ("lower_glob", C.c_double),
                ("device_time", C.c_double), ("run_time", C.c_double)]


class StreamInfo(C.Structure):
    _fields_ = [("alive", C.c_int64), ("open_leaves", C.c_int64), ("in_flight", C.c_int64), ("free_slots", C.c_int64),
                ("nodes", C.c_int64), ("osqp_iter", C.c_int64), ("chunks", C.c_int64), ("dropped", C.c_int64),
                ("improved", C.c_int32), ("active", C.c_int32), ("upper_glob", C.c_double)]


class SbInfo(C.Structure):
    _fields_ = [("chosen", C.c_int32), ("children", C.c_int32), ("iters", C.c_int32), ("device_time", C.c_double),
                ("run_time", C.c_double)]


class RfInfo(C.Structure):
    _fields_ = [("chosen", C.c_int32), ("feasible", C.c_int32), ("candidates", C.c_int32), ("iters", C.c_int32),
                ("device_time", C.c_double), ("run_time", C.c_double)]


class PolishInfo(C.Structure):
    _fields_ = [("accepted", C.c_int32), ("reason", C.c_int32), ("n_lower", C.c_int32), ("n_upper", C.c_int32),
                ("pri_before", C.c_double), ("dua_before", C.c_double), ("pri_after", C.c_double),
                ("dua_after", C.c_double), ("obj", C.c_double), ("device_time", C.c_double), ("run_time", C.c_double)]


class PolishRepairInfo(C.Structure):
    _fields_ = [("polish", PolishInfo), ("rounds", C.c_int32), ("stop", C.c_int32), ("n_added", C.c_int32),
                ("n_dropped", C.c_int32), ("accepted0", C.c_int32), ("reason0", C.c_int32)]


class PoolDigest(C.Structure):
    _fields_ = [("slot", C.c_int32), ("status_val", C.c_int32), ("iter", C.c_int32), ("int_inf", C.c_int32),
                ("nextvar", C.c_int32), ("reserved", C.c_int32), ("lower", C.c_double), ("heur_viol", C.c_double),
                ("heur_obj", C.c_double), ("pri_res", C.c_double), ("dua_res", C.c_double)]


# every symbol include/miosqp_amd.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "miosqp_qp_default_settings": (C.c_int, [C.POINTER(Settings)]),
    "miosqp_qp_constant": (C.c_int, [C.c_char_p]),
    "miosqp_qp_setup": (C.c_int, [C.POINTER(C.c_void_p), C.c_int32, C.c_int32, ip, ip, dp, ip, ip,
                                  dp, dp, dp, dp, C.POINTER(Settings)]),
    "miosqp_qp_update_bounds": (C.c_int, [C.c_void_p, dp, dp]),
    "miosqp_qp_update_lin_cost": (C.c_int, [C.c_void_p, dp]),
    "miosqp_qp_warm_start": (C.c_int, [C.c_void_p, dp, dp]),
    "miosqp_qp_solve": (C.c_int, [C.c_void_p, dp, dp, C.POINTER(Info)]),
    "miosqp_qp_set_integer_rows": (C.c_int, [C.c_void_p, C.c_int32, ip, C.c_int32]),
    "miosqp_qp_set_root": (C.c_int, [C.c_void_p, dp, dp, C.c_double, C.c_double]),
    "miosqp_qp_solve_node": (C.c_int, [C.c_void_p, dp, dp, dp, dp, dp, dp, C.POINTER(Info)]),
    "miosqp_qp_strong_branch": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.c_double, C.c_int32, ip, C.c_int32, C.c_double,
                                          dp, ip, ip, dp, C.POINTER(SbInfo)]),
    "miosqp_qp_round_and_fix": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.c_double, C.c_int32, C.c_int32, dp, ip, ip, dp, dp,
                                          C.POINTER(RfInfo)]),
    "miosqp_qp_polish": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.c_double, C.c_int32, dp, dp, C.POINTER(PolishInfo)]),
    "miosqp_qp_get_polish_stages": (C.c_int, [C.c_void_p, dp]),
    "miosqp_qp_polish_repair": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.c_double, C.c_int32, C.c_int32, dp, dp,
                                          C.POINTER(PolishRepairInfo)]),
    "miosqp_qp_get_polish_repair_trace": (C.c_int, [C.c_void_p, C.POINTER(C.c_int8), dp, dp]),
    "miosqp_qp_polish_many": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, C.c_double, C.c_int32, C.c_int32, dp, dp,
                                        C.POINTER(PolishRepairInfo)]),
    "miosqp_qp_get_polish_many_classes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int8)]),
    "miosqp_qp_polish_many_large": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, C.c_double, C.c_int32, C.c_int32,
                                              dp, dp, C.POINTER(PolishRepairInfo)]),
    "miosqp_qp_get_polish_many_large_classes": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int8)]),
    "miosqp_qp_solve_trees": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32, dp,
                                        C.POINTER(TreeInfo)]),
    "miosqp_qp_tree_form": (C.c_int, [C.c_void_p]),
    "miosqp_qp_solve_trees_models": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), dpp, dpp, dpp, dpp, dpp, dp, dpp, ip, ip, dpp,
                                               C.POINTER(TreeInfo), C.POINTER(ModelsStats)]),
    "miosqp_qp_tree_form_large": (C.c_int, [C.c_void_p, C.c_int32]),
    "miosqp_qp_solve_trees_models_large": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), dpp, dpp, dpp, dpp, dpp, dp, dpp, ip, ip,
                                                     C.c_int32, dpp, C.POINTER(TreeInfo), C.POINTER(ModelsStats)]),
    "miosqp_qp_solve_trees_rf": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, dp, C.POINTER(TreeInfo), C.POINTER(TreeRfInfo)]),
    "miosqp_qp_solve_trees_models_rf": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), dpp, dpp, dpp, dpp, dpp, dp, dpp, ip, ip,
                                                  C.c_int32, ip, ip, ip, dpp, C.POINTER(TreeInfo), C.POINTER(TreeRfInfo),
                                                  C.POINTER(ModelsStats)]),
    "miosqp_qp_solve_trees_sb": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32, C.c_int32,
                                           C.c_int32, C.c_int32, C.c_int32, C.c_double, dp, C.POINTER(TreeInfo),
                                           C.POINTER(TreeSbInfo)]),
    "miosqp_qp_solve_trees_models_sb": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), dpp, dpp, dpp, dpp, dpp, dp, dpp, ip, ip,
                                                  C.c_int32, ip, ip, ip, ip, dp, dpp, C.POINTER(TreeInfo), C.POINTER(TreeSbInfo),
                                                  C.POINTER(ModelsStats)]),
    "miosqp_qp_solve_trees_large": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32, C.c_int32,
                                              dp, C.POINTER(TreeInfo)]),
    "miosqp_qp_solve_trees_large_rf": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.POINTER(TreeInfo),
                                                 C.POINTER(TreeRfInfo)]),
    "miosqp_qp_solve_trees_large_sb": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32,
                                                 C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, dp,
                                                 C.POINTER(TreeInfo), C.POINTER(TreeSbInfo)]),
    "miosqp_qp_polish_models": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), dpp, dpp, dpp, dpp, dpp, C.c_double, dp, ip, ip, dpp,
                                          dpp, C.POINTER(C.c_void_p), C.POINTER(PolishRepairInfo), C.POINTER(PolishModelsStats)]),
    "miosqp_qp_polish_models_fits": (C.c_int, [C.c_void_p]),
    "miosqp_qp_polish_models_large": (C.c_int, [C.c_int32, C.POINTER(C.c_void_p), dpp, dpp, dpp, dpp, dpp, C.c_double, dp, ip, ip,
                                                dpp, dpp, C.POINTER(C.c_void_p), C.POINTER(PolishRepairInfo),
                                                C.POINTER(PolishModelsLargeStats)]),
    "miosqp_qp_polish_models_large_fits": (C.c_int, [C.c_void_p]),
    "miosqp_qp_setup_models": (C.c_int, [C.c_int32, C.POINTER(SetupModel), C.POINTER(C.c_void_p), C.POINTER(SetupModelsStats)]),
    "miosqp_qp_setup_models_auto": (C.c_int, [C.c_int32, C.POINTER(SetupModel), C.POINTER(C.c_void_p), C.POINTER(SetupModelsStats)]),
    "miosqp_qp_setup_models_large": (C.c_int, [C.c_int32, C.POINTER(SetupModel), C.POINTER(C.c_void_p), C.POINTER(SetupModelsStats),
                                               C.c_int32]),
    "miosqp_qp_setup_models_eligible_large": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Settings)]),
    "miosqp_qp_setup_models_large_auto": (C.c_int, [C.c_int32, C.POINTER(SetupModel), C.POINTER(C.c_void_p),
                                                    C.POINTER(SetupModelsStats), C.c_int32]),
    "miosqp_qp_setup_models_eligible_large_auto": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Settings)]),
    "miosqp_qp_setup_models_shape": (C.c_int, [C.c_int32, C.c_int32]),
    "miosqp_qp_setup_models_prepared": (C.c_int, [C.c_int32, C.POINTER(SetupModel), C.POINTER(C.c_void_p), C.POINTER(SetupModelsStats),
                                                  C.c_int32]),
    "miosqp_qp_debug_panel": (C.c_int, [C.c_void_p, C.c_int32, dp, C.c_int64, C.POINTER(C.c_int64)]),
    "miosqp_qp_setup_models_eligible": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(Settings)]),
    "miosqp_qp_setup_groups_live": (C.c_int, []),
    "miosqp_qp_setup_group": (C.c_int64, [C.c_void_p]),
    "miosqp_qp_debug_product_form": (C.c_int, [C.c_void_p, C.c_int32, dp, C.c_int64, ip, ip]),
    "miosqp_qp_solve_trees_lockstep": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32,
                                                 C.c_int32, dp, C.POINTER(TreeInfo), C.POINTER(LockstepStats)]),
    "miosqp_qp_solve_trees_lockstep_rf": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.POINTER(TreeInfo),
                                                    C.POINTER(LockstepStats), C.POINTER(LockstepRfStats)]),
    "miosqp_qp_solve_trees_lockstep_sb": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32,
                                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, dp,
                                                    C.POINTER(TreeInfo), C.POINTER(LockstepStats),
                                                    C.POINTER(LockstepSbStats)]),
    "miosqp_qp_solve_trees_lockstep_ahead": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32,
                                                       C.c_int32, C.c_int32, C.c_int32, dp, C.POINTER(TreeInfo),
                                                       C.POINTER(LockstepStats), C.POINTER(LockstepAheadStats)]),
    "miosqp_qp_solve_trees_refill": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp, C.c_int32, C.c_int32,
                                               C.c_int32, dp, C.POINTER(TreeInfo), C.POINTER(RefillStats)]),
    "miosqp_qp_search_create": (C.c_int, [C.c_void_p, C.c_int32]),
    "miosqp_qp_search_reset": (C.c_int, [C.c_void_p]),
    "miosqp_qp_search_add_leaf": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.c_int32, C.c_double]),
    "miosqp_qp_search_take_leaf": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "miosqp_qp_search_set_incumbent": (C.c_int, [C.c_void_p, C.c_double, dp]),
    "miosqp_qp_search_get_incumbent": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), dp]),
    "miosqp_qp_search_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.POINTER(SearchInfo)]),
    "miosqp_qp_stream_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]),
    "miosqp_qp_stream_begin": (C.c_int, [C.c_void_p]),
    "miosqp_qp_stream_add_leaf": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.c_int32, C.c_double]),
    "miosqp_qp_stream_take_leaf": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "miosqp_qp_stream_set_incumbent": (C.c_int, [C.c_void_p, C.c_double, dp]),
    "miosqp_qp_stream_get_incumbent": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), dp]),
    "miosqp_qp_stream_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.POINTER(StreamInfo)]),
    "miosqp_qp_solve_batch": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp,
                                        C.POINTER(Info)]),
    "miosqp_qp_solve_batch_q": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp, dp, dp, dp,
                                          C.POINTER(Info)]),
    "miosqp_qp_solve_tree": (C.c_int, [C.c_void_p, dp, dp, dp, dp, C.c_double, dp, C.c_int32, C.c_int32, dp,
                                       C.POINTER(TreeInfo)]),
    "miosqp_qp_pool_create": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "miosqp_qp_pool_reset": (C.c_int, [C.c_void_p]),
    "miosqp_qp_pool_write_node": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp]),
    "miosqp_qp_pool_read_node": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp, dp]),
    "miosqp_qp_pool_push": (C.c_int, [C.c_void_p, C.c_int32, ip, ip, ip, dp]),
    "miosqp_qp_pool_set_upper": (C.c_int, [C.c_void_p, C.c_double]),
    "miosqp_qp_pool_launch": (C.c_int, [C.c_void_p, C.c_int32]),
    "miosqp_qp_pool_collect": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(PoolDigest), C.c_int32, C.POINTER(C.c_int32),
                                         C.POINTER(C.c_int32), i64p]),
    "miosqp_qp_cleanup": (C.c_int, [C.c_void_p]),
    "miosqp_qp_last_error": (C.c_char_p, []),
    "miosqp_qp_debug_iterate": (C.c_int, [C.c_void_p, C.c_int32, dp, dp, dp]),
    "miosqp_qp_debug_factor": (C.c_int, [C.c_void_p, C.c_int32, dp, C.c_int64, ip, ip]),
    "miosqp_qp_get_scaling": (C.c_int, [C.c_void_p, dp, dp, dp]),
    "miosqp_qp_get_factor_stats": (C.c_int, [C.c_void_p, i64p]),
    "miosqp_qp_get_inverse_guard": (C.c_int, [C.c_void_p, dp]),
    "miosqp_qp_get_rho": (C.c_int, [C.c_void_p, dp]),
    "miosqp_qp_get_loop_stats": (C.c_int, [C.c_void_p, dp, i64p, C.c_int32]),
    "miosqp_qp_get_node_stats": (C.c_int, [C.c_void_p, dp, ip]),
    "miosqp_qp_get_loop_launches": (C.c_int, [C.c_void_p, i64p]),
    "miosqp_qp_get_batch_stats": (C.c_int, [C.c_void_p, dp, i64p, i64p, C.c_int32]),
    "miosqp_qp_debug_counter": (C.c_int64, [C.c_void_p, C.c_int32]),
    "miosqp_qp_debug_timeline": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_uint64), C.c_int32,
                                           C.POINTER(C.c_int32)]),
    "miosqp_qp_debug_clock": (C.c_int, [C.c_void_p, dp, dp]),
    "miosqp_qp_time_kernel": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, dp, dp]),
}

_LIB = None


def load():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C miosqp_amd/csrc` (there is no CPU fallback)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)  # AttributeError if the ABI is incomplete
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def last_error():
    msg = load().miosqp_qp_last_error()
    return msg.decode() if msg else ""


def as_d(a):
    return a.ctypes.data_as(dp)


def as_i(a):
    return a.ctypes.data_as(ip)


def source_digest():
    """16 hex digits identifying the device code (csrc/*.hip, *.inc, *.cpp, *.hpp): written into the PMC summaries under
    profiles/ by tools/pmc_merge.py and compared by bench.py, so that counter traffic of other code is not mixed with
    today's timing."""
    import glob
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(_PKG, "csrc")
    for f in sorted(glob.glob(os.path.join(src, "*"))):
        if f.endswith((".hip", ".inc", ".cpp", ".hpp")):
            h.update(os.path.basename(f).encode())
            h.update(open(f, "rb").read())
    return h.hexdigest()[:16]
