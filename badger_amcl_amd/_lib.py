"""ctypes binding of include/badger_pf.h.  Loading fails loudly when the HIP library is
missing; nothing here computes on the CPU."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SO = os.environ.get("BPF_LIB") or os.path.join(HERE, "libbadger_pf_hip.so")  # BPF_LIB: experiment builds

BPF_K_COUNT = 9


class PFState(C.Structure):
    _fields_ = [("sample_count", C.c_int), ("leaf_count", C.c_int), ("bin_count", C.c_int),
                ("converged", C.c_int), ("percent_converged", C.c_float),
                ("total", C.c_double), ("w_slow", C.c_double), ("w_fast", C.c_double), ("w_diff", C.c_double),
                ("last_status", C.c_int), ("resample_windows", C.c_int), ("evals", C.c_longlong),
                ("kld_on_device", C.c_int), ("reserved", C.c_int)]


class Cluster(C.Structure):
    _fields_ = [("count", C.c_int), ("weight", C.c_double), ("mean", C.c_double * 3), ("cov", C.c_double * 5)]


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * BPF_K_COUNT), ("launches", C.c_longlong * BPF_K_COUNT)]


class PoseHit(C.Structure):
    _fields_ = [("pose", C.c_double * 3), ("score", C.c_double), ("candidate", C.c_longlong), ("i", C.c_int),
                ("j", C.c_int), ("heading", C.c_int), ("reserved", C.c_int)]


class PoseSearchStats(C.Structure):
    _fields_ = [(name, C.c_longlong) for name in (
        "candidates", "block_candidates", "seed_candidates", "pruned_block_candidates", "expanded_block_candidates",
        "scored_candidates", "windows")]


assert C.sizeof(PoseSearchStats) == 56  # bpf_pose_search_stats
POSE_SEARCH_BLOCKS = (2, 4, 8, 16, 32, 64)  # the block sizes bpf_planar_search_poses_pruned takes


class PoseRefined(C.Structure):
    _fields_ = [("pose", C.c_double * 3), ("score", C.c_double), ("score_in", C.c_double), ("moved", C.c_int),
                ("reserved", C.c_int)]


assert C.sizeof(PoseRefined) == 48  # bpf_pose_refined


class PoseMoments(C.Structure):
    _fields_ = [("mean", C.c_double * 3), ("cov", C.c_double * 6), ("weight_sum", C.c_double),
                ("score_max", C.c_double), ("support", C.c_int), ("flags", C.c_int)]


assert C.sizeof(PoseMoments) == 96  # bpf_pose_moments
# the same layout for numpy (cov: xx, xy, xt, yy, yt, tt)
POSE_MOMENTS_DTYPE = np.dtype([("mean", "<f8", (3,)), ("cov", "<f8", (6,)), ("weight_sum", "<f8"),
                               ("score_max", "<f8"), ("support", "<i4"), ("flags", "<i4")])
assert POSE_MOMENTS_DTYPE.itemsize == 96


class MixtureComponent(C.Structure):
    _fields_ = [("mean", C.c_double * 3), ("rotation", C.c_double * 9), ("sigma", C.c_double * 3),
                ("count", C.c_int), ("reserved", C.c_int)]


assert C.sizeof(MixtureComponent) == 128  # bpf_mixture_component
# the same layout for numpy: an array of it is passed to the library as it is
MIXTURE_COMPONENT_DTYPE = np.dtype([("mean", "<f8", (3,)), ("rotation", "<f8", (3, 3)), ("sigma", "<f8", (3,)),
                                    ("count", "<i4"), ("reserved", "<i4")])
assert MIXTURE_COMPONENT_DTYPE.itemsize == 128

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p

# name -> (restype, argtypes); every symbol include/badger_pf.h declares
SIGNATURES = {
    "bpf_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "bpf_destroy": (None, [_vp]),
    "bpf_error_string": (C.c_char_p, [C.c_int]),
    "bpf_last_error_message": (C.c_char_p, [_vp]),
    "bpf_set_stream": (C.c_int, [_vp, _vp]),
    "bpf_synchronize": (C.c_int, [_vp]),
    "bpf_map2d_set": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_float), C.c_int, C.c_int, C.c_float,
                                C.c_float, C.c_double, C.c_double]),
    "bpf_map2d_build_distances_lut": (C.c_int, [_vp, C.c_double]),
    "bpf_map2d_get_distances_lut": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_size_t]),
    "bpf_map2d_calc_range": (C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, C.c_int, _dp]),
    "bpf_planar_init": (C.c_int, [_vp, C.c_int]),
    "bpf_planar_set_model_beam": (C.c_int, [_vp] + [C.c_double] * 6),
    "bpf_planar_set_model_likelihood_field": (C.c_int, [_vp] + [C.c_double] * 4),
    "bpf_planar_set_model_likelihood_field_prob": (C.c_int, [_vp] + [C.c_double] * 4 + [C.c_int] + [C.c_double] * 3),
    "bpf_planar_set_model_likelihood_field_gompertz": (C.c_int, [_vp] + [C.c_double] * 10),
    "bpf_planar_set_map_factors": (C.c_int, [_vp] + [C.c_double] * 3),
    "bpf_planar_set_scanner_pose": (C.c_int, [_vp, _dp]),
    "bpf_planar_apply_model_to_sample_set": (C.c_double, [_vp, _dp, C.c_int, C.c_int, _dp, _dp, C.c_int, C.c_double,
                                                          _ip]),
    "bpf_pf_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double]),
    "bpf_pf_set_resample_model": (C.c_int, [_vp, C.c_int]),
    "bpf_pf_set_population_size_parameters": (C.c_int, [_vp, C.c_double, C.c_double]),
    "bpf_pf_set_decay_rates": (C.c_int, [_vp, C.c_double, C.c_double]),
    "bpf_pf_srand48": (C.c_int, [_vp, C.c_long]),
    "bpf_pf_set_rng_state": (C.c_int, [_vp, C.c_uint64]),
    "bpf_pf_get_rng_state": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "bpf_pf_set_samples": (C.c_int, [_vp, _dp, C.c_int, C.c_int]),
    "bpf_pf_get_samples": (C.c_int, [_vp, _dp, C.c_int, _ip]),
    "bpf_pf_snapshot": (C.c_int, [_vp]),
    "bpf_pf_restore": (C.c_int, [_vp]),
    "bpf_pf_fill_weights": (C.c_int, [_vp, C.c_double]),
    "bpf_pf_update_sensor_planar": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double]),
    "bpf_pf_set_random_pose_generator": (C.c_int, [_vp, C.c_int]),
    "bpf_pf_set_uniform_pose_check": (C.c_int, [_vp, C.c_double, C.c_double, C.c_int]),
    "bpf_uniform_pose_retries": (C.c_int, [C.c_double, C.c_double]),
    "bpf_pf_set_kld_count": (C.c_int, [_vp, C.c_int]),
    "bpf_pf_get_kld_count": (C.c_int, [_vp, _ip]),
    "bpf_pf_update_resample": (C.c_int, [_vp]),
    "bpf_set_option": (C.c_int, [_vp, C.c_int, C.c_int]),
    "bpf_get_cells_walked": (C.c_int, [_vp, C.POINTER(C.c_ulonglong), C.c_int]),
    "bpf_pf_get_state": (C.c_int, [_vp, C.POINTER(PFState)]),
    "bpf_pf_init_with_gaussian": (C.c_int, [_vp, _dp, _dp, _dp]),
    "bpf_pf_init_with_random_poses": (C.c_int, [_vp]),
    "bpf_pf_init_with_mixture": (C.c_int, [_vp, C.POINTER(MixtureComponent), C.c_int]),
    "bpf_odom_set_model": (C.c_int, [_vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]),
    "bpf_pf_update_action": (C.c_int, [_vp, _dp, _dp, _dp]),
    "bpf_shard_update_action": (C.c_int, [_vp, _dp, _dp, _dp, C.c_longlong, C.c_longlong]),
    "bpf_pf_compute_cluster_stats": (C.c_int, [_vp, _ip, _dp, _dp]),
    "bpf_pf_get_cluster": (C.c_int, [_vp, C.c_int, C.POINTER(Cluster)]),
    "bpf_pf_get_max_weight_pose": (C.c_int, [_vp, _dp, _dp]),
    "bpf_map2d_build_distances_lut_reference": (C.c_int, [_vp, C.c_double]),
    "bpf_host_buffer_register": (C.c_int, [_vp, C.c_void_p, C.c_size_t]),
    "bpf_host_buffer_unregister": (C.c_int, [_vp, C.c_void_p]),
    "bpf_host_buffer_is_registered": (C.c_int, [_vp, C.c_void_p, C.c_size_t]),
    "bpf_seam_last_plan": (C.c_int, [_vp, _ip, _ip]),
    "bpf_kld_last_form": (C.c_int, [_vp, _ip]),
    "bpf_cloud_last_form": (C.c_int, [_vp, _ip]),
    "bpf_score_last_form": (C.c_int, [_vp, _ip]),
    "bpf_wire_laserscan_to_planar": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_float, C.c_float, C.c_double,
                                               C.c_double, C.c_double, C.c_double, _dp, _dp, _dp]),
    "bpf_wire_scan_angle_stats": (C.c_int, [C.c_double, C.c_double, _dp, _dp, _dp]),
    "bpf_wire_occupancy_grid_to_cells": (C.c_int, [C.POINTER(C.c_int8), C.c_int, C.c_int, C.c_double, C.c_double,
                                                   C.c_double, C.c_int, C.POINTER(C.c_int32), _ip, _ip,
                                                   C.POINTER(C.c_float), _dp]),
    "bpf_wire_decimate_cloud": (C.c_int, [C.POINTER(C.c_float), C.c_int, C.c_int, C.POINTER(C.c_float), C.c_int]),
    "bpf_wire_samples_to_pose_array": (C.c_int, [_dp, C.c_int, _dp]),
    "bpf_map3d_set": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t, _ip, _ip,
                                C.c_double, C.c_double]),
    "bpf_map3d_build_distances_lut": (C.c_int, [_vp, _ip, C.c_size_t, _ip, _ip, C.c_double, C.c_double]),
    "bpf_map3d_get_distances_lut": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t),
                                              C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_size_t)]),
    "bpf_cloud_init": (C.c_int, [_vp, C.c_int]),
    "bpf_cloud_set_model": (C.c_int, [_vp] + [C.c_double] * 3),
    "bpf_cloud_set_model_gompertz": (C.c_int, [_vp] + [C.c_double] * 9),
    "bpf_cloud_set_map_factors": (C.c_int, [_vp] + [C.c_double] * 3),
    "bpf_cloud_set_scanner_to_footprint_tf": (C.c_int, [_vp, _dp, _dp]),
    "bpf_cloud_apply_model_to_sample_set": (C.c_double, [_vp, _dp, C.c_int, C.POINTER(C.c_float), C.c_int, _ip]),
    "bpf_pf_update_sensor_cloud": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int]),
    "bpf_shard_score_planar": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double]),
    "bpf_shard_beam_counts_dev": (C.c_int, [_vp, C.POINTER(_vp), _ip]),
    "bpf_shard_score_planar_finish": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.c_longlong]),
    "bpf_shard_score_cloud": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int]),
    "bpf_shard_scalars_dev": (C.c_int, [_vp, C.POINTER(_vp)]),
    "bpf_shard_normalize_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "bpf_shard_build_cdf": (C.c_int, [_vp, _vp]),
    "bpf_shard_draw_window_dev": (C.c_int, [_vp, C.c_uint64, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp,
                                            C.c_int, _vp]),
    "bpf_shard_tail_small_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bpf_shard_adopt_dev": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]),
    "bpf_shard_converged_dev": (C.c_int, [_vp, _vp, _vp, C.c_int]),
    "bpf_shard_samples_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _ip]),
    "bpf_shard_stats_gathered_dev": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _ip]),
    "bpf_shard_stats_local_bins_dev": (C.c_int, [_vp, C.c_longlong, C.POINTER(_vp), _ip, _ip]),
    "bpf_shard_stats_label_dev": (C.c_int, [_vp, _vp, _ip, C.c_int, C.c_int, _ip]),
    "bpf_shard_stats_local_sums_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "bpf_shard_stats_finish_dev": (C.c_int, [_vp, _vp]),
    "bpf_shard_stats_finish_installed": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "bpf_shard_stats_host": (C.c_int, [_vp, _dp, C.c_int]),
    "bpf_shard_init_with_gaussian": (C.c_int, [_vp, _dp, _dp, _dp, C.c_longlong, C.c_int, C.c_longlong]),
    "bpf_shard_init_with_random_poses": (C.c_int, [_vp, C.c_longlong, C.c_int, C.c_longlong]),
    "bpf_shard_init_with_mixture": (C.c_int, [_vp, C.POINTER(MixtureComponent), C.c_int, C.c_longlong, C.c_int,
                                              C.c_longlong]),
    "bpf_shard_tree_local_bins_dev": (C.c_int, [_vp, C.c_longlong, C.POINTER(_vp), _ip, _ip]),
    "bpf_shard_tree_merge_dev": (C.c_int, [_vp, _vp, _ip, C.c_int, C.c_int, _ip, _ip]),
    "bpf_shard_tree_local_keys_dev": (C.c_int, [_vp, C.POINTER(_vp), _ip]),
    "bpf_shard_tree_from_keys": (C.c_int, [_vp, _ip, C.c_int, _ip, _ip]),
    "bpf_shard_tree_last_route": (C.c_int, [_vp, _ip]),
    "bpf_shard_init_with_gaussian_all": (C.c_int, [_vp, _dp, _dp, _dp]),
    "bpf_shard_init_with_random_poses_all": (C.c_int, [_vp]),
    "bpf_shard_init_with_mixture_all": (C.c_int, [_vp, C.POINTER(MixtureComponent), C.c_int]),
    "bpf_shard_global_leaf_count": (C.c_int, [_vp, _ip, _ip]),
    "bpf_shard_mailbox_create": (C.c_int, [_vp, C.c_int, C.c_int, C.c_longlong, _vp]),
    "bpf_shard_mailbox_connect": (C.c_int, [_vp, _vp]),
    "bpf_shard_mailbox_selftest": (C.c_int, [_vp, C.c_int]),
    "bpf_map3d_builder_generations": (C.c_int, [_vp, _ip]),
    "bpf_shard_mailbox_set_timeout_ms": (C.c_int, [_vp, C.c_int]),
    "bpf_shard_mailbox_error_stage": (C.c_int, [_vp, _ip, _ip]),
    "bpf_shard_bootstrap": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p, C.c_longlong, C.c_int, _ip]),
    "bpf_shard_shutdown": (C.c_int, [_vp]),
    "bpf_shard_connect_local": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int]),
    "bpf_shard_exchange_mode": (C.c_int, [_vp, _ip]),
    "bpf_shard_local_selftest": (C.c_int, [_vp, C.c_int]),
    "bpf_shard_exchange_probe": (C.c_int, [_vp, C.c_int, C.c_longlong, C.c_int, _dp]),
    "bpf_shard_update_sensor_planar": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.c_longlong]),
    "bpf_shard_update_resample": (C.c_int, [_vp, _ip, _ip, _ip, _ip, _ip, _ip]),
    "bpf_shard_update_sensor_cloud": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, C.c_longlong]),
    "bpf_shard_compute_cluster_stats": (C.c_int, [_vp, _ip, _dp, _dp, _ip]),
    "bpf_shard_get_max_weight_pose": (C.c_int, [_vp, _dp, _dp]),
    "bpf_shard_exchange_count": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bpf_pf_get_pose_array": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, _ip]),
    "bpf_shard_pose_rows_dev": (C.c_int, [_vp, C.c_longlong, C.c_longlong, C.c_int, C.POINTER(_vp), _ip]),
    "bpf_pose_array_from_rows_dev": (C.c_int, [_vp, _vp, C.c_longlong, C.c_int, _dp, C.c_int]),
    "bpf_shard_get_pose_array": (C.c_int, [_vp, C.c_int, C.c_longlong, C.c_int, _dp, C.c_int, _ip]),
    "bpf_shard_mailbox_update_sensor_planar": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.c_longlong]),
    "bpf_shard_mailbox_update_resample": (C.c_int, [_vp, _vp, _ip, _ip, _ip, _ip, _ip]),
    "bpf_shard_mailbox_destroy": (C.c_int, [_vp]),
    "bpf_shard_mailbox_totals": (C.c_int, [_vp, C.POINTER(_vp)]),
    "bpf_shard_mailbox_window": (C.c_int, [_vp, C.POINTER(_vp), _ip]),
    "bpf_drand48_skip": (C.c_uint64, [C.c_uint64, C.c_uint64]),
    "bpf_kld_reset": (C.c_int, [_vp]),
    "bpf_kld_feed": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _ip]),
    "bpf_kld_feed_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int, _ip]),
    "bpf_shard_begin_resample": (C.c_int, [_vp, C.c_uint64, C.c_int, _dp, _ip]),
    "bpf_shard_end_resample": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_uint64)]),
    "bpf_pf_resample_limit": (C.c_int, [_vp, C.c_int, _ip]),
    "bpf_shard_systematic_window_dev": (C.c_int, [_vp, C.c_uint64, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp,
                                                  C.c_int, _vp]),
    "bpf_shard_set_resample_form": (C.c_int, [_vp, C.c_int, C.c_double]),
    "bpf_shard_get_resample_form": (C.c_int, [_vp, _ip, _dp]),
    "bpf_shard_slice": (C.c_int, [_vp, C.POINTER(C.c_longlong), _ip, _ip]),
    "bpf_shard_inplace_select_dev": (C.c_int, [_vp, C.c_uint64, C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp, _ip,
                                               C.POINTER(C.c_longlong), _ip]),
    "bpf_shard_inplace_xy_sums_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "bpf_shard_inplace_converged_dev": (C.c_int, [_vp, _vp, C.c_int, C.POINTER(_vp)]),
    "bpf_shard_inplace_converged_finish": (C.c_int, [_vp, _vp, C.c_int]),
    "bpf_shard_set_multinomial_form": (C.c_int, [_vp, C.c_int]),
    "bpf_shard_get_multinomial_form": (C.c_int, [_vp, _ip]),
    "bpf_shard_inplace_mn_select_dev": (C.c_int, [_vp, C.c_uint64, _vp, C.c_int, C.c_int, C.c_int, _vp, _ip]),
    "bpf_shard_inplace_mn_bins_dev": (C.c_int, [_vp, C.POINTER(_vp), _ip, _ip]),
    "bpf_shard_inplace_mn_stop_dev": (C.c_int, [_vp, _vp, _ip, C.c_int, C.c_int, _ip, _ip, _ip, _ip,
                                                C.POINTER(C.c_longlong), _ip]),
    "bpf_shard_set_rebalance": (C.c_int, [_vp, C.c_int, C.c_double]),
    "bpf_shard_get_rebalance": (C.c_int, [_vp, _ip, _dp]),
    "bpf_shard_rebalance_last": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bpf_shard_resample_committed": (C.c_int, [_vp, _ip]),
    "bpf_shard_rebalance": (C.c_int, [_vp, C.POINTER(C.c_longlong)]),
    "bpf_shard_rebalance_plan": (C.c_int, [_vp, C.POINTER(C.c_longlong), C.c_int, C.c_int, C.POINTER(C.c_longlong),
                                           C.POINTER(C.c_longlong), _ip]),
    "bpf_shard_rebalance_export_dev": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_longlong)]),
    "bpf_shard_rebalance_import_dev": (C.c_int, [_vp, _vp, C.POINTER(C.c_longlong), C.c_longlong]),
    "bpf_kld_insert": (C.c_int, [_vp, _vp, C.c_int, C.c_int, C.c_int]),
    "bpf_kld_insert_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    "bpf_kld_stop_dev": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _ip, _ip, _ip, _ip]),
    "bpf_kld_leaf_count": (C.c_int, [_vp, _ip, _ip]),
    "bpf_planar_search_poses": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_longlong,
                                          C.c_longlong, C.c_int, C.POINTER(PoseHit), _ip]),
    "bpf_planar_search_space": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_longlong), _ip]),
    "bpf_pose_search_merge": (C.c_int, [C.POINTER(PoseHit), _ip, C.c_int, C.c_int, C.POINTER(PoseHit), _ip]),
    "bpf_pose_search_window": (C.c_int, []),
    "bpf_planar_search_poses_pruned": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                                 C.c_int, C.c_int, C.c_int, C.POINTER(PoseHit), _ip,
                                                 C.POINTER(PoseSearchStats)]),
    "bpf_planar_search_blocks": (C.c_int, [_vp, C.c_int, C.c_int, _ip]),
    "bpf_planar_search_pooled_lut": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_ushort), C.c_longlong,
                                               C.POINTER(C.c_longlong), _ip, _ip]),
    "bpf_planar_search_bounds": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                           C.c_longlong, C.c_longlong, _dp]),
    "bpf_cloud_search_poses": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_longlong,
                                         C.c_longlong, C.c_int, C.POINTER(PoseHit), _ip]),
    "bpf_cloud_search_space": (C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_longlong), _ip]),
    "bpf_pose_search_heading_table": (C.c_int, [C.c_int, _dp, _dp]),
    "bpf_planar_search_poses_joint": (C.c_int, [_vp, C.c_int, C.POINTER(_dp), C.POINTER(_dp), _ip, _dp, _dp, C.c_int,
                                                C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.POINTER(PoseHit),
                                                _ip]),
    "bpf_cloud_search_poses_joint": (C.c_int, [_vp, C.c_int, C.POINTER(C.POINTER(C.c_float)), _ip, _dp, C.c_int,
                                               C.c_int, C.c_longlong, C.c_longlong, C.c_int, C.POINTER(PoseHit),
                                               _ip]),
    "bpf_planar_search_joint_poses": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, C.POINTER(C.c_longlong),
                                                C.c_int, _dp]),
    "bpf_cloud_search_joint_poses": (C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int, C.POINTER(C.c_longlong),
                                               C.c_int, _dp]),
    "bpf_cloud_search_poses_pruned": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.POINTER(PoseHit), _ip,
                                                C.POINTER(PoseSearchStats)]),
    "bpf_cloud_search_blocks": (C.c_int, [_vp, C.c_int, C.c_int, _ip]),
    "bpf_cloud_search_pooled_lut": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_ubyte), C.c_longlong,
                                              C.POINTER(C.c_longlong), _ip, _ip, _ip]),
    "bpf_cloud_search_bounds": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_longlong, C.c_longlong, _dp]),
    "bpf_shard_search_poses": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_longlong,
                                         C.c_longlong, C.c_int, C.POINTER(PoseHit), _ip]),
    "bpf_shard_search_poses_pruned": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int,
                                                C.c_int, C.c_int, C.c_int, C.POINTER(PoseHit), _ip,
                                                C.POINTER(PoseSearchStats)]),
    "bpf_shard_cloud_search_poses": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_longlong,
                                               C.c_longlong, C.c_int, C.POINTER(PoseHit), _ip]),
    "bpf_shard_cloud_search_poses_pruned": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, C.c_int, C.c_int, C.c_int,
                                                      C.c_int, C.c_int, C.c_int, C.POINTER(PoseHit), _ip,
                                                      C.POINTER(PoseSearchStats)]),
    "bpf_planar_refine_poses": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, _dp, C.c_int, C.c_int, C.c_double, C.c_int,
                                          C.c_double, C.c_int, C.POINTER(PoseRefined), _ip]),
    "bpf_cloud_refine_poses": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, _dp, C.c_int, C.c_int, C.c_double,
                                         C.c_int, C.c_double, C.c_int, C.POINTER(PoseRefined), _ip]),
    "bpf_pose_refine_lattice": (C.c_int, [C.c_int, C.c_int, _ip, _ip]),
    "bpf_pose_mixture_from_hits": (C.c_int, [_dp, _dp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _dp,
                                             C.POINTER(MixtureComponent), _ip, _ip, _ip]),
    "bpf_planar_pose_moments": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, _dp, C.c_int, C.c_int, C.c_double, C.c_int,
                                          C.c_double, C.c_double, C.POINTER(PoseMoments), _dp]),
    "bpf_cloud_pose_moments": (C.c_int, [_vp, C.POINTER(C.c_float), C.c_int, _dp, C.c_int, C.c_int, C.c_double,
                                         C.c_int, C.c_double, C.c_double, C.POINTER(PoseMoments), _dp]),
    "bpf_pose_mixture_apply_moments": (C.c_int, [C.POINTER(MixtureComponent), C.c_int, _ip, C.POINTER(PoseMoments),
                                                 C.c_int, _dp, _dp, C.c_int]),
    "bpf_device_memory_info": (C.c_int, [C.c_int, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "bpf_profile_enable": (C.c_int, [_vp, C.c_int]),
    "bpf_profile_reset": (C.c_int, [_vp]),
    "bpf_profile_get": (C.c_int, [_vp, C.POINTER(Profile)]),
    "bpf_score_kernel_name": (C.c_char_p, [_vp]),
    "bpf_get_window_plan": (C.c_int, [_vp, _ip, _ip, _ip]),
}

_lib = None


def load():
    """Returns the loaded library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO):
        raise RuntimeError(
            "badger_amcl_amd: %s is missing. Build it with `python -m badger_amcl_amd.build` "
            "(needs hipcc). There is no CPU fallback for the sensor-update/resample path." % SO)
    L = C.CDLL(SO)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError here = header/library mismatch, on purpose
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L
