"""ctypes binding of csrc/libquasar_slam.so (C ABI: include/quasar_slam.h).

There is no CPU fallback: if the HIP library is missing or no GPU is present the product
path raises.  `build()` compiles the library in-tree with hipcc for gfx950.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("QUASAR_SLAM_LIB") or os.path.join(CSRC, "libquasar_slam.so")   # env: A/B builds of the same ABI
HEADER = os.path.join(os.path.dirname(_HERE), "include", "quasar_slam.h")

QS_CNT_NAMES = ("datagrams", "accepted", "rays", "cells", "hits", "closures", "landmarks", "rebases",
                "slam_windows", "slam_rounds", "slam_node_iters", "slam_misc_iters", "slam_cycles",
                "slam_realtime_100mhz", "slam_cyc_prepare", "slam_cyc_query", "slam_cyc_commit", "ekf_wrap_clamp", "edge_rays", "edge_overflow")
QS_FT_MAX_BOTS = 1024       # bots per qs_frontier_targets call (include/quasar_slam.h)
QS_STAGE_NAMES = ("decode", "slam", "raycast", "ekf", "slam_chain", "rc_rays", "rc_sort", "rc_raster")
UINT64_MAX = (1 << 64) - 1
QS_PLAN_STATUS = ("ok", "no_start", "no_goal", "unreachable")    # QS_PLAN_OK .. QS_PLAN_UNREACHABLE (include/quasar_slam.h)


class QsPlanParams(C.Structure):
    """struct qs_plan_params (include/quasar_slam.h)."""
    _fields_ = [("clearance", C.c_int32), ("snap_radius", C.c_int32), ("lookahead", C.c_int32), ("reserved", C.c_int32)]


class QsGainParams(C.Structure):
    """struct qs_gain_params (include/quasar_slam.h)."""
    _fields_ = [("range", C.c_int32), ("bias", C.c_uint32), ("reserved", C.c_int32 * 2)]


QS_GAIN_MAX_RANGE, QS_GAIN_DEFAULT_RANGE, QS_GAIN_DEFAULT_BIAS = 64, 24, 120     # include/quasar_slam.h, "frontier gain"


class QsSenseParams(C.Structure):
    """struct qs_sense_params (include/quasar_slam.h)."""
    _fields_ = [("max_range", C.c_double), ("noise_amp", C.c_double), ("no_return", C.c_float), ("dropout_q16", C.c_uint32),
                ("seed", C.c_uint64), ("first_record", C.c_uint64), ("reserved", C.c_int32 * 2)]


QS_SENSE_MAX_CELLS = 255                                                         # include/quasar_slam.h, "sensing a world"


class QsCheckParams(C.Structure):
    """struct qs_check_params (include/quasar_slam.h)."""
    _fields_ = [("tol", C.c_double), ("min_checked", C.c_int32), ("max_bad_percent", C.c_int32), ("count_missed", C.c_int32),
                ("reserved", C.c_int32)]


class QsSweepCheck(C.Structure):
    """struct qs_sweep_check (include/quasar_slam.h)."""
    _fields_ = [("agree", C.c_int32), ("nearer", C.c_int32), ("farther", C.c_int32), ("missed", C.c_int32), ("unseen", C.c_int32),
                ("checked", C.c_int32), ("bad", C.c_int32), ("status", C.c_int32), ("accepted_record", C.c_uint8),
                ("pad", C.c_uint8 * 7), ("sin_yaw", C.c_double), ("cos_yaw", C.c_double)]


# include/quasar_slam.h, "sweep check"
QS_BEAM_AGREE, QS_BEAM_NEARER, QS_BEAM_FARTHER, QS_BEAM_MISSED, QS_BEAM_UNSEEN, QS_BEAM_NO_RECORD = 0, 1, 2, 3, 4, 255
QS_CHECK_OK, QS_CHECK_NO_RECORD, QS_CHECK_UNDECIDED, QS_CHECK_CONTRADICTS = 0, 1, 2, 3


class QsMatchParams(C.Structure):
    """struct qs_match_params (include/quasar_slam.h)."""
    _fields_ = [("radius", C.c_int32), ("window", C.c_int32), ("angle_steps", C.c_int32), ("min_hits", C.c_int32),
                ("min_percent", C.c_int32), ("reserved", C.c_int32), ("angle_step", C.c_double)]


class QsSweepGraphParams(C.Structure):
    """struct qs_sweep_graph_params (include/quasar_slam.h)."""
    _fields_ = [("half_width", C.c_int32), ("reserved", C.c_int32), ("close", C.c_double), ("open", C.c_double)]


class QsSweepMatch(C.Structure):
    """struct qs_sweep_match (include/quasar_slam.h)."""
    _fields_ = [("ix", C.c_int32), ("iy", C.c_int32), ("it", C.c_int32), ("score", C.c_int32), ("score0", C.c_int32),
                ("hits", C.c_int32), ("accepted_record", C.c_uint8), ("accepted_match", C.c_uint8), ("pad", C.c_uint8 * 6),
                ("dx", C.c_double), ("dy", C.c_double), ("dyaw", C.c_double)]


class QsRelocParams(C.Structure):
    """struct qs_reloc_params (include/quasar_slam.h)."""
    _fields_ = [("radius", C.c_int32), ("n_rot", C.c_int32), ("sep", C.c_int32), ("sep_rot", C.c_int32), ("min_hits", C.c_int32),
                ("min_percent", C.c_int32), ("min_margin", C.c_int32), ("use_box", C.c_int32),
                ("x0", C.c_int32), ("y0", C.c_int32), ("x1", C.c_int32), ("y1", C.c_int32)]


class QsSweepReloc(C.Structure):
    """struct qs_sweep_reloc (include/quasar_slam.h)."""
    _fields_ = [("gx", C.c_int32), ("gy", C.c_int32), ("j", C.c_int32), ("score", C.c_int32), ("hits", C.c_int32),
                ("gx2", C.c_int32), ("gy2", C.c_int32), ("j2", C.c_int32), ("score2", C.c_int32), ("status", C.c_int32),
                ("accepted_record", C.c_uint8), ("accepted", C.c_uint8), ("pad", C.c_uint8 * 6),
                ("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double)]


class QsRelocRel(C.Structure):
    """struct qs_reloc_rel (include/quasar_slam.h)."""
    _fields_ = [("tx", C.c_double), ("ty", C.c_double), ("s", C.c_double), ("c", C.c_double)]


class QsGroupReloc(C.Structure):
    """struct qs_group_reloc (include/quasar_slam.h)."""
    _fields_ = [("gx", C.c_int32), ("gy", C.c_int32), ("j", C.c_int32), ("score", C.c_int32), ("hits", C.c_int32),
                ("gx2", C.c_int32), ("gy2", C.c_int32), ("j2", C.c_int32), ("score2", C.c_int32), ("status", C.c_int32),
                ("records", C.c_uint8), ("accepted", C.c_uint8), ("pad", C.c_uint8 * 6),
                ("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double)]


class QsTrailMatch(C.Structure):
    """struct qs_trail_match (include/quasar_slam.h)."""
    _fields_ = [("ix", C.c_int32), ("iy", C.c_int32), ("it", C.c_int32), ("score", C.c_int32), ("score0", C.c_int32),
                ("hits", C.c_int32), ("records", C.c_int32), ("anchor", C.c_int32), ("agent", C.c_uint8),
                ("accepted_match", C.c_uint8), ("pad", C.c_uint8 * 6),
                ("ax", C.c_double), ("ay", C.c_double), ("dx", C.c_double), ("dy", C.c_double), ("dyaw", C.c_double)]


class QsTrailReloc(C.Structure):
    """struct qs_trail_reloc (include/quasar_slam.h)."""
    _fields_ = [("gx", C.c_int32), ("gy", C.c_int32), ("j", C.c_int32), ("score", C.c_int32), ("hits", C.c_int32),
                ("gx2", C.c_int32), ("gy2", C.c_int32), ("j2", C.c_int32), ("score2", C.c_int32), ("status", C.c_int32),
                ("records", C.c_uint8), ("accepted", C.c_uint8), ("agent", C.c_uint8), ("pad", C.c_uint8), ("anchor", C.c_int32),
                ("x", C.c_double), ("y", C.c_double), ("yaw", C.c_double), ("ax", C.c_double), ("ay", C.c_double)]


QS_TRAIL_MAX_RECORDS = 64                                                     # include/quasar_slam.h, "trail matching"


class QsMergeResult(C.Structure):
    """struct qs_merge_result (include/quasar_slam.h)."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("n_local", C.c_uint64), ("n_global", C.c_uint64),
                ("fitness", C.c_double), ("rmse", C.c_double), ("T", C.c_double * 9)]


class QsViewParams(C.Structure):
    """struct qs_view_params (include/quasar_slam.h)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("scale", C.c_double), ("offset_x", C.c_double),
                ("offset_y", C.c_double), ("line_min", C.c_int32), ("line_max", C.c_int32), ("bg", C.c_uint8 * 4),
                ("line", C.c_uint8 * 4), ("free", C.c_uint8 * 4), ("occ", C.c_uint8 * 4), ("draw_occupied", C.c_int32),
                ("minify", C.c_int32), ("reserved", C.c_int32 * 2)]


QS_MERGE_STATUS = ("empty", "adopted", "merged", "rejected")     # QS_MERGE_EMPTY .. QS_MERGE_REJECTED (include/quasar_slam.h)


class QsConfig(C.Structure):
    """struct qs_config (include/quasar_slam.h)."""
    _fields_ = [
        ("size", C.c_int32),
        ("res", C.c_double), ("ox", C.c_double), ("oy", C.c_double),
        ("separation", C.c_double),
        ("min_dist", C.c_double), ("max_dist", C.c_double),
        ("closure_radius", C.c_double),
        ("min_poses_between", C.c_int32),
        ("closure_correction", C.c_double),
        ("max_agent", C.c_int32),
        ("bots_per_graph", C.c_int32),
        ("enable_counts", C.c_int32),
        ("enable_ekf", C.c_int32),
        ("ekf_metres_per_tick", C.c_double),
        ("device", C.c_int32),
        ("raycast_mode", C.c_int32),
        ("seq_stride", C.c_int32),
        ("shard_bots", C.c_int32),
        ("shard_rank", C.c_int32),
        ("exact_trig", C.c_int32),
        ("reserved", C.c_int32 * 3),
    ]


class QuasarError(RuntimeError):
    pass


def build(force=False, quiet=True):
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j4"] + (["-B"] if force else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        raise QuasarError("building libquasar_slam.so failed:\n" + res.stdout[-4000:])
    if not quiet:
        print(res.stdout)
    return LIB_PATH


_lib = None

_vp, _i32, _i64, _u64, _f64, _f32, _sz = (C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double,
                                          C.c_float, C.c_size_t)

# name -> (restype, argtypes); every function include/quasar_slam.h declares
SIGNATURES = {
    "qs_version": (C.c_char_p, []),
    "qs_config_default": (_i32, [C.POINTER(QsConfig)]),
    "qs_create": (_i32, [C.POINTER(QsConfig), C.POINTER(_vp)]),
    "qs_destroy": (_i32, [_vp]),
    "qs_last_error": (C.c_char_p, [_vp]),
    "qs_set_stream": (_i32, [_vp, _vp]),
    "qs_sync": (_i32, [_vp]),
    "qs_reset": (_i32, [_vp]),
    "qs_set_bot_offset": (_i32, [_vp, _i32, _f64]),
    "qs_ingest": (_i32, [_vp, _vp, _sz, _sz, _vp, _vp, _u64]),
    "qs_ingest_device": (_i32, [_vp, _vp, _sz, _sz, _vp, _vp, _u64]),
    "qs_last_batch": (_i32, [_vp, _vp, _vp, _sz]),
    "qs_ingest_sweeps": (_i32, [_vp, _vp, _sz, _sz, _vp, _u64]),
    "qs_ingest_sweeps_device": (_i32, [_vp, _vp, _sz, _sz, _vp, _u64]),
    "qs_last_sweeps": (_i32, [_vp, _vp, _vp, _sz]),
    "qs_set_sweep_filter": (_i32, [_vp, _f64, _f64]),
    "qs_set_sweep_graph": (_i32, [_vp, _i32, _vp]),
    "qs_sweep_graph": (_i32, [_vp, C.POINTER(_i32), C.POINTER(QsSweepGraphParams)]),
    "qs_sweep_signatures": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "qs_sweep_signatures_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "qs_last_sweep_nodes": (_i32, [_vp, _vp, _vp, _sz]),
    "qs_match_field": (_i32, [_vp, _i32, _vp]),
    "qs_match_sweeps": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "qs_match_sweeps_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "qs_ingest_sweeps_matched": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _u64]),
    "qs_ingest_sweeps_matched_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _u64]),
    "qs_last_sweep_matches": (_i32, [_vp, _vp, _sz]),
    "qs_relocalise_sweeps": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "qs_relocalise_sweeps_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp]),
    "qs_relocalise_groups": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz, C.c_double, _vp]),
    "qs_relocalise_groups_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp, _sz, C.c_double, _vp]),
    "qs_match_trails": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, C.c_double, _vp, _vp]),
    "qs_match_trails_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, C.c_double, _vp, _vp]),
    "qs_relocalise_trails": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, C.c_double, _vp, _vp]),
    "qs_relocalise_trails_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _sz, C.c_double, _vp, _vp]),
    "qs_sense_ranges": (_i32, [_vp, _vp, _sz, _i32, _vp, _vp, _vp]),
    "qs_sense_ranges_device": (_i32, [_vp, _vp, _sz, _i32, _vp, _vp, _vp]),
    "qs_sense_sweeps": (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz]),
    "qs_sense_sweeps_device": (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp, _sz]),
    "qs_sense_packets": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "qs_sense_packets_device": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "qs_check_sweeps": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "qs_check_sweeps_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _vp, _vp]),
    "qs_ingest_sweeps_checked": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _u64]),
    "qs_ingest_sweeps_checked_device": (_i32, [_vp, _vp, _vp, _sz, _sz, _vp, _u64]),
    "qs_last_sweep_checks": (_i32, [_vp, _vp, _sz]),
    "qs_last_hits": (_i32, [_vp, _vp, _vp, _sz]),
    "qs_set_bot_veil": (_i32, [_vp, _i32]),
    "qs_bot_veil": (_i32, [_vp, C.POINTER(_i32)]),
    "qs_bot_veil_place": (_i32, [_vp, _i32, _f64, _f64]),
    "qs_bot_veil_forget": (_i32, [_vp, _i32]),
    "qs_bot_veil_cells": (_i32, [_vp, _vp, _vp]),
    "qs_last_veiled": (_i32, [_vp, _vp, _sz]),
    "qs_bot_veil_stats": (_i32, [_vp, C.POINTER(_u64)]),
    "qs_bot_veil_time": (_i32, [_vp, C.POINTER(_f64), C.POINTER(_u64), _i32]),
    "qs_set_bot_veil_sweeps": (_i32, [_vp, _i32]),
    "qs_bot_veil_sweeps": (_i32, [_vp, C.POINTER(_i32)]),
    "qs_last_sweeps_veiled": (_i32, [_vp, _vp, _sz]),
    "qs_update_rays": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _u64]),
    "qs_world_to_grid": (_i32, [_vp, _vp, _sz, _i32, _vp]),
    "qs_grid_i8": (_i32, [_vp, _vp]),
    "qs_grid_i8_device": (_i32, [_vp, _vp]),
    "qs_grid_counts": (_i32, [_vp, _vp, _vp]),
    "qs_grid_logodds": (_i32, [_vp, _f32, _f32, _f32, _f32, _vp]),
    "qs_device_buffers": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_sz), C.POINTER(_vp), C.POINTER(_sz)]),
    "qs_slam_sizes": (_i32, [_vp, _i32, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]),
    "qs_slam_closures": (_i32, [_vp, _i32, _vp, _vp, _sz]),
    "qs_slam_closure_agents": (_i32, [_vp, _i32, _vp, _sz]),
    "qs_slam_landmarks": (_i32, [_vp, _i32, _vp, _vp, _sz]),
    "qs_slam_add_poses": (_i32, [_vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "qs_drift": (_i32, [_vp, _i32, _vp]),
    "qs_zone": (_i32, [_vp, _i32, _vp, C.POINTER(_i32)]),
    "qs_zone_packet": (_i32, [_vp, _i32, _i32, _vp]),
    "qs_fuse": (_i32, [_vp, C.POINTER(_vp), _sz]),
    "qs_fuse_buffers": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_vp), _sz]),
    "qs_fuse_buffers_range": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_vp), _sz, _sz, _sz, _i32]),
    "qs_fused_counts": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    "qs_counts_source": (_i32, [_vp, _i32]),
    "qs_epoch_query": (_i32, [_vp, _u64, _sz, C.POINTER(_i32)]),
    "qs_mark_fused": (_i32, [_vp]),
    "qs_dirty_tracking": (_i32, [_vp, _i32]),
    "qs_dirty_blocks": (_i32, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "qs_sparse_fuse_begin": (_i32, [_vp, _i32, _i32, C.POINTER(_vp), C.POINTER(_sz)]),
    "qs_sparse_fuse_plan": (_i32, [_vp, _vp, _vp, C.POINTER(_vp), C.POINTER(_sz)]),
    "qs_sparse_fuse_apply": (_i32, [_vp]),
    "qs_fused_counts_buffer": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_sz)]),
    "qs_rccl_unique_id": (_i32, [_vp]),
    "qs_rccl_comm_init": (_i32, [_vp, _vp, _i32, _i32, C.POINTER(_vp)]),
    "qs_rccl_comm_destroy": (_i32, [_vp]),
    "qs_sparse_fuse_rccl": (_i32, [_vp, _vp, _i32, _i32, _vp]),
    "qs_grid_to_pcd": (_i32, [_vp, _vp, _i32, _i32, _f64, _f64, _f64, _vp, _sz, C.POINTER(_sz)]),
    "qs_rasterise": (_i32, [_vp, _vp, _sz, _f64, _vp, _vp, _vp]),
    "qs_icp": (_i32, [_vp, _vp, _sz, _vp, _sz, _f64, _i32, _f64, _f64, _vp, _vp, _vp, _vp]),
    "qs_nn_search": (_i32, [_vp, _vp, _sz, _vp, _sz, _f64, _i32, _vp, _vp, _vp]),
    "qs_diag_mfma_f64_rate": (_i32, [_vp, C.POINTER(_f64)]),
    "qs_diag_latencies": (_i32, [_vp, _vp]),
    "qs_set_chain_form": (_i32, [_vp, _i32]),
    "qs_chain_form": (_i32, [_vp]),
    "qs_set_chain_lean": (_i32, [_vp, _i32, _i64]),
    "qs_chain_lean": (_i32, [_vp]),
    "qs_set_chain_lookahead": (_i32, [_vp, _i32]),
    "qs_chain_lookahead": (_i32, [_vp]),
    "qs_set_chain_plan": (_i32, [_vp, _i32]),
    "qs_chain_plan": (_i32, [_vp]),
    "qs_set_chain_scout": (_i32, [_vp, _i32]),
    "qs_chain_scout": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "qs_chain_plan_read": (_i32, [_vp, _i32, _vp, _vp, _vp, _sz, C.POINTER(_sz), C.POINTER(C.c_uint32)]),
    "qs_voxel_downsample": (_i32, [_vp, _vp, _sz, _f64, _vp, _sz, C.POINTER(_sz)]),
    "qs_voxel_downsample_device": (_i32, [_vp, _vp, _sz, _f64, _vp, _sz, C.POINTER(_sz)]),
    "qs_merge_reset": (_i32, [_vp]),
    "qs_merge_params": (_i32, [_vp, _f64, _i32, _f64]),
    "qs_merge_grid": (_i32, [_vp, _vp, _i32, _i32, _f64, _f64, _f64, _vp]),
    "qs_merge_grid_device": (_i32, [_vp, _vp, _i32, _i32, _f64, _f64, _f64, _vp]),
    "qs_merge_map": (_i32, [_vp, _vp, _vp]),
    "qs_merge_cloud": (_i32, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "qs_merge_global_map": (_i32, [_vp, _vp, _vp, _vp]),
    "qs_frontier_cells": (_i32, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "qs_frontier_members": (_i32, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "qs_frontier_clusters": (_i32, [_vp, _i32, _vp, _sz, C.POINTER(_sz)]),
    "qs_frontier_targets": (_i32, [_vp, _i32, _f64, _vp, _sz, _vp, _vp, _vp, _sz, C.POINTER(_sz), _vp]),
    "qs_traversable": (_i32, [_vp, _i32, _vp]),
    "qs_plan_field": (_i32, [_vp, _vp, _vp, _vp]),
    "qs_plan_paths": (_i32, [_vp, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _vp]),
    "qs_frontier_targets_by_path": (_i32, [_vp, _i32, _f64, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                           C.POINTER(_sz), _vp]),
    "qs_frontier_gain": (_i32, [_vp, _i32, _i32, _vp, _vp, _sz, C.POINTER(_sz)]),
    "qs_frontier_targets_by_gain": (_i32, [_vp, _i32, _f64, _vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                           C.POINTER(_sz), _vp, _vp]),
    "qs_territories": (_i32, [_vp, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp]),
    "qs_frontier_targets_by_territory": (_i32, [_vp, _i32, _vp, _vp, _sz, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                                C.POINTER(_sz), _vp]),
    "qs_render_view": (_i32, [_vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "qs_render_view_device": (_i32, [_vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "qs_ekf_init": (_i32, [_vp, _i32, _f64, _vp]),
    "qs_ekf_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _sz, _i32]),
    "qs_ekf_state": (_i32, [_vp, _i32, _vp, _vp]),
    "qs_counters": (_i32, [_vp, _vp]),
    "qs_checkpoint": (_i32, [_vp, _vp, _sz, C.POINTER(_sz)]),
    "qs_restore": (_i32, [_vp, _vp, _sz]),
    "qs_timing_enable": (_i32, [_vp, _i32]),
    "qs_stage_times": (_i32, [_vp, _vp, _vp, _i32]),
}


def load():
    """dlopen the HIP library and declare every entry point.  Raises if it is absent.
    A process that also uses torch must import torch BEFORE the first call of this function: the torch wheel bundles its
    own HIP runtime, and once the system's (which this library links) has initialised the GPU, torch's reports
    "No HIP GPUs are available".  dist.py and bench.py import torch first; a host that only maps never needs it."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise QuasarError(
            f"{LIB_PATH} not found: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950). "
            "There is no CPU fallback for the mapper path.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)            # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(ctx, rc, what):
    if rc != 0:
        msg = load().qs_last_error(ctx)
        raise QuasarError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
