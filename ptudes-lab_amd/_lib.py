"""ctypes binding of libptudes_mi.so (the C-ABI declared in include/ptudes_mi.h).

The library is the only compute backend: loading fails loudly when it has not been built, and every
handle constructor raises when no HIP device is present.  Nothing here imports torch.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# PTL_LIB_PATH: a diagnostic / experiment build of the same library (csrc/Makefile: make OUT=... PHASES=1 ...), A/B runs on the GPU box
LIB_PATH = os.environ.get("PTL_LIB_PATH") or os.path.join(_HERE, "csrc", "libptudes_mi.so")

PTL_F32, PTL_F64 = 0, 1
c_d_p = C.POINTER(C.c_double)
c_i64_p = C.POINTER(C.c_int64)


ABI_VERSION = 6  # PTL_ABI_VERSION of the include/ptudes_mi.h this binding was written against


class _Cfg(C.Structure):
    """A configuration struct of the header: starts with {struct_size, abi_version}, which the CALLER fills in before the library
    sees the struct (PTL_CFG_INIT) - ptl_*_default_cfg / ptl_*_create refuse a layout that is not theirs instead of overrunning it."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(type(self))
        self.abi_version = ABI_VERSION


class IcpCfg(_Cfg):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("max_range", C.c_double), ("min_range", C.c_double), ("voxel_size", C.c_double),
                ("max_points_per_voxel", C.c_int32), ("initial_threshold", C.c_double),
                ("min_motion_th", C.c_double), ("deskew", C.c_int32), ("max_iterations", C.c_int32),
                ("convergence", C.c_double), ("device_id", C.c_int32), ("scan_cols", C.c_int32),
                ("max_points_per_scan", C.c_int64), ("map_block_capacity", C.c_int64),
                ("map_table_capacity", C.c_int64), ("gn_workgroups", C.c_int32), ("rebuild_every", C.c_int32),
                ("gn_threads", C.c_int32), ("gn_lanes_per_point", C.c_int32), ("map_small_blocks", C.c_int64)]


class IcpStats(C.Structure):
    _fields_ = [("sigma", C.c_double), ("err_dt", C.c_double), ("err_drot", C.c_double),
                ("iterations", C.c_int32), ("n_corr_last", C.c_int32), ("n_in", C.c_int64),
                ("n_valid", C.c_int64), ("n_down", C.c_int64), ("n_src", C.c_int64),
                ("sum_cand", C.c_int64), ("map_voxels", C.c_int64), ("map_points", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class EkfCfg(_Cfg):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("init_grav", C.c_double * 3), ("init_bacc", C.c_double * 3), ("init_bgyr", C.c_double * 3),
                ("device_id", C.c_int32)]


class SeqCfg(_Cfg):
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("icp", IcpCfg), ("ekf", EkfCfg), ("n_scans", C.c_int64), ("points_per_scan", C.c_int64),
                ("n_imu", C.c_int64), ("use_imu_prediction", C.c_int32), ("with_ekf", C.c_int32), ("range_input", C.c_int32),
                ("resident_scans", C.c_int32)]


class PktFormat(_Cfg):
    """ptl_pkt_format: profile = PTL_PKT_* (packets.PROFILES order)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("profile", C.c_int32), ("pixels_per_column", C.c_int32),
                ("columns_per_frame", C.c_int32), ("columns_per_packet", C.c_int32)]


class PktField(_Cfg):
    """ptl_pkt_field (include/ptudes_mi.h): `bytes` at byte `offset` of a pixel, (word & mask) << shift (>> -shift)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("offset", C.c_int32), ("bytes", C.c_int32), ("mask", C.c_uint32),
                ("shift", C.c_int32)]


PKT_FIELDS = ("RANGE", "REFLECTIVITY", "SIGNAL", "NEAR_IR", "RANGE2", "REFLECTIVITY2", "SIGNAL2")  # PTL_PKT_FIELD_* in id order
PKT_MAX_FIELDS = 4


class PktSummary(C.Structure):
    _fields_ = [("frame_id", C.c_uint32), ("valid_columns", C.c_uint32), ("first_valid_id", C.c_uint32), ("last_valid_id", C.c_uint32),
                ("first_valid_ts", C.c_uint64), ("last_valid_ts", C.c_uint64), ("nonzero_ranges", C.c_uint32),
                ("ignored_columns", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class MapScoreCfg(_Cfg):
    """ptl_map_score_cfg (include/ptudes_mi.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("radius", C.c_double), ("min_neighbours", C.c_int32),
                ("sigma_floor", C.c_double)]


class MapScoreResult(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_scored", C.c_int64), ("n_sparse", C.c_int64), ("mean_plane_var", C.c_double),
                ("mean_entropy", C.c_double), ("mean_neighbours", C.c_double), ("radius", C.c_double), ("min_neighbours", C.c_int32),
                ("sigma_floor", C.c_double), ("device_ms", C.c_double)]


class RenderCfg(_Cfg):
    """ptl_render_cfg (include/ptudes_mi.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32), ("point_px", C.c_int32),
                ("max_frames_per_call", C.c_int32), ("z_lo", C.c_double), ("z_hi", C.c_double), ("background_rgba", C.c_uint32),
                ("edl_strength", C.c_double), ("edl_radius_px", C.c_int32)]


class RenderCam(C.Structure):
    """ptl_render_cam: view = the top three rows of the world -> camera matrix (+z forward, +x right, +y down), row-major"""
    _fields_ = [("view", C.c_double * 12), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("near_m", C.c_double), ("far_m", C.c_double)]


class MapCmpCfg(_Cfg):
    """ptl_map_cmp_cfg (include/ptudes_mi.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("max_dist", C.c_double), ("n_thresholds", C.c_int32),
                ("thresholds", C.c_double * 8)]


class MapCmpResult(C.Structure):
    _fields_ = [("n_query", C.c_int64), ("n_invalid", C.c_int64), ("n_matched", C.c_int64), ("n_within", C.c_int64 * 8),
                ("sum_dist", C.c_double), ("sum_dist2", C.c_double), ("max_dist2_seen", C.c_double), ("max_dist", C.c_double),
                ("n_thresholds", C.c_int32), ("thresholds", C.c_double * 8), ("device_ms", C.c_double)]


class CarveCfg(_Cfg):
    """ptl_carve_cfg (include/ptudes_mi.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("radius", C.c_double), ("margin", C.c_double), ("step", C.c_double),
                ("min_range", C.c_double), ("max_range", C.c_double)]


class CarveResult(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_scans", C.c_int64), ("n_scans_skipped", C.c_int64), ("n_rays", C.c_int64),
                ("n_rays_out_of_range", C.c_int64), ("n_no_return", C.c_int64), ("n_voxel_visits", C.c_int64), ("n_points_through", C.c_int64),
                ("n_points_supported", C.c_int64), ("sum_through", C.c_int64), ("sum_support", C.c_int64), ("radius", C.c_double),
                ("margin", C.c_double), ("step", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double), ("device_ms", C.c_double)]


class PaintResult(_Cfg):
    """ptl_paint_result (include/ptudes_mi.h): an output that carries the caller's {struct_size, abi_version} in front"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("n_points", C.c_int64), ("n_points_painted", C.c_int64),
                ("n_scans", C.c_int64), ("n_scans_skipped", C.c_int64), ("n_rays_matched", C.c_int64), ("n_rays_unmatched", C.c_int64),
                ("n_no_return", C.c_int64), ("sum_count", C.c_int64), ("device_ms", C.c_double)]


class GridCfg(_Cfg):
    """ptl_grid_cfg (include/ptudes_mi.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("cell", C.c_double), ("x0", C.c_double), ("y0", C.c_double),
                ("z_lo", C.c_double), ("z_hi", C.c_double), ("margin", C.c_double), ("step", C.c_double), ("min_range", C.c_double),
                ("max_range", C.c_double), ("max_pixels_per_scan", C.c_int64), ("nx", C.c_int32), ("ny", C.c_int32), ("scan_cols", C.c_int32)]


class GridResult(_Cfg):
    """ptl_grid_result (include/ptudes_mi.h): an output that carries the caller's {struct_size, abi_version} in front"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("n_scans", C.c_int64), ("n_scans_skipped", C.c_int64),
                ("n_rays", C.c_int64), ("n_rays_out_of_range", C.c_int64), ("n_no_return", C.c_int64), ("n_runs_voted", C.c_int64),
                ("n_ends_outside", C.c_int64), ("n_cells_free", C.c_int64), ("n_cells_hit", C.c_int64), ("sum_free", C.c_int64),
                ("sum_hit", C.c_int64), ("box_ix0", C.c_int32), ("box_iy0", C.c_int32), ("box_ix1", C.c_int32), ("box_iy1", C.c_int32),
                ("cell", C.c_double), ("x0", C.c_double), ("y0", C.c_double), ("z_lo", C.c_double), ("z_hi", C.c_double), ("margin", C.c_double),
                ("step", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double), ("nx", C.c_int32), ("ny", C.c_int32),
                ("device_ms", C.c_double)]


class CastCfg(_Cfg):
    """ptl_cast_cfg (include/ptudes_mi.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("radius", C.c_double), ("step", C.c_double), ("min_range", C.c_double),
                ("max_range", C.c_double)]


class CastResult(C.Structure):
    _fields_ = [("n_pixels", C.c_int64), ("n_no_return", C.c_int64), ("n_degenerate", C.c_int64), ("n_hit", C.c_int64), ("n_miss", C.c_int64),
                ("n_voxel_visits", C.c_int64), ("skipped", C.c_int32), ("reserved", C.c_int32), ("radius", C.c_double), ("step", C.c_double),
                ("min_range", C.c_double), ("max_range", C.c_double), ("device_ms", C.c_double)]


class PlaceCfg(_Cfg):
    """ptl_place_cfg (include/ptudes_mi.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("min_radius", C.c_double), ("max_radius", C.c_double),
                ("z_min", C.c_double), ("z_step", C.c_double), ("max_points_per_scan", C.c_int64), ("n_ring", C.c_int32), ("n_sector", C.c_int32),
                ("capacity", C.c_int32), ("reserved", C.c_int32)]


class PlaceInfo(C.Structure):
    """ptl_place_info: what became of a sweep's points, and the descriptor's non-zero cells"""
    _fields_ = [("n_points", C.c_int64), ("n_no_return", C.c_int64), ("n_non_finite", C.c_int64), ("n_out_of_radius", C.c_int64),
                ("n_no_sector", C.c_int64), ("n_below", C.c_int64), ("n_used", C.c_int64), ("n_cells", C.c_int64), ("sum_levels", C.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


PLACE_INFO_FIELDS = tuple(k for k, _ in PlaceInfo._fields_)  # the columns of an (n, 9) int64 array of infos


class PlaceResult(C.Structure):
    _fields_ = [("best_query", C.c_int64), ("best_entry", C.c_int64), ("n_compared", C.c_int64), ("best_dist", C.c_uint32),
                ("best_shift", C.c_int32), ("device_ms", C.c_double)]


class PoseSearchCfg(_Cfg):
    """ptl_pose_search_cfg (include/ptudes_mi.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("abi_version", C.c_uint32), ("max_dist", C.c_double), ("n_thresholds", C.c_int32),
                ("thresholds", C.c_double * 4)]


class PoseSearchResult(C.Structure):
    _fields_ = [("n_points", C.c_int64), ("n_invalid_points", C.c_int64), ("n_poses", C.c_int64), ("n_invalid_poses", C.c_int64),
                ("best_pose", C.c_int64 * 4), ("best_hits", C.c_int64 * 4), ("max_dist", C.c_double), ("n_thresholds", C.c_int32),
                ("thresholds", C.c_double * 4), ("device_ms", C.c_double)]


_vp = C.c_void_p
_vpp = C.POINTER(C.c_void_p)
# every exported symbol of include/ptudes_mi.h with its prototype
PROTOTYPES = {
    "ptl_abi_version": (C.c_int, []),
    "ptl_sizeof_cfg": (C.c_int64, [C.c_int]),
    "ptl_last_error": (C.c_char_p, []),
    "ptl_backend": (C.c_int, []),
    "ptl_device_count": (C.c_int, []),
    "ptl_icp_default_cfg": (C.c_int, [C.POINTER(IcpCfg), C.c_double, C.c_double]),
    "ptl_icp_create": (C.c_int, [C.POINTER(IcpCfg), _vpp]),
    "ptl_icp_destroy": (C.c_int, [_vp]),
    "ptl_icp_register_frame": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, c_d_p, C.c_double, c_d_p, c_d_p,
                                         C.POINTER(IcpStats)]),
    "ptl_icp_set_lazy_map_stats": (C.c_int, [_vp, C.c_int32]),
    "ptl_icp_num_poses": (C.c_int, [_vp, c_i64_p]),
    "ptl_icp_get_poses": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p]),
    "ptl_icp_get_prediction": (C.c_int, [_vp, c_d_p]),
    "ptl_icp_map_size": (C.c_int, [_vp, c_i64_p, c_i64_p]),
    "ptl_icp_map_points": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p]),
    "ptl_icp_last_frame_down": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p]),
    "ptl_icp_last_source": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p]),
    "ptl_icp_gn_wg_clocks": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_int32]),
    "ptl_range_stats": (C.c_int, [C.c_int, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_double, c_d_p]),
    "ptl_icp_debug_set_epoch": (C.c_int, [_vp, C.c_uint32]),
    "ptl_icp_debug_sums": (C.c_int, [_vp, c_d_p]),
    "ptl_diag_slots": (C.c_int, []),
    "ptl_diag_slot_name": (C.c_char_p, [C.c_int]),
    "ptl_icp_diag": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_int32]),
    "ptl_icp_debug_stall_workgroup": (C.c_int, [_vp, C.c_int32]),
    "ptl_icp_debug_limit_capacity": (C.c_int, [_vp, C.c_int32, C.c_int64]),
    "ptl_icp_debug_table": (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(C.c_int32), c_d_p, C.c_int64, c_i64_p]),
    "ptl_icp_deskew": (C.c_int, [_vp, c_d_p, c_d_p, C.c_int64, c_d_p]),
    "ptl_icp_map_add": (C.c_int, [_vp, c_d_p, C.c_int64, c_d_p, C.c_int]),
    "ptl_icp_linear_system": (C.c_int, [_vp, c_d_p, C.c_int64, C.c_double, C.c_double, c_d_p, c_i64_p, c_i64_p]),
    "ptl_icp_align": (C.c_int, [_vp, c_d_p, C.c_int64, c_d_p, C.c_double, C.c_double, c_d_p,
                                C.POINTER(C.c_int32)]),
    "ptl_lut_create": (C.c_int, [C.c_int, C.c_int32, C.c_int32, c_d_p, c_d_p, C.c_double, c_d_p, c_d_p, _vpp]),
    "ptl_lut_destroy": (C.c_int, [_vp]),
    "ptl_lut_apply": (C.c_int, [_vp, C.POINTER(C.c_uint32), c_d_p]),
    "ptl_traj_poses_at": (C.c_int, [C.c_int, c_d_p, c_d_p, C.c_int64, C.c_double, C.c_double, c_d_p, C.c_int64, c_d_p, c_i64_p]),
    "ptl_lut_dewarp": (C.c_int, [_vp, C.POINTER(C.c_uint32), c_d_p, c_d_p, c_i64_p]),
    "ptl_icp_set_active_beams": (C.c_int, [_vp, C.c_int32, C.c_int32]),
    "ptl_icp_register_range": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32), C.c_double, c_d_p, c_d_p,
                                         C.POINTER(IcpStats)]),
    "ptl_icp_profile": (C.c_int, [_vp, C.c_int, c_d_p, c_i64_p, C.c_int]),
    "ptl_icp_gn_phases": (C.c_int, [_vp, c_i64_p]),
    "ptl_ekf_default_cfg": (C.c_int, [C.POINTER(EkfCfg)]),
    "ptl_ekf_create": (C.c_int, [C.POINTER(EkfCfg), _vpp]),
    "ptl_ekf_destroy": (C.c_int, [_vp]),
    "ptl_ekf_process_imu": (C.c_int, [_vp, c_d_p, c_d_p, C.c_double]),
    "ptl_ekf_process_imu_batch": (C.c_int, [_vp, c_d_p, C.c_int64]),
    "ptl_ekf_process_pose": (C.c_int, [_vp, c_d_p, c_d_p]),
    "ptl_ekf_get_state": (C.c_int, [_vp, c_d_p, c_d_p]),
    "ptl_ekf_pose_mat": (C.c_int, [_vp, c_d_p]),
    "ptl_ekf_ts": (C.c_int, [_vp, c_d_p]),
    "ptl_ekf_log_enable": (C.c_int, [_vp, C.c_int64]),
    "ptl_ekf_smooth": (C.c_int, [_vp, c_d_p, c_d_p, c_d_p, c_d_p, C.c_int64, c_i64_p]),
    "ptl_ekf_smoother_log": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_icp_ekf_step": (C.c_int, [_vp, _vp, c_d_p, C.c_int64, _vp, C.c_int, C.c_int64, c_d_p, c_d_p, C.c_int32, c_d_p, c_d_p,
                                  c_d_p, C.POINTER(IcpStats)]),
    "ptl_seq_create": (C.c_int, [C.POINTER(SeqCfg), _vpp]),
    "ptl_seq_destroy": (C.c_int, [_vp]),
    "ptl_seq_upload_scan": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_float)]),
    "ptl_seq_upload_range": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_uint32)]),
    "ptl_seq_set_lut": (C.c_int, [_vp, _vp, C.c_int32]),
    "ptl_seq_upload_imu": (C.c_int, [_vp, c_d_p, c_i64_p]),
    "ptl_seq_run": (C.c_int, [_vp, C.c_int64]),
    "ptl_seq_advance": (C.c_int, [_vp, C.c_int64]),
    "ptl_seq_enqueue": (C.c_int, [_vp, C.c_int64]),
    "ptl_seq_wait": (C.c_int, [_vp]),
    "ptl_seq_copy_traj": (C.c_int, [_vp, _vp, C.c_int64, c_i64_p]),
    "ptl_device_sync": (C.c_int, [C.c_int]),
    "ptl_host_pin": (C.c_int, [C.c_int, _vp, C.c_uint64]),
    "ptl_host_unpin": (C.c_int, [_vp]),
    "ptl_seq_results": (C.c_int, [_vp, c_d_p, c_d_p, c_d_p, C.POINTER(IcpStats), C.c_int64, c_i64_p]),
    "ptl_seq_traj_device": (C.c_int, [_vp, _vpp, c_i64_p]),
    "ptl_seq_icp": (C.c_int, [_vp, _vpp]),
    "ptl_seq_profile": (C.c_int, [_vp, C.c_int, c_d_p, c_i64_p, C.c_int]),
    "ptl_seq_smoother_enable": (C.c_int, [_vp, C.c_int32]),
    "ptl_seq_smooth": (C.c_int, [_vp, c_d_p, c_d_p, c_d_p, c_d_p, c_i64_p]),
    "ptl_seq_smoother_log": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_batch_create": (C.c_int, [C.POINTER(SeqCfg), C.c_int32, _vpp]),
    "ptl_batch_destroy": (C.c_int, [_vp]),
    "ptl_batch_upload_scan": (C.c_int, [_vp, C.c_int32, C.c_int64, C.POINTER(C.c_float)]),
    "ptl_batch_set_lut": (C.c_int, [_vp, _vp, C.c_int32]),
    "ptl_batch_upload_range": (C.c_int, [_vp, C.c_int32, C.c_int64, C.POINTER(C.c_uint32)]),
    "ptl_batch_upload_imu": (C.c_int, [_vp, C.c_int32, c_d_p, c_i64_p]),
    "ptl_batch_run": (C.c_int, [_vp, C.c_int64]),
    "ptl_batch_enqueue": (C.c_int, [_vp, C.c_int64]),
    "ptl_batch_wait": (C.c_int, [_vp]),
    "ptl_batch_results": (C.c_int, [_vp, C.c_int32, c_d_p, c_d_p, c_d_p, C.POINTER(IcpStats), C.c_int64, c_i64_p]),
    "ptl_batch_copy_traj": (C.c_int, [_vp, C.c_int32, _vp, C.c_int64, c_i64_p]),
    "ptl_batch_smoother_enable": (C.c_int, [_vp, C.c_int32]),
    "ptl_batch_smooth": (C.c_int, [_vp]),
    "ptl_batch_smoothed": (C.c_int, [_vp, C.c_int32, c_d_p, c_d_p, c_d_p, c_d_p, c_i64_p]),
    "ptl_batch_smoother_log": (C.c_int, [_vp, C.c_int32, c_d_p, C.c_int64, c_i64_p, C.POINTER(C.c_int32)]),
    # IMU deskew (include/ptudes_mi.h)
    "ptl_ekf_knots_enable": (C.c_int, [_vp, C.c_int64]),
    "ptl_ekf_knots": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_icp_ekf_step_imu_deskew": (C.c_int, [_vp, _vp, c_d_p, C.c_int64, _vp, C.c_int, C.c_int64, C.c_double, C.c_double, c_d_p, C.c_int32,
                                              c_d_p, c_d_p, c_d_p, C.POINTER(IcpStats)]),
    "ptl_icp_deskew_modes": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int64, c_i64_p]),
    "ptl_icp_column_table": (C.c_int, [_vp, c_d_p]),
    "ptl_seq_imu_deskew_enable": (C.c_int, [_vp, C.c_int32, C.c_int64]),
    "ptl_seq_upload_sweep_times": (C.c_int, [_vp, c_d_p]),
    "ptl_seq_deskew_modes": (C.c_int, [_vp, C.POINTER(C.c_int32), C.c_int64, c_i64_p]),
    "ptl_seq_knots": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_batch_imu_deskew_enable": (C.c_int, [_vp, C.c_int32, C.c_int64]),
    "ptl_batch_upload_sweep_times": (C.c_int, [_vp, C.c_int32, c_d_p]),
    "ptl_batch_deskew_modes": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int32), C.c_int64, c_i64_p]),
    "ptl_batch_knots": (C.c_int, [_vp, C.c_int32, c_d_p, C.c_int64, c_i64_p, C.POINTER(C.c_int32)]),
    # posed scans into the world map (include/ptudes_mi.h)
    "ptl_traj_create": (C.c_int, [C.c_int, c_d_p, c_d_p, C.c_int64, C.c_double, C.c_double, _vpp]),
    "ptl_traj_destroy": (C.c_int, [_vp]),
    "ptl_icp_map_add_posed_range": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_uint32), c_d_p, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_icp_map_add_posed_xyz": (C.c_int, [_vp, _vp, C.POINTER(C.c_float), C.c_int32, C.c_int32, c_d_p, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_seq_map_build": (C.c_int, [_vp, _vp, _vp, c_d_p, C.c_int64, C.c_int64, c_i64_p, c_i64_p]),
    "ptl_batch_map_build": (C.c_int, [_vp, C.c_int32, _vp, _vp, c_d_p, C.c_int64, C.c_int64, c_i64_p, c_i64_p]),
    # lidar packets decoded on the device (include/ptudes_mi.h)
    "ptl_pkt_packet_bytes": (C.c_int64, [C.POINTER(PktFormat)]),
    "ptl_pktdec_create": (C.c_int, [C.POINTER(PktFormat), C.c_int32, C.c_int64, C.c_int32, _vpp]),
    "ptl_pktdec_destroy": (C.c_int, [_vp]),
    "ptl_pktdec_decode": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int32, _vp, _vp, _vp, _vp]),
    "ptl_pktdec_profile": (C.c_int, [_vp, C.c_int, c_d_p, c_i64_p, C.c_int]),
    # the channel fields of a pixel beside its range (include/ptudes_mi.h)
    "ptl_pkt_sizeof_field": (C.c_int64, []),
    "ptl_pkt_field_default": (C.c_int, [C.POINTER(PktFormat), C.c_int32, C.POINTER(PktField)]),
    "ptl_pktdec_decode_fields": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.c_int32, C.POINTER(PktField), C.c_int32, _vpp,
                                           _vp, _vp, _vp, _vp]),
    "ptl_seq_upload_packets": (C.c_int, [_vp, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(PktSummary), _vp]),
    "ptl_batch_upload_packets": (C.c_int, [_vp, C.c_int32, _vp, C.c_int64, _vp, C.c_int64, C.POINTER(PktSummary), _vp]),
    # sharpness of a map without ground truth (include/ptudes_mi.h)
    "ptl_map_score_default_cfg": (C.c_int, [C.POINTER(MapScoreCfg), C.c_double]),
    "ptl_icp_map_score": (C.c_int, [_vp, C.POINTER(MapScoreCfg), C.POINTER(MapScoreResult), c_d_p, C.POINTER(C.c_int32), c_d_p, c_d_p,
                                    C.c_int64, c_i64_p]),
    # frames of the fly-by drawn on the device (include/ptudes_mi.h)
    "ptl_render_sizeof_cfg": (C.c_int64, []),
    "ptl_render_default_cfg": (C.c_int, [C.POINTER(RenderCfg), C.c_int32, C.c_int32]),
    "ptl_render_create": (C.c_int, [C.POINTER(RenderCfg), C.c_int32, _vpp]),
    "ptl_render_destroy": (C.c_int, [_vp]),
    "ptl_render_set_palette": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "ptl_render_set_z_range": (C.c_int, [_vp, C.c_double, C.c_double]),
    "ptl_render_set_overlay":(C.c_int, [_vp, c_d_p, C.POINTER(C.c_uint32), C.c_int64, C.c_int32]),
    "ptl_render_set_point_colors": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32), C.c_int64]),
    "ptl_render_frames": (C.c_int, [_vp, _vp, C.POINTER(RenderCam), C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                    C.POINTER(C.c_uint64), c_i64_p, c_d_p]),
    "ptl_render_debug_set_early_reject": (C.c_int, [_vp, C.c_int32]),
    # distance of query points to a map's stored points (include/ptudes_mi.h)
    "ptl_map_cmp_sizeof_cfg": (C.c_int64, []),
    "ptl_map_cmp_default_cfg": (C.c_int, [C.POINTER(MapCmpCfg), C.c_double]),
    "ptl_icp_map_distance": (C.c_int, [_vp, C.POINTER(MapCmpCfg), c_d_p, C.c_int64, C.POINTER(MapCmpResult), c_d_p]),
    "ptl_icp_map_compare": (C.c_int, [_vp, _vp, C.POINTER(MapCmpCfg), C.POINTER(MapCmpResult), c_d_p, c_d_p, C.c_int64, c_i64_p]),
    # free space carved: through / support votes of a map's stored points (include/ptudes_mi.h)
    "ptl_carve_sizeof_cfg": (C.c_int64, []),
    "ptl_carve_default_cfg": (C.c_int, [C.POINTER(CarveCfg), C.c_double]),
    "ptl_carve_create": (C.c_int, [_vp, C.POINTER(CarveCfg), _vpp]),
    "ptl_carve_destroy": (C.c_int, [_vp]),
    "ptl_carve_add_posed_range": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_uint32), c_d_p, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_carve_add_posed_xyz": (C.c_int, [_vp, _vp, C.POINTER(C.c_float), C.c_int32, C.c_int32, c_d_p, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_carve_add_seq": (C.c_int, [_vp, _vp, _vp, c_d_p, C.c_int64, C.c_int64, c_i64_p, c_i64_p]),
    "ptl_carve_add_batch": (C.c_int, [_vp, _vp, C.c_int32, _vp, c_d_p, C.c_int64, C.c_int64, c_i64_p, c_i64_p]),
    "ptl_carve_read": (C.c_int, [_vp, C.POINTER(CarveResult), c_d_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int64, c_i64_p]),
    # a sweep's fit to a map at K candidate poses (include/ptudes_mi.h)
    "ptl_pose_search_sizeof_cfg": (C.c_int64, []),
    "ptl_pose_search_default_cfg": (C.c_int, [C.POINTER(PoseSearchCfg), C.c_double]),
    "ptl_icp_pose_hits": (C.c_int, [_vp, C.POINTER(PoseSearchCfg), c_d_p, C.c_int64, c_d_p, C.c_int64, C.POINTER(PoseSearchResult),
                                    C.POINTER(C.c_int32)]),
    # the map painted: a lidar field summed per stored point (include/ptudes_mi.h)
    "ptl_paint_sizeof_result": (C.c_int64, []),
    "ptl_paint_create": (C.c_int, [_vp, _vpp]),
    "ptl_paint_destroy": (C.c_int, [_vp]),
    "ptl_paint_add_posed_range": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), c_d_p, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_paint_add_posed_xyz": (C.c_int, [_vp, _vp, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_int32, C.c_int32, c_d_p, c_i64_p,
                                          C.POINTER(C.c_int32)]),
    "ptl_paint_read": (C.c_int, [_vp, C.POINTER(PaintResult), c_d_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int64, c_i64_p]),
    # the occupancy grid of a run: free / hit counts per cell (include/ptudes_mi.h)
    "ptl_grid_sizeof_cfg": (C.c_int64, []),
    "ptl_grid_sizeof_result": (C.c_int64, []),
    "ptl_grid_default_cfg": (C.c_int, [C.POINTER(GridCfg), C.c_double]),
    "ptl_grid_create": (C.c_int, [C.c_int32, C.POINTER(GridCfg), _vpp]),
    "ptl_grid_destroy": (C.c_int, [_vp]),
    "ptl_grid_add_posed_range": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_uint32), c_d_p, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_grid_add_posed_xyz": (C.c_int, [_vp, _vp, C.POINTER(C.c_float), C.c_int32, C.c_int32, c_d_p, c_i64_p, C.POINTER(C.c_int32)]),
    "ptl_grid_add_seq": (C.c_int, [_vp, _vp, _vp, c_d_p, C.c_int64, C.c_int64, c_i64_p, c_i64_p]),
    "ptl_grid_add_batch": (C.c_int, [_vp, _vp, C.c_int32, _vp, c_d_p, C.c_int64, C.c_int64, c_i64_p, c_i64_p]),
    "ptl_grid_read": (C.c_int, [_vp, C.POINTER(GridResult), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint32),
                                C.POINTER(C.c_uint32)]),
    "ptl_grid_clear": (C.c_int, [_vp]),
    # a sweep's rays cast through a saved map: the first stored point along each pixel's ray (include/ptudes_mi.h)
    "ptl_cast_sizeof_cfg": (C.c_int64, []),
    "ptl_cast_default_cfg": (C.c_int, [C.POINTER(CastCfg), C.c_double]),
    "ptl_cast_create": (C.c_int, [_vp, C.POINTER(CastCfg), _vpp]),
    "ptl_cast_destroy": (C.c_int, [_vp]),
    "ptl_cast_posed_range": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_uint32), c_d_p, C.POINTER(CastResult), C.POINTER(C.c_uint8), c_d_p, c_d_p,
                                       C.POINTER(C.c_int32)]),
    "ptl_cast_posed_xyz": (C.c_int, [_vp, _vp, C.POINTER(C.c_float), C.c_int32, C.c_int32, c_d_p, C.POINTER(CastResult), C.POINTER(C.c_uint8), c_d_p,
                                     c_d_p, C.POINTER(C.c_int32)]),
    "ptl_cast_points": (C.c_int, [_vp, c_d_p, C.c_int64, c_i64_p]),
    # revisited places: polar height descriptors matched at every heading (include/ptudes_mi.h)
    "ptl_place_sizeof_cfg": (C.c_int64, []),
    "ptl_place_default_cfg": (C.c_int, [C.POINTER(PlaceCfg)]),
    "ptl_place_create": (C.c_int, [C.c_int32, C.POINTER(PlaceCfg), _vpp]),
    "ptl_place_destroy": (C.c_int, [_vp]),
    "ptl_place_clear": (C.c_int, [_vp]),
    "ptl_place_size": (C.c_int, [_vp, c_i64_p]),
    "ptl_place_tables": (C.c_int, [_vp, c_d_p, c_d_p]),
    "ptl_place_profile": (C.c_int, [_vp, c_d_p, c_i64_p, C.c_int32]),
    "ptl_place_describe_range": (C.c_int, [_vp, _vp, C.POINTER(C.c_uint32), c_d_p, C.c_int32, c_i64_p, C.POINTER(PlaceInfo)]),
    "ptl_place_describe_xyz": (C.c_int, [_vp, _vp, C.c_int, C.c_int64, c_d_p, C.c_int32, c_i64_p, C.POINTER(PlaceInfo)]),
    "ptl_place_match": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(PlaceResult)]),
    "ptl_place_match_all": (C.c_int, [_vp, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_int32),
                                      C.POINTER(PlaceResult)]),
    "ptl_place_read": (C.c_int, [_vp, C.c_int64, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(PlaceInfo)]),
    "ptl_place_load": (C.c_int, [_vp, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(PlaceInfo)]),
    "ptl_batch_gn_phases": (C.c_int, [_vp, c_i64_p]),
    "ptl_batch_icp": (C.c_int, [_vp, C.c_int32, _vpp]),
    "ptl_batch_profile": (C.c_int, [_vp, C.c_int, c_d_p, c_i64_p, C.c_int]),
    "ptl_batch_set_driver": (C.c_int, [_vp, C.c_int32, C.c_int64]),
    "ptl_batch_reset": (C.c_int, [_vp]),
    "ptl_batch_seq_clocks": (C.c_int, [_vp, C.c_int32, c_i64_p]),
    "ptl_batch_set_team_workgroups": (C.c_int, [_vp, C.c_int32]),
    "ptl_batch_team_workgroups": (C.c_int, [_vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ptl_batch_exec_counters": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_uint64)]),
    "ptl_batch_sched_counters": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_uint64)]),
    "ptl_batch_status": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "ptl_batch_debug_stall_block": (C.c_int, [_vp, C.c_int32, C.c_int32]),
    "ptl_batch_debug_set_map_points_per_thread": (C.c_int, [_vp, C.c_int32, C.POINTER(C.c_int32)]),
    "ptl_build_info": (C.c_int, [C.POINTER(C.c_int32)]),
    "ptl_code_id": (C.c_char_p, []),
    "ptl_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "ptl_comm_create": (C.c_int, [C.POINTER(C.c_uint8), C.c_int32, C.c_int32, C.c_int32, _vpp]),
    "ptl_comm_destroy": (C.c_int, [_vp]),
    "ptl_gather_trajectories": (C.c_int, [_vp, _vp, C.c_int64, C.c_int64, c_i64_p, c_d_p, c_i64_p]),
    "ptl_batch_gather_trajectories": (C.c_int, [_vp, _vp, c_d_p, c_i64_p]),
}

_lib = None


def lib():
    """The loaded library.  Raises (never falls back) when libptudes_mi.so is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; "
                "g.build()' or make -C ptudes-lab_amd/csrc).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        older = bool(os.environ.get("PTL_LIB_PATH")) and os.environ.get("PTL_LIB_ALLOW_OLDER") == "1"  # A/B runs against a library built from an older commit
        for name, (res, args) in PROTOTYPES.items():
            if older and not hasattr(L, name):
                continue
            f = getattr(L, name)  # AttributeError if the library does not export a declared symbol
            f.restype = res
            f.argtypes = args
        if hasattr(L, "ptl_abi_version"):
            # the binding's layouts against the loaded library's, before any struct changes hands
            have = (L.ptl_abi_version(), [L.ptl_sizeof_cfg(i) for i in range(4)])
            want = (ABI_VERSION, [C.sizeof(t) for t in (IcpCfg, EkfCfg, SeqCfg, IcpStats)])
            if have != want and not older:
                raise RuntimeError(f"{LIB_PATH}: ABI version / sizeof(icp cfg, ekf cfg, seq cfg, icp stats) = {have}, this binding "
                                   f"(ptudes-lab_amd/_lib.py) was written for {want}: rebuild the library or update the binding")
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().ptl_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(msg)
        raise RuntimeError(f"libptudes_mi error {rc}: {msg}")


def dptr(a):
    return a.ctypes.data_as(c_d_p)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)
