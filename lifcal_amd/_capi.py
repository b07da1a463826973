"""ctypes view of include/lifcal_ba.h (struct layouts + prototypes).  Plumbing only."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LIFCAL_BA_LIB") or os.path.join(_HERE, "csrc", "liblifcal_ba.so")   # (LIFCAL_BA_LIB: a development build, e.g. make dev / make stamps)

dptr = C.POINTER(C.c_double)
uptr = C.POINTER(C.c_uint32)


class Problem(C.Structure):
    _fields_ = [
        ("n_obs", C.c_uint32), ("n_frames", C.c_uint32), ("n_points", C.c_uint32), ("n_constraints", C.c_uint32),
        ("u", dptr), ("v", dptr), ("mcx", dptr), ("mcy", dptr), ("pt", uptr), ("fr", uptr),
        ("cam", dptr), ("views", dptr), ("pts", dptr),
        ("spx", C.c_double), ("spy", C.c_double), ("scale", C.c_double),
        ("config", C.c_uint32), ("fixed_mask", C.c_uint32),
        ("lower", dptr), ("upper", dptr),
        ("c_i", uptr), ("c_j", uptr), ("c_dist", dptr), ("c_sigma", dptr),
        ("use_constraints", C.c_uint32), ("reserved", C.c_uint32),
    ]


class Options(C.Structure):
    _fields_ = [
        ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("initial_radius", C.c_double), ("max_radius", C.c_double), ("min_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
        ("loss_scale", C.c_double),
        ("max_iterations", C.c_int32), ("jacobi_scaling", C.c_int32), ("precision", C.c_int32), ("device", C.c_int32),
        ("rank", C.c_int32), ("world_size", C.c_int32), ("verbose", C.c_int32), ("deterministic", C.c_int32),
    ]


class Summary(C.Structure):
    _fields_ = [
        ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_radius", C.c_double),
        ("final_gradient_max_norm", C.c_double),
        ("iterations", C.c_int32), ("successful_steps", C.c_int32), ("unsuccessful_steps", C.c_int32),
        ("termination", C.c_int32),
        ("seconds_total", C.c_double), ("seconds_sweep", C.c_double), ("seconds_linear_solve", C.c_double),
    ]


class SweepOut(C.Structure):
    _fields_ = [
        ("cost", C.c_double), ("gradient_max_norm", C.c_double),
        ("n_reduced", C.c_uint32), ("n_promoted", C.c_uint32),
        ("S", dptr), ("rhs", dptr), ("gradient_reduced", dptr), ("point_gradient", dptr), ("point_hessian_inv", dptr),
        ("seconds", C.c_double),
    ]


class Stats(C.Structure):
    _fields_ = [("std_x", C.c_double), ("std_y", C.c_double), ("mae_x", C.c_double), ("mae_y", C.c_double),
                ("num_points", C.c_uint32), ("num_inliers", C.c_uint32)]


class Info(C.Structure):
    _fields_ = [("n_obs_local", C.c_uint32), ("n_points_local", C.c_uint32), ("n_groups", C.c_uint32),
                ("n_tiles", C.c_uint32), ("n_lenses", C.c_uint32), ("n_reduced", C.c_uint32), ("n_promoted", C.c_uint32),
                ("n_chunks", C.c_uint32), ("max_window_frames", C.c_uint32),
                ("device_bytes", C.c_uint64), ("stream", C.c_void_p)]


class StepOut(C.Structure):          # lifcal_ba_step_out
    _fields_ = [("delta_reduced", dptr), ("delta_points", dptr), ("lambda_reduced", dptr), ("lambda_points", dptr),
                ("gtd", C.c_double), ("ddd", C.c_double), ("step2", C.c_double), ("x2", C.c_double),
                ("cand_cost", C.c_double), ("chol_fail", C.c_double),
                ("route", C.c_int32), ("panel_in_lds", C.c_int32)]


class Profile(C.Structure):
    _fields_ = [("n_sweeps", C.c_uint32), ("special_points", C.c_double), ("ms_accumulate", C.c_double),
                ("ms_schur", C.c_double), ("ms_total", C.c_double), ("ms_exchange", C.c_double), ("n_sampled", C.c_uint32)]


class CovarianceOptions(C.Structure):   # lifcal_ba_covariance_options
    _fields_ = [("gauge_frame", C.c_int32), ("want_pose_blocks", C.c_int32), ("scale_by_residual_variance", C.c_int32),
                ("reserved", C.c_int32), ("null_rcond", C.c_double), ("estimable_tol", C.c_double)]


class CovarianceOut(C.Structure):       # lifcal_ba_covariance_out
    _fields_ = [("camera", dptr), ("pose", dptr), ("pose_band", dptr), ("camera_null", dptr),
                ("estimable_mask", C.c_uint32), ("null_rank", C.c_uint32), ("gauge_frame_used", C.c_int32), ("live_mask", C.c_uint32),
                ("sigma2", C.c_double), ("cost", C.c_double), ("seconds", C.c_double)]


class WindowReport(C.Structure):   # lifcal_ba_window_report
    _fields_ = [("first_frame", C.c_uint32), ("n_frames", C.c_uint32), ("n_fixed_frames", C.c_uint32), ("n_points", C.c_uint32), ("n_obs", C.c_uint32),
                ("n_dropped_constraints", C.c_uint32), ("summary", Summary)]


class Partition(C.Structure):      # lifcal_ba_partition
    _fields_ = [("world_size", C.c_uint32), ("n_frames", C.c_uint32), ("n_points", C.c_uint32), ("band_width", C.c_uint32), ("n_obs", C.c_uint64),
                ("point_owner", C.POINTER(C.c_int32)), ("rank_first", uptr), ("rank_frames", uptr), ("rank_obs", C.POINTER(C.c_uint64)), ("frame_used", C.POINTER(C.c_uint8))]


class PartitionArrays:
    """Owns the arrays of a lifcal_ba_partition filled by lifcal_ba_partition_points."""

    def __init__(self, problem: "ProblemArrays", world_size: int):
        lib = load_library()
        F, P = problem.struct.n_frames, problem.struct.n_points
        self.point_owner = np.zeros(max(P, 1), np.int32); self.rank_first = np.zeros(world_size, np.uint32); self.rank_frames = np.zeros(world_size, np.uint32)
        self.rank_obs = np.zeros(world_size, np.uint64); self.frame_used = np.zeros(max(F, 1), np.uint8)
        self.struct = Partition(world_size, 0, 0, 0, 0, self.point_owner.ctypes.data_as(C.POINTER(C.c_int32)), as_uptr(self.rank_first), as_uptr(self.rank_frames),
                                self.rank_obs.ctypes.data_as(C.POINTER(C.c_uint64)), self.frame_used.ctypes.data_as(C.POINTER(C.c_uint8)))
        rc = lib.lifcal_ba_partition_points(C.byref(problem.struct), C.byref(self.struct))
        if rc:
            raise RuntimeError(f"lifcal_ba_partition_points: {rc}")

    def shard_of(self, problem: "ProblemArrays", rank: int) -> "ProblemArrays":
        """the rank's local problem: only the observations of the points it owns (full parameter arrays)"""
        sel = np.flatnonzero(self.point_owner[problem.pt] == rank)
        return ProblemArrays(problem.u[sel], problem.v[sel], problem.mcx[sel], problem.mcy[sel], problem.pt[sel], problem.fr[sel], problem.cam, problem.views, problem.pts,
                             problem.struct.spx, problem.struct.scale, problem.struct.config, spy=problem.struct.spy, fixed_mask=problem.struct.fixed_mask,
                             lower=problem.lower, upper=problem.upper, use_constraints=0)


class PlanInfo(C.Structure):
    _fields_ = [("n_groups", C.c_uint32), ("n_tiles", C.c_uint32), ("n_lenses", C.c_uint32), ("n_promoted", C.c_uint32),
                ("n_reduced", C.c_uint32), ("max_group_obs", C.c_uint32), ("n_chunks", C.c_uint32),
                ("max_window_frames", C.c_uint32)]


class PlanStats(C.Structure):     # lifcal_ba_plan_statistics
    _fields_ = [("n_blocks", C.c_uint32), ("n_passes", C.c_uint32), ("pass_lanes", C.c_uint32), ("max_block_passes", C.c_uint32),
                ("n_lanes", C.c_uint64), ("pass_steps", C.c_uint64), ("tile_steps", C.c_uint64), ("n_obs_window", C.c_uint64),
                ("n_points_permuted", C.c_uint64), ("violations", C.c_uint64),
                ("block_cost_mean", C.c_double), ("block_cost_max", C.c_double)]


class PlanShape(C.Structure):     # lifcal_ba_plan_shape_figures
    _fields_ = [("tiles_0_steps", C.c_uint64), ("tiles_1_step", C.c_uint64), ("tiles_2_steps", C.c_uint64), ("tiles_odd_steps", C.c_uint64),
                ("tiles_even_steps", C.c_uint64), ("ell_rows", C.c_uint64), ("max_row_read", C.c_uint64), ("last_tile_row0", C.c_uint64),
                ("last_tile_steps", C.c_uint32), ("min_pass_points", C.c_uint32), ("max_pass_points", C.c_uint32),
                ("min_block_passes", C.c_uint32), ("max_block_passes", C.c_uint32), ("reserved", C.c_uint32)]


ALLREDUCE_FN =C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

class InitProblem(C.Structure):
    _fields_ = [("n", C.c_uint64), ("vdepth", C.POINTER(C.c_double)), ("fr", C.POINTER(C.c_uint32)), ("pt", C.POINTER(C.c_uint32)),
                ("n_frames", C.c_uint32), ("n_points", C.c_uint32), ("world_to_cam", C.POINTER(C.c_double)), ("pts", C.POINTER(C.c_double)),
                ("fL_init", C.c_double)]


class InitResult(C.Structure):
    _fields_ = [("B_init", C.c_double), ("bL0_init", C.c_double), ("n_used", C.c_uint64), ("rank", C.c_int32), ("reserved", C.c_int32)]


class InitArrays:
    """Owns contiguous copies of the inputs of lifcal_init_plenoptic / lo_init_plenoptic."""

    def __init__(self, vdepth, fr, pt, world_to_cam, pts, fL_init):
        self.vdepth = np.ascontiguousarray(vdepth, np.float64)
        self.fr = np.ascontiguousarray(fr, np.uint32)
        self.pt = np.ascontiguousarray(pt, np.uint32)
        # (F, 4, 4) matrices in mathematical (row, column) indexing -> Eigen's column-major storage
        w = np.asarray(world_to_cam, np.float64).reshape(-1, 4, 4)
        self.w2c = np.ascontiguousarray(np.transpose(w, (0, 2, 1)).reshape(-1, 16))
        self.pts = np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3))
        assert len(self.vdepth) == len(self.fr) == len(self.pt)
        self.struct = InitProblem(len(self.vdepth), as_dptr(self.vdepth), as_uptr(self.fr), as_uptr(self.pt), len(self.w2c), len(self.pts),
                                  as_dptr(self.w2c), as_dptr(self.pts), float(fL_init))


class MlaParams(C.Structure):      # include/lifcal_mla.h lifcal_mla_params
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("lens_diameter", C.c_float), ("lens_base_y", C.c_float * 2),
                ("rotation", C.c_float), ("offset", C.c_float * 2), ("rotation_on_grid", C.c_int32)]


class MlaPoints(C.Structure):      # lifcal_mla_points
    _fields_ = [("n", C.c_uint64), ("x", dptr), ("y", dptr), ("vdepth", dptr), ("fr", uptr), ("pt", uptr)]


class MlaObservations(C.Structure):  # lifcal_mla_observations
    _fields_ = [("capacity", C.c_uint64), ("n_obs", C.c_uint64), ("u", dptr), ("v", dptr), ("mcx", dptr), ("mcy", dptr),
                ("src", uptr), ("fr", uptr), ("pt", uptr)]


MLA_MORE = 1
_fptr = C.POINTER(C.c_float)
_iptr = C.POINTER(C.c_int32)

# every symbol include/lifcal_mla.h declares
MLA_PROTOTYPES = {
    "lifcal_mla_create": (C.c_int, [C.POINTER(MlaParams), C.c_int32, C.POINTER(C.c_void_p)]),
    "lifcal_mla_destroy": (None, [C.c_void_p]),
    "lifcal_mla_info": (C.c_int, [C.c_void_p, _iptr, _iptr, _iptr]),
    "lifcal_mla_get_lenses": (C.c_int, [C.c_void_p, _fptr, _fptr, _iptr]),
    "lifcal_mla_get_maps": (C.c_int, [C.c_void_p, _iptr, _iptr]),
    "lifcal_mla_get_web": (C.c_int, [C.c_void_p, dptr, dptr, dptr, _iptr]),
    "lifcal_mla_project": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(MlaPoints), C.POINTER(MlaObservations)]),
}

class CameraModel(C.Structure):    # include/lifcal_io.h lifcal_camera_model
    _fields_ = [("image_width", C.c_int32), ("image_height", C.c_int32), ("pixel_size", C.c_double),
                ("fL", C.c_double), ("bL0", C.c_double), ("B", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("n_radial", C.c_int32), ("radial", C.c_double * 8), ("tangential", C.c_int32), ("tangential_dist", C.c_double * 2),
                ("ml_center_adjustment", C.c_int32)]


class Protocol(C.Structure):       # lifcal_protocol
    _fields_ = [("model", CameraModel), ("refine_poses", C.c_int32), ("refine_points", C.c_int32), ("robust_cost", C.c_int32),
                ("std_x", C.c_double), ("std_y", C.c_double), ("mae_x", C.c_double), ("mae_y", C.c_double)]


# every symbol include/lifcal_io.h declares
IO_PROTOTYPES = {
    "lifcal_write_camera_model": (C.c_int, [C.c_char_p, C.POINTER(CameraModel)]),
    "lifcal_write_extrinsic_orientations_xml": (C.c_int, [C.c_char_p, C.c_uint32, _iptr, dptr]),
    "lifcal_write_extrinsic_orientations_txt": (C.c_int, [C.c_char_p, C.c_uint32, _iptr, dptr]),
    "lifcal_write_raw_image_points_csv": (C.c_int, [C.c_char_p, C.c_uint64, C.c_uint32, _iptr, uptr, dptr, dptr, dptr, dptr, uptr]),
    "lifcal_write_protocol": (C.c_int, [C.c_char_p, C.POINTER(Protocol)]),
    "lifcal_write_object_coordinates_ply": (C.c_int, [C.c_char_p, C.c_uint64, dptr]),
    "lifcal_write_object_coordinates_colmap_ids": (C.c_int, [C.c_char_p, C.c_uint64, _iptr, dptr]),
    "lifcal_write_camera_orientations_ply": (C.c_int, [C.c_char_p, C.c_uint32, dptr, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double]),
    "lifcal_write_camera_coordinates_ply": (C.c_int, [C.c_char_p, C.c_int32, C.c_uint64, dptr]),
    "lifcal_write_group_stats_csv": (C.c_int, [C.c_char_p, C.c_char_p, C.c_uint64, _iptr, dptr, C.c_void_p]),
}

class ColmapInfo(C.Structure):     # include/lifcal_colmap.h lifcal_colmap_info
    _fields_ = [("n_frames", C.c_uint32), ("n_points", C.c_uint32), ("n_image_points", C.c_uint64), ("binary", C.c_int32),
                ("camera_model_id", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("reserved", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("f", C.c_double)]


# every symbol include/lifcal_colmap.h declares
COLMAP_PROTOTYPES = {
    "lifcal_colmap_read": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "lifcal_colmap_get_info": (C.c_int, [C.c_void_p, C.POINTER(ColmapInfo)]),
    "lifcal_colmap_get_frames": (C.c_int, [C.c_void_p, _iptr, dptr, dptr, dptr]),
    "lifcal_colmap_get_points": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), dptr]),
    "lifcal_colmap_get_image_points": (C.c_int, [C.c_void_p, dptr, dptr, uptr, uptr]),
    "lifcal_colmap_free": (None, [C.c_void_p]),
}

class ObjectSpace(C.Structure):      # include/lifcal_ba.h lifcal_ba_object_space
    _fields_ = [("rms", C.c_double * 3), ("max_abs", C.c_double * 3), ("rms_rel_depth", C.c_double), ("n_used", C.c_uint64), ("n_skipped", C.c_uint64)]


class GroupStats(C.Structure):       # include/lifcal_ba.h lifcal_ba_group_stats: one 64-byte row per group
    _fields_ = [("sum_x", C.c_double), ("sum_y", C.c_double), ("sum_xx", C.c_double), ("sum_yy", C.c_double), ("sum_w", C.c_double),
                ("max_abs_x", C.c_double), ("max_abs_y", C.c_double), ("n", C.c_uint32), ("n_inliers", C.c_uint32)]


# the same row as a numpy structured dtype (tables are arrays of it)
GROUP_STATS_DTYPE = np.dtype([("sum_x", "<f8"), ("sum_y", "<f8"), ("sum_xx", "<f8"), ("sum_yy", "<f8"), ("sum_w", "<f8"),
                              ("max_abs_x", "<f8"), ("max_abs_y", "<f8"), ("n", "<u4"), ("n_inliers", "<u4")])
_gptr = C.POINTER(GroupStats)


class ResidualReportIO(C.Structure):  # lifcal_ba_residual_report_io
    _fields_ = [("inlier_threshold", C.c_double), ("ex", dptr), ("ey", dptr), ("weight", dptr), ("lens", uptr), ("lens_xy", dptr),
                ("per_frame", _gptr), ("per_point", _gptr), ("per_lens", _gptr), ("total", GroupStats), ("seconds", C.c_double)]


class DepthSampleCounts(C.Structure):   # include/lifcal_depth.h lifcal_depth_sample_counts
    _fields_ = [("direct", C.c_uint64), ("interpolated", C.c_uint64), ("failed", C.c_uint64)]


class DepthCamera(C.Structure):      # lifcal_depth_camera
    _fields_ = [("cam", C.c_double * 17), ("spx", C.c_double), ("spy", C.c_double), ("config", C.c_uint32), ("reserved", C.c_uint32)]


class DepthPoints(C.Structure):      # lifcal_depth_points
    _fields_ = [("n", C.c_uint64), ("x", dptr), ("y", dptr), ("vdepth", dptr), ("fr", uptr), ("views", dptr), ("n_frames", C.c_uint32), ("reserved", C.c_uint32),
                ("cam_cov", dptr), ("sigma_v", C.c_double), ("p_c", dptr), ("p_w", dptr), ("jac", dptr), ("dpc_dv", dptr), ("cov_pc", dptr), ("n_invalid", C.c_uint64)]


class DepthMapsArgs(C.Structure):    # lifcal_depth_maps
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("eval", C.c_int32), ("out_double", C.c_int32), ("out_on_device", C.c_int32), ("n_frames", C.c_uint32),
                ("frame", uptr), ("views", dptr), ("cam_cov", dptr), ("sigma_v", C.c_double), ("xyz", C.c_void_p), ("z", C.c_void_p), ("sigma_z", C.c_void_p),
                ("n_invalid", C.c_uint64), ("seconds", C.c_double)]


class DepthForward(C.Structure):     # lifcal_depth_forward
    _fields_ = [("n", C.c_uint64), ("p", dptr), ("fr", uptr), ("views", dptr), ("n_frames", C.c_uint32), ("reserved", C.c_uint32),
                ("x", dptr), ("y", dptr), ("vdepth", dptr), ("n_invalid", C.c_uint64)]


class DepthPairStats(C.Structure):   # lifcal_depth_pair_stats
    _fields_ = [("n_valid", C.c_uint64), ("n_compared", C.c_uint64), ("n_consistent", C.c_uint64), ("n_occluded", C.c_uint64), ("n_violation", C.c_uint64),
                ("sum_e", C.c_double), ("sum_e2", C.c_double)]


# the same row as a numpy structured dtype (the pair table is an array of it)
DEPTH_PAIR_DTYPE = np.dtype([("n_valid", "<u8"), ("n_compared", "<u8"), ("n_consistent", "<u8"), ("n_occluded", "<u8"), ("n_violation", "<u8"),
                             ("sum_e", "<f8"), ("sum_e2", "<f8")])


class DepthViewsArgs(C.Structure):   # lifcal_depth_views
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("span", C.c_uint32), ("out_on_device", C.c_int32), ("n_frames", C.c_uint32), ("reserved", C.c_uint32),
                ("frame", uptr), ("views", dptr), ("tol_iv", C.c_double), ("support", C.c_void_p), ("conflict", C.c_void_p), ("pair", C.c_void_p),
                ("seconds", C.c_double)]


class DepthFusionArgs(C.Structure):  # lifcal_depth_fusion
    _fields_ = [("first", C.c_int32), ("count", C.c_int32), ("span", C.c_uint32), ("out_on_device", C.c_int32), ("n_frames", C.c_uint32), ("out_double", C.c_int32),
                ("frame", uptr), ("views", dptr), ("tol_iv", C.c_double), ("min_support", C.c_uint32), ("max_conflict", C.c_uint32), ("capacity", C.c_uint64),
                ("xyz", C.c_void_p), ("n_merged", C.c_void_p), ("src", C.c_void_p), ("n_points", C.c_uint64), ("seconds", C.c_double)]


# every symbol include/lifcal_depth.h declares
DEPTH_PROTOTYPES = {
    "lifcal_depth_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "lifcal_depth_destroy": (None, [C.c_void_p]),
    "lifcal_depth_set_maps": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "lifcal_depth_sample": (C.c_int, [C.c_void_p, C.c_uint64, dptr, dptr, _iptr, dptr, C.POINTER(DepthSampleCounts)]),
    "lifcal_depth_back_project_points": (C.c_int, [C.c_int32, C.POINTER(DepthCamera), C.POINTER(DepthPoints)]),
    "lifcal_depth_back_project_maps": (C.c_int, [C.c_void_p, C.POINTER(DepthCamera), C.POINTER(DepthMapsArgs)]),
    "lifcal_depth_project_points": (C.c_int, [C.c_int32, C.POINTER(DepthCamera), C.POINTER(DepthForward)]),
    "lifcal_depth_check_maps": (C.c_int, [C.c_void_p, C.POINTER(DepthCamera), C.POINTER(DepthViewsArgs)]),
    "lifcal_depth_fuse_maps": (C.c_int, [C.c_void_p, C.POINTER(DepthCamera), C.POINTER(DepthFusionArgs)]),
}

class ResectProblem(C.Structure):    # include/lifcal_resect.h lifcal_resect_problem
    _fields_ = [("n_obs", C.c_uint32), ("n_frames", C.c_uint32), ("n_points", C.c_uint32), ("reserved", C.c_uint32),
                ("u", dptr), ("v", dptr), ("mcx", dptr), ("mcy", dptr), ("pt", uptr), ("fr", uptr),
                ("cam", dptr), ("pts", dptr), ("views", dptr),
                ("spx", C.c_double), ("spy", C.c_double), ("scale", C.c_double), ("config", C.c_uint32)]


class ResectFrame(C.Structure):      # lifcal_resect_frame: one 288-byte row per frame
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_radius", C.c_double), ("final_gradient_max_norm", C.c_double),
                ("H", C.c_double * 21), ("g", C.c_double * 6), ("sum_xx", C.c_double), ("sum_yy", C.c_double),
                ("n_obs", C.c_uint32), ("n_inliers", C.c_uint32),
                ("iterations", C.c_int32), ("successful_steps", C.c_int32), ("unsuccessful_steps", C.c_int32), ("termination", C.c_int32)]


# the same row as a numpy structured dtype (the table of a call is an array of it)
RESECT_FRAME_DTYPE = np.dtype([("initial_cost", "<f8"), ("final_cost", "<f8"), ("final_radius", "<f8"), ("final_gradient_max_norm", "<f8"),
                               ("H", "<f8", (21,)), ("g", "<f8", (6,)), ("sum_xx", "<f8"), ("sum_yy", "<f8"),
                               ("n_obs", "<u4"), ("n_inliers", "<u4"),
                               ("iterations", "<i4"), ("successful_steps", "<i4"), ("unsuccessful_steps", "<i4"), ("termination", "<i4")])

# every symbol include/lifcal_resect.h declares
RESECT_PROTOTYPES = {
    "lifcal_resect_frames": (C.c_int, [C.POINTER(ResectProblem), C.POINTER(Options), C.c_double, C.c_void_p, dptr]),
}


class IntersectProblem(C.Structure):    # include/lifcal_intersect.h lifcal_intersect_problem
    _fields_ = [("n_obs", C.c_uint32), ("n_frames", C.c_uint32), ("n_points", C.c_uint32), ("reserved", C.c_uint32),
                ("u", dptr), ("v", dptr), ("mcx", dptr), ("mcy", dptr), ("pt", uptr), ("fr", uptr),
                ("cam", dptr), ("views", dptr), ("pts", dptr),
                ("spx", C.c_double), ("spy", C.c_double), ("scale", C.c_double), ("config", C.c_uint32)]


class IntersectPoint(C.Structure):      # lifcal_intersect_point: one 144-byte row per point
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_radius", C.c_double), ("final_gradient_max_norm", C.c_double),
                ("H", C.c_double * 6), ("g", C.c_double * 3), ("sum_xx", C.c_double), ("sum_yy", C.c_double),
                ("n_obs", C.c_uint32), ("n_inliers", C.c_uint32),
                ("iterations", C.c_int32), ("successful_steps", C.c_int32), ("unsuccessful_steps", C.c_int32), ("termination", C.c_int32)]


# the same row as a numpy structured dtype (the table of a call is an array of it)
INTERSECT_POINT_DTYPE = np.dtype([("initial_cost", "<f8"), ("final_cost", "<f8"), ("final_radius", "<f8"), ("final_gradient_max_norm", "<f8"),
                                  ("H", "<f8", (6,)), ("g", "<f8", (3,)), ("sum_xx", "<f8"), ("sum_yy", "<f8"),
                                  ("n_obs", "<u4"), ("n_inliers", "<u4"),
                                  ("iterations", "<i4"), ("successful_steps", "<i4"), ("unsuccessful_steps", "<i4"), ("termination", "<i4")])

# every symbol include/lifcal_intersect.h declares
INTERSECT_PROTOTYPES = {
    "lifcal_intersect_points": (C.c_int, [C.POINTER(IntersectProblem), C.POINTER(Options), C.c_double, C.c_void_p, dptr]),
}

class StartFrame(C.Structure):          # include/lifcal_start.h lifcal_start_frame: one 72-byte row per frame
    _fields_ = [("sum_w", C.c_double), ("align_rms", C.c_double), ("eig", C.c_double * 2), ("sum_xx", C.c_double), ("sum_yy", C.c_double),
                ("n_obs", C.c_uint32), ("n_inliers", C.c_uint32), ("n_groups", C.c_uint32), ("n_used", C.c_uint32),
                ("status", C.c_int32), ("reserved", C.c_int32)]


class StartGroup(C.Structure):          # lifcal_start_group: one 48-byte row per (frame, point) group
    _fields_ = [("xyz", C.c_double * 3), ("rms_px", C.c_double), ("fr", C.c_uint32), ("pt", C.c_uint32), ("n_obs", C.c_uint32), ("status", C.c_int32)]


class StartPoint(C.Structure):          # lifcal_start_point: one 40-byte row per point
    _fields_ = [("sum_xx", C.c_double), ("sum_yy", C.c_double), ("min_pivot", C.c_double),
                ("n_obs", C.c_uint32), ("n_inliers", C.c_uint32), ("status", C.c_int32), ("reserved", C.c_int32)]


# the same rows as numpy structured dtypes
START_FRAME_DTYPE = np.dtype([("sum_w", "<f8"), ("align_rms", "<f8"), ("eig", "<f8", (2,)), ("sum_xx", "<f8"), ("sum_yy", "<f8"),
                              ("n_obs", "<u4"), ("n_inliers", "<u4"), ("n_groups", "<u4"), ("n_used", "<u4"), ("status", "<i4"), ("reserved", "<i4")])
START_GROUP_DTYPE = np.dtype([("xyz", "<f8", (3,)), ("rms_px", "<f8"), ("fr", "<u4"), ("pt", "<u4"), ("n_obs", "<u4"), ("status", "<i4")])
START_POINT_DTYPE = np.dtype([("sum_xx", "<f8"), ("sum_yy", "<f8"), ("min_pivot", "<f8"), ("n_obs", "<u4"), ("n_inliers", "<u4"), ("status", "<i4"), ("reserved", "<i4")])

# every symbol include/lifcal_start.h declares
START_PROTOTYPES = {
    "lifcal_start_poses": (C.c_int, [C.POINTER(ResectProblem), C.POINTER(Options), C.c_double, C.c_double, C.c_void_p, C.c_void_p, uptr, dptr]),
    "lifcal_start_points": (C.c_int, [C.POINTER(IntersectProblem), C.POINTER(Options), C.c_double, C.c_void_p, dptr]),
}

class RegisterProblem(C.Structure):     # include/lifcal_register.h lifcal_register_problem
    _fields_ = [("n_obs", C.c_uint32), ("n_frames", C.c_uint32), ("n_points", C.c_uint32), ("reserved", C.c_uint32),
                ("u", dptr), ("v", dptr), ("mcx", dptr), ("mcy", dptr), ("pt", uptr), ("fr", uptr),
                ("cam", dptr), ("views", dptr), ("pts", dptr),
                ("spx", C.c_double), ("spy", C.c_double), ("scale", C.c_double), ("config", C.c_uint32)]


class RegisterOptions(C.Structure):     # lifcal_register_options
    _fields_ = [("gate_px", C.c_double), ("inlier_threshold", C.c_double), ("min_shared", C.c_uint32), ("anchor_frame", C.c_int32),
                ("anchor_view", dptr), ("max_rounds", C.c_uint32), ("reserved", C.c_uint32)]


class RegisterFrame(C.Structure):       # lifcal_register_frame: one 64-byte row per frame
    _fields_ = [("sum_xx", C.c_double), ("sum_yy", C.c_double), ("final_cost", C.c_double),
                ("n_obs", C.c_uint32), ("n_obs_used", C.c_uint32), ("n_inliers", C.c_uint32), ("n_groups", C.c_uint32), ("n_used", C.c_uint32),
                ("n_shared", C.c_uint32), ("status", C.c_int32), ("round", C.c_int32), ("iterations", C.c_int32), ("termination", C.c_int32)]


class RegisterPoint(C.Structure):       # lifcal_register_point: one 56-byte row per point
    _fields_ = [("sum_xx", C.c_double), ("sum_yy", C.c_double), ("final_cost", C.c_double),
                ("n_obs", C.c_uint32), ("n_obs_used", C.c_uint32), ("n_inliers", C.c_uint32), ("n_frames_used", C.c_uint32),
                ("status", C.c_int32), ("round", C.c_int32), ("iterations", C.c_int32), ("termination", C.c_int32)]


class RegisterSummary(C.Structure):     # lifcal_register_summary
    _fields_ = [("anchor_frame", C.c_int32), ("n_rounds", C.c_uint32), ("n_frames_registered", C.c_uint32), ("n_points_mapped", C.c_uint32),
                ("n_groups", C.c_uint32), ("n_groups_used", C.c_uint32)]


# the same rows as numpy structured dtypes
REGISTER_FRAME_DTYPE = np.dtype([("sum_xx", "<f8"), ("sum_yy", "<f8"), ("final_cost", "<f8"),
                                 ("n_obs", "<u4"), ("n_obs_used", "<u4"), ("n_inliers", "<u4"), ("n_groups", "<u4"), ("n_used", "<u4"),
                                 ("n_shared", "<u4"), ("status", "<i4"), ("round", "<i4"), ("iterations", "<i4"), ("termination", "<i4")])
REGISTER_POINT_DTYPE = np.dtype([("sum_xx", "<f8"), ("sum_yy", "<f8"), ("final_cost", "<f8"),
                                 ("n_obs", "<u4"), ("n_obs_used", "<u4"), ("n_inliers", "<u4"), ("n_frames_used", "<u4"),
                                 ("status", "<i4"), ("round", "<i4"), ("iterations", "<i4"), ("termination", "<i4")])

# every symbol include/lifcal_register.h declares
REGISTER_PROTOTYPES = {
    "lifcal_register_default_options": (None, [C.POINTER(RegisterOptions)]),
    "lifcal_register_scene": (C.c_int, [C.POINTER(RegisterProblem), C.POINTER(Options), C.POINTER(RegisterOptions), C.c_void_p, C.c_void_p,
                                        C.POINTER(RegisterSummary), dptr]),
}

class Priors(C.Structure):              # include/lifcal_prior.h lifcal_ba_priors
    _fields_ = [("cam_mean", dptr), ("cam_info", dptr), ("n_pose_priors", C.c_uint32), ("reserved", C.c_uint32),
                ("pose_frame", uptr), ("pose_mean", dptr), ("pose_info", dptr)]


class PointPriors(C.Structure):         # include/lifcal_prior.h lifcal_ba_point_priors
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("point", uptr), ("mean", dptr), ("info", dptr)]


class Alignment(C.Structure):           # include/lifcal_align.h lifcal_alignment
    _fields_ = [("scale", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3), ("rms", C.c_double),
                ("n_used", C.c_uint32), ("reserved", C.c_uint32)]


# every symbol include/lifcal_align.h declares
ALIGN_PROTOTYPES = {
    "lifcal_align_fit": (C.c_int, [C.c_uint32, dptr, dptr, dptr, C.c_int32, C.POINTER(Alignment)]),
    "lifcal_align_apply": (C.c_int, [C.POINTER(Alignment), C.c_uint32, dptr, C.c_uint64, dptr]),
}


class GridImage(C.Structure):           # include/lifcal_grid.h lifcal_grid_image
    _fields_ = [("data", C.c_void_p), ("bits", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int64)]


class GridCentre(C.Structure):          # lifcal_grid_centre: one 48-byte row per lens
    _fields_ = [("cx", C.c_double), ("cy", C.c_double), ("sum_w", C.c_int64), ("sum_wx", C.c_int64), ("sum_wy", C.c_int64), ("peak", C.c_int64)]


GRID_CENTRE_DTYPE = np.dtype([("cx", "<f8"), ("cy", "<f8"), ("sum_w", "<i8"), ("sum_wx", "<i8"), ("sum_wy", "<i8"), ("peak", "<i8")])


class GridCentres(C.Structure):         # lifcal_grid_centres
    _fields_ = [("capacity", C.c_uint64), ("n", C.c_uint64), ("c", C.c_void_p)]


class GridLens(C.Structure):            # lifcal_grid_lens: one 32-byte row per centre
    _fields_ = [("sub", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("accepted", C.c_int32), ("dx", C.c_double), ("dy", C.c_double)]


GRID_LENS_DTYPE = np.dtype([("sub", "<i4"), ("x", "<i4"), ("y", "<i4"), ("accepted", "<i4"), ("dx", "<f8"), ("dy", "<f8")])


class GridReport(C.Structure):          # lifcal_grid_report
    _fields_ = [("capacity", C.c_uint64), ("lens", C.c_void_p), ("n_centres", C.c_uint64), ("n_accepted", C.c_uint64),
                ("n_rejected_label", C.c_uint64), ("n_rejected_residual", C.c_uint64), ("rms", C.c_double), ("max_residual", C.c_double),
                ("lattice_a", C.c_double * 2), ("lattice_b", C.c_double * 2), ("lattice_c", C.c_double * 2),
                ("lens_diameter", C.c_double), ("rotation", C.c_double), ("lens_base_y", C.c_double * 2), ("origin", C.c_double * 2)]


# every symbol include/lifcal_grid.h declares
GRID_PROTOTYPES = {
    "lifcal_grid_detect": (C.c_int, [C.POINTER(GridImage), C.c_double, C.c_int32, C.POINTER(GridCentres)]),
    "lifcal_grid_fit_centres": (C.c_int, [C.c_uint64, dptr, dptr, C.c_int32, C.c_int32, C.c_double, C.c_double, C.POINTER(MlaParams), C.POINTER(GridReport)]),
    "lifcal_grid_fit": (C.c_int, [C.POINTER(GridImage), C.c_double, C.c_double, C.c_int32, C.POINTER(MlaParams), C.POINTER(GridCentres), C.POINTER(GridReport)]),
}

class RawDepthImage(C.Structure):       # include/lifcal_rawdepth.h lifcal_rawdepth_image
    _fields_ = [("data", C.c_void_p), ("bits", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("on_device", C.c_int32), ("pitch", C.c_int64)]


class RawDepthOptions(C.Structure):     # lifcal_rawdepth_options
    _fields_ = [("n_hyp", C.c_int32), ("patch_radius", C.c_int32), ("min_neighbours", C.c_int32), ("min_contrast", C.c_int32),
                ("iv_min", C.c_double), ("iv_max", C.c_double), ("max_baseline", C.c_double), ("ambiguity_ratio", C.c_double)]


class RawDepthPlan(C.Structure):        # lifcal_rawdepth_plan
    _fields_ = [("options", RawDepthOptions), ("n_neighbours", C.c_int32), ("window", C.c_int32), ("lds_bytes", C.c_int32), ("reserved", C.c_int32)]


class RawDepthResult(C.Structure):      # lifcal_rawdepth_result
    _fields_ = [("out_on_device", C.c_int32), ("n_neighbours_used", C.c_int32), ("inv_depth", C.c_void_p), ("cost", C.c_void_p),
                ("status", C.c_void_p), ("n_neighbours", C.c_void_p), ("count", C.c_uint64 * 5), ("seconds", C.c_double)]


class RawDepthPointList(C.Structure):   # lifcal_rawdepth_point_list
    _fields_ = [("inv_depth", C.c_void_p), ("on_device", C.c_int32), ("depth_to_raw_im_scale", C.c_int32), ("capacity", C.c_uint64), ("n", C.c_uint64),
                ("x", dptr), ("y", dptr), ("vdepth", dptr), ("src", uptr), ("lens", _iptr)]


# every symbol include/lifcal_rawdepth.h declares
RAWDEPTH_PROTOTYPES = {
    "lifcal_rawdepth_check": (C.c_int, [C.POINTER(MlaParams), C.POINTER(RawDepthImage), C.POINTER(RawDepthOptions), C.POINTER(RawDepthPlan)]),
    "lifcal_rawdepth_estimate": (C.c_int, [C.c_void_p, C.POINTER(RawDepthImage), C.POINTER(RawDepthOptions), C.POINTER(RawDepthResult)]),
    "lifcal_rawdepth_points": (C.c_int, [C.c_void_p, C.POINTER(RawDepthPointList)]),
}

class DepthMapOptions(C.Structure):     # include/lifcal_depthmap.h lifcal_depthmap_options
    _fields_ = [("scale", C.c_int32), ("out_width", C.c_int32), ("out_height", C.c_int32), ("min_support", C.c_int32), ("fill_rounds", C.c_int32),
                ("fill_min_neighbours", C.c_int32), ("tol_iv", C.c_double), ("iv_min", C.c_double)]


class DepthMapPlan(C.Structure):        # lifcal_depthmap_plan
    _fields_ = [("options", DepthMapOptions), ("out_width", C.c_int32), ("out_height", C.c_int32), ("tq", C.c_int32), ("max_side", C.c_int32),
                ("max_samples_per_cell", C.c_int64)]


class DepthMapResult(C.Structure):      # lifcal_depthmap_result
    _fields_ = [("out_on_device", C.c_int32), ("reserved", C.c_int32), ("inv_depth", C.c_void_p), ("depth16", C.c_void_p), ("status", C.c_void_p),
                ("support", C.c_void_p), ("count", C.c_uint64 * 4), ("n_samples", C.c_uint64), ("seconds", C.c_double)]


# every symbol include/lifcal_depthmap.h declares
DEPTHMAP_PROTOTYPES = {
    "lifcal_depthmap_check": (C.c_int, [C.POINTER(MlaParams), C.c_int32, C.c_int32, C.POINTER(DepthMapOptions), C.POINTER(DepthMapPlan)]),
    "lifcal_depthmap_from_raw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(DepthMapOptions), C.POINTER(DepthMapResult)]),
}

class TotalFocusOptions(C.Structure):   # include/lifcal_totalfocus.h lifcal_totalfocus_options
    _fields_ = [("scale", C.c_int32), ("out_width", C.c_int32), ("out_height", C.c_int32), ("min_lenses", C.c_int32), ("white_level", C.c_int32),
                ("margin", C.c_double), ("max_reach", C.c_double), ("iv_min", C.c_double), ("default_iv", C.c_double)]


class TotalFocusPlan(C.Structure):      # lifcal_totalfocus_plan
    _fields_ = [("options", TotalFocusOptions), ("out_width", C.c_int32), ("out_height", C.c_int32), ("r_use", C.c_double),
                ("max_lenses_per_cell", C.c_int32), ("reserved", C.c_int32)]


class TotalFocusResult(C.Structure):    # lifcal_totalfocus_result
    _fields_ = [("out_on_device", C.c_int32), ("reserved", C.c_int32), ("image", C.c_void_p), ("n_lenses", C.c_void_p), ("status", C.c_void_p),
                ("count", C.c_uint64 * 4), ("seconds", C.c_double)]


# every symbol include/lifcal_totalfocus.h declares
TOTALFOCUS_PROTOTYPES = {
    "lifcal_totalfocus_check": (C.c_int, [C.POINTER(MlaParams), C.POINTER(RawDepthImage), C.POINTER(RawDepthImage), C.c_int32, C.c_int32,
                                          C.POINTER(TotalFocusOptions), C.POINTER(TotalFocusPlan)]),
    "lifcal_totalfocus_render": (C.c_int, [C.c_void_p, C.POINTER(RawDepthImage), C.POINTER(RawDepthImage), C.c_void_p, C.c_int32,
                                           C.POINTER(TotalFocusOptions), C.POINTER(TotalFocusResult)]),
}

class FeaturesOptions(C.Structure):     # include/lifcal_features.h lifcal_features_options
    _fields_ = [("win_r", C.c_int32), ("nms_r", C.c_int32), ("cell", C.c_int32), ("per_cell", C.c_int32), ("min_score", C.c_double)]


class FeaturesPlan(C.Structure):        # lifcal_features_plan
    _fields_ = [("options", FeaturesOptions), ("buckets_x", C.c_int32), ("buckets_y", C.c_int32), ("max_features", C.c_int64)]


class FeaturesList(C.Structure):        # lifcal_features_list
    _fields_ = [("capacity", C.c_uint64), ("n", C.c_uint64), ("x", dptr), ("y", dptr), ("ix", _iptr), ("iy", _iptr), ("score", dptr), ("desc", uptr),
                ("seconds", C.c_double)]


class FeaturesSet(C.Structure):         # lifcal_features_set
    _fields_ = [("n_frames", C.c_uint32), ("reserved", C.c_uint32), ("offset", uptr), ("desc", uptr), ("ix", _iptr), ("iy", _iptr)]


class MatchOptions(C.Structure):        # lifcal_match_options
    _fields_ = [("max_dist", C.c_int32), ("ratio_num", C.c_int32), ("ratio_den", C.c_int32), ("max_shift", C.c_int32)]


class MatchList(C.Structure):           # lifcal_match_list
    _fields_ = [("capacity", C.c_uint64), ("n", C.c_uint64), ("pair_start", C.POINTER(C.c_uint64)), ("i", uptr), ("j", uptr), ("dist", uptr),
                ("seconds", C.c_double)]


class Tracks(C.Structure):              # lifcal_tracks
    _fields_ = [("min_length", C.c_uint32), ("n_tracks", C.c_uint32), ("n_conflicts", C.c_uint64), ("capacity", C.c_uint64), ("n", C.c_uint64),
                ("fr", uptr), ("pt", uptr), ("feature", uptr)]


# every symbol include/lifcal_features.h declares
FEATURES_PROTOTYPES = {
    "lifcal_features_check": (C.c_int, [C.POINTER(RawDepthImage), C.POINTER(FeaturesOptions), C.POINTER(FeaturesPlan)]),
    "lifcal_features_detect": (C.c_int, [C.POINTER(RawDepthImage), C.c_void_p, C.c_int32, C.POINTER(FeaturesOptions), C.POINTER(FeaturesList)]),
    "lifcal_features_pattern": (C.c_int, [C.POINTER(C.c_int8)]),
    "lifcal_features_match_check": (C.c_int, [C.POINTER(FeaturesSet), C.c_uint32, uptr, C.POINTER(MatchOptions), C.POINTER(MatchOptions)]),
    "lifcal_features_match": (C.c_int, [C.POINTER(FeaturesSet), C.c_uint32, uptr, C.c_int32, C.POINTER(MatchOptions), C.POINTER(MatchList)]),
    "lifcal_tracks_link": (C.c_int, [C.c_uint32, uptr, C.c_uint32, uptr, C.POINTER(C.c_uint64), uptr, uptr, C.POINTER(Tracks)]),
}

class VerifyPoints(C.Structure):        # include/lifcal_verify.h lifcal_verify_points
    _fields_ = [("n_frames", C.c_uint32), ("reserved", C.c_uint32), ("offset", uptr), ("xyz", dptr), ("tol_lat", dptr), ("tol_dep", dptr)]


class VerifyOptions(C.Structure):       # lifcal_verify_options
    _fields_ = [("hypotheses", C.c_uint32), ("seed", C.c_uint32), ("min_inliers", C.c_int32), ("refine", C.c_int32), ("min_ratio", C.c_double)]


class VerifyPair(C.Structure):          # lifcal_verify_pair
    _fields_ = [("status", C.c_uint32), ("n_matches", C.c_uint32), ("n_usable", C.c_uint32), ("best_hypothesis", C.c_uint32),
                ("n_inliers_hypothesis", C.c_uint32), ("n_inliers", C.c_uint32), ("rounds_used", C.c_uint32), ("reserved", C.c_uint32),
                ("R", C.c_double * 9), ("t", C.c_double * 3), ("rms", C.c_double)]


class VerifyResult(C.Structure):        # lifcal_verify_result
    _fields_ = [("keep", C.POINTER(C.c_uint8)), ("e_par", dptr), ("e_perp", dptr), ("pair", C.POINTER(VerifyPair)), ("seconds", C.c_double)]


_u64ptr = C.POINTER(C.c_uint64)

# every symbol include/lifcal_verify.h declares
VERIFY_PROTOTYPES = {
    "lifcal_matches_verify_check": (C.c_int, [C.POINTER(VerifyPoints), C.c_uint32, uptr, _u64ptr, uptr, uptr, C.POINTER(VerifyOptions),
                                              C.POINTER(VerifyOptions)]),
    "lifcal_matches_verify": (C.c_int, [C.POINTER(VerifyPoints), C.c_uint32, uptr, _u64ptr, uptr, uptr, C.c_int32, C.POINTER(VerifyOptions),
                                        C.POINTER(VerifyResult)]),
}

class MarkerDictionary(C.Structure):    # include/lifcal_markers.h lifcal_marker_dictionary
    _fields_ = [("marker_bits", C.c_int32), ("n", C.c_uint32), ("words", C.POINTER(C.c_uint64))]


class MarkersOptions(C.Structure):      # lifcal_markers_options
    _fields_ = [("w", C.c_int32), ("contrast", C.c_int32), ("cell_contrast", C.c_int32), ("min_area", C.c_int32), ("min_side", C.c_int32),
                ("max_side", C.c_int32), ("max_border_errors", C.c_int32), ("max_correction", C.c_int32), ("refine_max", C.c_double)]


class MarkersPlan(C.Structure):         # lifcal_markers_plan
    _fields_ = [("options", MarkersOptions), ("min_distance", C.c_int32), ("tiles_x", C.c_int32), ("tiles_y", C.c_int32), ("reserved", C.c_int32),
                ("max_candidates", C.c_int64)]


# lifcal_marker and lifcal_marker_component as numpy record types (the lists are arrays of these)
MARKER_DTYPE = np.dtype([("id", np.int32), ("rotation", np.int32), ("hamming", np.int32), ("refined", np.int32), ("label", np.int32), ("area", np.int32),
                         ("corners", np.float64, (4, 2)), ("x", np.float64), ("y", np.float64)], align=True)
MARKER_COMPONENT_DTYPE = np.dtype([("label", np.int32), ("area", np.int32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32),
                                   ("ext", np.int32, (8, 2))], align=True)


class MarkerList(C.Structure):          # lifcal_marker_list
    _fields_ = [("capacity", C.c_uint64), ("n", C.c_uint64), ("markers", C.c_void_p), ("n_candidates", C.c_uint64), ("seconds", C.c_double)]


class MarkerComponents(C.Structure):    # lifcal_marker_components
    _fields_ = [("dark", C.c_void_p), ("labels", C.c_void_p), ("capacity", C.c_uint64), ("n", C.c_uint64), ("comp", C.c_void_p), ("seconds", C.c_double)]


class Constraints(C.Structure):         # lifcal_constraints
    _fields_ = [("capacity", C.c_uint64), ("n", C.c_uint64), ("id1", uptr), ("id2", uptr), ("distance", dptr), ("sigma", dptr),
                ("ids_capacity", C.c_uint64), ("n_ids", C.c_uint64), ("ids", uptr)]


class MarkerSeeds(C.Structure):         # lifcal_marker_seeds
    _fields_ = [("capacity", C.c_uint64), ("n_ids", C.c_uint64), ("n_unseeded", C.c_uint64), ("ids", uptr), ("xyz", dptr), ("seeded", C.POINTER(C.c_uint8))]


# every symbol include/lifcal_markers.h declares
MARKERS_PROTOTYPES = {
    "lifcal_markers_check": (C.c_int, [C.POINTER(RawDepthImage), C.POINTER(MarkerDictionary), C.POINTER(MarkersOptions), C.POINTER(MarkersPlan)]),
    "lifcal_markers_detect": (C.c_int, [C.POINTER(RawDepthImage), C.c_void_p, C.c_int32, C.POINTER(MarkerDictionary), C.POINTER(MarkersOptions),
                                        C.POINTER(MarkerList)]),
    "lifcal_markers_components": (C.c_int, [C.POINTER(RawDepthImage), C.c_void_p, C.c_int32, C.POINTER(MarkersOptions), C.POINTER(MarkerComponents)]),
    "lifcal_marker_dictionary_distance": (C.c_int, [C.POINTER(MarkerDictionary), _iptr]),
    "lifcal_marker_dictionary_generate": (C.c_int, [C.c_int32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), _iptr]),
    "lifcal_constraints_read": (C.c_int, [C.c_char_p, C.POINTER(Constraints)]),
    "lifcal_markers_seed_points": (C.c_int, [C.c_uint64, dptr, dptr, uptr, uptr, C.c_uint64, dptr, dptr, uptr, uptr, C.c_uint64, dptr,
                                             C.POINTER(MarkerSeeds)]),
    "lifcal_scene_scale_factor": (C.c_int, [dptr, dptr, C.c_double, dptr]),
}

# every symbol include/lifcal_prior.h declares
PRIOR_PROTOTYPES = {
    "lifcal_ba_check_point_priors": (C.c_int, [C.c_uint32, C.POINTER(PointPriors)]),
    "lifcal_ba_create_with_point_priors": (C.c_int, [C.c_void_p, C.POINTER(PointPriors), C.c_void_p, C.POINTER(C.c_void_p)]),
    "lifcal_ba_set_point_priors": (C.c_int, [C.c_void_p, C.POINTER(PointPriors)]),
    "lifcal_ba_point_prior_cost": (C.c_int, [C.c_void_p, dptr]),
    "lifcal_ba_check_priors": (C.c_int, [C.c_uint32, C.POINTER(Priors)]),
    "lifcal_ba_set_priors": (C.c_int, [C.c_void_p, C.POINTER(Priors)]),
    "lifcal_ba_prior_cost": (C.c_int, [C.c_void_p, dptr, dptr]),
    "lifcal_prior_from_covariance": (C.c_int, [dptr, C.c_uint32, C.c_uint64, C.c_double, dptr, uptr]),
}


class PriorArrays:
    """Owns contiguous copies of the arrays of a lifcal_ba_priors and the ctypes struct that points into them.
    camera = (mean[17], info[17, 17]) or None; poses = (frames[n], means[n, 6], infos[n, 6, 6]) or None."""

    def __init__(self, camera=None, poses=None):
        f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)).copy()
        p = Priors()
        self.cam_mean = self.cam_info = self.pose_frame = self.pose_mean = self.pose_info = None
        if camera is not None:
            self.cam_mean, self.cam_info = f8(camera[0]), f8(camera[1])
            if self.cam_mean.shape[0] != 17 or self.cam_info.shape[0] != 17 * 17:
                raise ValueError("camera prior: mean[17] and info[17, 17]")
            p.cam_mean, p.cam_info = as_dptr(self.cam_mean), as_dptr(self.cam_info)
        if poses is not None:
            self.pose_frame = np.ascontiguousarray(np.asarray(poses[0], dtype=np.uint32).reshape(-1)).copy()
            self.pose_mean, self.pose_info = f8(poses[1]), f8(poses[2])
            n = self.pose_frame.shape[0]
            if self.pose_mean.shape[0] != 6 * n or self.pose_info.shape[0] != 36 * n:
                raise ValueError("pose priors: frames[n], means[n, 6] and infos[n, 6, 6]")
            p.n_pose_priors = n
            p.pose_frame, p.pose_mean, p.pose_info = as_uptr(self.pose_frame), as_dptr(self.pose_mean), as_dptr(self.pose_info)
        self.struct = p


class PointPriorArrays:
    """Owns contiguous copies of the arrays of a lifcal_ba_point_priors: ids[n] strictly ascending, means[n, 3], infos[n, 3, 3]."""

    def __init__(self, ids, means, infos):
        self.point = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1)).copy()
        self.mean = np.ascontiguousarray(np.asarray(means, dtype=np.float64).reshape(-1)).copy()
        self.info = np.ascontiguousarray(np.asarray(infos, dtype=np.float64).reshape(-1)).copy()
        n = self.point.shape[0]
        if self.mean.shape[0] != 3 * n or self.info.shape[0] != 9 * n:
            raise ValueError("point priors: ids[n], means[n, 3] and infos[n, 3, 3]")
        p = PointPriors()
        p.n = n
        p.point, p.mean, p.info = as_uptr(self.point), as_dptr(self.mean), as_dptr(self.info)
        self.struct = p


# every symbol include/lifcal_ba.h declares: name -> (restype, argtypes)
PROTOTYPES = {
    "lifcal_ba_default_options": (None, [C.POINTER(Options)]),
    "lifcal_ba_create": (C.c_int, [C.POINTER(Problem), C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "lifcal_ba_solve": (C.c_int, [C.c_void_p, C.POINTER(Summary)]),
    "lifcal_ba_sweep": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(SweepOut)]),
    "lifcal_ba_sweep_enqueue": (C.c_int, [C.c_void_p, C.c_double]),
    "lifcal_ba_profile_begin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "lifcal_ba_profile_begin_sampled": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "lifcal_ba_profile_end": (C.c_int, [C.c_void_p, C.POINTER(Profile)]),
    "lifcal_ba_reproj_stats": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(Stats)]),
    "lifcal_ba_project_observations": (C.c_int, [C.c_void_p, dptr, dptr]),
    "lifcal_ba_set_fixed_frames": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    "lifcal_ba_default_covariance_options": (None, [C.POINTER(CovarianceOptions)]),
    "lifcal_ba_covariance": (C.c_int, [C.c_void_p, C.POINTER(CovarianceOptions), C.POINTER(CovarianceOut)]),
    "lifcal_ba_residual_report": (C.c_int, [C.c_void_p, C.POINTER(ResidualReportIO)]),
    "lifcal_ba_residual_groups": (C.c_int, [C.c_void_p, C.c_double, C.c_uint32, uptr, C.c_void_p]),
    "lifcal_ba_object_space_stats": (C.c_int, [C.c_void_p, C.c_uint64, dptr, dptr, dptr, uptr, uptr, dptr, dptr, C.POINTER(ObjectSpace)]),
    "lifcal_ba_solve_windowed": (C.c_int, [C.POINTER(Problem), C.POINTER(Options), C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(WindowReport), C.POINTER(C.c_uint32)]),
    "lifcal_ba_upload_parameters": (C.c_int, [C.c_void_p]),
    "lifcal_ba_download_parameters": (C.c_int, [C.c_void_p]),
    "lifcal_ba_set_allreduce": (C.c_int, [C.c_void_p, ALLREDUCE_FN, C.c_void_p]),
    "lifcal_ba_set_allgather": (C.c_int, [C.c_void_p, ALLGATHER_FN, C.c_void_p]),
    "lifcal_ba_comm_unique_id": (C.c_int, [C.c_void_p]),
    "lifcal_ba_comm_init_rccl": (C.c_int, [C.c_void_p, C.c_void_p]),
    "lifcal_ba_get_info": (C.c_int, [C.c_void_p, C.POINTER(Info)]),
    "lifcal_ba_debug_step": (C.c_int, [C.c_void_p, C.POINTER(StepOut)]),
    "lifcal_ba_destroy": (None, [C.c_void_p]),
    "lifcal_init_plenoptic": (C.c_int, [C.POINTER(InitProblem), C.c_int32, C.POINTER(InitResult)]),
    "lifcal_init_plenoptic_recalibration": (C.c_int, [C.c_double, C.c_double, C.POINTER(InitResult)]),
    "lifcal_ba_strerror": (C.c_char_p, [C.c_int]),
    "lifcal_ba_last_error": (C.c_char_p, []),
    "lifcal_ba_version": (C.c_char_p, []),
    "lifcal_ba_plan": (C.c_int, [C.POINTER(Problem), C.c_int32, C.c_int32, C.POINTER(PlanInfo), uptr, uptr]),
    "lifcal_ba_plan_stats": (C.c_int, [C.POINTER(Problem), C.c_int32, C.c_int32, C.POINTER(PlanStats)]),
    "lifcal_ba_plan_shape": (C.c_int, [C.POINTER(Problem), C.c_int32, C.c_int32, C.POINTER(PlanShape)]),
    "lifcal_ba_partition_points": (C.c_int, [C.POINTER(Problem), C.POINTER(Partition)]),
    "lifcal_ba_create_shard": (C.c_int, [C.POINTER(Problem), C.POINTER(Partition), C.POINTER(Options), C.POINTER(C.c_void_p)]),
    "lifcal_ba_plan_shard": (C.c_int, [C.POINTER(Problem), C.POINTER(Partition), C.c_int32, C.POINTER(PlanInfo)]),
}

# host-only helpers of include/lifcal_ba.h outside the lifcal_ba_ / lifcal_init_ families
HOST_PROTOTYPES = {
    "lifcal_group_index": (C.c_int, [C.c_uint32, C.c_uint32, uptr, uptr, uptr]),
}

_lib = None


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load the HIP extension.  Fails loudly: there is no Python/CPU fallback for the hot path."""
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise RuntimeError(
                f"lifcal_amd: native library {path} is missing. Build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the bundle-adjustment path.")
        lib = C.CDLL(path)
        for name, (res, args) in list(PROTOTYPES.items()) + list(MLA_PROTOTYPES.items()) + list(IO_PROTOTYPES.items()) + list(COLMAP_PROTOTYPES.items()) + list(DEPTH_PROTOTYPES.items()) + list(HOST_PROTOTYPES.items()) + list(RESECT_PROTOTYPES.items()) + list(INTERSECT_PROTOTYPES.items()) + list(START_PROTOTYPES.items()) + list(REGISTER_PROTOTYPES.items()) + list(PRIOR_PROTOTYPES.items()) + list(ALIGN_PROTOTYPES.items()) + list(GRID_PROTOTYPES.items()) + list(RAWDEPTH_PROTOTYPES.items()) + list(DEPTHMAP_PROTOTYPES.items()) + list(TOTALFOCUS_PROTOTYPES.items()) + list(FEATURES_PROTOTYPES.items()) + list(VERIFY_PROTOTYPES.items()) + list(MARKERS_PROTOTYPES.items()):
            fn = getattr(lib, name)   # AttributeError if a declared symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def as_dptr(a: np.ndarray):
    return a.ctypes.data_as(dptr) if a is not None else None


def as_uptr(a: np.ndarray):
    return a.ctypes.data_as(uptr) if a is not None else None


class ProblemArrays:
    """Owns contiguous numpy buffers and the ctypes struct that points into them."""

    def __init__(self, u, v, mcx, mcy, pt, fr, cam, views, pts, spx, scale, config, spy=None,
                 fixed_mask=0, lower=None, upper=None, c_i=None, c_j=None, c_dist=None, c_sigma=None,
                 use_constraints=1):
        f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
        u4 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
        self.u, self.v, self.mcx, self.mcy = f8(u), f8(v), f8(mcx), f8(mcy)
        self.pt, self.fr = u4(pt), u4(fr)
        self.cam = f8(cam).copy()
        self.views = f8(views).copy()
        self.pts = f8(pts).copy()
        assert self.cam.shape[0] == 17
        self.lower = f8(lower) if lower is not None else None
        self.upper = f8(upper) if upper is not None else None
        m = 0 if c_i is None else len(np.asarray(c_i).reshape(-1))
        self.c_i = u4(c_i) if m else None
        self.c_j = u4(c_j) if m else None
        self.c_dist = f8(c_dist) if m else None
        self.c_sigma = f8(c_sigma) if m else None
        p = Problem()
        p.n_obs = self.u.shape[0]
        p.n_frames = self.views.shape[0] // 6
        p.n_points = self.pts.shape[0] // 3
        p.n_constraints = m
        p.u, p.v, p.mcx, p.mcy = as_dptr(self.u), as_dptr(self.v), as_dptr(self.mcx), as_dptr(self.mcy)
        p.pt, p.fr = as_uptr(self.pt), as_uptr(self.fr)
        p.cam, p.views, p.pts = as_dptr(self.cam), as_dptr(self.views), as_dptr(self.pts)
        p.spx = float(spx)
        p.spy = float(spx if spy is None else spy)
        p.scale = float(scale)
        p.config = int(config)
        p.fixed_mask = int(fixed_mask)
        p.lower = as_dptr(self.lower) if self.lower is not None else None
        p.upper = as_dptr(self.upper) if self.upper is not None else None
        p.c_i = as_uptr(self.c_i) if m else None
        p.c_j = as_uptr(self.c_j) if m else None
        p.c_dist = as_dptr(self.c_dist) if m else None
        p.c_sigma = as_dptr(self.c_sigma) if m else None
        p.use_constraints = int(use_constraints)
        self.struct = p

    @classmethod
    def from_scene(cls, scene, initial=True):
        return cls(scene.u, scene.v, scene.mcx, scene.mcy, scene.pt, scene.fr,
                   scene.cam0 if initial else scene.cam_gt,
                   scene.views0 if initial else scene.views_gt,
                   scene.pts0 if initial else scene.pts_gt,
                   scene.spx, scene.scale, scene.config, fixed_mask=scene.fixed_mask,
                   lower=scene.lower, upper=scene.upper, c_i=scene.c_i, c_j=scene.c_j,
                   c_dist=scene.c_dist, c_sigma=scene.c_sigma, use_constraints=scene.use_constraints)


def default_options_py() -> Options:
    """The same defaults lifcal_ba_default_options() writes (used when the .so is not needed)."""
    o = Options()
    o.function_tolerance = 1e-6
    o.parameter_tolerance = 1e-8
    o.gradient_tolerance = 1e-10
    o.initial_radius = 1e4
    o.max_radius = 1e16
    o.min_radius = 1e-32
    o.min_relative_decrease = 1e-3
    o.min_lm_diagonal = 1e-6
    o.max_lm_diagonal = 1e32
    o.loss_scale = 0.5
    o.max_iterations = 200
    o.jacobi_scaling = 1
    o.precision = 0
    o.device = 0
    o.rank = 0
    o.world_size = 1
    o.verbose = 0
    o.deterministic = 0
    return o
