"""Host-side mirror of LiFCal's bundle-adjustment seam on top of the C ABI (include/lifcal_ba.h).

Names follow the reference (src/CameraCalibration.{h,cpp}):
    performBundleAdjustment()  <- CameraCalibration::performBundleAdjustment  (:774-992)
    calcReprojectionError()    <- CameraCalibration::calcReprojectionError    (:1026-1103)
    make_config()              <- the config bitmask assembly                  (:778-814)
The arithmetic lives in the HIP library; this file only flattens arguments and forwards them.
There is no Python/CPU fallback: if the library is missing, loading raises.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi as capi


def make_config(nRadialDistParam=2, tangentialDistParam=True, refinePoses=True, useRobustCostFunction=True,
                refine3Dpoints=True, mlCenterAdjustment=True) -> int:
    """reference src/CameraCalibration.cpp:778-814 (nRadialDistParam is clamped to 2 at :786)."""
    cfg = min(int(nRadialDistParam), 2) & 0x3
    if tangentialDistParam:
        cfg |= 0x004
    if refinePoses:
        cfg |= 0x100
    if useRobustCostFunction:
        cfg |= 0x200
    if refine3Dpoints:
        cfg |= 0x400
    if mlCenterAdjustment:
        cfg |= 0x800
    return cfg


class LifcalError(RuntimeError):
    pass


def _check(lib, rc, what):
    if rc != 0:
        err = LifcalError(f"{what}: {lib.lifcal_ba_strerror(rc).decode()} ({rc}) {lib.lifcal_ba_last_error().decode()}")
        err.code = rc   # the lifcal_ba_status value
        raise err


@dataclass
class Covariance:
    """Covariance of the calibrated parameters (BundleAdjustment.covariance, include/lifcal_ba.h lifcal_ba_covariance).

    camera       17 x 17 block of G = H^- (Ceres units: unit-variance pixel residuals unless scaled by sigma2)
    camera_std   sqrt of its diagonal; NaN where the slot is free but not determined by the data, 0 where it is fixed or absent
    estimable    17 bools: free slots whose variance does not depend on the gauge / null-space choice
    null_rank    null directions left after the gauge frame (e.g. the B / bL0 direction of an unconstrained scene)
    camera_null  null_rank x 17: camera components of those directions, parameter units
    poses        F x 6 x 6 blocks relative to the gauge frame, or None
    gauge_frame  the frame held constant for the computation, or -1
    sigma2       2 cost / (m - r): the residual variance estimate (an approximation under the Cauchy loss)
    """
    camera: np.ndarray
    camera_std: np.ndarray
    estimable: np.ndarray
    null_rank: int
    camera_null: np.ndarray
    poses: Optional[np.ndarray]
    gauge_frame: int
    sigma2: float
    live: np.ndarray
    pose_band: Optional[np.ndarray] = None
    seconds: float = 0.0
    cost: float = 0.0

    def camera_information(self, rcond: float = 1e-9):
        """(info[17, 17], rank): the camera block as the information matrix of a prior (BundleAdjustment.set_priors(camera=(mean,
        info))): the pseudo-inverse over the estimable slots, zero rows and columns elsewhere (prior_from_covariance)."""
        mask = sum(1 << j for j in range(17) if self.estimable[j])
        return prior_from_covariance(self.camera, mask, rcond)


def check_priors(n_frames: int, camera=None, poses=None):
    """Host-only check of a set of priors (lifcal_ba_check_priors): raises LifcalError with .code LIFCAL_BA_ERR_INVALID_ARG (-1)
    or LIFCAL_BA_ERR_OUT_OF_RANGE (-4); arguments as BundleAdjustment.set_priors."""
    lib = capi.load_library()
    arrs = capi.PriorArrays(camera, poses)
    _check(lib, lib.lifcal_ba_check_priors(int(n_frames), C.byref(arrs.struct)), "lifcal_ba_check_priors")


def check_point_priors(n_points: int, ids, means, infos):
    """Host-only check of a set of point priors (lifcal_ba_check_point_priors): raises LifcalError with .code
    LIFCAL_BA_ERR_INVALID_ARG (-1) or LIFCAL_BA_ERR_OUT_OF_RANGE (-4); ids[n] strictly ascending, means[n, 3], infos[n, 3, 3]."""
    lib = capi.load_library()
    arrs = capi.PointPriorArrays(ids, means, infos)
    _check(lib, lib.lifcal_ba_check_point_priors(int(n_points), C.byref(arrs.struct)), "lifcal_ba_check_point_priors")


@dataclass
class Alignment:
    """to ~ scale * R from + t (lifcal_align_fit): rms over the n_used points with a positive weight."""
    scale: float
    R: np.ndarray
    t: np.ndarray
    rms: float
    n_used: int

    def _struct(self):
        a = capi.Alignment()
        a.scale = float(self.scale); a.rms = float(self.rms); a.n_used = int(self.n_used)
        a.R[:] = [float(x) for x in np.asarray(self.R, np.float64).reshape(9)]
        a.t[:] = [float(x) for x in np.asarray(self.t, np.float64).reshape(3)]
        return a


def alignFit(src, dst, weights=None, with_scale: bool = True) -> Alignment:
    """Weighted closed-form dst ~ s R src + t over points src[n, 3], dst[n, 3] (Horn's quaternion method, lifcal_align_fit);
    with_scale False forces s = 1.  LifcalError (.code -1) for fewer than three weighted points, collinear points on either side, non-finite input; ValueError for
    arrays whose shapes disagree."""
    lib = capi.load_library()
    a = np.ascontiguousarray(np.asarray(src, np.float64).reshape(-1, 3))
    b = np.ascontiguousarray(np.asarray(dst, np.float64).reshape(-1, 3))
    if a.shape != b.shape:
        raise ValueError("alignFit: src[n, 3] and dst[n, 3]")
    w = None if weights is None else np.ascontiguousarray(np.asarray(weights, np.float64).reshape(-1))
    if w is not None and w.shape[0] != a.shape[0]:
        raise ValueError("alignFit: weights[n]")
    out = capi.Alignment()
    _check(lib, lib.lifcal_align_fit(a.shape[0], capi.as_dptr(a), capi.as_dptr(b), capi.as_dptr(w), 1 if with_scale else 0, C.byref(out)), "lifcal_align_fit")
    return Alignment(out.scale, np.array(out.R[:]).reshape(3, 3), np.array(out.t[:]), out.rms, out.n_used)


def alignApply(alignment: Alignment, views, pts):
    """(views', pts'): the scene moved by the alignment (lifcal_align_apply): P' = s R P + t, R_f' = R_f R^T, t_f' = s t_f - R_f' t.
    Copies; views[F, 6] and pts[P, 3] (either may be None)."""
    lib = capi.load_library()
    v = None if views is None else np.ascontiguousarray(np.asarray(views, np.float64).reshape(-1, 6)).copy()
    p = None if pts is None else np.ascontiguousarray(np.asarray(pts, np.float64).reshape(-1, 3)).copy()
    a = alignment._struct()
    _check(lib, lib.lifcal_align_apply(C.byref(a), 0 if v is None else v.shape[0], capi.as_dptr(v), 0 if p is None else p.shape[0], capi.as_dptr(p)), "lifcal_align_apply")
    return v, p


def alignScene(problem_arrays, ids, coords, with_scale: bool = True, weights=None) -> Alignment:
    """Moves the start values of a capi.ProblemArrays (views and pts, in place) onto control points: fits the current coordinates of
    the points `ids` to `coords[n, 3]` and applies the result to every pose and point.  Returns the Alignment."""
    ids = np.asarray(ids, np.int64).reshape(-1)
    pts = problem_arrays.pts.reshape(-1, 3)
    al = alignFit(pts[ids], coords, weights, with_scale)
    v, p = alignApply(al, problem_arrays.views, problem_arrays.pts)
    problem_arrays.views[:] = v.reshape(-1)
    problem_arrays.pts[:] = p.reshape(-1)
    return al


def prior_from_covariance(cov, use_mask: int, rcond: float = 1e-9):
    """(info, rank): pseudo-inverse of the sub-matrix of the n x n covariance selected by the bits of use_mask, zero rows and
    columns elsewhere; eigenvalues below rcond * lambda_max of the Jacobi-scaled sub-matrix count as null
    (lifcal_prior_from_covariance).  Host only."""
    lib = capi.load_library()
    a = np.ascontiguousarray(np.asarray(cov, dtype=np.float64))
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise LifcalError("prior_from_covariance: a square matrix")
    info = np.zeros_like(a)
    rank = np.zeros(1, np.uint32)
    _check(lib, lib.lifcal_prior_from_covariance(capi.as_dptr(a), a.shape[0], int(use_mask), float(rcond), capi.as_dptr(info), capi.as_uptr(rank)),
           "lifcal_prior_from_covariance")
    return info, int(rank[0])


class GroupTable:
    """One table of the residual report: `rows` is a structured array of capi.GROUP_STATS_DTYPE (sum_x, sum_y, sum_xx, sum_yy,
    sum_w, max_abs_x, max_abs_y, n, n_inliers), one row per group; an empty group is an all-zero row and its derived values are NaN."""

    def __init__(self, rows: np.ndarray):
        self.rows = rows

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, name):
        return self.rows[name]

    def _per_n(self, v):
        n = self.rows["n"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, v / n, np.nan)

    @property
    def n(self):
        return self.rows["n"]

    @property
    def n_inliers(self):
        return self.rows["n_inliers"]

    @property
    def mean_x(self):
        return self._per_n(self.rows["sum_x"])

    @property
    def mean_y(self):
        return self._per_n(self.rows["sum_y"])

    @property
    def rms_x(self):
        """sqrt(sum e_x^2 / n): not mean-removed, as calcReprojectionError defines its std_x (reference :1097)"""
        return np.sqrt(self._per_n(self.rows["sum_xx"]))

    @property
    def rms_y(self):
        return np.sqrt(self._per_n(self.rows["sum_yy"]))

    @property
    def mean_weight(self):
        return self._per_n(self.rows["sum_w"])


@dataclass
class ResidualReport:
    """BundleAdjustment.residualReport: e = projected - observed in raw pixels at the device-resident parameters.

    ex, ey, weight, lens   per observation in the caller's order (None without per_observation); weight is the Cauchy loss weight
                           1 / (1 + |e|^2 / loss_scale^2), 1 when the loss is off; lens is the lens id, an index into lens_xy
    lens_xy                (n_lenses, 2): the micro-lens centre (mcx, mcy) of every lens id
    per_frame, per_point, per_lens, total   GroupTable (total has one row)
    """
    ex: Optional[np.ndarray]
    ey: Optional[np.ndarray]
    weight: Optional[np.ndarray]
    lens: Optional[np.ndarray]
    lens_xy: np.ndarray
    per_frame: GroupTable
    per_point: GroupTable
    per_lens: GroupTable
    total: GroupTable
    inlier_threshold: float
    seconds: float


def sensor_cells(u, v, cell_px: float, raw_width: int, raw_height: int):
    """Key for a residual map over the sensor (BundleAdjustment.residualGroups): the raw image is cut into square cells of cell_px
    pixels, row-major; returns (key, n_keys, (cells_y, cells_x)).  Observations outside the image go to the nearest border cell."""
    nx = max(1, int(np.ceil(raw_width / cell_px))); ny = max(1, int(np.ceil(raw_height / cell_px)))
    cx = np.clip(np.floor(np.asarray(u, np.float64) / cell_px), 0, nx - 1).astype(np.uint32)
    cy = np.clip(np.floor(np.asarray(v, np.float64) / cell_px), 0, ny - 1).astype(np.uint32)
    return cy * np.uint32(nx) + cx, nx * ny, (ny, nx)


class BundleAdjustment:
    """One bundle-adjustment problem resident on one MI355X (one rank of a point-sharded job)."""

    def __init__(self, problem: capi.ProblemArrays, options: Optional[capi.Options] = None, partition: Optional["capi.PartitionArrays"] = None,
                 point_priors=None):
        """partition: `problem` is the rank's SHARD (only the observations of the points it owns, see capi.PartitionArrays.shard_of)
        and the handle is made with lifcal_ba_create_shard; None: the whole problem, lifcal_ba_create.
        point_priors = (ids[n] strictly ascending, means[n, 3], infos[n, 3, 3]): control points, the handle is made with
        lifcal_ba_create_with_point_priors and keeps this point set (set_point_priors replaces the values); not with a partition."""
        self.lib = capi.load_library()
        self.problem = problem
        if options is None:
            options = capi.Options()
            self.lib.lifcal_ba_default_options(C.byref(options))
        self.options = options
        self._h = C.c_void_p()
        self._hook = None
        self._partition = partition
        if point_priors is not None:
            if partition is not None:
                err = LifcalError("point priors are not supported on a shard handle (lifcal_ba_create_shard)")
                err.code = -1
                raise err
            arrs = capi.PointPriorArrays(*point_priors) if len(point_priors) else None   # (): a NULL prior set, exactly lifcal_ba_create
            _check(self.lib, self.lib.lifcal_ba_create_with_point_priors(C.byref(problem.struct), C.byref(arrs.struct) if arrs else None, C.byref(options), C.byref(self._h)),
                   "lifcal_ba_create_with_point_priors")
        elif partition is not None:
            _check(self.lib, self.lib.lifcal_ba_create_shard(C.byref(problem.struct), C.byref(partition.struct), C.byref(options), C.byref(self._h)), "lifcal_ba_create_shard")
        else:
            _check(self.lib, self.lib.lifcal_ba_create(C.byref(problem.struct), C.byref(options), C.byref(self._h)), "lifcal_ba_create")

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if self._h:
            self.lib.lifcal_ba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- the reference's two entry points ------------------------------------------------------
    def performBundleAdjustment(self) -> capi.Summary:
        """Runs LM to termination; cam/views/pts of `problem` are updated in place (reference :965-988)."""
        s = capi.Summary()
        _check(self.lib, self.lib.lifcal_ba_solve(self._h, C.byref(s)), "lifcal_ba_solve")
        return s

    def calcReprojectionError(self, inlierThreshold: float = 1.0) -> capi.Stats:
        st = capi.Stats()
        _check(self.lib, self.lib.lifcal_ba_reproj_stats(self._h, inlierThreshold, C.byref(st)), "lifcal_ba_reproj_stats")
        return st

    def projectObservations(self):
        """(x_proj, y_proj) per observation at the stored parameters, in the caller's observation order — the projected
        columns of reference storeRawImagePointsCsv (src/CameraCalibration.cpp:1504-1538)."""
        n = self.problem.struct.n_obs
        x = np.zeros(n); y = np.zeros(n)
        _check(self.lib, self.lib.lifcal_ba_project_observations(self._h, capi.as_dptr(x), capi.as_dptr(y)), "lifcal_ba_project_observations")
        return x, y

    def residualReport(self, inlierThreshold: float = 1.0, per_observation: bool = True) -> ResidualReport:
        """The reprojection errors behind calcReprojectionError, per observation and summed by frame, 3D point and micro lens
        (lifcal_ba_residual_report).  Every sum is taken in a fixed order: the report is bitwise reproducible."""
        p = self.problem.struct
        n, n_lenses = p.n_obs, self.info().n_lenses
        io = capi.ResidualReportIO()
        io.inlier_threshold = float(inlierThreshold)
        ex = ey = w = lens = None
        if per_observation:
            ex = np.zeros(n); ey = np.zeros(n); w = np.zeros(n); lens = np.zeros(n, np.uint32)
            io.ex, io.ey, io.weight, io.lens = capi.as_dptr(ex), capi.as_dptr(ey), capi.as_dptr(w), capi.as_uptr(lens)
        lens_xy = np.zeros((n_lenses, 2))
        tabs = [np.zeros(k, capi.GROUP_STATS_DTYPE) for k in (p.n_frames, p.n_points, n_lenses)]
        io.lens_xy = capi.as_dptr(lens_xy)
        io.per_frame, io.per_point, io.per_lens = (C.cast(t.ctypes.data, capi._gptr) for t in tabs)
        _check(self.lib, self.lib.lifcal_ba_residual_report(self._h, C.byref(io)), "lifcal_ba_residual_report")
        total = np.frombuffer(bytes(io.total), capi.GROUP_STATS_DTYPE).copy()
        return ResidualReport(ex, ey, w, lens, lens_xy, GroupTable(tabs[0]), GroupTable(tabs[1]), GroupTable(tabs[2]), GroupTable(total),
                              float(inlierThreshold), float(io.seconds))

    def residualGroups(self, key, n_keys: int, inlierThreshold: float = 1.0) -> GroupTable:
        """The statistics of residualReport for any grouping: key[i] < n_keys for every observation, in the caller's order
        (lifcal_ba_residual_groups; see sensor_cells for a map over the sensor)."""
        k = np.ascontiguousarray(key, np.uint32).reshape(-1)
        if len(k) != self.problem.struct.n_obs:
            raise LifcalError("residualGroups: one key per observation")
        rows = np.zeros(int(n_keys), capi.GROUP_STATS_DTYPE)
        _check(self.lib, self.lib.lifcal_ba_residual_groups(self._h, float(inlierThreshold), int(n_keys), capi.as_uptr(k), rows.ctypes.data), "lifcal_ba_residual_groups")
        return GroupTable(rows)

    def set_fixed_frames(self, fixed=None):
        """hold the poses of the frames with fixed[f] != 0 constant in the following sweeps / solves (None frees all)"""
        if fixed is None:
            _check(self.lib, self.lib.lifcal_ba_set_fixed_frames(self._h, None), "lifcal_ba_set_fixed_frames")
        else:
            m = np.ascontiguousarray(fixed, np.uint8)
            assert len(m) == self.problem.struct.n_frames
            _check(self.lib, self.lib.lifcal_ba_set_fixed_frames(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8))), "lifcal_ba_set_fixed_frames")

    def set_priors(self, camera=None, poses=None):
        """Gaussian priors 1/2 (x - mean)^T info (x - mean) for the following sweeps / solves (lifcal_ba_set_priors, include/lifcal_prior.h):
        camera = (mean[17], info[17, 17]) in the layout of the problem's cam, poses = (frames[n] strictly ascending, means[n, 6],
        infos[n, 6, 6]).  Replaces the priors the handle had; both None clears them.  Slots that are not free parameters of the
        handle (fixed_mask, absent distortion slots, constant poses) leave the term."""
        if camera is None and poses is None:
            return self.clear_priors()
        arrs = capi.PriorArrays(camera, poses)
        _check(self.lib, self.lib.lifcal_ba_set_priors(self._h, C.byref(arrs.struct)), "lifcal_ba_set_priors")

    def clear_priors(self):
        _check(self.lib, self.lib.lifcal_ba_set_priors(self._h, None), "lifcal_ba_set_priors")

    def prior_cost(self):
        """(camera, poses): 1/2 d^T info d of the camera prior and summed over the pose priors at the device-resident parameters."""
        c = np.zeros(2)
        _check(self.lib, self.lib.lifcal_ba_prior_cost(self._h, capi.as_dptr(c[0:1]), capi.as_dptr(c[1:2])), "lifcal_ba_prior_cost")
        return float(c[0]), float(c[1])

    def set_point_priors(self, ids, means, infos):
        """New means[n, 3] and infos[n, 3, 3] on the point set given at create (lifcal_ba_set_point_priors); a different set or a handle
        made without point_priors raises LifcalError (.code -1) and leaves the handle as it was."""
        arrs = capi.PointPriorArrays(ids, means, infos)
        _check(self.lib, self.lib.lifcal_ba_set_point_priors(self._h, C.byref(arrs.struct)), "lifcal_ba_set_point_priors")

    def clear_point_priors(self):
        """Every information matrix zero: the term leaves, the point set (and the layout) stays."""
        _check(self.lib, self.lib.lifcal_ba_set_point_priors(self._h, None), "lifcal_ba_set_point_priors")

    def point_prior_cost(self) -> float:
        """Sum of 1/2 d^T info d over the point priors at the device-resident points."""
        c = np.zeros(1)
        _check(self.lib, self.lib.lifcal_ba_point_prior_cost(self._h, capi.as_dptr(c)), "lifcal_ba_point_prior_cost")
        return float(c[0])

    def covariance(self, gauge_frame: int = -1, want_pose_blocks: bool = True, scale_by_residual_variance: bool = False,
                   null_rcond: Optional[float] = None, estimable_tol: Optional[float] = None, want_pose_band: bool = False) -> Covariance:
        """Covariance of the parameters at the device-resident point (lifcal_ba_covariance); the handle is left as it was.
        gauge_frame: -1 automatic (first observed frame when poses and points are both refined), >= 0 that frame, -2 none."""
        o = capi.CovarianceOptions()
        self.lib.lifcal_ba_default_covariance_options(C.byref(o))
        o.gauge_frame = int(gauge_frame); o.want_pose_blocks = 1 if want_pose_blocks else 0
        o.scale_by_residual_variance = 1 if scale_by_residual_variance else 0
        if null_rcond is not None:
            o.null_rcond = float(null_rcond)
        if estimable_tol is not None:
            o.estimable_tol = float(estimable_tol)
        F = self.problem.struct.n_frames
        cam = np.zeros((17, 17)); null = np.zeros((17, 17))
        poses = np.zeros((F, 6, 6)) if want_pose_blocks else None
        bw = self.info().max_window_frames - 1
        band = np.zeros((F, bw, 6, 6)) if want_pose_band and bw > 0 else None
        out = capi.CovarianceOut()
        out.camera, out.camera_null = capi.as_dptr(cam), capi.as_dptr(null)
        out.pose = capi.as_dptr(poses) if poses is not None else None
        out.pose_band = capi.as_dptr(band) if band is not None else None
        _check(self.lib, self.lib.lifcal_ba_covariance(self._h, C.byref(o), C.byref(out)), "lifcal_ba_covariance")
        live = np.array([(out.live_mask >> j) & 1 for j in range(17)], bool)
        est = np.array([(out.estimable_mask >> j) & 1 for j in range(17)], bool)
        std = np.where(live, np.sqrt(np.maximum(np.diag(cam), 0.0)), 0.0)
        std[live & ~est] = np.nan
        return Covariance(cam, std, est, int(out.null_rank), null[: out.null_rank].copy(), poses, int(out.gauge_frame_used),
                          float(out.sigma2), live, band, float(out.seconds), float(out.cost))

    def objectSpaceStats(self, x, y, vdepth, fr, pt):
        """The calibration judged in object space at the device-resident parameters (lifcal_ba_object_space_stats): for image
        points of the virtual image (x_v, y_v, virtual depth, frame, object point) returns (stats, ref_c, proj_c) with
        ref_c = RT P (reference storeResults :1256-1260) and proj_c = projectPointBack of the image point (:1276-1284), both (n, 3),
        and stats.rms / .max_abs per axis of proj_c - ref_c, .rms_rel_depth, .n_used, .n_skipped (vdepth < 2)."""
        x = np.ascontiguousarray(x, np.float64).reshape(-1); y = np.ascontiguousarray(y, np.float64).reshape(-1)
        vd = np.ascontiguousarray(vdepth, np.float64).reshape(-1)
        fr = np.ascontiguousarray(fr, np.uint32).reshape(-1); pt = np.ascontiguousarray(pt, np.uint32).reshape(-1)
        n = len(x)
        if not (len(y) == len(vd) == len(fr) == len(pt) == n):
            raise LifcalError("objectSpaceStats: arrays differ in length")
        ref = np.zeros((n, 3)); proj = np.zeros((n, 3))
        st = capi.ObjectSpace()
        _check(self.lib, self.lib.lifcal_ba_object_space_stats(self._h, n, capi.as_dptr(x), capi.as_dptr(y), capi.as_dptr(vd), capi.as_uptr(fr), capi.as_uptr(pt),
                                                               capi.as_dptr(ref), capi.as_dptr(proj), C.byref(st)), "lifcal_ba_object_space_stats")
        return st, ref, proj

    def resectFrames(self, views0=None, observations=None, options: Optional[capi.Options] = None, inlierThreshold: float = 1.0):
        """Resect frames against the handle's current (device-resident) camera and points, which stay constant
        (lifcal_amd.resection.resectFrames).  observations: (u, v, mcx, mcy, pt, fr) of the frames to localise, fr counting them
        from 0, with their start poses views0; None: the problem's own observations (and, without views0, its current poses).
        The handle and its parameters are left as they are."""
        from .resection import resectFrames
        self.download_parameters()
        pr = self.problem
        if observations is None:
            observations = (pr.u, pr.v, pr.mcx, pr.mcy, pr.pt, pr.fr)
            if views0 is None:
                views0 = pr.views
        if views0 is None:
            raise LifcalError("resectFrames: new observations need start poses")
        u, v, mcx, mcy, pt, fr = observations
        if options is None:
            options = capi.Options.from_buffer_copy(self.options); options.world_size = 1; options.rank = 0; options.precision = 0
        return resectFrames(pr.cam, pr.pts, u, v, mcx, mcy, pt, fr, views0, pr.struct.config, pr.struct.spx, pr.struct.scale, spy=pr.struct.spy,
                            options=options, inlierThreshold=inlierThreshold)

    def intersectPoints(self, pts0=None, observations=None, options: Optional[capi.Options] = None, inlierThreshold: float = 1.0):
        """Intersect points against the handle's current (device-resident) camera and poses, which stay constant
        (lifcal_amd.intersection.intersectPoints).  observations: (u, v, mcx, mcy, pt, fr) of the points to intersect, pt counting
        them from 0 and fr naming the handle's frames, with their start values pts0; None: the problem's own observations (and,
        without pts0, its current points).  The handle and its parameters are left as they are."""
        from .intersection import intersectPoints
        self.download_parameters()
        pr = self.problem
        if observations is None:
            observations = (pr.u, pr.v, pr.mcx, pr.mcy, pr.pt, pr.fr)
            if pts0 is None:
                pts0 = pr.pts
        if pts0 is None:
            raise LifcalError("intersectPoints: new observations need start points")
        u, v, mcx, mcy, pt, fr = observations
        if options is None:
            options = capi.Options.from_buffer_copy(self.options); options.world_size = 1; options.rank = 0; options.precision = 0
        return intersectPoints(pr.cam, pr.views, u, v, mcx, mcy, pt, fr, pts0, pr.struct.config, pr.struct.spx, pr.struct.scale, spy=pr.struct.spy,
                               options=options, inlierThreshold=inlierThreshold)

    def startPoses(self, observations=None, n_frames=None, options: Optional[capi.Options] = None, gatePx: float = 1.0, inlierThreshold: float = 1.0,
                   wantGroups: bool = False):
        """Closed-form start poses against the handle's current (device-resident) camera and points (lifcal_amd.start.startPoses).
        observations: (u, v, mcx, mcy, pt, fr) of the n_frames frames to localise, fr counting them from 0; None: the problem's own
        observations and frames.  The result's views are start values for resectFrames.  The handle is left as it is."""
        from .start import startPoses
        self.download_parameters()
        pr = self.problem
        if observations is None:
            observations = (pr.u, pr.v, pr.mcx, pr.mcy, pr.pt, pr.fr)
            if n_frames is None:
                n_frames = pr.struct.n_frames
        if n_frames is None:
            raise LifcalError("startPoses: new observations need their number of frames")
        u, v, mcx, mcy, pt, fr = observations
        if options is None:
            options = capi.Options.from_buffer_copy(self.options); options.world_size = 1; options.rank = 0; options.precision = 0
        return startPoses(pr.cam, pr.pts, u, v, mcx, mcy, pt, fr, n_frames, pr.struct.config, pr.struct.spx, pr.struct.scale, spy=pr.struct.spy,
                          options=options, gatePx=gatePx, inlierThreshold=inlierThreshold, wantGroups=wantGroups)

    def startPoints(self, observations=None, n_points=None, options: Optional[capi.Options] = None, inlierThreshold: float = 1.0):
        """Closed-form start points against the handle's current (device-resident) camera and poses (lifcal_amd.start.startPoints).
        observations: (u, v, mcx, mcy, pt, fr) of the n_points points to triangulate, pt counting them from 0 and fr naming the
        handle's frames; None: the problem's own observations and points.  The result's pts are start values for intersectPoints."""
        from .start import startPoints
        self.download_parameters()
        pr = self.problem
        if observations is None:
            observations = (pr.u, pr.v, pr.mcx, pr.mcy, pr.pt, pr.fr)
            if n_points is None:
                n_points = pr.struct.n_points
        if n_points is None:
            raise LifcalError("startPoints: new observations need their number of points")
        u, v, mcx, mcy, pt, fr = observations
        if options is None:
            options = capi.Options.from_buffer_copy(self.options); options.world_size = 1; options.rank = 0; options.precision = 0
        return startPoints(pr.cam, pr.views, u, v, mcx, mcy, pt, fr, n_points, pr.struct.config, pr.struct.spx, pr.struct.scale, spy=pr.struct.spy,
                           options=options, inlierThreshold=inlierThreshold)

    def registerScene(self, observations=None, n_frames=None, n_points=None, options: Optional[capi.Options] = None, gatePx: float = 1.0,
                      inlierThreshold: float = 1.0, minShared: int = 6, anchorFrame: int = -1, anchorView=None, maxRounds: int = 0):
        """Poses and points from micro-image rays alone against the handle's current (device-resident) camera
        (lifcal_amd.register.registerScene).  observations: (u, v, mcx, mcy, pt, fr) of a sequence with n_frames frames and n_points
        points, both counted from 0; None: the problem's own observations, frames and points.  The handle is left as it is."""
        from .register import registerScene
        self.download_parameters()
        pr = self.problem
        if observations is None:
            observations = (pr.u, pr.v, pr.mcx, pr.mcy, pr.pt, pr.fr)
            if n_frames is None:
                n_frames = pr.struct.n_frames
            if n_points is None:
                n_points = pr.struct.n_points
        if n_frames is None or n_points is None:
            raise LifcalError("registerScene: new observations need their numbers of frames and points")
        u, v, mcx, mcy, pt, fr = observations
        if options is None:
            options = capi.Options.from_buffer_copy(self.options); options.world_size = 1; options.rank = 0; options.precision = 0
        return registerScene(pr.cam, u, v, mcx, mcy, pt, fr, n_frames, n_points, pr.struct.config, pr.struct.spx, pr.struct.scale, spy=pr.struct.spy,
                             options=options, gatePx=gatePx, inlierThreshold=inlierThreshold, minShared=minShared, anchorFrame=anchorFrame,
                             anchorView=anchorView, maxRounds=maxRounds)

    # -- the benchmarked unit ------------------------------------------------------------------
    def sweep(self, radius: float = 1e4, want_matrices: bool = False):
        """One Jacobian+Schur sweep; returns a namespace with cost, gradient_max_norm, seconds and,
        if requested, S / rhs / gradient_reduced / point_gradient / point_hessian_inv (canonical order)."""
        info = self.info()
        out = capi.SweepOut()
        res = type("Sweep", (), {})()
        if want_matrices:
            n = info.n_reduced
            P = self.problem.struct.n_points
            res.S = np.zeros((n, n)); res.rhs = np.zeros(n); res.gradient_reduced = np.zeros(n)
            res.point_gradient = np.zeros(3 * P); res.point_hessian_inv = np.zeros(9 * P)
            out.S, out.rhs, out.gradient_reduced = capi.as_dptr(res.S), capi.as_dptr(res.rhs), capi.as_dptr(res.gradient_reduced)
            out.point_gradient, out.point_hessian_inv = capi.as_dptr(res.point_gradient), capi.as_dptr(res.point_hessian_inv)
        _check(self.lib, self.lib.lifcal_ba_sweep(self._h, float(radius), C.byref(out)), "lifcal_ba_sweep")
        res.cost = out.cost; res.gradient_max_norm = out.gradient_max_norm; res.seconds = out.seconds
        res.n_reduced = out.n_reduced; res.n_promoted = out.n_promoted
        return res

    def debug_step(self):
        """One LM step on the S | rhs of the sweep() just made, read back (lifcal_ba_debug_step): returns a namespace with
        delta_reduced (canonical order of sweep().S), delta_points (3P), lambda_reduced / lambda_points (the LM diagonal the step
        was damped with, same orders), the step scalars gtd, ddd, step2, x2, cand_cost, chol_fail,
        route (0 global-memory chain, 1 LDS chain, 2 twisted, 3 block odd-even reduction) and panel_in_lds.  The parameters stay
        as they are; anything but a sweep() in front of the call raises LifcalError (code LIFCAL_BA_ERR_INVALID_ARG)."""
        out = capi.StepOut()
        res = type("Step", (), {})()
        n, P3 = self.info().n_reduced, 3 * self.problem.struct.n_points
        res.delta_reduced = np.zeros(n); res.delta_points = np.zeros(P3); res.lambda_reduced = np.zeros(n); res.lambda_points = np.zeros(P3)
        out.delta_reduced, out.delta_points = capi.as_dptr(res.delta_reduced), capi.as_dptr(res.delta_points)
        out.lambda_reduced, out.lambda_points = capi.as_dptr(res.lambda_reduced), capi.as_dptr(res.lambda_points)
        _check(self.lib, self.lib.lifcal_ba_debug_step(self._h, C.byref(out)), "lifcal_ba_debug_step")
        for k in ("gtd", "ddd", "step2", "x2", "cand_cost", "chol_fail"):
            setattr(res, k, float(getattr(out, k)))
        res.route = int(out.route); res.panel_in_lds = bool(out.panel_in_lds)
        return res

    def sweep_enqueue(self, radius: float = 1e4):
        """Enqueue one sweep on the handle's stream without a host round trip (timing loops)."""
        rc = self.lib.lifcal_ba_sweep_enqueue(self._h, float(radius))
        if rc:
            _check(self.lib, rc, "lifcal_ba_sweep_enqueue")

    def profile_begin(self, max_sweeps: int, stride: int = 1):
        """The next max_sweeps sweeps form a profiled span; every stride-th one carries the dominant kernel's own time stamps
        (a stamped launch costs ~5 us of queue time: timing loops sample, lifcal_ba_profile_begin_sampled)."""
        _check(self.lib, self.lib.lifcal_ba_profile_begin_sampled(self._h, int(max_sweeps), int(stride)), "lifcal_ba_profile_begin_sampled")

    def profile_end(self) -> capi.Profile:
        p = capi.Profile()
        _check(self.lib, self.lib.lifcal_ba_profile_end(self._h, C.byref(p)), "lifcal_ba_profile_end")
        return p

    # -- plumbing --------------------------------------------------------------------------------
    def upload_parameters(self):
        _check(self.lib, self.lib.lifcal_ba_upload_parameters(self._h), "lifcal_ba_upload_parameters")

    def download_parameters(self):
        _check(self.lib, self.lib.lifcal_ba_download_parameters(self._h), "lifcal_ba_download_parameters")

    def info(self) -> capi.Info:
        i = capi.Info()
        _check(self.lib, self.lib.lifcal_ba_get_info(self._h, C.byref(i)), "lifcal_ba_get_info")
        return i

    def set_allreduce(self, fn):
        """fn(device_ptr:int, count:int, stream:int) -> 0 on success; must sum-reduce in place."""
        def tramp(ctx, buf, count, stream):
            try:
                return int(fn(int(buf or 0), int(count), int(stream or 0)))
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._hook = capi.ALLREDUCE_FN(tramp)
        _check(self.lib, self.lib.lifcal_ba_set_allreduce(self._h, self._hook, None), "lifcal_ba_set_allreduce")

    def set_allgather(self, fn):
        """fn(send_ptr:int, recv_ptr:int, count_per_rank:int, stream:int) -> 0 on success; recv is rank-major."""
        def tramp(ctx, send, recv, count, stream):
            try:
                return int(fn(int(send or 0), int(recv or 0), int(count), int(stream or 0)))
            except Exception:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        self._ghook = capi.ALLGATHER_FN(tramp)
        _check(self.lib, self.lib.lifcal_ba_set_allgather(self._h, self._ghook, None), "lifcal_ba_set_allgather")

    def comm_init_rccl(self, unique_id: bytes):
        buf = C.create_string_buffer(unique_id, 128)
        _check(self.lib, self.lib.lifcal_ba_comm_init_rccl(self._h, buf), "lifcal_ba_comm_init_rccl")


def performBundleAdjustmentWindowed(problem: capi.ProblemArrays, window_frames: int, overlap_frames: int, options: Optional[capi.Options] = None,
                                    comm_template: Optional[BundleAdjustment] = None):
    """Frame-windowed ("streaming") solve of a long sequence (lifcal_ba_solve_windowed): parameters of `problem` are updated in
    place, one window resident on the device at a time.  Returns the list of per-window reports."""
    lib = capi.load_library()
    if options is None:
        options = capi.Options(); lib.lifcal_ba_default_options(C.byref(options))
    step = window_frames - overlap_frames
    cap = max(1, (problem.struct.n_frames + step - 1) // max(step, 1) + 1)
    reps = (capi.WindowReport * cap)()
    n = C.c_uint32(cap)
    _check(lib, lib.lifcal_ba_solve_windowed(C.byref(problem.struct), C.byref(options), int(window_frames), int(overlap_frames),
                                             comm_template._h if comm_template is not None else None, reps, C.byref(n)), "lifcal_ba_solve_windowed")
    return [reps[i] for i in range(n.value)]


def comm_unique_id() -> bytes:
    lib = capi.load_library()
    buf = C.create_string_buffer(128)
    _check(lib, lib.lifcal_ba_comm_unique_id(buf), "lifcal_ba_comm_unique_id")
    return buf.raw


def initPlenopticParameters(vdepth, fr, pt, world_to_cam, pts, fL_init, device: int = 0):
    """Start values (B_init, bL0_init) of the plenoptic parameters — reference CameraCalibration::initPlenopticParameters
    (src/CameraCalibration.cpp:456-499).  vdepth / fr / pt: one entry per image point (virtual depth, frame, object point);
    world_to_cam: (F, 4, 4) matrices; pts: (P, 3); fL_init = fPH_init * pixelSize_totFoc.  Returns capi.InitResult."""
    lib = capi.load_library()
    arrs = capi.InitArrays(vdepth, fr, pt, world_to_cam, pts, fL_init)
    res = capi.InitResult()
    _check(lib, lib.lifcal_init_plenoptic(C.byref(arrs.struct), int(device), C.byref(res)), "lifcal_init_plenoptic")
    return res


def plan(problem: capi.ProblemArrays, rank: int = 0, world_size: int = 1):
    """Host-only layout planning (no GPU needed): returns (PlanInfo, obs_order, point_owner)."""
    lib = capi.load_library()
    info = capi.PlanInfo()
    order = np.zeros(max(problem.struct.n_obs, 1), np.uint32)
    owner = np.zeros(max(problem.struct.n_points, 1), np.uint32)
    _check(lib, lib.lifcal_ba_plan(C.byref(problem.struct), rank, world_size, C.byref(info), capi.as_uptr(order), capi.as_uptr(owner)), "lifcal_ba_plan")
    return info, order[: problem.struct.n_obs], owner[: problem.struct.n_points].astype(np.int32)


def plan_stats(problem: capi.ProblemArrays, rank: int = 0, world_size: int = 1) -> capi.PlanStats:
    """Host-only statistics of the LDS-window schedule create() would build in this environment (blocks, passes, lanes, observation
    steps, modelled block cost, points moved by the processing order) and a count of layout violations recounted from the plan's arrays."""
    lib = capi.load_library()
    st = capi.PlanStats()
    _check(lib, lib.lifcal_ba_plan_stats(C.byref(problem.struct), rank, world_size, C.byref(st)), "lifcal_ba_plan_stats")
    return st


def plan_shape(problem: capi.ProblemArrays, rank: int = 0, world_size: int = 1) -> capi.PlanShape:
    """Host-only: the same schedule tile by tile and pass by pass (tiles by their step count, points per pass, passes per block, the
    rows the last tile's clamped prefetch reads against the rows the padded arrays hold)."""
    lib = capi.load_library()
    sh = capi.PlanShape()
    _check(lib, lib.lifcal_ba_plan_shape(C.byref(problem.struct), rank, world_size, C.byref(sh)), "lifcal_ba_plan_shape")
    return sh
