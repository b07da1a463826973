"""Closed-form start values from micro-image rays (include/lifcal_start.h): poses for resectFrames and points
for intersectPoints, without an external structure-from-motion run.

With the camera block known every micro-image observation fixes a line in the camera frame.  The micro images of one (frame, point)
pair triangulate that point in the camera frame; a weighted rigid alignment of those points onto the known world points is the pose.
With poses known, the same lines carried into the world frame triangulate a point from all its frames.  The arithmetic lives in the
HIP library; this file flattens arguments and forwards them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError, _check


def _rms(rows, name):
    n = rows["n_obs"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(np.where((n > 0) & (rows["status"] == 0), rows[name] / n, np.nan))


@dataclass
class StartPosesResult:
    """startPoses: one entry per frame.

    views          (F, 6) poses {ax, ay, az, tx, ty, tz}; NaN for a frame whose status is not 0
    rows           structured array of capi.START_FRAME_DTYPE, the table as the library returns it
    groups         structured array of capi.START_GROUP_DTYPE in ascending (fr, pt) order (wantGroups), else None
    rms_x, rms_y   sqrt(sum e^2 / n) of e = projected - observed over all observations of the frame at the new pose (NaN: no pose)
    status         0: OK, 1: no observations, 2: fewer than three used groups, 3: degenerate (collinear points)
    """
    views: np.ndarray
    rows: np.ndarray
    groups: Optional[np.ndarray]
    seconds: float
    gate_px: float
    inlier_threshold: float

    @property
    def rms_x(self) -> np.ndarray:
        return _rms(self.rows, "sum_xx")

    @property
    def rms_y(self) -> np.ndarray:
        return _rms(self.rows, "sum_yy")

    @property
    def status(self) -> np.ndarray:
        return self.rows["status"]

    @property
    def n_used(self) -> np.ndarray:
        return self.rows["n_used"]


@dataclass
class StartPointsResult:
    """startPoints: one entry per point.

    pts            (P, 3) points; NaN for a point whose status is not 0
    rows           structured array of capi.START_POINT_DTYPE, the table as the library returns it
    rms_x, rms_y   sqrt(sum e^2 / n) of e = projected - observed at the new point (NaN: no point)
    status         0: OK, 1: no observations, 2: one observation, 3: singular, 4: behind the main lens in one of its frames
    """
    pts: np.ndarray
    rows: np.ndarray
    seconds: float
    inlier_threshold: float

    @property
    def rms_x(self) -> np.ndarray:
        return _rms(self.rows, "sum_xx")

    @property
    def rms_y(self) -> np.ndarray:
        return _rms(self.rows, "sum_yy")

    @property
    def status(self) -> np.ndarray:
        return self.rows["status"]


def _flatten(u, v, mcx, mcy, pt, fr, what):
    f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    u4 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
    u, v, mcx, mcy, pt, fr = f8(u), f8(v), f8(mcx), f8(mcy), u4(pt), u4(fr)
    if not (len(u) == len(v) == len(mcx) == len(mcy) == len(pt) == len(fr)):
        raise LifcalError(f"{what}: observation arrays differ in length")
    return u, v, mcx, mcy, pt, fr


def startPoses(cam, pts, u, v, mcx, mcy, pt, fr, n_frames, config, spx, scale, spy=None, options: Optional[capi.Options] = None,
               gatePx: float = 1.0, inlierThreshold: float = 1.0, wantGroups: bool = False) -> StartPosesResult:
    """Poses of n_frames frames from their observations alone, against the constant camera block `cam` (17 values, layout of
    lifcal_ba_problem.cam) and the constant object points `pts`.  Observations as in capi.ProblemArrays, in any order.  gatePx: the
    largest triangulation residual (RMS, pixels) of a (frame, point) group that takes part in the alignment; inf: no gate.  The
    views of the result are start values for resectFrames."""
    lib = capi.load_library()
    if options is None:
        options = capi.Options(); lib.lifcal_ba_default_options(C.byref(options))
    u, v, mcx, mcy, pt, fr = _flatten(u, v, mcx, mcy, pt, fr, "startPoses")
    f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    cam, pts = f8(cam), f8(pts)
    if len(cam) != 17 or len(pts) % 3 or n_frames < 0:
        raise LifcalError("startPoses: cam has 17 values, pts 3 per point")
    views = np.full(6 * int(n_frames), np.nan)
    p = capi.ResectProblem()
    p.n_obs, p.n_frames, p.n_points = len(u), int(n_frames), len(pts) // 3
    p.u, p.v, p.mcx, p.mcy, p.pt, p.fr = capi.as_dptr(u), capi.as_dptr(v), capi.as_dptr(mcx), capi.as_dptr(mcy), capi.as_uptr(pt), capi.as_uptr(fr)
    p.cam, p.pts, p.views = capi.as_dptr(cam), capi.as_dptr(pts), capi.as_dptr(views)
    p.spx, p.spy, p.scale, p.config = float(spx), float(spx if spy is None else spy), float(scale), int(config)
    rows = np.zeros(p.n_frames, capi.START_FRAME_DTYPE)
    groups = np.zeros(len(u), capi.START_GROUP_DTYPE) if wantGroups else None
    n_groups = np.zeros(1, np.uint32)
    seconds = C.c_double(0.0)
    _check(lib, lib.lifcal_start_poses(C.byref(p), C.byref(options), float(gatePx), float(inlierThreshold), rows.ctypes.data,
                                       groups.ctypes.data if wantGroups else None, capi.as_uptr(n_groups), C.byref(seconds)), "lifcal_start_poses")
    return StartPosesResult(views.reshape(-1, 6), rows, groups[:int(n_groups[0])].copy() if wantGroups else None, float(seconds.value),
                            float(gatePx), float(inlierThreshold))


def startPoints(cam, views, u, v, mcx, mcy, pt, fr, n_points, config, spx, scale, spy=None, options: Optional[capi.Options] = None,
                inlierThreshold: float = 1.0) -> StartPointsResult:
    """n_points points from all their observations, against the constant camera block `cam` and the constant poses `views` (F, 6).
    Observations as in capi.ProblemArrays, in any order.  The pts of the result are start values for intersectPoints."""
    lib = capi.load_library()
    if options is None:
        options = capi.Options(); lib.lifcal_ba_default_options(C.byref(options))
    u, v, mcx, mcy, pt, fr = _flatten(u, v, mcx, mcy, pt, fr, "startPoints")
    f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    cam, views = f8(cam), f8(views)
    if len(cam) != 17 or len(views) % 6 or n_points < 0:
        raise LifcalError("startPoints: cam has 17 values, views 6 per frame")
    pts = np.full(3 * int(n_points), np.nan)
    p = capi.IntersectProblem()
    p.n_obs, p.n_frames, p.n_points = len(u), len(views) // 6, int(n_points)
    p.u, p.v, p.mcx, p.mcy, p.pt, p.fr = capi.as_dptr(u), capi.as_dptr(v), capi.as_dptr(mcx), capi.as_dptr(mcy), capi.as_uptr(pt), capi.as_uptr(fr)
    p.cam, p.views, p.pts = capi.as_dptr(cam), capi.as_dptr(views), capi.as_dptr(pts)
    p.spx, p.spy, p.scale, p.config = float(spx), float(spx if spy is None else spy), float(scale), int(config)
    rows = np.zeros(p.n_points, capi.START_POINT_DTYPE)
    seconds = C.c_double(0.0)
    _check(lib, lib.lifcal_start_points(C.byref(p), C.byref(options), float(inlierThreshold), rows.ctypes.data, C.byref(seconds)), "lifcal_start_points")
    return StartPointsResult(pts.reshape(-1, 3), rows, float(seconds.value), float(inlierThreshold))
