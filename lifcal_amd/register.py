"""Register a scene from micro-image rays alone (include/lifcal_register.h): poses and points of a sequence
taken with a calibrated camera, without a structure-from-motion run.

One anchor frame defines the world.  Round by round the frames that share enough mapped points are aligned onto them and refined by
resection, new points are carried into the world through the registered frames, and all mapped points and registered poses are
refined by one Levenberg-Marquardt solve each.  The result is metric and is a start for BundleAdjustment.  The arithmetic lives in
the HIP library; this file flattens arguments and forwards them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError, _check
from .start import _flatten


def _rms(rows, name):
    n = rows["n_obs_used"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(np.where((n > 0) & (rows["status"] == 0), rows[name] / n, np.nan))


@dataclass
class RegisterResult:
    """registerScene: one entry per frame and per point.

    views          (F, 6) poses {ax, ay, az, tx, ty, tz}; NaN for a frame that was not registered
    pts            (P, 3) points; NaN for a point that was not mapped
    frame_rows     structured array of capi.REGISTER_FRAME_DTYPE, the table as the library returns it
    point_rows     structured array of capi.REGISTER_POINT_DTYPE
    summary        capi.RegisterSummary: anchor_frame, n_rounds, n_frames_registered, n_points_mapped, n_groups, n_groups_used
    rms_x, rms_y   sqrt(sum e^2 / n) of e = projected - observed over the registered part of the scene at the returned parameters
    """
    views: np.ndarray
    pts: np.ndarray
    frame_rows: np.ndarray
    point_rows: np.ndarray
    summary: capi.RegisterSummary
    seconds: float

    @property
    def registered(self) -> np.ndarray:
        return self.frame_rows["status"] == 0

    @property
    def mapped(self) -> np.ndarray:
        return self.point_rows["status"] == 0

    def _total(self, name) -> float:
        n = int(self.frame_rows["n_obs_used"][self.registered].sum())
        return float(np.sqrt(self.frame_rows[name][self.registered].sum() / n)) if n else float("nan")

    @property
    def rms_x(self) -> float:
        return self._total("sum_xx")

    @property
    def rms_y(self) -> float:
        return self._total("sum_yy")

    @property
    def frame_rms_x(self) -> np.ndarray:
        return _rms(self.frame_rows, "sum_xx")

    @property
    def frame_rms_y(self) -> np.ndarray:
        return _rms(self.frame_rows, "sum_yy")

    @property
    def point_rms_x(self) -> np.ndarray:
        return _rms(self.point_rows, "sum_xx")

    @property
    def point_rms_y(self) -> np.ndarray:
        return _rms(self.point_rows, "sum_yy")


def registerScene(cam, u, v, mcx, mcy, pt, fr, n_frames, n_points, config, spx, scale, spy=None, options: Optional[capi.Options] = None,
                  gatePx: float = 1.0, inlierThreshold: float = 1.0, minShared: int = 6, anchorFrame: int = -1, anchorView=None,
                  maxRounds: int = 0) -> RegisterResult:
    """Poses of n_frames frames and coordinates of n_points points from their observations alone, against the constant camera block
    `cam` (17 values, layout of lifcal_ba_problem.cam).  Observations as in capi.ProblemArrays, in any order; pt and fr are the
    tracks, which have to come from outside.  minShared: the used (frame, point) groups on mapped points a frame needs to be
    registered; anchorFrame: the frame that defines the world (-1: the one with the most used groups) and anchorView its pose
    (None: zeros); maxRounds: 0 runs until a round registers no frame."""
    lib = capi.load_library()
    if options is None:
        options = capi.Options(); lib.lifcal_ba_default_options(C.byref(options))
    u, v, mcx, mcy, pt, fr = _flatten(u, v, mcx, mcy, pt, fr, "registerScene")
    cam = np.ascontiguousarray(np.asarray(cam, dtype=np.float64).reshape(-1))
    if len(cam) != 17:
        raise LifcalError("registerScene: cam has 17 values")
    if n_frames < 0 or n_points < 0:
        raise LifcalError("registerScene: n_frames and n_points must not be negative")
    views, pts = np.full(6 * int(n_frames), np.nan), np.full(3 * int(n_points), np.nan)
    p = capi.RegisterProblem()
    p.n_obs, p.n_frames, p.n_points = len(u), int(n_frames), int(n_points)
    p.u, p.v, p.mcx, p.mcy, p.pt, p.fr = capi.as_dptr(u), capi.as_dptr(v), capi.as_dptr(mcx), capi.as_dptr(mcy), capi.as_uptr(pt), capi.as_uptr(fr)
    p.cam, p.views, p.pts = capi.as_dptr(cam), capi.as_dptr(views), capi.as_dptr(pts)
    p.spx, p.spy, p.scale, p.config = float(spx), float(spx if spy is None else spy), float(scale), int(config)
    r = capi.RegisterOptions()
    lib.lifcal_register_default_options(C.byref(r))
    r.gate_px, r.inlier_threshold, r.min_shared, r.anchor_frame, r.max_rounds = float(gatePx), float(inlierThreshold), int(minShared), int(anchorFrame), int(maxRounds)
    anchor = None
    if anchorView is not None:
        anchor = np.ascontiguousarray(np.asarray(anchorView, dtype=np.float64).reshape(-1))
        if len(anchor) != 6:
            raise LifcalError("registerScene: anchorView has 6 values")
        r.anchor_view = capi.as_dptr(anchor)
    frame_rows, point_rows = np.zeros(p.n_frames, capi.REGISTER_FRAME_DTYPE), np.zeros(p.n_points, capi.REGISTER_POINT_DTYPE)
    summary = capi.RegisterSummary()
    seconds = C.c_double(0.0)
    _check(lib, lib.lifcal_register_scene(C.byref(p), C.byref(options), C.byref(r), frame_rows.ctypes.data, point_rows.ctypes.data, C.byref(summary),
                                          C.byref(seconds)), "lifcal_register_scene")
    return RegisterResult(views.reshape(-1, 6), pts.reshape(-1, 3), frame_rows, point_rows, summary, float(seconds.value))
