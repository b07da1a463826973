"""Batched pose resection of frames against a calibrated camera (include/lifcal_resect.h).

Camera and object points are constants; every frame's pose is refined by a Levenberg-Marquardt solve of its own, all frames of a
call inside one kernel launch.  The arithmetic lives in the HIP library; this file flattens arguments and forwards them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError, _check

_TRI = np.tril_indices(6)


@dataclass
class ResectionResult:
    """resectFrames: one entry per frame (a frame without observations keeps its pose; its row is zero, termination 0).

    views          (F, 6) resected poses {ax, ay, az, tx, ty, tz}
    rows           structured array of capi.RESECT_FRAME_DTYPE, the table as the library returns it
    H, g           (F, 6, 6) undamped Gauss-Newton matrix J^T J of the pose at the final point and (F, 6) J^T r, parameter units
    rms_x, rms_y   sqrt(sum e^2 / n) of e = projected - observed at the final pose (NaN for an empty frame)
    """
    views: np.ndarray
    rows: np.ndarray
    seconds: float
    inlier_threshold: float

    @property
    def H(self) -> np.ndarray:
        H = np.zeros((len(self.rows), 6, 6))
        H[:, _TRI[0], _TRI[1]] = self.rows["H"]
        H[:, _TRI[1], _TRI[0]] = self.rows["H"]
        return H

    @property
    def g(self) -> np.ndarray:
        return self.rows["g"]

    def _rms(self, name):
        n = self.rows["n_obs"].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.sqrt(np.where(n > 0, self.rows[name] / n, np.nan))

    @property
    def rms_x(self) -> np.ndarray:
        return self._rms("sum_xx")

    @property
    def rms_y(self) -> np.ndarray:
        return self._rms("sum_yy")

    @property
    def n_obs(self) -> np.ndarray:
        return self.rows["n_obs"]

    @property
    def n_inliers(self) -> np.ndarray:
        return self.rows["n_inliers"]

    @property
    def iterations(self) -> np.ndarray:
        return self.rows["iterations"]

    @property
    def termination(self) -> np.ndarray:
        return self.rows["termination"]

    @property
    def final_cost(self) -> np.ndarray:
        return self.rows["final_cost"]

    def pose_information(self) -> np.ndarray:
        """(F, 6, 6): H per frame, the information matrix of a pose prior (BundleAdjustment.set_priors(poses=(frames, views, infos)))."""
        return self.H

    def pose_covariance(self) -> np.ndarray:
        """(F, 6, 6): inverse of H per frame (Ceres units: unit-variance pixel residuals).  NaN where H is not positive definite."""
        out = np.full((len(self.rows), 6, 6), np.nan)
        for f, Hf in enumerate(self.H):
            try:
                L = np.linalg.cholesky(Hf)
            except np.linalg.LinAlgError:
                continue
            Li = np.linalg.inv(L)
            out[f] = Li.T @ Li
        return out


def resectFrames(cam, pts, u, v, mcx, mcy, pt, fr, views0, config, spx, scale, spy=None, options: Optional[capi.Options] = None,
                 inlierThreshold: float = 1.0) -> ResectionResult:
    """Resect every frame against the constant camera block `cam` (17 values, layout of lifcal_ba_problem.cam) and the constant
    object points `pts`; views0 (F, 6) are the start poses.  Observations as in capi.ProblemArrays, in any order: the observations
    of a frame are summed in the order given.  The result of a frame depends on its own observations only, bit for bit."""
    lib = capi.load_library()
    if options is None:
        options = capi.Options(); lib.lifcal_ba_default_options(C.byref(options))
    f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    u4 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
    u, v, mcx, mcy, pt, fr = f8(u), f8(v), f8(mcx), f8(mcy), u4(pt), u4(fr)
    cam, pts, views = f8(cam), f8(pts), f8(views0).copy()
    if not (len(u) == len(v) == len(mcx) == len(mcy) == len(pt) == len(fr)):
        raise LifcalError("resectFrames: observation arrays differ in length")
    if len(cam) != 17 or len(pts) % 3 or len(views) % 6:
        raise LifcalError("resectFrames: cam has 17 values, pts 3 per point, views0 6 per frame")
    p = capi.ResectProblem()
    p.n_obs, p.n_frames, p.n_points = len(u), len(views) // 6, len(pts) // 3
    p.u, p.v, p.mcx, p.mcy, p.pt, p.fr = capi.as_dptr(u), capi.as_dptr(v), capi.as_dptr(mcx), capi.as_dptr(mcy), capi.as_uptr(pt), capi.as_uptr(fr)
    p.cam, p.pts, p.views = capi.as_dptr(cam), capi.as_dptr(pts), capi.as_dptr(views)
    p.spx, p.spy, p.scale, p.config = float(spx), float(spx if spy is None else spy), float(scale), int(config)
    rows = np.zeros(p.n_frames, capi.RESECT_FRAME_DTYPE)
    seconds = C.c_double(0.0)
    _check(lib, lib.lifcal_resect_frames(C.byref(p), C.byref(options), float(inlierThreshold), rows.ctypes.data, C.byref(seconds)), "lifcal_resect_frames")
    return ResectionResult(views.reshape(-1, 6), rows, float(seconds.value), float(inlierThreshold))
