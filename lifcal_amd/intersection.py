"""Batched intersection of 3D points against a calibrated camera and known poses (include/lifcal_intersect.h).

The counterpart of lifcal_amd.resection: camera and poses are constants; every point is refined by a Levenberg-Marquardt solve of
its own, all points of a call inside one kernel launch.  The arithmetic lives in the HIP library; this file flattens arguments and
forwards them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError, _check

_TRI = np.tril_indices(3)


@dataclass
class IntersectionResult:
    """intersectPoints: one entry per point (a point without observations keeps its coordinates; its row is zero, termination 0).

    pts            (P, 3) intersected points
    rows           structured array of capi.INTERSECT_POINT_DTYPE, the table as the library returns it
    H, g           (P, 3, 3) undamped Gauss-Newton matrix J^T J of the point at the final point and (P, 3) J^T r, parameter units
    rms_x, rms_y   sqrt(sum e^2 / n) of e = projected - observed at the final point (NaN for a point without observations)
    """
    pts: np.ndarray
    rows: np.ndarray
    seconds: float
    inlier_threshold: float

    @property
    def H(self) -> np.ndarray:
        H = np.zeros((len(self.rows), 3, 3))
        H[:, _TRI[0], _TRI[1]] = self.rows["H"]
        H[:, _TRI[1], _TRI[0]] = self.rows["H"]
        return H

    @property
    def g(self) -> np.ndarray:
        return self.rows["g"]

    def point_information(self) -> np.ndarray:
        """(P, 3, 3): H per point, the information matrix of a point prior (BundleAdjustment(..., point_priors=(ids, pts, infos)))."""
        return self.H

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

    def point_covariance(self) -> np.ndarray:
        """(P, 3, 3): inverse of H per point, the covariance of the point with camera and poses held constant (Ceres units:
        unit-variance pixel residuals).  NaN where H is not positive definite."""
        out = np.full((len(self.rows), 3, 3), np.nan)
        for k, Hk in enumerate(self.H):
            try:
                L = np.linalg.cholesky(Hk)
            except np.linalg.LinAlgError:
                continue
            Li = np.linalg.inv(L)
            out[k] = Li.T @ Li
        return out


def intersectPoints(cam, views, u, v, mcx, mcy, pt, fr, pts0, config, spx, scale, spy=None, options: Optional[capi.Options] = None,
                    inlierThreshold: float = 1.0) -> IntersectionResult:
    """Intersect every point against the constant camera block `cam` (17 values, layout of lifcal_ba_problem.cam) and the constant
    poses `views` (F, 6); pts0 (P, 3) are the start values.  Observations as in capi.ProblemArrays, in any order: the observations
    of a point are summed in the order given.  The result of a point depends on its own observations only, bit for bit."""
    lib = capi.load_library()
    if options is None:
        options = capi.Options(); lib.lifcal_ba_default_options(C.byref(options))
    f8 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    u4 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.uint32).reshape(-1))
    u, v, mcx, mcy, pt, fr = f8(u), f8(v), f8(mcx), f8(mcy), u4(pt), u4(fr)
    cam, views, pts = f8(cam), f8(views), f8(pts0).copy()
    if not (len(u) == len(v) == len(mcx) == len(mcy) == len(pt) == len(fr)):
        raise LifcalError("intersectPoints: observation arrays differ in length")
    if len(cam) != 17 or len(pts) % 3 or len(views) % 6:
        raise LifcalError("intersectPoints: cam has 17 values, views 6 per frame, pts0 3 per point")
    p = capi.IntersectProblem()
    p.n_obs, p.n_frames, p.n_points = len(u), len(views) // 6, len(pts) // 3
    p.u, p.v, p.mcx, p.mcy, p.pt, p.fr = capi.as_dptr(u), capi.as_dptr(v), capi.as_dptr(mcx), capi.as_dptr(mcy), capi.as_uptr(pt), capi.as_uptr(fr)
    p.cam, p.views, p.pts = capi.as_dptr(cam), capi.as_dptr(views), capi.as_dptr(pts)
    p.spx, p.spy, p.scale, p.config = float(spx), float(spx if spy is None else spy), float(scale), int(config)
    rows = np.zeros(p.n_points, capi.INTERSECT_POINT_DTYPE)
    seconds = C.c_double(0.0)
    _check(lib, lib.lifcal_intersect_points(C.byref(p), C.byref(options), float(inlierThreshold), rows.ctypes.data, C.byref(seconds)), "lifcal_intersect_points")
    return IntersectionResult(pts.reshape(-1, 3), rows, float(seconds.value), float(inlierThreshold))
