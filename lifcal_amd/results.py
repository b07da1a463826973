"""Host mirror of the reference's result writers (CameraCalibration::store*, src/CameraCalibration.cpp:1131-1287, :1296-1617) over
include/lifcal_io.h.  Host code inside liblifcal_ba.so; no GPU needed."""
from __future__ import annotations

import ctypes as C
import os
from typing import Sequence

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError


def camera_model(image_size: Sequence[int], pixel_size: float, camera: Sequence[float], config: int) -> capi.CameraModel:
    """camera[] as performBundleAdjustment leaves it (fL, bL0, B, cx, cy, radial.., tangential..) -> the members the
    reference copies it into (:965-988)."""
    n_rad = config & 3
    tan = bool(config & 0x004)
    m = capi.CameraModel()
    m.image_width, m.image_height, m.pixel_size = int(image_size[0]), int(image_size[1]), float(pixel_size)
    m.fL, m.bL0, m.B, m.cx, m.cy = (float(camera[i]) for i in range(5))
    m.n_radial = n_rad
    for i in range(n_rad):
        m.radial[i] = float(camera[5 + i])
    m.tangential = 1 if tan else 0
    if tan:
        m.tangential_dist[0], m.tangential_dist[1] = float(camera[5 + n_rad]), float(camera[6 + n_rad])
    m.ml_center_adjustment = 1 if config & 0x800 else 0
    return m


def _ok(rc, what):
    if rc != 0:
        raise LifcalError(f"{what}: {capi.load_library().lifcal_ba_last_error().decode() or 'cannot write'}")


def storeCameraModel(dir_results: str, model: capi.CameraModel):
    _ok(capi.load_library().lifcal_write_camera_model(os.path.join(dir_results, "CameraModel.xml").encode(), C.byref(model)), "storeCameraModel")


def storeExtrinsicOrientations(dir_results: str, frame_ids, views):
    ids = np.ascontiguousarray(frame_ids, np.int32); v = np.ascontiguousarray(views, np.float64).reshape(-1)
    _ok(capi.load_library().lifcal_write_extrinsic_orientations_xml(os.path.join(dir_results, "extrinsicOrientations.xml").encode(), len(ids),
                                                                    ids.ctypes.data_as(capi._iptr), capi.as_dptr(v)), "storeExtrinsicOrientations")


def storeExtrinsicOrientationsTxt(dir_results: str, frame_ids, views):
    ids = np.ascontiguousarray(frame_ids, np.int32); v = np.ascontiguousarray(views, np.float64).reshape(-1)
    _ok(capi.load_library().lifcal_write_extrinsic_orientations_txt(os.path.join(dir_results, "ExtrinsicOrientations.txt").encode(), len(ids),
                                                                    ids.ctypes.data_as(capi._iptr), capi.as_dptr(v)), "storeExtrinsicOrientationsTxt")


def storeRawImagePointsCsv(dir_results: str, frame_ids, fr, u, v, x_proj, y_proj, pt):
    ids = np.ascontiguousarray(frame_ids, np.int32)
    fr = np.ascontiguousarray(fr, np.uint32); pt = np.ascontiguousarray(pt, np.uint32)
    arrs = [np.ascontiguousarray(a, np.float64) for a in (u, v, x_proj, y_proj)]
    _ok(capi.load_library().lifcal_write_raw_image_points_csv(os.path.join(dir_results, "rawImagePoints.csv").encode(), len(fr), len(ids), ids.ctypes.data_as(capi._iptr),
                                                              capi.as_uptr(fr), *[capi.as_dptr(a) for a in arrs], capi.as_uptr(pt)), "storeRawImagePointsCsv")


def storeProtocol(dir_results: str, model: capi.CameraModel, config: int, stats):
    p = capi.Protocol()
    p.model = model
    p.refine_poses = 1 if config & 0x100 else 0
    p.refine_points = 1 if config & 0x400 else 0   # the flag as set (:1595), whether or not poses were refined
    p.robust_cost = 1 if config & 0x200 else 0
    p.std_x, p.std_y, p.mae_x, p.mae_y = stats.std_x, stats.std_y, stats.mae_x, stats.mae_y
    _ok(capi.load_library().lifcal_write_protocol(os.path.join(dir_results, "calibrationProtocol.txt").encode(), C.byref(p)), "storeProtocol")


def storeObjectCoordinates(dir_results: str, pts):
    """objectCoordinates.ply (:1131-1144)"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3)
    _ok(capi.load_library().lifcal_write_object_coordinates_ply(os.path.join(dir_results, "objectCoordinates.ply").encode(), len(p), capi.as_dptr(p)), "storeObjectCoordinates")


def storeObjectCoordinatesWithCOLMAPIDs(dir_results: str, colmap_ids, pts):
    """objectCoordinatesWithCOLMAPIDs.txt (:1146-1152)"""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 3); ids = np.ascontiguousarray(colmap_ids, np.int32).reshape(-1)
    if len(ids) != len(p):
        raise LifcalError("storeObjectCoordinatesWithCOLMAPIDs: one id per point")
    _ok(capi.load_library().lifcal_write_object_coordinates_colmap_ids(os.path.join(dir_results, "objectCoordinatesWithCOLMAPIDs.txt").encode(), len(p),
                                                                       ids.ctypes.data_as(capi._iptr), capi.as_dptr(p)), "storeObjectCoordinatesWithCOLMAPIDs")


def storeCameraOrientationsPly(dir_results: str, views, image_size: Sequence[int], camera: Sequence[float], pixel_size_tot_foc: float):
    """cameraOrientations.ply (:1154-1216): one frustum per frame, for viewing the poses next to the point cloud"""
    v = np.ascontiguousarray(views, np.float64).reshape(-1)
    _ok(capi.load_library().lifcal_write_camera_orientations_ply(os.path.join(dir_results, "cameraOrientations.ply").encode(), len(v) // 6, capi.as_dptr(v),
                                                                 int(image_size[0]), int(image_size[1]), float(camera[3]), float(camera[4]), float(camera[0]),
                                                                 float(pixel_size_tot_foc)), "storeCameraOrientationsPly")


def storeCameraCoordinates(dir_results: str, folder: str, frame_ids, fr, xyz):
    """<dir_results>/<folder>/cameraCoordinates_%04d.ply, one file per frame (:1218-1287).  folder: "refCameraCoordinates" with
    ref_c of BundleAdjustment.objectSpaceStats, "projectedCameraCoordinates" with proj_c; fr: frame index per point."""
    d = os.path.join(dir_results, folder)
    os.makedirs(d, exist_ok=True)
    fr = np.asarray(fr).reshape(-1); p = np.asarray(xyz, np.float64).reshape(-1, 3)
    if len(fr) != len(p):
        raise LifcalError("storeCameraCoordinates: one frame index per point")
    lib = capi.load_library()
    for f, fid in enumerate(np.asarray(frame_ids).reshape(-1)):
        sel = np.ascontiguousarray(p[fr == f])
        _ok(lib.lifcal_write_camera_coordinates_ply(d.encode(), int(fid), len(sel), capi.as_dptr(sel)), "storeCameraCoordinates")


def storeFusedCloudPly(dir_results: str, xyz, name: str = "fusedCloud.ply"):
    """The cloud of DepthMaps.fuseMaps (FusedCloud.xyz, world coordinates) in the format of objectCoordinates.ply (:1131-1144);
    a caller writes it next to the per-frame clouds of storeCameraCoordinates (:1218-1287)."""
    if hasattr(xyz, "cpu"):
        xyz = xyz.cpu().numpy()
    p = np.ascontiguousarray(xyz, np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise LifcalError("storeFusedCloudPly: xyz must be (n, 3)")
    _ok(capi.load_library().lifcal_write_object_coordinates_ply(os.path.join(dir_results, name).encode(), len(p), capi.as_dptr(p)), "storeFusedCloudPly")


def _group_csv(path: str, id_header: str, table, ids=None, xy=None):
    rows = np.ascontiguousarray(table.rows if hasattr(table, "rows") else table, capi.GROUP_STATS_DTYPE)
    ids = None if ids is None else np.ascontiguousarray(ids, np.int32).reshape(-1)
    xy = None if xy is None else np.ascontiguousarray(xy, np.float64).reshape(-1)
    if (ids is not None and len(ids) != len(rows)) or (xy is not None and len(xy) != 2 * len(rows)):
        raise LifcalError("storeGroupStatsCsv: one id and one (x, y) per row")
    _ok(capi.load_library().lifcal_write_group_stats_csv(path.encode(), id_header.encode(), len(rows), ids.ctypes.data_as(capi._iptr) if ids is not None else None,
                                                         capi.as_dptr(xy) if xy is not None else None, rows.ctypes.data), "storeGroupStatsCsv")


def storeGroupStatsCsv(path: str, id_header: str, table, ids=None, xy=None):
    """one table of BundleAdjustment.residualReport / residualGroups as CSV (lifcal_write_group_stats_csv): empty groups are left out"""
    _group_csv(path, id_header, table, ids, xy)


def storeResidualReport(dir_results: str, frame_ids, report):
    """residualsPerFrame.csv (frame.id per row), residualsPerPoint.csv and residualsPerLens.csv (with the lens centres) of a
    BundleAdjustment.residualReport; no reference counterpart."""
    _group_csv(os.path.join(dir_results, "residualsPerFrame.csv"), "frame", report.per_frame, ids=frame_ids)
    _group_csv(os.path.join(dir_results, "residualsPerPoint.csv"), "point", report.per_point)
    _group_csv(os.path.join(dir_results, "residualsPerLens.csv"), "lens", report.per_lens, xy=report.lens_xy)
