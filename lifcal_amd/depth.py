"""Host mirror of the two ends of the virtual-depth data flow over include/lifcal_depth.h.

    readDepthData()                  <- CameraCalibration::readDepthData            (src/CameraCalibration.cpp:350-451)
    DepthMaps.sample()               <- its per-point part for already decoded images (:385-448)
    DepthMaps.backProjectPoints()    <- CameraModel::projectPointBack as storeResults uses it (src/CameraModel.h:26-81, :1274-1285)
    DepthMaps.backProjectMaps()      <- the same for every pixel of a batch of depth maps (metric point cloud of a frame)
    projectPoints()                  the forward model projectPointBack inverts: 3D point -> (x_v, y_v, virtual depth)
    DepthMaps.checkMaps()            the maps of neighbouring frames against each other through the camera and the poses
    DepthMaps.fuseMaps()             one cloud from a batch of maps, filtered by that agreement
The arithmetic runs on the GPU inside liblifcal_ba.so; there is no Python or CPU fallback.  Only the PNG container is decoded
here (zlib + struct, 16-bit grayscale non-interlaced files as the reference's depth images are).
"""
from __future__ import annotations

import ctypes as C
import os
import struct
import zlib
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError


def _check(rc: int, what: str):
    if rc != 0:
        lib = capi.load_library()
        err = LifcalError(f"{what}: {lib.lifcal_ba_strerror(rc).decode()} ({rc}) {lib.lifcal_ba_last_error().decode()}")
        err.code = rc
        raise err


def depth_camera(cam, config: int, spx: float, spy: Optional[float] = None) -> capi.DepthCamera:
    """cam[17] in the layout of lifcal_ba_problem.cam, the nRadial / tangential bits of config, pixelSize_totFoc."""
    c = np.asarray(cam, np.float64).reshape(-1)
    if c.shape[0] != 17:
        raise LifcalError("depth_camera: cam must have 17 entries")
    d = capi.DepthCamera()
    for i in range(17):
        d.cam[i] = float(c[i])
    d.spx = float(spx); d.spy = float(spx if spy is None else spy)
    d.config = int(config) & 0x7
    return d


@dataclass
class BackProjection:
    """p_c: (n, 3) camera coordinates; p_w: (n, 3) world coordinates or None; jac: (n, 3, 17) d p_c / d cam or None; dpc_dv: (n, 3)
    or None; cov_pc: (n, 6) upper triangle (xx, xy, xz, yy, yz, zz) or None; n_invalid: points with vdepth <= 0 (NaN rows)."""
    p_c: np.ndarray
    p_w: Optional[np.ndarray]
    jac: Optional[np.ndarray]
    dpc_dv: Optional[np.ndarray]
    cov_pc: Optional[np.ndarray]
    n_invalid: int


@dataclass
class DenseBackProjection:
    """xyz: (count, H, W, 3); z, sigma_z: (count, H, W) or None (numpy arrays, or torch tensors on the device when
    device_out=True); n_invalid: pixels without a valid value (NaN); seconds: device time of the kernel."""
    xyz: object
    z: object
    sigma_z: object
    n_invalid: int
    seconds: float


def backProjectPoints(x, y, vdepth, cam, config: int, spx: float, spy: Optional[float] = None, fr=None, views=None, want_jacobian: bool = False,
                      cam_cov=None, sigma_v: float = 0.0, device: int = 0) -> BackProjection:
    """CameraModel::projectPointBack for a list of image points of the virtual image, in fp64 and bit-identical to the reference's
    order of operations.  With fr and views: also p_w = R^T (p_c - t).  want_jacobian: d p_c / d cam (the fixed ten undistortion
    sweeps differentiated as executed) and d p_c / d vdepth.  cam_cov (17 x 17, Covariance.camera): cov_pc = J G J^T + sigma_v^2 ..."""
    lib = capi.load_library()
    x = np.ascontiguousarray(x, np.float64).reshape(-1); y = np.ascontiguousarray(y, np.float64).reshape(-1)
    vd = np.ascontiguousarray(vdepth, np.float64).reshape(-1)
    n = len(x)
    if len(y) != n or len(vd) != n:
        raise LifcalError("backProjectPoints: x, y, vdepth differ in length")
    dc = depth_camera(cam, config, spx, spy)
    io = capi.DepthPoints()
    io.n = n; io.x, io.y, io.vdepth = capi.as_dptr(x), capi.as_dptr(y), capi.as_dptr(vd)
    p_c = np.zeros((n, 3)); io.p_c = capi.as_dptr(p_c)
    p_w = jac = dv = cov = None
    keep = []
    if fr is not None or views is not None:
        if fr is None or views is None:
            raise LifcalError("backProjectPoints: fr and views go together")
        fr_a = np.ascontiguousarray(fr, np.uint32).reshape(-1); vw = np.ascontiguousarray(views, np.float64).reshape(-1)
        if len(fr_a) != n:
            raise LifcalError("backProjectPoints: fr differs in length")
        keep += [fr_a, vw]
        io.fr, io.views, io.n_frames = capi.as_uptr(fr_a), capi.as_dptr(vw), len(vw) // 6
        p_w = np.zeros((n, 3)); io.p_w = capi.as_dptr(p_w)
    if want_jacobian or cam_cov is not None:
        jac = np.zeros((n, 3, 17)); dv = np.zeros((n, 3))
        io.jac, io.dpc_dv = capi.as_dptr(jac), capi.as_dptr(dv)
    if cam_cov is not None:
        G = np.ascontiguousarray(cam_cov, np.float64).reshape(-1)
        if G.shape[0] != 17 * 17:
            raise LifcalError("backProjectPoints: cam_cov must be 17 x 17")
        keep.append(G)
        io.cam_cov = capi.as_dptr(G); io.sigma_v = float(sigma_v)
        cov = np.zeros((n, 6)); io.cov_pc = capi.as_dptr(cov)
    _check(lib.lifcal_depth_back_project_points(int(device), C.byref(dc), C.byref(io)), "lifcal_depth_back_project_points")
    return BackProjection(p_c, p_w, jac, dv, cov, int(io.n_invalid))


STEP_IV = 1.0 / 65535.0   # one raw step of inverse virtual depth


@dataclass
class ForwardProjection:
    """x, y: (n,) virtual-image coordinates; vdepth: (n,); NaN rows for invalid points, n_invalid of them."""
    x: np.ndarray
    y: np.ndarray
    vdepth: np.ndarray
    n_invalid: int


@dataclass
class ViewCheck:
    """support, conflict: (count, H, W) uint8 (numpy, or torch tensors with device_out); pair: (count, 2 span) structured array
    (_capi.DEPTH_PAIR_DTYPE), slot j of source s is target s + j - span for j < span, s + j - span + 1 otherwise."""
    support: object
    conflict: object
    pair: np.ndarray
    span: int
    seconds: float

    def rms_steps(self) -> np.ndarray:
        """RMS of e over the consistent pixels of every pair slot, in raw steps of inverse virtual depth; NaN without any"""
        n = self.pair["n_consistent"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sqrt(self.pair["sum_e2"] / n) / STEP_IV

    def target(self, s: int, j: int) -> int:
        return s + j - self.span + (1 if j >= self.span else 0)


@dataclass
class FusedCloud:
    """xyz: (n, 3) world coordinates; n_merged: (n,) uint8 = 1 + support; src: (n,) uint32 = (m - first) H W + row W + col, ascending;
    n_points: the number that qualified (n = min(n_points, capacity))."""
    xyz: object
    n_merged: object
    src: object
    n_points: int
    seconds: float


def projectPoints(p, cam, config: int, spx: float, spy: Optional[float] = None, fr=None, views=None, device: int = 0) -> ForwardProjection:
    """The forward model projectPointBack inverts, in closed form: 3D points (n, 3) -> (x_v, y_v, virtual depth).  With fr and
    views the points are world points (p_c = R p + t), without them camera coordinates."""
    p = np.ascontiguousarray(p, np.float64)
    if p.size % 3 != 0 or (p.ndim > 1 and p.shape[-1] != 3):
        raise LifcalError("projectPoints: p must be (n, 3)")
    p = p.reshape(-1)
    n = len(p) // 3
    dc = depth_camera(cam, config, spx, spy)
    io = capi.DepthForward()
    io.n = n; io.p = capi.as_dptr(p)
    keep = []
    if fr is not None or views is not None:
        if fr is None or views is None:
            raise LifcalError("projectPoints: fr and views go together")
        fr_a = np.ascontiguousarray(fr, np.uint32).reshape(-1); vw = np.ascontiguousarray(views, np.float64).reshape(-1)
        if len(fr_a) != n:
            raise LifcalError("projectPoints: fr differs in length")
        keep += [fr_a, vw]
        io.fr, io.views, io.n_frames = capi.as_uptr(fr_a), capi.as_dptr(vw), len(vw) // 6
    x = np.zeros(n); y = np.zeros(n); v = np.zeros(n)
    io.x, io.y, io.vdepth = capi.as_dptr(x), capi.as_dptr(y), capi.as_dptr(v)
    _check(capi.load_library().lifcal_depth_project_points(int(device), C.byref(dc), C.byref(io)), "lifcal_depth_project_points")
    return ForwardProjection(x, y, v, int(io.n_invalid))


class DepthMaps:
    """The depth maps of some frames on the device: [height][width] uint16 each, as cv::imread(..., IMREAD_UNCHANGED) returns the
    reference's depth PNGs; pixel (col, row) is the virtual-image point (x_v, y_v) = (col, row)."""

    def __init__(self, width: int, height: int, max_maps: int = 1, device: int = 0):
        self._lib = capi.load_library()
        self._h = C.c_void_p()
        self.width, self.height, self.max_maps, self.device = int(width), int(height), int(max_maps), int(device)
        _check(self._lib.lifcal_depth_create(self.width, self.height, self.max_maps, self.device, C.byref(self._h)), "lifcal_depth_create")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lifcal_depth_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def setMaps(self, maps, first: int = 0):
        """maps: (count, H, W) or (H, W), a numpy array of uint16 or a torch tensor (uint16 / int16) on the handle's device, which is
        copied device to device.  A shape other than the handle's is an invalid argument.  The torch wheel carries its own HIP
        runtime and only the first runtime started in a process sees the GPU: a process that hands tensors over (or asks for
        device_out) lets torch initialise the GPU before the first call into this library."""
        if hasattr(maps, "data_ptr"):   # torch tensor
            t = maps
            shape = tuple(t.shape)
            if t.element_size() != 2 or t.is_floating_point() or not t.is_contiguous():
                raise LifcalError("setMaps: the tensor must be contiguous 16-bit integers")
            if not t.is_cuda or (t.device.index or 0) != self.device:
                raise LifcalError("setMaps: the tensor must live on the handle's device")
            import torch
            torch.cuda.synchronize(t.device)
            ptr, on_device, keep = C.c_void_p(t.data_ptr()), 1, t
        else:
            a = np.ascontiguousarray(maps, np.uint16)
            shape = a.shape
            ptr, on_device, keep = C.c_void_p(a.ctypes.data), 0, a
        if len(shape) == 2:
            shape = (1,) + tuple(shape)
        if len(shape) != 3 or shape[1] != self.height or shape[2] != self.width:
            err = LifcalError(f"setMaps: maps of shape {tuple(shape)} do not match the handle's {self.height} x {self.width} (-1)")
            err.code = -1   # LIFCAL_BA_ERR_INVALID_ARG
            raise err
        _check(self._lib.lifcal_depth_set_maps(self._h, int(first), int(shape[0]), ptr, on_device), "lifcal_depth_set_maps")
        del keep

    def sample(self, x, y, map_index=0):
        """readDepthData's per-point part (:385-448): returns (vdepth, counts) with counts.direct / .interpolated / .failed.
        A point whose pixel lies outside the image gives -1 (the reference reads out of bounds there)."""
        x = np.ascontiguousarray(x, np.float64).reshape(-1); y = np.ascontiguousarray(y, np.float64).reshape(-1)
        n = len(x)
        mi = np.ascontiguousarray(np.broadcast_to(np.asarray(map_index, np.int32), (n,)) if np.ndim(map_index) == 0 else map_index, np.int32).reshape(-1)
        if len(y) != n or len(mi) != n:
            raise LifcalError("sample: x, y, map_index differ in length")
        out = np.zeros(n)
        counts = capi.DepthSampleCounts()
        _check(self._lib.lifcal_depth_sample(self._h, n, capi.as_dptr(x), capi.as_dptr(y), mi.ctypes.data_as(capi._iptr), capi.as_dptr(out), C.byref(counts)),
               "lifcal_depth_sample")
        return out, counts

    def backProjectPoints(self, x, y, vdepth, cam, config: int, spx: float, **kw) -> BackProjection:
        return backProjectPoints(x, y, vdepth, cam, config, spx, device=self.device, **kw)

    def backProjectMaps(self, cam, config: int, spx: float, spy: Optional[float] = None, first: int = 0, count: Optional[int] = None, eval: int = 0,
                        out_double: bool = False, frames=None, views=None, cam_cov=None, sigma_v: float = 0.0, want_xyz: bool = True, want_z: bool = False,
                        want_sigma_z: bool = False, device_out: bool = False) -> DenseBackProjection:
        """Metric 3D of every pixel of maps first .. first+count-1 (direct decoding rule only; invalid pixels give NaN).
        eval 0: fp64 in the reference's order; eval 1: fp32 evaluation.  frames (one index per map) and views: world coordinates.
        cam_cov: 17 x 17 camera covariance, needed for sigma_z.  device_out: outputs are torch tensors on the handle's device."""
        count = self.max_maps - first if count is None else int(count)
        dc = depth_camera(cam, config, spx, spy)
        io = capi.DepthMapsArgs()
        io.first, io.count, io.eval, io.out_double, io.out_on_device = int(first), count, int(eval), 1 if out_double else 0, 1 if device_out else 0
        keep = []
        if frames is not None or views is not None:
            if frames is None or views is None:
                raise LifcalError("backProjectMaps: frames and views go together")
            fr_a = np.ascontiguousarray(frames, np.uint32).reshape(-1); vw = np.ascontiguousarray(views, np.float64).reshape(-1)
            if len(fr_a) != count:
                raise LifcalError("backProjectMaps: one frame index per map")
            keep += [fr_a, vw]
            io.frame, io.views, io.n_frames = capi.as_uptr(fr_a), capi.as_dptr(vw), len(vw) // 6
        if cam_cov is not None:
            G = np.ascontiguousarray(cam_cov, np.float64).reshape(-1)
            if G.shape[0] != 17 * 17:
                raise LifcalError("backProjectMaps: cam_cov must be 17 x 17")
            keep.append(G)
            io.cam_cov = capi.as_dptr(G); io.sigma_v = float(sigma_v)
        n = max(count, 0)
        shape3, shape1 = (n, self.height, self.width, 3), (n, self.height, self.width)
        if device_out:
            import torch
            dt = torch.float64 if out_double else torch.float32
            dev = torch.device("cuda", self.device)
            mk = lambda shp: torch.empty(shp, dtype=dt, device=dev)
            ptr = lambda t: C.c_void_p(t.data_ptr())
            torch.cuda.synchronize(dev)
        else:
            dt = np.float64 if out_double else np.float32
            mk = lambda shp: np.empty(shp, dt)
            ptr = lambda a: C.c_void_p(a.ctypes.data)
        xyz = mk(shape3) if want_xyz else None
        z = mk(shape1) if want_z else None
        sz = mk(shape1) if want_sigma_z else None
        if n:
            io.xyz = ptr(xyz) if xyz is not None else None
            io.z = ptr(z) if z is not None else None
            io.sigma_z = ptr(sz) if sz is not None else None
        _check(self._lib.lifcal_depth_back_project_maps(self._h, C.byref(dc), C.byref(io)), "lifcal_depth_back_project_maps")
        return DenseBackProjection(xyz, z, sz, int(io.n_invalid), float(io.seconds))

    def projectPoints(self, p, cam, config: int, spx: float, **kw) -> ForwardProjection:
        return projectPoints(p, cam, config, spx, device=self.device, **kw)

    def _views_io(self, io, who: str, frame, views, span, tol_steps, first, count):
        count = self.max_maps - int(first) if count is None else int(count)
        fr_a, vw = views_arguments(who, count, frame, views, span, tol_steps)
        io.first, io.count, io.span, io.n_frames = int(first), count, int(span), len(vw) // 6
        io.frame, io.views, io.tol_iv = capi.as_uptr(fr_a), capi.as_dptr(vw), float(tol_steps) * STEP_IV
        return count, (fr_a, vw)

    def checkMaps(self, cam, config: int, spx: float, frame, views, span: int = 1, tol_steps: float = 4.0, first: int = 0, count: Optional[int] = None,
                  spy: Optional[float] = None, want_support: bool = True, want_conflict: bool = True, device_out: bool = False) -> ViewCheck:
        """Every map of first .. first+count-1 against the maps of the batch at most `span` away, through the camera and the poses
        views[frame[m]]: per source pixel the number of targets that agree (support) and that see through it (conflict), per
        (source, target) the class counts and the sums of e = 1/v_obs - 1/v_pred over the agreeing pixels.  tol_steps: the
        tolerance in raw steps (1 / 65535) of inverse virtual depth.  device_out: support / conflict are torch tensors."""
        dc = depth_camera(cam, config, spx, spy)
        io = capi.DepthViewsArgs()
        count, keep = self._views_io(io, "checkMaps", frame, views, span, tol_steps, first, count)
        shape = (count, self.height, self.width)
        pair = np.zeros((count, 2 * int(span)), capi.DEPTH_PAIR_DTYPE)
        if device_out:
            import torch
            dev = torch.device("cuda", self.device)
            mk = lambda: torch.zeros(shape, dtype=torch.uint8, device=dev)
            ptr = lambda t: C.c_void_p(t.data_ptr())
            pair_t = torch.zeros(pair.nbytes, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            io.out_on_device, io.pair = 1, ptr(pair_t)
        else:
            mk = lambda: np.zeros(shape, np.uint8)
            ptr = lambda a: C.c_void_p(a.ctypes.data)
            io.pair = C.c_void_p(pair.ctypes.data)
        support = mk() if want_support else None
        conflict = mk() if want_conflict else None
        io.support = ptr(support) if support is not None else None
        io.conflict = ptr(conflict) if conflict is not None else None
        _check(self._lib.lifcal_depth_check_maps(self._h, C.byref(dc), C.byref(io)), "lifcal_depth_check_maps")
        if device_out:
            pair = np.frombuffer(pair_t.cpu().numpy().tobytes(), capi.DEPTH_PAIR_DTYPE).reshape(pair.shape).copy()
        del keep
        return ViewCheck(support, conflict, pair, int(span), float(io.seconds))

    def fuseMaps(self, cam, config: int, spx: float, frame, views, span: int = 1, tol_steps: float = 4.0, min_support: int = 1, max_conflict: int = 0,
                 capacity: Optional[int] = None, first: int = 0, count: Optional[int] = None, spy: Optional[float] = None, out_double: bool = False,
                 device_out: bool = False) -> FusedCloud:
        """One cloud from maps first .. first+count-1: a valid pixel with support >= min_support and conflict <= max_conflict (see
        checkMaps) that is not consistent with a lower map emits the depth-weighted mean of its own world point and those of the
        target pixels it agrees with.  Points come in ascending src.  capacity: room for that many points (default: all that
        qualify, found by a counting call first); fewer than n_points keeps the ordered prefix."""
        if min_support < 0 or max_conflict < 0 or (capacity is not None and capacity < 0):
            err = LifcalError("fuseMaps: min_support, max_conflict and capacity must not be negative (-1)")
            err.code = -1
            raise err
        dc = depth_camera(cam, config, spx, spy)
        io = capi.DepthFusionArgs()
        count, keep = self._views_io(io, "fuseMaps", frame, views, span, tol_steps, first, count)
        io.min_support, io.max_conflict, io.out_double = int(min_support), min(int(max_conflict), 0xFFFFFFFF), 1 if out_double else 0
        if capacity is None:
            io.capacity = 0
            _check(self._lib.lifcal_depth_fuse_maps(self._h, C.byref(dc), C.byref(io)), "lifcal_depth_fuse_maps")
            capacity = int(io.n_points)
        cap = int(capacity)
        if device_out:
            import torch
            dev = torch.device("cuda", self.device)
            xyz = torch.zeros((cap, 3), dtype=torch.float64 if out_double else torch.float32, device=dev)
            merged = torch.zeros(cap, dtype=torch.uint8, device=dev); src = torch.zeros(cap, dtype=torch.int32, device=dev)   # the bits of uint32
            ptr = lambda t: C.c_void_p(t.data_ptr())
            torch.cuda.synchronize(dev)
            io.out_on_device = 1
        else:
            xyz = np.zeros((cap, 3), np.float64 if out_double else np.float32)
            merged = np.zeros(cap, np.uint8); src = np.zeros(cap, np.uint32)
            ptr = lambda a: C.c_void_p(a.ctypes.data)
        io.capacity = cap
        if cap:
            io.xyz, io.n_merged, io.src = ptr(xyz), ptr(merged), ptr(src)
        _check(self._lib.lifcal_depth_fuse_maps(self._h, C.byref(dc), C.byref(io)), "lifcal_depth_fuse_maps")
        n = min(int(io.n_points), cap)
        del keep
        return FusedCloud(xyz[:n], merged[:n], src[:n], int(io.n_points), float(io.seconds))


def views_arguments(who: str, count: int, frame, views, span, tol_steps):
    """The checks checkMaps and fuseMaps make before anything reaches the device: (frame as uint32, views flat).  A bad argument
    raises LifcalError with code -1 (LIFCAL_BA_ERR_INVALID_ARG)."""
    def bad(msg):
        err = LifcalError(f"{who}: {msg} (-1)")
        err.code = -1
        return err
    if frame is None or views is None:
        raise bad("frame and views are required")
    if int(count) <= 0:
        raise bad("count must be positive")
    if int(span) != span or int(span) < 1 or int(span) > 127:
        raise bad("span must be in 1 .. 127")
    if not float(tol_steps) >= 0.0:
        raise bad("the tolerance must be a number >= 0")
    vw = np.ascontiguousarray(views, np.float64).reshape(-1)
    if len(vw) % 6 != 0:
        raise bad("views must hold six values per frame")
    f = np.asarray(frame).reshape(-1)
    if len(f) != int(count):
        raise bad("one frame index per map")
    if np.any(f < 0):
        raise bad("frame indices must not be negative")
    return np.ascontiguousarray(f, np.uint32), vw


# ------------------------------------------------------------------------------------------------ PNG container
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def read_png16(path: str) -> np.ndarray:
    """A 16-bit grayscale, non-interlaced PNG as an (H, W) uint16 array (what cv::imread(..., IMREAD_UNCHANGED) gives for the
    reference's depth images).  Any other kind of PNG is rejected: the depth coding is defined on the 16-bit values."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:8] != _PNG_SIGNATURE:
        raise LifcalError(f"read_png16: {path} is not a PNG file")
    pos, idat, header = 8, [], None
    while pos + 8 <= len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        if len(body) != length:
            raise LifcalError(f"read_png16: {path} is truncated")
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
        pos += 12 + length
    if header is None:
        raise LifcalError(f"read_png16: {path} has no IHDR chunk")
    width, height, bit_depth, color_type, compression, filter_method, interlace = header
    if bit_depth != 16 or color_type != 0:
        raise LifcalError(f"read_png16: {path} is not 16-bit grayscale (bit depth {bit_depth}, colour type {color_type})")
    if interlace != 0:
        raise LifcalError(f"read_png16: {path} is interlaced (Adam7), which is not supported")
    if compression != 0 or filter_method != 0:
        raise LifcalError(f"read_png16: {path} uses an unknown compression or filter method")
    raw = zlib.decompress(b"".join(idat))
    stride = 2 * width
    if len(raw) != height * (stride + 1):
        raise LifcalError(f"read_png16: {path} holds {len(raw)} bytes of image data, expected {height * (stride + 1)}")
    lines = np.frombuffer(raw, np.uint8).reshape(height, stride + 1)
    out = np.zeros((height, stride), np.uint8)
    prev = np.zeros(stride, np.uint8)
    for r in range(height):
        ft = int(lines[r, 0])
        cur = lines[r, 1:]
        if ft == 0:
            row = cur.copy()
        elif ft == 1:    # Sub: each of the two byte lanes is a running sum modulo 256
            row = np.cumsum(cur.reshape(-1, 2), axis=0, dtype=np.uint8).reshape(-1)
        elif ft == 2:    # Up
            row = cur + prev
        elif ft in (3, 4):   # Average / Paeth: sequential along the line
            row = np.zeros(stride, np.uint8)
            c = cur.astype(np.int32); up = prev.astype(np.int32)
            for i in range(stride):
                a = int(row[i - 2]) if i >= 2 else 0
                b = int(up[i])
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    cc = int(up[i - 2]) if i >= 2 else 0
                    p = a + b - cc
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - cc)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else cc)
                row[i] = (int(c[i]) + pred) & 0xFF
        else:
            raise LifcalError(f"read_png16: {path} has an unknown filter type {ft}")
        out[r] = row
        prev = row
    return out.view(">u2").astype(np.uint16)


def readDepthData(dir_depth_data: str, frame_ids: Sequence[int], image_points: Sequence, image_size: Sequence[int], device: int = 0):
    """CameraCalibration::readDepthData: the virtual depth of every image point of every frame from the frame's depth PNG.
    The files of the directory ending in .png are listed sorted and frame id k takes the (k - 1)-th (:369); the image must have
    image_size = (width, height) (:376).  image_points: per frame an (n_i, 2) array of (x_v, y_v).
    Returns (list of per-frame vdepth arrays, counts); -1 marks a point whose interpolation failed."""
    files = sorted(f for f in os.listdir(dir_depth_data) if f.endswith(".png"))
    if len(frame_ids) != len(image_points):
        raise LifcalError("readDepthData: one array of image points per frame")
    width, height = int(image_size[0]), int(image_size[1])
    F = len(frame_ids)
    if F == 0:
        return [], capi.DepthSampleCounts()
    with DepthMaps(width, height, F, device) as dm:
        xs, ys, mi = [], [], []
        for k, (fid, pts) in enumerate(zip(frame_ids, image_points)):
            if fid < 1 or fid > len(files):
                raise LifcalError(f"readDepthData: no depth image for frame id {fid} ({len(files)} files)")
            img = read_png16(os.path.join(dir_depth_data, files[fid - 1]))
            if img.shape != (height, width):
                raise LifcalError(f"readDepthData: wrong depth image size {img.shape[1]} x {img.shape[0]} in {files[fid - 1]}, expected {width} x {height}")
            dm.setMaps(img, first=k)
            p = np.asarray(pts, np.float64).reshape(-1, 2)
            xs.append(p[:, 0]); ys.append(p[:, 1]); mi.append(np.full(len(p), k, np.int32))
        vd, counts = dm.sample(np.concatenate(xs), np.concatenate(ys), np.concatenate(mi))
    cuts = np.cumsum([len(a) for a in xs])[:-1]
    return np.split(vd, cuts), counts


def depth_is_estimable(jac, camera_null, p_c) -> float:
    """The largest |J n| / |p_c| over the points and over the null directions n that lifcal_ba_covariance reports
    (Covariance.camera_null, null_rank x 17; jac: (n, 3, 17) from backProjectPoints).

    A variance propagated through J is meaningful only where this is ~0: the covariance is a g-inverse, and along a null direction
    the data say nothing.  In a scene without distance constraints B and bL0 are not determined on their own,
    and metric depth moves along exactly that direction, so the value is not small there; with distance constraints (or any other
    metric information) the null space is empty and the value is 0."""
    J = np.asarray(jac, np.float64).reshape(-1, 3, 17)
    N = np.asarray(camera_null, np.float64).reshape(-1, 17)
    if N.shape[0] == 0 or J.shape[0] == 0:
        return 0.0
    P = np.asarray(p_c, np.float64).reshape(-1, 3)
    ok = np.all(np.isfinite(P), axis=1)
    move = np.linalg.norm(np.einsum("nij,kj->nki", J[ok], N), axis=2)   # (n, null directions)
    return float(np.max(move / np.linalg.norm(P[ok], axis=1)[:, None])) if move.size else 0.0
