"""Virtual depth from the raw image, over include/lifcal_rawdepth.h: for every raw pixel the inverse
virtual depth from a multi-baseline plane sweep against the neighbouring micro images, and the status-0 pixels as the image
points MicroLensGrid.projectPointsToRawImage and depth.backProjectPoints take.

The sweep runs inside liblifcal_ba.so on the GPU; there is no Python or CPU fallback for it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError

STATUS_OK, STATUS_NO_LENS, STATUS_FLAT, STATUS_NO_MINIMUM, STATUS_AMBIGUOUS = range(5)
OPTION_NAMES = tuple(n for n, _ in capi.RawDepthOptions._fields_)


def _check(rc: int, what: str):
    if rc < 0:
        lib = capi.load_library()
        err = LifcalError(f"{what}: {lib.lifcal_ba_strerror(rc).decode()} ({rc}) {lib.lifcal_ba_last_error().decode()}")
        err.code = rc
        raise err


def make_options(**options) -> capi.RawDepthOptions:
    """lifcal_rawdepth_options from keywords (n_hyp, patch_radius, min_neighbours, min_contrast, iv_min, iv_max, max_baseline,
    ambiguity_ratio); what is not given stays 0 and takes the library's default."""
    o = capi.RawDepthOptions()
    for k, v in options.items():
        if k not in OPTION_NAMES:
            raise TypeError(f"estimateRawDepth: unknown option {k!r}")
        setattr(o, k, v)
    return o


def _image(raw):
    """(lifcal_rawdepth_image, what must outlive it) of a numpy array (rows may be strided) or a torch tensor on the device"""
    if hasattr(raw, "data_ptr"):   # torch tensor
        import torch
        if raw.dim() != 2 or raw.dtype not in (torch.uint8, torch.uint16, torch.int16) or not raw.is_cuda or raw.stride(1) != 1 or raw.stride(0) < raw.shape[1]:
            raise ValueError("raw image: a 2-D uint8 or uint16 tensor on the device with unit column stride")
        torch.cuda.synchronize(raw.device)
        bits = 8 if raw.dtype == torch.uint8 else 16
        return capi.RawDepthImage(raw.data_ptr(), bits, raw.shape[1], raw.shape[0], 1, raw.stride(0)), raw
    raw = np.asarray(raw)
    if raw.ndim != 2 or raw.dtype not in (np.uint8, np.uint16):
        raise ValueError("raw image: a 2-D uint8 or uint16 array (one channel)")
    if raw.strides[1] != raw.itemsize or raw.strides[0] % raw.itemsize or raw.strides[0] < raw.shape[1] * raw.itemsize:
        raw = np.ascontiguousarray(raw)
    return capi.RawDepthImage(raw.ctypes.data, 8 * raw.itemsize, raw.shape[1], raw.shape[0], 0, raw.strides[0] // raw.itemsize), raw


@dataclass
class RawPoints:
    """lifcal_rawdepth_points: the status-0 pixels as image points of the virtual image, ascending in src"""
    x: np.ndarray
    y: np.ndarray
    vdepth: np.ndarray
    src: np.ndarray      # pixel index py * width + px
    lens: np.ndarray     # index into MicroLensGrid.lenses()


@dataclass
class RawDepth:
    """inv_depth, cost: (H, W) float32; status, n_neighbours: (H, W) uint8 (numpy arrays, or torch tensors on the grid's device
    with device_out); counts: pixels per status; seconds: device time of the kernels; n_neighbours_used: neighbours per lens."""
    grid: object
    inv_depth: object
    cost: object
    status: object
    n_neighbours: object
    counts: np.ndarray
    seconds: float
    n_neighbours_used: int

    def points(self, scale: int = 1) -> RawPoints:
        lib = capi.load_library()
        iv = self.inv_depth
        if hasattr(iv, "data_ptr"):
            import torch
            torch.cuda.synchronize(iv.device)
            ptr, on_device = iv.data_ptr(), 1
        else:
            iv = np.ascontiguousarray(iv, np.float32)
            ptr, on_device = iv.ctypes.data, 0
        io = capi.RawDepthPointList(ptr, on_device, int(scale), 0, 0, None, None, None, None, None)
        _check(lib.lifcal_rawdepth_points(self.grid._h, C.byref(io)), "lifcal_rawdepth_points")
        n = int(io.n)
        out = RawPoints(np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, np.uint32), np.zeros(n, np.int32))
        if n == 0:
            return out
        io = capi.RawDepthPointList(ptr, on_device, int(scale), n, 0, capi.as_dptr(out.x), capi.as_dptr(out.y), capi.as_dptr(out.vdepth),
                                    capi.as_uptr(out.src), out.lens.ctypes.data_as(capi._iptr))
        rc = lib.lifcal_rawdepth_points(self.grid._h, C.byref(io))
        _check(rc, "lifcal_rawdepth_points")
        if rc != 0 or int(io.n) != n:
            raise LifcalError("lifcal_rawdepth_points: point count changed between the count and the fill call")
        return out

    def metric_points(self, cam, config: int, spx: float, spy: Optional[float] = None, scale: int = 1, **kw):
        """The status-0 pixels in metric camera coordinates through the calibrated camera (depth.backProjectPoints, whose
        keywords pass through): (RawPoints, BackProjection)."""
        from . import depth
        pts = self.points(scale)
        return pts, depth.backProjectPoints(pts.x, pts.y, pts.vdepth, cam, config, spx, spy, **kw)

    def depth_map(self, device_out: bool = False, **options):
        """inv_depth resampled onto the virtual-image grid in the depth PNG's encoding (depth_map.depthMapFromRaw, whose options
        pass through)."""
        from . import depth_map
        return depth_map.depthMapFromRaw(self.grid, self.inv_depth, device_out=device_out, **options)


def checkRawDepth(params: capi.MlaParams, raw, **options) -> capi.RawDepthPlan:
    """lifcal_rawdepth_check: the argument checks of estimateRawDepth for a grid with these parameters; needs no device."""
    lib = capi.load_library()
    img, keep = _image(raw)
    plan = capi.RawDepthPlan()
    opt = make_options(**options)
    _check(lib.lifcal_rawdepth_check(C.byref(params), C.byref(img), C.byref(opt), C.byref(plan)), "lifcal_rawdepth_check")
    return plan


def estimateRawDepth(grid, raw, device_out: bool = False, **options) -> RawDepth:
    """lifcal_rawdepth_estimate on the grid's device.  raw: (H, W) uint8 / uint16, a numpy array (rows may be strided) or a torch
    tensor on that device.  device_out: the four maps are torch tensors on the device."""
    lib = capi.load_library()
    img, keep = _image(raw)
    opt = make_options(**options)
    h, w = grid.height, grid.width
    res = capi.RawDepthResult()
    if device_out:
        import torch
        dev = torch.device("cuda", int(getattr(grid, "device", 0)))
        iv = torch.empty((h, w), dtype=torch.float32, device=dev); cost = torch.empty((h, w), dtype=torch.float32, device=dev)
        st = torch.empty((h, w), dtype=torch.uint8, device=dev); nn = torch.empty((h, w), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ptr = lambda t: t.data_ptr()
    else:
        iv = np.zeros((h, w), np.float32); cost = np.zeros((h, w), np.float32); st = np.zeros((h, w), np.uint8); nn = np.zeros((h, w), np.uint8)
        ptr = lambda a: a.ctypes.data
    res.out_on_device = 1 if device_out else 0
    res.inv_depth, res.cost, res.status, res.n_neighbours = ptr(iv), ptr(cost), ptr(st), ptr(nn)
    _check(lib.lifcal_rawdepth_estimate(grid._h, C.byref(img), C.byref(opt), C.byref(res)), "lifcal_rawdepth_estimate")
    return RawDepth(grid, iv, cost, st, nn, np.array(res.count[:], np.uint64), float(res.seconds), int(res.n_neighbours_used))
