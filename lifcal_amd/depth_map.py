"""The virtual-image depth map from the raw-pixel depth, over include/lifcal_depthmap.h: what
estimateRawDepth measures per raw pixel, resampled onto the virtual-image grid in the encoding of the depth PNGs, which is what
depth.DepthMaps (sample, backProjectMaps, checkMaps, fuseMaps) consumes.

The resampling runs inside liblifcal_ba.so on the GPU; there is no Python or CPU fallback for it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError

STATUS_MEASURED, STATUS_FILLED, STATUS_EMPTY, STATUS_REJECTED = range(4)
OPTION_NAMES = tuple(n for n, _ in capi.DepthMapOptions._fields_)


def _check(rc: int, what: str):
    if rc < 0:
        lib = capi.load_library()
        err = LifcalError(f"{what}: {lib.lifcal_ba_strerror(rc).decode()} ({rc}) {lib.lifcal_ba_last_error().decode()}")
        err.code = rc
        raise err


def make_options(**options) -> capi.DepthMapOptions:
    """lifcal_depthmap_options from keywords (scale, out_width, out_height, min_support, fill_rounds, fill_min_neighbours, tol_iv,
    iv_min); what is not given stays 0 and takes the library's default."""
    o = capi.DepthMapOptions()
    for k, v in options.items():
        if k not in OPTION_NAMES:
            raise TypeError(f"depthMapFromRaw: unknown option {k!r}")
        setattr(o, k, v)
    return o


@dataclass
class VirtualDepthMap:
    """inv_depth: (h, w) float32, NaN without a value; depth16: (h, w) uint16 in the depth PNG's encoding (int16 bits when it is a
    torch tensor); status: (h, w) uint8; support: (h, w) uint16 (likewise).  numpy arrays, or torch tensors on the grid's device
    with device_out.  counts: cells per status; n_samples: raw pixels used; seconds: device time of the kernels."""
    inv_depth: object
    depth16: object
    status: object
    support: object
    counts: np.ndarray
    seconds: float
    n_samples: int
    scale: int

    def to_depth_maps(self, depth_maps, index: int = 0):
        """depth16 as map `index` of a depth.DepthMaps handle of the same size (lifcal_depth_set_maps; device to device when the
        map is on the device)"""
        depth_maps.setMaps(self.depth16, first=int(index))
        return depth_maps

    def total_focus(self, grid, image, white=None, **options):
        """The total-focus image of the raw image at this map's depths (total_focus.totalFocusImage with this map's inv_depth and
        scale, whose other options pass through).  The maps come back on the device when this map is there."""
        from . import total_focus
        options.setdefault("device_out", hasattr(self.inv_depth, "data_ptr"))
        options.update(scale=self.scale, out_width=int(self.inv_depth.shape[1]), out_height=int(self.inv_depth.shape[0]))
        return total_focus.totalFocusImage(grid, image, self.inv_depth, white=white, **options)


def checkDepthMap(params: capi.MlaParams, width: int, height: int, **options) -> capi.DepthMapPlan:
    """lifcal_depthmap_check: the argument checks of depthMapFromRaw for a grid with these parameters; needs no device."""
    lib = capi.load_library()
    plan = capi.DepthMapPlan()
    opt = make_options(**options)
    _check(lib.lifcal_depthmap_check(C.byref(params), int(width), int(height), C.byref(opt), C.byref(plan)), "lifcal_depthmap_check")
    return plan


def depthMapFromRaw(grid, inv_depth, device_out: bool = False, **options) -> VirtualDepthMap:
    """lifcal_depthmap_from_raw on the grid's device.  inv_depth: (H, W) float32 as estimateRawDepth wrote it, a numpy array or a
    torch tensor on that device.  device_out: the four maps are torch tensors on the device."""
    lib = capi.load_library()
    h, w = grid.height, grid.width
    if hasattr(inv_depth, "data_ptr"):   # torch tensor
        import torch
        iv = inv_depth
        if tuple(iv.shape) != (h, w) or iv.dtype != torch.float32 or not iv.is_cuda or not iv.is_contiguous():
            raise ValueError("inv_depth: a contiguous (height, width) float32 tensor on the grid's device")
        torch.cuda.synchronize(iv.device)
        ptr_in, on_device = iv.data_ptr(), 1
    else:
        iv = np.ascontiguousarray(inv_depth, np.float32)
        if iv.shape != (h, w):
            raise ValueError("inv_depth: a (height, width) float32 array of the grid's size")
        ptr_in, on_device = iv.ctypes.data, 0
    opt = make_options(**options)
    plan = checkDepthMap(grid.params, w, h, **options)
    shape = (int(plan.out_height), int(plan.out_width))
    res = capi.DepthMapResult()
    if device_out:
        import torch
        dev = torch.device("cuda", int(getattr(grid, "device", 0)))
        out_iv = torch.empty(shape, dtype=torch.float32, device=dev); d16 = torch.empty(shape, dtype=torch.int16, device=dev)
        st = torch.empty(shape, dtype=torch.uint8, device=dev); sup = torch.empty(shape, dtype=torch.int16, device=dev)
        torch.cuda.synchronize(dev)
        ptr = lambda t: t.data_ptr()
    else:
        out_iv = np.zeros(shape, np.float32); d16 = np.zeros(shape, np.uint16); st = np.zeros(shape, np.uint8); sup = np.zeros(shape, np.uint16)
        ptr = lambda a: a.ctypes.data
    res.out_on_device = 1 if device_out else 0
    res.inv_depth, res.depth16, res.status, res.support = ptr(out_iv), ptr(d16), ptr(st), ptr(sup)
    _check(lib.lifcal_depthmap_from_raw(grid._h, ptr_in, on_device, C.byref(opt), C.byref(res)), "lifcal_depthmap_from_raw")
    del iv
    return VirtualDepthMap(out_iv, d16, st, sup, np.array(res.count[:], np.uint64), float(res.seconds), int(res.n_samples), int(plan.options.scale))
