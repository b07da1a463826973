"""The total-focus image from the raw image and the virtual-image depth map, over include/lifcal_totalfocus.h (DESIGN.md section
7v): the all-in-focus picture on the virtual-image grid, whose pixels are the image points (x, y) of projectPointsToRawImage,
RawDepth.points and DepthMaps.sample, and what a feature detector or an SfM run takes as its input.

The gather runs inside liblifcal_ba.so on the GPU; there is no Python or CPU fallback for it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError
from .raw_depth import _image

STATUS_OK, STATUS_NO_DEPTH, STATUS_NO_LENS, STATUS_DEFAULT_DEPTH = range(4)
OPTION_NAMES = tuple(n for n, _ in capi.TotalFocusOptions._fields_)


def _check(rc: int, what: str):
    if rc < 0:
        lib = capi.load_library()
        err = LifcalError(f"{what}: {lib.lifcal_ba_strerror(rc).decode()} ({rc}) {lib.lifcal_ba_last_error().decode()}")
        err.code = rc
        raise err


def make_options(**options) -> capi.TotalFocusOptions:
    """lifcal_totalfocus_options from keywords (scale, out_width, out_height, min_lenses, white_level, margin, max_reach, iv_min,
    default_iv); what is not given stays 0 and takes the library's default."""
    o = capi.TotalFocusOptions()
    for k, v in options.items():
        if k not in OPTION_NAMES:
            raise TypeError(f"totalFocusImage: unknown option {k!r}")
        setattr(o, k, v)
    return o


@dataclass
class TotalFocusImage:
    """image: (h, w) uint8 or uint16 like the raw image (int16 bits when it is a 16-bit torch tensor); n_lenses, status: (h, w)
    uint8.  numpy arrays, or torch tensors on the grid's device with device_out.  counts: cells per status; seconds: device time of
    the kernel."""
    image: object
    n_lenses: object
    status: object
    counts: np.ndarray
    seconds: float
    scale: int


def checkTotalFocus(params: capi.MlaParams, image_shape, bits: int, depth_shape, white_shape=None, **options) -> capi.TotalFocusPlan:
    """lifcal_totalfocus_check: the argument checks of totalFocusImage for a grid with these parameters, a raw image of
    image_shape = (height, width) and `bits`, a white image of white_shape (None: no white image) and a depth map of depth_shape;
    needs no device."""
    lib = capi.load_library()
    stand_in = np.zeros(1, np.uint16)   # the checks test the data pointers against NULL only
    img = capi.RawDepthImage(stand_in.ctypes.data, int(bits), int(image_shape[1]), int(image_shape[0]), 0, int(image_shape[1]))
    white = None
    if white_shape is not None:
        white = C.byref(capi.RawDepthImage(stand_in.ctypes.data, int(bits), int(white_shape[1]), int(white_shape[0]), 0, int(white_shape[1])))
    plan = capi.TotalFocusPlan()
    opt = make_options(**options)
    _check(lib.lifcal_totalfocus_check(C.byref(params), C.byref(img), white, int(depth_shape[1]), int(depth_shape[0]), C.byref(opt), C.byref(plan)),
           "lifcal_totalfocus_check")
    return plan


def totalFocusImage(grid, image, inv_depth, white=None, device_out: bool = False, **options) -> TotalFocusImage:
    """lifcal_totalfocus_render on the grid's device.  image, white (optional): (H, W) uint8 / uint16 of the grid's size, numpy
    arrays (rows may be strided) or torch tensors on that device; inv_depth: (out_height, out_width) float32, the inv_depth of
    depthMapFromRaw at the same scale, likewise.  device_out: the three maps are torch tensors on the device."""
    lib = capi.load_library()
    img, keep_img = _image(image)
    wht, keep_white = _image(white) if white is not None else (None, None)
    if len(inv_depth.shape) != 2:
        raise ValueError("inv_depth: a 2-D float32 map")
    # the size of the depth map is checked against the output's before anything is launched
    plan = capi.TotalFocusPlan()
    opt = make_options(**options)
    _check(lib.lifcal_totalfocus_check(C.byref(grid.params), C.byref(img), C.byref(wht) if wht is not None else None, int(inv_depth.shape[1]),
                                       int(inv_depth.shape[0]), C.byref(opt), C.byref(plan)), "lifcal_totalfocus_check")
    shape = (int(plan.out_height), int(plan.out_width))
    if hasattr(inv_depth, "data_ptr"):   # torch tensor
        import torch
        iv = inv_depth
        if iv.dtype != torch.float32 or not iv.is_cuda or not iv.is_contiguous():
            raise ValueError("inv_depth: a contiguous float32 tensor on the grid's device")
        torch.cuda.synchronize(iv.device)
        ptr_iv, on_device = iv.data_ptr(), 1
    else:
        iv = np.ascontiguousarray(inv_depth, np.float32)
        ptr_iv, on_device = iv.ctypes.data, 0
    bits = int(img.bits)
    res = capi.TotalFocusResult()
    if device_out:
        import torch
        dev = torch.device("cuda", int(getattr(grid, "device", 0)))
        out = torch.empty(shape, dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
        nl = torch.empty(shape, dtype=torch.uint8, device=dev); st = torch.empty(shape, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        ptr = lambda t: t.data_ptr()
    else:
        out = np.zeros(shape, np.uint8 if bits == 8 else np.uint16); nl = np.zeros(shape, np.uint8); st = np.zeros(shape, np.uint8)
        ptr = lambda a: a.ctypes.data
    res.out_on_device = 1 if device_out else 0
    res.image, res.n_lenses, res.status = ptr(out), ptr(nl), ptr(st)
    _check(lib.lifcal_totalfocus_render(grid._h, C.byref(img), C.byref(wht) if wht is not None else None, ptr_iv, on_device, C.byref(opt), C.byref(res)),
           "lifcal_totalfocus_render")
    del iv, keep_img, keep_white
    return TotalFocusImage(out, nl, st, np.array(res.count[:], np.uint64), float(res.seconds), int(plan.options.scale))
