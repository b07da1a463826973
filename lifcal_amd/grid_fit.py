"""The micro-lens grid from a white image, over include/lifcal_grid.h: lens centres on the GPU
(lifcal_grid_detect), the lattice fit on the host (lifcal_grid_fit_centres), and both twice in a row (lifcal_grid_fit).

The result is the parameter set MicroLensGrid / lifcal_mla_create takes in place of the values of the vendor's MLA calibration
file.  The detection runs inside liblifcal_ba.so on the GPU; there is no Python or CPU fallback for it.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _capi as capi
from .bundle_adjustment import LifcalError

DEFAULT_GATE_PX = 0.5


@dataclass
class GridReport:
    """lifcal_grid_report: per-centre labels, residuals against the fitted grid and accept flags, and the summary figures"""
    lens: np.ndarray                  # structured: sub, x, y, accepted, dx, dy (capi.GRID_LENS_DTYPE), one row per centre
    n_centres: int
    n_accepted: int
    n_rejected_label: int
    n_rejected_residual: int
    rms: float
    max_residual: float
    lattice_a: np.ndarray             # unconstrained fit: one column step
    lattice_b: np.ndarray             # ... the step from lens (0, x, y) to lens (1, x, y)
    lattice_c: np.ndarray             # ... one row step of a sub-grid
    lens_diameter: float              # the fitted model in double
    rotation: float
    lens_base_y: np.ndarray
    origin: np.ndarray                # centre of lens (0, 0, 0), pixels


@dataclass
class GridFit:
    params: capi.MlaParams
    report: GridReport
    centres: Optional[np.ndarray] = None   # structured (capi.GRID_CENTRE_DTYPE), when the fit came from an image

    def grid(self, device: int = 0):
        """The MicroLensGrid of the fitted parameters (maps and web built on `device`)."""
        from .mla import MicroLensGrid
        p = self.params
        return MicroLensGrid(p.width, p.height, p.lens_diameter, tuple(p.lens_base_y), p.rotation, tuple(p.offset), bool(p.rotation_on_grid), device)


def _check(rc: int, what: str):
    if rc < 0:
        lib = capi.load_library()
        raise LifcalError(f"{what}: {lib.lifcal_ba_strerror(rc).decode()} ({lib.lifcal_ba_last_error().decode()})")


def _image(white: np.ndarray):
    white = np.asarray(white)
    if white.ndim != 2 or white.dtype not in (np.uint8, np.uint16):
        raise ValueError("white image: a 2-D uint8 or uint16 array (one channel)")
    if white.strides[1] != white.itemsize or white.strides[0] % white.itemsize or white.strides[0] < white.shape[1] * white.itemsize:
        white = np.ascontiguousarray(white)
    img = capi.GridImage(white.ctypes.data, 8 * white.itemsize, white.shape[1], white.shape[0], white.strides[0] // white.itemsize)
    return white, img   # the array must outlive the struct


def _report(r: capi.GridReport, lens: np.ndarray) -> GridReport:
    return GridReport(lens, int(r.n_centres), int(r.n_accepted), int(r.n_rejected_label), int(r.n_rejected_residual), float(r.rms), float(r.max_residual),
                      np.array(r.lattice_a[:]), np.array(r.lattice_b[:]), np.array(r.lattice_c[:]), float(r.lens_diameter), float(r.rotation),
                      np.array(r.lens_base_y[:]), np.array(r.origin[:]))


def detectLensCentres(white: np.ndarray, lens_diameter_guess: float, device: int = 0) -> np.ndarray:
    """lifcal_grid_detect: the lens centres of a white image (rows may be strided), ascending in `peak`; structured array with
    cx, cy, sum_w, sum_wx, sum_wy, peak."""
    lib = capi.load_library()
    white, img = _image(white)
    out = capi.GridCentres(0, 0, None)
    _check(lib.lifcal_grid_detect(C.byref(img), float(lens_diameter_guess), int(device), C.byref(out)), "lifcal_grid_detect")
    n = int(out.n)
    c = np.zeros(n, capi.GRID_CENTRE_DTYPE)
    if n == 0:
        return c
    out = capi.GridCentres(n, 0, c.ctypes.data)
    rc = lib.lifcal_grid_detect(C.byref(img), float(lens_diameter_guess), int(device), C.byref(out))
    _check(rc, "lifcal_grid_detect")
    if rc != 0 or int(out.n) != n:
        raise LifcalError("lifcal_grid_detect: centre count changed between the count and the fill call")
    return c


def fitGridCentres(cx, cy, width: int, height: int, lens_diameter_guess: float, gate_px: float = DEFAULT_GATE_PX) -> GridFit:
    """lifcal_grid_fit_centres: host only, needs no device."""
    lib = capi.load_library()
    cx = np.ascontiguousarray(cx, np.float64); cy = np.ascontiguousarray(cy, np.float64)
    assert cx.shape == cy.shape and cx.ndim == 1
    lens = np.zeros(len(cx), capi.GRID_LENS_DTYPE)
    rep = capi.GridReport()
    rep.capacity, rep.lens = len(cx), (lens.ctypes.data if len(cx) else None)
    prm = capi.MlaParams()
    _check(lib.lifcal_grid_fit_centres(len(cx), capi.as_dptr(cx), capi.as_dptr(cy), int(width), int(height), float(lens_diameter_guess), float(gate_px),
                                       C.byref(prm), C.byref(rep)), "lifcal_grid_fit_centres")
    return GridFit(prm, _report(rep, lens))


def fitGrid(white: np.ndarray, lens_diameter_guess: float, gate_px: float = DEFAULT_GATE_PX, device: int = 0) -> GridFit:
    """lifcal_grid_fit: detect and fit, and both once more with the fitted diameter in place of the guess."""
    lib = capi.load_library()
    white, img = _image(white)
    prm = capi.MlaParams()
    cen = capi.GridCentres(0, 0, None)
    rep = capi.GridReport()
    _check(lib.lifcal_grid_fit(C.byref(img), float(lens_diameter_guess), float(gate_px), int(device), C.byref(prm), C.byref(cen), C.byref(rep)), "lifcal_grid_fit")
    n = int(cen.n)
    c = np.zeros(n, capi.GRID_CENTRE_DTYPE); lens = np.zeros(n, capi.GRID_LENS_DTYPE)
    cen = capi.GridCentres(n, 0, c.ctypes.data if n else None)
    rep = capi.GridReport()
    rep.capacity, rep.lens = n, (lens.ctypes.data if n else None)
    rc = lib.lifcal_grid_fit(C.byref(img), float(lens_diameter_guess), float(gate_px), int(device), C.byref(prm), C.byref(cen), C.byref(rep))
    _check(rc, "lifcal_grid_fit")
    if rc != 0 or int(cen.n) != n:
        raise LifcalError("lifcal_grid_fit: centre count changed between the count and the fill call")
    return GridFit(prm, _report(rep, lens), c)
