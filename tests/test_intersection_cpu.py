"""Host side of the batched point intersection (include/lifcal_intersect.h): the exported symbols, the row layout in ctypes and
numpy, and the argument checks of lifcal_intersect_points, which all answer before the device is touched (this file runs where no
GPU exists)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lifcal_amd import _capi as capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, OUT_OF_RANGE = -1, -4


@pytest.fixture(scope="module")
def lib(built):
    return capi.load_library()


def test_every_declared_symbol_is_exported_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "lifcal_intersect.h")).read()
    declared = set(re.findall(r"\b(lifcal_intersect_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"lifcal_intersect_points"}
    assert declared == set(capi.INTERSECT_PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    # the intersection entry point lives in its own header and table: include/lifcal_ba.h and capi.PROTOTYPES name none
    assert not [n for n in capi.PROTOTYPES if n.startswith("lifcal_intersect_")]
    assert "lifcal_intersect_" not in open(os.path.join(ROOT, "include", "lifcal_ba.h")).read()


def test_point_row_has_the_c_layout():
    # struct lifcal_intersect_point: 4 + 6 + 3 + 2 doubles, then 2 uint32 and 4 int32, no padding
    assert C.sizeof(capi.IntersectPoint) == 8 * 15 + 4 * 6 == 144
    offsets = {"initial_cost": 0, "final_cost": 8, "final_radius": 16, "final_gradient_max_norm": 24, "H": 32, "g": 80, "sum_xx": 104, "sum_yy": 112,
               "n_obs": 120, "n_inliers": 124, "iterations": 128, "successful_steps": 132, "unsuccessful_steps": 136, "termination": 140}
    assert [f[0] for f in capi.IntersectPoint._fields_] == list(offsets)
    dt = capi.INTERSECT_POINT_DTYPE
    assert dt.itemsize == 144 and list(dt.names) == list(offsets)
    for name, at in offsets.items():
        assert getattr(capi.IntersectPoint, name).offset == at, name
        assert dt.fields[name][1] == at, name
        assert dt.fields[name][0].itemsize == getattr(capi.IntersectPoint, name).size, name
    # struct lifcal_intersect_problem: 4 uint32, 9 pointers (cam, views, pts last), 3 doubles, 1 uint32 (+ tail padding)
    assert C.sizeof(capi.IntersectProblem) == 16 + 72 + 24 + 8
    names = [f[0] for f in capi.IntersectProblem._fields_]
    assert names == ["n_obs", "n_frames", "n_points", "reserved", "u", "v", "mcx", "mcy", "pt", "fr", "cam", "views", "pts", "spx", "spy", "scale", "config"]
    P = capi.IntersectProblem
    assert (P.n_obs.offset, P.n_frames.offset, P.n_points.offset, P.reserved.offset) == (0, 4, 8, 12)
    assert [getattr(P, n).offset for n in ("u", "v", "mcx", "mcy", "pt", "fr", "cam", "views", "pts")] == list(range(16, 88, 8))
    assert (P.spx.offset, P.spy.offset, P.scale.offset, P.config.offset) == (88, 96, 104, 112)


class Call:
    """a small, valid problem (two frames, three points, four observations) whose fields a test then spoils"""

    def __init__(self):
        self.u = np.array([10.0, 11.0, 12.0, 13.0]); self.v = self.u + 1.0; self.mcx = self.u + 0.5; self.mcy = self.v + 0.5
        self.pt = np.array([0, 1, 2, 1], np.uint32); self.fr = np.array([0, 0, 1, 1], np.uint32)
        self.cam = np.zeros(17); self.cam[:5] = [35.0, 34.15, 0.4, 511.3, 513.9]
        self.pts = np.arange(9, dtype=np.float64) + 500.0
        self.views = np.zeros(12)
        self.pts_in = self.pts.copy()
        self.rows = np.zeros(3, capi.INTERSECT_POINT_DTYPE)
        self.opt = capi.default_options_py()
        p = capi.IntersectProblem()
        p.n_obs, p.n_frames, p.n_points = 4, 2, 3
        p.u, p.v, p.mcx, p.mcy = (capi.as_dptr(a) for a in (self.u, self.v, self.mcx, self.mcy))
        p.pt, p.fr = capi.as_uptr(self.pt), capi.as_uptr(self.fr)
        p.cam, p.views, p.pts = capi.as_dptr(self.cam), capi.as_dptr(self.views), capi.as_dptr(self.pts)
        p.spx = p.spy = 0.011; p.scale = 2.0; p.config = 0x306
        self.p = p

    def run(self, lib, problem=True, options=True, rows=True):
        return lib.lifcal_intersect_points(C.byref(self.p) if problem else None, C.byref(self.opt) if options else None, 1.0,
                                           self.rows.ctypes.data if rows else None, None)

    def untouched(self):
        return not self.rows.view(np.uint8).any() and self.pts.tobytes() == self.pts_in.tobytes()


def test_null_arguments_are_invalid(lib):
    for kw in ("problem", "options", "rows"):
        c = Call()
        assert c.run(lib, **{kw: False}) == INVALID_ARG, kw
        assert c.untouched(), kw
    assert b"lifcal_intersect_points" in lib.lifcal_ba_last_error()
    for field in ("u", "v", "mcx", "mcy", "pt", "fr", "cam", "views", "pts"):
        c = Call()
        setattr(c.p, field, None)
        assert c.run(lib) == INVALID_ARG, field
        assert c.untouched(), field   # nothing was written
        assert b"lifcal_intersect_points" in lib.lifcal_ba_last_error()


def test_indices_out_of_range(lib):
    c = Call(); c.pt[2] = 3
    assert c.run(lib) == OUT_OF_RANGE
    assert b"observation 2" in lib.lifcal_ba_last_error()
    assert c.untouched()
    c = Call(); c.fr[3] = 2
    assert c.run(lib) == OUT_OF_RANGE
    assert b"observation 3" in lib.lifcal_ba_last_error()
    c = Call(); c.pt[0] = 0xFFFFFFFF
    assert c.run(lib) == OUT_OF_RANGE
    assert b"observation 0" in lib.lifcal_ba_last_error()


def test_unsupported_options_are_invalid(lib):
    c = Call(); c.opt.world_size = 2
    assert c.run(lib) == INVALID_ARG
    c = Call(); c.opt.precision = 1
    assert c.run(lib) == INVALID_ARG
    # deterministic is ignored (the result is always ordered): the call gets past the option checks and is stopped by the next one
    c = Call(); c.opt.deterministic = 1; c.fr[0] = 9
    assert c.run(lib) == OUT_OF_RANGE


def test_no_points_is_an_empty_success(lib):
    c = Call()
    c.p.n_obs = 0; c.p.n_points = 0
    assert c.run(lib) == 0
    assert c.untouched()
    # points, but not one observation: every row is the zero row of a point without observations, and no device is needed for it
    c = Call()
    c.p.n_obs = 0; c.rows["iterations"] = 7
    assert c.run(lib) == 0
    assert not c.rows.view(np.uint8).any() and c.pts.tobytes() == c.pts_in.tobytes()
