"""Host side of the batched pose resection (include/lifcal_resect.h): the exported symbols, the row layout in ctypes and numpy, and
the argument checks of lifcal_resect_frames, which all answer before the device is touched (this file runs where no GPU exists)."""
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
    hdr = open(os.path.join(ROOT, "include", "lifcal_resect.h")).read()
    declared = set(re.findall(r"\b(lifcal_resect_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"lifcal_resect_frames"}
    assert declared == set(capi.RESECT_PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    # the resection entry points live in their own header and table: include/lifcal_ba.h and capi.PROTOTYPES name none
    assert not [n for n in capi.PROTOTYPES if n.startswith("lifcal_resect_")]
    assert "lifcal_resect_" not in open(os.path.join(ROOT, "include", "lifcal_ba.h")).read()


def test_frame_row_has_the_c_layout():
    # struct lifcal_resect_frame: 4 + 21 + 6 + 2 doubles, then 2 uint32 and 4 int32, no padding
    assert C.sizeof(capi.ResectFrame) == 8 * 33 + 4 * 6 == 288
    offsets = {"initial_cost": 0, "final_cost": 8, "final_radius": 16, "final_gradient_max_norm": 24, "H": 32, "g": 200, "sum_xx": 248, "sum_yy": 256,
               "n_obs": 264, "n_inliers": 268, "iterations": 272, "successful_steps": 276, "unsuccessful_steps": 280, "termination": 284}
    assert [f[0] for f in capi.ResectFrame._fields_] == list(offsets)
    dt = capi.RESECT_FRAME_DTYPE
    assert dt.itemsize == 288 and list(dt.names) == list(offsets)
    for name, at in offsets.items():
        assert getattr(capi.ResectFrame, name).offset == at, name
        assert dt.fields[name][1] == at, name
        assert dt.fields[name][0].itemsize == getattr(capi.ResectFrame, name).size, name
    # struct lifcal_resect_problem: 4 uint32, 9 pointers, 3 doubles, 1 uint32 (+ tail padding)
    assert C.sizeof(capi.ResectProblem) == 16 + 72 + 24 + 8
    assert capi.ResectProblem.u.offset == 16 and capi.ResectProblem.views.offset == 80 and capi.ResectProblem.spx.offset == 88 and capi.ResectProblem.config.offset == 112


class Call:
    """a small, valid problem (two frames, three points, four observations) whose fields a test then spoils"""

    def __init__(self):
        self.u = np.array([10.0, 11.0, 12.0, 13.0]); self.v = self.u + 1.0; self.mcx = self.u + 0.5; self.mcy = self.v + 0.5
        self.pt = np.array([0, 1, 2, 1], np.uint32); self.fr = np.array([0, 0, 1, 1], np.uint32)
        self.cam = np.zeros(17); self.cam[:5] = [35.0, 34.15, 0.4, 511.3, 513.9]
        self.pts = np.arange(9, dtype=np.float64) + 500.0
        self.views = np.zeros(12)
        self.rows = np.zeros(2, capi.RESECT_FRAME_DTYPE)
        self.opt = capi.default_options_py()
        p = capi.ResectProblem()
        p.n_obs, p.n_frames, p.n_points = 4, 2, 3
        p.u, p.v, p.mcx, p.mcy = (capi.as_dptr(a) for a in (self.u, self.v, self.mcx, self.mcy))
        p.pt, p.fr = capi.as_uptr(self.pt), capi.as_uptr(self.fr)
        p.cam, p.pts, p.views = capi.as_dptr(self.cam), capi.as_dptr(self.pts), capi.as_dptr(self.views)
        p.spx = p.spy = 0.011; p.scale = 2.0; p.config = 0x306
        self.p = p

    def run(self, lib, problem=True, options=True, rows=True):
        return lib.lifcal_resect_frames(C.byref(self.p) if problem else None, C.byref(self.opt) if options else None, 1.0,
                                        self.rows.ctypes.data if rows else None, None)


def test_null_arguments_are_invalid(lib):
    assert Call().run(lib, problem=False) == INVALID_ARG
    assert Call().run(lib, options=False) == INVALID_ARG
    assert Call().run(lib, rows=False) == INVALID_ARG
    assert b"lifcal_resect_frames" in lib.lifcal_ba_last_error()
    for field in ("u", "v", "mcx", "mcy", "pt", "fr", "cam", "pts", "views"):
        c = Call()
        setattr(c.p, field, None)
        assert c.run(lib) == INVALID_ARG, field
        assert not c.rows.view(np.uint8).any() and not c.views.any(), field   # nothing was written


def test_indices_out_of_range(lib):
    c = Call(); c.pt[2] = 3
    assert c.run(lib) == OUT_OF_RANGE
    assert b"observation 2" in lib.lifcal_ba_last_error()
    c = Call(); c.fr[3] = 2
    assert c.run(lib) == OUT_OF_RANGE
    assert b"observation 3" in lib.lifcal_ba_last_error()
    c = Call(); c.fr[0] = 0xFFFFFFFF
    assert c.run(lib) == OUT_OF_RANGE


def test_unsupported_options_are_invalid(lib):
    c = Call(); c.opt.world_size = 2
    assert c.run(lib) == INVALID_ARG
    c = Call(); c.opt.precision = 1
    assert c.run(lib) == INVALID_ARG
    # deterministic is ignored (the result is always ordered): the call gets past the option checks and is stopped by the next one
    c = Call(); c.opt.deterministic = 1; c.pt[0] = 9
    assert c.run(lib) == OUT_OF_RANGE


def test_no_frames_is_an_empty_success(lib):
    c = Call()
    c.p.n_obs = 0; c.p.n_frames = 0
    assert c.run(lib) == 0
