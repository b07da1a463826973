"""The host side the one-call routes share (lifcal_amd/csrc/batch_call.hpp): every entry point takes the same
valid problem through its checks, sorts, group building and staging, all of which run in front of the device selection, and is then
refused for its device alone; and every entry point refuses the same spoiled problem with the same words behind its own name.

The device asked for is one no machine has, so the test asks the same with and without a GPU."""
import ctypes as C

import numpy as np
import pytest

from lifcal_amd import _capi as capi

NO_DEVICE, OUT_OF_RANGE = -2, -4
ROUTES = ["lifcal_resect_frames", "lifcal_intersect_points", "lifcal_start_poses", "lifcal_start_points", "lifcal_register_scene"]


@pytest.fixture(scope="module")
def lib(built):
    return capi.load_library()


class Call:
    """a valid problem of two frames, three points and six observations, and the outputs of one route, filled with a pattern"""

    def __init__(self, route):
        self.route = route
        self.u = np.array([10.0, 11.0, 12.0, 13.0, 14.0, 15.0]); self.v = self.u + 1.0; self.mcx = self.u + 0.5; self.mcy = self.v + 0.5
        self.pt = np.array([0, 1, 2, 2, 0, 1], np.uint32); self.fr = np.array([0, 1, 0, 1, 1, 0], np.uint32)
        self.cam = np.zeros(17); self.cam[:5] = [35.0, 34.15, 0.4, 511.3, 513.9]
        self.pts = np.arange(9, dtype=np.float64) + 500.0
        self.views = np.arange(12, dtype=np.float64) * 0.01
        frame_rows = {"lifcal_resect_frames": capi.RESECT_FRAME_DTYPE, "lifcal_start_poses": capi.START_FRAME_DTYPE, "lifcal_register_scene": capi.REGISTER_FRAME_DTYPE}
        point_rows = {"lifcal_intersect_points": capi.INTERSECT_POINT_DTYPE, "lifcal_start_points": capi.START_POINT_DTYPE, "lifcal_register_scene": capi.REGISTER_POINT_DTYPE}
        self.frows = np.zeros(2, frame_rows.get(route, np.uint8)); self.prows = np.zeros(3, point_rows.get(route, np.uint8))
        self.groups = np.zeros(6, capi.START_GROUP_DTYPE)
        for a in (self.frows, self.prows, self.groups):
            a.view(np.uint8)[:] = 0x77   # (a pattern: a call that writes a row changes it)
        self.n_groups = np.full(1, 77, np.uint32)
        self.summary = capi.RegisterSummary(); self.summary.n_groups = 77
        self.seconds = C.c_double(77.0)
        self.opt = capi.default_options_py()
        self.opt.device = 4096
        self.reg = capi.RegisterOptions(gate_px=1.0, inlier_threshold=1.0, min_shared=3, anchor_frame=-1, max_rounds=0)
        p = {"lifcal_resect_frames": capi.ResectProblem, "lifcal_start_poses": capi.ResectProblem, "lifcal_register_scene": capi.RegisterProblem}.get(route, capi.IntersectProblem)()
        p.n_obs, p.n_frames, p.n_points = 6, 2, 3
        p.u, p.v, p.mcx, p.mcy = (capi.as_dptr(a) for a in (self.u, self.v, self.mcx, self.mcy))
        p.pt, p.fr = capi.as_uptr(self.pt), capi.as_uptr(self.fr)
        p.cam, p.views, p.pts = capi.as_dptr(self.cam), capi.as_dptr(self.views), capi.as_dptr(self.pts)
        p.spx = p.spy = 0.011; p.scale = 2.0; p.config = 0x306
        self.p = p
        self.before = self.arrays()

    def arrays(self):
        return [a.tobytes() for a in (self.pts, self.views, self.frows, self.prows, self.groups)] + [bytes(self.summary)]

    def run(self, lib):
        P, O, S = C.byref(self.p), C.byref(self.opt), C.byref(self.seconds)
        if self.route == "lifcal_resect_frames":
            return lib.lifcal_resect_frames(P, O, 1.0, self.frows.ctypes.data, S)
        if self.route == "lifcal_intersect_points":
            return lib.lifcal_intersect_points(P, O, 1.0, self.prows.ctypes.data, S)
        if self.route == "lifcal_start_poses":
            return lib.lifcal_start_poses(P, O, 1.0, 1.0, self.frows.ctypes.data, self.groups.ctypes.data, capi.as_uptr(self.n_groups), S)
        if self.route == "lifcal_start_points":
            return lib.lifcal_start_points(P, O, 1.0, self.prows.ctypes.data, S)
        return lib.lifcal_register_scene(P, O, C.byref(self.reg), self.frows.ctypes.data, self.prows.ctypes.data, C.byref(self.summary), S)


@pytest.mark.parametrize("route", ROUTES)
def test_a_valid_problem_is_refused_for_its_device_alone(lib, route):
    c = Call(route)
    assert c.run(lib) == NO_DEVICE
    msg = lib.lifcal_ba_last_error()
    assert msg.startswith(route.encode() + b": "), msg
    assert c.arrays() == c.before
    assert c.seconds.value == 0.0   # (the time is zeroed behind the checks, in front of everything else)


@pytest.mark.parametrize("route", ROUTES)
def test_an_index_out_of_range_is_refused_in_the_same_words(lib, route):
    c = Call(route)
    c.pt[2] = c.p.n_points
    assert c.run(lib) == OUT_OF_RANGE
    assert lib.lifcal_ba_last_error() == route.encode() + b": observation 2 names point 3 / frame 0 out of range"
    assert c.arrays() == c.before and c.seconds.value == 77.0 and c.n_groups[0] == 77
