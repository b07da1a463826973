"""Host side of the registration chain (include/lifcal_register.h): the exported symbols, the row layouts in
ctypes and numpy, the argument checks, which all answer before the device is touched, and the method itself on the cpu arm of its
restatement (tests/register_reference.py), where no GPU exists: noise-free scenes are reproduced in the anchor's frame, and the
oracle's bundle adjustment started from the chain's result ends at the cost of the one started from ground truth.

Bars: noise-free 1e-6 rad, 1e-5 mm (translations), 1e-4 mm (points); chain: every frame registered, every observed point with a used
group mapped, final costs within 1e-4 relative (the same-valley bar of sections 7m / 7n), start RMS below 10 px per axis.

Measured here: noise-free 3.7e-11 rad, 1.8e-7 mm, 2.5e-6 mm; chains: final costs within 7.6e-7 relative, start RMS 0.10 .. 0.79 px per
axis, 4 .. 15 iterations of the bundle adjustment (5 .. 7 from ground truth)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle
from lifcal_amd import _capi as capi, scene
from tests import register_reference as rr
from tests.helpers import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, OUT_OF_RANGE = -1, -4


@pytest.fixture(scope="module")
def lib(built):
    return capi.load_library()


def test_every_declared_symbol_is_exported_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "lifcal_register.h")).read()
    declared = set(re.findall(r"\b(lifcal_register_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"lifcal_register_default_options", "lifcal_register_scene"}
    assert declared == set(capi.REGISTER_PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    assert not [n for n in list(capi.PROTOTYPES) + list(capi.START_PROTOTYPES) if n.startswith("lifcal_register_")]


def check_layout(struct, dtype, size, offsets):
    assert C.sizeof(struct) == size == dtype.itemsize
    assert [f[0] for f in struct._fields_] == list(offsets) == list(dtype.names)
    for name, at in offsets.items():
        assert getattr(struct, name).offset == at, name
        assert dtype.fields[name][1] == at, name
        assert dtype.fields[name][0].itemsize == getattr(struct, name).size, name


def test_rows_have_the_c_layout():
    check_layout(capi.RegisterFrame, capi.REGISTER_FRAME_DTYPE, 64,
                 {"sum_xx": 0, "sum_yy": 8, "final_cost": 16, "n_obs": 24, "n_obs_used": 28, "n_inliers": 32, "n_groups": 36, "n_used": 40, "n_shared": 44,
                  "status": 48, "round": 52, "iterations": 56, "termination": 60})
    check_layout(capi.RegisterPoint, capi.REGISTER_POINT_DTYPE, 56,
                 {"sum_xx": 0, "sum_yy": 8, "final_cost": 16, "n_obs": 24, "n_obs_used": 28, "n_inliers": 32, "n_frames_used": 36,
                  "status": 40, "round": 44, "iterations": 48, "termination": 52})
    assert C.sizeof(capi.RegisterSummary) == 24 and [f[0] for f in capi.RegisterSummary._fields_] == ["anchor_frame", "n_rounds", "n_frames_registered", "n_points_mapped", "n_groups", "n_groups_used"]
    assert C.sizeof(capi.RegisterOptions) == 40 and capi.RegisterOptions.anchor_view.offset == 24 and capi.RegisterOptions.max_rounds.offset == 32
    assert C.sizeof(capi.RegisterProblem) == C.sizeof(capi.IntersectProblem)
    assert [(f[0], getattr(capi.RegisterProblem, f[0]).offset) for f in capi.RegisterProblem._fields_] == [(f[0], getattr(capi.IntersectProblem, f[0]).offset) for f in capi.IntersectProblem._fields_]


def test_default_options(lib):
    r = capi.RegisterOptions(); r.gate_px = 9.0; r.min_shared = 99; r.anchor_frame = 5; r.max_rounds = 7
    lib.lifcal_register_default_options(C.byref(r))
    assert (r.gate_px, r.inlier_threshold, r.min_shared, r.anchor_frame, r.max_rounds) == (1.0, 1.0, 6, -1, 0) and not r.anchor_view
    lib.lifcal_register_default_options(None)   # (a null pointer is ignored)


class Call:
    """a small, valid problem (two frames, three points, four observations) whose fields a test then spoils"""

    def __init__(self):
        self.u = np.array([10.0, 11.0, 12.0, 13.0]); self.v = self.u + 1.0; self.mcx = self.u + 0.5; self.mcy = self.v + 0.5
        self.pt = np.array([0, 1, 2, 1], np.uint32); self.fr = np.array([0, 0, 1, 1], np.uint32)
        self.cam = np.zeros(17); self.cam[:5] = [35.0, 34.15, 0.4, 511.3, 513.9]
        self.pts = np.arange(9, dtype=np.float64) + 500.0
        self.views = np.arange(12, dtype=np.float64) * 0.01
        self.frows, self.prows = np.zeros(2, capi.REGISTER_FRAME_DTYPE), np.zeros(3, capi.REGISTER_POINT_DTYPE)
        self.frows["n_shared"] = 77; self.prows["n_frames_used"] = 77   # (a pattern: an answered call rewrites it, a refused one does not)
        self.summary = capi.RegisterSummary(); self.summary.n_groups = 77
        self.seconds = C.c_double(77.0)
        self.before = self.state()
        self.opt = capi.default_options_py()
        self.reg = capi.RegisterOptions(gate_px=1.0, inlier_threshold=1.0, min_shared=6, anchor_frame=-1, max_rounds=0)
        p = capi.RegisterProblem()
        p.n_obs, p.n_frames, p.n_points = 4, 2, 3
        p.u, p.v, p.mcx, p.mcy = (capi.as_dptr(a) for a in (self.u, self.v, self.mcx, self.mcy))
        p.pt, p.fr = capi.as_uptr(self.pt), capi.as_uptr(self.fr)
        p.cam, p.views, p.pts = capi.as_dptr(self.cam), capi.as_dptr(self.views), capi.as_dptr(self.pts)
        p.spx = p.spy = 0.011; p.scale = 2.0; p.config = 0x306
        self.p = p

    def state(self):
        return [a.tobytes() for a in (self.pts, self.views, self.frows, self.prows)] + [bytes(self.summary), self.seconds.value]

    def run(self, lib, problem=True, options=True, reg=True, frows=True, prows=True, summary=True):
        return lib.lifcal_register_scene(C.byref(self.p) if problem else None, C.byref(self.opt) if options else None, C.byref(self.reg) if reg else None,
                                         self.frows.ctypes.data if frows else None, self.prows.ctypes.data if prows else None,
                                         C.byref(self.summary) if summary else None, C.byref(self.seconds))

    def untouched(self):
        return self.before == self.state()


def test_null_arguments_are_invalid(lib):
    for kw in ("problem", "options", "reg", "frows", "prows", "summary"):
        c = Call()
        assert c.run(lib, **{kw: False}) == INVALID_ARG, kw
        assert c.untouched(), kw
        assert b"lifcal_register_scene" in lib.lifcal_ba_last_error()
    for field in ("u", "v", "mcx", "mcy", "pt", "fr", "cam", "views", "pts"):
        c = Call()
        setattr(c.p, field, None)
        assert c.run(lib) == INVALID_ARG, field
        assert c.untouched(), field


def test_indices_out_of_range(lib):
    c = Call(); c.pt[2] = 3
    assert c.run(lib) == OUT_OF_RANGE and b"observation 2" in lib.lifcal_ba_last_error() and c.untouched()
    c = Call(); c.fr[3] = 2
    assert c.run(lib) == OUT_OF_RANGE and b"observation 3" in lib.lifcal_ba_last_error() and c.untouched()
    c = Call(); c.pt[0] = 0xFFFFFFFF
    assert c.run(lib) == OUT_OF_RANGE and b"observation 0" in lib.lifcal_ba_last_error() and c.untouched()


def test_unsupported_options_are_invalid(lib):
    c = Call(); c.opt.world_size = 2
    assert c.run(lib) == INVALID_ARG and c.untouched()
    c = Call(); c.opt.precision = 1
    assert c.run(lib) == INVALID_ARG and c.untouched()
    c = Call(); c.p.config = 0x303
    assert c.run(lib) == INVALID_ARG and c.untouched()
    # deterministic is ignored (the result is always ordered): the call gets past the option checks and is stopped by the next one
    c = Call(); c.opt.deterministic = 1; c.fr[0] = 9
    assert c.run(lib) == OUT_OF_RANGE and c.untouched()


def test_register_options_are_checked(lib):
    for gate in (0.0, -1.0, float("nan"), float("-inf")):
        c = Call(); c.reg.gate_px = gate
        assert c.run(lib) == INVALID_ARG and c.untouched(), gate
        assert b"gate_px" in lib.lifcal_ba_last_error()
    for ms in (0, 2):
        c = Call(); c.reg.min_shared = ms
        assert c.run(lib) == INVALID_ARG and c.untouched() and b"min_shared" in lib.lifcal_ba_last_error()
    for af in (2, 1000):
        c = Call(); c.reg.anchor_frame = af
        assert c.run(lib) == INVALID_ARG and c.untouched() and b"anchor_frame" in lib.lifcal_ba_last_error()
    # the same checks hold for a call without observations, which no device is needed for: +inf is a valid gate, 0 is not
    c = Call(); c.p.n_obs = 0; c.reg.gate_px = float("inf")
    assert c.run(lib) == 0
    c = Call(); c.p.n_obs = 0; c.reg.gate_px = 0.0
    assert c.run(lib) == INVALID_ARG and c.untouched()


def test_no_observations_is_answered_on_the_host(lib):
    c = Call()
    c.p.n_obs = 0; c.p.n_frames = 0; c.p.n_points = 0
    assert c.run(lib) == 0
    assert c.state()[:4] == c.before[:4] and c.seconds.value == 0.0
    assert (c.summary.anchor_frame, c.summary.n_rounds, c.summary.n_frames_registered, c.summary.n_points_mapped, c.summary.n_groups) == (-1, 0, 0, 0, 0)
    # frames and points, but not one observation: status 1 and round -1 in every row, everything else zero, poses and points keep their bits
    c = Call()
    c.p.n_obs = 0
    assert c.run(lib) == 0
    assert np.all(c.frows["status"] == 1) and np.all(c.prows["status"] == 1) and np.all(c.frows["round"] == -1) and np.all(c.prows["round"] == -1)
    for rows in (c.frows, c.prows):
        zero = rows.copy(); zero["status"] = 0; zero["round"] = 0
        assert not zero.view(np.uint8).any()
    assert c.pts.tobytes() == c.before[0] and c.views.tobytes() == c.before[1] and c.seconds.value == 0.0
    assert (c.summary.anchor_frame, c.summary.n_rounds, c.summary.n_frames_registered, c.summary.n_points_mapped, c.summary.n_groups) == (-1, 0, 0, 0, 0)


# ---- the method, on the cpu arm of the restatement -----------------------------------------------------------------------------

def chain(sc, n_frames=None, n_points=None, obs=None, **kw):
    u, v, mcx, mcy, pt, fr = obs if obs is not None else (sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)
    return rr.register("cpu", sc.cam_gt, u, v, mcx, mcy, pt, fr, sc.spec.n_frames if n_frames is None else n_frames,
                       sc.spec.n_points if n_points is None else n_points, sc.config, sc.spx, sc.scale, **kw)


NOISE_FREE = [(S(6, 40, None, 0x906, 11, noise_px=0.0), 6), (S(24, 120, 6, 0xF06, 119, noise_px=0.0), 6), (S(12, 120, 3, 0xB06, 5, noise_px=0.0), 3)]


@pytest.mark.parametrize("spec,min_shared", NOISE_FREE, ids=["all_frames", "window6", "window3"])
def test_a_noise_free_scene_is_reproduced_in_the_anchors_frame(built, spec, min_shared):
    sc = scene.make_scene(spec)
    a = chain(sc, min_shared=min_shared).anchor_frame
    vg, pg = sc.views_gt.reshape(-1, 6), sc.pts_gt.reshape(-1, 3)
    r = chain(sc, min_shared=min_shared, anchor_frame=a, anchor_view=vg[a])
    assert r.anchor_frame == a and np.all(r.f_status == 0) and np.all(r.p_status == 0)
    da, dt, dp = np.abs(r.views[:, :3] - vg[:, :3]).max(), np.abs(r.views[:, 3:] - vg[:, 3:]).max(), np.abs(r.pts - pg).max()
    print(f"anchor {a}, {r.n_rounds} rounds: {da:.1e} rad, {dt:.1e} mm, points {dp:.1e} mm from ground truth")
    assert da <= 1e-6 and dt <= 1e-5 and dp <= 1e-4


CHAINS = {   # the four FAMILIES and three of the POINT_FAMILIES of tests/test_gpu_start.py, its p_window, the windowed scene of tests/helpers.py
    "r2_tan_robust": (S(6, 40, None, 0x306, 115, outlier_fraction=0.05), 6),
    "r0": (S(6, 40, None, 0x100, 7), 6),
    "r1_tan_adj_robust": (S(6, 40, None, 0xB05, 9, outlier_fraction=0.05), 6),
    "r2_tan_adj": (S(6, 40, None, 0x906, 11), 6),
    "p_r2_tan_adj_robust": (S(6, 40, None, 0xF06, 115, outlier_fraction=0.05), 6),
    "p_r0": (S(6, 40, None, 0x500, 7), 6),
    "p_r1_tan_adj": (S(6, 40, None, 0xD05, 9), 6),
    "p_window": (S(12, 120, 3, 0xB06, 5, outlier_fraction=0.05), 3),
    "windowed": (S(24, 120, 6, 0xF06, 119, outlier_fraction=0.02), 6),
}


def bundle_adjustment(sc, obs, views, pts):
    """the oracle's solve with the camera constant, poses and points free; returns the summary and the start RMS per axis"""
    pa = capi.ProblemArrays(*obs, sc.cam_gt, views, pts, sc.spx, sc.scale, sc.config | 0x500, fixed_mask=0x1FFFF)
    st = oracle.reproj_stats(pa, 1.0)
    return oracle.solve(pa), st


@pytest.mark.parametrize("key", list(CHAINS))
def test_bundle_adjustment_from_the_chain_ends_in_the_ground_truth_valley(built, key):
    spec, min_shared = CHAINS[key]
    sc = scene.make_scene(spec)
    r = chain(sc, min_shared=min_shared)
    assert np.all(r.f_status == 0) and r.n_rounds >= 1
    has_used = np.bincount(r.groups["pt"][r.groups["status"] == 0], minlength=spec.n_points) > 0
    assert np.array_equal(r.mapped, has_used) and np.all(r.p_status[~has_used & (r.p_n_obs > 0)] == 2)
    obs, v0, p0, m = rr.registered_part(r.views, r.pts, r.registered, r.mapped, sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)
    _, vg, pg, _ = rr.registered_part(sc.views_gt, sc.pts_gt, r.registered, r.mapped, sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)
    s1, st = bundle_adjustment(sc, obs, v0, p0)
    s2, _ = bundle_adjustment(sc, obs, vg, pg)
    dc = abs(s1.final_cost - s2.final_cost) / s2.final_cost
    print(f"{key}: anchor {r.anchor_frame}, {r.n_rounds} rounds, {int(r.mapped.sum())} of {spec.n_points} points, {int(m.sum())} of {sc.n_obs} observations; "
          f"start rms {st.std_x:.2f} {st.std_y:.2f} px; iterations {s1.iterations} (ground truth {s2.iterations}); final costs {dc:.1e} relative")
    assert dc <= 1e-4
    assert st.std_x < 10.0 and st.std_y < 10.0


@functools.lru_cache(maxsize=None)
def islands():
    """two scenes side by side: frames 0 .. 5 and points 0 .. 39 of the first, frames 6 .. 11 and points 40 .. 79 of the second"""
    a, b = scene.make_scene(S(6, 40, None, 0x306, 115, outlier_fraction=0.05)), scene.make_scene(S(6, 40, None, 0x306, 31, outlier_fraction=0.05))
    cat = lambda n: np.concatenate([getattr(a, n), getattr(b, n)])
    return a, (cat("u"), cat("v"), cat("mcx"), cat("mcy"), np.concatenate([a.pt, b.pt + 40]), np.concatenate([a.fr, b.fr + 6]))


def test_two_islands_register_the_anchors_island_only(built):
    a, obs = islands()
    r = chain(a, 12, 80, obs, anchor_frame=2)
    assert list(r.f_status) == [0] * 6 + [2] * 6 and sorted(r.f_round[:6]) == [0, 1, 1, 1, 1, 1] and np.all(r.f_round[6:] == -1)
    assert np.all(r.p_status[:40] == 0) and np.all(r.p_status[40:] == 2) and np.all(np.isin(r.p_round[:40], (0, 1))) and np.all(r.p_round[40:] == -1)
    assert np.all(np.isnan(r.views[6:])) and np.all(np.isnan(r.pts[40:])) and np.all(np.isfinite(r.views[:6])) and np.all(np.isfinite(r.pts[:40]))
    assert r.n_rounds == 1 and np.all(r.f_n_shared[6:] == 0) and np.all(r.f_n_obs_used[6:] == 0) and np.all(r.p_n_frames_used[:40] == 6)
    # without a chosen anchor the frame with the most used groups is taken, and its island registered
    r = chain(a, 12, 80, obs)
    assert r.anchor_frame == int(np.argmax(r.f_n_used)) and int(r.registered.sum()) == 6 and int(r.mapped.sum()) == 40


def test_a_frame_without_observations_and_max_rounds(built):
    spec = S(12, 120, 3, 0xB06, 5, outlier_fraction=0.05)
    sc = scene.make_scene(spec)
    keep = sc.fr != 7
    obs = tuple(getattr(sc, n)[keep] for n in ("u", "v", "mcx", "mcy", "pt", "fr"))
    r = chain(sc, obs=obs, min_shared=3, anchor_frame=2)
    assert r.f_status[7] == 1 and r.f_round[7] == -1 and np.all(np.isnan(r.views[7])) and r.f_n_obs[7] == 0
    assert np.all(np.delete(r.f_status, 7) == 0)   # (the window of 3 frames bridges the missing one)
    full = chain(sc, min_shared=3, anchor_frame=2)
    one = chain(sc, min_shared=3, anchor_frame=2, max_rounds=1)
    assert full.n_rounds > 1 and one.n_rounds == 1 and np.array_equal(one.f_round >= 0, (full.f_round >= 0) & (full.f_round <= 1))
    assert np.array_equal(one.f_round[one.registered], full.f_round[one.registered]) and np.all(one.f_status[~one.registered] == 2)
    assert np.array_equal(one.mapped, (full.p_round >= 0) & (full.p_round <= 1))
