"""Host side of the closed-form start values (include/lifcal_start.h): the exported symbols, the three row
layouts in ctypes and numpy, the argument checks of both entry points, which all answer before the device is touched, and the numpy
restatement itself (tests/start_reference.py), checked where no GPU exists: noise-free scenes are reproduced, its two alignment arms
agree, and the oracle's one-frame / one-point solves started from its output end in the valley they reach from ground truth.

Measured here: noise-free reprojection RMS 1.1e-9 px (0x506) and 1.8e-9 px (0xF06) at the poses, 8.7e-13 and 1.2e-12 px at the
points; arms 1.0e-15 .. 3.2e-15 rad and 2.0e-12 .. 3.6e-12 mm apart; chains: final costs within 9.1e-7 (poses) and 9.7e-7 (points)
relative, 1/2 d^T H d <= 9.3e-7 (poses) and 2.1e-6 (points) of the cost."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle
from lifcal_amd import _capi as capi, scene
from tests import start_reference as sr
from tests.helpers import S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, OUT_OF_RANGE = -1, -4


@pytest.fixture(scope="module")
def lib(built):
    return capi.load_library()


def test_every_declared_symbol_is_exported_and_listed(lib):
    hdr = open(os.path.join(ROOT, "include", "lifcal_start.h")).read()
    declared = set(re.findall(r"\b(lifcal_start_[a-z_0-9]+)\s*\(", hdr))
    assert declared == {"lifcal_start_poses", "lifcal_start_points"}
    assert declared == set(capi.START_PROTOTYPES)
    for name in declared:
        assert hasattr(lib, name), name
    # the entry points live in their own header and table: include/lifcal_ba.h, the sibling headers and capi.PROTOTYPES name none
    assert not [n for n in capi.PROTOTYPES if n.startswith("lifcal_start_")]
    for other in ("lifcal_ba.h", "lifcal_resect.h", "lifcal_intersect.h"):
        assert "lifcal_start_" not in open(os.path.join(ROOT, "include", other)).read(), other


def check_layout(struct, dtype, size, offsets):
    assert C.sizeof(struct) == size == dtype.itemsize
    assert [f[0] for f in struct._fields_] == list(offsets) == list(dtype.names)
    for name, at in offsets.items():
        assert getattr(struct, name).offset == at, name
        assert dtype.fields[name][1] == at, name
        assert dtype.fields[name][0].itemsize == getattr(struct, name).size, name


def test_rows_have_the_c_layout():
    check_layout(capi.StartFrame, capi.START_FRAME_DTYPE, 72,
                 {"sum_w": 0, "align_rms": 8, "eig": 16, "sum_xx": 32, "sum_yy": 40, "n_obs": 48, "n_inliers": 52, "n_groups": 56, "n_used": 60, "status": 64, "reserved": 68})
    check_layout(capi.StartGroup, capi.START_GROUP_DTYPE, 48, {"xyz": 0, "rms_px": 24, "fr": 32, "pt": 36, "n_obs": 40, "status": 44})
    check_layout(capi.StartPoint, capi.START_POINT_DTYPE, 40, {"sum_xx": 0, "sum_yy": 8, "min_pivot": 16, "n_obs": 24, "n_inliers": 28, "status": 32, "reserved": 36})


class Call:
    """a small, valid problem (two frames, three points, four observations) whose fields a test then spoils; kind: poses | points"""

    def __init__(self, kind):
        self.kind = kind
        self.u = np.array([10.0, 11.0, 12.0, 13.0]); self.v = self.u + 1.0; self.mcx = self.u + 0.5; self.mcy = self.v + 0.5
        self.pt = np.array([0, 1, 2, 1], np.uint32); self.fr = np.array([0, 0, 1, 1], np.uint32)
        self.cam = np.zeros(17); self.cam[:5] = [35.0, 34.15, 0.4, 511.3, 513.9]
        self.pts = np.arange(9, dtype=np.float64) + 500.0
        self.views = np.arange(12, dtype=np.float64) * 0.01
        self.rows = np.zeros(2, capi.START_FRAME_DTYPE) if kind == "poses" else np.zeros(3, capi.START_POINT_DTYPE)
        self.rows["reserved"] = 77   # (a pattern: an answered call rewrites it, a refused one does not)
        self.groups = np.zeros(4, capi.START_GROUP_DTYPE); self.groups["n_obs"] = 77
        self.n_groups = np.full(1, 77, np.uint32)
        self.seconds = C.c_double(77.0)
        self.before = [a.tobytes() for a in (self.pts, self.views, self.rows, self.groups, self.n_groups)]
        self.opt = capi.default_options_py()
        p = capi.ResectProblem() if kind == "poses" else capi.IntersectProblem()
        p.n_obs, p.n_frames, p.n_points = 4, 2, 3
        p.u, p.v, p.mcx, p.mcy = (capi.as_dptr(a) for a in (self.u, self.v, self.mcx, self.mcy))
        p.pt, p.fr = capi.as_uptr(self.pt), capi.as_uptr(self.fr)
        p.cam, p.views, p.pts = capi.as_dptr(self.cam), capi.as_dptr(self.views), capi.as_dptr(self.pts)
        p.spx = p.spy = 0.011; p.scale = 2.0; p.config = 0x306
        self.p = p

    def run(self, lib, problem=True, options=True, rows=True, gate=1.0):
        P, O, R = C.byref(self.p) if problem else None, C.byref(self.opt) if options else None, self.rows.ctypes.data if rows else None
        if self.kind == "poses":
            return lib.lifcal_start_poses(P, O, gate, 1.0, R, self.groups.ctypes.data, capi.as_uptr(self.n_groups), C.byref(self.seconds))
        return lib.lifcal_start_points(P, O, 1.0, R, C.byref(self.seconds))

    def untouched(self):
        return self.before == [a.tobytes() for a in (self.pts, self.views, self.rows, self.groups, self.n_groups)] and self.seconds.value == 77.0


KINDS = ["poses", "points"]


@pytest.mark.parametrize("kind", KINDS)
def test_null_arguments_are_invalid(lib, kind):
    for kw in ("problem", "options", "rows"):
        c = Call(kind)
        assert c.run(lib, **{kw: False}) == INVALID_ARG, kw
        assert c.untouched(), kw
    assert b"lifcal_start_" + kind.encode() in lib.lifcal_ba_last_error()
    for field in ("u", "v", "mcx", "mcy", "pt", "fr", "cam", "views", "pts"):
        c = Call(kind)
        setattr(c.p, field, None)
        assert c.run(lib) == INVALID_ARG, field
        assert c.untouched(), field
        assert b"lifcal_start_" + kind.encode() in lib.lifcal_ba_last_error()


@pytest.mark.parametrize("kind", KINDS)
def test_indices_out_of_range(lib, kind):
    c = Call(kind); c.pt[2] = 3
    assert c.run(lib) == OUT_OF_RANGE
    assert b"observation 2" in lib.lifcal_ba_last_error()
    assert c.untouched()
    c = Call(kind); c.fr[3] = 2
    assert c.run(lib) == OUT_OF_RANGE
    assert b"observation 3" in lib.lifcal_ba_last_error() and c.untouched()
    c = Call(kind); c.pt[0] = 0xFFFFFFFF
    assert c.run(lib) == OUT_OF_RANGE
    assert b"observation 0" in lib.lifcal_ba_last_error() and c.untouched()


@pytest.mark.parametrize("kind", KINDS)
def test_unsupported_options_are_invalid(lib, kind):
    c = Call(kind); c.opt.world_size = 2
    assert c.run(lib) == INVALID_ARG and c.untouched()
    c = Call(kind); c.opt.precision = 1
    assert c.run(lib) == INVALID_ARG and c.untouched()
    # deterministic is ignored (the result is always ordered): the call gets past the option checks and is stopped by the next one
    c = Call(kind); c.opt.deterministic = 1; c.fr[0] = 9
    assert c.run(lib) == OUT_OF_RANGE and c.untouched()


def test_gate_must_be_positive(lib):
    for gate in (0.0, -1.0, float("nan"), float("-inf")):
        c = Call("poses")
        assert c.run(lib, gate=gate) == INVALID_ARG, gate
        assert c.untouched(), gate
        assert b"gate_px" in lib.lifcal_ba_last_error()
    # +inf is a valid gate (none): a call without observations, which no device is needed for, succeeds with it and fails with 0
    c = Call("poses"); c.p.n_obs = 0
    assert c.run(lib, gate=float("inf")) == 0 and np.all(c.rows["status"] == 1)
    c = Call("poses"); c.p.n_obs = 0
    assert c.run(lib, gate=0.0) == INVALID_ARG and c.untouched()


@pytest.mark.parametrize("kind", KINDS)
def test_no_observations_is_answered_on_the_host(lib, kind):
    # nothing to compute: success, nothing written but the (zero) time
    c = Call(kind)
    c.p.n_obs = 0; c.p.n_frames = 0; c.p.n_points = 0
    assert c.run(lib) == 0
    assert c.rows.tobytes() == c.before[2] and c.pts.tobytes() == c.before[0] and c.views.tobytes() == c.before[1]
    # frames and points, but not one observation: every row is zero apart from its status 1, poses and points keep their bits, and
    # no device is needed for it
    c = Call(kind)
    c.p.n_obs = 0
    assert c.run(lib) == 0
    assert np.all(c.rows["status"] == 1)
    zero = c.rows.copy(); zero["status"] = 0
    assert not zero.view(np.uint8).any()
    assert c.pts.tobytes() == c.before[0] and c.views.tobytes() == c.before[1] and c.seconds.value == 0.0
    if kind == "poses":
        assert c.n_groups[0] == 0 and c.groups.tobytes() == c.before[3]


# ---- the restatement ----------------------------------------------------------------------------------------------------------

def rms_at(sc, views, pts):
    """reprojection RMS (pixels, both axes together) of the scene's observations at the given poses and points"""
    views, pts = np.asarray(views).reshape(-1, 6), np.asarray(pts).reshape(-1, 3)
    pc = np.einsum("nij,nj->ni", scene.euler_xyz(views[:, :3])[sc.fr], pts[sc.pt]) + views[sc.fr, 3:]
    e = scene.project(pc, np.stack([sc.mcx, sc.mcy], -1), sc.cam_gt, sc.config, sc.spx, sc.scale) - np.stack([sc.u, sc.v], -1)
    return float(np.sqrt(np.mean(np.sum(e * e, -1))))


def ref_poses(sc, arm="horn"):
    return sr.start_poses(sc.cam_gt, sc.pts_gt, sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.spec.n_frames, sc.config, sc.spx, sc.scale, arm=arm)


def ref_points(sc):
    return sr.start_points(sc.cam_gt, sc.views_gt, sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.spec.n_points, sc.config, sc.spx, sc.scale)


@pytest.mark.parametrize("config", [0x506, 0xF06])
def test_restatement_reproduces_a_noise_free_scene(config):
    sc = scene.make_scene(S(6, 40, None, config, 3, noise_px=0.0))
    a, p = ref_poses(sc), ref_points(sc)
    assert np.all(a.status == 0) and np.all(p.status == 0) and np.all(a.n_used == a.n_groups)
    r_pose, r_pts = rms_at(sc, a.views, sc.pts_gt), rms_at(sc, sc.views_gt, p.pts)
    d = np.abs(a.views - sc.views_gt.reshape(-1, 6))
    print(f"{config:#x}: rms at the poses {r_pose:.2e} px, at the points {r_pts:.2e} px; poses {d[:, :3].max():.1e} rad {d[:, 3:].max():.1e} mm, "
          f"points {np.abs(p.pts - sc.pts_gt.reshape(-1, 3)).max():.1e} mm from ground truth")
    assert r_pose <= 1e-7 and r_pts <= 1e-7


POSE_FAMILIES = {"r2_tan_robust": S(6, 40, None, 0x306, 115, outlier_fraction=0.05), "r1_tan_adj_robust": S(6, 40, None, 0xB05, 9, outlier_fraction=0.05)}


@functools.lru_cache(maxsize=None)
def family(key):
    return scene.make_scene(POSE_FAMILIES[key])


@pytest.mark.parametrize("key", list(POSE_FAMILIES))
def test_alignment_arms_agree(key):
    sc = family(key)
    a, b = ref_poses(sc, "horn"), ref_poses(sc, "kabsch")
    assert np.all(a.status == 0) and np.all(b.status == 0)
    da, dt = np.abs(a.views[:, :3] - b.views[:, :3]).max(), np.abs(a.views[:, 3:] - b.views[:, 3:]).max()
    print(f"{key}: SVD-Kabsch against Horn-eigh {da:.1e} rad, {dt:.1e} mm; relative eigenvalue gaps {[round(float((i.eig[0] - i.eig[1]) / i.eig[0]), 3) for i in a.info]}")
    assert da <= 1e-12
    assert dt <= 1e-8   # (|P| of 1e4 mm times the angle bar)


def flat_hessian_options():
    o = capi.default_options_py(); o.jacobi_scaling = 0; o.min_lm_diagonal = 1e-300
    return o


@pytest.mark.parametrize("key", list(POSE_FAMILIES))
def test_oracle_resection_from_the_restatement_ends_in_the_ground_truth_valley(built, key):
    """the same-valley bars of DESIGN.md section 7m: final costs within 1e-4 relative, 1/2 d^T H d <= 4e-4 of the cost"""
    sc = family(key)
    a = ref_poses(sc)
    worst = [0.0, 0.0]
    for f in range(6):
        m = sc.fr == f
        mk = lambda view: capi.ProblemArrays(sc.u[m], sc.v[m], sc.mcx[m], sc.mcy[m], sc.pt[m], np.zeros(int(m.sum()), np.uint32), sc.cam_gt, view, sc.pts_gt,
                                             sc.spx, sc.scale, sc.config, fixed_mask=0x1FFFF)
        pa, pb = mk(a.views[f].copy()), mk(sc.views_gt[6 * f: 6 * f + 6].copy())
        st = oracle.reproj_stats(pa, 1.0)
        s1, s2 = oracle.solve(pa), oracle.solve(pb)
        H = oracle.sweep(pb, radius=1e30, options=flat_hessian_options()).S[17:23, 17:23]
        d = pa.views - pb.views
        dc, dh = abs(s1.final_cost - s2.final_cost) / s2.final_cost, 0.5 * float(d @ H @ d) / s2.final_cost
        print(f"{key} frame {f}: start rms {st.std_x:.2f} {st.std_y:.2f} px, used {a.n_used[f]} of {a.n_groups[f]}; iterations {s1.iterations} (ground truth {s2.iterations}); "
              f"costs {dc:.1e} relative, 1/2 d^T H d {dh:.1e} of the cost")
        worst = [max(worst[0], dc), max(worst[1], dh)]
        assert dc <= 1e-4 and dh <= 4e-4
    print(f"{key}: worst {worst[0]:.1e}, {worst[1]:.1e}")


@pytest.mark.parametrize("key", list(POSE_FAMILIES))
def test_oracle_intersection_from_the_restatement_ends_in_the_ground_truth_valley(built, key):
    sc = family(key)
    p = ref_points(sc)
    assert np.all(p.status == 0)
    worst = [0.0, 0.0]
    oracle.set_fixed_frames(np.ones(6, np.uint8))
    try:
        for k in range(40):
            m = sc.pt == k
            mk = lambda pt0: capi.ProblemArrays(sc.u[m], sc.v[m], sc.mcx[m], sc.mcy[m], np.zeros(int(m.sum()), np.uint32), sc.fr[m], sc.cam_gt, sc.views_gt, pt0,
                                                sc.spx, sc.scale, sc.config | 0x500, fixed_mask=0x1FFFF)
            pa, pb = mk(p.pts[k].copy()), mk(sc.pts_gt[3 * k: 3 * k + 3].copy())
            s1, s2 = oracle.solve(pa), oracle.solve(pb)
            H = np.linalg.inv(oracle.sweep(pb, radius=1e30, options=flat_hessian_options()).point_hessian_inv.reshape(3, 3))
            d = pa.pts - pb.pts
            dc, dh = abs(s1.final_cost - s2.final_cost) / s2.final_cost, 0.5 * float(d @ H @ d) / s2.final_cost
            worst = [max(worst[0], dc), max(worst[1], dh)]
            assert dc <= 1e-4 and dh <= 4e-4, k
    finally:
        oracle.set_fixed_frames(None)
    print(f"{key}: start rms {rms_at(sc, sc.views_gt, p.pts):.4f} px (ground truth {rms_at(sc, sc.views_gt, sc.pts_gt):.4f}); worst costs {worst[0]:.1e} relative, "
          f"1/2 d^T H d {worst[1]:.1e} of the cost")
