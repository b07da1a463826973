"""Closed-form start values (include/lifcal_start.h) against the numpy restatement (tests/start_reference.py),
the CPU oracle and the two Levenberg-Marquardt calls they feed.

Bars
  groups   status, fr, pt, n_obs equal; |p_c - ref|_inf <= 16 eps cond(H_scaled) |p_c|_inf, the rounding bound of a 3x3 normal-equation
           solve (cond from the restatement); rms_px <= 1e-9 relative.  No group's rms_px lies within 1e-6 relative of the gate
           (asserted on the restatement), so the used sets must be equal.  The same bound for the points of lifcal_start_points.
  poses    against the restatement's alignment fed with the GPU's own group rows: angles <= 1e-11 rad, translation <= 1e-8 mm, n_used
           and status equal, sum_w <= 1e-12 relative.  align_rms is evaluated by either side at its own pose; the weighted RMS is
           1-Lipschitz in the residual vectors, which the pose bars move by at most 3 * 1e-11 * max |P| + sqrt(3) * 1e-8 mm: that
           distance (+ 1e-12 relative for the sums) is its bar.
  rows     sum_xx, sum_yy as RMS <= 1e-10 px, n_obs and n_inliers equal, against oracle.reproj_stats of the one-frame (one-point)
           problem at the returned pose (point).
  chains   startPoses -> resectFrames against resectFrames from views_gt (startPoints -> intersectPoints against the start from
           pts_gt): final costs within 1e-4 relative and 1/2 d^T H d <= 4e-4 of the cost, the same-valley bars of the far-start test
           of section 7m; n_used / n_groups >= 0.6 in every frame.

Measured on an MI355X over all cases below: p_c within 1.35 and points within 2.85 of eps cond |x| (bar 16), rms_px 1.3e-10 relative,
min_pivot 1.9e-15; angles 3.5e-16 rad, translation 3.2e-12 mm, sum_w 2.1e-16 relative, align_rms (125 .. 2444 mm) 4.5e-13 mm apart;
rows 1.5e-13 px; chains: final costs 9.1e-7 (poses) and 9.1e-7 (points) relative, 1/2 d^T H d 9.3e-7 and 2.8e-6 of the cost, the
figures of the restatement alone (tests/test_start_cpu.py); the resections take 3 .. 6 iterations from the start poses (2 .. 3 from
ground truth), the intersections 2 .. 10 (2 .. 9); used / groups 0.675 at least.  The 26 tests take 1.3 s on the GPU machine."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, _capi as capi, intersectPoints, resectFrames, scene, startPoints, startPoses
from tests import start_reference as sr
from tests import off_defaults as od
from tests.helpers import S, anisotropic_scene, spy_of

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
NAN6, NAN3 = np.full(6, np.nan).tobytes(), np.full(3, np.nan).tobytes()
FAMILIES = [   # the four families of tests/test_gpu_resection.py
    ("r2_tan_robust", S(6, 40, None, 0x306, 115, outlier_fraction=0.05)),
    ("r0", S(6, 40, None, 0x100, 7)),
    ("r1_tan_adj_robust", S(6, 40, None, 0xB05, 9, outlier_fraction=0.05)),
    ("r2_tan_adj", S(6, 40, None, 0x906, 11)),
]
POINT_FAMILIES = [   # three families of tests/test_gpu_intersection.py and a windowed scene whose points have from 3 observations
    ("p_r2_tan_adj_robust", S(6, 40, None, 0xF06, 115, outlier_fraction=0.05)),
    ("p_r0", S(6, 40, None, 0x500, 7)),
    ("p_r1_tan_adj", S(6, 40, None, 0xD05, 9)),
    ("p_window", S(12, 120, 3, 0xB06, 5, outlier_fraction=0.05)),
]
WIDE = S(2, 300, None, 0x306, 31, outlier_fraction=0.05)    # more groups per frame than one 256-lane pass
LONG = S(20, 12, None, 0x306, 21, outlier_fraction=0.05)    # 84 .. 156 observations per point (LONG of tests/test_gpu_intersection.py)
SPECS = dict(FAMILIES + POINT_FAMILIES + [("wide", WIDE), ("long", LONG)])


@functools.lru_cache(maxsize=None)
def scene_of(key):
    return scene.make_scene(SPECS[key])


class Obs:
    """the observations handed to a call: a selection (mask or positions, in that order) of a scene's, or arrays of its own"""

    def __init__(self, sc, idx=None, **replace):
        idx = np.arange(sc.n_obs) if idx is None else (np.flatnonzero(idx) if np.asarray(idx).dtype == bool else np.asarray(idx))
        self.sc = sc
        for name in ("u", "v", "mcx", "mcy", "pt", "fr"):
            setattr(self, name, replace.get(name, getattr(sc, name)[idx]).copy())
        self.pts = np.asarray(replace.get("pts", sc.pts_gt), np.float64).reshape(-1, 3)
        self.views = np.asarray(replace.get("views", sc.views_gt), np.float64).reshape(-1, 6)
        self.n_frames = replace.get("n_frames", len(self.views))
        self.n_points = replace.get("n_points", len(self.pts))

    def poses(self, gate=1.0):
        sc = self.sc
        return startPoses(sc.cam_gt, self.pts, self.u, self.v, self.mcx, self.mcy, self.pt, self.fr, self.n_frames, sc.config, sc.spx, sc.scale, spy=spy_of(sc),
                          gatePx=gate, wantGroups=True)

    def points(self):
        sc = self.sc
        return startPoints(sc.cam_gt, self.views, self.u, self.v, self.mcx, self.mcy, self.pt, self.fr, self.n_points, sc.config, sc.spx, sc.scale,
                           spy=spy_of(sc))

    def ref_groups(self, gate=1.0):
        sc = self.sc
        return sr.group_rows(sc.cam_gt, self.u, self.v, self.mcx, self.mcy, self.pt, self.fr, sc.config, sc.spx, sc.scale, spy=spy_of(sc), gate_px=gate)

    def ref_points(self):
        sc = self.sc
        return sr.start_points(sc.cam_gt, self.views, self.u, self.v, self.mcx, self.mcy, self.pt, self.fr, self.n_points, sc.config, sc.spx, sc.scale,
                               spy=spy_of(sc))


@functools.lru_cache(maxsize=None)
def batch(key):
    """(observations, startPoses result, startPoints result) of a whole scene, camera, points and poses at ground truth"""
    o = Obs(scene_of(key))
    return o, o.poses(), o.points()


MEASURED = {"p_c": [], "rms_px": [], "angles": [], "t": [], "align_rms": [], "x": [], "rows": []}


def check_groups(o, res, gate=1.0):
    """bar `groups` of the module docstring"""
    ref, cond = o.ref_groups(gate)
    tried = ref["status"] != 1
    if np.isfinite(gate):
        assert np.all(np.abs(ref["rms_px"][tried & (ref["status"] != 2)] - gate) > 1e-6 * gate)   # no group sits on the gate
    g = res.groups
    assert len(g) == len(ref)
    for name in ("status", "fr", "pt", "n_obs"):
        assert np.array_equal(g[name], ref[name]), name
    solved = np.isin(ref["status"], (0, 3, 4))
    err = np.max(np.abs(g["xyz"] - ref["xyz"]), axis=1)[solved] / (EPS * cond[solved] * np.max(np.abs(ref["xyz"]), axis=1)[solved])
    drms = np.abs(g["rms_px"] - ref["rms_px"])[solved] / ref["rms_px"][solved]
    MEASURED["p_c"].append(err.max()); MEASURED["rms_px"].append(drms.max())
    print(f"groups: {len(g)} ({np.bincount(g['status'], minlength=5)} by status), n_obs {g['n_obs'].min()} .. {g['n_obs'].max()}, scaled cond {cond[solved].min():.1e} .. {cond[solved].max():.1e}; "
          f"|dp_c| {err.max():.2f} of eps cond |p_c| (bar 16), rms_px {drms.max():.1e} relative")
    assert err.max() <= 16.0
    assert drms.max() <= 1e-9
    assert not g["xyz"][~solved].any() and not g["rms_px"][~solved].any()
    return ref


def check_poses(o, res):
    """bar `poses`: the alignment stage alone, fed with the GPU's own group rows"""
    views, status, n_groups, n_used, info = sr.poses_from_groups(res.groups, o.pts, o.n_frames)
    assert np.array_equal(res.rows["status"], status) and np.array_equal(res.rows["n_groups"], n_groups) and np.array_equal(res.rows["n_used"], n_used)
    assert np.array_equal(res.rows["n_obs"], np.bincount(o.fr, minlength=o.n_frames))
    for f in range(o.n_frames):
        if status[f] != 0:
            assert res.views[f].tobytes() == NAN6
            continue
        al = info[f]
        da, dt = np.max(np.abs(res.views[f, :3] - al.view[:3])), np.max(np.abs(res.views[f, 3:] - al.view[3:]))
        used = res.groups[(res.groups["fr"] == f) & (res.groups["status"] == 0)]
        bar = 3.0 * 1e-11 * np.max(np.linalg.norm(o.pts[used["pt"]], axis=1)) + np.sqrt(3.0) * 1e-8 + 1e-12 * al.align_rms
        dr = abs(res.rows["align_rms"][f] - al.align_rms)
        MEASURED["angles"].append(da); MEASURED["t"].append(dt); MEASURED["align_rms"].append(dr)
        print(f"frame {f}: used {n_used[f]} of {n_groups[f]}, gap {(al.eig[0] - al.eig[1]) / al.eig[0]:.3f}; angles {da:.1e} rad, t {dt:.1e} mm, align_rms {al.align_rms:.3f} mm ({dr:.1e} apart, bar {bar:.1e}), "
              f"sum_w {abs(res.rows['sum_w'][f] - al.sum_w) / al.sum_w:.1e} relative")
        assert da <= 1e-11
        assert dt <= 1e-8
        assert abs(res.rows["sum_w"][f] - al.sum_w) <= 1e-12 * al.sum_w
        assert dr <= bar
        assert np.max(np.abs(res.rows["eig"][f] - al.eig)) <= 1e-12 * abs(al.eig[0])


def check_stats(row, rms_x, rms_y, pa):
    st = oracle.reproj_stats(pa, 1.0)
    d = max(abs(rms_x - st.std_x), abs(rms_y - st.std_y))
    MEASURED["rows"].append(d)
    assert d <= 1e-10
    assert int(row["n_obs"]) == pa.struct.n_obs == st.num_points and int(row["n_inliers"]) == st.num_inliers


def check_pose_rows(o, res, nan_frames=()):
    """bar `rows` for the frames; nan_frames: frames with a NaN among their observations, whose error sums are NaN"""
    sc = o.sc
    for f in np.flatnonzero(res.status == 0):
        if f in nan_frames:
            assert np.isnan(res.rows["sum_xx"][f]) and int(res.rows["n_obs"][f]) == int(np.sum(o.fr == f))
            continue
        m = o.fr == f
        pa = capi.ProblemArrays(o.u[m], o.v[m], o.mcx[m], o.mcy[m], o.pt[m], np.zeros(int(m.sum()), np.uint32), sc.cam_gt, res.views[f].copy(), o.pts.reshape(-1),
                                sc.spx, sc.scale, sc.config, spy=spy_of(sc), fixed_mask=0x1FFFF)
        check_stats(res.rows[f], res.rms_x[f], res.rms_y[f], pa)
    bad = res.status != 0
    assert not res.rows["sum_xx"][bad].any() and not res.rows["n_inliers"][bad].any() and np.all(np.isnan(res.rms_x[bad]))


def check_points(o, res, only=None):
    """bars `groups` (for a point) and `rows` for the points"""
    sc = o.sc
    ref = o.ref_points()
    assert np.array_equal(res.status, ref.status)
    assert np.array_equal(res.rows["n_obs"], np.bincount(o.pt, minlength=o.n_points))
    ok = np.flatnonzero(res.status == 0)
    err = np.max(np.abs(res.pts[ok] - ref.pts[ok]), axis=1) / (EPS * ref.cond[ok] * np.max(np.abs(ref.pts[ok]), axis=1))
    dpiv = np.max(np.abs(res.rows["min_pivot"][ok] - ref.min_pivot[ok]))
    MEASURED["x"].append(err.max())
    print(f"points: {len(ok)} of {o.n_points} solved, n_obs {res.rows['n_obs'].min()} .. {res.rows['n_obs'].max()}, scaled cond {ref.cond[ok].min():.1e} .. {ref.cond[ok].max():.1e}; "
          f"|dP| {err.max():.2f} of eps cond |P| (bar 16), min_pivot {dpiv:.1e} apart")
    assert err.max() <= 16.0
    assert dpiv <= 1e-12   # (a pivot of a matrix with unit diagonal: an absolute measure)
    for k in range(o.n_points):
        if res.status[k] != 0:
            assert res.pts[k].tobytes() == NAN3 and res.rows["sum_xx"][k] == 0.0 and res.rows["n_inliers"][k] == 0
    oracle.set_fixed_frames(np.ones(len(o.views), np.uint8))   # (reproj_stats reads no mask; set as the one-point problems of the suite are)
    try:
        for k in (ok if only is None else only):
            m = o.pt == k
            pa = capi.ProblemArrays(o.u[m], o.v[m], o.mcx[m], o.mcy[m], np.zeros(int(m.sum()), np.uint32), o.fr[m], sc.cam_gt, o.views.reshape(-1), res.pts[k].copy(),
                                    sc.spx, sc.scale, sc.config | 0x500, spy=spy_of(sc), fixed_mask=0x1FFFF)
            check_stats(res.rows[k], res.rms_x[k], res.rms_y[k], pa)
    finally:
        oracle.set_fixed_frames(None)
    return ref


def print_measured():
    print("measured so far: " + ", ".join(f"{k} {max(v):.2e}" for k, v in MEASURED.items() if v))


@pytest.mark.parametrize("key", [c[0] for c in FAMILIES])
def test_groups_poses_and_rows_of_the_families(built, key):
    o, res, _ = batch(key)
    assert len(res.rows) == 6 and np.all(res.status == 0)
    check_groups(o, res)
    check_poses(o, res)
    check_pose_rows(o, res)
    print_measured()


@pytest.mark.parametrize("key", [c[0] for c in FAMILIES + POINT_FAMILIES])
def test_points_of_the_families(built, key):
    o, _, res = batch(key)
    assert np.all(res.status == 0)
    check_points(o, res)
    print_measured()


def test_poses_and_points_with_a_y_pitch_of_its_own(built):
    """spy = 1.25 spx (tests/helpers.anisotropic_scene) against the restatement with spy passed, on the families that have tangential
    terms and centre adjustment; the restatement without spy, which is what a pitch read from the x slot computes, lies millimetres
    away from it (4 .. 44 mm in the translations, metres in the points), where the bars are 1e-8 mm and 16 eps cond |P|"""
    for key in ("r2_tan_robust", "r1_tan_adj_robust"):
        o = Obs(anisotropic_scene(scene_of(key), od.A))
        sc = o.sc
        assert sc.spy == od.A * sc.spx
        res, pres = o.poses(), o.points()
        assert np.all(res.status == 0) and np.all(pres.status == 0)
        check_groups(o, res)
        check_poses(o, res)
        check_pose_rows(o, res)
        ref = check_points(o, pres)
        obs = (o.u, o.v, o.mcx, o.mcy, o.pt, o.fr)
        with_spy = sr.start_poses(sc.cam_gt, o.pts, *obs, o.n_frames, sc.config, sc.spx, sc.scale, spy=sc.spy)
        iso_poses = sr.start_poses(sc.cam_gt, o.pts, *obs, o.n_frames, sc.config, sc.spx, sc.scale)
        iso_points = sr.start_points(sc.cam_gt, o.views, *obs, o.n_points, sc.config, sc.spx, sc.scale)
        dv, dp = np.max(np.abs(with_spy.views - iso_poses.views), axis=1), np.max(np.abs(ref.pts - iso_points.pts), axis=1)
        print(f"{key}: restatement with spy = spx: poses {dv.min():.2e} .. {dv.max():.2e}, points {dp.min():.2e} .. {dp.max():.2e} mm away; "
              f"GPU poses {np.max(np.abs(res.views - with_spy.views)):.1e} from the restatement's")
        assert np.all(dv > 1e-2) and np.median(dp) > 1e-2
        assert np.max(np.abs(res.views - with_spy.views)) <= 1e-6   # (the whole chain; check_poses holds the alignment to 1e-11 / 1e-8)
    print_measured()


def raw_poses(o, views, gate=1.0):
    """lifcal_start_poses on a caller's own views buffer (the Python wrapper hands over NaNs)"""
    sc = o.sc
    lib = capi.load_library()
    cam, pts = np.ascontiguousarray(sc.cam_gt, np.float64), np.ascontiguousarray(o.pts.reshape(-1))
    arr = [np.ascontiguousarray(a, np.float64) for a in (o.u, o.v, o.mcx, o.mcy)] + [np.ascontiguousarray(a, np.uint32) for a in (o.pt, o.fr)]
    p = capi.ResectProblem()
    p.n_obs, p.n_frames, p.n_points = len(o.u), o.n_frames, len(o.pts)
    p.u, p.v, p.mcx, p.mcy = (capi.as_dptr(a) for a in arr[:4])
    p.pt, p.fr = capi.as_uptr(arr[4]), capi.as_uptr(arr[5])
    p.cam, p.pts, p.views = capi.as_dptr(cam), capi.as_dptr(pts), capi.as_dptr(views)
    p.spx = p.spy = float(sc.spx); p.scale = float(sc.scale); p.config = int(sc.config)
    rows = np.zeros(o.n_frames, capi.START_FRAME_DTYPE)
    opt = capi.default_options_py()
    assert lib.lifcal_start_poses(C.byref(p), C.byref(opt), gate, 1.0, rows.ctypes.data, None, None, None) == 0, lib.lifcal_ba_last_error()
    return rows


@pytest.mark.parametrize("key", [c[0] for c in FAMILIES])
def test_resection_from_the_start_poses_ends_in_the_ground_truth_valley(built, key):
    sc = scene_of(key)
    o, res, _ = batch(key)
    assert np.all(res.status == 0)
    ratio = res.rows["n_used"] / res.rows["n_groups"]
    assert np.all(ratio >= 0.6)   # the cap that keeps the gate from hiding a failure
    # the incoming views are never read: zeros instead of the wrapper's NaNs give the same bits
    views = np.zeros(36)
    rows = raw_poses(o, views)
    assert rows.tobytes() == res.rows.tobytes() and views.tobytes() == res.views.tobytes()
    args = (sc.cam_gt, sc.pts_gt, sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)
    got = resectFrames(*args, res.views, sc.config, sc.spx, sc.scale)
    near = resectFrames(*args, sc.views_gt, sc.config, sc.spx, sc.scale)
    d = got.views - near.views
    dc = np.abs(got.final_cost - near.final_cost) / near.final_cost
    dh = 0.5 * np.einsum("fi,fij,fj->f", d, near.H, d) / near.final_cost
    print(f"{key}: start rms x {np.round(res.rms_x, 2)} y {np.round(res.rms_y, 2)} px, used / groups {ratio.min():.3f} .. {ratio.max():.3f}; iterations {got.iterations} (from ground truth {near.iterations}); "
          f"final costs {dc.max():.1e} relative, 1/2 d^T H d {dh.max():.1e} of the cost")
    assert np.all(dc <= 1e-4)
    assert np.all(dh <= 4e-4)


@pytest.mark.parametrize("key", [c[0] for c in POINT_FAMILIES])
def test_intersection_from_the_start_points_ends_in_the_ground_truth_valley(built, key):
    sc = scene_of(key)
    _, _, res = batch(key)
    assert np.all(res.status == 0)
    args = (sc.cam_gt, sc.views_gt, sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)
    got = intersectPoints(*args, res.pts, sc.config, sc.spx, sc.scale)
    near = intersectPoints(*args, sc.pts_gt, sc.config, sc.spx, sc.scale)
    d = got.pts - near.pts
    dc = np.abs(got.final_cost - near.final_cost) / near.final_cost
    dh = 0.5 * np.einsum("pi,pij,pj->p", d, near.H, d) / near.final_cost
    n = res.rows["n_obs"]
    rms = np.sqrt((res.rows["sum_xx"] + res.rows["sum_yy"]).sum() / n.sum())
    print(f"{key}: observations per point {n.min()} .. {n.max()}, start rms {rms:.4f} px; iterations {got.iterations.min()} .. {got.iterations.max()} (from ground truth "
          f"{near.iterations.min()} .. {near.iterations.max()}); final costs {dc.max():.1e} relative, 1/2 d^T H d {dh.max():.1e} of the cost")
    if key == "p_window":
        assert n.min() == 3
    assert np.all(dc <= 1e-4)
    assert np.all(dh <= 4e-4)


def test_bitwise_reproducible_and_rows_independent(built):
    key = FAMILIES[0][0]
    sc = scene_of(key)
    o, res, pres = batch(key)
    again, pagain = o.poses(), o.points()
    for a, b in ((again.rows, res.rows), (again.groups, res.groups), (again.views, res.views), (pagain.rows, pres.rows), (pagain.pts, pres.pts)):
        assert a.tobytes() == b.tobytes()
    # frame 3 alone (its group rows then name frame 0), point 3 alone
    m = sc.fr == 3
    alone = Obs(sc, m, fr=np.zeros(int(m.sum()), np.uint32), n_frames=1).poses()
    g3 = res.groups[res.groups["fr"] == 3].copy(); g3["fr"] = 0
    assert alone.rows[0].tobytes() == res.rows[3].tobytes() and alone.views[0].tobytes() == res.views[3].tobytes() and alone.groups.tobytes() == g3.tobytes()
    m = sc.pt == 3
    alone = Obs(sc, m, pt=np.zeros(int(m.sum()), np.uint32), n_points=1).points()
    assert alone.rows[0].tobytes() == pres.rows[3].tobytes() and alone.pts[0].tobytes() == pres.pts[3].tobytes()
    # the frames' (points') observation blocks in reverse order, the order inside a block unchanged
    rev = Obs(sc, np.concatenate([np.flatnonzero(sc.fr == f) for f in reversed(range(6))])).poses()
    assert rev.rows.tobytes() == res.rows.tobytes() and rev.views.tobytes() == res.views.tobytes() and rev.groups.tobytes() == res.groups.tobytes()
    rev = Obs(sc, np.concatenate([np.flatnonzero(sc.pt == k) for k in reversed(range(40))])).points()
    assert rev.rows.tobytes() == pres.rows.tobytes() and rev.pts.tobytes() == pres.pts.tobytes()


def test_handle_methods_forward_to_the_free_functions(built):
    key = FAMILIES[0][0]
    sc = scene_of(key)
    _, res, pres = batch(key)
    pa = capi.ProblemArrays(sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.cam_gt, sc.views_gt, sc.pts_gt, sc.spx, sc.scale, sc.config, fixed_mask=0x1FFFF)
    with BundleAdjustment(pa) as ba:
        a, b = ba.startPoses(wantGroups=True), ba.startPoints()
    assert a.rows.tobytes() == res.rows.tobytes() and a.views.tobytes() == res.views.tobytes() and a.groups.tobytes() == res.groups.tobytes()
    assert b.rows.tobytes() == pres.rows.tobytes() and b.pts.tobytes() == pres.pts.tobytes()


def test_more_groups_than_one_pass_and_a_long_serial_run(built):
    o, res, _ = batch("wide")
    n = res.rows["n_groups"]
    assert np.all(n > 256) and np.all(n % 64 != 0) and len(res.groups) % 256 != 0
    check_groups(o, res); check_poses(o, res); check_pose_rows(o, res)
    # a group made of 70 repeated observations: the observations of frame 0's first used group cycled up to 70
    sc = o.sc
    k = res.groups["pt"][(res.groups["fr"] == 0) & (res.groups["status"] == 0)][0]
    first = np.flatnonzero((sc.fr == 0) & (sc.pt == k))
    rest = np.setdiff1d(np.arange(sc.n_obs), first)
    o70 = Obs(sc, np.concatenate([np.resize(first, 70), rest]))
    r70 = o70.poses()
    g70 = r70.groups[(r70.groups["fr"] == 0) & (r70.groups["pt"] == k)]
    assert g70["n_obs"][0] == 70 and g70["status"][0] == 0
    check_groups(o70, r70); check_poses(o70, r70); check_pose_rows(o70, r70)
    print_measured()


def test_more_observations_than_one_pass_of_the_wave_and_exactly_two(built):
    o, _, res = batch("long")
    n = res.rows["n_obs"]
    assert n.min() > 64 and np.sum(n > 128) >= 3 and np.all(n % 64 != 0) and np.all(res.status == 0)
    check_points(o, res)
    # point 6 cut down to two observations in two different frames; 11 points: the last workgroup has an idle wave
    sc = o.sc
    keep = sc.pt != 11
    i6 = np.flatnonzero(sc.pt == 6)
    second = i6[np.flatnonzero(sc.fr[i6] != sc.fr[i6[0]])[0]]
    keep[i6] = False; keep[[i6[0], second]] = True
    o2 = Obs(sc, keep, n_points=11)
    r2 = o2.points()
    assert r2.rows["n_obs"][6] == 2 and r2.status[6] == 0
    check_points(o2, r2, only=[5, 6, 7])
    others = np.setdiff1d(np.arange(11), [6])
    assert r2.rows[others].tobytes() == res.rows[others].tobytes() and r2.pts[others].tobytes() == res.pts[others].tobytes()
    print_measured()


def test_edges_of_the_poses(built):
    key = FAMILIES[0][0]
    sc = scene_of(key)
    o, res, _ = batch(key)
    used = lambda f: res.groups["pt"][(res.groups["fr"] == f) & (res.groups["status"] == 0)]
    keep = np.ones(sc.n_obs, bool)
    keep[sc.fr == 1] = False                                           # frame 1: empty
    two = used(2)[:2]
    keep[(sc.fr == 2) & ~np.isin(sc.pt, two)] = False                  # frame 2: two used groups
    singles = used(4)[:5]                                              # frame 4: five groups cut down to their first observation
    for k in singles:
        i = np.flatnonzero((sc.fr == 4) & (sc.pt == k)); keep[i[1:]] = False
    u = sc.u.copy()
    bad = used(5)[3]                                                   # frame 5: a NaN in the second observation of one group
    u[np.flatnonzero((sc.fr == 5) & (sc.pt == bad))[1]] = np.nan
    pt = sc.pt.copy(); pt[sc.fr == 3] += 40                            # frame 3: its points 40 .. 79 lie on one line
    line = np.outer(np.arange(40) + 1.0, [30.0, -20.0, 10.0]) + sc.pts_gt.reshape(-1, 3).mean(0)
    idx = np.flatnonzero(keep)
    oe = Obs(sc, idx, u=u[idx], pt=pt[idx], pts=np.concatenate([sc.pts_gt.reshape(-1, 3), line]))
    r = oe.poses()
    assert list(r.status) == [0, 1, 2, 3, 0, 0]
    for f in (1, 2, 3):
        assert r.views[f].tobytes() == NAN6 and r.rows["sum_xx"][f] == 0.0 and r.rows["align_rms"][f] == 0.0
    zero = r.rows[1:2].copy(); zero["status"] = 0
    assert not zero.view(np.uint8).any()
    assert r.rows["n_used"][2] == 2 and r.rows["n_groups"][2] == 2 and r.rows["sum_w"][2] > 0.0
    assert r.rows["n_used"][3] >= 3 and r.rows["eig"][3, 0] - r.rows["eig"][3, 1] <= 1e-9 * abs(r.rows["eig"][3, 0])
    print(f"collinear frame: eigenvalues {r.rows['eig'][3]}, relative gap {(r.rows['eig'][3, 0] - r.rows['eig'][3, 1]) / r.rows['eig'][3, 0]:.1e}")
    # frame 0 is as without all this, bit for bit; so is every group that was not touched
    assert r.rows[0].tobytes() == res.rows[0].tobytes() and r.views[0].tobytes() == res.views[0].tobytes()
    g = r.groups
    assert np.array_equal(g["status"][(g["fr"] == 4) & np.isin(g["pt"], singles)], np.ones(5, np.int32))
    assert r.rows["n_used"][4] == res.rows["n_used"][4] - 5 and r.rows["n_groups"][4] == 40
    nan_group = g[(g["fr"] == 5) & (g["pt"] == bad)]
    assert nan_group["status"][0] == 2 and not nan_group["xyz"].any() and r.rows["n_used"][5] == res.rows["n_used"][5] - 1
    same = lambda t, f, skip: t[(t["fr"] == f) & ~np.isin(t["pt"], skip)].tobytes()
    assert same(g, 4, singles) == same(res.groups, 4, singles) and same(g, 5, [bad]) == same(res.groups, 5, [bad]) and same(g, 0, []) == same(res.groups, 0, [])
    # statuses and counts are the restatement's; the poses that exist follow from the GPU's group rows
    check_groups(oe, r); check_poses(oe, r); check_pose_rows(oe, r, nan_frames=(5,))
    # no gate: every group that could be solved and lies in front of the camera is used
    rinf = o.poses(gate=float("inf"))
    check_groups(o, rinf, gate=float("inf")); check_poses(o, rinf)
    assert not np.any(rinf.groups["status"] == 4) and np.any(res.groups["status"] == 4)
    assert np.array_equal(rinf.rows["n_used"], np.bincount(rinf.groups["fr"][np.isin(res.groups["status"], (0, 4))], minlength=6))


def test_edges_of_the_points(built):
    key = POINT_FAMILIES[0][0]
    sc = scene_of(key)
    _, _, res = batch(key)
    keep = np.ones(sc.n_obs, bool)
    keep[sc.pt == 7] = False                                           # point 7: no observation
    i9 = np.flatnonzero(sc.pt == 9); keep[i9[1:]] = False              # point 9: a single observation
    r = Obs(sc, keep).points()
    assert r.status[7] == 1 and r.status[9] == 2 and r.rows["n_obs"][7] == 0 and r.rows["n_obs"][9] == 1
    zero = r.rows[[7, 9]].copy(); zero["status"] = 0; zero["n_obs"] = 0
    assert not zero.view(np.uint8).any()
    assert r.pts[7].tobytes() == NAN3 and r.pts[9].tobytes() == NAN3
    others = np.setdiff1d(np.arange(40), [7, 9])
    assert r.rows[others].tobytes() == res.rows[others].tobytes() and r.pts[others].tobytes() == res.pts[others].tobytes()
