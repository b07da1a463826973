"""lifcal_register_scene (include/lifcal_register.h) against the gpu arm of its restatement
(tests/register_reference.py: the same round logic driven from the host over startPoses, resectFrames and intersectPoints), the CPU
oracle and ground truth.

Bars
  driver     on every scene below, the noise-free ones included: anchor_frame, n_rounds, every frame's and point's status and round, n_shared, n_obs_used, n_frames_used, n_groups, n_used
             equal (no group of the driver sits within 1e-6 relative of the gate); poses and points within the project's full-solve
             bar 1e-6 (rad; translations relative to max |t|; points relative to |P|); iterations and termination of every last solve
             equal; their final_cost within 1e-8 relative of the driver's solve of the same step on the noisy scenes (bounded by
             the cost of 1e-6 px residuals on the noise-free ones, where it has no significant digits).
  rows       sum_xx, sum_yy as RMS within 1e-10 px, n_obs_used and n_inliers equal, against oracle.reproj_stats at the returned
             parameters over exactly the observations the row claims; final_cost within 1e-8 relative against oracle.cost of the same
             one-frame problem.  A point's last solve precedes the last pose refinement, so its final_cost is checked where no pose
             changes afterwards: a call whose min_shared no frame reaches (the anchor alone).
  noise-free 1e-6 rad, 1e-5 mm (translations), 1e-4 mm (points) from ground truth with the anchor at its true pose.
  end to end the handle's bundle adjustment from the result against the one from ground truth: final costs within 1e-4 relative.

Measured on an MI355X over all cases below: poses 3.4e-14 rad and 4.7e-13 of max |t|, points 1.6e-12 of |P| from the driver, every
integer and every iteration count equal (noise-free scenes: 5.0e-15 rad, 2.2e-14, 1.3e-15), final costs of the last solves 1.4e-11
relative from the driver's (noise-free: 0 .. 4.4e-15, 1.7e-20 apart); rows 2.1e-13 px, final costs 1.1e-13 (frames) and 4.1e-12 (points) relative; noise-free
2.7e-11 rad, 1.3e-7 mm, 3.2e-6 mm; end to end final costs within 5.7e-7 relative, start RMS 0.57 .. 0.63 px, the bundle adjustment takes
5 .. 15 iterations (5 .. 7 from ground truth)."""
import functools
import os

import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, _capi as capi, registerScene, scene
from tests import register_reference as rr
from tests import off_defaults as od
from tests.helpers import S, anisotropic_scene, spy_of

pytestmark = pytest.mark.gpu

NAN6, NAN3 = np.full(6, np.nan).tobytes(), np.full(3, np.nan).tobytes()
CASES = {   # spec, min_shared: the scenes of tests/test_register_cpu.py, then WIDE and LONG of tests/test_gpu_start.py
    "r2_tan_robust": (S(6, 40, None, 0x306, 115, outlier_fraction=0.05), 6),
    "r0": (S(6, 40, None, 0x100, 7), 6),
    "r1_tan_adj_robust": (S(6, 40, None, 0xB05, 9, outlier_fraction=0.05), 6),
    "r2_tan_adj": (S(6, 40, None, 0x906, 11), 6),
    "p_r2_tan_adj_robust": (S(6, 40, None, 0xF06, 115, outlier_fraction=0.05), 6),
    "p_r0": (S(6, 40, None, 0x500, 7), 6),
    "p_r1_tan_adj": (S(6, 40, None, 0xD05, 9), 6),
    "p_window": (S(12, 120, 3, 0xB06, 5, outlier_fraction=0.05), 3),
    "windowed": (S(24, 120, 6, 0xF06, 119, outlier_fraction=0.02), 6),
    "wide": (S(2, 300, None, 0x306, 31, outlier_fraction=0.05), 6),     # more than 256 groups per frame
    "long": (S(20, 12, None, 0x306, 21, outlier_fraction=0.05), 6),     # 84 .. 156 observations per point
    "nf_all_frames": (S(6, 40, None, 0x906, 11, noise_px=0.0), 6),
    "nf_window6": (S(24, 120, 6, 0xF06, 119, noise_px=0.0), 6),
    "nf_window3": (S(12, 120, 3, 0xB06, 5, noise_px=0.0), 3),
}
NOISY = [k for k in CASES if not k.startswith("nf_")]
MEASURED = {"rad": [], "t": [], "P": [], "rows": [], "cost": [], "driver_cost": []}


@functools.lru_cache(maxsize=None)
def scene_of(key):
    return scene.make_scene(CASES[key][0])


def obs_of(sc):
    return sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr


def device(key, obs=None, n_frames=None, n_points=None, **kw):
    sc = scene_of(key)
    spec, ms = CASES[key]
    kw.setdefault("minShared", ms)
    return registerScene(sc.cam_gt, *(obs_of(sc) if obs is None else obs), spec.n_frames if n_frames is None else n_frames,
                         spec.n_points if n_points is None else n_points, sc.config, sc.spx, sc.scale, **kw)


@functools.lru_cache(maxsize=None)
def device_default(key):
    return device(key)


@functools.lru_cache(maxsize=None)
def driver(key):
    sc = scene_of(key)
    spec, ms = CASES[key]
    return rr.register("gpu", sc.cam_gt, *obs_of(sc), spec.n_frames, spec.n_points, sc.config, sc.spx, sc.scale, min_shared=ms)


def assert_same_bookkeeping(got, ref):
    """bar `driver`, the integers"""
    g = ref.groups
    tried = ~np.isin(g["status"], (1, 2))
    assert np.all(np.abs(g["rms_px"][tried] - 1.0) > 1e-6)   # no group sits on the gate
    s = got.summary
    assert (s.anchor_frame, s.n_rounds, s.n_groups, s.n_groups_used) == (ref.anchor_frame, ref.n_rounds, len(g), int(np.sum(g["status"] == 0)))
    assert (s.n_frames_registered, s.n_points_mapped) == (int(ref.registered.sum()), int(ref.mapped.sum()))
    f, p = got.frame_rows, got.point_rows
    for name, want in (("status", ref.f_status), ("round", ref.f_round), ("n_obs", ref.f_n_obs), ("n_obs_used", ref.f_n_obs_used), ("n_groups", ref.f_n_groups),
                       ("n_used", ref.f_n_used), ("n_shared", ref.f_n_shared)):
        assert np.array_equal(f[name], want), name
    for name, want in (("status", ref.p_status), ("round", ref.p_round), ("n_obs", ref.p_n_obs), ("n_obs_used", ref.p_n_obs_used), ("n_frames_used", ref.p_n_frames_used)):
        assert np.array_equal(p[name], want), name
    assert np.array_equal(got.registered, ref.registered) and np.array_equal(got.mapped, ref.mapped)
    for k in np.flatnonzero(~got.registered):
        assert got.views[k].tobytes() == NAN6
    for k in np.flatnonzero(~got.mapped):
        assert got.pts[k].tobytes() == NAN3


@pytest.mark.parametrize("key", list(CASES))
def test_the_chain_on_the_device_is_the_drivers(built, key):
    got, ref = device_default(key), driver(key)
    assert_same_bookkeeping(got, ref)
    reg, mp = ref.registered, ref.mapped
    da = np.abs(got.views[reg, :3] - ref.views[reg, :3]).max()
    dt = np.abs(got.views[reg, 3:] - ref.views[reg, 3:]).max() / max(np.abs(ref.views[reg, 3:]).max(), 1e-300)
    dp = (np.linalg.norm(got.pts[mp] - ref.pts[mp], axis=1) / np.linalg.norm(ref.pts[mp], axis=1)).max()
    MEASURED["rad"].append(da); MEASURED["t"].append(dt); MEASURED["P"].append(dp)
    fi = [(int(got.frame_rows["iterations"][f]), int(got.frame_rows["termination"][f])) for f in np.flatnonzero(reg)]
    pi = [(int(got.point_rows["iterations"][k]), int(got.point_rows["termination"][k])) for k in np.flatnonzero(mp)]
    print(f"{key}: anchor {ref.anchor_frame}, {ref.n_rounds} rounds, {int(reg.sum())} frames, {int(mp.sum())} points; {da:.1e} rad, t {dt:.1e} and P {dp:.1e} relative; "
          f"rms {got.rms_x:.3f} {got.rms_y:.3f} px; kernel time {got.seconds * 1e3:.2f} ms; so far " + ", ".join(f"{k} {max(v):.1e}" for k, v in MEASURED.items() if v))
    # the final cost of every last solve against the driver's solve of the same step (a point's last solve precedes the last pose
    # refinement, so the oracle at the returned parameters cannot be asked, see check_rows)
    fc = np.array([[got.frame_rows["final_cost"][f], ref.f_last[int(f)][0]] for f in np.flatnonzero(reg) if f != ref.anchor_frame]).reshape(-1, 2)
    pc = np.array([[got.point_rows["final_cost"][k], ref.p_last[int(k)][0]] for k in np.flatnonzero(mp)]).reshape(-1, 2)
    c = np.concatenate([fc, pc])
    dc = np.abs(c[:, 0] - c[:, 1]) / np.maximum(c[:, 1], 1e-300)
    print(f"{key}: final costs of the last solves {c[:, 1].min():.2e} .. {c[:, 1].max():.2e}, from the driver's at most {dc.max():.1e} relative ({np.abs(c[:, 0] - c[:, 1]).max():.1e} absolute)")
    assert fi == [ref.f_last[int(f)][1:] for f in np.flatnonzero(reg)]
    assert pi == [ref.p_last[int(k)][1:] for k in np.flatnonzero(mp)]
    assert da <= 1e-6 and dt <= 1e-6 and dp <= 1e-6
    if key in NOISY:   # (the bar of the rows' final_cost)
        MEASURED["driver_cost"].append(dc.max())
        assert dc.max() <= 1e-8
    else:
        # A noise-free solve ends at a cost that is the square of the distance left to a zero-residual solution when a tolerance
        # fired: a number that is sensitive to the last bits of its inputs, without common digits between two runs.  It is bounded, not compared: below
        # the cost of residuals of 1e-6 px, four digits under the noise of any real scene.
        n = np.concatenate([got.frame_rows["n_obs_used"][[f for f in np.flatnonzero(reg) if f != ref.anchor_frame]], got.point_rows["n_obs_used"][mp]])
        assert np.all(c <= (n * 1e-12)[:, None])
    if key == "wide":
        assert np.all(got.frame_rows["n_groups"] > 256) and int(mp.sum()) == 287
    if key == "long":
        assert got.point_rows["n_obs_used"].min() > 64


def one_frame(sc, got, f, obs=None):
    u, v, mcx, mcy, pt, fr = obs_of(sc) if obs is None else obs
    m = (fr == f) & got.mapped[pt]
    return capi.ProblemArrays(u[m], v[m], mcx[m], mcy[m], pt[m], np.zeros(int(m.sum()), np.uint32), sc.cam_gt, got.views[f].copy(), np.nan_to_num(got.pts).reshape(-1),
                              sc.spx, sc.scale, (sc.config & rr.MODEL_BITS) | 0x100, spy=spy_of(sc), fixed_mask=0x1FFFF)


def one_point(sc, got, k, obs=None):
    u, v, mcx, mcy, pt, fr = obs_of(sc) if obs is None else obs
    m = (pt == k) & got.registered[fr]
    return capi.ProblemArrays(u[m], v[m], mcx[m], mcy[m], np.zeros(int(m.sum()), np.uint32), fr[m], sc.cam_gt, np.nan_to_num(got.views).reshape(-1), got.pts[k].copy(),
                              sc.spx, sc.scale, (sc.config & rr.MODEL_BITS) | 0x500, spy=spy_of(sc), fixed_mask=0x1FFFF)


def check_stats(row, pa):
    st = oracle.reproj_stats(pa, 1.0)
    n = int(row["n_obs_used"])
    d = max(abs(np.sqrt(row["sum_xx"] / n) - st.std_x), abs(np.sqrt(row["sum_yy"] / n) - st.std_y))
    MEASURED["rows"].append(d)
    assert d <= 1e-10
    assert n == pa.struct.n_obs == st.num_points and int(row["n_inliers"]) == st.num_inliers


def check_rows(sc, got, point_costs=False, obs=None):
    """bar `rows`"""
    oracle.set_fixed_frames(None)
    for f in np.flatnonzero(got.registered):
        pa = one_frame(sc, got, f, obs)
        check_stats(got.frame_rows[f], pa)
        if got.frame_rows["round"][f] > 0:
            c = oracle.cost(pa)
            MEASURED["cost"].append(abs(got.frame_rows["final_cost"][f] - c) / c)
            assert abs(got.frame_rows["final_cost"][f] - c) <= 1e-8 * c
        else:   # the anchor has no solve
            assert got.frame_rows["final_cost"][f] == 0.0 and got.frame_rows["iterations"][f] == 0
    oracle.set_fixed_frames(np.ones(len(got.views), np.uint8))   # (as the one-point problems of the suite are set up)
    try:
        for k in np.flatnonzero(got.mapped):
            pa = one_point(sc, got, k, obs)
            check_stats(got.point_rows[k], pa)
            if point_costs:
                c = oracle.cost(pa)
                MEASURED["cost"].append(abs(got.point_rows["final_cost"][k] - c) / c)
                assert abs(got.point_rows["final_cost"][k] - c) <= 1e-8 * c
    finally:
        oracle.set_fixed_frames(None)
    bad = ~got.registered
    assert not got.frame_rows["sum_xx"][bad].any() and not got.frame_rows["n_inliers"][bad].any() and not got.frame_rows["n_obs_used"][bad].any()
    bad = ~got.mapped
    assert not got.point_rows["sum_xx"][bad].any() and not got.point_rows["n_inliers"][bad].any() and not got.point_rows["n_obs_used"][bad].any()


@pytest.mark.parametrize("key", ["r2_tan_robust", "r1_tan_adj_robust", "p_window", "wide", "long"])
def test_rows_against_the_oracle(built, key):
    check_rows(scene_of(key), device_default(key))
    print(f"{key}: rows within {max(MEASURED['rows']):.1e} px, final costs within {max(MEASURED['cost']):.1e} relative")


def test_a_scene_with_a_y_pitch_of_its_own_is_registered_like_the_drivers(built):
    """spy = 1.25 spx (tests/helpers.anisotropic_scene) through the whole chain, the bars of `driver` and `rows`; the driver with
    spy = spx, which is what a pitch read from the x slot computes, ends millimetres away"""
    key = "r1_tan_adj_robust"
    spec, ms = CASES[key]
    sc = anisotropic_scene(scene_of(key), od.A)
    got = registerScene(sc.cam_gt, *obs_of(sc), spec.n_frames, spec.n_points, sc.config, sc.spx, sc.scale, spy=sc.spy, minShared=ms)
    ref = rr.register("gpu", sc.cam_gt, *obs_of(sc), spec.n_frames, spec.n_points, sc.config, sc.spx, sc.scale, min_shared=ms, spy=sc.spy)
    iso = rr.register("gpu", sc.cam_gt, *obs_of(sc), spec.n_frames, spec.n_points, sc.config, sc.spx, sc.scale, min_shared=ms)
    assert_same_bookkeeping(got, ref)
    reg, mp = ref.registered, ref.mapped
    assert reg.sum() == spec.n_frames and mp.sum() >= 30
    da = np.abs(got.views[reg, :3] - ref.views[reg, :3]).max()
    dt = np.abs(got.views[reg, 3:] - ref.views[reg, 3:]).max() / np.abs(ref.views[reg, 3:]).max()
    dp = (np.linalg.norm(got.pts[mp] - ref.pts[mp], axis=1) / np.linalg.norm(ref.pts[mp], axis=1)).max()
    both = mp & iso.mapped
    wrong = np.median(np.linalg.norm(iso.pts[both] - ref.pts[both], axis=1) / np.linalg.norm(ref.pts[both], axis=1))
    print(f"anisotropic {key}: {ref.n_rounds} rounds, {int(mp.sum())} points; {da:.1e} rad, t {dt:.1e} and P {dp:.1e} relative; the driver with spy = spx: P {wrong:.1e} relative")
    assert da <= 1e-6 and dt <= 1e-6 and dp <= 1e-6
    assert wrong > 1e-3
    assert [(int(got.frame_rows["iterations"][f]), int(got.frame_rows["termination"][f])) for f in np.flatnonzero(reg)] == [ref.f_last[int(f)][1:] for f in np.flatnonzero(reg)]
    assert [(int(got.point_rows["iterations"][k]), int(got.point_rows["termination"][k])) for k in np.flatnonzero(mp)] == [ref.p_last[int(k)][1:] for k in np.flatnonzero(mp)]
    check_rows(sc, got)


def test_min_shared_not_reached_leaves_the_anchor_alone(built):
    key = "r2_tan_robust"
    sc = scene_of(key)
    got = device(key, minShared=41, anchorFrame=3)
    s = got.summary
    assert (s.anchor_frame, s.n_rounds, s.n_frames_registered) == (3, 0, 1)
    assert list(got.frame_rows["status"]) == [2, 2, 2, 0, 2, 2] and list(got.frame_rows["round"]) == [-1, -1, -1, 0, -1, -1]
    used = got.frame_rows["n_used"]
    assert s.n_points_mapped == used[3] == got.frame_rows["n_shared"][3] and np.all(got.frame_rows["n_shared"] <= used) and np.all(got.frame_rows["n_shared"] > 0)
    assert got.views[3].tobytes() == np.zeros(6).tobytes() and np.all(got.point_rows["round"][got.mapped] == 0) and np.all(got.point_rows["n_frames_used"][got.mapped] == 1)
    check_rows(sc, got, point_costs=True)
    print(f"anchor alone: {s.n_points_mapped} points, final costs within {max(MEASURED['cost']):.1e} relative")


@pytest.mark.parametrize("key", ["nf_all_frames", "nf_window6", "nf_window3"])
def test_a_noise_free_scene_is_reproduced_in_the_anchors_frame(built, key):
    sc = scene_of(key)
    vg, pg = sc.views_gt.reshape(-1, 6), sc.pts_gt.reshape(-1, 3)
    a = device_default(key).summary.anchor_frame
    r = device(key, anchorFrame=a, anchorView=vg[a])
    assert r.summary.anchor_frame == a and np.all(r.registered) and np.all(r.mapped) and r.views[a].tobytes() == vg[a].tobytes()
    da, dt, dp = np.abs(r.views[:, :3] - vg[:, :3]).max(), np.abs(r.views[:, 3:] - vg[:, 3:]).max(), np.abs(r.pts - pg).max()
    print(f"{key}: anchor {a}, {r.summary.n_rounds} rounds: {da:.1e} rad, {dt:.1e} mm, points {dp:.1e} mm from ground truth")
    assert da <= 1e-6 and dt <= 1e-5 and dp <= 1e-4


@pytest.mark.parametrize("key", ["r2_tan_robust", "windowed", "wide"])
def test_bundle_adjustment_on_the_device_from_the_result(built, key):
    sc = scene_of(key)
    got = device_default(key)
    obs, v0, p0, m = rr.registered_part(got.views, got.pts, got.registered, got.mapped, *obs_of(sc))
    _, vg, pg, _ = rr.registered_part(sc.views_gt, sc.pts_gt, got.registered, got.mapped, *obs_of(sc))
    out = []
    for views, pts in ((v0, p0), (vg, pg)):
        pa = capi.ProblemArrays(*obs, sc.cam_gt, views, pts, sc.spx, sc.scale, sc.config | 0x500, fixed_mask=0x1FFFF)
        with BundleAdjustment(pa) as ba:
            out.append(ba.performBundleAdjustment())
    dc = abs(out[0].final_cost - out[1].final_cost) / out[1].final_cost
    print(f"{key}: {int(m.sum())} of {sc.n_obs} observations; start rms {got.rms_x:.2f} {got.rms_y:.2f} px; iterations {out[0].iterations} (ground truth {out[1].iterations}); "
          f"final costs {dc:.1e} relative")
    assert dc <= 1e-4
    assert got.rms_x < 10.0 and got.rms_y < 10.0


def test_the_same_call_twice_gives_the_same_bits(built):
    for key in ("windowed", "wide"):
        a, b = device_default(key), device(key)
        for x, y in ((a.views, b.views), (a.pts, b.pts), (a.frame_rows, b.frame_rows), (a.point_rows, b.point_rows)):
            assert x.tobytes() == y.tobytes()
        assert bytes(a.summary) == bytes(b.summary)


def test_two_islands_and_untouched_outputs(built):
    from tests.test_register_cpu import islands
    sc, obs = islands()
    r = registerScene(sc.cam_gt, *obs, 12, 80, sc.config, sc.spx, sc.scale, anchorFrame=2)
    f, p = r.frame_rows, r.point_rows
    assert list(f["status"]) == [0] * 6 + [2] * 6 and sorted(f["round"][:6]) == [0, 1, 1, 1, 1, 1] and np.all(f["round"][6:] == -1)
    assert np.all(p["status"][:40] == 0) and np.all(p["status"][40:] == 2) and np.all(np.isin(p["round"][:40], (0, 1))) and np.all(p["round"][40:] == -1)
    assert (r.summary.n_rounds, r.summary.n_frames_registered, r.summary.n_points_mapped) == (1, 6, 40)
    assert np.all(f["n_shared"][6:] == 0) and np.all(p["n_frames_used"][:40] == 6) and np.all(f["n_used"][6:] > 0)
    for k in range(6, 12):
        assert r.views[k].tobytes() == NAN6
    for k in range(40, 80):
        assert r.pts[k].tobytes() == NAN3
    check_rows(sc, r, obs=tuple(np.asarray(a) for a in obs))
    # the island alone gives the same bits for its frames and points
    m = obs[5] < 6
    alone = registerScene(sc.cam_gt, *(a[m] for a in obs), 6, 40, sc.config, sc.spx, sc.scale, anchorFrame=2)
    assert alone.views.tobytes() == r.views[:6].tobytes() and alone.pts.tobytes() == r.pts[:40].tobytes()
    assert alone.frame_rows.tobytes() == f[:6].tobytes() and alone.point_rows.tobytes() == p[:40].tobytes()
    # without a chosen anchor: the frame with the most used groups, the lowest index on ties
    r = registerScene(sc.cam_gt, *obs, 12, 80, sc.config, sc.spx, sc.scale)
    assert r.summary.anchor_frame == int(np.argmax(r.frame_rows["n_used"])) and r.summary.n_frames_registered == 6


def test_a_frame_without_observations_and_max_rounds(built):
    key = "p_window"
    sc = scene_of(key)
    keep = sc.fr != 7
    obs = tuple(a[keep] for a in obs_of(sc))
    r = device(key, obs=obs, anchorFrame=2)
    spec, ms = CASES[key]
    ref = rr.register("gpu", sc.cam_gt, *obs, spec.n_frames, spec.n_points, sc.config, sc.spx, sc.scale, min_shared=ms, anchor_frame=2)
    assert_same_bookkeeping(r, ref)
    assert r.frame_rows["status"][7] == 1 and r.views[7].tobytes() == NAN6
    zero = r.frame_rows[7:8].copy(); zero["status"] = 0; zero["round"] = 0
    assert not zero.view(np.uint8).any()
    full, one = device(key, anchorFrame=2), device(key, anchorFrame=2, maxRounds=1)
    ref1 = rr.register("gpu", sc.cam_gt, *obs_of(sc), spec.n_frames, spec.n_points, sc.config, sc.spx, sc.scale, min_shared=ms, anchor_frame=2, max_rounds=1)
    assert_same_bookkeeping(one, ref1)
    assert full.summary.n_rounds > 1 and one.summary.n_rounds == 1
    assert np.array_equal(one.registered, (full.frame_rows["round"] >= 0) & (full.frame_rows["round"] <= 1))
    assert np.array_equal(one.mapped, (full.point_rows["round"] >= 0) & (full.point_rows["round"] <= 1))


def test_handle_method_forwards_to_the_free_function(built):
    key = "r2_tan_robust"
    sc = scene_of(key)
    res = device_default(key)
    pa = capi.ProblemArrays.from_scene(sc)   # the perturbed start values, the camera free: the solve moves the camera block
    cam0 = pa.cam.copy()
    with BundleAdjustment(pa) as ba:
        ba.performBundleAdjustment()
        a = ba.registerScene()
        cam, views_after = ba.problem.cam.copy(), ba.problem.views.copy()
        ba.download_parameters()
        assert ba.problem.views.tobytes() == views_after.tobytes() and ba.problem.cam.tobytes() == cam.tobytes()   # the handle is left as it is
    assert cam.tobytes() != cam0.tobytes() and cam.tobytes() != np.asarray(sc.cam_gt, np.float64).tobytes()
    spec, ms = CASES[key]
    free = registerScene(cam, *obs_of(sc), spec.n_frames, spec.n_points, sc.config, sc.spx, sc.scale)
    assert a.frame_rows.tobytes() == free.frame_rows.tobytes() and a.point_rows.tobytes() == free.point_rows.tobytes()
    assert a.views.tobytes() == free.views.tobytes() and a.pts.tobytes() == free.pts.tobytes() and bytes(a.summary) == bytes(free.summary)
    assert a.views.tobytes() != res.views.tobytes()   # (not the result at the ground-truth camera)
    with pytest.raises(Exception, match="negative"):
        registerScene(cam, *obs_of(sc), -1, spec.n_points, sc.config, sc.spx, sc.scale)


def test_the_batch_calls_keep_their_bits(built):
    """resectFrames and intersectPoints share their kernels' source with the masked instantiations: their results on r2_tan_robust
    are those recorded before the masks existed (tests/golden/register_control.npz, written on an MI355X)"""
    want = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "register_control.npz"))
    got = rr.control_calls()
    for name in ("resect_views", "resect_rows", "intersect_pts", "intersect_rows"):
        assert got[name].tobytes() == want[name].tobytes(), name
