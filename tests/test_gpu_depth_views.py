"""Cross-view check and fusion of depth maps on the GPU (include/lifcal_depth.h (d)-(f)): the forward model,
checkMaps and fuseMaps against the restatements of tests/depth_views_reference.py on its five-map fixture, the shapes at which the
kernels take another path, reproducibility, the sensitivity to a wrong B, and the error codes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lifcal_amd import _capi as capi, depth
from lifcal_amd.bundle_adjustment import LifcalError
from tests import depth_reference as dr
from tests import depth_views_reference as vr

pytestmark = pytest.mark.gpu
SPX = vr.SPX_FIX
CFG = vr.CONFIG_FIX
TOL = vr.TOL_STEPS_FIX
FRAMES = np.arange(vr.N_FIX)


def camera_for(base, config):
    cam = np.zeros(17); cam[:5] = base[:5]
    nr = config & 3
    cam[5:5 + nr] = base[5:5 + nr]
    if config & 4:
        cam[5 + nr:7 + nr] = base[7:9]
    return cam


@pytest.fixture(scope="module")
def maps(built):
    """the fixture on the device, as maps 0 .. 4 of a handle of five"""
    raw, cam, views = vr.views_fixture()
    with depth.DepthMaps(vr.W_FIX, vr.H_FIX, vr.N_FIX) as dm:
        dm.setMaps(raw)
        yield dm, raw, cam, views


def assert_pairs_equal(got, want, sums=True):
    for k in ("n_valid", "n_compared", "n_consistent", "n_occluded", "n_violation"):
        assert np.array_equal(got[k], want[k]), k
    if sums:
        for k in ("sum_e", "sum_e2"):
            print(f"{k}: largest relative deviation {np.max(np.abs(got[k] - want[k]) / np.where(want[k] != 0, np.abs(want[k]), 1.0)):.3e}")
            assert np.all(np.abs(got[k] - want[k]) <= 1e-12 * np.abs(want[k])), k


# ------------------------------------------------------------------------------------------------ 1. the forward model
@pytest.mark.parametrize("config", [0x0, 0x1, 0x2, 0x4, 0x5, 0x6])
def test_project_points_is_bit_identical_to_forward_exact(built, config):
    rs = np.random.default_rng(500 + config)
    n = 5000
    cam = camera_for(dr.CAM_ROUND_TRIP, config)
    v = rs.uniform(2.0, 20.0, n)
    b = cam[1] + v * cam[2]
    Z = cam[0] * b / (b - cam[0])
    rad = 5.6 * np.sqrt(rs.uniform(0, 1, n)); ang = rs.uniform(0, 2 * np.pi, n)
    p = np.stack([rad * np.cos(ang) / cam[1] * Z, rad * np.sin(ang) / cam[1] * Z, Z], -1)
    p_clean = p.copy()
    p[3, 2] = 0.0; p[4, 2] = -7.0; p[5, 2] = cam[0]; p[6, 0] = np.nan; p[7, 1] = np.inf; p[8, 2] = np.nan   # Z <= 0, Z == fL, not finite
    p[9, 2] = 20.0; p[10, 2] = 1.0e6                                                                       # v <= 0 on either side of the pole
    x, y, vv, ok = vr.forward_exact(p, cam, config, SPX)
    assert int((~ok).sum()) == 8
    r = depth.projectPoints(p, cam, config, SPX)
    assert np.array_equal(r.x, x, equal_nan=True) and np.array_equal(r.y, y, equal_nan=True) and np.array_equal(r.vdepth, vv, equal_nan=True)
    assert r.n_invalid == 8 and np.all(np.isnan(r.x[~ok])) and np.all(np.isnan(r.y[~ok])) and np.all(np.isnan(r.vdepth[~ok]))
    # world points through poses: p_c from the restatement of frame_eval, at the bar test_points_are_bit_identical... uses for p_w
    views = np.column_stack([rs.uniform(-0.3, 0.3, (4, 3)), rs.uniform(-200, 200, (4, 3))])
    fr = rs.integers(0, 4, n)
    p_w = np.concatenate([vr.to_world(vr.frame_table(views[f]), p_clean[i:i + 1]) for i, f in enumerate(fr)])
    p_w[6] = np.nan
    p_c = np.concatenate([vr.to_camera(vr.frame_table(views[f]), p_w[i:i + 1]) for i, f in enumerate(fr)])
    xw, yw, vw, okw = vr.forward_exact(p_c, cam, config, SPX)
    g = depth.projectPoints(p_w, cam, config, SPX, fr=fr, views=views)
    assert g.n_invalid == int((~okw).sum()) == 1 and np.isnan(g.x[6]) and np.isnan(g.vdepth[6])
    for got, want in ((g.x, xw), (g.y, yw), (g.vdepth, vw)):
        assert np.max(np.abs(got[okw] - want[okw])) <= 1e-12 * np.max(np.abs(want[okw]))
    # backProjectPoints(projectPoints(p)) returns p at the bar of section 7i.2
    ok_c = np.ones(n, bool); ok_c[3:11] = False
    back = depth.backProjectPoints(r.x[ok_c], r.y[ok_c], r.vdepth[ok_c], cam, config, SPX).p_c
    err = np.max(np.abs(back - p[ok_c]) / p[ok_c, 2:3])
    print(f"config {config:#x}: GPU forward + back round trip {err:.3e} of Z")
    assert err < 1e-13


# ------------------------------------------------------------------------------------------------ 2. checkMaps on the fixture
@pytest.mark.parametrize("span", [1, 2])
def test_check_maps_matches_the_restatement(maps, span):
    dm, raw, cam, views = maps
    support, conflict, pair, per_pair, nearest = vr.fixture_check(span)
    assert nearest > 1e-9                                        # tests/test_depth_views_cpu.py holds the other preconditions
    r = dm.checkMaps(cam, CFG, SPX, FRAMES, views, span=span, tol_steps=TOL)
    assert r.support.dtype == np.uint8 and np.array_equal(r.support, support) and np.array_equal(r.conflict, conflict)
    assert_pairs_equal(r.pair, pair)
    for s in range(vr.N_FIX):
        for j in range(2 * span):
            assert r.target(s, j) == vr.slot_target(s, j, span)
            if not 0 <= r.target(s, j) < vr.N_FIX:
                assert r.pair[s, j].tobytes() == bytes(56)       # slots outside the batch are zero
    print(f"span {span}: rms in steps {np.round(r.rms_steps(), 3).tolist()}, device time {r.seconds * 1e3:.3f} ms")
    assert np.allclose(r.rms_steps(), vr.rms_steps(pair), rtol=1e-9, equal_nan=True)
    only = dm.checkMaps(cam, CFG, SPX, FRAMES, views, span=span, tol_steps=TOL, want_support=False)
    assert only.support is None and np.array_equal(only.conflict, conflict) and only.pair.tobytes() == r.pair.tobytes()


def test_check_maps_with_a_y_pixel_pitch_of_its_own(built):
    """The fixture's scene rendered and cross-checked with spy = 1.25 spx: the maps are consistent with that pitch and with no other,
    so the restatement at spy = spx (what a pitch read from the x slot computes) classes a tenth of the pixels differently, where
    the comparison is exact"""
    spy = 1.25 * SPX
    cam, views = vr.fixture_camera(), vr.fixture_views()
    raw = vr.render_maps(cam, views, vr.W_FIX, vr.H_FIX, spy=spy)
    support, conflict, pair, _, nearest = vr.check_ref(raw, cam, CFG, SPX, FRAMES, views, 1, TOL * vr.STEP, details=True, spy=spy)
    iso_support, _, iso_pair = vr.check_ref(raw, cam, CFG, SPX, FRAMES, views, 1, TOL * vr.STEP)
    n_con, n_cmp, n_iso = int(pair["n_consistent"].sum()), int(pair["n_compared"].sum()), int(iso_pair["n_consistent"].sum())
    print(f"spy = 1.25 spx: {n_con} of {n_cmp} compared pixels consistent (at spy = spx: {n_iso}), nearest |e| to the threshold {nearest:.2e}")
    assert nearest > 1e-9 and n_con > 0.8 * n_cmp and n_iso < n_con - 1000 and np.mean(iso_support != support) > 0.05
    with depth.DepthMaps(vr.W_FIX, vr.H_FIX, vr.N_FIX) as dm:
        dm.setMaps(raw)
        r = dm.checkMaps(cam, CFG, SPX, FRAMES, views, span=1, tol_steps=TOL, spy=spy)
    assert np.array_equal(r.support, support) and np.array_equal(r.conflict, conflict)
    assert_pairs_equal(r.pair, pair)
    assert np.allclose(r.rms_steps(), vr.rms_steps(pair), rtol=1e-9, equal_nan=True)


# ------------------------------------------------------------------------------------------------ 3. shapes
def test_check_maps_shapes(built):
    raw, cam, views = vr.views_fixture()
    tol = TOL * vr.STEP
    with depth.DepthMaps(vr.W_FIX, vr.H_FIX, 7) as dm:
        # the batch at first = 1 (its first pixel is not 8-byte aligned), map 3 of it never set
        dm.setMaps(raw[:2], first=1); dm.setMaps(raw[3:], first=4)
        holed = np.array(raw); holed[2] = 0
        for span in (1, 2):
            want = vr.check_ref(holed, cam, CFG, SPX, FRAMES, views, span, tol)
            r = dm.checkMaps(cam, CFG, SPX, FRAMES, views, span=span, tol_steps=TOL, first=1, count=5)
            assert np.array_equal(r.support, want[0]) and np.array_equal(r.conflict, want[1])
            assert_pairs_equal(r.pair, want[2])
            assert np.all(r.pair[2]["n_valid"] == 0) and np.all(r.support[2] == 0)          # nothing from the unset map
            for s in range(5):
                for j in range(2 * span):
                    if r.target(s, j) == 2:
                        assert r.pair[s, j]["n_compared"] == 0 and r.pair[s, j]["n_valid"] > 0   # all no data against it
        dm.setMaps(raw[2], first=3)
        # count = 1: no target
        one = dm.checkMaps(cam, CFG, SPX, [0], views, span=1, tol_steps=TOL, first=2, count=1)
        assert not one.support.any() and not one.conflict.any() and one.pair.tobytes() == bytes(2 * 56)
        # span > count
        want = vr.check_ref(raw[:3], cam, CFG, SPX, FRAMES[:3], views, 7, tol)
        r = dm.checkMaps(cam, CFG, SPX, FRAMES[:3], views, span=7, tol_steps=TOL, first=1, count=3)
        assert r.pair.shape == (3, 14) and np.array_equal(r.support, want[0]) and np.array_equal(r.conflict, want[1])
        assert_pairs_equal(r.pair, want[2])
        # tol = 0: only e == 0 is consistent, and the sign of e decides between the other two.  The last bit of a sine reaches e
        # at about 1e-16, so a restatement whose smallest |e| is above 1e-13 has the signs of the GPU
        want = vr.check_ref(raw, cam, CFG, SPX, FRAMES, views, 1, 0.0, details=True)
        assert want[4] > 1e-13
        r = dm.checkMaps(cam, CFG, SPX, FRAMES, views, span=1, tol_steps=0.0, first=1, count=5)
        assert np.array_equal(r.support, want[0]) and np.array_equal(r.conflict, want[1])
        assert_pairs_equal(r.pair, want[2], sums=False)
        assert np.all(r.pair["n_consistent"] == 0) and np.all(r.pair["sum_e2"] == 0.0)
    # a 4 x 3 map: one workgroup, most of it idle
    small, cam_s, views_s = vr.small_fixture()
    want = vr.check_ref(small, cam_s, CFG, SPX, FRAMES[:3], views_s, 1, tol, details=True)
    assert want[4] > 1e-9 and want[2]["n_consistent"].sum() >= 12 and want[2]["n_occluded"].sum() > 0 and want[2]["n_violation"].sum() > 0
    with depth.DepthMaps(4, 3, 3) as dm:
        dm.setMaps(small)
        r = dm.checkMaps(cam_s, CFG, SPX, FRAMES[:3], views_s, span=1, tol_steps=TOL)
        assert np.array_equal(r.support, want[0]) and np.array_equal(r.conflict, want[1])
        assert_pairs_equal(r.pair, want[2])
        xyz, merged, src = vr.fuse_ref(small, cam_s, CFG, SPX, FRAMES[:3], views_s, 1, tol)
        f = dm.fuseMaps(cam_s, CFG, SPX, FRAMES[:3], views_s, out_double=True)
        assert f.n_points == len(src) > 0 and np.array_equal(f.src, src) and np.array_equal(f.n_merged, merged)
        assert np.max(np.abs(f.xyz - xyz)) <= 1e-12 * 520.0


def test_device_pointer_outputs_equal_host_outputs(built):
    """outputs written into torch tensors on the device.  Of two HIP runtimes in one process only the first to start sees the GPU
    (DESIGN.md section 7i.4), and this process has the library's running already, so the check runs in a fresh one."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "depth_views_device_pointers.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "device pointers ok" in p.stdout


# ------------------------------------------------------------------------------------------------ 4. reproducibility
def test_two_calls_give_the_same_bits(maps):
    dm, raw, cam, views = maps
    a = dm.checkMaps(cam, CFG, SPX, FRAMES, views, span=2, tol_steps=TOL)
    b = dm.checkMaps(cam, CFG, SPX, FRAMES, views, span=2, tol_steps=TOL)
    assert a.pair.tobytes() == b.pair.tobytes() and np.array_equal(a.support, b.support) and np.array_equal(a.conflict, b.conflict)
    f = dm.fuseMaps(cam, CFG, SPX, FRAMES, views, span=2, tol_steps=TOL, out_double=True)
    g = dm.fuseMaps(cam, CFG, SPX, FRAMES, views, span=2, tol_steps=TOL, out_double=True)
    assert f.n_points == g.n_points > 0 and f.xyz.tobytes() == g.xyz.tobytes() and f.src.tobytes() == g.src.tobytes() and f.n_merged.tobytes() == g.n_merged.tobytes()


# ------------------------------------------------------------------------------------------------ 5. fuseMaps
@pytest.mark.parametrize("span", [1, 2])
def test_fuse_maps_matches_the_restatement(maps, span):
    dm, raw, cam, views = maps
    xyz, merged, src = vr.fuse_ref(raw, cam, CFG, SPX, FRAMES, views, span, TOL * vr.STEP)
    scene_depth = 520.0
    d = dm.fuseMaps(cam, CFG, SPX, FRAMES, views, span=span, tol_steps=TOL, out_double=True)
    assert d.n_points == len(src) > 1000 and d.xyz.dtype == np.float64 and d.xyz.shape == (len(src), 3)
    assert np.array_equal(d.src, src) and np.array_equal(d.n_merged, merged) and d.src.dtype == np.uint32 and d.n_merged.dtype == np.uint8
    err = np.max(np.abs(d.xyz - xyz))
    print(f"span {span}: {d.n_points} points, merged {np.bincount(d.n_merged).tolist()}, largest deviation {err:.3e} mm, device time {d.seconds * 1e3:.3f} ms")
    assert err <= 1e-12 * scene_depth
    f = dm.fuseMaps(cam, CFG, SPX, FRAMES, views, span=span, tol_steps=TOL)
    assert f.xyz.dtype == np.float32 and f.n_points == d.n_points and np.array_equal(f.src, src)
    assert np.all(np.abs(f.xyz.astype(np.float64) - xyz) <= 0.5 * np.spacing(np.abs(xyz).astype(np.float32)).astype(np.float64) + 1e-12 * scene_depth)
    assert np.array_equal(f.xyz, d.xyz.astype(np.float32))                     # the float output is the rounding of the double one
    # a capacity below n_points keeps the ordered prefix
    cut = dm.fuseMaps(cam, CFG, SPX, FRAMES, views, span=span, tol_steps=TOL, out_double=True, capacity=777)
    assert cut.n_points == d.n_points and len(cut.src) == 777
    assert cut.xyz.tobytes() == d.xyz[:777].tobytes() and np.array_equal(cut.src, src[:777]) and np.array_equal(cut.n_merged, merged[:777])
    zero = dm.fuseMaps(cam, CFG, SPX, FRAMES, views, span=span, tol_steps=TOL, capacity=0)
    assert zero.n_points == d.n_points and len(zero.src) == 0
    # min_support = 0, max_conflict = 255: every valid pixel that does not defer
    xyz0, merged0, src0 = vr.fuse_ref(raw, cam, CFG, SPX, FRAMES, views, span, TOL * vr.STEP, min_support=0, max_conflict=255)
    every = dm.fuseMaps(cam, CFG, SPX, FRAMES, views, span=span, tol_steps=TOL, min_support=0, max_conflict=255, out_double=True)
    valid = int(np.isfinite(dr.decode_direct(raw)).sum())
    assert every.n_points == len(src0) and d.n_points < every.n_points < valid
    assert np.array_equal(every.src, src0) and np.array_equal(every.n_merged, merged0) and np.max(np.abs(every.xyz - xyz0)) <= 1e-12 * scene_depth


# ------------------------------------------------------------------------------------------------ 6. sensitivity
def test_a_wrong_B_shows_on_every_neighbouring_pair(maps):
    """The maps as rendered and the poses held; B x 1.01 against the true camera, RMS of e over the consistent pixels in raw steps.
    Only "larger" is asserted.  Measured on the MI355X: see DESIGN.md section 7q."""
    dm, raw, cam, views = maps
    true = dm.checkMaps(cam, CFG, SPX, FRAMES, views, span=1, tol_steps=TOL).rms_steps()
    off = dm.checkMaps(vr.fixture_camera(1.01), CFG, SPX, FRAMES, views, span=1, tol_steps=TOL).rms_steps()
    for s in range(vr.N_FIX):
        for j in range(2):
            if 0 <= s + (1 if j else -1) < vr.N_FIX:
                print(f"pair {s} -> {s + (1 if j else -1)}: true camera {true[s, j]:.3f} steps, B x 1.01 {off[s, j]:.3f} steps")
                assert off[s, j] > true[s, j]


# ------------------------------------------------------------------------------------------------ 7. error codes
def test_error_codes(maps):
    dm, raw, cam, views = maps
    lib = capi.load_library()
    fr = np.ascontiguousarray(FRAMES, np.uint32); vw = np.ascontiguousarray(views, np.float64).reshape(-1)
    support = np.zeros(raw.shape, np.uint8)

    def camera(config=CFG):
        return depth.depth_camera(cam, config, SPX)

    def views_io(kind, **change):
        io = capi.DepthViewsArgs() if kind == "check" else capi.DepthFusionArgs()
        io.first, io.count, io.span, io.n_frames, io.tol_iv = 0, 5, 1, 5, TOL * vr.STEP
        io.frame, io.views = capi.as_uptr(fr), capi.as_dptr(vw)
        if kind == "check":
            io.support = C.c_void_p(support.ctypes.data)
        for k, val in change.items():
            setattr(io, k, val)
        return io

    for kind, fn in (("check", lib.lifcal_depth_check_maps), ("fuse", lib.lifcal_depth_fuse_maps)):
        dc = camera()
        assert fn(dm._h, C.byref(dc), C.byref(views_io(kind))) == 0
        assert fn(None, C.byref(dc), C.byref(views_io(kind))) == -1
        assert fn(dm._h, None, C.byref(views_io(kind))) == -1
        assert fn(dm._h, C.byref(dc), None) == -1
        bad_cam = camera(); bad_cam.config = 0x3
        assert fn(dm._h, C.byref(bad_cam), C.byref(views_io(kind))) == -1
        for change in (dict(views=None), dict(frame=None), dict(span=0), dict(tol_iv=-1e-9), dict(tol_iv=float("nan")), dict(count=0), dict(count=-1)):
            assert fn(dm._h, C.byref(dc), C.byref(views_io(kind, **change))) == -1, (kind, change)
        for change in (dict(first=1), dict(first=-1), dict(count=6), dict(n_frames=4)):
            assert fn(dm._h, C.byref(dc), C.byref(views_io(kind, **change))) == -4, (kind, change)
        assert b"lifcal_depth_" in lib.lifcal_ba_last_error()
    # the forward model
    p = np.array([[1.0, 2.0, 400.0]]); out = [np.zeros(1) for _ in range(3)]
    frame = np.array([2], np.uint32)

    def forward_io(**change):
        io = capi.DepthForward()
        io.n, io.p = 1, capi.as_dptr(p)
        io.x, io.y, io.vdepth = (capi.as_dptr(o) for o in out)
        for k, val in change.items():
            setattr(io, k, val)
        return io
    dc = camera()
    assert lib.lifcal_depth_project_points(0, C.byref(dc), C.byref(forward_io())) == 0 and np.isfinite(out[2][0])
    assert lib.lifcal_depth_project_points(0, None, C.byref(forward_io())) == -1
    assert lib.lifcal_depth_project_points(0, C.byref(dc), None) == -1
    assert lib.lifcal_depth_project_points(0, C.byref(dc), C.byref(forward_io(p=None))) == -1
    bad_cam = camera(); bad_cam.config = 0x7
    assert lib.lifcal_depth_project_points(0, C.byref(bad_cam), C.byref(forward_io())) == -1
    assert lib.lifcal_depth_project_points(0, C.byref(dc), C.byref(forward_io(fr=capi.as_uptr(frame)))) == -1          # fr without views
    assert lib.lifcal_depth_project_points(0, C.byref(dc), C.byref(forward_io(fr=capi.as_uptr(frame), views=capi.as_dptr(vw), n_frames=2))) == -4
    assert lib.lifcal_depth_project_points(0, C.byref(dc), C.byref(forward_io(fr=capi.as_uptr(frame), views=capi.as_dptr(vw), n_frames=5))) == 0
    # through the wrappers
    def code(fn, *a, **k):
        with pytest.raises(LifcalError) as e:
            fn(*a, **k)
        return e.value.code
    assert code(dm.checkMaps, cam, CFG, SPX, FRAMES, views, first=3) == -1                  # two maps left, five frame indices
    assert code(dm.checkMaps, cam, CFG, SPX, FRAMES, views, first=3, count=5) == -4
    assert code(dm.checkMaps, cam, CFG, SPX, [0, 1, 2, 3, 9], views) == -4
    assert code(dm.fuseMaps, cam, 0x3, SPX, FRAMES, views) == -1
    assert code(dm.fuseMaps, cam, CFG, SPX, FRAMES, views, span=0) == -1
    assert code(depth.projectPoints, p, cam, CFG, SPX, fr=[7], views=views) == -4
    empty = depth.projectPoints(np.zeros((0, 3)), cam, CFG, SPX)
    assert empty.x.shape == (0,) and empty.n_invalid == 0
