"""The host side of the cross-view depth feature, no GPU needed: the numpy restatements of
tests/depth_views_reference.py against the existing ones, the fixture's preconditions, the emit-rule invariants, the ctypes layouts
and the argument checks the wrappers make before anything reaches the device."""
import ctypes as C
import os

import numpy as np
import pytest

from lifcal_amd import _capi as capi, depth, results
from lifcal_amd.bundle_adjustment import LifcalError
from tests import depth_reference as dr
from tests import depth_views_reference as vr

SPX = 0.011


def camera_for(base, config):
    cam = np.zeros(17); cam[:5] = base[:5]
    nr = config & 3
    cam[5:5 + nr] = base[5:5 + nr]
    if config & 4:
        cam[5 + nr:7 + nr] = base[7:9]
    return cam


def round_trip_points(cam, n, seed):
    rs = np.random.default_rng(seed)
    v = rs.uniform(2.0, 20.0, n)
    b = cam[1] + v * cam[2]
    Z = cam[0] * b / (b - cam[0])
    rad = 5.6 * np.sqrt(rs.uniform(0, 1, n)); ang = rs.uniform(0, 2 * np.pi, n)
    return np.stack([rad * np.cos(ang) / cam[1] * Z, rad * np.sin(ang) / cam[1] * Z, Z], -1)


@pytest.mark.parametrize("config", [0x0, 0x1, 0x2, 0x4, 0x5, 0x6])
def test_forward_exact_agrees_with_forward_ref_and_inverts_back_project(config):
    cam = camera_for(dr.CAM_ROUND_TRIP, config)
    p = round_trip_points(cam, 4000, 300 + config)
    x, y, v, ok = vr.forward_exact(p, cam, config, SPX)
    xr, yr, vr_ = dr.forward_ref(p, cam, config, SPX)
    assert np.all(ok)
    for got, want in ((x, xr), (y, yr), (v, vr_)):
        assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-15
    back = dr.back_project_cam(x, y, v, cam, config, SPX)
    assert np.max(np.abs(back - p) / p[:, 2:3]) < 1e-13          # the bar of section 7i.2
    # and the other way round: forward_exact o back_project_cam returns (x, y, v)
    rs = np.random.default_rng(config)
    xv = rs.uniform(0, 1023, 4000); yv = rs.uniform(0, 1023, 4000); vv = rs.uniform(2.0, 20.0, 4000)
    x2, y2, v2, ok2 = vr.forward_exact(dr.back_project_cam(xv, yv, vv, cam, config, SPX), cam, config, SPX)
    assert np.all(ok2)
    assert np.max(np.abs(x2 - xv)) < 1e-9 and np.max(np.abs(y2 - yv)) < 1e-9 and np.max(np.abs(v2 - vv) / vv) < 1e-12


def test_forward_exact_marks_invalid_points():
    cam = camera_for(dr.CAM_ROUND_TRIP, 0x6)
    p = np.array([[1.0, 2.0, 400.0], [1.0, 2.0, 0.0], [1.0, 2.0, -5.0], [1.0, 2.0, cam[0]], [np.nan, 2.0, 400.0], [1.0, np.inf, 400.0],
                  [1.0, 2.0, 20.0],      # Z < fL: b < 0, v < 0
                  [1.0, 2.0, 1.0e6]])    # b -> fL < bL0: v < 0
    x, y, v, ok = vr.forward_exact(p, cam, 0x6, SPX)
    assert ok.tolist() == [True] + [False] * 7
    assert np.all(np.isnan(x[1:])) and np.all(np.isnan(y[1:])) and np.all(np.isnan(v[1:])) and np.isfinite(v[0])


def test_fixture_preconditions():
    """each class on at least 20 pixels of some pair, and no compared pixel within 1e-9 of the threshold: the class comparison of
    the GPU tests then needs no exclusions (the GPU's frame tables differ from numpy's in the last bit of a sine)"""
    raw, cam, views = vr.views_fixture()
    assert raw.shape == (5, 61, 83) and raw.dtype == np.uint16
    assert (raw.shape[2] % 4, (raw.shape[1] * raw.shape[2]) % 2, (raw.shape[1] * raw.shape[2] * 2) % 8) == (3, 1, 6)
    step = np.diff(views, axis=0)
    assert np.all(np.abs(step[:, :3]) <= 0.05) and np.all(np.abs(step[:, 3:]) < 10.0) and np.max(np.abs(step[:, :3])) >= 0.01
    for span in (1, 2):
        support, conflict, pair, per_pair, nearest = vr.fixture_check(span)
        print(f"span {span}: nearest |e| to the threshold {nearest / vr.STEP:.3f} steps")
        assert nearest > 1e-9
        best = {k: 0 for k in ("no data", "consistent", "occluded", "violation")}
        for (s, t), (cls, e, tpix, v_obs) in per_pair.items():
            counts = {"no data": int(np.sum(cls == vr.NO_DATA)), "consistent": int(np.sum(cls == vr.CONSISTENT)),
                      "occluded": int(np.sum(cls == vr.OCCLUDED)), "violation": int(np.sum(cls == vr.VIOLATION))}
            if all(c >= 20 for c in counts.values()):
                best = counts
            if abs(t - s) == 1:
                print(f"  {s} -> {t}: {counts}")
        assert all(c >= 20 for c in best.values()), best          # one pair shows all four
        assert np.sum(~np.isfinite(dr.decode_direct(raw))) >= 5 * 12   # invalid sources exist
        assert support.max() <= 2 * span and conflict.max() <= 2 * span
        assert np.all(support[~np.isfinite(dr.decode_direct(raw))] == 0)
        # slots whose target lies outside the batch are zero
        for s in range(5):
            for j in range(2 * span):
                if not 0 <= vr.slot_target(s, j, span) < 5:
                    assert all(pair[s, j][k] == 0 for k in vr.PAIR_DTYPE.names)


def test_true_camera_is_sharper_than_a_wrong_B():
    raw, cam, views = vr.views_fixture()
    _, _, pair, _, _ = vr.fixture_check(1)
    _, _, off = vr.check_ref(raw, vr.fixture_camera(1.01), vr.CONFIG_FIX, vr.SPX_FIX, np.arange(5), views, 1, vr.TOL_STEPS_FIX * vr.STEP)
    a, b = vr.rms_steps(pair), vr.rms_steps(off)
    print("rms in steps, true camera:", a[np.isfinite(a)], "B x 1.01:", b[np.isfinite(b)])
    assert np.all(b[np.isfinite(a)] > a[np.isfinite(a)])


@pytest.mark.parametrize("span", [1, 2])
def test_emit_rule_invariants(span):
    raw, cam, views = vr.views_fixture()
    support, conflict, pair, per_pair, _ = vr.fixture_check(span)
    H, W = raw.shape[1:]
    for kw in (dict(), dict(min_support=0, max_conflict=255)):
        xyz, merged, src = vr.fuse_ref(raw, cam, vr.CONFIG_FIX, vr.SPX_FIX, np.arange(5), views, span, vr.TOL_STEPS_FIX * vr.STEP, **kw)
        assert len(src) > 100 and np.all(np.diff(src.astype(np.int64)) > 0)          # ascending, no pixel twice
        s_of, pix = (src // (H * W)).astype(np.int64), (src % (H * W)).astype(np.int64)
        for s, p in zip(s_of[::7], pix[::7]):
            for t in range(max(0, s - span), s):
                assert per_pair[(s, t)][0][p] != vr.CONSISTENT                        # it would have deferred
        assert np.array_equal(merged, 1 + support.reshape(5, -1)[s_of, pix])
        assert np.all(np.isfinite(xyz))
        # a fused point lies between the depths that went into it: within the tolerance of the pixel's own world point
        own = np.concatenate([vr.to_world(vr.frame_table(views[s]), dr.back_project_cam(pix[s_of == s] % W, pix[s_of == s] // W,
                              dr.decode_direct(raw[s]).reshape(-1)[pix[s_of == s]], cam, vr.CONFIG_FIX, vr.SPX_FIX)) for s in range(5) if np.any(s_of == s)])
        assert np.max(np.linalg.norm(xyz - own, axis=1)) < 1.0                        # mm, at a scene depth of 500
    valid = int(np.isfinite(dr.decode_direct(raw)).sum())
    assert len(src) < valid                                                           # some valid pixels defer


def test_layouts_match_the_header():
    assert C.sizeof(capi.DepthPairStats) == 56 == capi.DEPTH_PAIR_DTYPE.itemsize == vr.PAIR_DTYPE.itemsize
    assert [f[0] for f in capi.DepthPairStats._fields_] == list(capi.DEPTH_PAIR_DTYPE.names) == list(vr.PAIR_DTYPE.names)
    assert C.sizeof(capi.DepthForward) == 8 + 3 * 8 + 8 + 3 * 8 + 8
    assert C.sizeof(capi.DepthViewsArgs) == 6 * 4 + 2 * 8 + 8 + 3 * 8 + 8 and capi.DepthViewsArgs.tol_iv.offset == 40
    assert C.sizeof(capi.DepthFusionArgs) == 6 * 4 + 2 * 8 + 8 + 2 * 4 + 8 + 3 * 8 + 8 + 8 and capi.DepthFusionArgs.capacity.offset == 56
    for name in ("lifcal_depth_project_points", "lifcal_depth_check_maps", "lifcal_depth_fuse_maps"):
        assert name in capi.DEPTH_PROTOTYPES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lifcal_depth.h")).read()
    for name in ("lifcal_depth_forward", "lifcal_depth_pair_stats", "lifcal_depth_views", "lifcal_depth_fusion"):
        assert f"}} {name};" in header


def test_wrappers_refuse_bad_arguments_before_the_device():
    cam = camera_for(dr.CAM_ROUND_TRIP, 0x6)

    def code(fn, *a, **k):
        with pytest.raises(LifcalError) as e:
            fn(*a, **k)
        return getattr(e.value, "code", None)
    views = np.zeros((3, 6))
    good = dict(who="checkMaps", count=3, frame=[0, 1, 2], views=views, span=1, tol_steps=4.0)
    fr, vw = depth.views_arguments(**good)
    assert fr.dtype == np.uint32 and vw.shape == (18,)
    for change in (dict(frame=None), dict(views=None), dict(count=0), dict(count=-2), dict(span=0), dict(span=128), dict(span=1.5), dict(tol_steps=-1.0),
                   dict(tol_steps=float("nan")), dict(views=np.zeros(7)), dict(frame=[0, 1]), dict(frame=[0, -1, 2])):
        assert code(depth.views_arguments, **{**good, **change}) == -1, change
    with pytest.raises(LifcalError, match="17 entries"):
        depth.projectPoints(np.zeros((2, 3)), cam[:5], 0x6, SPX)
    with pytest.raises(LifcalError, match=r"\(n, 3\)"):
        depth.projectPoints(np.zeros((2, 2)), cam, 0x6, SPX)
    with pytest.raises(LifcalError, match="go together"):
        depth.projectPoints(np.zeros((2, 3)), cam, 0x6, SPX, fr=[0, 0])
    with pytest.raises(LifcalError, match="differs in length"):
        depth.projectPoints(np.zeros((2, 3)), cam, 0x6, SPX, fr=[0], views=np.zeros(6))
    with pytest.raises(LifcalError, match=r"\(n, 3\)"):
        results.storeFusedCloudPly("/nonexistent", np.zeros((4, 2)))


def test_fused_cloud_writer(built, tmp_path):
    """host code of the library: the fused cloud in the format of objectCoordinates.ply"""
    rs = np.random.default_rng(3)
    xyz = rs.uniform(-50, 600, (37, 3)).astype(np.float32)
    results.storeFusedCloudPly(str(tmp_path), xyz)
    results.storeObjectCoordinates(str(tmp_path), xyz.astype(np.float64))
    a = (tmp_path / "fusedCloud.ply").read_text(); b = (tmp_path / "objectCoordinates.ply").read_text()
    assert a == b and f"element vertex {len(xyz)}" in a
