"""The depth feature on the GPU (include/lifcal_depth.h): the sampler, projectPointBack for image points with
its Jacobian and covariance, the dense path in both evaluation options, the chain depth PNG -> readDepthData -> start values ->
observations, the object-space comparison at a solver handle, and the error codes.  Everything is compared with the restatements
of tests/depth_reference.py (the reference's operations line by line), not with another GPU path."""
import os
import subprocess
import sys

import numpy as np
import pytest

from lifcal_amd import BundleAdjustment, MicroLensGrid, initPlenopticParameters, _capi as capi, depth, results, scene
from lifcal_amd.bundle_adjustment import LifcalError
from tests import depth_reference as dr
from tests.helpers import S, problem

pytestmark = pytest.mark.gpu
SPX = 0.011
DEFAULT = np.array([35.0, 34.15, 0.40, 511.3, 513.9, 5e-5, -2e-7, 1e-5, -1e-5] + [0.0] * 8)   # the scenes' camera (scene.SceneSpec)


def camera_for(base, config):
    """base = (fL, bL0, B, cx, cy, k1, k2, p1, p2, ...) laid out for `config`"""
    cam = np.zeros(17); cam[:5] = base[:5]
    nr = config & 3
    cam[5:5 + nr] = base[5:5 + nr]
    if config & 4:
        cam[5 + nr:7 + nr] = base[7:9]
    return cam


# ------------------------------------------------------------------------------------------------ (a) sampler
def test_sampler_is_bit_identical_to_the_restatement(built):
    img, x, y = dr.sampler_fixture()
    want, dist = dr.sample_ref(img, x, y)
    classes = dict(direct=int(np.sum(dist == 0)), near=int(np.sum((dist >= 2) & (dist <= 5))), far=int(np.sum(dist > 5)), failed=int(np.sum(dist == -1)))
    print("sampler classes (direct / dist 2..5 / dist > 5 / failed):", classes, "dist 1:", int(np.sum(dist == 1)))
    assert all(c >= 50 for c in classes.values()), classes      # the fixture takes every path
    assert np.sum(dist == 1) == 0 and np.sum(dist == -2) == 0    # a 3 x 3 window holds nine values; every centre is inside
    other = np.zeros_like(img); other[::2] = 40000
    with depth.DepthMaps(img.shape[1], img.shape[0], 3) as dm:
        dm.setMaps(np.stack([other, img]), first=1)
        got, counts = dm.sample(x, y, 2)
        assert np.array_equal(got, want)
        assert (counts.direct, counts.interpolated, counts.failed) == (classes["direct"], classes["near"] + classes["far"], classes["failed"])
        # per-point map indices, and a map that was never set is all invalid
        mi = np.where(np.arange(len(x)) % 2 == 0, 2, 1).astype(np.int32)
        got2, _ = dm.sample(x, y, mi)
        want_other, _ = dr.sample_ref(other, x, y)
        assert np.array_equal(got2, np.where(mi == 2, want, want_other))
        got0, c0 = dm.sample(x[:100], y[:100], 0)
        assert np.all(got0 == -1.0) and c0.failed == 100
        # outside the image: -1, counted as failed (the reference reads out of bounds there)
        xo = np.array([-1.6, 10.0, img.shape[1] - 0.4, 5.0, np.nan, 1e300]); yo = np.array([5.0, -1.6, 5.0, img.shape[0] - 0.4, 3.0, 3.0])
        wo, do = dr.sample_ref(img, xo[:4], yo[:4])
        go, co = dm.sample(xo, yo, 2)
        assert np.all(do == -2) and np.all(go == -1.0) and co.failed == 6 and co.direct == co.interpolated == 0


# ------------------------------------------------------------------------------------------------ (b) points
@pytest.mark.parametrize("config", [0x0, 0x1, 0x2, 0x4, 0x5, 0x6])
def test_points_are_bit_identical_and_invert_the_forward_model(built, config):
    rs = np.random.default_rng(100 + config)
    n = 5000
    cam = camera_for(DEFAULT, config)
    x = rs.uniform(0, 1023, n); y = rs.uniform(0, 1023, n); v = rs.uniform(2.2, 20.0, n)
    v[::97] = -1.0; v[5] = 0.0; v[6] = np.nan                   # failed samples
    bad = ~(v > 0)
    views = np.column_stack([rs.uniform(-0.3, 0.3, (4, 3)), rs.uniform(-200, 200, (4, 3))])
    fr = rs.integers(0, 4, n)
    r = depth.backProjectPoints(x, y, v, cam, config, SPX, fr=fr, views=views)
    want = dr.back_project_cam(x[~bad], y[~bad], v[~bad], cam, config, SPX)
    assert np.array_equal(r.p_c[~bad], want)                    # fp64, the reference's order, no contraction
    assert np.all(np.isnan(r.p_c[bad])) and np.all(np.isnan(r.p_w[bad])) and r.n_invalid == int(bad.sum())
    R = np.stack([dr.euler_xyz(a[:3]) for a in views])
    pw = np.einsum("nji,nj->ni", R[fr[~bad]], want - views[fr[~bad], 3:])
    assert np.max(np.abs(r.p_w[~bad] - pw)) <= 1e-12 * np.max(np.abs(pw))
    # the round trip, at the camera and the bar of tests/test_depth_cpu.py
    cam_rt = camera_for(dr.CAM_ROUND_TRIP, config)
    vv = rs.uniform(2.0, 20.0, n)
    b = cam_rt[1] + vv * cam_rt[2]
    Z = cam_rt[0] * b / (b - cam_rt[0])
    rad = 5.6 * np.sqrt(rs.uniform(0, 1, n)); ang = rs.uniform(0, 2 * np.pi, n)
    p = np.stack([rad * np.cos(ang) / cam_rt[1] * Z, rad * np.sin(ang) / cam_rt[1] * Z, Z], -1)
    xv, yv, v2 = dr.forward_ref(p, cam_rt, config, SPX)
    got = depth.backProjectPoints(xv, yv, v2, cam_rt, config, SPX).p_c
    err = np.max(np.abs(got - p) / p[:, 2:3])
    print(f"config {config:#x}: GPU round trip {err:.3e} of Z")
    assert err < 1e-13


@pytest.fixture(scope="module")
def cfg2_covariance(built):
    """G of a real lifcal_ba_covariance call on cfg2, at its solution"""
    sc = scene.make_scene(scene.baseline_spec("cfg2"))
    pa = problem(sc)
    with BundleAdjustment(pa) as ba:
        ba.performBundleAdjustment()
        cov = ba.covariance()
    return sc, pa, cov


def test_jacobian_against_the_complex_step(built, cfg2_covariance):
    sc, pa, cov = cfg2_covariance
    rs = np.random.default_rng(7)
    n = 2000
    for config in (0x6, 0x1, 0x4, 0x0):
        cam = camera_for(DEFAULT, config)
        x = rs.uniform(0, 1023, n); y = rs.uniform(0, 1023, n); v = rs.uniform(2.3, 12.0, n)
        r = depth.backProjectPoints(x, y, v, cam, config, SPX, want_jacobian=True)
        J, dv = dr.jacobian_complex_step(x, y, v, cam, config, SPX)
        row = np.linalg.norm(J, axis=2, keepdims=True)
        err = np.max(np.abs(r.jac - J) / row)
        err_v = np.max(np.abs(r.dpc_dv - dv) / np.linalg.norm(dv, axis=1, keepdims=True))
        print(f"config {config:#x}: jacobian {err:.2e} of the row norm, d/dv {err_v:.2e}")
        assert err < 1e-9 and err_v < 1e-9
        nc = 5 + (config & 3) + (2 if config & 4 else 0)
        assert np.all(r.jac[:, :, nc:] == 0.0)                   # absent slots
    # covariance of the points through the camera block of the solved cfg2 problem
    G = cov.camera
    x = sc.img_x[:n]; y = sc.img_y[:n]; v = sc.img_vd[:n]
    r = depth.backProjectPoints(x, y, v, pa.cam, sc.config, sc.spx, cam_cov=G, sigma_v=0.01)
    full = np.einsum("nij,jk,nlk->nil", r.jac, G, r.jac) + 0.01 ** 2 * np.einsum("ni,nl->nil", r.dpc_dv, r.dpc_dv)
    iu = np.triu_indices(3)
    want = full[:, iu[0], iu[1]]
    sd = np.sqrt(np.abs(np.einsum("nii->ni", full)))
    scale = (sd[:, iu[0]] * sd[:, iu[1]]) + 1e-300
    assert np.max(np.abs(r.cov_pc - want) / scale) < 1e-9
    assert np.all(r.cov_pc[:, [0, 3, 5]] >= 0)


def test_depth_is_estimable_orders_constrained_and_free_scenes(built):
    """without distance constraints B and bL0 are not determined on their own: metric depth moves along the null
    direction, and a propagated variance means nothing there.  Only the ordering is asserted; measured: 1.09 for the free scene
    (null_rank 1: a unit step along the null direction moves the points by more than their distance), 0 for the constrained one
    (null_rank 0).  Both values are in DESIGN.md 7i."""
    vals = {}
    for name, spec in [("free", S(6, 40, None, 0x506, 117)), ("constrained", S(6, 40, None, 0x506, 117, n_constraints=3))]:
        sc = scene.make_scene(spec)
        pa = problem(sc)
        with BundleAdjustment(pa) as ba:
            ba.performBundleAdjustment()
            cov = ba.covariance()
        r = depth.backProjectPoints(sc.img_x, sc.img_y, sc.img_vd, pa.cam, sc.config, sc.spx, want_jacobian=True)
        vals[name] = depth.depth_is_estimable(r.jac, cov.camera_null, r.p_c)
        print(f"depth_is_estimable [{name}]: {vals[name]:.3e} (null_rank {cov.null_rank})")
    assert vals["constrained"] < vals["free"]


# ------------------------------------------------------------------------------------------------ (c) dense
def dense_fixture(W=250, H=37, count=3, seed=5):
    """maps whose width is no multiple of four (a lane's four pixels straddle lines and maps) with every kind of invalid value"""
    rs = np.random.default_rng(seed)
    v = rs.uniform(2.3, 12.0, (count, H, W))
    raw = dr.encode_vdepth(v)
    raw[rs.random(raw.shape) < 0.2] = 0
    raw[0, 3:6, 7:19] = 65535
    raw[1, 10:14, 100:120] = 20000
    raw[-1, -1, -5:] = 0
    return raw


def dense_reference(raw, cam, config, dtype=np.float64, spy=None):
    count, H, W = raw.shape
    v = dr.decode_direct(raw)
    ok = np.isfinite(v)
    rows, cols = np.mgrid[0:H, 0:W]
    cols = np.broadcast_to(cols, raw.shape); rows = np.broadcast_to(rows, raw.shape)
    out = np.full(raw.shape + (3,), np.nan, dtype)
    out[ok] = dr.back_project_cam(cols[ok], rows[ok], v[ok], cam, config, SPX, spy=spy, dtype=dtype)
    return out, v, ok


@pytest.mark.parametrize("config", [0x6, 0x0, 0x1, 0x4])
def test_dense_fp64_is_bit_identical(built, config):
    raw = dense_fixture()
    cam = camera_for(DEFAULT, config)
    want, v, ok = dense_reference(raw, cam, config)
    with depth.DepthMaps(raw.shape[2], raw.shape[1], 4) as dm:
        for first in (0, 1):                                    # first = 1: the batch does not start on an 8-byte boundary
            dm.setMaps(raw, first=first)
            r = dm.backProjectMaps(cam, config, SPX, first=first, count=3, out_double=True, want_z=True)
            assert r.xyz.dtype == np.float64 and np.array_equal(r.xyz, want, equal_nan=True)
            assert np.array_equal(r.z, want[..., 2], equal_nan=True)
            assert r.n_invalid == int((~ok).sum())
            f = dm.backProjectMaps(cam, config, SPX, first=first, count=3, want_z=True)
            assert f.xyz.dtype == np.float32 and np.array_equal(f.xyz, want.astype(np.float32), equal_nan=True)
            assert np.array_equal(f.z, want[..., 2].astype(np.float32), equal_nan=True) and f.n_invalid == r.n_invalid
        one = dm.backProjectMaps(cam, config, SPX, first=2, count=1, out_double=True)   # a sub-range
        assert np.array_equal(one.xyz[0], want[1], equal_nan=True)


def test_dense_sigma_z_matches_the_closed_form(built, cfg2_covariance):
    sc, pa, cov = cfg2_covariance
    raw = dense_fixture(seed=6)
    cam, config, sigma_v = pa.cam, sc.config, 0.02
    G = cov.camera
    v = dr.decode_direct(raw)
    fL, bL0, B = cam[0], cam[1], cam[2]
    b = bL0 + v * B; d = b - fL
    g = np.stack([b * b / (d * d), -fL * fL / (d * d), -v * fL * fL / (d * d)], -1)
    gv = -B * fL * fL / (d * d)
    s2 = np.einsum("...i,ij,...j->...", g, G[:3, :3], g) + gv * gv * sigma_v ** 2
    want = np.sqrt(np.maximum(s2, 0.0))
    with depth.DepthMaps(raw.shape[2], raw.shape[1], 3) as dm:
        dm.setMaps(raw)
        r = dm.backProjectMaps(cam, config, sc.spx, cam_cov=G, sigma_v=sigma_v, want_xyz=False, want_z=True, want_sigma_z=True)
        rd = dm.backProjectMaps(cam, config, sc.spx, cam_cov=G, sigma_v=sigma_v, want_xyz=False, want_sigma_z=True, out_double=True)
    assert r.xyz is None and r.sigma_z.dtype == np.float32
    ok = np.isfinite(v)
    assert np.all(np.isnan(r.sigma_z[~ok])) and np.all(np.isnan(r.z[~ok]))
    w32 = want[ok].astype(np.float32)
    assert np.all(np.abs(r.sigma_z[ok] - w32) <= np.spacing(w32))          # within one ulp of float32
    assert np.allclose(rd.sigma_z[ok], want[ok], rtol=1e-9, atol=0)
    assert np.array_equal(r.z[ok], (fL * b[ok] / d[ok]).astype(np.float32))  # z needs no undistortion


def test_dense_fp32_option_against_the_float32_restatement(built):
    """The fp32 option is measured against back_project_ref evaluated in float32 on the same pixels, not against the fp64 kernel.
    The bar is four times the largest deviation of that float32 restatement from the fp64 restatement (packed FMA and a different
    operation order are allowed for by the factor).  Deviations are the largest component error relative to Z of the pixel.
    Measured on the MI355X (scene camera, v in 2.3 .. 12, where fL / (b - fL) reaches 500): float32 restatement against fp64
    4.69e-5, fp32 kernel against the float32 restatement 5.09e-5 (bar 1.87e-4), fp32 kernel against fp64 4.69e-5; the same
    figures with and without distortion, so they are the rounding of b = bL0 + v B in float32, not the undistortion."""
    raw = dense_fixture(W=256, H=64, count=2, seed=8)
    for config in (0x6, 0x0):
        cam = camera_for(DEFAULT, config)
        ref64, v, ok = dense_reference(raw, cam, config)
        ref32, _, _ = dense_reference(raw, cam, config, dtype=np.float32)
        Z = ref64[ok][:, 2:3]
        dev_ref = np.max(np.abs(ref32[ok].astype(np.float64) - ref64[ok]) / Z)
        with depth.DepthMaps(raw.shape[2], raw.shape[1], 2) as dm:
            dm.setMaps(raw)
            r = dm.backProjectMaps(cam, config, SPX, eval=1, want_z=True)
        assert r.xyz.dtype == np.float32 and r.n_invalid == int((~ok).sum()) and np.all(np.isnan(r.xyz[~ok]))
        dev = np.max(np.abs(r.xyz[ok].astype(np.float64) - ref32[ok].astype(np.float64)) / Z)
        dev64 = np.max(np.abs(r.xyz[ok].astype(np.float64) - ref64[ok]) / Z)
        print(f"config {config:#x}: float32 restatement vs fp64 {dev_ref:.3e}; fp32 kernel vs float32 restatement {dev:.3e}, vs fp64 {dev64:.3e}")
        assert dev <= 4.0 * dev_ref
        assert np.array_equal(r.z[ok], r.xyz[ok][:, 2])


def test_a_y_pixel_pitch_of_its_own(built):
    """spy = 1.25 spx through backProjectPoints (with its Jacobian), projectPoints and backProjectMaps in both evaluation options, each
    at the bar its test above holds at spy = spx; the restatement at spy = spx, which a pitch read from the x slot computes, lies
    far outside every one of them"""
    from tests import depth_views_reference as vr
    spy = 1.25 * SPX
    rs = np.random.default_rng(41)
    n = 3000
    for config in (0x6, 0x5, 0x0):
        cam = camera_for(DEFAULT, config)
        x = rs.uniform(0, 1023, n); y = rs.uniform(0, 1023 / 1.25, n); v = rs.uniform(2.3, 12.0, n)
        r = depth.backProjectPoints(x, y, v, cam, config, SPX, spy=spy, want_jacobian=True)
        want, iso = dr.back_project_cam(x, y, v, cam, config, SPX, spy=spy), dr.back_project_cam(x, y, v, cam, config, SPX)
        assert np.array_equal(r.p_c, want)
        moved = np.abs(want - iso) / want[:, 2:3]
        assert np.median(moved[:, 1]) > 1e-3                            # the y pitch moves Y of every point (and, through r^2, X where there is distortion)
        J, dv = dr.jacobian_complex_step(x, y, v, cam, config, SPX, spy=spy)
        J_iso, _ = dr.jacobian_complex_step(x, y, v, cam, config, SPX)
        row = np.linalg.norm(J, axis=2, keepdims=True)
        err, err_v = np.max(np.abs(r.jac - J) / row), np.max(np.abs(r.dpc_dv - dv) / np.linalg.norm(dv, axis=1, keepdims=True))
        wrong = np.median(np.max(np.abs(J_iso - J) / row, axis=(1, 2)))
        print(f"config {config:#x}: Y moves by {np.median(moved[:, 1]):.2e} of Z; jacobian {err:.2e} of the row norm, d/dv {err_v:.2e}; the one at spy = spx {wrong:.2e}")
        assert err < 1e-9 and err_v < 1e-9 and wrong > 1e-3
        # the forward model and the round trip
        cam_rt = camera_for(dr.CAM_ROUND_TRIP, config)
        vv = rs.uniform(2.0, 20.0, n)
        b = cam_rt[1] + vv * cam_rt[2]
        Z = cam_rt[0] * b / (b - cam_rt[0])
        rad = 5.6 * np.sqrt(rs.uniform(0, 1, n)); ang = rs.uniform(0, 2 * np.pi, n)
        p = np.stack([rad * np.cos(ang) / cam_rt[1] * Z, rad * np.sin(ang) / cam_rt[1] * Z, Z], -1)
        xe, ye, ve, ok = vr.forward_exact(p, cam_rt, config, SPX, spy=spy)
        _, ye_iso, _, _ = vr.forward_exact(p, cam_rt, config, SPX)
        f = depth.projectPoints(p, cam_rt, config, SPX, spy=spy)
        assert np.all(ok) and f.n_invalid == 0
        assert np.array_equal(f.x, xe) and np.array_equal(f.y, ye) and np.array_equal(f.vdepth, ve)
        assert np.median(np.abs(ye - ye_iso)) > 1.0                     # pixels
        xv, yv, v2 = dr.forward_ref(p, cam_rt, config, SPX, spy=spy)
        back = depth.backProjectPoints(xv, yv, v2, cam_rt, config, SPX, spy=spy).p_c
        rt = np.max(np.abs(back - p) / p[:, 2:3])
        print(f"config {config:#x}: GPU round trip {rt:.3e} of Z")
        assert rt < 1e-13
    # dense, fp64 bit for bit and the fp32 option at four times the float32 restatement's own deviation
    raw = dense_fixture(W=250, H=37, count=2, seed=12)
    for config in (0x6, 0x0):
        cam = camera_for(DEFAULT, config)
        ref64, v, ok = dense_reference(raw, cam, config, spy=spy)
        ref32, _, _ = dense_reference(raw, cam, config, dtype=np.float32, spy=spy)
        iso64, _, _ = dense_reference(raw, cam, config)
        Z = ref64[ok][:, 2:3]
        assert np.median(np.abs(ref64[ok] - iso64[ok])[:, 1:2] / Z) > 1e-4
        dev_ref = np.max(np.abs(ref32[ok].astype(np.float64) - ref64[ok]) / Z)
        with depth.DepthMaps(raw.shape[2], raw.shape[1], 2) as dm:
            dm.setMaps(raw)
            d = dm.backProjectMaps(cam, config, SPX, spy=spy, out_double=True, want_z=True)
            r32 = dm.backProjectMaps(cam, config, SPX, spy=spy, eval=1)
        assert np.array_equal(d.xyz, ref64, equal_nan=True) and np.array_equal(d.z, ref64[..., 2], equal_nan=True) and d.n_invalid == int((~ok).sum())
        dev = np.max(np.abs(r32.xyz[ok].astype(np.float64) - ref32[ok].astype(np.float64)) / Z)
        wrong = np.max(np.abs(iso64[ok] - ref64[ok]) / Z)
        print(f"config {config:#x}: dense fp32 kernel vs float32 restatement {dev:.3e} (bar {4.0 * dev_ref:.3e}); the restatement at spy = spx {wrong:.3e}")
        assert dev <= 4.0 * dev_ref and wrong > 100.0 * dev_ref


def test_dense_world_coordinates(built):
    raw = dense_fixture(seed=9)
    config = 0x6
    cam = camera_for(DEFAULT, config)
    want, v, ok = dense_reference(raw, cam, config)
    rs = np.random.default_rng(2)
    views = np.column_stack([rs.uniform(-0.4, 0.4, (2, 3)), rs.uniform(-300, 300, (2, 3))])
    frames = np.array([1, 0, 1])
    R = np.stack([dr.euler_xyz(a[:3]) for a in views])
    pw = np.einsum("mji,mhwj->mhwi", R[frames], want - views[frames, 3:][:, None, None, :])
    with depth.DepthMaps(raw.shape[2], raw.shape[1], 3) as dm:
        dm.setMaps(raw)
        r = dm.backProjectMaps(cam, config, SPX, out_double=True, frames=frames, views=views, want_z=True)
        assert np.max(np.abs(r.xyz[ok] - pw[ok])) <= 1e-12 * np.max(np.abs(pw[ok])) and np.all(np.isnan(r.xyz[~ok]))
        assert np.array_equal(r.z, want[..., 2], equal_nan=True)  # z stays the camera-frame depth
        f = dm.backProjectMaps(cam, config, SPX, frames=frames, views=views)
        assert np.array_equal(f.xyz, r.xyz.astype(np.float32), equal_nan=True)
        e = dm.backProjectMaps(cam, config, SPX, eval=1, frames=frames, views=views)
        assert np.max(np.abs(e.xyz[ok] - pw[ok])) <= 1e-3 * np.max(np.abs(pw[ok]))


def test_device_pointers_through_torch_tensors(built):
    """maps handed over as a torch tensor on the device, outputs written into torch tensors.  The torch wheel carries a HIP runtime
    of its own, and of two runtimes in one process only the first to start sees the GPU: a process that shares tensors with the
    library lets torch initialise first.  This process has the library's runtime running already, so the check runs in a fresh one."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "depth_device_pointers.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "device pointers ok" in p.stdout


# ------------------------------------------------------------------------------------------------ chain
def test_depth_images_through_the_chain(built, tmp_path):
    """depth PNGs rendered from a scene -> readDepthData -> initPlenopticParameters and projectPointsToRawImage, which accept the
    sampled depths as they accept the scene's.  The coding quantises 1/v to 1/65535, so |1/v - 1/v_true| <= 0.5/65535."""
    sp = S(6, 80, None, 0x506, 9301)
    sc = scene.make_scene(sp)
    W, H = sp.raw_width // sp.scale, sp.raw_height // sp.scale
    F = sp.n_frames
    px = (sc.img_x + 0.5).astype(np.int64); py = (sc.img_y + 0.5).astype(np.int64)
    key = (sc.img_fr.astype(np.int64) * H + py) * W + px
    _, first_idx, cnt = np.unique(key, return_index=True, return_counts=True)
    alone = np.zeros(len(key), bool); alone[first_idx[cnt == 1]] = True       # two points on one pixel cannot both keep their depth
    assert alone.mean() > 0.95
    folder = tmp_path / "depth"; os.makedirs(folder)
    frame_ids = [3, 1, 6, 2, 5, 4]                                            # frame k of the scene has id frame_ids[k]
    for k in range(F):
        img = np.zeros((H, W), np.uint16)
        m = sc.img_fr == k
        img[py[m], px[m]] = dr.encode_vdepth(sc.img_vd[m])
        dr.write_png16(str(folder / f"depth_{frame_ids[k]:04d}.png"), img, filters=(1,))
    (folder / "notes.txt").write_text("not an image")
    pts = [np.column_stack([sc.img_x[sc.img_fr == k], sc.img_y[sc.img_fr == k]]) for k in range(F)]
    per_frame, counts = depth.readDepthData(str(folder), frame_ids, pts, (W, H))
    vd = np.concatenate(per_frame)
    assert len(vd) == len(sc.img_vd) and counts.direct == len(vd) and counts.failed == 0
    assert np.max(np.abs(1.0 / vd[alone] - 1.0 / sc.img_vd[alone])) <= 0.5 / 65535 + 4 * np.finfo(float).eps
    with pytest.raises(LifcalError, match="wrong depth image size"):
        depth.readDepthData(str(folder), frame_ids, pts, (W, H + 1))
    with pytest.raises(LifcalError, match="no depth image"):
        depth.readDepthData(str(folder), [7] + frame_ids[1:], pts, (W, H))
    # downstream: the start values and the observations
    M = np.tile(np.eye(4), (F, 1, 1))
    views = sc.views0.reshape(-1, 6)
    M[:, :3, :3] = scene.euler_xyz(views[:, :3]); M[:, :3, 3] = views[:, 3:]
    a = initPlenopticParameters(vd, sc.img_fr, sc.img_pt, M, sc.pts0.reshape(-1, 3), sc.cam0[0])
    b = initPlenopticParameters(sc.img_vd, sc.img_fr, sc.img_pt, M, sc.pts0.reshape(-1, 3), sc.cam0[0])
    assert a.rank == b.rank == 2 and a.n_used == b.n_used and np.isfinite(a.B_init) and np.isfinite(a.bL0_init)
    g = MicroLensGrid(sp.raw_width, sp.raw_height, sp.lens_diameter, sp.lens_base_y, sp.grid_rotation, sp.grid_offset)
    oa = g.projectPointsToRawImage(sc.img_x, sc.img_y, vd, sp.scale, fr=sc.img_fr, pt=sc.img_pt)
    ob = g.projectPointsToRawImage(sc.img_x, sc.img_y, sc.img_vd, sp.scale, fr=sc.img_fr, pt=sc.img_pt)
    print(f"chain: B_init {a.B_init:.6f} / {b.B_init:.6f}, bL0_init {a.bL0_init:.6f} / {b.bL0_init:.6f}, observations {len(oa.u)} / {len(ob.u)}")
    assert len(oa.u) > 0 and set(np.unique(oa.src)) <= set(range(len(vd)))


# ------------------------------------------------------------------------------------------------ (d) object space
def _object_space_numpy(sc, cam, views, pts):
    R = scene.euler_xyz(views.reshape(-1, 6)[:, :3]); t = views.reshape(-1, 6)[:, 3:]
    ref = np.einsum("nij,nj->ni", R[sc.img_fr], pts.reshape(-1, 3)[sc.img_pt]) + t[sc.img_fr]
    proj = dr.back_project_cam(sc.img_x, sc.img_y, sc.img_vd, cam, sc.config, sc.spx)
    use = sc.img_vd >= 2.0
    e = (proj - ref)[use]
    return ref, proj, np.sqrt(np.mean(e * e, axis=0)), np.max(np.abs(e), axis=0), np.sqrt(np.mean((e[:, 2] / ref[use, 2]) ** 2)), int(use.sum())


def test_object_space_statistics(built, tmp_path):
    """make_scene generates its virtual-image points without distortion (scene.py:346-347) and projectPointBack undistorts, so the
    scene is distortion-free (0x500); distance constraints fix the B / bL0 direction, which the images alone do not determine."""
    sc = scene.make_scene(S(6, 60, None, 0x500, 9401, n_constraints=4))
    with BundleAdjustment(problem(sc, initial=False)) as ba:                   # ground truth
        st, ref, proj = ba.objectSpaceStats(sc.img_x, sc.img_y, sc.img_vd, sc.img_fr, sc.img_pt)
    assert st.n_used == len(sc.img_x) and st.n_skipped == 0
    err = np.max(np.abs(proj - ref) / np.linalg.norm(ref, axis=1, keepdims=True))
    print(f"object space at the ground truth: {err:.3e}")
    assert err < 1e-9
    pa = problem(sc)
    with BundleAdjustment(pa) as ba:
        st0, _, _ = ba.objectSpaceStats(sc.img_x, sc.img_y, sc.img_vd, sc.img_fr, sc.img_pt)
        ba.performBundleAdjustment()
        vd = sc.img_vd.copy(); vd[:3] = [1.5, -1.0, 0.0]                      # skipped: v < 2 (two of them failed samples)
        st1, ref, proj = ba.objectSpaceStats(sc.img_x, sc.img_y, vd, sc.img_fr, sc.img_pt)
        st2, _, _ = ba.objectSpaceStats(sc.img_x, sc.img_y, vd, sc.img_fr, sc.img_pt)
    assert st1.n_skipped == 3 and st1.n_used == len(vd) - 3 and np.all(np.isnan(proj[1:3])) and np.all(np.isfinite(proj[0]))
    sc_cut = type("Cut", (), dict(img_x=sc.img_x, img_y=sc.img_y, img_vd=vd, img_fr=sc.img_fr, img_pt=sc.img_pt, config=sc.config, spx=sc.spx))
    with np.errstate(all="ignore"):
        ref_n, proj_n, rms, mx, rel, used = _object_space_numpy(sc_cut, pa.cam, pa.views, pa.pts)
    assert used == st1.n_used
    assert np.allclose(ref, ref_n, rtol=1e-12, atol=1e-9) and np.array_equal(proj[3:], proj_n[3:])
    assert np.allclose(list(st1.rms), rms, rtol=1e-9) and np.allclose(list(st1.max_abs), mx, rtol=1e-9) and st1.rms_rel_depth == pytest.approx(rel, rel=1e-9)
    assert (list(st1.rms), list(st1.max_abs), st1.rms_rel_depth) == (list(st2.rms), list(st2.max_abs), st2.rms_rel_depth)   # reproducible
    print(f"relative depth error: {st0.rms_rel_depth:.3e} at the start values, {st1.rms_rel_depth:.3e} after the solve")
    assert st1.rms_rel_depth < st0.rms_rel_depth
    # the two folders of storeResults, written from ref_c / proj_c
    ids = [11, 12, 13, 14, 15, 16]
    results.storeCameraCoordinates(str(tmp_path), "refCameraCoordinates", ids, sc.img_fr, ref)
    results.storeCameraCoordinates(str(tmp_path), "projectedCameraCoordinates", ids, sc.img_fr, proj)
    for folder, arr in (("refCameraCoordinates", ref), ("projectedCameraCoordinates", proj)):
        for f, fid in enumerate(ids):
            lines = (tmp_path / folder / f"cameraCoordinates_{fid:04d}.ply").read_text().splitlines()
            want = arr[sc.img_fr == f]
            assert lines[2] == f"element vertex {len(want)}" and len(lines) == 8 + len(want)
            back = np.array([[float(t) for t in ln.split()[:3]] for ln in lines[8:]])
            assert np.allclose(back, want, rtol=5.0001e-6, atol=0, equal_nan=True)   # six significant digits


# ------------------------------------------------------------------------------------------------ errors
def test_error_codes(built):
    lib = capi.load_library()
    raw = dense_fixture()
    cam = camera_for(DEFAULT, 0x6)
    with depth.DepthMaps(raw.shape[2], raw.shape[1], 3) as dm:
        def code(fn, *a, **k):
            with pytest.raises(LifcalError) as e:
                fn(*a, **k)
            return e.value.code
        assert code(dm.setMaps, raw, first=1) == -4                            # three maps from index 1 of three
        assert code(dm.setMaps, raw[:, :-1, :]) == -1                          # size mismatch
        assert code(dm.setMaps, raw[:, :, :-2]) == -1
        dm.setMaps(raw)
        assert code(dm.sample, [1.0, 2.0], [1.0, 2.0], [0, 3]) == -4           # map index out of range
        assert code(dm.sample, [1.0], [1.0], -1) == -4
        assert code(dm.backProjectMaps, cam, 0x6, SPX, first=2, count=2) == -4
        assert code(dm.backProjectMaps, cam, 0x6, SPX, want_sigma_z=True) == -1   # sigma_z needs the covariance
        assert code(dm.backProjectMaps, cam, 0x6, SPX, eval=2) == -1
        assert code(dm.backProjectMaps, cam, 0x6, SPX, frames=[0, 1, 2], views=np.zeros(12)) == -4
        assert code(dm.backProjectMaps, cam, 0x3, SPX) == -1                   # three radial coefficients
        assert lib.lifcal_depth_set_maps(dm._h, 0, 1, None, 0) == -1
        assert lib.lifcal_depth_sample(dm._h, 1, None, None, None, None, None) == -1
        assert lib.lifcal_depth_back_project_maps(dm._h, None, None) == -1
        empty, c = dm.sample([], [], 0)
        assert len(empty) == 0 and c.direct == c.failed == 0
        z = dm.backProjectMaps(cam, 0x6, SPX, first=0, count=0)
        assert z.xyz.shape == (0, raw.shape[1], raw.shape[2], 3) and z.n_invalid == 0
    assert code(depth.backProjectPoints, [1.0], [1.0], [3.0], cam, 0x6, SPX, fr=[2], views=np.zeros(12)) == -4
    assert code(depth.backProjectPoints, [1.0], [1.0], [3.0], cam, 0x3, SPX) == -1
    r = depth.backProjectPoints([], [], [], cam, 0x6, SPX)
    assert r.p_c.shape == (0, 3) and r.n_invalid == 0
    sc = scene.make_scene(S(4, 12, None, 0x500, 9501))
    with BundleAdjustment(problem(sc)) as ba:
        assert code(ba.objectSpaceStats, sc.img_x[:2], sc.img_y[:2], sc.img_vd[:2], [0, 99], sc.img_pt[:2]) == -4
        assert code(ba.objectSpaceStats, sc.img_x[:2], sc.img_y[:2], sc.img_vd[:2], sc.img_fr[:2], [0, 10 ** 6]) == -4
        st, ref, proj = ba.objectSpaceStats([], [], [], [], [])
        assert st.n_used == 0 and st.n_skipped == 0 and ref.shape == (0, 3)
