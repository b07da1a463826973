"""The host side of the depth feature, no GPU needed: the PNG container reader, the four writers for the rest
of the reference's storeResults (src/CameraCalibration.cpp:1131-1287), the numpy restatement of projectPointBack against its
closed-form inverse, and the C ABI tables of include/lifcal_depth.h."""
import ctypes as C
import os
import re
import struct
import zlib

import numpy as np
import pytest

from lifcal_amd import _capi as capi, depth, results
from lifcal_amd.bundle_adjustment import LifcalError
from tests import depth_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = dr.CAM_ROUND_TRIP
SPX = 0.011


# ------------------------------------------------------------------------------------------------ PNG
write_png16 = dr.write_png16


def test_png_reader_round_trips_16_bit_grayscale(tmp_path):
    rs = np.random.default_rng(5)
    img = rs.integers(0, 65536, (37, 53), dtype=np.uint16)
    img[0, 0], img[-1, -1], img[3, 4] = 0, 65535, 256
    for name, filters in [("none", (0,)), ("sub", (1,)), ("up", (2,)), ("avg", (3,)), ("paeth", (4,)), ("mixed", (4, 1, 0, 3, 2))]:
        p = str(tmp_path / f"{name}.png")
        write_png16(p, img, filters)
        got = depth.read_png16(p)
        assert got.dtype == np.uint16 and got.shape == img.shape and np.array_equal(got, img), name


def test_png_reader_rejects_other_kinds(tmp_path):
    img = np.zeros((4, 4), np.uint16)
    for name, kw, word in [("eight", dict(bit_depth=8), "16-bit"), ("rgb", dict(color_type=2), "16-bit"), ("adam7", dict(interlace=1), "interlaced")]:
        p = str(tmp_path / f"{name}.png")
        write_png16(p, img, **kw)
        with pytest.raises(LifcalError, match=word):
            depth.read_png16(p)
    p = str(tmp_path / "text.png")
    open(p, "wb").write(b"not a png at all")
    with pytest.raises(LifcalError, match="not a PNG"):
        depth.read_png16(p)


# ------------------------------------------------------------------------------------------------ writers
def _g(v):
    return "%g" % v


PTS = np.array([[1.5, -2.25, 1000.123456789], [1e-7, 123456789.0, -0.000123456789], [0.0, 1 / 3, -2 / 3], [100000.0, 1000000.0, 999999.5]])


def test_object_coordinates_ply(tmp_path, built):
    results.storeObjectCoordinates(str(tmp_path), PTS)
    text = (tmp_path / "objectCoordinates.ply").read_text()
    head = "ply\nformat ascii 1.0\nelement vertex 4\nproperty float x\nproperty float y\nproperty float z\nproperty uchar intensity\nend_header\n"
    assert text == head + "".join(f"{_g(p[0])} {_g(p[1])} {_g(p[2])} 0\n" for p in PTS)
    back = np.array([[float(t) for t in line.split()[:3]] for line in text[len(head):].splitlines()])
    assert np.allclose(back, PTS, rtol=5e-6, atol=0)          # six significant digits
    assert "1e-07 1.23457e+08 -0.000123457 0" in text           # std::ofstream << double is %g


def test_object_coordinates_with_colmap_ids(tmp_path, built):
    ids = [7, 100003, 12, 5]
    results.storeObjectCoordinatesWithCOLMAPIDs(str(tmp_path), ids, PTS)
    text = (tmp_path / "objectCoordinatesWithCOLMAPIDs.txt").read_text()
    assert text == "# COLMAP_ID X Y Z\n" + "".join(f"{i} {_g(p[0])} {_g(p[1])} {_g(p[2])}\n" for i, p in zip(ids, PTS))
    with pytest.raises(LifcalError):
        results.storeObjectCoordinatesWithCOLMAPIDs(str(tmp_path), ids[:2], PTS)


def test_camera_orientations_ply(tmp_path, built):
    """the frustum in float as the reference builds it (:1170-1180), moved to the world by the inverse pose; six digits are printed,
    so the numbers are compared at 1e-5 relative (plus 1e-5 of the frustum size, where a component cancels)"""
    views = np.array([[0.1, -0.2, 0.3, 10.0, -20.5, 1 / 3], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [-1.2, 0.7, 2.9, 1e-3, 100.0, -7.25]])
    W, H = 1024, 768
    results.storeCameraOrientationsPly(str(tmp_path), views, (W, H), CAM, SPX)
    lines = (tmp_path / "cameraOrientations.ply").read_text().splitlines()
    head = ["ply", "format ascii 1.0", "element vertex 15", "property float x", "property float y", "property float z", "property uchar red",
            "property uchar green", "property uchar blue", "element face 12", "property list uchar int vertex_index", "end_header"]
    assert lines[:12] == head and len(lines) == 12 + 15 + 12
    f32 = np.float32
    cx, cy, f, fL, w, h = f32(CAM[3]), f32(CAM[4]), f32(CAM[0] / SPX), f32(CAM[0] * 3), f32(W), f32(H)
    corners = [(0.0, 0.0, 0.0), ((0 - cx) / f * fL, (0 - cy) / f * fL, fL), ((0 - cx) / f * fL, (h - 1 - cy) / f * fL, fL),
               ((w - 1 - cx) / f * fL, (h - 1 - cy) / f * fL, fL), ((w - 1 - cx) / f * fL, (0 - cy) / f * fL, fL)]
    assert all(isinstance(c, f32) for c in corners[3])
    k = 12
    for v in views:
        M = np.eye(4); M[:3, :3] = dr.euler_xyz(v[:3]); M[:3, 3] = v[3:]
        Mi = np.linalg.inv(M)
        for c in corners:
            want = (Mi @ np.array([float(c[0]), float(c[1]), float(c[2]), 1.0]))[:3]
            tok = lines[k].split(); k += 1
            assert tok[3:] == ["0", "0", "255"]
            assert np.allclose([float(t) for t in tok[:3]], want, rtol=1e-5, atol=1e-5 * float(fL))
    faces = [ln.split() for ln in lines[27:]]
    assert faces[:4] == [["3", "0", "1", "2"], ["3", "0", "2", "3"], ["3", "0", "3", "4"], ["3", "0", "4", "1"]]
    assert faces[8:] == [["3", "10", "11", "12"], ["3", "10", "12", "13"], ["3", "10", "13", "14"], ["3", "10", "14", "11"]]


def test_camera_coordinates_folders(tmp_path, built):
    fr = np.array([0, 0, 1, 2, 2, 2])
    xyz = np.arange(18, dtype=np.float64).reshape(6, 3) * 1.2345678 - 3.0
    xyz[4] = np.nan                                             # a failed sample stays a NaN line
    results.storeCameraCoordinates(str(tmp_path), "projectedCameraCoordinates", [3, 12, 10007], fr, xyz)
    d = tmp_path / "projectedCameraCoordinates"
    assert sorted(os.listdir(d)) == ["cameraCoordinates_0003.ply", "cameraCoordinates_0012.ply", "cameraCoordinates_10007.ply"]
    text = (d / "cameraCoordinates_10007.ply").read_text().splitlines()
    assert text[2] == "element vertex 3" and text[7] == "end_header"
    assert text[8] == " ".join(_g(v) for v in xyz[3]) + " 0"
    assert text[9].split()[3] == "0" and all("nan" in t for t in text[9].split()[:3])
    assert (d / "cameraCoordinates_0012.ply").read_text().splitlines()[8] == " ".join(_g(v) for v in xyz[2]) + " 0"


# ------------------------------------------------------------------------------------------------ the restatement against its inverse
def _random_camera_points(n, seed):
    """v in [2, 20], MLA-plane radius up to 5.6 mm"""
    rs = np.random.default_rng(seed)
    v = rs.uniform(2.0, 20.0, n)
    b = CAM[1] + v * CAM[2]
    Z = CAM[0] * b / (b - CAM[0])
    rad = 5.6 * np.sqrt(rs.uniform(0.0, 1.0, n)); ang = rs.uniform(0.0, 2 * np.pi, n)
    return np.stack([rad * np.cos(ang) / CAM[1] * Z, rad * np.sin(ang) / CAM[1] * Z, Z], -1)


@pytest.mark.parametrize("config", [0x0, 0x1, 0x2, 0x4, 0x5, 0x6])
def test_back_projection_inverts_the_forward_model(config):
    """back_project_ref(forward_ref(p)) = p on 200 000 points, v in [2, 20], MLA-plane radius up to 5.6 mm, the default distortion
    k = (5e-5, -2e-7), p = (1e-5, -1e-5), camera depth_reference.CAM_ROUND_TRIP (why not the default camera: see there).
    Measured for the restatement alone: 5.4e-15 of Z with the reference's ten sweeps (the same with five: what is left is the
    rounding of b amplified by fL / (b - fL) <= 27; 1.7e-11 with three).  The bar is 1e-13."""
    cam = np.zeros(17); cam[:5] = CAM[:5]
    nr = config & 3
    cam[5:5 + nr] = CAM[5:5 + nr]
    if config & 4:
        cam[5 + nr:7 + nr] = CAM[7:9]
    p = _random_camera_points(200_000, 17)
    x, y, v = dr.forward_ref(p, cam, config, SPX)
    got = dr.back_project_cam(x, y, v, cam, config, SPX)
    err = np.max(np.abs(got - p) / p[:, 2:3])
    print(f"config {config:#x}: round trip {err:.3e} of Z")
    assert err < 1e-13


def test_ten_sweeps_have_not_converged_at_twenty_times_the_distortion():
    """Measured: 7.5e-14 of Z with ten sweeps at 20 x the default distortion, 5.4e-15 with twenty: the accuracy of the undistortion
    is that of the reference's fixed ten sweeps, which have not converged there.  Asserted at 1e-10 only."""
    cam = CAM.copy(); cam[5:9] *= 20.0
    p = _random_camera_points(200_000, 18)
    x, y, v = dr.forward_ref(p, cam, 0x6, SPX)
    e10 = np.max(np.abs(dr.back_project_cam(x, y, v, cam, 0x6, SPX) - p) / p[:, 2:3])
    e20 = np.max(np.abs(dr.back_project_cam(x, y, v, cam, 0x6, SPX, sweeps=20) - p) / p[:, 2:3])
    print(f"20 x distortion: {e10:.3e} with ten sweeps, {e20:.3e} with twenty")
    assert e10 < 1e-10 and e20 < 1e-13 and e20 < e10


def test_complex_step_matches_a_central_difference():
    rs = np.random.default_rng(3)
    x = rs.uniform(0, 1023, 50); y = rs.uniform(0, 1023, 50); v = rs.uniform(2.2, 12.0, 50)
    J, dv = dr.jacobian_complex_step(x, y, v, CAM, 0x6, SPX)
    for s, h in [(0, 1e-6), (2, 1e-7), (3, 1e-4), (5, 1e-9)]:
        cp, cm = CAM.copy(), CAM.copy(); cp[s] += h; cm[s] -= h
        fd = (dr.back_project_cam(x, y, v, cp, 0x6, SPX) - dr.back_project_cam(x, y, v, cm, 0x6, SPX)) / (2 * h)
        assert np.allclose(J[:, :, s], fd, rtol=1e-4, atol=1e-6 * np.max(np.abs(fd)))
    assert np.all(J[:, :, 9:] == 0.0)
    fd = (dr.back_project_cam(x, y, v + 1e-6, CAM, 0x6, SPX) - dr.back_project_cam(x, y, v - 1e-6, CAM, 0x6, SPX)) / 2e-6
    assert np.allclose(dv, fd, rtol=1e-5)


def test_sampler_restatement_on_a_hand_made_map():
    img = np.zeros((12, 16), np.uint16)
    img[2, 3] = dr.encode_vdepth(4.0)
    v, d = dr.sample_ref(img, [3.2, 2.51, -3.0], [1.6, 2.4, 2.0])
    iv = 1.0 - float(img[2, 3]) / 65535.0
    assert v[0] == 1.0 / iv == v[1] and d[0] == 0 and v[2] == -1.0 and d[2] == -2
    v, d = dr.sample_ref(img, [9.0], [9.0])                     # one valid value in the whole map: every window fails
    assert v[0] == -1.0 and d[0] == -1
    img[5:9, 5:9] = dr.encode_vdepth(3.0)                       # 16 values: dist 3 around (9, 9) sees 3 x 3 = 9 of them, dist 4 all 16
    v, d = dr.sample_ref(img, [9.0], [9.0])
    iv3 = 1.0 - float(img[5, 5]) / 65535.0
    total = 0.0
    for _ in range(16):
        total += iv3
    assert d[0] == 4 and v[0] == 16.0 / total


# ------------------------------------------------------------------------------------------------ C ABI tables
def test_depth_symbols_and_struct_sizes(built):
    hdr = open(os.path.join(ROOT, "include", "lifcal_depth.h")).read()
    declared = set(re.findall(r"\b(lifcal_depth_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(capi.DEPTH_PROTOTYPES), declared ^ set(capi.DEPTH_PROTOTYPES)
    lib = capi.load_library()
    for name in sorted(declared) + ["lifcal_ba_object_space_stats", "lifcal_write_object_coordinates_ply", "lifcal_write_object_coordinates_colmap_ids",
                                    "lifcal_write_camera_orientations_ply", "lifcal_write_camera_coordinates_ply"]:
        assert hasattr(lib, name), name
    assert "lifcal_ba_object_space_stats" in capi.PROTOTYPES
    assert {"lifcal_write_object_coordinates_ply", "lifcal_write_object_coordinates_colmap_ids", "lifcal_write_camera_orientations_ply",
            "lifcal_write_camera_coordinates_ply"} <= set(capi.IO_PROTOTYPES)
    # sizes implied by the headers on LP64
    assert C.sizeof(capi.DepthSampleCounts) == 3 * 8
    assert C.sizeof(capi.DepthCamera) == 17 * 8 + 2 * 8 + 2 * 4
    assert C.sizeof(capi.DepthPoints) == 8 + 5 * 8 + 2 * 4 + 8 + 8 + 5 * 8 + 8
    assert C.sizeof(capi.DepthMapsArgs) == 6 * 4 + 3 * 8 + 8 + 3 * 8 + 8 + 8
    assert C.sizeof(capi.ObjectSpace) == 7 * 8 + 2 * 8
    # the field lists follow the header's declaration order
    for cls, cname in [(capi.DepthPoints, "lifcal_depth_points"), (capi.DepthMapsArgs, "lifcal_depth_maps"), (capi.DepthCamera, "lifcal_depth_camera")]:
        body = re.search(r"typedef struct " + cname + r" \{(.*?)\} " + cname + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"(\w+)(?:\[\d+\])?\s*(?:,|$)", decl.strip())]
        assert names == [f for f, _ in cls._fields_], (cname, names)


def test_depth_calls_validate_before_touching_a_device(built):
    """NULL arguments give LIFCAL_BA_ERR_INVALID_ARG whether or not a GPU is present"""
    lib = capi.load_library()
    assert lib.lifcal_depth_create(16, 16, 1, 0, None) == -1
    h = C.c_void_p()
    assert lib.lifcal_depth_create(0, 16, 1, 0, C.byref(h)) == -1 and not h.value
    assert lib.lifcal_depth_set_maps(None, 0, 1, None, 0) == -1
    assert lib.lifcal_depth_sample(None, 0, None, None, None, None, None) == -1
    assert lib.lifcal_depth_back_project_points(0, None, None) == -1
    assert lib.lifcal_depth_back_project_maps(None, None, None) == -1
    assert lib.lifcal_ba_object_space_stats(None, 0, None, None, None, None, None, None, None, None) == -1
    lib.lifcal_depth_destroy(None)
    dc = depth.depth_camera(CAM, 0x3, SPX)                       # three radial coefficients: the solver clamps to two, so does this
    io = capi.DepthPoints()
    assert lib.lifcal_depth_back_project_points(0, C.byref(dc), C.byref(io)) == -1
