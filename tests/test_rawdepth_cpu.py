"""Virtual depth from the raw image, what needs no GPU: the exports and struct layouts of
include/lifcal_rawdepth.h, the argument checks (they come before any device is touched), the numpy restatement's accuracy on the
rendered scenes, where the bars of the GPU tests are set, and the renderer's geometry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lifcal_amd import _capi as capi, raw_depth, raw_image, white_image, LifcalError
from tests import rawdepth_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(name):
    w, h, d, base_y, rot, off, on_grid = ref.grid_arguments(name)
    return capi.MlaParams(w, h, d, (C.c_float * 2)(*base_y), rot, (C.c_float * 2)(*off), 1 if on_grid else 0)


def test_exports_and_layout(built):
    hdr = open(os.path.join(ROOT, "include", "lifcal_rawdepth.h")).read()
    declared = set(re.findall(r"\b(lifcal_rawdepth_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(capi.RAWDEPTH_PROTOTYPES) and len(declared) == 3, declared ^ set(capi.RAWDEPTH_PROTOTYPES)
    lib = capi.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/lifcal_rawdepth.h but not exported"
    # sizes and offsets implied by include/lifcal_rawdepth.h on LP64
    assert C.sizeof(capi.RawDepthImage) == 32 and capi.RawDepthImage.pitch.offset == 24
    assert C.sizeof(capi.RawDepthOptions) == 48 and capi.RawDepthOptions.iv_min.offset == 16
    assert C.sizeof(capi.RawDepthPlan) == 64 and capi.RawDepthPlan.n_neighbours.offset == 48
    assert C.sizeof(capi.RawDepthResult) == 8 + 4 * 8 + 5 * 8 + 8 and capi.RawDepthResult.count.offset == 40
    assert C.sizeof(capi.RawDepthPointList) == 8 + 8 + 8 + 8 + 5 * 8 and capi.RawDepthPointList.x.offset == 32
    # the defaults land where the ctypes view reads them
    plan = raw_depth.checkRawDepth(params("d14"), np.zeros((160, 200), np.uint8))
    o = plan.options
    assert (o.n_hyp, o.patch_radius, o.min_neighbours, o.min_contrast) == (64, 1, 2, 8)
    assert (o.iv_min, o.iv_max, o.max_baseline, o.ambiguity_ratio) == (0.04, 0.5, 1.05, 1.5)
    assert raw_depth.checkRawDepth(params("d23_16"), np.zeros((144, 176), np.uint16)).options.min_contrast == 2048


def test_argument_errors(built):
    """every check runs before a device is looked for: wrong size, K out of range, iv_max > 0.5, more than 18 neighbours, no image"""
    lib = capi.load_library()
    p = params("d14")
    img = np.zeros((160, 200), np.uint8)

    def check(image=img, prm=p, **o):
        im, keep = raw_depth._image(image)
        opt = raw_depth.make_options(**o)
        return lib.lifcal_rawdepth_check(C.byref(prm) if prm is not None else None, C.byref(im), C.byref(opt), None)

    assert check() == 0
    assert check(np.zeros((160, 201), np.uint8)) == -1 and b"size" in lib.lifcal_ba_last_error()
    assert check(np.zeros((161, 200), np.uint8)) == -1
    for K in (7, 257, -1):
        assert check(n_hyp=K) == -1 and b"n_hyp" in lib.lifcal_ba_last_error()
    assert check(n_hyp=8) == 0 and check(n_hyp=256) == 0
    assert check(iv_max=0.5000001) == -1 and b"iv_max" in lib.lifcal_ba_last_error()
    assert check(iv_min=0.3, iv_max=0.3) == -1 and check(iv_min=-0.1) == -1 and check(iv_max=float("nan")) == -1
    assert check(max_baseline=2.1) == 0
    assert check(max_baseline=2.7) == -1 and b"18" in lib.lifcal_ba_last_error()
    assert check(max_baseline=0.5) == -1 and b"no neighbour" in lib.lifcal_ba_last_error()
    assert check(patch_radius=3) == -1 and check(min_neighbours=19) == -1 and check(min_neighbours=-1) == -1
    assert check(ambiguity_ratio=0.9) == -1 and check(min_contrast=-1) == -1
    assert check(prm=None) == -1
    for field, value in (("data", None), ("bits", 12), ("pitch", 199), ("width", 0)):
        im = capi.RawDepthImage(img.ctypes.data, 8, 200, 160, 0, 200); setattr(im, field, value)
        assert lib.lifcal_rawdepth_check(C.byref(p), C.byref(im), None, None) == -1, field
    im = capi.RawDepthImage(img.ctypes.data, 8, 200, 160, 0, 200)
    assert lib.lifcal_rawdepth_check(C.byref(p), None, None, None) == -1 and b"no image" in lib.lifcal_ba_last_error()
    assert lib.lifcal_rawdepth_check(C.byref(p), C.byref(im), None, None) == 0          # no options: all defaults
    # the entry points themselves refuse a missing grid, image or result without touching a device
    res = capi.RawDepthResult()
    assert lib.lifcal_rawdepth_estimate(None, C.byref(im), None, C.byref(res)) == -1
    io = capi.RawDepthPointList()
    assert lib.lifcal_rawdepth_points(None, C.byref(io)) == -1
    # a lens neighbourhood beyond 64 KB of LDS is out of range
    big = capi.MlaParams(256, 200, 60.0, (C.c_float * 2)(*ref.BASE_Y), 0.0, (C.c_float * 2)(0.0, 0.0), 1)
    im = capi.RawDepthImage(img.ctypes.data, 8, 256, 200, 0, 256)
    assert lib.lifcal_rawdepth_check(C.byref(big), C.byref(im), None, None) == -4 and b"LDS" in lib.lifcal_ba_last_error()
    with pytest.raises(LifcalError, match="18"):
        raw_depth.checkRawDepth(p, img, max_baseline=3.0)
    with pytest.raises(TypeError):
        raw_depth.checkRawDepth(p, img, n_hypotheses=3)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_plan_matches_restatement_tables(built, name):
    """6 and 18 neighbours at the two baselines, the same for both sub-grids, and a window that holds every shift of the tables"""
    check_plan(name)


@pytest.mark.parametrize("name", list(ref.GEOMETRY_CASES))
def test_plan_matches_restatement_tables_on_other_geometries(built, name):
    """the same on the rotated, the squeezed and the rotation-off-grid lattice: 1.05 d still selects 6 and 2.1 d 18 where the six
    nearest are not equidistant"""
    check_plan(name)


def check_plan(name):
    w, h, d, rot, off, bits, pr, _, base_y, on_grid = ref.case(name)
    img = np.zeros((h, w), np.uint8 if bits == 8 else np.uint16)
    for mb, n in ((1.05, 6), (2.1, 18)):
        opt = ref.options(bits, patch_radius=pr, max_baseline=mb)
        tab = ref.tables(d, base_y, rot, opt, on_grid)
        plan = raw_depth.checkRawDepth(params(name), img, patch_radius=pr, max_baseline=mb)
        assert plan.n_neighbours == n == len(tab.delta[0]) == len(tab.delta[1])
        # a neighbour of sub-grid 0 is minus a neighbour of sub-grid 1
        a = sorted((round(x, 6), round(y, 6)) for x, y in tab.delta[0]); b = sorted((round(-x, 6), round(-y, 6)) for x, y in tab.delta[1])
        assert a == b
        reach = int(np.floor(tab.valid_r - pr + 0.5)) + pr + int(np.ceil(np.abs(tab.shift).max() / 64.0)) + 1
        assert plan.window == 2 * reach + 1 and plan.lds_bytes <= 62 * 1024


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_accuracy(built, name):
    """the restatement against the true depth of every scene of the case, with noise, at the case's neighbour sets: the issue's
    coverage and outlier conditions hold, and inlier RMS and |median e| stay within the recorded figures, whose double is the bar
    of the GPU tests.  (The recorded figures are the largest over noise 0 and NOISE; this test runs the noisy half.)"""
    from oracle.mla import MicroLensGrid
    gd = ref.grid_data(name, MicroLensGrid(*ref.grid_arguments(name)))
    for scn in ref.SCENE_NAMES:
        cov_min, out_max = ref.CONDITIONS[scn]
        for mb in ref.ACCURACY_BASELINES[name]:
            est = ref.run(name, scn, ref.NOISE, gd, max_baseline=mb)
            a = ref.accuracy(name, scn, est, gd.cx, gd.cy, gd.map_ml)
            print(f"{name} {scn} max_baseline {mb}: coverage {a['coverage']:.3f}, outliers {a['outliers']:.4f}, inlier rms {a['rms']:.5f}, "
                  f"|median| {a['median']:.5f} over {a['n']} pixels; counts {est.counts.tolist()}")
            assert a["coverage"] >= cov_min and a["outliers"] <= out_max, (scn, mb, a)
            assert a["rms"] <= ref.MEASURED[name]["rms"] and a["median"] <= ref.MEASURED[name]["median"], (scn, mb, a)
            assert int(est.counts.sum()) == est.status.size


def oracle_grid(name):
    from oracle.mla import MicroLensGrid
    return ref.grid_data(name, MicroLensGrid(*ref.grid_arguments(name)))


def lenses_lie_on_rendered_lattice(name, gd):
    """the largest distance of a lens centre of the library from the nearest centre the image is rendered with (for d14_rot_off
    that is the UNROTATED lattice)"""
    w, h, d, _, off, _, _, _, base_y, _ = ref.case(name)
    tx, ty = white_image.grid_centres(w, h, d, base_y, ref.grid_rotation(name), off, 1.5)
    dist = np.hypot(gd.cx.astype(np.float64)[:, None] - tx[None, :], gd.cy.astype(np.float64)[:, None] - ty[None, :]).min(axis=1)
    return float(dist.max())


@pytest.mark.parametrize("name", list(ref.GEOMETRY_CASES))
def test_restatement_accuracy_on_other_geometries(built, name):
    """the twin of test_restatement_accuracy on the rotated, the squeezed and the rotation-off-grid lattice, at noise 0 and NOISE
    and with 6 and 18 neighbours: this is where MEASURED of these cases is measured.  First the case is shown not to be vacuous:
    the library's lenses lie where the image was rendered (on the unrotated lattice for d14_rot_off, whatever its rotation says)."""
    gd = oracle_grid(name)
    off_lattice = lenses_lie_on_rendered_lattice(name, gd)
    print(f"{name}: {len(gd.cx)} lenses, at most {off_lattice:.2e} px from the rendered lattice, sub-grids {np.bincount(gd.sub).tolist()}")
    assert off_lattice < 1e-3
    for scn in ref.SCENE_NAMES:
        cov_min, out_max = ref.CONDITIONS[scn]
        for mb in ref.ACCURACY_BASELINES[name]:
            for noise in (0.0, ref.NOISE):
                est = ref.run(name, scn, noise, gd, max_baseline=mb)
                a = ref.accuracy(name, scn, est, gd.cx, gd.cy, gd.map_ml)
                print(f"{name} {scn} max_baseline {mb} noise {noise}: coverage {a['coverage']:.3f}, outliers {a['outliers']:.4f}, inlier rms {a['rms']:.5f}, "
                      f"|median| {a['median']:.5f} over {a['n']} pixels; counts {est.counts.tolist()}")
                assert a["coverage"] >= cov_min and a["outliers"] <= out_max, (scn, mb, noise, a)
                assert a["rms"] <= ref.MEASURED[name]["rms"] and a["median"] <= ref.MEASURED[name]["median"], (scn, mb, noise, a)
                assert int(est.counts.sum()) == est.status.size


# name: the rotation the mutant's tables are built for (on the grid) instead of the case's own
WRONG_ROTATION = {"d14": -0.003, "d14_rot": -0.03, "d17_sq": 0.021, "d14_rot_off": 0.03}


@pytest.mark.parametrize("name", list(WRONG_ROTATION))
def test_wrong_rotation_in_the_tables_is_seen_only_on_the_rotated_grids(built, name):
    """a mutation check: the restatement with its tables built for the WRONG rotation (the sign flipped; for d14_rot_off the
    rotation taken to be the grid's), mid scene at NOISE, against the conditions and bars of the accuracy tests.  The kernel's
    tables and the restatement's are built the same way, so equal bytes cannot see such a mistake; only the true depth can.
    On d14 (0.003 rad) the mutant passes every condition and bar at both neighbour sets: that is the gap the cases of CASES leave.
    On d14_rot, d17_sq and d14_rot_off it fails the outlier cap with 18 neighbours, all three asserted (measured: outliers 0.248,
    0.078, 0.036 against 0.015; with 6 neighbours 0.119, 0.029, 0.0095, the last within the cap, so 18 it is)."""
    gd = oracle_grid(name)
    cov_min, out_max = ref.CONDITIONS["mid"]
    bars = ref.BARS[name]
    passes = {}
    for mb in (1.05, 2.1):
        good = ref.accuracy(name, "mid", ref.run(name, "mid", ref.NOISE, gd, max_baseline=mb), gd.cx, gd.cy, gd.map_ml)
        a = ref.accuracy(name, "mid", ref.run(name, "mid", ref.NOISE, gd, tables_rotation=WRONG_ROTATION[name], max_baseline=mb), gd.cx, gd.cy, gd.map_ml)
        passes[mb] = a["coverage"] >= cov_min and a["outliers"] <= out_max and a["rms"] <= bars["rms"] and a["median"] <= bars["median"]
        print(f"{name} max_baseline {mb} tables for rotation {WRONG_ROTATION[name]}: coverage {a['coverage']:.3f}, outliers {a['outliers']:.4f}, "
              f"inlier rms {a['rms']:.5f} (bar {bars['rms']:.5f}), |median| {a['median']:.5f} (bar {bars['median']:.5f}): "
              f"{'passes' if passes[mb] else 'FAILS'}; the right tables: outliers {good['outliers']:.4f}, inlier rms {good['rms']:.5f}")
        assert good["coverage"] >= cov_min and good["outliers"] <= out_max and good["rms"] <= bars["rms"] and good["median"] <= bars["median"]
        if mb == 2.1 and name != "d14":
            assert a["outliers"] > out_max or a["rms"] > bars["rms"], (name, a, bars)
    if name == "d14":
        assert passes[1.05] and passes[2.1]          # the gap: a sign error of the rotation would pass the tests on CASES alone
    else:
        assert not passes[2.1]


def test_renderer_geometry():
    """a point of the texture lands where lifcal_mla_project's formula says: a Gaussian spot at the virtual-image point X at
    virtual depth v shows in the lens with centre c at xr = (X - c) / v + c.  X lies between three adjacent lenses; the spot's
    centroid over a 9 x 9 window about the predicted position is compared for every lens that holds the window; 16-bit, so
    quantisation is below 1e-4 of the peak, and the window cuts the spot (sigma 1 raw pixel) beyond 3.5 sigma: the tolerance of
    0.03 px covers the cut and the 3 x 3 supersampling."""
    w, h, d, v = 160, 128, 23.2, 4.0
    cx, cy = white_image.grid_centres(w, h, d, ref.BASE_Y, 0.0, (0.0, 0.0), 1.5)
    near = np.argsort((cx - 80.0) ** 2 + (cy - 64.0) ** 2)[:3]
    X = np.array([cx[near].mean() + 0.37, cy[near].mean() - 0.21])
    spot = lambda x, y: np.exp(-((x - X[0]) ** 2 + (y - X[1]) ** 2) / (2.0 * v ** 2))
    img = raw_image.render_raw_image(w, h, cx, cy, d, raw_image.plane_depth(v), spot, bits=16, level=1.0).astype(np.float64)
    seen = 0
    for lcx, lcy in zip(cx, cy):
        xr, yr = (X[0] - lcx) / v + lcx, (X[1] - lcy) / v + lcy
        if np.hypot(xr - lcx, yr - lcy) > 0.98 * d / 2 - 6.0:
            continue
        x0, y0 = int(round(xr)) - 4, int(round(yr)) - 4
        win = img[y0:y0 + 9, x0:x0 + 9]
        assert win.shape == (9, 9) and win.max() > 0.8 * 65535
        yy, xx = np.mgrid[y0:y0 + 9, x0:x0 + 9]
        gx, gy = (win * xx).sum() / win.sum(), (win * yy).sum() / win.sum()
        assert abs(gx - xr) < 0.03 and abs(gy - yr) < 0.03, (lcx, lcy, gx - xr, gy - yr)
        seen += 1
    assert seen >= 3                                   # the point shows in several micro images, as a plenoptic 2.0 camera has it
    # a depth step: the depth a pixel shows is the depth AT the virtual point it shows
    dep = raw_image.step_depth(3.0, 6.0, 80.0)
    for px, c in ((70.0, 76.0), (82.0, 76.0), (77.5, 76.0)):
        vv = float(raw_image.virtual_depth_at(px, 60.0, c, 60.0, dep))
        assert vv == float(dep(c + vv * (px - c), 60.0))
    # the band-limited texture holds its band and its range, and is a function of its seed
    tex = raw_image.band_limited_texture(3, 20.0, 50.0)
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float64)
    t = tex(xx, yy)
    assert 0.0 <= t.min() < 0.2 and 0.8 < t.max() <= 1.0 and np.array_equal(t, raw_image.band_limited_texture(3, 20.0, 50.0)(xx, yy))
    spec = np.abs(np.fft.fft2((t - t.mean()) * np.outer(np.hanning(256), np.hanning(256))))
    f = np.hypot(*np.meshgrid(np.fft.fftfreq(256), np.fft.fftfreq(256)))
    assert spec[f > 1.0 / 15.0].max() < 0.05 * spec.max()
