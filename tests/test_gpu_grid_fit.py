"""The micro-lens grid from a white image on the GPU (include/lifcal_grid.h): lifcal_grid_detect against the
numpy restatement (same peaks, same integer moments, same bits of cx / cy), lifcal_grid_fit end to end against the true grid,
vignetting and defects, 8- against 16-bit input, the count protocol, and the chain into projectPointsToRawImage."""
import ctypes as C
import functools

import numpy as np
import pytest

from lifcal_amd import _capi as capi, grid_fit, scene, white_image, MicroLensGrid
from tests import grid_fit_reference as ref

pytestmark = pytest.mark.gpu

ALL_CASES = ("d14", "d23", "d7", "d9_pitch")


def _device_image(name, noise=0.0):
    """the case's image as the device entry points get it; d9_pitch sits in a wider array (row pitch 232 > width 200)"""
    img = ref.make_case(name, noise)
    if name != "d9_pitch":
        return img
    wide = np.full((img.shape[0], img.shape[1] + 32), 255, img.dtype)   # what lies beyond the width must not be read as image
    wide[:, :img.shape[1]] = img
    return wide[:, :img.shape[1]]


def _same_centres(got, want):
    assert len(got) == len(want) and len(got) > 0
    assert np.array_equal(got["peak"], want["peak"])                                   # same pixels, same (ascending) order
    assert np.all(np.diff(got["peak"]) > 0)
    for f in ("sum_w", "sum_wx", "sum_wy"):
        assert np.array_equal(got[f], want[f]), f
    assert got["cx"].tobytes() == want["cx"].tobytes() and got["cy"].tobytes() == want["cy"].tobytes()


@pytest.mark.parametrize("name", ALL_CASES)
def test_detect_is_the_restatement(built, name):
    """tile edges, halos and the border margin all occur: 333 x 251 is no multiple of any tile, 7.5 px lenses put peaks right at
    the margin, 23.2 px lenses span box tiles"""
    w, h, d, rot, off, bits = ref.CASES[name]
    for noise, gf in ((0.0, 1.0), (0.01, 0.9), (0.01, 1.1)):
        _same_centres(grid_fit.detectLensCentres(_device_image(name, noise), gf * d), ref.detect_case(name, noise, gf * d))


@pytest.mark.parametrize("name", ALL_CASES)
def test_fit_end_to_end(built, name):
    w, h, d, rot, off, bits = ref.CASES[name]
    tx, ty = ref.true_centres(name)
    inn = ref.interior(tx, ty, w, h, d)
    for gf in (0.9, 1.0, 1.1):
        got = grid_fit.fitGrid(_device_image(name, 0.01), gf * d)
        p = got.params
        fx, fy = white_image.grid_centres(w, h, p.lens_diameter, tuple(p.lens_base_y), p.rotation, tuple(p.offset))
        err = ref.grid_error(fx, fy, tx[inn], ty[inn])
        print(f"{name} guess {gf} d: grid error {err:.4f} px, rms {got.report.rms:.4f} px, d {got.report.lens_diameter:.5f}")
        assert err <= ref.ACCURACY_BAR, (name, gf, err)
        assert got.report.n_accepted == got.report.n_centres == len(got.centres) >= inn.sum()
        assert -1.0 <= p.lens_base_y[0] < 0.0 and p.rotation_on_grid == 1
    # the second pass is the restatement's second pass: detection at the fitted diameter
    c2, f2, g2 = ref.two_pass(ref.make_case(name, 0.01), 1.1 * d)
    _same_centres(got.centres, c2)
    assert np.array_equal(got.report.lens["x"], f2.label[:, 1]) and abs(got.report.lens_diameter - float(f2.d)) < 1e-9


def test_from_white_image_matches_the_true_grid(built):
    name = "d23"
    w, h, d, rot, off, bits = ref.CASES[name]
    with _closing(MicroLensGrid(w, h, d, (0.5, 0.8660254), rot, off)) as true:
        tcx, tcy, _ = true.lenses()
    with _closing(MicroLensGrid.from_white_image(_device_image(name, 0.01), 1.05 * d)) as g:
        fcx, fcy, _ = g.lenses()
        assert g.grid_fit.report.n_accepted > 150
    inside = (tcx > 0) & (tcx < w - 1) & (tcy > 0) & (tcy < h - 1)
    assert inside.sum() > 150
    assert ref.grid_error(fcx.astype(np.float64), fcy.astype(np.float64), tcx[inside].astype(np.float64), tcy[inside].astype(np.float64)) <= ref.ACCURACY_BAR
    finside = (fcx > 0) & (fcx < w - 1) & (fcy > 0) & (fcy < h - 1)
    assert ref.grid_error(tcx.astype(np.float64), tcy.astype(np.float64), fcx[finside].astype(np.float64), fcy[finside].astype(np.float64)) <= ref.ACCURACY_BAR


class _closing:
    def __init__(self, g):
        self.g = g

    def __enter__(self):
        return self.g

    def __exit__(self, *a):
        self.g.close()


def test_vignetting_loses_no_lens(built):
    """corners at 30 % of the centre's brightness: every interior lens is found, and the detection is still the restatement's"""
    name = "d14"
    w, h, d, rot, off, bits = ref.CASES[name]
    img = ref.make_case(name, 0.01, vignetting=0.3)
    got = grid_fit.detectLensCentres(img, d)
    _same_centres(got, ref.detect(img, d))
    tx, ty = ref.true_centres(name)
    inn = ref.interior(tx, ty, w, h, d)
    assert ref.grid_error(got["cx"], got["cy"], tx[inn], ty[inn]) < 0.5          # a detected centre at every interior lens
    assert len(got) == len(ref.detect_case(name, 0.01, d))                        # as many as without vignetting
    fit = grid_fit.fitGrid(img, d)
    assert fit.report.n_accepted == fit.report.n_centres == len(got)


def test_saturated_centre(built):
    """gain 1.5: the disc tops are clipped flat (box-sum ties are broken by the lower pixel index); same lenses, same grid"""
    name = "d14"
    w, h, d, rot, off, bits = ref.CASES[name]
    img = ref.make_case(name, 0.0, gain=1.5)
    assert (img == 255).mean() > 0.1
    got = grid_fit.detectLensCentres(img, d)
    _same_centres(got, ref.detect(img, d))
    assert len(got) == len(ref.detect_case(name, 0.0, d))
    fit = grid_fit.fitGrid(img, d)
    tx, ty = ref.true_centres(name)
    inn = ref.interior(tx, ty, w, h, d)
    p = fit.params
    fx, fy = white_image.grid_centres(w, h, p.lens_diameter, tuple(p.lens_base_y), p.rotation, tuple(p.offset))
    assert fit.report.n_accepted == fit.report.n_centres and ref.grid_error(fx, fy, tx[inn], ty[inn]) <= ref.ACCURACY_BAR


def test_defects(built):
    """three hot pixels, one blocked lens and one dust spot that moves its lens's centroid (restatement, CPU) by at least 0.5 px:
    the dusty lens is rejected, the blocked one is absent, the rest stays within the bar"""
    name = "d14"
    w, h, d, rot, off, bits = ref.CASES[name]
    tx, ty = ref.true_centres(name, margin=1.5)
    dusty = int(np.argmin((tx - 100.0) ** 2 + (ty - 90.0) ** 2)); blocked = int(np.argmin((tx - 220.0) ** 2 + (ty - 150.0) ** 2))
    dust = (float(tx[dusty]) + 0.25 * d, float(ty[dusty]) + 0.1 * d, 0.3 * d, 0.05)
    hot = ((int(round(tx[dusty])) + 60, int(round(ty[dusty])) + 2), (31, 200), (250, 40))
    img = ref.make_case(name, 0.01, hot_pixels=hot, blocked=(blocked,), dust=dust)
    clean = ref.detect_case(name, 0.01, d)
    want = ref.detect(img, d)
    k_clean = int(np.argmin((clean["cx"] - tx[dusty]) ** 2 + (clean["cy"] - ty[dusty]) ** 2))
    k = int(np.argmin((want["cx"] - tx[dusty]) ** 2 + (want["cy"] - ty[dusty]) ** 2))
    shift = np.hypot(want["cx"][k] - clean["cx"][k_clean], want["cy"][k] - clean["cy"][k_clean])
    assert shift >= 0.5, shift                                                     # the premise, checked on the CPU
    assert len(want) == len(clean) - 1                                             # the blocked lens draws no disc
    fit = grid_fit.fitGrid(img, d)
    lens = fit.report.lens
    k2 = int(np.argmin((fit.centres["cx"] - tx[dusty]) ** 2 + (fit.centres["cy"] - ty[dusty]) ** 2))
    assert lens["accepted"][k2] == 0 and lens["accepted"].sum() == len(lens) - 1 == fit.report.n_accepted
    assert np.hypot(fit.centres["cx"] - tx[blocked], fit.centres["cy"] - ty[blocked]).min() > 0.4 * d
    inn = ref.interior(tx, ty, w, h, d)
    p = fit.params
    fx, fy = white_image.grid_centres(w, h, p.lens_diameter, tuple(p.lens_base_y), p.rotation, tuple(p.offset))
    assert ref.grid_error(fx, fy, tx[inn], ty[inn]) <= ref.ACCURACY_BAR


def test_8_and_16_bit_give_the_same_peaks(built):
    """the same scene in both forms (16-bit = 8-bit x 257, full scale onto full scale): same peaks, and since every sum scales by
    257, the same centres"""
    for name in ("d14", "d7"):
        w, h, d, rot, off, bits = ref.CASES[name]
        a8 = ref.make_case(name, 0.01)
        a16 = a8.astype(np.uint16) * np.uint16(257)
        c8, c16 = grid_fit.detectLensCentres(a8, d), grid_fit.detectLensCentres(a16, d)
        assert np.array_equal(c8["peak"], c16["peak"]) and len(c8) > 300
        assert np.array_equal(c8["sum_w"] * 257, c16["sum_w"]) and np.array_equal(c8["sum_wx"] * 257, c16["sum_wx"])
        assert np.array_equal(c8["cx"], c16["cx"]) and np.array_equal(c8["cy"], c16["cy"])
    # an independently quantised 16-bit rendering finds the same interior lenses (a peak right at the border margin may fall on
    # either side of it when the rounding differs)
    w, h, d, rot, off, bits = ref.CASES["d14"]
    r16 = grid_fit.detectLensCentres(ref.make_case("d14", 0.0, bits=16), d)
    r8 = grid_fit.detectLensCentres(ref.make_case("d14", 0.0), d)
    inn = ref.interior(r8["cx"], r8["cy"], w, h, d)
    assert inn.sum() > 300 and ref.grid_error(r16["cx"], r16["cy"], r8["cx"][inn], r8["cy"][inn]) < 0.05


def test_count_protocol_and_reproducibility(built):
    lib = capi.load_library()
    name = "d23"
    w, h, d, rot, off, bits = ref.CASES[name]
    img = ref.make_case(name, 0.01)
    gi = capi.GridImage(img.ctypes.data, bits, w, h, w)
    want = ref.detect_case(name, 0.01, d)
    out = capi.GridCentres(0, 0, None)
    assert lib.lifcal_grid_detect(C.byref(gi), d, 0, C.byref(out)) == capi.MLA_MORE and out.n == len(want)   # capacity 0 counts
    buf = np.full(len(want), -1, capi.GRID_CENTRE_DTYPE)
    out = capi.GridCentres(len(want) - 1, 0, buf.ctypes.data)
    assert lib.lifcal_grid_detect(C.byref(gi), d, 0, C.byref(out)) == capi.MLA_MORE and out.n == len(want)
    assert np.all(buf["peak"] == -1) and np.all(buf["sum_w"] == -1)                                         # nothing written
    out = capi.GridCentres(len(want), 0, buf.ctypes.data)
    assert lib.lifcal_grid_detect(C.byref(gi), d, 0, C.byref(out)) == 0 and out.n == len(want)
    first = buf.tobytes()
    buf2 = np.full(len(want) + 3, -1, capi.GRID_CENTRE_DTYPE)
    out = capi.GridCentres(len(buf2), 0, buf2.ctypes.data)
    assert lib.lifcal_grid_detect(C.byref(gi), d, 0, C.byref(out)) == 0 and out.n == len(want)
    assert buf2[:len(want)].tobytes() == first and np.all(buf2["peak"][len(want):] == -1)
    # lifcal_grid_fit: the same protocol for its centres and its per-lens table, and the same bytes twice
    prm = capi.MlaParams(); cen = capi.GridCentres(0, 0, None); rep = capi.GridReport()
    assert lib.lifcal_grid_fit(C.byref(gi), d, 0.5, 0, C.byref(prm), C.byref(cen), C.byref(rep)) == capi.MLA_MORE
    n = int(cen.n)
    assert n == rep.n_centres > 150 and prm.lens_diameter == 0.0
    lens = np.full(n, -1, capi.GRID_LENS_DTYPE)
    rep = capi.GridReport(); rep.capacity, rep.lens = n - 1, lens.ctypes.data
    assert lib.lifcal_grid_fit(C.byref(gi), d, 0.5, 0, C.byref(prm), None, C.byref(rep)) == capi.MLA_MORE and np.all(lens["x"] == -1)
    a, b = grid_fit.fitGrid(img, d), grid_fit.fitGrid(img, d)
    assert a.centres.tobytes() == b.centres.tobytes() and a.report.lens.tobytes() == b.report.lens.tobytes()
    assert bytes(a.params) == bytes(b.params) and a.report.rms == b.report.rms
    assert lib.lifcal_grid_fit(C.byref(gi), d, 0.5, 0, C.byref(prm), None, None) == 0 and bytes(prm) == bytes(a.params)   # parameters only


@functools.lru_cache(maxsize=None)
def _chain_scene():
    return scene.make_scene(scene.baseline_spec("tiny"))


def test_chain_into_projection(built):
    """a small scene through projectPointsToRawImage with the fitted grid and with the true one: the same number of observations
    for every image point that lies deeper than the bar inside its nearest lens's validity disc, lens centres within the bar"""
    sc = _chain_scene()
    sp = sc.spec
    w, h, d = sp.raw_width, sp.raw_height, sp.lens_diameter
    tx, ty = white_image.grid_centres(w, h, d, sp.lens_base_y, sp.grid_rotation, sp.grid_offset, margin=1.5)
    img = white_image.render_white_image(w, h, tx, ty, d, bits=8, noise=0.01, seed=3)
    with _closing(MicroLensGrid(w, h, d, sp.lens_base_y, sp.grid_rotation, sp.grid_offset)) as true, \
            _closing(MicroLensGrid.from_white_image(img, 24.0)) as fitted:
        a = true.projectPointsToRawImage(sc.img_x, sc.img_y, sc.img_vd, sp.scale)
        b = fitted.projectPointsToRawImage(sc.img_x, sc.img_y, sc.img_vd, sp.scale)
        tcx, tcy, _ = true.lenses()
    n = len(sc.img_x)
    xu, yu = sp.scale * (sc.img_x + 0.5) - 0.5, sp.scale * (sc.img_y + 0.5) - 0.5
    nearest = np.sqrt(((xu[:, None] - tcx[None, :].astype(np.float64)) ** 2 + (yu[:, None] - tcy[None, :].astype(np.float64)) ** 2).min(axis=1))
    firm = nearest < (d * 0.5 - 1.0) - ref.ACCURACY_BAR
    assert firm.sum() > 0.5 * n
    ca, cb = np.bincount(a.src, minlength=n), np.bincount(b.src, minlength=n)
    assert ca[firm].sum() > 500
    assert np.array_equal(ca[firm], cb[firm]), np.flatnonzero(firm & (ca != cb))
    same = firm & (ca == cb)
    ia, ib = np.flatnonzero(same[a.src]), np.flatnonzero(same[b.src])
    assert np.array_equal(a.src[ia], b.src[ib])
    dist = np.hypot(a.mcx[ia] - b.mcx[ib], a.mcy[ia] - b.mcy[ib])
    print(f"chain: {len(ia)} observations of {firm.sum()} image points, lens centres differ by at most {dist.max():.4f} px")
    assert dist.max() <= ref.ACCURACY_BAR
