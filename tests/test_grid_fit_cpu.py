"""The micro-lens grid from a white image, what needs no GPU: the numpy restatement against ground truth,
the host fit lifcal_grid_fit_centres against the restatement, the conventions, the outlier gate, the error codes, and the
exports and struct layouts of include/lifcal_grid.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lifcal_amd import _capi as capi, grid_fit, white_image, LifcalError
from tests import grid_fit_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_CASES = ("d14", "d23", "d7")


@pytest.mark.parametrize("name", CPU_CASES)
def test_restatement_against_ground_truth(name):
    """detect + fit twice (as lifcal_grid_fit does) on the rendered image: the fitted grid's centres against the true ones over
    the lenses wholly inside the image, at noise 0 and 0.01 of full scale and with guesses 0.9, 1.0, 1.1 d; no centre rejected"""
    w, h, d, rot, off, bits = ref.CASES[name]
    tx, ty = ref.true_centres(name)
    inn = ref.interior(tx, ty, w, h, d)
    assert inn.sum() >= 150
    for noise in (0.0, 0.01):
        for gf in (0.9, 1.0, 1.1):
            c, f, _ = ref.two_pass(ref.make_case(name, noise), gf * d)
            err = ref.grid_error(*f.centres(w, h), tx[inn], ty[inn])
            print(f"{name} noise {noise} guess {gf} d: {len(c)} centres, grid error {err:.4f} px, rms {float(f.rms):.4f} px, d {float(f.d):.5f}")
            assert f.n_rejected_label == 0 and f.n_rejected_residual == 0 and f.accepted.all()
            assert len(c) >= inn.sum()                       # every interior lens was found
            assert err <= ref.ACCURACY_BAR, (name, noise, gf, err)
            assert abs(float(f.d) - d) < 1e-3 and abs(float(f.rot) - rot) < 1e-4


@pytest.mark.parametrize("name", CPU_CASES)
def test_host_fit_matches_restatement(built, name):
    """lifcal_grid_fit_centres on the restatement's centres: labels and accept flags identical, residuals (centre minus fitted
    centre) within 16 x the difference between the restatement's float64 and longdouble arms (measured 5e-14 .. 3.5e-13 px between
    the arms, 0 .. 6e-14 px between the library and the float64 arm)"""
    w, h, d, rot, off, bits = ref.CASES[name]
    for noise, gf in ((0.0, 1.0), (0.01, 0.9), (0.01, 1.1)):
        c = ref.detect_case(name, noise, gf * d)
        f64 = ref.fit(c["cx"], c["cy"], w, h, gf * d)
        fld = ref.fit(c["cx"], c["cy"], w, h, gf * d, dtype=np.longdouble)
        arms = float(np.abs((f64.residual - fld.residual).astype(np.float64)).max())
        got = grid_fit.fitGridCentres(c["cx"], c["cy"], w, h, gf * d)
        lens = got.report.lens
        diff = max(np.abs(lens["dx"] - f64.residual[:, 0]).max(), np.abs(lens["dy"] - f64.residual[:, 1]).max())
        print(f"{name} noise {noise} guess {gf} d: float64 vs longdouble {arms:.2e} px, library vs float64 {diff:.2e} px")
        assert arms > 0
        assert diff <= 16 * arms, (diff, arms)
        assert np.array_equal(lens["sub"], f64.label[:, 0]) and np.array_equal(lens["x"], f64.label[:, 1]) and np.array_equal(lens["y"], f64.label[:, 2])
        assert np.array_equal(lens["accepted"] != 0, f64.accepted)
        r = got.report
        assert r.n_centres == len(c) and r.n_accepted == int(f64.accepted.sum()) and r.n_rejected_label == 0 and r.n_rejected_residual == 0
        assert abs(r.rms - float(f64.rms)) <= 16 * arms and abs(r.max_residual - float(f64.max_residual)) <= 16 * arms
        assert abs(r.lens_diameter - float(f64.d)) <= 1e-12 * d and abs(r.rotation - float(f64.rot)) <= 1e-12
        p = got.params
        assert (p.width, p.height, p.rotation_on_grid) == (w, h, 1)
        assert p.lens_diameter == np.float32(r.lens_diameter) and p.rotation == np.float32(r.rotation)
        assert p.offset[0] == np.float32(r.origin[0] - (w / 2 - 0.5)) and p.offset[1] == np.float32(-(r.origin[1] - (h / 2 - 0.5)))
        # the unconstrained lattice vectors: A along the row, B to the next row's lens, C two rows up (image y points down)
        assert abs(np.hypot(*r.lattice_a) - d) < 0.01 and abs(np.hypot(*r.lattice_b) - d) < 0.01 and abs(np.hypot(*r.lattice_c) - 2 * 0.8660254 * d) < 0.02
        assert r.lattice_a[0] > 0 and r.lattice_c[1] < 0


def test_conventions(built):
    """lens_base_y[0] in [-1, 0), lens_base_y[1] > 0, origin within one diameter of the image centre, rotation_on_grid = 1; a grid
    given as lens_base_y = (0.5, 0.866) comes back as -0.5 with the same set of centres"""
    name = "d14"
    w, h, d, rot, off, bits = ref.CASES[name]
    tx, ty = white_image.grid_centres(w, h, d, (0.5, 0.8660254), rot, off)
    tx2, ty2 = ref.true_centres(name)
    assert ref.grid_error(tx, ty, tx2, ty2) < 1e-9 and len(tx) == len(tx2)          # the same lattice under both parameter sets
    img = white_image.render_white_image(w, h, *white_image.grid_centres(w, h, d, (0.5, 0.8660254), rot, off, 1.5), d, bits=bits)
    c = ref.detect(img, d)
    got = grid_fit.fitGridCentres(c["cx"], c["cy"], w, h, d)
    p, r = got.params, got.report
    assert -1.0 <= p.lens_base_y[0] < 0.0 and abs(p.lens_base_y[0] + 0.5) < 1e-3 and abs(p.lens_base_y[1] - 0.8660254) < 1e-3
    assert p.rotation_on_grid == 1
    assert np.hypot(r.origin[0] - (w - 1) / 2, r.origin[1] - (h - 1) / 2) <= d
    org = (r.lens["sub"] == 0) & (r.lens["x"] == 0) & (r.lens["y"] == 0)
    assert org.sum() == 1 and np.hypot(c["cx"][org][0] - r.origin[0], c["cy"][org][0] - r.origin[1]) < 0.1
    fx, fy = white_image.grid_centres(w, h, p.lens_diameter, tuple(p.lens_base_y), p.rotation, tuple(p.offset))
    inn = ref.interior(tx, ty, w, h, d)
    assert ref.grid_error(fx, fy, tx[inn], ty[inn]) <= ref.ACCURACY_BAR


def test_outlier_gate(built):
    """one centre moved by 1 px, one removed, one spurious centre added to a clean list of 399: exactly the moved and the spurious
    one are rejected (restatement and library alike) and the fitted grid stays within the bar"""
    name = "d14"
    w, h, d, rot, off, bits = ref.CASES[name]
    c = ref.detect_case(name, 0.0, d)
    cx, cy = c["cx"].copy(), c["cy"].copy()
    assert 300 <= len(cx) <= 400
    moved, removed = 57, 211
    cx[moved] += 0.8; cy[moved] -= 0.6
    spur = (cx[120] + 0.45 * d, cy[120] + 0.1 * d)
    cx = np.delete(cx, removed); cy = np.delete(cy, removed)
    at = 300                                                     # anywhere in the list: the fit does not need the order
    cx = np.insert(cx, at, spur[0]); cy = np.insert(cy, at, spur[1])
    want = np.ones(len(cx), bool); want[moved] = False; want[at] = False
    f = ref.fit(cx, cy, w, h, d)
    got = grid_fit.fitGridCentres(cx, cy, w, h, d)
    assert np.array_equal(f.accepted, want) and np.array_equal(got.report.lens["accepted"] != 0, want)
    assert (got.report.n_rejected_label, got.report.n_rejected_residual) == (1, 1) == (f.n_rejected_label, f.n_rejected_residual)
    assert (~want).sum() <= 0.05 * len(cx)
    assert abs(np.hypot(got.report.lens["dx"][moved], got.report.lens["dy"][moved]) - 1.0) < 0.05
    tx, ty = ref.true_centres(name)
    inn = ref.interior(tx, ty, w, h, d)
    p = got.params
    fx, fy = white_image.grid_centres(w, h, p.lens_diameter, tuple(p.lens_base_y), p.rotation, tuple(p.offset))
    assert ref.grid_error(fx, fy, tx[inn], ty[inn]) <= ref.ACCURACY_BAR
    assert ref.grid_error(*f.centres(w, h), tx[inn], ty[inn]) <= ref.ACCURACY_BAR


def test_errors(built):
    lib = capi.load_library()
    name = "d14"
    w, h, d, rot, off, bits = ref.CASES[name]
    c = ref.detect_case(name, 0.0, d)
    cx, cy = np.ascontiguousarray(c["cx"]), np.ascontiguousarray(c["cy"])
    prm = capi.MlaParams()

    def call(x, y, guess=d, gate=0.5, n=None, params=prm, report=None):
        return lib.lifcal_grid_fit_centres(len(x) if n is None else n, capi.as_dptr(x), capi.as_dptr(y), w, h, guess, gate,
                                           C.byref(params) if params is not None else None, C.byref(report) if report is not None else None)

    assert call(cx, cy) == 0
    for guess in (5.9, 64.1, float("nan")):
        assert call(cx, cy, guess=guess) == -1
    assert b"guess" in lib.lifcal_ba_last_error()
    assert call(cx[:11], cy[:11]) == -1 and b"12" in lib.lifcal_ba_last_error()
    assert call(cx[:3], cy[:3], n=0) == -1
    lx = np.arange(20, dtype=np.float64) * d + 20.0
    assert call(lx, np.full(20, 128.0)) == -1                                  # collinear
    row3 = np.concatenate([lx, lx + d / 2]), np.concatenate([np.full(20, 120.0), np.full(20, 120.0 + 0.866 * d)])
    assert call(*row3) == -1                                                   # two rows only
    bad = cx.copy(); bad[17] = np.nan
    assert call(bad, cy) == -1 and b"finite" in lib.lifcal_ba_last_error()
    bad = cy.copy(); bad[3] = np.inf
    assert call(cx, bad) == -1
    rx, ry = white_image.grid_centres(w, h, d, ref.BASE_Y, np.deg2rad(20.0), off, margin=-1.0)
    assert len(rx) > 200 and call(np.ascontiguousarray(rx), np.ascontiguousarray(ry)) == -1 and b"rotation" in lib.lifcal_ba_last_error()
    rx, ry = white_image.grid_centres(w, h, d, ref.BASE_Y, np.deg2rad(8.0), off, margin=-1.0)
    assert call(np.ascontiguousarray(rx), np.ascontiguousarray(ry)) == 0 and abs(prm.rotation - np.deg2rad(8.0)) < 1e-6
    assert call(cx, cy, gate=-1.0) == -1
    # null pointers
    assert call(cx, cy, params=None) == -1
    assert lib.lifcal_grid_fit_centres(len(cx), None, capi.as_dptr(cy), w, h, d, 0.5, C.byref(prm), None) == -1
    assert lib.lifcal_grid_fit_centres(len(cx), capi.as_dptr(cx), None, w, h, d, 0.5, C.byref(prm), None) == -1
    # report capacity: 0 gives the summary only, 1 .. n - 1 is an error, a null table with a capacity too
    rep = capi.GridReport()
    assert call(cx, cy, report=rep) == 0 and rep.n_centres == len(cx) == rep.n_accepted and rep.rms > 0
    lens = np.zeros(len(cx), capi.GRID_LENS_DTYPE)
    rep = capi.GridReport(); rep.capacity, rep.lens = len(cx) - 1, lens.ctypes.data
    assert call(cx, cy, report=rep) == -1 and not lens["accepted"].any()
    rep = capi.GridReport(); rep.capacity, rep.lens = len(cx), None
    assert call(cx, cy, report=rep) == -1
    with pytest.raises(LifcalError, match="12"):
        grid_fit.fitGridCentres(cx[:5], cy[:5], w, h, d)
    # the detection's argument checks come before the device is looked for
    img = ref.make_case(name, 0.0)
    gi = capi.GridImage(img.ctypes.data, 8, w, h, w)
    out = capi.GridCentres(0, 0, None)
    assert lib.lifcal_grid_detect(None, d, 0, C.byref(out)) == -1 and lib.lifcal_grid_detect(C.byref(gi), d, 0, None) == -1
    assert lib.lifcal_grid_detect(C.byref(gi), 5.0, 0, C.byref(out)) == -1 and lib.lifcal_grid_detect(C.byref(gi), 65.0, 0, C.byref(out)) == -1
    for field, value in (("bits", 12), ("pitch", w - 1), ("width", 0), ("data", None)):
        g2 = capi.GridImage(img.ctypes.data, 8, w, h, w); setattr(g2, field, value)
        assert lib.lifcal_grid_detect(C.byref(g2), d, 0, C.byref(out)) == -1, field
    out = capi.GridCentres(4, 0, None)
    assert lib.lifcal_grid_detect(C.byref(gi), d, 0, C.byref(out)) == -1        # a capacity without an array
    assert lib.lifcal_grid_fit(C.byref(gi), d, 0.5, 0, None, None, None) == -1 and lib.lifcal_grid_fit(None, d, 0.5, 0, C.byref(prm), None, None) == -1
    assert lib.lifcal_grid_fit(C.byref(gi), 70.0, 0.5, 0, C.byref(prm), None, None) == -1


def test_detection_has_no_cpu_fallback(built):
    """either the device does the work or the call fails loudly: the library itself says which (LIFCAL_BA_ERR_NO_DEVICE = -2)"""
    lib = capi.load_library()
    img = ref.make_case("d14", 0.0)
    gi = capi.GridImage(img.ctypes.data, 8, img.shape[1], img.shape[0], img.shape[1])
    out = capi.GridCentres(0, 0, None)
    rc = lib.lifcal_grid_detect(C.byref(gi), 14.3, 0, C.byref(out))
    if rc == capi.MLA_MORE:                        # a gfx950 device is present
        assert out.n == len(ref.detect_case("d14", 0.0, 14.3))
        return
    assert rc == -2 and out.n == 0 and b"no CPU fallback" in lib.lifcal_ba_last_error()
    with pytest.raises(LifcalError, match="no CPU fallback"):
        grid_fit.detectLensCentres(img, 14.3)
    with pytest.raises(LifcalError, match="no CPU fallback"):
        grid_fit.fitGrid(img, 14.3)


def test_exports_and_layout(built):
    hdr = open(os.path.join(ROOT, "include", "lifcal_grid.h")).read()
    declared = set(re.findall(r"\b(lifcal_grid_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(capi.GRID_PROTOTYPES) and len(declared) == 3, declared ^ set(capi.GRID_PROTOTYPES)
    lib = capi.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/lifcal_grid.h but not exported"
    # sizes and offsets implied by include/lifcal_grid.h on LP64
    assert C.sizeof(capi.GridImage) == 8 + 3 * 4 + 4 + 8 and capi.GridImage.pitch.offset == 24
    assert C.sizeof(capi.GridCentre) == 48 == capi.GRID_CENTRE_DTYPE.itemsize and capi.GridCentre.peak.offset == 40
    assert C.sizeof(capi.GridCentres) == 24
    assert C.sizeof(capi.GridLens) == 32 == capi.GRID_LENS_DTYPE.itemsize and capi.GridLens.dx.offset == 16
    assert C.sizeof(capi.GridReport) == 2 * 8 + 4 * 8 + 2 * 8 + 6 * 8 + 2 * 8 + 4 * 8 and capi.GridReport.origin.offset == 144
    assert [n for n, _ in capi.GridCentre._fields_] == list(capi.GRID_CENTRE_DTYPE.names)
    assert [n for n, _ in capi.GridLens._fields_] == list(capi.GRID_LENS_DTYPE.names)
    # a field written by the library lands where the ctypes view reads it
    c = ref.detect_case("d14", 0.0, 14.3)
    got = grid_fit.fitGridCentres(c["cx"], c["cy"], 320, 256, 14.3)
    assert got.report.origin[0] == pytest.approx(got.params.offset[0] + 159.5, abs=1e-4) and got.report.lens_base_y[1] == pytest.approx(0.8660254, abs=1e-3)


def test_renderer_options():
    """white_image: quantisation, saturation, vignetting, hot pixels, blocked lenses and a dust spot do what they say"""
    w, h, d = 96, 80, 14.0
    cx, cy = white_image.grid_centres(w, h, d, margin=1.5)
    a8 = white_image.render_white_image(w, h, cx, cy, d, bits=8)
    a16 = white_image.render_white_image(w, h, cx, cy, d, bits=16)
    assert a8.dtype == np.uint8 and a16.dtype == np.uint16 and a8.shape == (h, w)
    # a pixel's 3 x 3 samples average the fall-off around the disc centre: just below the level of 0.8 of full scale
    assert 0.78 * 255 <= a8.max() <= round(0.8 * 255) and 0.78 * 65535 <= a16.max() <= round(0.8 * 65535) and a8.min() == 0
    assert np.abs(a16.astype(float) / 257.0 - a8).max() <= 0.51
    assert white_image.render_white_image(w, h, cx, cy, d, gain=1.5).max() == 255
    v = white_image.render_white_image(w, h, cx, cy, d, vignetting=0.3)
    assert a8[0, 0] > 100 and abs(int(v[0, 0]) - 0.3 * int(a8[0, 0])) <= 1 and abs(int(v[34:46, 40:56].max()) - int(a8[34:46, 40:56].max())) <= 2
    n1 = white_image.render_white_image(w, h, cx, cy, d, noise=0.01, seed=1)
    assert 0.005 * 255 < np.std(n1.astype(float) - a8) < 0.015 * 255
    assert np.array_equal(n1, white_image.render_white_image(w, h, cx, cy, d, noise=0.01, seed=1))
    assert white_image.render_white_image(w, h, cx, cy, d, hot_pixels=[(5, 7)])[7, 5] == 255
    k = int(np.argmin((cx - 48) ** 2 + (cy - 40) ** 2))
    b = white_image.render_white_image(w, h, cx, cy, d, blocked=[k])
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (xx - cx[k]) ** 2 + (yy - cy[k]) ** 2 < (0.4 * d) ** 2
    assert b[disc].max() == 0 and np.array_equal(b[~((xx - cx[k]) ** 2 + (yy - cy[k]) ** 2 < (0.5 * d) ** 2)], a8[~((xx - cx[k]) ** 2 + (yy - cy[k]) ** 2 < (0.5 * d) ** 2)])
    du = white_image.render_white_image(w, h, cx, cy, d, dust=(cx[k] + 2.0, cy[k], 2.5, 0.2))
    spot = (xx - cx[k] - 2.0) ** 2 + (yy - cy[k]) ** 2 <= 2.5 ** 2
    assert np.all(du[spot] <= 0.2 * a8[spot] + 1) and np.array_equal(du[~spot], a8[~spot])
