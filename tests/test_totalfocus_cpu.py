"""The total-focus image from the raw image and the virtual-image depth map, what needs no GPU: the exports
and struct layouts of include/lifcal_totalfocus.h, the argument checks (they come before any device is touched), the plan against
the numpy restatement, the restatement's rules on a hand-made case, and its accuracy and conditions on the rendered scenes, where
the bars of the GPU tests are set."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lifcal_amd import _capi as capi, total_focus, white_image, LifcalError
from tests import rawdepth_reference as ref
from tests import totalfocus_reference as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def params(name):
    w, h, d, base_y, rot, off, on_grid = ref.grid_arguments(name)
    return capi.MlaParams(w, h, d, (C.c_float * 2)(*base_y), rot, (C.c_float * 2)(*off), 1 if on_grid else 0)


def oracle_grid(name):
    from oracle.mla import MicroLensGrid
    return ref.grid_data(name, MicroLensGrid(*ref.grid_arguments(name)))


def test_exports_and_layout(built):
    import lifcal_amd
    hdr = open(os.path.join(ROOT, "include", "lifcal_totalfocus.h")).read()
    declared = set(re.findall(r"\b(lifcal_totalfocus_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(capi.TOTALFOCUS_PROTOTYPES) and len(declared) == 2, declared ^ set(capi.TOTALFOCUS_PROTOTYPES)
    lib = capi.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/lifcal_totalfocus.h but not exported"
    for name in ("totalFocusImage", "checkTotalFocus", "TotalFocusImage"):
        assert hasattr(lifcal_amd, name)
    assert hasattr(lifcal_amd.MicroLensGrid, "totalFocusImage") and hasattr(lifcal_amd.VirtualDepthMap, "total_focus")
    # sizes and offsets implied by include/lifcal_totalfocus.h on LP64
    assert C.sizeof(capi.TotalFocusOptions) == 56 and capi.TotalFocusOptions.white_level.offset == 16 and capi.TotalFocusOptions.margin.offset == 24
    assert C.sizeof(capi.TotalFocusPlan) == 80 and capi.TotalFocusPlan.out_width.offset == 56 and capi.TotalFocusPlan.r_use.offset == 64
    assert capi.TotalFocusPlan.max_lenses_per_cell.offset == 72
    assert C.sizeof(capi.TotalFocusResult) == 8 + 3 * 8 + 4 * 8 + 8 and capi.TotalFocusResult.count.offset == 32 and capi.TotalFocusResult.seconds.offset == 64
    # the defaults land where the ctypes view reads them
    plan = total_focus.checkTotalFocus(params("d14"), (160, 200), 8, (160, 200))
    o = plan.options
    assert (o.scale, o.out_width, o.out_height, o.min_lenses, o.white_level) == (1, 200, 160, 1, 255)
    assert (o.margin, o.max_reach, o.iv_min, o.default_iv) == (1.5, 4.0, 0.04, 0.0)
    assert (plan.out_width, plan.out_height) == (200, 160)
    assert total_focus.checkTotalFocus(params("d23_16"), (144, 176), 16, (144, 176)).options.white_level == 65535


def test_argument_errors(built):
    """every check runs before a device is looked for"""
    lib = capi.load_library()
    p = params("d14")
    data = np.zeros(4, np.uint16)

    def image(width=200, height=160, bits=8, pitch=None, ptr=data.ctypes.data):
        return capi.RawDepthImage(ptr, bits, width, height, 0, width if pitch is None else pitch)

    def check(img=None, white=None, depth=(200, 160), prm=p, **o):
        opt = total_focus.make_options(**o)
        img = image() if img is None else img
        return lib.lifcal_totalfocus_check(C.byref(prm) if prm is not None else None, C.byref(img) if img else None, C.byref(white) if white is not None else None,
                                           depth[0], depth[1], C.byref(opt), None)

    assert check() == 0
    assert check(prm=None) == -1
    assert lib.lifcal_totalfocus_check(C.byref(p), None, None, 200, 160, None, None) == -1 and b"no image" in lib.lifcal_ba_last_error()
    assert check(img=image(ptr=None)) == -1
    assert check(img=image(width=201)) == -1 and b"size" in lib.lifcal_ba_last_error()
    assert check(img=image(height=159)) == -1
    assert check(img=image(bits=12)) == -1 and b"bits" in lib.lifcal_ba_last_error()
    assert check(img=image(pitch=199)) == -1 and b"pitch" in lib.lifcal_ba_last_error()
    assert check(img=image(pitch=213)) == 0
    # the white image: same bits, same size
    assert check(white=image()) == 0 and check(white=image(pitch=230)) == 0
    assert check(white=image(bits=16)) == -1 and b"bits" in lib.lifcal_ba_last_error()
    assert check(white=image(width=199)) == -1 and b"white image size" in lib.lifcal_ba_last_error()
    assert check(white=image(ptr=None)) == -1 and check(white=image(pitch=100)) == -1
    # the depth map is the output's size
    assert check(depth=(199, 160)) == -1 and b"depth map size" in lib.lifcal_ba_last_error()
    assert check(depth=(200, 161)) == -1
    assert check(depth=(100, 80), scale=2) == 0 and check(depth=(200, 160), scale=2) == -1
    assert check(depth=(61, 47), out_width=61, out_height=47) == 0
    assert check(scale=-1) == -1 and b"scale" in lib.lifcal_ba_last_error()
    assert check(depth=(1, 1), scale=160) == 0
    assert check(scale=161) == -1 and b"no cells" in lib.lifcal_ba_last_error()
    assert check(out_width=-1) == -1 and check(out_height=-5) == -1
    # the options
    assert check(margin=-0.5) == -1 and b"margin" in lib.lifcal_ba_last_error() and check(margin=float("nan")) == -1
    assert check(margin=5.6) == 0 and check(margin=5.7) == -1 and b"r_use" in lib.lifcal_ba_last_error()       # valid_r = 6.15
    assert check(max_reach=-1.0) == -1 and check(max_reach=8.5) == -1 and check(max_reach=float("nan")) == -1 and b"max_reach" in lib.lifcal_ba_last_error()
    assert check(max_reach=8.0) == 0 and check(max_reach=0.25) == 0
    assert check(iv_min=-0.1) == -1 and check(iv_min=1.5) == -1 and check(iv_min=1e-4) == -1 and check(iv_min=float("nan")) == -1
    assert b"iv_min" in lib.lifcal_ba_last_error()
    assert check(iv_min=1.0) == 0 and check(iv_min=0.001) == 0
    assert check(default_iv=0.03) == -1 and check(default_iv=1.01) == -1 and check(default_iv=-0.2) == -1 and check(default_iv=float("nan")) == -1
    assert b"default_iv" in lib.lifcal_ba_last_error()
    assert check(default_iv=0.04) == 0 and check(default_iv=1.0) == 0 and check(default_iv=0.2, iv_min=0.2) == 0 and check(default_iv=0.1, iv_min=0.2) == -1
    assert check(min_lenses=-1) == -1 and check(min_lenses=256) == -1 and b"min_lenses" in lib.lifcal_ba_last_error()
    assert check(min_lenses=255) == 0
    assert check(white_level=-1) == -1 and check(white_level=256) == -1 and b"white_level" in lib.lifcal_ba_last_error()
    assert check(white_level=255) == 0 and check(img=image(bits=16), white_level=65535) == 0 and check(img=image(bits=16), white_level=65536) == -1
    assert lib.lifcal_totalfocus_check(C.byref(p), C.byref(image()), None, 200, 160, None, None) == 0      # no options: all defaults
    # 2^31 cells are out of range
    assert check(depth=(65536, 32768), out_width=65536, out_height=32768) == -4 and b"2^31" in lib.lifcal_ba_last_error()
    # a lattice with rows so close that 2^18 lenses could reach one cell
    flat = capi.MlaParams(200, 160, 14.3, (C.c_float * 2)(-0.5, 1.0e-4), 0.0, (C.c_float * 2)(0.0, 0.0), 1)
    assert check(prm=flat) == -4 and b"lenses" in lib.lifcal_ba_last_error()
    # the entry point itself refuses a missing grid, depth or result without touching a device
    res = capi.TotalFocusResult()
    iv = np.zeros((160, 200), np.float32)
    assert lib.lifcal_totalfocus_render(None, C.byref(image()), None, iv.ctypes.data, 0, None, C.byref(res)) == -1
    with pytest.raises(LifcalError, match="scale"):
        total_focus.checkTotalFocus(p, (160, 200), 8, (160, 200), scale=-2)
    with pytest.raises(LifcalError, match="depth map size"):
        total_focus.checkTotalFocus(p, (160, 200), 8, (160, 199))
    with pytest.raises(LifcalError, match="white image size"):
        total_focus.checkTotalFocus(p, (160, 200), 8, (160, 200), white_shape=(160, 199))
    with pytest.raises(TypeError):
        total_focus.checkTotalFocus(p, (160, 200), 8, (160, 200), scales=2)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_plan_matches_restatement(built, name):
    w, h, d, _, _, bits = ref.CASES[name][:6]
    for kw in (dict(), dict(scale=2), dict(scale=3, margin=0.5, max_reach=2.5), dict(out_width=77, out_height=301, iv_min=0.25, max_reach=8.0, white_level=100)):
        want = tref.plan(w, h, bits, d, ref.BASE_Y[1], **kw)
        got = total_focus.checkTotalFocus(params(name), (h, w), bits, (want["out_height"], want["out_width"]), **kw)
        assert (got.out_width, got.out_height, got.r_use, got.max_lenses_per_cell) == (want["out_width"], want["out_height"], want["r_use"], want["max_lenses_per_cell"]), (kw, want)
        o = want["options"]
        assert all(getattr(got.options, k) == o[k] for k in tref.DEFAULTS), kw
        # the bound the 64-bit sums rely on: num white_level < max_lenses_per_cell 2^28 2^16 < 2^63
        assert got.max_lenses_per_cell * 4096 * 65535 * 65535 < 2 ** 63
    assert tref.plan(w, h, bits, d, ref.BASE_Y[1])["max_lenses_per_cell"] == 12 * 11


# ---------------------------------------------------------------------------------------------------------------- a hand-made case
HAND = (64, 48, 14.3)


def hand_grid():
    w, h, d = HAND
    cx, cy = white_image.grid_centres(w, h, d, ref.BASE_Y, 0.0, (0.0, 0.0), 1.5)
    return cx.astype(np.float32), cy.astype(np.float32)


def test_restatement_rules_on_a_hand_made_case():
    """the rules of the header on a 64 x 48 grid with d = 14.3 (valid_r = 6.15, r_use = 4.65)"""
    w, h, d = HAND
    cx, cy = hand_grid()
    iv = np.full((h, w), 0.25, np.float32)
    # a constant grey comes back exactly: (2 * 4096 n g + 4096 n) / (2 * 4096 n) = g
    grey = np.full((h, w), 93, np.uint8)
    tf = tref.render(grey, iv, cx, cy, d)
    assert np.all(tf.image[tf.status == 0] == 93) and tf.counts[0] > 0.95 * w * h and int(tf.counts.sum()) == w * h
    assert not np.any(tf.status == 1) and not np.any(tf.status == 3) and np.all(tf.image[tf.status == 2] == 0)
    assert np.all((tf.n_lenses >= 1) == (tf.status == 0))
    # at v = 4 a cell is seen by the lenses within 4 * 4.65 = 18.6 px: about pi 18.6^2 / (0.866 d^2) = 6
    inner = tf.n[16:-16, 16:-16]                 # the pictures lie within 14 px of the cell: these cells lose none to the border
    assert 3 <= inner.min() and inner.max() <= 9 and abs(inner.mean() - np.pi * 18.6 ** 2 / (0.8660254 * d * d)) < 0.5
    # one lens by hand: the cell (30, 20) and the lens nearest to it
    j = int(np.argmin((cx.astype(np.float64) - 30.0) ** 2 + (cy.astype(np.float64) - 20.0) ** 2))
    ramp = (np.arange(w)[None, :] * 3 + np.arange(h)[:, None]).astype(np.uint8)           # I(x, y) = 3 x + y <= 236
    one = tref.render(ramp, iv, cx[j:j + 1], cy[j:j + 1], d)
    px = float(cx[j]) + (30.0 - float(cx[j])) * 0.25; py = float(cy[j]) + (20.0 - float(cy[j])) * 0.25
    Sx, Sy = int(np.floor(64.0 * px + 0.5)), int(np.floor(64.0 * py + 0.5))
    assert one.status[20, 30] == 0 and one.n[20, 30] == 1
    # bilinear interpolation of a linear image is the image at the rounded position: (3 Sx + Sy) / 64, rounded half up
    assert one.image[20, 30] == (2 * (3 * Sx + Sy) * 64 + 4096) // (2 * 4096)
    # devignetting: image = white k / white_level, rounded, comes back as k to within one grey level
    tx, ty = white_image.grid_centres(w, h, d, ref.BASE_Y, 0.0, (0.0, 0.0), 1.5)
    white = white_image.render_white_image(w, h, tx, ty, d, **tref.WHITE)
    k, wl = 150, 204
    shaded = np.floor(white.astype(np.float64) * k / wl + 0.5).astype(np.uint8)
    tw = tref.render(shaded, iv, cx, cy, d, white=white, white_level=wl)
    ok = tw.status == 0
    assert ok.sum() > 0.95 * w * h and np.abs(tw.image[ok].astype(int) - k).max() <= 1
    plain = tref.render(shaded, iv, cx, cy, d)
    assert np.abs(plain.image[plain.status == 0].astype(int) - k).max() > 20                # without the white image the shading stays
    # a white image that is dark wherever the cell looks: den = 0, status 2 with the count kept
    dark = tref.render(shaded, iv, cx, cy, d, white=np.zeros_like(white))
    assert np.all(dark.status == 2) and np.array_equal(dark.n, tf.n) and not dark.image.any()
    # the clamp at full scale
    bright = tref.render(np.full((h, w), 255, np.uint8), iv, cx, cy, d, white=np.full((h, w), 100, np.uint8), white_level=255)
    assert np.all(bright.image[bright.status == 0] == 255)
    # no depth: NaN, below iv_min, above 1
    holes = iv.copy(); holes[20, 30] = np.nan; holes[21, 30] = 0.03; holes[22, 30] = 1.5
    th = tref.render(grey, holes, cx, cy, d)
    assert th.status[20:23, 30].tolist() == [1, 1, 1] and th.image[20:23, 30].tolist() == [0, 0, 0] and th.n_lenses[20:23, 30].tolist() == [0, 0, 0]
    assert th.counts.tolist() == [tf.counts[0] - 3, 3, tf.counts[2], 0]
    td = tref.render(grey, holes, cx, cy, d, default_iv=0.25)
    assert td.status[20:23, 30].tolist() == [3, 3, 3] and td.image[20:23, 30].tolist() == [93, 93, 93] and np.array_equal(td.n, tf.n)
    assert td.counts.tolist() == [tf.counts[0] - 3, 0, tf.counts[2], 3]
    # min_lenses above the n of a cell: status 2 with n_lenses kept
    few = tref.render(grey, iv, cx, cy, d, min_lenses=6)
    assert np.array_equal(few.n, tf.n) and np.array_equal(few.status == 2, tf.n < 6) and np.array_equal(few.n_lenses, tf.n_lenses)
    assert 0 < (few.status == 2).sum() < w * h and not few.image[few.status == 2].any() and np.all(few.image[few.status == 0] == 93)
    # max_reach caps the lenses of a far cell: at v = 10 the disc test alone admits 46.5 px (every lens of this small grid whose
    # picture falls into the image), max_reach 1 only d = 14.3 px: a lens and its six neighbours at most
    far = np.full((h, w), 0.1, np.float32)
    wide, capped = tref.render(grey, far, cx, cy, d, max_reach=8.0), tref.render(grey, far, cx, cy, d, max_reach=1.0)
    assert wide.n[24, 32] > 15 and 1 <= capped.n[24, 32] <= 7
    lens_distance = np.hypot(cx.astype(np.float64) - 32.0, cy.astype(np.float64) - 24.0)
    assert capped.n[24, 32] == int((lens_distance <= d).sum())


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_accuracy_with_true_depth(built, name):
    """the restatement against the truth with the TRUE depth, every scene, scale 1 and 2, noise 0 and NOISE: the issue's conditions
    (every interior cell has status 0 and a lens; registration) hold, and the RMS stays within the recorded figure, whose double is
    the bar of the GPU tests"""
    gd = oracle_grid(name)
    for scn in ref.SCENE_NAMES:
        for noise in (0.0, ref.NOISE):
            for scale in tref.SCALES:
                tf = tref.run_true(name, scn, noise, gd, scale)
                a = tref.accuracy(name, scn, tf, scale)
                print(f"{name} {scn} noise {noise} scale {scale} true depth: {tref.describe(a)}; counts {tf.counts.tolist()}")
                assert a["share"] == 1.0 and a["min_lenses"] >= 1, (scn, noise, scale, a)
                tref.check_registration(a, (name, scn, noise, scale))
                assert a["rms"] <= tref.MEASURED[name]["rms"], (scn, noise, scale, a)
                assert int(tf.counts.sum()) == tf.status.size


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_accuracy_with_chained_depth(built, name):
    """the same from the depth map of the restatement chain (raw-depth restatement with 18 neighbours, then the depth-map
    restatement), with noise: a cell of the interior has status 0 exactly where the depth map has a value.  (The recorded figures
    are the largest over noise 0 and NOISE; this test runs the noisy half, which the depth-map tests compute anyway.)"""
    gd = oracle_grid(name)
    for scn in ref.SCENE_NAMES:
        for scale in tref.SCALES:
            tf, dm = tref.run_chained(name, scn, ref.NOISE, gd, scale)
            a = tref.accuracy(name, scn, tf, scale)
            inner = tref.interior(name, scn, scale)
            print(f"{name} {scn} scale {scale} chained depth: {tref.describe(a)}; counts {tf.counts.tolist()}")
            assert np.array_equal(inner & (tf.status == 0), inner & (dm.status <= 1)), (scn, scale)
            tref.check_registration(a, (name, scn, scale))
            assert a["rms"] <= tref.MEASURED[name]["rms"], (scn, scale, a)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_restatement_uses_the_white_image(built, name):
    """the vignetted raw image with its white image is as close to the truth as the unshaded one (within the same bar); without the
    white image it is not"""
    gd = oracle_grid(name)
    for scn in ("mid", "step"):
        tw = tref.run_true(name, scn, ref.NOISE, gd, 1, white=True)
        aw = tref.accuracy(name, scn, tw, 1)
        plain = tref.render(tref.vignetted_case(name, scn, ref.NOISE), tref.true_depth(name, scn, 1), gd.cx, gd.cy, ref.CASES[name][2])
        ap = tref.accuracy(name, scn, plain, 1)
        print(f"{name} {scn}: with the white image {tref.describe(aw)}; without it rms {ap['rms']:.5f}")
        assert aw["share"] == 1.0 and aw["rms"] <= tref.MEASURED[name]["rms"], (scn, aw)
        tref.check_registration(aw, (name, scn))
        assert ap["rms"] > tref.BARS[name]["rms"], (scn, ap)


@pytest.mark.parametrize("name", list(ref.GEOMETRY_CASES))
def test_restatement_accuracy_on_other_geometries(built, name):
    """the twin of the two accuracy tests above on the rotated, the squeezed and the rotation-off-grid lattice of
    rawdepth_reference.GEOMETRY_CASES, with the true depth and with the depth map of the restatement chain, at noise 0 and NOISE:
    this is where MEASURED of these cases is measured"""
    gd = oracle_grid(name)
    for scn in ref.SCENE_NAMES:
        for noise in (0.0, ref.NOISE):
            for scale in tref.SCALES:
                tf = tref.run_true(name, scn, noise, gd, scale)
                a = tref.accuracy(name, scn, tf, scale)
                print(f"{name} {scn} noise {noise} scale {scale} true depth: {tref.describe(a)}; counts {tf.counts.tolist()}")
                assert a["share"] == 1.0 and a["min_lenses"] >= 1, (scn, noise, scale, a)
                tref.check_registration(a, (name, scn, noise, scale))
                assert a["rms"] <= tref.MEASURED[name]["rms"], (scn, noise, scale, a)
                tf, dm = tref.run_chained(name, scn, noise, gd, scale)
                a = tref.accuracy(name, scn, tf, scale)
                inner = tref.interior(name, scn, scale)
                print(f"{name} {scn} noise {noise} scale {scale} chained depth: {tref.describe(a)}; counts {tf.counts.tolist()}")
                assert np.array_equal(inner & (tf.status == 0), inner & (dm.status <= 1)), (scn, noise, scale)
                tref.check_registration(a, (name, scn, noise, scale))
                assert a["rms"] <= tref.MEASURED[name]["rms"], (scn, noise, scale, a)
