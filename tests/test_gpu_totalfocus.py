"""The total-focus image on the GPU (include/lifcal_totalfocus.h): lifcal_totalfocus_render against the numpy
restatement byte for byte, against itself across calls and pointer kinds, at its edges, and from the raw image to the picture
against the texture the scenes were rendered from."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lifcal_amd import LifcalError, MicroLensGrid, _capi as capi, total_focus
from tests import depthmap_reference as dref
from tests import rawdepth_reference as ref
from tests import totalfocus_reference as tref

pytestmark = pytest.mark.gpu

_GRIDS = {}
FIELDS = ("image", "n_lenses", "status")


def case(name):
    """(grid, its data for the restatements), made once per case"""
    if name not in _GRIDS:
        g = MicroLensGrid(*ref.grid_arguments(name))
        _GRIDS[name] = (g, ref.grid_data(name, g))
    return _GRIDS[name]


def handed_over(name, img, extra=None):
    """an image as the case hands it over: d9_pitch in host rows wider than the image"""
    extra = ref.CASES[name][7] if extra is None else extra
    if not extra:
        return img
    wide = np.full((img.shape[0], img.shape[1] + extra), 255, img.dtype)   # bright columns the kernel must never read
    wide[:, :img.shape[1]] = img
    view = wide[:, :img.shape[1]]
    assert view.strides[0] == wide.shape[1] * img.itemsize
    return view


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equals_restatement(got, want, what):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero(a.ravel() != b.ravel())
        assert bad.size == 0, (what, f, bad.size, bad[:8], a.ravel()[bad[:8]], b.ravel()[bad[:8]])
    assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == got.status.size, (what, got.counts, want.counts)


@pytest.mark.parametrize("scale", tref.SCALES)
@pytest.mark.parametrize("name", list(ref.CASES))
def test_equals_restatement(built, name, scale):
    """image, n_lenses, status and the counts with the TRUE depth at the cell centres: the mid scene and the step scene (two
    depths, so two reaches in one tile), with noise, without and with a white image"""
    g, gd = case(name)
    for scn in tref.EQUALITY_SCENES:
        iv = tref.true_depth(name, scn, scale)
        want = tref.run_true(name, scn, ref.NOISE, gd, scale)
        got = g.totalFocusImage(handed_over(name, ref.make_case(name, scn, ref.NOISE)), iv, scale=scale)
        print(f"{name} {scn} scale {scale}: counts {got.counts.tolist()}, {got.seconds * 1e3:.3f} ms")
        assert got.scale == scale and got.status.shape == tref.out_shape(name, scale)
        assert_equals_restatement(got, want, (name, scn, scale))
        assert want.counts[0] > 0.95 * want.status.size and want.n.max() > 1          # the comparison is of real pictures
        want = tref.run_true(name, scn, ref.NOISE, gd, scale, white=True)
        got = g.totalFocusImage(handed_over(name, tref.vignetted_case(name, scn, ref.NOISE)), iv, white=handed_over(name, tref.white_case(name), 7),
                                scale=scale, white_level=tref.white_level(name))
        assert_equals_restatement(got, want, (name, scn, scale, "white"))
        assert want.counts[0] > 0.95 * want.status.size


@pytest.mark.parametrize("name", list(ref.CASES))
def test_equals_restatement_on_the_chained_depth_map(built, name):
    """once per case, the depth map of the restatement chain (raw-depth restatement with 18 neighbours, then the depth-map
    restatement): the near scene, whose map has cells without a value"""
    g, gd = case(name)
    want, dm = tref.run_chained(name, "near", ref.NOISE, gd, 1)
    got = g.totalFocusImage(handed_over(name, ref.make_case(name, "near", ref.NOISE)), dm.inv_depth)
    assert_equals_restatement(got, want, name)
    assert want.counts[0] > 0 and want.counts[1] > 0 and np.array_equal(got.status == 1, np.isnan(dm.inv_depth))


@pytest.mark.parametrize("name", list(ref.CASES))
def test_reach_cap_and_default_depth(built, name):
    """max_reach 1.0 on the far scene, where the disc test alone admits v r_use > d: the cap bites; default_iv on a map with NaN
    cells, without and with a white image; min_lenses above what some cells have"""
    g, gd = case(name)
    d = ref.CASES[name][2]
    img = ref.make_case(name, "far", ref.NOISE)
    iv = tref.true_depth(name, "far", 2)
    free = tref.run_true(name, "far", ref.NOISE, gd, 2)
    want = tref.render(img, iv, gd.cx, gd.cy, d, scale=2, max_reach=1.0)
    assert_equals_restatement(g.totalFocusImage(handed_over(name, img), iv, scale=2, max_reach=1.0), want, (name, "max_reach"))
    assert want.counts[0] > 0 and want.n.max() < free.n.max() and 0 < want.n.max() <= 7     # a lens and its six neighbours at most
    holes = np.array(tref.true_depth(name, "mid", 2))
    holes[5:40, 10:30] = np.nan; holes[::7, ::5] = np.nan; holes[3, :] = 0.01; holes[:, 2] = 1.25
    img = ref.make_case(name, "mid", ref.NOISE)
    for kw in (dict(), dict(default_iv=0.25), dict(default_iv=0.125, min_lenses=9)):
        want = tref.render(img, holes, gd.cx, gd.cy, d, scale=2, **kw)
        assert_equals_restatement(g.totalFocusImage(handed_over(name, img), holes, scale=2, **kw), want, (name, kw))
        assert (want.counts[1] > 0) == (not kw) and (want.counts[3] > 0) == bool(kw) and want.counts[0] + want.counts[3] > 0
    assert want.counts[2] > 0        # min_lenses 9 leaves cells of the mid scene without a pixel
    want = tref.render(tref.vignetted_case(name, "mid", ref.NOISE), holes, gd.cx, gd.cy, d, white=tref.white_case(name), scale=2, default_iv=0.25)
    got = g.totalFocusImage(tref.vignetted_case(name, "mid", ref.NOISE), holes, white=tref.white_case(name), scale=2, default_iv=0.25)
    assert_equals_restatement(got, want, (name, "default_iv with a white image"))


@pytest.mark.parametrize("name", list(ref.CASES))
def test_same_bytes_across_calls(built, name):
    """two calls give the same bytes; the outputs are optional"""
    g, _ = case(name)
    img = np.ascontiguousarray(ref.make_case(name, "step", ref.NOISE))
    white = np.ascontiguousarray(tref.white_case(name))
    iv = np.ascontiguousarray(tref.true_depth(name, "step", 1))
    first = g.totalFocusImage(img, iv, white=white)
    again = g.totalFocusImage(img, iv, white=white)
    for f in FIELDS:
        assert same_bytes(getattr(first, f), getattr(again, f)), f
    assert np.array_equal(first.counts, again.counts) and first.seconds > 0 and first.counts[0] > 0
    lib = capi.load_library()
    h, w = img.shape
    bits = 8 * img.itemsize
    out = np.full(first.image.shape, 9, first.image.dtype)
    res = capi.TotalFocusResult(); res.image = out.ctypes.data
    ci = capi.RawDepthImage(img.ctypes.data, bits, w, h, 0, w); cw = capi.RawDepthImage(white.ctypes.data, bits, w, h, 0, w)
    assert lib.lifcal_totalfocus_render(g._h, C.byref(ci), C.byref(cw), iv.ctypes.data, 0, None, C.byref(res)) == 0
    assert same_bytes(out, first.image) and list(res.count) == first.counts.tolist()


def test_device_pointers_through_torch_tensors(built):
    """image, white image and depth handed over as torch tensors on the device and the maps written into torch tensors give the
    bytes of the host-pointer path, and VirtualDepthMap.total_focus runs device to device.  Of two HIP runtimes in one process only
    the first to start sees the GPU; this process has the library's running already, so the check runs in a fresh one."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "totalfocus_device_pointers.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "device pointers ok" in p.stdout


def test_all_nan_depth_is_all_status_one(built):
    g, _ = case("d14")
    w, h = ref.CASES["d14"][:2]
    got = g.totalFocusImage(ref.make_case("d14", "mid"), np.full((h // 2, w // 2), np.nan, np.float32), scale=2)
    n = (w // 2) * (h // 2)
    assert got.counts.tolist() == [0, n, 0, 0] and np.all(got.status == 1) and not got.image.any() and not got.n_lenses.any()


def test_output_sizes_other_than_the_default(built):
    """a smaller output is the top-left part of the picture; in a larger one the cells beyond the lenses' reach have no lens"""
    name = "d14"
    g, gd = case(name)
    w, h, d = ref.CASES[name][:3]
    img = ref.make_case(name, "step", ref.NOISE)
    depth = ref.scene_depth(name, "step")
    for ow, oh in ((61, 47), (w + 64, h + 64)):
        xu, yu = tref.cell_centres(ow, oh, 1)
        iv = (1.0 / depth(xu, yu)).astype(np.float32)
        got = g.totalFocusImage(img, iv, out_width=ow, out_height=oh)
        assert got.status.shape == (oh, ow)
        assert_equals_restatement(got, tref.render(img, iv, gd.cx, gd.cy, d, out_width=ow, out_height=oh), (ow, oh))
        assert got.counts[0] > 0
    # r_use v = 4.65 * 5.5 = 25.6 px beyond the last lens that shows in the image, whose centre lies within d / 2 of its edge
    assert np.all(got.status[:, w + 40:] == 2) and np.all(got.status[h + 40:, :] == 2) and not got.n_lenses[:, w + 40:].any()
    full = g.totalFocusImage(img, tref.true_depth(name, "step", 1))
    small = g.totalFocusImage(img, tref.true_depth(name, "step", 1)[:47, :61], out_width=61, out_height=47)
    assert same_bytes(small.image, np.ascontiguousarray(full.image[:47, :61]))


def test_scale_that_does_not_divide_the_image(built):
    name = "d9_pitch"                       # 203 x 131
    g, gd = case(name)
    img = ref.make_case(name, "step", ref.NOISE)
    xu, yu = tref.cell_centres(67, 43, 3)
    iv = (1.0 / ref.scene_depth(name, "step")(xu, yu)).astype(np.float32)
    got = g.totalFocusImage(handed_over(name, img), iv, scale=3)
    assert got.status.shape == (43, 67) and got.scale == 3
    assert_equals_restatement(got, tref.render(img, iv, gd.cx, gd.cy, ref.CASES[name][2], scale=3), "scale 3")
    assert got.counts[0] > 0.95 * 43 * 67


def test_depth_of_the_wrong_size_is_refused(built):
    g, _ = case("d14")
    img = ref.make_case("d14", "mid")
    with pytest.raises(LifcalError, match="depth map size"):
        g.totalFocusImage(img, np.full((160, 199), 0.25, np.float32))
    with pytest.raises(LifcalError, match="depth map size"):
        g.totalFocusImage(img, np.full((160, 200), 0.25, np.float32), scale=2)
    with pytest.raises(LifcalError, match="white image"):
        g.totalFocusImage(img, np.full((160, 200), 0.25, np.float32), white=np.zeros((160, 200), np.uint16))
    with pytest.raises(TypeError):
        g.totalFocusImage(img, np.full((160, 200), 0.25, np.float32), min_lens=2)
    with pytest.raises(TypeError):
        total_focus.totalFocusImage(g, img, np.full((160, 200), 0.25, np.float32), scales=2)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_accuracy_with_true_depth(built, name):
    """every scene at noise 0 and NOISE, scale 1 and 2, with the true depth: every interior cell has status 0 and a lens
    (condition 1), the picture is registered to better than a cell (condition 2), and the RMS against the texture stays within the
    bar, twice the restatement's measured figure (condition 3)"""
    g, _ = case(name)
    bar = tref.BARS[name]["rms"]
    for scn in ref.SCENE_NAMES:
        for noise in (0.0, ref.NOISE):
            img = handed_over(name, ref.make_case(name, scn, noise))
            for scale in tref.SCALES:
                a = tref.accuracy(name, scn, g.totalFocusImage(img, tref.true_depth(name, scn, scale), scale=scale), scale)
                print(f"{name} {scn} noise {noise} scale {scale} true depth: {tref.describe(a)}")
                assert a["share"] == 1.0 and a["min_lenses"] >= 1, (scn, noise, scale, a)
                tref.check_registration(a, (name, scn, noise, scale))
                assert a["rms"] <= bar, (scn, noise, scale, a, bar)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_accuracy_from_the_raw_image_alone(built, name):
    """estimateRawDepth, depth_map() and total_focus() on every scene at noise 0 and NOISE, scale 1 and 2: the interior cells with
    status 0 are those the depth map has a value for (condition 4; section 7u's conditions bound their share from below),
    registration, and the RMS within the same bar"""
    g, _ = case(name)
    bar = tref.BARS[name]["rms"]
    for scn in ref.SCENE_NAMES:
        for noise in (0.0, ref.NOISE):
            img = handed_over(name, ref.make_case(name, scn, noise))
            est = g.estimateRawDepth(img, patch_radius=ref.CASES[name][6], max_baseline=dref.MAX_BASELINE)
            for scale in tref.SCALES:
                dm = est.depth_map(scale=scale)
                tf = dm.total_focus(g, img)
                a = tref.accuracy(name, scn, tf, scale)
                inner = tref.interior(name, scn, scale)
                print(f"{name} {scn} noise {noise} scale {scale} chained: {tref.describe(a)}")
                assert tf.scale == scale and np.array_equal(inner & (tf.status == 0), inner & (dm.status <= 1)), (scn, noise, scale)
                tref.check_registration(a, (name, scn, noise, scale))
                assert a["rms"] <= bar, (scn, noise, scale, a, bar)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_white_image_is_used(built, name):
    """the raw image shaded by a white image with fall-off and vignetting: with that white image passed the RMS against the
    texture stays within the same bar (condition 5); the same input without it exceeds the bar"""
    g, _ = case(name)
    bar = tref.BARS[name]["rms"]
    for scn in ("mid", "step"):
        img, iv = tref.vignetted_case(name, scn, ref.NOISE), tref.true_depth(name, scn, 1)
        aw = tref.accuracy(name, scn, g.totalFocusImage(img, iv, white=tref.white_case(name), white_level=tref.white_level(name)), 1)
        ap = tref.accuracy(name, scn, g.totalFocusImage(img, iv), 1)
        print(f"{name} {scn}: with the white image {tref.describe(aw)}; without it rms {ap['rms']:.5f}; bar {bar:.5f}")
        assert aw["share"] == 1.0 and aw["rms"] <= bar, (scn, aw, bar)
        tref.check_registration(aw, (name, scn))
        assert ap["rms"] > bar, (scn, ap, bar)
