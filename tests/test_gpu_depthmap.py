"""The virtual-image depth map from the raw-pixel depth on the GPU (include/lifcal_depthmap.h):
lifcal_depthmap_from_raw against the numpy restatement byte for byte, against itself across calls and pointer kinds, at its
edges, through the consumers of include/lifcal_depth.h, and from the raw image to the map against the true depth."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lifcal_amd import MicroLensGrid, _capi as capi, depth, depth_map, scene
from tests import depthmap_reference as dref
from tests import rawdepth_reference as ref

pytestmark = pytest.mark.gpu

_GRIDS = {}
FIELDS = ("inv_depth", "depth16", "status", "support")


def case(name):
    """(grid, its data for the restatements), made once per case"""
    if name not in _GRIDS:
        g = MicroLensGrid(*ref.grid_arguments(name))
        _GRIDS[name] = (g, ref.grid_data(name, g))
    return _GRIDS[name]


def raw_depth_of(name, scn, noise=ref.NOISE):
    """the raw-depth restatement's inv_depth: the comparison does not depend on the sweep kernel"""
    _, gd = case(name)
    return ref.run(name, scn, noise, gd, max_baseline=dref.MAX_BASELINE).inv_depth


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equals_restatement(got, want, what):
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, a.shape, b.shape)
        bits = "u%d" % a.itemsize
        bad = np.flatnonzero(a.ravel().view(bits) != b.ravel().view(bits))
        assert bad.size == 0, (what, f, bad.size, bad[:8], a.ravel()[bad[:8]], b.ravel()[bad[:8]])
    assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == got.status.size, (what, got.counts, want.counts)
    assert got.n_samples == want.n_samples, what


@pytest.mark.parametrize("scale", dref.SCALES)
@pytest.mark.parametrize("name", list(ref.CASES))
def test_equals_restatement(built, name, scale):
    """all four maps, the counts and n_samples: the step scene (two depths and an occlusion edge) and the near scene (sparse, so
    rejection and fill both happen), with noise"""
    g, gd = case(name)
    for scn in ("step", "near"):
        want = dref.run(name, scn, ref.NOISE, gd, scale)
        got = depth_map.depthMapFromRaw(g, raw_depth_of(name, scn), scale=scale)
        print(f"{name} {scn} scale {scale}: counts {got.counts.tolist()}, {got.n_samples} samples, {got.seconds * 1e3:.3f} ms")
        assert got.scale == scale and got.status.shape == (ref.CASES[name][1] // scale, ref.CASES[name][0] // scale)
        assert_equals_restatement(got, want, (name, scn, scale))
        assert want.counts[0] > 0 and (scn != "near" or (want.counts[1] > 0 and want.counts[3] > 0))   # the comparison is of real maps


@pytest.mark.parametrize("name", list(ref.CASES))
def test_same_bytes_across_calls(built, name):
    """two calls give the same bytes; the outputs are optional"""
    g, _ = case(name)
    iv = raw_depth_of(name, "near")
    first = depth_map.depthMapFromRaw(g, iv)
    again = depth_map.depthMapFromRaw(g, iv)
    for f in FIELDS:
        assert same_bytes(getattr(first, f), getattr(again, f)), f
    assert np.array_equal(first.counts, again.counts) and first.n_samples == again.n_samples and first.seconds > 0 and first.counts[0] > 0
    lib = capi.load_library()
    src = np.ascontiguousarray(iv, np.float32)
    st = np.full(first.status.shape, 9, np.uint8)
    res = capi.DepthMapResult(); res.status = st.ctypes.data
    assert lib.lifcal_depthmap_from_raw(g._h, src.ctypes.data, 0, None, C.byref(res)) == 0
    assert same_bytes(st, first.status) and list(res.count) == first.counts.tolist() and res.n_samples == first.n_samples


def test_device_pointers_through_torch_tensors(built):
    """inv_depth handed over as a torch tensor on the device and the maps written into torch tensors give the bytes of the
    host-pointer path, and to_depth_maps copies device to device.  Of two HIP runtimes in one process only the first to start
    sees the GPU; this process has the library's running already, so the check runs in a fresh one."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "depthmap_device_pointers.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "device pointers ok" in p.stdout


def test_all_nan_input_is_all_empty(built):
    g, _ = case("d14")
    w, h = ref.CASES["d14"][:2]
    got = depth_map.depthMapFromRaw(g, np.full((h, w), np.nan, np.float32), scale=2)
    n = (w // 2) * (h // 2)
    assert got.counts.tolist() == [0, 0, n, 0] and got.n_samples == 0
    assert np.all(got.status == 2) and np.all(np.isnan(got.inv_depth)) and not got.depth16.any() and not got.support.any()


def test_output_sizes_other_than_the_default(built):
    """a smaller output clips the footprints; in a larger one the cells no footprint reaches are empty.  With iv_min = 0.125 a
    sample of d14 (valid_r = 6.15) lies at most 7 valid_r = 43.05 beyond its pixel and covers at most 4 cells more."""
    name = "d14"
    g, gd = case(name)
    w, h = ref.CASES[name][:2]
    iv = raw_depth_of(name, "step")
    for ow, oh in ((61, 47), (w + 64, h + 64)):
        kw = dict(out_width=ow, out_height=oh, iv_min=0.125)
        got = depth_map.depthMapFromRaw(g, iv, **kw)
        assert got.status.shape == (oh, ow)
        assert_equals_restatement(got, dref.depth_map(iv, gd.map_ml, gd.cx, gd.cy, **kw), (ow, oh))
        assert got.counts[0] > 0
    assert np.all(got.status[:, w + 48:] == 2) and np.all(got.status[h + 48:, :] == 2)


def test_min_support_one_without_fill(built):
    name = "d9_pitch"
    g, gd = case(name)
    iv = raw_depth_of(name, "near")
    kw = dict(min_support=1, fill_rounds=-1)
    got = depth_map.depthMapFromRaw(g, iv, **kw)
    assert got.counts[1] == 0 and got.counts[3] == 0 and got.counts[0] > 0 and got.counts[2] > 0
    assert not np.any(got.status == 1) and not np.any(got.status == 3)
    assert_equals_restatement(got, dref.depth_map(iv, gd.map_ml, gd.cx, gd.cy, **kw), kw)


def test_scale_that_does_not_divide_the_image(built):
    name = "d9_pitch"                       # 203 x 131
    g, gd = case(name)
    iv = raw_depth_of(name, "step")
    got = depth_map.depthMapFromRaw(g, iv, scale=3)
    assert got.status.shape == (43, 67)
    assert_equals_restatement(got, dref.depth_map(iv, gd.map_ml, gd.cx, gd.cy, scale=3), "scale 3")
    assert got.counts[0] > 0.9 * 43 * 67


def test_round_trip_through_the_sampler(built):
    """to_depth_maps then lifcal_depth_sample at the integer cells: every cell with a depth16 comes back as 1 / iv' with
    |iv' - q_cell / Q| <= 0.5 / 65535 (the encoding's half step) + 2^-21 (the rounding of the float map, far above its 2^-25);
    every other cell takes the interpolation or the failed route"""
    name = "d14"
    g, gd = case(name)
    got = depth_map.depthMapFromRaw(g, raw_depth_of(name, "near"))
    oh, ow = got.status.shape
    with depth.DepthMaps(ow, oh, 1) as dm:
        got.to_depth_maps(dm, 0)
        Y, X = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
        vd, counts = dm.sample(X.ravel(), Y.ravel(), 0)
    vd = vd.reshape(oh, ow)
    direct = got.depth16 > 0
    assert not np.any(direct & (got.status > 1)) and direct.sum() > 0.9 * (got.status <= 1).sum()
    assert counts.direct == int(direct.sum()) > 0 and counts.direct + counts.interpolated + counts.failed == ow * oh
    assert counts.interpolated + counts.failed == int((~direct).sum()) > 0
    err = np.abs(1.0 / vd[direct] - got.inv_depth[direct].astype(np.float64))
    print(f"{int(direct.sum())} direct cells, {counts.interpolated} interpolated, {counts.failed} failed; largest |iv' - iv| {err.max():.3e}")
    assert err.max() <= 0.5 / 65535 + 2.0 ** -21


def test_back_projection_of_the_map(built):
    """lifcal_depth_back_project_maps on a mid plane through the camera of scene.baseline_spec("tiny"): a finite z at exactly the
    cells with depth16 > 0"""
    name = "d14"
    g, gd = case(name)
    got = depth_map.depthMapFromRaw(g, raw_depth_of(name, "mid"), fill_rounds=-1)
    oh, ow = got.status.shape
    spec = scene.baseline_spec("tiny")
    cam = np.zeros(17); cam[:5] = [spec.fL, spec.bL0, spec.B, 0.5 * (ow - 1), 0.5 * (oh - 1)]
    with depth.DepthMaps(ow, oh, 1) as dm:
        got.to_depth_maps(dm, 0)
        bp = dm.backProjectMaps(cam, 0, spec.pixel_size * spec.scale, want_xyz=False, want_z=True)
    z = bp.z[0]
    assert np.array_equal(np.isfinite(z), got.depth16 > 0) and bp.n_invalid == int((got.depth16 == 0).sum())
    assert 0 < bp.n_invalid < 0.1 * ow * oh
    z_of = lambda iv: spec.fL * (spec.bL0 + spec.B / iv) / ((spec.bL0 + spec.B / iv) - spec.fL)
    ok = got.depth16 > 0
    assert np.allclose(z[ok], z_of(1.0 - got.depth16[ok] / 65535.0), rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", list(ref.CASES))
def test_end_to_end_against_true_depth(built, name):
    """estimateRawDepth then depth_map() on every scene at noise 0 and NOISE, scale 1 and 2: inlier RMS and |median e| within the
    bars (twice the restatement's measured figures), and the issue's conditions on measured share, covered share, outliers and the
    step's band"""
    g, _ = case(name)
    bars = dref.BARS[name]
    for scn in ref.SCENE_NAMES:
        for noise in (0.0, ref.NOISE):
            img = np.array(ref.make_case(name, scn, noise))
            est = g.estimateRawDepth(img, patch_radius=ref.CASES[name][6], max_baseline=dref.MAX_BASELINE)
            for scale in dref.SCALES:
                a = dref.accuracy(name, scn, est.depth_map(scale=scale), scale)
                print(f"{name} {scn} noise {noise} scale {scale}: {dref.describe(a)}")
                dref.check_conditions(scn, a)
                assert a["rms"] <= bars["rms"] and a["median"] <= bars["median"], (scn, noise, scale, a, bars)
