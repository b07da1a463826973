"""The image chain on lattices other than the one of rawdepth_reference.CASES (DESIGN.md sections 7t to 7v): raw depth, the
virtual-image depth map and the total-focus image on a grid rotated by 0.03 rad, on a squeezed lattice whose six nearest
neighbours are not equidistant, and on a grid whose rotation is not the lattice's (rawdepth_reference.GEOMETRY_CASES).  Each stage
against its numpy restatement byte for byte, raw depth and the whole chain against the true depth and texture of the rendered
scenes.  The kernel's neighbour tables and the restatement's are built the same way; what tells a wrong rotation convention is
the true depth of an image rendered through white_image.grid_centres (tests/test_rawdepth_cpu.py shows that these grids can
tell and that the grids of CASES cannot)."""
import numpy as np
import pytest

from lifcal_amd import MicroLensGrid, depth_map, white_image
from tests import depthmap_reference as dref
from tests import rawdepth_reference as ref
from tests import totalfocus_reference as tref

pytestmark = pytest.mark.gpu

_GRIDS = {}
NAMES = list(ref.GEOMETRY_CASES)


def case(name):
    """(grid, its data for the restatements), made once per case"""
    if name not in _GRIDS:
        g = MicroLensGrid(*ref.grid_arguments(name))
        _GRIDS[name] = (g, ref.grid_data(name, g))
    return _GRIDS[name]


def estimate(name, scn, noise, **opts):
    g, _ = case(name)
    return g.estimateRawDepth(ref.make_case(name, scn, noise), patch_radius=ref.case(name)[6], **opts)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_maps(got, want, fields, what):
    for f in fields:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        bits = "u%d" % a.itemsize
        bad = np.flatnonzero(a.ravel().view(bits) != b.ravel().view(bits))
        assert bad.size == 0, (what, f, bad.size, bad[:8], a.ravel()[bad[:8]], b.ravel()[bad[:8]])
    assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == got.status.size, (what, got.counts, want.counts)


@pytest.mark.parametrize("name", NAMES)
def test_lenses_lie_on_the_rendered_lattice(built, name):
    """the case is not vacuous: the library's lens centres lie where the image was rendered, for d14_rot_off on the UNROTATED
    lattice whatever its rotation says (float centres against double ones: 1.4e-5 px on the CPU oracle's grid)"""
    _, gd = case(name)
    w, h, d, _, off, _, _, _, base_y, on_grid = ref.case(name)
    tx, ty = white_image.grid_centres(w, h, d, base_y, ref.grid_rotation(name), off, 1.5)
    dist = np.hypot(gd.cx.astype(np.float64)[:, None] - tx[None, :], gd.cy.astype(np.float64)[:, None] - ty[None, :]).min(axis=1)
    print(f"{name}: {len(gd.cx)} lenses, at most {dist.max():.2e} px from the rendered lattice, sub-grids {np.bincount(gd.sub).tolist()}")
    assert dist.max() < 1e-3 and (on_grid or ref.case(name)[3] != 0.0)
    assert np.bincount(gd.sub).min() > 0.4 * len(gd.cx)


@pytest.mark.parametrize("max_baseline,n_nb", [(1.05, 6), (2.1, 18)])
@pytest.mark.parametrize("name", NAMES)
def test_raw_depth_equals_restatement(built, name, max_baseline, n_nb):
    """status, n_neighbours and the counts equal, inv_depth and cost the same bytes, with 6 and with 18 neighbours at K = 64 on
    the step scene with noise"""
    _, gd = case(name)
    want = ref.run(name, "step", ref.NOISE, gd, max_baseline=max_baseline, n_hyp=64)
    got = estimate(name, "step", ref.NOISE, max_baseline=max_baseline, n_hyp=64)
    assert got.n_neighbours_used == n_nb
    bad = np.flatnonzero(got.status.ravel() != want.status.ravel())
    print(f"{name} N={n_nb} K=64 noise {ref.NOISE}: counts {got.counts.tolist()}, {bad.size} status differences, {got.seconds * 1e3:.3f} ms")
    assert bad.size == 0, (bad[:8], got.status.ravel()[bad[:8]], want.status.ravel()[bad[:8]])
    assert np.array_equal(got.n_neighbours, want.n_neighbours)
    assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == got.status.size
    assert same_bytes(got.inv_depth, want.inv_depth), np.flatnonzero(got.inv_depth.view(np.uint32).ravel() != want.inv_depth.view(np.uint32).ravel())[:8]
    assert same_bytes(got.cost, want.cost)
    assert got.counts[0] > 0.3 * (got.status != 1).sum()          # the comparison is of real estimates


@pytest.mark.parametrize("name", NAMES)
def test_raw_depth_against_true_depth(built, name):
    """e = inv_depth - 1 / v_true over the status-0 pixels of every scene, at noise 0 and NOISE, with 6 and with 18 neighbours:
    coverage and outlier share within rawdepth_reference.CONDITIONS, inlier RMS and |median| within the bars (twice the
    restatement's measured figures on this case)"""
    _, gd = case(name)
    bars = ref.BARS[name]
    for scn in ref.SCENE_NAMES:
        cov_min, out_max = ref.CONDITIONS[scn]
        for mb in ref.ACCURACY_BASELINES[name]:
            for noise in (0.0, ref.NOISE):
                a = ref.accuracy(name, scn, estimate(name, scn, noise, max_baseline=mb), gd.cx, gd.cy, gd.map_ml)
                print(f"{name} {scn} max_baseline {mb} noise {noise}: coverage {a['coverage']:.3f}, outliers {a['outliers']:.4f}, "
                      f"inlier rms {a['rms']:.5f}, |median| {a['median']:.5f} over {a['n']} pixels")
                assert a["coverage"] >= cov_min and a["outliers"] <= out_max, (scn, mb, noise, a)
                assert a["rms"] <= bars["rms"] and a["median"] <= bars["median"], (scn, mb, noise, a, bars)


@pytest.mark.parametrize("scale", dref.SCALES)
@pytest.mark.parametrize("name", NAMES)
def test_depth_map_equals_restatement(built, name, scale):
    """all four maps, the counts and n_samples from the raw-depth restatement's inv_depth: the step scene and the near scene
    (sparse, so rejection and fill both happen), with noise"""
    g, gd = case(name)
    for scn in ("step", "near"):
        iv = ref.run(name, scn, ref.NOISE, gd, max_baseline=dref.MAX_BASELINE).inv_depth
        want = dref.run(name, scn, ref.NOISE, gd, scale)
        got = depth_map.depthMapFromRaw(g, iv, scale=scale)
        print(f"{name} {scn} scale {scale}: counts {got.counts.tolist()}, {got.n_samples} samples, {got.seconds * 1e3:.3f} ms")
        assert got.scale == scale and got.status.shape == tref.out_shape(name, scale)
        assert_same_maps(got, want, ("inv_depth", "depth16", "status", "support"), (name, scn, scale))
        assert got.n_samples == want.n_samples
        assert want.counts[0] > 0 and (scn != "near" or (want.counts[1] > 0 and want.counts[3] > 0))   # the comparison is of real maps


@pytest.mark.parametrize("scale", tref.SCALES)
@pytest.mark.parametrize("name", NAMES)
def test_total_focus_equals_restatement(built, name, scale):
    """image, n_lenses, status and the counts with the TRUE depth at the cell centres, mid and step scene with noise; at scale 1
    also once on the depth map of the restatement chain (near scene, whose map has cells without a value)"""
    g, gd = case(name)
    for scn in tref.EQUALITY_SCENES:
        want = tref.run_true(name, scn, ref.NOISE, gd, scale)
        got = g.totalFocusImage(ref.make_case(name, scn, ref.NOISE), tref.true_depth(name, scn, scale), scale=scale)
        print(f"{name} {scn} scale {scale}: counts {got.counts.tolist()}, {got.seconds * 1e3:.3f} ms")
        assert got.scale == scale and got.status.shape == tref.out_shape(name, scale)
        assert_same_maps(got, want, ("image", "n_lenses", "status"), (name, scn, scale))
        assert want.counts[0] > 0.95 * want.status.size and want.n.max() > 1          # the comparison is of real pictures
    if scale == 1:
        want, dm = tref.run_chained(name, "near", ref.NOISE, gd, 1)
        got = g.totalFocusImage(ref.make_case(name, "near", ref.NOISE), dm.inv_depth)
        print(f"{name} near chained: counts {got.counts.tolist()}, {got.seconds * 1e3:.3f} ms")
        assert_same_maps(got, want, ("image", "n_lenses", "status"), (name, "chained"))
        assert want.counts[0] > 0 and want.counts[1] > 0 and want.n.max() > 1 and np.array_equal(got.status == 1, np.isnan(dm.inv_depth))


@pytest.mark.parametrize("name", NAMES)
def test_chain_from_the_raw_image_alone(built, name):
    """estimateRawDepth, depth_map() and total_focus() on every scene at noise 0 and NOISE, scale 1 and 2: the depth map within
    depthmap_reference's conditions and bars, the picture registered to better than a cell, with a pixel exactly where the map has
    a value, and its RMS against the texture within totalfocus_reference's bar"""
    g, _ = case(name)
    dbars, tbar = dref.BARS[name], tref.BARS[name]["rms"]
    for scn in ref.SCENE_NAMES:
        for noise in (0.0, ref.NOISE):
            img = ref.make_case(name, scn, noise)
            est = g.estimateRawDepth(img, patch_radius=ref.case(name)[6], max_baseline=dref.MAX_BASELINE)
            for scale in dref.SCALES:
                dm = est.depth_map(scale=scale)
                a = dref.accuracy(name, scn, dm, scale)
                print(f"{name} {scn} noise {noise} scale {scale}: {dref.describe(a)}")
                dref.check_conditions(scn, a)
                assert a["rms"] <= dbars["rms"] and a["median"] <= dbars["median"], (scn, noise, scale, a, dbars)
                tf = dm.total_focus(g, img)
                t = tref.accuracy(name, scn, tf, scale)
                inner = tref.interior(name, scn, scale)
                print(f"{name} {scn} noise {noise} scale {scale} chained: {tref.describe(t)}")
                assert tf.scale == scale and np.array_equal(inner & (tf.status == 0), inner & (dm.status <= 1)), (scn, noise, scale)
                tref.check_registration(t, (name, scn, noise, scale))
                assert t["rms"] <= tbar, (scn, noise, scale, t, tbar)
