"""Virtual depth from the raw image on the GPU (include/lifcal_rawdepth.h): lifcal_rawdepth_estimate against
the numpy restatement byte for byte, against itself across calls and pointer kinds, against the true depth of rendered scenes,
and lifcal_rawdepth_points through lifcal_mla_project and the calibrated camera."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lifcal_amd import MicroLensGrid, _capi as capi, raw_depth, scene
from tests import rawdepth_reference as ref

pytestmark = pytest.mark.gpu

_GRIDS = {}


def setup(name):
    """(grid, its data for the restatement), made once per case"""
    if name not in _GRIDS:
        g = MicroLensGrid(*ref.grid_arguments(name))
        _GRIDS[name] = (g, ref.grid_data(name, g))
    return _GRIDS[name]


def image(name, scn, noise):
    """the case's image as the case hands it over: d9_pitch in host rows wider than the image"""
    img = ref.make_case(name, scn, noise)
    extra = ref.CASES[name][7]
    if not extra:
        return img
    wide = np.full((img.shape[0], img.shape[1] + extra), 255, img.dtype)   # bright columns the kernel must never read
    wide[:, :img.shape[1]] = img
    view = wide[:, :img.shape[1]]
    assert view.strides[0] == wide.shape[1] * img.itemsize
    return view


def estimate(name, scn, noise, **opts):
    g, _ = setup(name)
    return g.estimateRawDepth(image(name, scn, noise), patch_radius=ref.CASES[name][6], **opts)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("max_baseline,n_nb", [(1.05, 6), (2.1, 18)])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_equals_restatement(built, name, max_baseline, n_nb):
    """status, n_neighbours and the counts equal, inv_depth and cost the same bytes: every case with 6 and with 18 neighbours,
    at K = 64 with noise and at K = 16 without, on the step scene (two depths and an occlusion edge in one image)"""
    _, gd = setup(name)
    for K, noise in ((64, ref.NOISE), (16, 0.0)):
        want = ref.run(name, "step", noise, gd, max_baseline=max_baseline, n_hyp=K)
        got = estimate(name, "step", noise, max_baseline=max_baseline, n_hyp=K)
        assert got.n_neighbours_used == n_nb
        bad = np.flatnonzero(got.status.ravel() != want.status.ravel())
        print(f"{name} N={n_nb} K={K} noise {noise}: counts {got.counts.tolist()}, {bad.size} status differences, {got.seconds * 1e3:.3f} ms")
        assert bad.size == 0, (bad[:8], got.status.ravel()[bad[:8]], want.status.ravel()[bad[:8]])
        assert np.array_equal(got.n_neighbours, want.n_neighbours)
        assert np.array_equal(got.counts, want.counts) and int(got.counts.sum()) == got.status.size
        assert same_bytes(got.inv_depth, want.inv_depth), np.flatnonzero(got.inv_depth.view(np.uint32).ravel() != want.inv_depth.view(np.uint32).ravel())[:8]
        assert same_bytes(got.cost, want.cost)
        assert got.counts[0] > 0.3 * (got.status != 1).sum() or K == 16          # the comparison is of real estimates


@pytest.mark.parametrize("name", list(ref.CASES))
def test_same_bytes_across_calls(built, name):
    """two calls give the same bytes; the outputs are optional"""
    g, _ = setup(name)
    first = estimate(name, "mid", ref.NOISE, max_baseline=2.1)
    again = estimate(name, "mid", ref.NOISE, max_baseline=2.1)
    for f in ("inv_depth", "cost", "status", "n_neighbours"):
        assert same_bytes(getattr(first, f), getattr(again, f)), f
    assert np.array_equal(first.counts, again.counts) and first.seconds > 0 and first.counts[0] > 0
    # outputs are optional: a call that asks for the status alone
    lib = capi.load_library()
    img, keep = raw_depth._image(image(name, "mid", ref.NOISE))
    st = np.zeros(first.status.shape, np.uint8)
    res = capi.RawDepthResult(); res.status = st.ctypes.data
    opt = raw_depth.make_options(patch_radius=ref.CASES[name][6], max_baseline=2.1)
    assert lib.lifcal_rawdepth_estimate(g._h, C.byref(img), C.byref(opt), C.byref(res)) == 0
    assert same_bytes(st, first.status) and list(res.count) == first.counts.tolist()


def test_device_pointers_through_torch_tensors(built):
    """the raw image handed over as a torch tensor on the device (dense and with a row pitch) and the maps written into torch
    tensors give the bytes of the host-pointer path.  The torch wheel carries a HIP runtime of its own, and of two runtimes in one
    process only the first to start sees the GPU; this process has the library's running already, so the check runs in a fresh one."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rawdepth_device_pointers.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "device pointers ok" in p.stdout


@pytest.mark.parametrize("name", list(ref.CASES))
def test_accuracy_against_true_depth(built, name):
    """e = inv_depth - 1 / v_true over the status-0 pixels of every scene, at noise 0 and NOISE: inlier RMS and |median| within
    the bars (twice the restatement's measured figures), coverage and outlier share within the issue's conditions"""
    _, gd = setup(name)
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


def test_points_project_back_to_their_pixels(built):
    """points(): ascending src; fed to lifcal_mla_project at scale 1, every point with 2 < v < 20 has an observation in its own
    lens at its source pixel.  lifcal_mla_project works in float: xr = (xu - lcx) / v + lcx with xu, lcx, v rounded to float, so
    |xr - px| <= ulp(xu) / (2 v) (rounding xu) + ulp(xu - lcx) / (2 v) (the difference) + ulp(q) / 2 (the quotient, |q| <= d / 2)
    + ulp(xr) / 2 (the sum), and with |xu| < 2 width, v > 2 that is below ulp(width) / 2 + ulp(width) / 4 + ulp(width) = 1.75
    ulp(width): the test allows 2 ulp of float(max(width, height)).  lifcal_mla_project gives no observation for a virtual point
    left of or above the image and looks lenses up at their centre pixel clamped into the image (its documented contract), so
    the points compared are those with xu, yu >= 0 whose lens centre lies inside the image."""
    name = "d14"
    g, gd = setup(name)
    w, h = ref.CASES[name][:2]
    est = estimate(name, "step", 0.0, max_baseline=2.1)
    pts = est.points()
    wx, wy, wv, wsrc, wlens = ref.points(est.inv_depth, gd.map_ml, gd.cx, gd.cy)
    assert len(pts.src) == int(est.counts[0]) > 1000 and np.all(np.diff(pts.src.astype(np.int64)) > 0)
    assert np.array_equal(pts.src, wsrc) and np.array_equal(pts.lens, wlens)
    assert same_bytes(pts.x, wx) and same_bytes(pts.y, wy) and same_bytes(pts.vdepth, wv)
    obs = g.projectPointsToRawImage(pts.x, pts.y, pts.vdepth, 1)
    px, py = (pts.src % w).astype(np.float64), (pts.src // w).astype(np.float64)
    lcx, lcy = gd.cx.astype(np.float64)[pts.lens], gd.cy.astype(np.float64)[pts.lens]
    use = (pts.vdepth > 2) & (pts.vdepth < 20) & (pts.x >= 0) & (pts.y >= 0) & (lcx >= 0) & (lcx <= w - 1) & (lcy >= 0) & (lcy <= h - 1)
    assert use.sum() > 0.8 * len(use)
    own = (obs.mcx == lcx[obs.src]) & (obs.mcy == lcy[obs.src])
    err = np.maximum(np.abs(obs.u - px[obs.src]), np.abs(obs.v - py[obs.src]))
    tol = 2.0 * float(np.spacing(np.float32(max(w, h))))
    hit = np.zeros(len(use), bool)
    hit[obs.src[own & (err <= tol)]] = True
    print(f"{int(use.sum())} of {len(use)} points compared, {int((use & ~hit).sum())} without their pixel, largest error among own-lens observations "
          f"{err[own & use[obs.src]].max():.3e} px (tolerance {tol:.3e})")
    assert hit[use].all()
    # scale 2: the same virtual points in a virtual image of half the resolution
    p2 = est.points(scale=2)
    w2 = ref.points(est.inv_depth, gd.map_ml, gd.cx, gd.cy, scale=2)
    assert same_bytes(p2.x, w2[0]) and same_bytes(p2.y, w2[1]) and same_bytes(p2.vdepth, wv) and np.array_equal(p2.src, wsrc)


def test_metric_points_of_a_plane(built):
    """metric_points through the calibrated camera of scene.baseline_spec("tiny") without distortion: z = fL b / (b - fL),
    b = bL0 + B / iv, a decreasing function of iv.  The median commutes with it, so |median z - z_true| is bounded by the larger
    of |z(iv_true +- bar_median) - z_true|; for the inliers z - z_true = g e + z'' e^2 / 2 with |e| <= 0.02, hence e^2 <= 0.02 |e|
    and rms(z - z_true) <= bar_rms (|g| + 0.01 max |z''|), g and z'' taken over [iv_true - 0.02, iv_true + 0.02]."""
    name, scn = "d14", "far"
    spec = scene.baseline_spec("tiny")
    cam = np.zeros(17); cam[:5] = [spec.fL, spec.bL0, spec.B, 0.5 * (ref.CASES[name][0] - 1), 0.5 * (ref.CASES[name][1] - 1)]
    spx = spec.pixel_size * spec.scale
    z_of = lambda iv: spec.fL * (spec.bL0 + spec.B / iv) / ((spec.bL0 + spec.B / iv) - spec.fL)
    iv_true = 1.0 / ref.SCENE_DEPTHS[name][scn]
    est = estimate(name, scn, ref.NOISE, max_baseline=2.1)
    pts, bp = est.metric_points(cam, 0, spx)
    assert bp.n_invalid == 0 and bp.p_c.shape == (len(pts.src), 3)
    z = bp.p_c[:, 2]
    assert np.allclose(z, z_of(1.0 / pts.vdepth), rtol=1e-12, atol=0)
    inl = np.abs(1.0 / pts.vdepth - iv_true) <= ref.OUTLIER
    grid_iv = np.linspace(iv_true - ref.OUTLIER, iv_true + ref.OUTLIER, 4001)
    zz = z_of(grid_iv)
    g1 = np.abs(np.gradient(zz, grid_iv)).max()
    g2 = np.abs(np.gradient(np.gradient(zz, grid_iv), grid_iv)[2:-2]).max()
    bars = ref.BARS[name]
    bar_med = max(abs(z_of(iv_true + bars["median"]) - z_of(iv_true)), abs(z_of(iv_true - bars["median"]) - z_of(iv_true)))
    bar_rms = bars["rms"] * (g1 + 0.5 * ref.OUTLIER * g2)
    med, rms = abs(np.median(z[inl]) - z_of(iv_true)), float(np.sqrt(np.mean((z[inl] - z_of(iv_true)) ** 2)))
    print(f"z_true {z_of(iv_true):.2f}: |median z - z_true| {med:.3f} (bar {bar_med:.3f}), inlier rms {rms:.3f} (bar {bar_rms:.3f}), {int(inl.sum())} of {len(inl)} inliers")
    assert inl.sum() > 0.98 * len(inl)
    assert med <= bar_med and rms <= bar_rms


def test_count_protocol(built):
    """capacity 0 counts; a capacity below n writes nothing and returns LIFCAL_MLA_MORE; n entries fill; src and lens are optional"""
    lib = capi.load_library()
    g, gd = setup("d14")
    est = estimate("d14", "mid", 0.0)
    iv = np.ascontiguousarray(est.inv_depth)
    n = int(est.counts[0])
    io = capi.RawDepthPointList(iv.ctypes.data, 0, 1, 0, 0, None, None, None, None, None)
    assert lib.lifcal_rawdepth_points(g._h, C.byref(io)) == capi.MLA_MORE and io.n == n
    x = np.full(n, -7.0); y = np.full(n, -7.0); v = np.full(n, -7.0)
    io = capi.RawDepthPointList(iv.ctypes.data, 0, 1, n - 1, 0, capi.as_dptr(x), capi.as_dptr(y), capi.as_dptr(v), None, None)
    assert lib.lifcal_rawdepth_points(g._h, C.byref(io)) == capi.MLA_MORE and io.n == n
    assert np.all(x == -7.0) and np.all(y == -7.0) and np.all(v == -7.0)
    io = capi.RawDepthPointList(iv.ctypes.data, 0, 1, n, 0, capi.as_dptr(x), capi.as_dptr(y), capi.as_dptr(v), None, None)
    assert lib.lifcal_rawdepth_points(g._h, C.byref(io)) == 0 and io.n == n
    wx, wy, wv, _, _ = ref.points(est.inv_depth, gd.map_ml, gd.cx, gd.cy)
    assert same_bytes(x, wx) and same_bytes(y, wy) and same_bytes(v, wv)
    # a map without a status-0 pixel has no points
    none = np.full(iv.shape, np.nan, np.float32)
    io = capi.RawDepthPointList(none.ctypes.data, 0, 1, 0, 0, None, None, None, None, None)
    assert lib.lifcal_rawdepth_points(g._h, C.byref(io)) == 0 and io.n == 0
    # bad arguments
    io = capi.RawDepthPointList(iv.ctypes.data, 0, 0, 0, 0, None, None, None, None, None)
    assert lib.lifcal_rawdepth_points(g._h, C.byref(io)) == -1
    io = capi.RawDepthPointList(iv.ctypes.data, 0, 1, n, 0, None, None, None, None, None)
    assert lib.lifcal_rawdepth_points(g._h, C.byref(io)) == -1
    assert lib.lifcal_rawdepth_points(None, C.byref(io)) == -1


def test_window_too_large_is_out_of_range(built):
    """a grid whose lens neighbourhood does not fit 64 KB of LDS is refused, not handled some other way"""
    g = MicroLensGrid(256, 200, 60.0, ref.BASE_Y)
    img = np.zeros((200, 256), np.uint8)
    with pytest.raises(Exception, match="LDS") as ei:
        g.estimateRawDepth(img)
    assert ei.value.code == -4
