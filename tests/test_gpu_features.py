"""Feature tracks on the GPU (include/lifcal_features.h): lifcal_features_detect and lifcal_features_match
against the numpy restatement byte for byte, against themselves across calls and pointer kinds, at their edges, the issue's
conditions and accuracy on what the GPU gives, and the tracks through DepthMaps.sample and projectPointsToRawImage."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lifcal_amd import MicroLensGrid, _capi as capi, depth, features
from tests import features_reference as fref
from tests import rawdepth_reference as ref
from tests import totalfocus_reference as tref

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "ix", "iy", "score", "desc")
_GRIDS = {}
_CHAINS = {}


def case(name):
    if name not in _GRIDS:
        g = MicroLensGrid(*ref.grid_arguments(name))
        _GRIDS[name] = (g, ref.grid_data(name, g))
    return _GRIDS[name]


def assert_feats_equal(got, want, what, least=0):
    assert want.n >= least, (what, want.n)                        # the comparison is of real content
    assert got.n == want.n, (what, got.n, want.n)
    for f in FIELDS:
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero(a.ravel() != b.ravel())
        assert a.tobytes() == b.tobytes(), (what, f, bad.size, bad[:8], a.ravel()[bad[:8]], b.ravel()[bad[:8]])


def assert_matches_equal(got, want, what):
    assert got.pair_start.tobytes() == want.pair_start.tobytes(), (what, got.pair_start, want.pair_start)
    for f in ("i", "j", "dist"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (what, f, a[:16], b[:16])


def assert_tracks_equal(got, want, what):
    assert (got.n_tracks, got.n_conflicts) == (want.n_tracks, want.n_conflicts), what
    assert got.fr.tobytes() == want.fr.tobytes() and got.pt.tobytes() == want.pt.tobytes() and got.feature.tobytes() == want.feature.tobytes(), what


def chain_on_gpu(name):
    """the chain frames of a case through the GPU: raw image -> lifcal_totalfocus_render with the true depth at scale 1"""
    if name not in _CHAINS:
        g, _ = case(name)
        _CHAINS[name] = [g.totalFocusImage(fref.chain_raw(name, k), tref.true_depth(name, "mid", 1)) for k in range(fref.CHAIN_FRAMES)]
    return _CHAINS[name]


def check_sequence(key, images, statuses, shape, bar):
    """detect, match and link on the GPU equal the restatement in every byte, and what the GPU gives meets the conditions"""
    want_f, want_m, want_l = fref.run_sequence(key, images, statuses)
    feats, m, tracks = features.trackSequence(images, statuses)
    for k, (a, b) in enumerate(zip(feats, want_f)):
        assert_feats_equal(a, b, (key, k), least=30)
    assert_matches_equal(m, want_m, key)
    assert np.array_equal(m.pairs, fref.sequence_pairs(len(images))) and len(m.i) > 0
    assert_tracks_equal(tracks, want_l, key)
    e = fref.evaluate(feats, tracks, shape)
    print(f"{key}: features {[f.n for f in feats]}, {len(m.i)} matches, {fref.describe_eval(e)}, bar {bar:.4f}, "
          f"detect {sum(f.seconds for f in feats) * 1e3:.3f} ms, match {m.seconds * 1e3:.3f} ms")
    fref.check_conditions(e, key)
    assert 0 < e["rms"] <= bar, (key, e, bar)
    return feats, m, tracks


@pytest.mark.parametrize("noise", (0.0, ref.NOISE))
def test_direct_sequence(built, noise):
    """the five direct frames: features (frames 0 and 4 among them), matches and tracks in equal bytes, conditions and accuracy"""
    check_sequence(("direct", noise), [fref.direct_frame(k, noise) for k in range(fref.DIRECT_FRAMES)], None, fref.DIRECT_SHAPE, fref.BARS["direct"]["rms"])


@pytest.mark.parametrize("name", fref.CHAIN_CASES)
def test_chain_sequence(built, name):
    """raw image -> total focus on the GPU -> features with the status map, 8 and 16 bit"""
    tfs = chain_on_gpu(name)
    _, gd = case(name)
    for tf, (img, st) in zip(tfs, fref.chain_totalfocus(name, gd)):       # section 7v: the GPU's picture is the restatement's
        assert tf.image.tobytes() == img.tobytes() and tf.status.tobytes() == st.tobytes()
    check_sequence(("chain", name), [tf.image for tf in tfs], [tf.status for tf in tfs], fref.chain_shape(name), fref.BARS[name]["rms"])


def test_pitched_rows_and_a_hole_in_the_status_map(built):
    """d9_pitch's 203 x 131 in host rows wider than the image, with a status map that has a hand-made hole"""
    w, h = ref.CASES["d9_pitch"][:2]
    img = fref.sampled_frame(1, (h, w))
    wide = np.full((h, w + 13), 255, np.uint8); wide[:, :w] = img
    view = wide[:, :w]
    assert view.strides[0] == w + 13
    status = np.zeros((h, w), np.uint8); status[50:53, 90:92] = 2; status[100, 30] = 1; status[20, 150:160] = 3
    want = fref.detect(img, status)
    free = fref.detect(img)
    assert_feats_equal(features.detectFeatures(view, status), want, "pitch and hole", least=30)
    assert_feats_equal(features.detectFeatures(view), free, "pitch", least=30)
    assert want.n < free.n and np.all((np.abs(want.ix - 90) > 15) | (np.abs(want.iy - 50) > 15))


def handmade_frames(counts, seed=3, flips=10, span=100):
    """frames that share descriptors: frame f holds counts[f] of 257 base descriptors in an order of its own, `flips` random
    bits changed in each, at random integer positions"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 32, (max(max(counts), 1), 8), dtype=np.uint64).astype(np.uint32)
    pos = rng.integers(0, span, (len(base), 2))
    out = []
    for n in counts:
        pick = rng.permutation(len(base))[:n]
        d = base[pick].copy()
        for r in range(n):
            for b in rng.integers(0, 256, flips):
                d[r, b >> 5] ^= np.uint32(1 << (int(b) & 31))
        xy = pos[pick] + rng.integers(-6, 7, (n, 2))
        out.append(fref.Feats(xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64), xy[:, 0].astype(np.int32), xy[:, 1].astype(np.int32), np.ones(n),
                              d.reshape(n, 8)))
    return out


def test_match_on_hand_made_descriptors(built):
    # feature counts 0, 1, 63, 64, 65 and 257 (one block of 256 queries and candidates, and one more), every pair both ways
    counts = [1, 63, 64, 65, 257, 0]
    feats = handmade_frames(counts)
    pairs = [(a, b) for a in range(6) for b in range(6) if a != b]
    for kw in (dict(), dict(max_dist=256, ratio_num=1, ratio_den=1), dict(max_shift=8), dict(max_shift=3, max_dist=40), dict(max_dist=20, ratio_num=1, ratio_den=2)):
        want = fref.match(feats, pairs, **kw)
        got = features.matchFeatures(feats, pairs, **kw)
        assert_matches_equal(got, want, kw)
        assert len(want.i) > 60, (kw, len(want.i))
    # the gate bites: without it more pairs match than with max_shift 3
    assert len(fref.match(feats, pairs, max_dist=40).i) > len(fref.match(feats, pairs, max_shift=3, max_dist=40).i) > 0
    # no feature in a frame: no match, pair_start still written
    got = features.matchFeatures([feats[5], feats[2], feats[5]], [(0, 1), (1, 2), (0, 2)])
    assert got.pair_start.tolist() == [0, 0, 0, 0] and len(got.i) == 0
    # one feature against one: the second-best is 257, so max_dist alone decides
    one = fref.Feats(np.zeros(1), np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1), np.zeros((1, 8), np.uint32))
    other = fref.Feats(np.zeros(1), np.zeros(1), np.zeros(1, np.int32), np.zeros(1, np.int32), np.ones(1), np.array([[0xffffffff, 0x7, 0, 0, 0, 0, 0, 0]], np.uint32))
    got = features.matchFeatures([one, other], [(0, 1)])
    assert (got.i.tolist(), got.j.tolist(), got.dist.tolist()) == ([0], [0], [35])
    assert len(features.matchFeatures([one, other], [(0, 1)], max_dist=34).i) == 0
    assert len(features.matchFeatures([one, other], [(0, 1)], max_shift=1).i) == 1
    # two identical candidates never match, whatever the ratio; tied distances take the lowest index and fail the ratio as well
    q = np.zeros((1, 8), np.uint32); q[0, 0] = 0xff
    twins = np.zeros((3, 8), np.uint32); twins[0, 0] = 0xff; twins[1, 0] = 0xff; twins[2] = 0xffffffff
    ties = np.zeros((3, 8), np.uint32); ties[0, 0] = 0xff ^ 0x1; ties[1, 0] = 0xff ^ 0x2; ties[2] = 0xffffffff
    mk = lambda d: fref.Feats(np.zeros(len(d)), np.zeros(len(d)), np.arange(len(d), dtype=np.int32), np.zeros(len(d), np.int32), np.ones(len(d)), d)
    for cand in (twins, ties):
        for kw in (dict(), dict(ratio_num=1, ratio_den=1, max_dist=256)):
            got = features.matchFeatures([mk(q), mk(cand)], [(0, 1), (1, 0)], **kw)
            assert_matches_equal(got, fref.match([mk(q), mk(cand)], [(0, 1), (1, 0)], **kw), "twins")
            assert len(got.i) == 0
    # with the gate the twin that is too far away is no candidate, and the other one matches
    got = features.matchFeatures([mk(q), mk(twins[::-1].copy())], [(0, 1)], max_shift=1)
    assert (got.i.tolist(), got.j.tolist(), got.dist.tolist()) == ([0], [1], [0])
    # capacity too small, then the second call
    lib = capi.load_library()
    off = np.array([0, counts[2], counts[2] + counts[3]], np.uint32)
    desc = np.ascontiguousarray(np.concatenate([feats[2].desc, feats[3].desc]))
    fs = capi.FeaturesSet(2, 0, capi.as_uptr(off), capi.as_uptr(desc), None, None)
    pr = np.array([[0, 1]], np.uint32); start = np.zeros(2, np.uint64)
    want = fref.match([feats[2], feats[3]], pr)
    mi = np.full(len(want.i), 77, np.uint32); mj = mi.copy(); md = mi.copy()
    lst = capi.MatchList(len(want.i) - 1, 0, start.ctypes.data_as(C.POINTER(C.c_uint64)), capi.as_uptr(mi), capi.as_uptr(mj), capi.as_uptr(md), 0.0)
    assert lib.lifcal_features_match(C.byref(fs), 1, capi.as_uptr(pr), 0, None, C.byref(lst)) == 1
    assert lst.n == len(want.i) > 10 and start.tolist() == [0, len(want.i)] and np.all(mi == 77)
    lst.capacity = lst.n
    assert lib.lifcal_features_match(C.byref(fs), 1, capi.as_uptr(pr), 0, None, C.byref(lst)) == 0
    assert mi.tobytes() == want.i.tobytes() and mj.tobytes() == want.j.tobytes() and md.tobytes() == want.dist.tobytes()


def test_detect_edges(built):
    img = fref.direct_frame(2)
    # an image smaller than 2 * 16 + 1 in one dimension: zero features; 33 x 33 has one candidate position
    for shape in ((32, 200), (160, 32), (1, 1), (33, 33), (33, 40), (34, 33)):
        small = np.ascontiguousarray(img[40:40 + shape[0], :shape[1]])
        assert_feats_equal(features.detectFeatures(small, min_score=1e-9), fref.detect(small, min_score=1e-9), shape)
    assert features.detectFeatures(np.ascontiguousarray(img[:32, :])).n == 0
    # a constant image and pure vertical stripes: score 0 everywhere
    h, w = 96, 128
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    assert features.detectFeatures(np.full((h, w), 90, np.uint8)).n == 0
    assert features.detectFeatures(np.where(xx % 6 < 3, 200, 40).astype(np.uint8)).n == 0
    # stripes with every fourth row dimmed: the scores tie exactly, the first in (y, x) order wins
    lattice = fref.tie_lattice(h, w)
    want = fref.detect(lattice)
    assert_feats_equal(features.detectFeatures(lattice), want, "ties", least=8)
    assert want.ix.tolist() == [28, 34, 40, 46, 52, 64, 70, 76, 82] and np.all(want.iy == 28)
    for kw in (dict(nms_r=1), dict(nms_r=6, win_r=1), dict(win_r=2, cell=8, per_cell=2)):
        assert_feats_equal(features.detectFeatures(lattice, **kw), fref.detect(lattice, **kw), kw)
    # per_cell 1 and 16, cell 16 and 64 (a bucket of four sub-tiles), and a cell that is no multiple of the sub-tile
    for kw in (dict(per_cell=1), dict(per_cell=16, nms_r=1, min_score=1e-7), dict(cell=16), dict(cell=64), dict(cell=64, per_cell=16, nms_r=2), dict(cell=40), dict(cell=8)):
        want = fref.detect(img, **kw)
        assert_feats_equal(features.detectFeatures(img, **kw), want, kw, least=20)
    assert fref.detect(img, per_cell=16, nms_r=1, min_score=1e-7).n > fref.detect(img).n > fref.detect(img, per_cell=1).n
    # an all-invalid status map, and one with a single invalid pixel in the middle
    assert features.detectFeatures(img, np.full(img.shape, 2, np.uint8)).n == 0
    st = np.zeros(img.shape, np.uint8); st[80, 100] = 1
    assert_feats_equal(features.detectFeatures(img, st), fref.detect(img, st), "one invalid pixel", least=30)
    # 16-bit images alternating 0 / 65535, where |g| reaches 4 * 65535, the bound behind A, C < 2^42: pixel by pixel (Sobel sees
    # nothing at period 2: no feature) and in blocks of 16, whose junctions are plateaus of tied scores
    fine = (((xx + yy) & 1) * 65535).astype(np.uint16)
    blocks = ((((xx // 16) + (yy // 16)) & 1) * 65535).astype(np.uint16)
    assert 49 * (4 * 65535) ** 2 < 2 ** 42
    for im16, least in ((fine, 0), (blocks, 20), (np.where(yy < 50, fine, blocks), 5)):
        assert np.isfinite(fref.score_map(im16, 3)).all()
        assert_feats_equal(features.detectFeatures(im16), fref.detect(im16), "16-bit extremes", least=least)


def test_capacity_too_small_then_the_second_call(built):
    lib = capi.load_library()
    img = np.ascontiguousarray(fref.direct_frame(0))
    want = fref.detect(img)
    h, w = img.shape
    ci = capi.RawDepthImage(img.ctypes.data, 8, w, h, 0, w)
    n = want.n
    x = np.full(n, 7.0); y = x.copy(); sc = x.copy(); ix = np.full(n, 7, np.int32); iy = ix.copy(); desc = np.full((n, 8), 7, np.uint32)
    lst = capi.FeaturesList(n - 1, 0, capi.as_dptr(x), capi.as_dptr(y), ix.ctypes.data_as(capi._iptr), iy.ctypes.data_as(capi._iptr), capi.as_dptr(sc), capi.as_uptr(desc), 0.0)
    assert lib.lifcal_features_detect(C.byref(ci), None, 0, None, C.byref(lst)) == 1
    assert lst.n == n and np.all(x == 7.0) and np.all(desc == 7) and np.all(ix == 7)
    lst.capacity = 0; lst.x = None
    assert lib.lifcal_features_detect(C.byref(ci), None, 0, None, C.byref(lst)) == 1 and lst.n == n       # capacity 0 just counts
    lst.capacity = n; lst.x = capi.as_dptr(x)
    assert lib.lifcal_features_detect(C.byref(ci), None, 0, None, C.byref(lst)) == 0 and lst.n == n and lst.seconds > 0
    got = fref.Feats(x, y, ix, iy, sc, desc)
    assert_feats_equal(got, want, "second call", least=30)
    assert lib.lifcal_features_detect(C.byref(ci), None, 99, None, C.byref(lst)) == -2 and b"no HIP device" in lib.lifcal_ba_last_error()


def test_same_bytes_across_calls(built):
    img, st = chain_on_gpu("d23_16")[1].image, chain_on_gpu("d23_16")[1].status
    a, b = features.detectFeatures(img, st), features.detectFeatures(img, st)
    assert a.n >= 30 and a.seconds > 0
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    feats = handmade_frames([257, 200, 129])
    m1, m2 = features.matchFeatures(feats, max_shift=10), features.matchFeatures(feats, max_shift=10)
    assert len(m1.i) > 50 and m1.seconds > 0
    for f in ("pair_start", "i", "j", "dist"):
        assert getattr(m1, f).tobytes() == getattr(m2, f).tobytes(), f


def test_device_pointers_through_torch_tensors(built):
    """image and status handed over as torch tensors on the device give the bytes of the host-pointer path, and the chain raw image
    -> depth -> depth map -> total focus -> features runs without the pictures leaving the device.  Of two HIP runtimes in one
    process only the first to start sees the GPU; this process has the library's running already, so the check runs in a fresh one."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "features_device_pointers.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "device pointers ok" in p.stdout


def test_tracks_feed_the_projection(built):
    """the chain's end on d14: raw depth -> depth map per frame, the tracks sampled with DepthMaps.sample and passed through
    projectPointsToRawImage with fr and pt: every tracked image point yields at least one observation, fr and pt arrive unchanged"""
    name = "d14"
    g, _ = case(name)
    tfs = chain_on_gpu(name)
    _, _, tracks = features.trackSequence([tf.image for tf in tfs], [tf.status for tf in tfs])
    h, w = fref.chain_shape(name)
    with depth.DepthMaps(w, h, fref.CHAIN_FRAMES) as maps:
        for k in range(fref.CHAIN_FRAMES):
            est = g.estimateRawDepth(fref.chain_raw(name, k), patch_radius=ref.CASES[name][6], max_baseline=2.1)
            est.depth_map(scale=1).to_depth_maps(maps, k)
        x, y, fr, pt = tracks.image_points()
        vd, counts = maps.sample(x, y, fr.astype(np.int32))
    print(f"{tracks.n_tracks} tracks, {len(x)} image points: {counts.direct} direct, {counts.interpolated} interpolated, {counts.failed} failed; "
          f"vdepth {vd.min():.3f} .. {vd.max():.3f}")
    assert len(x) >= 2 * tracks.n_tracks > 0 and counts.failed == 0 and np.all(vd > 1.0)
    obs = g.projectPointsToRawImage(x, y, vd, 1, fr=fr, pt=pt)
    assert np.array_equal(np.unique(obs.src), np.arange(len(x)))        # every image point yields at least one observation
    assert np.array_equal(obs.fr, fr[obs.src]) and np.array_equal(obs.pt, pt[obs.src]) and len(obs.u) > len(x)
