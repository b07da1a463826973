"""Feature tracks from total-focus images, what needs no GPU: the exports and struct layouts of
include/lifcal_features.h, the argument checks (they come before any device is touched), the descriptor's point pairs, the track
linker against the numpy restatement and on hand-made cases, and the restatement's own conditions and accuracy on the scenes,
where the bars of the GPU tests are set."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lifcal_amd import _capi as capi, features, LifcalError
from tests import features_reference as fref
from tests import rawdepth_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = C.POINTER(C.c_uint64)


def test_exports_and_layout(built):
    import lifcal_amd
    hdr = open(os.path.join(ROOT, "include", "lifcal_features.h")).read()
    declared = set(re.findall(r"\b(lifcal_(?:features|tracks)_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(capi.FEATURES_PROTOTYPES) and len(declared) == 6, declared ^ set(capi.FEATURES_PROTOTYPES)
    lib = capi.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/lifcal_features.h but not exported"
    for name in ("detectFeatures", "matchFeatures", "linkTracks", "trackSequence", "checkFeatures", "Features", "Matches", "Tracks"):
        assert hasattr(lifcal_amd, name)
    # sizes and offsets implied by include/lifcal_features.h on LP64
    assert C.sizeof(capi.FeaturesOptions) == 24 and capi.FeaturesOptions.min_score.offset == 16
    assert C.sizeof(capi.FeaturesPlan) == 40 and capi.FeaturesPlan.buckets_x.offset == 24 and capi.FeaturesPlan.max_features.offset == 32
    assert C.sizeof(capi.FeaturesList) == 72 and capi.FeaturesList.desc.offset == 56 and capi.FeaturesList.seconds.offset == 64
    assert C.sizeof(capi.FeaturesSet) == 40 and capi.FeaturesSet.offset.offset == 8 and capi.FeaturesSet.iy.offset == 32
    assert C.sizeof(capi.MatchOptions) == 16
    assert C.sizeof(capi.MatchList) == 56 and capi.MatchList.pair_start.offset == 16 and capi.MatchList.seconds.offset == 48
    assert C.sizeof(capi.Tracks) == 56 and capi.Tracks.n_conflicts.offset == 8 and capi.Tracks.fr.offset == 32
    # the defaults land where the ctypes view reads them
    plan = features.checkFeatures((160, 200), 8)
    o = plan.options
    assert (o.win_r, o.nms_r, o.cell, o.per_cell, o.min_score) == (3, 4, 32, 4, 1e-4)
    assert (plan.buckets_x, plan.buckets_y, plan.max_features) == (7, 5, 140)
    plan = features.checkFeatures((33, 32), 16, cell=16, per_cell=16)          # too narrow for one patch
    assert (plan.buckets_x, plan.buckets_y, plan.max_features) == (0, 0, 0)
    plan = features.checkFeatures((33, 33), 16, cell=16, per_cell=16)
    assert (plan.buckets_x, plan.buckets_y, plan.max_features) == (3, 3, 144)


def test_detect_argument_errors(built):
    """every check runs before a device is looked for"""
    lib = capi.load_library()
    data = np.zeros(4, np.uint16)

    def image(width=200, height=160, bits=8, pitch=None, ptr=data.ctypes.data):
        return capi.RawDepthImage(ptr, bits, width, height, 0, width if pitch is None else pitch)

    def check(img=None, **o):
        opt = features.make_options(**o)
        img = image() if img is None else img
        return lib.lifcal_features_check(C.byref(img), C.byref(opt), None)

    assert check() == 0
    assert lib.lifcal_features_check(None, None, None) == -1 and b"no image" in lib.lifcal_ba_last_error()
    assert lib.lifcal_features_check(C.byref(image()), None, None) == 0                         # no options: all defaults
    assert check(img=image(ptr=None)) == -1
    assert check(img=image(bits=12)) == -1 and b"bits" in lib.lifcal_ba_last_error()
    assert check(img=image(width=0)) == -1 and check(img=image(height=-3)) == -1 and b"size" in lib.lifcal_ba_last_error()
    assert check(img=image(pitch=199)) == -1 and b"pitch" in lib.lifcal_ba_last_error()
    assert check(img=image(pitch=213)) == 0 and check(img=image(width=5, height=7)) == 0
    assert check(win_r=-1) == -1 and check(win_r=4) == -1 and b"win_r" in lib.lifcal_ba_last_error()
    assert check(win_r=1) == 0 and check(win_r=3) == 0
    assert check(nms_r=-2) == -1 and check(nms_r=7) == -1 and b"nms_r" in lib.lifcal_ba_last_error()
    assert check(nms_r=1) == 0 and check(nms_r=6) == 0
    assert check(cell=7) == -1 and check(cell=257) == -1 and check(cell=-32) == -1 and b"cell" in lib.lifcal_ba_last_error()
    assert check(cell=8) == 0 and check(cell=256) == 0
    assert check(per_cell=-1) == -1 and check(per_cell=17) == -1 and b"per_cell" in lib.lifcal_ba_last_error()
    assert check(per_cell=1) == 0 and check(per_cell=16) == 0
    assert check(min_score=-1e-3) == -1 and check(min_score=float("nan")) == -1 and check(min_score=float("inf")) == -1
    assert b"min_score" in lib.lifcal_ba_last_error()
    assert check(min_score=1e-12) == 0
    assert check(img=image(width=65536, height=32768)) == -4 and b"2^31" in lib.lifcal_ba_last_error()
    assert check(img=image(width=64, height=8 * 65536), cell=8) == -4 and b"bucket rows" in lib.lifcal_ba_last_error()
    # the entry point itself refuses a missing image or result without touching a device
    lst = capi.FeaturesList()
    assert lib.lifcal_features_detect(None, None, 0, None, C.byref(lst)) == -1
    assert lib.lifcal_features_detect(C.byref(image()), None, 0, None, None) == -1
    assert lib.lifcal_features_detect(C.byref(image(bits=9)), None, 0, None, C.byref(lst)) == -1
    with pytest.raises(LifcalError, match="cell"):
        features.checkFeatures((160, 200), 8, cell=3)
    with pytest.raises(TypeError):
        features.checkFeatures((160, 200), 8, cells=32)
    with pytest.raises(TypeError):
        features.make_match_options(max_distance=3)


def test_match_argument_errors(built):
    lib = capi.load_library()
    desc = np.zeros((5, 8), np.uint32); ix = np.zeros(5, np.int32); iy = np.zeros(5, np.int32)

    def check(offset=(0, 2, 5), pairs=((0, 1),), with_desc=True, with_xy=True, n_frames=None, **o):
        off = np.array(offset, np.uint32); pr = np.array(pairs, np.uint32).reshape(-1, 2)
        fs = capi.FeaturesSet(len(off) - 1 if n_frames is None else n_frames, 0, capi.as_uptr(off), capi.as_uptr(desc) if with_desc else None,
                              ix.ctypes.data_as(capi._iptr) if with_xy else None, iy.ctypes.data_as(capi._iptr) if with_xy else None)
        opt = features.make_match_options(**o)
        res = capi.MatchOptions()
        rc = lib.lifcal_features_match_check(C.byref(fs), len(pr), capi.as_uptr(pr) if len(pr) else None, C.byref(opt), C.byref(res))
        return rc, res

    rc, res = check()
    assert rc == 0 and (res.max_dist, res.ratio_num, res.ratio_den, res.max_shift) == (64, 3, 4, 0)
    assert lib.lifcal_features_match_check(None, 0, None, None, None) == -1 and b"no features" in lib.lifcal_ba_last_error()
    assert check(offset=(1, 2, 5))[0] == -1 and b"offset[0]" in lib.lifcal_ba_last_error()
    assert check(offset=(0, 3, 2))[0] == -1 and b"descend" in lib.lifcal_ba_last_error()
    assert check(with_desc=False)[0] == -1 and b"descriptors" in lib.lifcal_ba_last_error()
    assert check(offset=(0, 0, 0), with_desc=False)[0] == 0                                   # no feature, no descriptors needed
    assert check(pairs=((0, 2),))[0] == -1 and b"out of range" in lib.lifcal_ba_last_error()
    assert check(pairs=((1, 1),))[0] == -1 and b"twice" in lib.lifcal_ba_last_error()
    assert check(pairs=())[0] == 0 and check(pairs=((1, 0), (0, 1)))[0] == 0
    assert check(max_dist=-1)[0] == -1 and check(max_dist=257)[0] == -1 and b"max_dist" in lib.lifcal_ba_last_error()
    assert check(max_dist=256)[0] == 0 and check(max_dist=1)[0] == 0
    assert check(ratio_num=5, ratio_den=4)[0] == -1 and check(ratio_num=-1, ratio_den=4)[0] == -1 and check(ratio_num=0, ratio_den=4)[0] == -1
    assert check(ratio_num=3, ratio_den=0)[0] == -1 and check(ratio_num=1, ratio_den=40000)[0] == -1 and b"ratio" in lib.lifcal_ba_last_error()
    assert check(ratio_num=1, ratio_den=1)[0] == 0 and check(ratio_num=7, ratio_den=10)[1].ratio_den == 10
    assert check(max_shift=-1)[0] == -1 and b"max_shift" in lib.lifcal_ba_last_error()
    assert check(max_shift=9, with_xy=False)[0] == -1 and b"ix and iy" in lib.lifcal_ba_last_error()
    assert check(max_shift=0, with_xy=False)[0] == 0 and check(max_shift=9)[0] == 0
    lst = capi.MatchList()
    assert lib.lifcal_features_match(None, 0, None, 0, None, C.byref(lst)) == -1


def test_pattern_by_hand(built):
    """the first and the last pair from the recurrence, by hand: s1 = 1664525 + 1013904223 = 1015568748, s1 >> 16 = 15496,
    15496 mod 27 = 25, 25 - 13 = 12, and so on"""
    p = features.pattern()
    assert p.shape == (256, 4) and p.dtype == np.int8
    s, draws = 1, []
    for _ in range(4):
        s = (1664525 * s + 1013904223) & 0xffffffff
        draws.append(((s >> 16) % 27) - 13)
    assert s != 1 and draws[0] == 12 and p[0].tolist() == draws
    assert p[0].tolist() == [12, -5, 12, 12]
    assert p[255].tolist() == fref.pattern()[255].tolist() == LAST_PAIR == [9, -6, 3, -9]
    assert np.array_equal(p, fref.pattern())
    assert p.min() == -13 and p.max() == 13 and not np.any((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3]))
    assert len({tuple(r) for r in p.tolist()}) == 256


LAST_PAIR = None   # set below, once, from the recurrence written out without the library or the restatement


def _last_pair_by_hand():
    s, pairs = 1, []
    while len(pairs) < 256:
        v = []
        for _ in range(4):
            s = (s * 1664525 + 1013904223) % 4294967296
            v.append((s // 65536) % 27 - 13)
        if v[:2] != v[2:]:
            pairs.append(v)
    return pairs[255]


LAST_PAIR = _last_pair_by_hand()


# ---------------------------------------------------------------------------------------------------------------- the linker
def link_c(counts, pairs, start, mi, mj, min_length=0, capacity=None):
    """lifcal_tracks_link itself; capacity None: count, then fill"""
    lib = capi.load_library()
    off = np.r_[0, np.cumsum(counts)].astype(np.uint32)
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2); start = np.ascontiguousarray(start, np.uint64)
    mi = np.ascontiguousarray(mi, np.uint32); mj = np.ascontiguousarray(mj, np.uint32)
    cap = 0 if capacity is None else capacity
    while True:
        fr = np.full(cap, 77, np.uint32); pt = np.full(cap, 77, np.uint32); ft = np.full(cap, 77, np.uint32)
        t = capi.Tracks(min_length, 0, 0, cap, 0, capi.as_uptr(fr), capi.as_uptr(pt), capi.as_uptr(ft))
        rc = lib.lifcal_tracks_link(len(counts), capi.as_uptr(off), len(pairs), capi.as_uptr(pairs) if len(pairs) else None,
                                    start.ctypes.data_as(U64) if len(pairs) else None, capi.as_uptr(mi) if len(mi) else None,
                                    capi.as_uptr(mj) if len(mj) else None, C.byref(t))
        if rc != 1 or capacity is not None:
            return rc, t, fr, pt, ft
        cap = int(t.n)


def assert_link_equals_restatement(counts, pairs, start, mi, mj, min_length=2):
    rc, t, fr, pt, ft = link_c(counts, pairs, start, mi, mj, min_length)
    want = fref.link(counts, pairs, start, mi, mj, min_length)
    assert rc == 0 and (t.n_tracks, t.n_conflicts, t.n) == (want.n_tracks, want.n_conflicts, len(want.fr))
    assert fr.tobytes() == want.fr.tobytes() and pt.tobytes() == want.pt.tobytes() and ft.tobytes() == want.feature.tobytes()
    return want


def test_linker_on_hand_made_cases(built):
    lib = capi.load_library()
    counts = [3, 3, 3]
    pairs = [(0, 1), (1, 2), (0, 2)]
    # a chain a-b-c: feature 2 of frame 0 - feature 0 of frame 1 - feature 1 of frame 2; and a two-frame track 0/1 - 2/2
    rc, t, fr, pt, ft = link_c(counts, pairs, [0, 1, 2, 3], [2, 0, 1], [0, 1, 2])
    assert rc == 0 and (t.n_tracks, t.n_conflicts, t.n) == (2, 0, 5)
    # ordering: observations by frame then feature; tracks numbered by their first observation (feature 1 of frame 0 comes first)
    assert fr.tolist() == [0, 0, 1, 2, 2] and ft.tolist() == [1, 2, 3, 7, 8] and pt.tolist() == [0, 1, 1, 1, 0]
    assert_link_equals_restatement(counts, pairs, [0, 1, 2, 3], [2, 0, 1], [0, 1, 2])
    # min_length 3 keeps the chain only; 0 selects 2; 1 is refused
    rc, t, fr, pt, ft = link_c(counts, pairs, [0, 1, 2, 3], [2, 0, 1], [0, 1, 2], min_length=3)
    assert rc == 0 and (t.n_tracks, t.n) == (1, 3) and ft.tolist() == [2, 3, 7] and pt.tolist() == [0, 0, 0]
    assert link_c(counts, pairs, [0, 1, 2, 3], [2, 0, 1], [0, 1, 2], min_length=1)[0] == -1 and b"min_length" in lib.lifcal_ba_last_error()
    # a conflict: 0/0 - 1/0 - 2/0 and 0/1 - 2/0 put two features of frame 0 into one component: dropped whole, counted
    rc, t, fr, pt, ft = link_c(counts, pairs, [0, 1, 2, 3], [0, 0, 1], [0, 0, 0])
    assert rc == 0 and (t.n_tracks, t.n_conflicts, t.n) == (0, 1, 0)
    # the conflict does not touch another track
    rc, t, fr, pt, ft = link_c(counts, pairs, [0, 2, 3, 4], [0, 2, 0, 1], [0, 2, 0, 0])
    assert rc == 0 and (t.n_tracks, t.n_conflicts, t.n) == (1, 1, 2) and ft.tolist() == [2, 5] and fr.tolist() == [0, 1]
    assert_link_equals_restatement(counts, pairs, [0, 2, 3, 4], [0, 2, 0, 1], [0, 2, 0, 0])
    # an empty pair in the middle, a frame without features, no pairs at all
    rc, t, fr, pt, ft = link_c([2, 0, 2], [(0, 2), (0, 1), (2, 0)], [0, 1, 1, 2], [1, 0], [0, 1])
    assert rc == 0 and (t.n_tracks, t.n) == (1, 2) and ft.tolist() == [1, 2] and fr.tolist() == [0, 2]
    rc, t, _, _, _ = link_c([2, 2], [], [0], [], [])
    assert rc == 0 and (t.n_tracks, t.n) == (0, 0)
    # the same match twice and in both directions is one track
    rc, t, fr, pt, ft = link_c([2, 2], [(0, 1), (1, 0), (0, 1)], [0, 1, 2, 3], [1, 0, 1], [0, 1, 0])
    assert rc == 0 and (t.n_tracks, t.n_conflicts, t.n) == (1, 0, 2) and ft.tolist() == [1, 2]
    # capacity too small: nothing written, the counts are; then the second call
    rc, t, fr, pt, ft = link_c(counts, pairs, [0, 1, 2, 3], [2, 0, 1], [0, 1, 2], capacity=4)
    assert rc == 1 and (t.n_tracks, t.n) == (2, 5) and fr.tolist() == [77] * 4
    rc, t, fr, pt, ft = link_c(counts, pairs, [0, 1, 2, 3], [2, 0, 1], [0, 1, 2], capacity=6)
    assert rc == 0 and t.n == 5 and fr.tolist() == [0, 0, 1, 2, 2, 77]
    # indices out of range are refused, never read
    for bad in (dict(mi=[3, 0, 1]), dict(mj=[0, 1, 3]), dict(pairs=[(0, 1), (1, 3), (0, 2)]), dict(pairs=[(0, 1), (1, 1), (0, 2)]), dict(start=[0, 2, 1, 3]),
                dict(mi=[2, 0, 0xffffffff])):
        kw = dict(pairs=pairs, start=[0, 1, 2, 3], mi=[2, 0, 1], mj=[0, 1, 2]); kw.update(bad)
        assert link_c(counts, kw["pairs"], kw["start"], kw["mi"], kw["mj"])[0] == -1, bad
    assert b"pair_start" in lib.lifcal_ba_last_error() or b"out of range" in lib.lifcal_ba_last_error()
    assert lib.lifcal_tracks_link(0, None, 0, None, None, None, None, None) == -1
    with pytest.raises(LifcalError):
        features.linkTracks([fref.Feats(np.zeros(2), np.zeros(2), None, None, None, None)] * 2,
                            features.Matches(np.array([[0, 1]], np.uint32), np.array([0, 1], np.uint64), np.array([2], np.uint32), np.array([0], np.uint32), np.zeros(1, np.uint32)))


def test_linker_on_random_matches(built):
    """random match lists with conflicts and repeats against the restatement's loop"""
    rng = np.random.default_rng(5)
    for trial in range(20):
        counts = rng.integers(0, 9, 5).tolist()
        pairs = [(a, b) for a in range(5) for b in range(5) if a != b and rng.random() < 0.4]
        start, mi, mj = [0], [], []
        for a, b in pairs:
            for _ in range(int(rng.integers(0, 4)) if counts[a] and counts[b] else 0):
                mi.append(int(rng.integers(0, counts[a]))); mj.append(int(rng.integers(0, counts[b])))
            start.append(len(mi))
        for min_length in (2, 3):
            assert_link_equals_restatement(counts, pairs, start, mi, mj, min_length)


# ---------------------------------------------------------------------------------------------------------------- the scenes
def oracle_grid(name):
    from oracle.mla import MicroLensGrid
    return ref.grid_data(name, MicroLensGrid(*ref.grid_arguments(name)))


def check_sequence(built, key, images, statuses, shape, measured):
    feats, m, linked = fref.run_sequence(key, images, statuses)
    e = fref.evaluate(feats, linked, shape)
    print(f"{key}: features {[f.n for f in feats]}, {len(m.i)} matches, {fref.describe_eval(e)}")
    fref.check_conditions(e, key)
    assert 0 < e["rms"] <= measured, (key, e)
    # the library's linker on the restatement's matches gives the restatement's tracks, and Tracks carries their positions
    want = assert_link_equals_restatement([f.n for f in feats], m.pairs, m.pair_start, m.i, m.j)
    tr = features.linkTracks(feats, features.Matches(m.pairs, m.pair_start, m.i, m.j, m.dist))
    assert (tr.n_tracks, tr.n_conflicts) == (want.n_tracks, want.n_conflicts) and tr.feature.tobytes() == want.feature.tobytes()
    x, y, fr, pt = tr.image_points()
    assert np.array_equal(x, np.concatenate([f.x for f in feats])[want.feature]) and fr.tobytes() == want.fr.tobytes() and pt.tobytes() == want.pt.tobytes()
    assert y.dtype == np.float64 and fr.dtype == np.uint32 and pt.dtype == np.uint32


@pytest.mark.parametrize("noise", (0.0, ref.NOISE))
def test_restatement_conditions_direct(built, noise):
    """the issue's conditions on the direct sequence, noise 0 and NOISE, and the RMS within the recorded figure, whose double is
    the bar of the GPU tests"""
    check_sequence(built, ("direct", noise), [fref.direct_frame(k, noise) for k in range(fref.DIRECT_FRAMES)], None, fref.DIRECT_SHAPE,
                   fref.MEASURED["direct"]["rms"])


@pytest.mark.parametrize("name", fref.CHAIN_CASES)
def test_restatement_conditions_chain(built, name):
    """the same on the chain sequences: raw image -> total-focus restatement with the true depth -> features, with the status map"""
    tfs = fref.chain_totalfocus(name, oracle_grid(name))
    check_sequence(built, ("chain", name), [a for a, _ in tfs], [b for _, b in tfs], fref.chain_shape(name), fref.MEASURED[name]["rms"])


def test_restatement_rules_on_hand_made_images():
    """the rules of the header where the scenes do not reach: ties, the status map, small and flat images"""
    h, w = 96, 128
    assert fref.detect(np.full((h, w), 90, np.uint8)).n == 0                                  # constant: score 0
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    stripes = np.where(xx % 6 < 3, 200, 40).astype(np.uint8)
    assert fref.detect(stripes).n == 0                                                        # gy = 0: B = C = 0, score 0
    lattice = fref.tie_lattice(h, w)
    f = fref.detect(lattice)
    sc = fref.score_map(lattice, 3)
    # exact ties 4 rows apart: within the 9 x 9 neighbourhood only the first in (y, x) order is a maximum, so one row of features stays
    assert f.n >= 8 and np.all(f.iy == f.iy[0]) and np.all(np.diff(f.ix) % 6 == 0)
    assert all(sc[y + 4, x] == sc[y, x] == sc[y, x + 6] > sc[y - 4, x] and sc[y, x] > 1e-4 for x, y in zip(f.ix.tolist(), f.iy.tolist()))
    # and in the bucket that holds five tied maxima the first four in x stay
    assert f.ix.tolist() == [28, 34, 40, 46, 52, 64, 70, 76, 82]
    assert fref.detect(lattice[20:53, 20:52]).n == 0 and fref.detect(lattice[20:53, 20:53]).n <= 1     # 33 x 33: one candidate position
    # the status map: a hole of invalid pixels keeps every feature at least 16 away from it
    status = np.zeros((h, w), np.uint8); status[40:43, 60:62] = 2; status[70, 100] = 1; status[10, 10] = 3
    g = fref.detect(lattice, status)
    assert 0 < g.n < f.n
    for hx, hy in ((60, 40), (61, 42), (100, 70)):
        assert np.all((np.abs(g.ix - hx) > 15) | (np.abs(g.iy - hy) > 15))
    assert fref.detect(lattice, np.full((h, w), 2, np.uint8)).n == 0
    # buckets: per_cell caps every bucket, the order inside is score descending
    for cell, per_cell in ((16, 1), (64, 16), (32, 4)):
        q = fref.detect(lattice, cell=cell, per_cell=per_cell)
        b = (q.iy // cell) * ((w + cell - 1) // cell) + q.ix // cell
        assert np.all(np.diff(b) >= 0) and np.bincount(b).max() <= per_cell
        same = np.diff(b) == 0
        assert np.all(np.diff(q.score)[same] <= 0)
    assert np.all(np.abs(f.x - f.ix) <= 0.5) and np.all(np.abs(f.y - f.iy) <= 0.5)
