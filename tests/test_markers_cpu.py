"""Fiducial markers without a device (include/lifcal_markers.h): properties of the numpy restatement, the host
ABI (checks with every refusal, dictionary distance and generator, constraints reader, start values, scale factor) against the
restatement, the Python layer around them, and the accuracy measurement that fills markers_reference.MEASURED."""
import ctypes as C

import numpy as np
import pytest

from lifcal_amd import LifcalError, _capi as capi, marker_image as mi, markers
from lifcal_amd.features import Tracks
from tests import markers_reference as mr

INVALID, NO_DEVICE, OUT_OF_RANGE, NUMERIC = -1, -2, -4, -7


def refused(code, fn, *a, **kw):
    with pytest.raises(LifcalError) as e:
        fn(*a, **kw)
    assert e.value.code == code, (e.value.code, code, str(e.value))
    return str(e.value)

# ------------------------------------------------------------------------------------------------ the restatement


def test_rotation_of_words():
    m = 4
    B = mr.word_bits(0b1010_0000_0110_0001, m)
    w = int(sum(int(B[r, c]) << (r * m + c) for r in range(m) for c in range(m)))
    assert np.array_equal(mr.word_bits(mr.rot_word(w, m), m), np.rot90(B, -1))          # a quarter turn clockwise
    assert mr.rotations(w, m)[0] == w and mr.rot_word(mr.rotations(w, m)[3], m) == w


@pytest.mark.parametrize("m", [3, 4, 5])
def test_every_word_decodes_at_all_four_rotations(built, m):
    """a drawn marker of every dictionary word, turned by k quarter turns, comes back with its id, rotation k and distance 0, and
    corner 0 is the marker's own top-left"""
    words, dmin = mr.dictionary(m, 12, 5)
    for j, w in enumerate(words):
        for k in range(4):
            img = mr.hand_marker(int(w), m, angle_quarter=k)
            rec, nc = mr.detect(img, words, m)
            assert nc == 1 and len(rec) == 1, (m, j, k)
            assert (rec["id"][0], rec["rotation"][0], rec["hamming"][0], rec["refined"][0]) == (j, k, 0, 1), (m, j, k, rec)
            side = 6.0 * (m + 2)
            corners = np.array([(11.5, 11.5), (11.5 + side, 11.5), (11.5 + side, 11.5 + side), (11.5, 11.5 + side)])
            assert np.allclose(rec["corners"][0], np.roll(corners, -k, axis=0), atol=1e-9), (k, rec["corners"][0])
            assert abs(rec["x"][0] - (11.5 + side / 2)) < 1e-9 and abs(rec["y"][0] - (11.5 + side / 2)) < 1e-9


def test_label_map_on_hand_made_shapes():
    d = np.zeros((6, 8), np.uint8)
    d[0, 5] = 1; d[1, 4] = 1; d[2, 3] = 1          # a diagonal: one component under 8-connectivity, label 5
    d[4, 0:3] = 1; d[5, 2] = 1                     # an L, label 32
    d[4, 6] = 1                                    # alone, label 38
    lab = mr.label_map(d)
    assert lab[0, 5] == lab[1, 4] == lab[2, 3] == 5 and lab[4, 0] == lab[4, 2] == lab[5, 2] == 32 and lab[4, 6] == 38
    assert np.all(lab[d == 0] == -1)
    # a U whose lowest index lies at the end of one arm: the other arm learns it only through the bottom
    u = np.zeros((7, 7), np.uint8)
    u[0:6, 5] = 1; u[5, 1:6] = 1; u[2:6, 1] = 1
    assert set(mr.label_map(u)[u == 1]) == {5}
    # extremes with ties: a plus sign
    p = np.full((40, 40), 255, np.uint8)
    p[10:31, 20] = 0; p[20, 10:31] = 0
    _, labels, table = mr.components(p, min_side=2, min_area=4)
    assert len(table) == 1 and table["label"][0] == 10 * 40 + 20 and table["area"][0] == 41
    assert [tuple(e) for e in table["ext"][0]] == [(10, 20), (30, 20), (20, 10), (20, 30), (20, 10), (30, 20), (10, 20), (20, 10)]


def test_quad_rules():
    sq = [(10, 10), (30, 10), (10, 10), (10, 30), (10, 10), (30, 30), (10, 30), (30, 10)]   # an axis-aligned square's extremes
    assert mr.quad(sq, 12) == [(9.5, 9.5), (30.5, 9.5), (30.5, 30.5), (9.5, 30.5)]
    di = [(0, 20), (40, 20), (20, 0), (20, 40), (20, 0), (20, 40), (0, 20), (40, 20)]       # a diamond's: the diagonal set is degenerate
    assert mr.quad(di, 12) == [(20.0, -0.5), (40.5, 20.0), (20.0, 40.5), (-0.5, 20.0)]
    assert mr.quad(sq, 29) is None and mr.quad(sq, 28) is not None                          # 2 * 20 * 20 = 800 against min_side^2

# ------------------------------------------------------------------------------------------------ the host ABI


def test_checks_and_refusals(built):
    d = markers.Dictionary.generate(4, 50, 1)
    plan = markers.checkMarkers((131, 203), 8, d)
    o = plan.options
    assert (o.w, o.contrast, o.cell_contrast, o.min_area, o.min_side, o.max_side, o.max_border_errors, o.refine_max) == (7, 12, 24, 32, 12, 131, 0, 3.0)
    assert plan.min_distance == d.min_distance == mr.dictionary()[1] and o.max_correction == (d.min_distance - 1) // 2
    assert (plan.tiles_x, plan.tiles_y, plan.max_candidates) == (7, 5, 131 * 203 // 32)
    assert markers.checkMarkers((100, 100), 16, d, max_correction=-1).options.max_correction == 0
    assert markers.checkMarkers((100, 100), 16, None).min_distance == 0
    for bad, word in ((dict(w=32), "w outside"), (dict(w=-1), "w outside"), (dict(contrast=256), "contrast"), (dict(cell_contrast=300), "cell_contrast"),
                      (dict(min_area=-3), "min_area"), (dict(min_side=1), "min_side"), (dict(min_side=20, max_side=19), "max_side"),
                      (dict(max_border_errors=-1), "max_border_errors"), (dict(max_border_errors=21), "max_border_errors"),
                      (dict(max_correction=(d.min_distance - 1) // 2 + 1), "max_correction"), (dict(max_correction=-2), "max_correction"),
                      (dict(refine_max=-1.0), "refine_max"), (dict(refine_max=float("inf")), "refine_max")):
        assert word in refused(INVALID, markers.checkMarkers, (100, 100), 8, d, **bad), bad
    assert "without a dictionary" in refused(INVALID, markers.checkMarkers, (100, 100), 8, None, max_correction=1)
    refused(INVALID, markers.checkMarkers, (100, 100), 12, d)
    refused(INVALID, markers.checkMarkers, (0, 100), 8, d)
    refused(OUT_OF_RANGE, markers.checkMarkers, (1 << 16, 1 << 15), 8, d)
    with pytest.raises(TypeError):
        markers.checkMarkers((100, 100), 8, d, no_such_option=1)
    # the image's pitch and pointer
    lib = capi.load_library()
    px = np.zeros(4, np.uint8)
    img = capi.RawDepthImage(px.ctypes.data, 8, 50, 50, 0, 49)
    assert lib.lifcal_markers_check(C.byref(img), None, None, None) == INVALID and b"pitch" in lib.lifcal_ba_last_error()
    img = capi.RawDepthImage(None, 8, 50, 50, 0, 50)
    assert lib.lifcal_markers_check(C.byref(img), None, None, None) == INVALID
    assert lib.lifcal_markers_check(None, None, None, None) == INVALID
    # the argument checks of the device calls come before any device is touched
    img = capi.RawDepthImage(px.ctypes.data, 8, 50, 50, 0, 50)
    assert lib.lifcal_markers_detect(C.byref(img), None, 0, None, None, None) == INVALID
    lst = capi.MarkerList()
    assert lib.lifcal_markers_detect(C.byref(img), None, 0, None, None, C.byref(lst)) == INVALID and b"dictionary" in lib.lifcal_ba_last_error()
    assert lib.lifcal_markers_components(C.byref(img), None, 0, None, None) == INVALID


def test_dictionaries_that_are_refused(built):
    refused(INVALID, markers.Dictionary, 2, [1])
    refused(INVALID, markers.Dictionary, 8, [1])
    refused(INVALID, markers.Dictionary, 4, [])
    refused(INVALID, markers.Dictionary, 3, [1 << 9])                   # a bit above marker_bits^2
    sym = markers.Dictionary(3, [0b000_010_000])                        # its own rotation: distance 0
    assert sym.min_distance == 0
    assert "coincide" in refused(INVALID, markers.checkMarkers, (50, 50), 8, sym)
    twice = markers.Dictionary(4, [0x1234, 0x0f11, mr.rot_word(0x1234, 4)])
    assert twice.min_distance == 0
    refused(INVALID, markers.Dictionary.generate, 2, 5)
    refused(INVALID, markers.Dictionary.generate, 4, 0)
    refused(INVALID, markers.Dictionary.generate, 4, 5000)
    refused(OUT_OF_RANGE, markers.Dictionary.generate, 3, 400)          # 512 words of nine bits do not hold 400 rotation classes


@pytest.mark.parametrize("m,n,seed", [(3, 10, 1), (4, 50, 1), (4, 250, 3), (5, 30, 7), (6, 250, 3), (7, 20, 0)])
def test_generator_and_distance(built, m, n, seed):
    want, dmin = mr.dictionary(m, n, seed)
    got = markers.Dictionary.generate(m, n, seed)
    assert got.words.tobytes() == want.tobytes() and got.min_distance == dmin >= 1
    assert np.array_equal(markers.Dictionary.from_bits(got.bits()).words, got.words)
    assert np.array_equal(got.bits()[1], mr.word_bits(int(want[1]) if n > 1 else 0, m)) or n == 1
    # the distance sees rotations: with one word replaced by a rotation of another it is 0
    if n > 2:
        w = want.copy(); w[n - 1] = mr.rot_word(int(w[0]), m)
        assert markers.Dictionary(m, w).min_distance == 0 == mr.dictionary_distance(w, m)


def test_constraints_reader(built, tmp_path):
    p = tmp_path / "constraints.txt"
    # a line of blanks only is not empty in the reference's sense: it is a malformed line
    p.write_text("7 3 0.25 0.001\n   \n")
    assert "line 2" in refused(INVALID, markers.readConstraints, p)
    p.write_text("# id1 id2 distance sigma\n\n7 3 0.25 0.001\n3 12 1.5e-1 2e-3\r\n#7 7 1 1\n 12 7 0.3 0.01  \n\n")
    got = markers.readConstraints(p)
    want = mr.read_constraints(p)
    for a, b in zip((got.id1, got.id2, got.distance, got.sigma, got.ids), want):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (a, b)
    assert got.n == 3 and got.ids.tolist() == [7, 3, 12]
    for text, line in (("1 2 0.5\n", "line 1"), ("1 2 0.5 0.1\n1 x 0.5 0.1\n", "line 2"), ("1 2 0.5 0.1 9\n", "line 1"), ("-1 2 0.5 0.1\n", "line 1"),
                       ("1 2 -0.5 0.1\n", "line 1"), ("1 2 0.5 0\n", "line 1"), ("1 2 nan 0.1\n", "line 1"), ("1.5 2 0.5 0.1\n", "line 1")):
        p.write_text(text)
        assert line in refused(INVALID, markers.readConstraints, p), text
    p.write_text("# nothing\n")
    assert markers.readConstraints(p).n == 0
    assert "cannot open" in refused(INVALID, markers.readConstraints, tmp_path / "missing.txt")


def _tracks(x, y, fr, pt):
    return Tracks(np.asarray(fr, np.uint32), np.asarray(pt, np.uint32), np.arange(len(x), dtype=np.uint32), np.asarray(x, np.float64), np.asarray(y, np.float64),
                  int(max(pt)) + 1 if len(pt) else 0, 0)


def _markers(ids, x, y):
    n = len(ids)
    z = np.zeros(n, np.int32)
    return markers.Markers(np.asarray(ids, np.int32), z, z, z + 1, z, z, np.zeros((n, 4, 2)), np.asarray(x, np.float64), np.asarray(y, np.float64))


def test_seeding_with_ties_and_add_markers(built):
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(6, 3))
    # frame 0: points at equal distance from marker 4 (the first in the list wins); frame 1 holds marker 9 first; frame 2 has no track
    tr = _tracks([10, 30, 20, 20, 50, 51, 70], [20, 20, 10, 30, 50, 50, 70], [0, 0, 0, 0, 1, 1, 1], [2, 3, 4, 5, 0, 1, 2])
    per_frame = [_markers([4], [20.0], [20.0]), _markers([9, 4], [50.4, 70.0], [50.0, 70.0]), _markers([9, 1], [5.0, 6.0], [5.0, 6.0])]
    ids, xyz, seeded = markers.seedMarkerPoints(per_frame, tr, pts)
    mx, my, mfr, mid = markers._marker_observations(per_frame)
    w_ids, w_xyz, w_seeded = mr.seed_points(mx, my, mfr, mid, tr.x, tr.y, tr.fr, tr.pt, pts)
    assert ids.tobytes() == w_ids.tobytes() and xyz.tobytes() == w_xyz.tobytes() and np.array_equal(seeded, w_seeded)
    assert ids.tolist() == [4, 9, 1] and seeded.tolist() == [True, True, False]
    assert np.array_equal(xyz[0], pts[2]) and np.array_equal(xyz[1], pts[0]) and np.all(xyz[2] == 0)
    # a marker whose later-listed observation has the lower frame is seeded from that frame
    ids, xyz, _ = markers.seedMarkerPoints([None, _markers([4], [70.0], [70.0]), None], tr, pts)
    assert ids.tolist() == [4] and np.array_equal(xyz[0], pts[2])
    lib = capi.load_library()
    refused(OUT_OF_RANGE, markers.seedMarkerPoints, per_frame, tr, pts[:5])
    assert lib.lifcal_markers_seed_points(0, None, None, None, None, 0, None, None, None, None, 0, None, None) == INVALID
    # addMarkers: marker observations in front, their ids kept; only the tracks whose ids clash (1 and 4) move, above every id
    out = markers.addMarkers(tr, [None] * 3, per_frame)
    assert out.pt[:5].tolist() == [4, 9, 4, 9, 1] and out.fr[:5].tolist() == [0, 1, 1, 2, 2] and np.all(out.feature[:5] == markers.NO_FEATURE)
    assert out.pt[5:].tolist() == [2, 3, 11, 5, 0, 10, 2] and out.x[5:].tolist() == tr.x.tolist() and out.n_tracks == 9
    assert out.track_ids.tolist() == [0, 10, 2, 3, 11, 5] and out.marker_ids.tolist() == [1, 4, 9] and out.n_points == 12
    # mergePoints: row = point id; tracks where addMarkers put them, seeded markers from their start values, NaN where no id is
    ids, xyz, seeded = markers.seedMarkerPoints(per_frame, tr, pts)
    merged = markers.mergePoints(out, pts, ids[seeded], xyz[seeded])
    assert merged.shape == (12, 3) and np.array_equal(merged[out.track_ids], pts)
    assert np.array_equal(merged[4], pts[2]) and np.array_equal(merged[9], pts[0])          # the seeds of markers 4 and 9
    assert np.isnan(merged[[1, 6, 7, 8]]).all() and np.isfinite(merged[[0, 2, 3, 4, 5, 9, 10, 11]]).all()   # marker 1 was not seeded
    for k in range(len(out.pt)):                                                            # every observation finds its own point
        if out.feature[k] != markers.NO_FEATURE:
            assert np.array_equal(merged[out.pt[k]], pts[tr.pt[k - 5]])
    with pytest.raises(ValueError):
        markers.mergePoints(out, pts[:5], ids, xyz)
    with pytest.raises(ValueError):
        markers.mergePoints(out, pts, [7], xyz[:1])
    v, p, f = markers.scaleScene(np.zeros((3, 6)), merged, 4, 9, 0.5)                       # the ids are rows now
    assert abs(np.linalg.norm(p[4] - p[9]) - 0.5) < 1e-15
    with pytest.raises(ValueError):
        markers.addMarkers(tr, [None] * 3, [_markers([4, 4], [1.0, 2.0], [1.0, 2.0]), None, None])


def test_scale_factor_and_scene(built):
    p1, p2 = np.array([0.1, -0.2, 3.0]), np.array([0.4, 0.2, 3.0])
    f = markers.sceneScaleFactor(p1, p2, 0.25)
    assert f == mr.scale_factor(p1, p2, 0.25) and abs(f - 0.5) < 1e-15
    refused(NUMERIC, markers.sceneScaleFactor, p1, p1, 0.25)
    refused(NUMERIC, markers.sceneScaleFactor, p1, p2 * np.nan, 0.25)
    refused(INVALID, markers.sceneScaleFactor, p1, p2, 0.0)
    refused(INVALID, markers.sceneScaleFactor, p1, p2, float("inf"))
    rng = np.random.default_rng(0)
    views, pts = rng.normal(size=(3, 6)), rng.normal(size=(5, 3))
    v, p, f = markers.scaleScene(views, pts, 1, 3, 0.75)
    assert abs(np.linalg.norm(p[1] - p[3]) - 0.75) < 1e-14 and np.allclose(p, f * pts, rtol=1e-15, atol=0)
    assert np.allclose(v[:, 3:], f * views[:, 3:], rtol=1e-14)     # t_f' = s t_f; the rotations are lifcal_align_apply's business


def test_detection_needs_a_device(built):
    """no CPU fallback: without a device the call fails with NO_DEVICE (on a machine with one it returns the restatement's markers)"""
    words, _ = mr.dictionary()
    img = mr.hand_marker(int(words[3]), 4)
    try:
        got = markers.detectMarkers(img, markers.Dictionary(4, words))
    except LifcalError as e:
        assert e.code == NO_DEVICE and "no CPU fallback" in str(e)
    else:
        assert got.id.tolist() == [3]

# ------------------------------------------------------------------------------------------------ renderer and accuracy


def test_renderer_truth():
    words, _ = mr.dictionary()
    m = mi.place(3, mr.word_bits(words[3], 4), 60.0, 50.0, 40, 30.0, 0.15, 45.0)
    c = m.corners
    # the centre is where the diagonals of the projected square meet, and is not the mean of the corners under perspective
    ctr = mr._meet(tuple(c[0]), tuple(c[2] - c[0]), tuple(c[1]), tuple(c[3] - c[1]))
    assert np.allclose(ctr, m.centre, atol=1e-9) and np.linalg.norm(c.mean(axis=0) - m.centre) > 0.3
    T = mi.marker_texture([m])
    assert T(*m.centre) in (0.0, 1.0) and T(5.0, 5.0) == 1.0
    u, v = m.image_of(0.5 / 6, 0.5)                  # the middle of a border cell
    assert T(u, v) == 0.0
    img16 = mi.render_markers((100, 120), [m], bits=16, blur=0.5, noise=1.0, shading=0.2, seed=1)
    assert img16.dtype == np.uint16 and img16.shape == (100, 120) and img16.max() > 40000 and img16.min() < 12000


def test_accuracy_of_the_restatement():
    """the rendered set (markers_reference.rendered_poses: sides 20 to 64, 12 rotations, two perspectives, blur, noise, shading)
    through the restatement alone: every marker found, none extra, and the centre errors that MEASURED records"""
    words, _ = mr.dictionary()
    per_image = [(mr.detect(img, words, 4)[0], placed) for img, placed in mr.rendered_set()]
    e = mr.evaluate(per_image)
    print(e)
    assert e["total"] == 24 and len(mr.rendered_set()) <= 6
    mr.check_conditions(e, "restatement")
    m = mr.MEASURED["rendered"]
    assert abs(e["rms"] - m["rms"]) <= 0.0005 and abs(e["max"] - m["max"]) <= 0.0005, (e, m)   # MEASURED is what is measured here
    # without the edge refinement the centre is an order of magnitude worse: the refinement is part of the feature
    coarse = mr.evaluate([(mr.detect(img, words, 4, refine_max=1e-9)[0], placed) for img, placed in mr.rendered_set()])
    print(coarse)
    assert coarse["refined"] == 0 and coarse["rms"] > 5 * e["rms"]


def test_accuracy_of_the_chain_restatement():
    """the chain's frames (marker texture -> render_raw_image -> total-focus restatement with the true depth) through the
    restatement of the detector: both markers in all three frames, and the centre errors that MEASURED records"""
    words, _ = mr.chain_dictionary()
    per_frame = []
    for k in range(mr.CHAIN_FRAMES):
        img, status = mr.chain_totalfocus_restated(k)
        per_frame.append(mr.detect(img, words, mr.CHAIN_BITS, status)[0])
    e = mr.evaluate_chain(per_frame)
    print(e)
    mr.check_chain_conditions(e, "restatement")
    m = mr.MEASURED["chain"]
    assert abs(e["rms"] - m["rms"]) <= 0.0005 and abs(e["max"] - m["max"]) <= 0.0005, (e, m)
