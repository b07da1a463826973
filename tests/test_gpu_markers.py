"""Fiducial markers on the GPU (include/lifcal_markers.h): lifcal_markers_components and lifcal_markers_detect
against the numpy restatement byte for byte (dark map, label map, candidate table, marker list), across calls and pointer kinds,
the labelling across tile seams, the quad choice, the decode and the refinement at their edges, and the issue's conditions and
accuracy on what the GPU returns."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

from lifcal_amd import marker_image as mi
from lifcal_amd import markers
from tests import markers_reference as mr

pytestmark = pytest.mark.gpu


def gpu_dictionary(m=4, n=50, seed=1):
    words, dmin = mr.dictionary(m, n, seed)
    return markers.Dictionary(m, words), words


def records(mk):
    rec = np.zeros(mk.n, mr.MARKER_DTYPE)
    for f in ("id", "rotation", "hamming", "refined", "label", "area", "corners", "x", "y"):
        rec[f] = getattr(mk, f)
    return rec


def check_components(img, status=None, what="", **opts):
    """dark map, label map and candidate table of the GPU equal the restatement's in every byte"""
    want_dark, want_labels, want_table = mr.components(img, status, **opts)
    got = markers.markerComponents(img, status, **opts)
    assert got.dark.dtype == want_dark.dtype and got.dark.tobytes() == want_dark.tobytes(), (what, "dark", np.argwhere(got.dark != want_dark)[:8])
    assert got.labels.dtype == want_labels.dtype and got.labels.tobytes() == want_labels.tobytes(), (what, "labels", np.argwhere(got.labels != want_labels)[:8])
    assert got.candidates.dtype == want_table.dtype, (what, got.candidates.dtype, want_table.dtype)
    assert got.candidates.tobytes() == want_table.tobytes(), (what, "table", got.candidates, want_table)
    return got


def check_detect(img, m=4, n=50, status=None, what="", seed=1, **opts):
    """the marker list of the GPU equals the restatement's in every byte; returns it as records"""
    d, words = gpu_dictionary(m, n, seed)
    want, want_nc = mr.detect(img, words, m, status, **opts)
    got = markers.detectMarkers(img, d, status, **opts)
    rec = records(got)
    assert got.n_candidates == want_nc, (what, got.n_candidates, want_nc)
    assert rec.tobytes() == want.tobytes(), (what, rec, want)
    return rec


def scene_203(bits):
    """203 x 131 (no multiple of any tile), three markers, a status map with a hole through one marker's border, in rows wider
    than the image"""
    words, _ = mr.dictionary()
    placed = [mi.place(5, mr.word_bits(words[5], 4), 48.3, 50.2, 44, 17.0, 0.1, 40.0), mi.place(9, mr.word_bits(words[9], 4), 120.7, 40.4, 30, 52.0),
              mi.place(21, mr.word_bits(words[21], 4), 150.2, 95.6, 36, 80.0, 0.12, 200.0)]
    img = mi.render_markers((131, 203), placed, bits=bits, blur=0.7, noise=1.5, shading=0.2, seed=7)
    wide = np.full((131, 240), 99, img.dtype)
    wide[:, :203] = img
    status = np.zeros((131, 203), np.uint8)
    status[::17, ::13] = 3                       # valid as well
    cx, cy = placed[1].corners[:2].mean(axis=0)  # the middle of marker 9's first edge
    status[int(cy) - 4:int(cy) + 5, int(cx) - 1:int(cx) + 2] = 1
    return wide[:, :203], status, placed


@pytest.mark.parametrize("bits", [8, 16])
def test_equal_bytes_with_the_restatement(built, bits):
    img, status, placed = scene_203(bits)
    assert img.strides[0] > img.shape[1] * img.itemsize
    first = check_components(img, status, what=bits)
    rec = check_detect(img, status=status, what=bits)
    # the hole takes dark pixels out of marker 9's border, which stays one component (a ring with a cut), so the marker is still read
    assert sorted(rec["id"]) == [5, 9, 21] and first.candidates["label"].tolist() == sorted(first.candidates["label"].tolist())
    plain = check_components(img, what=(bits, "no status"))
    lost = (plain.dark == 1) & (first.dark == 0)
    assert lost.sum() >= 10 and np.all(status[lost] == 1)
    assert sorted(check_detect(img, what=(bits, "no status"))["id"]) == [5, 9, 21]
    # two calls in a row
    again = markers.markerComponents(img, status)
    assert again.dark.tobytes() == first.dark.tobytes() and again.labels.tobytes() == first.labels.tobytes()
    assert again.candidates.tobytes() == first.candidates.tobytes()
    d, _ = gpu_dictionary()
    assert records(markers.detectMarkers(img, d, status)).tobytes() == rec.tobytes()


def test_device_pointers_through_torch_tensors(built):
    """image and status handed over as torch tensors on the device give the bytes of the host-pointer path.  Of two HIP runtimes in
    one process only the first to start sees the GPU; this process has the library's running already, so the check runs in a
    fresh one."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "markers_device_pointers.py")
    p = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300)
    print(p.stdout[-2000:], p.stderr[-2000:])
    assert p.returncode == 0 and "device pointers ok" in p.stdout


# ------------------------------------------------------------------------------------------------ labelling

def comb(shape=(96, 96)):
    """a spine along the bottom and one-pixel teeth up to the top, two pixels apart: every tooth crosses the horizontal seams, and
    the lowest index (the first tooth's tip) is far from where the teeth meet"""
    img = np.full(shape, 255, np.uint8)
    img[shape[0] - 3, 2:shape[1] - 2] = 0
    img[2:shape[0] - 3, 2:shape[1] - 2:3] = 0
    return img


def checkerboard(shape=(96, 96)):
    """dark pixels that touch only diagonally"""
    yy, xx = np.indices(shape)
    img = np.where((yy + xx) % 2 == 0, 0, 255).astype(np.uint8)
    img[[0, -1], :] = 255
    img[:, [0, -1]] = 255
    return img


def border_touchers(shape=(96, 96)):
    img = np.full(shape, 255, np.uint8)
    img[0:3, 10:40] = 0; img[-3:, 50:90] = 0; img[20:60, 0:3] = 0; img[30:80, -3:] = 0   # top, bottom, left, right
    img[40:60, 40:60] = 0; img[44:56, 44:56] = 255                                        # and a ring that touches none
    return img


def blocks_of(areas, shape=(64, 96)):
    """solid dark blocks, 8 wide, of the given areas (the last row of a block may be short)"""
    img = np.full(shape, 255, np.uint8)
    for k, a in enumerate(areas):
        x, y = 6 + 20 * k, 8
        for i in range(a):
            img[y + i // 8, x + i % 8] = 0
    return img


LABEL_SCENES = {
    "serpentine": lambda: mr.serpentine(),
    "comb": comb,
    "checkerboard": checkerboard,
    "borders": border_touchers,
    "all dark": lambda: np.zeros((70, 100), np.uint8),
    "all bright": lambda: np.full((70, 100), 255, np.uint8),
}


@pytest.mark.parametrize("name", list(LABEL_SCENES))
def test_labelling_across_seams(built, name):
    img = LABEL_SCENES[name]()
    got = check_components(img, what=name, min_side=2)
    n_labels = len(np.unique(got.labels[got.labels >= 0]))
    dark = img == 0
    if name in ("serpentine", "comb", "checkerboard"):
        # the thresholding makes exactly the drawn pixels dark, and they are one component whose label is its lowest index
        assert np.array_equal(got.dark.astype(bool), dark) and n_labels == 1
        assert got.labels[dark].min() == got.labels[dark].max() == np.flatnonzero(dark.ravel())[0]
        assert len(got.candidates) == 1 and got.candidates["area"][0] == dark.sum()
    elif name == "borders":
        assert n_labels == 5 and len(got.candidates) == 1 and got.candidates["x0"][0] == 40    # only the ring touches no border
    else:
        assert n_labels == 0 and len(got.candidates) == 0 and not got.dark.any()
    if name == "checkerboard":   # with 4-connectivity every pixel would be a component of its own
        assert got.candidates["area"][0] == dark.sum() > 4000


def test_components_of_min_area_and_one_less(built):
    img = blocks_of([32, 31, 33])
    got = check_components(img, what="areas", min_side=2)
    assert got.candidates["area"].tolist() == [32, 33]
    got = check_components(img, what="areas 33", min_side=2, min_area=33)
    assert got.candidates["area"].tolist() == [33]

# ------------------------------------------------------------------------------------------------ quad


def star(tips, shape=(64, 64), centre=(32, 32)):
    """one-pixel lines from the centre to the tips (offsets)"""
    img = np.full(shape, 255, np.uint8)
    for dx, dy in tips:
        n = max(abs(dx), abs(dy))
        for i in range(n + 1):
            img[centre[1] + int(round(dy * i / n)), centre[0] + int(round(dx * i / n))] = 0
    return img


@pytest.mark.parametrize("angle", [0.0, 22.5, 45.0, 67.5])
def test_quad_choice_on_rotated_squares(built, angle):
    """with a refine_max that no corner can meet the marker keeps the corners of step 4: at 0 degrees they come from the diagonal
    set (the axis set is degenerate), at 45 from the axis set, and in between from whichever is larger; all lie within 1.5 pixels
    of the true corners"""
    words, _ = mr.dictionary()
    placed = [mi.place(12, mr.word_bits(words[12], 4), 60.3, 58.6, 48, angle)]
    img = mi.render_markers((120, 120), placed, blur=0.5)
    rec = check_detect(img, what=angle, refine_max=1e-9)
    assert len(rec) == 1 and rec["id"][0] == 12 and rec["refined"][0] == 0
    assert np.all(np.abs(rec["corners"][0] - placed[0].corners) < 1.5), (rec["corners"][0], placed[0].corners)
    assert np.all(rec["corners"][0] * 2 == np.round(rec["corners"][0] * 2))                     # pixel centres moved by half a pixel or not at all
    rec = check_detect(img, what=(angle, "refined"))
    assert rec["refined"][0] == 1 and np.all(np.abs(rec["corners"][0] - placed[0].corners) < 0.25)


def test_quad_tie_and_min_side(built):
    # both corner sets have the double area 576: the candidate table is the restatement's and no marker comes of it
    tips = [(12, 0), (-12, 0), (0, 12), (0, -12), (8, 9), (-8, -9), (8, -9), (-8, 9)]
    img = star(tips)
    got = check_components(img, what="tie")
    ext = [tuple(e) for e in got.candidates["ext"][0]]
    assert mr.quad(ext, 12) == [(23.5, 22.5), (40.5, 22.5), (40.5, 41.5), (23.5, 41.5)]          # the diagonal set, moved outwards
    assert len(check_detect(img, what="tie")) == 0
    # a marker whose box is exactly 24 pixels wide
    words, _ = mr.dictionary()
    img = mr.hand_marker(int(words[7]), 4, cell=4)
    assert len(check_detect(img, what="min_side", min_side=24)) == 1
    assert len(check_detect(img, what="min_side - 1", min_side=25)) == 0

# ------------------------------------------------------------------------------------------------ decode


def flipped(word, bits):
    for b in bits:
        word ^= 1 << b
    return word


def test_decode_correction_and_border(built):
    words, dmin = mr.dictionary()
    bound = (dmin - 1) // 2
    assert bound >= 1
    w = int(words[17])
    rec = check_detect(mr.hand_marker(flipped(w, range(bound)), 4, angle_quarter=2), what="max_correction flips")
    assert len(rec) == 1 and (rec["id"][0], rec["rotation"][0], rec["hamming"][0]) == (17, 2, bound)
    assert len(check_detect(mr.hand_marker(flipped(w, range(bound + 1)), 4, angle_quarter=2), what="one flip more")) == 0
    assert len(check_detect(mr.hand_marker(flipped(w, [3]), 4), what="exact only", max_correction=-1)) == 0
    # one white border cell
    img = mr.hand_marker(w, 4)
    img[12 + 6 * 2:12 + 6 * 3, 12:18] = 230          # cell (2, 0)
    assert len(check_detect(img, what="border 0")) == 0
    rec = check_detect(img, what="border 1", max_border_errors=1)
    assert len(rec) == 1 and rec["id"][0] == 17


def test_marker_at_the_image_border_and_twice(built):
    words, _ = mr.dictionary()
    # two pixels from the border: the outward samples of the refinement leave the image and are skipped
    img = mr.hand_marker(int(words[30]), 4, margin=2)
    rec = check_detect(img, what="margin 2")
    assert len(rec) == 1 and rec["id"][0] == 30 and rec["refined"][0] == 1
    assert len(check_detect(mr.hand_marker(int(words[30]), 4, margin=0), what="margin 0")) == 0          # the box touches the border
    # the same id twice: listed twice, and unique() keeps the first with a warning
    img = np.concatenate([mr.hand_marker(int(words[30]), 4), mr.hand_marker(int(words[30]), 4, angle_quarter=1)], axis=1)
    rec = check_detect(img, what="twice")
    assert rec["id"].tolist() == [30, 30] and sorted(rec["rotation"].tolist()) == [0, 1]
    d, _ = gpu_dictionary()
    both = markers.detectMarkers(img, d)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        one = both.unique()
    assert one.n == 1 and one.label[0] == both.label[0] and len(caught) == 1 and "30" in str(caught[0].message)


@pytest.mark.parametrize("m,n", [(4, 1), (4, 250), (6, 1), (6, 250)])
def test_dictionary_sizes(built, m, n):
    """one word and 250 words at 36 and 64 cells: the lane loops over the entries and over the cells"""
    words, dmin = mr.dictionary(m, n, 3)
    j = n - 1
    img = mr.hand_marker(int(words[j]), m, cell=5, angle_quarter=3)
    rec = check_detect(img, m=m, n=n, seed=3, what=(m, n))
    assert len(rec) == 1 and (rec["id"][0], rec["rotation"][0], rec["hamming"][0]) == (j, 3, 0)

# ------------------------------------------------------------------------------------------------ refinement


def test_refinement_all_or_nothing(built):
    words, _ = mr.dictionary()
    clean = mr.hand_marker(int(words[2]), 4, cell=10, margin=15)
    rec = check_detect(clean, what="clean")
    assert rec["refined"][0] == 1
    # a dark bar along the middle of the top edge, 5 pixels thick: no station of that edge sees a crossing within 4 pixels
    img = clean.copy()
    img[10:15, 15 + 7:15 + 60 - 7] = 20
    rec = check_detect(img, what="occluded")
    assert len(rec) == 1 and rec["id"][0] == 2 and rec["refined"][0] == 0
    assert rec["corners"][0].tolist() == [[14.5, 14.5], [74.5, 14.5], [74.5, 74.5], [14.5, 74.5]]
    # refine_max binding: the corners of a blurred marker move by a good part of a pixel
    placed = [mi.place(2, mr.word_bits(words[2], 4), 50.4, 50.7, 40, 10.0)]
    blurred = mi.render_markers((100, 100), placed, blur=0.8)
    free = check_detect(blurred, what="free")
    bound = check_detect(blurred, what="bound", refine_max=0.05)
    assert free["refined"][0] == 1 and bound["refined"][0] == 0
    moved = np.sqrt(((free["corners"][0] - bound["corners"][0]) ** 2).sum(axis=1))
    assert moved.max() > 0.05 and moved.max() < 3.0

# ------------------------------------------------------------------------------------------------ conditions and accuracy


def test_conditions_and_accuracy_on_the_rendered_set(built):
    per_image = []
    for k, (img, placed) in enumerate(mr.rendered_set()):
        check_components(img, what=("rendered", k))
        per_image.append((check_detect(img, what=("rendered", k)), placed))
    e = mr.evaluate(per_image)
    print(e, mr.BARS)
    mr.check_conditions(e, "rendered set on the GPU")


def test_chain_markers_through_the_raw_image(built):
    """a marker texture -> render_raw_image -> lifcal_totalfocus_render on the GPU with its status map -> detectMarkers: both ids in
    all three frames of the chain's warp, the list equal to the restatement's on the same total-focus image, the centres against
    the truth under the protocol of the rendered set"""
    from lifcal_amd import MicroLensGrid
    from tests import rawdepth_reference as ref
    from tests import totalfocus_reference as tref
    g = MicroLensGrid(*ref.grid_arguments(mr.CHAIN_CASE))
    words, _ = mr.chain_dictionary()
    d = markers.Dictionary(mr.CHAIN_BITS, words)
    per_frame = []
    for k in range(mr.CHAIN_FRAMES):
        tf = g.totalFocusImage(mr.chain_raw(k), tref.true_depth(mr.CHAIN_CASE, "mid", 1))
        rec = records(markers.detectMarkers(tf.image, d, tf.status))
        want, _ = mr.detect(np.asarray(tf.image), words, mr.CHAIN_BITS, np.asarray(tf.status))
        assert rec.tobytes() == want.tobytes(), (k, rec, want)
        assert sorted(rec["id"].tolist()) == [1, 4], (k, rec)
        per_frame.append(rec)
    e = mr.evaluate_chain(per_frame)
    print(e, mr.BARS["chain"])
    mr.check_chain_conditions(e, "chain on the GPU")


def test_chain_tracks_markers_scale_and_solver(built, tmp_path):
    """three frames of the chain: trackSequence on the total-focus images, registerScene for the tracks' poses and points,
    seedMarkerPoints + addMarkers + mergePoints, scaleScene by the first constraint of a constraints file: the two markers of
    that constraint are then `distance` apart to rounding, and BundleAdjustment takes the scene with use_constraints = 1 (created,
    one sweep, finite cost).  The camera is test_gpu_verify's chain camera; the virtual depth is the scene's (4 throughout)."""
    from lifcal_amd import BundleAdjustment, MicroLensGrid, _capi as capi, features, registerScene
    from tests import rawdepth_reference as ref
    from tests import totalfocus_reference as tref
    name = mr.CHAIN_CASE
    w, h = ref.CASES[name][:2]
    g = MicroLensGrid(*ref.grid_arguments(name))
    tfs = [g.totalFocusImage(mr.chain_raw(k), tref.true_depth(name, "mid", 1)) for k in range(mr.CHAIN_FRAMES)]
    images, statuses = [tf.image for tf in tfs], [tf.status for tf in tfs]
    words, _ = mr.chain_dictionary()
    per_frame = markers.detectMarkerSequence(images, markers.Dictionary(mr.CHAIN_BITS, words), statuses)
    assert [sorted(mk.id.tolist()) for mk in per_frame] == [[1, 4]] * mr.CHAIN_FRAMES
    path = tmp_path / "constraints.txt"
    path.write_text("# id1 id2 distance sigma\n1 4 0.25 0.001\n")
    con = markers.readConstraints(path)
    # tracks, and their poses and points from the micro-image rays
    feats, _, tracks = features.trackSequence(images, statuses)
    assert tracks.n_tracks >= 10
    cam = np.zeros(17); cam[:5] = [35.0, 34.15, 0.40, (w - 1) / 2.0, (h - 1) / 2.0]
    config, spx, vdepth = 0x0, 0.011, ref.SCENE_DEPTHS[name]["mid"]
    obs = g.projectPointsToRawImage(tracks.x, tracks.y, np.full(len(tracks.x), vdepth), 1, fr=tracks.fr, pt=tracks.pt)
    r = registerScene(cam, obs.u, obs.v, obs.mcx, obs.mcy, obs.pt, obs.fr, mr.CHAIN_FRAMES, tracks.n_tracks, config, spx, 1)
    assert r.registered.all() and r.mapped.all()
    # the markers join: start values, ids as point ids, one point array whose rows are the ids
    ids, xyz, seeded = markers.seedMarkerPoints(per_frame, tracks, r.pts)
    assert sorted(ids.tolist()) == [1, 4] and seeded.all()
    marked = markers.addMarkers(tracks, feats, per_frame)
    assert marked.pt[:2 * mr.CHAIN_FRAMES].tolist() == [i for mk in per_frame for i in mk.id.tolist()]
    assert np.flatnonzero(marked.track_ids != np.arange(tracks.n_tracks)).tolist() == [1, 4] and marked.n_points == tracks.n_tracks + 2
    pts = markers.mergePoints(marked, r.pts, ids, xyz)
    assert np.isfinite(pts).all() and np.array_equal(pts[marked.track_ids], r.pts)
    views, pts, factor = markers.scaleScene(r.views, pts, con.id1[0], con.id2[0], con.distance[0])
    # to rounding: every scaled coordinate is half an ulp off at most, so a coordinate difference one ulp of the largest coordinate
    # and the distance sqrt(3) of that; twice that, and four ulps of the distance for the factor itself
    bound = 2 * np.sqrt(3) * np.spacing(np.abs(pts[[1, 4]]).max()) + 4 * np.finfo(float).eps * con.distance[0]
    got = np.linalg.norm(pts[1] - pts[4])
    print(f"{tracks.n_tracks} tracks, factor {factor:.6g}, distance {got!r} against {con.distance[0]!r}, bound {bound:.2e}")
    assert abs(got - con.distance[0]) <= bound
    # the solver takes it with the constraint switched on
    ob = g.projectPointsToRawImage(marked.x, marked.y, np.full(len(marked.x), vdepth), 1, fr=marked.fr, pt=marked.pt)
    pa = capi.ProblemArrays(ob.u, ob.v, ob.mcx, ob.mcy, ob.pt, ob.fr, cam, views.reshape(-1), pts.reshape(-1), spx, 1, config,
                            c_i=con.id1, c_j=con.id2, c_dist=con.distance, c_sigma=con.sigma, use_constraints=1)
    assert pa.struct.n_constraints == 1 and pa.struct.n_points == marked.n_points
    with BundleAdjustment(pa) as ba:
        cost = ba.sweep(1e4).cost
    print("cost of the first sweep", cost)
    assert np.isfinite(cost) and cost > 0.0
