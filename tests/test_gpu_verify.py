"""Geometric verification of feature matches on the GPU (include/lifcal_verify.h): lifcal_matches_verify
against the numpy restatement byte for byte after the hypothesis stage and after every refit round (the restatement refits with
the library's own lifcal_align_fit, so the fitted transform is an input and not a second eigen-solver's opinion), against itself
across calls, the issue's conditions on what the GPU gives, the statuses of the edge scene, the linker on raw and on filtered
matches, and the chain image -> features -> virtual depth -> metric points -> verified tracks."""
import numpy as np
import pytest

from lifcal_amd import depth, features, verify
from tests import depth_reference as dr
from tests import features_reference as fref
from tests import verify_reference as vr
from tests.test_verify_cpu import as_arguments, library_fit

pytestmark = pytest.mark.gpu

SEEDS = (1, 20241105)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def assert_equal_bytes(got, want, what):
    assert got.keep.dtype == np.uint8 and got.keep.tobytes() == want.keep.tobytes(), (what, "keep", np.flatnonzero(got.keep != want.keep)[:8])
    for f in ("e_par", "e_perp"):
        a, b = bits(getattr(got, f)), bits(getattr(want, f))
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (what, f, bad.size, bad[:8], getattr(got, f)[bad[:8]], getattr(want, f)[bad[:8]])
    for f in vr.PAIR_DTYPE.names:
        assert got.pair[f].tobytes() == want.pair[f].tobytes(), (what, f, got.pair[f], want.pair[f])
    assert got.pair.tobytes() == want.pair.tobytes(), what


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("hypotheses", (256, 512))
@pytest.mark.parametrize("name", ("rigid", "moving", "edge"))
def test_bytes_equal_the_restatement(built, name, hypotheses, seed):
    """best_hypothesis, n_inliers_hypothesis, keep, e_par, e_perp and the pair rows after the hypothesis stage (refine = -1) and
    after one, two and three refit rounds"""
    sc = vr.scene(name)
    pts, m = as_arguments(sc)
    for refine in (-1, 1, 2, 3):
        o = dict(hypotheses=hypotheses, seed=seed, refine=refine)
        got = verify.verifyMatches(pts, m, **o)
        want = vr.verify(sc.points, sc.pairs, sc.pair_start, sc.mi, sc.mj, fit=library_fit, **o)
        assert_equal_bytes(got, want, (name, o))
        assert got.seconds > 0.0
        assert (got.pair["rounds_used"] <= max(refine, 0)).all()
        if refine == 1 and name != "edge":
            assert (got.pair["rounds_used"] == 1).any()   # the comparison after a refit is of a refit that happened
    # the transforms of the refit are near the independent Kabsch fit's: same counts, same matches
    want = vr.verify(sc.points, sc.pairs, sc.pair_start, sc.mi, sc.mj, hypotheses=hypotheses, seed=seed, refine=3)
    assert (got.pair["status"] == want.pair["status"]).all() and (got.keep == want.keep).all()
    ok = got.pair["status"] == vr.OK
    assert np.abs(got.pair["R"][ok] - want.pair["R"][ok]).max() <= 100 * vr.MEASURED["refit"]["dR"]
    assert np.abs(got.pair["t"][ok] - want.pair["t"][ok]).max() <= 100 * vr.MEASURED["refit"]["dt"]


def test_same_bytes_across_calls(built):
    for name in ("rigid", "edge"):
        pts, m = as_arguments(vr.scene(name))
        a = verify.verifyMatches(pts, m, hypotheses=512, seed=3)
        b = verify.verifyMatches(pts, m, hypotheses=512, seed=3)
        assert_equal_bytes(a, b, name)
    pts, m = as_arguments(vr.scene("rigid"))
    a, c = verify.verifyMatches(pts, m, seed=3), verify.verifyMatches(pts, m, seed=4)
    assert c.pair["best_hypothesis"].tobytes() != a.pair["best_hypothesis"].tobytes()   # the seed is read


@pytest.mark.parametrize("name", ("rigid", "moving"))
def test_conditions_on_the_gpu(built, name):
    sc = vr.scene(name)
    got = verify.verifyMatches(*as_arguments(sc))
    ev = vr.evaluate(sc, got)
    print(name, ev, f"{got.seconds * 1e3:.3f} ms")
    vr.check_conditions(ev, name)


def test_edge_statuses(built):
    sc = vr.scene("edge")
    got = verify.verifyMatches(*as_arguments(sc))
    assert tuple(got.pair["status"]) == vr.EDGE_EXPECTED
    assert tuple(got.pair["n_usable"][:8]) == vr.EDGE_USABLE
    assert (got.pair["best_hypothesis"][[0, 1, 2, 8]] == vr.NO_HYPOTHESIS).all()
    assert (got.pair["n_inliers"][5:8] == vr.EDGE_USABLE[5:]).all()
    for p, row in enumerate(got.pair):
        s = slice(int(sc.pair_start[p]), int(sc.pair_start[p + 1]))
        assert got.keep[s].sum() == (row["n_inliers"] if row["status"] == vr.OK else 0)
        assert np.isnan(got.e_par[s]).sum() == (row["n_matches"] if row["status"] in (vr.FEW, vr.DEGENERATE) else row["n_matches"] - row["n_usable"])
    # a loose acceptance takes the three- and four-match pairs, a strict one refuses everything
    loose = verify.verifyMatches(*as_arguments(sc), min_inliers=3, min_ratio=1.0)
    assert tuple(loose.pair["status"][:8]) == (vr.FEW,) * 3 + (vr.OK,) * 5
    # no pairs, and pairs without matches
    pts, m = as_arguments(sc)
    none = verify.verifyMatches(pts, features.Matches(m.pairs[:0], np.zeros(1, np.uint64), m.i[:0], m.j[:0], m.dist[:0]))
    assert len(none.keep) == 0 and len(none.pair) == 0
    empty = verify.verifyMatches(pts, features.Matches(m.pairs[:2], np.zeros(3, np.uint64), m.i[:0], m.j[:0], m.dist[:0]))
    assert tuple(empty.pair["status"]) == (vr.FEW, vr.FEW) and empty.seconds == 0.0


def test_linker_on_filtered_matches(built):
    """on the raw matches of `rigid` the tracks hold planted observations; on the filtered ones none, and the true tracks stay"""
    sc = vr.scene("rigid")
    pts, m = as_arguments(sc)
    got = verify.verifyMatches(pts, m)
    feats = [features.Features(np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n), np.zeros((n, 8), np.uint32))
             for n in sc.counts]
    raw, clean = features.linkTracks(feats, m), features.linkTracks(feats, m.filtered(got.keep))
    true = features.linkTracks(feats, m.filtered(sc.kind == 0))
    local = lambda t: t.feature - sc.points.offset[t.fr]
    assert (local(raw) >= 600).sum() > 0 or raw.n_conflicts > 0
    assert (local(clean) >= 600).sum() == 0 and clean.n_conflicts == 0
    assert len(set(clean.feature.tolist()) & set(true.feature.tolist())) >= vr.KEPT_TRUE * len(true.feature)


# ---------------------------------------------------------------------------------------------------------------- the image chain
def chain_camera():
    """the scenes' camera without distortion, its principal point at the centre of the direct sequence's frames"""
    h, w = fref.DIRECT_SHAPE
    cam = np.zeros(17); cam[:5] = [35.0, 34.15, 0.40, (w - 1) / 2.0, (h - 1) / 2.0]
    return cam, 0x0, 0.011


def test_chain_through_track_sequence(built):
    """Frames of the direct sequence's kind under a warp of scale 1 (verify_reference.rigid_frame: the warp of d14 and of the
    direct sequence scales and so is not rigid), a fronto-parallel constant virtual depth, featurePoints inside
    trackSequence(verify=...).  tol_px = 0.75: the summed tolerance across the ray is the 1.5 pixels beyond which section 7w
    calls an observation wrong.  The verified tracks hold no wrong observation, and hardly any right one is lost."""
    h, w = fref.DIRECT_SHAPE
    images = [vr.rigid_frame(k) for k in range(vr.RIGID_FRAMES)]
    cam, config, spx = chain_camera()
    raw_value = dr.encode_vdepth(vr.RIGID_VDEPTH)
    with depth.DepthMaps(w, h, len(images)) as dm:
        dm.setMaps(np.full((len(images), h, w), raw_value, np.uint16))
        feats, m, raw = features.trackSequence(images)                      # verify=None: as ever
        feats2, m2, tracks, v = features.trackSequence(images, verify=dict(depth_maps=dm, cam=cam, config=config, spx=spx, tol_px=0.75))
        points = verify.featurePoints(feats, dm, cam, config, spx, tol_px=0.75)
        # a map that holds no depth: every feature NaN, every pair FEW
        dm.setMaps(np.zeros((len(images), h, w), np.uint16))
        blind = verify.featurePoints(feats, dm, cam, config, spx)
    assert all(a.x.tobytes() == b.x.tobytes() for a, b in zip(feats, feats2)) and m.i.tobytes() == m2.i.tobytes() and m.j.tobytes() == m2.j.tobytes()
    assert np.isnan(blind.xyz).all() and np.isnan(blind.tol_lat).all() and np.isnan(blind.tol_dep).all()
    assert (verify.verifyMatches(blind, m).pair["status"] == vr.FEW).all()
    # the points: the restatement of the back-projection, and the tolerances from its derivative and its neighbour
    x = np.concatenate([f.x for f in feats]); y = np.concatenate([f.y for f in feats])
    sampled, _ = dr.sample_ref(np.full((h, w), raw_value, np.uint16), x, y)
    vd = float(sampled[0])
    assert (sampled == vd).all() and abs(vd - vr.RIGID_VDEPTH) < 1e-3
    want = dr.back_project_cam(x, y, sampled, cam, config, spx)
    assert np.array_equal(points.xyz, want) and (points.tol_lat > 0).all() and (points.tol_dep > 0).all()
    beside = dr.back_project_cam(x + 1.0, y, np.full(len(x), vd), cam, config, spx)
    assert np.allclose(points.tol_lat, 0.75 * np.linalg.norm(beside - want, axis=1), rtol=1e-12)
    dz = (dr.back_project_cam(x, y, np.full(len(x), vd + 1e-6), cam, config, spx) - dr.back_project_cam(x, y, np.full(len(x), vd - 1e-6), cam, config, spx)) / 2e-6
    assert np.allclose(points.tol_dep, np.linalg.norm(dz, axis=1) * (4.0 / 65535.0) * vd * vd, rtol=1e-6)
    # trackSequence did what the three calls do
    again = verify.verifyMatches(points, m)
    assert again.keep.tobytes() == v.keep.tobytes() and again.pair.tobytes() == v.pair.tobytes()
    assert (v.pair["status"] == vr.OK).all(), v.pair["status"]
    e_raw, e = vr.evaluate_tracks(feats, raw, (h, w)), vr.evaluate_tracks(feats, tracks, (h, w))
    print(f"chain: features {[f.n for f in feats]}, {len(m.i)} matches, {int(v.keep.sum())} kept; raw {e_raw['tracks']} tracks, {e_raw['wrong']} wrong; "
          f"verified {e['tracks']} tracks, {e['wrong']} wrong, {e['conflicts']} conflicts; inliers {v.pair['n_inliers']}, rms {v.pair['rms']} mm, {v.seconds * 1e3:.3f} ms")
    assert e["wrong"] == 0 and not (set(tracks.feature.tolist()) & e_raw["wrong_obs"])
    assert len(e["right_obs"] & e_raw["right_obs"]) >= vr.KEPT_TRUE * len(e_raw["right_obs"])
    # matches spoilt on purpose: every seventh match gets another partner; none of them survives, the rest does
    j = m.j.copy()
    spoilt = np.zeros(len(j), bool)
    for p, (a, b) in enumerate(m.pairs):
        s = np.arange(int(m.pair_start[p]), int(m.pair_start[p + 1]))[::7]
        nb = feats[b].n
        far = np.array([int(np.argmax(np.hypot(feats[b].x - feats[b].x[j[k]], feats[b].y - feats[b].y[j[k]]))) for k in s])
        assert nb > 1
        j[s] = far; spoilt[s] = True
    vs = verify.verifyMatches(points, features.Matches(m.pairs, m.pair_start, m.i, j, m.dist))
    assert (vs.pair["status"] == vr.OK).all() and not vs.keep[spoilt].any()
    assert vs.keep[~spoilt].sum() >= vr.KEPT_TRUE * v.keep[~spoilt].sum()
