"""Geometric verification of feature matches, what needs no GPU: the exports and struct layouts of
include/lifcal_verify.h, the argument checks (they come before any device is touched), the sampler and the triad by hand, the
restatement's conditions on the scenes, the refit (lifcal_align_fit, host code) against a numpy Kabsch fit, Matches.filtered and
the linker on filtered matches.  (The host code itself runs under the sanitizers as a program of its own:
make -C lifcal_amd/csrc verify_host_check.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lifcal_amd
from lifcal_amd import _capi as capi, features, verify, LifcalError
from tests import verify_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = C.POINTER(C.c_uint64)


def as_arguments(sc):
    pts = verify.FeaturePoints(sc.points.offset, sc.points.xyz, sc.points.tol_lat, sc.points.tol_dep)
    m = features.Matches(sc.pairs, sc.pair_start, sc.mi, sc.mj, np.zeros(len(sc.mi), np.uint32))
    return pts, m


def library_fit(frm, to, w):
    """lifcal_align_fit as the `fit` of the restatement: the refit that lifcal_matches_verify runs"""
    frm = np.ascontiguousarray(frm, np.float64); to = np.ascontiguousarray(to, np.float64); w = np.ascontiguousarray(w, np.float64)
    al = capi.Alignment()
    rc = capi.load_library().lifcal_align_fit(len(w), capi.as_dptr(frm), capi.as_dptr(to), capi.as_dptr(w), 0, C.byref(al))
    if rc != 0:
        return False, None, None
    return True, np.array(al.R[:]).reshape(3, 3), np.array(al.t[:])


def reference(name, fit=vr.kabsch, **options):
    sc = vr.scene(name)
    key = ("verify", name, fit.__name__, tuple(sorted(options.items())))
    return vr.cached(key, lambda: vr.verify(sc.points, sc.pairs, sc.pair_start, sc.mi, sc.mj, fit=fit, **options))


def test_exports_and_layout(built):
    hdr = open(os.path.join(ROOT, "include", "lifcal_verify.h")).read()
    declared = set(re.findall(r"\b(lifcal_matches_[a-z_0-9]+)\s*\(", hdr))
    assert declared == set(capi.VERIFY_PROTOTYPES) and len(declared) == 2, declared ^ set(capi.VERIFY_PROTOTYPES)
    lib = capi.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in include/lifcal_verify.h but not exported"
    for name in ("featurePoints", "verifyMatches", "checkVerify", "FeaturePoints", "Verification"):
        assert hasattr(lifcal_amd, name)
    assert hasattr(features.Matches, "filtered")
    # sizes and offsets implied by include/lifcal_verify.h on LP64
    assert C.sizeof(capi.VerifyPoints) == 40 and capi.VerifyPoints.offset.offset == 8 and capi.VerifyPoints.tol_dep.offset == 32
    assert C.sizeof(capi.VerifyOptions) == 24 and capi.VerifyOptions.refine.offset == 12 and capi.VerifyOptions.min_ratio.offset == 16
    assert C.sizeof(capi.VerifyPair) == 136 and capi.VerifyPair.R.offset == 32 and capi.VerifyPair.t.offset == 104 and capi.VerifyPair.rms.offset == 128
    assert C.sizeof(capi.VerifyResult) == 40 and capi.VerifyResult.pair.offset == 24 and capi.VerifyResult.seconds.offset == 32
    assert verify.PAIR_DTYPE.itemsize == 136 and verify.PAIR_DTYPE == vr.PAIR_DTYPE
    for name, (_, offset) in [(n, verify.PAIR_DTYPE.fields[n][:2]) for n in verify.PAIR_DTYPE.names]:
        assert getattr(capi.VerifyPair, name).offset == offset, name
    # the defaults land where the ctypes view reads them
    o = verify.checkVerify(*as_arguments(vr.scene("edge")))
    assert (o.hypotheses, o.seed, o.min_inliers, o.refine, o.min_ratio) == (256, 0, 8, 2, 0.25)
    o = verify.checkVerify(*as_arguments(vr.scene("edge")), hypotheses=4096, seed=9, min_inliers=3, refine=-7, min_ratio=1.0)
    assert (o.hypotheses, o.seed, o.min_inliers, o.refine, o.min_ratio) == (4096, 9, 3, -1, 1.0)


def test_argument_errors(built):
    """every check runs before a device is looked for"""
    lib = capi.load_library()
    sc = vr.scene("rigid")
    base = dict(offset=sc.points.offset.copy(), xyz=sc.points.xyz, tol_lat=sc.points.tol_lat, tol_dep=sc.points.tol_dep, pairs=sc.pairs.copy(),
                start=sc.pair_start.copy(), mi=sc.mi.copy(), mj=sc.mj.copy())

    def check(null=(), no_points=False, **o):
        a = dict(base)
        opt = {k: o.pop(k) for k in list(o) if k in verify.OPTION_NAMES}
        a.update(o)
        ptr = lambda name, conv: None if name in null else conv(np.ascontiguousarray(a[name]))
        keep = {k: np.ascontiguousarray(v) for k, v in a.items()}
        a = keep
        vp = capi.VerifyPoints(len(a["offset"]) - 1, 0, ptr("offset", capi.as_uptr), ptr("xyz", capi.as_dptr), ptr("tol_lat", capi.as_dptr),
                               ptr("tol_dep", capi.as_dptr))
        vo = verify.make_verify_options(**opt)
        return lib.lifcal_matches_verify_check(None if no_points else C.byref(vp), len(a["pairs"]), ptr("pairs", capi.as_uptr),
                                               None if "start" in null else a["start"].ctypes.data_as(U64), ptr("mi", capi.as_uptr),
                                               ptr("mj", capi.as_uptr), C.byref(vo), None)

    assert check() == 0
    assert check(no_points=True) == -1 and b"no points" in lib.lifcal_ba_last_error()
    for name in ("offset", "xyz", "tol_lat", "tol_dep", "pairs", "start", "mi", "mj"):
        assert check(null=(name,)) == -1, name
    assert check(hypotheses=255) == -1 and check(hypotheses=300) == -1 and check(hypotheses=4352) == -1 and b"hypotheses" in lib.lifcal_ba_last_error()
    assert check(hypotheses=256) == 0 and check(hypotheses=4096) == 0
    assert check(min_ratio=-0.01) == -1 and check(min_ratio=1.01) == -1 and check(min_ratio=float("nan")) == -1 and b"min_ratio" in lib.lifcal_ba_last_error()
    assert check(min_ratio=1.0) == 0
    assert check(refine=5) == -1 and b"refine" in lib.lifcal_ba_last_error()
    assert check(refine=4) == 0 and check(refine=-3) == 0
    assert check(min_inliers=-1) == -1 and b"min_inliers" in lib.lifcal_ba_last_error()
    pairs = sc.pairs.copy(); pairs[1] = (2, 2)
    assert check(pairs=pairs) == -1 and b"twice" in lib.lifcal_ba_last_error()
    pairs = sc.pairs.copy(); pairs[2] = (0, 3)
    assert check(pairs=pairs) == -1 and b"out of range" in lib.lifcal_ba_last_error()
    mi = sc.mi.copy(); mi[5] = sc.counts[0]
    assert check(mi=mi) == -1 and b"feature out of range" in lib.lifcal_ba_last_error()
    mj = sc.mj.copy(); mj[-1] = 0xFFFFFFFF
    assert check(mj=mj) == -1 and b"feature out of range" in lib.lifcal_ba_last_error()
    start = sc.pair_start.copy(); start[1], start[2] = start[2], start[1]
    assert check(start=start) == -1 and b"descends" in lib.lifcal_ba_last_error()
    offset = sc.points.offset.copy(); offset[0] = 1
    assert check(offset=offset) == -1
    # the call itself makes the same checks first, and only then looks for a device
    pts, m = as_arguments(sc)
    with pytest.raises(LifcalError) as e:
        verify.verifyMatches(pts, m, hypotheses=300)
    assert e.value.code == -1


def test_sampler_by_hand():
    """the first draws of hypothesis 0 of pair 0 with seed 5, step by step"""
    s = (5 + 0x9E3779B9 + 0x85EBCA6B) % 2 ** 32
    assert s == 0x24234429
    draws = []
    for _ in range(3):
        s = (1664525 * s + 1013904223) % 2 ** 32
        draws.append((s * 1000) >> 32)
    assert len(set(draws)) == 3   # no repeat among these, so they are k0, k1, k2 as drawn
    assert vr.sample(5, 0, 4, 1000)[0].tolist() == draws
    # with m = 3 the redraws are exercised: always a permutation of 0, 1, 2
    k = vr.sample(1, 2, 512, 3)
    assert (np.sort(k, axis=1) == np.arange(3)).all()
    # states of different pairs and hypotheses differ
    assert len({tuple(r) for r in vr.sample(1, 0, 256, 10 ** 6)} | {tuple(r) for r in vr.sample(1, 1, 256, 10 ** 6)}) == 512


def test_triad_by_hand():
    q0, q1, q2 = np.array([[1.0, 2.0, 3.0]]), np.array([[4.0, 2.0, 3.0]]), np.array([[1.0, 6.0, 3.0]])
    e1, e2, e3, c, ok = vr.triad(q0, q1, q2)
    assert ok[0] and e1[0].tolist() == [1, 0, 0] and e2[0].tolist() == [0, 1, 0] and e3[0].tolist() == [0, 0, 1]
    assert c[0].tolist() == [2.0, 10.0 / 3.0, 3.0]
    assert not vr.triad(q0, q1, np.array([[7.0, 2.0, 3.0]]))[4][0]   # collinear
    assert not vr.triad(q0, q0, q2)[4][0]                            # a repeated point
    # a quarter turn about z and a shift, from one triple: the closed form gives it back exactly
    pa = np.concatenate([q0, q1, q2]); pb = np.stack([-pa[:, 1] + 10.0, pa[:, 0] - 20.0, pa[:, 2] + 5.0], axis=1)
    R, t, valid = vr.transforms(pa, pb, np.array([[0, 1, 2]]))
    assert valid[0] and R[0].tolist() == [[0, -1, 0], [1, 0, 0], [0, 0, 1]] and t[0].tolist() == [10.0, -20.0, 5.0]


@pytest.mark.parametrize("name", ["rigid", "moving"])
def test_scene_by_construction(name):
    """under the true motion every true match is an inlier and no planted or second-body match is"""
    sc = vr.scene(name)
    assert [int(sc.pair_start[p + 1] - sc.pair_start[p]) for p in range(3)] == [600, 257, 64]
    P = sc.points
    for p, (a, b) in enumerate(sc.pairs):
        s = slice(int(sc.pair_start[p]), int(sc.pair_start[p + 1]))
        gi = int(P.offset[a]) + sc.mi[s].astype(np.int64); gj = int(P.offset[b]) + sc.mj[s].astype(np.int64)
        keep, _, _ = vr.residuals(*sc.motion[p], P.xyz[gi], P.xyz[gj], P.tol_dep[gi] + P.tol_dep[gj], P.tol_lat[gi] + P.tol_lat[gj])
        assert keep[sc.kind[s] == 0].all() and not keep[sc.kind[s] != 0].any()
        planted = np.mean(sc.kind[s] == 1)
        assert 0.2 <= planted <= 0.4, planted


@pytest.mark.parametrize("name", ["rigid", "moving"])
def test_restatement_conditions(name):
    with np.errstate(all="raise"):
        res = reference(name)
    ev = vr.evaluate(vr.scene(name), res)
    print(name, ev)
    vr.check_conditions(ev, name)
    got = dict(kept_true=min(e["kept_true"] for e in ev), planted=max(e["planted"] for e in ev), motion=max(e["motion"] for e in ev))
    print(name, got)
    m = vr.MEASURED[name]
    assert got["kept_true"] == m["kept_true"] and got["planted"] == m["planted"] and abs(got["motion"] - m["motion"]) <= 0.05 * m["motion"], (got, m)


def test_restatement_edge():
    with np.errstate(all="raise"):
        res = reference("edge")
    assert tuple(res.pair["status"]) == vr.EDGE_EXPECTED
    assert tuple(res.pair["n_usable"][:8]) == vr.EDGE_USABLE and tuple(res.pair["n_matches"][:8]) == tuple(m + 3 for m in vr.EDGE_USABLE)
    for p in range(len(res.pair)):
        s = slice(int(vr.scene("edge").pair_start[p]), int(vr.scene("edge").pair_start[p + 1]))
        row = res.pair[p]
        assert res.keep[s].sum() == (row["n_inliers"] if row["status"] == vr.OK else 0)
        assert np.isnan(res.e_par[s]).sum() == (row["n_matches"] if row["status"] in (vr.FEW, vr.DEGENERATE) else row["n_matches"] - row["n_usable"])
    assert (res.pair["n_inliers"][5:8] == vr.EDGE_USABLE[5:]).all()


def refit_deviation():
    """lifcal_align_fit against the Kabsch fit on the inlier sets of the scenes' pairs: the largest |dR| (Frobenius) and |dt|"""
    dR = dt = 0.0
    for name in ("rigid", "moving", "edge"):
        sc, res = vr.scene(name), reference(name)
        P = sc.points
        for p, (a, b) in enumerate(sc.pairs):
            s = slice(int(sc.pair_start[p]), int(sc.pair_start[p + 1]))
            k = res.keep[s].astype(bool)
            if k.sum() < 3:
                continue
            gi = int(P.offset[a]) + sc.mi[s][k].astype(np.int64); gj = int(P.offset[b]) + sc.mj[s][k].astype(np.int64)
            w = 1.0 / (P.tol_dep[gi] + P.tol_dep[gj]) ** 2
            ok1, R1, t1 = library_fit(P.xyz[gi].reshape(-1), P.xyz[gj].reshape(-1), w)
            ok2, R2, t2 = vr.kabsch(P.xyz[gi], P.xyz[gj], w)
            assert ok1 and ok2
            dR = max(dR, float(np.linalg.norm(R1 - R2))); dt = max(dt, float(np.linalg.norm(t1 - t2)))
    return dR, dt


def test_refit_against_kabsch(built):
    """the bar is 100 times the largest deviation measured on the host that wrote MEASURED: both fits are closed forms in
    doubles, they differ by rounding only"""
    dR, dt = refit_deviation()
    print(f"refit: |dR| {dR:.3e}  |dt| {dt:.3e} mm")
    assert dR <= 100 * vr.MEASURED["refit"]["dR"] and dt <= 100 * vr.MEASURED["refit"]["dt"], (dR, dt)
    # a collinear inlier set is refused, which ends the refit rounds
    line = np.linspace(0.0, 1.0, 10)[:, None] * np.array([1.0, 2.0, 3.0])
    assert library_fit(line.reshape(-1), (line + 1.0).reshape(-1), np.ones(10))[0] is False
    assert vr.kabsch(line, line + 1.0, np.ones(10))[0] is False


def test_restatement_with_library_refit(built):
    """the conditions hold with the refit that the library runs, too"""
    for name in ("rigid", "moving"):
        res = reference(name, fit=library_fit)
        vr.check_conditions(vr.evaluate(vr.scene(name), res), name)
        assert (res.keep == reference(name).keep).all()


def test_filtered_and_linker(built):
    sc = vr.scene("rigid")
    pts, m = as_arguments(sc)
    res = reference("rigid")
    f = m.filtered(res.keep)
    assert f.pair_start.dtype == np.uint64 and f.pair_start[0] == 0 and f.pair_start[-1] == res.keep.sum() == len(f.i) == len(f.j) == len(f.dist)
    for p in range(3):
        s = slice(int(sc.pair_start[p]), int(sc.pair_start[p + 1]))
        k = res.keep[s].astype(bool)
        i, j, _ = f.of_pair(p)
        assert (i == sc.mi[s][k]).all() and (j == sc.mj[s][k]).all()
    assert len(m.filtered(np.zeros(len(m.i), bool)).i) == 0 and (m.filtered(np.ones(len(m.i), np.uint8)).pair_start == m.pair_start).all()
    with pytest.raises(ValueError):
        m.filtered(res.keep[:-1])
    feats = [features.Features(np.zeros(n), np.zeros(n), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n), np.zeros((n, 8), np.uint32))
             for n in sc.counts]
    N = 600   # features below N are scene points, those from N on are planted partners
    raw, clean = features.linkTracks(feats, m), features.linkTracks(feats, f)
    local = lambda t: t.feature - sc.points.offset[t.fr]
    assert (local(raw) >= N).sum() > 0
    assert (local(clean) >= N).sum() == 0 and clean.n_conflicts == 0
    # every track of the true matches alone is there again: the same scene points in the same frames
    true = features.linkTracks(feats, m.filtered(sc.kind == 0))
    assert clean.n_tracks == true.n_tracks and (clean.feature == true.feature).all() and (clean.pt == true.pt).all()

