"""The rule of include/lifcal_verify.h in plain numpy, and the synthetic scenes of its tests.

Loops over pairs, vectorised over hypotheses and matches.  Every sum is written out in the header's order (no einsum, no dot),
square roots and divisions are numpy's correctly rounded ones, and nothing is computed that would raise a floating-point flag:
invalid hypotheses are masked before they are divided.  The refit is an input: `fit(from, to, w)` returns (ok, R, t).  The GPU
tests pass the library's lifcal_align_fit there, so that every stage's bytes can be compared without asking two eigen-solvers
for equal bits; `kabsch` (SVD) is the independent fit that checks the refit itself, to a tolerance.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

OK, FEW, DEGENERATE, REJECTED = 0, 1, 2, 3
NO_HYPOTHESIS = 0xFFFFFFFF
DEFAULTS = dict(hypotheses=256, seed=0, min_inliers=8, refine=2, min_ratio=0.25)
PAIR_DTYPE = np.dtype([("status", "<u4"), ("n_matches", "<u4"), ("n_usable", "<u4"), ("best_hypothesis", "<u4"), ("n_inliers_hypothesis", "<u4"),
                       ("n_inliers", "<u4"), ("rounds_used", "<u4"), ("reserved", "<u4"), ("R", "<f8", (9,)), ("t", "<f8", (3,)), ("rms", "<f8")])
assert PAIR_DTYPE.itemsize == 136


@dataclass
class Points:
    """per feature of the concatenated list: offset (F + 1,) uint32, xyz (N, 3), tol_lat (N,), tol_dep (N,)"""
    offset: np.ndarray
    xyz: np.ndarray
    tol_lat: np.ndarray
    tol_dep: np.ndarray


@dataclass
class Result:
    keep: np.ndarray
    e_par: np.ndarray
    e_perp: np.ndarray
    pair: np.ndarray


# ---------------------------------------------------------------------------------------------------------------- the rule
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def usable(points: Points) -> np.ndarray:
    xyz = np.asarray(points.xyz, np.float64).reshape(-1, 3)
    fin = np.isfinite(xyz).all(axis=1) & np.isfinite(points.tol_lat) & np.isfinite(points.tol_dep)
    ok = fin.copy()
    ok[fin] = (xyz[fin, 2] > 0.0) & (points.tol_lat[fin] > 0.0) & (points.tol_dep[fin] > 0.0)
    return ok


def sample(seed: int, p: int, H: int, m: int) -> np.ndarray:
    """(H, 3) indices into the usable list of pair p; m >= 3"""
    M32 = np.uint64(0xFFFFFFFF)
    h = np.arange(H, dtype=np.uint64)
    s = (np.uint64(seed) + np.uint64((0x9E3779B9 * (p + 1)) & 0xFFFFFFFF) + ((np.uint64(0x85EBCA6B) * (h + np.uint64(1))) & M32)) & M32

    def draw(s, sel):
        s = s.copy()
        s[sel] = (np.uint64(1664525) * s[sel] + np.uint64(1013904223)) & M32
        return s, (s * np.uint64(m)) >> np.uint64(32)

    every = np.ones(H, bool)
    s, k0 = draw(s, every)
    s, k1 = draw(s, every)
    while True:
        again = k1 == k0
        if not again.any():
            break
        s, v = draw(s, again)
        k1[again] = v[again]
    s, k2 = draw(s, every)
    while True:
        again = (k2 == k0) | (k2 == k1)
        if not again.any():
            break
        s, v = draw(s, again)
        k2[again] = v[again]
    return np.stack([k0, k1, k2], axis=1).astype(np.int64)


def triad(q0, q1, q2):
    """e1, e2, e3, c, ok over the leading axes; where not ok the vectors are those of a stand-in triple"""
    d1, d2 = q1 - q0, q2 - q0
    n = cross3(d1, d2)
    l1, l2, ln = dot3(d1, d1), dot3(d2, d2), dot3(n, n)
    ok = ln > (1.0e-6 * l1) * l2
    d1 = np.where(ok[..., None], d1, np.array([1.0, 0.0, 0.0]))
    n = np.where(ok[..., None], n, np.array([0.0, 0.0, 1.0]))
    l1 = np.where(ok, l1, 1.0); ln = np.where(ok, ln, 1.0)
    e1 = d1 / np.sqrt(l1)[..., None]
    e3 = n / np.sqrt(ln)[..., None]
    e2 = cross3(e3, e1)
    c = ((q0 + q1) + q2) / 3.0
    return e1, e2, e3, c, ok


def transforms(pa, pb, k):
    """the hypotheses of the samples k (H, 3) over the usable points pa, pb (m, 3): R (H, 3, 3), t (H, 3), valid (H,)"""
    a1, a2, a3, ca, oka = triad(pa[k[:, 0]], pa[k[:, 1]], pa[k[:, 2]])
    b1, b2, b3, cb, okb = triad(pb[k[:, 0]], pb[k[:, 1]], pb[k[:, 2]])
    R = (b1[:, :, None] * a1[:, None, :] + b2[:, :, None] * a2[:, None, :]) + b3[:, :, None] * a3[:, None, :]
    t = cb - np.stack([dot3(R[:, r, :], ca) for r in range(3)], axis=1)
    valid = oka & okb & np.isfinite(R).all(axis=(1, 2)) & np.isfinite(t).all(axis=1)
    return R, t, valid


def residuals(R, t, pa, pb, td, tl):
    """the inlier test of the usable matches (m) under the transforms R (..., 3, 3), t (..., 3): keep, e_par, e_perp of shape
    (..., m)"""
    R = np.asarray(R, np.float64); t = np.asarray(t, np.float64)
    lead = R.shape[:-2]
    Rb = R.reshape(lead + (1, 3, 3)); tb = t.reshape(lead + (1, 3))
    e = np.stack([(dot3(Rb[..., r, :], pa) + tb[..., r]) - pb[:, r] for r in range(3)], axis=-1)
    r = pb / np.sqrt(dot3(pb, pb))[:, None]
    par = dot3(e, r)
    perp = np.sqrt(np.maximum(0.0, dot3(e, e) - par * par))
    return (np.abs(par) <= td) & (perp <= tl), par, perp


def kabsch(frm, to, w):
    """weighted rigid fit by SVD: (ok, R (3, 3), t (3,)) of to ~ R frm + t; not ok for fewer than three or collinear points"""
    frm = np.asarray(frm, np.float64).reshape(-1, 3); to = np.asarray(to, np.float64).reshape(-1, 3); w = np.asarray(w, np.float64)
    if len(frm) < 3:
        return False, None, None
    W = w.sum()
    cf = (w[:, None] * frm).sum(axis=0) / W; ct = (w[:, None] * to).sum(axis=0) / W
    f, g = frm - cf, to - ct
    for s in (f, g):
        ev = np.linalg.eigvalsh((w[:, None] * s).T @ s)
        if not ev[2] > 0.0 or ev[1] < 1e-12 * ev[2]:
            return False, None, None
    U, _, Vt = np.linalg.svd((w[:, None] * g).T @ f)
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    R = U @ D @ Vt
    return True, R, ct - R @ cf


def verify(points: Points, pairs, pair_start, mi, mj, fit=kabsch, **options) -> Result:
    """include/lifcal_verify.h, stage by stage"""
    o = dict(DEFAULTS)
    for k, v in options.items():
        if k not in o:
            raise TypeError(k)
        if v != 0:
            o[k] = v
    H, seed, refine = int(o["hypotheses"]), int(o["seed"]), max(int(o["refine"]), 0)
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    start = np.asarray(pair_start, np.uint64).astype(np.int64)
    mi = np.asarray(mi, np.int64); mj = np.asarray(mj, np.int64)
    n = int(start[-1]) if len(pairs) else 0
    xyz = np.asarray(points.xyz, np.float64).reshape(-1, 3)
    good = usable(points)
    keep = np.zeros(n, np.uint8); e_par = np.full(n, np.nan); e_perp = np.full(n, np.nan)
    rows = np.zeros(len(pairs), PAIR_DTYPE)
    for p, (fa, fb) in enumerate(pairs):
        row = rows[p]
        ks = np.arange(start[p], start[p + 1])
        gi = int(points.offset[fa]) + mi[ks]; gj = int(points.offset[fb]) + mj[ks]
        u = good[gi] & good[gj]
        ks, gi, gj = ks[u], gi[u], gj[u]
        m = len(ks)
        row["status"] = FEW; row["n_matches"] = int(start[p + 1] - start[p]); row["n_usable"] = m
        row["best_hypothesis"] = NO_HYPOTHESIS
        if m < 3:
            continue
        pa, pb = xyz[gi], xyz[gj]
        td = points.tol_dep[gi] + points.tol_dep[gj]; tl = points.tol_lat[gi] + points.tol_lat[gj]
        R, t, valid = transforms(pa, pb, sample(seed, p, H, m))
        if not valid.any():
            row["status"] = DEGENERATE
            continue
        R = np.where(valid[:, None, None], R, 0.0); t = np.where(valid[:, None], t, 0.0)
        counts = residuals(R, t, pa, pb, td, tl)[0].sum(axis=1)
        counts = np.where(valid, counts, -1)
        best = int(np.argmax(counts))   # the first of equals
        row["best_hypothesis"] = best; row["n_inliers_hypothesis"] = int(counts[best])
        Rc, tc = R[best], t[best]
        kc, par, perp = residuals(Rc, tc, pa, pb, td, tl)
        rounds = 0
        for _ in range(refine):
            ok, Rn, tn = fit(pa[kc].reshape(-1), pb[kc].reshape(-1), 1.0 / (td[kc] * td[kc]))
            if not ok:
                break
            kn, parn, perpn = residuals(Rn, tn, pa, pb, td, tl)
            if kn.sum() < kc.sum():
                break
            Rc, tc, kc, par, perp = np.asarray(Rn, np.float64), np.asarray(tn, np.float64), kn, parn, perpn
            rounds += 1
        cnt = int(kc.sum())
        good_pair = cnt >= int(o["min_inliers"]) and not (float(cnt) < float(o["min_ratio"]) * float(m))
        row["status"] = OK if good_pair else REJECTED
        row["n_inliers"] = cnt; row["rounds_used"] = rounds
        row["R"] = np.asarray(Rc).reshape(9); row["t"] = tc
        S = 0.0
        for a, b in zip(par[kc], perp[kc]):   # in order, one term after the other
            S = S + (a * a + b * b)
        row["rms"] = math.sqrt(S / float(cnt)) if cnt else 0.0
        e_par[ks] = par; e_perp[ks] = perp
        if good_pair:
            keep[ks] = kc
    return Result(keep, e_par, e_perp, rows)


# ---------------------------------------------------------------------------------------------------------------- scenes
@dataclass
class Scene:
    points: Points
    pairs: np.ndarray        # (P, 2) uint32
    pair_start: np.ndarray   # (P + 1,) uint64
    mi: np.ndarray
    mj: np.ndarray
    kind: np.ndarray         # per match: 0 a true match of the dominant body, 1 planted, 2 a match of the second body
    motion: list             # per pair: (R, t) of the dominant body, p_b = R p_a + t
    clean: list              # per pair: the noise-free p_a of its matches
    counts: tuple            # features per frame


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _random_motion(rng, max_deg, max_mm):
    return _rotation(rng.normal(size=3), math.radians(max_deg) * rng.uniform(0.5, 1.0)), _unit(rng.normal(size=3)) * max_mm * rng.uniform(0.5, 1.0)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def tolerances(xyz):
    z = xyz[:, 2]
    return 1.0e-3 * z, 2.0e-6 * z * z   # tol_lat, tol_dep


def _noisy(rng, xyz):
    """noise uniform within a third of each tolerance, along and across the ray"""
    tl, tdp = tolerances(xyz)
    r = _unit(xyz)
    side = rng.normal(size=xyz.shape)
    side = _unit(side - (side * r).sum(axis=1, keepdims=True) * r)
    return xyz + r * (rng.uniform(-1, 1, len(xyz)) * tdp / 3.0)[:, None] + side * (rng.uniform(0, 1, len(xyz)) * tl / 3.0)[:, None]


def make_motion_scene(moving: bool, seed: int = 7, sizes=(600, 257, 64), planted: float = 0.3) -> Scene:
    """`rigid` (moving = False) and `moving`: 3 frames, the pairs (0, 1), (1, 2), (0, 2) with sizes[] matches.  Points uniform in
    a frustum, Z from 300 to 1500 mm; frame f sees them through a motion of up to 5 degrees and 40 mm; with `moving` a quarter of
    the points ride on a second body with a further motion per frame.  A share `planted` of the matches of every pair get as
    their partner an extra feature: the true partner displaced by 5 to 10 summed tolerances, along or across the ray."""
    rng = np.random.default_rng(seed)
    N = max(sizes)
    Z = rng.uniform(300.0, 1500.0, N)
    X = np.stack([Z * rng.uniform(-0.3, 0.3, N), Z * rng.uniform(-0.2, 0.2, N), Z], axis=1)
    second = (rng.uniform(size=N) < 0.25) if moving else np.zeros(N, bool)
    frames = [(np.eye(3), np.zeros(3))] + [_random_motion(rng, 5.0, 40.0) for _ in range(2)]
    extra = [(np.eye(3), np.zeros(3))] + [_random_motion(rng, 4.0, 60.0) for _ in range(2)]
    true_xyz = []
    for f in range(3):
        Rf, tf = frames[f]
        P = X @ Rf.T + tf
        Re, te = extra[f]
        P[second] = (X[second] @ Re.T + te) @ Rf.T + tf
        true_xyz.append(P)
    noisy = [_noisy(rng, P) for P in true_xyz]
    extras = [[] for _ in range(3)]   # planted partners, appended to their frame's features
    pairs = np.array([(0, 1), (1, 2), (0, 2)], np.uint32)
    mi, mj, kind, start, motion, clean = [], [], [], [0], [], []
    for p, (a, b) in enumerate(pairs):
        sel = np.sort(rng.choice(N, sizes[p], replace=False))
        is_planted = rng.uniform(size=len(sel)) < planted
        for i, pl in zip(sel, is_planted):
            mi.append(i)
            if not pl:
                mj.append(i); kind.append(2 if second[i] else 0)
                continue
            q = true_xyz[b][i]
            tl_a, td_a = tolerances(true_xyz[a][i][None]); tl_b, td_b = tolerances(q[None])
            r = _unit(q)
            if rng.uniform() < 0.5:
                q2 = q + r * rng.choice([-1.0, 1.0]) * rng.uniform(5.0, 10.0) * float(td_a[0] + td_b[0])
            else:
                side = rng.normal(size=3); side = _unit(side - (side @ r) * r)
                q2 = q + side * rng.uniform(5.0, 10.0) * float(tl_a[0] + tl_b[0])
            mj.append(N + len(extras[b])); extras[b].append(q2); kind.append(1)
        start.append(len(mi))
        Ra, ta = frames[a]; Rb, tb = frames[b]
        Rab = Rb @ Ra.T
        motion.append((Rab, tb - Rab @ ta))
        clean.append(true_xyz[a][sel])
    xyz, counts = [], []
    for f in range(3):
        ex = np.array(extras[f]).reshape(-1, 3)
        xyz.append(np.concatenate([noisy[f], _noisy(rng, ex) if len(ex) else ex]))
        counts.append(len(xyz[-1]))
    xyz = np.ascontiguousarray(np.concatenate(xyz))
    offset = np.zeros(4, np.uint32); offset[1:] = np.cumsum(counts)
    # the tolerances a caller would state: from the measured (noisy) depth
    tl, tdp = tolerances(xyz)
    return Scene(Points(offset, xyz, np.ascontiguousarray(tl), np.ascontiguousarray(tdp)), pairs, np.array(start, np.uint64),
                 np.array(mi, np.uint32), np.array(mj, np.uint32), np.array(kind, np.uint8), motion, clean, tuple(counts))


EDGE_USABLE = (0, 1, 2, 3, 4, 255, 256, 257)
EDGE_EXPECTED = (FEW, FEW, FEW, REJECTED, REJECTED, OK, OK, OK, DEGENERATE, REJECTED)   # then the collinear pair and the pure outliers


def make_edge_scene(seed: int = 11) -> Scene:
    """pair k = frames (2 k, 2 k + 1).  Pairs 0 .. 7: EDGE_USABLE usable true matches of a rigid motion without noise, and three
    matches that are not usable (a NaN coordinate, Z <= 0, a zero tolerance) among them; pair 8: 50 matches whose points are
    collinear in frame a; pair 9: 100 matches between unrelated points."""
    rng = np.random.default_rng(seed)
    xyz, counts, pairs, mi, mj, kind, start, motion, clean = [], [], [], [], [], [], [0], [], []
    tols = []

    def cloud(n):
        Z = rng.uniform(300.0, 1500.0, n)
        return np.stack([Z * rng.uniform(-0.3, 0.3, n), Z * rng.uniform(-0.2, 0.2, n), Z], axis=1)

    cases = [(m, "rigid") for m in EDGE_USABLE] + [(50, "collinear"), (100, "outliers")]
    for k, (m, what) in enumerate(cases):
        R, t = _random_motion(rng, 5.0, 40.0)
        A = cloud(m + 3)
        if what == "collinear":
            A = np.array([0.0, 0.0, 400.0]) + np.linspace(0.0, 1.0, m + 3)[:, None] * np.array([100.0, 50.0, 300.0])
        B = A @ R.T + t
        if what == "outliers":
            B = cloud(m + 3)
        tla, tda = tolerances(A); tlb, tdb = tolerances(B)
        if what == "rigid":
            bad = np.sort(rng.choice(m + 3, 3, replace=False)) if m else np.arange(3)
            A[bad[0], 1] = np.nan
            B[bad[1], 2] = -B[bad[1], 2]
            tla[bad[2]] = 0.0
        else:
            A, B, tla, tda, tlb, tdb = A[:m], B[:m], tla[:m], tda[:m], tlb[:m], tdb[:m]
        n = len(A)
        perm = rng.permutation(n)   # feature j of frame b is the partner of feature perm[j] of frame a
        xyz += [A, B[perm]]; tols += [(tla, tda), (tlb[perm], tdb[perm])]
        counts += [n, n]
        inv = np.argsort(perm)
        pairs.append((2 * k, 2 * k + 1))
        mi += list(range(n)); mj += list(inv); kind += [1 if what == "outliers" else 0] * n
        start.append(len(mi)); motion.append((R, t)); clean.append(A.copy())
    offset = np.zeros(len(counts) + 1, np.uint32); offset[1:] = np.cumsum(counts)
    pts = Points(offset, np.ascontiguousarray(np.concatenate(xyz)), np.ascontiguousarray(np.concatenate([a for a, _ in tols])),
                 np.ascontiguousarray(np.concatenate([b for _, b in tols])))
    return Scene(pts, np.array(pairs, np.uint32), np.array(start, np.uint64), np.array(mi, np.uint32), np.array(mj, np.uint32), np.array(kind, np.uint8),
                 motion, clean, tuple(counts))


_CACHE = {}


def scene(name: str) -> Scene:
    """`rigid`, `moving`, `edge`: made once, shared by the tests, never modified"""
    if name not in _CACHE:
        _CACHE[name] = make_edge_scene() if name == "edge" else make_motion_scene(name == "moving")
    return _CACHE[name]


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------- conditions
KEPT_TRUE = 0.90      # at least this share of a pair's true matches stays
KEPT_PLANTED = 0.03   # planted (and second-body) matches among what stays: at most this share, the cap of DESIGN.md section 7w


def evaluate(sc: Scene, res) -> list:
    """per pair: the share of the true matches kept, the share of planted and second-body matches among the kept, and the
    largest distance, in units of the summed tolerances along and across the ray, by which the recovered motion moves a
    noise-free point of the pair away from where the true motion puts it"""
    out = []
    tl, tdp = sc.points.tol_lat, sc.points.tol_dep
    for p, (a, b) in enumerate(sc.pairs):
        s = slice(int(sc.pair_start[p]), int(sc.pair_start[p + 1]))
        kind, keep = sc.kind[s], np.asarray(res.keep[s], bool)
        true = kind == 0
        row = res.pair[p]
        R, t = np.asarray(row["R"]).reshape(3, 3), np.asarray(row["t"])
        Rt, tt = sc.motion[p]
        A = sc.clean[p][true]
        Btrue = A @ Rt.T + tt
        d = (A @ R.T + t) - Btrue
        r = _unit(Btrue)
        par = (d * r).sum(axis=1)
        perp = np.sqrt(np.maximum(0.0, (d * d).sum(axis=1) - par * par))
        gi = int(sc.points.offset[a]) + sc.mi[s][true].astype(np.int64); gj = int(sc.points.offset[b]) + sc.mj[s][true].astype(np.int64)
        out.append(dict(status=int(row["status"]), true=int(true.sum()), kept_true=float(keep[true].sum() / max(1, true.sum())),
                        kept=int(keep.sum()), planted=float(keep[~true].sum() / max(1, keep.sum())),
                        motion=float(max(np.max(np.abs(par) / (tdp[gi] + tdp[gj])), np.max(perp / (tl[gi] + tl[gj]))))))
    return out


def check_conditions(ev: list, what):
    for p, e in enumerate(ev):
        assert e["status"] == OK, (what, p, e)
        assert e["kept_true"] >= KEPT_TRUE, (what, p, e)
        assert e["planted"] <= KEPT_PLANTED, (what, p, e)
        assert e["motion"] <= 1.0, (what, p, e)


# ---------------------------------------------------------------------------------------------------------------- the image chain
# The warp of the direct and chain sequences of tests/features_reference.py scales frame k by 1 + 0.02 k, which at a constant
# depth is no rigid motion.  The chain test of the verification therefore uses frames of its own: the same texture, size, level
# and noise as the direct sequence, through the same rotation and shift but with scale 1.  At a fronto-parallel constant virtual
# depth and a camera without distortion the back-projection is a similarity of the pixel coordinates, so these frames are
# rigid motions of one plane.
RIGID_FRAMES = 4
RIGID_VDEPTH = 4.0


def rigid_warp(k: int, shape):
    """pixel (x, y) of frame k shows the texture at rigid_warp(k, shape)(x, y): a rotation of 1.5 k degrees about the image
    centre and a shift of (6.5 k, -3.7 k)"""
    h, w = shape
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    c, s = math.cos(math.radians(1.5 * k)), math.sin(math.radians(1.5 * k))

    def f(x, y):
        x = np.asarray(x, np.float64) - cx; y = np.asarray(y, np.float64) - cy
        return c * x - s * y + cx + 6.5 * k, s * x + c * y + cy - 3.7 * k
    return f


def rigid_frame(k: int) -> np.ndarray:
    from tests import features_reference as fref
    from tests import rawdepth_reference as ref

    def make():
        h, w = fref.DIRECT_SHAPE
        yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        v = fref.LEVEL * ref.texture()(*rigid_warp(k, (h, w))(xx, yy)) * 255.0
        v = v + np.random.default_rng(100 + k).normal(0.0, ref.NOISE * 255.0, v.shape)
        img = np.clip(np.floor(v + 0.5), 0.0, 255.0).astype(np.uint8)
        img.setflags(write=False)
        return img
    return cached(("rigid_frame", k), make)


def evaluate_tracks(feats, tracks, shape) -> dict:
    """the rule of features_reference.evaluate under rigid_warp: every observation mapped onto the texture; a track is wrong when
    an observation lies more than WRONG pixels from the track's mean.  Returns the counts and the wrong tracks' observations."""
    from tests import features_reference as fref
    x = np.concatenate([f.x for f in feats]); y = np.concatenate([f.y for f in feats])
    tx = np.zeros(len(tracks.fr)); ty = np.zeros(len(tracks.fr))
    for k in range(len(feats)):
        sel = tracks.fr == k
        tx[sel], ty[sel] = rigid_warp(k, shape)(x[tracks.feature[sel]], y[tracks.feature[sel]])
    wrong, wrong_obs, right_obs = 0, set(), set()
    for t in range(tracks.n_tracks):
        sel = tracks.pt == t
        dist = np.hypot(tx[sel] - tx[sel].mean(), ty[sel] - ty[sel].mean())
        if dist.max() > fref.WRONG:
            wrong += 1
            wrong_obs |= set(tracks.feature[sel][dist > fref.WRONG].tolist())
        else:
            right_obs |= set(tracks.feature[sel].tolist())
    return dict(tracks=int(tracks.n_tracks), wrong=wrong, conflicts=int(tracks.n_conflicts), wrong_obs=wrong_obs, right_obs=right_obs)


# Measured with this restatement and the Kabsch refit at the default options (tests/test_verify_cpu.py prints the figures): per
# scene the least share of true matches kept over its pairs, the largest share of planted matches among the kept, the largest
# motion error in units of the tolerances; `refit`: the largest deviation of lifcal_align_fit from the Kabsch fit on the scenes'
# inlier sets, |dR| (Frobenius) and |dt| / mm.
MEASURED = {
    "rigid": dict(kept_true=1.0, planted=0.0, motion=0.0458),
    "moving": dict(kept_true=1.0, planted=0.0, motion=0.0857),
    "refit": dict(dR=2.08e-15, dt=6.06e-13),
}
