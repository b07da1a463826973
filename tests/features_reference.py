"""numpy restatement of include/lifcal_features.h: detection, matching and the track linker, the scenes
and the truth their tests share, and the accuracy the restatement was measured to have.

The restatement follows the header with other means than the kernels: score and non-maximum suppression on the whole image at
once (no tiles), the buckets applied by one sort, the descriptor bits by fancy indexing into one box-sum image, matching as an
all-pairs distance matrix, the linker as a plain loop.  Everything summed is an integer and numpy's float64 steps are IEEE without
fused multiply-add: equal bytes are expected.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from lifcal_amd import raw_image, white_image
from tests import rawdepth_reference as ref

PATCH_R = 15
DETECT_DEFAULTS = dict(win_r=3, nms_r=4, cell=32, per_cell=4, min_score=1.0e-4)
MATCH_DEFAULTS = dict(max_dist=64, ratio_num=3, ratio_den=4, max_shift=0)
NO_BEST = 257


# ---------------------------------------------------------------------------------------------------------------- detection
def pattern() -> np.ndarray:
    """(256, 4) int8: ax, ay, bx, by"""
    s = 1
    out = []

    def draw():
        nonlocal s
        s = (1664525 * s + 1013904223) % (1 << 32)
        return ((s >> 16) % 27) - 13

    while len(out) < 256:
        v = [draw() for _ in range(4)]
        if (v[0], v[1]) != (v[2], v[3]):
            out.append(v)
    return np.array(out, np.int8)


@dataclass
class Feats:
    x: np.ndarray
    y: np.ndarray
    ix: np.ndarray
    iy: np.ndarray
    score: np.ndarray
    desc: np.ndarray

    @property
    def n(self):
        return len(self.x)


def _shift(a: np.ndarray, dy: int, dx: int, fill) -> np.ndarray:
    """out[y, x] = a[y + dy, x + dx], `fill` outside"""
    h, w = a.shape
    r = max(abs(dy), abs(dx))
    p = np.full((h + 2 * r, w + 2 * r), fill, a.dtype)
    p[r:r + h, r:r + w] = a
    return p[r + dy:r + dy + h, r + dx:r + dx + w]


def score_map(img: np.ndarray, win_r: int) -> np.ndarray:
    I = img.astype(np.int64)
    bits = 8 * img.dtype.itemsize
    full = float((1 << bits) - 1)
    s = lambda dy, dx: _shift(I, dy, dx, 0)
    gx = (s(-1, 1) + 2 * s(0, 1) + s(1, 1)) - (s(-1, -1) + 2 * s(0, -1) + s(1, -1))
    gy = (s(1, -1) + 2 * s(1, 0) + s(1, 1)) - (s(-1, -1) + 2 * s(-1, 0) + s(-1, 1))
    A, B, C = ref._box(gx * gx, win_r), ref._box(gx * gy, win_r), ref._box(gy * gy, win_r)
    dA, dB, dC = A.astype(np.float64), B.astype(np.float64), C.astype(np.float64)
    return ((dA * dC - dB * dB) / (dA + dC + 1.0)) / (full * full)


def _parabola(sm, s0, sp):
    den = (sm - 2.0 * s0) + sp
    with np.errstate(divide="ignore", invalid="ignore"):
        o = np.where(den < 0.0, (0.5 * (sm - sp)) / np.where(den < 0.0, den, -1.0), 0.0)
    return np.clip(o, -0.5, 0.5)


def describe(img: np.ndarray, ix, iy) -> np.ndarray:
    S = ref._box(img.astype(np.int64), 2)
    p = pattern().astype(np.int64)
    ix = np.asarray(ix, np.int64)[:, None]; iy = np.asarray(iy, np.int64)[:, None]
    bits = S[iy + p[None, :, 1], ix + p[None, :, 0]] < S[iy + p[None, :, 3], ix + p[None, :, 2]]
    words = (bits.reshape(-1, 8, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)[None, None, :]).sum(axis=2)
    return words.astype(np.uint32)


def detect(img: np.ndarray, status=None, **kw) -> Feats:
    o = dict(DETECT_DEFAULTS); o.update({k: v for k, v in kw.items() if v})
    H, W = img.shape
    lo = PATCH_R + 1
    empty = Feats(np.zeros(0), np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0), np.zeros((0, 8), np.uint32))
    if W < 2 * lo + 1 or H < 2 * lo + 1:
        return empty
    sc = score_map(img, o["win_r"])
    nr = o["nms_r"]
    is_max = np.ones((H, W), bool)
    for dy in range(-nr, nr + 1):
        for dx in range(-nr, nr + 1):
            if dy == 0 and dx == 0:
                continue
            q = _shift(sc, dy, dx, -np.inf)
            is_max &= (q < sc) | ((q == sc) & ((dy > 0) | ((dy == 0) & (dx > 0))))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    cand = is_max & (sc >= o["min_score"]) & (xx >= lo) & (xx <= W - 1 - lo) & (yy >= lo) & (yy <= H - 1 - lo)
    if status is not None:
        valid = ((status == 0) | (status == 3)).astype(np.int64)
        cand &= ref._box(valid, PATCH_R) == (2 * PATCH_R + 1) ** 2
    ys, xs = np.nonzero(cand)
    if not ys.size:
        return empty
    s0 = sc[ys, xs]
    nbx = (W + o["cell"] - 1) // o["cell"]
    bucket = (ys // o["cell"]) * nbx + xs // o["cell"]
    order = np.lexsort((xs, ys, -s0, bucket))
    ys, xs, s0, bucket = ys[order], xs[order], s0[order], bucket[order]
    first = np.r_[True, bucket[1:] != bucket[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(len(bucket)), 0))
    keep = (np.arange(len(bucket)) - start) < o["per_cell"]
    ys, xs, s0 = ys[keep], xs[keep], s0[keep]
    ox = _parabola(sc[ys, xs - 1], s0, sc[ys, xs + 1]); oy = _parabola(sc[ys - 1, xs], s0, sc[ys + 1, xs])
    return Feats(xs.astype(np.float64) + ox, ys.astype(np.float64) + oy, xs.astype(np.int32), ys.astype(np.int32), s0, describe(img, xs, ys))


# ---------------------------------------------------------------------------------------------------------------- matching
@dataclass
class Match:
    pairs: np.ndarray
    pair_start: np.ndarray
    i: np.ndarray
    j: np.ndarray
    dist: np.ndarray


def _bits(desc: np.ndarray) -> np.ndarray:
    return np.unpackbits(np.ascontiguousarray(desc, np.uint32).view(np.uint8).reshape(len(desc), 32), axis=1).astype(np.int64)


def _best(D: np.ndarray):
    """per row: best, lowest arg (or -1), second"""
    n, m = D.shape
    if m == 0:
        return np.full(n, NO_BEST), np.full(n, -1), np.full(n, NO_BEST)
    arg = np.argmin(D, axis=1)
    best = D[np.arange(n), arg]
    E = D.copy(); E[np.arange(n), arg] = 999
    second = np.minimum(E.min(axis=1), NO_BEST)
    none = best >= 999
    return np.where(none, NO_BEST, best), np.where(none, -1, arg), second


def match(feats, pairs, **kw) -> Match:
    o = dict(MATCH_DEFAULTS); o.update({k: v for k, v in kw.items() if v})
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    start, I, J, Dd = [0], [], [], []
    for a, b in pairs.tolist():
        fa, fb = feats[a], feats[b]
        ba, bb = _bits(fa.desc), _bits(fb.desc)
        D = ba @ (1 - bb).T + (1 - ba) @ bb.T                     # all pairs
        if o["max_shift"] > 0:
            far = (np.abs(fa.ix.astype(np.int64)[:, None] - fb.ix.astype(np.int64)[None, :]) > o["max_shift"]) | \
                  (np.abs(fa.iy.astype(np.int64)[:, None] - fb.iy.astype(np.int64)[None, :]) > o["max_shift"])
            D = np.where(far, 999, D)
        best_a, arg_a, sec_a = _best(D)
        best_b, arg_b, sec_b = _best(D.T)
        for i in range(fa.n):
            j = int(arg_a[i])
            if j < 0 or int(arg_b[j]) != i:
                continue
            d = int(best_a[i])
            if d <= o["max_dist"] and o["ratio_den"] * d < o["ratio_num"] * int(sec_a[i]) and o["ratio_den"] * d < o["ratio_num"] * int(sec_b[j]):
                I.append(i); J.append(j); Dd.append(d)
        start.append(len(I))
    return Match(pairs, np.array(start, np.uint64), np.array(I, np.uint32), np.array(J, np.uint32), np.array(Dd, np.uint32))


# ---------------------------------------------------------------------------------------------------------------- linker
@dataclass
class Linked:
    fr: np.ndarray
    pt: np.ndarray
    feature: np.ndarray
    n_tracks: int
    n_conflicts: int


def link(counts, pairs, pair_start, mi, mj, min_length: int = 2) -> Linked:
    """counts: features per frame"""
    offset = np.r_[0, np.cumsum(counts)].astype(np.int64)
    N = int(offset[-1])
    frame_of = np.repeat(np.arange(len(counts)), counts)
    comp = list(range(N))                 # component label per feature; merging relabels the whole component (a plain loop)
    members = {g: [g] for g in range(N)}
    for p, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        for k in range(int(pair_start[p]), int(pair_start[p + 1])):
            u, v = comp[int(offset[a]) + int(mi[k])], comp[int(offset[b]) + int(mj[k])]
            if u == v:
                continue
            u, v = min(u, v), max(u, v)
            for g in members.pop(v):
                comp[g] = u
                members[u].append(g)
    fr, pt, ft = [], [], []
    n_tracks = n_conflicts = 0
    label = {}
    for u in sorted(members, key=lambda u: min(members[u])):
        ms = members[u]
        if len(ms) < 2:
            continue
        frames = [int(frame_of[g]) for g in ms]
        if len(set(frames)) < len(frames):
            n_conflicts += 1
            continue
        if len(ms) < min_length:
            continue
        label[u] = n_tracks
        n_tracks += 1
    for g in range(N):
        if comp[g] in label:
            fr.append(int(frame_of[g])); pt.append(label[comp[g]]); ft.append(g)
    return Linked(np.array(fr, np.uint32), np.array(pt, np.uint32), np.array(ft, np.uint32), n_tracks, n_conflicts)


def sequence_pairs(n_frames: int, window: int = 2) -> np.ndarray:
    return np.array([(a, b) for a in range(n_frames) for b in range(a + 1, min(n_frames, a + 1 + window))], np.uint32).reshape(-1, 2)


# ---------------------------------------------------------------------------------------------------------------- scenes and truth
LEVEL = 0.9
DIRECT_SHAPE = (160, 200)          # height, width
DIRECT_FRAMES = 5
CHAIN_CASES = ("d14", "d23_16")
CHAIN_FRAMES = 3


def warp(k: int, shape):
    """frame k shows the texture through a rotation of 1.5 k degrees and a scale of 1 + 0.02 k about the image centre and a
    shift of (6.5 k, -3.7 k): pixel (x, y) of frame k shows the texture at warp(k, shape)(x, y)"""
    h, w = shape
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    ang, sc = math.radians(1.5 * k), 1.0 + 0.02 * k
    c, s = sc * math.cos(ang), sc * math.sin(ang)

    def f(x, y):
        x = np.asarray(x, np.float64) - cx; y = np.asarray(y, np.float64) - cy
        return c * x - s * y + cx + 6.5 * k, s * x + c * y + cy - 3.7 * k
    return f


def warped_texture(k: int, shape):
    T, f = ref.texture(), warp(k, shape)
    return lambda x, y: T(*f(x, y))


@functools.lru_cache(maxsize=None)
def sampled_frame(k: int, shape, noise: float = ref.NOISE) -> np.ndarray:
    """the warped texture of frame k sampled at the pixel centres of an image of `shape` = (height, width), 8 bit"""
    h, w = shape
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    v = LEVEL * warped_texture(k, shape)(xx, yy) * 255.0
    if noise:
        v = v + np.random.default_rng(100 + k).normal(0.0, noise * 255.0, v.shape)
    img = np.clip(np.floor(v + 0.5), 0.0, 255.0).astype(np.uint8)
    img.setflags(write=False)
    return img


def direct_frame(k: int, noise: float = ref.NOISE) -> np.ndarray:
    """frame k of the direct sequence"""
    return sampled_frame(k, DIRECT_SHAPE, noise)


def tie_lattice(h: int, w: int) -> np.ndarray:
    """vertical stripes of period 6 everywhere (score 0: no gradient in y); inside a frame of 24 pixels every fourth row is at half
    brightness.  There the scores repeat exactly every 6 columns and 4 rows, and towards the frame they fall, so the
    neighbourhood of a maximum holds exact ties and the first in (y, x) order wins"""
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    img = np.where(xx % 6 < 3, 200, 40)
    img[24:h - 24, 24:w - 24] = (img // np.where(yy % 4 == 0, 2, 1))[24:h - 24, 24:w - 24]
    return img.astype(np.uint8)


def chain_shape(name: str):
    w, h = ref.CASES[name][:2]
    return h, w


@functools.lru_cache(maxsize=None)
def chain_raw(name: str, k: int) -> np.ndarray:
    """the raw image of frame k of a case's chain sequence: the warped texture at the mid scene's depth, with noise"""
    w, h, d, rot, off, bits, _, _ = ref.CASES[name]
    tx, ty = white_image.grid_centres(w, h, d, ref.BASE_Y, rot, off, 1.5)
    img = raw_image.render_raw_image(w, h, tx, ty, d, ref.scene_depth(name, "mid"), warped_texture(k, (h, w)), bits=bits, noise=ref.NOISE, seed=11 + k)
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------------------------------------------------------- conditions
WRONG = 1.5


def evaluate(feats, linked, shape) -> dict:
    """the issue's conditions on a sequence: every observation mapped through its frame's warp onto the texture; a track is
    wrong when an observation lies more than WRONG pixels from the track's mean; rms: the distance of the observations of the
    right tracks from their track's mean"""
    x = np.concatenate([f.x for f in feats]); y = np.concatenate([f.y for f in feats])
    n_frames = len(feats)
    m = min(f.n for f in feats)
    tx = np.zeros(len(linked.fr)); ty = np.zeros(len(linked.fr))
    for k in range(n_frames):
        sel = linked.fr == k
        tx[sel], ty[sel] = warp(k, shape)(x[linked.feature[sel]], y[linked.feature[sel]])
    wrong = full = 0
    d2 = []
    for t in range(linked.n_tracks):
        sel = linked.pt == t
        dist = np.hypot(tx[sel] - tx[sel].mean(), ty[sel] - ty[sel].mean())
        full += int(sel.sum() == n_frames)
        if dist.max() > WRONG:
            wrong += 1
        else:
            d2.append(dist ** 2)
    rms = float(np.sqrt(np.mean(np.concatenate(d2)))) if d2 else 0.0
    return dict(tracks=int(linked.n_tracks), m=int(m), full=full, wrong=wrong, conflicts=int(linked.n_conflicts), rms=rms)


def check_conditions(e: dict, what):
    assert e["tracks"] >= e["m"], (what, e)
    assert e["full"] >= 0.4 * e["m"], (what, e)
    assert e["wrong"] <= 0.03 * e["tracks"], (what, e)
    assert e["conflicts"] <= 0.03 * e["tracks"], (what, e)


def describe_eval(e: dict) -> str:
    return (f"{e['tracks']} tracks, m {e['m']}, {e['full']} in all frames, {e['wrong']} wrong, {e['conflicts']} conflicts, rms {e['rms']:.4f}")


# Measured with this restatement (tests/test_features_cpu.py prints the figures): the RMS distance, in pixels of the texture, of
# the observations of the right tracks from their track's mean.  The bars of the GPU tests are twice that: the margin covers other
# seeds, not other arithmetic (the kernels' bytes are the restatement's).
MEASURED = {
    "direct": dict(rms=0.2956),      # with noise; 0.2220 without
    "d14": dict(rms=0.3395),
    "d23_16": dict(rms=0.4122),
}
BARS = {name: dict(rms=2 * m["rms"]) for name, m in MEASURED.items()}

_CACHE = {}


def cached(key, make):
    """computed once, shared by the tests, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def run_sequence(key, images, statuses=None):
    """(features per frame, matches, linked tracks) of the restatement on a sequence, cached under key"""
    def make():
        feats = [detect(im, None if statuses is None else statuses[k]) for k, im in enumerate(images)]
        m = match(feats, sequence_pairs(len(feats)))
        return feats, m, link([f.n for f in feats], m.pairs, m.pair_start, m.i, m.j)
    return cached(("sequence", key), make)


def chain_totalfocus(name: str, gd):
    """the chain frames of a case as (image, status) pairs of the total-focus restatement with the true depth at scale 1"""
    from tests import totalfocus_reference as tref

    def make():
        out = []
        for k in range(CHAIN_FRAMES):
            tf = tref.render(chain_raw(name, k), tref.true_depth(name, "mid", 1), gd.cx, gd.cy, ref.CASES[name][2])
            out.append((tf.image, tf.status))
        return out
    return cached(("chain", name), make)
