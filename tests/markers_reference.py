"""numpy restatement of include/lifcal_markers.h, written from the header and not from the device code:
steps 1 to 7 of the detector, the dictionary's distance and generator, and the three host functions (constraints reader, start
values of the marker points, scale factor).  Integers are Python / int64 integers, doubles are Python floats (IEEE, no fused
multiply-add) evaluated in the order the header writes.  The labelling is done by repeated minimum propagation.

The file also holds the test scenes and MEASURED / BARS in the manner of features_reference.py.
"""
from __future__ import annotations

import math

import numpy as np

from lifcal_amd import marker_image as mi

MARKER_DTYPE = np.dtype([("id", np.int32), ("rotation", np.int32), ("hamming", np.int32), ("refined", np.int32), ("label", np.int32), ("area", np.int32),
                         ("corners", np.float64, (4, 2)), ("x", np.float64), ("y", np.float64)], align=True)
COMPONENT_DTYPE = np.dtype([("label", np.int32), ("area", np.int32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32),
                            ("ext", np.int32, (8, 2))], align=True)

# ------------------------------------------------------------------------------------------------ dictionary


def rot_word(w: int, m: int) -> int:
    out = 0
    for r in range(m):
        for c in range(m):
            if (w >> ((m - 1 - c) * m + r)) & 1:
                out |= 1 << (r * m + c)
    return out


def rotations(w: int, m: int):
    out = [int(w)]
    for _ in range(3):
        out.append(rot_word(out[-1], m))
    return out


def _pop(v: int) -> int:
    return bin(v).count("1")


def word_distance(a: int, b: int, m: int, k0: int) -> int:
    return min(_pop(a ^ r) for r in rotations(b, m)[k0:])


def dictionary_distance(words, m: int) -> int:
    words = [int(w) for w in words]
    best = 65
    for i, a in enumerate(words):
        best = min(best, word_distance(a, a, m, 1))
        for b in words[i + 1:]:
            best = min(best, word_distance(a, b, m, 0))
    return best


def generate(m: int, n: int, seed: int):
    """(words, min_distance) of lifcal_marker_dictionary_generate"""
    nb, s, tau, refused = m * m, seed & 0xffffffff, (m * m) // 2, 0
    draws = (nb + 15) // 16
    out, out_rot = [], []
    while len(out) < n:
        word = 0
        for i in range(draws):
            s = (1664525 * s + 1013904223) & 0xffffffff
            word |= ((s >> 16) & 0xffff) << (16 * i)
        word &= (1 << nb) - 1
        ok = word_distance(word, word, m, 1) >= tau
        if ok:
            for rs in out_rot:
                if min(_pop(word ^ r) for r in rs) < tau:
                    ok = False
                    break
        if ok:
            out.append(word); out_rot.append(rotations(word, m)); refused = 0
            continue
        refused += 1
        if refused == 2000:
            if tau == 1:
                raise ValueError("the space of words is exhausted")
            tau -= 1; refused = 0
    return np.array(out, np.uint64), dictionary_distance(out, m)


def word_bits(w: int, m: int) -> np.ndarray:
    return np.array([[(int(w) >> (r * m + c)) & 1 for c in range(m)] for r in range(m)], np.uint8)

# ------------------------------------------------------------------------------------------------ options


def resolve(shape, bits: int, words=None, m: int = 0, **kw) -> dict:
    """the options with the defaults of lifcal_markers_check filled in (the refusals are the library's business)"""
    h, w = shape
    o = dict(w=0, contrast=0, cell_contrast=0, min_area=0, min_side=0, max_side=0, max_border_errors=0, max_correction=0, refine_max=0.0)
    o.update(kw)
    o["w"] = o["w"] or 7
    o["contrast"] = o["contrast"] or 12
    o["cell_contrast"] = o["cell_contrast"] or min(2 * o["contrast"], 255)
    o["min_area"] = o["min_area"] or 32
    o["min_side"] = o["min_side"] or 12
    o["max_side"] = o["max_side"] or max(min(h, w), o["min_side"])
    o["refine_max"] = o["refine_max"] or 3.0
    if words is not None:
        bound = (dictionary_distance(words, m) - 1) // 2
        o["max_correction"] = bound if o["max_correction"] == 0 else (0 if o["max_correction"] == -1 else o["max_correction"])
    else:
        o["max_correction"] = 0
    unit = 1 if bits == 8 else 256
    o["C"] = o["contrast"] * unit
    o["C_cell"] = o["cell_contrast"] * unit
    return o

# ------------------------------------------------------------------------------------------------ steps 1 to 3


def dark_map(img: np.ndarray, status, w: int, C: int) -> np.ndarray:
    I = img.astype(np.int64)
    H, W = I.shape
    S = np.zeros((H + 1, W + 1), np.int64)
    S[1:, 1:] = I.cumsum(0).cumsum(1)
    y0 = np.maximum(np.arange(H) - w, 0); y1 = np.minimum(np.arange(H) + w, H - 1) + 1
    x0 = np.maximum(np.arange(W) - w, 0); x1 = np.minimum(np.arange(W) + w, W - 1) + 1
    total = S[y1][:, x1] - S[y0][:, x1] - S[y1][:, x0] + S[y0][:, x0]
    n = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    valid = np.ones((H, W), bool) if status is None else ((status == 0) | (status == 3))
    return (valid & (n * I + n * C < total)).astype(np.uint8)


def label_map(dark: np.ndarray) -> np.ndarray:
    """repeated minimum propagation over the 8-neighbourhood until nothing changes"""
    H, W = dark.shape
    BIG = np.int64(1) << 40
    d = dark.astype(bool)
    lab = np.where(d, np.arange(H * W, dtype=np.int64).reshape(H, W), BIG)
    while True:
        p = np.pad(lab, 1, constant_values=BIG)
        m = lab
        for dy in range(3):
            for dx in range(3):
                m = np.minimum(m, p[dy:dy + H, dx:dx + W])
        m = np.where(d, m, BIG)
        if np.array_equal(m, lab):
            break
        lab = m
    return np.where(d, lab, -1).astype(np.int32)


def component_table(labels: np.ndarray, o: dict) -> np.ndarray:
    """the candidates of step 3 as COMPONENT_DTYPE records, by ascending label"""
    H, W = labels.shape
    flat = labels.reshape(-1).astype(np.int64)
    idx = np.flatnonzero(flat >= 0)
    area = np.bincount(flat[idx], minlength=H * W) if len(idx) else np.zeros(H * W, np.int64)
    out = []
    for lab in np.flatnonzero(area >= o["min_area"]):
        px = idx[flat[idx] == lab]   # ascending linear index
        x, y = px % W, px // W
        ext = []
        for proj in (x, y, x + y, x - y):
            for k in (int(np.argmin(proj)), int(np.argmax(proj))):   # the first of equals: the lowest linear index
                ext.append((int(x[k]), int(y[k])))
        x0, x1, y0, y1 = ext[0][0], ext[1][0], ext[2][1], ext[3][1]
        sx, sy = x1 - x0 + 1, y1 - y0 + 1
        if (sx >= o["min_side"] and sy >= o["min_side"] and sx <= o["max_side"] and sy <= o["max_side"] and x0 >= 1 and y0 >= 1 and x1 <= W - 2
                and y1 <= H - 2):
            out.append((int(lab), int(area[lab]), x0, y0, x1, y1, ext))
    rec = np.zeros(len(out), COMPONENT_DTYPE)
    for k, v in enumerate(out):
        rec[k] = v
    return rec


def components(img: np.ndarray, status=None, **kw):
    """(dark, labels, candidate table) as lifcal_markers_components returns them"""
    o = resolve(img.shape, 8 * img.dtype.itemsize, **kw)
    dark = dark_map(img, status, o["w"], o["C"])
    labels = label_map(dark)
    return dark, labels, component_table(labels, o)

# ------------------------------------------------------------------------------------------------ steps 4 to 7


def _sign(v: int) -> int:
    return (v > 0) - (v < 0)


def quad(ext, min_side: int):
    """q_0 .. q_3 of step 4 as a list of (x, y), or None"""
    sets = ([ext[4], ext[7], ext[5], ext[6]], [ext[2], ext[1], ext[3], ext[0]])
    a2 = [sum(int(s[i][0]) * int(s[(i + 1) % 4][1]) - int(s[(i + 1) % 4][0]) * int(s[i][1]) for i in range(4)) for s in sets]
    pick = sets[1] if a2[1] > a2[0] else sets[0]
    if max(a2[0], a2[1]) < min_side * min_side:
        return None
    sx = sum(int(p[0]) for p in pick); sy = sum(int(p[1]) for p in pick)
    return [(float(int(p[0])) + 0.5 * float(_sign(4 * int(p[0]) - sx)), float(int(p[1])) + 0.5 * float(_sign(4 * int(p[1]) - sy))) for p in pick]


def sample(I, X: float, Y: float):
    """the value of a sample (an int), or None where the header rejects / skips"""
    if not (abs(X) < 1048576.0) or not (abs(Y) < 1048576.0):
        return None
    H, W = len(I), len(I[0])
    Sx = math.floor(64.0 * X + 0.5); Sy = math.floor(64.0 * Y + 0.5)
    ix, iy, fx, fy = Sx >> 6, Sy >> 6, Sx & 63, Sy & 63
    if ix < 0 or ix + 1 > W - 1 or iy < 0 or iy + 1 > H - 1:
        return None
    return ((64 - fx) * (64 - fy) * I[iy][ix] + fx * (64 - fy) * I[iy][ix + 1] + (64 - fx) * fy * I[iy + 1][ix] + fx * fy * I[iy + 1][ix + 1])


def _meet(M, T, M2, T2):
    det = T[0] * T2[1] - T[1] * T2[0]
    if det == 0.0:
        return None
    q = ((M2[0] - M[0]) * T2[1] - (M2[1] - M[1]) * T2[0]) / det
    return (M[0] + q * T[0], M[1] + q * T[1])


def read_word(I, q, m: int, o: dict):
    """step 5 up to the word: (word, lo, hi) or None"""
    n = m + 2
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = q
    dx1 = x1 - x2; dx2 = x3 - x2; sx = ((x0 - x1) + x2) - x3
    dy1 = y1 - y2; dy2 = y3 - y2; sy = ((y0 - y1) + y2) - y3
    den = dx1 * dy2 - dy1 * dx2
    if den == 0.0:
        return None
    g = (sx * dy2 - sy * dx2) / den; h = (dx1 * sy - dy1 * sx) / den
    a = (x1 - x0) + g * x1; b = (x3 - x0) + h * x3; c = x0
    d = (y1 - y0) + g * y1; e = (y3 - y0) + h * y3; f = y0
    V = [[0] * n for _ in range(n)]
    for r in range(n):
        for cc in range(n):
            tot = 0
            for bv in range(3):
                for bu in range(3):
                    u = ((float(cc) + 0.25) + (0.5 * (float(bu) + 0.5)) / 3.0) / float(n)
                    v = ((float(r) + 0.25) + (0.5 * (float(bv) + 0.5)) / 3.0) / float(n)
                    w = (g * u + h * v) + 1.0
                    if not (w > 0.0):
                        return None
                    val = sample(I, ((a * u + b * v) + c) / w, ((d * u + e * v) + f) / w)
                    if val is None:
                        return None
                    tot += val
            V[r][cc] = tot
    lo = min(min(row) for row in V); hi = max(max(row) for row in V)
    if hi - lo < 9 * 4096 * o["C_cell"]:
        return None
    border, word = 0, 0
    for r in range(n):
        for cc in range(n):
            white = 2 * V[r][cc] > lo + hi
            if r in (0, n - 1) or cc in (0, n - 1):
                border += 1 if white else 0
            elif white:
                word |= 1 << ((r - 1) * m + (cc - 1))
    if border > o["max_border_errors"]:
        return None
    return word, lo, hi


def match_word(word: int, rot_table, max_correction: int):
    """(id, rotation, hamming) or None; rot_table[j] = the four rotations of word j"""
    best = None
    for j, rs in enumerate(rot_table):
        for k, r in enumerate(rs):
            key = (_pop(word ^ r), j, k)
            if best is None or key < best:
                best = key
    if best[0] > max_correction:
        return None
    return best[1], best[2], best[0]


def refine(I, p, T: int, refine_max: float):
    """step 6: the refined corners or None"""
    lines = []
    for e in range(4):
        (Ax, Ay), (Bx, By) = p[e], p[(e + 1) % 4]
        dx = Bx - Ax; dy = By - Ay
        L = math.sqrt(dx * dx + dy * dy)
        if L == 0.0:
            return None
        nx = dy / L; ny = (-dx) / L
        pts = []
        for k in range(12):
            s = 0.15 + (0.7 * (float(k) + 0.5)) / 12.0
            Px = Ax + s * dx; Py = Ay + s * dy
            best, prev = None, None
            for i in range(17):
                oi = -4.0 + 0.5 * float(i)
                v = sample(I, Px + oi * nx, Py + oi * ny)
                if v is not None and prev is not None and 18 * prev < T <= 18 * v:
                    oc = (-4.0 + 0.5 * float(i - 1)) + 0.5 * (float(T - 18 * prev) / float(18 * v - 18 * prev))
                    if best is None or abs(oc) < abs(best):
                        best = oc
                prev = v
            if best is not None:
                pts.append((Px + best * nx, Py + best * ny))
        N = len(pts)
        if N < 4:
            return None
        sumx = 0.0; sumy = 0.0
        for x, y in pts:
            sumx += x; sumy += y
        mx = sumx / float(N); my = sumy / float(N)
        sxx = 0.0; sxy = 0.0; syy = 0.0
        for x, y in pts:
            ddx = x - mx; ddy = y - my
            sxx += ddx * ddx; sxy += ddx * ddy; syy += ddy * ddy
        lam = ((sxx + syy) + math.sqrt((sxx - syy) * (sxx - syy) + 4.0 * (sxy * sxy))) / 2.0
        lines.append(((mx, my), (lam - syy, sxy) if sxx >= syy else (sxy, lam - sxx)))
    out = []
    for e in range(4):
        b = (e + 3) % 4
        c = _meet(lines[b][0], lines[b][1], lines[e][0], lines[e][1])
        if c is None or not (abs(c[0]) < 1.0e300) or not (abs(c[1]) < 1.0e300):
            return None
        ddx = c[0] - p[e][0]; ddy = c[1] - p[e][1]
        if ddx * ddx + ddy * ddy > refine_max * refine_max:
            return None
        out.append(c)
    return out


def decode(I, comp, rot_table, m: int, o: dict):
    """steps 4 to 7 on one candidate: a MARKER_DTYPE tuple or None"""
    q = quad([tuple(int(v) for v in e) for e in comp["ext"]], o["min_side"])
    if q is None:
        return None
    got = read_word(I, q, m, o)
    if got is None:
        return None
    word, lo, hi = got
    hit = match_word(word, rot_table, o["max_correction"])
    if hit is None:
        return None
    j, k, ham = hit
    p = [q[(i + k) % 4] for i in range(4)]
    better = refine(I, p, lo + hi, o["refine_max"])
    refined = 0 if better is None else 1
    if better is not None:
        p = better
    ctr = _meet(p[0], (p[2][0] - p[0][0], p[2][1] - p[0][1]), p[1], (p[3][0] - p[1][0], p[3][1] - p[1][1]))
    if ctr is None:
        return None
    return (j, k, ham, refined, int(comp["label"]), int(comp["area"]), [list(c) for c in p], ctr[0], ctr[1])


def detect(img: np.ndarray, words, m: int, status=None, **kw):
    """(markers as MARKER_DTYPE records by ascending label, n_candidates) as lifcal_markers_detect returns them"""
    o = resolve(img.shape, 8 * img.dtype.itemsize, words, m, **kw)
    labels = label_map(dark_map(img, status, o["w"], o["C"]))
    cands = component_table(labels, o)
    I = img.astype(np.int64).tolist()
    rot_table = [rotations(int(w), m) for w in words]
    found = [d for d in (decode(I, c, rot_table, m, o) for c in cands) if d is not None]
    rec = np.zeros(len(found), MARKER_DTYPE)
    for k, v in enumerate(found):
        rec[k] = v
    return rec, len(cands)

# ------------------------------------------------------------------------------------------------ host functions


def read_constraints(path):
    """(id1, id2, distance, sigma, ids) of lifcal_constraints_read"""
    a, b, dist, sig, ids = [], [], [], [], []
    with open(path) as fh:
        for line in fh.read().split("\n"):
            line = line.rstrip("\r")
            if not line or line[0] == "#":
                continue
            t = line.split()
            if len(t) != 4:
                raise ValueError(line)
            i, j, d, s = int(t[0]), int(t[1]), float(t[2]), float(t[3])
            a.append(i); b.append(j); dist.append(d); sig.append(s)
            for v in (i, j):
                if v not in ids:
                    ids.append(v)
    return np.array(a, np.uint32), np.array(b, np.uint32), np.array(dist, np.float64), np.array(sig, np.float64), np.array(ids, np.uint32)


def seed_points(mx, my, mfr, mid, tx, ty, tfr, tpt, pts):
    """(ids, xyz, seeded) of lifcal_markers_seed_points"""
    ids, first = [], []
    for k in range(len(mid)):
        if int(mid[k]) not in ids:
            ids.append(int(mid[k])); first.append(k)
        elif mfr[k] < mfr[first[ids.index(int(mid[k]))]]:
            first[ids.index(int(mid[k]))] = k
    xyz = np.zeros((len(ids), 3)); seeded = np.zeros(len(ids), bool)
    for i, k in enumerate(first):
        best, arg = None, None
        for t in range(len(tx)):
            if tfr[t] != mfr[k]:
                continue
            dx = float(tx[t]) - float(mx[k]); dy = float(ty[t]) - float(my[k])
            d2 = dx * dx + dy * dy
            if best is None or d2 < best:
                best, arg = d2, t
        if arg is not None:
            seeded[i] = True
            xyz[i] = pts[int(tpt[arg])]
    return np.array(ids, np.uint32), xyz, seeded


def scale_factor(p1, p2, distance: float) -> float:
    dx = float(p1[0]) - float(p2[0]); dy = float(p1[1]) - float(p2[1]); dz = float(p1[2]) - float(p2[2])
    return distance / math.sqrt(dx * dx + dy * dy + dz * dz)

# ------------------------------------------------------------------------------------------------ scenes

_CACHE = {}


def cached(key, make):
    """computed once, shared by the tests, never modified"""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def dictionary(m: int = 4, n: int = 50, seed: int = 1):
    """(words, min_distance) of the generator, cached"""
    return cached(("dict", m, n, seed), lambda: generate(m, n, seed))


SHAPE = (192, 256)               # height, width of the rendered set
SIDES = (20, 28, 40, 64)
PERSPECTIVES = (0.0, 0.15)
N_ROTATIONS = 12                 # every 7.5 degrees; a quarter turn more with every step, so that all four decoded rotations occur
BLUR, NOISE, SHADING = 0.8, 2.0, 0.3


def rendered_poses():
    """the 24 poses of the rendered set: 12 rotations x 2 perspectives, the four sides in turn (six poses each), as
    (id, side, angle, perspective, tilt)"""
    out = []
    for p, persp in enumerate(PERSPECTIVES):
        for i in range(N_ROTATIONS):
            k = p * N_ROTATIONS + i
            out.append((k, SIDES[(i + p) % 4], 7.5 * i + 90.0 * (i % 4), persp, 30.0 * i))
    return out


def rendered_layout():
    """shelf packing of the poses into images of SHAPE, largest first: a list (one entry per image) of lists of PlacedMarker"""
    words, _ = dictionary()
    H, W = SHAPE
    poses = sorted(rendered_poses(), key=lambda t: (-t[1], t[0]))
    images, cur, x, y, shelf = [], [], 4, 4, 0
    for k, side, angle, persp, tilt in poses:
        pitch = int(math.ceil(1.4143 * side * (1.0 + persp))) + 10
        if x + pitch > W - 4:
            x, y, shelf = 4, y + shelf, 0
        if y + pitch > H - 4:
            images.append(cur)
            cur, x, y, shelf = [], 4, 4, 0
        cur.append(mi.place(k, word_bits(words[k], 4), x + 0.5 * pitch + 0.31, y + 0.5 * pitch - 0.17, side, angle, persp, tilt))
        x += pitch
        shelf = max(shelf, pitch)
    images.append(cur)
    return images


def rendered_set():
    """[(image, placed markers)] of the rendered set, cached: blur, noise, shading and a fixed seed"""
    def make():
        return [(mi.render_markers(SHAPE, placed, blur=BLUR, noise=NOISE, shading=SHADING, seed=100 + k), placed)
                for k, placed in enumerate(rendered_layout())]
    return cached("rendered", make)


def evaluate(per_image) -> dict:
    """per_image: [(markers record array, placed markers)].  found: markers of the truth reported with their id and the centre
    within 2 pixels; extra: reported markers that are none of those; rms, max: centre error of the found ones in pixels"""
    found, extra, total, refined, err = 0, 0, 0, 0, []
    for rec, placed in per_image:
        total += len(placed)
        truth = {p.id: p.centre for p in placed}
        seen = set()
        for r in rec:
            t = truth.get(int(r["id"]))
            e = None if t is None else math.hypot(float(r["x"]) - t[0], float(r["y"]) - t[1])
            if e is None or e > 2.0 or int(r["id"]) in seen:
                extra += 1
                continue
            seen.add(int(r["id"])); found += 1; refined += int(r["refined"]); err.append(e)
    err = np.array(err) if err else np.zeros(1)
    return dict(total=total, found=found, extra=extra, refined=refined, rms=float(np.sqrt(np.mean(err ** 2))), max=float(err.max()))


def check_conditions(e: dict, what=""):
    assert e["found"] == e["total"], (what, e)        # the cap on missed markers is zero
    assert e["extra"] == 0, (what, e)
    assert e["refined"] >= 0.9 * e["total"], (what, e)
    assert e["rms"] <= BARS["rendered"]["rms"] and e["max"] <= BARS["rendered"]["max"], (what, e, BARS)


def hand_marker(word: int, m: int, cell: int = 6, margin: int = 12, angle_quarter: int = 0, white: int = 230, black: int = 20, shape=None, at=(0, 0),
                dtype=np.uint8) -> np.ndarray:
    """an axis-aligned marker of cell x cell pixel cells drawn exactly, rotated by angle_quarter quarter turns clockwise"""
    n = m + 2
    cells = np.zeros((n, n), np.int64)
    cells[1:-1, 1:-1] = word_bits(word, m)
    cells = np.rot90(cells, -angle_quarter)
    tile = np.kron(cells, np.ones((cell, cell), np.int64))
    side = n * cell
    h, w = shape or (side + 2 * margin, side + 2 * margin)
    img = np.full((h, w), white, np.int64)
    y, x = margin + at[1], margin + at[0]
    img[y:y + side, x:x + side] = np.where(tile > 0, white, black)
    return img.astype(dtype)


def serpentine(shape=(96, 96), gap: int = 2) -> np.ndarray:
    """an image whose dark pixels are one one-pixel path: it runs along every other row, joined alternately at the right and
    the left end, from the bottom row upwards, so that it crosses every vertical tile seam in every row it runs along and every
    horizontal seam, and reaches the pixel with the lowest index, in the top row, last"""
    h, w = shape
    img = np.full(shape, 255, np.uint8)
    rows = list(range(1, h - 1, gap))
    for k, y in enumerate(rows):
        img[y, 1:w - 1] = 0
        if k + 1 < len(rows):
            xj = w - 2 if k % 2 == 0 else 1
            img[y:rows[k + 1] + 1, xj] = 0
    return img


# ------------------------------------------------------------------------------------------------ the raw-image chain
CHAIN_CASE = "d14"               # one of features_reference.CHAIN_CASES
CHAIN_FRAMES = 3
CHAIN_BITS = 3                   # 5 x 5 cells of 11 to 13 pixels: the total-focus image resolves about 2.5 v = 10 pixels at v = 4


def chain_dictionary():
    return dictionary(CHAIN_BITS, 6, 2)


def chain_markers():
    """two markers on a white ground in the virtual image of the case"""
    words, _ = chain_dictionary()
    return [mi.place(1, word_bits(words[1], CHAIN_BITS), 52.3, 80.4, 56, 8.0), mi.place(4, word_bits(words[4], CHAIN_BITS), 142.6, 78.2, 64, -5.0)]


def chain_raw(k: int) -> np.ndarray:
    """the raw image of frame k: the marker texture seen through features_reference.warp(k) at the mid scene's depth, with noise"""
    from lifcal_amd import raw_image, white_image
    from tests import features_reference as fref
    from tests import rawdepth_reference as ref

    def make():
        w, h, d, rot, off, bits, _, _ = ref.CASES[CHAIN_CASE]
        tx, ty = white_image.grid_centres(w, h, d, ref.BASE_Y, rot, off, 1.5)
        T, f = mi.marker_texture(chain_markers()), fref.warp(k, (h, w))
        img = raw_image.render_raw_image(w, h, tx, ty, d, ref.scene_depth(CHAIN_CASE, "mid"), lambda x, y: T(*f(x, y)), bits=bits, noise=ref.NOISE, seed=31 + k)
        img.setflags(write=False)
        return img
    return cached(("chain raw", k), make)


def chain_truth(k: int) -> dict:
    """id -> the centre of the marker in frame k: the pixel whose warp is the marker's centre on the texture"""
    from tests import features_reference as fref
    from tests import rawdepth_reference as ref
    w, h = ref.CASES[CHAIN_CASE][:2]
    f = fref.warp(k, (h, w))
    o = np.array(f(0.0, 0.0), np.float64); A = np.array([np.array(f(1.0, 0.0)) - o, np.array(f(0.0, 1.0)) - o]).T   # the warp is affine
    return {m.id: tuple(np.linalg.solve(A, np.array(m.centre) - o)) for m in chain_markers()}


def chain_totalfocus_restated(k: int):
    """(image, status) of frame k through the total-focus restatement with the true depth at scale 1"""
    from lifcal_amd import white_image
    from tests import rawdepth_reference as ref
    from tests import totalfocus_reference as tref

    def make():
        w, h, d, rot, off = ref.CASES[CHAIN_CASE][:5]
        tx, ty = white_image.grid_centres(w, h, d, ref.BASE_Y, rot, off, 1.5)
        tf = tref.render(chain_raw(k), tref.true_depth(CHAIN_CASE, "mid", 1), tx, ty, d)
        return tf.image, tf.status
    return cached(("chain tf", k), make)


def evaluate_chain(per_frame) -> dict:
    """per_frame[k]: the marker records of frame k.  The protocol of evaluate(): ids, extras, centre errors against chain_truth"""
    found, extra, total, err = 0, 0, 0, []
    for k, rec in enumerate(per_frame):
        truth = chain_truth(k)
        total += len(truth)
        seen = set()
        for r in rec:
            t = truth.get(int(r["id"]))
            e = None if t is None else math.hypot(float(r["x"]) - t[0], float(r["y"]) - t[1])
            if e is None or e > 2.0 or int(r["id"]) in seen:
                extra += 1
                continue
            seen.add(int(r["id"])); found += 1; err.append(e)
    err = np.array(err) if err else np.zeros(1)
    return dict(total=total, found=found, extra=extra, rms=float(np.sqrt(np.mean(err ** 2))), max=float(err.max()))


def check_chain_conditions(e: dict, what=""):
    assert e["found"] == e["total"] and e["extra"] == 0, (what, e)
    assert e["rms"] <= BARS["chain"]["rms"] and e["max"] <= BARS["chain"]["max"], (what, e, BARS)


# The rendered set through the restatement on the CPU (tests/test_markers_cpu.py::test_accuracy_of_the_restatement prints these):
# 24 of 24 found, none extra, 24 refined.
MEASURED = {
    "rendered": dict(rms=0.0292, max=0.0978),
    # the chain's three frames (raw image -> total-focus restatement with the true depth -> restatement of the detector): 6 of 6
    "chain": dict(rms=0.0940, max=0.1520),
}
BARS = {name: dict(rms=2 * v["rms"], max=2 * v["max"]) for name, v in MEASURED.items()}
