"""numpy restatement of lifcal_rawdepth_estimate (include/lifcal_rawdepth.h), the cases and scenes its
tests share, and the accuracy it was measured to have.

The restatement follows the header line by line with other means than the kernel: the tables are built from Python floats (IEEE
double, no fused multiply-add, libm's cos / sin / sqrt as on the host side of the library), the matching cost of one (neighbour,
hypothesis) pair is formed for the whole image at once by slicing shifted copies of the int64 image, and the selection rules are
applied to the full [K][height][width] cost volume, which the kernel never stores.  Equal bits are expected.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from lifcal_amd import raw_image, white_image

DEFAULTS = dict(n_hyp=64, iv_min=0.04, iv_max=0.5, patch_radius=1, max_baseline=1.05, min_neighbours=2, min_contrast=0, ambiguity_ratio=1.5)
MAX_NEIGHBOURS = 18


def options(bits: int, **kw) -> dict:
    o = dict(DEFAULTS); o.update(kw)
    if not o["min_contrast"]:
        o["min_contrast"] = 8 if bits == 8 else 2048
    return o


# ---------------------------------------------------------------------------------------------------------------- tables
@dataclass
class Tables:
    iv: list            # [K] hypotheses
    step: float
    delta: list         # [2][N] (dx, dy): lattice vectors to the neighbours of a lens of sub-grid 0 / 1
    shift: np.ndarray   # [2][N][K][2] int64, 1/64 pixel
    valid_r: float


def f32(x) -> float:
    return float(np.float32(x))


def lattice(d32, base_y32, rot32, rotation_on_grid=True):
    """A, C, D of DESIGN.md section 7s from the float parameters widened to double"""
    d, bx, by = f32(d32), f32(base_y32[0]), f32(base_y32[1])
    rot = f32(rot32) if rotation_on_grid else 0.0
    c, s = math.cos(rot), math.sin(rot)
    e1, e2 = (c, -s), (-s, -c)
    A = (d * e1[0], d * e1[1])
    Cv = (2.0 * by * d * e2[0], 2.0 * by * d * e2[1])
    D = ((1.0 + bx) * d * e1[0] + by * d * e2[0], (1.0 + bx) * d * e1[1] + by * d * e2[1])
    return A, Cv, D


def neighbours(d32, base_y32, rot32, max_baseline, rotation_on_grid=True):
    A, Cv, D = lattice(d32, base_y32, rot32, rotation_on_grid)
    limit = max_baseline * f32(d32)
    out = []
    for sub in (0, 1):
        cand = []
        for use_d in (0, 1):
            for x in range(-8, 9):
                for y in range(-8, 9):
                    vx = float(x) * A[0] + float(y) * Cv[0]
                    vy = float(x) * A[1] + float(y) * Cv[1]
                    if use_d:
                        vx, vy = (vx + D[0], vy + D[1]) if sub == 0 else (vx - D[0], vy - D[1])
                    elif x == 0 and y == 0:
                        continue
                    ln = math.sqrt(vx * vx + vy * vy)
                    if ln <= limit:
                        cand.append((ln, math.atan2(vy, vx), vx, vy))
        cand.sort()
        out.append([(c[2], c[3]) for c in cand])
    return out


def tables(d32, base_y32, rot32, opt: dict, rotation_on_grid=True) -> Tables:
    K = opt["n_hyp"]
    step = (opt["iv_max"] - opt["iv_min"]) / float(K - 1)
    iv = [opt["iv_min"] + float(k) * step for k in range(K)]
    delta = neighbours(d32, base_y32, rot32, opt["max_baseline"], rotation_on_grid)
    assert len(delta[0]) == len(delta[1]) <= MAX_NEIGHBOURS
    shift = np.zeros((2, len(delta[0]), K, 2), np.int64)
    for sub in (0, 1):
        for n, (dx, dy) in enumerate(delta[sub]):
            for k in range(K):
                t = 1.0 - iv[k]
                shift[sub, n, k, 0] = int(math.floor(64.0 * (dx * t) + 0.5))
                shift[sub, n, k, 1] = int(math.floor(64.0 * (dy * t) + 0.5))
    valid_r = float(np.float32(np.float32(d32) * np.float32(0.5)) - np.float32(1.0))
    return Tables(iv, step, delta, shift, valid_r)


def sub_grid_of(cx, cy, d32, base_y32, rot32, offset32, width, height, rotation_on_grid=True):
    """0 / 1 per lens, from the row of the lattice its centre lies on (the list holds sub-grid 0 first, this does not use that)"""
    rot = f32(rot32) if rotation_on_grid else 0.0
    ox, oy = f32(offset32[0]) + width / 2.0 - 0.5, -f32(offset32[1]) + height / 2.0 - 0.5
    e2 = (-math.sin(rot), -math.cos(rot))
    t = ((np.asarray(cx, np.float64) - ox) * e2[0] + (np.asarray(cy, np.float64) - oy) * e2[1]) / (f32(base_y32[1]) * f32(d32))
    r = np.floor(t + 0.5)
    assert np.abs(t - r).max() < 0.01
    return (r.astype(np.int64) & 1).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- the estimate
@dataclass
class Estimate:
    inv_depth: np.ndarray      # float32, NaN unless status 0
    cost: np.ndarray           # float32, NaN unless status 0 or 4
    status: np.ndarray         # uint8
    n_neighbours: np.ndarray   # uint8, 0 unless status 0 or 4
    counts: np.ndarray         # [5]


def _box(a: np.ndarray, w: int) -> np.ndarray:
    """sum over the (2w+1)^2 window, zero outside the array"""
    h, wd = a.shape
    p = np.zeros((h + 2 * w, wd + 2 * w), a.dtype)
    p[w:w + h, w:w + wd] = a
    out = np.zeros_like(a)
    for dy in range(2 * w + 1):
        for dx in range(2 * w + 1):
            out += p[dy:dy + h, dx:dx + wd]
    return out


def _window_minmax(a: np.ndarray, w: int):
    h, wd = a.shape
    lo = np.full((h + 2 * w, wd + 2 * w), np.iinfo(np.int64).max, np.int64); hi = np.full_like(lo, -1)
    lo[w:w + h, w:w + wd] = a; hi[w:w + h, w:w + wd] = a
    mn, mx = a.copy(), a.copy()
    for dy in range(2 * w + 1):
        for dx in range(2 * w + 1):
            mn = np.minimum(mn, lo[dy:dy + h, dx:dx + wd]); mx = np.maximum(mx, hi[dy:dy + h, dx:dx + wd])
    return mn, mx


def estimate(img: np.ndarray, cx32, cy32, map_ml: np.ndarray, sub: np.ndarray, tab: Tables, opt: dict) -> Estimate:
    H, W = img.shape
    I = img.astype(np.int64)
    w, K = opt["patch_radius"], opt["n_hyp"]
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    lens = np.where(map_ml >= 0, map_ml, 0)
    ox = xx - np.asarray(cx32, np.float32).astype(np.float64)[lens]
    oy = yy - np.asarray(cy32, np.float32).astype(np.float64)[lens]
    r0, r1 = tab.valid_r - w, tab.valid_r - w - 1
    xi, yi = xx.astype(np.int64), yy.astype(np.int64)
    patch_inside = (xi >= w) & (xi <= W - 1 - w) & (yi >= w) & (yi <= H - 1 - w)
    st1 = (map_ml < 0) | (not r0 >= 0) | (ox * ox + oy * oy > r0 * r0) | ~patch_inside
    mn, mx = _window_minmax(I, w)
    st2 = (mx - mn) < opt["min_contrast"]
    psub = np.asarray(sub)[lens]

    total = np.zeros((K, H, W), np.int64)
    count = np.zeros((K, H, W), np.int64)
    for s in (0, 1):
        in_sub = (psub == s) & ~st1
        if not in_sub.any():
            continue
        for n, (dx, dy) in enumerate(tab.delta[s]):
            for k in range(K):
                sx, sy = int(tab.shift[s, n, k, 0]), int(tab.shift[s, n, k, 1])
                ix, fx, iy, fy = sx >> 6, sx & 63, sy >> 6, sy & 63
                tx = ox - dx * tab.iv[k]; ty = oy - dy * tab.iv[k]
                ok = in_sub & (r1 >= 0) & (tx * tx + ty * ty <= r1 * r1)
                ok &= (xi - w + ix >= 0) & (xi + w + ix + 1 <= W - 1) & (yi - w + iy >= 0) & (yi + w + iy + 1 <= H - 1)
                if not ok.any():
                    continue
                # the abs-difference plane wherever the 2 x 2 support of the shifted sample lies inside the image
                x0, x1 = max(0, -ix), min(W, W - 1 - ix)          # x in [x0, x1): 0 <= x + ix and x + ix + 1 <= W - 1
                y0, y1 = max(0, -iy), min(H, H - 1 - iy)
                D = np.zeros((H, W), np.int64)
                if x1 > x0 and y1 > y0:
                    a = I[y0 + iy:y1 + iy, x0 + ix:x1 + ix]; b = I[y0 + iy:y1 + iy, x0 + ix + 1:x1 + ix + 1]
                    c = I[y0 + iy + 1:y1 + iy + 1, x0 + ix:x1 + ix]; e = I[y0 + iy + 1:y1 + iy + 1, x0 + ix + 1:x1 + ix + 1]
                    B = (64 - fx) * (64 - fy) * a + fx * (64 - fy) * b + (64 - fx) * fy * c + fx * fy * e
                    D[y0:y1, x0:x1] = np.abs(4096 * I[y0:y1, x0:x1] - B)
                P = _box(D, w)
                total[k][ok] += P[ok]
                count[k][ok] += 1

    with np.errstate(divide="ignore", invalid="ignore"):
        cost = np.where(count >= opt["min_neighbours"], total.astype(np.float64) / count.astype(np.float64), np.inf)
    inf = np.full((1, H, W), np.inf)
    cm = np.concatenate([inf, cost[:-1]]); cp = np.concatenate([cost[1:], inf])
    locmin = np.isfinite(cost) & (cost < cm) & (cost <= cp)
    kb = np.argmin(cost, axis=0)                                   # the lowest k of least cost
    take = lambda a: np.take_along_axis(a, kb[None], axis=0)[0]
    c0, c_m, c_p, nb = take(cost), take(cm), take(cp), take(count)
    with np.errstate(invalid="ignore"):
        den = (c_m - 2.0 * c0) + c_p
        st3 = ~np.isfinite(c0) | (kb == 0) | (kb == K - 1) | ~np.isfinite(c_m) | ~np.isfinite(c_p) | ~(den > 0)
        far = np.abs(np.arange(K)[:, None, None] - kb[None]) >= 3
        st4 = (locmin & far & (cost < opt["ambiguity_ratio"] * c0[None])).any(axis=0)
        iv = np.asarray(tab.iv)[kb] + ((0.5 * (c_m - c_p)) / den) * tab.step
    status = np.where(st1, 1, np.where(st2, 2, np.where(st3, 3, np.where(st4, 4, 0)))).astype(np.uint8)
    inv_depth = np.where(status == 0, iv, np.nan).astype(np.float32)
    has_min = (status == 0) | (status == 4)
    with np.errstate(invalid="ignore"):
        out_cost = np.where(has_min, c0 / (4096.0 * float((2 * w + 1) ** 2)), np.nan).astype(np.float32)
    nn = np.where(has_min, nb, 0).astype(np.uint8)
    return Estimate(inv_depth, out_cost, status, nn, np.bincount(status.ravel(), minlength=5)[:5].astype(np.uint64))


def points(inv_depth: np.ndarray, map_ml: np.ndarray, cx32, cy32, scale: int = 1):
    """lifcal_rawdepth_points: x, y, vdepth, src, lens of the status-0 pixels, ascending pixel index"""
    H, W = inv_depth.shape
    src = np.flatnonzero(~np.isnan(inv_depth.ravel()) & (map_ml.ravel() >= 0))
    lens = map_ml.ravel()[src]
    v = 1.0 / inv_depth.ravel()[src].astype(np.float64)
    px, py = (src % W).astype(np.float64), (src // W).astype(np.float64)
    lcx, lcy = np.asarray(cx32, np.float32).astype(np.float64)[lens], np.asarray(cy32, np.float32).astype(np.float64)[lens]
    xu = lcx + v * (px - lcx); yu = lcy + v * (py - lcy)
    return (xu + 0.5) / float(scale) - 0.5, (yu + 0.5) / float(scale) - 0.5, v, src.astype(np.uint32), lens.astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- cases and scenes
# name: (width, height, lens diameter, rotation, offset, bits, patch radius, extra columns of the host rows)
CASES = {
    "d14": (200, 160, 14.3, 0.003, (0.7, -0.4), 8, 1, 0),
    "d23_16": (176, 144, 23.2, 0.0, (0.0, 0.0), 16, 2, 0),
    "d9_pitch": (203, 131, 9.3, 0.0, (0.0, 0.0), 8, 1, 13),
}
BASE_Y = (-0.5, 0.8660254)
# Grids beyond the lattice of CASES (BASE_Y, rotation on the grid and next to zero), for the tests of the whole image chain on other
# geometries; a table of its own, so that the tests parametrised over CASES stay what they are.  The record of CASES and then
# lens_base_y, rotation_on_grid.  d14_rot: d14 turned by 0.03 rad.  d17_sq: the squeezed lattice of tests/test_gpu_mla.py's
# rotated_neg, whose six nearest neighbours are not equidistant (four at 0.995 d, two at d).  d14_rot_off: the rotation is not the
# grid's (rotation_on_grid = 0), so the lenses lie on the UNROTATED lattice, and the image is rendered there.  (At 16 bit with patch
# radius 2 the restatement does not meet CONDITIONS on 14.3-pixel lenses, coverage 0.04 near and 0.66 mid, so it is d14's 8 bit
# with radius 1.)
GEOMETRY_CASES = {
    "d14_rot": (200, 160, 14.3, 0.03, (3.7, -5.4), 8, 1, 0, BASE_Y, True),
    "d17_sq": (211, 157, 17.35, -0.021, (5.25, 7.5), 8, 1, 0, (0.5, 0.86), True),
    "d14_rot_off": (200, 160, 14.3, 0.03, (0.7, -0.4), 8, 1, 0, BASE_Y, False),
}
# a grid of lenses so small that at patch radius 2 no pair counts (valid_r = 2.25: r0 = 0.25, r1 < 0), for the option tests
OPTION_CASES = {"d6": (96, 80, 6.5, 0.0, (0.0, 0.0), 8, 1, 0, BASE_Y, True)}


def case(name: str) -> tuple:
    """the record of a case of any table, with lens_base_y and rotation_on_grid (BASE_Y and on the grid for CASES)"""
    if name in CASES:
        return CASES[name] + (BASE_Y, True)
    return GEOMETRY_CASES[name] if name in GEOMETRY_CASES else OPTION_CASES[name]


def grid_rotation(name: str) -> float:
    """the rotation of the lattice the lenses lie on: the case's, or 0 where the rotation is not the grid's"""
    c = case(name)
    return c[3] if c[9] else 0.0


STEP_X, STEP_EXCLUDE = 100.3, 12.0
# The scenes: fronto-parallel planes at a near, a middle and a far virtual depth, and one depth step at x_v = STEP_X.
# near / mid / far / (left, right of the step).  The 9.3-pixel lenses of d9_pitch cannot measure the depths of the other two
# cases: with w = 1 a pixel lies within 2.65 px of its centre and its match within 1.65 px of the neighbour's, so at v = 4 the
# disparity of 2.3 px leaves at most one neighbour for two thirds of the pixels (measured: coverage 29 % at v = 4, 1 % at 2.6,
# whatever the texture).  Its scenes are the same four at depths its geometry reaches; the conditions below are unchanged.
SCENE_DEPTHS = {
    "d14": dict(near=2.6, mid=4.0, far=7.0, step=(3.2, 5.5)),
    "d23_16": dict(near=2.6, mid=4.0, far=7.0, step=(3.2, 5.5)),
    "d9_pitch": dict(near=4.5, mid=5.5, far=7.0, step=(5.0, 7.0)),
}
SCENE_DEPTHS.update({name: SCENE_DEPTHS["d14"] for name in GEOMETRY_CASES})
SCENE_DEPTHS["d6"] = SCENE_DEPTHS["d9_pitch"]
SCENE_NAMES = ("near", "mid", "far", "step")
TEXTURE = dict(seed=7, lambda_min=18.0, lambda_max=60.0)   # at least 2.5 v raw pixels in the virtual image up to v = 7
NOISE = 0.004
# (coverage at least, outlier share at most) per scene: the conditions of the issue, so that the status gates cannot hide a
# failure.  Coverage: status-0 pixels among the pixels not in status 1; outliers: status-0 pixels with |e| > OUTLIER.
CONDITIONS = {"near": (0.30, 0.04), "mid": (0.70, 0.015), "far": (0.70, 0.015), "step": (0.60, 0.015)}
OUTLIER = 0.02
# neighbour sets the accuracy is measured and tested with (max_baseline): d9_pitch's conditions need the 18
ACCURACY_BASELINES = {"d14": (1.05, 2.1), "d23_16": (1.05, 2.1), "d9_pitch": (2.1,)}
ACCURACY_BASELINES.update({name: (1.05, 2.1) for name in GEOMETRY_CASES})


def scene_depth(name: str, scene: str):
    v = SCENE_DEPTHS[name][scene]
    return raw_image.step_depth(v[0], v[1], STEP_X) if scene == "step" else raw_image.plane_depth(v)


@functools.lru_cache(maxsize=None)
def texture():
    return raw_image.band_limited_texture(TEXTURE["seed"], TEXTURE["lambda_min"], TEXTURE["lambda_max"])


@functools.lru_cache(maxsize=None)
def make_case(name: str, scene: str, noise: float = 0.0) -> np.ndarray:
    """the rendered raw image of a case (cached: shared by the tests, never modified)"""
    w, h, d, _, off, bits, _, _, base_y, _ = case(name)
    tx, ty = white_image.grid_centres(w, h, d, base_y, grid_rotation(name), off, 1.5)
    img = raw_image.render_raw_image(w, h, tx, ty, d, scene_depth(name, scene), texture(), bits=bits, noise=noise, seed=11)
    img.setflags(write=False)
    return img


def true_inverse_depth(name: str, scene: str, cx32, cy32, map_ml: np.ndarray) -> np.ndarray:
    """1 / v of what each pixel shows, through the centre of the lens the library assigns it to (NaN without a lens); also
    the virtual-image x of the pixel, which the step scene's exclusion band needs"""
    w, h = case(name)[:2]
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    lens = np.where(map_ml >= 0, map_ml, 0)
    lcx, lcy = np.asarray(cx32, np.float64)[lens], np.asarray(cy32, np.float64)[lens]
    v = raw_image.virtual_depth_at(xx, yy, lcx, lcy, scene_depth(name, scene))
    return np.where(map_ml >= 0, 1.0 / v, np.nan), lcx + v * (xx - lcx)


def accuracy(name: str, scene: str, est, cx32, cy32, map_ml) -> dict:
    """inlier RMS and |median| of e = iv - 1 / v_true over the status-0 pixels, coverage and outlier share"""
    truth, xv = true_inverse_depth(name, scene, cx32, cy32, map_ml)
    use = np.ones(est.status.shape, bool)
    if scene == "step":
        use = np.abs(xv - STEP_X) > STEP_EXCLUDE
    ok = (est.status == 0) & use
    e = est.inv_depth[ok].astype(np.float64) - truth[ok]
    inl = np.abs(e) <= OUTLIER
    return dict(coverage=float(ok.sum()) / float(((est.status != 1) & use).sum()), outliers=float((~inl).sum()) / max(1, e.size),
                rms=float(np.sqrt(np.mean(e[inl] ** 2))), median=float(abs(np.median(e))), n=int(e.size))


# Measured with this restatement (tests/test_rawdepth_cpu.py prints the figures): the largest inlier RMS and |median e| over the
# scenes of a case at noise 0 and NOISE, 6 and 18 neighbours, K = 64.  The bars are twice that: the margin covers other seeds, not
# other arithmetic (the kernel's bits are the restatement's).
MEASURED = {
    "d14": dict(rms=0.00386, median=0.00076),        # near scene with noise; far scene with 18 neighbours
    "d23_16": dict(rms=0.00100, median=0.00076),     # step scene with noise; mid scene with 18 neighbours
    "d9_pitch": dict(rms=0.00446, median=0.00117),   # near scene with noise; far scene
    # GEOMETRY_CASES, measured the same way (tests/test_rawdepth_cpu.py runs both noise levels for them)
    "d14_rot": dict(rms=0.00410, median=0.00059),        # near scene with noise, 6 neighbours; near scene, 18 neighbours
    "d17_sq": dict(rms=0.00303, median=0.00134),         # near scene with noise, 6 neighbours; far scene, 6 neighbours
    "d14_rot_off": dict(rms=0.00375, median=0.00067),    # near scene with noise, 6 neighbours; far scene, 6 neighbours
}
BARS = {name: dict(rms=2 * m["rms"], median=2 * m["median"]) for name, m in MEASURED.items()}


# ---------------------------------------------------------------------------------------------------------------- shared runs
@dataclass
class GridData:
    cx: np.ndarray        # float32 lens centres, list order
    cy: np.ndarray
    map_ml: np.ndarray    # [height][width] int32
    sub: np.ndarray       # sub-grid per lens


def grid_data(name: str, grid) -> GridData:
    """what the restatement needs of a micro-lens grid: `grid` has lenses() and maps() (lifcal_amd.MicroLensGrid on the GPU, or
    oracle.mla.MicroLensGrid, whose lists and maps are the same bits)"""
    w, h, d, rot, off, _, _, _, base_y, on_grid = case(name)
    cx, cy, _ = grid.lenses()
    map_ml, _ = grid.maps()
    return GridData(cx, cy, map_ml, sub_grid_of(cx, cy, d, base_y, rot, off, w, h, on_grid))


def grid_arguments(name: str):
    """positional arguments of MicroLensGrid for a case"""
    w, h, d, rot, off, _, _, _, base_y, on_grid = case(name)
    return w, h, d, base_y, rot, off, on_grid


_RUNS = {}


def run(name: str, scene: str, noise: float, gd: GridData, tables_rotation=None, **opts) -> Estimate:
    """the restatement on a case's image (cached: computed once, shared by the tests, never modified).  patch_radius is the case's
    unless given.  tables_rotation: build the tables for a lattice turned by this angle instead of the case's own, a deliberately
    WRONG restatement for the tests that show which cases can tell."""
    key = (name, scene, noise, tables_rotation, tuple(sorted(opts.items())))
    if key not in _RUNS:
        w, h, d, rot, off, bits, pr, _, base_y, on_grid = case(name)
        opt = options(bits, **{"patch_radius": pr, **opts})
        tab = tables(d, base_y, rot, opt, on_grid) if tables_rotation is None else tables(d, base_y, tables_rotation, opt, True)
        _RUNS[key] = estimate(make_case(name, scene, noise), gd.cx, gd.cy, gd.map_ml, gd.sub, tab, opt)
    return _RUNS[key]
