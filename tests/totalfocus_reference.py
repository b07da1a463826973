"""numpy restatement of lifcal_totalfocus_render (include/lifcal_totalfocus.h), the scenes, truth and white
images its tests share, and the accuracy it was measured to have on the scenes of tests/rawdepth_reference.py.

The restatement follows the header with other means than the kernel: it loops over ALL lenses of the list, and for each lens it
applies the tests of the header to every cell at once; there are no bins and no tiles.  The sums are int64 arrays and the pixel is
an integer division of whole arrays.  Python floats are IEEE doubles without fused multiply-add, and all that is summed is an
integer: equal bytes are expected.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from lifcal_amd import white_image
from tests import depthmap_reference as dref
from tests import rawdepth_reference as ref

DEFAULTS = dict(scale=1, out_width=0, out_height=0, min_lenses=1, white_level=0, margin=1.5, max_reach=4.0, iv_min=0.04, default_iv=0.0)
OK, NO_DEPTH, NO_LENS, DEFAULT_DEPTH = range(4)


def options(width: int, height: int, bits: int, **kw) -> dict:
    """the options with the defaults of the header filled in"""
    o = dict(DEFAULTS); o.update(kw)
    for k, v in DEFAULTS.items():
        if k not in ("out_width", "out_height", "default_iv", "white_level") and o[k] == 0:
            o[k] = v
    if not o["white_level"]:
        o["white_level"] = (1 << bits) - 1
    if not o["out_width"]:
        o["out_width"] = width // o["scale"]
    if not o["out_height"]:
        o["out_height"] = height // o["scale"]
    return o


def valid_radius(d32) -> float:
    return float(np.float32(np.float32(d32) * np.float32(0.5)) - np.float32(1.0))


def plan(width: int, height: int, bits: int, d32, base_y1_32, **kw) -> dict:
    """what lifcal_totalfocus_check reports: output size, r_use and the bound on the lenses of one cell"""
    o = options(width, height, bits, **kw)
    span = 2.0 * (o["max_reach"] + 1.0)
    bound = (math.floor(span / float(np.float32(base_y1_32))) + 1.0) * (math.floor(span) + 1.0)
    return dict(out_width=o["out_width"], out_height=o["out_height"], r_use=valid_radius(d32) - o["margin"], max_lenses_per_cell=int(bound), options=o)


@dataclass
class TotalFocus:
    image: np.ndarray       # uint8 / uint16 like the raw image
    n_lenses: np.ndarray    # uint8
    status: np.ndarray      # uint8
    counts: np.ndarray      # [4] uint64
    n: np.ndarray           # int64 lenses that counted, unsaturated (not an output of the library)


def _bilinear(I: np.ndarray, ix, iy, fx, fy):
    return (64 - fx) * (64 - fy) * I[iy, ix] + fx * (64 - fy) * I[iy, ix + 1] + (64 - fx) * fy * I[iy + 1, ix] + fx * fy * I[iy + 1, ix + 1]


def render(img: np.ndarray, inv_depth: np.ndarray, cx32, cy32, d32, white=None, **kw) -> TotalFocus:
    H, W = img.shape
    bits = 8 * img.dtype.itemsize
    full = (1 << bits) - 1
    o = options(W, H, bits, **kw)
    ow, oh = o["out_width"], o["out_height"]
    assert inv_depth.shape == (oh, ow)
    d = float(np.float32(d32))
    r_use = valid_radius(d32) - o["margin"]
    r_use2 = r_use * r_use
    reach = o["max_reach"] * d
    reach2 = reach * reach
    scale = float(o["scale"])
    iv_all = inv_depth.astype(np.float64).ravel()
    with np.errstate(invalid="ignore"):
        has = ~np.isnan(iv_all) & (iv_all >= o["iv_min"]) & (iv_all <= 1.0)
    active = has | (o["default_iv"] > 0.0)
    iv_all = np.where(has, iv_all, o["default_iv"])
    cells = np.flatnonzero(active)
    iv = iv_all[cells]
    xu = ((cells % ow).astype(np.float64) + 0.5) * scale - 0.5
    yu = ((cells // ow).astype(np.float64) + 0.5) * scale - 0.5
    I = img.astype(np.int64)
    Wh = white.astype(np.int64) if white is not None else None
    num = np.zeros(cells.size, np.int64); den = np.zeros(cells.size, np.int64); n = np.zeros(cells.size, np.int64)
    for cx, cy in zip(np.asarray(cx32, np.float32).astype(np.float64).tolist(), np.asarray(cy32, np.float32).astype(np.float64).tolist()):
        dx = xu - cx; dy = yu - cy
        k = np.flatnonzero(dx * dx + dy * dy <= reach2)
        if not k.size:
            continue
        ox = dx[k] * iv[k]; oy = dy[k] * iv[k]
        m = ox * ox + oy * oy <= r_use2
        k, ox, oy = k[m], ox[m], oy[m]
        Sx = np.floor(64.0 * (cx + ox) + 0.5).astype(np.int64); Sy = np.floor(64.0 * (cy + oy) + 0.5).astype(np.int64)
        ix, fx, iy, fy = Sx >> 6, Sx & 63, Sy >> 6, Sy & 63
        m = (ix >= 0) & (ix + 1 <= W - 1) & (iy >= 0) & (iy + 1 <= H - 1)
        k, ix, fx, iy, fy = k[m], ix[m], fx[m], iy[m], fy[m]
        if not k.size:
            continue
        num[k] += _bilinear(I, ix, iy, fx, fy)
        if Wh is not None:
            den[k] += _bilinear(Wh, ix, iy, fx, fy)
        n[k] += 1
    enough = n >= o["min_lenses"]
    if Wh is None:
        pixel = (2 * num + 4096 * n) // np.maximum(2 * 4096 * n, 1)
    else:
        enough &= den > 0
        pixel = np.minimum(full, (2 * num * o["white_level"] + den) // np.maximum(2 * den, 1))
    status = np.full(ow * oh, NO_DEPTH, np.uint8)
    status[cells] = np.where(enough, np.where(has[cells], OK, DEFAULT_DEPTH), NO_LENS)
    image = np.zeros(ow * oh, img.dtype); image[cells] = np.where(enough, pixel, 0)
    n_all = np.zeros(ow * oh, np.int64); n_all[cells] = n
    return TotalFocus(image.reshape(oh, ow), np.minimum(n_all, 255).astype(np.uint8).reshape(oh, ow), status.reshape(oh, ow),
                      np.bincount(status, minlength=4)[:4].astype(np.uint64), n_all.reshape(oh, ow))


# ---------------------------------------------------------------------------------------------------------------- scenes and truth
SCALES = (1, 2)
LEVEL = 0.9                                             # render_raw_image's level: texture value 1 as a fraction of full scale
WHITE = dict(fill=0.94, falloff=0.7, level=0.8, vignetting=0.6)
EQUALITY_SCENES = ("mid", "step")


def cell_centres(ow: int, oh: int, scale: int):
    Y, X = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
    return (X + 0.5) * float(scale) - 0.5, (Y + 0.5) * float(scale) - 0.5


def out_shape(name: str, scale: int):
    w, h = ref.case(name)[:2]
    return h // scale, w // scale


@functools.lru_cache(maxsize=None)
def truth(name: str, scale: int) -> np.ndarray:
    """level * T(xu, yu) * full at the cell centres: what the total-focus image shows of any scene of the case (the texture lies
    on the virtual image, whatever the depth)"""
    oh, ow = out_shape(name, scale)
    xu, yu = cell_centres(ow, oh, scale)
    t = LEVEL * ref.texture()(xu, yu) * float((1 << ref.case(name)[5]) - 1)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def true_depth(name: str, scene: str, scale: int) -> np.ndarray:
    """the TRUE inverse virtual depth sampled at the cell centres, as the float map the library takes"""
    oh, ow = out_shape(name, scale)
    xu, yu = cell_centres(ow, oh, scale)
    iv = (1.0 / ref.scene_depth(name, scene)(xu, yu)).astype(np.float32)
    iv.setflags(write=False)
    return iv


@functools.lru_cache(maxsize=None)
def white_case(name: str) -> np.ndarray:
    """a white image of the case's grid with fall-off inside every disc and vignetting across the sensor"""
    w, h, d, _, off, bits, _, _, base_y, _ = ref.case(name)
    tx, ty = white_image.grid_centres(w, h, d, base_y, ref.grid_rotation(name), off, 1.5)
    wh = white_image.render_white_image(w, h, tx, ty, d, bits=bits, **WHITE)
    wh.setflags(write=False)
    return wh


def white_level(name: str) -> int:
    return int(math.floor(WHITE["level"] * float((1 << ref.case(name)[5]) - 1) + 0.5))


@functools.lru_cache(maxsize=None)
def vignetted_case(name: str, scene: str, noise: float) -> np.ndarray:
    """what the sensor records behind lenses that shade like white_case: raw * white / white's level, rounded"""
    full = float((1 << ref.case(name)[5]) - 1)
    raw = ref.make_case(name, scene, noise).astype(np.float64)
    img = np.clip(np.floor(raw * white_case(name).astype(np.float64) / (WHITE["level"] * full) + 0.5), 0.0, full).astype(ref.make_case(name, scene, noise).dtype)
    img.setflags(write=False)
    return img


# ---------------------------------------------------------------------------------------------------------------- accuracy
def interior(name: str, scene: str, scale: int) -> np.ndarray:
    """cells at least ceil(1.5 d / scale) from the border; on `step` without the cells within STEP_EXCLUDE of the step"""
    oh, ow = out_shape(name, scale)
    m = int(math.ceil(1.5 * ref.case(name)[2] / scale))
    Y, X = np.meshgrid(np.arange(oh), np.arange(ow), indexing="ij")
    inner = (X >= m) & (X <= ow - 1 - m) & (Y >= m) & (Y <= oh - 1 - m)
    if scene == "step":
        xu, _ = cell_centres(ow, oh, scale)
        inner &= np.abs(xu - ref.STEP_X) > ref.STEP_EXCLUDE
    return inner


def accuracy(name: str, scene: str, tf, scale: int) -> dict:
    """over the status-0 interior cells, as fractions of full scale: RMS of pixel - truth, and the same against truth displaced by
    one cell in +x, -x, +y, -y (the interior keeps a margin, so the displaced cells exist); the share of interior cells with
    status 0 and the fewest lenses among them"""
    full = float((1 << ref.case(name)[5]) - 1)
    inner = interior(name, scene, scale)
    status, image, nl = np.asarray(tf.status), np.asarray(tf.image).astype(np.float64), np.asarray(tf.n_lenses)
    use = inner & (status == OK)
    t = truth(name, scale)
    rms = lambda ref_img: float(np.sqrt(np.mean((image[use] - ref_img[use]) ** 2))) / full if use.any() else 0.0
    moved = [rms(np.roll(t, s, axis=ax)) for ax in (1, 0) for s in (1, -1)]
    return dict(rms=rms(t), displaced=min(moved), share=float(use.sum()) / float(inner.sum()), min_lenses=int(nl[use].min()) if use.any() else 0,
                n=int(use.sum()))


def describe(a: dict) -> str:
    return f"rms {a['rms']:.5f}, least displaced rms {a['displaced']:.5f}, status-0 share {a['share']:.4f}, at least {a['min_lenses']} lenses, {a['n']} cells"


def check_registration(a: dict, what):
    """condition 2 of the issue: the image is registered to the grid to better than one cell"""
    assert a["displaced"] > a["rms"], (what, a)


# Measured with this restatement (tests/test_totalfocus_cpu.py prints the figures): the largest RMS of pixel - truth over the
# status-0 interior cells, as a fraction of full scale, over the four scenes of a case, scale 1 and 2, noise 0 and NOISE, with the
# true depth and with the depth map of the restatement chain (18 neighbours).  The bars are twice that: the margin covers other
# seeds, not other arithmetic (the kernel's bytes are the restatement's).
# The error is the capture's own blur (a raw pixel averages v virtual pixels), so it grows with the depth and the far scene sets
# every figure: d14 near / mid / far with the true depth 0.0088 / 0.0191 / 0.0497.  The vignetted image with its white image stays
# below the same figures; without the white image it reads 0.105 .. 0.158.
MEASURED = {
    "d14": dict(rms=0.04972),        # far scene with noise, chained depth, scale 1
    "d23_16": dict(rms=0.05029),     # far scene, true depth with the white image, scale 2
    "d9_pitch": dict(rms=0.05135),   # far scene with noise, chained depth, scale 1
    # rawdepth_reference.GEOMETRY_CASES: the same over the true and the chained depth, without the white image
    "d14_rot": dict(rms=0.04971),        # far scene, chained depth, scale 2
    "d17_sq": dict(rms=0.04993),         # far scene with noise, chained depth, scale 2
    "d14_rot_off": dict(rms=0.04973),    # far scene with noise, chained depth, scale 1
}
BARS = {name: dict(rms=2 * m["rms"]) for name, m in MEASURED.items()}

_RENDERS = {}


def run_true(name: str, scene: str, noise: float, gd, scale: int = 1, white: bool = False, **kw) -> TotalFocus:
    """the restatement with the true depth (cached: computed once, shared by the tests, never modified); white: the vignetted
    raw image with its white image"""
    key = ("true", name, scene, noise, scale, white, tuple(sorted(kw.items())))
    if key not in _RENDERS:
        d = ref.case(name)[2]
        if white:
            _RENDERS[key] = render(vignetted_case(name, scene, noise), true_depth(name, scene, scale), gd.cx, gd.cy, d, white=white_case(name), scale=scale,
                                   white_level=white_level(name), **kw)
        else:
            _RENDERS[key] = render(ref.make_case(name, scene, noise), true_depth(name, scene, scale), gd.cx, gd.cy, d, scale=scale, **kw)
    return _RENDERS[key]


def run_chained(name: str, scene: str, noise: float, gd, scale: int = 1, **kw):
    """(the restatement on the depth map of the restatement chain, that depth map), cached likewise"""
    key = ("chained", name, scene, noise, scale, tuple(sorted(kw.items())))
    dm = dref.run(name, scene, noise, gd, scale)
    if key not in _RENDERS:
        _RENDERS[key] = render(ref.make_case(name, scene, noise), dm.inv_depth, gd.cx, gd.cy, ref.case(name)[2], scale=scale, **kw)
    return _RENDERS[key], dm
