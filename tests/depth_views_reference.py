"""Restatements that the cross-view depth tests compare the GPU paths with (include/lifcal_depth.h (d)-(f)).

    forward_exact       the forward model of lifcal_depth_project_points, operation by operation (what projectPointBack inverts)
    frame_table         lifcal::frame_eval: R row-major, then t
    pair_transform      RT_t * RT_s^-1 as the per-pair table of the kernels forms it
    check_ref           lifcal_depth_check_maps: support, conflict and the pair table
    fuse_ref            lifcal_depth_fuse_maps: the ordered fused cloud
    views_fixture       five rendered maps of 83 x 61 with their poses; small_fixture: three of 4 x 3
Every operation is an IEEE double operation in the kernels' order; numpy does not contract a * b + c.  The only operations the
GPU does differently are the sines and cosines of frame_eval (another libm), which is why world coordinates and sums are compared
at 1e-12 and everything upstream of a pose bit for bit.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import depth_reference as dr

STEP = 1.0 / 65535.0             # one raw step of inverse virtual depth
NO_DATA, CONSISTENT, OCCLUDED, VIOLATION = 0, 1, 2, 3
PAIR_DTYPE = np.dtype([("n_valid", "<u8"), ("n_compared", "<u8"), ("n_consistent", "<u8"), ("n_occluded", "<u8"), ("n_violation", "<u8"),
                       ("sum_e", "<f8"), ("sum_e2", "<f8")])


def forward_exact(p_c, cam, config, spx, spy=None):
    """camera coordinates (n, 3) -> (x_v, y_v, v, ok).  Invalid points (a coordinate not finite, Z <= 0, Z == fL, v not > 0) give
    NaN in all three and ok False.  Powers are repeated products, the two distortion formulas are the reference's
    (src/CameraModel.h:205-241) evaluated at the undistorted point."""
    fL, bL0, B, cx, cy, radial, tangential = dr.camera_parts(np.asarray(cam, np.float64), config)
    spy = spx if spy is None else spy
    p_c = np.asarray(p_c, np.float64).reshape(-1, 3)
    X, Y, Z = p_c[:, 0].copy(), p_c[:, 1].copy(), p_c[:, 2].copy()
    ok = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z) & (Z > 0.0) & (Z != fL)
    X[~ok] = 0.0; Y[~ok] = 0.0; Z[~ok] = 2.0 * fL + 1.0        # any harmless value: the rows are overwritten below
    x_u = X / Z * bL0
    y_u = Y / Z * bL0
    dx = np.zeros_like(x_u); dy = np.zeros_like(y_u)
    if len(radial) > 0:                                          # radialDistortion (:205-223)
        r0 = x_u * x_u + y_u * y_u
        delta_r = radial[0] * r0
        r_prev = r0
        for i in range(1, len(radial)):
            r_i = r_prev * r0
            delta_r = delta_r + radial[i] * r_i
            r_prev = r_i
        dx = dx + x_u * delta_r
        dy = dy + y_u * delta_r
    if tangential is not None:                                   # tangentialDistortion (:228-241)
        r_2 = x_u * x_u + y_u * y_u
        dx = dx + (tangential[0] * (r_2 + 2.0 * x_u * x_u) + 2.0 * tangential[1] * x_u * y_u)
        dy = dy + (tangential[1] * (r_2 + 2.0 * y_u * y_u) + 2.0 * tangential[0] * x_u * y_u)
    b = fL * Z / (Z - fL)
    v = (b - bL0) / B
    ok &= v > 0.0
    s = bL0 + v * B
    x_v = (x_u + dx) * s / bL0 / spx + cx
    y_v = (y_u + dy) * s / bL0 / spy + cy
    x_v[~ok] = np.nan; y_v[~ok] = np.nan; v = np.where(ok, v, np.nan)
    return x_v, y_v, v, ok


def frame_table(view):
    """frame_eval of device_model.hpp: R = Rx Ry Rz row-major at [0..8], t at [9..11]"""
    s0, c0, s1, c1, s2, c2 = np.sin(view[0]), np.cos(view[0]), np.sin(view[1]), np.cos(view[1]), np.sin(view[2]), np.cos(view[2])
    return np.array([c1 * c2, -c1 * s2, s1,
                     c0 * s2 + s0 * s1 * c2, c0 * c2 - s0 * s1 * s2, -s0 * c1,
                     s0 * s2 - c0 * s1 * c2, s0 * c2 + c0 * s1 * s2, c0 * c1,
                     view[3], view[4], view[5]])


def to_camera(ft, p_w):
    """p_c = R p_w + t in the order of the kernels"""
    return np.stack([ft[3 * j] * p_w[:, 0] + ft[3 * j + 1] * p_w[:, 1] + ft[3 * j + 2] * p_w[:, 2] + ft[9 + j] for j in range(3)], -1)


def to_world(ft, p_c):
    """p_w = R^T (p_c - t), depth::to_world"""
    d0 = p_c[:, 0] - ft[9]; d1 = p_c[:, 1] - ft[10]; d2 = p_c[:, 2] - ft[11]
    return np.stack([ft[j] * d0 + ft[3 + j] * d1 + ft[6 + j] * d2 for j in range(3)], -1)


def pair_transform(ft_s, ft_t):
    """M = R_t R_s^T (row-major at [0..8]) and t_t - M t_s (at [9..11]): source camera coordinates -> target camera coordinates"""
    out = np.zeros(12)
    for a in range(3):
        for b in range(3):
            out[3 * a + b] = ft_t[3 * a] * ft_s[3 * b] + ft_t[3 * a + 1] * ft_s[3 * b + 1] + ft_t[3 * a + 2] * ft_s[3 * b + 2]
    for a in range(3):
        out[9 + a] = ft_t[9 + a] - (out[3 * a] * ft_s[9] + out[3 * a + 1] * ft_s[10] + out[3 * a + 2] * ft_s[11])
    return out


def slot_target(s, j, span):
    return s + j - span + (1 if j >= span else 0)


def _pair_pixels(raw, cam, config, spx, fts, s, t, tol_iv, spy=None):
    """One source map against one target.  For every pixel of s (flattened row-major): class, e, the sampled target pixel
    (flattened index, -1 without one) and its v_obs."""
    count, H, W = raw.shape
    v_s = dr.decode_direct(raw[s]).reshape(-1)
    ok_s = np.isfinite(v_s)
    idx = np.nonzero(ok_s)[0]
    cls = np.full(H * W, -1, np.int64); e_all = np.zeros(H * W); tpix = np.full(H * W, -1, np.int64); vobs_all = np.full(H * W, np.nan)
    if len(idx) == 0:
        return cls, e_all, tpix, vobs_all
    rows, cols = idx // W, idx % W
    p_s = dr.back_project_cam(cols, rows, v_s[idx], cam, config, spx, spy=spy)
    p_t = to_camera(pair_transform(fts[s], fts[t]), p_s)         # the 12 entries are laid out like a frame table
    x_t, y_t, v_pred, okf = forward_exact(p_t, cam, config, spx, spy=spy)
    with np.errstate(invalid="ignore"):
        fx = x_t + 0.5; fy = y_t + 0.5
        okf = okf & (fx > -1.0e9) & (fx < 1.0e9) & (fy > -1.0e9) & (fy < 1.0e9)
    px = np.where(okf, np.trunc(np.where(okf, fx, 0.0)), -1).astype(np.int64)   # (int) of C: truncation towards zero
    py = np.where(okf, np.trunc(np.where(okf, fy, 0.0)), -1).astype(np.int64)
    inside = okf & (px >= 0) & (px < W) & (py >= 0) & (py < H)
    v_t = dr.decode_direct(raw[t]).reshape(-1)
    flat = np.where(inside, py * W + px, 0)
    v_obs = np.where(inside, v_t[flat], np.nan)
    have = inside & np.isfinite(v_obs)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = 1.0 / v_obs - 1.0 / v_pred
    c = np.full(len(idx), NO_DATA, np.int64)
    c[have & (np.abs(e) <= tol_iv)] = CONSISTENT
    c[have & (e < -tol_iv)] = OCCLUDED
    c[have & (e > tol_iv)] = VIOLATION
    cls[idx] = c
    e_all[idx] = np.where(have, e, 0.0)
    tpix[idx] = np.where(have, flat, -1)
    vobs_all[idx] = v_obs
    return cls, e_all, tpix, vobs_all


def check_ref(raw, cam, config, spx, frame, views, span=1, tol_iv=4 * STEP, details=False, spy=None):
    """lifcal_depth_check_maps on host arrays: raw (count, H, W) uint16.  Returns (support, conflict, pair) with pair a
    (count, 2 span) array of PAIR_DTYPE; details=True adds {(s, t): (cls, e, target pixel, v_obs)} and the distance of the nearest
    |e| to the threshold.  sum_e / sum_e2 are plain numpy sums: the comparison is at 1e-12, not bitwise."""
    raw = np.asarray(raw, np.uint16)
    count, H, W = raw.shape
    views = np.asarray(views, np.float64).reshape(-1, 6)
    fts = [frame_table(views[f]) for f in np.asarray(frame).reshape(-1)]
    support = np.zeros((count, H * W), np.uint8); conflict = np.zeros((count, H * W), np.uint8)
    pair = np.zeros((count, 2 * span), PAIR_DTYPE)
    per_pair = {}
    nearest = np.inf
    for s in range(count):
        for j in range(2 * span):
            t = slot_target(s, j, span)
            if t < 0 or t >= count:
                continue
            cls, e, tpix, v_obs = _pair_pixels(raw, cam, config, spx, fts, s, t, tol_iv, spy=spy)
            con = cls == CONSISTENT
            support[s] += con.astype(np.uint8); conflict[s] += (cls == VIOLATION).astype(np.uint8)
            row = pair[s, j]
            row["n_valid"] = int(np.sum(cls >= 0)); row["n_compared"] = int(np.sum(cls > 0))
            row["n_consistent"] = int(con.sum()); row["n_occluded"] = int(np.sum(cls == OCCLUDED)); row["n_violation"] = int(np.sum(cls == VIOLATION))
            row["sum_e"] = float(np.sum(e[con])); row["sum_e2"] = float(np.sum(e[con] * e[con]))
            if np.any(cls > 0):
                nearest = min(nearest, float(np.min(np.abs(np.abs(e[cls > 0]) - tol_iv))))
            per_pair[(s, t)] = (cls, e, tpix, v_obs)
    support = support.reshape(count, H, W); conflict = conflict.reshape(count, H, W)
    if details:
        return support, conflict, pair, per_pair, nearest
    return support, conflict, pair


def depth_weight(v, cam):
    """1 / (g v^2)^2 with g = dz/dv = -B fL^2 / (b - fL)^2, b = bL0 + v B: the inverse variance of z for noise uniform in 1/v"""
    fL, bL0, B = cam[0], cam[1], cam[2]
    b = bL0 + v * B
    d = b - fL
    g = -B * fL * fL / (d * d)
    gv = g * v * v
    return 1.0 / (gv * gv)


def fuse_ref(raw, cam, config, spx, frame, views, span=1, tol_iv=4 * STEP, min_support=1, max_conflict=0):
    """lifcal_depth_fuse_maps.  Returns (xyz (n, 3), n_merged (n,), src (n,)) in ascending src.

    A pixel emits when it is valid, support >= min_support, conflict <= max_conflict and no target with a smaller map index is
    CONSISTENT with it.  The counts are the pixel's own: consistency is judged from the source pixel towards the nearest pixel of
    the target, so it is not symmetric.  Pixel a of map 1 may be consistent with pixel b of map 0 (and defer) while b, sampled the
    other way, lands on a neighbour of a and finds that one inconsistent, or the reverse: a surface point can then be emitted by
    both maps, or at a depth edge by neither.  That is the price of nearest-pixel sampling and is left as it is."""
    raw = np.asarray(raw, np.uint16)
    count, H, W = raw.shape
    cam = np.asarray(cam, np.float64)
    views = np.asarray(views, np.float64).reshape(-1, 6)
    fts = [frame_table(views[f]) for f in np.asarray(frame).reshape(-1)]
    support, conflict, pair, per_pair, _ = check_ref(raw, cam, config, spx, frame, views, span, tol_iv, details=True)
    xyz, merged, src = [], [], []
    for s in range(count):
        v_s = dr.decode_direct(raw[s]).reshape(-1)
        valid = np.isfinite(v_s)
        lower = np.zeros(H * W, bool)
        for t in range(max(0, s - span), s):
            lower |= per_pair[(s, t)][0] == CONSISTENT
        sup = support[s].reshape(-1); con = conflict[s].reshape(-1)
        emit = np.nonzero(valid & (sup >= min_support) & (con <= max_conflict) & ~lower)[0]
        if len(emit) == 0:
            continue
        p_own = to_world(fts[s], dr.back_project_cam(emit % W, emit // W, v_s[emit], cam, config, spx))
        w = depth_weight(v_s[emit], cam)
        acc = w[:, None] * p_own
        wsum = w.copy()
        for t in range(s + 1, min(count, s + span + 1)):         # ascending t; lower targets are never consistent here
            cls, _, tpix, v_obs = per_pair[(s, t)]
            sel = cls[emit] == CONSISTENT
            k = emit[sel]
            if len(k) == 0:
                continue
            p_t = to_world(fts[t], dr.back_project_cam(tpix[k] % W, tpix[k] // W, v_obs[k], cam, config, spx))
            wt = depth_weight(v_obs[k], cam)
            acc[sel] = acc[sel] + wt[:, None] * p_t
            wsum[sel] = wsum[sel] + wt
        xyz.append(acc / wsum[:, None]); merged.append(1 + sup[emit].astype(np.int64)); src.append(s * H * W + emit)
    if not xyz:
        return np.zeros((0, 3)), np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    return np.concatenate(xyz), np.concatenate(merged).astype(np.uint8), np.concatenate(src).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ the fixture
W_FIX, H_FIX, N_FIX = 83, 61, 5
CONFIG_FIX = 0x6
SPX_FIX = 0.011
TOL_STEPS_FIX = 4.0


def fixture_camera(B_scale=1.0):
    cam = dr.CAM_ROUND_TRIP.copy()
    cam[3], cam[4] = 40.7, 29.6                                  # the principal point inside the 83 x 61 map
    cam[2] *= B_scale
    return cam


def fixture_views():
    """Map m looks at the scene from a pose a few hundredths of a radian and a few millimetres further on: the rotation about y
    sweeps the view over the scene, the translation takes most of that sweep back, and a little roll, tilt and depth change ride
    along so that no transform is axis-aligned."""
    m = np.arange(N_FIX, dtype=np.float64)
    return np.column_stack([0.004 * m, 0.02 * m, -0.006 * m, -8.4 * m, 0.7 * m, 1.5 * m])


def scene_surface(x, y):
    """world depth of the scene along z: a tilted back plane with a small box in front of it"""
    plane = 520.0 + 0.35 * x - 0.25 * y
    box = (x > -1.0) & (x < 3.2) & (y > -1.6) & (y < 1.9)
    return np.where(box, 480.0, plane)


def render_maps(cam, views, W, H, spy=None):
    """One map per pose.  Every pixel is rendered by bisection on v until the back-projected world point lies on the surface
    (60 halvings: to the last bit), then encoded with dr.encode_vdepth.  A ray that crosses the box's edge finds the side wall."""
    rows, cols = np.mgrid[0:H, 0:W]
    cols = cols.reshape(-1).astype(np.float64); rows = rows.reshape(-1).astype(np.float64)
    raw = np.zeros((len(views), H, W), np.uint16)
    for m in range(len(views)):
        ft = frame_table(views[m])

        def gap(v):
            p_w = to_world(ft, dr.back_project_cam(cols, rows, v, cam, CONFIG_FIX, SPX_FIX, spy=spy))
            return p_w[:, 2] - scene_surface(p_w[:, 0], p_w[:, 1])
        lo = np.full(len(cols), 2.0); hi = np.full(len(cols), 20.0)   # Z falls as v rises: gap(lo) > 0 > gap(hi)
        assert np.all(gap(lo) > 0) and np.all(gap(hi) < 0)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            behind = gap(mid) > 0
            lo = np.where(behind, mid, lo); hi = np.where(behind, hi, mid)
        raw[m] = dr.encode_vdepth(0.5 * (lo + hi)).reshape(H, W)
    return raw


@functools.lru_cache(maxsize=None)
def views_fixture():
    """(raw (5, 61, 83) uint16, cam, views (5, 6)): the scene rendered from the five poses.  A few pixels are blanked so that
    invalid sources and invalid targets occur."""
    cam = fixture_camera()
    views = fixture_views()
    raw = render_maps(cam, views, W_FIX, H_FIX)
    for m in range(N_FIX):
        raw[m, 5 + m:8 + m, 10:14] = 0                           # never measured
        raw[m, 50, 70 - m] = 65535                               # iv = 0
    raw.setflags(write=False); cam.setflags(write=False); views.setflags(write=False)
    return raw, cam, views


@functools.lru_cache(maxsize=None)
def small_fixture():
    """three maps of 4 x 3 (one workgroup, most of it idle) looking at the box's edge: (raw, cam, views)"""
    cam = fixture_camera()
    cam[3], cam[4] = 1.6, 1.1
    views = 0.05 * fixture_views()[:3]
    views[:, 3] += 0.95                                          # the box's left edge (x = -1) into the middle column
    raw = render_maps(cam, views, 4, 3)
    raw.setflags(write=False); cam.setflags(write=False); views.setflags(write=False)
    return raw, cam, views


@functools.lru_cache(maxsize=None)
def fixture_check(span):
    """check_ref of the fixture at its tolerance, computed once per span and shared by the tests"""
    raw, cam, views = views_fixture()
    return check_ref(raw, cam, CONFIG_FIX, SPX_FIX, np.arange(N_FIX), views, span, TOL_STEPS_FIX * STEP, details=True)


def rms_steps(pair):
    """RMS of e over the consistent pixels of every pair slot in raw steps, NaN where there are none"""
    n = pair["n_consistent"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(pair["sum_e2"] / n) / STEP
