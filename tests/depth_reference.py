"""Restatements of the reference's virtual-depth code that the depth tests compare the GPU paths with.

    sample_ref          CameraCalibration::readDepthData, the per-point part (src/CameraCalibration.cpp:385-448), in Python loops
    back_project_ref    CameraModel::projectPointBack (src/CameraModel.h:26-81) with radialDistortion / tangentialDistortion
                        (:205-241), line by line in plain arithmetic: it runs on float64, float32 and complex128 arrays alike
    forward_ref         the closed-form inverse of back_project_ref: camera coordinates -> (x_v, y_v, virtual depth)
Every operation is an IEEE operation of the array's type in the reference's order; numpy does not contract a * b + c.
"""
from __future__ import annotations

import struct
import zlib

import numpy as np


# The camera of the round-trip checks.  Metric depth is Z = fL b / (b - fL) with b = bL0 + v B, so a rounding error of b (a few
# eps b: b is itself recovered from Z through v) reaches Z amplified by fL / (b - fL).  The project's default camera (fL 35,
# bL0 34.15, B 0.4) has b = fL at v = 2.125: inside the range v in [2, 20] the round trip is asked for, Z has a pole there, and no
# arithmetic meets a relative bar around it.  With bL0 = 35.5 the amplification is at most 35 / 1.3 = 27 over the whole range
# (27 x 3 eps = 9e-15, a tenth of the 1e-13 bar), so the bar measures the undistortion and not the pole.  Distortion: the project's default.
CAM_ROUND_TRIP = np.array([35.0, 35.5, 0.40, 511.3, 513.9, 5e-5, -2e-7, 1e-5, -1e-5] + [0.0] * 8)


def camera_parts(cam, config):
    """(fL, bL0, B, cx, cy, radial list, tangential pair or None) of cam[17] as storeResults hands them over (:1107-1116)"""
    nr = config & 3
    radial = [cam[5 + i] for i in range(nr)]
    tangential = (cam[5 + nr], cam[6 + nr]) if config & 4 else None
    return cam[0], cam[1], cam[2], cam[3], cam[4], radial, tangential


def _inverse_depth_table():
    """iv = 1 - value / 65535 for the valid raw values (value > 0, 0 < iv <= 0.5), None otherwise (:391-396)"""
    tab = [None] * 65536
    for value in range(1, 65536):
        iv = float(value) / 65535.0
        iv = 1.0 - iv
        if iv <= 0.5 and iv > 0.0:
            tab[value] = iv
    return tab


def sample_ref(image, x, y):
    """readDepthData for one decoded image (H, W) uint16 and image points (x, y).  Returns (vdepth, dist): dist[i] = 0 for a
    direct value, the window half-width that succeeded for an interpolated one, -1 where the interpolation failed (vdepth = -1).
    A centre pixel outside the image (where the reference reads out of bounds) gives -1 / dist -2."""
    H, W = image.shape
    tab = _inverse_depth_table()
    cols = [[int(v) for v in image[:, c]] for c in range(W)]   # cols[x][y]
    out = np.zeros(len(x)); used = np.zeros(len(x), np.int64)
    for i in range(len(x)):
        cx = int(float(x[i]) + 0.5); cy = int(float(y[i]) + 0.5)   # C truncation
        if cx < 0 or cx >= W or cy < 0 or cy >= H:
            out[i] = -1.0; used[i] = -2
            continue
        iv = tab[cols[cx][cy]]
        if iv is not None:
            out[i] = 1.0 / iv
            continue
        out[i] = -1.0; used[i] = -1
        for dist in range(1, 50):
            num = 0
            total = 0.0
            y0 = max(cy - dist, 0); y1 = min(cy + dist, H - 1)
            for xx in range(max(cx - dist, 0), min(cx + dist, W - 1) + 1):   # `if(x<0) x=0` / `break` of the reference: the clipped window
                for value in cols[xx][y0:y1 + 1]:
                    if value:
                        iv = tab[value]
                        if iv is not None:
                            num += 1
                            total += iv
            if num >= 10:
                out[i] = float(num) / total; used[i] = dist
                break
    return out, used


def back_project_ref(x_v, y_v, v_depth, spx, spy, fL, bL0, B, cx, cy, radial, tangential, sweeps=10):
    """projectPointBack; radial: list of 0..2 coefficients, tangential: pair or None.  Returns (X, Y, Z)."""
    one = x_v * 0 + 1          # carries the array type (float32 / float64 / complex128) into the constants
    two = one + one
    projected_x = (x_v - cx) * spx
    projected_y = (y_v - cy) * spy
    projected_z = v_depth * B
    projected_x = (projected_x / (bL0 + projected_z)) * bL0
    projected_y = (projected_y / (bL0 + projected_z)) * bL0
    n_radial = len(radial)
    if n_radial > 0 or tangential is not None:
        projected_x_dist = projected_x
        projected_y_dist = projected_y
        delta_rad_x = one * 0; delta_rad_y = one * 0; delta_tan_x = one * 0; delta_tan_y = one * 0
        for _ in range(sweeps):
            if n_radial > 0:       # radialDistortion (:205-223)
                r0 = projected_x * projected_x + projected_y * projected_y
                delta_r = radial[0] * r0
                r_prev = r0
                for i in range(1, n_radial):
                    r_i = r_prev * r0
                    delta_r = delta_r + radial[i] * r_i
                    r_prev = r_i
                delta_rad_x = projected_x * delta_r
                delta_rad_y = projected_y * delta_r
            if tangential is not None:   # tangentialDistortion (:228-241)
                r_2 = projected_x * projected_x + projected_y * projected_y
                delta_tan_x = tangential[0] * (r_2 + two * projected_x * projected_x) + two * tangential[1] * projected_x * projected_y
                delta_tan_y = tangential[1] * (r_2 + two * projected_y * projected_y) + two * tangential[0] * projected_x * projected_y
            projected_x = projected_x_dist - delta_rad_x - delta_tan_x
            projected_y = projected_y_dist - delta_rad_y - delta_tan_y
    projected_z = projected_z + bL0
    Z = fL * projected_z / (projected_z - fL)
    X = projected_x / bL0 * Z
    Y = projected_y / bL0 * Z
    return X, Y, Z


def back_project_cam(x_v, y_v, v_depth, cam, config, spx, spy=None, sweeps=10, dtype=np.float64):
    """back_project_ref on cam[17] / config, everything cast to dtype first; returns an (n, 3) array"""
    dt = np.dtype(dtype).type
    cam = np.asarray(cam).astype(dtype)
    fL, bL0, B, cx, cy, radial, tangential = camera_parts(cam, config)
    X, Y, Z = back_project_ref(np.asarray(x_v).astype(dtype), np.asarray(y_v).astype(dtype), np.asarray(v_depth).astype(dtype), dt(spx),
                               dt(spx if spy is None else spy), fL, bL0, B, cx, cy, radial, tangential, sweeps)
    return np.stack([X, Y, Z], -1)


def forward_ref(p_c, cam, config, spx, spy=None):
    """camera coordinates (n, 3) -> (x_v, y_v, v): the model projectPointBack inverts, in closed form"""
    fL, bL0, B, cx, cy, radial, tangential = camera_parts(np.asarray(cam, np.float64), config)
    spy = spx if spy is None else spy
    X, Y, Z = p_c[:, 0], p_c[:, 1], p_c[:, 2]
    x_u = X / Z * bL0
    y_u = Y / Z * bL0
    r2 = x_u * x_u + y_u * y_u
    delta_r = 0.0
    for i, k in enumerate(radial):
        delta_r = delta_r + k * r2 ** (i + 1)
    dx = x_u * delta_r; dy = y_u * delta_r
    if tangential is not None:
        dx = dx + tangential[0] * (r2 + 2 * x_u * x_u) + 2 * tangential[1] * x_u * y_u
        dy = dy + tangential[1] * (r2 + 2 * y_u * y_u) + 2 * tangential[0] * x_u * y_u
    x_d = x_u + dx; y_d = y_u + dy
    v = (fL * Z / (Z - fL) - bL0) / B
    x_v = x_d * (bL0 + v * B) / bL0 / spx + cx
    y_v = y_d * (bL0 + v * B) / bL0 / spy + cy
    return x_v, y_v, v


def jacobian_complex_step(x_v, y_v, v_depth, cam, config, spx, spy=None, h=1e-30):
    """d p_c / d cam (n, 3, 17) and d p_c / d v (n, 3) by the complex step: exact to rounding, the function is rational"""
    n = len(x_v)
    J = np.zeros((n, 3, 17)); dv = np.zeros((n, 3))
    for s in range(18):
        c = np.asarray(cam, np.complex128).copy()
        vd = np.asarray(v_depth, np.complex128).copy()
        if s < 17:
            c[s] += 1j * h
        else:
            vd = vd + 1j * h
        p = back_project_cam(x_v, y_v, vd, c, config, spx, spy, dtype=np.complex128)
        if s < 17:
            J[:, :, s] = p.imag / h
        else:
            dv = p.imag / h
    return J, dv


def euler_xyz(a):
    """R = Rx(a0) Ry(a1) Rz(a2) (RigidBody::getTransformationMatrix, src/CameraModel.h:246-264)"""
    c0, s0, c1, s1, c2, s2 = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    return np.array([[c1 * c2, -c1 * s2, s1],
                     [c0 * s2 + s0 * s1 * c2, c0 * c2 - s0 * s1 * s2, -s0 * c1],
                     [s0 * s2 - c0 * s1 * c2, s0 * c2 + c0 * s1 * s2, c0 * c1]])


def encode_vdepth(v):
    """the raw 16-bit value of a virtual depth: rint((1 - 1/v) 65535)"""
    return np.rint((1.0 - 1.0 / np.asarray(v, np.float64)) * 65535.0).astype(np.uint16)


def decode_direct(raw):
    """vdepth of raw values by the direct rule, NaN where invalid (float64, the reference's operations)"""
    value = raw.astype(np.float64)
    iv = value / 65535.0
    iv = 1.0 - iv
    ok = (raw > 0) & (iv <= 0.5) & (iv > 0.0)
    out = np.full(raw.shape, np.nan)
    out[ok] = 1.0 / iv[ok]
    return out


def sampler_fixture(seed=20241022, W=256, H=192, n_points=4000):
    """The map and the points of the sampler test: a smooth surface in 2.3 .. 3.2 with a band near 9, 30 % of the pixels zeroed at
    random, the left 110 columns zero, a 25 x 25 hole, a 4 x 4 patch of 65535 (iv = 0) and one of 20000 (v < 2); 4000 points, 50
    of them in the hole and some up to 0.49 px outside the border."""
    rs = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    v = 2.75 + 0.45 * np.sin(xx / 37.0) * np.cos(yy / 29.0)
    v[60:70, :] = 9.0 + 0.2 * np.sin(xx[60:70, :] / 11.0)
    img = encode_vdepth(v)
    img[rs.random((H, W)) < 0.30] = 0
    img[:, :110] = 0
    img[100:125, 180:205] = 0
    img[20:24, 150:154] = 65535
    img[30:34, 160:164] = 20000
    x = rs.uniform(-0.49, W - 0.51, n_points); y = rs.uniform(-0.49, H - 0.51, n_points)
    x[:50] = rs.uniform(181.0, 203.0, 50); y[:50] = rs.uniform(101.0, 123.0, 50)             # inside the hole
    x[50:60] = -0.49; x[60:70] = W - 0.51; y[70:80] = -0.49; y[80:90] = H - 0.51              # just outside the border
    x[90:110] = rs.uniform(150.0, 153.0, 20); y[90:110] = rs.uniform(20.0, 23.0, 20)         # the 65535 patch
    x[110:130] = rs.uniform(160.0, 163.0, 20); y[110:130] = rs.uniform(30.0, 33.0, 20)       # the 20000 patch
    return img, x, y


# ---- a PNG writer for the tests (the product only reads) ----
def _chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xFFFFFFFF)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)


def write_png16(path, img, filters=(0,), bit_depth=16, color_type=0, interlace=0):
    """a 16-bit grayscale PNG with the given per-line filter types (cycled), written with zlib and struct alone"""
    H, W = img.shape
    rows = img.astype(">u2").view(np.uint8).reshape(H, 2 * W).astype(np.int64)
    raw = bytearray()
    prev = np.zeros(2 * W, np.int64)
    for r in range(H):
        ft = filters[r % len(filters)]
        cur = rows[r]
        left = np.concatenate([[0, 0], cur[:-2]]); upleft = np.concatenate([[0, 0], prev[:-2]])
        if ft == 0:
            enc = cur
        elif ft == 1:
            enc = cur - left
        elif ft == 2:
            enc = cur - prev
        elif ft == 3:
            enc = cur - ((left + prev) >> 1)
        else:
            enc = cur - np.array([_paeth(int(a), int(b), int(c)) for a, b, c in zip(left, prev, upleft)])
        raw.append(ft); raw += bytes((enc & 0xFF).astype(np.uint8))
        prev = cur
    data = zlib.compress(bytes(raw))
    half = len(data) // 2   # two IDAT chunks: the stream may be split anywhere
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, bit_depth, color_type, 0, 0, interlace)) +
                _chunk(b"tEXt", b"Comment\x00depth") + _chunk(b"IDAT", data[:half]) + _chunk(b"IDAT", data[half:]) + _chunk(b"IEND", b""))
