"""Synthetic white images: a numpy renderer of what a plenoptic sensor records of a diffuse white surface, one bright disc per
micro lens.  Tests and tools use it to make inputs with a known grid for lifcal_amd.grid_fit.

A disc is rendered with a radial fall-off, 1 - falloff (rho / R)^2 inside R = fill * diameter / 2 and zero outside, sampled at
3 x 3 points per pixel.  Options: global vignetting, Gaussian noise, 8- or 16-bit quantisation, saturation (a gain above what
the number format holds), hot pixels, blocked lenses and a dust spot.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np


def grid_centres(width: int, height: int, lens_diameter: float, lens_base_y: Sequence[float] = (-0.5, 0.8660254), rotation: float = 0.0,
                 offset: Sequence[float] = (0.0, 0.0), margin: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
    """Centres (double) of the grid lifcal_mla_create builds from these parameters (MicroLensGrid::createGrid), for every lens
    within `margin` diameters of the image: centre(k, x, y) = offset_cv + R(rotation) g, image y pointing down."""
    d, (bx, by) = float(lens_diameter), (float(lens_base_y[0]), float(lens_base_y[1]))
    ox, oy = offset[0] + width / 2.0 - 0.5, -offset[1] + height / 2.0 - 0.5
    n = int(np.ceil(np.hypot(width, height) / (d * min(1.0, 2.0 * by)))) + 3
    x, y = np.meshgrid(np.arange(-n, n + 1, dtype=np.float64), np.arange(-n, n + 1, dtype=np.float64), indexing="ij")
    gx = np.concatenate([(x * d).ravel(), ((x + 1.0 + bx) * d).ravel()])
    gy = np.concatenate([(2.0 * y * by * d).ravel(), ((2.0 * y + 1.0) * by * d).ravel()])
    c, s = np.cos(rotation), np.sin(rotation)
    cx, cy = ox + (gx * c - gy * s), oy - (gx * s + gy * c)
    keep = (cx > -margin * d) & (cx < width - 1 + margin * d) & (cy > -margin * d) & (cy < height - 1 + margin * d)
    return cx[keep], cy[keep]


def render_white_image(width: int, height: int, cx, cy, lens_diameter: float, *, bits: int = 8, fill: float = 0.94, falloff: float = 0.7,
                       level: float = 0.8, gain: float = 1.0, vignetting: float = 1.0, noise: float = 0.0, seed: int = 0,
                       hot_pixels: Sequence[Tuple[int, int]] = (), blocked: Sequence[int] = (),
                       dust: Optional[Tuple[float, float, float, float]] = None, supersample: int = 3) -> np.ndarray:
    """The white image of lenses at (cx[i], cy[i]) as uint8 (bits = 8) or uint16 (bits = 16).

    level: disc centre as a fraction of full scale before `gain` (gain * level > 1 saturates the disc centres);
    vignetting: brightness of the image corners relative to its centre (quadratic in the distance from the centre);
    noise: sigma of additive Gaussian noise as a fraction of full scale;  hot_pixels: (x, y) set to full scale;
    blocked: indices into cx / cy of lenses that stay dark;  dust: (x, y, radius, transmission) of a round absorbing spot."""
    assert bits in (8, 16)
    cx = np.asarray(cx, np.float64); cy = np.asarray(cy, np.float64)
    img = np.zeros((height, width), np.float64)
    R = 0.5 * fill * float(lens_diameter)
    ss = int(supersample)
    sub = (np.arange(ss, dtype=np.float64) + 0.5) / ss - 0.5
    skip = set(int(b) for b in blocked)
    for i in range(len(cx)):
        if i in skip:
            continue
        x0, x1 = max(0, int(np.floor(cx[i] - R - 1))), min(width - 1, int(np.ceil(cx[i] + R + 1)))
        y0, y1 = max(0, int(np.floor(cy[i] - R - 1))), min(height - 1, int(np.ceil(cy[i] + R + 1)))
        if x1 < x0 or y1 < y0:
            continue
        xs = (np.arange(x0, x1 + 1, dtype=np.float64)[:, None] + sub[None, :]).ravel() - cx[i]
        ys = (np.arange(y0, y1 + 1, dtype=np.float64)[:, None] + sub[None, :]).ravel() - cy[i]
        q = (ys[:, None] ** 2 + xs[None, :] ** 2) / (R * R)
        v = np.where(q <= 1.0, 1.0 - falloff * q, 0.0)
        v = v.reshape(y1 - y0 + 1, ss, x1 - x0 + 1, ss).mean(axis=(1, 3))
        img[y0:y1 + 1, x0:x1 + 1] = np.maximum(img[y0:y1 + 1, x0:x1 + 1], v)
    yy, xx = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), indexing="ij")
    if vignetting != 1.0:
        mx, my = (width - 1) / 2.0, (height - 1) / 2.0
        img *= 1.0 - (1.0 - vignetting) * ((xx - mx) ** 2 + (yy - my) ** 2) / (mx * mx + my * my)
    if dust is not None:
        dx, dy, dr, dt = dust
        img *= np.where((xx - dx) ** 2 + (yy - dy) ** 2 <= dr * dr, dt, 1.0)
    img *= level * gain
    if noise > 0.0:
        img += np.random.default_rng(seed).normal(0.0, noise, img.shape)
    full = float((1 << bits) - 1)
    out = np.clip(np.floor(img * full + 0.5), 0.0, full)
    for (hx, hy) in hot_pixels:
        out[int(hy), int(hx)] = full
    return out.astype(np.uint8 if bits == 8 else np.uint16)
