"""Synthetic raw images of a focused plenoptic camera: a numpy renderer of what the sensor records behind the micro-lens array
of a scene given as a texture on the virtual image with a virtual depth per virtual-image point.  Tests and tools use it to make
inputs with known depth for lifcal_amd.raw_depth, as white_image.py does for the grid fit.

The geometry is the inverse of lifcal_mla_project's: the pixel p of the micro image with centre c shows the virtual-image point
x_v = c + v (p - c), where v is the virtual depth AT x_v.  v is found per sample by the fixed-point iteration
v <- depth_fn(c + v (p - c)); it converges in one step on a fronto-parallel plane and in a few wherever |p - c| |grad v| < 1.
"""
from __future__ import annotations

from typing import Callable

import numpy as np


def band_limited_texture(seed: int, lambda_min: float, lambda_max: float, n_waves: int = 48) -> Callable:
    """T(x, y) in [0, 1]: a sum of n_waves sinusoids with wavelengths drawn log-uniformly from [lambda_min, lambda_max]
    (virtual-image pixels), uniform directions and phases.  A micro image at virtual depth v shows it demagnified by v, so the
    wavelengths must be at least 2.5 v for the raw image to sample it (asserted by nobody: the caller chooses the band)."""
    rng = np.random.default_rng(seed)
    lam = np.exp(rng.uniform(np.log(lambda_min), np.log(lambda_max), n_waves))
    ang = rng.uniform(0.0, 2.0 * np.pi, n_waves)
    ph = rng.uniform(0.0, 2.0 * np.pi, n_waves)
    kx, ky = 2.0 * np.pi / lam * np.cos(ang), 2.0 * np.pi / lam * np.sin(ang)
    norm = 1.0 / (2.5 * np.sqrt(n_waves / 2.0))   # 2.5 sigma of the sum fills the half range

    def texture(x, y):
        x = np.asarray(x, np.float64); y = np.asarray(y, np.float64)
        s = np.zeros(np.broadcast(x, y).shape)
        for i in range(n_waves):
            s += np.sin(kx[i] * x + ky[i] * y + ph[i])
        return np.clip(0.5 + 0.5 * norm * s, 0.0, 1.0)

    return texture


def plane_depth(v: float) -> Callable:
    return lambda x, y: np.full(np.broadcast(x, y).shape, float(v))


def step_depth(v_left: float, v_right: float, x_step: float) -> Callable:
    return lambda x, y: np.where(np.asarray(x) + 0.0 * np.asarray(y) < x_step, float(v_left), float(v_right))


def virtual_depth_at(px, py, cx, cy, depth_fn: Callable, iterations: int = 12):
    """The virtual depth seen by raw positions (px, py) of the micro image centred at (cx, cy)."""
    ox, oy = np.asarray(px, np.float64) - cx, np.asarray(py, np.float64) - cy
    v = depth_fn(cx + 0.0 * ox, cy + 0.0 * oy)
    for _ in range(iterations):
        v = depth_fn(cx + v * ox, cy + v * oy)
    return v


def render_raw_image(width: int, height: int, cx, cy, lens_diameter: float, depth_fn: Callable, texture_fn: Callable, *, fill: float = 0.98,
                     bits: int = 8, noise: float = 0.0, seed: int = 0, level: float = 0.9, supersample: int = 3) -> np.ndarray:
    """The raw image of lenses at (cx[i], cy[i]) as uint8 (bits = 8) or uint16 (bits = 16): raw(p) = T(c + v (p - c)) inside the
    disc of radius fill * lens_diameter / 2 of each lens, zero between the discs, averaged over supersample^2 points per pixel.

    level: texture value 1 as a fraction of full scale;  noise: sigma of additive Gaussian noise as a fraction of full scale."""
    assert bits in (8, 16)
    cx = np.asarray(cx, np.float64); cy = np.asarray(cy, np.float64)
    img = np.zeros((height, width), np.float64)
    R = 0.5 * fill * float(lens_diameter)
    ss = int(supersample)
    sub = (np.arange(ss, dtype=np.float64) + 0.5) / ss - 0.5
    for i in range(len(cx)):
        x0, x1 = max(0, int(np.floor(cx[i] - R - 1))), min(width - 1, int(np.ceil(cx[i] + R + 1)))
        y0, y1 = max(0, int(np.floor(cy[i] - R - 1))), min(height - 1, int(np.ceil(cy[i] + R + 1)))
        if x1 < x0 or y1 < y0:
            continue
        xs = (np.arange(x0, x1 + 1, dtype=np.float64)[:, None] + sub[None, :]).ravel()
        ys = (np.arange(y0, y1 + 1, dtype=np.float64)[:, None] + sub[None, :]).ravel()
        X, Y = np.meshgrid(xs, ys)
        inside = (X - cx[i]) ** 2 + (Y - cy[i]) ** 2 <= R * R
        v = virtual_depth_at(X, Y, cx[i], cy[i], depth_fn)
        t = np.where(inside, texture_fn(cx[i] + v * (X - cx[i]), cy[i] + v * (Y - cy[i])), 0.0)
        t = t.reshape(y1 - y0 + 1, ss, x1 - x0 + 1, ss).mean(axis=(1, 3))
        own = inside.reshape(y1 - y0 + 1, ss, x1 - x0 + 1, ss).any(axis=(1, 3))
        img[y0:y1 + 1, x0:x1 + 1] = np.where(own, t, img[y0:y1 + 1, x0:x1 + 1])
    img *= level
    if noise > 0.0:
        img += np.random.default_rng(seed).normal(0.0, noise, img.shape)
    full = float((1 << bits) - 1)
    return np.clip(np.floor(img * full + 0.5), 0.0, full).astype(np.uint8 if bits == 8 else np.uint16)
