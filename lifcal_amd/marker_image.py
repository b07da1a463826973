"""Synthetic marker images: a set of square binary markers (include/lifcal_markers.h) seen through projective maps, as an
image (supersampled, blurred, shaded, with noise) or as a texture function on the virtual image for
raw_image.render_raw_image, so that markers can go through the raw-image chain.  In the manner of white_image.py: tests and tools
use it to make inputs whose truth (the centre and the corners of every marker) is known."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Sequence

import numpy as np


@dataclass
class PlacedMarker:
    """One marker in the image.  bits: (m, m) of 0 / 1 (1 = white), the marker's own orientation; H: 3 x 3, maps the marker's
    unit square (u to the right, v down, the black border included) onto the image, (x, y, 1) ~ H (u, v, 1)."""
    id: int
    bits: np.ndarray
    H: np.ndarray

    def image_of(self, u, v):
        p = self.H @ np.array([u, v, 1.0])
        return p[0] / p[2], p[1] / p[2]

    @property
    def centre(self):
        """the image of the square's centre: the intersection of the diagonals of the projected square"""
        return self.image_of(0.5, 0.5)

    @property
    def corners(self) -> np.ndarray:
        """(4, 2): own top-left, top-right, bottom-right, bottom-left (clockwise with y down)"""
        return np.array([self.image_of(u, v) for u, v in ((0, 0), (1, 0), (1, 1), (0, 1))])


def marker_homography(cx: float, cy: float, side: float, angle_deg: float = 0.0, perspective: float = 0.0, tilt_deg: float = 0.0) -> np.ndarray:
    """Unit square -> image: a square of `side` pixels about (cx, cy), rotated by angle_deg (clockwise on the screen, y down), then
    seen under a perspective that scales the image by 1 -/+ perspective at half a side from the centre along the direction
    tilt_deg."""
    a, t = np.deg2rad(angle_deg), np.deg2rad(tilt_deg)
    S = np.array([[side, 0, -0.5 * side], [0, side, -0.5 * side], [0, 0, 1.0]])
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    k = perspective / (0.5 * side)
    P = np.array([[1, 0, 0], [0, 1, 0], [k * np.cos(t), k * np.sin(t), 1.0]])
    T = np.array([[1, 0, cx], [0, 1, cy], [0, 0, 1.0]])
    return T @ P @ R @ S


def place(id: int, bits, cx, cy, side, angle_deg=0.0, perspective=0.0, tilt_deg=0.0) -> PlacedMarker:
    return PlacedMarker(int(id), np.asarray(bits, np.uint8), marker_homography(cx, cy, side, angle_deg, perspective, tilt_deg))


def marker_texture(markers: Sequence[PlacedMarker], background: float = 1.0) -> Callable:
    """texture(x, y) in [0, 1]: `background` outside every marker, 0 on black cells (the border among them), 1 on white cells.
    x, y: arrays of image (or virtual-image) coordinates, pixel centres at integers."""
    inv = [np.linalg.inv(m.H) for m in markers]

    def texture(x, y):
        x = np.asarray(x, np.float64); y = np.asarray(y, np.float64)
        out = np.full(np.broadcast(x, y).shape, float(background))
        for m, G in zip(markers, inv):
            n = m.bits.shape[0] + 2
            cells = np.zeros((n, n))
            cells[1:-1, 1:-1] = m.bits
            w = G[2, 0] * x + G[2, 1] * y + G[2, 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                u = (G[0, 0] * x + G[0, 1] * y + G[0, 2]) / w
                v = (G[1, 0] * x + G[1, 1] * y + G[1, 2]) / w
            inside = (w > 0) & (u >= 0) & (u < 1) & (v >= 0) & (v < 1)
            c = np.clip(np.floor(np.where(inside, u, 0.0) * n).astype(np.int64), 0, n - 1)
            r = np.clip(np.floor(np.where(inside, v, 0.0) * n).astype(np.int64), 0, n - 1)
            out = np.where(inside, cells[r, c], out)
        return out
    return texture


def _blur(a: np.ndarray, sigma: float) -> np.ndarray:
    if sigma <= 0:
        return a
    r = int(np.ceil(4 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    p = np.pad(a, r, mode="edge")
    p = sum(k[i] * p[:, i:i + a.shape[1]] for i in range(2 * r + 1))
    return sum(k[i] * p[i:i + a.shape[0], :] for i in range(2 * r + 1))


def render_markers(shape, markers: Sequence[PlacedMarker], *, bits: int = 8, supersample: int = 4, blur: float = 0.0, noise: float = 0.0,
                   shading: float = 0.0, white: float = 0.85, black: float = 0.12, seed: int = 0, texture: Callable = None) -> np.ndarray:
    """(H, W) uint8 / uint16.  Every pixel is the mean of supersample^2 samples of the texture over its square; then a Gaussian blur of
    sigma `blur` pixels, a linear shading that runs from 1 - shading to 1 across the image diagonal, `white` / `black` as
    fractions of full scale, and Gaussian noise of sigma `noise` grey levels of an 8-bit image (scaled for 16 bit)."""
    h, w = shape
    T = marker_texture(markers) if texture is None else texture
    s = int(supersample)
    off = (np.arange(s) + 0.5) / s - 0.5
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    acc = np.zeros((h, w))
    for oy in off:
        for ox in off:
            acc += T(xx + ox, yy + oy)
    img = black + (white - black) * _blur(acc / (s * s), blur)
    img *= 1.0 - shading * (1.0 - (xx / max(w - 1, 1) + yy / max(h - 1, 1)) / 2.0)
    full = float((1 << bits) - 1)
    img = img * full
    if noise > 0:
        img = img + np.random.default_rng(seed).normal(0.0, noise * (full / 255.0), img.shape)
    return np.clip(np.floor(img + 0.5), 0, full).astype(np.uint8 if bits == 8 else np.uint16)
