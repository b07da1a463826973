"""Times lifcal_features_detect and lifcal_features_match (include/lifcal_features.h).

Detection: the 2048 x 2048 total-focus image of section 7v's workload (a raw image of 11 k lenses at d = 21 px over a smooth depth
field, rendered to the virtual image with the true depth), with its status map, 8 and 16 bit, host pointers.  Matching: a sequence
of `frames` frames of 2048 x 2048 that show one texture through a growing rotation, scale and shift (sampled directly, 8 bit),
every frame against the next `window`.  Per row the feature or match counts, the kernel time (HIP events: detect + describe, or
match) and the host clock around whole calls, median / min / max of `reps` calls after one warm-up call.  Prints one JSON line.
Run under rocprofv3 --kernel-trace --stats for the per-kernel times.

usage: features_timing.py [reps] [--size N] [--frames F] [--window W]"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

args = sys.argv[1:]
opt = {}
for flag in ("--size", "--frames", "--window"):
    if flag in args:
        i = args.index(flag)
        opt[flag] = args[i + 1]
        del args[i:i + 2]
reps = int(args[0]) if args else 7
W = H = int(opt.get("--size", 2048))
F, WINDOW = int(opt.get("--frames", 20)), int(opt.get("--window", 2))
D, ROT, OFF, BASE_Y = 21.0, 0.002, (0.3, -0.6), (-0.5, 0.8660254)
depth_fn = lambda x, y: 4.0 + 2.0 * np.sin(np.asarray(x) / 300.0) * np.cos(np.asarray(y) / 400.0)

from lifcal_amd import MicroLensGrid, detectFeatures, linkTracks, matchFeatures, raw_image, totalFocusImage, white_image

texture = raw_image.band_limited_texture(7, 18.0, 60.0)
tx, ty = white_image.grid_centres(W, H, D, BASE_Y, ROT, OFF, 1.5)
raw8 = raw_image.render_raw_image(W, H, tx, ty, D, depth_fn, texture, bits=8, noise=0.004, seed=11, supersample=1)
g = MicroLensGrid(W, H, D, BASE_Y, ROT, OFF)
Y, X = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
iv = (1.0 / depth_fn(X, Y)).astype(np.float32)
out = {"width": W, "height": H, "reps": reps, "frames": F, "window": WINDOW, "detect": [], "match": {}}


def stats(prefix, values):
    return {f"{prefix}_median": float(np.median(values)), f"{prefix}_min": float(np.min(values)), f"{prefix}_max": float(np.max(values))}


for bits, raw in ((8, raw8), (16, raw8.astype(np.uint16) * 257)):
    tf = totalFocusImage(g, raw, iv)
    for with_status in (True, False):
        ks, ts = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            f = detectFeatures(tf.image, tf.status if with_status else None)
            if r:
                ts.append((time.perf_counter() - t0) * 1e3); ks.append(f.seconds * 1e3)
        row = {"bits": bits, "status": with_status, "n_features": f.n, "invalid_pixels": int((tf.status != 0).sum())}
        row.update(stats("kernel_ms", ks)); row.update(stats("call_ms", ts))
        out["detect"].append(row)

# the sequence: frame k shows the texture rotated by 0.3 k degrees, scaled by 1 + 0.004 k and shifted by (6.5 k, -3.7 k)
feats = []
for k in range(F):
    ang, sc = math.radians(0.3 * k), 1.0 + 0.004 * k
    c, s = sc * math.cos(ang), sc * math.sin(ang)
    xx, yy = X - (W - 1) / 2.0, Y - (H - 1) / 2.0
    v = 0.9 * texture(c * xx - s * yy + (W - 1) / 2.0 + 6.5 * k, s * xx + c * yy + (H - 1) / 2.0 - 3.7 * k) * 255.0
    feats.append(detectFeatures(np.clip(np.floor(v + 0.5), 0.0, 255.0).astype(np.uint8)))
for max_shift in (0, 200):
    ks, ts = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        m = matchFeatures(feats, window=WINDOW, max_shift=max_shift)
        if r:
            ts.append((time.perf_counter() - t0) * 1e3); ks.append(m.seconds * 1e3)
    tr = linkTracks(feats, m)
    row = {"n_pairs": int(len(m.pairs)), "features_per_frame": [f.n for f in feats][:4], "n_matches": int(len(m.i)), "n_tracks": tr.n_tracks,
           "n_conflicts": tr.n_conflicts}
    row.update(stats("kernel_ms", ks)); row.update(stats("call_ms", ts))
    out["match"][f"max_shift_{max_shift}"] = row
print(json.dumps(out))
