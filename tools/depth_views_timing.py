"""Device time of the cross-view check (lifcal_depth_check_maps) and of the fusion (lifcal_depth_fuse_maps).

A batch of 2048 x 2048 depth maps (24 by default: 201 MB of raw values, beyond the 256 MiB Infinity Cache together with the
outputs) of a fronto-parallel plane seen from poses that move a few millimetres and turn a hundredth of a radian about the optical
axis per map, so that nearly every source pixel finds a valid target pixel: the full arithmetic and the full gather load.  Virtual
depth depends on Z alone, so such a map is one raw value per frame; one raw step of noise and 5 % invalid pixels are added.  Per
span the median of the calls' HIP-event time over the repeats is printed, per call and per (source, target) pair, next to
k_depth_dense's time per map (profiles/depth/README.md) as the yardstick.  Per-kernel times of the profiler: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o depth_views -- python tools/depth_views_timing.py
and read the k_depth_views / k_views_fold / k_views_scan / k_depth_fuse rows of the stats file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lifcal_amd import depth  # noqa: E402

CAM = np.array([35.0, 35.5, 0.40, 1023.3, 1021.9, 5e-5, -2e-7, 1e-5, -1e-5] + [0.0] * 8)
SPX = 0.0055
DENSE_MS_PER_MAP = (0.055, 0.063)   # k_depth_dense, fp64, profiles/depth/README.md


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=24)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--config", type=lambda s: int(s, 0), default=0x6)
    ap.add_argument("--spans", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--tol-steps", type=float, default=4.0)
    ap.add_argument("--out", default=None, help="write the rows as JSON to this file")
    args = ap.parse_args()
    W = H = args.size
    n = args.maps
    rs = np.random.default_rng(1)
    m = np.arange(n, dtype=np.float64)
    views = np.column_stack([0 * m, 0 * m, 0.01 * m, 3.0 * m, -2.0 * m, 1.5 * m])
    fL, bL0, B = CAM[0], CAM[1], CAM[2]
    rows = []
    with depth.DepthMaps(W, H, n) as dm:
        for k in range(n):
            Z = 500.0 + views[k, 5]                  # the plane z_w = 500 in the frame of map k
            v = (fL * Z / (Z - fL) - bL0) / B
            raw = np.rint((1.0 - 1.0 / v) * 65535.0) + rs.integers(-1, 2, (H, W))
            raw = raw.astype(np.uint16)
            raw[rs.random((H, W)) < 0.05] = 0
            dm.setMaps(raw, first=k)
        frames = np.arange(n)
        for span in args.spans:
            pairs = sum(1 for s in range(n) for t in range(n) if 0 < abs(t - s) <= span)
            for name in ("checkMaps", "fuseMaps"):
                times = []
                for k in range(args.repeats + 2):   # two warm-up calls
                    if name == "checkMaps":
                        r = dm.checkMaps(CAM, args.config, SPX, frames, views, span=span, tol_steps=args.tol_steps)
                        extra = dict(compared=int(r.pair["n_compared"].sum()), consistent=int(r.pair["n_consistent"].sum()),
                                     rms_steps=float(np.nanmedian(r.rms_steps())))
                    else:
                        cap = None if k == 0 else extra["n_points"]
                        r = dm.fuseMaps(CAM, args.config, SPX, frames, views, span=span, tol_steps=args.tol_steps, capacity=cap)
                        extra = dict(n_points=int(r.n_points))
                    if k >= 2:
                        times.append(r.seconds)
                    del r
                t = float(np.median(times))
                row = dict(call=name, maps=n, size=args.size, span=span, pairs=pairs, ms_per_call=t * 1e3, spread_ms=(max(times) - min(times)) * 1e3,
                           ms_per_pair=t / pairs * 1e3, ms_per_source_map=t / n * 1e3, **extra)
                rows.append(row)
                print(f"{name:9s} span {span}: {row['ms_per_call']:.3f} ms per call (spread {row['spread_ms']:.3f}), {pairs} pairs: {row['ms_per_pair']:.4f} ms per pair, "
                      f"{row['ms_per_source_map']:.4f} ms per source map (k_depth_dense: {DENSE_MS_PER_MAP[0]} to {DENSE_MS_PER_MAP[1]} ms per map)  {extra}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
