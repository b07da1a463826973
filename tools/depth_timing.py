"""Device time of the dense back-projection (lifcal_depth_back_project_maps) and of the sampler (lifcal_depth_sample).

A batch of 2048 x 2048 depth maps large enough to exceed the 256 MiB Infinity Cache (8 maps: 67 MB in, 403 MB of float xyz out) is
back-projected with torch tensors on the device as outputs; per variant the median of the kernel's HIP-event time over the
repeats is printed, with the bytes and the arithmetic operations the algorithm needs per pixel (counted below from the model, not
read from counters) over that time.  Per-kernel times of the profiler: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o depth -- python tools/depth_timing.py
and read the k_depth_dense / k_depth_sample rows of the stats file.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lifcal_amd import depth  # noqa: E402

CAM = np.array([35.0, 34.15, 0.40, 1023.3, 1021.9, 5e-5, -2e-7, 1e-5, -1e-5] + [0.0] * 8)
SPX = 0.0055
STREAM_CEILING = 6.29e12   # bytes/s: measured float4 copy on the MI355X (8.0 TB/s spec)
LANE_OPS_PEAK = 256 * 4 * 16 * 2.4e9   # vector instructions x lanes per second: 39.3 T (fp64 FMA peak 78.6 TFLOP/s counts two per FMA;
                                        # a packed fp32 instruction does two of these per lane)


def ops_per_pixel(config, world, sigma):
    """arithmetic operations of projectPointBack per valid pixel, counted from the model (a division counts as one)"""
    nr, tan = config & 3, bool(config & 4)
    sweep = (3 + 1 + (3 if nr > 1 else 0) + 2 if nr else 0) + (3 + 16 if tan else 0) + 4
    n = 3 + 11 + (10 * sweep if (nr or tan) else 0) + 8
    return n + (18 if world else 0) + (27 if sigma else 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, default=8)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--config", type=lambda s: int(s, 0), default=0x6)
    ap.add_argument("--sample-points", type=int, default=200_000)
    ap.add_argument("--out", default=None, help="write the rows as JSON to this file")
    args = ap.parse_args()
    import torch
    W = H = args.size
    rs = np.random.default_rng(1)
    yy, xx = np.mgrid[0:H, 0:W]
    rows = []
    G = np.zeros((17, 17)); G[0, 0], G[1, 1], G[2, 2], G[1, 2], G[2, 1] = 1e-4, 4e-4, 1e-6, -1.5e-5, -1.5e-5
    with depth.DepthMaps(W, H, args.maps) as dm:
        for m in range(args.maps):
            v = 2.75 + 0.45 * np.sin((xx + 31 * m) / 137.0) * np.cos(yy / 229.0)
            raw = np.rint((1.0 - 1.0 / v) * 65535.0).astype(np.uint16)
            raw[rs.random((H, W)) < 0.05] = 0
            dm.setMaps(raw, first=m)
        views = np.column_stack([rs.uniform(-0.3, 0.3, (args.maps, 3)), rs.uniform(-200, 200, (args.maps, 3))])
        frames = np.arange(args.maps)
        npix = args.maps * W * H
        variants = [("xyz", dict()), ("xyz+z+sigma_z", dict(want_z=True, want_sigma_z=True, cam_cov=G, sigma_v=0.01)),
                    ("world xyz+z+sigma_z", dict(want_z=True, want_sigma_z=True, cam_cov=G, sigma_v=0.01, frames=frames, views=views))]
        for ev in (0, 1):
            for name, kw in variants:
                times = []
                for k in range(args.repeats + 2):   # two warm-up calls per variant
                    r = dm.backProjectMaps(CAM, args.config, SPX, eval=ev, device_out=True, **kw)
                    if k >= 2:
                        times.append(r.seconds)
                    del r
                t = float(np.median(times))
                nbytes = 2 + 12 + (8 if "want_z" in kw else 0)
                ops = ops_per_pixel(args.config, "frames" in kw, "want_sigma_z" in kw)
                row = dict(eval="fp64" if ev == 0 else "fp32", variant=name, ms_per_map=t / args.maps * 1e3, spread_ms=(max(times) - min(times)) / args.maps * 1e3,
                           bytes_per_pixel=nbytes, ops_per_pixel=ops, bytes_per_s=npix * nbytes / t, lane_ops_per_s=npix * ops / t)
                row["share_of_stream"] = row["bytes_per_s"] / STREAM_CEILING
                row["share_of_lane_ops"] = row["lane_ops_per_s"] / LANE_OPS_PEAK
                rows.append(row)
                print(f"{row['eval']} {name:22s} {row['ms_per_map']:.4f} ms/map (spread {row['spread_ms']:.4f})  {row['bytes_per_s'] / 1e12:.3f} TB/s "
                      f"({100 * row['share_of_stream']:.1f} % of the {STREAM_CEILING / 1e12:.2f} TB/s copy ceiling)  {row['lane_ops_per_s'] / 1e12:.2f} T lane-ops/s "
                      f"({100 * row['share_of_lane_ops']:.1f} % of {LANE_OPS_PEAK / 1e12:.1f} T)", flush=True)
        torch.cuda.synchronize()
        # the sampler: image points over map 0, a third of them on invalid pixels
        n = args.sample_points
        x = rs.uniform(0, W - 1, n); y = rs.uniform(0, H - 1, n)
        walls = []
        for k in range(5):
            t0 = time.perf_counter(); vd, counts = dm.sample(x, y, 0); walls.append(time.perf_counter() - t0)
        row = dict(sampler_points=n, wall_ms=float(np.median(walls[1:])) * 1e3, direct=int(counts.direct), interpolated=int(counts.interpolated), failed=int(counts.failed))
        rows.append(row)
        print(f"sampler: {n} points, {row['wall_ms']:.3f} ms per call (host clock, upload + kernel + download); direct {row['direct']} interpolated {row['interpolated']} "
              f"failed {row['failed']}", flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
