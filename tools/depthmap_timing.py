"""Times lifcal_depthmap_from_raw (include/lifcal_depthmap.h) on the workload of section 7t: a 2048 x 2048
raw image of 11 k lenses at d = 21 px over a smooth depth field, lifcal_rawdepth_estimate at its defaults (K = 64, 6 neighbours),
then the virtual-image depth map at scale 1 and 2.  Per scale: the status counts, the samples, the footprint cells (the atomics
of one scatter pass), the kernel time (HIP events, result.seconds) and the host clock around whole calls with host and with device
pointers, median / min / max of `reps` calls after one warm-up call.  Prints one JSON line.  Run under rocprofv3 --kernel-trace
--stats for the per-kernel times.

usage: depthmap_timing.py [reps] [--image file.npy]   (the rendered 8-bit image, to skip the rendering; --save-image file.npy writes it)"""
import json
import sys
import time

import numpy as np

args = sys.argv[1:]
opt = {}
for flag in ("--image", "--save-image"):
    if flag in args:
        i = args.index(flag)
        opt[flag] = args[i + 1]
        del args[i:i + 2]
reps = int(args[0]) if args else 7
W = H = 2048
D, ROT, OFF, BASE_Y = 21.0, 0.002, (0.3, -0.6), (-0.5, 0.8660254)

if "--image" in opt:
    img = np.load(opt["--image"])
else:
    from lifcal_amd import raw_image, white_image
    tx, ty = white_image.grid_centres(W, H, D, BASE_Y, ROT, OFF, 1.5)
    depth_fn = lambda x, y: 4.0 + 2.0 * np.sin(np.asarray(x) / 300.0) * np.cos(np.asarray(y) / 400.0)
    img = raw_image.render_raw_image(W, H, tx, ty, D, depth_fn, raw_image.band_limited_texture(7, 18.0, 60.0), bits=8, noise=0.004, seed=11, supersample=1)
    if "--save-image" in opt:
        np.save(opt["--save-image"], img)
        sys.exit(0)

use_torch = "--no-torch" not in args
if use_torch:
    import torch   # the first HIP runtime of the process sees the GPU: torch before the library when tensors are handed over
    torch.cuda.init(); torch.zeros(1, device="cuda"); torch.cuda.synchronize()
from lifcal_amd import MicroLensGrid, depthMapFromRaw
from tests import depthmap_reference as dref

g = MicroLensGrid(W, H, D, BASE_Y, ROT, OFF)
est = g.estimateRawDepth(img)
est = g.estimateRawDepth(img, device_out=use_torch)
iv_host = est.inv_depth.cpu().numpy() if use_torch else est.inv_depth
map_ml, _ = g.maps()
cx, cy, _ = g.lenses()
out = {"width": W, "height": H, "lens_diameter": D, "n_lenses": g.n_lenses, "rawdepth_counts": est.counts.tolist(), "rawdepth_kernel_ms": est.seconds * 1e3, "scales": []}
for scale in (1, 2):
    o = dref.options(W, H, scale=scale)
    src, q, X0, X1, Y0, Y1 = dref.samples(iv_host, map_ml, cx, cy, o)
    fw = np.minimum(X1, o["out_width"] - 1.0) - np.maximum(X0, 0.0) + 1.0
    fh = np.minimum(Y1, o["out_height"] - 1.0) - np.maximum(Y0, 0.0) + 1.0
    cells = int((np.maximum(fw, 0.0) * np.maximum(fh, 0.0)).sum())
    row = {"scale": scale, "footprint_cells": cells}
    for kind, iv in (("host", iv_host),) + ((("device", est.inv_depth),) if use_torch else ()):
        ks, ts = [], []
        for r in range(reps + 1):
            t0 = time.perf_counter()
            dm = depthMapFromRaw(g, iv, device_out=(kind == "device"), scale=scale)
            if r:
                ts.append((time.perf_counter() - t0) * 1e3); ks.append(dm.seconds * 1e3)
        row.update({"counts": dm.counts.tolist(), "n_samples": dm.n_samples, "cells_per_sample": cells / max(1, dm.n_samples),
                    f"kernel_ms_median_{kind}": float(np.median(ks)), f"kernel_ms_min_{kind}": float(np.min(ks)), f"kernel_ms_max_{kind}": float(np.max(ks)),
                    f"call_ms_median_{kind}": float(np.median(ts)), f"call_ms_min_{kind}": float(np.min(ts))})
    out["scales"].append(row)
print(json.dumps(out))
