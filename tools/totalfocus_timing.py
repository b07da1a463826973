"""Times lifcal_totalfocus_render (include/lifcal_totalfocus.h) on the workload of section 7t: a 2048 x 2048
raw image of 11 k lenses at d = 21 px over a smooth depth field, with the TRUE depth of that field at the cell centres as the depth
map (the timing then does not depend on the sweep), at scale 1 and 2, without and with a white image, 8 and 16 bit.  Per row: the
status counts, the mean lenses per cell, the kernel time (HIP events, result.seconds) and the host clock around whole calls with
host and with device pointers, median / min / max of `reps` calls after one warm-up call.  Prints one JSON line.  Run under
rocprofv3 --kernel-trace --stats for the per-kernel times.

usage: totalfocus_timing.py [reps] [--size N] [--image file.npy] [--no-torch]
  (--image: the rendered 8-bit image, to skip the rendering; --save-image file.npy writes it and leaves)"""
import json
import sys
import time

import numpy as np

args = sys.argv[1:]
opt = {}
for flag in ("--image", "--save-image", "--size"):
    if flag in args:
        i = args.index(flag)
        opt[flag] = args[i + 1]
        del args[i:i + 2]
use_torch = "--no-torch" not in args
args = [a for a in args if a != "--no-torch"]
reps = int(args[0]) if args else 7
W = H = int(opt.get("--size", 2048))
D, ROT, OFF, BASE_Y = 21.0, 0.002, (0.3, -0.6), (-0.5, 0.8660254)
depth_fn = lambda x, y: 4.0 + 2.0 * np.sin(np.asarray(x) / 300.0) * np.cos(np.asarray(y) / 400.0)

from lifcal_amd import raw_image, white_image
tx, ty = white_image.grid_centres(W, H, D, BASE_Y, ROT, OFF, 1.5)
if "--image" in opt:
    img8 = np.load(opt["--image"])
else:
    img8 = raw_image.render_raw_image(W, H, tx, ty, D, depth_fn, raw_image.band_limited_texture(7, 18.0, 60.0), bits=8, noise=0.004, seed=11, supersample=1)
    if "--save-image" in opt:
        np.save(opt["--save-image"], img8)
        sys.exit(0)
white8 = white_image.render_white_image(W, H, tx, ty, D, bits=8, vignetting=0.6, supersample=1)
images = {8: (img8, white8), 16: (img8.astype(np.uint16) * 257, white8.astype(np.uint16) * 257)}

if use_torch:
    import torch   # the first HIP runtime of the process sees the GPU: torch before the library when tensors are handed over
    torch.cuda.init(); torch.zeros(1, device="cuda"); torch.cuda.synchronize()
from lifcal_amd import MicroLensGrid, totalFocusImage

g = MicroLensGrid(W, H, D, BASE_Y, ROT, OFF)
out = {"width": W, "height": H, "lens_diameter": D, "n_lenses": g.n_lenses, "reps": reps, "rows": []}


def on_device(a):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


for scale in (1, 2):
    oh, ow = H // scale, W // scale
    Y, X = np.meshgrid(np.arange(oh, dtype=np.float64), np.arange(ow, dtype=np.float64), indexing="ij")
    iv = (1.0 / depth_fn((X + 0.5) * scale - 0.5, (Y + 0.5) * scale - 0.5)).astype(np.float32)
    for bits in (8, 16):
        img, white = images[bits]
        for with_white in (False, True):
            row = {"scale": scale, "bits": bits, "white": with_white}
            kinds = (("host", img, white, iv),) + ((("device", on_device(img), on_device(white), torch.from_numpy(iv).cuda()),) if use_torch else ())
            for kind, a_img, a_white, a_iv in kinds:
                ks, ts = [], []
                for r in range(reps + 1):
                    t0 = time.perf_counter()
                    tf = totalFocusImage(g, a_img, a_iv, white=a_white if with_white else None, device_out=(kind == "device"), scale=scale)
                    if r:
                        ts.append((time.perf_counter() - t0) * 1e3); ks.append(tf.seconds * 1e3)
                if kind == "host":
                    row.update({"counts": tf.counts.tolist(), "mean_lenses_per_cell": float(tf.n_lenses.mean())})
                row.update({f"kernel_ms_median_{kind}": float(np.median(ks)), f"kernel_ms_min_{kind}": float(np.min(ks)), f"kernel_ms_max_{kind}": float(np.max(ks)),
                            f"call_ms_median_{kind}": float(np.median(ts)), f"call_ms_min_{kind}": float(np.min(ts))})
            out["rows"].append(row)
print(json.dumps(out))
