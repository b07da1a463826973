"""Device time of lifcal_ba_covariance at the bench workload (metric_web, 334 frames) and at BASELINE configs[3] (1000 frames).

Prints one line per workload: the call's device time (HIP events around sweep + K1..K4), the same call without the pose blocks
(sweep + K1 + K3 + host C+), and one LM solve for comparison.  Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o cov -- python tools/cov_timing.py
and read the k_cov_* rows of the stats file (K1 k_cov_chol_w, K2 k_cov_selinv, K3 k_cov_backsolve, K4 k_cov_combine).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lifcal_amd import BundleAdjustment, _capi as capi, scene  # noqa: E402


def make(name):
    spec = scene.baseline_spec(name)
    if not name.endswith("_web"):
        return scene.make_scene(spec)
    from lifcal_amd.mla import MicroLensGrid
    grid = MicroLensGrid(spec.raw_width, spec.raw_height, spec.lens_diameter, spec.lens_base_y, spec.grid_rotation, spec.grid_offset, True, device=0)

    def selector(img_x, img_y, img_vd, img_fr, img_pt, scale):
        o = grid.projectPointsToRawImage(img_x, img_y, img_vd, int(scale), fr=img_fr, pt=img_pt)
        return o.src, o.mcx, o.mcy
    sc = scene.make_scene(spec, lens_selector=selector)
    grid.close()
    return sc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="metric_web,cfg4")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    for name in args.workloads.split(","):
        sc = make(name)
        pa = capi.ProblemArrays.from_scene(sc)
        with BundleAdjustment(pa) as ba:
            s = ba.performBundleAdjustment()
            info = ba.info()
            full, cam = [], []
            for _ in range(args.repeats):
                t = time.perf_counter(); c = ba.covariance(); wall = time.perf_counter() - t
                full.append((c.seconds, wall))
                cam.append(ba.covariance(want_pose_blocks=False).seconds)
            sw = min(ba.sweep(1e4).seconds for _ in range(5))
        dev = sorted(f[0] for f in full)[len(full) // 2]
        wall = sorted(f[1] for f in full)[len(full) // 2]
        print(f"{name}: F={pa.struct.n_frames} bw={info.max_window_frames - 1} promoted={info.n_promoted} "
              f"covariance device {dev * 1e3:.3f} ms (wall {wall * 1e3:.3f} ms), camera only {sorted(cam)[len(cam) // 2] * 1e3:.3f} ms, "
              f"one sweep {sw * 1e3:.3f} ms, LM solve {s.seconds_total * 1e3:.1f} ms over {s.iterations} iterations "
              f"({s.seconds_total / max(s.iterations, 1) * 1e3:.2f} ms per iteration); null_rank {c.null_rank}, gauge frame {c.gauge_frame}, "
              f"sigma2 {c.sigma2:.4g}")


if __name__ == "__main__":
    main()
