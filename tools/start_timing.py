"""Time of lifcal_start_poses and lifcal_start_points on the bench workload (metric_web: ~1.0 M observations, 334 frames, 24 720
points), and what the two calls that follow them make of the start values.

Camera, poses and points are the values of a full solve of the scene.  After one warm-up the two calls alternate --repeats times in
one process; medians are printed:
  (a) startPoses: the kernels' HIP-event time (two lens passes, k_start_groups, k_start_align) and the wall time of the whole call
      (two counting sorts, group cut, staging, upload, download); frame statuses, used groups, start RMS
  (b) startPoints: likewise (frame table, two lens passes, k_start_points)
and, once each, resectFrames from (a) and intersectPoints from (b): iterations and terminations, for orientation.
There is no earlier route to compare with: nothing in the library produced start values before.
With --out the numbers are also written as JSON.  Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o start -- python tools/start_timing.py
and read the k_start_groups / k_start_align / k_start_points / k_resect_lens rows of the stats file.
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

from lifcal_amd import BundleAdjustment, _capi as capi, intersectPoints, resectFrames, startPoints, startPoses  # noqa: E402
from tools.cov_timing import make  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="metric_web")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--gate", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = {}
    for name in args.workloads.split(","):
        sc = make(name)
        full = capi.ProblemArrays.from_scene(sc)
        with BundleAdjustment(full) as ba:
            ba.performBundleAdjustment()
        cam, views, pts = full.cam.copy(), full.views.copy(), full.pts.copy()
        F, P = len(views) // 6, len(pts) // 3
        obs = (sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)

        def poses():
            t = time.perf_counter()
            r = startPoses(cam, pts, *obs, F, sc.config, sc.spx, sc.scale, gatePx=args.gate, wantGroups=True)
            return r, time.perf_counter() - t

        def points():
            t = time.perf_counter()
            r = startPoints(cam, views, *obs, P, sc.config, sc.spx, sc.scale)
            return r, time.perf_counter() - t

        a, _ = poses(); b, _ = points()   # warm-up (code objects, stream pool, allocator)
        adev, awall, bdev, bwall = [], [], [], []
        for _ in range(args.repeats):
            a, w = poses(); adev.append(a.seconds); awall.append(w)
            b, w = points(); bdev.append(b.seconds); bwall.append(w)
        g = a.groups
        ok = a.status == 0
        n = b.rows["n_obs"].astype(np.float64)
        okp = b.status == 0
        res = dict(n_obs=int(len(sc.u)), n_frames=int(F), n_points=int(P), n_groups=int(len(g)), obs_per_group_mean=float(g["n_obs"].mean()), obs_per_group_max=int(g["n_obs"].max()),
                   gate_px=args.gate,
                   poses_kernel_ms=median(adev) * 1e3, poses_kernel_ms_min=min(adev) * 1e3, poses_kernel_ms_max=max(adev) * 1e3, poses_call_wall_ms=median(awall) * 1e3,
                   frame_status={int(k): int(c) for k, c in zip(*np.unique(a.status, return_counts=True))},
                   group_status={int(k): int(c) for k, c in zip(*np.unique(g["status"], return_counts=True))},
                   used_share_min=float((a.rows["n_used"][ok] / a.rows["n_groups"][ok]).min()) if ok.any() else None,
                   poses_start_rms_px=float(np.sqrt((a.rows["sum_xx"][ok] + a.rows["sum_yy"][ok]).sum() / max(a.rows["n_obs"][ok].sum(), 1))),
                   poses_start_rms_px_worst_frame=float(np.nanmax(np.hypot(a.rms_x, a.rms_y))) if ok.any() else None,
                   pose_distance_to_solve=[float(np.nanmax(np.abs(a.views[:, :3] - views.reshape(-1, 6)[:, :3]))), float(np.nanmax(np.abs(a.views[:, 3:] - views.reshape(-1, 6)[:, 3:])))],
                   points_kernel_ms=median(bdev) * 1e3, points_kernel_ms_min=min(bdev) * 1e3, points_kernel_ms_max=max(bdev) * 1e3, points_call_wall_ms=median(bwall) * 1e3,
                   point_status={int(k): int(c) for k, c in zip(*np.unique(b.status, return_counts=True))},
                   obs_per_point_mean=float(n.mean()), obs_per_point_min=int(n.min()), obs_per_point_max=int(n.max()),
                   points_start_rms_px=float(np.sqrt((b.rows["sum_xx"][okp] + b.rows["sum_yy"][okp]).sum() / max(n[okp].sum(), 1))),
                   point_distance_to_solve_mm=float(np.nanmax(np.abs(b.pts - pts.reshape(-1, 3)))))
        # the calls they feed, once each (frames / points without a start value keep the solve's)
        v0 = np.where(ok[:, None], a.views, views.reshape(-1, 6))
        p0 = np.where(okp[:, None], b.pts, pts.reshape(-1, 3))
        rs = resectFrames(cam, pts, *obs, v0, sc.config, sc.spx, sc.scale)
        it = intersectPoints(cam, views, *obs, p0, sc.config | 0x500, sc.spx, sc.scale)
        res.update(resect_kernel_ms=rs.seconds * 1e3, resect_iterations=[int(rs.iterations.min()), float(rs.iterations.mean()), int(rs.iterations.max())],
                   resect_terminations={int(k): int(c) for k, c in zip(*np.unique(rs.termination, return_counts=True))},
                   intersect_kernel_ms=it.seconds * 1e3, intersect_iterations=[int(it.iterations.min()), float(it.iterations.mean()), int(it.iterations.max())],
                   intersect_terminations={int(k): int(c) for k, c in zip(*np.unique(it.termination, return_counts=True))})
        results[name] = res
        print(f"{name}: N={res['n_obs']} F={F} P={P} groups={res['n_groups']} ({res['obs_per_group_mean']:.2f} observations per group, at most {res['obs_per_group_max']}), gate {args.gate} px\n"
              f"  startPoses: kernels {res['poses_kernel_ms']:.3f} ms (min {res['poses_kernel_ms_min']:.3f}, max {res['poses_kernel_ms_max']:.3f}), whole call {res['poses_call_wall_ms']:.2f} ms; "
              f"frame status {res['frame_status']}, group status {res['group_status']}, least used share {res['used_share_min']}, start rms {res['poses_start_rms_px']:.3f} px "
              f"(worst frame {res['poses_start_rms_px_worst_frame']}), from the solve's poses at most {res['pose_distance_to_solve'][0]:.2e} rad {res['pose_distance_to_solve'][1]:.2e} mm\n"
              f"  startPoints: kernels {res['points_kernel_ms']:.3f} ms (min {res['points_kernel_ms_min']:.3f}, max {res['points_kernel_ms_max']:.3f}), whole call {res['points_call_wall_ms']:.2f} ms; "
              f"point status {res['point_status']}, {res['obs_per_point_mean']:.1f} observations per point ({res['obs_per_point_min']} .. {res['obs_per_point_max']}), start rms {res['points_start_rms_px']:.4f} px, "
              f"from the solve's points at most {res['point_distance_to_solve_mm']:.2e} mm\n"
              f"  resectFrames from these poses: kernels {res['resect_kernel_ms']:.3f} ms, iterations {res['resect_iterations']}, terminations {res['resect_terminations']}; "
              f"intersectPoints from these points: kernels {res['intersect_kernel_ms']:.3f} ms, iterations {res['intersect_iterations']}, terminations {res['intersect_terminations']}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
