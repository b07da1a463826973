"""Time of lifcal_resect_frames on the bench workload's frames (metric_web: 334 frames, ~1.0 M observations, ~3000 per frame) next
to the route that existed before it: the same data as ONE <2,17,6> problem with every camera slot in fixed_mask, created and solved.

Camera and points are the values of a full solve of the scene; the poses start at the scene's views0.  After one warm-up of each
route the two alternate --repeats times in one process; medians are printed.
  (a) resection: the kernels' HIP-event time (lens pass + k_resect) and the wall time of the whole call (host sort, upload, download)
  (b) joint solve: wall time of lifcal_ba_create + lifcal_ba_solve + destroy, and of the solve alone (its summary's seconds_total)
With --out the numbers are also written as JSON.  Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o resect -- python tools/resect_timing.py
and read the k_resect / k_resect_lens rows of the stats file.
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

from lifcal_amd import BundleAdjustment, _capi as capi, resectFrames  # noqa: E402
from tools.cov_timing import make  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="metric_web")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = {}
    for name in args.workloads.split(","):
        sc = make(name)
        full = capi.ProblemArrays.from_scene(sc)
        with BundleAdjustment(full) as ba:
            ba.performBundleAdjustment()
        cam, pts = full.cam.copy(), full.pts.copy()
        config = sc.config & ~0x400   # poses only: the arity of the joint route

        def resect():
            t = time.perf_counter()
            r = resectFrames(cam, pts, sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.views0, config, sc.spx, sc.scale)
            return r, time.perf_counter() - t

        def joint():
            pa = capi.ProblemArrays(sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, cam, sc.views0, pts, sc.spx, sc.scale, config, fixed_mask=0x1FFFF)
            t = time.perf_counter()
            with BundleAdjustment(pa) as ba:
                s = ba.performBundleAdjustment()
            return pa, s, time.perf_counter() - t

        r, _ = resect(); pa, s, _ = joint()   # warm-up (code objects, stream pool, allocator)
        dpose = float(np.max(np.abs(pa.views.reshape(-1, 6) - r.views)))
        dcost = abs(s.final_cost - float(r.final_cost.sum())) / s.final_cost
        dev, wall, jwall, jsolve = [], [], [], []
        for _ in range(args.repeats):
            r, w = resect(); dev.append(r.seconds); wall.append(w)
            pa, s, w = joint(); jwall.append(w); jsolve.append(s.seconds_total)
        n = r.n_obs.astype(np.float64)
        it = r.iterations
        res = dict(n_obs=int(len(sc.u)), n_frames=int(len(r.rows)), obs_per_frame_mean=float(n.mean()), obs_per_frame_max=int(n.max()),
                   resect_kernel_ms=median(dev) * 1e3, resect_kernel_ms_min=min(dev) * 1e3, resect_kernel_ms_max=max(dev) * 1e3,
                   resect_call_wall_ms=median(wall) * 1e3,
                   joint_create_solve_wall_ms=median(jwall) * 1e3, joint_solve_ms=median(jsolve) * 1e3, joint_solve_ms_min=min(jsolve) * 1e3, joint_solve_ms_max=max(jsolve) * 1e3,
                   joint_iterations=int(s.iterations), joint_termination=int(s.termination),
                   resect_iterations_min=int(it.min()), resect_iterations_mean=float(it.mean()), resect_iterations_max=int(it.max()),
                   resect_rejected_steps=int(r.rows["unsuccessful_steps"].sum()),
                   resect_terminations={int(k): int(c) for k, c in zip(*np.unique(r.termination, return_counts=True))},
                   pose_diff_max=dpose, cost_diff_rel=float(dcost))
        # observation evaluations of the resection: per LM iteration one candidate (values), per accepted step one sweep (Jacobian), plus
        # the first sweep and the epilogue
        evals = float(np.sum(n * (it + r.rows["successful_steps"] + 2)))
        res["resect_obs_evaluations"] = evals
        res["resect_obs_evaluations_per_s"] = evals / (median(dev) + 1e-300)
        results[name] = res
        print(f"{name}: N={res['n_obs']} F={res['n_frames']} ({res['obs_per_frame_mean']:.0f} observations per frame, max {res['obs_per_frame_max']}): "
              f"resection kernels {res['resect_kernel_ms']:.3f} ms (min {res['resect_kernel_ms_min']:.3f}, max {res['resect_kernel_ms_max']:.3f}), whole call {res['resect_call_wall_ms']:.2f} ms, "
              f"iterations per frame {res['resect_iterations_min']} / {res['resect_iterations_mean']:.2f} / {res['resect_iterations_max']}, "
              f"{res['resect_obs_evaluations_per_s'] / 1e9:.2f} G observation evaluations per s; "
              f"joint <2,17,6> route: create + solve {res['joint_create_solve_wall_ms']:.2f} ms, solve alone {res['joint_solve_ms']:.2f} ms "
              f"(min {res['joint_solve_ms_min']:.2f}, max {res['joint_solve_ms_max']:.2f}) in {res['joint_iterations']} iterations; "
              f"poses agree to {dpose:.2e}, summed cost to {dcost:.2e}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
