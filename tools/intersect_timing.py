"""Time of lifcal_intersect_points on the bench workload's points (metric_web: ~1.0 M observations on 16.7 k - 24.7 k points) next to
the route that existed before it: the same data as ONE <2,17,6,3> problem with every camera slot in fixed_mask and every frame
constant (lifcal_ba_set_fixed_frames), created and solved.

Camera, poses and points are the values of a full solve of the scene; both routes start at the scene's pts0.  After one warm-up of
each route the two alternate --repeats times in one process; medians are printed.
  (a) intersection: the kernels' HIP-event time (frame table, lens pass, k_intersect) and the wall time of the whole call (host
      sort, upload, download); iterations per point
  (b) joint solve: wall time of lifcal_ba_create + set_fixed_frames + lifcal_ba_solve + destroy, and of the solve alone (its
      summary's seconds_total).  If the library refuses that problem the refusal is reported and (a) stands alone.
With --out the numbers are also written as JSON.  Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o intersect -- python tools/intersect_timing.py
and read the k_intersect / k_intersect_frames / k_resect_lens rows of the stats file.
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

from lifcal_amd import BundleAdjustment, LifcalError, _capi as capi, intersectPoints  # noqa: E402
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
        cam, views = full.cam.copy(), full.views.copy()
        config = sc.config | 0x500   # the arity of the joint route
        F = len(views) // 6

        def intersect():
            t = time.perf_counter()
            r = intersectPoints(cam, views, sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.pts0, config, sc.spx, sc.scale)
            return r, time.perf_counter() - t

        def joint():
            pa = capi.ProblemArrays(sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, cam, views, sc.pts0, sc.spx, sc.scale, config, fixed_mask=0x1FFFF)
            t = time.perf_counter()
            with BundleAdjustment(pa) as ba:
                ba.set_fixed_frames(np.ones(F, np.uint8))
                s = ba.performBundleAdjustment()
            return pa, s, time.perf_counter() - t

        r, _ = intersect()   # warm-up (code objects, stream pool, allocator)
        refusal = None
        try:
            pa, s, _ = joint()
        except LifcalError as e:
            refusal = str(e)
        dev, wall, jwall, jsolve = [], [], [], []
        for _ in range(args.repeats):
            r, w = intersect(); dev.append(r.seconds); wall.append(w)
            if refusal is None:
                pa, s, w = joint(); jwall.append(w); jsolve.append(s.seconds_total)
        n = r.n_obs.astype(np.float64)
        it = r.iterations
        res = dict(n_obs=int(len(sc.u)), n_points=int(len(r.rows)), n_frames=int(F), obs_per_point_mean=float(n.mean()), obs_per_point_min=int(n.min()), obs_per_point_max=int(n.max()),
                   intersect_kernel_ms=median(dev) * 1e3, intersect_kernel_ms_min=min(dev) * 1e3, intersect_kernel_ms_max=max(dev) * 1e3,
                   intersect_call_wall_ms=median(wall) * 1e3,
                   intersect_iterations_min=int(it.min()), intersect_iterations_mean=float(it.mean()), intersect_iterations_max=int(it.max()),
                   intersect_rejected_steps=int(r.rows["unsuccessful_steps"].sum()),
                   intersect_terminations={int(k): int(c) for k, c in zip(*np.unique(r.termination, return_counts=True))},
                   idle_lane_share_first_pass=float(np.mean(np.maximum(0.0, 64.0 - n) / 64.0)))
        # observation evaluations of the intersection: per LM iteration one candidate (values), per accepted step one sweep (Jacobian),
        # plus the first sweep and the epilogue
        evals = float(np.sum(n * (it + r.rows["successful_steps"] + 2)))
        res["intersect_obs_evaluations"] = evals
        res["intersect_obs_evaluations_per_s"] = evals / (median(dev) + 1e-300)
        line = (f"{name}: N={res['n_obs']} P={res['n_points']} F={F} ({res['obs_per_point_mean']:.1f} observations per point, {res['obs_per_point_min']} .. {res['obs_per_point_max']}): "
                f"intersection kernels {res['intersect_kernel_ms']:.3f} ms (min {res['intersect_kernel_ms_min']:.3f}, max {res['intersect_kernel_ms_max']:.3f}), whole call {res['intersect_call_wall_ms']:.2f} ms, "
                f"iterations per point {res['intersect_iterations_min']} / {res['intersect_iterations_mean']:.2f} / {res['intersect_iterations_max']}, {res['intersect_rejected_steps']} rejected steps, "
                f"terminations {res['intersect_terminations']}, {res['intersect_obs_evaluations_per_s'] / 1e9:.2f} G observation evaluations per s; ")
        if refusal is None:
            dpts = float(np.max(np.abs(pa.pts.reshape(-1, 3) - r.pts)))
            dcost = abs(s.final_cost - float(r.final_cost.sum())) / s.final_cost
            res.update(joint_create_solve_wall_ms=median(jwall) * 1e3, joint_solve_ms=median(jsolve) * 1e3, joint_solve_ms_min=min(jsolve) * 1e3, joint_solve_ms_max=max(jsolve) * 1e3,
                       joint_iterations=int(s.iterations), joint_termination=int(s.termination), point_diff_max=dpts, cost_diff_rel=float(dcost))
            line += (f"joint <2,17,6,3> route (camera fixed by mask, all frames constant): create + solve {res['joint_create_solve_wall_ms']:.2f} ms, solve alone {res['joint_solve_ms']:.2f} ms "
                     f"(min {res['joint_solve_ms_min']:.2f}, max {res['joint_solve_ms_max']:.2f}) in {res['joint_iterations']} iterations (termination {res['joint_termination']}); "
                     f"points agree to {dpts:.2e} mm, summed cost to {dcost:.2e}")
        else:
            res["joint_refusal"] = refusal
            line += f"joint <2,17,6,3> route: the library refuses the problem ({refusal}); no baseline"
        results[name] = res
        print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
