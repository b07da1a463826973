"""Time of lifcal_register_scene on the bench workload (metric_web: ~1.0 M observations, 334 frames, 24 720 points), and what a
bundle adjustment makes of its result.

The camera is that of a full solve of the scene; poses and points are not handed over.  After one warm-up the call is repeated
--repeats times in one process; medians are printed: the HIP-event time between the staging upload and the final download (all
kernels of all rounds and the one-word read-backs between them) and the wall time of the whole call (three counting sorts, group
cut, staging, upload, download); rounds, frames registered, points mapped, the RMS at the returned parameters.  Then, once,
lifcal_ba_solve over the registered part from the result (camera constant, poses and points free): its iterations and final cost,
next to the same solve from the full solve's poses and points.
There is no earlier route to compare with: nothing in the library registered a scene before.
With --out the numbers are also written as JSON.
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

from lifcal_amd import BundleAdjustment, _capi as capi, registerScene  # noqa: E402
from tools.cov_timing import make  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="metric_web")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--gate", type=float, default=1.0)
    ap.add_argument("--min-shared", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = {}
    for name in args.workloads.split(","):
        sc = make(name)
        full = capi.ProblemArrays.from_scene(sc)
        with BundleAdjustment(full) as ba:
            ba.performBundleAdjustment()
        cam, views, pts = full.cam.copy(), full.views.copy().reshape(-1, 6), full.pts.copy().reshape(-1, 3)
        F, P = len(views), len(pts)
        obs = (sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)

        def call():
            t = time.perf_counter()
            r = registerScene(cam, *obs, F, P, sc.config, sc.spx, sc.scale, gatePx=args.gate, minShared=args.min_shared)
            return r, time.perf_counter() - t

        r, _ = call()   # warm-up (code objects, stream pool, allocator)
        dev, wall = [], []
        for _ in range(args.repeats):
            r, w = call(); dev.append(r.seconds); wall.append(w)
        s = r.summary
        reg, mp = r.registered, r.mapped
        m = reg[sc.fr] & mp[sc.pt]
        fmap, pmap = np.cumsum(reg) - 1, np.cumsum(mp) - 1
        sub = tuple(a[m] for a in obs[:4]) + (pmap[sc.pt[m]].astype(np.uint32), fmap[sc.fr[m]].astype(np.uint32))
        solves = []
        for v0, p0 in ((r.views[reg], r.pts[mp]), (views[reg], pts[mp])):
            pa = capi.ProblemArrays(*sub, cam, v0, p0, sc.spx, sc.scale, sc.config | 0x500, fixed_mask=0x1FFFF)
            with BundleAdjustment(pa) as ba:
                solves.append(ba.performBundleAdjustment())
        res = dict(n_obs=int(len(sc.u)), n_frames=int(F), n_points=int(P), gate_px=args.gate, min_shared=args.min_shared,
                   anchor_frame=int(s.anchor_frame), rounds=int(s.n_rounds), frames_registered=int(s.n_frames_registered), points_mapped=int(s.n_points_mapped),
                   n_groups=int(s.n_groups), n_groups_used=int(s.n_groups_used), observations_registered=int(m.sum()),
                   kernel_ms=median(dev) * 1e3, kernel_ms_min=min(dev) * 1e3, kernel_ms_max=max(dev) * 1e3, call_wall_ms=median(wall) * 1e3,
                   start_rms_px=[r.rms_x, r.rms_y],
                   pose_iterations=[int(r.frame_rows["iterations"][reg].min()), int(r.frame_rows["iterations"][reg].max())],
                   point_iterations=[int(r.point_rows["iterations"][mp].min()), int(r.point_rows["iterations"][mp].max())],
                   ba_iterations=int(solves[0].iterations), ba_final_cost=float(solves[0].final_cost), ba_termination=int(solves[0].termination),
                   ba_iterations_from_solve=int(solves[1].iterations), ba_final_cost_from_solve=float(solves[1].final_cost))
        results[name] = res
        print(f"{name}: N={res['n_obs']} F={F} P={P}, gate {args.gate} px, min_shared {args.min_shared}\n"
              f"  registerScene: anchor {res['anchor_frame']}, {res['rounds']} rounds, {res['frames_registered']} frames, {res['points_mapped']} points, "
              f"{res['observations_registered']} observations; kernels and read-backs {res['kernel_ms']:.3f} ms (min {res['kernel_ms_min']:.3f}, max {res['kernel_ms_max']:.3f}), "
              f"whole call {res['call_wall_ms']:.2f} ms; rms {r.rms_x:.4f} {r.rms_y:.4f} px; last solves: poses {res['pose_iterations']}, points {res['point_iterations']} iterations\n"
              f"  lifcal_ba_solve from the result: {res['ba_iterations']} iterations to {res['ba_final_cost']:.9e} (termination {res['ba_termination']}); "
              f"from the full solve's values: {res['ba_iterations_from_solve']} iterations to {res['ba_final_cost_from_solve']:.9e}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
