"""Time of lifcal_ba_residual_report at the bench workload (metric_web, 334 frames, ~1.0 M observations) next to the route that
existed before it: lifcal_ba_project_observations, then numpy bincount grouping by frame and by point on the host.

Prints one line per workload (medians of --repeats warm calls after one LM solve): the report's device time (HIP events around its
kernels), its wall time with all tables and all per-observation arrays copied back, its wall time with the tables alone, and the
wall time of the old route.  With --out the numbers are also written as JSON.  Per-kernel times: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o res -- python tools/residual_timing.py
and read the k_residuals / k_group_stats rows of the stats file.
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

from lifcal_amd import BundleAdjustment, _capi as capi  # noqa: E402
from tools.cov_timing import make  # noqa: E402


def median(v):
    return sorted(v)[len(v) // 2]


def old_route(ba, pa):
    """what a caller did before: both projected columns to the host, then the sums per frame and per point in numpy (no lens
    grouping: the lens ids were not available)"""
    x, y = ba.projectObservations()
    ex, ey = x - pa.u, y - pa.v
    out = []
    for key, m in ((pa.fr, pa.struct.n_frames), (pa.pt, pa.struct.n_points)):
        out.append([np.bincount(key, weights=t, minlength=m) for t in (ex, ey, ex * ex, ey * ey)] + [np.bincount(key, minlength=m)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="metric_web")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    results = {}
    for name in args.workloads.split(","):
        sc = make(name)
        pa = capi.ProblemArrays.from_scene(sc)
        with BundleAdjustment(pa) as ba:
            s = ba.performBundleAdjustment()
            info = ba.info()
            t = time.perf_counter(); ba.residualReport(); first = time.perf_counter() - t   # builds the indices
            old_route(ba, pa)
            dev, wall, wall_tables, old = [], [], [], []
            for _ in range(args.repeats):
                t = time.perf_counter(); r = ba.residualReport(); wall.append(time.perf_counter() - t); dev.append(r.seconds)
                t = time.perf_counter(); ba.residualReport(per_observation=False); wall_tables.append(time.perf_counter() - t)
                t = time.perf_counter(); old_route(ba, pa); old.append(time.perf_counter() - t)
        res = dict(n_obs=int(pa.struct.n_obs), n_frames=int(pa.struct.n_frames), n_points=int(pa.struct.n_points), n_lenses=int(info.n_lenses),
                   first_call_ms=first * 1e3, report_device_ms=median(dev) * 1e3, report_wall_ms=median(wall) * 1e3,
                   report_tables_only_wall_ms=median(wall_tables) * 1e3, old_route_wall_ms=median(old) * 1e3, lm_solve_ms=s.seconds_total * 1e3)
        results[name] = res
        print(f"{name}: N={res['n_obs']} F={res['n_frames']} P={res['n_points']} lenses={res['n_lenses']}: report device {res['report_device_ms']:.3f} ms, "
              f"wall {res['report_wall_ms']:.3f} ms (tables only {res['report_tables_only_wall_ms']:.3f} ms, first call {res['first_call_ms']:.1f} ms); "
              f"project_observations + numpy bincount by frame and point {res['old_route_wall_ms']:.3f} ms; LM solve {res['lm_solve_ms']:.1f} ms")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
