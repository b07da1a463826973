"""Solve time of the bench workload (metric_web: ~1.0 M observations, 334 frames, 24 720 points) without priors and with a camera
prior plus a prior on every one of the 334 poses (lifcal_ba_set_priors), alternating, three solves each in one process.

    python tools/prior_timing.py out.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/prior_timing.py out.json     (kernel time of k_priors)

Prints one row per solve (host clock around lifcal_ba_solve, iterations, costs, prior_cost()) and writes them as JSON.
Figures: profiles/priors/README.md.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lifcal_amd import BundleAdjustment, _capi as capi, scene   # noqa: E402
from lifcal_amd.mla import MicroLensGrid   # noqa: E402


def metric_web_scene():
    spec = scene.baseline_spec("metric_web")
    grid = MicroLensGrid(spec.raw_width, spec.raw_height, spec.lens_diameter, spec.lens_base_y, spec.grid_rotation, spec.grid_offset, True, device=0)

    def selector(img_x, img_y, img_vd, img_fr, img_pt, scale):
        o = grid.projectPointsToRawImage(img_x, img_y, img_vd, int(scale), fr=img_fr, pt=img_pt)
        return o.src, o.mcx, o.mcy
    sc = scene.make_scene(spec, lens_selector=selector)
    grid.close()
    return sc


def main():
    out_path = sys.argv[1]
    sc = metric_web_scene()
    F = len(sc.views0.reshape(-1)) // 6
    sig_cam = 0.05 * np.abs(sc.cam0) + 1e-4
    cam_info = np.zeros((17, 17)); cam_info[np.arange(9), np.arange(9)] = 1.0 / sig_cam[:9] ** 2
    sig_pose = np.array([0.01, 0.01, 0.01, 1.0, 1.0, 1.0])
    infos = np.tile(np.diag(1.0 / sig_pose ** 2), (F, 1, 1))
    rows = []
    for mode in ("none", "priors", "none", "priors", "none", "priors"):
        pa = capi.ProblemArrays.from_scene(sc)
        with BundleAdjustment(pa) as ba:
            if mode == "priors":
                ba.set_priors(camera=(sc.cam0, cam_info), poses=(np.arange(F), sc.views0.reshape(F, 6), infos))
            t0 = time.perf_counter()
            s = ba.performBundleAdjustment()
            dt = time.perf_counter() - t0
            pc = ba.prior_cost()
        rows.append(dict(mode=mode, n_obs=int(sc.n_obs), frames=F, wall_s=dt, seconds_total=s.seconds_total, iterations=s.iterations, termination=s.termination,
                         initial_cost=s.initial_cost, final_cost=s.final_cost, prior_cost=pc))
        print(rows[-1], flush=True)
    json.dump(rows, open(out_path, "w"), indent=1)


if __name__ == "__main__":
    main()
