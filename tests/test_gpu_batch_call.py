"""The five one-call routes one after another in one process (lifcal_amd/csrc/batch_call.hpp): every call
returns its stream to the pool and the next one takes it out again, so the second call of a route runs on a stream another route
used, with that route's events, device block and error state long gone.

Bar: the second result of every route has the bits of its first (each route's own GPU test asserts that two calls in a row give
the same bits: tests/test_gpu_resection.py, test_gpu_intersection.py, test_gpu_start.py, test_gpu_register.py), and every call
reports a kernel time above zero."""
import numpy as np
import pytest

from lifcal_amd import intersectPoints, registerScene, resectFrames, scene, startPoints, startPoses
from tests.helpers import S

pytestmark = pytest.mark.gpu

SPEC = S(3, 8, None, 0xF06, 115, outlier_fraction=0.05)


def routes(sc):
    obs = (sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)
    tail = (sc.config, sc.spx, sc.scale)
    return {
        "resect": lambda: resectFrames(sc.cam_gt, sc.pts_gt, *obs, sc.views0, *tail),
        "intersect": lambda: intersectPoints(sc.cam_gt, sc.views_gt, *obs, sc.pts0, *tail),
        "start_poses": lambda: startPoses(sc.cam_gt, sc.pts_gt, *obs, SPEC.n_frames, *tail, wantGroups=True),
        "start_points": lambda: startPoints(sc.cam_gt, sc.views_gt, *obs, SPEC.n_points, *tail),
        "register": lambda: registerScene(sc.cam_gt, *obs, SPEC.n_frames, SPEC.n_points, *tail, minShared=3),   # (frame 0 shares 3 used groups)
    }


def bits(name, r):
    if name == "register":
        return [r.views.tobytes(), r.pts.tobytes(), r.frame_rows.tobytes(), r.point_rows.tobytes(), bytes(r.summary)]
    out = [(r.views if name in ("resect", "start_poses") else r.pts).tobytes(), r.rows.tobytes()]
    return out + [r.groups.tobytes()] if name == "start_poses" else out


def test_every_route_repeats_its_bits_on_a_stream_another_route_used(built):
    sc = scene.make_scene(SPEC)
    per_pair = sc.n_obs / len(np.unique(sc.fr.astype(np.int64) * SPEC.n_points + sc.pt))
    calls = routes(sc)
    first = {name: call() for name, call in calls.items()}
    second = {name: calls[name]() for name in reversed(list(calls))}
    print(f"{sc.n_obs} observations, {per_pair:.1f} per (point, frame) pair; kernel times in ms: "
          + ", ".join(f"{n} {first[n].seconds * 1e3:.3f} / {second[n].seconds * 1e3:.3f}" for n in calls))
    assert 3.0 <= per_pair <= 8.0
    for name in calls:
        assert bits(name, second[name]) == bits(name, first[name]), name
        assert first[name].seconds > 0.0 and second[name].seconds > 0.0, name
    # the calls did something: every frame and point solved, started and registered
    assert np.all(first["resect"].rows["iterations"] > 0) and np.all(first["intersect"].rows["iterations"] > 0)
    assert np.all(first["start_poses"].rows["status"] == 0) and np.all(first["start_points"].rows["status"] == 0)
    assert np.all(first["register"].registered) and np.all(first["register"].mapped)
