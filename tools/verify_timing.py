"""Times lifcal_matches_verify (include/lifcal_verify.h) at section 7w's workload: `frames` frames that see
`points` scene points through small rigid motions, every frame matched against the next `window` (37 pairs for 20 frames), every
point matched in every pair, 30 % of the matches with a displaced partner.  Per row (hypotheses, refine) the kernel time (HIP
events around k_verify_score and every k_verify_classify) and the host clock around whole calls, median / min / max of `reps`
calls after one warm-up call, and the point tests per second of the kernel time.  Prints one JSON line.
Run under rocprofv3 --kernel-trace --stats for the per-kernel times.

usage: verify_timing.py [reps] [--points N] [--frames F] [--window W]"""
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

args = sys.argv[1:]
opt = {}
for flag in ("--points", "--frames", "--window"):
    if flag in args:
        i = args.index(flag)
        opt[flag] = args[i + 1]
        del args[i:i + 2]
reps = int(args[0]) if args else 7
N, F, WINDOW = int(opt.get("--points", 8000)), int(opt.get("--frames", 20)), int(opt.get("--window", 2))

from lifcal_amd import FeaturePoints, Matches, verifyMatches
from lifcal_amd.features import sequence_pairs

rng = np.random.default_rng(5)
Z = rng.uniform(300.0, 1500.0, N)
X = np.stack([Z * rng.uniform(-0.3, 0.3, N), Z * rng.uniform(-0.2, 0.2, N), Z], axis=1)


def rotation(axis, angle):
    a = axis / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


xyz = []
for f in range(F):
    R, t = rotation(rng.normal(size=3), math.radians(rng.uniform(0.0, 5.0))), rng.uniform(-25.0, 25.0, 3)
    P = X @ R.T + t
    lat, dep = 1.0e-3 * P[:, 2], 2.0e-6 * P[:, 2] ** 2
    r = P / np.linalg.norm(P, axis=1, keepdims=True)
    side = np.cross(r, rng.normal(size=P.shape)); side /= np.linalg.norm(side, axis=1, keepdims=True)
    true = P + r * (rng.uniform(-1, 1, N) * dep / 3.0)[:, None] + side * (rng.uniform(0, 1, N) * lat / 3.0)[:, None]
    far = P + side * (rng.uniform(10.0, 20.0, N) * lat)[:, None]     # the partners of the spoilt matches: features N .. 2 N - 1
    xyz.append(np.concatenate([true, far]))
xyz = np.ascontiguousarray(np.concatenate(xyz))
offset = (2 * N * np.arange(F + 1)).astype(np.uint32)
points = FeaturePoints(offset, xyz, 1.0e-3 * xyz[:, 2], 2.0e-6 * xyz[:, 2] ** 2)
pairs = sequence_pairs(F, WINDOW)
mi = np.tile(np.arange(N, dtype=np.uint32), len(pairs))
spoilt = rng.uniform(size=len(mi)) < 0.3
mj = np.where(spoilt, mi + N, mi).astype(np.uint32)
matches = Matches(pairs, (N * np.arange(len(pairs) + 1)).astype(np.uint64), mi, mj, np.zeros(len(mi), np.uint32))

out = {"points": N, "frames": F, "window": WINDOW, "n_pairs": int(len(pairs)), "n_matches": int(len(mi)), "reps": reps, "rows": []}


def stats(prefix, values):
    return {f"{prefix}_median": float(np.median(values)), f"{prefix}_min": float(np.min(values)), f"{prefix}_max": float(np.max(values))}


for hypotheses, refine in ((1024, -1), (1024, 2), (256, 2), (4096, 2)):
    ks, ts = [], []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        v = verifyMatches(points, matches, hypotheses=hypotheses, refine=refine, seed=1)
        if r:
            ts.append((time.perf_counter() - t0) * 1e3); ks.append(v.seconds * 1e3)
    row = {"hypotheses": hypotheses, "refine": refine, "pairs_ok": int((v.pair["status"] == 0).sum()), "kept": int(v.keep.sum()),
           "kept_spoilt": int(v.keep[spoilt].sum()), "true": int((~spoilt).sum()), "rounds_used": int(v.pair["rounds_used"].sum()),
           "point_tests": int(len(mi)) * hypotheses}
    row.update(stats("kernel_ms", ks)); row.update(stats("call_ms", ts))
    row["tests_per_second"] = row["point_tests"] / (row["kernel_ms_median"] * 1e-3)
    out["rows"].append(row)
print(json.dumps(out))
