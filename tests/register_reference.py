"""The registration chain of include/lifcal_register.h restated as a driver: the round logic in Python, written
from the header's definition, with two arms that share it.

  arm     groups                                     alignment                  Levenberg-Marquardt solves
  cpu     start_reference.group_rows                 start_reference.align      one-frame / one-point oracle.solve
  gpu     startPoses(..., wantGroups=True), dummy    start_reference.align      the public resectFrames / intersectPoints on the
          points, only the group table is taken                                 compacted observation subsets of each step

The cpu arm needs no GPU and carries the method's own bars (tests/test_register_cpu.py); the gpu arm is what lifcal_register_scene is
compared with (tests/test_gpu_register.py): the same kernels' arithmetic, driven from the host one call per step."""
import types

import numpy as np

import oracle
from lifcal_amd import _capi as capi
from lifcal_amd.scene import euler_xyz
from tests import start_reference as sr

MODEL_BITS = 0xA07   # nRadial, tangential, ROBUST, ML_CENTER_ADJ


def _groups(arm, cam, u, v, mcx, mcy, pt, fr, n_frames, n_points, config, spx, scale, gate_px, spy=None):
    if arm == "cpu":
        return sr.group_rows(cam, u, v, mcx, mcy, pt, fr, config, spx, scale, spy=spy, gate_px=gate_px)[0]
    from lifcal_amd import startPoses
    return startPoses(cam, np.zeros((n_points, 3)), u, v, mcx, mcy, pt, fr, n_frames, config, spx, scale, spy=spy, gatePx=gate_px, wantGroups=True).groups


class _Solver:
    """one LM solve per frame (over its observations of mapped points) or per point (over its observations in registered frames)"""

    def __init__(self, arm, cam, u, v, mcx, mcy, pt, fr, config, spx, scale, options, spy=None):
        self.arm, self.cam, self.obs, self.pt, self.fr = arm, cam, (u, v, mcx, mcy), pt, fr
        self.config, self.spx, self.scale, self.options = config, spx, scale, options
        self.spy = spy   # None: spx

    def poses(self, frames, views, pts, mapped):
        """refines views[frames] in place; returns {frame: (final_cost, iterations, termination)}"""
        P = np.nan_to_num(pts)
        out = {}
        if self.arm == "cpu":
            for f in frames:
                m = (self.fr == f) & mapped[self.pt]
                pa = capi.ProblemArrays(*(a[m] for a in self.obs), self.pt[m], np.zeros(int(m.sum()), np.uint32), self.cam, views[f].copy(), P,
                                        self.spx, self.scale, (self.config & MODEL_BITS) | 0x100, spy=self.spy, fixed_mask=0x1FFFF)
                s = oracle.solve(pa, self.options)
                views[f] = pa.views
                out[f] = (s.final_cost, s.iterations, s.termination)
            return out
        from lifcal_amd import resectFrames
        frames = np.asarray(frames)
        m = np.isin(self.fr, frames) & mapped[self.pt]
        local = np.zeros(int(self.fr.max()) + 1, np.uint32); local[frames] = np.arange(len(frames))
        res = resectFrames(self.cam, P, *(a[m] for a in self.obs), self.pt[m], local[self.fr[m]], views[frames], self.config, self.spx, self.scale, spy=self.spy, options=self.options)
        views[frames] = res.views
        for k, f in enumerate(frames):
            out[int(f)] = (float(res.final_cost[k]), int(res.iterations[k]), int(res.termination[k]))
        return out

    def points(self, points, views, pts, registered):
        """refines pts[points] in place; returns {point: (final_cost, iterations, termination)}"""
        V = np.nan_to_num(views)
        out = {}
        if self.arm == "cpu":
            oracle.set_fixed_frames(np.ones(len(V), np.uint8))
            try:
                for k in points:
                    m = (self.pt == k) & registered[self.fr]
                    pa = capi.ProblemArrays(*(a[m] for a in self.obs), np.zeros(int(m.sum()), np.uint32), self.fr[m], self.cam, V, pts[k].copy(),
                                            self.spx, self.scale, (self.config & MODEL_BITS) | 0x500, spy=self.spy, fixed_mask=0x1FFFF)
                    c0 = oracle.cost(pa)
                    if not np.isfinite(c0):
                        out[k] = (c0, 0, 0)
                        continue
                    s = oracle.solve(pa, self.options)
                    pts[k] = pa.pts
                    out[k] = (s.final_cost, s.iterations, s.termination)
            finally:
                oracle.set_fixed_frames(None)
            return out
        from lifcal_amd import intersectPoints
        points = np.asarray(points)
        m = np.isin(self.pt, points) & registered[self.fr]
        local = np.zeros(int(self.pt.max()) + 1, np.uint32); local[points] = np.arange(len(points))
        res = intersectPoints(self.cam, V, *(a[m] for a in self.obs), local[self.pt[m]], self.fr[m], pts[points], self.config, self.spx, self.scale, spy=self.spy, options=self.options)
        pts[points] = res.pts
        for j, k in enumerate(points):
            out[int(k)] = (float(res.final_cost[j]), int(res.iterations[j]), int(res.termination[j]))
        return out


def register(arm, cam, u, v, mcx, mcy, pt, fr, n_frames, n_points, config, spx, scale, gate_px=1.0, min_shared=6, anchor_frame=-1, anchor_view=None,
             max_rounds=0, options=None, spy=None):
    """the chain; returns a namespace with views (F, 6) and pts (P, 3) (NaN where not written), the group table, per frame status,
    round, n_obs, n_obs_used, n_groups, n_used, n_shared and last (final_cost, iterations, termination), per point status, round,
    n_obs, n_obs_used, n_frames_used and last, and anchor_frame, n_rounds"""
    u, v, mcx, mcy = (np.asarray(a, np.float64) for a in (u, v, mcx, mcy))
    pt, fr = np.asarray(pt, np.int64), np.asarray(fr, np.int64)
    F, P = int(n_frames), int(n_points)
    out = types.SimpleNamespace(views=np.full((F, 6), np.nan), pts=np.full((P, 3), np.nan), anchor_frame=-1, n_rounds=0)
    out.f_n_obs, out.p_n_obs = np.bincount(fr, minlength=F), np.bincount(pt, minlength=P)
    out.f_status, out.f_round = np.where(out.f_n_obs > 0, 2, 1), np.full(F, -1)
    out.p_status, out.p_round = np.where(out.p_n_obs > 0, 2, 1), np.full(P, -1)
    out.f_n_shared, out.f_last, out.p_last = np.zeros(F, np.int64), {}, {}
    out.groups = groups = _groups(arm, cam, u, v, mcx, mcy, pt, fr, F, P, config, spx, scale, gate_px, spy) if len(u) else np.zeros(0, capi.START_GROUP_DTYPE)
    used = groups[groups["status"] == 0]           # (ascending (fr, pt) order)
    out.f_n_groups, out.f_n_used = np.bincount(groups["fr"], minlength=F), np.bincount(used["fr"], minlength=F)
    registered, mapped = np.zeros(F, bool), np.zeros(P, bool)
    out.registered, out.mapped = registered, mapped

    def finish():
        for f in np.flatnonzero(out.f_round <= 0):
            out.f_n_shared[f] = int(np.sum((used["fr"] == f) & mapped[used["pt"]]))
        out.f_n_obs_used = np.array([int(np.sum((fr == f) & mapped[pt])) if registered[f] else 0 for f in range(F)], np.int64)
        out.p_n_obs_used = np.array([int(np.sum((pt == k) & registered[fr])) if mapped[k] else 0 for k in range(P)], np.int64)
        out.p_n_frames_used = np.array([len(np.unique(fr[(pt == k) & registered[fr]])) if mapped[k] else 0 for k in range(P)], np.int64)
        return out

    if len(used) == 0:
        return finish()
    solver = _Solver(arm, np.asarray(cam, np.float64), u, v, mcx, mcy, pt, fr, config, spx, scale, options, spy)
    views, pts = out.views, out.pts

    def extend(r):
        R, t = euler_xyz(np.nan_to_num(views[:, :3])), views[:, 3:]
        g = used[registered[used["fr"]] & ~mapped[used["pt"]]]
        for k in np.unique(g["pt"]):
            gk = g[g["pt"] == k]               # (ascending frame order)
            w = 1.0 / gk["xyz"][:, 2] ** 2
            Pw = np.einsum("nji,nj->ni", R[gk["fr"]], gk["xyz"] - t[gk["fr"]])
            pts[k] = (w[:, None] * Pw).sum(0) / w.sum()
            mapped[k] = True; out.p_status[k] = 0; out.p_round[k] = r

    def refine_points():
        out.p_last.update(solver.points(np.flatnonzero(mapped), views, pts, registered))

    a = int(np.argmax(out.f_n_used)) if anchor_frame < 0 else int(anchor_frame)   # (argmax: the lowest index on ties)
    out.anchor_frame = a
    views[a] = np.zeros(6) if anchor_view is None else np.asarray(anchor_view, np.float64)
    registered[a] = True; out.f_status[a] = 0; out.f_round[a] = 0; out.f_last[a] = (0.0, 0, 0)
    extend(0); refine_points()
    r = 1
    while max_rounds == 0 or r <= max_rounds:
        new = []
        for f in np.flatnonzero(~registered & (out.f_n_groups > 0)):
            sel = used[(used["fr"] == f) & mapped[used["pt"]]]
            out.f_n_shared[f] = len(sel)
            if len(sel) < min_shared:
                continue
            al = sr.align(pts[sel["pt"]], sel["xyz"], 1.0 / sel["xyz"][:, 2] ** 2)
            if al.status == 0:
                views[f] = al.view; new.append(int(f))
            else:
                out.f_status[f] = 3            # (tried again in the next round)
        if not new:
            break
        out.f_last.update(solver.poses(new, views, pts, mapped))
        registered[new] = True; out.f_status[new] = 0; out.f_round[new] = r
        out.n_rounds = r
        extend(r); refine_points()
        out.f_last.update(solver.poses([int(f) for f in np.flatnonzero(registered) if f != a], views, pts, mapped))
        r += 1
    return finish()


def registered_part(views, pts, registered, mapped, u, v, mcx, mcy, pt, fr):
    """the observations of mapped points in registered frames with frames and points renumbered from 0: what a bundle adjustment
    started from a registration works on.  Returns (u, v, mcx, mcy, pt, fr), views (F', 6), pts (P', 3) and the kept observations."""
    pt, fr = np.asarray(pt, np.int64), np.asarray(fr, np.int64)
    m = registered[fr] & mapped[pt]
    fmap, pmap = np.cumsum(registered) - 1, np.cumsum(mapped) - 1
    obs = tuple(np.asarray(a)[m] for a in (u, v, mcx, mcy)) + (pmap[pt[m]].astype(np.uint32), fmap[fr[m]].astype(np.uint32))
    return obs, np.asarray(views).reshape(-1, 6)[registered], np.asarray(pts).reshape(-1, 3)[mapped], m


def control_calls():
    """one resectFrames and one intersectPoints call on the scene r2_tan_robust from its perturbed start values, as byte arrays: the
    control that the two batch calls keep their arithmetic (tests/golden/register_control.npz holds what they gave before the masked
    instantiations of their kernels existed)"""
    from lifcal_amd import intersectPoints, resectFrames, scene
    sc = scene.make_scene(scene.SceneSpec(6, 40, None, 0x306, 115, outlier_fraction=0.05))
    obs = (sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr)
    a = resectFrames(sc.cam_gt, sc.pts_gt, *obs, sc.views0, sc.config, sc.spx, sc.scale)
    b = intersectPoints(sc.cam_gt, sc.views_gt, *obs, sc.pts0, sc.config, sc.spx, sc.scale)
    as_bytes = lambda x: np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8)
    return {"resect_views": as_bytes(a.views), "resect_rows": as_bytes(a.rows), "intersect_pts": as_bytes(b.pts), "intersect_rows": as_bytes(b.rows)}
