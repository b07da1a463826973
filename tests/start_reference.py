"""numpy restatement of the closed-form start values (include/lifcal_start.h): the two rows of an
observation, the triangulation of a group, the gate, the weighted alignment in two arms (SVD-Kabsch and Horn's quaternion through
numpy's eigh), the Euler extraction and the triangulation of a point in the world frame.  Written from the formulas of the section,
not from the kernels: no fused multiply-adds, numpy's own summation order, LAPACK for every factorisation."""
import types

import numpy as np

from lifcal_amd import _capi as capi
from lifcal_amd.scene import euler_xyz

CFG_TAN, CFG_ADJ = 0x004, 0x800
EPS = float(np.finfo(np.float64).eps)


def cam_consts(cam, config, spx, spy, scale, fold=True):
    """the camera-only quantities (CamConsts of device_model.hpp); fold: signs folded as the solver does, else as stored with the
    scale through float (calcReprojectionError's rule)"""
    cam = np.asarray(cam, np.float64)
    nr = config & 3
    tan = bool(config & CFG_TAN)
    sc = float(scale) if fold else float(np.float32(scale))
    th = np.abs(cam[:3]) if fold else cam[:3]
    craw = (cam[3:5] + 0.5) * sc - 0.5
    if fold:
        craw = np.abs(craw)
    c = types.SimpleNamespace(nr=nr, tan=tan, adj=bool(config & CFG_ADJ))
    c.fL, c.bL0, c.B = (float(x) for x in th)
    c.craw = craw
    c.sp = np.array([spx / sc, spy / sc])
    D = c.fL - c.bL0
    c.e, c.zC0, c.gamma, c.beta = c.fL / D, c.fL * c.bL0 / D, c.fL * c.B / D, c.B / D
    c.a = c.bL0 / (c.bL0 + c.B)
    c.k = [cam[5] if nr > 0 else 0.0, cam[6] if nr > 1 else 0.0]
    c.p = [cam[5 + nr], cam[6 + nr]] if tan else [0.0, 0.0]
    return c


def distortion(c, x):
    """Delta(x) of an (n, 2) array (Distortion<NR, TAN>::eval, values only)"""
    r2 = np.sum(x * x, -1)
    g = c.k[0] * r2 + c.k[1] * r2 * r2
    d = x * g[:, None]
    if c.tan:
        xy = x[:, 0] * x[:, 1]
        d = d + np.stack([c.p[0] * (r2 + 2.0 * x[:, 0] ** 2) + 2.0 * c.p[1] * xy, c.p[1] * (r2 + 2.0 * x[:, 1] ** 2) + 2.0 * c.p[0] * xy], -1)
    return d


def undistort(c, y):
    """the solution of x + Delta(x) = y by ten fixed-point sweeps from x = y (none without distortion), as lens_eval"""
    x = y.copy()
    if c.nr > 0 or c.tan:
        for _ in range(10):
            x = y - distortion(c, x)
    return x


def rays(c, u, v, mcx, mcy):
    """A (n, 2, 3), b (n, 2): the two rows of every observation, A p_c = b for the camera-frame point p_c"""
    uv, m = np.stack([u, v], -1).astype(np.float64), np.stack([mcx, mcy], -1).astype(np.float64)
    cu = undistort(c, (m - c.craw) * c.sp)
    w = cu * c.a if c.adj else cu
    if c.adj:
        ml = undistort(c, (uv - c.craw) * c.sp) - w
    else:
        ml = (uv - m) * c.sp
    s = ml + c.beta * w
    A = np.zeros((len(uv), 2, 3))
    A[:, 0, 0] = c.gamma / c.sp[0]; A[:, 1, 1] = c.gamma / c.sp[1]
    A[:, :, 2] = -s / c.sp
    b = (s * c.zC0 - c.gamma * c.e * w) / c.sp
    return A, b


def solve_scaled(H, g):
    """x of H x = g through the Jacobi-scaled matrix d H d (unit diagonal) and its Cholesky factor; returns x, ok, the scaled
    matrix and its smallest pivot"""
    with np.errstate(all="ignore"):
        d = 1.0 / np.sqrt(np.diag(H))
        Hs = H * np.outer(d, d)
        if not np.all(np.isfinite(Hs)):
            return np.zeros(3), False, Hs, np.nan
        try:
            L = np.linalg.cholesky(Hs)
        except np.linalg.LinAlgError:
            return np.zeros(3), False, Hs, 0.0
        y = np.linalg.solve(L.T, np.linalg.solve(L, d * g))
        x = d * y
    return x, bool(np.all(np.isfinite(x))), Hs, float(np.min(np.diag(L)) ** 2)


def group_rows(cam, u, v, mcx, mcy, pt, fr, config, spx, scale, spy=None, gate_px=1.0):
    """the group table (capi.START_GROUP_DTYPE) in ascending (fr, pt) order, the observations of a group in the order given, and the
    condition number of every group's scaled matrix (NaN where it was not formed)"""
    c = cam_consts(cam, config, spx, spx if spy is None else spy, scale)
    A, b = rays(c, u, v, mcx, mcy)
    order = np.lexsort((np.arange(len(pt)), pt, fr))   # (fr, pt)-major, stable
    key = np.stack([np.asarray(fr)[order], np.asarray(pt)[order]], -1).astype(np.int64)
    cuts = np.concatenate([[0], np.flatnonzero(np.any(np.diff(key, axis=0) != 0, axis=1)) + 1, [len(order)]]) if len(order) else np.zeros(1, np.int64)
    rows = np.zeros(len(cuts) - 1, capi.START_GROUP_DTYPE)
    cond = np.full(len(rows), np.nan)
    for g in range(len(rows)):
        idx = order[cuts[g]:cuts[g + 1]]
        rows["fr"][g], rows["pt"][g], rows["n_obs"][g] = key[cuts[g], 0], key[cuts[g], 1], len(idx)
        if len(idx) == 1:
            rows["status"][g] = 1
            continue
        Ag, bg = A[idx].reshape(-1, 3), b[idx].reshape(-1)
        x, ok, Hs, _ = solve_scaled(Ag.T @ Ag, Ag.T @ bg)
        if not ok:
            rows["status"][g] = 2
            continue
        cond[g] = np.linalg.cond(Hs)
        rho = (Ag @ x - bg) / (x[2] + c.zC0)
        rms = float(np.sqrt(np.sum(rho * rho) / len(idx)))
        rows["xyz"][g], rows["rms_px"][g] = x, rms
        rows["status"][g] = 3 if x[2] <= 0.0 else (4 if rms > gate_px else 0)
    return rows, cond


def euler_from_R(R):
    """the XYZ angles of frame_eval's R = Rx Ry Rz"""
    a1 = np.arcsin(np.clip(R[0, 2], -1.0, 1.0))
    if 1.0 - abs(R[0, 2]) < 1e-12:
        return np.array([np.arctan2(R[2, 1], R[1, 1]), a1, 0.0])
    return np.array([np.arctan2(-R[1, 2], R[2, 2]), a1, np.arctan2(-R[0, 1], R[0, 0])])


def horn_matrix(M):
    """Horn's symmetric 4x4 matrix of the moment M = sum w (P - Pm)(p_c - cm)^T: its largest eigenvector is the quaternion of the
    rotation that carries the world points onto the camera-frame points"""
    (Sxx, Sxy, Sxz), (Syx, Syy, Syz), (Szx, Szy, Szz) = M
    return np.array([[Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx],
                     [Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz],
                     [Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy],
                     [Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz]])


def quat_R(q):
    q0, qx, qy, qz = q / np.linalg.norm(q)
    return np.array([[q0 * q0 + qx * qx - qy * qy - qz * qz, 2 * (qx * qy - q0 * qz), 2 * (qx * qz + q0 * qy)],
                     [2 * (qy * qx + q0 * qz), q0 * q0 - qx * qx + qy * qy - qz * qz, 2 * (qy * qz - q0 * qx)],
                     [2 * (qz * qx - q0 * qy), 2 * (qz * qy + q0 * qx), q0 * q0 - qx * qx - qy * qy + qz * qz]])


def align(P, pc, w, arm="horn"):
    """the weighted rigid alignment R P + t ~ p_c; returns a namespace with view (6), R, t, sum_w, align_rms, eig (the two largest
    eigenvalues of Horn's matrix) and status (0, or 3: degenerate)"""
    sw = float(np.sum(w))
    Pm, cm = (w[:, None] * P).sum(0) / sw, (w[:, None] * pc).sum(0) / sw
    M = np.einsum("n,ni,nj->ij", w, P - Pm, pc - cm)
    lam, V = np.linalg.eigh(horn_matrix(M))
    out = types.SimpleNamespace(sum_w=sw, eig=np.array([lam[3], lam[2]]), status=0, view=None, R=None, t=None, align_rms=0.0)
    if not (lam[3] - lam[2] > 1e-9 * abs(lam[3])):
        out.status = 3
        return out
    if arm == "horn":
        R = quat_R(V[:, 3])
    else:   # Kabsch: M = U S V^T, R = V diag(1, 1, det) U^T
        U, _, Vt = np.linalg.svd(M)
        R = Vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))]) @ U.T
    ang = euler_from_R(R)
    t = cm - R @ Pm
    out.view = np.concatenate([ang, t])
    out.R, out.t = euler_xyz(ang), t
    d = P @ out.R.T + t - pc
    out.align_rms = float(np.sqrt(np.sum(w * np.sum(d * d, -1)) / sw))
    return out


def poses_from_groups(groups, pts, n_frames, arm="horn"):
    """per frame the alignment over its used groups, weight 1 / Z_c^2; returns views (F, 6) (NaN where no pose exists), and the
    lists status, n_groups, n_used and the align namespaces (None where none was made)"""
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    views = np.full((n_frames, 6), np.nan)
    status, n_groups, n_used, info = [], [], [], []
    for f in range(n_frames):
        g = groups[groups["fr"] == f]
        used = g[g["status"] == 0]
        n_groups.append(len(g)); n_used.append(len(used)); info.append(None)
        if len(g) == 0:
            status.append(1)
        elif len(used) < 3:
            status.append(2)
        else:
            pc = used["xyz"]
            al = align(pts[used["pt"]], pc, 1.0 / pc[:, 2] ** 2, arm)
            info[-1] = al
            status.append(al.status)
            if al.status == 0:
                views[f] = al.view
    return views, status, n_groups, n_used, info


def start_poses(cam, pts, u, v, mcx, mcy, pt, fr, n_frames, config, spx, scale, spy=None, gate_px=1.0, arm="horn"):
    groups, cond = group_rows(cam, u, v, mcx, mcy, pt, fr, config, spx, scale, spy, gate_px)
    views, status, n_groups, n_used, info = poses_from_groups(groups, pts, n_frames, arm)
    return types.SimpleNamespace(views=views, status=np.array(status), n_groups=np.array(n_groups), n_used=np.array(n_used), info=info, groups=groups, cond=cond)


def start_points(cam, views, u, v, mcx, mcy, pt, fr, n_points, config, spx, scale, spy=None):
    """per point the rows of all its observations carried into the world frame (A_w = A R_f, b_w = b - A t_f) and their scaled
    Cholesky solution; returns pts (P, 3) (NaN where none exists), status, cond and min_pivot"""
    c = cam_consts(cam, config, spx, spx if spy is None else spy, scale)
    A, b = rays(c, u, v, mcx, mcy)
    views = np.asarray(views, np.float64).reshape(-1, 6)
    R, t = euler_xyz(views[:, :3]), views[:, 3:]
    fr = np.asarray(fr, np.int64)
    Aw = np.einsum("nij,njk->nik", A, R[fr]) if len(fr) else A
    bw = b - np.einsum("nij,nj->ni", A, t[fr]) if len(fr) else b
    pts = np.full((n_points, 3), np.nan)
    status, cond, piv = np.zeros(n_points, np.int32), np.full(n_points, np.nan), np.zeros(n_points)
    for k in range(n_points):
        idx = np.flatnonzero(np.asarray(pt) == k)
        if len(idx) < 2:
            status[k] = 1 if len(idx) == 0 else 2
            continue
        Ak, bk = Aw[idx].reshape(-1, 3), bw[idx].reshape(-1)
        x, ok, Hs, piv[k] = solve_scaled(Ak.T @ Ak, Ak.T @ bk)
        if not ok:
            status[k] = 3
            continue
        cond[k] = np.linalg.cond(Hs)
        zq = (R[fr[idx]] @ x)[:, 2] + t[fr[idx], 2] + c.zC0
        if np.any(zq <= 0.0):
            status[k] = 4
            continue
        pts[k] = x
    return types.SimpleNamespace(pts=pts, status=status, cond=cond, min_pivot=piv)
