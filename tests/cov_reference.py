"""Dense numpy restatement of the covariance algebra of lifcal_ba_covariance, on a reduced matrix it is given.

The matrix is the undamped reduced system in the canonical order of the C ABI: [camera 0..16 | poses 6F | promoted points 3Q].
Dead columns (fixed / structurally absent camera slots, constant or unobserved poses) are named by the `live` mask; their rows and
columns of the result are zero.  The gauge frame, if any, is removed from the pose columns before the algebra.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

NCAM = 17


def n_camera_slots(config: int) -> int:
    """live camera slots of a configuration: fL, bL0, B, cx, cy + radial + 2 tangential"""
    return 5 + min(config & 3, 2) + (2 if config & 4 else 0)


def live_mask(config, fixed_mask, n_frames, n_promoted, frame_used=None, fixed_frames=None):
    """canonical live mask of the reduced system of a problem"""
    nc = n_camera_slots(config)
    cam = np.array([j < nc and not (fixed_mask >> j) & 1 for j in range(NCAM)], bool)
    poses = bool(config & 0x100)
    fr = np.full(n_frames, poses, bool)
    if frame_used is not None:
        fr &= np.asarray(frame_used, bool)
    if fixed_frames is not None:
        fr &= ~np.asarray(fixed_frames, bool)
    return np.concatenate([cam, np.repeat(fr, 6), np.ones(3 * n_promoted, bool)])


@dataclass
class CovRef:
    G: np.ndarray              # n x n g-inverse of H, canonical order, zero on dead columns and on the gauge frame
    camera: np.ndarray         # 17 x 17
    poses: np.ndarray          # F x 6 x 6
    null_rank: int             # null directions of the arrow Schur complement C (after the gauge frame)
    estimable: np.ndarray      # 17 bools
    camera_null: np.ndarray    # null_rank x 17: camera components of the null directions (parameter units, unit length)
    C: np.ndarray              # arrow Schur complement on the live arrow slots
    eig: np.ndarray            # eigenvalues of the Jacobi-scaled C, ascending


def covariance(S, live, n_frames, gauge_frame=-1, null_rcond=1e-11, estimable_tol=1e-6):
    S = np.asarray(S, float)
    n = S.shape[0]
    live = np.asarray(live, bool).copy()
    if gauge_frame >= 0:
        live[NCAM + 6 * gauge_frame: NCAM + 6 * gauge_frame + 6] = False
    idx = np.arange(n)
    pose = (idx >= NCAM) & (idx < NCAM + 6 * n_frames)
    f = idx[live & pose]
    a = idx[live & ~pose]
    A = S[np.ix_(f, f)]
    B = S[np.ix_(f, a)]
    D = S[np.ix_(a, a)]
    if len(f):
        np.linalg.cholesky(A)   # S_ff must be positive definite once the gauge frame is held
        Ainv = np.linalg.inv(A)
        Y = np.linalg.solve(A, B)
    else:
        Ainv = np.zeros((0, 0)); Y = np.zeros((0, len(a)))
    C = D - B.T @ Y
    C = 0.5 * (C + C.T)
    d = np.sqrt(np.maximum(np.diag(C), 0.0))
    d[d == 0] = 1.0
    w, V = np.linalg.eigh(C / np.outer(d, d))
    keep = w > null_rcond * max(w.max(), 0.0) if len(w) else np.zeros(0, bool)
    Cp = ((V[:, keep] / w[keep]) @ V[:, keep].T) / np.outer(d, d)
    G = np.zeros((n, n))
    G[np.ix_(a, a)] = Cp
    G[np.ix_(f, a)] = -Y @ Cp
    G[np.ix_(a, f)] = (-Y @ Cp).T
    G[np.ix_(f, f)] = Ainv + Y @ Cp @ Y.T
    Vn = V[:, ~keep]
    cam_pos = a < NCAM
    estimable = np.zeros(NCAM, bool)
    for k, j in enumerate(a):
        if j < NCAM:
            estimable[j] = np.all(np.abs(Vn[k]) <= estimable_tol)
    Vu = Vn / d[:, None]
    Vu = Vu / np.maximum(np.linalg.norm(Vu, axis=0), 1e-300)
    cam_null = np.zeros((Vn.shape[1], NCAM))
    cam_null[:, a[cam_pos]] = Vu[cam_pos].T
    poses = np.zeros((n_frames, 6, 6))
    for fr in range(n_frames):
        s = slice(NCAM + 6 * fr, NCAM + 6 * fr + 6)
        poses[fr] = G[s, s]
    return CovRef(G, G[:NCAM, :NCAM].copy(), poses, int((~keep).sum()), estimable, cam_null, C, np.sort(w))


def first_observed_frame(fr):
    return int(np.min(np.asarray(fr)))


def scaled_null_count(S, live, rcond):
    """eigenvalues of the Jacobi-scaled H on its live columns below rcond * max: the null space of the full system"""
    l = np.flatnonzero(live)
    H = S[np.ix_(l, l)]
    d = np.sqrt(np.abs(np.diag(H))); d[d == 0] = 1.0
    w = np.linalg.eigvalsh(H / np.outer(d, d))
    return int((w < rcond * w.max()).sum()), np.sort(w)
