"""The damped normal equations of one Levenberg-Marquardt step, matrix-free, in long double (numpy only): the reference the step of
every solver route is measured against (tests/test_gpu_step.py; pinned without a GPU by tests/test_step_reference_cpu.py).

Per scalar residual one sparse row of the Jacobian is kept (camera 17 | its pose 6 | its point 3), built exactly as
tests/test_oracle_schur.py::dense_system builds its dense rows: oracle.residual_block (arity 3), the sqrt(rho') weighting of the
Cauchy loss, oracle.constraint_block rows, and the columns the configuration does not refine zeroed.  With

    g = J^T r,  h = diag(J^T J),  sigma = 1 / (1 + sqrt(h))  (1 without Jacobi scaling),
    lambda = clip(h sigma^2, 1e-6, 1e32) / (radius sigma^2),        y(delta) = J^T (J delta) + lambda delta + g

the measure of a step is the row-wise backward error

    eta_i(delta) = |y_i| / ((|J|^T (|J| |delta|))_i + lambda_i |delta_i| + |g_i|)

over the live rows (h_i > 0): eta_B over camera, poses and promoted points, eta_P over the eliminated points.  Column order of
every full vector: camera 17 | 6 F poses | 3 P points.
"""
import ctypes as C

import numpy as np

import oracle

LD = np.longdouble
EPS = 2.0 ** -53


def _residual_blocks(pa):
    """r [N, 2] and J [N, 2, 26] of every observation at the parameters of `pa` (one oracle call per observation, on raw addresses)"""
    L = C.CDLL(oracle.build())   # (a handle of its own: oracle.lib() keeps the typed prototype)
    fn = L.lo_residual_block
    vp, d = C.c_void_p, C.c_double
    fn.argtypes = [C.c_uint32, C.c_int, vp, vp, vp, d, d, d, d, d, d, d, vp, vp]
    fn.restype = C.c_int
    N = int(pa.struct.n_obs)
    R = np.zeros((N, 2)); J = np.zeros((N, 2, 26))
    cam, vb, pb, rb, jb = pa.cam.ctypes.data, pa.views.ctypes.data, pa.pts.ctypes.data, R.ctypes.data, J.ctypes.data
    cfg, spx, spy, scale = int(pa.struct.config), pa.struct.spx, pa.struct.spy, pa.struct.scale
    u, v, mcx, mcy, fr, pt = (a.tolist() for a in (pa.u, pa.v, pa.mcx, pa.mcy, pa.fr, pa.pt))
    for i in range(N):
        rc = fn(cfg, 3, cam, vb + 48 * fr[i], pb + 24 * pt[i], u[i], v[i], mcx[i], mcy[i], spx, spy, scale, rb + 16 * i, jb + 416 * i)
        assert rc == 0
    return R, J


class NormalEquations:
    """J, r, g, h, lambda of the problem `pa` at its own parameters and the given radius."""

    def __init__(self, pa, radius, jacobi_scaling=True, fixed_frames=None, loss_scale=0.5, lm_min=1e-6, lm_max=1e32):
        st = pa.struct
        F, P, N = int(st.n_frames), int(st.n_points), int(st.n_obs)
        cfg = int(st.config)
        self.F, self.P, self.N, self.n = F, P, N, 17 + 6 * F + 3 * P
        self.nb = 17 + 6 * F
        self.radius = float(radius)
        self.refine_poses = bool(cfg & 0x100)
        self.refine_points = self.refine_poses and bool(cfg & 0x400)   # the reference's functor arities: points only with poses
        self.n_cam = 5 + (cfg & 3) + (2 if cfg & 4 else 0)             # structurally present camera slots
        self.fixed_mask = int(st.fixed_mask)
        self.fixed_frames = np.zeros(F, bool) if fixed_frames is None else np.asarray(fixed_frames, bool).copy()
        R, J = _residual_blocks(pa)
        cost = 0.0
        if cfg & 0x200:
            b = loss_scale ** 2
            s = np.sum(R * R, 1)
            cost = float(np.sum(0.5 * b * np.log1p(s / b)))
            w = np.sqrt(1.0 / (1.0 + s / b))
            R = R * w[:, None]; J = J * w[:, None, None]
        else:
            cost = float(0.5 * np.sum(R * R))
        self.fr = np.repeat(pa.fr.astype(np.int64), 2); self.pt = np.repeat(pa.pt.astype(np.int64), 2)
        self.r = R.reshape(-1).astype(LD)
        J = J.reshape(2 * N, 26)
        Jc, Jv, Jp = J[:, :17].copy(), J[:, 17:23].copy(), J[:, 23:].copy()
        # distance constraints: one row each over the two points
        self.constrained = bool(self.refine_points and st.use_constraints and st.n_constraints)
        M = int(st.n_constraints) if self.constrained else 0
        self.ci = pa.c_i[:M].astype(np.int64) if M else np.zeros(0, np.int64)
        self.cj = pa.c_j[:M].astype(np.int64) if M else np.zeros(0, np.int64)
        Ci = np.zeros((M, 3)); Cj = np.zeros((M, 3)); rc = np.zeros(M)
        for c in range(M):
            i, j = int(self.ci[c]), int(self.cj[c])
            rr, JJ = oracle.constraint_block(pa.pts[3 * i:3 * i + 3], pa.pts[3 * j:3 * j + 3], pa.c_dist[c], pa.c_sigma[c])
            Ci[c], Cj[c], rc[c] = JJ[:3], JJ[3:], rr
            cost += 0.5 * rr * rr
        self.rc = rc.astype(LD)
        self.cost = cost
        self.promoted = sorted(set(int(j) for j in self.cj))   # the second point of a constraint stays in the reduced system
        # columns that are not refined
        for k in range(17):
            if (self.fixed_mask >> k) & 1:
                Jc[:, k] = 0.0
        if not self.refine_poses:
            Jv[:] = 0.0
        else:
            Jv[self.fixed_frames[self.fr]] = 0.0
        if not self.refine_points:
            Jp[:] = 0.0
        self._A = tuple(a.astype(LD) for a in (Jc, Jv, Jp, Ci, Cj))
        self._absA = tuple(np.abs(a) for a in self._A)
        self.g = self._JT(self.r, self.rc, self._A)
        one_r, one_c = np.ones(2 * N, LD), np.ones(M, LD)
        self.h = self._JT(one_r, one_c, tuple(a * a for a in self._A))
        self.live = np.asarray(self.h > 0)
        hs = self.h.astype(np.float64)
        self.sigma = 1.0 / (1.0 + np.sqrt(hs)) if jacobi_scaling else np.ones(self.n)
        self._lm = (lm_min, lm_max)
        self.set_radius(radius)
        # row classes
        self.rows_B = np.zeros(self.n, bool); self.rows_B[:self.nb] = True
        for q in self.promoted:
            self.rows_B[self.nb + 3 * q:self.nb + 3 * q + 3] = True
        self.rows_P = ~self.rows_B
        self.observed_points = np.zeros(P, bool); self.observed_points[np.unique(pa.pt)] = True
        if M:
            self.observed_points[self.ci] = True; self.observed_points[self.cj] = True

    def set_radius(self, radius):
        """the same Jacobian at another trust-region radius (only lambda depends on it)"""
        self.radius = float(radius)
        hs, sig = self.h.astype(np.float64), self.sigma
        self.lam = np.where(self.live, np.clip(hs * sig * sig, *self._lm) / (self.radius * sig * sig), 0.0).astype(LD)
        return self

    # ---- products ----------------------------------------------------------------------------------------------------------------
    def _J(self, x, A):
        Jc, Jv, Jp, Ci, Cj = A
        F, P = self.F, self.P
        xc = x[:17]; xv = x[17:self.nb].reshape(F, 6); xp = x[self.nb:].reshape(P, 3)
        t = Jc @ xc + np.sum(Jv * xv[self.fr], 1) + np.sum(Jp * xp[self.pt], 1)
        tc = np.sum(Ci * xp[self.ci], 1) + np.sum(Cj * xp[self.cj], 1)
        return t, tc

    def _JT(self, t, tc, A):
        Jc, Jv, Jp, Ci, Cj = A
        F, P = self.F, self.P
        out = np.zeros(self.n, LD)
        out[:17] = Jc.T @ t
        ov = np.zeros((F, 6), LD); op = np.zeros((P, 3), LD)
        np.add.at(ov, self.fr, Jv * t[:, None])
        np.add.at(op, self.pt, Jp * t[:, None])
        if len(tc):
            np.add.at(op, self.ci, Ci * tc[:, None]); np.add.at(op, self.cj, Cj * tc[:, None])
        out[17:self.nb] = ov.reshape(-1); out[self.nb:] = op.reshape(-1)
        return out

    def JtJ(self, x, absolute=False):
        """J^T (J x), or |J|^T (|J| x)"""
        A = self._absA if absolute else self._A
        return self._JT(*self._J(np.asarray(x, LD), A), A)

    def y(self, delta):
        d = np.asarray(delta, LD)
        return self.JtJ(d) + self.lam * d + self.g

    # ---- the measure -------------------------------------------------------------------------------------------------------------
    def eta_rows(self, delta):
        """eta_i of every row; NaN on the dead rows"""
        d = np.asarray(delta, LD)
        num = np.abs(self.y(d))
        den = self.JtJ(np.abs(d), absolute=True) + self.lam * np.abs(d) + np.abs(self.g)
        out = np.full(self.n, np.nan)
        ok = self.live & np.asarray(den > 0)
        out[ok] = (num[ok] / den[ok]).astype(np.float64)
        assert not np.any(self.live & ~ok), "a live row with an empty denominator"
        return out

    def eta(self, delta):
        """(eta_B, eta_P): the maxima over the live rows of the reduced part and of the eliminated points (0.0 where there is none)"""
        e = self.eta_rows(delta)
        mx = lambda m: float(np.max(e[m])) if np.any(m) else 0.0
        return mx(self.rows_B & self.live), mx(self.rows_P & self.live)

    # ---- which rows are left out ---------------------------------------------------------------------------------------------------
    def expected_dead(self):
        """the number of dead columns by the list of their causes: structurally absent camera slots, fixed_mask slots, constant
        frames (all of them when poses are not refined), point blocks that are not refined, unobserved points"""
        n = 17 - self.n_cam
        n += bin(self.fixed_mask & ((1 << self.n_cam) - 1)).count("1")
        n += 6 * (int(np.sum(self.fixed_frames)) if self.refine_poses else self.F)
        n += 3 * (int(np.sum(~self.observed_points)) if self.refine_points else self.P)
        return n

    def check_dead_rows(self):
        dead = int(np.sum(~self.live))
        assert dead == self.expected_dead(), (dead, self.expected_dead())
        return dead

    # ---- vectors in the canonical reduced order (camera 17 | poses | promoted points ascending) ------------------------------------
    def split(self, delta_reduced, delta_points):
        """full step from the reduced step in canonical order and the 3P point steps (promoted points: the reduced entries win)"""
        x = np.zeros(self.n, LD)
        x[:self.nb] = delta_reduced[:self.nb]
        x[self.nb:] = np.asarray(delta_points, LD)
        for k, q in enumerate(self.promoted):
            x[self.nb + 3 * q:self.nb + 3 * q + 3] = delta_reduced[self.nb + 3 * k:self.nb + 3 * k + 3]
        return x

    def reduced(self, full):
        out = np.zeros(self.nb + 3 * len(self.promoted), full.dtype)
        out[:self.nb] = full[:self.nb]
        for k, q in enumerate(self.promoted):
            out[self.nb + 3 * k:self.nb + 3 * k + 3] = full[self.nb + 3 * q:self.nb + 3 * q + 3]
        return out


def oracle_sweep(pa, radius, options=None, fixed_frames=None):
    """the oracle's reduced system for `pa` (oracle.sweep; the constant frames are process-wide state of the oracle: set and cleared here)"""
    try:
        if fixed_frames is not None:
            oracle.set_fixed_frames(np.asarray(fixed_frames, np.uint8))
        sw = oracle.sweep(pa, radius=radius, options=options, threads=4)
    finally:
        if fixed_frames is not None:
            oracle.set_fixed_frames(None)
    assert sw.rc == 0
    return sw


def reference_step(ne, sw):
    """The CPU reference step from the oracle's sweep `sw`: delta_B = solve(S, rhs) and, for every eliminated point,
    delta_p = -Uinv (g_p + (J^T J delta)_p) with delta zero on the eliminated points.  Returns the full step (long double)."""
    assert sw.n_promoted == len(ne.promoted), (sw.n_promoted, len(ne.promoted))
    dB = np.linalg.solve(sw.S, sw.rhs)
    x = ne.split(dB, np.zeros(3 * ne.P))
    yp = (ne.g + ne.JtJ(x))[ne.nb:].reshape(ne.P, 3)
    Ui = np.asarray(sw.point_hessian_inv, LD).reshape(ne.P, 3, 3)
    dp = -np.einsum("pij,pj->pi", Ui, yp)
    elim = ne.rows_P[ne.nb:].reshape(ne.P, 3)[:, 0] & ne.live[ne.nb:].reshape(ne.P, 3)[:, 0]
    dp[~elim] = 0.0
    return ne.split(dB, dp.reshape(-1))


def solve_eta(S, rhs, delta):
    """row-wise backward error of delta as a solution of S delta = rhs: |S delta - rhs|_i / ((|S| |delta|)_i + |rhs_i|), maximum over the
    rows whose denominator is not zero (an identity row with zero right-hand side and zero solution has none)"""
    Sl = np.asarray(S, LD); d = np.asarray(delta, LD); b = np.asarray(rhs, LD)
    num = np.abs(Sl @ d - b)
    den = np.abs(Sl) @ np.abs(d) + np.abs(b)
    ok = np.asarray(den > 0)
    assert not np.any(num[~ok] > 0)
    return float(np.max(num[ok] / den[ok])) if np.any(ok) else 0.0
