"""Gaussian priors on camera and poses (include/lifcal_prior.h), the references the tests measure against (numpy only).

The oracle has no priors.  What it gives is combined here with the analytic terms of 1/2 d^T Lambda d, d = x - mean:

  embed()              Lambda in the canonical reduced order [camera 17 | views 6 F | promoted points] of lifcal_ba_sweep_out
  live_slots()         which of these slots are free parameters (the others leave the term, rows and columns)
  PriorEquations       tests/step_reference.NormalEquations with the rows Lambda_LL^(1/2) appended to J and Lambda_LL^(1/2) d to r:
                       Ceres' view of one extra residual block per prior, without a loss
  dense_reduced()      the dense Schur complement of such equations (small scenes)
"""
import numpy as np

from tests import step_reference as sr

LD = sr.LD


def embed(n_frames, n_promoted=0, camera=None, poses=None):
    """Lambda [n, n] and mean [n], n = 17 + 6 F + 3 Q; camera = (mean[17], info[17, 17]), poses = (frames, means[k, 6], infos[k, 6, 6])"""
    n = 17 + 6 * n_frames + 3 * n_promoted
    Lam = np.zeros((n, n)); mean = np.zeros(n)
    if camera is not None:
        A = np.asarray(camera[1], np.float64).reshape(17, 17)
        Lam[:17, :17] = 0.5 * (A + A.T); mean[:17] = np.asarray(camera[0], np.float64).reshape(17)
    if poses is not None:
        frames = np.asarray(poses[0]).reshape(-1)
        means = np.asarray(poses[1], np.float64).reshape(len(frames), 6); infos = np.asarray(poses[2], np.float64).reshape(len(frames), 6, 6)
        for k, f in enumerate(frames):
            a = 17 + 6 * int(f)
            Lam[a:a + 6, a:a + 6] = 0.5 * (infos[k] + infos[k].T); mean[a:a + 6] = means[k]
    return Lam, mean


def live_slots(config, fixed_mask, n_frames, n_promoted=0, fixed_frames=None):
    """bool [n]: camera slots that are structurally present and not in fixed_mask, poses that are refined and not held constant,
    promoted points"""
    n_cam = 5 + (config & 3) + (2 if config & 4 else 0)
    live = np.zeros(17 + 6 * n_frames + 3 * n_promoted, bool)
    for j in range(n_cam):
        live[j] = not ((fixed_mask >> j) & 1)
    ff = np.zeros(n_frames, bool) if fixed_frames is None else np.asarray(fixed_frames, bool)
    if config & 0x100:
        live[17:17 + 6 * n_frames] = np.repeat(~ff, 6)
    live[17 + 6 * n_frames:] = True
    return live


def masked(Lam, live):
    """Lambda_LL in place of Lambda: rows and columns of the slots that are not free zeroed"""
    return Lam * np.outer(live, live)


def prior_terms(Lam, mean, x, live):
    """(cost, Lambda_LL d) at the canonical reduced vector x (promoted entries of d are irrelevant: their rows of Lambda are zero)"""
    L = masked(Lam, live).astype(LD)
    d = np.asarray(x, LD) - np.asarray(mean, LD)
    Ld = L @ d
    return float(0.5 * d @ Ld), np.asarray(Ld, np.float64)


class PriorEquations(sr.NormalEquations):
    """The normal equations of `pa` with the prior rows appended: J <- [J; Lambda_LL^(1/2)], r <- [r; Lambda_LL^(1/2) d].
    Lam / mean: embed() over camera and poses (n_promoted = 0; the rows have no entries on points)."""

    def __init__(self, pa, radius, Lam, mean, jacobi_scaling=True, fixed_frames=None, **kw):
        super().__init__(pa, radius, jacobi_scaling=jacobi_scaling, fixed_frames=fixed_frames, **kw)
        nb = self.nb
        st = pa.struct
        live = live_slots(int(st.config), int(st.fixed_mask), self.F, 0, fixed_frames)
        LL = masked(np.asarray(Lam, np.float64)[:nb, :nb], live[:nb])
        # the square root through the unit-diagonal matrix (the slots have units twelve orders of magnitude apart: a plain eigh would
        # be exact to 1e-16 of the LARGEST entry only)
        dg = np.sqrt(np.where(np.diag(LL) > 0, np.diag(LL), 1.0))
        w, V = np.linalg.eigh(LL / np.outer(dg, dg))
        keep = w > 0
        rows = (np.sqrt(w[keep])[:, None] * V[:, keep].T) * dg[None, :]          # k x nb: rows^T rows = Lambda_LL
        self._L = rows.astype(LD); self._absL = np.abs(self._L)
        x = np.concatenate([pa.cam, pa.views]).astype(LD)
        self.r_prior = self._L @ (x - np.asarray(mean, LD)[:nb])
        self.cost_observations = self.cost
        self.cost_prior = float(0.5 * self.r_prior @ self.r_prior)
        self.cost = self.cost_observations + self.cost_prior
        self.g = self.g.copy(); self.g[:nb] += self._L.T @ self.r_prior
        self.h = self.h.copy(); self.h[:nb] += np.sum(self._L * self._L, 0)
        self.live = np.asarray(self.h > 0)
        hs = self.h.astype(np.float64)
        self.sigma = 1.0 / (1.0 + np.sqrt(hs)) if jacobi_scaling else np.ones(self.n)
        self.set_radius(radius)

    def JtJ(self, x, absolute=False):
        x = np.asarray(x, LD)
        out = super().JtJ(x, absolute)
        L = self._absL if absolute else self._L
        out[:self.nb] += L.T @ (L @ x[:self.nb])
        return out


def dense_reduced(ne):
    """(S, rhs) of the damped normal equations `ne` in the canonical reduced order, points that are not promoted eliminated:
    H = J^T J + diag(lambda) column by column, identity rows on the dead slots, S = H_BB - H_BP H_PP^-1 H_PB, rhs = -g_B + H_BP H_PP^-1 g_P"""
    n = ne.n
    H = np.zeros((n, n), LD)
    e = np.zeros(n, LD)
    for k in range(n):
        e[k] = 1.0
        H[:, k] = ne.JtJ(e)
        e[k] = 0.0
    H[np.arange(n), np.arange(n)] += ne.lam
    g = ne.g.copy()
    dead = ~ne.live
    H[dead, :] = 0.0; H[:, dead] = 0.0; H[dead, dead] = 1.0; g[dead] = 0.0
    B = np.flatnonzero(ne.rows_B); Pm = np.flatnonzero(ne.rows_P)
    # canonical order of the reduced part: camera | poses | promoted points ascending = ascending full index.  The eliminated points
    # do not couple (the second point of a constraint is promoted): H_PP is 3 x 3 block diagonal, inverted by cofactors in long double
    S = H[np.ix_(B, B)].copy(); rhs = -g[B].copy()
    for p0 in Pm[::3]:
        idx = np.arange(p0, p0 + 3)
        assert np.all(ne.rows_P[idx])
        U = H[np.ix_(idx, idx)]
        cof = np.array([[U[(i + 1) % 3, (j + 1) % 3] * U[(i + 2) % 3, (j + 2) % 3] - U[(i + 1) % 3, (j + 2) % 3] * U[(i + 2) % 3, (j + 1) % 3]
                         for j in range(3)] for i in range(3)], LD)
        Ui = cof.T / (U[0] @ cof[0])
        W = H[np.ix_(B, idx)]
        S -= W @ Ui @ W.T
        rhs += W @ (Ui @ g[idx])
    return S.astype(np.float64), rhs.astype(np.float64)
