"""Gaussian priors on 3D points and the scene alignment (include/lifcal_prior.h, include/lifcal_align.h): the
references the tests measure against (numpy only).  The oracle has no priors.

  PointPriorEquations  tests/step_reference.NormalEquations with the rows Lambda^(1/2) on the three columns of a prior-ed point
                       appended to J and Lambda^(1/2) d, d = P - mean, to r: Ceres' view of one extra residual block per prior,
                       without a loss.  A problem that does not refine its points drops the rows.
  reduced_system()     S and rhs of such equations (prior_reference.dense_reduced: H_PP stays 3 x 3 block diagonal) with the
                       eliminated points' gradients and inverse blocks
  control_priors()     the prior set of the sweep and step tests: Lambda = strength s s^T o R with s the square root of the
                       undamped U_p diagonal of the prior-free equations, means one scaled unit off the start values
  umeyama()            the SVD solution of to ~ s R from + t (Kabsch / Umeyama), weighted
"""
import numpy as np

from tests import prior_reference as pr
from tests import step_reference as sr

LD = sr.LD


def sqrt_rows(A):
    """rows [k, 3] with rows^T rows = A (symmetric PSD 3 x 3), through the unit-diagonal matrix"""
    A = 0.5 * (np.asarray(A, np.float64) + np.asarray(A, np.float64).T)
    dg = np.sqrt(np.where(np.diag(A) > 0, np.diag(A), 1.0))
    w, V = np.linalg.eigh(A / np.outer(dg, dg))
    keep = w > 0
    return (np.sqrt(w[keep])[:, None] * V[:, keep].T) * dg[None, :]


class PointPriorEquations(sr.NormalEquations):
    """The normal equations of `pa` with the point-prior rows appended.  ids[n], means[n, 3], infos[n, 3, 3]."""

    def __init__(self, pa, radius, ids, means, infos, jacobi_scaling=True, **kw):
        super().__init__(pa, radius, jacobi_scaling=jacobi_scaling, **kw)
        ids = np.asarray(ids, np.int64).reshape(-1)
        means = np.asarray(means, np.float64).reshape(len(ids), 3)
        infos = np.asarray(infos, np.float64).reshape(len(ids), 3, 3)
        self.cost_observations = self.cost
        self.cost_prior = 0.0
        self._pp = []            # (first column, rows [k, 3] long double, |rows|)
        if not self.refine_points:
            return
        self.g = self.g.copy(); self.h = self.h.copy()
        P = pa.pts.reshape(-1, 3)
        for q, m, A in zip(ids, means, infos):
            L = sqrt_rows(A).astype(LD)
            c = self.nb + 3 * int(q)
            r = L @ (P[q].astype(LD) - m.astype(LD))
            self._pp.append((c, L, np.abs(L)))
            self.cost_prior += float(0.5 * r @ r)
            self.g[c:c + 3] += L.T @ r
            self.h[c:c + 3] += np.sum(L * L, 0)
            self.observed_points[q] = True
        self.cost = self.cost_observations + self.cost_prior
        self.live = np.asarray(self.h > 0)
        hs = self.h.astype(np.float64)
        self.sigma = 1.0 / (1.0 + np.sqrt(hs)) if jacobi_scaling else np.ones(self.n)
        self.set_radius(radius)

    def JtJ(self, x, absolute=False):
        x = np.asarray(x, LD)
        out = super().JtJ(x, absolute)
        for c, L, aL in self._pp:
            M = aL if absolute else L
            out[c:c + 3] += M.T @ (M @ x[c:c + 3])
        return out


def point_blocks(ne):
    """(U [P, 3, 3], g [P, 3]) of `ne`: the damped point blocks J_p^T J_p + diag(lambda_p) and the point gradients, long double"""
    U = np.zeros((ne.P, 3, 3), LD)
    e = np.zeros(ne.n, LD)
    for k in range(3):
        e[:] = 0.0
        e[ne.nb + k::3] = 1.0            # the points do not couple through observations: one probe per coordinate serves all of them
        col = ne.JtJ(e)[ne.nb:].reshape(ne.P, 3)
        U[:, :, k] = col
    # a distance constraint couples its two points: the probe above added the partner's column; take those blocks one by one
    for q in set(int(i) for i in np.concatenate([ne.ci, ne.cj])):
        for k in range(3):
            e[:] = 0.0
            e[ne.nb + 3 * q + k] = 1.0
            U[q, :, k] = ne.JtJ(e)[ne.nb + 3 * q:ne.nb + 3 * q + 3]
    lam = ne.lam[ne.nb:].reshape(ne.P, 3)
    for k in range(3):
        U[:, k, k] += lam[:, k]
    return U, ne.g[ne.nb:].reshape(ne.P, 3).copy()


def inv3(U):
    U = np.asarray(U, LD)
    cof = np.array([[U[(i + 1) % 3, (j + 1) % 3] * U[(i + 2) % 3, (j + 2) % 3] - U[(i + 1) % 3, (j + 2) % 3] * U[(i + 2) % 3, (j + 1) % 3]
                     for j in range(3)] for i in range(3)], LD)
    return cof.T / (U[0] @ cof[0])


def reduced_system(ne):
    """S, rhs (prior_reference.dense_reduced), gradient_reduced in the canonical reduced order, and for the eliminated live points the
    gradient [P, 3] and the inverse of the damped block [P, 3, 3] (zero elsewhere)"""
    S, rhs = pr.dense_reduced(ne)
    g = ne.g.copy(); g[~ne.live] = 0.0
    g_red = np.asarray(ne.reduced(g), np.float64)
    U, gp = point_blocks(ne)
    Ui = np.zeros((ne.P, 3, 3)); gpo = np.zeros((ne.P, 3))
    for q in range(ne.P):
        c = ne.nb + 3 * q
        if ne.rows_P[c] and ne.live[c]:
            Ui[q] = inv3(U[q]).astype(np.float64); gpo[q] = gp[q].astype(np.float64)
    return S, rhs, g_red, gpo, Ui


def random_correlation(rng, n=3):
    A = rng.normal(size=(n, n))
    A = A @ A.T + 0.1 * np.eye(n)
    d = 1.0 / np.sqrt(np.diag(A))
    return A * np.outer(d, d)


def control_priors(ne_free, pts, ids, seed=0, strength=0.3):
    """(ids, means, infos): Lambda = strength s s^T o R per point with s = sqrt(diag U_p) of the undamped prior-free equations
    `ne_free` and R a random correlation matrix; means one scaled unit off the start values `pts`.  A point without observations
    has no U_p: it takes the median scale of the others."""
    ids = np.asarray(sorted(int(i) for i in ids), np.uint32)
    rng = np.random.default_rng(2000 + seed)
    h = np.asarray(ne_free.h[ne_free.nb:], np.float64).reshape(-1, 3)
    seen = h[ids][h[ids].min(1) > 0]
    med = np.median(seen, 0) if len(seen) else np.ones(3)     # (points that are not refined have no U_p at all: unit scale)
    P = np.asarray(pts, np.float64).reshape(-1, 3)
    means, infos = [], []
    for q in ids:
        s = np.sqrt(np.where(h[q] > 0, h[q], med))
        means.append(P[q] + rng.normal(size=3) / s)
        infos.append(strength * random_correlation(rng) * np.outer(s, s))
    return ids, np.array(means), np.array(infos)


def prior_cost(pts, ids, means, infos):
    P = np.asarray(pts, LD).reshape(-1, 3)
    c = LD(0)
    for q, m, A in zip(ids, np.asarray(means, LD).reshape(-1, 3), np.asarray(infos, LD).reshape(-1, 3, 3)):
        d = P[int(q)] - m
        c += 0.5 * d @ (0.5 * (A + A.T)) @ d
    return float(c)


def umeyama(src, dst, w=None, with_scale=True):
    """(s, R, t, rms) minimising sum w |dst - s R src - t|^2 (Umeyama 1991; Kabsch with s = 1), through numpy's SVD"""
    a = np.asarray(src, np.float64).reshape(-1, 3); b = np.asarray(dst, np.float64).reshape(-1, 3)
    w = np.ones(len(a)) if w is None else np.asarray(w, np.float64)
    W = w.sum()
    ca, cb = (w[:, None] * a).sum(0) / W, (w[:, None] * b).sum(0) / W
    A, B = a - ca, b - cb
    C = (w[:, None] * B).T @ A / W                     # sum w b a^T
    U, D, Vt = np.linalg.svd(C)
    E = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ E @ Vt
    s = float(np.sum(D * np.diag(E)) / (np.sum(w[:, None] * A * A) / W)) if with_scale else 1.0
    t = cb - s * R @ ca
    res = b - (s * a @ R.T + t)
    return s, R, t, float(np.sqrt(np.sum(w[:, None] * res * res) / W))
