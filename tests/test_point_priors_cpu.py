"""Priors on 3D points and the scene alignment without a GPU (include/lifcal_prior.h, include/lifcal_align.h):
every refusal of lifcal_ba_check_point_priors, the consistency of tests/point_prior_reference.py with a plain dense solve, and
lifcal_align_fit / lifcal_align_apply against an SVD solution in numpy."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
import lifcal_amd
from lifcal_amd import LifcalError, _capi as capi, scene
from tests import point_prior_reference as ppr
from tests import prior_reference as pr
from tests import step_reference as sr
from tests.helpers import S, problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, OUT_OF_RANGE = -1, -4
LD = np.longdouble


def spd3(rng):
    A = rng.normal(size=(3, 3))
    return A @ A.T + 0.1 * np.eye(3)


def good(rng, ids=(1, 4, 9)):
    return np.array(ids), rng.normal(size=(len(ids), 3)), np.array([spd3(rng) for _ in ids])


def rejected(code, n_points, ids, means, infos):
    with pytest.raises(LifcalError) as e:
        lifcal_amd.check_point_priors(n_points, ids, means, infos)
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_symbols_and_layout(built):
    lib = capi.load_library()
    for header, table in (("lifcal_prior.h", capi.PRIOR_PROTOTYPES), ("lifcal_align.h", capi.ALIGN_PROTOTYPES)):
        hdr = open(os.path.join(ROOT, "include", header)).read()
        declared = set(re.findall(r"\b(lifcal_(?:ba_)?[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
        assert declared == set(table), declared ^ set(table)
        for name in declared:
            assert hasattr(lib, name), name
    assert C.sizeof(capi.PointPriors) == 32 and capi.PointPriors.point.offset == 8 and capi.PointPriors.info.offset == 24
    assert C.sizeof(capi.Alignment) == 8 * 14 + 8 and capi.Alignment.n_used.offset == 8 * 14
    for name in ("check_point_priors", "alignFit", "alignApply", "alignScene"):
        assert hasattr(lifcal_amd, name)
    for name in ("set_point_priors", "clear_point_priors", "point_prior_cost"):
        assert hasattr(lifcal_amd.BundleAdjustment, name)
    assert hasattr(lifcal_amd.IntersectionResult, "point_information")


def test_check_point_priors_accepts_sound_priors(built):
    rng = np.random.default_rng(1)
    ids, means, infos = good(rng)
    lifcal_amd.check_point_priors(10, ids, means, infos)
    lifcal_amd.check_point_priors(10, [], np.zeros((0, 3)), np.zeros((0, 3, 3)))
    lifcal_amd.check_point_priors(10, ids, means, np.zeros((3, 3, 3)))        # a zero matrix is positive semi-definite
    semi = infos.copy(); semi[1] = 0.0; semi[1, 2, 2] = 4.0                     # rank one
    lifcal_amd.check_point_priors(10, ids, means, semi)
    A = infos.copy(); A[0, 0, 2] += 0.5e-12 * np.sqrt(A[0, 0, 0] * A[0, 2, 2])  # asymmetric inside the tolerance
    lifcal_amd.check_point_priors(10, ids, means, A)


def test_check_point_priors_null_pointers(built):
    lib = capi.load_library()
    assert lib.lifcal_ba_check_point_priors(10, None) == INVALID_ARG
    p = capi.PointPriors(); p.n = 2
    assert lib.lifcal_ba_check_point_priors(10, C.byref(p)) == INVALID_ARG
    p.n = 0
    assert lib.lifcal_ba_check_point_priors(10, C.byref(p)) == 0


def test_check_point_priors_non_finite_mean(built):
    ids, means, infos = good(np.random.default_rng(2))
    means[1, 2] = np.nan
    assert "non-finite mean" in rejected(INVALID_ARG, 10, ids, means, infos)


def test_check_point_priors_non_finite_info(built):
    ids, means, infos = good(np.random.default_rng(3))
    infos[2, 1, 1] = np.inf
    assert "non-finite entry" in rejected(INVALID_ARG, 10, ids, means, infos)


def test_check_point_priors_asymmetric(built):
    ids, means, infos = good(np.random.default_rng(4))
    infos[0, 0, 1] += 1e-9 * np.sqrt(infos[0, 0, 0] * infos[0, 1, 1])
    assert "not symmetric" in rejected(INVALID_ARG, 10, ids, means, infos)


def test_check_point_priors_negative_diagonal(built):
    ids, means, infos = good(np.random.default_rng(5))
    infos[1] = np.diag([1.0, -1e-3, 1.0])
    assert "negative diagonal" in rejected(INVALID_ARG, 10, ids, means, infos)


def test_check_point_priors_not_psd(built):
    ids, means, infos = good(np.random.default_rng(6))
    infos[2] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    assert "positive semi-definite" in rejected(INVALID_ARG, 10, ids, means, infos)


@pytest.mark.parametrize("ids", [(4, 1, 9), (1, 4, 4)], ids=["descending", "repeated"])
def test_check_point_priors_ids_not_strictly_ascending(built, ids):
    _, means, infos = good(np.random.default_rng(7))
    assert "ascending" in rejected(INVALID_ARG, 10, np.array(ids), means, infos)


def test_check_point_priors_id_out_of_range(built):
    ids, means, infos = good(np.random.default_rng(8), ids=(1, 4, 10))
    assert "point 10 of 10" in rejected(OUT_OF_RANGE, 10, ids, means, infos)
    lifcal_amd.check_point_priors(11, ids, means, infos)


# ---- the reference's own consistency --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,spec", [("full", S(6, 40, None, 0x506, 101)), ("constraints", S(6, 40, None, 0x506, 117, n_constraints=3))])
def test_reduced_system_of_the_augmented_equations_against_a_dense_solve(built, name, spec):
    """S and rhs of dense_reduced() on the augmented equations against S = H_BB - H_BP H_PP^-1 H_PB and rhs = -g_B + H_BP H_PP^-1 g_P
    formed from the FULL augmented J^T J + diag(lambda) with numpy's solve over the whole point block: 1e-12 block-scaled"""
    sc = scene.make_scene(spec)
    pa = problem(sc)
    ne0 = sr.NormalEquations(pa, 1e4)
    ids = [3, 11, 17, 25, 38]
    if ne0.constrained:
        ids = sorted(set([int(ne0.ci[0]), int(ne0.cj[1])] + ids[:3]))
    ids, means, infos = ppr.control_priors(ne0, pa.pts, ids)
    ne = ppr.PointPriorEquations(pa, 1e4, ids, means, infos)
    assert ne.cost_prior > 1e-6 * ne.cost_observations
    assert abs(ne.cost_prior - ppr.prior_cost(pa.pts, ids, means, infos)) <= 1e-13 * ne.cost_prior
    S_, rhs, g_red, gp, Ui = ppr.reduced_system(ne)
    n = ne.n
    H = np.zeros((n, n), LD); e = np.zeros(n, LD)
    for k in range(n):
        e[k] = 1.0; H[:, k] = ne.JtJ(e); e[k] = 0.0
    H[np.arange(n), np.arange(n)] += ne.lam
    g = ne.g.copy()
    dead = ~ne.live
    H[dead, :] = 0.0; H[:, dead] = 0.0; H[dead, dead] = 1.0; g[dead] = 0.0
    # the prior is in the blocks of its points and nowhere else
    H0 = np.zeros((n, n), LD)
    for k in range(n):
        e[k] = 1.0; H0[:, k] = ne0.JtJ(e); e[k] = 0.0
    D = np.asarray(H - H0, np.float64); D[np.arange(n), np.arange(n)] -= np.asarray(ne.lam, np.float64)
    for q, A in zip(ids, infos):
        c = ne.nb + 3 * int(q)
        assert np.allclose(D[c:c + 3, c:c + 3], 0.5 * (A + A.T), rtol=1e-12, atol=0)
        D[c:c + 3, c:c + 3] = 0.0
    D[dead, :] = 0.0; D[:, dead] = 0.0
    assert np.max(np.abs(D)) <= 1e-12 * np.max(np.abs(np.asarray(H0, np.float64)))
    # S and rhs from the full matrix: H_BB - H_BP X, -g_B + H_BP y with X, y from numpy's solve over the WHOLE point block (Jacobi-
    # scaled: the columns have units orders apart)
    B = np.flatnonzero(ne.rows_B); Pm = np.flatnonzero(ne.rows_P)
    Hf, gf = np.asarray(H, np.float64), np.asarray(g, np.float64)
    sp = 1.0 / np.sqrt(np.diag(Hf)[Pm])
    Xy = sp[:, None] * np.linalg.solve(Hf[np.ix_(Pm, Pm)] * np.outer(sp, sp), sp[:, None] * np.column_stack([Hf[np.ix_(Pm, B)], gf[Pm]]))
    S2 = Hf[np.ix_(B, B)] - Hf[np.ix_(B, Pm)] @ Xy[:, :-1]
    rhs2 = -gf[B] + Hf[np.ix_(B, Pm)] @ Xy[:, -1]
    dg = np.sqrt(np.abs(np.diag(S_)))
    eS = np.max(np.abs(S2 - S_) / np.outer(dg, dg)); er = np.max(np.abs(rhs2 - rhs) / dg) / np.max(np.abs(rhs) / dg)
    print(f"[{name}] S {eS:.2e}  rhs {er:.2e}")
    assert eS <= 1e-12 and er <= 1e-12


# ---- alignment ------------------------------------------------------------------------------------------------------------------------
def rot(rng, angle=None):
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    th = rng.uniform(0.2, 2.5) if angle is None else angle
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def align_case(n, weighted, with_scale, noise, seed):
    rng = np.random.default_rng(seed)
    src = rng.uniform(-300.0, 300.0, size=(n, 3))                 # mm, the size of a calibration field
    R, t, s = rot(rng), rng.uniform(-500.0, 500.0, size=3), (rng.uniform(0.3, 3.0) if with_scale else 1.0)
    dst = s * src @ R.T + t + noise * rng.normal(size=(n, 3))
    w = rng.uniform(0.2, 5.0, size=n) if weighted else None
    return src, dst, w


ALIGN_CASES = [(n, wt, sc, nz) for n in (3, 4, 10) for wt in (False, True) for sc in (False, True) for nz in (0.0, 1e-4)]
# Agreement of Horn's quaternion solution (Jacobi eigenvectors, long double sums) with the SVD solution (LAPACK, float64 sums), the
# maxima measured over these 24 inputs: R 1.8e-14 (largest entry difference), t 2.3e-15 of |t| + scene size, scale 4.6e-16 relative,
# rms 2.4e-15 of the scene size (on exact data both rms values ARE this rounding floor, ~1e-13 mm).  The bars are ten times that.
BAR_R, BAR_T, BAR_S, BAR_RMS = 1.8e-13, 2.3e-14, 4.6e-15, 2.4e-14


@pytest.mark.parametrize("n,weighted,with_scale,noise", ALIGN_CASES)
def test_align_fit_against_the_svd_solution(built, n, weighted, with_scale, noise):
    src, dst, w = align_case(n, weighted, with_scale, noise, seed=100 * n + 10 * weighted + with_scale + (5 if noise else 0))
    al = lifcal_amd.alignFit(src, dst, w, with_scale)
    s, R, t, rms = ppr.umeyama(src, dst, w, with_scale)
    size = np.max(np.abs(dst))
    eR, et, es = np.max(np.abs(al.R - R)), np.max(np.abs(al.t - t)) / (np.linalg.norm(t) + size), abs(al.scale - s) / s
    erms = abs(al.rms - rms) / size
    print(f"ALIGN n={n} w={weighted} s={with_scale} noise={noise}: R {eR:.2e}  t {et:.2e}  scale {es:.2e}  rms {al.rms:.3e} vs {rms:.3e} ({erms:.2e} of the size)")
    assert al.n_used == n and abs(np.linalg.det(al.R) - 1.0) <= 1e-14
    if not with_scale:
        assert al.scale == 1.0
    assert eR <= BAR_R and et <= BAR_T and es <= BAR_S and erms <= BAR_RMS
    assert (1e-5 < al.rms < 1e-3) if noise else (al.rms <= 1e-12 * size)


def test_align_fit_zero_weights_leave_points_out(built):
    src, dst, _ = align_case(6, False, True, 0.0, seed=9)
    dst2 = dst.copy(); dst2[[1, 4]] += 50.0
    w = np.ones(6); w[[1, 4]] = 0.0
    al = lifcal_amd.alignFit(src, dst2, w, True)
    ref = lifcal_amd.alignFit(np.delete(src, [1, 4], 0), np.delete(dst, [1, 4], 0), None, True)
    assert al.n_used == 4 and np.allclose(al.R, ref.R, atol=1e-14) and np.allclose(al.t, ref.t, atol=1e-10) and al.rms < 1e-10


def align_rejected(src, dst, w=None, with_scale=True):
    with pytest.raises(LifcalError) as e:
        lifcal_amd.alignFit(src, dst, w, with_scale)
    assert e.value.code == INVALID_ARG
    return str(e.value)


def test_align_fit_refusals(built):
    src, dst, _ = align_case(5, False, True, 0.0, seed=11)
    assert "fewer than three" in align_rejected(src[:2], dst[:2])
    assert "fewer than three" in align_rejected(src, dst, np.array([1.0, 1.0, 0.0, 0.0, -1.0]))
    line = np.outer(np.linspace(-1.0, 1.0, 5), np.array([3.0, -2.0, 1.0])) + np.array([10.0, 20.0, 30.0])
    assert "collinear" in align_rejected(line, dst)
    assert "collinear" in align_rejected(np.tile(src[:1], (5, 1)), dst)
    assert "`to`" in align_rejected(src, line) and "`to`" in align_rejected(src, np.tile(dst[:1], (5, 1)))   # the given side as well
    for arr in ("src", "dst", "w"):
        a, b, w = src.copy(), dst.copy(), np.ones(5)
        {"src": a, "dst": b, "w": w}[arr].reshape(-1)[3] = np.nan
        assert "non-finite" in align_rejected(a, b, w)
    lib = capi.load_library()
    out = capi.Alignment()
    assert lib.lifcal_align_fit(5, None, capi.as_dptr(dst), None, 1, C.byref(out)) == INVALID_ARG
    assert lib.lifcal_align_apply(None, 0, None, 0, None) == INVALID_ARG


@pytest.mark.parametrize("with_scale", [False, True])
def test_align_apply_keeps_every_camera_frame_point(built, with_scale):
    """R_f' P' + t_f' = s (R_f P + t_f) for random poses and points, through the oracle's rigid transform of a view"""
    rng = np.random.default_rng(21 + with_scale)
    F, P = 7, 30
    views = np.concatenate([rng.uniform(-1.2, 1.2, size=(F, 3)), rng.uniform(-400.0, 400.0, size=(F, 3))], 1)
    pts = rng.uniform(-300.0, 300.0, size=(P, 3))
    al = lifcal_amd.Alignment(rng.uniform(0.4, 2.5) if with_scale else 1.0, rot(rng, 0.3), rng.uniform(-200.0, 200.0, size=3), 0.0, 0)
    v2, p2 = lifcal_amd.alignApply(al, views, pts)
    assert np.allclose(p2, al.scale * pts @ al.R.T + al.t, rtol=0, atol=1e-12 * 1000.0)
    size = 0.0; worst = 0.0
    for f in range(F):
        RT0, RT1 = oracle.rigid_transform(views[f]), oracle.rigid_transform(v2[f])
        X0 = pts @ RT0[:, :3].T + RT0[:, 3]
        X1 = p2 @ RT1[:, :3].T + RT1[:, 3]
        size = max(size, np.max(np.abs(al.scale * X0)))
        worst = max(worst, np.max(np.abs(X1 - al.scale * X0)))
        assert 0.0 <= v2[f, 0] <= np.pi and np.all(np.abs(v2[f, 1:3]) <= np.pi)
    print(f"alignApply with_scale={with_scale}: camera-frame error {worst:.2e} of scene size {size:.2e}")
    assert worst <= 1e-12 * size
    # the inputs are untouched, the inverse alignment brings the scene back
    inv = lifcal_amd.Alignment(1.0 / al.scale, al.R.T, -(al.R.T @ al.t) / al.scale, 0.0, 0)
    v3, p3 = lifcal_amd.alignApply(inv, v2, p2)
    assert np.allclose(p3, pts, rtol=0, atol=1e-12 * 1000.0)
    for f in range(F):
        assert np.allclose(oracle.rigid_transform(v3[f]), oracle.rigid_transform(views[f]), rtol=0, atol=1e-12 * 1000.0)


def test_align_scene_moves_a_problem_onto_its_marks(built):
    sc = scene.make_scene(S(6, 40, None, 0x506, 101))
    pa = problem(sc)
    rng = np.random.default_rng(31)
    mv = lifcal_amd.Alignment(1.7, rot(rng, 0.3), np.array([120.0, -80.0, 140.0]), 0.0, 0)
    v, p = lifcal_amd.alignApply(mv, pa.views, pa.pts)
    moved = problem(sc); moved.views[:] = v.reshape(-1); moved.pts[:] = p.reshape(-1)
    ids = np.array([2, 9, 17, 26, 35])
    al = lifcal_amd.alignScene(moved, ids, pa.pts.reshape(-1, 3)[ids], with_scale=True)
    assert abs(al.scale * mv.scale - 1.0) <= 1e-13 and al.rms <= 1e-10
    assert np.allclose(moved.pts, pa.pts, rtol=0, atol=1e-9)
    for f in range(6):
        assert np.allclose(oracle.rigid_transform(moved.views[6 * f:6 * f + 6]), oracle.rigid_transform(pa.views[6 * f:6 * f + 6]), rtol=0, atol=1e-9)
