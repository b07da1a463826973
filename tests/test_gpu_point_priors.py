"""Gaussian priors on 3D points and the control-point chain on the MI355X (include/lifcal_prior.h, include/lifcal_align.h; DESIGN.md
section 7r), through the C ABI.

The oracle has no priors: the references are the augmented normal equations of tests/point_prior_reference.py (numpy, long double)
and their dense Schur complement.  Bars are the project's own (tests/test_gpu_parity.py, tests/test_gpu_priors.py,
tests/test_gpu_step.py).  The prior set of the sweep and step tests is scaled by the undamped U_p diagonal of the reference
equations, so that Lambda is of the size of U_p and a misplaced entry stands out at O(1).

Figures measured on an MI355X: DESIGN.md section 7r."""
import functools
import types

import numpy as np
import pytest

import lifcal_amd
from lifcal_amd import BundleAdjustment, LifcalError, _capi as capi, scene
from tests import point_prior_reference as ppr
from tests import step_reference as sr
from tests.helpers import S, problem, scaled_max_err, vec_err
from tests.test_gpu_covariance import problem_copy
from tests.test_gpu_priors import SCENES, UNDAMPED, options, scene_of, stationarity, summary_tuple, sweep_tuple
from tests.test_gpu_step import MARGIN, candidate_cost, set_route_env

pytestmark = pytest.mark.gpu

SWEEP_SCENES = ["full", "constraints", "constraints_adj_robust", "windowed", "r2_tan_robust", "full_unobserved", "windowed_many"]


def problem_of(name):
    """a fresh problem of the scene; full_unobserved: `full` without the observations of point 7 (a prior-only point);
    windowed_many: `windowed`, with 70 of its 120 points prior-ed (more than one workgroup of k_point_priors, its strided cost loop)"""
    if name == "windowed_many":
        return problem(scene_of("windowed"))
    if name != "full_unobserved":
        return problem(scene_of(name))
    sc = scene_of("full")
    keep = sc.pt != 7
    return capi.ProblemArrays(sc.u[keep], sc.v[keep], sc.mcx[keep], sc.mcy[keep], sc.pt[keep], sc.fr[keep], sc.cam0, sc.views0, sc.pts0,
                              sc.spx, sc.scale, sc.config, fixed_mask=sc.fixed_mask)


@functools.lru_cache(maxsize=None)
def free_equations(name, radius):
    return sr.NormalEquations(problem_of(name), radius)


@functools.lru_cache(maxsize=None)
def prior_set(name, seed=0, strength=0.3):
    """five points (windowed_many: 70): in the constraint scenes one eliminated first point c_i and one promoted second point c_j
    among them, in full_unobserved the point without observations"""
    ne0 = free_equations(name, UNDAMPED)
    P = ne0.P
    ids = {3 % P, (P // 3 + 1) % P, P // 2, (2 * P) // 3 + 2, P - 2}
    if ne0.constrained:
        ci = next(int(i) for i in ne0.ci if int(i) not in set(int(j) for j in ne0.cj))
        cj = next(int(j) for j in ne0.cj if int(j) != ci)
        ids = set(sorted(ids - {ci, cj})[:3]) | {ci, cj}
    if name == "full_unobserved":
        ids = set(sorted(ids - {7})[:4]) | {7}
    if name == "windowed_many":
        ids = {q for q in range(P) if q % 12 not in (0, 5, 7, 9, 11)}
        assert len(ids) == 70 > 64
    else:
        assert len(ids) == 5
    return ppr.control_priors(ne0, problem_of(name).pts, ids, seed=seed, strength=strength)


@functools.lru_cache(maxsize=None)
def reference_sweep(name, radius):
    """computed once, shared, never written to"""
    pa = problem_of(name)
    ne = ppr.PointPriorEquations(pa, radius, *prior_set(name))
    S_, rhs, g_red, gp, Ui = ppr.reduced_system(ne)
    for a in (S_, rhs, g_red, gp, Ui):
        a.setflags(write=False)
    return types.SimpleNamespace(ne=ne, S=S_, rhs=rhs, gradient_reduced=g_red, point_gradient=gp, point_hessian_inv=Ui, cost=ne.cost,
                                 cost_prior=ne.cost_prior, cost_observations=ne.cost_observations, n_promoted=len(ne.promoted))


def check_sweep(tag, got, ref, ids, pc):
    ne = ref.ne
    e_cost = abs(got.cost - ref.cost) / ref.cost
    e_S = scaled_max_err(got.S, ref.S)
    e_rhs, e_g = vec_err(got.rhs, ref.rhs), vec_err(got.gradient_reduced, ref.gradient_reduced)
    gp = got.point_gradient.reshape(-1, 3); Ui = got.point_hessian_inv.reshape(-1, 3, 3)
    e_gp = e_Ui = 0.0
    for q in ids:
        q = int(q)
        promoted = q in ne.promoted
        g_ref = np.asarray(ne.g[ne.nb + 3 * q:ne.nb + 3 * q + 3], np.float64) if promoted else ref.point_gradient[q]
        e_gp = max(e_gp, float(np.max(np.abs(gp[q] - g_ref)) / (np.max(np.abs(g_ref)) or 1.0)))   # (points not refined: both are zero)
        if not promoted and ne.refine_points:
            d = np.sqrt(np.abs(np.diag(ref.point_hessian_inv[q])))
            e_Ui = max(e_Ui, float(np.max(np.abs(Ui[q] - ref.point_hessian_inv[q]) / np.outer(d, d))))
    e_pc = abs(pc - ref.cost_prior) / ref.cost_prior if ref.cost_prior else abs(pc)
    print(f"[{tag}] prior cost {ref.cost_prior:.6e} of {ref.cost:.6e}: cost {e_cost:.2e}  S {e_S:.2e}  rhs {e_rhs:.2e}  gradient {e_g:.2e}  "
          f"point gradient {e_gp:.2e}  U^-1 {e_Ui:.2e}  point_prior_cost {e_pc:.2e}")
    assert e_cost <= 1e-12
    assert e_S <= 1e-9 and np.array_equal(got.S, got.S.T)
    assert e_rhs <= 1e-9
    assert e_g <= 1e-10
    assert e_gp <= 1e-9 and e_Ui <= 1e-9
    assert e_pc <= 1e-12


# ---- 1. one sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [0, 1], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("name", SWEEP_SCENES)
def test_one_sweep_against_the_augmented_equations(built, name, deterministic):
    pa = problem_of(name)
    ids, means, infos = prior_set(name)
    ref = reference_sweep(name, UNDAMPED)
    if name.startswith("constraints"):
        assert ref.n_promoted > 0 and any(int(q) in ref.ne.promoted for q in ids) and any(int(q) in set(ref.ne.ci.tolist()) for q in ids)
    with BundleAdjustment(pa, options(deterministic=deterministic), point_priors=(ids, means, infos)) as ba:
        got = ba.sweep(UNDAMPED, want_matrices=True)
        pc = ba.point_prior_cost()
    assert got.n_promoted == ref.n_promoted
    if name == "r2_tan_robust":          # points not refined: the term is dropped (bit-level: test_dropped_term below)
        assert ref.cost_prior == 0.0 and pc == 0.0
    else:
        assert ref.cost_prior > 1e-6 * ref.cost_observations, "the prior is too weak to be seen in the cost"
    check_sweep(f"{name} det={deterministic}", got, ref, ids, pc)


# ---- 2. precision = 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["full", "constraints_adj_robust"])
def test_one_sweep_precision1_against_the_precision0_arm(built, name):
    """The prior points are special points: the global-atomic kernels evaluate them in fp64 under either precision, so what the priors
    change in a sweep (this handle with the priors against this handle with the priors cleared) is the same under precision 1 and 0.
    Reference: the precision-1 sweep with the priors cleared plus the change the precision-0 arm of the same configuration sees; bars
    of tests/test_gpu_priors.py::test_one_sweep_precision1_against_its_own_prior_free_sweep."""
    ids, means, infos = prior_set(name, seed=1)
    arms = {}
    for precision in (0, 1):
        with BundleAdjustment(problem_of(name), options(precision=precision), point_priors=(ids, means, infos)) as ba:
            w = ba.sweep(UNDAMPED, want_matrices=True)
            ba.clear_point_priors()
            assert ba.point_prior_cost() == 0.0
            arms[precision] = (w, ba.sweep(UNDAMPED, want_matrices=True))
    (w0, b0), (w1, b1) = arms[0], arms[1]
    ref_S, ref_rhs, ref_g, ref_cost = b1.S + (w0.S - b0.S), b1.rhs + (w0.rhs - b0.rhs), b1.gradient_reduced + (w0.gradient_reduced - b0.gradient_reduced), b1.cost + (w0.cost - b0.cost)
    e_cost, e_S = abs(w1.cost - ref_cost) / ref_cost, scaled_max_err(w1.S, ref_S)
    e_rhs, e_g = vec_err(w1.rhs, ref_rhs), vec_err(w1.gradient_reduced, ref_g)
    gp0 = (w0.point_gradient - b0.point_gradient).reshape(-1, 3); gp1 = (w1.point_gradient - b1.point_gradient).reshape(-1, 3)
    e_gp = float(np.max(np.abs(gp1[ids] - gp0[ids])) / np.max(np.abs(gp0[ids])))
    print(f"[{name} precision=1] cost {e_cost:.2e}  S {e_S:.2e}  rhs {e_rhs:.2e}  gradient {e_g:.2e}  point gradient {e_gp:.2e}; "
          f"prior cost {w0.cost - b0.cost:.6e} of {w0.cost:.6e}; precision 1 against 0 itself: S {scaled_max_err(w1.S, w0.S):.2e}")
    assert w0.cost - b0.cost > 1e-6 * b0.cost
    assert e_cost <= 1e-12
    assert e_S <= 1e-9 and np.array_equal(w1.S, w1.S.T)
    assert e_rhs <= 1e-9 and e_g <= 1e-10 and e_gp <= 1e-9


# ---- 3. dropped term --------------------------------------------------------------------------------------------------------------
def test_dropped_term_where_points_are_not_refined(built):
    name = "r2_tan_robust"
    assert not (SCENES[name].config & 0x400)
    ids, means, infos = prior_set(name)
    with BundleAdjustment(problem_of(name), options(deterministic=1)) as ba:
        a = ba.sweep(1e4, want_matrices=True)
    with BundleAdjustment(problem_of(name), options(deterministic=1), point_priors=(ids, means, infos)) as ba:
        b = ba.sweep(1e4, want_matrices=True)
        assert ba.point_prior_cost() == 0.0
    assert a.cost == b.cost and np.array_equal(a.S, b.S) and np.array_equal(a.rhs, b.rhs)
    assert sweep_tuple(a) == sweep_tuple(b)


# ---- 4. nothing changes without priors --------------------------------------------------------------------------------------------
def info_tuple(i):
    return (i.n_obs_local, i.n_points_local, i.n_groups, i.n_tiles, i.n_lenses, i.n_reduced, i.n_promoted, i.n_chunks, i.max_window_frames)


def test_without_priors_nothing_changes(built):
    name = "constraints_adj_robust"
    empty = (np.zeros(0, np.uint32), np.zeros((0, 3)), np.zeros((0, 3, 3)))
    results = []
    for point_priors in (None, (), empty):                 # lifcal_ba_create, the new entry with NULL, the new entry with n = 0
        pa = problem_of(name)
        with BundleAdjustment(pa, options(deterministic=1), point_priors=point_priors) as ba:
            info = info_tuple(ba.info())
            sw = ba.sweep(1e4, want_matrices=True)
            assert ba.point_prior_cost() == 0.0
            s = ba.performBundleAdjustment()
        results.append((info, sweep_tuple(sw), summary_tuple(s), pa.cam.tobytes(), pa.views.tobytes(), pa.pts.tobytes()))
    assert results[0] == results[1], "lifcal_ba_create_with_point_priors(NULL) is not lifcal_ba_create"
    assert results[0] == results[2], "lifcal_ba_create_with_point_priors(n = 0) is not lifcal_ba_create"
    # lifcal_ba_plan of the problem describes that layout, and the prior-ed layout moves nothing but the path of its points
    pi, _, _ = lifcal_amd.plan(problem_of(name))
    assert (pi.n_groups, pi.n_tiles, pi.n_lenses, pi.n_reduced, pi.n_promoted, pi.n_chunks, pi.max_window_frames) == results[0][0][2:]
    with BundleAdjustment(problem_of(name), options(deterministic=1), point_priors=prior_set(name)) as ba:
        wp = info_tuple(ba.info())
    assert tuple(wp[k] for k in (0, 1, 4, 5, 6)) == tuple(results[0][0][k] for k in (0, 1, 4, 5, 6))


# ---- 5. one LM step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", [("full", 1), ("windowed", 2)], ids=["default_route", "segmented_chain"])
def test_lm_step_against_the_augmented_normal_equations(built, monkeypatch, name, route):
    set_route_env(monkeypatch, {})
    pa = problem_of(name)
    ids, means, infos = prior_set(name, seed=3)
    radius = 1e4
    ne0 = free_equations(name, radius)
    ne = ppr.PointPriorEquations(pa, radius, ids, means, infos)
    S_, rhs, g_red, gp, Ui = ppr.reduced_system(ne)
    ref_sw = types.SimpleNamespace(S=S_, rhs=rhs, point_hessian_inv=Ui, n_promoted=len(ne.promoted))
    with BundleAdjustment(pa, point_priors=(ids, means, infos)) as ba:
        sw = ba.sweep(radius, want_matrices=True)
        st = ba.debug_step()
    assert st.route == route and st.chol_fail == 0.0
    n_red = sw.n_reduced
    e_S, e_rhs = scaled_max_err(sw.S, ref_sw.S), vec_err(sw.rhs, ref_sw.rhs)
    print(f"[{name}] S {e_S:.2e}  rhs {e_rhs:.2e}")
    assert e_S <= 1e-9 and e_rhs <= 1e-9
    # the solver alone, on its own system
    eta_gpu = sr.solve_eta(sw.S, sw.rhs, st.delta_reduced)
    eta_lapack = sr.solve_eta(sw.S, sw.rhs, np.linalg.solve(sw.S, sw.rhs))
    bound = MARGIN * max(eta_lapack, n_red * sr.EPS)
    print(f"[{name}] eta solver {eta_gpu:.3e}  lapack {eta_lapack:.3e}  bound {bound:.3e}")
    assert eta_gpu <= bound
    # the whole step on the augmented normal equations
    eB_ref, eP_ref = ne.eta(sr.reference_step(ne, ref_sw))
    eB, eP = ne.eta(ne.split(st.delta_reduced, st.delta_points))
    bB, bP = MARGIN * max(eB_ref, ne.n * sr.EPS), MARGIN * max(eP_ref, ne.n * sr.EPS)
    print(f"[{name}] eta_B {eB:.3e}  reference {eB_ref:.3e}  bound {bB:.3e} | eta_P {eP:.3e}  reference {eP_ref:.3e}  bound {bP:.3e}")
    assert eB <= bB and eP <= bP
    # the step of the prior-free equations is NOT a solution of the augmented ones: the measure sees the prior
    osw = sr.oracle_sweep(pa, radius)
    _, eP_free = ne.eta(sr.reference_step(ne0, osw))
    assert eP_free > 1e3 * bP
    # the candidate's cost carries the prior term at P + delta
    cc = candidate_cost(pa, ne, st)
    cp = ppr.prior_cost(pa.pts + st.delta_points, ids, means, infos)
    print(f"[{name}] cand_cost {st.cand_cost:.17g}  oracle at x + delta {cc:.17g} + prior {cp:.17g}")
    assert abs(st.cand_cost - (cc + cp)) <= 1e-10 * (cc + cp)
    assert cp > 1e-6 * cc


# ---- 6. solve ---------------------------------------------------------------------------------------------------------------------
def metric_priors(pts, ids, sigma):
    ids = np.asarray(ids, np.uint32)
    return ids, np.asarray(pts, np.float64).reshape(-1, 3)[ids].copy(), np.tile(np.eye(3) / sigma ** 2, (len(ids), 1, 1))


MARKS = (2, 9, 17, 26, 35)


def test_solve_is_stationary_for_the_augmented_cost_and_reproducible(built):
    """five control points (0.05 mm) make the augmented matrix non-singular; the parent's code path is made non-singular by holding
    frame 0 and fixing B.  q of the prior solve is at most 10 times q of the parent's path (the check and bar of
    tests/test_gpu_priors.py::test_solve_is_stationary_for_the_augmented_cost); a second run gives the same bits."""
    sc = scene_of("full")
    F = len(sc.views0.reshape(-1)) // 6
    pri = metric_priors(sc.pts0, MARKS, 0.05)
    runs = []
    for _ in range(2):
        pa = problem(sc)
        with BundleAdjustment(pa, options(deterministic=1), point_priors=pri) as ba:
            s = ba.performBundleAdjustment()
            sw = ba.sweep(UNDAMPED, want_matrices=True)
            pc = ba.point_prior_cost()
        runs.append((summary_tuple(s), pc, sweep_tuple(sw), pa.cam.tobytes(), pa.views.tobytes(), pa.pts.tobytes()))
    assert runs[0] == runs[1]
    q_prior = stationarity(sw)
    assert abs(s.final_cost - sw.cost) <= 1e-12 * sw.cost and pc > 0
    fixed = np.zeros(F, np.uint8); fixed[0] = 1
    pb = capi.ProblemArrays(sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.cam0, sc.views0, sc.pts0, sc.spx, sc.scale, sc.config, fixed_mask=1 << 2)
    with BundleAdjustment(pb) as ba:
        ba.set_fixed_frames(fixed)
        s0 = ba.performBundleAdjustment()
        sw0 = ba.sweep(UNDAMPED, want_matrices=True)
    q_parent = stationarity(sw0)
    print(f"q prior {q_prior:.3e} ({s.iterations} iterations, termination {s.termination}, cost {s.final_cost:.6e}, prior part {pc:.3e})  "
          f"q parent {q_parent:.3e} ({s0.iterations} iterations, termination {s0.termination}, cost {s0.final_cost:.6e})")
    assert s.termination in (1, 2, 3) and s0.termination in (1, 2, 3)
    assert q_prior <= 10.0 * q_parent


# ---- 7. the control chain ---------------------------------------------------------------------------------------------------------
def rms_of(st):
    return float(np.hypot(st.std_x, st.std_y))


def test_control_chain_align_then_solve_with_priors(built):
    sc = scene.make_scene(S(6, 40, None, 0x506, 101, noise_px=0.0))
    marks = np.array(MARKS)
    gt = sc.pts_gt.reshape(-1, 3)[marks]
    assert abs(np.linalg.det(np.column_stack([gt[1:4] - gt[0]]))) > 1.0 and np.linalg.matrix_rank(gt[1:] - gt[0]) == 3   # not coplanar
    start = problem(sc)
    with BundleAdjustment(start) as ba:
        st0 = ba.calcReprojectionError()
        ba.performBundleAdjustment()
        st_free = ba.calcReprojectionError()
    # the scene somewhere else: a rigid motion of ~0.3 rad and 200 mm
    rng = np.random.default_rng(41)
    ax = rng.normal(size=3); ax /= np.linalg.norm(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.3) * K + (1 - np.cos(0.3)) * K @ K
    t = rng.normal(size=3); t *= 200.0 / np.linalg.norm(t)
    v, p = lifcal_amd.alignApply(lifcal_amd.Alignment(1.0, R, t, 0.0, 0), sc.views0, sc.pts0)
    pa = problem(sc); pa.views[:] = v.reshape(-1); pa.pts[:] = p.reshape(-1)
    assert np.max(np.abs(pa.pts.reshape(-1, 3)[marks] - gt)) > 50.0
    al = lifcal_amd.alignScene(pa, marks, gt, with_scale=False)
    assert al.scale == 1.0 and al.n_used == 5 and al.rms < 2.0      # the start points are 0.5 mm off
    sigma = 1e-3
    with BundleAdjustment(pa, point_priors=(marks, gt, np.tile(np.eye(3) / sigma ** 2, (5, 1, 1)))) as ba:
        st1 = ba.calcReprojectionError()
        s = ba.performBundleAdjustment()
        st2 = ba.calcReprojectionError()
        pc = ba.point_prior_cost()
    d0 = max(abs(st1.std_x - st0.std_x), abs(st1.std_y - st0.std_y), abs(st1.mae_x - st0.mae_x), abs(st1.mae_y - st0.mae_y))
    dev = np.linalg.norm(pa.pts.reshape(-1, 3)[marks] - gt, axis=1)
    print(f"alignment rms {al.rms:.3e} mm; reprojection before the solve against the unmoved start {d0:.2e} px; termination {s.termination} after "
          f"{s.iterations} iterations, prior cost {pc:.3e}; marks off by {dev} mm (5 sigma = {5 * sigma}); rms {rms_of(st2):.3e} px against {rms_of(st_free):.3e} prior-free")
    assert d0 <= 1e-9 and st1.num_points == st0.num_points
    assert s.termination in (1, 2, 3)
    assert np.all(dev <= 5 * sigma)
    assert rms_of(st2) <= 1.01 * rms_of(st_free)


# ---- 8. covariance ----------------------------------------------------------------------------------------------------------------
def test_covariance_control_points_add_information_and_close_the_null_direction(built):
    from tests.test_gpu_priors import solved_full
    pa = solved_full()
    pri = metric_priors(pa.pts, MARKS, 1e-3)
    with BundleAdjustment(problem_copy(pa), options(deterministic=1)) as ba:
        c0 = ba.covariance(gauge_frame=0)
    with BundleAdjustment(problem_copy(pa), options(deterministic=1), point_priors=pri) as ba:
        c1 = ba.covariance(gauge_frame=0)
        assert ba.point_prior_cost() == 0.0          # at its own means
        ba.clear_point_priors()
        c2 = ba.covariance(gauge_frame=0)
    e = np.flatnonzero(c0.estimable)
    ratio = np.diag(c1.camera)[e] / np.diag(c0.camera)[e]
    print(f"null_rank {c0.null_rank} -> {c1.null_rank}; posterior / prior-free variance on the estimable slots {ratio}; camera_null {c0.camera_null}")
    assert c0.gauge_frame == 0 and c1.gauge_frame == 0
    assert np.all(c1.estimable[e]) and np.all(ratio <= 1.0 + 1e-9) and np.all(ratio > 0.0)
    assert c0.null_rank >= 1 and np.max(np.abs(c0.camera_null[0])) > 0 and not c0.estimable[2]
    assert c1.null_rank == 0 and c1.estimable[1] and c1.estimable[2] and np.all(np.isfinite(c1.camera_std[:5]))
    assert c2.null_rank == c0.null_rank and not c2.estimable[2]      # cleared: the null direction is back


# ---- 9. refusals ------------------------------------------------------------------------------------------------------------------
def test_set_point_priors_refusals_leave_the_handle_as_it_was(built):
    name = "full"
    ids, means, infos = prior_set(name, seed=7)
    with BundleAdjustment(problem_of(name), options(deterministic=1), point_priors=(ids, means, infos)) as ba:
        a = ba.sweep(1e4, want_matrices=True)
        other = ids.copy(); other[2] += 1
        assert other[2] not in ids
        with pytest.raises(LifcalError) as e:
            ba.set_point_priors(other, means, infos)                       # a different point set
        assert e.value.code == -1 and "point set" in str(e.value)
        with pytest.raises(LifcalError) as e:
            ba.set_point_priors(ids[:4], means[:4], infos[:4])             # a subset
        assert e.value.code == -1
        bad = infos.copy(); bad[1] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        with pytest.raises(LifcalError) as e:
            ba.set_point_priors(ids, means, bad)                           # not positive semi-definite
        assert e.value.code == -1 and "semi-definite" in str(e.value)
        b = ba.sweep(1e4, want_matrices=True)
        pc = ba.point_prior_cost()
        # and an accepted replacement does change the sweep
        ba.set_point_priors(ids, means, 2.0 * infos)
        c = ba.sweep(1e4, want_matrices=True)
        assert abs(ba.point_prior_cost() - 2.0 * pc) <= 1e-15 * pc
    assert sweep_tuple(a) == sweep_tuple(b)
    assert c.cost > b.cost
    with BundleAdjustment(problem_of(name), options(deterministic=1)) as ba:          # a handle from lifcal_ba_create
        a = ba.sweep(1e4, want_matrices=True)
        with pytest.raises(LifcalError) as e:
            ba.set_point_priors(ids, means, infos)
        assert e.value.code == -1 and "lifcal_ba_create_with_point_priors" in str(e.value)
        b = ba.sweep(1e4, want_matrices=True)
        assert ba.point_prior_cost() == 0.0
    assert sweep_tuple(a) == sweep_tuple(b)
    with pytest.raises(LifcalError) as e:
        BundleAdjustment(problem_of(name), options(world_size=2, rank=0), point_priors=(ids, means, infos))
    assert e.value.code == -1 and "world_size" in str(e.value)
    with pytest.raises(LifcalError) as e:
        BundleAdjustment(problem_of(name), None, point_priors=(np.array([1, 2, 40]), means[:3], infos[:3]))   # point 40 of 40
    assert e.value.code == -4
