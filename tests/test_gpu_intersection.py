"""Batched point intersection (include/lifcal_intersect.h) against the CPU oracle.

The reference of every point is the oracle's own solve of that point as a one-point <2,17,6,3> problem: the point's observations
with pt = 0, its start value, the camera constant by mask (fixed_mask = 0x1FFFF), the poses constant through
oracle.set_fixed_frames (cleared in a finally), config | 0x500, the same options.
Bars: the project's full-solve bars per point — identical iteration count, accepted / rejected steps and
termination, initial cost <= 1e-12 and final cost <= 1e-8 relative, point <= 1e-6 mm, RMS <= 1e-10, n_obs and inliers equal, radius
<= 1e-6 relative — and H <= 1e-9 block-scaled, g <= 1e-10 of the cancelling terms sqrt(H_jj 2 cost) against the oracle's sweep at the
intersected point (radius 1e30, min_lm_diagonal 1e-300, no Jacobi scaling): its point_hessian_inv is then the inverse of H, its
point_gradient is g (the measures of check_frame in tests/test_gpu_resection.py).
The point with ONE observation has no such reference: its H has rank 2, the oracle's inverse does not exist, and its cost is zero,
so there are no cancelling terms to measure g by.  Its H and g are compared with the sum over the oracle's autodiff residual block
(oracle.residual_block, Cauchy corrector applied here), H at the same 1e-9 block-scaled, g at sqrt(H_jj) * 1e-10: what a residual
that differs by the project's RMS bar of 1e-10 px moves J^T r by.
Measured on an MI355X over the 232 points checked below: H 3.4e-16 .. 7.8e-14, g 2.3e-16 .. 5.0e-13 of the cancelling terms (the
one-observation point: H 4.1e-16, g 1.1e-13 of its measure); relative to max |g| of the converged point (9e-10 .. 0.1) the same
differences read 2e-13 .. 5e-5, the larger the smaller |g| is (1e-5 at |g| = 6e-8, 5e-5 at 9e-10, the one-observation point): the
rounding of either arithmetic, and why that ratio is printed, not asserted."""
import functools

import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, _capi as capi, intersectPoints, scene
from tests import off_defaults as od
from tests.helpers import S, anisotropic_scene, spy_of, scaled_max_err, vec_err

pytestmark = pytest.mark.gpu

TERM_NONE, TERM_FUNCTION, TERM_PARAMETER, TERM_MAX_ITERATIONS = 0, 1, 2, 4
FAMILIES = [
    ("r2_tan_adj_robust", S(6, 40, None, 0xF06, 115, outlier_fraction=0.05)),
    ("r0", S(6, 40, None, 0x500, 7)),
    ("r1_tan_adj", S(6, 40, None, 0xD05, 9)),
    ("r2_tan", S(6, 40, None, 0x506, 11)),
]
LONG = S(20, 12, None, 0x306, 21, outlier_fraction=0.05)
LONG_OBS = [127, 127, 84, 147, 100, 150, 107, 156, 113, 133, 99, 108]
ERRS = {"H": [], "g": []}   # the measured H / g errors of every checked point (printed by the tests, module docstring)


@functools.lru_cache(maxsize=None)
def scene_of(key):
    return scene.make_scene(dict(FAMILIES + [("long", LONG)])[key])


def intersect(sc, keep=None, options=None, order=None, pts0=None, pt=None):
    """all points of the scene in ONE call, camera and poses at ground truth; keep: mask of the observations handed over,
    order: their order, pt / pts0: another point numbering"""
    idx = np.arange(sc.n_obs) if keep is None else np.flatnonzero(keep)
    if order is not None:
        idx = idx[order]
    points = sc.pt[idx] if pt is None else pt
    p0 = sc.pts0 if pts0 is None else pts0
    return intersectPoints(sc.cam_gt, sc.views_gt, sc.u[idx], sc.v[idx], sc.mcx[idx], sc.mcy[idx], points, sc.fr[idx], p0, sc.config, sc.spx, sc.scale,
                           spy=spy_of(sc), options=options)


def one_point_problem(sc, k, keep, point):
    m = (sc.pt == k) if keep is None else ((sc.pt == k) & keep)
    return capi.ProblemArrays(sc.u[m], sc.v[m], sc.mcx[m], sc.mcy[m], np.zeros(int(m.sum()), np.uint32), sc.fr[m], sc.cam_gt, sc.views_gt, point,
                              sc.spx, sc.scale, sc.config | 0x500, spy=spy_of(sc), fixed_mask=0x1FFFF)


def block_sums(sc, pa, point, loss_scale):
    """H = J^T J and g = J^T r of the point over the oracle's autodiff residual blocks, the Cauchy corrector (rho'' < 0) applied"""
    views = np.asarray(sc.views_gt).reshape(-1, 6)
    H, g = np.zeros((3, 3)), np.zeros(3)
    for i in range(pa.struct.n_obs):
        r, J = oracle.residual_block(sc.config | 0x500, 3, sc.cam_gt, views[pa.fr[i]], point, pa.u[i], pa.v[i], pa.mcx[i], pa.mcy[i], sc.spx, sc.scale,
                                     spy=spy_of(sc))
        J = J[:, 23:26]
        if sc.config & 0x200:
            w = 1.0 / np.sqrt(1.0 + float(r @ r) / loss_scale ** 2)
            r, J = r * w, J * w
        H += J.T @ J; g += J.T @ r
    return H, g


def check_point(sc, k, res, keep=None, options=None, pts0=None, single=False):
    """point k of the result against its one-point oracle solve: the table of the module docstring; returns the oracle's summary"""
    row = res.rows[k]
    start = np.asarray(sc.pts0 if pts0 is None else pts0).reshape(-1, 3)[k]
    oracle.set_fixed_frames(np.ones(len(sc.views_gt.reshape(-1)) // 6, np.uint8))
    try:
        pa = one_point_problem(sc, k, keep, start)
        s = oracle.solve(pa, options)
        st = oracle.reproj_stats(pa, 1.0)
        got = (int(row["iterations"]), int(row["successful_steps"]), int(row["unsuccessful_steps"]), int(row["termination"]))
        ref = (s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination)
        print(f"point {k}: n {row['n_obs']} (it, ok, rejected, termination) {got} oracle {ref}; cost {row['final_cost']:.12e} oracle {s.final_cost:.12e}; "
              f"point diff {np.max(np.abs(res.pts[k] - pa.pts)):.2e}; rms diff {abs(res.rms_x[k] - st.std_x):.2e} {abs(res.rms_y[k] - st.std_y):.2e}")
        assert got == ref
        assert abs(row["initial_cost"] - s.initial_cost) <= 1e-12 * s.initial_cost
        if single:
            assert row["final_cost"] <= 1e-10 and s.final_cost <= 1e-10   # one observation: the minimum is zero, no relative measure
        else:
            assert abs(row["final_cost"] - s.final_cost) <= 1e-8 * s.final_cost
        assert np.max(np.abs(res.pts[k] - pa.pts)) <= 1e-6
        assert abs(res.rms_x[k] - st.std_x) <= 1e-10 and abs(res.rms_y[k] - st.std_y) <= 1e-10
        assert int(row["n_obs"]) == pa.struct.n_obs == st.num_points and int(row["n_inliers"]) == st.num_inliers
        assert abs(row["final_radius"] - s.final_radius) <= 1e-6 * s.final_radius
        # H, g: at the point where the kernel evaluated them, the intersected point
        at = one_point_problem(sc, k, keep, res.pts[k])
        loss_scale = (options if options is not None else capi.default_options_py()).loss_scale
        if single:
            H_ref, g_ref = block_sums(sc, at, res.pts[k], loss_scale)
            g_terms = np.sqrt(np.abs(np.diag(H_ref)))
            assert np.linalg.matrix_rank(H_ref) == 2
        else:
            o = capi.default_options_py(); o.jacobi_scaling = 0; o.min_lm_diagonal = 1e-300; o.loss_scale = loss_scale
            sw = oracle.sweep(at, radius=1e30, options=o)
            H_ref, g_ref = np.linalg.inv(sw.point_hessian_inv.reshape(3, 3)), sw.point_gradient[:3]
            # g at a (near) minimiser: what is left of sums that cancel, so the error is relative to the size of those sums,
            # |J_j| |r| = sqrt(H_jj 2 cost) (check_frame's measure)
            g_terms = np.sqrt(np.abs(np.diag(H_ref)) * 2.0 * sw.cost)
    finally:
        oracle.set_fixed_frames(None)
    eh, eg = scaled_max_err(res.H[k], H_ref), float(np.max(np.abs(res.g[k] - g_ref) / g_terms))
    ERRS["H"].append(eh); ERRS["g"].append(eg)
    print(f"point {k}: H err {eh:.2e}  g err {eg:.2e} of the cancelling terms ({vec_err(res.g[k], g_ref):.2e} of max |g| = {np.max(np.abs(g_ref)):.2e})")
    assert eh <= 1e-9
    assert eg <= 1e-10
    return s


def print_ranges():
    print(f"measured over {len(ERRS['H'])} points so far: H {min(ERRS['H']):.1e} .. {max(ERRS['H']):.1e}, g {min(ERRS['g']):.1e} .. {max(ERRS['g']):.1e}")


@functools.lru_cache(maxsize=None)
def batch(key):
    return intersect(scene_of(key))


@pytest.mark.parametrize("key", [c[0] for c in FAMILIES])
def test_every_point_follows_its_one_point_oracle_solve(built, key):
    sc, res = scene_of(key), batch(key)
    n = np.bincount(sc.pt, minlength=40)
    assert res.pts.shape == (40, 3) and np.array_equal(res.n_obs, n)
    sums = [check_point(sc, k, res) for k in range(40)]
    print(f"{key}: observations per point {n.min()} .. {n.max()}, iterations {min(s.iterations for s in sums)} .. {max(s.iterations for s in sums)}, "
          f"terminations {sorted(set(s.termination for s in sums))}")
    print_ranges()
    assert set(s.termination for s in sums) <= {TERM_FUNCTION, TERM_PARAMETER}
    cov = res.point_covariance()
    assert np.all(np.isfinite(cov)) and np.allclose(np.einsum("pij,pjk->pik", cov, res.H), np.eye(3), atol=1e-6)


def test_both_tolerance_terminations_occur(built):
    """|x| of the parameter-tolerance test is that of the oracle's one-point program (17 camera values as stored + the point; the
    constant poses are no blocks): PARAMETER terminations occur in the named scenes, next to FUNCTION ones"""
    terms = np.concatenate([batch(c[0]).termination for c in FAMILIES])
    assert TERM_FUNCTION in terms and TERM_PARAMETER in terms


def test_rejected_steps_walk_the_decrease_factor_path(built):
    key = FAMILIES[0][0]
    sc = scene_of(key)
    pts0 = np.asarray(sc.pts_gt).reshape(-1, 3) + np.array([0.0, 0.0, 20000.0])
    res = intersect(sc, pts0=pts0)
    sums = [check_point(sc, k, res, pts0=pts0) for k in range(40)]
    print_ranges()
    assert all(9 <= s.iterations <= 17 and 1 <= s.unsuccessful_steps <= 8 and s.termination == TERM_FUNCTION for s in sums)
    assert (sums[3].iterations, sums[3].unsuccessful_steps) == (17, 5) and sums[17].unsuccessful_steps == 8
    assert (int(res.rows["iterations"][3]), int(res.rows["unsuccessful_steps"][3])) == (17, 5) and int(res.rows["unsuccessful_steps"][17]) == 8
    assert int(res.rows["unsuccessful_steps"].max()) >= 5
    # The same minimum as from pts0.  Both solves stop on the function tolerance, when one step lowers the cost by <= f_tol * cost
    # = 1e-6; an LM solve that converges at least linearly with a ratio <= 0.99 is then within 100 f_tol = 1e-4 * cost of the
    # minimum, which is the slack allowed here, not rounding.  In coordinates: each end point lies in the ellipsoid
    # 1/2 d^T H d <= 1e-4 * cost around the minimiser (H the Gauss-Newton matrix there), so the two are apart by at most twice its
    # half-axis in the H norm: 1/2 d^T H d <= 4e-4 * cost.  (A plain bound in mm would have to know how flat the depth direction of
    # each point is; H does.)
    near = batch(key)
    d = res.pts - near.pts
    dc = np.max(np.abs(res.final_cost - near.final_cost) / near.final_cost)
    dh = np.max(0.5 * np.einsum("pi,pij,pj->p", d, near.H, d) / near.final_cost)
    print(f"far start against pts0: points {np.max(np.abs(d)):.2e} mm apart, 1/2 d^T H d {dh:.2e} of the cost, final costs {dc:.2e} relative")
    assert dc <= 1e-4
    assert dh <= 4e-4


# away from the default scalars and options (tests/off_defaults.py): name -> (y pitch / x pitch, options, far start).  On the oracle's
# H at pts0 of r2_tan_adj_robust, h s^2 is 0.23 .. 0.61 in x and y and 5e-4 .. 0.04 in z: min_lm_diagonal = 0.9 clips all three of
# every point, max_lm_diagonal = 0.5 x and y of the points above it.  At the radius 1e4 the damping is 1e-4 of the Hessian, so each
# clamp runs once more where it decides the step: two iterations from the radius 1 (the oracle's cost then stands 6e-3 .. 0.6
# relative away from the one without min_lm_diagonal, and 1e-6 .. 0.2 without max_lm_diagonal on 24 of the 40 points)
TWO_STEPS = dict(initial_radius=1.0, max_iterations=2)
OFF_DEFAULTS = {
    "aniso_125": (od.A, {}, False),
    "loss_scale_02": (None, dict(loss_scale=0.2), False),
    "lm_min_binds": (None, dict(min_lm_diagonal=0.9), False),
    "lm_min_binds_two_steps": (None, dict(min_lm_diagonal=0.9, **TWO_STEPS), False),
    "lm_max_binds": (None, dict(max_lm_diagonal=0.5), False),
    "lm_max_binds_two_steps": (None, dict(max_lm_diagonal=0.5, **TWO_STEPS), False),
    "min_relative_decrease_09": (None, dict(min_relative_decrease=0.9), True),
    "initial_radius_small": (None, dict(initial_radius=1e-2), False),
}


def oracle_points(sc, options, pts0=None):
    """the oracle's one-point solves of all 40 points with `options`"""
    start = np.asarray(sc.pts0 if pts0 is None else pts0).reshape(-1, 3)
    oracle.set_fixed_frames(np.ones(len(sc.views_gt.reshape(-1)) // 6, np.uint8))
    try:
        return [oracle.solve(one_point_problem(sc, k, None, start[k]), options) for k in range(40)]
    finally:
        oracle.set_fixed_frames(None)


@pytest.mark.parametrize("name", list(OFF_DEFAULTS))
def test_points_follow_the_oracle_away_from_the_default_scalars_and_options(built, name):
    a, kw, far = OFF_DEFAULTS[name]
    key = FAMILIES[0][0]
    sc = scene_of(key) if a is None else anisotropic_scene(scene_of(key), a)
    o = od.options(**kw)
    pts0 = np.asarray(sc.pts_gt).reshape(-1, 3) + np.array([0.0, 0.0, 20000.0]) if far else None
    res = intersect(sc, options=o, pts0=pts0)
    sums = [check_point(sc, k, res, options=o, pts0=pts0) for k in range(40)]
    print_ranges()
    # the oracle's side of the case: what the scalar or option changed against the defaults
    if name == "aniso_125":
        iso = batch(key)   # the y errors are in pixels of another pitch (and weigh 1 / a^2 in the cost: not the same minimiser)
        assert np.median(np.abs(res.rms_y - iso.rms_y)) > 1e-3 and np.median(np.abs(res.rms_y - iso.rms_y)) > 10 * np.median(np.abs(res.rms_x - iso.rms_x))
    elif name == "min_relative_decrease_09":
        base = oracle_points(sc, od.options(), pts0)
        assert all(s.unsuccessful_steps > 0 for s in sums)
        assert sum(od.tuple_of(s) != od.tuple_of(b) for s, b in zip(sums, base)) >= 3   # and the option decided some of them
    elif name == "initial_radius_small":
        assert all(s.iterations >= b.iterations + 5 for s, b in zip(sums, oracle_points(sc, od.options())))
    elif name == "loss_scale_02":
        assert all(s.final_cost < b.final_cost for s, b in zip(sums, oracle_points(sc, od.options())))
    elif "two_steps" in name:
        d = np.array([abs(s.final_cost - b.final_cost) / b.final_cost for s, b in zip(sums, oracle_points(sc, od.options(**TWO_STEPS)))])
        assert np.sum(d > 1e-6) >= (40 if "min" in name else 20)


def test_more_observations_than_one_pass_of_the_wave(built):
    sc, res = scene_of("long"), batch("long")
    n = np.bincount(sc.pt, minlength=12)
    assert list(n) == LONG_OBS
    assert np.all(n > 64) and np.sum(n > 128) >= 3 and np.all(n % 64 != 0)   # two or three passes of the stride loop, a ragged last one
    for k in range(12):
        check_point(sc, k, res)
    print_ranges()


def reduced(sc):
    """the long scene with three points cut down and the last point dropped (11 points: the last workgroup has an idle wave)"""
    keep = sc.pt != 11
    keep[sc.pt == 1] = False                                   # point 1: no observations
    i4 = np.flatnonzero(sc.pt == 4); keep[i4[1:]] = False      # point 4: one observation
    i6 = np.flatnonzero(sc.pt == 6)                            # point 6: two observations in two different frames
    second = i6[np.flatnonzero(sc.fr[i6] != sc.fr[i6[0]])[0]]
    keep[i6] = False; keep[[i6[0], second]] = True
    return keep, np.asarray(sc.pts0).reshape(-1, 3)[:11]


def test_empty_point_one_and_two_observation_points_and_iteration_limit(built):
    sc = scene_of("long")
    keep, pts0 = reduced(sc)
    res = intersect(sc, keep, pts0=pts0)
    assert len(res.rows) == 11 and len(res.rows) % 4 != 0
    assert list(res.n_obs[[1, 4, 6]]) == [0, 1, 2]
    assert not res.rows[1:2].view(np.uint8).any() and res.rows["termination"][1] == TERM_NONE
    assert res.pts[1].tobytes() == pts0[1].tobytes()
    assert np.isnan(res.rms_x[1]) and np.isnan(res.rms_y[1]) and np.all(np.isnan(res.point_covariance()[1]))
    for k in range(11):
        if k != 1:
            check_point(sc, k, res, keep, pts0=pts0, single=(k == 4))
    o = capi.default_options_py(); o.max_iterations = 2
    res2 = intersect(sc, keep, options=o, pts0=pts0)
    for k in range(11):
        if k != 1:
            assert res2.rows["termination"][k] in (TERM_FUNCTION, TERM_PARAMETER, TERM_MAX_ITERATIONS) and res2.rows["iterations"][k] <= 2
            assert res2.rows["termination"][k] == TERM_MAX_ITERATIONS or res.rows["iterations"][k] <= 2   # an earlier end is the unlimited solve's
            check_point(sc, k, res2, keep, options=o, pts0=pts0, single=(k == 4))
    assert TERM_MAX_ITERATIONS in res2.rows["termination"]
    assert res2.rows["termination"][1] == TERM_NONE and not res2.rows[1:2].view(np.uint8).any()
    print_ranges()


def test_non_finite_start_keeps_the_point_and_reports_minus_one(built):
    """a start value whose cost is not finite (NaN, infinite coordinates): the point keeps its bits, termination -1, no iteration;
    its neighbours in the same workgroup are solved as if it were not there"""
    key = FAMILIES[0][0]
    sc, res = scene_of(key), batch(key)
    pts0 = np.asarray(sc.pts0, np.float64).reshape(-1, 3).copy()
    pts0[5] = np.nan; pts0[18, 2] = np.inf
    bad = intersect(sc, pts0=pts0)
    for k in (5, 18):
        row = bad.rows[k]
        assert int(row["termination"]) == -1 and int(row["iterations"]) == 0 and int(row["successful_steps"]) == 0 and int(row["unsuccessful_steps"]) == 0
        assert not np.isfinite(row["initial_cost"]) and int(row["n_obs"]) == int(res.rows["n_obs"][k])
        assert bad.pts[k].tobytes() == pts0[k].tobytes()
    others = np.setdiff1d(np.arange(40), [5, 18])
    assert bad.rows[others].tobytes() == res.rows[others].tobytes() and bad.pts[others].tobytes() == res.pts[others].tobytes()


def test_bitwise_reproducible_and_points_independent(built):
    key = FAMILIES[0][0]
    sc, res = scene_of(key), batch(key)
    again = intersect(sc)
    assert again.rows.tobytes() == res.rows.tobytes() and again.pts.tobytes() == res.pts.tobytes()
    # point 3 alone
    m = sc.pt == 3
    alone = intersect(sc, m, pts0=np.asarray(sc.pts0).reshape(-1, 3)[3], pt=np.zeros(int(m.sum()), np.uint32))
    assert len(alone.rows) == 1
    assert alone.rows[0].tobytes() == res.rows[3].tobytes() and alone.pts[0].tobytes() == res.pts[3].tobytes()
    # the points' observation blocks in reverse point order, the order inside a point unchanged
    order = np.concatenate([np.flatnonzero(sc.pt == k) for k in reversed(range(40))])
    rev = intersect(sc, order=order)
    assert rev.rows.tobytes() == res.rows.tobytes() and rev.pts.tobytes() == res.pts.tobytes()


def test_consistent_with_the_joint_solve(built):
    """Solve the 0x506 family jointly, then intersect the handle's points against its camera and poses: without constraints every
    observation belongs to one point, so the points' start costs add up to the joint solve's final cost."""
    sc = scene_of(FAMILIES[3][0])
    pa = capi.ProblemArrays.from_scene(sc)
    with BundleAdjustment(pa) as ba:
        s = ba.performBundleAdjustment()
        res = ba.intersectPoints()
    assert abs(res.rows["initial_cost"].sum() - s.final_cost) <= 1e-12 * s.final_cost
    assert np.all(res.rows["final_cost"] <= res.rows["initial_cost"])
    drop = float((res.rows["initial_cost"] - res.rows["final_cost"]).sum())
    move = float(np.max(np.abs(res.pts - pa.pts.reshape(-1, 3))))
    print(f"joint solve: {s.iterations} iterations, final cost {s.final_cost:.12e}; intersection lowers it by {drop:.3e} ({drop / s.final_cost:.2e} relative), "
          f"largest point move {move:.3e} mm (the f_tol slack of the joint solve)")
    # the free function with the handle's arrays: the same bits as the convenience method
    free = intersectPoints(pa.cam, pa.views, pa.u, pa.v, pa.mcx, pa.mcy, pa.pt, pa.fr, pa.pts, sc.config, sc.spx, sc.scale)
    assert free.rows.tobytes() == res.rows.tobytes() and free.pts.tobytes() == res.pts.tobytes()
