"""Batched pose resection (include/lifcal_resect.h) against the CPU oracle.

The reference of every frame is the oracle's own solve of that frame as a one-frame <2,17,6> problem: the frame's observations
with fr = 0, its start pose, camera and points constant (fixed_mask = 0x1FFFF, points not refined), the same config and options.
Bars: the project's full-solve bars per frame — identical iteration count, accepted / rejected steps and
termination, final cost <= 1e-8 relative, pose <= 1e-6, RMS <= 1e-10 — and H <= 1e-9 block-scaled, g <= 1e-10 against the oracle's
sweep at the final point (radius 1e30, min_lm_diagonal 1e-300, no Jacobi scaling: the route of systems_at in
tests/test_gpu_precision1.py, and that test's measure of a gradient at a minimiser: relative to the sums it cancels from).
Measured on an MI355X over all cases below: H 1e-16 .. 3e-14, g 8e-15 .. 4e-13 of the cancelling sums; relative to max |g| of the
converged frame (0.04 .. 70 where the sums are 1e5 .. 1e7) the same differences read 3e-11 .. 1e-7, which is the rounding of either
arithmetic and why that ratio is printed, not asserted."""
import functools

import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, _capi as capi, resectFrames, scene
from tests import off_defaults as od
from tests.helpers import S, anisotropic_scene, spy_of, scaled_max_err, vec_err

pytestmark = pytest.mark.gpu

TERM_NONE, TERM_FUNCTION, TERM_PARAMETER, TERM_MAX_ITERATIONS = 0, 1, 2, 4
FAMILIES = [
    ("r2_tan_robust", S(6, 40, None, 0x306, 115, outlier_fraction=0.05)),
    ("r0", S(6, 40, None, 0x100, 7)),
    ("r1_tan_adj_robust", S(6, 40, None, 0xB05, 9, outlier_fraction=0.05)),
    ("r2_tan_adj", S(6, 40, None, 0x906, 11)),
]
REJECTS = S(6, 40, None, 0x306, 115, outlier_fraction=0.05, init_rot_deg=25.0, init_trans_mm=100.0)
LONG = S(3, 150, None, 0x306, 21, outlier_fraction=0.05)
# starts from which some accepted steps of the defaults gain less than 0.9 of what the model promises (the oracle, defaults against
# min_relative_decrease = 0.9: frame 1 of the first (10, 9, 0, 1) -> (13, 9, 3, 1), frame 4 of the second (9, 8, 0, 1) -> (17, 11, 5, 1); the other frames unchanged)
REJECTS_FAR = S(6, 40, None, 0x306, 115, outlier_fraction=0.05, init_rot_deg=25.0, init_trans_mm=500.0)
REJECTS_117 = S(6, 40, None, 0x306, 117, outlier_fraction=0.05, init_rot_deg=35.0, init_trans_mm=100.0)


@functools.lru_cache(maxsize=None)
def scene_of(key):
    return scene.make_scene(dict(FAMILIES + [("rejects", REJECTS), ("rejects_far", REJECTS_FAR), ("rejects_117", REJECTS_117), ("long", LONG)])[key])


def resect(sc, keep=None, options=None, order=None, views0=None, fr=None, n_frames=None):
    """all frames of the scene in ONE call, camera and points at ground truth; keep: mask of the observations handed over,
    order: their order, fr / n_frames / views0: another frame numbering"""
    idx = np.arange(sc.n_obs) if keep is None else np.flatnonzero(keep)
    if order is not None:
        idx = idx[order]
    frames = sc.fr[idx] if fr is None else fr
    v0 = sc.views0 if views0 is None else views0
    assert n_frames is None or len(v0) == 6 * n_frames
    return resectFrames(sc.cam_gt, sc.pts_gt, sc.u[idx], sc.v[idx], sc.mcx[idx], sc.mcy[idx], sc.pt[idx], frames, v0, sc.config, sc.spx, sc.scale,
                        spy=spy_of(sc), options=options)


def one_frame_problem(sc, f, keep, view):
    m = (sc.fr == f) if keep is None else ((sc.fr == f) & keep)
    return capi.ProblemArrays(sc.u[m], sc.v[m], sc.mcx[m], sc.mcy[m], sc.pt[m], np.zeros(int(m.sum()), np.uint32), sc.cam_gt, view, sc.pts_gt,
                              sc.spx, sc.scale, sc.config, spy=spy_of(sc), fixed_mask=0x1FFFF)


def check_frame(sc, f, res, keep=None, options=None):
    """frame f of the result against its one-frame oracle solve: the table of the module docstring; returns the oracle's summary"""
    row = res.rows[f]
    pa = one_frame_problem(sc, f, keep, sc.views0[6 * f: 6 * f + 6])
    s = oracle.solve(pa, options)
    st = oracle.reproj_stats(pa, 1.0)
    got = (int(row["iterations"]), int(row["successful_steps"]), int(row["unsuccessful_steps"]), int(row["termination"]))
    ref = (s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination)
    print(f"frame {f}: n {row['n_obs']} (it, ok, rejected, termination) {got} oracle {ref}; cost {row['final_cost']:.12e} oracle {s.final_cost:.12e}; "
          f"pose diff {np.max(np.abs(res.views[f] - pa.views)):.2e}; rms diff {abs(res.rms_x[f] - st.std_x):.2e} {abs(res.rms_y[f] - st.std_y):.2e}")
    assert got == ref
    assert abs(row["initial_cost"] - s.initial_cost) <= 1e-12 * s.initial_cost
    assert abs(row["final_cost"] - s.final_cost) <= 1e-8 * s.final_cost
    assert np.max(np.abs(res.views[f] - pa.views)) <= 1e-6
    assert abs(res.rms_x[f] - st.std_x) <= 1e-10 and abs(res.rms_y[f] - st.std_y) <= 1e-10
    assert int(row["n_obs"]) == pa.struct.n_obs == st.num_points and int(row["n_inliers"]) == st.num_inliers
    assert abs(row["final_radius"] - s.final_radius) <= 1e-6 * s.final_radius
    # H, g: the oracle's sweep at the point where the kernel evaluated them, the resected pose
    o = capi.default_options_py(); o.jacobi_scaling = 0; o.min_lm_diagonal = 1e-300
    if options is not None:
        o.loss_scale = options.loss_scale
    sw = oracle.sweep(one_frame_problem(sc, f, keep, res.views[f]), radius=1e30, options=o)
    H_ref, g_ref = sw.S[17:23, 17:23], sw.gradient_reduced[17:23]
    # g at a (near) minimiser: its entries are what is left of sums that cancel by five to seven orders of magnitude, so the error of
    # either arithmetic is relative to the size of those sums, |J_j| |r| = sqrt(H_jj 2 cost), not to the remainder (the measure of
    # test_fp32_arm_converges_to_the_fp64_arm for a gradient at a minimiser, with the fp64 bar 1e-10 in place of its fp32 one)
    g_terms = np.sqrt(np.abs(np.diag(H_ref)) * 2.0 * sw.cost)
    eh, eg = scaled_max_err(res.H[f], H_ref), float(np.max(np.abs(res.g[f] - g_ref) / g_terms))
    print(f"frame {f}: H err {eh:.2e}  g err {eg:.2e} of the cancelling terms ({vec_err(res.g[f], g_ref):.2e} of max |g| = {np.max(np.abs(g_ref)):.2e})")
    assert eh <= 1e-9
    assert eg <= 1e-10
    assert abs(row["final_gradient_max_norm"] - np.max(np.abs(g_ref))) <= 1e-6 * np.max(np.abs(g_ref)) + 1e-9
    return s


@functools.lru_cache(maxsize=None)
def batch(key):
    return resect(scene_of(key))


@pytest.mark.parametrize("key", [c[0] for c in FAMILIES])
def test_every_frame_follows_its_one_frame_oracle_solve(built, key):
    sc, res = scene_of(key), batch(key)
    terms = set()
    for f in range(6):
        terms.add(check_frame(sc, f, res).termination)
    assert terms <= {TERM_FUNCTION, TERM_PARAMETER}
    cov = res.pose_covariance()
    assert np.all(np.isfinite(cov)) and np.allclose(np.einsum("fij,fjk->fik", cov, res.H), np.eye(6), atol=1e-6)


def test_rejected_steps_walk_the_decrease_factor_path(built):
    sc = scene_of("rejects")
    res = resect(sc)
    sums = [check_frame(sc, f, res) for f in range(6)]
    assert (sums[1].iterations, sums[1].successful_steps, sums[1].unsuccessful_steps) == (14, 9, 4)   # the case is the one the bars were set on
    assert all(s.unsuccessful_steps == 0 and 6 <= s.iterations <= 7 for k, s in enumerate(sums) if k != 1)
    assert int(res.rows["unsuccessful_steps"][1]) == 4


# away from the default scalars and options (tests/off_defaults.py): name -> (scene, y pitch / x pitch, options).  On the oracle's H at
# the start poses of r2_tan_robust, h s^2 of the three rotations is 0.92 .. 0.999 and of the three translations 0 .. 0.17, so
# max_lm_diagonal = 0.5 clips the former and min_lm_diagonal = 0.9 the latter, in every frame.  At the radius 1e4 the damping is
# 1e-4 of the Hessian and LM corrects what is left of a wrong one, so each clamp runs once more where it decides the step: two
# iterations from the radius 1, after which the oracle's cost stands 3e-4 .. 0.6 (relative) away from the one without the clamp
TWO_STEPS = dict(initial_radius=1.0, max_iterations=2)
OFF_DEFAULTS = {
    "aniso_125": ("r2_tan_robust", od.A, {}),
    "loss_scale_02": ("r2_tan_robust", None, dict(loss_scale=0.2)),
    "lm_min_binds": ("r2_tan_robust", None, dict(min_lm_diagonal=0.9)),
    "lm_min_binds_two_steps": ("r2_tan_robust", None, dict(min_lm_diagonal=0.9, **TWO_STEPS)),
    "lm_max_binds": ("r2_tan_robust", None, dict(max_lm_diagonal=0.5)),
    "lm_max_binds_two_steps": ("r2_tan_robust", None, dict(max_lm_diagonal=0.5, **TWO_STEPS)),
    "min_relative_decrease_09": ("rejects_far", None, dict(min_relative_decrease=0.9)),
    "min_relative_decrease_09_other_scene": ("rejects_117", None, dict(min_relative_decrease=0.9)),
    "initial_radius_small": ("r2_tan_robust", None, dict(initial_radius=1e-2)),
}


@pytest.mark.parametrize("name", list(OFF_DEFAULTS))
def test_frames_follow_the_oracle_away_from_the_default_scalars_and_options(built, name):
    key, a, kw = OFF_DEFAULTS[name]
    sc = scene_of(key) if a is None else anisotropic_scene(scene_of(key), a)
    o = od.options(**kw)
    res = resect(sc, options=o)
    sums = [check_frame(sc, f, res, options=o) for f in range(6)]
    # the oracle's side of the case: what the scalar or option changed against the defaults
    defaults = lambda **kw: [oracle.solve(one_frame_problem(sc, f, None, sc.views0[6 * f: 6 * f + 6]), od.options(**kw)) for f in range(6)]
    if name == "aniso_125":
        iso = batch(key)   # the y errors are in pixels of another pitch (and weigh 1 / a^2 in the cost: not the same minimiser)
        assert np.min(np.abs(res.rms_y - iso.rms_y)) > 1e-3 and np.min(np.abs(res.rms_y - iso.rms_y)) > 10 * np.min(np.abs(res.rms_x - iso.rms_x))
    elif name.startswith("min_relative_decrease_09"):   # the option decides: steps the defaults accept are rejected
        moved = [(od.tuple_of(s), od.tuple_of(b)) for s, b in zip(sums, defaults()) if od.tuple_of(s) != od.tuple_of(b)]
        print(f"{name}: (iterations, accepted, rejected, termination) with the option against the defaults: {moved}")
        assert moved and all(s[2] >= b[2] + 2 for s, b in moved)
    elif name == "initial_radius_small":
        assert all(s.iterations >= b.iterations + 5 for s, b in zip(sums, defaults()))
    elif name == "loss_scale_02":
        assert all(s.final_cost < 0.7 * b.final_cost for s, b in zip(sums, defaults()))
    elif "two_steps" in name:   # the cost after two steps is not the one with 1e-6 / 1e32, by a thousand times its bar at least
        assert all(abs(s.final_cost - b.final_cost) > 1e-5 * b.final_cost for s, b in zip(sums, defaults(**TWO_STEPS)))


def test_more_observations_than_one_pass_of_the_workgroup(built):
    sc, res = scene_of("long"), batch("long")
    n = np.bincount(sc.fr, minlength=3)
    assert np.all(n > 3 * 256) and np.all(n % 64 != 0)   # several passes of the stride loop, a ragged last wave
    for f in range(3):
        check_frame(sc, f, res)


def test_empty_frame_two_point_frame_and_iteration_limit(built):
    sc = scene_of("long")
    keep = np.ones(sc.n_obs, bool)
    keep[sc.fr == 1] = False                      # frame 1: no observations
    keep[(sc.fr == 0) & (sc.pt > 1)] = False      # frame 0: the observations of points 0 and 1
    assert keep[sc.fr == 0].sum() == 13
    res = resect(sc, keep)
    assert not res.rows[1:2].view(np.uint8).any() and res.rows["termination"][1] == TERM_NONE
    assert res.views[1].tobytes() == sc.views0[6:12].tobytes()
    assert np.isnan(res.rms_x[1]) and np.all(np.isnan(res.pose_covariance()[1]))
    assert check_frame(sc, 0, res, keep).iterations == 6
    check_frame(sc, 2, res, keep)
    o = capi.default_options_py(); o.max_iterations = 2
    res2 = resect(sc, keep, options=o)
    for f in (0, 2):
        assert res2.rows["termination"][f] == TERM_MAX_ITERATIONS and res2.rows["iterations"][f] == 2
        check_frame(sc, f, res2, keep, options=o)
    assert res2.rows["termination"][1] == TERM_NONE


def test_bitwise_reproducible_and_frames_independent(built):
    key = FAMILIES[0][0]
    sc, res = scene_of(key), batch(key)
    again = resect(sc)
    assert again.rows.tobytes() == res.rows.tobytes() and again.views.tobytes() == res.views.tobytes()
    # frame 3 alone
    m = sc.fr == 3
    alone = resect(sc, m, views0=sc.views0[18:24], fr=np.zeros(int(m.sum()), np.uint32), n_frames=1)
    assert alone.rows[0].tobytes() == res.rows[3].tobytes() and alone.views[0].tobytes() == res.views[3].tobytes()
    # the frames' observation blocks in reverse frame order, the order inside a frame unchanged
    order = np.concatenate([np.flatnonzero(sc.fr == f) for f in reversed(range(6))])
    rev = resect(sc, order=order)
    assert rev.rows.tobytes() == res.rows.tobytes() and rev.views.tobytes() == res.views.tobytes()


def test_agrees_with_the_joint_solve_on_the_minimiser(built):
    """The same six frames as ONE <2,17,6> problem with every camera slot fixed: one trust-region radius and one set of
    termination tests for all frames, so only the minimiser is shared with the resection, not the trajectory."""
    key = FAMILIES[0][0]
    sc, res = scene_of(key), batch(key)
    pa = capi.ProblemArrays(sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.cam_gt, sc.views0, sc.pts_gt, sc.spx, sc.scale, sc.config, fixed_mask=0x1FFFF)
    with BundleAdjustment(pa) as ba:
        s = ba.performBundleAdjustment()
        via_handle = ba.resectFrames(views0=sc.views0)
    dpose = np.max(np.abs(pa.views.reshape(-1, 6) - res.views))
    dcost = abs(s.final_cost - res.final_cost.sum()) / s.final_cost
    print(f"joint solve: {s.iterations} iterations, pose diff {dpose:.2e}, cost diff {dcost:.2e}")
    assert dpose <= 1e-5
    assert dcost <= 1e-6
    # the convenience of the handle: its camera and points (constant in this problem) and the same start poses give the same bits
    assert via_handle.rows.tobytes() == res.rows.tobytes() and via_handle.views.tobytes() == res.views.tobytes()
