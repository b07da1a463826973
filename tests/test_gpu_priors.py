"""Gaussian priors on camera and poses on the MI355X (include/lifcal_prior.h).

The oracle has no priors: every reference here is what the oracle gives plus the analytic terms of 1/2 d^T Lambda d
(tests/prior_reference.py).  Bars are the project's own (tests/test_gpu_parity.py, tests/test_gpu_step.py).
The priors of the sweep tests are scaled by the oracle's own diagonal, so that Lambda is of the size of S on every slot and a
misplaced entry stands out at O(1) of the block-scaled measure.

Figures measured on an MI355X: DESIGN.md section 7p."""
import functools
import re
import types

import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, LifcalError, _capi as capi, scene
from tests import prior_reference as pr
from tests import step_reference as sr
from tests.helpers import S, bounded_problem, problem, scaled_max_err, vec_err
from tests.test_gpu_covariance import problem_copy
from tests.test_gpu_step import MARGIN, candidate_cost, set_route_env

pytestmark = pytest.mark.gpu

UNDAMPED = 1e30   # the radius tests/test_gpu_covariance.py hands the oracle for undamped matrices
SCENES = {
    # the 6-frame / 40-point families of tests/test_gpu_resection.py
    "r0": S(6, 40, None, 0x100, 7),                                             # nc = 5
    "r2_tan_robust": S(6, 40, None, 0x306, 115, outlier_fraction=0.05),         # nc = 9
    "r1_tan_adj_robust": S(6, 40, None, 0xB05, 9, outlier_fraction=0.05),       # nc = 8
    # promoted points: the camera columns sit at 6 F + 3 Q, Q > 0
    "constraints": S(6, 40, None, 0x506, 117, n_constraints=3),
    "constraints_adj_robust": S(6, 40, None, 0xF06, 118, n_constraints=4, outlier_fraction=0.03),
    "full": S(6, 40, None, 0x506, 101),
    "recalib": S(8, 60, None, 0xF06, 120, recalib=True, outlier_fraction=0.02),
    "windowed": S(24, 120, 6, 0xF06, 119, outlier_fraction=0.02),
}


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return scene.make_scene(SCENES[name])


def options(**kw):
    o = capi.default_options_py()
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@functools.lru_cache(maxsize=None)
def oracle_sweep_of(name, radius):
    """computed once, shared, never written to"""
    sw = oracle.sweep(problem(scene_of(name)), radius=radius, threads=oracle.hardware_threads())
    assert sw.rc == 0
    for a in (sw.S, sw.rhs, sw.gradient_reduced):
        a.setflags(write=False)
    return sw


def spd(rng, n):
    A = rng.normal(size=(n, n))
    A = A @ A.T + 0.1 * np.eye(n)
    d = 1.0 / np.sqrt(np.diag(A))
    return A * np.outer(d, d)           # unit diagonal, dense off-diagonals


def scaled_priors(name, frames, seed=0, strength=0.3):
    """a dense camera prior (all 17 slots, the dead ones coupled too) and pose priors on `frames`, Lambda = strength s_i s_j R_ij
    with s = sqrt of the oracle's diagonal and R a random correlation matrix; means one scaled unit around the start values"""
    sc = scene_of(name)
    sw = oracle_sweep_of(name, UNDAMPED)
    rng = np.random.default_rng(1000 + seed)
    s = np.sqrt(np.abs(np.diag(sw.S)))
    sc_cam = s[:17]
    cam = (sc.cam0 + rng.normal(size=17) / sc_cam, strength * spd(rng, 17) * np.outer(sc_cam, sc_cam))
    F = len(sc.views0.reshape(-1)) // 6
    v0 = sc.views0.reshape(F, 6)
    means, infos = [], []
    for f in frames:
        sf = s[17 + 6 * f:23 + 6 * f]
        means.append(v0[f] + rng.normal(size=6) / sf)
        infos.append(strength * spd(rng, 6) * np.outer(sf, sf))
    return cam, (np.asarray(frames, np.uint32), np.array(means), np.array(infos))


def reduced_x(pa, n_reduced):
    x = np.zeros(n_reduced)
    x[:17] = pa.cam; x[17:17 + len(pa.views)] = pa.views
    return x


def block_scaled_vec(a, b, diag):
    d = np.sqrt(np.abs(diag)) + 1e-300
    return float(np.max(np.abs(a - b) / d) / (np.max(np.abs(b) / d) + 1e-300))


def check_prior_sweep(tag, got, base, Lam, mean, x, live, dead_identity=True):
    """`got` (with priors) against `base` (without) plus the analytic terms: the sweep bars of tests/test_gpu_parity.py, the vectors
    also in the block-scaled measure (one slot's error against that slot's scale)"""
    cost_p, Ld = pr.prior_terms(Lam, mean, x, live)
    L = pr.masked(Lam, live)
    ref_S, ref_rhs, ref_g, ref_cost = base.S + L, base.rhs - Ld, base.gradient_reduced + Ld, base.cost + cost_p
    dg = np.diag(ref_S)
    e_cost = abs(got.cost - ref_cost) / ref_cost
    e_S = scaled_max_err(got.S, ref_S)
    e_rhs, e_g = vec_err(got.rhs, ref_rhs), vec_err(got.gradient_reduced, ref_g)
    s_rhs, s_g = block_scaled_vec(got.rhs, ref_rhs, dg), block_scaled_vec(got.gradient_reduced, ref_g, dg)
    print(f"[{tag}] prior cost {cost_p:.6e} of {ref_cost:.6e}: cost {e_cost:.2e}  S {e_S:.2e}  rhs {e_rhs:.2e} ({s_rhs:.2e} block-scaled)  "
          f"gradient {e_g:.2e} ({s_g:.2e})  max |Lambda| / |S| {np.max(np.abs(np.diag(L)) / np.abs(np.diag(base.S))):.2f}")
    assert cost_p > 1e-6 * base.cost, "the prior is too weak to be seen in the cost"   # (six orders above the bar on the cost)
    assert e_cost <= 1e-12
    assert e_S <= 1e-9 and np.array_equal(got.S, got.S.T)
    assert e_rhs <= 1e-9 and s_rhs <= 1e-9
    assert e_g <= 1e-10 and s_g <= 1e-10
    if dead_identity:   # rows of fixed or absent slots are still identity rows with rhs 0
        n = len(live)
        dead = np.flatnonzero(~live)
        assert np.array_equal(got.S[dead], np.eye(n)[dead]) and np.array_equal(got.S[:, dead], np.eye(n)[:, dead])
        assert np.all(got.rhs[dead] == 0.0) and np.all(got.gradient_reduced[dead] == 0.0)


SWEEP_SCENES = ["r0", "r2_tan_robust", "r1_tan_adj_robust", "constraints", "constraints_adj_robust", "full"]


# ---- 1. one sweep -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [0, 1], ids=["hot_rows", "deterministic"])
@pytest.mark.parametrize("name", SWEEP_SCENES)
def test_one_sweep_against_the_oracle_plus_the_terms(built, name, deterministic):
    sc = scene_of(name)
    pa = problem(sc)
    F = pa.struct.n_frames
    ref = oracle_sweep_of(name, UNDAMPED)
    cam, poses = scaled_priors(name, (0, F // 2, F - 1))
    Lam, mean = pr.embed(F, ref.n_promoted, cam, poses)
    live = pr.live_slots(sc.config, sc.fixed_mask, F, ref.n_promoted)
    if name.startswith("constraints"):
        assert ref.n_promoted > 0
    with BundleAdjustment(pa, options(deterministic=deterministic)) as ba:
        ba.set_priors(camera=cam, poses=poses)
        got = ba.sweep(UNDAMPED, want_matrices=True)
        pc = ba.prior_cost()
    assert got.n_reduced == ref.n_reduced and got.n_promoted == ref.n_promoted
    check_prior_sweep(f"{name} det={deterministic}", got, ref, Lam, mean, reduced_x(pa, ref.n_reduced), live)
    cost_p, _ = pr.prior_terms(Lam, mean, reduced_x(pa, ref.n_reduced), live)
    assert abs(pc[0] + pc[1] - cost_p) <= 1e-12 * cost_p and pc[0] > 0 and (pc[1] > 0) == bool(sc.config & 0x100)


@pytest.mark.parametrize("name", ["r2_tan_robust", "constraints_adj_robust"])
def test_one_sweep_precision1_against_its_own_prior_free_sweep(built, name):
    sc = scene_of(name)
    pa = problem(sc)
    F = pa.struct.n_frames
    cam, poses = scaled_priors(name, (0, F // 2, F - 1), seed=1)
    with BundleAdjustment(pa, options(precision=1)) as ba:
        base = ba.sweep(UNDAMPED, want_matrices=True)
        ba.set_priors(camera=cam, poses=poses)
        got = ba.sweep(UNDAMPED, want_matrices=True)
    Lam, mean = pr.embed(F, base.n_promoted, cam, poses)
    live = pr.live_slots(sc.config, sc.fixed_mask, F, base.n_promoted)
    check_prior_sweep(f"{name} precision=1", got, base, Lam, mean, reduced_x(pa, base.n_reduced), live)


# ---- 2. dropped slots -------------------------------------------------------------------------------------------------------------
def sweep_tuple(sw):
    """every output of a sweep as bits (x + 0.0: the sign of a zero is no bit of the result)"""
    return (sw.cost, sw.gradient_max_norm) + tuple((a + 0.0).tobytes() for a in (sw.S, sw.rhs, sw.gradient_reduced, sw.point_gradient, sw.point_hessian_inv))


def test_slots_that_are_not_free_leave_the_prior(built):
    """recalib: fL and B are in fixed_mask, the camera matrix couples them; frame 2 is held by set_fixed_frames and has a pose prior"""
    name = "recalib"
    sc = scene_of(name)
    F = len(sc.views0.reshape(-1)) // 6
    assert sc.fixed_mask == 0b101
    cam, poses = scaled_priors(name, (0, 2, F - 1), seed=2)
    assert cam[1][0, 1] != 0 and cam[1][2, 3] != 0
    keep = np.ones(17, bool); keep[[0, 2]] = False
    cam_zeroed = (cam[0], cam[1] * np.outer(keep, keep))
    infos_zeroed = poses[2].copy(); infos_zeroed[1] = 0.0                     # frame 2's matrix zeroed
    poses_zeroed = (poses[0], poses[1], infos_zeroed)
    fixed = np.zeros(F, np.uint8); fixed[2] = 1
    det = options(deterministic=1)
    with BundleAdjustment(problem(sc), det) as ba:
        ba.set_priors(camera=cam, poses=poses)
        ba.set_fixed_frames(fixed)                      # after the priors: the mask is applied again before the sweep
        a = ba.sweep(1e4, want_matrices=True)
        ca = ba.prior_cost()
        ba.set_fixed_frames(None)
        a_free = ba.sweep(1e4, want_matrices=True)      # the pose prior of frame 2 is active again
    with BundleAdjustment(problem(sc), det) as ba:
        ba.set_fixed_frames(fixed)
        ba.set_priors(camera=cam_zeroed, poses=poses_zeroed)
        b = ba.sweep(1e4, want_matrices=True)
        cb = ba.prior_cost()
    with BundleAdjustment(problem(sc), det) as ba:
        ba.set_priors(camera=cam_zeroed, poses=poses)
        c_free = ba.sweep(1e4, want_matrices=True)
    assert sweep_tuple(a) == sweep_tuple(b) and ca == cb
    assert sweep_tuple(a_free) == sweep_tuple(c_free)
    assert a_free.cost > a.cost                          # frame 2's term
    # and against the oracle, which holds frame 2 as well
    ref = sr.oracle_sweep(problem(sc), 1e4, fixed_frames=fixed)
    Lam, mean = pr.embed(F, 0, cam, poses)
    live = pr.live_slots(sc.config, sc.fixed_mask, F, 0, fixed)
    # (the damped radius: the LM diagonal moves with the prior's diagonal, so S is compared off the diagonal and through rhs)
    cost_p, Ld = pr.prior_terms(Lam, mean, reduced_x(problem(sc), ref.n_reduced), live)
    assert abs(a.cost - (ref.cost + cost_p)) <= 1e-12 * a.cost
    assert vec_err(a.gradient_reduced, ref.gradient_reduced + Ld) <= 1e-10
    off = ~np.eye(ref.n_reduced, dtype=bool)
    refS = ref.S + pr.masked(Lam, live)
    assert np.max(np.abs(a.S - refS)[off] / np.sqrt(np.abs(np.outer(np.diag(refS), np.diag(refS))))[off]) <= 1e-9


# ---- 3. one LM step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,route", [("full", 1), ("windowed", 2)], ids=["default_route", "segmented_chain"])
def test_lm_step_against_the_augmented_normal_equations(built, monkeypatch, name, route):
    set_route_env(monkeypatch, {})
    sc = scene_of(name)
    pa = problem(sc)
    F = pa.struct.n_frames
    cam, poses = scaled_priors(name, (0, F // 2, F - 1), seed=3)
    Lam, mean = pr.embed(F, 0, cam, poses)
    live = pr.live_slots(sc.config, sc.fixed_mask, F)
    radius = 1e4
    ne0 = sr.NormalEquations(pa, radius)
    ne = pr.PriorEquations(pa, radius, Lam, mean)
    osw = sr.oracle_sweep(pa, radius)
    cost_p, Ld = pr.prior_terms(Lam, mean, reduced_x(pa, osw.n_reduced), live)
    # the oracle's reduced system + the terms; the LM diagonal of the reduced slots moves with the prior's diagonal
    dlam = ne.reduced(np.asarray(ne.lam - ne0.lam, np.float64))
    ref_sw = types.SimpleNamespace(S=osw.S + pr.masked(Lam, live) + np.diag(dlam), rhs=osw.rhs - Ld, point_hessian_inv=osw.point_hessian_inv,
                                   n_promoted=osw.n_promoted)
    with BundleAdjustment(pa) as ba:
        ba.set_priors(camera=cam, poses=poses)
        sw = ba.sweep(radius, want_matrices=True)
        st = ba.debug_step()
    assert st.route == route and st.chol_fail == 0.0
    n_red = sw.n_reduced
    assert scaled_max_err(sw.S, ref_sw.S) <= 1e-9 and vec_err(sw.rhs, ref_sw.rhs) <= 1e-9
    # (b) the solver alone, on its own system
    eta_gpu = sr.solve_eta(sw.S, sw.rhs, st.delta_reduced)
    eta_lapack = sr.solve_eta(sw.S, sw.rhs, np.linalg.solve(sw.S, sw.rhs))
    bound = MARGIN * max(eta_lapack, n_red * sr.EPS)
    print(f"[{name}] (b) eta solver {eta_gpu:.3e}  lapack {eta_lapack:.3e}  bound {bound:.3e}")
    assert eta_gpu <= bound
    # (c) the whole step on the augmented normal equations
    eB_ref, eP_ref = ne.eta(sr.reference_step(ne, ref_sw))
    eB, eP = ne.eta(ne.split(st.delta_reduced, st.delta_points))
    bB, bP = MARGIN * max(eB_ref, ne.n * sr.EPS), MARGIN * max(eP_ref, ne.n * sr.EPS)
    print(f"[{name}] (c) eta_B {eB:.3e}  reference {eB_ref:.3e}  bound {bB:.3e} | eta_P {eP:.3e}  reference {eP_ref:.3e}  bound {bP:.3e}")
    assert eB <= bB and eP <= bP
    # the step of the prior-free equations is NOT a solution of the augmented ones: the measure sees the prior
    eB_free, _ = ne.eta(sr.reference_step(ne0, osw))
    assert eB_free > 1e3 * bB
    # the candidate's cost carries the prior term at x + delta
    cc = candidate_cost(pa, ne, st)
    xc = reduced_x(pa, n_red) + st.delta_reduced
    cp, _ = pr.prior_terms(Lam, mean, xc, live)
    print(f"[{name}] cand_cost {st.cand_cost:.17g}  oracle at x + delta {cc:.17g} + prior {cp:.17g}")
    assert abs(st.cand_cost - (cc + cp)) <= 1e-10 * (cc + cp)
    assert cp > 1e-6 * cc


# ---- 4. no prior, no change -------------------------------------------------------------------------------------------------------
def summary_tuple(s):
    return (s.initial_cost, s.final_cost, s.final_radius, s.final_gradient_max_norm, s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination)


def test_without_a_prior_nothing_changes(built):
    name = "constraints_adj_robust"
    sc = scene_of(name)
    cam, poses = scaled_priors(name, (0, 3, 5), seed=4)
    zero_cam = (cam[0], np.zeros((17, 17)))
    zero_poses = (poses[0], poses[1], np.zeros((3, 6, 6)))
    results = []
    for mode in ("never", "zero", "cleared"):
        pa = problem(sc)
        with BundleAdjustment(pa, options(deterministic=1)) as ba:
            if mode == "zero":
                ba.set_priors(camera=zero_cam, poses=zero_poses)
            if mode == "cleared":
                ba.set_priors(camera=cam, poses=poses)
                ba.sweep(1e4)
                ba.clear_priors()
                assert ba.prior_cost() == (0.0, 0.0)
            sw = ba.sweep(1e4, want_matrices=True)
            s = ba.performBundleAdjustment()
        results.append((sweep_tuple(sw), summary_tuple(s), pa.cam.tobytes(), pa.views.tobytes(), pa.pts.tobytes()))
    assert results[0] == results[1], "all-zero matrices changed a bit"
    assert results[0] == results[2], "clear_priors left something behind"


# ---- 5. solves --------------------------------------------------------------------------------------------------------------------
def prior_free_sweep_at(pa, radius=UNDAMPED, fixed=None, opts=None):
    with BundleAdjustment(problem_copy(pa), opts) as ba:
        if fixed is not None:
            ba.set_fixed_frames(fixed)
        return ba.sweep(radius, want_matrices=True)


def test_solve_a_strong_prior_pins_B(built):
    """(a) |B - mean| / mean against |g_B| / Lambda_BB, (b) final_cost = observations + prior at the returned parameters"""
    sc = scene_of("full")
    pa = problem(sc)
    mean = sc.cam0.copy()
    info = np.zeros((17, 17)); info[2, 2] = 1e12 / mean[2] ** 2
    with BundleAdjustment(pa) as ba:
        ba.set_priors(camera=(mean, info))
        s = ba.performBundleAdjustment()
        pc = ba.prior_cost()
        ba.clear_priors()
        free = ba.sweep(UNDAMPED, want_matrices=True)     # the observations alone at the returned (device-resident) parameters
    assert s.termination in (1, 2, 3), s.termination
    g_B = free.gradient_reduced[2]
    dev, predicted = abs(pa.cam[2] - mean[2]) / mean[2], abs(g_B) / info[2, 2]
    print(f"B {pa.cam[2]!r} mean {mean[2]!r}: |B - mean| / mean {dev:.3e}  |g_B| / Lambda_BB {predicted:.3e}  g_B {g_B:.6e}  iterations {s.iterations}")
    print(f"final_cost {s.final_cost!r}  observations {free.cost!r} + prior {pc[0]!r}")
    assert dev <= predicted
    assert abs(s.final_cost - (free.cost + pc[0])) <= 1e-12 * s.final_cost
    assert pc[1] == 0.0


def stationarity(sw):
    """q = 1/2 rhs^T S^-1 rhs / cost of an undamped sweep: the relative cost decrease the Gauss-Newton model still sees"""
    return float(0.5 * sw.rhs @ np.linalg.solve(sw.S, sw.rhs) / sw.cost)


def test_solve_is_stationary_for_the_augmented_cost(built):
    """(c) priors on frame 0 (6 x 6) and on B make the augmented matrix non-singular; the parent's code path is made non-singular by
    holding frame 0 and fixing B.  q of the prior solve is at most 10 times q of the parent's path."""
    sc = scene_of("full")
    F = len(sc.views0.reshape(-1)) // 6
    rng = np.random.default_rng(5)
    info = np.zeros((17, 17)); info[2, 2] = 1.0 / (0.01 * sc.cam0[2]) ** 2
    A = spd(rng, 6)
    sig = np.array([1e-3, 1e-3, 1e-3, 0.05, 0.05, 0.05])                      # rad, mm
    poses = (np.array([0]), sc.views0.reshape(F, 6)[:1], A / np.outer(sig, sig))
    pa = problem(sc)
    with BundleAdjustment(pa) as ba:
        ba.set_priors(camera=(sc.cam0, info), poses=poses)
        s = ba.performBundleAdjustment()
        sw = ba.sweep(UNDAMPED, want_matrices=True)
        pc = ba.prior_cost()
    q_prior = stationarity(sw)
    assert abs(s.final_cost - sw.cost) <= 1e-12 * sw.cost and pc[0] > 0 and pc[1] > 0
    # the parent's path
    fixed = np.zeros(F, np.uint8); fixed[0] = 1
    pb = capi.ProblemArrays(sc.u, sc.v, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.cam0, sc.views0, sc.pts0, sc.spx, sc.scale, sc.config, fixed_mask=1 << 2)
    with BundleAdjustment(pb) as ba:
        ba.set_fixed_frames(fixed)
        s0 = ba.performBundleAdjustment()
        sw0 = ba.sweep(UNDAMPED, want_matrices=True)
    q_parent = stationarity(sw0)
    print(f"q prior {q_prior:.3e} ({s.iterations} iterations, termination {s.termination}, cost {s.final_cost:.6e})  "
          f"q parent {q_parent:.3e} ({s0.iterations} iterations, termination {s0.termination}, cost {s0.final_cost:.6e})")
    assert s.termination in (1, 2, 3) and s0.termination in (1, 2, 3)
    assert q_prior <= 10.0 * q_parent


def test_solve_recalib_with_box_bounds_and_a_camera_prior(built, monkeypatch, capfd):
    """(d) the line-search path: terminates by a tolerance, every accepted step lowered the augmented cost (the x_cost column of
    LIFCAL_TRACE), final_cost = observations + prior"""
    monkeypatch.setenv("LIFCAL_TRACE", "1")
    sc = scene_of("recalib")
    pa = bounded_problem(sc)
    assert pa.lower is not None
    info = np.zeros((17, 17))
    for k in (1, 3, 4):
        info[k, k] = 1.0 / (0.02 * abs(sc.cam0[k]) + 1e-3) ** 2
    info[3, 4] = info[4, 3] = 0.5 * np.sqrt(info[3, 3] * info[4, 4])
    with BundleAdjustment(pa) as ba:
        ba.set_priors(camera=(sc.cam0, info))
        capfd.readouterr()
        s = ba.performBundleAdjustment()
        err = capfd.readouterr().err
        pc = ba.prior_cost()
        ba.clear_priors()
        free = ba.sweep(UNDAMPED)
    costs = [float(m) for m in re.findall(r"x_cost (\S+) cand", err)] + [float(m) for m in re.findall(r"done: .* cost (\S+)", err)]
    changes = [b - a for a, b in zip(costs, costs[1:]) if b != a]
    print(f"termination {s.termination} iterations {s.iterations} accepted {s.successful_steps}; {len(costs)} cost samples, {len(changes)} changes, "
          f"largest {max(changes, default=0.0):.3e}; final {s.final_cost!r} = {free.cost!r} + {pc[0]!r}")
    assert s.termination in (1, 2, 3), s.termination
    assert len(costs) >= 2 and costs[0] == s.initial_cost and costs[-1] == s.final_cost
    assert len(changes) == s.successful_steps and all(c < 0 for c in changes)
    assert pc[0] > 0 and abs(s.final_cost - (free.cost + pc[0])) <= 1e-12 * s.final_cost
    assert np.all(pa.cam[[1, 3, 4]] >= pa.lower[[1, 3, 4]]) and np.all(pa.cam[[1, 3, 4]] <= pa.upper[[1, 3, 4]])


# ---- 6. covariance ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solved_full():
    pa = problem(scene_of("full"))
    oracle.solve(pa, threads=oracle.hardware_threads())
    for a in (pa.cam, pa.views, pa.pts):
        a.setflags(write=False)
    return pa


@functools.lru_cache(maxsize=None)
def covariances_around_a_prior_on_B():
    """(sigma, covariance without the prior, with a prior of standard deviation 1 % of B on B, after clear_priors)"""
    pa = solved_full()
    with BundleAdjustment(problem_copy(pa), options(deterministic=1)) as ba:
        c0 = ba.covariance()
        sigma = 0.01 * pa.cam[2]
        info = np.zeros((17, 17)); info[2, 2] = 1.0 / sigma ** 2
        ba.set_priors(camera=(pa.cam, info))
        c1 = ba.covariance()
        ba.clear_priors()
        c2 = ba.covariance()
    print(f"null_rank {c0.null_rank} -> {c1.null_rank}; var(B) {c1.camera[2, 2]!r} against sigma^2 {sigma ** 2!r}; std(bL0) {np.sqrt(c1.camera[1, 1]):.3e}")
    return sigma, c0, c1, c2


def test_covariance_a_prior_on_B_closes_the_null_direction(built):
    sigma, c0, c1, c2 = covariances_around_a_prior_on_B()
    assert c0.null_rank >= 1 and not c0.estimable[1] and not c0.estimable[2]
    assert c1.null_rank == 0 and c1.estimable[1] and c1.estimable[2]
    assert c1.camera[2, 2] > 0 and np.isfinite(c1.camera_std[1])
    assert c1.cost == c0.cost                    # d = 0: the prior adds nothing to the cost at its own mean
    assert np.array_equal(c2.camera, c0.camera) and c2.null_rank == c0.null_rank


def test_covariance_variance_of_B_is_at_most_the_prior_variance(built):
    """var(B) <= sigma^2, as the issue states it, with no allowance.  The observations of this scene carry no information on B alone
    (B and bL0 share the null direction), so the posterior variance EQUALS sigma^2 in exact arithmetic and the comparison is one
    between two roundings.  Measured on an MI355X: var(B) = 1.6019600596239026e-05, sigma^2 = 1.6019600596238968e-05, 3.6e-15
    relative ABOVE: this test fails by that rounding; the other properties of the case are held by the test above."""
    sigma, c0, c1, c2 = covariances_around_a_prior_on_B()
    assert c1.camera[2, 2] <= sigma ** 2, (c1.camera[2, 2], sigma ** 2, c1.camera[2, 2] / sigma ** 2 - 1.0)


def test_covariance_posterior_is_at_most_the_prior(built):
    pa = solved_full()
    with BundleAdjustment(problem_copy(pa), options(deterministic=1)) as ba:
        c0 = ba.covariance()
    info, rank = c0.camera_information()
    e = np.flatnonzero(c0.estimable)
    assert rank == len(e) and len(e) >= 5
    with BundleAdjustment(problem_copy(pa), options(deterministic=1)) as ba:
        ba.set_priors(camera=(pa.cam, info))
        c1 = ba.covariance()
    ratio = np.diag(c1.camera)[e] / np.diag(c0.camera)[e]
    print(f"posterior / prior variance on the estimable slots {ratio}")
    assert np.array_equal(c1.estimable, c0.estimable)
    assert np.all(ratio <= 1.0) and np.all(ratio > 0.0)
    # same observations, the prior is their own information: the variance halves
    assert np.allclose(ratio, 0.5, atol=1e-3)


# ---- 7. reproducibility, refusals -------------------------------------------------------------------------------------------------
def test_a_solve_with_priors_is_reproducible(built):
    name = "constraints_adj_robust"
    sc = scene_of(name)
    cam, poses = scaled_priors(name, (0, 3, 5), seed=6, strength=0.05)
    runs = []
    for _ in range(2):
        pa = problem(sc)
        with BundleAdjustment(pa, options(deterministic=1)) as ba:
            ba.set_priors(camera=cam, poses=poses)
            s = ba.performBundleAdjustment()
            pc = ba.prior_cost()
        runs.append((summary_tuple(s), pc, pa.cam.tobytes(), pa.views.tobytes(), pa.pts.tobytes()))
    assert runs[0] == runs[1]
    assert runs[0][0][7] in (1, 2, 3) and runs[0][1][0] > 0 and runs[0][1][1] > 0


def test_set_priors_refusals_leave_the_handle_as_it_was(built):
    sc = scene_of("full")
    cam, poses = scaled_priors("full", (0, 3, 5), seed=7)
    with BundleAdjustment(problem(sc), options(deterministic=1)) as ba:
        ba.set_priors(camera=cam, poses=poses)
        a = ba.sweep(1e4, want_matrices=True)
        bad = cam[1].copy(); bad[0, 0] = -1.0
        with pytest.raises(LifcalError) as e:
            ba.set_priors(camera=(cam[0], bad))
        assert e.value.code == -1
        with pytest.raises(LifcalError) as e:
            ba.set_priors(poses=(np.array([0, 3, 6]), poses[1], poses[2]))      # frame 6 of 6
        assert e.value.code == -4
        b = ba.sweep(1e4, want_matrices=True)
    assert sweep_tuple(a) == sweep_tuple(b)
    with BundleAdjustment(problem(sc), options(world_size=2, rank=0)) as ba:
        with pytest.raises(LifcalError) as e:
            ba.set_priors(camera=cam)
        assert e.value.code == -1 and "world_size" in str(e.value)
