"""One Levenberg-Marquardt step of every route of the reduced solver, read back (BundleAdjustment.debug_step) and measured against
the damped normal equations (tests/step_reference.py), not through a whole solve: LM corrects its own mistakes, so a step wrong by
1e-6 relative in one pose block, one arrow row or one point passes every trajectory test, while it stands four orders of magnitude
above the bounds here (tests/test_step_reference_cpu.py shows the measure moving).

Per case: create, sweep(radius, want_matrices), debug_step, at the radii 1e4 (the solve's first) and 7, on one handle.
  (a) the route the case names is the route that ran
  (b) the solver alone: row-wise backward error of delta_B on the GPU's own (S, rhs) against numpy.linalg.solve on the same system
  (c) the whole step: eta_B / eta_P of (delta_B, delta_P) on the matrix-free normal equations against the CPU reference step
  (d) gtd, ddd, step2, x2 against the same sums in long double from the returned delta, gradients and LM diagonal
  (e) on the cases away from the default scalars and options: the returned LM diagonal against clip(h s^2, min, max) / (radius s^2)
      of the reference, entry by entry, so that a clamp that binds is tested by its formula and not through the step
The margin of 32 over the reference in (b) and (c) is reasoned, not measured: the reference and the kernels eliminate in different
orders (LAPACK's pivoted LU; the chain, the two-ended chain, the odd-even reduction), the row-wise backward error is not bounded
by Cholesky's analysis and scatters between two correct solvers (LU and Cholesky on the oracle's systems differ by up to 8x).
"""
import dataclasses
from typing import Callable, Optional

import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, LifcalError, _capi as capi, scene
from lifcal_amd.bundle_adjustment import plan_stats
from tests import off_defaults as od, step_reference as sr
from tests.helpers import S, anisotropic, problem

pytestmark = pytest.mark.gpu

MARGIN = 32.0
RADII = (1e4, 7.0)
LD = np.longdouble
GLOBAL_CHAIN, LDS_CHAIN, TWISTED, ODD_EVEN = 0, 1, 2, 3
ROUTE_ENV = ("LIFCAL_CR", "LIFCAL_TWISTED", "LIFCAL_DISABLE_BANDW")
SWEEP_ENV = ("LIFCAL_SWEEP_KERNEL", "LIFCAL_DISABLE_V2", "LIFCAL_SWEEP_WAVES")


@dataclasses.dataclass
class Case:
    id: str
    spec: scene.SceneSpec
    route: int
    env: dict = dataclasses.field(default_factory=dict)
    options: dict = dataclasses.field(default_factory=dict)
    fixed_frames: Optional[tuple] = None
    whole_step: bool = True        # (c); off where the Jacobian is evaluated in fp32
    panel_in_lds: bool = True
    radii: tuple = RADII
    transform: Optional[Callable] = None   # scene -> ProblemArrays in place of helpers.problem
    lambdas: Optional[float] = None   # (e): its bar


W24 = dict(outlier_fraction=0.02)
CASES = [
    # the chain in LDS
    Case("lds_six_frames", S(6, 40, None, 0x506, 101), LDS_CHAIN),
    Case("lds_poses_only", S(6, 40, None, 0x306, 115), LDS_CHAIN),
    Case("lds_camera_only", S(6, 40, None, 0x006, 113), LDS_CHAIN),
    Case("lds_recalib", S(8, 60, None, 0xF06, 120, recalib=True), LDS_CHAIN),
    Case("lds_constraints", S(6, 40, None, 0xF06, 118, n_constraints=4, outlier_fraction=0.03), LDS_CHAIN),
    Case("lds_window6", S(24, 120, 6, 0xF06, 119, **W24), LDS_CHAIN, env={"LIFCAL_TWISTED": "0"}),
    Case("lds_window6_frames_0_7_constant", S(24, 120, 6, 0xF06, 119, **W24), LDS_CHAIN, env={"LIFCAL_TWISTED": "0"}, fixed_frames=(0, 7)),
    Case("lds_no_jacobi_scaling", S(6, 40, None, 0x506, 101), LDS_CHAIN, options={"jacobi_scaling": 0}),
    Case("lds_deterministic", S(6, 40, None, 0x506, 101), LDS_CHAIN, options={"deterministic": 1}),
    Case("lds_precision1", S(6, 40, None, 0x506, 101), LDS_CHAIN, options={"precision": 1}, whole_step=False),
    # the chain from both ends
    Case("twisted_f23_smallest", S(23, 100, 6, 0xF06, 6104), TWISTED),
    Case("twisted_f24_other_parity", S(24, 120, 6, 0xF06, 6101, **W24), TWISTED),
    Case("twisted_bw1", S(31, 200, 2, 0x506, 6105), TWISTED),   # (31 frames: from 32 super-blocks on create() takes the odd-even reduction by itself)
    Case("twisted_w10_recalib", S(41, 300, 10, 0xF06, 6103, recalib=True, **W24), TWISTED),
    # block odd-even reduction
    Case("cr_window2_m6_padded", S(40, 200, 2, 0x506, 6105), ODD_EVEN, env={"LIFCAL_CR": "1"}),
    Case("cr_window4_f97", S(97, 500, 4, 0xF06, 6204), ODD_EVEN, env={"LIFCAL_CR": "1"}),
    Case("cr_window11_nq15", S(60, 300, 11, 0xF06, 6208), ODD_EVEN, env={"LIFCAL_CR": "1"}),
    Case("cr_23_arrow_rows", S(40, 220, 4, 0xF06, 6206, n_constraints=2, **W24), ODD_EVEN, env={"LIFCAL_CR": "1"}),
    Case("cr_29_arrow_rows", S(36, 200, 3, 0x506, 6207, n_constraints=4), ODD_EVEN, env={"LIFCAL_CR": "1"}),
    # the chain in global memory, panel in LDS
    Case("global_window6_forced", S(24, 120, 6, 0xF06, 119, **W24), GLOBAL_CHAIN, env={"LIFCAL_DISABLE_BANDW": "1"}),
    Case("global_six_frames_forced", S(6, 40, None, 0x506, 101), GLOBAL_CHAIN, env={"LIFCAL_DISABLE_BANDW": "1"}),
    Case("global_natural_40_constraints", S(24, 120, 6, 0xF06, 6209, n_constraints=40), GLOBAL_CHAIN),
]
# the panel of the global chain in global memory too: (80 + 6 (6 bw + NA + 1)) doubles do not fit 64 KiB of LDS from 1353 panel rows on;
# six frames: bw = 5, NA = 3 Q + 9, so Q >= 438 promoted points, which 652 constraints among 800 points give (650: Q = 436, 1348 rows)
GLOBAL_PANEL = Case("global_panel_in_global_memory", S(6, 800, None, 0x506, 6210, n_constraints=652), GLOBAL_CHAIN, panel_in_lds=False, radii=(1e4,))


# ---- away from the default scalars and options (tests/off_defaults.py; tests/test_off_defaults_cpu.py holds the conditions) --------------
# spy = 1.25 spx, scale 1 and 3, other loss scales, LM-diagonal clamps that bind; all of them with (e), at 1e-12 where the Jacobian is fp64
ANISO = lambda sc: anisotropic(sc, od.A)
E = dict(lambdas=1e-12)
ADJ_ROBUST_CONSTRAINTS = S(6, 40, None, 0xF06, 118, n_constraints=4, outlier_fraction=0.03)
CLAMP_CASES = [Case(name, od.BASE, LDS_CHAIN, options=kw, **E) for name, (kw, _) in od.CLAMPS.items()]
ANISO_125 = Case("aniso_125", od.BASE, LDS_CHAIN, transform=ANISO, **E)
OFF_DEFAULT_CASES = [
    ANISO_125,
    Case("aniso_125_adj_robust_constraints", ADJ_ROBUST_CONSTRAINTS, LDS_CHAIN, transform=ANISO, **E),
    # (e) of the fp32 evaluator: h is a sum of squares of Jacobian entries rounded to float32, not a sum that agrees to 1e-10 with the
    # reference's.  An entry carries a few roundings of 2^-24 = 6e-8, its square twice that, and the sum of squares no more than its
    # worst term: 16 roundings, 1e-6, is the bar (measured on an MI355X: 1.1e-7 on the reduced rows, 1.8e-7 on the points, three
    # roundings; the fp64 arms measure 3e-16 .. 2e-14)
    Case("aniso_125_precision1", od.BASE, LDS_CHAIN, options={"precision": 1}, whole_step=False, transform=ANISO, lambdas=16 * 2.0 ** -24),
    Case("aniso_125_deterministic", od.BASE, LDS_CHAIN, options={"deterministic": 1}, transform=ANISO, **E),
    Case("scale_1", od.SCALE_1, LDS_CHAIN, **E),
    Case("scale_3", od.SCALE_3, LDS_CHAIN, **E),
    Case("scale_3_aniso_125", od.SCALE_3, LDS_CHAIN, transform=ANISO, **E),
] + [Case(name, od.ROBUST, LDS_CHAIN, options={"loss_scale": ls}, **E) for name, ls in od.LOSS_SCALES.items()] + CLAMP_CASES
# the clamp cases and aniso_125 once more per damping site of the full sweep: k_sweep2, the global-atomic kernels
# with k_schur, and k_sweep3 with two waves per role (all fp64 and unordered: no pairing here that create() refuses or redirects)
SWEEP_SETTINGS = [{"LIFCAL_SWEEP_KERNEL": "2"}, {"LIFCAL_DISABLE_V2": "1"}, {"LIFCAL_SWEEP_WAVES": "2"}]
# lanes per pass of the plan create() makes in each of them (lifcal_ba_plan_stats: 128 is k_sweep3 with two waves per role, 256 k_sweep3
# and k_sweep2), so that a fallback to k_sweep3 cannot take a case's damping site away unnoticed
PASS_LANES = {"LIFCAL_SWEEP_KERNEL": {"2": 256}, "LIFCAL_SWEEP_WAVES": {"2": 128}}
OFF_DEFAULT_CASES += [dataclasses.replace(c, id=c.id + "_" + "_".join(f"{k[7:].lower()}_{v}" for k, v in env.items()), env=env)
                      for env in SWEEP_SETTINGS for c in CLAMP_CASES + [ANISO_125]]


def make_options(case):
    o = capi.default_options_py()
    for k, v in case.options.items():
        setattr(o, k, v)
    return o


def set_route_env(monkeypatch, env):
    for k in ROUTE_ENV + SWEEP_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def long_sum(terms):
    """(sum, sum of |terms|, count) in long double"""
    t = np.asarray(terms, LD).reshape(-1)
    return float(np.sum(t)), float(np.sum(np.abs(t))), t.size


def step_scalars_reference(pa, ne, sw, st, frame_live):
    """gtd, ddd, step2, x2 as k_update_reduced and k_backsub count them, from the returned step, the sweep's gradients, the returned
    LM diagonal and the stored parameters: each as (sum, sum of |terms|, number of terms)"""
    F, P, nb = ne.F, ne.P, ne.nb
    dB, dP = st.delta_reduced, st.delta_points.reshape(P, 3)
    elim = np.zeros(P, bool)
    if ne.refine_points:
        elim = ne.observed_points.copy(); elim[ne.promoted] = False
    prom = np.zeros(P, bool); prom[ne.promoted] = True
    gP, lP = sw.point_gradient.reshape(P, 3), st.lambda_points.reshape(P, 3)
    gtd = long_sum(np.concatenate([np.asarray(sw.gradient_reduced, LD) * dB, (np.asarray(gP[elim], LD) * dP[elim]).reshape(-1)]))
    ddd = long_sum(np.concatenate([np.asarray(st.lambda_reduced, LD) * dB * dB, (np.asarray(lP[elim], LD) * dP[elim] * dP[elim]).reshape(-1)]))
    # camera: all 17 slots, the step after the box projection; poses: live frames; points: eliminated and promoted ones
    cam_new = pa.cam + dB[:17]
    if pa.lower is not None:
        cam_new = np.maximum(cam_new, pa.lower)
    if pa.upper is not None:
        cam_new = np.minimum(cam_new, pa.upper)
    views = pa.views.reshape(F, 6); dV = dB[17:nb].reshape(F, 6)
    live_f = frame_live if ne.refine_poses else np.zeros(F, bool)
    pts = pa.pts.reshape(P, 3)
    moved = elim | prom
    step2 = long_sum(np.concatenate([np.asarray(cam_new - pa.cam, LD) ** 2, np.asarray((views + dV) - views, LD)[live_f].reshape(-1) ** 2, np.asarray(dP[moved], LD).reshape(-1) ** 2]))
    x2 = long_sum(np.concatenate([np.asarray(pa.cam, LD) ** 2, np.asarray(views[live_f], LD).reshape(-1) ** 2, np.asarray(pts[moved], LD).reshape(-1) ** 2]))
    return dict(gtd=gtd, ddd=ddd, step2=step2, x2=x2)


def candidate_cost(pa, ne, st, loss_scale=0.5):
    """the oracle's cost at x + delta (camera through the box projection, as the kernels apply it)"""
    sc_pa = capi.ProblemArrays(pa.u, pa.v, pa.mcx, pa.mcy, pa.pt, pa.fr, pa.cam, pa.views, pa.pts, pa.struct.spx, pa.struct.scale, pa.struct.config,
                               spy=pa.struct.spy, fixed_mask=pa.struct.fixed_mask, lower=pa.lower, upper=pa.upper, c_i=pa.c_i, c_j=pa.c_j,
                               c_dist=pa.c_dist, c_sigma=pa.c_sigma, use_constraints=pa.struct.use_constraints)
    cam = pa.cam + st.delta_reduced[:17]
    if pa.lower is not None:
        cam = np.maximum(cam, pa.lower)
    if pa.upper is not None:
        cam = np.minimum(cam, pa.upper)
    sc_pa.cam[:] = cam
    sc_pa.views[:] = pa.views + st.delta_reduced[17:ne.nb]
    sc_pa.pts[:] = pa.pts + st.delta_points
    return oracle.cost(sc_pa, loss_scale=loss_scale, threads=4)


def check_case(case, monkeypatch):
    set_route_env(monkeypatch, case.env)
    sc = scene.make_scene(case.spec)
    pa = problem(sc) if case.transform is None else case.transform(sc)
    o = make_options(case)
    F = case.spec.n_frames
    fixed = None
    if case.fixed_frames is not None:
        fixed = np.zeros(F, np.uint8); fixed[list(case.fixed_frames)] = 1
    ne = sr.NormalEquations(pa, RADII[0], jacobi_scaling=bool(o.jacobi_scaling), fixed_frames=fixed, loss_scale=o.loss_scale,
                            lm_min=o.min_lm_diagonal, lm_max=o.max_lm_diagonal)
    n_dead = ne.check_dead_rows()
    frame_live = np.zeros(F, bool); frame_live[np.unique(pa.fr)] = True
    if fixed is not None:
        frame_live &= fixed == 0
    failures = []

    def expect(ok, what):
        if not ok:
            failures.append(what)

    with BundleAdjustment(pa, o) as ba:
        if fixed is not None:
            ba.set_fixed_frames(fixed)
        info = ba.info()
        for k, v in case.env.items():
            if k == "LIFCAL_DISABLE_V2":
                assert info.n_chunks == 0 and info.n_tiles > 0, (info.n_chunks, info.n_tiles)   # every point through the global-atomic kernels
            elif k in PASS_LANES:
                st = plan_stats(pa)
                assert info.n_chunks == st.n_blocks > 0 and st.pass_lanes == PASS_LANES[k][v], (info.n_chunks, st.n_blocks, st.pass_lanes)
                assert info.n_tiles == st.n_passes * (st.pass_lanes // 64), (info.n_tiles, st.n_passes)   # no point left to the other kernels
        for radius in case.radii:
            tag = f"[{case.id} r={radius:g}]"
            sw = ba.sweep(radius, want_matrices=True)
            st = ba.debug_step()
            n_red = sw.n_reduced
            # (a) the route
            print(f"{tag} route {st.route} panel_in_lds {int(st.panel_in_lds)} n_reduced {n_red} n_full {ne.n} dead rows {n_dead} promoted {sw.n_promoted}"
                  f" | sweep {case.env or 'k_sweep3 (default)'}: {info.n_chunks} window blocks, {info.n_tiles} tiles")
            assert st.route == case.route and st.panel_in_lds == case.panel_in_lds, (st.route, st.panel_in_lds)
            assert sw.n_promoted == len(ne.promoted) and n_red == ne.nb + 3 * len(ne.promoted)
            # (b) the solver alone, on its own system
            eta_gpu = sr.solve_eta(sw.S, sw.rhs, st.delta_reduced)
            eta_lapack = sr.solve_eta(sw.S, sw.rhs, np.linalg.solve(sw.S, sw.rhs))
            bound = MARGIN * max(eta_lapack, n_red * sr.EPS)
            print(f"{tag} (b) eta solver {eta_gpu:.3e}  lapack {eta_lapack:.3e}  bound {bound:.3e}")
            expect(eta_gpu <= bound, f"{tag} (b) eta {eta_gpu:.3e} > {bound:.3e}")
            dead_red = ~ne.live[:ne.nb]
            expect(np.all(st.delta_reduced[:ne.nb][dead_red] == 0.0), f"{tag} (b) a dead, fixed or constant slot moved")
            expect(np.all(st.lambda_reduced[:ne.nb][dead_red] == 0.0), f"{tag} (b) a dead slot is damped")
            dead_pts = ~ne.live[ne.nb:]
            expect(np.all(st.delta_points[dead_pts] == 0.0), f"{tag} (b) a point that is not refined or not observed moved")
            expect(st.chol_fail == 0.0, f"{tag} (b) chol_fail {st.chol_fail}")
            # (c) the whole step on the normal equations
            if case.whole_step:
                ne.set_radius(radius)
                osw = sr.oracle_sweep(pa, radius, options=o, fixed_frames=fixed)
                eB_ref, eP_ref = ne.eta(sr.reference_step(ne, osw))
                eB, eP = ne.eta(ne.split(st.delta_reduced, st.delta_points))
                bB, bP = MARGIN * max(eB_ref, ne.n * sr.EPS), MARGIN * max(eP_ref, ne.n * sr.EPS)
                print(f"{tag} (c) eta_B {eB:.3e}  reference {eB_ref:.3e}  bound {bB:.3e} | eta_P {eP:.3e}  reference {eP_ref:.3e}  bound {bP:.3e}")
                expect(eB <= bB, f"{tag} (c) eta_B {eB:.3e} > {bB:.3e}")
                expect(eP <= bP, f"{tag} (c) eta_P {eP:.3e} > {bP:.3e}")
            # (d) the scalars of the step-quality test
            for name, (val, mag, cnt) in step_scalars_reference(pa, ne, sw, st, frame_live).items():
                got = getattr(st, name)
                tol = 8 * cnt * sr.EPS * mag
                print(f"{tag} (d) {name} {got:.17g}  long double {val:.17g}  |diff| {abs(got - val):.3e}  tolerance {tol:.3e}")
                expect(abs(got - val) <= tol, f"{tag} (d) {name}: {got!r} against {val!r}, tolerance {tol:.3e}")
            # (e) the LM diagonal itself: clip(h s^2, min, max) / (radius s^2) of the reference on every live row.  Both sides are one
            # fp64 multiply, clip and divide of sums h that agree to 1e-10 (the sweep's bar), so 1e-12 is two orders above them
            if case.lambdas is not None:
                ne.set_radius(radius)
                lam = ne.lam.astype(np.float64)
                lam_B, live_B = ne.reduced(lam), ne.reduced(ne.live)
                elim_rows = (ne.rows_P & ne.live)[ne.nb:]
                below, above = od.clip_counts(ne, o.min_lm_diagonal, o.max_lm_diagonal)
                eB = float(np.max(np.abs(st.lambda_reduced[live_B] - lam_B[live_B]) / lam_B[live_B]))
                eP = float(np.max(np.abs(st.lambda_points[elim_rows] - lam[ne.nb:][elim_rows]) / lam[ne.nb:][elim_rows])) if np.any(elim_rows) else 0.0
                print(f"{tag} (e) lambda: reduced {eB:.3e}  points {eP:.3e}  ({case.lambdas:g}); clipped from below {below}, from above {above} of {int(np.sum(ne.live))}")
                expect(eB <= case.lambdas, f"{tag} (e) lambda_reduced off by {eB:.3e}")
                expect(eP <= case.lambdas, f"{tag} (e) lambda_points off by {eP:.3e}")
            # the candidate's cost belongs to x + delta: two fp64 evaluations of the model summed in different orders (the suite holds
            # the sweep's cost to 1e-12 of the oracle's at these sizes; the candidate point is rebuilt here from delta in the same fp64 adds)
            cc = candidate_cost(pa, ne, st, o.loss_scale)
            print(f"{tag} cand_cost {st.cand_cost:.17g}  oracle at x + delta {cc:.17g}  relative {abs(st.cand_cost - cc) / cc:.3e}")
            expect(abs(st.cand_cost - cc) <= 1e-10 * cc, f"{tag} cand_cost {st.cand_cost!r} against {cc!r}")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_step_solves_the_normal_equations(built, monkeypatch, case):
    check_case(case, monkeypatch)


@pytest.mark.parametrize("case", OFF_DEFAULT_CASES, ids=[c.id for c in OFF_DEFAULT_CASES])
def test_step_away_from_the_default_scalars_and_options(built, monkeypatch, case):
    check_case(case, monkeypatch)


def test_step_of_the_global_chain_with_its_panel_in_global_memory(built, monkeypatch):
    """438 promoted points in a six-frame scene: the 1354 rows of the panel do not fit the LDS of k_band_chol (Dev::panel_g)"""
    check_case(GLOBAL_PANEL, monkeypatch)


# ---- the handle around a debug_step ---------------------------------------------------------------------------------------------------
def _deterministic():
    o = capi.default_options_py(); o.deterministic = 1
    return o


def test_sweep_after_a_step_repeats_the_sweep_bitwise(built, monkeypatch):
    set_route_env(monkeypatch, {})
    sc = scene.make_scene(S(24, 120, 6, 0xF06, 119, **W24))
    with BundleAdjustment(problem(sc), _deterministic()) as ba:
        a = ba.sweep(1e4, want_matrices=True)
        ba.debug_step()
        b = ba.sweep(1e4, want_matrices=True)
    assert a.cost == b.cost and a.gradient_max_norm == b.gradient_max_norm
    for name in ("S", "rhs", "gradient_reduced", "point_gradient", "point_hessian_inv"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_solve_after_a_step_equals_the_solve_of_a_fresh_handle(built, monkeypatch):
    set_route_env(monkeypatch, {})
    sc = scene.make_scene(S(24, 120, 6, 0xF06, 119, **W24))
    pa, pb = problem(sc), problem(sc)
    with BundleAdjustment(pa, _deterministic()) as ba:
        ba.sweep(1e4)
        ba.debug_step()
        s1 = ba.performBundleAdjustment()
    with BundleAdjustment(pb, _deterministic()) as ba:
        s0 = ba.performBundleAdjustment()
    assert (s1.iterations, s1.successful_steps, s1.unsuccessful_steps, s1.termination) == (s0.iterations, s0.successful_steps, s0.unsuccessful_steps, s0.termination)
    assert s1.final_cost == s0.final_cost and s1.initial_cost == s0.initial_cost
    assert np.array_equal(pa.cam, pb.cam) and np.array_equal(pa.views, pb.views) and np.array_equal(pa.pts, pb.pts)


def test_step_without_a_sweep_in_front_is_refused(built, monkeypatch):
    set_route_env(monkeypatch, {})
    sc = scene.make_scene(S(6, 40, None, 0x506, 101))
    invalid = -1   # LIFCAL_BA_ERR_INVALID_ARG

    def refused(ba):
        with pytest.raises(LifcalError) as e:
            ba.debug_step()
        return e.value.code == invalid

    with BundleAdjustment(problem(sc)) as ba:
        assert refused(ba)                      # fresh handle
        ba.sweep(1e4)
        ba.debug_step()
        assert refused(ba)                      # the block was consumed by the step before
        ba.sweep(1e4)
        ba.upload_parameters()
        assert refused(ba)                      # the parameters the block belongs to were replaced
        ba.performBundleAdjustment()
        assert refused(ba)                      # after a solve
        ba.sweep(1e4)
        assert ba.debug_step().chol_fail == 0.0  # and a sweep makes it valid again
    o = capi.default_options_py(); o.world_size = 2; o.rank = 0
    with BundleAdjustment(problem(sc), o) as ba:
        assert refused(ba)                      # more than one rank
