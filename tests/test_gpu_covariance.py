"""lifcal_ba_covariance on the MI355X: parity with the dense reference algebra (tests/cov_reference.py) on the oracle's matrix, gauge
invariance, the statistics it claims, no side effects on the handle, the refusals, and the bench / configs[3] sizes."""
import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, LifcalError, _capi as capi, scene
from tests import cov_reference as cr
from tests.helpers import SMALL_CASES, S, problem

pytestmark = pytest.mark.gpu

CASES = dict(SMALL_CASES)
CASES["cfg2"] = scene.baseline_spec("cfg2")


def det_options(**kw):
    o = capi.default_options_py()
    o.deterministic = 1
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def at_oracle_solution(spec):
    sc = scene.make_scene(spec)
    pa = problem(sc)
    oracle.solve(pa, threads=oracle.hardware_threads())
    return sc, pa


def reference_for(sc, pa):
    o = capi.default_options_py()
    o.jacobi_scaling = 0
    sw = oracle.sweep(pa, radius=1e30, options=o, threads=oracle.hardware_threads())
    F = pa.struct.n_frames
    live = cr.live_mask(sc.config, sc.fixed_mask, F, sw.n_promoted, frame_used=np.bincount(sc.fr, minlength=F) > 0)
    full = bool(sc.config & 0x100) and bool(sc.config & 0x400)
    gauge = cr.first_observed_frame(sc.fr) if full else -1
    return cr.covariance(sw.S, live, F, gauge, null_rcond=1e-9, estimable_tol=1e-3), gauge


def block_scaled(A, B):
    d = np.sqrt(np.abs(np.diag(B))) + 1e-300
    return np.max(np.abs(A - B) / np.outer(d, d)) if A.size else 0.0


# parity bars, block-scaled: 5e-6 on the estimable camera block, 3e-5 on the pose blocks (measured on the MI355X: <= 9.6e-7 and
# <= 7.9e-6).
# The pose blocks carry Y C+ Y^T, and C+ carries the null direction of C, which two independently summed matrices (device, oracle)
# fix only to ~1e-7 (7h.5): the large non-estimable B / bL0 entries of C+ amplify that into the pose blocks
PARITY = ["r2_tan_full", "r2_tan_adj_robust", "r1_adj", "r0", "camera_only", "poses_only", "points_flag_without_poses", "constraints",
          "constraints_adj_robust", "windowed", "recalib", "cfg2"]


@pytest.mark.parametrize("name", PARITY)
def test_parity_with_the_reference_algebra(built, name):
    sc, pa = at_oracle_solution(CASES[name])
    ref, gauge = reference_for(sc, pa)
    with BundleAdjustment(problem_copy(pa), det_options()) as ba:
        cov = ba.covariance()
    assert cov.gauge_frame == gauge
    assert cov.null_rank == ref.null_rank
    assert np.array_equal(cov.estimable, ref.estimable), (cov.estimable, ref.estimable)
    e = np.flatnonzero(ref.estimable)
    err_cam = block_scaled(cov.camera[np.ix_(e, e)], ref.camera[np.ix_(e, e)])
    err_pose = max((block_scaled(cov.poses[f], ref.poses[f]) for f in range(pa.struct.n_frames) if np.any(ref.poses[f])), default=0.0)
    print(f"[{name}] null_rank {cov.null_rank} camera {err_cam:.2e} poses {err_pose:.2e}")
    assert err_cam < 5e-6 and err_pose < 3e-5
    for f in range(pa.struct.n_frames):
        if not np.any(ref.poses[f]):
            assert np.all(cov.poses[f] == 0)
    std = cov.camera_std
    assert np.all(np.isnan(std[cov.live & ~cov.estimable])) and np.all(std[~cov.live] == 0)
    assert np.all(np.isfinite(std[cov.estimable])) and np.all(std[cov.estimable] > 0)


def problem_copy(pa):
    s = pa.struct
    n = s.n_constraints
    return capi.ProblemArrays(pa.u, pa.v, pa.mcx, pa.mcy, pa.pt, pa.fr, pa.cam, pa.views, pa.pts, s.spx, s.scale, s.config,
                              spy=s.spy, fixed_mask=s.fixed_mask, lower=pa.lower, upper=pa.upper,
                              c_i=pa.c_i if n else None, c_j=pa.c_j if n else None, c_dist=pa.c_dist if n else None,
                              c_sigma=pa.c_sigma if n else None, use_constraints=s.use_constraints)


def test_gauge_invariance(built):
    sc, pa = at_oracle_solution(CASES["windowed"])
    F = pa.struct.n_frames
    with BundleAdjustment(problem_copy(pa), det_options()) as ba:
        a = ba.covariance(gauge_frame=0)
        b = ba.covariance(gauge_frame=F // 2)
    assert a.gauge_frame == 0 and b.gauge_frame == F // 2
    assert np.array_equal(a.estimable, b.estimable) and a.null_rank == b.null_rank
    e = np.flatnonzero(a.estimable)
    # bar as on the CPU (tests/test_covariance_cpu.py: the null direction of C is known to ~1e-7)
    assert block_scaled(a.camera[np.ix_(e, e)], b.camera[np.ix_(e, e)]) < 5e-6
    assert np.all(a.poses[0] == 0) and np.all(b.poses[F // 2] == 0)
    assert np.abs(a.poses[F // 2]).max() > 0 and np.abs(b.poses[0]).max() > 0
    assert block_scaled(a.poses[F - 1], b.poses[F - 1]) > 1e-3   # pose blocks are relative to their gauge frame


def test_statistics_of_repeated_noisy_solves(built):
    """independent of any oracle: 64 seeded N(0, 0.1^2) px noise draws around noiseless observations, each solved from the ground
    truth; the sample spread of every estimable camera slot must match 0.1 sqrt(G_jj), the mean Mahalanobis statistic its dimension"""
    spec = S(8, 60, None, 0x506, 131)   # squared loss, no outliers
    sc = scene.make_scene(spec)
    gt = problem(sc, initial=False)
    with BundleAdjustment(gt, det_options()) as ba:
        x, y = ba.projectObservations()
    clean = capi.ProblemArrays(x, y, sc.mcx, sc.mcy, sc.pt, sc.fr, sc.cam_gt, sc.views_gt, sc.pts_gt, sc.spx, sc.scale, sc.config)
    with BundleAdjustment(clean, det_options()) as ba:
        cov = ba.covariance(want_pose_blocks=False)
    e = np.flatnonzero(cov.estimable)
    assert len(e) >= 5
    rng = np.random.default_rng(2026)
    est = []
    for _ in range(64):
        pa = capi.ProblemArrays(x + rng.normal(0, 0.1, len(x)), y + rng.normal(0, 0.1, len(y)), sc.mcx, sc.mcy, sc.pt, sc.fr,
                                sc.cam_gt, sc.views_gt, sc.pts_gt, sc.spx, sc.scale, sc.config)
        with BundleAdjustment(pa, det_options()) as ba:
            ba.performBundleAdjustment()
        est.append(pa.cam.copy())
    est = np.array(est)
    ratio = est[:, e].std(axis=0, ddof=1) / (0.1 * np.sqrt(np.diag(cov.camera)[e]))
    Ginv = np.linalg.inv(0.01 * cov.camera[np.ix_(e, e)])
    dlt = est[:, e] - sc.cam_gt[e]
    maha = np.einsum("ni,ij,nj->n", dlt, Ginv, dlt)
    print(f"sample / predicted std {ratio}; mean Mahalanobis {maha.mean():.2f} over {len(e)} slots")
    assert np.all((ratio > 0.7) & (ratio < 1.3)), ratio
    assert abs(maha.mean() - len(e)) <= 0.25 * len(e)


def summary_tuple(s):
    return (s.initial_cost, s.final_cost, s.final_radius, s.final_gradient_max_norm, s.iterations, s.successful_steps,
            s.unsuccessful_steps, s.termination)


def test_no_side_effects(built):
    sc = scene.make_scene(CASES["windowed"])
    F = len(sc.views0) // 6
    fixed = np.zeros(F, np.uint8); fixed[3] = 1
    pa, pb = problem(sc), problem(sc)
    with BundleAdjustment(pa, det_options()) as a, BundleAdjustment(pb, det_options()) as b:
        a.set_fixed_frames(fixed); b.set_fixed_frames(fixed)
        c1 = a.covariance(gauge_frame=0, want_pose_band=True)
        c2 = a.covariance(gauge_frame=0, want_pose_band=True)
        for k in ("camera", "poses", "camera_null", "pose_band"):
            assert np.array_equal(getattr(c1, k), getattr(c2, k)), k
        assert (c1.null_rank, c1.sigma2, c1.gauge_frame) == (c2.null_rank, c2.sigma2, c2.gauge_frame)
        assert np.array_equal(c1.estimable, c2.estimable)
        assert np.array_equal(pa.cam, pb.cam) and np.array_equal(pa.views, pb.views)
        sa, sb = a.performBundleAdjustment(), b.performBundleAdjustment()
        assert summary_tuple(sa) == summary_tuple(sb)
        assert np.array_equal(pa.cam, pb.cam) and np.array_equal(pa.views, pb.views) and np.array_equal(pa.pts, pb.pts)
        ta, tb = a.calcReprojectionError(), b.calcReprojectionError()
        assert (ta.std_x, ta.std_y, ta.mae_x, ta.mae_y, ta.num_inliers) == (tb.std_x, tb.std_y, tb.mae_x, tb.mae_y, tb.num_inliers)
        assert np.array_equal(pa.views[18:24], problem(sc).views[18:24])   # the caller's constant pose survived both calls


def refused(ba):
    with pytest.raises(LifcalError) as ei:
        ba.covariance()
    msg = str(ei.value)
    assert "(-1)" in msg and "lifcal_ba_covariance" in msg
    return msg


def test_refusals(built, monkeypatch):
    sc = scene.make_scene(CASES["r2_tan_full"])
    with BundleAdjustment(problem(sc), det_options(precision=1)) as ba:
        assert "precision" in refused(ba)
        ba.performBundleAdjustment()
    # a rank of a two-rank job (it would solve with its peer and a collective; the refusal comes before any device work)
    with BundleAdjustment(problem(sc), det_options(world_size=2, rank=0, deterministic=0)) as ba:
        assert "world_size" in refused(ba)
    monkeypatch.setenv("LIFCAL_DISABLE_BANDW", "1")   # the band window does not fit: the global-memory factorisation only
    with BundleAdjustment(problem(sc), det_options()) as ba:
        assert "LDS" in refused(ba)
        s = ba.performBundleAdjustment()
        assert s.termination in (1, 2, 3)


def metric_web_scene():
    from lifcal_amd.mla import MicroLensGrid
    spec = scene.baseline_spec("metric_web")
    grid = MicroLensGrid(spec.raw_width, spec.raw_height, spec.lens_diameter, spec.lens_base_y, spec.grid_rotation, spec.grid_offset, True, device=0)

    def selector(img_x, img_y, img_vd, img_fr, img_pt, scale):
        o = grid.projectPointsToRawImage(img_x, img_y, img_vd, int(scale), fr=img_fr, pt=img_pt)
        return o.src, o.mcx, o.mcy
    sc = scene.make_scene(spec, lens_selector=selector)
    grid.close()
    return sc


def test_size_metric_web_against_its_own_matrix(built):
    sc = metric_web_scene()
    pa = problem(sc)
    with BundleAdjustment(pa) as ba:
        ba.performBundleAdjustment()
        cov = ba.covariance()
        sw = ba.sweep(float("inf"), want_matrices=True)
    F = pa.struct.n_frames
    live = cr.live_mask(sc.config, sc.fixed_mask, F, sw.n_promoted, frame_used=np.bincount(sc.fr, minlength=F) > 0)
    ref = cr.covariance(sw.S, live, F, cr.first_observed_frame(sc.fr), null_rcond=1e-9, estimable_tol=1e-3)
    e = np.flatnonzero(ref.estimable)
    err = block_scaled(cov.camera[np.ix_(e, e)], ref.camera[np.ix_(e, e)])
    print(f"[metric_web] null_rank {cov.null_rank} camera {err:.2e} device {cov.seconds * 1e3:.3f} ms")
    assert cov.null_rank == ref.null_rank == 1
    assert np.array_equal(cov.estimable, ref.estimable)
    assert err < 5e-6   # measured 1.04e-6: the floor of DESIGN.md 7h.5


def test_size_configs3(built):
    sc = scene.make_scene(scene.baseline_spec("cfg4"))   # BASELINE configs[3]: 1000 frames, 50k points
    with BundleAdjustment(problem(sc)) as ba:
        ba.performBundleAdjustment()
        cov = ba.covariance()
    print(f"[configs3] null_rank {cov.null_rank} device {cov.seconds * 1e3:.3f} ms estimable {cov.estimable.astype(int)}")
    assert cov.null_rank == 1 and cov.gauge_frame == 0
    assert np.all(np.isfinite(cov.poses)) and np.all(np.isfinite(cov.camera))
