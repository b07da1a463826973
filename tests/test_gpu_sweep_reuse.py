"""Tables are state of a parameter set and the reduced block has two copies (lifcal_amd/csrc/sweep_state.hpp): a sweep builds its
tables only where the parameters changed, and accumulates into the copy of the block that the previous sweep's k_finalize
zero-filled.  What a handle carries from call to call must never show in a result: the comparator is always a FRESH handle made
at the same parameters, whose first sweep builds everything from scratch, and with options.deterministic = 1 "equal" is bitwise."""
import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, _capi as capi, scene
from tests.helpers import S, bounded_problem, problem

pytestmark = pytest.mark.gpu

FIELDS = ("S", "rhs", "gradient_reduced", "point_gradient", "point_hessian_inv")

# regular points in LDS-window blocks | regular blocks AND special points (constraints: the global-atomic kernels, k_zero_special)
SCENES = [("windowed", S(24, 120, 6, 0xF06, 7301, outlier_fraction=0.02)),
          ("windowed_constraints", S(24, 300, 6, 0xF06, 7302, n_constraints=12, outlier_fraction=0.03))]


def opts(precision=0):
    o = capi.default_options_py(); o.deterministic = 1; o.precision = precision
    return o


def take(g):
    return (g.cost, g.gradient_max_norm) + tuple(getattr(g, k).copy() for k in FIELDS)


def same(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))


def fresh_sweep(pa, radius, precision=0, fixed=None):
    with BundleAdjustment(pa, opts(precision)) as ba:
        if fixed is not None:
            ba.set_fixed_frames(fixed)
        return take(ba.sweep(radius, want_matrices=True))


def moved(sc, seed):
    """another parameter set for the same observations"""
    pa = problem(sc)
    rng = np.random.default_rng(seed)
    pa.cam[:9] *= 1.0 + 1e-4 * rng.standard_normal(9)
    pa.views += 1e-4 * rng.standard_normal(pa.views.shape)
    pa.pts += 1e-4 * rng.standard_normal(pa.pts.shape)
    return pa


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name,spec", SCENES, ids=[c[0] for c in SCENES])
def test_upload_between_sweeps_rebuilds_the_tables(built, name, spec, precision):
    """(a) the stale-tables trap"""
    sc = scene.make_scene(spec)
    pa = problem(sc)
    other = moved(sc, 1)
    with BundleAdjustment(pa, opts(precision)) as ba:
        first = take(ba.sweep(1e3, want_matrices=True))
        pa.cam[:] = other.cam; pa.views[:] = other.views; pa.pts[:] = other.pts
        ba.upload_parameters()
        second = take(ba.sweep(1e3, want_matrices=True))
    assert not same(first, second)
    assert same(first, fresh_sweep(problem(sc), 1e3, precision))
    assert same(second, fresh_sweep(moved(sc, 1), 1e3, precision))


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name,spec", SCENES, ids=[c[0] for c in SCENES])
def test_stats_and_projection_between_sweeps(built, name, spec, precision):
    """(b) calcReprojectionError and projectObservations borrow the candidate table arrays (unfolded tables)"""
    sc = scene.make_scene(spec)
    with BundleAdjustment(problem(sc), opts(precision)) as ba:
        first = take(ba.sweep(1e3, want_matrices=True))
        st0 = ba.calcReprojectionError()
        x0, y0 = ba.projectObservations()
        second = take(ba.sweep(1e3, want_matrices=True))
        st1 = ba.calcReprojectionError()
        x1, y1 = ba.projectObservations()
    assert same(first, second)
    assert same(first, fresh_sweep(problem(sc), 1e3, precision))
    assert (st0.std_x, st0.std_y, st0.mae_x, st0.mae_y, st0.num_inliers) == (st1.std_x, st1.std_y, st1.mae_x, st1.mae_y, st1.num_inliers)
    assert np.array_equal(x0, x1, equal_nan=True) and np.array_equal(y0, y1, equal_nan=True)


@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("name,spec", SCENES, ids=[c[0] for c in SCENES])
def test_consecutive_sweeps_at_alternating_radii(built, name, spec, precision):
    """(c) both copies of the block, and the zero-fill done by k_finalize (the damping enters the block: a copy that was not zero
    would carry the other radius' system into this one)"""
    sc = scene.make_scene(spec)
    radii = (1e3, 7.0, 1e3, 7.0, 1e3)
    with BundleAdjustment(problem(sc), opts(precision)) as ba:
        got = [take(ba.sweep(r, want_matrices=True)) for r in radii]
        ba.sweep_enqueue(7.0); ba.sweep_enqueue(1e3); ba.sweep_enqueue(7.0)   # ... and without a host round trip in between
        got.append(take(ba.sweep(1e3, want_matrices=True)))
    want = {r: fresh_sweep(problem(sc), r, precision) for r in set(radii)}
    assert not same(want[1e3], want[7.0])
    for r, g in zip(radii + (1e3,), got):
        assert same(g, want[r]), r


@pytest.mark.parametrize("precision", [0, 1])
def test_fixed_frames_between_sweeps(built, precision):
    """(d) the frame mask enters no table, but it starts a new solve: the diagonal-only pass runs again, on the copy k_finalize cleaned"""
    name, spec = SCENES[0]
    sc = scene.make_scene(spec)
    mask = np.zeros(spec.n_frames, np.uint8); mask[[0, 3, 4, 11]] = 1
    with BundleAdjustment(problem(sc), opts(precision)) as ba:
        free = take(ba.sweep(1e3, want_matrices=True))
        ba.set_fixed_frames(mask)
        held = take(ba.sweep(1e3, want_matrices=True))
        ba.set_fixed_frames(None)
        free_again = take(ba.sweep(1e3, want_matrices=True))
    assert not same(free, held)
    assert same(held, fresh_sweep(problem(sc), 1e3, precision, fixed=mask))
    assert same(free, fresh_sweep(problem(sc), 1e3, precision)) and same(free, free_again)


def summary_key(s):
    return (s.iterations, s.successful_steps, s.unsuccessful_steps, s.termination, s.initial_cost, s.final_cost, s.final_radius, s.final_gradient_max_norm)


ROUTES = {
    # camera only: sixteen iterations, seven accepted, eight rejected steps (tests/test_gpu_paths.py pins the counts on both routes)
    "device_loop": (lambda: scene.make_scene(S(6, 40, None, 0x006, 113)), problem, None),
    "host_loop": (lambda: scene.make_scene(S(6, 40, None, 0x006, 113)), problem, "1"),
    # the recalibration pattern with a tight box: the line search backtracks (tests/test_gpu_deterministic.py)
    "bounded_backtracking": (lambda: scene.make_scene(S(8, 60, None, 0xF06, 3112, recalib=True, outlier_fraction=0.02)), bounded_problem, None),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_solve_on_a_used_handle_equals_the_solve_of_a_fresh_one(built, monkeypatch, route):
    """(e) the whole trajectory — final parameters, iteration count, accepted and rejected steps, final radius (every accept and
    every reject moves it by its own rule, so an equal radius after equal counts is the equal sequence) — of
      * a handle that carries everything a handle can carry into a solve: sweeps at another point and another radius, stats and
        projection calls, a whole earlier solve, then the start parameters uploaded again;
      * a fresh handle whose parameters are uploaded once more in front of the solve, so that nothing it built is taken over.
    The scenes take rejected AND accepted steps on their route; the oracle (CPU) says so, and the counts are its counts."""
    make, mk, host_lm = ROUTES[route]
    if host_lm:
        monkeypatch.setenv("LIFCAL_HOST_LM", host_lm)
    else:
        monkeypatch.delenv("LIFCAL_HOST_LM", raising=False)
    sc = make()
    so = oracle.solve(mk(sc), threads=4)
    assert so.successful_steps >= 1 and so.unsuccessful_steps >= 1

    pf = mk(sc)
    with BundleAdjustment(pf, opts()) as ba:
        ba.upload_parameters()
        sf = ba.performBundleAdjustment()
        stf = ba.calcReprojectionError()

    pu = mk(sc)
    start = (pu.cam.copy(), pu.views.copy(), pu.pts.copy())
    with BundleAdjustment(pu, opts()) as ba:
        ba.sweep(3.0); ba.calcReprojectionError(); ba.projectObservations(); ba.sweep(1e5)
        s1 = ba.performBundleAdjustment()
        first = (pu.cam.copy(), pu.views.copy(), pu.pts.copy())
        ba.sweep(11.0); ba.calcReprojectionError()
        pu.cam[:] = start[0]; pu.views[:] = start[1]; pu.pts[:] = start[2]
        ba.upload_parameters()
        ba.sweep(2.0)
        s2 = ba.performBundleAdjustment()
        stu = ba.calcReprojectionError()

    print(route, "fresh", summary_key(sf), "used", summary_key(s1), summary_key(s2), "oracle", so.iterations, so.successful_steps, so.unsuccessful_steps)
    assert (sf.iterations, sf.successful_steps, sf.unsuccessful_steps, sf.termination) == (so.iterations, so.successful_steps, so.unsuccessful_steps, so.termination)
    assert summary_key(s1) == summary_key(sf) and summary_key(s2) == summary_key(sf)
    for a, b in zip(first, (pf.cam, pf.views, pf.pts)):
        assert np.array_equal(a, b)
    assert np.array_equal(pu.cam, pf.cam) and np.array_equal(pu.views, pf.views) and np.array_equal(pu.pts, pf.pts)
    assert (stu.std_x, stu.std_y, stu.mae_x, stu.mae_y) == (stf.std_x, stf.std_y, stf.mae_x, stf.mae_y)


def test_precision_1_solve_on_a_used_handle(built):
    """(f) options.precision = 1 takes the host loop, and an accepted step rebuilds the current tables (the fp32 lens table has no
    candidate twin): same comparison, against that mode's own fresh handle"""
    sc = scene.make_scene(scene.baseline_spec("cfg2"))
    pf = problem(sc)
    with BundleAdjustment(pf, opts(1)) as ba:
        sf = ba.performBundleAdjustment()
    pu = problem(sc)
    start = (pu.cam.copy(), pu.views.copy(), pu.pts.copy())
    with BundleAdjustment(pu, opts(1)) as ba:
        ba.sweep(3.0); ba.calcReprojectionError()
        s1 = ba.performBundleAdjustment()
        pu.cam[:] = start[0]; pu.views[:] = start[1]; pu.pts[:] = start[2]
        ba.upload_parameters()
        s2 = ba.performBundleAdjustment()
    assert sf.successful_steps >= 1
    assert summary_key(s1) == summary_key(sf) and summary_key(s2) == summary_key(sf)
    assert np.array_equal(pu.cam, pf.cam) and np.array_equal(pu.views, pf.views) and np.array_equal(pu.pts, pf.pts)
