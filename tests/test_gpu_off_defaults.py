"""The sweep, the value kernels and the full solve away from the scalars and options every other GPU test runs on (tests/off_defaults.py):
a y pixel pitch of 1.25 times the x pitch, scale 1 and 3, loss scales 0.2 and 3, LM-diagonal clamps that bind, and the loop options
(initial / max / min radius, min_relative_decrease, gradient_tolerance) on both LM loops, the device's and the host's.  The bars are
those of tests/test_gpu_parity.py, tests/test_gpu_project_observations.py and tests/test_gpu_residual_report.py, unchanged;
tests/test_off_defaults_cpu.py asserts on the CPU that every case here has the property it is named for."""
import functools

import numpy as np
import pytest

import oracle
from lifcal_amd import BundleAdjustment, scene
from tests import off_defaults as od
from tests.helpers import S, anisotropic, problem
from tests.test_gpu_parity import check_sweep
from tests.test_gpu_residual_report import check_report

pytestmark = pytest.mark.gpu

ANISO = lambda sc: anisotropic(sc, od.A)
R1_ADJ = S(5, 30, None, 0xD01, 103)
R2_ADJ_ROBUST = S(5, 30, None, 0xF02, 109, outlier_fraction=0.05)

# name -> (spec, scene -> problem, options)
SWEEPS = {
    "aniso_125_0x506": (od.BASE, ANISO, {}),
    "aniso_125_0xD01": (R1_ADJ, ANISO, {}),
    "aniso_125_0xF02": (R2_ADJ_ROBUST, ANISO, {}),
    "scale_1": (od.SCALE_1, problem, {}),
    "scale_3": (od.SCALE_3, problem, {}),
    **{name: (od.ROBUST, problem, dict(loss_scale=ls)) for name, ls in od.LOSS_SCALES.items()},
    **{name: (od.BASE, problem, kw) for name, (kw, _) in od.CLAMPS.items()},
}
SOLVES = {
    "aniso_125": (od.BASE, ANISO, {}),
    "scale_1": (od.SCALE_1, problem, {}),
    "scale_3": (od.SCALE_3, problem, {}),
    **{name: (od.ROBUST, problem, dict(loss_scale=ls)) for name, ls in od.LOSS_SCALES.items()},
    **{"loop_" + name: (od.BASE, problem, kw) for name, kw in od.LOOP.items()},
}
VALUES = {
    "aniso_125": (od.BASE, ANISO),
    "aniso_125_adj_robust": (od.ROBUST, ANISO),
    "scale_3": (od.SCALE_3, problem),
    "scale_3_aniso_125": (od.SCALE_3, ANISO),
}


_SCENES = {}


def make(spec, mk):
    """the problem of `spec` through `mk`, one make_scene per spec for the module"""
    key = repr(spec)
    if key not in _SCENES:
        _SCENES[key] = scene.make_scene(spec)
    return mk(_SCENES[key])


@pytest.mark.parametrize("name", list(SWEEPS))
def test_sweep_matches_oracle(built, name):
    spec, mk, kw = SWEEPS[name]
    o = od.options(**kw)
    for radius in (1e4, 7.0):
        ref = oracle.sweep(make(spec, mk), radius=radius, options=o, threads=4)
        assert ref.rc == 0
        with BundleAdjustment(make(spec, mk), o) as ba:
            check_sweep(ba.sweep(radius, want_matrices=True), ref)


@pytest.mark.parametrize("name", list(VALUES))
def test_value_kernels_match_oracle(built, name):
    """calcReprojectionError, project_observations and the residual report at the parameters as stored (no sign folding)"""
    spec, mk = VALUES[name]
    pa = make(spec, mk)
    so, err = oracle.reproj_stats(pa, 1.0, want_errors=True)
    # x and y are told apart by every statistic, by more than its bar: a swapped axis or a pitch from the other slot cannot pass
    assert abs(so.std_x - so.std_y) > 1e-3 and abs(so.mae_x - so.mae_y) > 1e-3
    with BundleAdjustment(pa) as ba:
        st = ba.calcReprojectionError()
        x, y = ba.projectObservations()
        print(f"{name}: std {st.std_x:.6f} {st.std_y:.6f} oracle diff {abs(st.std_x - so.std_x):.2e} {abs(st.std_y - so.std_y):.2e}; "
              f"projection diff {np.max(np.abs(x - (pa.u + err[:, 0]))):.2e} {np.max(np.abs(y - (pa.v + err[:, 1]))):.2e}")
        assert abs(st.std_x - so.std_x) < 1e-10 and abs(st.std_y - so.std_y) < 1e-10
        assert abs(st.mae_x - so.mae_x) < 1e-9 and abs(st.mae_y - so.mae_y) < 1e-9
        assert (st.num_points, st.num_inliers) == (so.num_points, so.num_inliers)
        assert np.max(np.abs(x - (pa.u + err[:, 0]))) < 1e-9 and np.max(np.abs(y - (pa.v + err[:, 1]))) < 1e-9
        check_report(ba, pa, bool(spec.config & 0x200), 1.0)
    if mk is ANISO:
        # the isotropic problem's y error really is another number, its x error the same one
        iso = oracle.reproj_stats(make(spec, problem), 1.0)
        assert abs(iso.std_y - so.std_y) > 1e-3 * so.std_y and abs(iso.std_x - so.std_x) < 1e-10


@functools.lru_cache(maxsize=None)
def oracle_solve(name):
    spec, mk, kw = SOLVES[name]
    pb = make(spec, mk)
    so = oracle.solve(pb, od.options(**kw), threads=4)
    return so, pb


@pytest.mark.parametrize("loop", ["device", "host"])
@pytest.mark.parametrize("name", list(SOLVES))
def test_solve_matches_oracle(built, monkeypatch, name, loop):
    spec, mk, kw = SOLVES[name]
    monkeypatch.delenv("LIFCAL_HOST_LM", raising=False)
    if loop == "host":
        monkeypatch.setenv("LIFCAL_HOST_LM", "1")
    o = od.options(**kw)
    pa, p0 = make(spec, mk), make(spec, mk)
    with BundleAdjustment(pa, o) as ba:
        s = ba.performBundleAdjustment()
        st = ba.calcReprojectionError()
    so, pb = oracle_solve(name)
    print(f"{name} [{loop} loop]: {od.tuple_of(s)} oracle {od.tuple_of(so)}; final cost {s.final_cost:.12e} oracle {so.final_cost:.12e}; "
          f"final radius {s.final_radius:.6g} oracle {so.final_radius:.6g}")
    assert (s.iterations, s.termination) == (so.iterations, so.termination)
    assert (s.successful_steps, s.unsuccessful_steps) == (so.successful_steps, so.unsuccessful_steps)
    assert abs(s.initial_cost - so.initial_cost) <= 1e-12 * so.initial_cost
    assert abs(s.final_cost - so.final_cost) <= 1e-8 * so.final_cost
    live = 5 + (spec.config & 3) + (2 if spec.config & 4 else 0)
    assert np.allclose(pa.cam[:5], pb.cam[:5], rtol=1e-6, atol=0)
    assert np.allclose(pa.cam[5:live], pb.cam[5:live], rtol=1e-6, atol=1e-6 * np.abs(pb.cam[5:live]).max() if live > 5 else 0.0)
    assert np.all(pa.cam[live:] == 0.0)
    assert np.allclose(pa.views, pb.views, rtol=0, atol=1e-6 * (1 + np.abs(pb.views).max()))
    assert np.allclose(pa.pts, pb.pts, rtol=0, atol=1e-6 * (1 + np.abs(pb.pts).max()))
    so_st = oracle.reproj_stats(pa)
    assert abs(st.std_x - so_st.std_x) < 1e-10 and abs(st.std_y - so_st.std_y) < 1e-10
    assert abs(st.mae_x - so_st.mae_x) < 1e-9 and abs(st.mae_y - so_st.mae_y) < 1e-9
    assert (st.num_points, st.num_inliers) == (so_st.num_points, so_st.num_inliers)
    key = name[len("loop_"):] if name.startswith("loop_") else name
    if key in od.UNTOUCHED:
        assert s.iterations == 0
        for a, b in ((pa.cam, p0.cam), (pa.views, p0.views), (pa.pts, p0.pts)):
            assert a.tobytes() == b.tobytes()
    if key == "max_radius_caps":
        assert s.final_radius == 3e4 and so.final_radius == 3e4 and s.iterations == 30
    if key == "gradient_tolerance_after_steps":
        assert s.termination == od.TERM_GRADIENT and s.iterations >= 2
    if key == "min_radius_at_once":
        assert s.termination == od.TERM_MIN_RADIUS
    if key == "min_relative_decrease_rejects":
        assert s.unsuccessful_steps >= 3
