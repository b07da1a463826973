"""The conditions under which the off-default GPU tests (tests/test_gpu_step.py, tests/test_gpu_off_defaults.py and the batch routes)
say something, asserted on the CPU references alone: the anisotropic problem is the isotropic one exactly, every clamp case clips
what it claims to, every loop-option case ends or bends the oracle's trajectory the way its name says."""
import numpy as np
import pytest

import oracle
from lifcal_amd import scene
from tests import off_defaults as od, step_reference as sr
from tests.helpers import S, anisotropic, problem


@pytest.mark.parametrize("spec", [od.BASE, od.ROBUST, S(6, 40, None, 0xF06, 120, recalib=True)], ids=["0x506", "0xF06_robust", "0xF06_bounds"])
def test_anisotropic_problem_is_the_isotropic_one(spec):
    """spy = a spx with v, mcy and the raw principal point divided by a: r_x unchanged, r_y divided by a (|r| <= 37 pixels: 1e-11 is
    a few hundred roundings of the y chain), and an anisotropy that is really there"""
    sc = scene.make_scene(spec)
    pa, pb = problem(sc), anisotropic(sc, od.A)
    assert pb.struct.spy == od.A * pb.struct.spx and pa.struct.spy == pa.struct.spx
    r, q = oracle.residuals(pa), oracle.residuals(pb)
    dx, dy = np.max(np.abs(q[:, 0] - r[:, 0])), np.max(np.abs(od.A * q[:, 1] - r[:, 1]))
    print(f"max |r_x' - r_x| = {dx:.3g}, max |a r_y' - r_y| = {dy:.3g}, max |r| = {np.max(np.abs(r)):.3g}")
    assert dx <= 1e-11 and dy <= 1e-11
    assert np.max(np.abs(q[:, 1] - r[:, 1])) > 0.1          # a y pitch read from the x slot would show
    craw = lambda c: (c + 0.5) * sc.scale - 0.5
    assert abs(craw(pb.cam[4]) * od.A - craw(pa.cam[4])) <= 1e-12 * craw(pa.cam[4]) and pb.cam[3] == pa.cam[3]
    if sc.lower is not None:
        for k in (1, 3):
            assert pb.lower[k] == pa.lower[k] and pb.upper[k] == pa.upper[k]
        assert pb.lower[4] < pb.cam[4] < pb.upper[4]
        assert abs(craw(pb.lower[4]) * od.A - craw(pa.lower[4])) <= 1e-12 * craw(pa.lower[4])
        assert np.all(np.isinf(pb.lower[5:])) and np.all(np.isinf(pb.upper[5:]))


def test_anisotropic_problem_solves_like_any_other():
    """oracle: (14, 13, 0, 1), final cost 10.09"""
    s = oracle.solve(anisotropic(scene.make_scene(od.BASE), od.A), threads=4)
    assert s.termination == od.TERM_FUNCTION and 5 <= s.iterations <= 40 and s.final_cost < 1e-3 * s.initial_cost


@pytest.mark.parametrize("name", list(od.CLAMPS))
def test_clamp_cases_clip(name):
    kw, sides = od.CLAMPS[name]
    o = od.options(**kw)
    pa = problem(scene.make_scene(od.BASE))
    ne = sr.NormalEquations(pa, od.RADIUS, jacobi_scaling=bool(o.jacobi_scaling), lm_min=o.min_lm_diagonal, lm_max=o.max_lm_diagonal)
    below, above = od.clip_counts(ne, o.min_lm_diagonal, o.max_lm_diagonal)
    print(f"{name}: {below} below, {above} above of {int(np.sum(ne.live))} live entries")
    if "below" in sides:
        assert below >= 20
    if "above" in sides:
        assert above >= 20
    # the reference's lambda is the clamped one on exactly those entries
    t = (ne.h.astype(np.float64) * ne.sigma ** 2)
    free = ne.live & (t >= o.min_lm_diagonal) & (t <= o.max_lm_diagonal)
    lam = ne.lam.astype(np.float64)
    assert np.allclose(lam[free], ne.h.astype(np.float64)[free] / od.RADIUS, rtol=1e-14, atol=0)
    lo = ne.live & (t < o.min_lm_diagonal)
    assert np.allclose(lam[lo], o.min_lm_diagonal / (od.RADIUS * ne.sigma[lo] ** 2), rtol=1e-15, atol=0)
    hi = ne.live & (t > o.max_lm_diagonal)
    assert np.allclose(lam[hi], o.max_lm_diagonal / (od.RADIUS * ne.sigma[hi] ** 2), rtol=1e-15, atol=0)


def test_default_clamp_never_binds():
    """why the cases above are needed: with 1e-6 / 1e32 nothing is clipped on the suite's scenes"""
    ne = sr.NormalEquations(problem(scene.make_scene(od.BASE)), od.RADIUS)
    assert od.clip_counts(ne, 1e-6, 1e32) == (0, 0)


def solve(**kw):
    return oracle.solve(problem(scene.make_scene(od.BASE)), od.options(**kw), threads=4)


def test_loop_option_cases_have_the_property_they_are_named_for():
    s = {name: solve(**kw) for name, kw in od.LOOP.items()}
    t = {name: od.tuple_of(v) for name, v in s.items()}
    for name, v in t.items():
        print(name, v, s[name].final_radius)
    assert t["defaults"][3] == od.TERM_FUNCTION and t["defaults"][2] == 0
    assert t["gradient_tolerance_at_the_first_sweep"] == (0, 0, 0, od.TERM_GRADIENT)
    g = t["gradient_tolerance_after_steps"]
    assert g[3] == od.TERM_GRADIENT and g[0] >= 2 and g[0] < t["defaults"][0]
    assert t["min_radius_at_once"] == (0, 0, 0, od.TERM_MIN_RADIUS)
    m = s["max_radius_caps"]
    assert t["max_radius_caps"][3] == od.TERM_MAX_ITERATIONS and t["max_radius_caps"][0] == 30 and m.final_radius == 3e4
    assert s["defaults"].final_radius > 3e4                       # the cap is what held it
    assert t["initial_radius_small"][3] == od.TERM_FUNCTION and t["initial_radius_small"][0] > t["defaults"][0] + 5
    r = t["min_relative_decrease_rejects"]
    assert r[3] == od.TERM_FUNCTION and r[2] >= 3
    for name in ("lm_min_2", "lm_max_05", "lm_1e2_1e6_unscaled"):
        assert t[name][3] == od.TERM_FUNCTION and t[name] != t["defaults"], name


def test_loss_scale_and_scale_cases_differ_from_the_defaults():
    """the trajectories the GPU has to follow are not the default one"""
    sc = scene.make_scene(od.ROBUST)
    its = {ls: oracle.solve(problem(sc), od.options(loss_scale=ls), threads=4).iterations for ls in (0.2, 0.5, 3.0)}
    print("iterations by loss_scale", its)
    assert len(set(its.values())) == 3
    c = {ls: oracle.cost(problem(sc), loss_scale=ls, threads=4) for ls in (0.2, 0.5, 3.0)}
    assert c[0.2] < c[0.5] < c[3.0]
    n = {spec.scale: scene.make_scene(spec).n_obs for spec in (od.SCALE_1, od.BASE, od.SCALE_3)}
    print("observations by scale", n)
    assert all(900 <= v <= 1400 for v in n.values())
    for spec in (od.SCALE_1, od.SCALE_3):
        s = oracle.solve(problem(scene.make_scene(spec)), threads=4)
        assert s.termination == od.TERM_FUNCTION and s.iterations <= 40
