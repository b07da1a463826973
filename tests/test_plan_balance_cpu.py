"""The planner's processing order and block cut: inside a block the points are processed in order of falling mean
observations per (point, frame) pair, the group ids follow that order, and the blocks are cut to even out their modelled cost.
Host only: lifcal_ba_plan_stats recounts the layout contracts from the finished arrays (`violations`), LIFCAL_PLAN_BALANCE=0 is the
plan of the point order and of blocks cut by observation count, the reference of the comparisons."""
import itertools
import re

import pytest

import lifcal_amd
from lifcal_amd import scene
from tests.helpers import S, oracle_lens_selector, problem

SCENES = {
    "all_visible": S(6, 40, None, 0x506, 603),
    "windowed": S(24, 120, 6, 0xF06, 604),
    "constraints": S(6, 40, None, 0x506, 605, n_constraints=3),
    "w8_f30_300_points": S(30, 300, 8, 0xF06, 1204, outlier_fraction=0.02),
    "w8_f40_2500_points": scene.SceneSpec(40, 2500, 8, 0xF06, 4242, outlier_fraction=0.02),
}
# (LIFCAL_SWEEP_KERNEL, LIFCAL_SWEEP_WAVES): 256-lane frame-ordered passes, point-ordered passes, 128-lane passes
LAYOUTS = [("3", None), ("2", None), ("3", "2")]
BLOCKS = [None, "1", "3", "64"]


def _setenv(monkeypatch, name, value):
    if value is None:
        monkeypatch.delenv(name, raising=False)
    else:
        monkeypatch.setenv(name, value)


@pytest.mark.parametrize("name", list(SCENES))
def test_layout_contracts_hold_for_every_plan(built, monkeypatch, name):
    """every regular point in exactly one pass, lanes <= pass_lanes, points <= the block's Z-matrix cap, lanes sorted by frame, lane
    sizes adding up to the observations, group ids of a point and of a pass one run each with no special point's groups inside"""
    pa = problem(scene.make_scene(SCENES[name]))
    permuted = 0
    for balance, (kernel, waves), blocks in itertools.product((None, "0"), LAYOUTS, BLOCKS):
        _setenv(monkeypatch, "LIFCAL_PLAN_BALANCE", balance)
        _setenv(monkeypatch, "LIFCAL_SWEEP_KERNEL", kernel)
        _setenv(monkeypatch, "LIFCAL_SWEEP_WAVES", waves)
        _setenv(monkeypatch, "LIFCAL_V2_BLOCKS", blocks)
        st = lifcal_amd.plan_stats(pa)
        tag = (name, balance, kernel, waves, blocks)
        assert st.violations == 0, tag
        assert st.pass_lanes == (128 if waves == "2" else 256), tag
        assert st.n_blocks >= 1 and st.n_passes >= st.n_blocks and st.n_obs_window > 0, tag
        if balance == "0":
            assert st.n_points_permuted == 0, tag
        else:
            permuted += st.n_points_permuted
    print(name, "points moved by the processing order, summed over the plans:", permuted)
    # the scenes with several points per pass and mixed pair sizes must actually exercise the new order
    if name in ("w8_f30_300_points", "w8_f40_2500_points", "windowed"):
        assert permuted > 0


@pytest.fixture(scope="module")
def big_scenes():
    spec = scene.baseline_spec("metric_web")
    return {"cfg3": scene.make_scene(scene.baseline_spec("cfg3")),
            "metric_web": scene.make_scene(spec, lens_selector=oracle_lens_selector(spec))}


@pytest.mark.parametrize("name", ["cfg3", "metric_web"])
def test_balanced_plan_against_the_plan_of_the_point_order(built, monkeypatch, big_scenes, name):
    """never more blocks and never a larger modelled maximum than the observation-count cut (it is the fallback of the block cut); on the
    bench scene the slowest block falls to <= 0.945x and the observation steps of the passes to <= 0.925x: half the reductions a replica
    of the planner measured (-11.1 % and -15.0 %)"""
    pa = problem(big_scenes[name])
    for var in ("LIFCAL_SWEEP_KERNEL", "LIFCAL_SWEEP_WAVES", "LIFCAL_V2_BLOCKS", "LIFCAL_GROUP_SPLIT", "LIFCAL_PLAN_COST", "LIFCAL_DISABLE_V2"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("LIFCAL_PLAN_BALANCE", "0")
    old = lifcal_amd.plan_stats(pa)
    monkeypatch.delenv("LIFCAL_PLAN_BALANCE")
    new = lifcal_amd.plan_stats(pa)
    for tag, st in (("point order", old), ("balanced", new)):
        print(f"[{name}] {tag}: blocks {st.n_blocks} passes {st.n_passes} lanes {st.n_lanes} pass steps {st.pass_steps} tile steps {st.tile_steps} "
              f"block cost mean {st.block_cost_mean:.0f} max {st.block_cost_max:.0f} max passes {st.max_block_passes} moved {st.n_points_permuted}")
    assert old.violations == 0 and new.violations == 0
    assert old.n_points_permuted == 0 and new.n_points_permuted > 0
    assert new.n_obs_window == old.n_obs_window
    assert new.n_blocks <= old.n_blocks
    assert new.block_cost_max <= old.block_cost_max
    if name == "metric_web":
        assert new.block_cost_max <= 0.945 * old.block_cost_max
        assert new.pass_steps <= 0.925 * old.pass_steps


@pytest.mark.parametrize("blocks", [None, "3"], ids=["default_blocks", "three_blocks"])
def test_planner_threads_do_not_change_the_balanced_layout(built, capfd, monkeypatch, blocks):
    """the blocks of a candidate cut are solved by the planner's host threads; the fingerprint of the layout (LIFCAL_PLAN_HASH) is the same
    with one thread, three and eight"""
    pa = problem(scene.make_scene(SCENES["w8_f40_2500_points"]))
    monkeypatch.delenv("LIFCAL_PLAN_BALANCE", raising=False)
    monkeypatch.setenv("LIFCAL_PLAN_HASH", "1")
    _setenv(monkeypatch, "LIFCAL_V2_BLOCKS", blocks)
    seen = {}
    for threads in ("1", "3", "8"):
        monkeypatch.setenv("LIFCAL_PLAN_THREADS", threads)
        capfd.readouterr()
        st = lifcal_amd.plan_stats(pa)
        m = re.search(r"\[plan\] hash ([0-9a-f]{16})", capfd.readouterr().err)
        assert m
        assert st.violations == 0 and st.n_points_permuted > 0
        seen[threads] = (m.group(1), st.n_blocks, st.n_passes, st.n_lanes, st.pass_steps, st.block_cost_max)
    assert seen["1"] == seen["3"] == seen["8"]


def test_unknown_sweep_kernel_values_plan_like_the_default(built, capfd, monkeypatch):
    """LIFCAL_SWEEP_KERNEL knows 2; every other value (4 named a kernel pair that is gone) is the default: 256-lane passes and the
    layout fingerprint (LIFCAL_PLAN_HASH) of the plan built with the variable unset"""
    pa = problem(scene.make_scene(SCENES["w8_f30_300_points"]))
    for var in ("LIFCAL_SWEEP_WAVES", "LIFCAL_V2_BLOCKS", "LIFCAL_GROUP_SPLIT", "LIFCAL_PLAN_COST", "LIFCAL_PLAN_BALANCE", "LIFCAL_DISABLE_V2"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("LIFCAL_PLAN_HASH", "1")
    seen = {}
    for kernel in (None, "4", "junk"):
        _setenv(monkeypatch, "LIFCAL_SWEEP_KERNEL", kernel)
        capfd.readouterr()
        st = lifcal_amd.plan_stats(pa)
        m = re.search(r"\[plan\] hash ([0-9a-f]{16})", capfd.readouterr().err)
        assert m
        assert st.violations == 0 and st.pass_lanes == 256, kernel
        seen[kernel] = m.group(1)
    assert seen["4"] == seen[None] and seen["junk"] == seen[None], seen
