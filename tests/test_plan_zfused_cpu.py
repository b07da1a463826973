"""The plans tests/test_gpu_sweep_zfused.py runs on hold what the two-round emission of k_sweep3 can break (host only, through
lifcal_amd.plan_stats and lifcal_amd.plan_shape): blocks of several passes (the counters eval_done and factor_done are monotone over the
kernel), passes of ONE point and of 64 (the factor phase on one lane and on all of wave 0), and, with LIFCAL_GROUP_SPLIT=2, groups cut
into several lanes, which add their parts of L^-1 W to the same cells of Z."""
import lifcal_amd
from lifcal_amd import _capi as capi, scene
from tests.helpers import S
from tests.test_gpu_sweep_loads import CUTS, PLAIN


def plan(monkeypatch, spec, v2_blocks, split=None, waves=None):
    for k in ("LIFCAL_PLAN_BALANCE", "LIFCAL_SWEEP_KERNEL", "LIFCAL_DISABLE_V2", "LIFCAL_GROUP_SPLIT", "LIFCAL_SWEEP_WAVES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LIFCAL_V2_BLOCKS", str(v2_blocks))
    if split is not None:
        monkeypatch.setenv("LIFCAL_GROUP_SPLIT", str(split))
    if waves is not None:
        monkeypatch.setenv("LIFCAL_SWEEP_WAVES", str(waves))
    pa = capi.ProblemArrays.from_scene(scene.make_scene(eval("S(%s)" % spec, {"S": S})))
    return lifcal_amd.plan_stats(pa), lifcal_amd.plan_shape(pa)


def test_the_cuts_hold_passes_of_one_and_of_64_points_and_blocks_of_several_passes(monkeypatch):
    st, sh = {}, {}
    for cut in ("w3", "w300", "few1"):
        st[cut], sh[cut] = plan(monkeypatch, CUTS[cut][0], CUTS[cut][1])
        print(cut, "blocks", st[cut].n_blocks, "passes", st[cut].n_passes, "points per pass", sh[cut].min_pass_points, sh[cut].max_pass_points,
              "passes per block", sh[cut].min_block_passes, sh[cut].max_block_passes)
        assert st[cut].n_blocks == CUTS[cut][2] and st[cut].violations == 0 and st[cut].pass_lanes == 256
    assert sh["w3"].min_block_passes >= 4 and sh["w3"].max_block_passes <= 5
    assert sh["w300"].min_pass_points == 1
    assert sh["few1"].max_pass_points == 64 and sh["few1"].min_block_passes >= 3


def test_group_split_two_cuts_groups_into_more_lanes(monkeypatch):
    whole, _ = plan(monkeypatch, PLAIN, 3)
    split, sh = plan(monkeypatch, PLAIN, 3, split=2)
    print("lanes: unsplit %d, split %d; passes %d -> %d" % (whole.n_lanes, split.n_lanes, whole.n_passes, split.n_passes))
    assert split.violations == 0 and split.n_blocks == 3
    assert split.n_lanes > whole.n_lanes
    assert sh.min_block_passes >= 3


def test_two_waves_per_role_keep_the_cases(monkeypatch):
    for cut in ("w3", "w300", "few1"):
        st, sh = plan(monkeypatch, CUTS[cut][0], CUTS[cut][1], waves=2)
        assert st.violations == 0 and st.pass_lanes == 128 and 1 <= sh.min_pass_points <= sh.max_pass_points <= 32
