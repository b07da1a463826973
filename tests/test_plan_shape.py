"""lifcal_ba_plan_shape (host only): the LDS-window schedule tile by tile and pass by pass, and that the cuts of
tests/test_gpu_sweep_loads.py contain every edge case of k_sweep3's evaluator path that the file names: a wave's observation loop
over 0, 1, 2 and an odd number >= 3 of rows (prologue order, the odd tail of the loop unrolled by two), a pass of ONE point and a pass
of 64 (the factor phase's lanes beyond the pass's points read point 0 through the padded v2_passpt), blocks of one pass and of at least
three, and the last tile of the last block, whose prologue and clamped prefetch must stay inside the rows the padded arrays hold."""
import pytest

import lifcal_amd
from lifcal_amd import _capi as capi, scene
from tests.helpers import S
from tests.test_gpu_sweep_loads import CUTS


def shapes(monkeypatch, spec, v2_blocks, waves=None):
    for k in ("LIFCAL_PLAN_BALANCE", "LIFCAL_SWEEP_KERNEL", "LIFCAL_DISABLE_V2", "LIFCAL_GROUP_SPLIT", "LIFCAL_SWEEP_WAVES"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("LIFCAL_V2_BLOCKS", str(v2_blocks))
    if waves:
        monkeypatch.setenv("LIFCAL_SWEEP_WAVES", str(waves))
    pa = capi.ProblemArrays.from_scene(scene.make_scene(eval("S(%s)" % spec, {"S": S})))
    return lifcal_amd.plan_stats(pa), lifcal_amd.plan_shape(pa)


@pytest.mark.parametrize("waves", [None, 2])
@pytest.mark.parametrize("cut", sorted(CUTS))
def test_shape_agrees_with_the_totals_of_plan_stats(monkeypatch, cut, waves):
    st, sh = shapes(monkeypatch, CUTS[cut][0], CUTS[cut][1], waves)
    tiles = sh.tiles_0_steps + sh.tiles_1_step + sh.tiles_2_steps + sh.tiles_odd_steps + sh.tiles_even_steps
    assert st.violations == 0 and st.pass_lanes == (128 if waves == 2 else 256) and tiles == st.n_passes * (st.pass_lanes // 64)
    assert sh.max_block_passes == st.max_block_passes and 1 <= sh.min_block_passes <= sh.max_block_passes
    assert 1 <= sh.min_pass_points <= sh.max_pass_points <= st.pass_lanes // 4
    # every row of the payload belongs to one tile; the arrays hold the payload and a row of padding
    assert sh.last_tile_row0 + sh.last_tile_steps == st.tile_steps and sh.ell_rows == st.tile_steps + 1
    # no wave reads beyond the arrays: an empty last tile reads the padding row, any other its own last row at most
    assert sh.max_row_read < sh.ell_rows and sh.max_row_read >= sh.last_tile_row0 + max(sh.last_tile_steps, 1) - 1


def test_the_cuts_of_the_sweep_loads_tests_hold_every_named_case(monkeypatch):
    sh = {}
    for name, (spec, v, blocks) in CUTS.items():
        st, sh[name] = shapes(monkeypatch, spec, v)
        print(name, {n: getattr(sh[name], n) for n, _ in sh[name]._fields_})
        assert st.n_blocks == blocks and st.pass_lanes == 256
    assert sh["w300"].tiles_0_steps > 0 and sh["w80"].tiles_1_step > 0 and sh["w3"].tiles_2_steps > 0 and sh["w3"].tiles_odd_steps > 0
    assert sh["w300"].min_pass_points == 1 and sh["few1"].max_pass_points == 64
    assert sh["w20"].max_block_passes == 1 and sh["w3"].min_block_passes >= 3 and sh["few1"].min_block_passes >= 3
    # the last tile of the last block: empty (its wave reads only the padding row) and not empty
    assert sh["w300"].last_tile_steps == 0 and sh["w300"].last_tile_row0 == sh["w300"].ell_rows - 1
    assert sh["few1"].last_tile_steps > 0
