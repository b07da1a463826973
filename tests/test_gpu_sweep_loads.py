"""The evaluator loads of k_sweep3 (profiles/sweep_loads/): the point scales of the factor phase are requested behind
the observation loop, on EVERY lane (v2_passpt is padded with point 0, so the lanes beyond the pass's points read point 0's scales
and do not use them), and the pass prefetch fetches no word nobody reads.  What that can break is the factor phase of passes with one
and with 64 points, the first and the last pass of a block, and the prefetch of the last pass; the cases below also cover the loop's
prologue, its odd tail and the clamped prefetch of the last tile.  The 30-frame, 300-point scene of tests/test_gpu_sweep_tail.py is cut
several ways and a three-frame scene added (CUTS); that the cuts together hold every one of those cases — tiles of 0, 1, 2 and an odd number >= 3 of steps, passes
of 1 and of 64 points, blocks of one and of at least three passes, the last tile's reads inside the padded arrays — is asserted on the
CPU in tests/test_plan_shape.py through lifcal_amd.plan_shape, and again here on the figures the child processes record.  The reference
of the sweeps is the global-atomic path (LIFCAL_DISABLE_V2), in child processes as in tests/test_gpu_sweep_hot_rows.py, at that file's
bars."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import scaled_max_err, vec_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = "30, 300, 8, 0xF06, 1221, outlier_fraction=0.02"
CONSTRAINED = PLAIN + ", n_constraints=3"
# three frames, every point in all of them: three lanes per point and a window narrow enough for the cap of 64 points per pass
FEW_FRAMES = "3, 300, None, 0xF06, 1223, outlier_fraction=0.02"
# name -> (scene, LIFCAL_V2_BLOCKS, blocks of the plan).  What each adds (tests/test_plan_shape.py): w3 blocks of 4 and 5 passes, tiles of 2, odd and
# even steps; w20 one-pass blocks; w80 a tile of ONE step; w300 passes of ONE point, three empty tiles per pass, an empty last tile; few1 passes
# of 64 points, a block of five passes, a last tile that is not empty
CUTS = {"w3": (PLAIN, 3, 3), "w20": (PLAIN, 20, 20), "w80": (PLAIN, 80, 70), "w300": (PLAIN, 300, 206), "few1": (FEW_FRAMES, 1, 1)}

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import lifcal_amd
from lifcal_amd import BundleAdjustment, _capi as capi, scene
from tests.helpers import S
sc = scene.make_scene(S(%s))
precision = %d
st = lifcal_amd.plan_stats(capi.ProblemArrays.from_scene(sc))
sh = lifcal_amd.plan_shape(capi.ProblemArrays.from_scene(sc))
o = capi.default_options_py(); o.precision = precision
with BundleAdjustment(capi.ProblemArrays.from_scene(sc), o) as ba:
    r = ba.sweep(123.0, want_matrices=True)
    r2 = ba.sweep(123.0, want_matrices=True)
    r3 = ba.sweep(123.0, want_matrices=True)
    chunks = ba.info().n_chunks
o = capi.default_options_py(); o.precision = precision; o.max_iterations = 1
pa = capi.ProblemArrays.from_scene(sc)
with BundleAdjustment(pa, o) as ba:
    s = ba.performBundleAdjustment()
np.savez(sys.argv[1], S=r.S, rhs=r.rhs, cost=r.cost, gmax=r.gradient_max_norm, pg=r.point_gradient, ui=r.point_hessian_inv, gr=r.gradient_reduced,
         S2=r2.S, cost2=r2.cost, rhs2=r2.rhs, S3=r3.S, cost3=r3.cost, rhs3=r3.rhs, chunks=chunks, blocks=st.n_blocks, passes=st.n_passes,
         longest=st.max_block_passes, lanes=st.pass_lanes, n_lanes=st.n_lanes, pass_steps=st.pass_steps, tile_steps=st.tile_steps,
         violations=st.violations, shape=np.array([getattr(sh, n) for n, _ in sh._fields_], np.int64), shape_names=np.array([n for n, _ in sh._fields_]), pts=pa.pts, views=pa.views, pts0=sc.pts0, steps=s.successful_steps)
"""


def run_child(out_dir, spec_args, env_extra, tag, precision=0):
    out = os.path.join(str(out_dir), tag + ".npz")
    env = dict(os.environ); env.update(env_extra)
    for k in ("LIFCAL_PLAN_BALANCE", "LIFCAL_SWEEP_KERNEL"):
        env.pop(k, None)
    subprocess.check_call([sys.executable, "-c", _CHILD % (ROOT, spec_args, precision), out], env=env, cwd=ROOT)
    return np.load(out)


@pytest.fixture(scope="module")
def atomic_reference(built, tmp_path_factory):
    """sweep and one LM step of each scene on the global-atomic kernels (fp64), computed once"""
    d = tmp_path_factory.mktemp("sweep_loads_ref")
    return {spec: run_child(d, spec, {"LIFCAL_DISABLE_V2": "1"}, "ref%d" % k) for k, spec in enumerate((PLAIN, CONSTRAINED, FEW_FRAMES))}


@pytest.fixture(scope="module")
def window_runs(built, tmp_path_factory):
    """every cut on k_sweep3 (fp64, four waves per role), computed once for the tests that share them"""
    d = tmp_path_factory.mktemp("sweep_loads_win")
    return {name: run_child(d, spec, {"LIFCAL_V2_BLOCKS": str(v)}, name) for name, (spec, v, _) in CUTS.items()}


def check_fp64_sweep(a, b):
    cost = abs(float(a["cost"]) - float(b["cost"])) / float(b["cost"])
    errs = (scaled_max_err(a["S"], b["S"]), vec_err(a["rhs"], b["rhs"]), vec_err(a["pg"], b["pg"]), vec_err(a["ui"], b["ui"]))
    print("cost %.2e S %.2e rhs %.2e point gradients %.2e U^-1 %.2e" % ((cost,) + errs))
    assert cost <= 1e-13
    assert errs[0] < 1e-10 and errs[1] < 1e-10
    assert errs[2] < 1e-11 and errs[3] < 1e-10


def shape_of(a):
    return dict(zip([str(n) for n in a["shape_names"]], [int(x) for x in a["shape"]]))


def test_the_scenes_hold_what_the_change_can_break(window_runs):
    """the plans the child processes ran on (tests/test_plan_shape.py asserts the same on the CPU)"""
    sh = {name: shape_of(a) for name, a in window_runs.items()}
    for name, (_, v, blocks) in CUTS.items():
        a = window_runs[name]
        print("%s: blocks %d passes %d %s" % (name, int(a["blocks"]), int(a["passes"]), sh[name]))
        assert int(a["blocks"]) == blocks and int(a["violations"]) == 0 and int(a["lanes"]) == 256 and int(a["chunks"]) >= 1
        assert sh[name]["max_row_read"] < sh[name]["ell_rows"]
    assert sh["w300"]["tiles_0_steps"] > 0 and sh["w80"]["tiles_1_step"] > 0 and sh["w3"]["tiles_2_steps"] > 0 and sh["w3"]["tiles_odd_steps"] > 0
    assert sh["w300"]["min_pass_points"] == 1 and sh["few1"]["max_pass_points"] == 64
    assert sh["w20"]["max_block_passes"] == 1 and sh["w3"]["min_block_passes"] >= 3 and sh["few1"]["min_block_passes"] >= 3
    assert sh["w300"]["last_tile_steps"] == 0 and sh["few1"]["last_tile_steps"] > 0


@pytest.mark.parametrize("cut", sorted(CUTS))
def test_sweep_equals_the_atomic_path(window_runs, atomic_reference, cut):
    check_fp64_sweep(window_runs[cut], atomic_reference[CUTS[cut][0]])


@pytest.mark.parametrize("v2_blocks", [3, 300])
def test_sweep_with_constraints_equals_the_atomic_path(tmp_path, atomic_reference, v2_blocks):
    a = run_child(tmp_path, CONSTRAINED, {"LIFCAL_V2_BLOCKS": str(v2_blocks)}, "con")
    assert int(a["blocks"]) >= 3
    check_fp64_sweep(a, atomic_reference[CONSTRAINED])


@pytest.mark.parametrize("cut", ["w3", "w300", "few1"])
def test_sweep_with_two_waves_per_role_equals_the_atomic_path(tmp_path, atomic_reference, cut):
    spec, v, _ = CUTS[cut]
    a = run_child(tmp_path, spec, {"LIFCAL_V2_BLOCKS": str(v), "LIFCAL_SWEEP_WAVES": "2"}, "w2")
    assert int(a["lanes"]) == 128
    check_fp64_sweep(a, atomic_reference[spec])


@pytest.mark.parametrize("cut", ["w3", "w300", "few1"])
def test_fp32_evaluation_sweep_equals_its_fp64_arm(tmp_path, atomic_reference, cut):
    """options.precision = 1 against the fp64 sweep of the scene, at the bars of tests/test_gpu_sweep_tail.py"""
    spec, v, blocks = CUTS[cut]
    a, b = run_child(tmp_path, spec, {"LIFCAL_V2_BLOCKS": str(v)}, "f32", precision=1), atomic_reference[spec]
    assert int(a["blocks"]) == blocks
    cost = abs(float(a["cost"]) - float(b["cost"])) / float(b["cost"])
    errs = (scaled_max_err(a["S"], b["S"]), vec_err(a["rhs"], b["rhs"]), vec_err(a["gr"], b["gr"]))
    print("cost %.2e S %.2e rhs %.2e reduced gradient %.2e" % ((cost,) + errs))
    assert cost <= 2e-6
    assert errs[0] < 2e-5 and errs[1] < 2e-4 and errs[2] < 2e-4


@pytest.mark.parametrize("cut", sorted(CUTS))
def test_three_sweeps_in_a_row_on_one_handle_are_equal(window_runs, cut):
    a = window_runs[cut]
    for k in ("2", "3"):
        cost = abs(float(a["cost" + k]) - float(a["cost"])) / float(a["cost"])
        errs = (scaled_max_err(a["S" + k], a["S"]), vec_err(a["rhs" + k], a["rhs"]))
        print("sweep %s: cost %.2e S %.2e rhs %.2e" % ((k, cost) + errs))
        assert cost <= 1e-12 and errs[0] <= 1e-12 and errs[1] <= 1e-12


@pytest.mark.parametrize("cut", sorted(CUTS))
def test_one_lm_step_equals_the_atomic_path(window_runs, atomic_reference, cut):
    a, b = window_runs[cut], atomic_reference[CUTS[cut][0]]
    assert int(a["steps"]) == 1 and int(b["steps"]) == 1 and np.any(b["pts"] != b["pts0"])
    errs = (vec_err(a["pts"], b["pts"]), vec_err(a["views"], b["views"]))
    print("points %.2e poses %.2e" % errs)
    assert errs[0] <= 1e-10 and errs[1] <= 1e-10
