"""The seams of k_sweep3: write-once outputs stored past the L2 (A blocks, camera part of W, point gradients, U^-1,
point damping), the window flush with the words of every block first, k_finalize with its inputs requested together.  The smallest
shape that can go wrong is several blocks of several passes with split groups, where the 48-byte A pieces of different waves share
128-byte lines: 300 points over 30 frames cut into three blocks, also with distance constraints; and one scene of a single block
with a single pass, where the flush follows the first pass directly.  The reference of the sweeps is the global-atomic path
(LIFCAL_DISABLE_V2), which has none of these seams; k_backsub reads every streamed array, so one LM step is compared as well."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lifcal_amd
from lifcal_amd import BundleAdjustment, _capi as capi, scene
from tests.helpers import S, problem, scaled_max_err, vec_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = "30, 300, 8, 0xF06, 1221, outlier_fraction=0.02"
CONSTRAINED = "30, 300, 8, 0xF06, 1221, outlier_fraction=0.02, n_constraints=3"
ONE_PASS = "6, 40, None, 0xF06, 102, outlier_fraction=0.05"

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import lifcal_amd
from lifcal_amd import BundleAdjustment, _capi as capi, scene
from tests.helpers import S
sc = scene.make_scene(S(%s))
precision = %d
st = lifcal_amd.plan_stats(capi.ProblemArrays.from_scene(sc))
o = capi.default_options_py(); o.precision = precision
with BundleAdjustment(capi.ProblemArrays.from_scene(sc), o) as ba:
    r = ba.sweep(123.0, want_matrices=True)
    r2 = ba.sweep(123.0, want_matrices=True)     # the other copy of the reduced block, zero-filled by the first sweep's k_finalize
    chunks = ba.info().n_chunks
o = capi.default_options_py(); o.precision = precision; o.max_iterations = 1
pa = capi.ProblemArrays.from_scene(sc)
with BundleAdjustment(pa, o) as ba:
    s = ba.performBundleAdjustment()
np.savez(sys.argv[1], S=r.S, rhs=r.rhs, cost=r.cost, pg=r.point_gradient, ui=r.point_hessian_inv, gr=r.gradient_reduced,
         S2=r2.S, cost2=r2.cost, chunks=chunks, blocks=st.n_blocks, passes=st.n_passes, max_passes=st.max_block_passes, lanes=st.pass_lanes,
         pts=pa.pts, views=pa.views, cam=pa.cam, pts0=sc.pts0, steps=s.successful_steps)
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
    d = tmp_path_factory.mktemp("sweep_tail_ref")
    return {spec: run_child(d, spec, {"LIFCAL_DISABLE_V2": "1"}, "ref%d" % k) for k, spec in enumerate((PLAIN, CONSTRAINED, ONE_PASS))}


@pytest.fixture(scope="module")
def window_runs(built, tmp_path_factory):
    """the same on k_sweep3 with three blocks (default kernel), computed once for the tests that share it"""
    d = tmp_path_factory.mktemp("sweep_tail_win")
    return {spec: run_child(d, spec, {"LIFCAL_V2_BLOCKS": "3"}, "win%d" % k) for k, spec in enumerate((PLAIN, CONSTRAINED))}


def check_fp64_sweep(a, b):
    cost = abs(float(a["cost"]) - float(b["cost"])) / float(b["cost"])
    errs = (scaled_max_err(a["S"], b["S"]), vec_err(a["rhs"], b["rhs"]), vec_err(a["pg"], b["pg"]), vec_err(a["ui"], b["ui"]))
    print("cost %.2e S %.2e rhs %.2e point gradients %.2e U^-1 %.2e" % ((cost,) + errs))
    assert cost <= 1e-13
    assert errs[0] < 1e-10 and errs[1] < 1e-10
    assert errs[2] < 1e-11 and errs[3] < 1e-10


@pytest.mark.parametrize("spec_args", [PLAIN, CONSTRAINED], ids=["three_blocks", "three_blocks_constraints"])
def test_sweep_equals_the_atomic_path(window_runs, atomic_reference, spec_args):
    a, b = window_runs[spec_args], atomic_reference[spec_args]
    assert int(a["chunks"]) >= 2 and int(b["chunks"]) == 0 and int(a["blocks"]) >= 2 and int(a["max_passes"]) >= 2 and int(a["lanes"]) == 256
    check_fp64_sweep(a, b)


@pytest.mark.parametrize("spec_args", [PLAIN, CONSTRAINED], ids=["three_blocks", "three_blocks_constraints"])
def test_sweep_with_two_waves_per_role_equals_the_atomic_path(tmp_path, atomic_reference, spec_args):
    a = run_child(tmp_path, spec_args, {"LIFCAL_V2_BLOCKS": "3", "LIFCAL_SWEEP_WAVES": "2"}, "w2")
    assert int(a["chunks"]) >= 2 and int(a["lanes"]) == 128 and int(a["max_passes"]) >= 2
    check_fp64_sweep(a, atomic_reference[spec_args])


@pytest.mark.parametrize("spec_args", [PLAIN, CONSTRAINED], ids=["three_blocks", "three_blocks_constraints"])
def test_fp32_evaluation_sweep_equals_its_fp64_arm(tmp_path, atomic_reference, spec_args):
    """options.precision = 1 against the fp64 sweep of the scene, at the bars of tests/test_gpu_precision1.py"""
    a, b = run_child(tmp_path, spec_args, {"LIFCAL_V2_BLOCKS": "3"}, "f32", precision=1), atomic_reference[spec_args]
    assert int(a["chunks"]) >= 2 and int(a["max_passes"]) >= 2
    cost = abs(float(a["cost"]) - float(b["cost"])) / float(b["cost"])
    errs = (scaled_max_err(a["S"], b["S"]), vec_err(a["rhs"], b["rhs"]), vec_err(a["gr"], b["gr"]))
    print("cost %.2e S %.2e rhs %.2e reduced gradient %.2e" % ((cost,) + errs))
    assert cost <= 2e-6
    assert errs[0] < 2e-5 and errs[1] < 2e-4 and errs[2] < 2e-4


def test_single_block_single_pass_equals_the_atomic_path(tmp_path, atomic_reference):
    """one block whose only pass is also its last: nothing is fetched ahead, the flush follows the first pass directly"""
    a = run_child(tmp_path, ONE_PASS, {"LIFCAL_V2_BLOCKS": "1"}, "one")
    assert int(a["chunks"]) == 1 and int(a["blocks"]) == 1 and int(a["passes"]) == 1
    check_fp64_sweep(a, atomic_reference[ONE_PASS])


@pytest.mark.parametrize("spec_args", [PLAIN, CONSTRAINED], ids=["three_blocks", "three_blocks_constraints"])
def test_one_lm_step_equals_the_atomic_path(window_runs, atomic_reference, spec_args):
    """the back-substitution reads the A blocks, the camera part of W, the point gradients, U^-1 and the point damping: every streamed array"""
    a, b = window_runs[spec_args], atomic_reference[spec_args]
    assert int(a["steps"]) == 1 and int(b["steps"]) == 1 and np.any(b["pts"] != b["pts0"])
    errs = (vec_err(a["pts"], b["pts"]), vec_err(a["views"], b["views"]))
    print("points %.2e poses %.2e" % errs)
    assert errs[0] <= 1e-10 and errs[1] <= 1e-10


@pytest.mark.parametrize("spec_args", [PLAIN, CONSTRAINED], ids=["three_blocks", "three_blocks_constraints"])
def test_two_sweeps_in_a_row_on_one_handle_are_equal(window_runs, spec_args):
    """the second sweep accumulates into the copy of the reduced block that the first one's k_finalize zero-filled"""
    a = window_runs[spec_args]
    cost = abs(float(a["cost2"]) - float(a["cost"])) / float(a["cost"])
    err = scaled_max_err(a["S2"], a["S"])
    print("cost %.2e S %.2e" % (cost, err))
    assert cost <= 1e-12 and err <= 1e-12


def test_ordered_sweeps_are_bitwise_equal(built, monkeypatch):
    """options.deterministic = 1: two handles give the same bits"""
    monkeypatch.delenv("LIFCAL_PLAN_BALANCE", raising=False)
    monkeypatch.setenv("LIFCAL_V2_BLOCKS", "3")
    sc = scene.make_scene(S(30, 300, 8, 0xF06, 1221, outlier_fraction=0.02))
    assert lifcal_amd.plan_stats(problem(sc)).n_blocks >= 2
    o = capi.default_options_py(); o.deterministic = 1
    runs = []
    for handle in range(2):
        with BundleAdjustment(problem(sc), o) as ba:
            g = ba.sweep(1e3, want_matrices=True)
            runs.append((g.S.copy(), g.rhs.copy(), g.point_gradient.copy()))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
