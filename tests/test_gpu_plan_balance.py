"""The planner's processing order on the GPU: points of a block processed by falling mean pair size, group ids renumbered
to follow, blocks cut by modelled cost.  The smallest shape that can go wrong is several blocks of several passes with mixed pair
sizes: 300 points over 30 frames cut into three blocks.  With distance constraints, promoted and special points sit inside the block
ranges and the renumbering has to step around their groups.  The reference of the sweeps is the global-atomic path (LIFCAL_DISABLE_V2),
which uses no passes at all; the solve (its back-substitution reads the A blocks by group id) is held against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lifcal_amd
import oracle
from lifcal_amd import BundleAdjustment, _capi as capi, scene
from tests.helpers import S, problem, scaled_max_err, vec_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = "30, 300, 8, 0xF06, 1221, outlier_fraction=0.02"
CONSTRAINED = "30, 300, 8, 0xF06, 1221, outlier_fraction=0.02, n_constraints=3"

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import lifcal_amd
from lifcal_amd import BundleAdjustment, _capi as capi, scene
from tests.helpers import S
sc = scene.make_scene(S(%s))
pa = capi.ProblemArrays.from_scene(sc)
st = lifcal_amd.plan_stats(pa)
if %d:
    assert st.pass_lanes == 256, st.pass_lanes   # the plan of the default kernel, k_sweep3 with four waves per role
    assert st.violations == 0 and st.n_points_permuted > 0 and st.n_blocks >= 2 and st.max_block_passes >= 2, (st.violations, st.n_points_permuted, st.n_blocks, st.max_block_passes)
with BundleAdjustment(pa) as ba:
    r = ba.sweep(123.0, want_matrices=True)
    info = ba.info()
np.savez(sys.argv[1], S=r.S, rhs=r.rhs, cost=r.cost, pg=r.point_gradient, ui=r.point_hessian_inv, chunks=info.n_chunks, moved=st.n_points_permuted)
"""


def run_child(out_dir, spec_args, env_extra, tag, balanced):
    out = os.path.join(str(out_dir), tag + ".npz")
    env = dict(os.environ); env.update(env_extra)
    env.pop("LIFCAL_PLAN_BALANCE", None)
    subprocess.check_call([sys.executable, "-c", _CHILD % (ROOT, spec_args, 1 if balanced else 0), out], env=env, cwd=ROOT)
    return np.load(out)


@pytest.fixture(scope="module")
def atomic_reference(built, tmp_path_factory):
    """the sweep of each scene on the global-atomic kernels, computed once"""
    d = tmp_path_factory.mktemp("plan_balance_ref")
    return {spec: run_child(d, spec, {"LIFCAL_DISABLE_V2": "1"}, "ref%d" % k, False) for k, spec in enumerate((PLAIN, CONSTRAINED))}


@pytest.mark.parametrize("spec_args,env", [
    (PLAIN, {"LIFCAL_V2_BLOCKS": "3"}),
    (CONSTRAINED, {"LIFCAL_V2_BLOCKS": "3"}),
], ids=["three_blocks", "three_blocks_constraints"])
def test_sweep_on_the_balanced_plan_equals_the_atomic_path(built, tmp_path, atomic_reference, spec_args, env):
    a = run_child(tmp_path, spec_args, env, "bal", True)
    b = atomic_reference[spec_args]
    assert int(a["chunks"]) >= 2 and int(b["chunks"]) == 0 and int(a["moved"]) > 0
    cost = abs(float(a["cost"]) - float(b["cost"])) / float(b["cost"])
    errs = (scaled_max_err(a["S"], b["S"]), vec_err(a["rhs"], b["rhs"]), vec_err(a["pg"], b["pg"]), vec_err(a["ui"], b["ui"]))
    print("cost %.2e S %.2e rhs %.2e point gradients %.2e U^-1 %.2e" % ((cost,) + errs))
    assert cost <= 1e-13
    assert errs[0] < 1e-10 and errs[1] < 1e-10
    assert errs[2] < 1e-11 and errs[3] < 1e-10


@pytest.mark.parametrize("spec", [S(30, 300, 8, 0xF06, 1221, outlier_fraction=0.02), S(30, 300, 8, 0xF06, 1221, outlier_fraction=0.02, n_constraints=3)],
                         ids=["three_blocks", "three_blocks_constraints"])
def test_solve_on_the_balanced_plan_follows_the_oracle(built, monkeypatch, spec):
    monkeypatch.delenv("LIFCAL_PLAN_BALANCE", raising=False)
    monkeypatch.setenv("LIFCAL_V2_BLOCKS", "3")
    sc = scene.make_scene(spec)
    pa, pb = problem(sc), problem(sc)
    assert lifcal_amd.plan_stats(pa).n_points_permuted > 0
    with BundleAdjustment(pa) as ba:
        s = ba.performBundleAdjustment()
        st = ba.calcReprojectionError()
    so = oracle.solve(pb, threads=4)
    assert (s.iterations, s.termination) == (so.iterations, so.termination)
    assert abs(s.final_cost - so.final_cost) <= 1e-8 * so.final_cost
    so_st = oracle.reproj_stats(pa)
    assert abs(st.std_x - so_st.std_x) < 1e-10 and abs(st.std_y - so_st.std_y) < 1e-10
    assert abs(st.mae_x - so_st.mae_x) < 1e-9 and abs(st.mae_y - so_st.mae_y) < 1e-9


def test_ordered_sweeps_on_the_balanced_plan_are_bitwise_equal(built, monkeypatch):
    """options.deterministic = 1: two handles on the balanced plan give the same bits"""
    monkeypatch.delenv("LIFCAL_PLAN_BALANCE", raising=False)
    monkeypatch.setenv("LIFCAL_V2_BLOCKS", "3")
    sc = scene.make_scene(S(30, 300, 8, 0xF06, 1221, outlier_fraction=0.02))
    assert lifcal_amd.plan_stats(problem(sc)).n_points_permuted > 0
    o = capi.default_options_py(); o.deterministic = 1
    runs = []
    for handle in range(2):
        with BundleAdjustment(problem(sc), o) as ba:
            g = ba.sweep(1e3, want_matrices=True)
            runs.append((np.float64(g.cost), g.S.copy(), g.rhs.copy(), g.gradient_reduced.copy(), g.point_gradient.copy(), g.point_hessian_inv.copy()))
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
