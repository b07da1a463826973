"""k_sweep3 with evaluator wave 0's chain between barriers P2 and P4 re-ordered (profiles/sweep_factor_chain/): the
point factor is cut in two around publish(factor_done) — the head writes L^-1 and the rhs column of Z, the tail (point index, U^-1, lam,
g, the bad-U count and max |g|) runs from registers behind the publish, with the count and the maximum reduced over the wave to ONE LDS
atomic each — and wave 0 works on its frame-level values while it waits for the other evaluator waves, looking at eval_done without
blocking and factoring at the first look that finds it complete.  What that can break: passes of ONE point (the tail and the wave
reductions run on one lane, 63 lanes carry the neutral element), passes of 64 (the reductions run over a full wave), blocks of several
passes (the counters stay monotone), lanes of one point spread over waves, frames held constant, two evaluator waves (the look with
WR = 2), the fp32 evaluation, and the ordered emission of options.deterministic (which keeps its order and its bits).  The scenes and
cuts are those of tests/test_gpu_sweep_loads.py, the reference is the global-atomic path (LIFCAL_DISABLE_V2) in child processes, the
bars are that file's (check_fp64_sweep).  gradient_max_norm — the reduced max |g| — equals the atomic path's to 1e-10 relative in every
fp64 case.  options.precision = 1 exists on k_sweep3 only, so its reference is the fp64 atomic path and its bars are the fp32 ones of
tests/test_gpu_sweep_loads.py; gradient_max_norm is held to the bar of the gradients there (2e-4).
A failed factorisation of a damped U (bad-U count non-zero, the point's rows of Z zero) is NOT tested here: no scene of the suite
produces one, and the count is not handed to the caller of a sweep."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.helpers import scaled_max_err, vec_err
from tests.test_gpu_sweep_loads import CONSTRAINED, CUTS, FEW_FRAMES, PLAIN, check_fp64_sweep

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXED = (3, 4)   # two neighbouring frames of the 30: both inside the frame window of a block, whichever way the scene is cut
THREE = ("w3", "w300", "few1")

_CHILD = r"""
import json, sys, numpy as np
cfg = json.loads(sys.argv[2])
sys.path.insert(0, cfg["root"])
import lifcal_amd
from lifcal_amd import BundleAdjustment, _capi as capi, scene
from tests.helpers import S
sc = scene.make_scene(eval("S(%s)" % cfg["spec"], {"S": S}))
st = lifcal_amd.plan_stats(capi.ProblemArrays.from_scene(sc))
def options(**kw):
    o = capi.default_options_py(); o.precision = cfg["precision"]; o.deterministic = cfg["deterministic"]
    for k, v in kw.items(): setattr(o, k, v)
    return o
out = {}
with BundleAdjustment(capi.ProblemArrays.from_scene(sc), options()) as ba:
    if cfg["fixed"]:
        m = np.zeros(ba.problem.struct.n_frames, np.uint8); m[cfg["fixed"]] = 1
        ba.set_fixed_frames(m)
    for k in ("", "2", "3"):
        r = ba.sweep(123.0, want_matrices=True)
        out.update({"S" + k: r.S, "rhs" + k: r.rhs, "cost" + k: r.cost, "pg" + k: r.point_gradient, "ui" + k: r.point_hessian_inv,
                    "gr" + k: r.gradient_reduced, "gmax" + k: r.gradient_max_norm})
if cfg["step"]:
    pa = capi.ProblemArrays.from_scene(sc)
    with BundleAdjustment(pa, options(max_iterations=1)) as ba:
        s = ba.performBundleAdjustment()
    out.update(pts=pa.pts, views=pa.views, pts0=sc.pts0, steps=s.successful_steps)
np.savez(sys.argv[1], blocks=st.n_blocks, passes=st.n_passes, lanes=st.pass_lanes, n_lanes=st.n_lanes, violations=st.violations, **out)
"""


def run_child(out_dir, spec, env_extra, tag, precision=0, deterministic=0, fixed=(), step=False):
    out = os.path.join(str(out_dir), tag + ".npz")
    env = dict(os.environ); env.update(env_extra)
    for k in ("LIFCAL_PLAN_BALANCE", "LIFCAL_SWEEP_KERNEL"):
        env.pop(k, None)
    cfg = dict(root=ROOT, spec=spec, precision=precision, deterministic=deterministic, fixed=list(fixed), step=step)
    subprocess.check_call([sys.executable, "-c", _CHILD, out, json.dumps(cfg)], env=env, cwd=ROOT)
    return np.load(out)


def cut_env(cut, **extra):
    env = {"LIFCAL_V2_BLOCKS": str(CUTS[cut][1])}
    env.update(extra)
    return env


def check_gmax(a, b, bar=1e-10):
    """the reduced max |g| (with the frame and camera gradients' maxima: gradient_max_norm) against the reference's"""
    ga, gb = float(a["gmax"]), float(b["gmax"])
    err = abs(ga - gb) / gb
    print("gradient_max_norm %.17g against %.17g: %.2e" % (ga, gb, err))
    assert gb > 0 and err <= bar


def check_sweep(a, b):
    check_fp64_sweep(a, b)
    check_gmax(a, b)


@pytest.fixture(scope="module")
def atomic_reference(built, tmp_path_factory):
    """sweeps and one LM step of each scene on the global-atomic kernels (fp64), computed once"""
    d = tmp_path_factory.mktemp("sweep_factor_chain_ref")
    ref = {spec: run_child(d, spec, {"LIFCAL_DISABLE_V2": "1"}, "ref%d" % k, step=True) for k, spec in enumerate((PLAIN, CONSTRAINED, FEW_FRAMES))}
    ref["fixed"] = run_child(d, PLAIN, {"LIFCAL_DISABLE_V2": "1"}, "ref_fixed", fixed=FIXED)
    return ref


@pytest.fixture(scope="module")
def window_runs(built, tmp_path_factory):
    """the three cuts on k_sweep3 (fp64, four waves per role): three sweeps on one handle and one LM step, computed once"""
    d = tmp_path_factory.mktemp("sweep_factor_chain_win")
    return {cut: run_child(d, CUTS[cut][0], cut_env(cut), cut, step=True) for cut in THREE}


@pytest.mark.parametrize("cut", THREE)
def test_sweep_equals_the_atomic_path(window_runs, atomic_reference, cut):
    a = window_runs[cut]
    assert int(a["blocks"]) == CUTS[cut][2] and int(a["violations"]) == 0 and int(a["lanes"]) == 256
    check_sweep(a, atomic_reference[CUTS[cut][0]])


def test_split_groups_across_waves_equal_the_atomic_path(tmp_path, window_runs, atomic_reference):
    """LIFCAL_GROUP_SPLIT=2: the lanes of one point sit in several waves, so wave 0 factors points whose U other waves emitted"""
    a = run_child(tmp_path, PLAIN, cut_env("w3", LIFCAL_GROUP_SPLIT="2"), "split")
    assert int(a["n_lanes"]) > int(window_runs["w3"]["n_lanes"]) and int(a["violations"]) == 0
    check_sweep(a, atomic_reference[PLAIN])


def test_sweep_with_constraints_equals_the_atomic_path(tmp_path, atomic_reference):
    a = run_child(tmp_path, CONSTRAINED, cut_env("w3"), "con")
    assert int(a["blocks"]) >= 3
    check_sweep(a, atomic_reference[CONSTRAINED])


def test_sweep_with_two_fixed_frames_equals_the_atomic_path(tmp_path, atomic_reference):
    """lanes of a frame held constant head no run: wave 0 still takes its looks, the factor and the rest of its round B"""
    a, b = run_child(tmp_path, PLAIN, cut_env("w3"), "fixed", fixed=FIXED), atomic_reference["fixed"]
    for f in FIXED:   # identity rows, zero right-hand side: the pose is not a column of the problem (and the mask reached the reference)
        blk = slice(17 + 6 * f, 17 + 6 * f + 6)
        assert np.array_equal(a["S"][blk, blk], np.eye(6)) and np.all(a["rhs"][blk] == 0) and np.array_equal(b["S"][blk, blk], np.eye(6))
    assert np.any(b["S"] != atomic_reference[PLAIN]["S"])
    check_sweep(a, b)


@pytest.mark.parametrize("cut", THREE)
def test_sweep_with_two_waves_per_role_equals_the_atomic_path(tmp_path, atomic_reference, cut):
    """LIFCAL_SWEEP_WAVES=2: wave 0 looks at a counter that ONE other wave completes"""
    a = run_child(tmp_path, CUTS[cut][0], cut_env(cut, LIFCAL_SWEEP_WAVES="2"), "w2")
    assert int(a["lanes"]) == 128
    check_sweep(a, atomic_reference[CUTS[cut][0]])


@pytest.mark.parametrize("cut", THREE)
def test_fp32_evaluation_sweep_equals_its_fp64_arm(tmp_path, atomic_reference, cut):
    """options.precision = 1 against the fp64 sweep of the scene, at the bars of tests/test_gpu_sweep_loads.py"""
    a, b = run_child(tmp_path, CUTS[cut][0], cut_env(cut), "f32", precision=1), atomic_reference[CUTS[cut][0]]
    assert int(a["blocks"]) == CUTS[cut][2]
    cost = abs(float(a["cost"]) - float(b["cost"])) / float(b["cost"])
    errs = (scaled_max_err(a["S"], b["S"]), vec_err(a["rhs"], b["rhs"]), vec_err(a["gr"], b["gr"]))
    print("cost %.2e S %.2e rhs %.2e reduced gradient %.2e" % ((cost,) + errs))
    assert cost <= 2e-6
    assert errs[0] < 2e-5 and errs[1] < 2e-4 and errs[2] < 2e-4
    check_gmax(a, b, bar=2e-4)


@pytest.mark.parametrize("cut,split", [("w3", 0), ("w3", 2), ("w300", 0), ("few1", 0)])
def test_deterministic_sweep_is_bitwise_repeatable_and_equals_the_atomic_path(tmp_path, atomic_reference, cut, split):
    env = cut_env(cut, **({"LIFCAL_GROUP_SPLIT": str(split)} if split else {}))
    a = run_child(tmp_path, CUTS[cut][0], env, "det_a", deterministic=1)
    b = run_child(tmp_path, CUTS[cut][0], env, "det_b", deterministic=1)
    for k in ("S", "rhs", "cost", "pg", "ui", "gr", "gmax", "S3", "rhs3", "cost3", "gmax3"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("S", "rhs", "cost", "pg", "ui", "gr", "gmax"):
        assert np.array_equal(a[k], a[k + "3"]), k   # and the third sweep of a handle equals its first
    check_sweep(a, atomic_reference[CUTS[cut][0]])


@pytest.mark.parametrize("cut", THREE)
def test_third_sweep_on_one_handle_equals_the_first(window_runs, cut):
    """at the bar profiles/sweep_zfused/ measured it at (1e-12)"""
    a = window_runs[cut]
    for k in ("2", "3"):
        cost = abs(float(a["cost" + k]) - float(a["cost"])) / float(a["cost"])
        errs = (scaled_max_err(a["S" + k], a["S"]), vec_err(a["rhs" + k], a["rhs"]))
        print("sweep %s: cost %.2e S %.2e rhs %.2e" % ((k, cost) + errs))
        assert cost <= 1e-12 and errs[0] <= 1e-12 and errs[1] <= 1e-12
        assert abs(float(a["gmax" + k]) - float(a["gmax"])) <= 1e-12 * float(a["gmax"])


@pytest.mark.parametrize("cut", THREE)
def test_one_lm_step_equals_the_atomic_path(window_runs, atomic_reference, cut):
    a, b = window_runs[cut], atomic_reference[CUTS[cut][0]]
    assert int(a["steps"]) == 1 and int(b["steps"]) == 1 and np.any(b["pts"] != b["pts0"])
    errs = (vec_err(a["pts"], b["pts"]), vec_err(a["views"], b["views"]))
    print("points %.2e poses %.2e" % errs)
    assert errs[0] <= 1e-10 and errs[1] <= 1e-10
