"""The hot rows of k_sweep3: the ~75 words every block adds to (camera x camera block, camera entries of hdiag / gB /
rhsacc, cost, max |g_p|) go to row `block % HOT_ROWS` of the copy of the reduced block, and are folded onto the canonical words by
k_finalize (no exchange) or by k_fold_hot (in front of an exchange, behind a trial sweep of the line search).  What can go wrong depends
on how the blocks fall on the rows, so the scene of tests/test_gpu_sweep_tail.py (300 points over 30 frames) is cut into 3 blocks, 20
blocks and 38 blocks (LIFCAL_V2_BLOCKS=40).  With the 8 rows the library is built with (kernels.hpp: HOT_ROWS, chosen by measurement,
profiles/sweep_hot_rows/) that is: 5 rows stay zero; rows 0-3 are shared by three blocks and rows 4-7 by two; rows 0-5 by five blocks
and rows 6-7 by four.  (With 16 rows: 13 rows stay zero; rows 0-3 shared by two blocks; up to three blocks per row.)  Also with
distance constraints, whose kernels add to the canonical words beside the rows.  The reference of the sweeps is the global-atomic path
(LIFCAL_DISABLE_V2), which has neither rows nor fold."""
import os
import subprocess
import sys

import numpy as np
import pytest

import lifcal_amd
import oracle
from lifcal_amd import BundleAdjustment, scene
from tests.helpers import S, bounded_problem, scaled_max_err, vec_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PLAIN = "30, 300, 8, 0xF06, 1221, outlier_fraction=0.02"
CONSTRAINED = "30, 300, 8, 0xF06, 1221, outlier_fraction=0.02, n_constraints=3"
BLOCKS = {3: 3, 20: 20, 40: 38}   # LIFCAL_V2_BLOCKS -> blocks of the plan (plan_stats, checked on the CPU)

_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import lifcal_amd
from lifcal_amd import BundleAdjustment, _capi as capi, scene, comm_unique_id
from tests.helpers import S
sc = scene.make_scene(S(%s))
precision, rccl = %d, %d
st = lifcal_amd.plan_stats(capi.ProblemArrays.from_scene(sc))
o = capi.default_options_py(); o.precision = precision
with BundleAdjustment(capi.ProblemArrays.from_scene(sc), o) as ba:
    if rccl:
        ba.comm_init_rccl(comm_unique_id())
    r = ba.sweep(123.0, want_matrices=True)
    r2 = ba.sweep(123.0, want_matrices=True)     # the other copy of the reduced block, zero-filled by the first sweep's k_finalize
    r3 = ba.sweep(123.0, want_matrices=True)     # the first copy again, after its rows held values
    chunks = ba.info().n_chunks
gather_calls, Sh, rhsh, costh = 0, r.S, r.rhs, r.cost
if rccl:
    # the same forced exchange through counting hooks (an all-gather among one rank is a copy): whether a handle packs slabs depends on
    # the problem alone, so a gather call per sweep here says that the RCCL handle above went through pack / all-gather / unpack too
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    calls = {"gather": 0}
    def hook(ptr, count, stream):
        return 0
    def ghook(send, recv, count, stream):
        hip.hipStreamSynchronize(stream)
        hip.hipMemcpy(recv, send, count * 8, 3)
        hip.hipDeviceSynchronize()   # (a device-to-device hipMemcpy may return before it is done, and the library's stream does not wait for the null stream)
        calls["gather"] += 1
        return 0
    with BundleAdjustment(capi.ProblemArrays.from_scene(sc), o) as ba:
        ba.set_allreduce(hook); ba.set_allgather(ghook)
        rh = ba.sweep(123.0, want_matrices=True)
        gather_calls, Sh, rhsh, costh = calls["gather"], rh.S, rh.rhs, rh.cost
o = capi.default_options_py(); o.precision = precision; o.max_iterations = 1
pa = capi.ProblemArrays.from_scene(sc)
with BundleAdjustment(pa, o) as ba:
    s = ba.performBundleAdjustment()
np.savez(sys.argv[1], S=r.S, rhs=r.rhs, cost=r.cost, gmax=r.gradient_max_norm, gather_calls=gather_calls, Sh=Sh, rhsh=rhsh, costh=costh, pg=r.point_gradient, ui=r.point_hessian_inv, gr=r.gradient_reduced,
         S2=r2.S, cost2=r2.cost, rhs2=r2.rhs, S3=r3.S, cost3=r3.cost, rhs3=r3.rhs, chunks=chunks, blocks=st.n_blocks, lanes=st.pass_lanes,
         pts=pa.pts, views=pa.views, pts0=sc.pts0, steps=s.successful_steps)
"""


def run_child(out_dir, spec_args, env_extra, tag, precision=0, rccl=0):
    out = os.path.join(str(out_dir), tag + ".npz")
    env = dict(os.environ); env.update(env_extra)
    for k in ("LIFCAL_PLAN_BALANCE", "LIFCAL_SWEEP_KERNEL"):
        env.pop(k, None)
    subprocess.check_call([sys.executable, "-c", _CHILD % (ROOT, spec_args, precision, rccl), out], env=env, cwd=ROOT)
    return np.load(out)


@pytest.fixture(scope="module")
def atomic_reference(built, tmp_path_factory):
    """sweep and one LM step of each scene on the global-atomic kernels (fp64), computed once"""
    d = tmp_path_factory.mktemp("hot_rows_ref")
    return {spec: run_child(d, spec, {"LIFCAL_DISABLE_V2": "1"}, "ref%d" % k) for k, spec in enumerate((PLAIN, CONSTRAINED))}


@pytest.fixture(scope="module")
def plain_20_blocks(built, tmp_path_factory):
    """the plain scene on k_sweep3 with 20 blocks (default kernel), computed once for the tests that share it"""
    return run_child(tmp_path_factory.mktemp("hot_rows_win"), PLAIN, {"LIFCAL_V2_BLOCKS": "20"}, "win20")


def check_fp64_sweep(a, b):
    cost = abs(float(a["cost"]) - float(b["cost"])) / float(b["cost"])
    errs = (scaled_max_err(a["S"], b["S"]), vec_err(a["rhs"], b["rhs"]), vec_err(a["pg"], b["pg"]), vec_err(a["ui"], b["ui"]))
    # max |g|: the larger of max |g_p| (the last word of a row, folded by a max of its own) and the reduced gradient's maximum; as a
    # maximum of entries that meet the bars above (point gradients 1e-11, rhs 1e-10 of their largest entry) it meets the weaker one
    gmax = abs(float(a["gmax"]) - float(b["gmax"])) / float(b["gmax"])
    print("cost %.2e S %.2e rhs %.2e point gradients %.2e U^-1 %.2e max |g| %.2e (%.6e, max |g_p| %.6e)" % ((cost,) + errs + (gmax, float(a["gmax"]), float(np.max(np.abs(a["pg"]))))))
    assert cost <= 1e-13
    assert errs[0] < 1e-10 and errs[1] < 1e-10
    assert errs[2] < 1e-11 and errs[3] < 1e-10
    assert gmax <= 1e-10


@pytest.mark.parametrize("spec_args", [PLAIN, CONSTRAINED], ids=["plain", "constraints"])
@pytest.mark.parametrize("v2_blocks", sorted(BLOCKS))
def test_sweep_equals_the_atomic_path(tmp_path, plain_20_blocks, atomic_reference, v2_blocks, spec_args):
    a = plain_20_blocks if (v2_blocks == 20 and spec_args == PLAIN) else run_child(tmp_path, spec_args, {"LIFCAL_V2_BLOCKS": str(v2_blocks)}, "win")
    b = atomic_reference[spec_args]
    assert int(a["blocks"]) == BLOCKS[v2_blocks] and int(a["chunks"]) >= 2 and int(b["chunks"]) == 0 and int(a["lanes"]) == 256
    check_fp64_sweep(a, b)


def test_sweep_with_two_waves_per_role_equals_the_atomic_path(tmp_path, atomic_reference):
    a = run_child(tmp_path, PLAIN, {"LIFCAL_V2_BLOCKS": "20", "LIFCAL_SWEEP_WAVES": "2"}, "w2")
    assert int(a["blocks"]) == 20 and int(a["lanes"]) == 128
    check_fp64_sweep(a, atomic_reference[PLAIN])


def test_fp32_evaluation_sweep_equals_its_fp64_arm(tmp_path, atomic_reference):
    """options.precision = 1 against the fp64 sweep of the scene, at the bars of tests/test_gpu_sweep_tail.py"""
    a, b = run_child(tmp_path, PLAIN, {"LIFCAL_V2_BLOCKS": "20"}, "f32", precision=1), atomic_reference[PLAIN]
    assert int(a["blocks"]) == 20
    cost = abs(float(a["cost"]) - float(b["cost"])) / float(b["cost"])
    errs = (scaled_max_err(a["S"], b["S"]), vec_err(a["rhs"], b["rhs"]), vec_err(a["gr"], b["gr"]))
    print("cost %.2e S %.2e rhs %.2e reduced gradient %.2e" % ((cost,) + errs))
    assert cost <= 2e-6
    assert errs[0] < 2e-5 and errs[1] < 2e-4 and errs[2] < 2e-4


def test_three_sweeps_in_a_row_on_one_handle_are_equal(plain_20_blocks):
    """the third sweep accumulates into the copy whose rows the first one filled and the second one's k_finalize zero-filled"""
    a = plain_20_blocks
    for k in ("2", "3"):
        cost = abs(float(a["cost" + k]) - float(a["cost"])) / float(a["cost"])
        errs = (scaled_max_err(a["S" + k], a["S"]), vec_err(a["rhs" + k], a["rhs"]))
        print("sweep %s: cost %.2e S %.2e rhs %.2e" % ((k, cost) + errs))
        assert cost <= 1e-12 and errs[0] <= 1e-12 and errs[1] <= 1e-12


def test_one_lm_step_equals_the_atomic_path(plain_20_blocks, atomic_reference):
    """solver, back-substitution and the LM kernels read the folded canonical words"""
    a, b = plain_20_blocks, atomic_reference[PLAIN]
    assert int(a["steps"]) == 1 and int(b["steps"]) == 1 and np.any(b["pts"] != b["pts0"])
    errs = (vec_err(a["pts"], b["pts"]), vec_err(a["views"], b["views"]))
    print("points %.2e poses %.2e" % errs)
    assert errs[0] <= 1e-10 and errs[1] <= 1e-10


def test_sweep_through_the_exchange_equals_the_sweep_without(tmp_path, plain_20_blocks):
    """LIFCAL_FORCE_EXCHANGE on a library RCCL communicator: k_fold_hot in front of pack / all-gather / unpack, k_finalize does not fold"""
    a, b = run_child(tmp_path, PLAIN, {"LIFCAL_V2_BLOCKS": "20", "LIFCAL_FORCE_EXCHANGE": "1"}, "xch", rccl=1), plain_20_blocks
    assert int(a["blocks"]) == 20
    assert int(a["gather_calls"]) == 1   # the problem packs slabs: the forced exchange is pack / all-gather / unpack, not the (empty) all-reduce
    for S_, rhs_, cost_, arm in ((a["S"], a["rhs"], a["cost"], "RCCL"), (a["Sh"], a["rhsh"], a["costh"], "hooks")):
        cost = abs(float(cost_) - float(b["cost"])) / float(b["cost"])
        errs = (scaled_max_err(S_, b["S"]), vec_err(rhs_, b["rhs"]))
        print("%s: cost %.2e S %.2e rhs %.2e" % ((arm, cost) + errs))
        assert cost <= 1e-12 and errs[0] <= 1e-9 and errs[1] <= 1e-9


def test_bounded_pose_point_problem_on_20_blocks_matches_oracle(built, monkeypatch):
    """the trial sweeps of the line search (eval_trial: block kernels -> k_fold_hot -> k_dirderiv, no k_finalize) on 20 blocks: the
    problem of tests/test_gpu_parity.py::test_bounded_pose_point_problem_matches_oracle on the 30-frame scene, where the oracle's solve
    runs three line searches that backtrack (checked on the CPU with LO_DEBUG_LS=1)"""
    monkeypatch.delenv("LIFCAL_PLAN_BALANCE", raising=False)
    monkeypatch.delenv("LIFCAL_SWEEP_KERNEL", raising=False)
    monkeypatch.setenv("LIFCAL_V2_BLOCKS", "20")
    sc = scene.make_scene(S(30, 300, 8, 0xF06, 1221, outlier_fraction=0.02))
    pa, pb = bounded_problem(sc), bounded_problem(sc)
    assert lifcal_amd.plan_stats(pa).n_blocks >= 17
    with BundleAdjustment(pa) as ba:
        s = ba.performBundleAdjustment()
    so = oracle.solve(pb, threads=4)
    print("iterations %d / %d termination %d / %d final cost %.12e / %.12e" % (s.iterations, so.iterations, s.termination, so.termination, s.final_cost, so.final_cost))
    assert (s.iterations, s.termination) == (so.iterations, so.termination)
    assert abs(s.final_cost - so.final_cost) <= 1e-8 * so.final_cost
