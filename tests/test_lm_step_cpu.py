"""The trust-region rules of lifcal_amd/csrc/lm_step.hpp, compiled as plain C++ (no HIP) behind a C shim and driven with hand-made
scalars.  The host loop of lifcal_ba_solve and k_lm_control both call these functions, so what holds here holds on both routes.
Expected values are computed here from the rules of ceres 2.1 and compared with ==.

The accepted radius is r / max(1/3, 1 - (2 rho - 1)^3) with three multiplications, 2 rho, t t and (t t) t, the last of them fused with
the subtraction from 1 (one rounding): the header spells the fused multiply-add out because that is what the device compiler has always
made of the expression.  fma_1_minus() below evaluates the same thing in exact rational arithmetic and rounds once."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["RADIUS", "DECREASE", "X_COST", "GMAX", "ITER", "INVALID", "STEP_OK", "SUCCESSFUL", "UNSUCCESSFUL", "TERMINATION", "COMMIT", "INITIAL_COST", "N"]
FUNCTION_TOLERANCE, PARAMETER_TOLERANCE, GRADIENT_TOLERANCE, MAX_ITERATIONS, MIN_RADIUS, INVALID_STEPS = 1, 2, 3, 4, 5, 6   # include/lifcal_ba.h

SHIM = r"""
#include "lm_step.hpp"
using namespace lifcal;
extern "C" {
int shim_index(int k) { static const int idx[] = {%s}; return idx[k]; }
void shim_reset(double* lm, double radius) { lm_reset(lm, radius); }
void shim_take_sweep(double* lm, const LmOpts* o, double cost, double gmax, double bad) { lm_take_sweep(lm, *o, cost, gmax, bad); }
int shim_open_iteration(double* lm, const LmOpts* o) { return lm_open_iteration(lm, *o) ? 1 : 0; }
int shim_check_step(double* lm, double gtd, double ddd, double chol_fail) { return lm_check_step(lm, gtd, ddd, chol_fail) ? 1 : 0; }
void shim_judge_step(double* lm, const LmOpts* o, double cand_cost, double step2, double x2) { lm_judge_step(lm, *o, cand_cost, step2, x2); }
}
""" % ", ".join("LM_" + n for n in NAMES)


class LmOpts(C.Structure):
    _fields_ = [("f_tol", C.c_double), ("p_tol", C.c_double), ("g_tol", C.c_double), ("min_rel_decrease", C.c_double),
                ("max_radius", C.c_double), ("min_radius", C.c_double), ("max_iterations", C.c_int)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the header must compile without hipcc")
    d = tmp_path_factory.mktemp("lm_step")
    src, lib = os.path.join(str(d), "shim.cpp"), os.path.join(str(d), "liblm_step_shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror", "-I", os.path.join(ROOT, "lifcal_amd", "csrc"), "-o", lib, src])
    so = C.CDLL(lib)
    dp, op = C.POINTER(C.c_double), C.POINTER(LmOpts)
    so.shim_index.argtypes = [C.c_int]
    so.shim_reset.argtypes = [dp, C.c_double]; so.shim_reset.restype = None
    so.shim_take_sweep.argtypes = [dp, op, C.c_double, C.c_double, C.c_double]; so.shim_take_sweep.restype = None
    so.shim_open_iteration.argtypes = [dp, op]
    so.shim_check_step.argtypes = [dp, C.c_double, C.c_double, C.c_double]
    so.shim_judge_step.argtypes = [dp, op, C.c_double, C.c_double, C.c_double]; so.shim_judge_step.restype = None
    return so


R0 = 1e4


class Loop:
    """one solve's state; x_cost 100, gradient norm 1 unless told otherwise"""

    def __init__(self, so, cost=100.0, gmax=1.0, bad=0.0, **opts):
        self.so = so
        self.ix = {n: so.shim_index(k) for k, n in enumerate(NAMES)}
        o = dict(f_tol=1e-6, p_tol=1e-8, g_tol=1e-10, min_rel_decrease=1e-3, max_radius=1e16, min_radius=1e-32, max_iterations=200)
        o.update(opts)
        self.o = LmOpts(**o)
        self.lm = (C.c_double * self.ix["N"])()
        so.shim_reset(self.lm, R0)
        self.take_sweep(cost, gmax, bad)

    def __getitem__(self, name):
        return self.lm[self.ix[name]]

    def __setitem__(self, name, v):
        self.lm[self.ix[name]] = v

    def take_sweep(self, cost, gmax=1.0, bad=0.0):
        self.so.shim_take_sweep(self.lm, C.byref(self.o), cost, gmax, bad)

    def open(self):
        return bool(self.so.shim_open_iteration(self.lm, C.byref(self.o)))

    def check(self, gtd=-30.0, ddd=10.0, chol_fail=0.0):   # model cost change 0.5 * (10 + 30) = 20
        return bool(self.so.shim_check_step(self.lm, gtd, ddd, chol_fail))

    def judge(self, cand_cost, step2=1.0, x2=100.0):
        self.so.shim_judge_step(self.lm, C.byref(self.o), cand_cost, step2, x2)

    def step(self, cand_cost, **kw):
        """one whole iteration with a valid step; an accepted candidate is taken in as the next point"""
        assert self.open() and self.check()
        self.judge(cand_cost, **kw)
        if self["COMMIT"] != 0.0:
            self.take_sweep(cand_cost)

    def counts(self):
        return (self["ITER"], self["SUCCESSFUL"], self["UNSUCCESSFUL"], self["TERMINATION"])


def fma_1_minus(tt, t):
    """1 - tt * t, rounded once"""
    return float(1 - Fraction(tt) * Fraction(t))


def accepted_radius(r, x_cost, cand_cost, model_change, max_radius):
    rho = (x_cost - cand_cost) / model_change
    t = 2.0 * rho - 1.0
    return min(max_radius, r / max(1.0 / 3.0, fma_1_minus(t * t, t)))


def test_initial_gradient_tolerance_ends_the_solve_at_iteration_0(shim):
    L = Loop(shim, gmax=1e-10)   # g_tol = 1e-10, "<="
    assert L.counts() == (0.0, 0.0, 0.0, GRADIENT_TOLERANCE)
    assert L["INITIAL_COST"] == 100.0 and L["X_COST"] == 100.0 and L["RADIUS"] == R0
    L = Loop(shim, gmax=1.0000001e-10)
    assert L["TERMINATION"] == 0.0 and L.open() and L["ITER"] == 1.0


def test_non_finite_initial_cost_is_an_error_state(shim):
    for c in (math.inf, math.nan):
        L = Loop(shim, cost=c, gmax=0.0)   # (reported before the gradient test)
        assert L["TERMINATION"] == -1.0 and L["ITER"] == 0.0


def test_gradient_tolerance_is_tested_only_after_a_successful_step(shim):
    L = Loop(shim)
    L.step(150.0)                                  # rejected: the point, and so its gradient, is the old one
    assert L.counts() == (1.0, 0.0, 1.0, 0.0) and L["STEP_OK"] == 0.0
    L["GMAX"] = 1e-12                              # hand-made: below the tolerance, behind an unsuccessful step
    assert L.open() and L["TERMINATION"] == 0.0 and L["ITER"] == 2.0
    assert L.check()
    L.judge(90.0)
    assert L["COMMIT"] == 1.0 and L["STEP_OK"] == 1.0
    L.take_sweep(90.0, gmax=1e-12)                 # not the first sweep: no test inside
    assert L["TERMINATION"] == 0.0
    assert not L.open()
    assert L.counts() == (2.0, 1.0, 1.0, GRADIENT_TOLERANCE)


@pytest.mark.parametrize("why", ["chol_fail", "bad_point_block", "model_increase", "model_zero", "model_nan", "model_inf"])
def test_five_invalid_steps_in_a_row_terminate_and_each_earlier_one_halves_the_radius(shim, why):
    L = Loop(shim, bad=1.0 if why == "bad_point_block" else 0.0)   # (the flag of the sweep invalidates the first step, see below)
    r = R0
    for k in range(5):
        assert L.open()
        kw = {"chol_fail": dict(chol_fail=1.0), "bad_point_block": dict(chol_fail=0.0 if k == 0 else 1.0), "model_increase": dict(gtd=10.0, ddd=5.0),
              "model_zero": dict(gtd=10.0, ddd=10.0), "model_nan": dict(gtd=math.nan), "model_inf": dict(gtd=-math.inf)}[why]
        assert not L.check(**kw)
        if k < 4:
            r = r * 0.5
            assert L.counts() == (k + 1.0, 0.0, k + 1.0, 0.0) and L["RADIUS"] == r and L["INVALID"] == k + 1.0 and L["STEP_OK"] == 0.0
    assert L["TERMINATION"] == INVALID_STEPS and L["RADIUS"] == R0 / 16 and L["ITER"] == 5.0 and L["UNSUCCESSFUL"] == 4.0


def test_the_flag_of_a_fresh_sweep_counts_once(shim):
    """a point block that was not positive definite invalidates the step computed from THAT sweep; the re-sweep at the halved radius
    is not taken in, the next step is judged on its own"""
    L = Loop(shim, bad=1.0)
    assert L.open() and not L.check()
    assert L["RADIUS"] == R0 / 2 and L["INVALID"] == 1.0
    assert L.open() and L.check() and L["INVALID"] == 0.0


def test_one_valid_step_resets_the_invalid_counter(shim):
    L = Loop(shim)
    for _ in range(4):
        assert L.open() and not L.check(chol_fail=1.0)
    assert L["INVALID"] == 4.0
    assert L.open() and L.check() and L["INVALID"] == 0.0
    L.judge(150.0)
    for k in range(4):
        assert L.open() and not L.check(chol_fail=1.0)
        assert L["TERMINATION"] == 0.0 and L["INVALID"] == k + 1.0
    assert L.open() and not L.check(chol_fail=1.0)
    assert L["TERMINATION"] == INVALID_STEPS


def test_rejected_steps_divide_the_radius_by_2_4_8_and_an_accepted_step_resets_the_divisor(shim):
    L = Loop(shim)
    r = R0
    for k, div in enumerate((2.0, 4.0, 8.0, 16.0)):
        L.step(100.0 + 1.0 + k)                    # cost goes up: rho < 0
        r = r / div
        assert L["RADIUS"] == r and L["COMMIT"] == 0.0 and L["X_COST"] == 100.0
        assert L.counts() == (k + 1.0, 0.0, k + 1.0, 0.0)
    L.step(85.0)                                   # rho = 0.75
    r = accepted_radius(r, 100.0, 85.0, 20.0, 1e16)
    assert L["RADIUS"] == r and L["X_COST"] == 85.0 and L["DECREASE"] == 2.0
    L.step(86.0)
    assert L["RADIUS"] == r / 2.0
    L.step(86.0)
    assert L["RADIUS"] == r / 2.0 / 4.0
    # rho exactly at min_relative_decrease is a rejection (">")
    L2 = Loop(shim, min_rel_decrease=0.25)
    L2.step(95.0)                                  # rho = 5 / 20
    assert L2["COMMIT"] == 0.0 and L2["RADIUS"] == R0 / 2.0 and L2["UNSUCCESSFUL"] == 1.0


@pytest.mark.parametrize("cand_cost", [99.9, 98.7, 97.3, 93.1, 90.0, 86.3, 85.0, 83.9, 82.2, 81.1, 80.0, 77.7, 60.0])
def test_accepted_radius(shim, cand_cost):
    L = Loop(shim)
    L.step(cand_cost)
    want = accepted_radius(R0, 100.0, cand_cost, 20.0, 1e16)
    assert L["COMMIT"] == 1.0 and L.counts() == (1.0, 1.0, 0.0, 0.0)
    assert L["RADIUS"] == want
    assert R0 / 2.0 <= want <= 3.0 * R0 + 1e-9
    # a second accepted step starts from the new radius
    L.step(cand_cost - 10.0)
    assert L["RADIUS"] == accepted_radius(want, cand_cost, cand_cost - 10.0, 20.0, 1e16)


def test_accepted_radius_is_capped_at_max_radius(shim):
    L = Loop(shim, max_radius=2.5 * R0)
    L.step(80.0)                                   # rho = 1: the divisor is 1/3, uncapped 3 r
    assert accepted_radius(R0, 100.0, 80.0, 20.0, 1e16) == R0 / (1.0 / 3.0) > 2.5 * R0
    assert L["RADIUS"] == 2.5 * R0 and L["COMMIT"] == 1.0


def test_parameter_and_function_tolerance_fire_before_rho_is_looked_at(shim):
    # a step too short to matter ends the solve although its cost change would have been a rejection (or an acceptance)
    for cand in (150.0, 85.0, math.inf):
        L = Loop(shim)
        assert L.open() and L.check()
        x2 = 100.0
        L.judge(cand, step2=(1e-8 * (math.sqrt(x2) + 1e-8)) ** 2 * 0.999, x2=x2)
        assert L.counts() == (1.0, 0.0, 0.0, PARAMETER_TOLERANCE) and L["RADIUS"] == R0 and L["COMMIT"] == 0.0
    # |cost change| <= f_tol * cost in EITHER direction ends it: an increase inside the tolerance is not a rejected step
    for cand in (100.0 + 0.9e-4, 100.0 - 0.9e-4, 100.0):
        L = Loop(shim)
        assert L.open() and L.check()
        L.judge(cand)
        assert abs(100.0 - cand) <= 1e-6 * 100.0
        assert L.counts() == (1.0, 0.0, 0.0, FUNCTION_TOLERANCE) and L["RADIUS"] == R0 and L["COMMIT"] == 0.0
    # the parameter tolerance is the first of the two
    L = Loop(shim)
    assert L.open() and L.check()
    L.judge(100.0, step2=0.0)
    assert L["TERMINATION"] == PARAMETER_TOLERANCE
    # just outside both: an ordinary decision
    L = Loop(shim)
    L.step(100.0 + 1.1e-4)
    assert L.counts() == (1.0, 0.0, 1.0, 0.0) and L["RADIUS"] == R0 / 2.0


@pytest.mark.parametrize("cand", [math.inf, math.nan, -math.inf])
def test_a_non_finite_candidate_cost_is_a_rejection_not_a_termination(shim, cand):
    L = Loop(shim)
    L.step(cand)
    assert L.counts() == (1.0, 0.0, 1.0, 0.0) and L["RADIUS"] == R0 / 2.0 and L["COMMIT"] == 0.0 and L["X_COST"] == 100.0


def test_max_iterations_and_min_radius_are_tested_at_the_top_of_an_iteration(shim):
    L = Loop(shim, max_iterations=2)
    L.step(90.0); L.step(150.0)
    assert L.counts() == (2.0, 1.0, 1.0, 0.0)      # the second iteration ran to its end
    assert not L.open()
    assert L.counts() == (2.0, 1.0, 1.0, MAX_ITERATIONS)
    L = Loop(shim, max_iterations=0)
    assert not L.open() and L.counts() == (0.0, 0.0, 0.0, MAX_ITERATIONS)
    L = Loop(shim, min_radius=R0 / 8.0)
    L.step(150.0)                                  # r / 2
    assert L["TERMINATION"] == 0.0
    L.step(150.0)                                  # r / 8: equal to the bound is not below it
    assert L["RADIUS"] == R0 / 8.0 and L["TERMINATION"] == 0.0
    L.step(150.0)                                  # r / 64
    assert L["TERMINATION"] == 0.0 and L["RADIUS"] == R0 / 64.0
    assert not L.open()
    assert L.counts() == (3.0, 0.0, 3.0, MIN_RADIUS)
    # max_iterations is looked at first
    L = Loop(shim, max_iterations=1, min_radius=R0)
    L.step(150.0)
    assert not L.open() and L["TERMINATION"] == MAX_ITERATIONS
