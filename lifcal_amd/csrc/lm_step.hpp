// lm_step.hpp — the trust-region decisions of the Levenberg-Marquardt loop, written once: the host loop of lifcal_ba_solve and
// k_lm_control both call them.  Ceres 2.1 TrustRegionMinimizer / LevenbergMarquardtStrategy, restated.  The procedure works on the
// state array lm[LM_N] and is cut where a caller has work of its own to do:
//   1  lm_take_sweep                      cost / gradient norm of a fresh point, the rules of the very first sweep
//   2  lm_open_iteration, lm_check_step   top-of-iteration tests and ++iter | model cost change and step validity (two calls: the
//                                         host launches the linear solve only behind the first, the device makes them back to back)
//   3  lm_judge_step                      parameter / function tolerance, rho, accept or reject
// Between 2 and 3 the host runs the line search of a bounded problem, which may replace cand_cost, step2 and x2.
// Nothing from HIP in here: the header also compiles as plain C++ (tests/test_lm_step_cpu.py drives it through a C shim).
#pragma once
#include <math.h>
#include "../../include/lifcal_ba.h"

#if defined(__HIPCC__)
#define LIFCAL_LM_HD __host__ __device__
#else
#define LIFCAL_LM_HD
#endif

namespace lifcal {

// the state of the loop: device-resident under k_lm_control (the host mirrors it once per iteration), a local array in the host loop
enum { LM_RADIUS = 0, LM_DECREASE = 1, LM_X_COST = 2, LM_GMAX = 3, LM_ITER = 4, LM_INVALID = 5, LM_STEP_OK = 6, LM_SUCCESSFUL = 7, LM_UNSUCCESSFUL = 8,
       LM_TERMINATION = 9, LM_COMMIT = 10 /* the step just judged was accepted */, LM_FRESH = 11, LM_INITIAL_COST = 12, LM_LAST_REL = 13, LM_LAST_STEP = 14, LM_LAST_CHANGE = 15, LM_SWEEPS = 16,
       LM_SEQ = 17 /* round counter of the host mirror */, LM_T0 = 18, LM_TICKS_LINEAR = 19 /* 100 MHz ticks: linear solve + candidate evaluation */,
       LM_BAD = 20 /* the fresh sweep met a point block that is not positive definite */, LM_MODEL_CHANGE = 21, LM_N = 24 };
struct LmOpts { double f_tol, p_tol, g_tol, min_rel_decrease, max_radius, min_radius; int max_iterations; };
constexpr double LM_DBL_MAX = 1.7976931348623157e308;
LIFCAL_LM_HD inline bool lm_finite(double v) { return fabs(v) < 1.7e308; }

LIFCAL_LM_HD inline void lm_reset(double* lm, double initial_radius) {
  for (int i = 0; i < LM_N; ++i) lm[i] = 0.0;
  lm[LM_RADIUS] = initial_radius; lm[LM_DECREASE] = 2.0; lm[LM_STEP_OK] = 1.0; lm[LM_FRESH] = 1.0; lm[LM_INITIAL_COST] = -1.0;
}

// stage 1: the sweep at a NEW point (a re-sweep of the same point at another radius is not taken in: its flag is not re-read)
LIFCAL_LM_HD inline void lm_take_sweep(double* lm, const LmOpts& o, double cost, double gmax, double bad) {
  lm[LM_X_COST] = cost; lm[LM_GMAX] = gmax; lm[LM_BAD] = bad;
  if (lm[LM_INITIAL_COST] < 0.0) {   // the first sweep of the solve
    lm[LM_INITIAL_COST] = cost;
    if (!lm_finite(cost)) { lm[LM_TERMINATION] = -1.0; return; }   // non-finite cost at the initial point
    if (gmax <= o.g_tol) { lm[LM_TERMINATION] = (double)LIFCAL_BA_TERM_GRADIENT_TOLERANCE; return; }
  }
  lm[LM_FRESH] = 0.0;
}

// stage 2, first half: top of the loop.  false: the solve has ended
LIFCAL_LM_HD inline bool lm_open_iteration(double* lm, const LmOpts& o) {
  if (lm[LM_ITER] >= (double)o.max_iterations) { lm[LM_TERMINATION] = (double)LIFCAL_BA_TERM_MAX_ITERATIONS; return false; }
  if (lm[LM_STEP_OK] != 0.0 && lm[LM_GMAX] <= o.g_tol) { lm[LM_TERMINATION] = (double)LIFCAL_BA_TERM_GRADIENT_TOLERANCE; return false; }
  if (lm[LM_RADIUS] < o.min_radius) { lm[LM_TERMINATION] = (double)LIFCAL_BA_TERM_MIN_RADIUS; return false; }
  lm[LM_ITER] += 1.0;
  return true;
}

// stage 2, second half: gtd = g^T d, ddd = d^T Lambda d of the step just solved.  false: invalid (radius halved; the fifth in a row ends the solve)
LIFCAL_LM_HD inline bool lm_check_step(double* lm, double gtd, double ddd, double chol_fail) {
  // model_cost_change = -g^T d - 1/2 d^T J^T J d with (J^T J + Lambda) d = -g  =>  1/2 (d^T Lambda d - g^T d)
  const double mcc = 0.5 * (ddd - gtd);
  const bool valid = chol_fail == 0.0 && lm[LM_BAD] == 0.0 && lm_finite(mcc) && mcc > 0.0;
  lm[LM_MODEL_CHANGE] = mcc; lm[LM_BAD] = 0.0;
  if (valid) { lm[LM_INVALID] = 0.0; return true; }
  lm[LM_INVALID] += 1.0;
  if (lm[LM_INVALID] >= 5.0) { lm[LM_TERMINATION] = (double)LIFCAL_BA_TERM_INVALID_STEPS; return false; }
  lm[LM_RADIUS] *= 0.5; lm[LM_STEP_OK] = 0.0; lm[LM_UNSUCCESSFUL] += 1.0;
  return false;
}

// stage 3.  Afterwards the solve has ended (LM_TERMINATION), or LM_COMMIT says whether the candidate becomes the current point
LIFCAL_LM_HD inline void lm_judge_step(double* lm, const LmOpts& o, double cand_cost, double step2, double x2) {
  lm[LM_COMMIT] = 0.0;
  if (!lm_finite(cand_cost)) cand_cost = LM_DBL_MAX;
  const double step_norm = sqrt(step2), x_norm = sqrt(x2);
  lm[LM_LAST_STEP] = step_norm;
  if (step_norm <= o.p_tol * (x_norm + o.p_tol)) { lm[LM_TERMINATION] = (double)LIFCAL_BA_TERM_PARAMETER_TOLERANCE; return; }
  const double cost_change = lm[LM_X_COST] - cand_cost;
  lm[LM_LAST_CHANGE] = cost_change;
  if (fabs(cost_change) <= o.f_tol * lm[LM_X_COST]) { lm[LM_TERMINATION] = (double)LIFCAL_BA_TERM_FUNCTION_TOLERANCE; return; }
  const double rel = (cand_cost >= LM_DBL_MAX) ? -LM_DBL_MAX : cost_change / lm[LM_MODEL_CHANGE];
  lm[LM_LAST_REL] = rel;
  if (rel > o.min_rel_decrease) {
    // radius /= max(1/3, 1 - t^3): t * t, then ONE fused multiply-add — what the device compiler has always made of
    // "1.0 - t * t * t" (the trajectories the tests pinned ran with it), spelled out so that a host compiler makes the same bits
    const double t = 2.0 * rel - 1.0;
    lm[LM_RADIUS] = fmin(o.max_radius, lm[LM_RADIUS] / fmax(1.0 / 3.0, fma(-(t * t), t, 1.0)));
    lm[LM_DECREASE] = 2.0;
    lm[LM_COMMIT] = 1.0; lm[LM_FRESH] = 1.0; lm[LM_STEP_OK] = 1.0; lm[LM_SUCCESSFUL] += 1.0;
  } else {
    lm[LM_RADIUS] = lm[LM_RADIUS] / lm[LM_DECREASE]; lm[LM_DECREASE] *= 2.0; lm[LM_STEP_OK] = 0.0; lm[LM_UNSUCCESSFUL] += 1.0;
  }
}

// what the caller of lifcal_ba_solve is told, from the final state
inline void lm_fill_summary(const double* lm, lifcal_ba_summary* s) {
  s->initial_cost = lm[LM_INITIAL_COST]; s->final_cost = lm[LM_X_COST]; s->final_radius = lm[LM_RADIUS]; s->final_gradient_max_norm = lm[LM_GMAX];
  s->iterations = (int32_t)lm[LM_ITER]; s->successful_steps = (int32_t)lm[LM_SUCCESSFUL]; s->unsuccessful_steps = (int32_t)lm[LM_UNSUCCESSFUL];
  s->termination = lm[LM_TERMINATION] != 0.0 ? (int32_t)lm[LM_TERMINATION] : LIFCAL_BA_TERM_MAX_ITERATIONS;
}

}  // namespace lifcal
