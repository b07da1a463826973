/*
 * lifcal_intersect.h — batched intersection of 3D points against a calibrated camera and known poses.
 *
 * The counterpart of lifcal_resect.h with the roles of points and frames exchanged: camera and poses are constants; every point
 * {X, Y, Z} is refined by a Levenberg-Marquardt solve of its own (own trust-region radius, own termination tests: Ceres semantics
 * of a one-point <2,17,6,3> problem whose camera block and pose blocks are held constant).  All points of a call are solved inside
 * one kernel launch, one wave per point, and every sum has one fixed order: the result of a point depends on its own observations
 * (in the caller's order) only, bit for bit.
 *
 * Part of the same shared library as include/lifcal_ba.h; status codes, options, config bits and termination reasons are those of
 * that header.  Every function returns 0 or a negative lifcal_ba_status; nothing throws.
 */
#ifndef LIFCAL_INTERSECT_H
#define LIFCAL_INTERSECT_H

#include "lifcal_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lifcal_intersect_problem {
  uint32_t n_obs, n_frames, n_points, reserved;
  const double* u;        /* as lifcal_ba_problem, any order */
  const double* v;
  const double* mcx;
  const double* mcy;
  const uint32_t* pt;
  const uint32_t* fr;
  const double* cam;      /* [17] constant, layout and sign folding of lifcal_ba_problem.cam */
  const double* views;    /* [6F] constant */
  double* pts;            /* [3P] in: start values, out: intersected points */
  double spx, spy, scale;
  uint32_t config;        /* nRadial / tangential / ROBUST / ML_CENTER_ADJ bits; the REFINE_* bits are ignored */
} lifcal_intersect_problem;

typedef struct lifcal_intersect_point {   /* one 144-byte row per point, no padding */
  double initial_cost, final_cost, final_radius, final_gradient_max_norm;
  double H[6];            /* undamped Gauss-Newton matrix J^T J of the point at the final point (loss through the corrector, as the
                             sweep), lower triangle row-major, parameter units (no Jacobi scaling); with camera and poses constant
                             its inverse is the covariance of the point */
  double g[3];            /* J^T r there */
  double sum_xx, sum_yy;  /* of e = projected - observed at the final point, parameters as stored (calcReprojectionError's rule) */
  uint32_t n_obs, n_inliers;   /* |e|^2 <= inlier_threshold^2 */
  int32_t iterations, successful_steps, unsuccessful_steps;
  int32_t termination;    /* lifcal_ba_termination; NONE for a point without observations; -1: the cost at the start values is not
                             finite (the point is left as it was) */
} lifcal_intersect_point;

/* Options are read as lifcal_ba_solve reads them: tolerances, radii, LM-diagonal clamps, loss_scale, max_iterations,
 * jacobi_scaling, device.  world_size > 1 and precision = 1 are LIFCAL_BA_ERR_INVALID_ARG; deterministic is ignored (the result
 * is always ordered).  Arguments are checked on the host before the device is touched: a null pointer is
 * LIFCAL_BA_ERR_INVALID_ARG, pt >= n_points or fr >= n_frames LIFCAL_BA_ERR_OUT_OF_RANGE.  A point without observations keeps its
 * coordinates, its row is all zeros.  The observations of a point are summed in the caller's order. */
int lifcal_intersect_points(const lifcal_intersect_problem* p, const lifcal_ba_options* o, double inlier_threshold,
                            lifcal_intersect_point* per_point /* [P] */, double* seconds /* kernel time, HIP events, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* LIFCAL_INTERSECT_H */
