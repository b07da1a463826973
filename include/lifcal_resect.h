/*
 * lifcal_resect.h — batched pose resection of frames against a calibrated camera.
 *
 * Camera and object points are constants; every frame's pose {ax, ay, az, tx, ty, tz} is refined by a Levenberg-Marquardt solve
 * of its own (own trust-region radius, own termination tests: Ceres semantics of a one-frame <2,17,6> problem whose camera block
 * is held constant).  All frames of a call are solved inside one kernel launch, one workgroup per frame, and every sum has one
 * fixed order: the result of a frame depends on its own observations (in the caller's order) only, bit for bit.
 *
 * Part of the same shared library as include/lifcal_ba.h; status codes, options, config bits and termination reasons are those of
 * that header.  Every function returns 0 or a negative lifcal_ba_status; nothing throws.
 */
#ifndef LIFCAL_RESECT_H
#define LIFCAL_RESECT_H

#include "lifcal_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lifcal_resect_problem {
  uint32_t n_obs, n_frames, n_points, reserved;
  const double* u;        /* as lifcal_ba_problem, any order */
  const double* v;
  const double* mcx;
  const double* mcy;
  const uint32_t* pt;
  const uint32_t* fr;
  const double* cam;      /* [17] constant, layout and sign folding of lifcal_ba_problem.cam */
  const double* pts;      /* [3P] constant */
  double* views;          /* [6F] in: start values, out: resected poses */
  double spx, spy, scale;
  uint32_t config;        /* nRadial / tangential / ROBUST / ML_CENTER_ADJ bits; the REFINE_* bits are ignored */
} lifcal_resect_problem;

typedef struct lifcal_resect_frame {   /* one row per frame */
  double initial_cost, final_cost, final_radius, final_gradient_max_norm;
  double H[21];           /* undamped Gauss-Newton matrix J^T J of the pose at the final point (loss through the corrector, as the
                             sweep), lower triangle row-major, parameter units (no Jacobi scaling) */
  double g[6];            /* J^T r there */
  double sum_xx, sum_yy;  /* of e = projected - observed at the final point, parameters as stored (calcReprojectionError's rule) */
  uint32_t n_obs, n_inliers;   /* |e|^2 <= inlier_threshold^2 */
  int32_t iterations, successful_steps, unsuccessful_steps;
  int32_t termination;    /* lifcal_ba_termination; NONE for a frame without observations; -1: the cost at the start values is not
                             finite (the pose is left as it was) */
} lifcal_resect_frame;

/* Options are read as lifcal_ba_solve reads them: tolerances, radii, LM-diagonal clamps, loss_scale, max_iterations,
 * jacobi_scaling, device.  world_size > 1 and precision = 1 are LIFCAL_BA_ERR_INVALID_ARG; deterministic is ignored (the result
 * is always ordered).  Arguments are checked on the host before the device is touched: a null pointer is
 * LIFCAL_BA_ERR_INVALID_ARG, pt >= n_points or fr >= n_frames LIFCAL_BA_ERR_OUT_OF_RANGE.  A frame without observations keeps its
 * pose, its row is all zeros.  The observations of a frame are summed in the caller's order. */
int lifcal_resect_frames(const lifcal_resect_problem* p, const lifcal_ba_options* o, double inlier_threshold,
                         lifcal_resect_frame* per_frame /* [F] */, double* seconds /* kernel time, HIP events, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* LIFCAL_RESECT_H */
