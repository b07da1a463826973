/*
 * lifcal_prior.h — Gaussian priors on the camera block and on poses of a bundle-adjustment handle.
 *
 * A prior is a quadratic term 1/2 d^T Lambda d, d = x - mean (plain differences, no angle wrap), on reduced parameters only:
 * the 17 camera slots (one 17 x 17 information matrix) and single poses (one 6 x 6 matrix per prior-ed frame).  It is what Ceres
 * computes for one extra residual block r = Lambda^(1/2) d per prior without a loss function: the term adds to the cost (of the
 * sweep and of a candidate), to the gradient (gradient_reduced += Lambda d, rhs -= Lambda d), to the Gauss-Newton matrix (S +=
 * Lambda on the camera x camera block and on the (f, f) band blocks) and to the Hessian diagonal behind the Jacobi scaling and the
 * LM clamp.  Slots that are not free parameters of the handle leave the term, rows and columns: camera slots in fixed_mask or
 * structurally absent, poses of a problem without the refine-poses bit, poses held by lifcal_ba_set_fixed_frames (the mask is
 * applied again after every lifcal_ba_set_fixed_frames).  initial_cost / final_cost of lifcal_ba_solve include the term;
 * lifcal_ba_reproj_stats and the residual report see observations only.  lifcal_ba_covariance reports the posterior covariance.
 *
 * The result of a sweep or a solve with priors has the same bits on every run as far as the prior is concerned, whatever
 * options.deterministic says: every word receives one add from the prior kernel, in stream order behind the sweep kernels.
 *
 * Priors on 3D points are the second part of this header: one 3 x 3 information matrix per control point,
 * the point set fixed when the handle is created.
 *
 * Not covered: points held exactly constant, priors that couple camera and poses, two poses, two points or a point with a pose,
 * handles with world_size > 1 and lifcal_ba_create_shard (LIFCAL_BA_ERR_INVALID_ARG), and lifcal_ba_solve_windowed, which creates
 * its own handles and carries no priors.
 */
#ifndef LIFCAL_PRIOR_H
#define LIFCAL_PRIOR_H

#include "lifcal_ba.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lifcal_ba_priors {
  const double* cam_mean;     /* [17], layout of lifcal_ba_problem.cam, values as stored (no sign folding); NULL: no camera prior */
  const double* cam_info;     /* [17*17] row-major, symmetric positive semi-definite information matrix; NULL iff cam_mean is NULL */
  uint32_t n_pose_priors, reserved;
  const uint32_t* pose_frame; /* [n] strictly ascending frame indices */
  const double* pose_mean;    /* [6n]  ax, ay, az, tx, ty, tz */
  const double* pose_info;    /* [36n] row-major, symmetric PSD */
} lifcal_ba_priors;

/* Host only, no device, no handle.  LIFCAL_BA_ERR_INVALID_ARG: a null pointer where a count says otherwise (or only one of cam_mean /
 * cam_info), a non-finite entry, |a_ij - a_ji| > 1e-12 sqrt(a_ii a_jj), a negative diagonal entry, an eigenvalue below
 * -1e-12 lambda_max, frames not strictly ascending.  LIFCAL_BA_ERR_OUT_OF_RANGE: pose_frame >= n_frames. */
int lifcal_ba_check_priors(uint32_t n_frames, const lifcal_ba_priors* p);

/* Replaces the priors of the handle (p == NULL clears them).  Checks first (lifcal_ba_check_priors) and leaves the handle unchanged
 * on error; copies everything and uploads once.  The matrices are symmetrised ((a_ij + a_ji) / 2).  A new prior starts a new solve:
 * the Jacobi scaling is taken again at the next sweep. */
int lifcal_ba_set_priors(lifcal_ba_handle* h, const lifcal_ba_priors* p);

/* 1/2 d^T Lambda d of the camera prior and the sum of it over the pose priors, at the device-resident parameters, over the live
 * slots (either pointer may be NULL).  0 and 0 without priors. */
int lifcal_ba_prior_cost(lifcal_ba_handle* h, double* cam_cost, double* pose_cost);

/* Host only: the bridge from lifcal_ba_covariance to a prior.  info = pseudo-inverse of the sub-matrix of cov (n x n, row-major,
 * n <= 64) selected by use_mask (bit i: row / column i), zero rows and columns elsewhere.  The rank is decided as
 * lifcal_ba_covariance decides it: on the sub-matrix Jacobi-scaled to unit diagonal, eigenvalues below rcond * lambda_max count as
 * null; *rank (may be NULL) receives the number kept, and info is the Moore-Penrose inverse of the sub-matrix over that many of its
 * largest eigenvalues.  Pass estimable_mask for the camera block, 0x3F for a pose block. */
int lifcal_prior_from_covariance(const double* cov, uint32_t n, uint64_t use_mask, double rcond, double* info, uint32_t* rank);

/* ---- priors on 3D points: control points with known coordinates ----
 *
 * 1/2 d^T Lambda d with d = P - mean per prior-ed point, what Ceres computes for one extra residual block Lambda^(1/2) d without a
 * loss function.  It adds to the cost (sweep, candidate, initial_cost / final_cost), to the point gradient, to the point block U_p
 * and to the Hessian diagonal behind the Jacobi scaling and the LM clamp, and through them to the Schur complement, rhs, the
 * back-substitution and the gradient norm.  A prior on an endpoint of a distance constraint (eliminated or promoted) and on a point
 * without observations is supported.  A problem without LIFCAL_BA_CFG_REFINE_POINTS (or without refined poses: the points are no
 * parameters then) drops the term: cost 0, nothing added.  lifcal_ba_reproj_stats and the residual report see observations only.
 * Three or more control points that are not collinear fix datum and scale of a scene.
 *
 * The planner treats prior-ed points like constraint points, so the point set belongs to the handle's layout and is fixed at
 * create; means and matrices can be replaced afterwards.  The prior's contribution has the same bits on every run, whatever
 * options.deterministic says. */
typedef struct lifcal_ba_point_priors {
  uint32_t n, reserved;
  const uint32_t* point;   /* [n] strictly ascending point ids */
  const double*   mean;    /* [3n] */
  const double*   info;    /* [9n] row-major, symmetric PSD 3x3 information matrices */
} lifcal_ba_point_priors;

/* Host only.  The rules and codes of lifcal_ba_check_priors on 3 x 3 matrices: LIFCAL_BA_ERR_INVALID_ARG for a null array with n > 0,
 * a non-finite entry, an asymmetric matrix, a negative diagonal entry, an eigenvalue below -1e-12 lambda_max, ids not strictly
 * ascending; LIFCAL_BA_ERR_OUT_OF_RANGE for a point id >= n_points. */
int lifcal_ba_check_point_priors(uint32_t n_points, const lifcal_ba_point_priors* p);

/* lifcal_ba_create with control points.  p == NULL or n == 0: exactly lifcal_ba_create (same layout, same results).  Checks first
 * (lifcal_ba_check_point_priors); options.world_size > 1 with n > 0 is LIFCAL_BA_ERR_INVALID_ARG.  The matrices are symmetrised. */
int lifcal_ba_create_with_point_priors(const lifcal_ba_problem* problem, const lifcal_ba_point_priors* p,
                                       const lifcal_ba_options* options, lifcal_ba_handle** out);

/* New means and matrices on the SAME point set (p == NULL: every matrix zero, the term leaves).  LIFCAL_BA_ERR_INVALID_ARG, with the
 * handle left as it was, for a handle that lifcal_ba_create_with_point_priors did not create and for a point set that differs from
 * the one given there; the codes of lifcal_ba_check_point_priors otherwise.  New values start a new solve: the Jacobi scaling is
 * taken again at the next sweep. */
int lifcal_ba_set_point_priors(lifcal_ba_handle* h, const lifcal_ba_point_priors* p);

/* Sum of 1/2 d^T Lambda d over the point priors at the device-resident points.  0 without priors or where the term is dropped. */
int lifcal_ba_point_prior_cost(lifcal_ba_handle* h, double* cost);

#ifdef __cplusplus
}
#endif
#endif /* LIFCAL_PRIOR_H */
