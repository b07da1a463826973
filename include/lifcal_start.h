/*
 * lifcal_start.h — closed-form start values from micro-image rays: poses for lifcal_resect_frames and
 * points for lifcal_intersect_points, without an external structure-from-motion run.
 *
 * With the camera block known, every micro-image observation (u, v, mcx, mcy) fixes a line in the camera frame (two rows that are
 * linear in the camera-frame point).  The micro images of one (frame, point) pair — a GROUP — triangulate that point metrically in
 * the camera frame; a weighted rigid alignment (Horn's quaternion method) of those points onto the known world points is the pose
 * of the frame.  With poses known the same lines, carried into the world frame, triangulate a point from all its frames.
 * Nothing is iterated apart from the ten fixed-point sweeps of the distortion inverse and the Jacobi rotations of a 4x4 matrix.
 * Every sum has one fixed order: the row of a frame (a point) depends on its own observations only, bit for bit.
 *
 * Part of the same shared library as include/lifcal_ba.h; status codes, options and config bits are those of that header, the
 * problem structs those of lifcal_resect.h and lifcal_intersect.h.  Every function returns 0 or a negative lifcal_ba_status;
 * nothing throws.
 */
#ifndef LIFCAL_START_H
#define LIFCAL_START_H

#include "lifcal_resect.h"
#include "lifcal_intersect.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status of a group (one (frame, point) pair) */
enum {
  LIFCAL_START_GROUP_USED = 0,
  LIFCAL_START_GROUP_SINGLE = 1,      /* a single observation: a line, not a point */
  LIFCAL_START_GROUP_SINGULAR = 2,    /* a non-positive or non-finite pivot, or a non-finite result */
  LIFCAL_START_GROUP_BEHIND = 3,      /* Z_c <= 0 */
  LIFCAL_START_GROUP_GATED = 4        /* rms_px > gate_px */
};

/* status of a frame */
enum {
  LIFCAL_START_FRAME_OK = 0,
  LIFCAL_START_FRAME_EMPTY = 1,       /* no observations: every other field of the row is zero */
  LIFCAL_START_FRAME_FEW = 2,         /* fewer than three used groups */
  LIFCAL_START_FRAME_DEGENERATE = 3   /* eig[0] - eig[1] <= 1e-9 |eig[0]|: the used points are collinear (or a sum is not finite) */
};

/* status of a point */
enum {
  LIFCAL_START_POINT_OK = 0,
  LIFCAL_START_POINT_EMPTY = 1,       /* no observations: every other field of the row is zero */
  LIFCAL_START_POINT_SINGLE = 2,      /* one observation */
  LIFCAL_START_POINT_SINGULAR = 3,    /* a non-positive or non-finite pivot, or a non-finite result */
  LIFCAL_START_POINT_BEHIND = 4       /* Z_c + zC0 <= 0 in one of its frames at the solution */
};

typedef struct lifcal_start_frame {   /* one 72-byte row per frame, no padding */
  double sum_w;           /* sum of the weights w = 1 / Z_c^2 of the used groups */
  double align_rms;       /* sqrt(sum w |R P + t - p_c|^2 / sum w), mm (status 0) */
  double eig[2];          /* the two largest eigenvalues of Horn's 4x4 matrix (status 0 and 3) */
  double sum_xx, sum_yy;  /* of e = projected - observed over ALL observations of the frame at the new pose, parameters as stored
                             (calcReprojectionError's rule), status 0 */
  uint32_t n_obs, n_inliers;   /* |e|^2 <= inlier_threshold^2 (status 0) */
  uint32_t n_groups, n_used;
  int32_t status, reserved;
} lifcal_start_frame;

typedef struct lifcal_start_group {   /* one 48-byte row per group, in ascending (fr, pt) order */
  double xyz[3];          /* the triangulated camera-frame point p_c, mm (zero for status 1 and 2) */
  double rms_px;          /* sqrt(sum (rho_x^2 + rho_y^2) / n_obs), rho = (row p_c - rhs) / (Z_c + zC0) (zero for status 1 and 2) */
  uint32_t fr, pt, n_obs;
  int32_t status;
} lifcal_start_group;

typedef struct lifcal_start_point {   /* one 40-byte row per point, no padding */
  double sum_xx, sum_yy;  /* of e = projected - observed at the new point, parameters as stored (status 0) */
  double min_pivot;       /* smallest Cholesky pivot of the Jacobi-scaled 3x3 matrix (1: orthogonal rows; status 0, 3 and 4) */
  uint32_t n_obs, n_inliers;
  int32_t status, reserved;
} lifcal_start_point;

/* Poses of all frames of p.  p->views is OUTPUT ONLY: its incoming values are never read, views[6f .. 6f+5] is written for a
 * frame of status 0 and keeps its bits otherwise; p->pts are constants.  Groups are taken in ascending (fr, pt) order, the
 * observations of a group in the caller's order.  gate_px > 0 is the largest triangulation residual of a used group (+infinity:
 * no gate); anything else is LIFCAL_BA_ERR_INVALID_ARG.  groups (capacity n_obs rows) and n_groups may be NULL.
 * Options: device is read; world_size > 1 and precision = 1 are LIFCAL_BA_ERR_INVALID_ARG; deterministic is ignored.  Arguments
 * are checked on the host before the device is touched, as lifcal_resect_frames checks them. */
int lifcal_start_poses(const lifcal_resect_problem* p, const lifcal_ba_options* o, double gate_px, double inlier_threshold,
                       lifcal_start_frame* per_frame /* [F] */, lifcal_start_group* groups /* [n_obs] capacity, or NULL */,
                       uint32_t* n_groups /* out, or NULL */, double* seconds /* kernel time, HIP events, or NULL */);

/* Points of p from all their observations.  p->pts is OUTPUT ONLY: pts[3k .. 3k+2] is written for a point of status 0 and keeps
 * its bits otherwise; p->views are constants.  The observations of a point are summed in the caller's order.  No gate. */
int lifcal_start_points(const lifcal_intersect_problem* p, const lifcal_ba_options* o, double inlier_threshold,
                        lifcal_start_point* per_point /* [P] */, double* seconds /* kernel time, HIP events, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* LIFCAL_START_H */
