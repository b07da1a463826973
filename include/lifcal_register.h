/*
 * lifcal_register.h — register a scene from micro-image rays alone: poses of the frames and coordinates of
 * the points of a sequence taken with a calibrated camera, without start values from outside.
 *
 * The (frame, point) groups of lifcal_start.h triangulate every point metrically in the camera frame of each of its frames.  One
 * ANCHOR frame defines the world; its groups give the first points.  Round by round the frames that share enough mapped points are
 * aligned onto them (Horn), refined by resection, new points are carried into the world through the registered frames, and all
 * mapped points (by intersection) and all registered poses (by resection) are refined by one Levenberg-Marquardt solve each.  The
 * result is metric and is a start for lifcal_ba_create; what has to come from outside are the tracks (pt, fr of an observation).
 * The whole chain runs on the device; the host reads one word per round.  Every sum has one fixed order: the same call twice gives
 * the same bits.
 *
 * Part of the same shared library as include/lifcal_ba.h; status codes, options and config bits are those of that header.  Every
 * function returns 0 or a negative lifcal_ba_status; nothing throws.
 */
#ifndef LIFCAL_REGISTER_H
#define LIFCAL_REGISTER_H

#include "lifcal_start.h"

#ifdef __cplusplus
extern "C" {
#endif

/* status of a frame */
enum {
  LIFCAL_REGISTER_FRAME_OK = 0,           /* registered: its pose is written */
  LIFCAL_REGISTER_FRAME_EMPTY = 1,        /* no observations */
  LIFCAL_REGISTER_FRAME_UNREACHED = 2,    /* never had min_shared used groups on mapped points */
  LIFCAL_REGISTER_FRAME_DEGENERATE = 3    /* had them, but the alignment was degenerate in every round it was tried */
};

/* status of a point */
enum {
  LIFCAL_REGISTER_POINT_OK = 0,           /* mapped: its coordinates are written */
  LIFCAL_REGISTER_POINT_EMPTY = 1,        /* no observations */
  LIFCAL_REGISTER_POINT_UNREACHED = 2     /* no used group in a registered frame */
};

typedef struct lifcal_register_problem {  /* lifcal_resect_problem without known points */
  uint32_t n_obs, n_frames, n_points, reserved;
  const double *u, *v, *mcx, *mcy;        /* [n_obs] as in lifcal_ba_problem, any order */
  const uint32_t *pt, *fr;                /* [n_obs] */
  const double* cam;                      /* [17] constant */
  double* views;                          /* [6 n_frames] OUTPUT ONLY: written for registered frames, other frames keep their bits */
  double* pts;                            /* [3 n_points] OUTPUT ONLY: written for mapped points, other points keep their bits */
  double spx, spy, scale;
  uint32_t config;                        /* nRadial / tangential / ROBUST / ML_CENTER_ADJ bits */
} lifcal_register_problem;

typedef struct lifcal_register_options {
  double gate_px;             /* 1.0; > 0, +infinity: no gate (the rule of lifcal_start_poses) */
  double inlier_threshold;    /* 1.0 */
  uint32_t min_shared;        /* 6; >= 3: the used groups on mapped points a frame needs to be registered */
  int32_t anchor_frame;       /* -1: the frame with the most used groups, the lowest index on ties */
  const double* anchor_view;  /* [6] the pose given to the anchor frame; NULL: zeros (world = the anchor's camera frame) */
  uint32_t max_rounds;        /* 0: until a round registers no frame */
  uint32_t reserved;
} lifcal_register_options;

typedef struct lifcal_register_frame {    /* one 64-byte row per frame, no padding */
  double sum_xx, sum_yy;      /* of e = projected - observed over the n_obs_used observations at the returned poses and points,
                                 parameters as stored (calcReprojectionError's rule); status 0 */
  double final_cost;          /* of the frame's last pose solve (zero for the anchor, which has none) */
  uint32_t n_obs, n_obs_used; /* all observations of the frame | those of mapped points (status 0) */
  uint32_t n_inliers;         /* |e|^2 <= inlier_threshold^2 among the n_obs_used */
  uint32_t n_groups, n_used;  /* its (frame, point) groups | those of group status 0 */
  uint32_t n_shared;          /* used groups on mapped points when the frame was aligned, or at the end of the call if it never was */
  int32_t status, round;      /* round: 0 the anchor, r >= 1 the round that registered the frame, -1 not registered */
  int32_t iterations, termination;   /* of its last pose solve (lifcal_ba_termination) */
} lifcal_register_frame;

typedef struct lifcal_register_point {    /* one 56-byte row per point, no padding */
  double sum_xx, sum_yy;      /* as above over the point's n_obs_used observations; status 0 */
  double final_cost;          /* of the point's last solve */
  uint32_t n_obs, n_obs_used; /* all observations of the point | those in registered frames (status 0) */
  uint32_t n_inliers;
  uint32_t n_frames_used;     /* registered frames with an observation of the point (status 0) */
  int32_t status, round;      /* round: the round whose extension mapped the point, -1 not mapped */
  int32_t iterations, termination;
} lifcal_register_point;

typedef struct lifcal_register_summary {
  int32_t anchor_frame;       /* -1: there was none (no used group) */
  uint32_t n_rounds;          /* the last round r >= 1 that registered a frame (0: the anchor alone) */
  uint32_t n_frames_registered, n_points_mapped;
  uint32_t n_groups, n_groups_used;
} lifcal_register_summary;

void lifcal_register_default_options(lifcal_register_options* r);

/* Poses and points of p from its observations and the constant camera block alone.
 *   groups    exactly those of lifcal_start_poses: ascending (fr, pt) order, statuses 0 - 4, the gate.
 *   round 0   the anchor gets anchor_view.  Extend: every unmapped point with a used group in a registered frame becomes
 *             P = sum w R_f^T (p_c - t_f) / sum w, w = 1 / Z_c^2, over those groups.  Refine points: one solve with the semantics of
 *             lifcal_intersect_points for every mapped point over all its observations in registered frames.
 *   round r   every unregistered frame with >= min_shared used groups on mapped points is aligned onto them (the alignment of
 *             lifcal_start_poses over those groups); if that is not degenerate, one solve with the semantics of lifcal_resect_frames
 *             over its observations of mapped points follows and the frame is registered.  No frame registered: the call ends.
 *             Else extend, refine points, refine poses (every registered frame but the anchor).
 * The options o are read as lifcal_resect_frames and lifcal_intersect_points read them; world_size > 1 and precision = 1 are
 * LIFCAL_BA_ERR_INVALID_ARG, deterministic is ignored.  min_shared < 3, a gate_px that is not > 0 and an anchor_frame >= n_frames
 * are LIFCAL_BA_ERR_INVALID_ARG, an index out of range LIFCAL_BA_ERR_OUT_OF_RANGE; arguments are checked on the host before the
 * device is touched.  A call without observations or without a used group is answered with n_rounds = 0 and nothing registered. */
int lifcal_register_scene(const lifcal_register_problem* p, const lifcal_ba_options* o, const lifcal_register_options* r,
                          lifcal_register_frame* per_frame /* [F] */, lifcal_register_point* per_point /* [P] */,
                          lifcal_register_summary* summary, double* seconds /* kernel time, HIP events, or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* LIFCAL_REGISTER_H */
