/*
 * lifcal_ba.h — C ABI of the MI355X-native plenoptic bundle-adjustment solver.
 *
 * Drop-in boundary: the body of LiFCal's CameraCalibration::performBundleAdjustment()
 * (reference src/CameraCalibration.cpp:774-992), i.e. everything between
 * "ceres::Problem minimizationProblem" (:858) and "ceres::Solve" (:965), plus
 * calcReprojectionError() (:1026-1103).  The reference has no FFI of its own; these entry
 * points are what a binding for that seam would call (see INTEGRATION.md for the adapter).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - All parameter arrays are owned by the caller; lifcal_ba_solve() updates them IN PLACE on
 *     return (Ceres semantics: reference :892-911 registers the caller's own storage).
 *   - Every function returns 0 on success or a negative lifcal_ba_status; nothing throws.
 *   - A handle is not re-entrant; one host thread drives it.
 *   - There is NO CPU fallback: without a usable gfx950 device create() fails with
 *     LIFCAL_BA_ERR_NO_DEVICE.
 */
#ifndef LIFCAL_BA_H
#define LIFCAL_BA_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* reference: #define MAX_NUMBER_OF_CAMERA_PARAMETERS 17  (src/CalibrationData/CalibrationData.h:19) */
#define LIFCAL_BA_MAX_CAMERA_PARAMETERS 17

/* config bitmask — identical bit layout to reference src/CameraCalibration.cpp:778-814 and the
 * decoder in src/BundleAdjustment/BundleAdjustment.h:28-79 */
#define LIFCAL_BA_CFG_NRADIAL_MASK   0x000003u  /* number of radial coefficients (0..2)           */
#define LIFCAL_BA_CFG_TANGENTIAL     0x000004u  /* two tangential coefficients                    */
#define LIFCAL_BA_CFG_REFINE_POSES   0x000100u  /* Model.refineExtrinsicOrientations              */
#define LIFCAL_BA_CFG_ROBUST         0x000200u  /* Model.robustCostFunction -> CauchyLoss(0.5)    */
#define LIFCAL_BA_CFG_REFINE_POINTS  0x000400u  /* Model.refineCoordinatesPoints                  */
#define LIFCAL_BA_CFG_ML_CENTER_ADJ  0x000800u  /* Model.adjustMicroLensCenters                   */

typedef enum {
  LIFCAL_BA_OK               =  0,
  LIFCAL_BA_ERR_INVALID_ARG  = -1,
  LIFCAL_BA_ERR_NO_DEVICE    = -2,  /* no gfx950 device / HIP runtime failure at create        */
  LIFCAL_BA_ERR_HIP          = -3,  /* a HIP call failed later (see lifcal_ba_last_error)      */
  LIFCAL_BA_ERR_OUT_OF_RANGE = -4,  /* an index in pt/fr/c_i/c_j exceeds n_points/n_frames     */
  LIFCAL_BA_ERR_NOMEM        = -5,
  LIFCAL_BA_ERR_COMM         = -6,  /* all-reduce hook / RCCL failure                           */
  LIFCAL_BA_ERR_NUMERIC      = -7   /* non-finite cost at the initial point                     */
} lifcal_ba_status;

/* termination reasons of lifcal_ba_solve (Ceres 2.1 TrustRegionMinimizer vocabulary) */
typedef enum {
  LIFCAL_BA_TERM_NONE               = 0,
  LIFCAL_BA_TERM_FUNCTION_TOLERANCE = 1,  /* |dcost| <= f_tol * cost                           */
  LIFCAL_BA_TERM_PARAMETER_TOLERANCE= 2,  /* |step| <= p_tol (|x| + p_tol)                     */
  LIFCAL_BA_TERM_GRADIENT_TOLERANCE = 3,  /* max|g| <= g_tol                                    */
  LIFCAL_BA_TERM_MAX_ITERATIONS     = 4,
  LIFCAL_BA_TERM_MIN_RADIUS         = 5,  /* trust-region radius below 1e-32                    */
  LIFCAL_BA_TERM_INVALID_STEPS      = 6   /* 5 consecutive invalid steps (Cholesky failed ...)  */
} lifcal_ba_termination;

/*
 * The problem, flattened from the reference's host structures:
 *   cam    <- double camera[17] = {fL, bL0, B, cx, cy, k_1..k_nRad, p_1, p_2, 0...}   (:821-853)
 *   views  <- double views[6F], per frame {ax, ay, az, tx, ty, tz}, Euler XYZ          (:864-868)
 *   pts    <- std::vector<Eigen::Vector3d> p3d_w, contiguous 24-byte records           (CameraCalibration.h:102)
 *   u,v    <- frame::rawImageCoordinates[k]           (CalibrationData.h:40)
 *   mcx,mcy<- frame::microLensCenter[k]               (CalibrationData.h:41)
 *   pt     <- frame::objectCoordinatesByRawID[k] - p3d_w.data()   (CalibrationData.h:42)
 *   fr     <- index of the frame the observation belongs to
 *   spx,spy<- pixelSize_totFoc (both), scale <- (double)depth_to_raw_im_scale          (:882)
 *   c_*    <- std::vector<Constraint>{pointID_1, pointID_2, distance, sigma}; they are used only
 *             when REFINE_POINTS is set and use_constraints != 0 (reference :916: not in recalib)
 *   fixed_mask / lower / upper <- recalib: SubsetManifold(17,{0,2}) and box bounds (:927-953).
 *             lower/upper may be NULL (unbounded); otherwise 17 entries, +-INFINITY = unbounded.
 * Observations may be given in any order (the reference's is frame-major); the library re-sorts
 * internally and never returns per-observation data in its own order.
 */
typedef struct lifcal_ba_problem {
  uint32_t n_obs, n_frames, n_points, n_constraints;
  const double*   u;
  const double*   v;
  const double*   mcx;
  const double*   mcy;
  const uint32_t* pt;
  const uint32_t* fr;
  double* cam;    /* [17]  in/out */
  double* views;  /* [6F]  in/out */
  double* pts;    /* [3P]  in/out */
  double spx, spy, scale;
  uint32_t config;
  uint32_t fixed_mask;       /* bit i set -> camera[i] held constant */
  const double* lower;       /* [17] or NULL */
  const double* upper;       /* [17] or NULL */
  const uint32_t* c_i;       /* [M] or NULL */
  const uint32_t* c_j;
  const double*   c_dist;
  const double*   c_sigma;
  uint32_t use_constraints;  /* 0: ignore c_* (recalib), 1: add them when REFINE_POINTS */
  uint32_t reserved;
} lifcal_ba_problem;

/* Solver options; defaults = what the reference hard-codes (:955-961) + Ceres 2.1 defaults. */
typedef struct lifcal_ba_options {
  double function_tolerance;    /* 1e-6  (:958) */
  double parameter_tolerance;   /* 1e-8  (:959) */
  double gradient_tolerance;    /* 1e-10 (Ceres default) */
  double initial_radius;        /* 1e4   (Ceres default initial_trust_region_radius) */
  double max_radius;            /* 1e16 */
  double min_radius;            /* 1e-32 */
  double min_relative_decrease; /* 1e-3 */
  double min_lm_diagonal;       /* 1e-6 */
  double max_lm_diagonal;       /* 1e32 */
  double loss_scale;            /* 0.5: CauchyLoss(0.5) (:892) */
  int32_t max_iterations;       /* 200 (:960) */
  int32_t jacobi_scaling;       /* 1 */
  int32_t precision;            /* 0: fp64 everywhere; 1: residual and Jacobian of an observation evaluated in fp32 (observation stored relative to its
                                   micro-lens centre, fp32 lens table: 12 B per observation in the sweep's stream), every accumulation, the
                                   elimination and the solve in fp64; accept/reject decisions use fp64 costs (BASELINE configs[4])              */
  int32_t device;               /* HIP device ordinal */
  int32_t rank;                 /* this process' rank in the point-sharded job (0 if single GPU) */
  int32_t world_size;           /* number of ranks (1 if single GPU) */
  int32_t verbose;              /* 1: print Ceres-style per-iteration table to stdout (:957) */
  int32_t deterministic;        /* 1: bitwise reproducible results — LDS accumulation in wave order, per-block window slabs summed in block order
                                   instead of the cross-block f64 atomics, value kernels summed per workgroup in order; points with distance
                                   constraints, tracks longer than the LDS window and the camera-only / pose-only arities emit their global
                                   atomics one wave after the other (slow when every point takes that path).  Every problem structure,
                                   box bounds included, is supported.                                                                     */
} lifcal_ba_options;

typedef struct lifcal_ba_summary {
  double initial_cost, final_cost;
  double final_radius;
  double final_gradient_max_norm;
  int32_t iterations;             /* LM iterations taken (Ceres counts iteration 0 separately) */
  int32_t successful_steps, unsuccessful_steps;
  int32_t termination;            /* lifcal_ba_termination */
  double seconds_total, seconds_sweep, seconds_linear_solve;
} lifcal_ba_summary;

/* One Jacobian+Schur sweep (the benchmarked unit).  Host pointers may be NULL to
 * skip the copy-back.  Canonical reduced ordering of S/rhs: [camera 0..16 | views 6F | promoted
 * points 3 each, in ascending point id]; fixed / structurally-dead camera slots are returned as
 * identity rows with rhs 0.  S is row-major n_red x n_red, symmetric, both triangles filled. */
typedef struct lifcal_ba_sweep_out {
  double cost;                   /* 1/2 sum rho(|r|^2) (+ constraints) at the current point      */
  double gradient_max_norm;      /* max |J^T r| over all free parameters                          */
  uint32_t n_reduced;            /* 17 + 6F + 3*n_promoted                                        */
  uint32_t n_promoted;
  double* S;                     /* [n_reduced^2] or NULL                                         */
  double* rhs;                   /* [n_reduced]   or NULL:  S * delta_reduced = rhs               */
  double* gradient_reduced;      /* [n_reduced]   or NULL:  J_B^T r before elimination            */
  double* point_gradient;        /* [3P]          or NULL:  J_P^T r                               */
  double* point_hessian_inv;     /* [9P]          or NULL:  (U_p + D_p)^-1 row-major              */
  double seconds;                /* device time of the sweep kernels (HIP events)                 */
} lifcal_ba_sweep_out;

/* reference calcReprojectionError (:1026-1103) */
typedef struct lifcal_ba_stats {
  double std_x, std_y;   /* sqrt(sum e^2 / N): RMS, not mean-removed (:1097-1098) */
  double mae_x, mae_y;   /* MAX abs error despite the name (:1083-1084)           */
  uint32_t num_points, num_inliers;   /* |e|^2 <= thr^2 (:1088)                   */
} lifcal_ba_stats;

typedef struct lifcal_ba_handle lifcal_ba_handle;

/* Multi-GPU: observations are sharded by 3D point across ranks (one process per GPU).  The only
 * data-path exchange is a sum all-reduce of f64 device buffers.  Either install a hook (the host
 * language supplies the collective, e.g. torch.distributed -> RCCL) or let the library own an
 * RCCL communicator (lifcal_ba_comm_init_rccl).  `stream` is the hipStream_t the buffer was
 * produced on; the hook must leave the reduced result in place, ordered on that stream. */
typedef int (*lifcal_ba_allreduce_fn)(void* ctx, void* device_buf, size_t count_f64, void* stream);
/* Optional second collective.  Points are owned in first-frame order, so the partial reduced system of a rank is
 * non-zero only in ONE contiguous range of frames (+ the small camera block): instead of summing the whole block the
 * library packs that range into a slab, ALL-GATHERS the equally sized slabs (count_f64 doubles per rank; recv holds
 * world_size * count_f64, rank-major) and adds them up locally - about half the bytes of the all-reduce, and it is the
 * path the library-owned RCCL communicator takes by itself.  With hooks it is used when BOTH hooks are installed (the
 * all-reduce is still needed for a few small buffers); LIFCAL_DENSE_ALLREDUCE=1 forces the plain all-reduce. */
typedef int (*lifcal_ba_allgather_fn)(void* ctx, const void* device_send, void* device_recv, size_t count_f64, void* stream);

void lifcal_ba_default_options(lifcal_ba_options* o);

/* replaces reference :858-953 (problem construction): validates, sorts observations point-major,
 * builds the tile layout and uploads everything to HBM. */
int lifcal_ba_create(const lifcal_ba_problem* p, const lifcal_ba_options* o, lifcal_ba_handle** out);

/* replaces reference :965 (ceres::Solve) + :967-988 is the caller's unpack of cam[] */
int lifcal_ba_solve(lifcal_ba_handle* h, lifcal_ba_summary* s);

/* one Jacobian+Schur sweep at trust-region radius `radius` on the CURRENT device-resident point */
int lifcal_ba_sweep(lifcal_ba_handle* h, double radius, lifcal_ba_sweep_out* out);

/* the same sweep without the host round trip: kernels are only enqueued on the handle's stream (read the
 * result later with lifcal_ba_sweep, or synchronise the stream).  Used for back-to-back timing. */
int lifcal_ba_sweep_enqueue(lifcal_ba_handle* h, double radius);

/* HIP-event instrumentation of the sweeps on the stream the kernels run on.  The dominant kernel carries its own start / stop
 * events (written by its dispatch packet: no extra barrier packets in the queue); one record opens the span before the first
 * profiled sweep, one closes it behind the last.  begin() reserves events for up to max_sweeps sweeps; end() synchronises and averages. */
typedef struct lifcal_ba_profile {
  uint32_t n_sweeps;
  double special_points;  /* points worked by the special-point kernels (k_sweep + k_schur: constraints, oversized groups,
                             camera-only / pose-only arities); their time is part of ms_schur, NOT of ms_accumulate        */
  double ms_accumulate;   /* the dominant kernel of the regular points by its own dispatch time stamps: k_sweep3 or k_sweep2 (fused
                             residual + Jacobian + accumulation + point elimination)                                       */
  double ms_schur;        /* ms_total - ms_accumulate: special points, constraints, exchange, k_finalize, gaps (tables: only where the parameters changed) */
  double ms_total;        /* first kernel of the first sweep to the end of the last one, divided by the sweep count    */
  double ms_exchange;     /* world_size > 1: pack + collective + unpack of the partial reduced blocks (part of ms_schur)  */
  uint32_t n_sampled;     /* sweeps of the span whose dominant kernel carried the time stamps (ms_accumulate / ms_exchange average THESE) */
} lifcal_ba_profile;
/* The next max_sweeps sweeps form a span (ms_total: two event records, before the first and behind the last).  A SAMPLED sweep's
 * dominant kernel carries its own start / stop events, which costs ~5 us of queue time per sampled sweep: _begin samples every
 * sweep, _begin_sampled every stride-th (0, stride, 2 stride, ...) so that a timing loop is measured nearly undisturbed.            */
int lifcal_ba_profile_begin(lifcal_ba_handle* h, uint32_t max_sweeps);
int lifcal_ba_profile_begin_sampled(lifcal_ba_handle* h, uint32_t max_sweeps, uint32_t stride);
int lifcal_ba_profile_end(lifcal_ba_handle* h, lifcal_ba_profile* out);

/* replaces reference :1026-1103 (evaluated on the device-resident parameters) */
int lifcal_ba_reproj_stats(lifcal_ba_handle* h, double inlier_threshold, lifcal_ba_stats* out);
/* The x_proj / y_proj columns of reference storeRawImagePointsCsv (:1504-1538): the model's projection of every observation at
 * the stored parameters, [n_obs] host arrays in the caller's observation order, evaluated as reproj_stats evaluates it.
 * With world_size > 1 a rank fills the observations of the points it owns and leaves NaN elsewhere. */
int lifcal_ba_project_observations(lifcal_ba_handle* h, double* x_proj, double* y_proj);

/* ---- covariance of the parameters ----
 * Evaluated at the device-resident parameters (like lifcal_ba_reproj_stats) on the UNDAMPED Gauss-Newton matrix H of the reduced
 * system: Ceres semantics (robust loss through the corrector, points eliminated as in the solve), G = H^- for unit-variance pixel
 * residuals.  With poses and points both refined and no frame held constant, one gauge frame is held constant for the call: that
 * removes the six rigid directions of the scene.  What is left of the null space (the arrow Schur complement C: camera slots +
 * promoted points) is measured on the Jacobi-scaled C: eigenvalues below null_rcond * lambda_max count as null, and G uses the
 * pseudo-inverse of the rest.  A camera slot is ESTIMABLE when the null directions have no component on it (relative size
 * <= estimable_tol in the scaled coordinates); the variance of an estimable slot does not depend on the g-inverse chosen.
 * Pose blocks are relative to the gauge frame (and to the minimum-norm choice in the scaled coordinates of C).  Fixed slots,
 * structurally absent slots, constant poses and the gauge frame are zero rows / columns.  The handle is left as it was: fixed-frame
 * mask, Jacobi scaling state, LM state and parameters.  One rank, options.precision = 0, the LDS-window band factorisation. */
typedef struct lifcal_ba_covariance_options {
  int32_t gauge_frame;                 /* -1: automatic (first observed frame, when a gauge exists), >= 0: this frame, -2: none      */
  int32_t want_pose_blocks;            /* 1: fill out->pose                                                                          */
  int32_t scale_by_residual_variance;  /* 1: multiply G by sigma2 = 2 cost / (m - r) (an approximation under the Cauchy loss)       */
  int32_t reserved;
  double null_rcond;                   /* 1e-9: eigenvalue threshold of the scaled C, relative to its largest                        */
  double estimable_tol;                /* 1e-3: largest null-vector component (unit vector, scaled coordinates) of an estimable slot */
} lifcal_ba_covariance_options;

typedef struct lifcal_ba_covariance_out {
  double* camera;            /* [17 * 17] row-major, caller-allocated                                                                 */
  double* pose;              /* [F * 36] or NULL: 6x6 block of every pose (order ax, ay, az, tx, ty, tz)                              */
  double* pose_band;         /* [F * bw * 36] or NULL: S_ff^-1 blocks (j, j+dd), dd = 1..bw (bw: max_window_frames - 1), unscaled, gauge-relative */
  double* camera_null;       /* [17 * 17] or NULL: first null_rank rows = camera components of the null directions (parameter units)  */
  uint32_t estimable_mask;   /* bit j: camera slot j is live and estimable                                                            */
  uint32_t null_rank;        /* null directions of C left after the gauge frame                                                       */
  int32_t gauge_frame_used;  /* -1: none                                                                                              */
  uint32_t live_mask;        /* bit j: camera slot j is a free parameter                                                              */
  double sigma2;             /* 2 cost / (m - r), reported whether or not it was applied                                              */
  double cost;               /* cost at the evaluated parameters                                                                      */
  double seconds;            /* device time of the call (sweep + K1..K4)                                                              */
} lifcal_ba_covariance_out;

void lifcal_ba_default_covariance_options(lifcal_ba_covariance_options* o);
int lifcal_ba_covariance(lifcal_ba_handle* h, const lifcal_ba_covariance_options* o, lifcal_ba_covariance_out* out);

/* ---- calibration judged in object space ----
 * The numeric form of the reference's refCameraCoordinates / projectedCameraCoordinates folders (storeResults :1218-1287), at the
 * device-resident parameters: for image points of the virtual image (x_v, y_v, virtual depth, frame, object point; host arrays)
 * ref_c = RT P (:1256-1260) and proj_c = projectPointBack of the image point (:1276-1284, as include/lifcal_depth.h evaluates it:
 * camera as stored, spx / spy of the problem), both [3n] host arrays or NULL.  The statistics are those of proj_c - ref_c over the
 * points with vdepth >= 2 (the reference leaves smaller ones out of its initial fit, :482; they are counted in n_skipped),
 * summed per workgroup and then over the workgroups in a fixed order: the result is reproducible.  One rank. */
typedef struct lifcal_ba_object_space {
  double rms[3];          /* sqrt(mean (proj_c - ref_c)^2) per axis     */
  double max_abs[3];      /* largest |proj_c - ref_c| per axis          */
  double rms_rel_depth;   /* RMS of (z_proj - z_ref) / z_ref            */
  uint64_t n_used, n_skipped;
} lifcal_ba_object_space;
int lifcal_ba_object_space_stats(lifcal_ba_handle* h, uint64_t n, const double* x, const double* y, const double* vdepth, const uint32_t* fr,
                                 const uint32_t* pt, double* ref_c, double* proj_c, lifcal_ba_object_space* out);

/* ---- residual report: the reprojection errors grouped by frame, point and micro lens ----
 * Evaluated at the device-resident parameters exactly as lifcal_ba_reproj_stats evaluates them (parameters as stored, no sign
 * folding).  e = projected - observed in raw pixels.  Every table is a segmented sum in a fixed order (no atomics): the output is
 * bitwise reproducible whatever options.deterministic says.  A lens id is the planner's de-duplicated lens index (exact-bit equal
 * (mcx, mcy) share one id); it is stable for the handle and lens_xy[2 id], lens_xy[2 id + 1] are the (mcx, mcy) of its observations.
 * One rank (world_size > 1: LIFCAL_BA_ERR_INVALID_ARG); every arity, options.precision 0 and 1.  The handle is left as it was. */
typedef struct lifcal_ba_group_stats {      /* 64 bytes, one row per group; an empty group is all zeros */
  double sum_x, sum_y;        /* sum of e_x, e_y -> mean offset                                                         */
  double sum_xx, sum_yy;      /* sum of e_x^2, e_y^2 -> RMS as calcReprojectionError defines it                         */
  double sum_w;               /* sum of the loss weight rho'(|e|^2); equals n when the loss is off                      */
  double max_abs_x, max_abs_y;
  uint32_t n, n_inliers;      /* |e|^2 <= thr^2, the reference's rule (:1088)                                           */
} lifcal_ba_group_stats;

/* (the structure carries the suffix _io: in C a typedef and a function cannot share the name lifcal_ba_residual_report) */
typedef struct lifcal_ba_residual_report_io {
  double inlier_threshold;             /* in */
  double* ex; double* ey;              /* [n_obs] or NULL, caller's observation order                                   */
  double* weight;                      /* [n_obs] or NULL: 1 / (1 + |e|^2 / loss_scale^2) if the config has the robust bit, else 1 */
  uint32_t* lens;                      /* [n_obs] or NULL: lens id of the observation, < n_lenses                        */
  double* lens_xy;                     /* [2 * n_lenses] or NULL: centre of lens id k                                    */
  lifcal_ba_group_stats* per_frame;    /* [n_frames] or NULL */
  lifcal_ba_group_stats* per_point;    /* [n_points] or NULL */
  lifcal_ba_group_stats* per_lens;     /* [n_lenses] or NULL (n_lenses: lifcal_ba_get_info)                              */
  lifcal_ba_group_stats total;         /* out */
  double seconds;                      /* out: device time of the call */
} lifcal_ba_residual_report_io;
int lifcal_ba_residual_report(lifcal_ba_handle* h, lifcal_ba_residual_report_io* io);

/* the same statistics for any grouping the caller chooses (sensor cells, depth bins, ...): key[i] < n_keys for every observation,
 * caller's order; out[n_keys].  The keys are checked on the host before anything is launched (LIFCAL_BA_ERR_INVALID_ARG). */
int lifcal_ba_residual_groups(lifcal_ba_handle* h, double inlier_threshold, uint32_t n_keys, const uint32_t* key, lifcal_ba_group_stats* out);

/* Host-only: the index the grouped sums walk, a stable counting sort.  off[n_keys + 1], idx[n]: idx[off[k] .. off[k + 1]) are the
 * positions i with key[i] == k, ascending.  LIFCAL_BA_ERR_INVALID_ARG for a key >= n_keys (or a null pointer). */
int lifcal_group_index(uint32_t n, uint32_t n_keys, const uint32_t* key, uint32_t* off, uint32_t* idx);

/* Poses held constant: fixed[f] != 0 keeps views[6f..6f+5] at their stored values in every following sweep / solve (ceres
 * SetParameterBlockConstant on that pose block: the frame's observations still constrain camera and points, its six columns
 * leave the reduced system).  fixed == NULL frees all poses again.  No reference counterpart; it is what the frame-windowed
 * driver below needs to carry finished frames into the next window (BASELINE configs[4] "streaming"). */
int lifcal_ba_set_fixed_frames(lifcal_ba_handle* h, const uint8_t* fixed /* [n_frames] or NULL */);

/* Frame-windowed ("streaming") bundle adjustment for long sequences (BASELINE configs[4]: recalib, 2000 frames): the frame axis is
 * cut into windows of `window_frames` frames that advance by window_frames - overlap_frames; each window is ONE ordinary problem
 * (its frames, the points they observe, the camera block with the caller's fixed_mask / bounds) created, solved and destroyed
 * in turn, so only one window is resident on the device.  From the second window on, the first overlap_frames poses — already
 * refined by the previous window — are held constant, and points whose observations all lie in earlier windows keep their
 * values.  Parameters are updated in place like lifcal_ba_solve; `per_window`, if not NULL, receives one summary per window
 * (capacity *n_windows on entry, count on return).  With world_size > 1 every window is sharded by 3D point as usual; the
 * collective hooks / communicator of `comm_template` (a handle created on the SAME options, may be NULL at world_size 1) are reused. */
typedef struct lifcal_ba_window_report {
  uint32_t first_frame, n_frames, n_fixed_frames, n_points, n_obs;
  uint32_t n_dropped_constraints;   /* distance constraints touching the window whose second point lies outside it (not applied) */
  lifcal_ba_summary summary;
} lifcal_ba_window_report;
int lifcal_ba_solve_windowed(const lifcal_ba_problem* p, const lifcal_ba_options* o, uint32_t window_frames, uint32_t overlap_frames,
                             lifcal_ba_handle* comm_template, lifcal_ba_window_report* per_window, uint32_t* n_windows);

/* re-upload cam/views/pts from the caller's arrays (e.g. to re-run from a new initial point) */
int lifcal_ba_upload_parameters(lifcal_ba_handle* h);
/* copy the device-resident cam/views/pts back into the caller's arrays */
int lifcal_ba_download_parameters(lifcal_ba_handle* h);

int lifcal_ba_set_allreduce(lifcal_ba_handle* h, lifcal_ba_allreduce_fn fn, void* ctx);
int lifcal_ba_set_allgather(lifcal_ba_handle* h, lifcal_ba_allgather_fn fn, void* ctx);
/* RCCL path: rank 0 calls unique_id (128 bytes), distributes it, every rank calls init */
int lifcal_ba_comm_unique_id(void* out128);
int lifcal_ba_comm_init_rccl(lifcal_ba_handle* h, const void* unique_id128);

/* introspection used by bench.py / tests */
typedef struct lifcal_ba_info {
  uint32_t n_obs_local, n_points_local, n_groups, n_tiles, n_lenses, n_reduced, n_promoted;
  uint32_t n_chunks, max_window_frames;
  uint64_t device_bytes;
  void* stream;          /* hipStream_t all kernels are launched on */
} lifcal_ba_info;
int lifcal_ba_get_info(lifcal_ba_handle* h, lifcal_ba_info* out);

/* One Levenberg-Marquardt step, read back (tests: the step is checked against the damped normal equations, not inferred from
 * parameters).  The last operation on the handle must have been lifcal_ba_sweep(h, radius, ...): the step is taken on that sweep's
 * S | rhs, at that radius.  Runs what an iteration of lifcal_ba_solve runs between its sweep and its decision — the linear solve of
 * the reduced system on the route create() chose, the candidate point (reduced part, back-substitution of the points), its cost —
 * and leaves the handle as a rejected step leaves it: parameters unchanged, candidate arrays written, the sweep's block consumed
 * (a second call without a new sweep is refused).  LIFCAL_BA_ERR_INVALID_ARG otherwise, and with world_size > 1. */
typedef struct lifcal_ba_step_out {
  double* delta_reduced;   /* [n_reduced] or NULL: canonical order of lifcal_ba_sweep_out; dead and fixed slots 0              */
  double* delta_points;    /* [3P] or NULL: step of every refined, observed point (eliminated or promoted), 0 elsewhere         */
  double* lambda_reduced;  /* [n_reduced] or NULL: the LM diagonal the step was damped with, same order; 0 on dead slots        */
  double* lambda_points;   /* [3P] or NULL: ... of the points, as delta_points                                                  */
  double gtd, ddd;         /* g . delta and sum lambda_i delta_i^2 over all columns: the model cost change is (ddd - gtd) / 2     */
  double step2, x2;        /* |x_candidate - x|^2 and |x|^2 over the blocks the step-size test counts                           */
  double cand_cost;        /* cost at x + delta                                                                                 */
  double chol_fail;        /* != 0: a pivot of the factorisation was not positive                                               */
  int32_t route;           /* 0 global-memory chain, 1 LDS chain, 2 two-ended (twisted) chain, 3 block odd-even reduction       */
  int32_t panel_in_lds;    /* route 0: the panel of the chain lives in LDS (1) or in global memory (0)                          */
} lifcal_ba_step_out;
int lifcal_ba_debug_step(lifcal_ba_handle* h, lifcal_ba_step_out* out);

void lifcal_ba_destroy(lifcal_ba_handle* h);
const char* lifcal_ba_strerror(int code);
const char* lifcal_ba_last_error(void);
const char* lifcal_ba_version(void);

/* Host-only planning (no device needed): the observation re-ordering create() performs.
 * Exposed so the CPU test-suite can check the layout invariants without a GPU. */
typedef struct lifcal_ba_plan_info {
  uint32_t n_groups, n_tiles, n_lenses, n_promoted, n_reduced, max_group_obs, n_chunks, max_window_frames;
} lifcal_ba_plan_info;
int lifcal_ba_plan(const lifcal_ba_problem* p, int32_t rank, int32_t world_size,
                   lifcal_ba_plan_info* info,
                   uint32_t* obs_order /* [n_obs] or NULL: sorted position -> input index, UINT32_MAX-padded */,
                   uint32_t* point_owner /* [n_points] or NULL: rank owning each point */);

/* The schedule of the LDS-window sweep that lifcal_ba_create builds for `rank` with default options in this environment (the same
 * decision code: LIFCAL_SWEEP_KERNEL, LIFCAL_SWEEP_WAVES, LIFCAL_V2_BLOCKS, LIFCAL_GROUP_SPLIT, LIFCAL_DISABLE_V2, LIFCAL_PLAN_COST,
 * LIFCAL_PLAN_BALANCE), as the planner's cost model sees it.  options.deterministic / options.precision = 1 set four waves per
 * role at create; this entry point takes no options.  pass_lanes is 256, or 128 with LIFCAL_SWEEP_WAVES=2.  Host-only.  `violations` is recounted from the finished layout arrays, not taken from the
 * planner's own bookkeeping: every regular point in exactly one pass, lanes and points of a pass within their caps, the lanes of a
 * pass sorted by frame (frame-ordered kernels), lane sizes adding up to the observations, a point's and a pass's group ids each one
 * contiguous run that no other point's groups share.  0 on a sound plan.  The block costs are those of the passes as built. */
typedef struct lifcal_ba_plan_statistics {
  uint32_t n_blocks, n_passes, pass_lanes, max_block_passes;
  uint64_t n_lanes;            /* lanes over all passes ((point, frame) pairs after splitting)                                   */
  uint64_t pass_steps;         /* sum over passes of the largest lane: observation steps the blocks walk                        */
  uint64_t tile_steps;         /* sum over the 64-lane tiles of their largest lane: rows of the padded observation payload      */
  uint64_t n_obs_window;       /* observations on the LDS-window path                                                           */
  uint64_t n_points_permuted;  /* regular points whose processing position differs from their first-frame position              */
  uint64_t violations;
  double block_cost_mean, block_cost_max;   /* modelled cost of a block (C_STEP steps + C_PASS + C_LANE lanes, summed over its passes) */
} lifcal_ba_plan_statistics;
int lifcal_ba_plan_stats(const lifcal_ba_problem* p, int32_t rank, int32_t world_size, lifcal_ba_plan_statistics* out);

/* Host-only: the same schedule tile by tile and pass by pass, for tests that need a scene to contain the edge cases of the window
 * kernels (a wave's observation loop over 0, 1, 2 or an odd number of rows; passes of one point and of the cap; the last tile's
 * clamped prefetch).  A tile is 64 consecutive lanes of a pass, its steps the rows of the padded observation payload it owns. */
typedef struct lifcal_ba_plan_shape_figures {
  uint64_t tiles_0_steps, tiles_1_step, tiles_2_steps, tiles_odd_steps /* odd and >= 3 */, tiles_even_steps /* even and >= 4 */;
  uint64_t ell_rows;           /* rows of 64 words the padded observation arrays hold (the payload's rows + padding)          */
  uint64_t max_row_read;       /* highest row any wave reads with its prologue and its clamped prefetch: must be < ell_rows   */
  uint64_t last_tile_row0;     /* first row of the last tile of the last block                                               */
  uint32_t last_tile_steps;
  uint32_t min_pass_points, max_pass_points;    /* points per pass (np): at most 64                                          */
  uint32_t min_block_passes, max_block_passes;
  uint32_t reserved;
} lifcal_ba_plan_shape_figures;
int lifcal_ba_plan_shape(const lifcal_ba_problem* p, int32_t rank, int32_t world_size, lifcal_ba_plan_shape_figures* out);

/* ---- shard-local problems (multi-GPU without handing every rank the whole observation list) ----
 * lifcal_ba_create takes the WHOLE problem on every rank and keeps the observations of the points the rank owns.  For long
 * sequences (BASELINE configs[3], configs[4]) a launcher can instead partition ONCE from the index arrays alone (pt, fr: 8 bytes
 * per observation) with lifcal_ba_partition, hand each rank only the observations of its points, and create the rank's handle
 * with lifcal_ba_create_shard.  The resulting layout, kernels and collectives are those of lifcal_ba_create.
 * Host-only, no device needed for the partition.  Distance constraints are not supported on shards (they couple points across
 * ranks: use lifcal_ba_create). */
typedef struct lifcal_ba_partition {
  uint32_t world_size, n_frames, n_points, band_width;   /* band_width: max over points of (last frame - first frame)          */
  uint64_t n_obs;                                        /* observations of the whole problem                                   */
  int32_t*  point_owner;    /* [n_points] caller-allocated: rank owning the point, -1 = not observed                            */
  uint32_t* rank_first;     /* [world_size] caller-allocated: first frame observed by the rank's points                         */
  uint32_t* rank_frames;    /* [world_size] caller-allocated: number of frames from rank_first to the last frame they observe   */
  uint64_t* rank_obs;       /* [world_size] caller-allocated: observations of the rank's points                                 */
  uint8_t*  frame_used;     /* [n_frames] caller-allocated: frame observed by any point                                         */
} lifcal_ba_partition;
/* fills the caller-allocated arrays of `part` (world_size must be set) from the index arrays of the whole problem: only p->n_obs,
 * n_frames, n_points, pt and fr are read.  Same ownership rule as lifcal_ba_create (points in first-frame order, contiguous
 * ranges balanced by observation count). */
int lifcal_ba_partition_points(const lifcal_ba_problem* index_only, lifcal_ba_partition* part);
/* `local` holds ONLY the observations of the points `rank` owns (any order), but the full cam / views / pts arrays (pts of other
 * ranks' points are neither read nor written until the final gather). */
int lifcal_ba_create_shard(const lifcal_ba_problem* local, const lifcal_ba_partition* part, const lifcal_ba_options* o, lifcal_ba_handle** out);
/* host-only planning of a shard (what lifcal_ba_plan is for whole problems): the CPU test-suite compares the two */
int lifcal_ba_plan_shard(const lifcal_ba_problem* local, const lifcal_ba_partition* part, int32_t rank, lifcal_ba_plan_info* info);

/* ---- start values of the plenoptic parameters ----
 * Replaces reference src/CameraCalibration.cpp:456-499 (CameraCalibration::initPlenopticParameters): with
 * bL = fL z / (z - fL), z the camera-frame depth of the object point of an image point, the linear model
 * bL = v B + bL0 (v = virtual depth) is fitted over all image points of all frames in the least-squares sense; a row is
 * dropped (zeroed, as the reference does) when v < 2 or bL < 0.  The reference solves with Eigen::JacobiSVD, i.e. the
 * minimum-norm solution with singular values below 2 eps sigma_max treated as zero; so does this.
 * Inputs are plain host arrays, one entry per image point in the reference's frame-major order (any order works).  The
 * sums run on the device (one reduction kernel), the 2x2 solve on the host. */
typedef struct lifcal_init_problem {
  uint64_t n;                 /* image points over all frames (reference: sum of frames[i].imageCoordinates.size())      */
  const double* vdepth;       /* [n] virtual depth of the point (reference virtualDepthValues[i][p])                      */
  const uint32_t* fr;         /* [n] frame of the point                                                                    */
  const uint32_t* pt;         /* [n] index of its object point (reference objectCoordinatesByID[p] - p3d_w.data())        */
  uint32_t n_frames, n_points;
  const double* world_to_cam; /* [n_frames][16] COLUMN-major, as Eigen::Matrix4d frame::worldToCam stores it              */
  const double* pts;          /* [n_points][3]                                                                             */
  double fL_init;             /* fPH_init * pixelSize_totFoc (reference :460)                                              */
} lifcal_init_problem;
typedef struct lifcal_init_result {
  double B_init, bL0_init;    /* x[0], x[1] of the reference (:492-493)                                                    */
  uint64_t n_used;            /* rows that entered the fit                                                                 */
  int32_t rank;               /* numerical rank of the n x 2 system (2 unless degenerate)                                  */
  int32_t reserved;
} lifcal_init_result;
int lifcal_init_plenoptic(const lifcal_init_problem* p, int32_t device, lifcal_init_result* out);
/* Replaces reference src/CameraCalibration.cpp:503-512 (CameraCalibration::initPlenopticParametersRecalibration): recalib mode takes fL
 * and B from the previous calibration (calibData->getFixedParameters) and starts bL0 at fL - 2 B.  Host arithmetic, no device. */
int lifcal_init_plenoptic_recalibration(double fL_fixed, double B_fixed, lifcal_init_result* out);

#ifdef __cplusplus
}
#endif
#endif /* LIFCAL_BA_H */
