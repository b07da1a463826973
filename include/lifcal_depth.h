/* lifcal_depth.h — C ABI of the two ends of the virtual-depth data flow: reading virtual depth out of the
 * 16-bit depth images, and turning (x_v, y_v, virtual depth) into metric 3D through the calibrated camera.  Same shared library as
 * include/lifcal_ba.h (liblifcal_ba.so), same error codes and lifcal_ba_last_error().
 *
 * Replaces, in the reference:
 *   CameraCalibration::readDepthData (per image point)   src/CameraCalibration.cpp:385-448   -> lifcal_depth_sample
 *   CameraModel::projectPointBack                        src/CameraModel.h:26-81             -> lifcal_depth_back_project_points
 *   its use on the image points of a frame               src/CameraCalibration.cpp:1274-1285
 * and adds the dense form (every pixel of a depth map, lifcal_depth_back_project_maps) and, in parts (d)-(f), the forward model and
 * the maps of several frames against each other (check and fusion).  The PNG files stay with the caller (the
 * Python side decodes them); a map here is the decoded image: [height][width] uint16, row-major, pixel (col, row) is the
 * virtual-image point (x_v, y_v) = (col, row).
 *
 * Arithmetic.  The sampler and the fp64 back-projection repeat the reference's IEEE double operations in its order, without fused
 * multiply-add: results are bit-identical to a line-by-line restatement.  The undistortion inside projectPointBack is the
 * reference's fixed-point iteration with its fixed TEN sweeps, no convergence test: its accuracy is that of the reference (about
 * 1e-16 of Z at the project's default distortion, about 5e-12 at twenty times that distortion, where ten sweeps have not converged).
 * Derivatives are those of the iteration as executed (forward mode through the ten sweeps), not of the implicit inverse.
 *
 * Uncertainty.  cov_pc / sigma_z propagate the camera covariance G that lifcal_ba_covariance writes to out->camera.  A propagated
 * variance is meaningful only for quantities that do not move along the null directions lifcal_ba_covariance reports
 * (out->camera_null): in a scene without distance constraints B and bL0 are not determined on their own,
 * and metric depth depends on exactly that direction.  Check |J n| for every null direction n (the Python side has
 * depth_is_estimable for it) before trusting the numbers.
 *
 * Everything runs on the GPU; there is no CPU fallback (LIFCAL_BA_ERR_NO_DEVICE without a gfx950 device).  One rank.
 */
#ifndef LIFCAL_DEPTH_H
#define LIFCAL_DEPTH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct lifcal_depth_handle lifcal_depth_handle;

/* A handle owns max_maps depth maps of width x height on the device (all zero, i.e. all invalid, until set). */
int lifcal_depth_create(int32_t width, int32_t height, int32_t max_maps, int32_t device, lifcal_depth_handle** out);
void lifcal_depth_destroy(lifcal_depth_handle* h);
/* maps: count * height * width values for maps first .. first+count-1; on_device != 0: `maps` is a device pointer on the
 * handle's device (e.g. a torch tensor), copied device to device.  LIFCAL_BA_ERR_OUT_OF_RANGE when the range leaves max_maps. */
int lifcal_depth_set_maps(lifcal_depth_handle* h, int32_t first, int32_t count, const uint16_t* maps, int32_t on_device);

/* ---- (a) readDepthData for already decoded images, one lane per image point ----
 * pixel = ((int)(x + 0.5), (int)(y + 0.5)), C truncation.  A raw value is valid when value > 0 and iv = 1 - value / 65535 lies
 * in (0, 0.5]; a valid centre pixel gives 1 / iv.  Otherwise windows of half-width dist = 1 .. 49, clipped to the image, are
 * summed (x outer, y inner) until one holds at least ten valid values: the result is count / sum of iv.  -1.0 when dist = 49 fails.
 * The reference reads out of bounds for a centre pixel outside the image; here such a point gives -1.0 and counts as failed. */
typedef struct lifcal_depth_sample_counts {
  uint64_t direct, interpolated, failed;
} lifcal_depth_sample_counts;
/* host arrays of length n; map_index[i] in [0, max_maps), else LIFCAL_BA_ERR_OUT_OF_RANGE; counts may be NULL */
int lifcal_depth_sample(lifcal_depth_handle* h, uint64_t n, const double* x, const double* y, const int32_t* map_index, double* vdepth,
                        lifcal_depth_sample_counts* counts);

/* The camera as storeResults hands it to projectPointBack (src/CameraCalibration.cpp:1107-1116): cam in the layout of
 * lifcal_ba_problem.cam, used as stored (no sign folding, cx / cy in virtual-image pixels); config: the nRadial and tangential bits
 * of the lifcal_ba config mask (the other bits are ignored); spx, spy: pixelSize_totFoc. */
typedef struct lifcal_depth_camera {
  double cam[17];
  double spx, spy;
  uint32_t config;
  uint32_t reserved;
} lifcal_depth_camera;

/* ---- (b) projectPointBack for a list of image points, fp64 ---- */
typedef struct lifcal_depth_points {
  uint64_t n;
  const double* x;        /* [n] x_v */
  const double* y;        /* [n] y_v */
  const double* vdepth;   /* [n]; vdepth <= 0 (a failed sample) gives NaN in every output of the point and is counted */
  const uint32_t* fr;     /* [n] frame of the point, or NULL */
  const double* views;    /* [6 n_frames] {ax, ay, az, tx, ty, tz} as in lifcal_ba_problem.views, or NULL */
  uint32_t n_frames;
  uint32_t reserved;
  const double* cam_cov;  /* [17 * 17] row-major (lifcal_ba_covariance out->camera), needed for cov_pc */
  double sigma_v;         /* 1-sigma of the virtual depth, 0: none */
  double* p_c;            /* [3n] out: camera coordinates */
  double* p_w;            /* [3n] out or NULL: R^T (p_c - t), (R, t) = RigidBody::getTransformationMatrix(views[fr]); needs fr and views */
  double* jac;            /* [n][3][17] out or NULL: d p_c / d cam slot; dead or absent slots are zero */
  double* dpc_dv;         /* [n][3] out or NULL: d p_c / d vdepth */
  double* cov_pc;         /* [n][6] out or NULL: upper triangle (xx, xy, xz, yy, yz, zz) of J G J^T + sigma_v^2 (dp/dv)(dp/dv)^T */
  uint64_t n_invalid;     /* out: points with vdepth <= 0 */
} lifcal_depth_points;
int lifcal_depth_back_project_points(int32_t device, const lifcal_depth_camera* cam, lifcal_depth_points* io);

/* ---- (c) the dense path: every pixel of maps first .. first+count-1 ----
 * A pixel is decoded by the direct rule of (a) only (no interpolation); an invalid pixel gives NaN in every output and is counted.
 * eval 0: fp64 in the reference's order as in (b), bit-identical to it (float outputs are its float32 rounding).
 * eval 1: fp32 evaluation with the x / y components as packed pairs; deviates from eval 0 by the float32 rounding of the chain.
 * z = fL b / (b - fL), b = bL0 + v B; sigma_z^2 = g G3 g^T + (dz/dv)^2 sigma_v^2 with g = dz / d(fL, bL0, B) and G3 that block of
 * cam_cov (both evaluated in fp64 under eval 0, in fp32 under eval 1). */
typedef struct lifcal_depth_maps {
  int32_t first, count;
  int32_t eval;            /* 0: fp64, 1: fp32 */
  int32_t out_double;      /* 0: outputs are float (the result PLYs are `property float`), 1: double */
  int32_t out_on_device;   /* 0: xyz / z / sigma_z are host pointers, 1: device pointers on the handle's device, 16-byte aligned */
  uint32_t n_frames;
  const uint32_t* frame;   /* [count] host: frame of each map, or NULL; with views: outputs xyz in WORLD coordinates */
  const double* views;     /* [6 n_frames] host, or NULL */
  const double* cam_cov;   /* [17 * 17] host, needed for sigma_z */
  double sigma_v;
  void* xyz;               /* [count][height][width][3] or NULL */
  void* z;                 /* [count][height][width] or NULL: camera-frame depth (also when xyz is in world coordinates) */
  void* sigma_z;           /* [count][height][width] or NULL */
  uint64_t n_invalid;      /* out */
  double seconds;          /* out: device time of the kernel (HIP events) */
} lifcal_depth_maps;
int lifcal_depth_back_project_maps(lifcal_depth_handle* h, const lifcal_depth_camera* cam, lifcal_depth_maps* io);

/* ---- (d) the forward model: what projectPointBack inverts, in closed form, fp64, one lane per point ----
 * With fr and views (they go together) p are world points and p_c = R p + t; without them p are camera coordinates.
 *   x_u = X / Z * bL0, y_u likewise; delta = radialDistortion(x_u, y_u) + tangentialDistortion(x_u, y_u) (src/CameraModel.h:205-241)
 *   b = fL Z / (Z - fL), v = (b - bL0) / B, x_v = (x_u + delta_x) (bL0 + v B) / bL0 / spx + cx, y_v likewise with spy, cy.
 * A point is invalid when a coordinate is not finite, Z <= 0, Z == fL or v is not > 0: NaN in x, y, vdepth, counted in n_invalid. */
typedef struct lifcal_depth_forward {
  uint64_t n;
  const double* p;        /* [3n] */
  const uint32_t* fr;     /* [n] frame of the point, or NULL */
  const double* views;    /* [6 n_frames], or NULL */
  uint32_t n_frames;
  uint32_t reserved;
  double* x;              /* [n] out: x_v */
  double* y;              /* [n] out: y_v */
  double* vdepth;         /* [n] out */
  uint64_t n_invalid;     /* out */
} lifcal_depth_forward;
int lifcal_depth_project_points(int32_t device, const lifcal_depth_camera* cam, lifcal_depth_forward* io);

/* ---- (e) every map of a batch against its neighbours ----
 * Source map s is checked against the targets t of the batch with 0 < |t - s| <= span.  Per valid source pixel (direct rule) and
 * target: back-project as in (c), go into the target's camera (RT_t RT_s^-1), apply (d) -> (x_t, y_t, v_pred), take the target
 * pixel ((int)(x_t + 0.5), (int)(y_t + 0.5)) (C truncation, outside the image as in lifcal_depth_sample), decode it by the direct
 * rule -> v_obs, e = 1 / v_obs - 1 / v_pred.  Classes:
 *   no data      (d) invalid, or the target pixel outside the image or invalid
 *   consistent   |e| <= tol_iv
 *   occluded     e < -tol_iv  (the target sees something nearer)
 *   violation    e >  tol_iv  (the target sees through the point)
 * sum_e / sum_e2 are formed per workgroup in a fixed tree and the workgroups are added in ascending order: two calls give the
 * same bits. */
typedef struct lifcal_depth_pair_stats {
  uint64_t n_valid;        /* valid pixels of the source map */
  uint64_t n_compared;     /* of these: consistent + occluded + violation */
  uint64_t n_consistent, n_occluded, n_violation;
  double sum_e, sum_e2;    /* over the consistent pixels */
} lifcal_depth_pair_stats;

typedef struct lifcal_depth_views {
  int32_t first, count;    /* maps first .. first+count-1 of the handle, count >= 1 */
  uint32_t span;           /* 1 .. 127 */
  int32_t out_on_device;   /* 0: support / conflict / pair are host pointers, 1: device pointers on the handle's device */
  uint32_t n_frames;
  uint32_t reserved;
  const uint32_t* frame;   /* [count] host: frame of each map */
  const double* views;     /* [6 n_frames] host */
  double tol_iv;           /* >= 0, in inverse virtual depth; one raw step is 1 / 65535 */
  uint8_t* support;        /* [count][height][width] or NULL: targets in class consistent; 0 on invalid source pixels */
  uint8_t* conflict;       /* [count][height][width] or NULL: targets in class violation */
  lifcal_depth_pair_stats* pair;   /* [count][2 span] or NULL: slot j of source s is target s + j - span for j < span and
                                      s + j - span + 1 otherwise; slots whose target lies outside the batch are all zero */
  double seconds;          /* out: device time (HIP events) */
} lifcal_depth_views;
int lifcal_depth_check_maps(lifcal_depth_handle* h, const lifcal_depth_camera* cam, lifcal_depth_views* io);

/* ---- (f) one cloud from a batch of maps ----
 * A source pixel emits one point when it is valid, support >= min_support, conflict <= max_conflict (both as in (e), the pixel's
 * own counts) and no target with a smaller map index is consistent with it (it defers to the lower map).  The point is
 * sum w_k p_k / sum w_k over the pixel's own world point and the world points of the target pixels it was consistent with (the
 * sampled pixel's centre with its own v_obs through the target's pose), added in ascending t, with
 * w = 1 / (g v^2)^2, g = dz/dv = -B fL^2 / (b - fL)^2, b = bL0 + v B: the inverse variance of z for noise uniform in 1 / v.
 * Points come out in ascending src, two calls give the same bits.  n_points is the number that qualified; when capacity is
 * smaller the first `capacity` are written and the call still returns LIFCAL_BA_OK. */
typedef struct lifcal_depth_fusion {
  int32_t first, count;
  uint32_t span;
  int32_t out_on_device;   /* 0: xyz / n_merged / src are host pointers, 1: device pointers on the handle's device */
  uint32_t n_frames;
  int32_t out_double;      /* 0: xyz is float, 1: double */
  const uint32_t* frame;   /* [count] host */
  const double* views;     /* [6 n_frames] host */
  double tol_iv;
  uint32_t min_support, max_conflict;
  uint64_t capacity;       /* points xyz / n_merged / src have room for; 0: count only */
  void* xyz;               /* [capacity][3] world coordinates */
  uint8_t* n_merged;       /* [capacity] or NULL: 1 + support */
  uint32_t* src;           /* [capacity] or NULL: (m - first) height width + row width + col */
  uint64_t n_points;       /* out */
  double seconds;          /* out */
} lifcal_depth_fusion;
int lifcal_depth_fuse_maps(lifcal_depth_handle* h, const lifcal_depth_camera* cam, lifcal_depth_fusion* io);

#ifdef __cplusplus
}
#endif
#endif
