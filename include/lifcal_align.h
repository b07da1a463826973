/* lifcal_align.h — C ABI of the scene alignment: the similarity or rigid motion that carries points of a scene
 * onto given coordinates, and its application to poses and points.  Host code only (no GPU needed), same shared library as
 * include/lifcal_ba.h.
 *
 * A prior on a 3D point (include/lifcal_prior.h) is usable when the start values already live in the frame of the control points.
 * A registered scene lives in its anchor frame, a COLMAP model in an arbitrary similarity frame: lifcal_align_fit finds
 * to ~ s R from + t from the control points' current and given coordinates, lifcal_align_apply moves the whole scene.
 */
#ifndef LIFCAL_ALIGN_H
#define LIFCAL_ALIGN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct lifcal_alignment {
  double scale, R[9], t[3];   /* to ~ scale * R from + t, R row-major */
  double rms;                 /* sqrt(sum w |to - scale R from - t|^2 / sum w) over the points used */
  uint32_t n_used, reserved;  /* points with a positive weight */
} lifcal_alignment;

/* Weighted least squares in closed form (Horn 1987, unit quaternion as the eigenvector of the 4 x 4 matrix of the cross sums; the
 * scale is the one that minimises the residual for that rotation).  from, to: [3n]; w: [n] weights or NULL for unit weights, points
 * with w <= 0 are left out; with_scale == 0 forces scale = 1.  Sums run in index order in extended precision.
 * LIFCAL_BA_ERR_INVALID_ARG: a null pointer, fewer than three points with a positive weight, collinear points on either side (the
 * second-largest eigenvalue of the centred scatter of `from` or of `to` below 1e-12 of the largest), a non-finite input. */
int lifcal_align_fit(uint32_t n, const double* from, const double* to, const double* w, int32_t with_scale, lifcal_alignment* out);

/* In place.  Points: P' = s R P + t.  Poses (views: [6 n_frames] ax ay az tx ty tz, camera = R_f world + t_f): R_f' = R_f R^T,
 * t_f' = s t_f - R_f' t, so that every camera-frame coordinate is scaled by s and every projection keeps its place; the angles are
 * the Euler angles (0, 1, 2) of R_f', first angle in [0, pi], as the COLMAP ingestion extracts them.  Either array may be NULL with
 * a count of 0. */
int lifcal_align_apply(const lifcal_alignment* a, uint32_t n_frames, double* views, uint64_t n_points, double* pts);

#ifdef __cplusplus
}
#endif
#endif /* LIFCAL_ALIGN_H */
