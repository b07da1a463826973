/* lifcal_verify.h — geometric verification of feature matches: a batched rigid RANSAC over the pairs of
 * frames that lifcal_features_match matched.  Every feature of a plenoptic camera has a virtual depth, so it is a metric point
 * in its camera's frame (lifcal_depth_back_project_points), and two frames of a rigid scene are related by one rigid motion of
 * those points; three matches determine it in closed form.  Same shared library as include/lifcal_ba.h (liblifcal_ba.so), same
 * error codes and lifcal_ba_last_error().  Argument checks come first and need no device; the scoring of the hypotheses and the
 * classification of the matches run on the GPU and have no CPU fallback (LIFCAL_BA_ERR_NO_DEVICE without a gfx950 device); the
 * refit is host code (lifcal_align_fit).
 *
 * The rule, exactly.  Doubles are IEEE without fused multiply-add, evaluated in the order written; square roots and divisions
 * are correctly rounded.  A sum of three terms is (a + b) + c; a . b = (a0 b0 + a1 b1) + a2 b2; |a|^2 = a . a;
 * a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0); (R p)_r = (R[r][0] p0 + R[r][1] p1) + R[r][2] p2.  Apart from the
 * refit's transform, two calls give the same bytes, equal to those of the numpy restatement in tests/verify_reference.py; the
 * refit is deterministic too (fixed sweep order), so two calls of one build agree in every byte.
 *
 * Usable.  A feature is usable when xyz[0..2], tol_lat and tol_dep are finite, xyz[2] > 0 and both tolerances are > 0; a match
 *   when both of its features are.  u_0 .. u_(m-1) are the usable matches of a pair in their order, p_a(k), p_b(k) their points
 *   in frame a and frame b.  m < 3: status FEW.
 * Sampling.  Hypothesis h of pair p starts a 32-bit state at  s = seed + 0x9E3779B9 (p + 1) + 0x85EBCA6B (h + 1)  (mod 2^32).  A
 *   draw is  s = 1664525 s + 1013904223 (mod 2^32), then the value ((uint64)s m) >> 32.  k0 = a draw; k1 = a draw, repeated while
 *   k1 == k0; k2 = a draw, repeated while k2 == k0 or k2 == k1.  q_i = p(k_i) on each side.
 * Triad, on each side.  d1 = q1 - q0, d2 = q2 - q0, n = d1 x d2.  The hypothesis is invalid (it counts no inlier and cannot be
 *   chosen) unless |n|^2 > (1e-6 |d1|^2) |d2|^2 on both sides and all of R and t below are finite.
 *   e1 = d1 / sqrt(|d1|^2), e3 = n / sqrt(|n|^2) (component by component), e2 = e3 x e1.
 * Transform.  R[r][c] = (e1b[r] e1a[c] + e2b[r] e2a[c]) + e3b[r] e3a[c];  c = ((q0 + q1) + q2) / 3.0 on each side;
 *   t = cb - R ca.
 * Inlier test of a usable match under (R, t).  e = ((R p_a) + t) - p_b;  r = p_b / sqrt(|p_b|^2);  e_par = e . r;
 *   e_perp = sqrt(max(0, |e|^2 - e_par e_par));  Td = tol_dep_i + tol_dep_j, Tl = tol_lat_i + tol_lat_j;
 *   inlier when |e_par| <= Td and e_perp <= Tl.
 * Choice.  Of the valid hypotheses the one with the most inliers, of equals the lowest h.  None valid: status DEGENERATE.
 * Refinement, up to `refine` rounds.  lifcal_align_fit(from = p_a, to = p_b of the current inliers in their order,
 *   w = 1 / (Td Td), with_scale = 0); a failed fit (collinear points, fewer than three) ends the rounds.  The matches are
 *   classified again under the fitted (R, t); when that counts at least as many inliers as before, the new transform and its
 *   classification stay and rounds_used grows by one, otherwise the rounds end with the previous ones.
 * Acceptance.  With n = the final count: status REJECTED when n < min_inliers or (double)n < min_ratio (double)m, else OK.
 * Output.  keep = inlier under the final transform, and 0 throughout a pair whose status is not OK.  e_par, e_perp: under the
 *   final transform; NaN for a match that is not usable and throughout a pair FEW or DEGENERATE.
 *   rms = sqrt(S / (double)n), S = the sum over the final inliers, in their order, of (e_par e_par + e_perp e_perp); 0 when n = 0.
 */
#ifndef LIFCAL_VERIFY_H
#define LIFCAL_VERIFY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define LIFCAL_VERIFY_OK 0
#define LIFCAL_VERIFY_FEW 1          /* fewer than 3 usable matches */
#define LIFCAL_VERIFY_DEGENERATE 2   /* no valid hypothesis */
#define LIFCAL_VERIFY_REJECTED 3     /* too few inliers */
#define LIFCAL_VERIFY_NO_HYPOTHESIS 0xffffffffu

/* per feature of the concatenated list: frame f holds offset[f] .. offset[f+1] - 1, as in lifcal_features_set.  Host pointers. */
typedef struct lifcal_verify_points {
  uint32_t n_frames, reserved;
  const uint32_t* offset;   /* [n_frames + 1], offset[0] = 0, not descending, offset[n_frames] < 2^31 */
  const double* xyz;        /* [offset[n_frames]][3] camera-frame coordinates, mm */
  const double* tol_lat;    /* [offset[n_frames]] tolerance across the viewing ray, mm */
  const double* tol_dep;    /* [offset[n_frames]] tolerance along the viewing ray, mm */
} lifcal_verify_points;

/* 0 (0.0) in a field selects its default */
typedef struct lifcal_verify_options {
  uint32_t hypotheses;   /* a multiple of 256, up to 4096; default 256 */
  uint32_t seed;         /* seed of the sampling */
  int32_t min_inliers;   /* >= 1; default 8 */
  int32_t refine;        /* refit rounds, 1 .. 4; default 2; a negative value: none */
  double min_ratio;      /* in [0, 1]; default 0.25 */
} lifcal_verify_options;

/* one row per pair, 136 bytes without padding */
typedef struct lifcal_verify_pair {
  uint32_t status;
  uint32_t n_matches, n_usable;
  uint32_t best_hypothesis;        /* LIFCAL_VERIFY_NO_HYPOTHESIS when FEW or DEGENERATE */
  uint32_t n_inliers_hypothesis;   /* its count, from the scoring stage */
  uint32_t n_inliers;              /* the final count */
  uint32_t rounds_used;            /* refits that were kept */
  uint32_t reserved;
  double R[9], t[3];               /* p_b ~ R p_a + t, R row-major; zeros when FEW or DEGENERATE */
  double rms;
} lifcal_verify_pair;

/* the arrays per match are indexed like mi and mj: pair_start[n_pairs] entries each */
typedef struct lifcal_verify_result {
  uint8_t* keep;
  double* e_par;
  double* e_perp;
  lifcal_verify_pair* pair;   /* [n_pairs] */
  double seconds;             /* out: device time of the kernels (HIP events) */
} lifcal_verify_result;

/* Host only: exactly the checks lifcal_matches_verify makes of its arguments.  pairs, pair_start, mi, mj as
 * lifcal_features_match took and wrote them.  LIFCAL_BA_ERR_INVALID_ARG for a null pointer, a frame or feature index out of
 * range, a pair (a, a), a pair_start that descends, or an option outside its range; LIFCAL_BA_ERR_OUT_OF_RANGE for 2^31 matches
 * and more.  Nothing outside the arrays is read.  options and resolved (the options with the defaults filled in; refine < 0
 * comes back as -1) may be NULL. */
int lifcal_matches_verify_check(const lifcal_verify_points* pts, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start,
                                const uint32_t* mi, const uint32_t* mj, const lifcal_verify_options* options, lifcal_verify_options* resolved);

int lifcal_matches_verify(const lifcal_verify_points* pts, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start,
                          const uint32_t* mi, const uint32_t* mj, int32_t device, const lifcal_verify_options* opt, lifcal_verify_result* out);

#ifdef __cplusplus
}
#endif
#endif
