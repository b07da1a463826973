/* lifcal_markers.h — fiducial markers in total-focus images: square binary markers of a caller's dictionary
 * are detected, decoded and centred, so that a marker's id can serve as a point id and its centre as an image point (the
 * reference's doCalibration_aruco_calib), and the host pieces that go with it: the constraints file, start values for the marker
 * points and the scale of the scene from the first constraint.  Same shared library as include/lifcal_ba.h (liblifcal_ba.so),
 * same error codes and lifcal_ba_last_error().  Argument checks come first and need no device; detection runs on the GPU and
 * has no CPU fallback (LIFCAL_BA_ERR_NO_DEVICE without a gfx950 device).
 *
 * The algorithm, exactly.  Image arithmetic is integer (int64); doubles are IEEE without fused multiply-add, evaluated in the
 * order written, with parentheses as written and otherwise left to right.  Two calls give the same bytes, equal to those of the
 * numpy restatement in tests/markers_reference.py.  I(x, y) is the image, x = column, y = row, pixel centres at integers;
 * full = 2^bits - 1.  Valid pixel: status 0 or 3; without a status map every pixel is valid.
 *
 * 1. Dark map.  sum(x, y), n(x, y) = the sum of I and the number of pixels over the (2w+1)^2 window about (x, y) clipped to the
 *   image (every pixel of the image counts, valid or not).  C = contrast (full + 1) / 256.
 *     dark(x, y)  <=>  (x, y) is valid  and  n I(x, y) + n C < sum.
 *   Large dark areas are hollowed; only the ring along a marker's outer edge has to stay connected.
 *
 * 2. Components.  The 8-connected components of the dark pixels.  label(x, y) = the lowest linear index y width + x of the
 *   pixel's component, -1 for a pixel that is not dark.  Per component: the area (pixels), and the eight extreme pixels for the
 *   projections, in this order:  min x, max x, min y, max y, min x+y, max x+y, min x-y, max x-y;  of tied pixels the one with the
 *   lowest linear index.  The box is x0 = min x, x1 = max x, y0 = min y, y1 = max y (inclusive); its sides are x1 - x0 + 1 and
 *   y1 - y0 + 1.
 *
 * 3. Candidates, by ascending label: area >= min_area;  both box sides >= min_side and <= max_side;  x0 >= 1, y0 >= 1,
 *   x1 <= width - 2, y1 <= height - 2.  max_candidates = width height / min_area (integer division) always suffices.
 *
 * 4. Quad.  Two corner sets of extreme pixels, both clockwise in the image (y down):
 *     diagonal set:  min x+y,  max x-y,  max x+y,  min x-y;      axis set:  min y,  max x,  max y,  min x.
 *   A2 = sum over i of (x_i y_{i+1} - x_{i+1} y_i), indices mod 4, in integers.  The set with the larger A2 wins, a tie goes to
 *   the diagonal set; A2 < min_side^2 rejects the candidate.  With S = the sum of the four corners (per axis), corner pixel
 *   (px, py) becomes the point  (px + 0.5 sign(4 px - Sx),  py + 0.5 sign(4 py - Sy)),  sign(0) = 0.  These are q_0 .. q_3.
 *
 * 5. Decode.  m = marker_bits, n = m + 2.  The unit square goes onto the quad, (0,0) -> q_0, (1,0) -> q_1, (1,1) -> q_2,
 *   (0,1) -> q_3, by (Heckbert), with (x_i, y_i) = q_i:
 *     dx1 = x1 - x2,  dx2 = x3 - x2,  sx = ((x0 - x1) + x2) - x3,  the same in y;   den = dx1 dy2 - dy1 dx2  (0 rejects);
 *     g = (sx dy2 - sy dx2) / den,   h = (dx1 sy - dy1 sx) / den,
 *     a = (x1 - x0) + g x1,  b = (x3 - x0) + h x3,  c = x0,   d = (y1 - y0) + g y1,  e = (y3 - y0) + h y3,  f = y0;
 *     w = (g u + h v) + 1.0   (not w > 0 rejects),   X = ((a u + b v) + c) / w,   Y = ((d u + e v) + f) / w.
 *   Cell (r, c), r = row along v, c = column along u, is sampled at the 3 x 3 positions  u = ((c + 0.25) + (0.5 (bu + 0.5)) / 3.0) / n,
 *   v = ((r + 0.25) + (0.5 (bv + 0.5)) / 3.0) / n,  bu, bv = 0, 1, 2.  A sample at (X, Y):  not |X| < 2^20 or not |Y| < 2^20
 *   rejects;  Sx = floor(64.0 X + 0.5), Sy likewise, as integers;  ix = Sx >> 6, fx = Sx & 63 (arithmetic), iy, fy likewise;
 *   ix < 0, ix + 1 > width - 1, iy < 0 or iy + 1 > height - 1 rejects the candidate;  the value is the integer bilinear form of
 *   lifcal_rawdepth.h, 4096 x a grey level:
 *     (64-fx)(64-fy) I(ix,iy) + fx (64-fy) I(ix+1,iy) + (64-fx) fy I(ix,iy+1) + fx fy I(ix+1,iy+1).
 *   (Validity plays no part from here on.)  V(r, c) = the sum of the cell's nine values;  lo, hi = the least and largest V.
 *   C_cell = cell_contrast (full + 1) / 256;  hi - lo < 9 * 4096 * C_cell rejects.  A cell is white  <=>  2 V > lo + hi.
 *   More than max_border_errors white cells among the 4 (n - 1) cells with r or c in {0, n - 1} rejects.
 *   Word: bit (r - 1) m + (c - 1) is set when the inner cell (r, c) is white, r, c = 1 .. m.
 *   Rotation of a word B (as an m x m grid, bit r m + c = B[r][c]) by 90 degrees clockwise:  rot(B)[r][c] = B[m-1-c][r];
 *   rot_k = rot applied k times.  Over all dictionary words j and k = 0 .. 3:  D(j, k) = popcount(word xor rot_k(dict_j)); the
 *   least D wins, ties go to the lowest j, then the lowest k;  D > max_correction rejects.  id = j, rotation = k, hamming = D.
 *   The marker's corners are  p_i = q_{(i + k) mod 4}: p_0 is the marker's own top-left, clockwise.
 *
 * 6. Sub-pixel edges.  Edge e runs from A = p_e to B = p_{(e+1) mod 4}.  dx = Bx - Ax, dy = By - Ay, L = sqrt(dx dx + dy dy),
 *   the outward normal is (nx, ny) = (dy / L, (-dx) / L); an edge with L = 0 has no crossing.  Station k = 0 .. 11:  s = 0.15 + (0.7 (k + 0.5)) / 12.0,
 *   P = (Ax + s dx, Ay + s dy).  Sample i = 0 .. 16 at offset o_i = -4.0 + 0.5 i:  (X, Y) = (Px + o_i nx, Py + o_i ny), rounded
 *   and read as in step 5, value v_i; a sample that step 5 would reject on is skipped instead.  With T = lo + hi of step 5,
 *   neighbours i, i + 1, neither skipped, hold a crossing when  18 v_i < T <= 18 v_{i+1};  its offset is
 *     o = o_i + 0.5 ((double)(T - 18 v_i) / (double)(18 v_{i+1} - 18 v_i)).
 *   Of a station's crossings the one with the least |o| wins (of equals the lowest i); its point is (Px + o nx, Py + o ny).
 *   An edge needs at least 4 stations with a crossing.  Its line, from those points in station order, N of them:
 *     mx = (sum x) / N, my likewise;  sxx = sum (x - mx)(x - mx),  sxy = sum (x - mx)(y - my),  syy = sum (y - my)(y - my);
 *     lambda = ((sxx + syy) + sqrt((sxx - syy)(sxx - syy) + 4.0 (sxy sxy))) / 2.0;
 *     direction t = (lambda - syy, sxy) when sxx >= syy, else (sxy, lambda - sxx).
 *   Refined corner e = the intersection of line (e + 3) mod 4 (point M, direction T) with line e (point M', direction T'):
 *     det = Tx T'y - Ty T'x  (0 fails),   q = ((M'x - Mx) T'y - (M'y - My) T'x) / det,   corner = (Mx + q Tx, My + q Ty).
 *   All or nothing: when an edge has fewer than 4 crossings, a det is 0, a corner has |x| or |y| not below 1e300 (a corner that is not finite among them), or a corner moves by
 *   ddx ddx + ddy ddy > refine_max^2, the marker keeps the corners of step 5 and refined = 0.  No trigonometric function anywhere.
 *
 * 7. Centre: the intersection of the diagonals p_0 p_2 and p_1 p_3:  T = p_2 - p_0, T' = p_3 - p_1,
 *     det = Tx T'y - Ty T'x  (0 rejects the marker),  q = ((p_1x - p_0x) T'y - (p_1y - p_0y) T'x) / det,  (x, y) = p_0 + q T.
 *   This is the point the reference's getCenterMarker computes; it is not bit-identical to it, because the reference evaluates in
 *   float on OpenCV's float corners (and finds those corners by another method).
 *
 * The markers are listed by ascending label.  A marker id found twice is listed twice.
 *
 * Dictionary: caller data, marker_bits = 3 .. 7 and n words of marker_bits^2 bits (bit r m + c = cell (r, c), 1 = white).  The
 * reference's indexDictionary names one of OpenCV's predefined tables; those are not part of this library and have to be
 * supplied as words by the caller.  min_distance = the least popcount(dict_i xor rot_k(dict_j)) over i < j, k = 0 .. 3, and
 * popcount(dict_i xor rot_k(dict_i)) over k = 1 .. 3.  A dictionary with min_distance 0 is refused; so is
 * max_correction > (min_distance - 1) / 2, which makes a decode unique.
 *
 * lifcal_marker_dictionary_generate.  A 32-bit state s starts at seed; a draw is s = 1664525 s + 1013904223 (mod 2^32), value
 * (s >> 16) & 0xffff (the generator of lifcal_features_pattern).  A word takes ceil(m^2 / 16) draws, draw i shifted left by 16 i,
 * cut to m^2 bits.  tau starts at m^2 / 2 (integer).  A word is accepted when its distance (as for min_distance) to every
 * accepted word and to its own rotations is >= tau; after 2000 refusals in a row tau goes down by one (never below 1) and the
 * count restarts, as it does after every acceptance.
 */
#ifndef LIFCAL_MARKERS_H
#define LIFCAL_MARKERS_H
#include <stdint.h>
#include "lifcal_mla.h"
#include "lifcal_rawdepth.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LIFCAL_MARKERS_MAX_WORDS 4096

typedef struct lifcal_marker_dictionary {
  int32_t marker_bits;     /* m, 3 .. 7 */
  uint32_t n;              /* 1 .. LIFCAL_MARKERS_MAX_WORDS */
  const uint64_t* words;   /* [n] host; bits above m^2 must be 0 */
} lifcal_marker_dictionary;

/* 0 (0.0) in a field selects its default */
typedef struct lifcal_markers_options {
  int32_t w;                   /* window radius of the dark map, 1 .. 31; default 7 */
  int32_t contrast;            /* 1 .. 255, in 1/256 of the grey range; default 12 */
  int32_t cell_contrast;       /* 1 .. 255; default min(2 contrast, 255) */
  int32_t min_area;            /* >= 1; default 32 */
  int32_t min_side;            /* 2 .. 32768; default 12 */
  int32_t max_side;            /* >= min_side; default max(min(width, height), min_side) */
  int32_t max_border_errors;   /* 0 .. 4 (n - 1); default 0 */
  int32_t max_correction;      /* 0: the bound (min_distance - 1) / 2; -1: none (exact words only); else 1 .. the bound */
  double refine_max;           /* > 0 and finite, pixels; default 3 */
} lifcal_markers_options;

typedef struct lifcal_markers_plan {
  lifcal_markers_options options;   /* with the defaults filled in (max_correction -1 has become 0) */
  int32_t min_distance;             /* of the dictionary; 0 without one */
  int32_t tiles_x, tiles_y;         /* 32 x 32 pixel tiles of the dark map and the labelling */
  int32_t reserved;
  int64_t max_candidates;           /* width height / min_area */
} lifcal_markers_plan;

typedef struct lifcal_marker {
  int32_t id, rotation, hamming, refined;
  int32_t label, area;
  double corners[4][2];   /* p_0 .. p_3 as (x, y) */
  double x, y;            /* the centre */
} lifcal_marker;

/* count-then-fill as lifcal_mla_project: n and n_candidates are set whenever the call does not fail (a negative code leaves them as they were); capacity < n writes no marker and returns LIFCAL_MLA_MORE */
typedef struct lifcal_marker_list {
  uint64_t capacity;
  uint64_t n;              /* out */
  lifcal_marker* markers;  /* [capacity] host, or NULL when capacity = 0 */
  uint64_t n_candidates;   /* out: components that passed step 3 */
  double seconds;          /* out: device time of the kernels (HIP events) */
} lifcal_marker_list;

typedef struct lifcal_marker_component {
  int32_t label, area;
  int32_t x0, y0, x1, y1;
  int32_t ext[8][2];       /* (x, y) of the extreme pixels in the order of step 2 */
} lifcal_marker_component;

/* the first stage on its own: maps and the candidate table of step 3.  Count-then-fill for comp; the maps are written whenever
 * they are given */
typedef struct lifcal_marker_components {
  uint8_t* dark;           /* [height][width] host, or NULL */
  int32_t* labels;         /* [height][width] host, or NULL */
  uint64_t capacity;
  uint64_t n;              /* out: candidates */
  lifcal_marker_component* comp;   /* [capacity] host, or NULL when capacity = 0 */
  double seconds;          /* out */
} lifcal_marker_components;

/* Host only: exactly the checks lifcal_markers_detect makes of image, dictionary and options (image->data is only tested
 * against NULL).  dictionary may be NULL (as for lifcal_markers_components): then max_correction must be 0 or -1 and
 * max_border_errors is checked against marker_bits = 7.  options and plan may be NULL.  LIFCAL_BA_ERR_OUT_OF_RANGE for 2^31
 * pixels and more. */
int lifcal_markers_check(const lifcal_rawdepth_image* image, const lifcal_marker_dictionary* dictionary, const lifcal_markers_options* options,
                         lifcal_markers_plan* plan);

/* image: one channel, a host pointer or (on_device = 1) a device pointer on `device`.  status: NULL or [height][width] uint8_t with
 * row pitch = width, a pointer of the same kind as the image's.  One image per call. */
int lifcal_markers_detect(const lifcal_rawdepth_image* image, const uint8_t* status, int32_t device, const lifcal_marker_dictionary* dictionary,
                          const lifcal_markers_options* options, lifcal_marker_list* out);

int lifcal_markers_components(const lifcal_rawdepth_image* image, const uint8_t* status, int32_t device, const lifcal_markers_options* options,
                              lifcal_marker_components* out);

/* Host only.  min_distance (may be NULL) as defined above; LIFCAL_BA_ERR_INVALID_ARG for a malformed dictionary. */
int lifcal_marker_dictionary_distance(const lifcal_marker_dictionary* dictionary, int32_t* min_distance);

/* Host only.  out[n]; min_distance may be NULL.  marker_bits 3 .. 7, n 1 .. LIFCAL_MARKERS_MAX_WORDS;
 * LIFCAL_BA_ERR_OUT_OF_RANGE when tau = 1 still refuses 2000 words in a row (n larger than the space holds). */
int lifcal_marker_dictionary_generate(int32_t marker_bits, uint32_t n, uint32_t seed, uint64_t* out, int32_t* min_distance);

/* The reference's constraints file: lines `id1 id2 distance sigma`; empty lines and lines that start with # are skipped.
 * Count-then-fill for both lists (n and n_ids are set whenever the call does not fail; too small a capacity of either writes nothing and returns
 * LIFCAL_MLA_MORE).  ids: the distinct ids in order of first appearance.  LIFCAL_BA_ERR_INVALID_ARG for a file that cannot be
 * opened and for a line that does not hold two non-negative integers and two finite numbers, distance > 0, sigma > 0. */
typedef struct lifcal_constraints {
  uint64_t capacity;
  uint64_t n;              /* out */
  uint32_t* id1;           /* [capacity] each, or NULL when capacity = 0 */
  uint32_t* id2;
  double* distance;
  double* sigma;
  uint64_t ids_capacity;
  uint64_t n_ids;          /* out */
  uint32_t* ids;           /* [ids_capacity] */
} lifcal_constraints;
int lifcal_constraints_read(const char* path, lifcal_constraints* io);

/* Start values of the marker points (the reference's addArucoMarkersToData): marker observations (mx, my, mfr, mid)[n_markers]
 * and tracked image points (tx, ty, tfr, tpt)[n_tracked] with their 3D points pts[n_points][3] (tpt < n_points).  For every
 * distinct marker id, in order of first appearance in the list: the frame of its first observation with the lowest frame
 * index; among the tracked points of that frame the one with the least (tx - mx)(tx - mx) + (ty - my)(ty - my) in double, strict
 * <, so the first in the list wins ties; the marker's start value is that point's 3D point.  ids_out[k], xyz_out[k][3],
 * seeded[k] (0 when the frame holds no tracked point; xyz is then 0) for k < n_ids; count-then-fill on capacity. */
typedef struct lifcal_marker_seeds {
  uint64_t capacity;
  uint64_t n_ids;          /* out */
  uint64_t n_unseeded;     /* out */
  uint32_t* ids;           /* [capacity] */
  double* xyz;             /* [capacity][3] */
  uint8_t* seeded;         /* [capacity] */
} lifcal_marker_seeds;
int lifcal_markers_seed_points(uint64_t n_markers, const double* mx, const double* my, const uint32_t* mfr, const uint32_t* mid, uint64_t n_tracked,
                               const double* tx, const double* ty, const uint32_t* tfr, const uint32_t* tpt, uint64_t n_points, const double* pts,
                               lifcal_marker_seeds* io);

/* distance / |P1 - P2| (the reference's scaleData), |.| = sqrt(dx dx + dy dy + dz dz); LIFCAL_BA_ERR_INVALID_ARG for a
 * non-positive or non-finite distance, LIFCAL_BA_ERR_NUMERIC for coinciding or non-finite points.  Apply it with
 * lifcal_align_apply (scale = factor, R = identity, t = 0). */
int lifcal_scene_scale_factor(const double* p1, const double* p2, double distance, double* factor);

#ifdef __cplusplus
}
#endif
#endif
