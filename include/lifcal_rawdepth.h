/* lifcal_rawdepth.h — virtual depth from the raw image of a focused plenoptic camera: for every raw pixel
 * the inverse virtual depth, measured by a multi-baseline plane sweep against the neighbouring micro images, and the status-0
 * pixels as the image points lifcal_mla_project and lifcal_depth_back_project_points take.  Same shared library as
 * include/lifcal_ba.h (liblifcal_ba.so), same error codes and lifcal_ba_last_error().  Argument checks come first and need no
 * device; the work runs on the GPU and there is no CPU fallback (LIFCAL_BA_ERR_NO_DEVICE without a gfx950 device).
 *
 * Geometry.  A virtual-image point at virtual depth v shows in every micro lens within v d / 2 of it; between two lenses whose
 * centres are Delta apart its two pictures are Delta (1 - 1/v) apart (lifcal_mla_project: xr = (xu - lcx) / v + lcx).  Sweeping
 * iv = 1/v and comparing the patch about a pixel with the patch at p + Delta (1 - iv) of each neighbour measures iv.
 *
 * The algorithm, exactly.  Floating-point steps are IEEE double without fused multiply-add, in the order written; image
 * arithmetic is integer.  Two calls give the same bytes, equal to those of the numpy restatement in tests/rawdepth_reference.py.
 *
 * Tables (host).  d, bx, by, rotation: the floats of lifcal_mla_params widened to double (rotation = 0 without rotation_on_grid).
 *   step = (iv_max - iv_min) / (K - 1),  iv_k = iv_min + k step.
 *   e1 = (cos, -sin), e2 = (-sin, -cos);  A = d e1,  C = ((2 by) d) e2,  D = ((1 + bx) d) e1 + (by d) e2   (section 7s).
 *   Neighbours of a lens of sub-grid 0: the non-zero x A + y C and the (x A + y C) + D, integer x, y, of length
 *   sqrt(vx vx + vy vy) <= max_baseline d; of sub-grid 1: the same with - D.  More than 18 is LIFCAL_BA_ERR_INVALID_ARG.
 *   Shift of neighbour n at hypothesis k, per component, in 1/64 pixel:  S = floor(64 (Delta_n (1 - iv_k)) + 0.5).
 *
 * Per pixel p = (px, py).  i = map_ml[p] (lifcal_mla_get_maps: the disc of radius valid_r = d/2 - 1 of lens i),
 *   o = p - (cx[i], cy[i]) with the float centres widened to double, w = patch_radius.
 *   status 1 (no estimate possible): i < 0, or ox ox + oy oy > (valid_r - w)^2, or the (2w+1)^2 patch about p leaves the image.
 *   status 2 (flat): max - min over the patch about p is below min_contrast.
 *
 * Per hypothesis k and neighbour n.  The pair counts when
 *   tx = ox - Delta_x iv_k, ty likewise, tx tx + ty ty <= (valid_r - w - 1)^2   (the match lies inside the neighbour's disc), and
 *   with ix = S_x >> 6, iy = S_y >> 6 (arithmetic):  px - w + ix >= 0, px + w + ix + 1 <= width - 1, and the same in y
 *   (the shifted patch with its 2 x 2 bilinear support lies inside the image).
 * For a pair that counts, with fx = S_x & 63, fy = S_y & 63, the sum over the patch offsets delta of
 *   | 4096 I(q) - ((64-fx)(64-fy) I(r) + fx (64-fy) I(r + (1,0)) + (64-fx) fy I(r + (0,1)) + fx fy I(r + (1,1))) |,
 *   q = p + delta, r = q + (ix, iy), is added to sum_k, and n_k is incremented.
 * cost_k = (double)sum_k / (double)n_k when n_k >= min_neighbours, +infinity otherwise.
 *
 * Selection.  k is a local minimum when cost_k is finite, cost_k < cost_{k-1} and cost_k <= cost_{k+1} (a missing or infinite
 * neighbour counts as +infinity).  kb is the lowest k of least cost; c0, c-, c+ are the costs at kb, kb - 1, kb + 1.
 *   status 3 (no usable minimum): no finite cost, kb = 0 or K - 1, c- or c+ infinite, or den = (c- - 2 c0) + c+ <= 0.
 *   status 4 (ambiguous): some local minimum k with |k - kb| >= 3 has cost_k < ambiguity_ratio c0.
 *   status 0 otherwise:  inv_depth = (float)(iv_kb + ((0.5 (c- - c+)) / den) step).
 * Precedence 1, 2, 3, 4, 0.  cost = (float)(c0 / (4096 (2w+1)^2)) and n_neighbours = n_kb under status 0 and 4; everywhere else
 * inv_depth and cost are NaN and n_neighbours is 0.
 */
#ifndef LIFCAL_RAWDEPTH_H
#define LIFCAL_RAWDEPTH_H
#include <stdint.h>
#include "lifcal_mla.h"
#ifdef __cplusplus
extern "C" {
#endif

/* one channel of a raw image, width x height equal to the grid's */
typedef struct lifcal_rawdepth_image {
  const void* data;      /* uint8_t when bits = 8, uint16_t when bits = 16 */
  int32_t bits;          /* 8 or 16 */
  int32_t width, height;
  int32_t on_device;     /* 0: host pointer; 1: device pointer on the grid's device (e.g. a torch tensor) */
  int64_t pitch;         /* elements from one row to the next, >= width */
} lifcal_rawdepth_image;

/* 0 (0.0) in a field selects its default */
typedef struct lifcal_rawdepth_options {
  int32_t n_hyp;             /* K, 8 .. 256; default 64 */
  int32_t patch_radius;      /* w, 1 or 2; default 1 */
  int32_t min_neighbours;    /* >= 1; default 2 */
  int32_t min_contrast;      /* grey levels; default 8 (8-bit), 2048 (16-bit) */
  double iv_min, iv_max;     /* 0 < iv_min < iv_max <= 0.5; defaults 0.04 and 0.5 */
  double max_baseline;       /* lens diameters; default 1.05 (the 6 nearest lenses); 2.1 gives 18 */
  double ambiguity_ratio;    /* >= 1; default 1.5 */
} lifcal_rawdepth_options;

#define LIFCAL_RAWDEPTH_OK 0          /* status values */
#define LIFCAL_RAWDEPTH_NO_LENS 1
#define LIFCAL_RAWDEPTH_FLAT 2
#define LIFCAL_RAWDEPTH_NO_MINIMUM 3
#define LIFCAL_RAWDEPTH_AMBIGUOUS 4

typedef struct lifcal_rawdepth_result {
  int32_t out_on_device;     /* 0: the four maps are host pointers; 1: device pointers on the grid's device */
  int32_t n_neighbours_used; /* out: neighbours per lens the options selected */
  float* inv_depth;          /* [height][width] or NULL */
  float* cost;               /* [height][width] or NULL: mean absolute grey-level difference at the minimum */
  uint8_t* status;           /* [height][width] or NULL */
  uint8_t* n_neighbours;     /* [height][width] or NULL: pairs that counted at the minimum */
  uint64_t count[5];         /* out: pixels per status */
  double seconds;            /* out: device time of the kernels (HIP events) */
} lifcal_rawdepth_result;

/* what the argument checks of lifcal_rawdepth_estimate derive before any device is touched */
typedef struct lifcal_rawdepth_plan {
  lifcal_rawdepth_options options;   /* with the defaults filled in */
  int32_t n_neighbours;              /* neighbours per lens that max_baseline selects */
  int32_t window;                    /* side of the square neighbourhood one lens keeps in LDS, pixels */
  int32_t lds_bytes;                 /* LDS of one workgroup: the window as 16-bit plus the lens's pixel list */
  int32_t reserved;
} lifcal_rawdepth_plan;

/* Host only: exactly the checks lifcal_rawdepth_estimate makes of `image` and `options` for a grid with these parameters
 * (image->data is only tested against NULL).  plan may be NULL. */
int lifcal_rawdepth_check(const lifcal_mla_params* grid_params, const lifcal_rawdepth_image* image, const lifcal_rawdepth_options* options,
                          lifcal_rawdepth_plan* plan);

/* LIFCAL_BA_ERR_INVALID_ARG for a bad argument or option (more than 18 neighbours among them), LIFCAL_BA_ERR_OUT_OF_RANGE when
 * the neighbourhood of one lens (a square of about (1 + 2 max_baseline) d pixels, 16-bit) does not fit 64 KB of LDS. */
int lifcal_rawdepth_estimate(lifcal_mla_handle* grid, const lifcal_rawdepth_image* image, const lifcal_rawdepth_options* options,
                             lifcal_rawdepth_result* out);

/* The status-0 pixels (inv_depth not NaN) as image points of the virtual image, in ascending pixel index src = py width + px:
 *   v = 1 / (double)inv_depth,  xu = cx[i] + v (px - cx[i]),  x = (xu + 0.5) / depth_to_raw_im_scale - 0.5,  y likewise;
 * the inverse of lifcal_mla_project's mapping for the same scale, so x, y, vdepth are what lifcal_mla_points and
 * lifcal_depth_points take.  Count-then-fill as lifcal_mla_project: n is always set; capacity < n writes nothing and returns
 * LIFCAL_MLA_MORE.  The output arrays are host pointers. */
typedef struct lifcal_rawdepth_point_list {
  const float* inv_depth;    /* [height][width] of the grid, as lifcal_rawdepth_estimate wrote it */
  int32_t on_device;         /* 0: inv_depth is a host pointer; 1: a device pointer on the grid's device */
  int32_t depth_to_raw_im_scale;   /* >= 1 */
  uint64_t capacity;
  uint64_t n;                /* out */
  double* x;                 /* capacity entries each, or NULL when capacity = 0 */
  double* y;
  double* vdepth;
  uint32_t* src;             /* or NULL */
  int32_t* lens;             /* or NULL: index into lifcal_mla_get_lenses */
} lifcal_rawdepth_point_list;
int lifcal_rawdepth_points(lifcal_mla_handle* grid, lifcal_rawdepth_point_list* io);

#ifdef __cplusplus
}
#endif
#endif
