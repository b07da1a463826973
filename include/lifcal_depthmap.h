/* lifcal_depthmap.h — the virtual-image depth map from the raw-pixel depth: the inverse virtual depth per raw
 * pixel that lifcal_rawdepth_estimate measures (include/lifcal_rawdepth.h), resampled onto the virtual-image grid in the encoding
 * of the depth PNGs, which is what lifcal_depth_sample, lifcal_depth_back_project_maps, lifcal_depth_check_maps and
 * lifcal_depth_fuse_maps consume (include/lifcal_depth.h: pixel (col, row) is (x_v, y_v), iv = 1 - value / 65535).  Same shared
 * library as include/lifcal_ba.h (liblifcal_ba.so), same error codes and lifcal_ba_last_error().  Argument checks come first and
 * need no device; the work runs on the GPU and there is no CPU fallback (LIFCAL_BA_ERR_NO_DEVICE without a gfx950 device).
 *
 * The algorithm, exactly.  Doubles are IEEE without fused multiply-add, evaluated in the order written.  Everything that is
 * accumulated is an integer, so the result does not depend on the order of the atomics: two calls give the same bytes, equal to
 * those of the numpy restatement in tests/depthmap_reference.py.
 *
 * Constants.  Q = 2^20,  tq = floor(tol_iv Q + 0.5).
 *
 * Sample.  A raw pixel p = (px, py) is a sample when map_ml[p] = i >= 0 (lifcal_mla_get_maps), inv_depth[p] is not NaN and, with
 *   iv = (double)inv_depth[p],  iv_min <= iv <= 1  (lifcal_rawdepth_estimate writes no iv above 0.5 plus half a hypothesis step; the
 *   upper limit keeps q within 2^20 for any input).  For a sample
 *   v = 1 / iv,
 *   xu = cx[i] + v (px - cx[i])  with the float centres widened to double,  x = (xu + 0.5) / scale - 0.5,  y likewise
 *   (the formulas of lifcal_rawdepth_points),
 *   h = (0.5 v) / scale,
 *   q = floor(iv Q + 0.5).
 * Its footprint is the set of cells X0 .. X1 x Y0 .. Y1 clipped to the output, with
 *   X0 = ceil(x - h),  X1 = ceil(x + h) - 1,  Y0 = ceil(y - h),  Y1 = ceil(y + h) - 1:
 * the cells whose centre lies in the square of side v / scale about (x, y), half open.  For constant v the footprints of adjacent
 * pixels of one micro image tile the virtual image without overlap.  An empty footprint after clipping is not an error.
 *
 * Pass 1.  front[cell] = min q over the samples whose footprint holds the cell.  In this camera model a larger v is a nearer
 *   object, so the smallest iv is the foreground.
 * Pass 2.  Over the same samples, those with q <= front[cell] + tq add q to sum[cell] and 1 to n[cell].
 * Resolve.  Per cell:  no sample: status 2, support 0.  n < min_support: status 3 (a lone front value), support = min(n, 65535).
 *   Otherwise status 0,  q_cell = floor((2 sum + n) / (2 n)) by integer division,  support = min(n, 65535).
 * Fill.  fill_rounds Jacobi rounds: each reads the map of the round's start and writes a new one.  For a cell with status 2 or 3,
 *   of its 8 neighbours inside the map that have a value (status 0 or 1) at the round's start:  qmin is their minimum, the front
 *   neighbours are those with q <= qmin + tq, c is their count and S their sum.  When c >= fill_min_neighbours: status 1,
 *   q_cell = floor((2 S + c) / (2 c)),  support 0.
 * Outputs.  For a cell with a value (status 0 or 1):
 *   inv_depth = (float)((double)q_cell / Q),
 *   value = floor(65535.0 (1.0 - (double)q_cell / Q) + 0.5),
 *   depth16 = value when the direct rule of lifcal_depth_sample accepts it (value > 0 and 1.0 - value / 65535.0 in (0, 0.5]), else
 *   0; the float map keeps the value.  A cell without a value has inv_depth NaN and depth16 0.
 *
 * The bound the accumulation relies on.  Pass 2 adds ((q - front[cell]) << 24) + 1 to one 64-bit word per cell (sum = n front +
 * the upper 40 bits), so n must stay below 2^24 and n tq below 2^40.  A sample reaches a cell only from a lens whose centre lies
 * within (valid_r + 0.5) / iv_min + scale raw pixels of it, so n <= max_samples_per_cell = min(width height, (2 R + 1)^2) with
 * R = ceil((valid_r + 0.5) / iv_min + scale + d / 2), valid_r = d / 2 - 1; the checks refuse options that break either limit
 * (LIFCAL_BA_ERR_OUT_OF_RANGE).
 */
#ifndef LIFCAL_DEPTHMAP_H
#define LIFCAL_DEPTHMAP_H
#include <stdint.h>
#include "lifcal_mla.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 0 (0.0) in a field selects its default */
typedef struct lifcal_depthmap_options {
  int32_t scale;                  /* depth_to_raw_im_scale, >= 1; default 1 */
  int32_t out_width, out_height;  /* default width / scale, height / scale (integer division) */
  int32_t min_support;            /* fewest front samples for a measured cell, >= 1; default 2 */
  int32_t fill_rounds;            /* default 2; negative: no fill */
  int32_t fill_min_neighbours;    /* fewest front neighbours for a filled cell, 1 .. 8; default 3 */
  double tol_iv;                  /* cluster width in inverse virtual depth, in (0, 0.5]; default 0.02 */
  double iv_min;                  /* samples below it are skipped, in (0, 1]; default 0.04.  Bounds the footprint at
                                     floor(1 / (iv_min scale)) + 1 cells per side */
} lifcal_depthmap_options;

#define LIFCAL_DEPTHMAP_MEASURED 0    /* status values */
#define LIFCAL_DEPTHMAP_FILLED 1
#define LIFCAL_DEPTHMAP_EMPTY 2
#define LIFCAL_DEPTHMAP_REJECTED 3

/* what the argument checks of lifcal_depthmap_from_raw derive before any device is touched */
typedef struct lifcal_depthmap_plan {
  lifcal_depthmap_options options;    /* with the defaults filled in */
  int32_t out_width, out_height;
  int32_t tq;
  int32_t max_side;                   /* largest footprint side in cells: floor(1 / (iv_min scale)) + 1 */
  int64_t max_samples_per_cell;       /* the bound on n above */
} lifcal_depthmap_plan;

typedef struct lifcal_depthmap_result {
  int32_t out_on_device;     /* 0: the four maps are host pointers; 1: device pointers on the grid's device */
  int32_t reserved;
  float* inv_depth;          /* [out_height][out_width] or NULL: NaN where there is no value */
  uint16_t* depth16;         /* [out_height][out_width] or NULL: the depth PNG's encoding, 0 where invalid */
  uint8_t* status;           /* [out_height][out_width] or NULL */
  uint16_t* support;         /* [out_height][out_width] or NULL: front samples, saturated at 65535 */
  uint64_t count[4];         /* out: cells per status */
  uint64_t n_samples;        /* out: samples used */
  double seconds;            /* out: device time of the kernels (HIP events) */
} lifcal_depthmap_result;

/* Host only: exactly the checks lifcal_depthmap_from_raw makes of the options for a grid with these parameters and a raw depth
 * of width x height (which must be the grid's).  options and plan may be NULL. */
int lifcal_depthmap_check(const lifcal_mla_params* grid_params, int32_t width, int32_t height, const lifcal_depthmap_options* options,
                          lifcal_depthmap_plan* plan);

/* inv_depth: [height][width] of the grid as lifcal_rawdepth_estimate wrote it; on_device 0: a host pointer, 1: a device pointer
 * on the grid's device (e.g. a torch tensor).  LIFCAL_BA_ERR_INVALID_ARG for a bad argument or option,
 * LIFCAL_BA_ERR_OUT_OF_RANGE when the bound above or 2^31 cells are exceeded. */
int lifcal_depthmap_from_raw(lifcal_mla_handle* grid, const float* inv_depth, int32_t on_device, const lifcal_depthmap_options* options,
                             lifcal_depthmap_result* out);

#ifdef __cplusplus
}
#endif
#endif
