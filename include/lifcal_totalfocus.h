/* lifcal_totalfocus.h — the total-focus image from the raw image and the virtual-image depth map: the
 * all-in-focus picture on the virtual-image grid, the image whose pixels (x, y) lifcal_mla_project, lifcal_rawdepth_points,
 * lifcal_depth_sample and the COLMAP ingestion (include/lifcal_colmap.h) speak of.  Every cell gathers its picture from all micro
 * lenses that see it at the depth the map gives (include/lifcal_depthmap.h).  Same shared library as include/lifcal_ba.h
 * (liblifcal_ba.so), same error codes and lifcal_ba_last_error().  Argument checks come first and need no device; the work runs on
 * the GPU and there is no CPU fallback (LIFCAL_BA_ERR_NO_DEVICE without a gfx950 device).
 *
 * The algorithm, exactly.  Doubles are IEEE without fused multiply-add, evaluated in the order written.  Everything that is summed
 * is an integer and the lenses of a cell are selected by geometry alone, so any enumeration that covers them gives the same bytes:
 * two calls give the same bytes, equal to those of the numpy restatement in tests/totalfocus_reference.py.
 *
 * Constants.  d = lens_diameter widened to double,  valid_r = the float radius of the discs of lifcal_mla_get_maps (d/2 - 1 in
 *   float arithmetic) widened,  r_use = valid_r - margin,  reach2 = (max_reach d) (max_reach d),  full = 2^bits - 1.
 *
 * Cell (X, Y).  iv = (double)inv_depth[Y][X].  When iv is NaN or outside [iv_min, 1] the cell has no depth: with default_iv > 0 it
 *   goes on with iv = default_iv (and ends in status 3 where a cell with a depth ends in status 0), otherwise it gets status 1,
 *   pixel 0 and n_lenses 0.
 *   xu = ((double)X + 0.5) scale - 0.5,  yu likewise: the inverse of x = (xu + 0.5) / scale - 0.5 of lifcal_rawdepth_points.
 *
 * Lens j of lifcal_mla_get_lenses' list, float centres widened to double, counts for the cell when all of these hold:
 *   dx = xu - cx[j],  dy = yu - cy[j],  dx dx + dy dy <= reach2;
 *   ox = dx iv,  oy = dy iv,  ox ox + oy oy <= r_use r_use   (the picture of the point, p = c + (x_u - c) / v as in
 *   lifcal_mla_project, lies inside the lens's disc, and with the default margin its 2 x 2 support does too);
 *   Sx = floor(64 (cx[j] + ox) + 0.5),  ix = Sx >> 6 (arithmetic),  fx = Sx & 63,  the same in y, and
 *   ix >= 0,  ix + 1 <= width - 1,  iy >= 0,  iy + 1 <= height - 1.
 * It contributes
 *   B = (64-fx)(64-fy) I(ix,iy) + fx (64-fy) I(ix+1,iy) + (64-fx) fy I(ix,iy+1) + fx fy I(ix+1,iy+1)
 * (the bilinear form of include/lifcal_rawdepth.h) and, with a white image, Bw, the same form on the white image.
 *   num = sum of B,  den = sum of Bw,  n = the number of lenses that count.
 *
 * Result.  Without a white image, when n >= min_lenses:  pixel = floor((2 num + 4096 n) / (2 * 4096 n)).
 *   With a white image, when n >= min_lenses and den > 0:  pixel = min(full, floor((2 num white_level + den) / (2 den))) in 64-bit
 *   integers: a ratio of sums, so the bright centre of a micro image weighs more than its dim rim, and a factor common to the raw
 *   and the white image (vignetting) cancels.
 *   If neither holds: status 2, pixel 0, n_lenses = min(n, 255).
 *   Otherwise status 0 when the depth came from the map and 3 when it came from default_iv;  n_lenses = min(n, 255).
 *
 * The bound the sums rely on.  The lenses lie on a lattice with rows by d apart and d between the lenses of a row (by =
 * lens_base_y[1]), so at most  max_lenses_per_cell = (floor(2 (max_reach + 1) / by) + 1) (floor(2 (max_reach + 1)) + 1)  of them lie
 * within max_reach d plus one ring of a point.  B <= 4096 * 65535 < 2^28 and white_level < 2^16, so num white_level stays below
 * 2^63 while max_lenses_per_cell < 2^18; the checks refuse anything else (LIFCAL_BA_ERR_OUT_OF_RANGE).
 */
#ifndef LIFCAL_TOTALFOCUS_H
#define LIFCAL_TOTALFOCUS_H
#include <stdint.h>
#include "lifcal_mla.h"
#include "lifcal_rawdepth.h"
#ifdef __cplusplus
extern "C" {
#endif

/* 0 (0.0) in a field selects its default */
typedef struct lifcal_totalfocus_options {
  int32_t scale;                  /* depth_to_raw_im_scale, >= 1; default 1 */
  int32_t out_width, out_height;  /* default width / scale, height / scale (integer division) */
  int32_t min_lenses;             /* fewest lenses for a pixel, 1 .. 255; default 1 */
  int32_t white_level;            /* the grey level of the white image that maps to full brightness, 1 .. full; default full */
  double margin;                  /* raw pixels kept clear of the rim of a lens's disc, >= 0 with r_use >= 0.5; default 1.5 */
  double max_reach;               /* lenses farther than this many diameters are not used, in (0, 8]; default 4 */
  double iv_min;                  /* depths below it count as no depth, in [0.001, 1]; default 0.04 */
  double default_iv;              /* depth of the cells without one, 0 (none, the default) or in [iv_min, 1] */
} lifcal_totalfocus_options;

#define LIFCAL_TOTALFOCUS_OK 0             /* status values */
#define LIFCAL_TOTALFOCUS_NO_DEPTH 1
#define LIFCAL_TOTALFOCUS_NO_LENS 2
#define LIFCAL_TOTALFOCUS_DEFAULT_DEPTH 3

/* what the argument checks of lifcal_totalfocus_render derive before any device is touched */
typedef struct lifcal_totalfocus_plan {
  lifcal_totalfocus_options options;   /* with the defaults filled in */
  int32_t out_width, out_height;
  double r_use;
  int32_t max_lenses_per_cell;         /* the bound on n above */
  int32_t reserved;
} lifcal_totalfocus_plan;

typedef struct lifcal_totalfocus_result {
  int32_t out_on_device;     /* 0: the three maps are host pointers; 1: device pointers on the grid's device */
  int32_t reserved;
  void* image;               /* [out_height][out_width] or NULL: uint8_t or uint16_t, the raw image's bits */
  uint8_t* n_lenses;         /* [out_height][out_width] or NULL: lenses that counted, saturated at 255 */
  uint8_t* status;           /* [out_height][out_width] or NULL */
  uint64_t count[4];         /* out: cells per status */
  double seconds;            /* out: device time of the kernels (HIP events) */
} lifcal_totalfocus_result;

/* Host only: exactly the checks lifcal_totalfocus_render makes of `image`, `white` (or NULL) and `options` for a grid with these
 * parameters and a depth map of depth_width x depth_height, which must be the output size (the data pointers are only tested
 * against NULL).  options and plan may be NULL. */
int lifcal_totalfocus_check(const lifcal_mla_params* grid_params, const lifcal_rawdepth_image* image, const lifcal_rawdepth_image* white,
                            int32_t depth_width, int32_t depth_height, const lifcal_totalfocus_options* options, lifcal_totalfocus_plan* plan);

/* image, white (or NULL: no white image): one channel each, of the grid's size and of the same bits.  inv_depth:
 * [out_height][out_width] float, the inv_depth map of lifcal_depthmap_from_raw at the same scale (or a decoded depth PNG:
 * iv = 1 - value / 65535, NaN where value = 0); depth_on_device 0: a host pointer, 1: a device pointer on the grid's device.
 * LIFCAL_BA_ERR_INVALID_ARG for a bad argument or option, LIFCAL_BA_ERR_OUT_OF_RANGE when the bound above or 2^31 cells are
 * exceeded. */
int lifcal_totalfocus_render(lifcal_mla_handle* grid, const lifcal_rawdepth_image* image, const lifcal_rawdepth_image* white,
                             const float* inv_depth, int32_t depth_on_device, const lifcal_totalfocus_options* options,
                             lifcal_totalfocus_result* out);

#ifdef __cplusplus
}
#endif
#endif
