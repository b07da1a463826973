/* lifcal_grid.h — the micro-lens grid from a white image: the six numbers lifcal_mla_create takes
 * (lens_diameter, lens_base_y, rotation, offset) measured from a raw exposure of a diffuse white surface, in which every micro
 * lens draws one bright disc, instead of read from the vendor's MLA calibration file.  Same shared library as
 * include/lifcal_ba.h (liblifcal_ba.so), same error codes and lifcal_ba_last_error().
 *
 * Three entry points: lifcal_grid_detect finds the lens centres on the GPU (box sum, local maxima, integer centroids; no CPU
 * fallback: LIFCAL_BA_ERR_NO_DEVICE without a gfx950 device); lifcal_grid_fit_centres fits the lattice to a list of centres on
 * the host (no device, no handle); lifcal_grid_fit runs detect and fit, and then both once more with the fitted diameter in
 * place of the guess.
 *
 * The model fitted is the one lifcal_mla_create builds (MicroLensGrid::createGrid, src/MicroLensGrid/MicroLensGrid.cpp:186-270):
 * the centre of lens (k, x, y) is  offset_cv + R(rotation) g  with image y pointing down,
 *     g = (x d, 2 y by d)                 on sub-grid 0,
 *     g = ((x + 1 + bx) d, (2 y + 1) by d) on sub-grid 1,      d = lens_diameter, bx = lens_base_y[0], by = lens_base_y[1]
 * a rectangular lattice with a two-lens basis, six parameters.  It is not a general oblique lattice; the general lattice
 * vectors of the unconstrained fit are reported next to it, and the per-lens residuals show what the model does not hold.
 *
 * Conventions (one lattice has many equivalent parameter sets):
 *   - the row vector A is the lattice vector nearest to +x; |rotation| < 10 degrees, LIFCAL_BA_ERR_INVALID_ARG otherwise;
 *   - lens_base_y[0] in [-1, 0)  (-0.5 for a hexagonal array), lens_base_y[1] > 0;
 *   - the origin lens (sub-grid 0, x = y = 0) is the fitted node nearest to the image centre;
 *   - rotation_on_grid = 1.
 * A white image cannot tell the three lens types apart: which physical lens has type 0 (x mod 3 in lifcal_mla_get_lenses) is
 * arbitrary, it follows from where the origin fell.
 */
#ifndef LIFCAL_GRID_H
#define LIFCAL_GRID_H
#include <stdint.h>
#include "lifcal_mla.h"
#ifdef __cplusplus
extern "C" {
#endif

/* a white image in host memory: one channel (a colour sensor's caller passes one channel or the sum) */
typedef struct lifcal_grid_image {
  const void* data;      /* uint8_t when bits = 8, uint16_t when bits = 16 */
  int32_t bits;          /* 8 or 16 */
  int32_t width, height;
  int64_t pitch;         /* elements from one row to the next, >= width */
} lifcal_grid_image;

/* one lens centre: cx = sum_wx / sum_w, cy = sum_wy / sum_w (one division each of the exact integer moments of the second
 * centroid round; weight = pixel value minus the minimum over the disc of radius guess / 2) */
typedef struct lifcal_grid_centre {
  double cx, cy;
  int64_t sum_w, sum_wx, sum_wy;
  int64_t peak;          /* pixel index y * width + x of the box-sum maximum the lens was found at */
} lifcal_grid_centre;

/* count-then-fill, as lifcal_mla_project: n is always set; capacity < n writes nothing and returns LIFCAL_MLA_MORE */
typedef struct lifcal_grid_centres {
  uint64_t capacity;
  uint64_t n;            /* out */
  lifcal_grid_centre* c; /* capacity entries, or NULL when capacity = 0 */
} lifcal_grid_centres;

/* Lens centres of a white image, in ascending order of `peak`.  Supports 6 <= lens_diameter_guess <= 64 pixels and a true
 * diameter within 10 % of the guess.  Lenses whose peak is closer than ceil(guess / 2) + 1 pixels to the border are left out. */
int lifcal_grid_detect(const lifcal_grid_image* image, double lens_diameter_guess, int32_t device, lifcal_grid_centres* out);

typedef struct lifcal_grid_lens {
  int32_t sub, x, y;     /* label: sub-grid, column, row */
  int32_t accepted;      /* 1 = used by the fit, 0 = rejected (label or residual gate) */
  double dx, dy;         /* centre minus the fitted grid's node with that label, pixels */
} lifcal_grid_lens;

typedef struct lifcal_grid_report {
  uint64_t capacity;     /* in: entries of `lens` (0 and NULL: no per-lens table) */
  lifcal_grid_lens* lens;
  uint64_t n_centres, n_accepted, n_rejected_label, n_rejected_residual;
  double rms, max_residual;                               /* of the accepted centres, pixels */
  double lattice_a[2], lattice_b[2], lattice_c[2];        /* unconstrained fit, image coordinates: one column step, the step
                                                             from lens (0, x, y) to lens (1, x, y), one row step of a sub-grid */
  double lens_diameter, rotation, lens_base_y[2], origin[2];   /* the fitted model in double; origin = centre of lens (0, 0, 0) */
} lifcal_grid_report;

/* Host only.  Labels the centres from a seed at the image centre, fits the six-parameter model and fills `params` (ready for
 * lifcal_mla_create) and, when given, `report`.  A centre is rejected when its label is more than 0.25 of a cell from an
 * integer, or when its residual exceeds max(gate_px, 4 rms), after which the fit is repeated once.  Returns
 * LIFCAL_BA_ERR_INVALID_ARG for non-finite input, fewer than 12 accepted centres, centres that span fewer than three rows or
 * columns, |rotation| >= 10 degrees, or report->capacity between 1 and n - 1.  Centres are taken in the order given (detect's). */
int lifcal_grid_fit_centres(uint64_t n, const double* cx, const double* cy, int32_t width, int32_t height,
                            double lens_diameter_guess, double gate_px, lifcal_mla_params* params, lifcal_grid_report* report);

/* detect + fit, then detect + fit again with the fitted diameter in place of the guess (always, so that the result does not
 * depend on a threshold).  The image is uploaded once.  centres / report (either may be NULL) receive the second pass;
 * LIFCAL_MLA_MORE when one of their capacities is too small (centres->n and report->n_centres are set, nothing else written). */
int lifcal_grid_fit(const lifcal_grid_image* image, double lens_diameter_guess, double gate_px, int32_t device,
                    lifcal_mla_params* params, lifcal_grid_centres* centres, lifcal_grid_report* report);

#ifdef __cplusplus
}
#endif
#endif
