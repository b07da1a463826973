// grid_fit.hpp — the micro-lens grid from a white image (include/lifcal_grid.h): the shapes grid_fit.hip's
// kernels and its host driver share.
//
// k_grid_box, k_grid_peaks and k_grid_centroid are compiled in a translation unit of their own, like k_point_priors
// (point_priors.hpp says why): the code object of lifcal_ba.hip holds the same kernels at the same places with or without them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lifcal {

// lifcal_ba.hip: sets the thread's text behind lifcal_ba_last_error()
void set_last_error(const char* text);

namespace grid {

constexpr double kGuessMin = 6.0, kGuessMax = 64.0;
constexpr int kBoxRMax = 16;      // round(0.25 * 64)
constexpr int kPeakMMax = 25;     // floor(0.4 * 64)

// k_grid_box: one workgroup sums a kBoxX x kBoxY tile from an LDS copy with a halo of r
constexpr int kBoxX = 64, kBoxY = 32, kBoxThreads = 256;
// k_grid_peaks: one workgroup decides a kPeakX x kPeakY tile from an LDS copy of the box sums with a halo of m
constexpr int kPeakX = 32, kPeakY = 32, kPeakThreads = 256;
// k_grid_centroid: one wave per peak, four to a workgroup
constexpr int kCentroidThreads = 256;

// what the three stages derive from the guess (the restatement in tests/grid_fit_reference.py derives the same)
struct Sizes {
  int r;        // box radius: round(0.25 guess)
  int m;        // peak window radius: floor(0.4 guess)
  int border;   // peaks closer than this to the border are dropped: ceil(0.5 guess) + 1
  double R, R2; // centroid disc: 0.5 guess and its square
};

struct Centre {   // = lifcal_grid_centre
  double cx, cy;
  int64_t sum_w, sum_wx, sum_wy;
  int64_t peak;
};

}  // namespace grid
}  // namespace lifcal
