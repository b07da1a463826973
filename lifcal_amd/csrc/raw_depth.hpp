// raw_depth.hpp — virtual depth from the raw image (include/lifcal_rawdepth.h): what raw_depth.hip and the
// grid handle's owner (lifcal_ba.hip, mla.hpp) share.
//
// k_rawdepth_* are compiled in a translation unit of their own, like k_point_priors and k_grid_* (point_priors.hpp says why): the
// code object of lifcal_ba.hip holds the same kernels at the same places with or without them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lifcal_mla.h"

namespace lifcal {

// lifcal_ba.hip: sets the thread's text behind lifcal_ba_last_error()
void set_last_error(const char* text);

// what raw_depth.hip reads of a lifcal_mla_handle: the parameters it was made from and its arrays on `device`
struct MlaView {
  lifcal_mla_params prm;
  int32_t device;
  int32_t n_lenses, n_sub0;     // lenses 0 .. n_sub0-1 are sub-grid 0, the rest sub-grid 1 (createGrid's list order)
  float valid_r;                // radius of the discs of map_ml
  const float* cx;              // [n_lenses] device
  const float* cy;
  const int32_t* map_ml;        // [height][width] device, -1 = no lens
};
// mla.hpp; false for a null handle
bool mla_view(const lifcal_mla_handle* h, MlaView* out);

namespace rawdepth {

constexpr int kThreads = 256;          // one workgroup per lens
constexpr int kMaxNeighbours = 18;
constexpr int kMaxHyp = 256;
constexpr int kLdsLimit = 64 * 1024;   // window + pixel list of one lens; larger is LIFCAL_BA_ERR_OUT_OF_RANGE

}  // namespace rawdepth
}  // namespace lifcal
