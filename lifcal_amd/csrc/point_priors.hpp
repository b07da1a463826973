// point_priors.hpp — Gaussian priors on 3D points (include/lifcal_prior.h second part): what the host driver
// (lifcal_ba.hip, priors.hpp) and the kernel's own translation unit (point_priors.hip) share.
//
// k_point_priors is compiled in a translation unit of its own, so that it lies in a code object of its own: the code object of
// lifcal_ba.hip, with every kernel of the flagship path, then holds the same kernels at the same places whether or not this
// feature exists (measured: one more kernel in that code object costs the flagship sweep 0.5 %).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lifcal {

struct PointPriorSet {
  uint32_t n;
  const uint32_t* point;         // n point ids, strictly ascending (all of them special points of the plan)
  const double *mean, *info;     // 3 n, 9 n row-major
  double* ptacc;                 // Dev::ptacc: P x 36, U at 0..5 (00 10 20 11 21 22), the gradient at 6..8
};

constexpr uint32_t PP_THREADS = 64;

// cost (and, unless cost_only, the blocks into ptacc) of the priors at `pts`; the cost is added to *cost_out.  Stream-ordered.
hipError_t launch_k_point_priors(const PointPriorSet& pp, int cost_only, const double* pts, double* cost_out, hipStream_t stream);

}  // namespace lifcal
