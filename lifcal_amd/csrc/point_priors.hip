// point_priors.hip — k_point_priors, in a code object of its own (point_priors.hpp says why).
//
// Prior k sits on point pp.point[k]; all of them are special points of the plan, so their blocks are gathered in ptacc (U at 0..5 as
// 00 10 20 11 21 22, the gradient at 6..8) by k_sweep and k_constraints and are read from there by k_promote_diag, k_jacobi, k_schur
// and k_backsub.  The kernel is stream-ordered behind the first two and in front of the others, and every word gets ONE plain add
// from one lane (the ids are strictly ascending: one writer per word): the same bits on every run, whatever options.deterministic.
#include "point_priors.hpp"

namespace lifcal {

// (Lambda d) of prior k at `pts` into ld, each row summed in ascending column order; returns 1/2 d^T Lambda d
__device__ __forceinline__ double point_prior_term(const PointPriorSet& pp, const double* pts, uint32_t k, double* ld) {
  const double* A = pp.info + 9 * (size_t)k;
  const double* m = pp.mean + 3 * (size_t)k;
  const double* P = pts + 3 * (size_t)pp.point[k];
  const double d0 = P[0] - m[0], d1 = P[1] - m[1], d2 = P[2] - m[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) ld[i] = (A[3 * i] * d0 + A[3 * i + 1] * d1) + A[3 * i + 2] * d2;
  return 0.5 * ((d0 * ld[0] + d1 * ld[1]) + d2 * ld[2]);
}

// One lane per prior (workgroups of one wave).  Workgroup 0 sums the costs first: lane l takes the priors l, l + 64, ... in
// ascending order, the wave reduction has a fixed shape, lane 0 adds the sum once to *cost_out.
__global__ __launch_bounds__(PP_THREADS) void k_point_priors(PointPriorSet pp, int cost_only, const double* pts, double* cost_out) {
  const uint32_t lane = threadIdx.x;
  double ld[3];
  if (blockIdx.x == 0) {
    double s = 0.0;
    for (uint32_t k = lane; k < pp.n; k += PP_THREADS) s += point_prior_term(pp, pts, k, ld);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (lane == 0) *cost_out += s;
  }
  const uint32_t k = blockIdx.x * PP_THREADS + lane;
  if (cost_only || k >= pp.n) return;
  (void)point_prior_term(pp, pts, k, ld);
  const double* A = pp.info + 9 * (size_t)k;
  double* acc = pp.ptacc + (size_t)pp.point[k] * 36;
  acc[0] += A[0]; acc[1] += A[3]; acc[2] += A[6]; acc[3] += A[4]; acc[4] += A[7]; acc[5] += A[8];
#pragma unroll
  for (int i = 0; i < 3; ++i) acc[6 + i] += ld[i];
}

hipError_t launch_k_point_priors(const PointPriorSet& pp, int cost_only, const double* pts, double* cost_out, hipStream_t stream) {
  hipLaunchKernelGGL(k_point_priors, dim3(cost_only ? 1u : (pp.n + PP_THREADS - 1) / PP_THREADS), dim3(PP_THREADS), 0, stream, pp, cost_only, pts, cost_out);
  return hipGetLastError();
}

}  // namespace lifcal
