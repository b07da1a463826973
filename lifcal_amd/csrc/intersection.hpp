// intersection.hpp — lifcal_intersect_points (include/lifcal_intersect.h): its kernels, then the host driver (included at the end
// of lifcal_ba.hip, behind resection.hpp, whose k_resect_lens and obs_pose_eval it reuses).  DESIGN.md section 7m.
//
//   k_intersect_frames  the frame_eval table of every pose, once per call (the poses are constant)
//   k_resect_lens       (resection.hpp) c_u of every observation and the camera constants, folded | as stored
//   k_intersect         one wave64 per point, persistent over the point's whole Levenberg-Marquardt solve: sweep (residual and
//                       J_P = Jq R per observation -> the 3x3 normal equations of the point), fold, step (every lane, the same
//                       bits: Jacobi scaling, LM diagonal, damped Cholesky), candidate cost, the decisions of lm_step.hpp on a
//                       state array in LDS that is the wave's own, epilogue (H, g, error sums at the final point)
// The kernel has no barrier, no atomic and no wait: the four waves of a workgroup are four unrelated solves.  Every sum has
// ONE order: a lane adds its observations in ascending position (the caller's order inside the point), the 64 lanes are folded by
// the xor butterfly, after which every lane holds the same bits, so everything behind a fold, branches included, is wave-uniform
// by construction.  The lane count is a constant, never chosen from the batch.
#pragma once
#include "../../include/lifcal_intersect.h"

namespace lifcal {

constexpr int IS_THREADS = 256, IS_WAVES = IS_THREADS / 64;
constexpr int IS_NH = 6, IS_G = 6, IS_COST = 9, IS_SXX = 10, IS_SYY = 11, IS_INL = 12, IS_NSWEEP = 10, IS_NEPI = 13;   // accumulator slots of a lane

struct IntersectArgs {
  const uint32_t* off;               // [P + 1] CSR of the observations by point
  const uint32_t* fr;                // [N] point-sorted, like u .. mcy
  const double *u, *v, *mcx, *mcy;
  const double *cu, *cu_stats;       // [2N] c_u for the folded parameters | for the parameters as stored
  const CamConsts* camc;             // [2] likewise
  const double *cam, *ft;            // [17], [F][FRAME_STRIDE]
  double* pts;                       // [3P] in / out
  lifcal_intersect_point* rows;      // [P], zeroed by the host
  LmOpts lo;
  double initial_radius, lm_min, lm_max, thr2;
  uint32_t n_points, robust, jacobi;
  // the MASKED instantiations only (lifcal_register_scene, register.hpp): the points with pmask[p] != 0 are solved, over their
  // observations in the frames with fstate[fr] == 1 (registered), and report to reg_rows instead of rows
  const uint32_t *fstate, *pmask;    // [F], [P]
  lifcal_register_point* reg_rows;   // [P]
};

__global__ __launch_bounds__(256) void k_intersect_frames(const double* __restrict__ views, uint32_t F, double* __restrict__ ft) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f < F) {
    double o[FRAME_STRIDE];
    frame_eval(views + 6 * (size_t)f, o);
#pragma unroll
    for (int k = 0; k < FRAME_STRIDE; ++k) ft[(size_t)f * FRAME_STRIDE + k] = o[k];
  }
}

// the inputs of one observation (loaded one step ahead of their use); the frame's table row is gathered at the use
struct IsObs { double u, v, mx, my, cux, cuy; uint32_t fr; };
LIFCAL_DEV IsObs is_load(const IntersectArgs& a, const double* __restrict__ cu, uint32_t i) {
  IsObs o;
  const double2 w = *reinterpret_cast<const double2*>(cu + 2 * (size_t)i);
  o.u = a.u[i]; o.v = a.v[i]; o.mx = a.mcx[i]; o.my = a.mcy[i]; o.cux = w.x; o.cuy = w.y; o.fr = a.fr[i];
  return o;
}

// normal equations of the point P over its observations [b, e), this lane's share: acc[0..5] H (lower, row-major), [6..8] g = J^T r,
// [9] cost; EPI: no cost, but [10], [11] sums of e_x^2, e_y^2 and [12] the inlier count of the plain errors
template <int NR, bool TAN, bool ADJ, bool EPI, bool MASKED = false>
LIFCAL_DEV void is_sweep(const IntersectArgs& a, const CamConsts& c, const double* __restrict__ cu, uint32_t b, uint32_t e, uint32_t lane,
                         double P0, double P1, double P2, double (&acc)[IS_NEPI]) {
#pragma unroll
  for (int k = 0; k < IS_NEPI; ++k) acc[k] = 0.0;
  double lmant = 1.0; int lexp = 0;   // Cauchy cost as a running mantissa / exponent product, one log per lane (as rs_sweep)
  uint32_t i = b + lane;
  IsObs nx = is_load(a, cu, min(i, e - 1));   // (clamped position: an unconditional load)
  for (; i < e; i += 64u) {
    const IsObs o = nx;
    nx = is_load(a, cu, min(i + 64u, e - 1));
    if (MASKED && a.fstate[o.fr] != 1u) continue;
    const double* __restrict__ ft = a.ft + (size_t)o.fr * FRAME_STRIDE;
    double R[12];
#pragma unroll
    for (int k = 0; k < 6; ++k) { const double2 w = *reinterpret_cast<const double2*>(ft + 2 * k); R[2 * k] = w.x; R[2 * k + 1] = w.y; }
    double r[2], Jq[2][3];
    obs_pose_eval<NR, TAN, ADJ>(c, R[0] * P0 + R[1] * P1 + R[2] * P2 + R[9], R[3] * P0 + R[4] * P1 + R[5] * P2 + R[10], R[6] * P0 + R[7] * P1 + R[8] * P2 + R[11],
                                o.mx, o.my, o.cux, o.cuy, o.u, o.v, r, Jq);
    const double sq = r[0] * r[0] + r[1] * r[1];
    if (EPI) { acc[IS_SXX] += r[0] * r[0]; acc[IS_SYY] += r[1] * r[1]; if (sq <= a.thr2) acc[IS_INL] += 1.0; }
    if (a.robust) {  // ceres::CauchyLoss + Corrector with rho'' < 0: r and J scaled by sqrt(rho'), as rs_sweep
      const double sum = 1.0 + sq * c.loss_c;
      if (!EPI) { int ex; lmant = frexp(lmant * sum, &ex); lexp += ex; }
      const double sc = sqrt(fmax(1.0 / sum, 2.2250738585072014e-308));
      r[0] *= sc; r[1] *= sc;
#pragma unroll
      for (int k = 0; k < 3; ++k) { Jq[0][k] *= sc; Jq[1][k] *= sc; }
    } else if (!EPI) {
      acc[IS_COST] += 0.5 * sq;
    }
    // J_P = Jq R (p_c = R P + t)
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      double J[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) J[k] = Jq[q][0] * R[k] + Jq[q][1] * R[3 + k] + Jq[q][2] * R[6 + k];
      int t = 0;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        acc[IS_G + m] += J[m] * r[q];
#pragma unroll
        for (int n = 0; n <= m; ++n) acc[t++] += J[m] * J[n];
      }
    }
  }
  if (!EPI && a.robust) acc[IS_COST] = 0.5 * c.loss_b * (log(lmant) + (double)lexp * 0.6931471805599453);
}

// value-only cost of the point at P, this lane's share (the candidate of a step)
template <int NR, bool TAN, bool ADJ, bool MASKED = false>
LIFCAL_DEV double is_cost(const IntersectArgs& a, const CamConsts& c, const double* __restrict__ cu, uint32_t b, uint32_t e, uint32_t lane,
                          double P0, double P1, double P2) {
  double cost = 0.0, lmant = 1.0; int lexp = 0;
  uint32_t i = b + lane;
  IsObs nx = is_load(a, cu, min(i, e - 1));
  for (; i < e; i += 64u) {
    const IsObs o = nx;
    nx = is_load(a, cu, min(i + 64u, e - 1));
    if (MASKED && a.fstate[o.fr] != 1u) continue;
    const double* __restrict__ ft = a.ft + (size_t)o.fr * FRAME_STRIDE;
    double R[12];
#pragma unroll
    for (int k = 0; k < 6; ++k) { const double2 w = *reinterpret_cast<const double2*>(ft + 2 * k); R[2 * k] = w.x; R[2 * k + 1] = w.y; }
    GroupConsts g;
    group_prepare(c, R[0] * P0 + R[1] * P1 + R[2] * P2 + R[9], R[3] * P0 + R[4] * P1 + R[5] * P2 + R[10], R[6] * P0 + R[7] * P1 + R[8] * P2 + R[11], g);
    double rx, ry;
    obs_value<NR, TAN, ADJ>(c, g, o.mx, o.my, o.cux, o.cuy, o.u, o.v, rx, ry);
    const double sq = rx * rx + ry * ry;
    if (a.robust) { int ex; lmant = frexp(lmant * (1.0 + sq * c.loss_c), &ex); lexp += ex; }
    else cost += 0.5 * sq;
  }
  if (a.robust) cost = 0.5 * c.loss_b * (log(lmant) + (double)lexp * 0.6931471805599453);
  return cost;
}

// The damped step of the 3x3 system, rs_step at three unknowns: (sig H sig + D2) y = sig g with
// D2 = clamp(diag(sig H sig), min, max) / radius, delta = -sig y; gtd = g^T delta, ddd = delta^T Lambda delta with Lambda = D2 / sig^2.
// false: a pivot of the Cholesky factorisation is not positive.  Every lane of the wave runs it on the same bits.
LIFCAL_DEV bool is_step(const double* H, const double* g, const double* sig, double radius, double lm_min, double lm_max, double* delta, double& gtd, double& ddd) {
  double A[IS_NH], D2[3], y[3];
  int t = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j, ++t) A[t] = H[t] * sig[i] * sig[j];
    D2[i] = fmin(fmax(A[t - 1], lm_min), lm_max) / radius;
    A[t - 1] += D2[i];
    y[i] = sig[i] * g[i];
  }
  bool ok = true;
#define IS_A(i, j) A[(i) * ((i) + 1) / 2 + (j)]
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double d = IS_A(j, j);
#pragma unroll
    for (int k = 0; k < j; ++k) d -= IS_A(j, k) * IS_A(j, k);
    if (!(d > 0.0) || !lm_finite(d)) ok = false;
    d = sqrt(d); IS_A(j, j) = d;
    const double di = 1.0 / d;
#pragma unroll
    for (int i = j + 1; i < 3; ++i) {
      double s = IS_A(i, j);
#pragma unroll
      for (int k = 0; k < j; ++k) s -= IS_A(i, k) * IS_A(j, k);
      IS_A(i, j) = s * di;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = y[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= IS_A(i, k) * y[k];
    y[i] = s / IS_A(i, i);
  }
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 3; ++k) s -= IS_A(k, i) * y[k];
    y[i] = s / IS_A(i, i);
  }
#undef IS_A
  gtd = 0.0; ddd = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) { const double dl = -y[i] * sig[i]; delta[i] = dl; gtd += g[i] * dl; ddd += D2[i] * y[i] * y[i]; }
  return ok;
}

// (three waves per SIMD: the allocation this bound asks for holds without a spill)
template <int NR, bool TAN, bool ADJ, bool MASKED = false>
__global__ __launch_bounds__(IS_THREADS, 3) void k_intersect(IntersectArgs a) {
  // The LM state of a wave: its own row, which no other wave touches.  All 64 lanes run the decisions of lm_step.hpp on it and
  // store the same bits to the same words in the same instruction, so a lane reads back what it wrote: the single-thread
  // program, 64 times in lockstep.  No barrier is needed (and none exists: the waves end after different numbers of iterations).
  __shared__ double s_lm[IS_WAVES][LM_N];
  double* lm = s_lm[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * IS_WAVES + (threadIdx.x >> 6)));   // wave w of block b owns point 4 b + w
  if (p >= a.n_points) return;
  const uint32_t b = a.off[p], e = a.off[p + 1];
  if (b == e) return;   // no observations: coordinates and (zeroed) row stay as they are
  if (MASKED) {   // not mapped, or no observation in a registered frame: a no-op that keeps coordinates and row
    if (!a.pmask[p]) return;
    double n = 0.0;
    for (uint32_t i = b + lane; i < e; i += 64u) if (a.fstate[a.fr[i]] == 1u) n += 1.0;
    if (wave_sum(n) == 0.0) return;
  }
  const CamConsts& c = a.camc[0];   // (read where used: a copy would sit in some 90 scalar registers for the whole solve)
  double acc[IS_NEPI], H[IS_NH], g[3], sig[3];
  double P0 = a.pts[3 * (size_t)p], P1 = a.pts[3 * (size_t)p + 1], P2 = a.pts[3 * (size_t)p + 2];
  double cam2 = 0.0;
  for (int k = 0; k < LIFCAL_BA_MAX_CAMERA_PARAMETERS; ++k) cam2 += a.cam[k] * a.cam[k];
  lm_reset(lm, a.initial_radius);

  // sweep + fold: afterwards every lane holds the same H, g and cost, and everything below is computed by all lanes alike
  auto sweep = [&]() {
    is_sweep<NR, TAN, ADJ, false, MASKED>(a, c, a.cu, b, e, lane, P0, P1, P2, acc);
#pragma unroll
    for (int k = 0; k < IS_NSWEEP; ++k) acc[k] = wave_sum(acc[k]);
#pragma unroll
    for (int k = 0; k < IS_NH; ++k) H[k] = acc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k] = acc[IS_G + k];
    lm_take_sweep(lm, a.lo, acc[IS_COST], fmax(fmax(fabs(g[0]), fabs(g[1])), fabs(g[2])), 0.0);
  };
  sweep();
#pragma unroll
  for (int k = 0; k < 3; ++k) sig[k] = a.jacobi ? 1.0 / (1.0 + sqrt(H[k * (k + 1) / 2 + k])) : 1.0;   // Jacobi scaling, fixed at iteration 0

  // every pass opens one LM iteration (lm_open_iteration counts them), so max_iterations + 1 passes reach the MAX_ITERATIONS exit
  for (int pass = 0; pass <= a.lo.max_iterations; ++pass) {
    if (lm[LM_TERMINATION] != 0.0 || !lm_open_iteration(lm, a.lo)) break;
    double delta[3], gtd, ddd;
    const bool ok = is_step(H, g, sig, lm[LM_RADIUS], a.lm_min, a.lm_max, delta, gtd, ddd);
    if (!lm_check_step(lm, gtd, ddd, ok ? 0.0 : 1.0)) continue;   // invalid step: the same system at half the radius (or the solve has ended)
    const double C0 = P0 + delta[0], C1 = P1 + delta[1], C2 = P2 + delta[2];
    const double cand = wave_sum(is_cost<NR, TAN, ADJ, MASKED>(a, c, a.cu, b, e, lane, C0, C1, C2));
    // |x|^2 over the camera block as stored and the point: the program of the one-point problem (its constant poses are no blocks)
    const double d0 = C0 - P0, d1 = C1 - P1, d2 = C2 - P2;
    double step2 = 0.0, x2 = cam2;
    step2 += d0 * d0; step2 += d1 * d1; step2 += d2 * d2;
    x2 += P0 * P0; x2 += P1 * P1; x2 += P2 * P2;
    lm_judge_step(lm, a.lo, cand, step2, x2);
    if (lm[LM_TERMINATION] == 0.0 && lm[LM_COMMIT] != 0.0) { P0 = C0; P1 = C1; P2 = C2; sweep(); }   // rejected: re-damp the stored H, g
  }

  // epilogue at the final point, parameters as stored (calcReprojectionError's rule: no sign folding, scale through float)
  if (MASKED) {   // the point and the solve's figures; the error sums of the row are taken once, at the end of the call
    if (lane == 0) {
      double* out = a.pts + 3 * (size_t)p;
      out[0] = P0; out[1] = P1; out[2] = P2;
      lifcal_register_point* row = a.reg_rows + p;
      row->final_cost = lm[LM_X_COST]; row->iterations = (int32_t)lm[LM_ITER];
      row->termination = lm[LM_TERMINATION] != 0.0 ? (int32_t)lm[LM_TERMINATION] : LIFCAL_BA_TERM_MAX_ITERATIONS;
    }
    return;
  }
  const CamConsts& cs = a.camc[1];
  is_sweep<NR, TAN, ADJ, true>(a, cs, a.cu_stats, b, e, lane, P0, P1, P2, acc);
#pragma unroll
  for (int k = 0; k < IS_NEPI; ++k) if (k != IS_COST) acc[k] = wave_sum(acc[k]);
  if (lane == 0) {
    double* out = a.pts + 3 * (size_t)p;
    out[0] = P0; out[1] = P1; out[2] = P2;
    lifcal_intersect_point* row = a.rows + p;
    row->initial_cost = lm[LM_INITIAL_COST]; row->final_cost = lm[LM_X_COST]; row->final_radius = lm[LM_RADIUS]; row->final_gradient_max_norm = lm[LM_GMAX];
#pragma unroll
    for (int k = 0; k < IS_NH; ++k) row->H[k] = acc[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) row->g[k] = acc[IS_G + k];
    row->sum_xx = acc[IS_SXX]; row->sum_yy = acc[IS_SYY];
    row->n_obs = e - b; row->n_inliers = (uint32_t)acc[IS_INL];
    row->iterations = (int32_t)lm[LM_ITER]; row->successful_steps = (int32_t)lm[LM_SUCCESSFUL]; row->unsuccessful_steps = (int32_t)lm[LM_UNSUCCESSFUL];
    row->termination = lm[LM_TERMINATION] != 0.0 ? (int32_t)lm[LM_TERMINATION] : LIFCAL_BA_TERM_MAX_ITERATIONS;   // as lm_fill_summary
  }
}

}  // namespace lifcal

namespace {

int intersect_impl(const lifcal_intersect_problem* p, const lifcal_ba_options* o, double inlier_threshold, lifcal_intersect_point* per_point, double* seconds) {
  if (int rc = batch_checks("lifcal_intersect_points", p, o, per_point, true)) return rc;
  if (seconds) *seconds = 0.0;
  const uint32_t N = p->n_obs, F = p->n_frames, P = p->n_points;
  if (!P) return 0;
  if (!N) { std::memset(per_point, 0, (size_t)P * sizeof(lifcal_intersect_point)); return 0; }   // no point has an observation (N > 0 implies F > 0)
  // the observations point-major, inside a point in the caller's order (stable counting sort)
  std::vector<uint32_t> off((size_t)P + 1), idx(N);
  if (int rc = lifcal_group_index(N, P, p->pt, off.data(), idx.data())) return rc;
  ByteLayout L;
  const size_t at_u = L.take((size_t)N * 8), at_v = L.take((size_t)N * 8), at_mx = L.take((size_t)N * 8), at_my = L.take((size_t)N * 8), at_fr = L.take((size_t)N * 4),
               at_off = L.take(((size_t)P + 1) * 4), at_cam = L.take(LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8), at_pts = L.take((size_t)P * 24), at_views = L.take((size_t)F * 48);
  const size_t in_bytes = L.bytes;
  const size_t at_cu = L.take((size_t)N * 16), at_cus = L.take((size_t)N * 16), at_camc = L.take(2 * sizeof(CamConsts)), at_ft = L.take((size_t)F * FRAME_STRIDE * 8),
               at_rows = L.take((size_t)P * sizeof(lifcal_intersect_point));
  std::vector<unsigned char> host(in_bytes);
  stage_observations(host, idx, N, p, at_u, at_v, at_mx, at_my, at_fr, p->fr);
  std::memcpy(host.data() + at_off, off.data(), off.size() * 4);
  std::memcpy(host.data() + at_cam, p->cam, LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8);
  std::memcpy(host.data() + at_pts, p->pts, (size_t)P * 24);
  std::memcpy(host.data() + at_views, p->views, (size_t)F * 48);

  if (int rc = mla::select_device(o->device, "lifcal_intersect_points")) return rc;
  BatchCall D(o->device, "lifcal_intersect_points");
  D.open(L.bytes);
  D.upload(host.data(), in_bytes);
  D.zero(at_rows, (size_t)P * sizeof(lifcal_intersect_point));
  D.begin();
  if (D.ok()) {
    unsigned char* const dev = D.dev;
    hipStream_t const stream = D.stream;
    IntersectArgs a{};   // (the mask fields of the MASKED instantiations stay null)
    a.off = (const uint32_t*)(dev + at_off); a.fr = (const uint32_t*)(dev + at_fr);
    a.u = (const double*)(dev + at_u); a.v = (const double*)(dev + at_v); a.mcx = (const double*)(dev + at_mx); a.mcy = (const double*)(dev + at_my);
    a.cu = (const double*)(dev + at_cu); a.cu_stats = (const double*)(dev + at_cus); a.camc = (const CamConsts*)(dev + at_camc);
    a.cam = (const double*)(dev + at_cam); a.ft = (const double*)(dev + at_ft); a.pts = (double*)(dev + at_pts);
    a.rows = (lifcal_intersect_point*)(dev + at_rows);
    a.lo = LmOpts{o->function_tolerance, o->parameter_tolerance, o->gradient_tolerance, o->min_relative_decrease, o->max_radius, o->min_radius, o->max_iterations};
    a.initial_radius = o->initial_radius; a.lm_min = o->min_lm_diagonal; a.lm_max = o->max_lm_diagonal; a.thr2 = inlier_threshold * inlier_threshold;
    a.n_points = P; a.robust = (p->config & LIFCAL_BA_CFG_ROBUST) ? 1u : 0u; a.jacobi = o->jacobi_scaling ? 1u : 0u;
    const uint32_t lens_grid = (N + 255u) / 256u, frame_grid = (F + 255u) / 256u, point_grid = (P + (uint32_t)IS_WAVES - 1u) / (uint32_t)IS_WAVES;
    const ModelCfg cfg = model_cfg(p->config);
    // (a dispatch table that refuses the configuration returns from here: D waits for the stream)
    hipLaunchKernelGGL(k_intersect_frames, dim3(frame_grid), dim3(256), 0, stream, (const double*)(dev + at_views), F, (double*)(dev + at_ft));
    for (int fold = 1; fold >= 0; --fold)
      if (int rc = launch_lens_pass(cfg, stream, lens_grid, a.cam, p->spx, p->spy, p->scale, o->loss_scale, fold, N, a.mcx, a.mcy, (CamConsts*)(dev + at_camc), (double*)(dev + (fold ? at_cu : at_cus)))) return rc;
#define CALL_INTERSECT(NR, TAN, ADJ) hipLaunchKernelGGL((k_intersect<NR, TAN, ADJ>), dim3(point_grid), dim3(IS_THREADS), 0, stream, a)
    DISPATCH_CFG(&cfg, CALL_INTERSECT);
#undef CALL_INTERSECT
  }
  D.end();
  D.download(p->pts, at_pts, (size_t)P * 24);
  D.download(per_point, at_rows, (size_t)P * sizeof(lifcal_intersect_point));
  return D.finish(seconds);
}

}  // namespace

extern "C" int lifcal_intersect_points(const lifcal_intersect_problem* p, const lifcal_ba_options* o, double inlier_threshold, lifcal_intersect_point* per_point, double* seconds) {
  return guard_abi("lifcal_intersect_points", [&] { return intersect_impl(p, o, inlier_threshold, per_point, seconds); });
}
