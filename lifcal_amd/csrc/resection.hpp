// resection.hpp — lifcal_resect_frames (include/lifcal_resect.h): its two kernels, then the host driver (included at the end of
// lifcal_ba.hip, behind lifcal_group_index and mla::select_device).  DESIGN.md section 7k.
//
//   k_resect_lens  the undistorted lens centre c_u of every observation, once per call (the camera is constant), and the camera
//                  constants; launched for the folded parameters (the solve) and for the parameters as stored (the epilogue)
//   k_resect       one workgroup per frame, persistent over the frame's whole Levenberg-Marquardt solve: sweep (residual and
//                  d r / d p_c per observation -> the 6x6 normal equations of the pose), step (one lane: Jacobi scaling, LM
//                  diagonal, damped Cholesky), candidate cost, the decisions of lm_step.hpp on a state array in LDS, epilogue
//                  (H, g, error sums at the final pose).  The host is not involved between iterations.
// Every sum has ONE order: a thread adds its observations in ascending position (the caller's order inside the frame), the lanes
// of a wave are folded by the xor butterfly, the waves in wave order through LDS.  No atomics.  The order depends on the workgroup
// size, which is therefore the same for every call (RS_THREADS), not a tuning choice made per problem.
#pragma once
#include "../../include/lifcal_resect.h"
#include "../../include/lifcal_register.h"

namespace lifcal {

constexpr int RS_THREADS = 256, RS_WAVES = RS_THREADS / 64;
constexpr int RS_NH = 21, RS_G = 21, RS_COST = 27, RS_SXX = 28, RS_SYY = 29, RS_INL = 30, RS_NSWEEP = 28, RS_NEPI = 31;   // accumulator slots of a thread
enum { RS_STOP = 0, RS_RETRY = 1, RS_CANDIDATE = 2, RS_COMMIT = 3 };

struct ResectArgs {
  const uint32_t* off;               // [F + 1] CSR of the observations by frame
  const uint32_t* pt;                // [N] frame-sorted, like u .. mcy
  const double *u, *v, *mcx, *mcy;
  const double *cu, *cu_stats;       // [2N] c_u for the folded parameters | for the parameters as stored
  const CamConsts* camc;             // [2] likewise
  const double *cam, *pts;           // [17], [3P]
  double* views;                     // [6F] in / out
  lifcal_resect_frame* rows;         // [F], zeroed by the host
  LmOpts lo;
  double initial_radius, lm_min, lm_max, thr2;
  uint32_t robust, jacobi;
  // the MASKED instantiations only (lifcal_register_scene, register.hpp): the frames with fstate[f] == fwant apart from skip_frame
  // are solved, over their observations of the points with pmask[pt] != 0, and report to reg_rows instead of rows
  const uint32_t *pmask, *fstate;    // [P], [F]
  lifcal_register_frame* reg_rows;   // [F]
  uint32_t fwant, skip_frame;
};

template <int NR, bool TAN>
__global__ __launch_bounds__(256) void k_resect_lens(const double* cam, double spx, double spy, double scale, double loss_scale, int fold, uint32_t n,
                                                     const double* __restrict__ mcx, const double* __restrict__ mcy, CamConsts* camc_out, double* __restrict__ cu_out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  CamConsts c;   // (every camera slot constant: chm = 0, no camera column exists here)
  cam_prepare(cam, spx, spy, fold ? scale : (double)(float)scale, NR, TAN, 0x1FFFFu, loss_scale, fold != 0, c);
  if (t == 0) *camc_out = c;
  if (t < n) {
    double o[4];
    lens_eval<NR, TAN>(c, mcx[t], mcy[t], false, o);
    *reinterpret_cast<double2*>(cu_out + 2 * (size_t)t) = make_double2(o[2], o[3]);
  }
}

// residual and Jq = d r / d(camera-frame point) of one observation: obs_eval without its camera columns
template <int NR, bool TAN, bool ADJ>
LIFCAL_DEV void obs_pose_eval(const CamConsts& c, double X, double Y, double Z, double mx, double my, double cux, double cuy, double u, double v,
                              double r[2], double Jq[2][3]) {
  const double iZq = 1.0 / (Z + c.zC0), gz = c.gamma * iZq;
  const double wx = ADJ ? cux * c.a : cux, wy = ADJ ? cuy * c.a : cuy;
  const double qx = (X + wx * c.e) * iZq, qy = (Y + wy * c.e) * iZq;
  const double mlx = c.gamma * qx - c.beta * wx, mly = c.gamma * qy - c.beta * wy;
  const double qxZ = -gz * qx, qyZ = -gz * qy;
  double px, py;
  double j00 = gz, j01 = 0.0, j02 = qxZ, j10 = 0.0, j11 = gz, j12 = qyZ;  // d proj / d (X,Y,Z)
  if (ADJ) {
    px = mlx + wx; py = mly + wy;
    if (NR > 0 || TAN) {
      Distortion<NR, TAN> d; d.eval(px, py, c, true);
      const double b00 = 1.0 + d.A00, b01 = d.A01, b10 = d.A10, b11 = 1.0 + d.A11;
      j00 = b00 * gz; j01 = b01 * gz; j02 = b00 * qxZ + b01 * qyZ;
      j10 = b10 * gz; j11 = b11 * gz; j12 = b10 * qxZ + b11 * qyZ;
      px += d.dx; py += d.dy;
    }
  } else {
    px = mlx + (mx - c.craw[0]) * c.sp[0]; py = mly + (my - c.craw[1]) * c.sp[1];
  }
  r[0] = px * c.isp[0] + c.craw[0] - u;
  r[1] = py * c.isp[1] + c.craw[1] - v;
  Jq[0][0] = j00 * c.isp[0]; Jq[0][1] = j01 * c.isp[0]; Jq[0][2] = j02 * c.isp[0];
  Jq[1][0] = j10 * c.isp[1]; Jq[1][1] = j11 * c.isp[1]; Jq[1][2] = j12 * c.isp[1];
}

// the inputs of one observation (loaded one step ahead of their use)
struct RsObs { double u, v, mx, my, cux, cuy, P0, P1, P2; };
LIFCAL_DEV RsObs rs_load(const ResectArgs& a, const double* __restrict__ cu, uint32_t i) {
  RsObs o;
  const double* P = a.pts + 3 * (size_t)a.pt[i];
  const double2 w = *reinterpret_cast<const double2*>(cu + 2 * (size_t)i);
  o.u = a.u[i]; o.v = a.v[i]; o.mx = a.mcx[i]; o.my = a.mcy[i]; o.cux = w.x; o.cuy = w.y;
  o.P0 = P[0]; o.P1 = P[1]; o.P2 = P[2];
  return o;
}

// the threads' accumulators -> out[0 .. K): xor butterfly inside a wave, then the waves in wave order.  Called by all threads.
template <int K, int KA>
LIFCAL_DEV void rs_fold(double (&acc)[KA], double* red /* LDS [RS_WAVES * K] */, double* out /* LDS [K] */) {
  static_assert(K <= KA && K <= 64, "one lane per value in the second stage");
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = wave_sum(acc[k]);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave * K + k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < (uint32_t)K) {
    double s = red[threadIdx.x];
    for (uint32_t w = 1; w < (blockDim.x >> 6); ++w) s += red[w * K + threadIdx.x];
    out[threadIdx.x] = s;
  }
  __syncthreads();
}

// normal equations of the pose over the observations [b, e) of the frame whose table is ft: acc[0..20] H (lower, row-major),
// [21..26] g = J^T r, [27] cost; EPI: no cost, but [28], [29] sums of e_x^2, e_y^2 and [30] the inlier count of the plain errors
template <int NR, bool TAN, bool ADJ, bool EPI, bool MASKED = false>
LIFCAL_DEV void rs_sweep(const ResectArgs& a, const CamConsts& c, const double* ft, const double* __restrict__ cu, uint32_t b, uint32_t e,
                         double (&acc)[RS_NEPI]) {
#pragma unroll
  for (int k = 0; k < RS_NEPI; ++k) acc[k] = 0.0;
  double lmant = 1.0; int lexp = 0;   // Cauchy cost as a running mantissa / exponent product, one log per thread (as k_cost)
  const double c0 = ft[12], s0 = ft[13], n0 = ft[2], n1 = ft[5], n2 = ft[8];
  uint32_t i = b + threadIdx.x;
  RsObs nx = rs_load(a, cu, min(i, e - 1));   // (clamped position: an unconditional load)
  for (; i < e; i += blockDim.x) {
    const RsObs o = nx;
    nx = rs_load(a, cu, min(i + blockDim.x, e - 1));
    if (MASKED && !a.pmask[a.pt[i]]) continue;
    const double Y0 = ft[0] * o.P0 + ft[1] * o.P1 + ft[2] * o.P2, Y1 = ft[3] * o.P0 + ft[4] * o.P1 + ft[5] * o.P2, Y2 = ft[6] * o.P0 + ft[7] * o.P1 + ft[8] * o.P2;
    double r[2], Jq[2][3];
    obs_pose_eval<NR, TAN, ADJ>(c, Y0 + ft[9], Y1 + ft[10], Y2 + ft[11], o.mx, o.my, o.cux, o.cuy, o.u, o.v, r, Jq);
    const double sq = r[0] * r[0] + r[1] * r[1];
    if (EPI) { acc[RS_SXX] += r[0] * r[0]; acc[RS_SYY] += r[1] * r[1]; if (sq <= a.thr2) acc[RS_INL] += 1.0; }
    if (a.robust) {  // ceres::CauchyLoss + Corrector with rho'' < 0: r and J scaled by sqrt(rho'), as k_sweep
      const double sum = 1.0 + sq * c.loss_c;
      if (!EPI) { int ex; lmant = frexp(lmant * sum, &ex); lexp += ex; }
      const double sc = sqrt(fmax(1.0 / sum, 2.2250738585072014e-308));
      r[0] *= sc; r[1] *= sc;
#pragma unroll
      for (int k = 0; k < 3; ++k) { Jq[0][k] *= sc; Jq[1][k] *= sc; }
    } else if (!EPI) {
      acc[RS_COST] += 0.5 * sq;
    }
    // J_pose = Jq [Gr | I], Gr = [e_x x Y, (0, c0, s0) x Y, R[:,2] x Y] with Y = R P (frame_eval's axes, group_transform's Gr)
    const double G01 = c0 * Y2 - s0 * Y1, G02 = n1 * Y2 - n2 * Y1, G11 = s0 * Y0, G12 = n2 * Y0 - n0 * Y2, G21 = -c0 * Y0, G22 = n0 * Y1 - n1 * Y0;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      double J[6];
      J[0] = Jq[q][2] * Y1 - Jq[q][1] * Y2;
      J[1] = Jq[q][0] * G01 + Jq[q][1] * G11 + Jq[q][2] * G21;
      J[2] = Jq[q][0] * G02 + Jq[q][1] * G12 + Jq[q][2] * G22;
      J[3] = Jq[q][0]; J[4] = Jq[q][1]; J[5] = Jq[q][2];
      int t = 0;
#pragma unroll
      for (int m = 0; m < 6; ++m) {
        acc[RS_G + m] += J[m] * r[q];
#pragma unroll
        for (int n = 0; n <= m; ++n) acc[t++] += J[m] * J[n];
      }
    }
  }
  if (!EPI && a.robust) acc[RS_COST] = 0.5 * c.loss_b * (log(lmant) + (double)lexp * 0.6931471805599453);
}

// value-only cost of the frame at the pose whose table is ft (the candidate of a step)
template <int NR, bool TAN, bool ADJ, bool MASKED = false>
LIFCAL_DEV double rs_cost(const ResectArgs& a, const CamConsts& c, const double* ft, const double* __restrict__ cu, uint32_t b, uint32_t e) {
  double cost = 0.0, lmant = 1.0; int lexp = 0;
  uint32_t i = b + threadIdx.x;
  RsObs nx = rs_load(a, cu, min(i, e - 1));
  for (; i < e; i += blockDim.x) {
    const RsObs o = nx;
    nx = rs_load(a, cu, min(i + blockDim.x, e - 1));
    if (MASKED && !a.pmask[a.pt[i]]) continue;
    GroupConsts g;
    group_prepare(c, ft[0] * o.P0 + ft[1] * o.P1 + ft[2] * o.P2 + ft[9], ft[3] * o.P0 + ft[4] * o.P1 + ft[5] * o.P2 + ft[10],
                  ft[6] * o.P0 + ft[7] * o.P1 + ft[8] * o.P2 + ft[11], g);
    double rx, ry;
    obs_value<NR, TAN, ADJ>(c, g, o.mx, o.my, o.cux, o.cuy, o.u, o.v, rx, ry);
    const double sq = rx * rx + ry * ry;
    if (a.robust) { int ex; lmant = frexp(lmant * (1.0 + sq * c.loss_c), &ex); lexp += ex; }
    else cost += 0.5 * sq;
  }
  if (a.robust) cost = 0.5 * c.loss_b * (log(lmant) + (double)lexp * 0.6931471805599453);
  return cost;
}

// One lane: the damped step of the 6x6 system.  (sig H sig + D2) y = sig g with D2 = clamp(diag(sig H sig), min, max) / radius
// (ceres LevenbergMarquardtStrategy on the Jacobi-scaled matrix), delta = -sig y; gtd = g^T delta, ddd = delta^T Lambda delta with
// Lambda = D2 / sig^2, the two numbers lm_check_step takes.  false: a pivot of the Cholesky factorisation is not positive.
LIFCAL_DEV bool rs_step(const double* H, const double* g, const double* sig, double radius, double lm_min, double lm_max, double* delta, double& gtd, double& ddd) {
  double A[RS_NH], D2[6], y[6];
  int t = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j, ++t) A[t] = H[t] * sig[i] * sig[j];
    D2[i] = fmin(fmax(A[t - 1], lm_min), lm_max) / radius;
    A[t - 1] += D2[i];
    y[i] = sig[i] * g[i];
  }
  bool ok = true;
#define RS_A(i, j) A[(i) * ((i) + 1) / 2 + (j)]
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = RS_A(j, j);
#pragma unroll
    for (int k = 0; k < j; ++k) d -= RS_A(j, k) * RS_A(j, k);
    if (!(d > 0.0) || !lm_finite(d)) ok = false;
    d = sqrt(d); RS_A(j, j) = d;
    const double di = 1.0 / d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double s = RS_A(i, j);
#pragma unroll
      for (int k = 0; k < j; ++k) s -= RS_A(i, k) * RS_A(j, k);
      RS_A(i, j) = s * di;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double s = y[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= RS_A(i, k) * y[k];
    y[i] = s / RS_A(i, i);
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) s -= RS_A(k, i) * y[k];
    y[i] = s / RS_A(i, i);
  }
#undef RS_A
  gtd = 0.0; ddd = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) { const double dl = -y[i] * sig[i]; delta[i] = dl; gtd += g[i] * dl; ddd += D2[i] * y[i] * y[i]; }
  return ok;
}

template <int NR, bool TAN, bool ADJ, bool MASKED = false>
__global__ __launch_bounds__(RS_THREADS) void k_resect(ResectArgs a) {
  __shared__ double s_ft[FRAME_STRIDE], s_ftc[FRAME_STRIDE], s_x[6], s_xc[6], s_sig[6], s_delta[6], s_lm[LM_N];
  __shared__ double s_acc[RS_NEPI], s_cand[1], s_cam2[1], s_red[RS_WAVES * RS_NEPI];
  __shared__ int s_state;
  const uint32_t f = blockIdx.x, tid = threadIdx.x;
  const uint32_t b = a.off[f], e = a.off[f + 1];
  if (b == e) return;   // no observations: pose and (zeroed) row stay as they are
  if (MASKED && (a.fstate[f] != a.fwant || f == a.skip_frame)) return;
  const CamConsts c = a.camc[0];
  double acc[RS_NEPI];
  if (MASKED) {   // no observation of a mapped point: a no-op that keeps pose and row
    acc[0] = 0.0;
    for (uint32_t i = b + tid; i < e; i += blockDim.x) if (a.pmask[a.pt[i]]) acc[0] += 1.0;
    rs_fold<1>(acc, s_red, s_cand);
    if (s_cand[0] == 0.0) return;
  }

  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) s_x[k] = a.views[6 * (size_t)f + k];
    frame_eval(s_x, s_ft);
    lm_reset(s_lm, a.initial_radius);
    double c2 = 0.0;
    for (int k = 0; k < LIFCAL_BA_MAX_CAMERA_PARAMETERS; ++k) c2 += a.cam[k] * a.cam[k];
    s_cam2[0] = c2;
  }
  __syncthreads();
  rs_sweep<NR, TAN, ADJ, false, MASKED>(a, c, s_ft, a.cu, b, e, acc);
  rs_fold<RS_NSWEEP>(acc, s_red, s_acc);
  if (tid == 0) {
    double gmax = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      gmax = fmax(gmax, fabs(s_acc[RS_G + k]));
      s_sig[k] = a.jacobi ? 1.0 / (1.0 + sqrt(s_acc[k * (k + 1) / 2 + k])) : 1.0;   // Jacobi scaling, fixed at iteration 0
    }
    lm_take_sweep(s_lm, a.lo, s_acc[RS_COST], gmax, 0.0);
  }
  __syncthreads();

  // every pass opens one LM iteration (lm_open_iteration counts them), so max_iterations + 1 passes reach the MAX_ITERATIONS exit
  for (int pass = 0; pass <= a.lo.max_iterations; ++pass) {
    if (tid == 0) {
      int st = RS_STOP;
      if (s_lm[LM_TERMINATION] == 0.0 && lm_open_iteration(s_lm, a.lo)) {
        double gtd, ddd;
        const bool ok = rs_step(s_acc, s_acc + RS_G, s_sig, s_lm[LM_RADIUS], a.lm_min, a.lm_max, s_delta, gtd, ddd);
        if (lm_check_step(s_lm, gtd, ddd, ok ? 0.0 : 1.0)) {
#pragma unroll
          for (int k = 0; k < 6; ++k) s_xc[k] = s_x[k] + s_delta[k];
          frame_eval(s_xc, s_ftc);
          st = RS_CANDIDATE;
        } else if (s_lm[LM_TERMINATION] == 0.0) {
          st = RS_RETRY;   // invalid step: the same system at half the radius
        }
      }
      s_state = st;
    }
    __syncthreads();
    int st = s_state;
    if (st == RS_STOP) break;
    if (st == RS_CANDIDATE) {
      acc[0] = rs_cost<NR, TAN, ADJ, MASKED>(a, c, s_ftc, a.cu, b, e);
      rs_fold<1>(acc, s_red, s_cand);
      if (tid == 0) {
        double step2 = 0.0, x2 = s_cam2[0];   // |x|^2 over the camera block as stored and the pose: the program of the one-frame problem
#pragma unroll
        for (int k = 0; k < 6; ++k) { const double dx = s_xc[k] - s_x[k]; step2 += dx * dx; x2 += s_x[k] * s_x[k]; }
        lm_judge_step(s_lm, a.lo, s_cand[0], step2, x2);
        st = RS_STOP;
        if (s_lm[LM_TERMINATION] == 0.0) {
          st = RS_RETRY;
          if (s_lm[LM_COMMIT] != 0.0) {
            st = RS_COMMIT;
#pragma unroll
            for (int k = 0; k < 6; ++k) s_x[k] = s_xc[k];
#pragma unroll
            for (int k = 0; k < FRAME_STRIDE; ++k) s_ft[k] = s_ftc[k];
          }
        }
        s_state = st;
      }
      __syncthreads();
      st = s_state;
      if (st == RS_STOP) break;
      if (st == RS_COMMIT) {
        rs_sweep<NR, TAN, ADJ, false, MASKED>(a, c, s_ft, a.cu, b, e, acc);
        rs_fold<RS_NSWEEP>(acc, s_red, s_acc);
        if (tid == 0) {
          double gmax = 0.0;
#pragma unroll
          for (int k = 0; k < 6; ++k) gmax = fmax(gmax, fabs(s_acc[RS_G + k]));
          lm_take_sweep(s_lm, a.lo, s_acc[RS_COST], gmax, 0.0);
        }
      }
    }
    __syncthreads();   // s_state is read by everyone before the next pass rewrites it; the state of lane 0 is visible
  }

  // epilogue at the final pose, parameters as stored (calcReprojectionError's rule: no sign folding, scale through float)
  __syncthreads();
  if (MASKED) {   // the pose and the solve's figures; the error sums of the row are taken once, at the end of the call
    if (tid < 6) a.views[6 * (size_t)f + tid] = s_x[tid];
    if (tid == 0) {
      lifcal_register_frame* row = a.reg_rows + f;
      row->final_cost = s_lm[LM_X_COST]; row->iterations = (int32_t)s_lm[LM_ITER];
      row->termination = s_lm[LM_TERMINATION] != 0.0 ? (int32_t)s_lm[LM_TERMINATION] : LIFCAL_BA_TERM_MAX_ITERATIONS;
    }
    return;
  }
  const CamConsts cs = a.camc[1];
  rs_sweep<NR, TAN, ADJ, true>(a, cs, s_ft, a.cu_stats, b, e, acc);
  rs_fold<RS_NEPI>(acc, s_red, s_acc);
  if (tid < 6) a.views[6 * (size_t)f + tid] = s_x[tid];
  if (tid == 0) {
    lifcal_resect_frame* row = a.rows + f;
    row->initial_cost = s_lm[LM_INITIAL_COST]; row->final_cost = s_lm[LM_X_COST]; row->final_radius = s_lm[LM_RADIUS]; row->final_gradient_max_norm = s_lm[LM_GMAX];
    for (int k = 0; k < RS_NH; ++k) row->H[k] = s_acc[k];
    for (int k = 0; k < 6; ++k) row->g[k] = s_acc[RS_G + k];
    row->sum_xx = s_acc[RS_SXX]; row->sum_yy = s_acc[RS_SYY];
    row->n_obs = e - b; row->n_inliers = (uint32_t)s_acc[RS_INL];
    row->iterations = (int32_t)s_lm[LM_ITER]; row->successful_steps = (int32_t)s_lm[LM_SUCCESSFUL]; row->unsuccessful_steps = (int32_t)s_lm[LM_UNSUCCESSFUL];
    row->termination = s_lm[LM_TERMINATION] != 0.0 ? (int32_t)s_lm[LM_TERMINATION] : LIFCAL_BA_TERM_MAX_ITERATIONS;   // as lm_fill_summary
  }
}

}  // namespace lifcal

namespace {

int resect_impl(const lifcal_resect_problem* p, const lifcal_ba_options* o, double inlier_threshold, lifcal_resect_frame* per_frame, double* seconds) {
  if (int rc = batch_checks("lifcal_resect_frames", p, o, per_frame, false)) return rc;
  if (seconds) *seconds = 0.0;
  const uint32_t N = p->n_obs, F = p->n_frames, P = p->n_points;
  if (!F) return 0;
  // the observations frame-major, inside a frame in the caller's order (stable counting sort)
  std::vector<uint32_t> off((size_t)F + 1), idx(N);
  if (int rc = lifcal_group_index(N, F, p->fr, off.data(), idx.data())) return rc;
  ByteLayout L;
  const size_t at_u = L.take((size_t)N * 8), at_v = L.take((size_t)N * 8), at_mx = L.take((size_t)N * 8), at_my = L.take((size_t)N * 8), at_pt = L.take((size_t)N * 4),
               at_off = L.take(((size_t)F + 1) * 4), at_cam = L.take(LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8), at_pts = L.take((size_t)P * 24), at_views = L.take((size_t)F * 48);
  const size_t in_bytes = L.bytes;
  const size_t at_cu = L.take((size_t)N * 16), at_cus = L.take((size_t)N * 16), at_camc = L.take(2 * sizeof(CamConsts)), at_rows = L.take((size_t)F * sizeof(lifcal_resect_frame));
  std::vector<unsigned char> host(in_bytes);
  stage_observations(host, idx, N, p, at_u, at_v, at_mx, at_my, at_pt, p->pt);
  std::memcpy(host.data() + at_off, off.data(), off.size() * 4);
  std::memcpy(host.data() + at_cam, p->cam, LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8);
  if (P) std::memcpy(host.data() + at_pts, p->pts, (size_t)P * 24);
  std::memcpy(host.data() + at_views, p->views, (size_t)F * 48);

  if (int rc = mla::select_device(o->device, "lifcal_resect_frames")) return rc;
  BatchCall D(o->device, "lifcal_resect_frames");
  D.open(L.bytes);
  D.upload(host.data(), in_bytes);
  D.zero(at_rows, (size_t)F * sizeof(lifcal_resect_frame));
  D.begin();
  if (D.ok()) {
    unsigned char* const dev = D.dev;
    hipStream_t const stream = D.stream;
    ResectArgs a{};   // (the mask fields of the MASKED instantiations stay null)
    a.off = (const uint32_t*)(dev + at_off); a.pt = (const uint32_t*)(dev + at_pt);
    a.u = (const double*)(dev + at_u); a.v = (const double*)(dev + at_v); a.mcx = (const double*)(dev + at_mx); a.mcy = (const double*)(dev + at_my);
    a.cu = (const double*)(dev + at_cu); a.cu_stats = (const double*)(dev + at_cus); a.camc = (const CamConsts*)(dev + at_camc);
    a.cam = (const double*)(dev + at_cam); a.pts = (const double*)(dev + at_pts); a.views = (double*)(dev + at_views);
    a.rows = (lifcal_resect_frame*)(dev + at_rows);
    a.lo = LmOpts{o->function_tolerance, o->parameter_tolerance, o->gradient_tolerance, o->min_relative_decrease, o->max_radius, o->min_radius, o->max_iterations};
    a.initial_radius = o->initial_radius; a.lm_min = o->min_lm_diagonal; a.lm_max = o->max_lm_diagonal; a.thr2 = inlier_threshold * inlier_threshold;
    a.robust = (p->config & LIFCAL_BA_CFG_ROBUST) ? 1u : 0u; a.jacobi = o->jacobi_scaling ? 1u : 0u;
    const uint32_t lens_grid = std::max(1u, (N + 255u) / 256u);
    const ModelCfg cfg = model_cfg(p->config);
    // (a dispatch table that refuses the configuration returns from here: D waits for the stream)
    for (int fold = 1; fold >= 0; --fold)
      if (int rc = launch_lens_pass(cfg, stream, lens_grid, a.cam, p->spx, p->spy, p->scale, o->loss_scale, fold, N, a.mcx, a.mcy, (CamConsts*)(dev + at_camc), (double*)(dev + (fold ? at_cu : at_cus)))) return rc;
#define CALL_RESECT(NR, TAN, ADJ) hipLaunchKernelGGL((k_resect<NR, TAN, ADJ>), dim3(F), dim3(RS_THREADS), 0, stream, a)
    DISPATCH_CFG(&cfg, CALL_RESECT);
#undef CALL_RESECT
  }
  D.end();
  D.download(p->views, at_views, (size_t)F * 48);
  D.download(per_frame, at_rows, (size_t)F * sizeof(lifcal_resect_frame));
  return D.finish(seconds);
}

}  // namespace

extern "C" int lifcal_resect_frames(const lifcal_resect_problem* p, const lifcal_ba_options* o, double inlier_threshold, lifcal_resect_frame* per_frame, double* seconds) {
  return guard_abi("lifcal_resect_frames", [&] { return resect_impl(p, o, inlier_threshold, per_frame, seconds); });
}
