// start.hpp — lifcal_start_poses and lifcal_start_points (include/lifcal_start.h): closed-form start values from micro-image
// rays.  Its kernels, then the host drivers (included at the end of lifcal_ba.hip, behind resection.hpp and intersection.hpp,
// whose k_resect_lens, rs_fold and k_intersect_frames it reuses).  DESIGN.md section 7n.
//
//   k_resect_lens    (resection.hpp) c_u of every observation and the camera constants, folded | as stored
//   start_ray        the two rows of one observation: linear in the camera-frame point once (u, v) is given
//   k_start_groups   one lane per (frame, point) group: the 3x3 normal equations of the group's rows, serially in the caller's
//                    order, Jacobi-scaled Cholesky in registers -> camera-frame point, triangulation residual, status
//   k_start_align    one workgroup per frame: weighted centroids and centred moment of its used groups (two passes, rs_fold),
//                    Horn's 4x4 matrix, cyclic Jacobi, R, t, Euler angles (one lane), then the alignment residual over the groups
//                    and the reprojection sums over the frame's observations at the new pose
//   k_start_points   one wave64 per point: the rows of all its observations carried into the world frame, nine accumulators, the
//                    xor butterfly, the 3x3 solve in every lane, the reprojection sums at the new point.  No barrier, no atomic.
// Every sum has ONE order: a lane adds in ascending position, lanes are folded by wave_sum / rs_fold.
#pragma once
#include "../../include/lifcal_start.h"

namespace lifcal {

constexpr int ST_THREADS = 256, ST_WAVES = ST_THREADS / 64;

// The two rows of one observation, [ax 0 azx] p_c = bx and [0 ay azy] p_c = by, divided by the pixel size so that the residual
// over Zq = Z + zC0 is the reprojection error in pixels to first order.  From ml = gamma q - beta w, q = ((X, Y) + w e) / Zq:
// s = ml + beta w = gamma q, hence gamma X - s_x Z = s_x zC0 - gamma e w_x (and likewise in y).  ml comes from the observation:
// without mlCenterAdj the c_raw and c_d terms cancel, with it the distorted point is inverted by lens_eval's ten sweeps.
template <int NR, bool TAN, bool ADJ>
LIFCAL_DEV void start_ray(const CamConsts& c, double u, double v, double mx, double my, double cux, double cuy,
                          double& ax, double& azx, double& bx, double& ay, double& azy, double& by) {
  const double wx = ADJ ? cux * c.a : cux, wy = ADJ ? cuy * c.a : cuy;
  double mlx, mly;
  if (ADJ) {
    const double px = (u - c.craw[0]) * c.sp[0], py = (v - c.craw[1]) * c.sp[1];
    double x = px, y = py;
    if (NR > 0 || TAN) {
      Distortion<NR, TAN> d;
      for (int it = 0; it < 10; ++it) { d.eval(x, y, c, false); x = px - d.dx; y = py - d.dy; }
    }
    mlx = x - wx; mly = y - wy;
  } else {
    mlx = (u - mx) * c.sp[0]; mly = (v - my) * c.sp[1];
  }
  const double sx = mlx + c.beta * wx, sy = mly + c.beta * wy, ge = c.gamma * c.e;
  ax = c.gamma * c.isp[0]; azx = -sx * c.isp[0]; bx = (sx * c.zC0 - ge * wx) * c.isp[0];
  ay = c.gamma * c.isp[1]; azy = -sy * c.isp[1]; by = (sy * c.zC0 - ge * wy) * c.isp[1];
}

// x of H x = g (H: lower triangle, row-major) through the Jacobi-scaled matrix d H d, d = 1 / sqrt(diag H), and its Cholesky
// factor in registers.  false: a pivot is not positive or not finite, or the result is not finite.  min_pivot: the smallest pivot
// of the scaled matrix (its diagonal is 1, so this is 1 for orthogonal columns and falls towards 0 as they align).
LIFCAL_DEV bool start_solve3(const double (&H)[6], const double (&g)[3], double (&x)[3], double& min_pivot) {
  double d[3], A[6], y[3];
  d[0] = 1.0 / sqrt(H[0]); d[1] = 1.0 / sqrt(H[2]); d[2] = 1.0 / sqrt(H[5]);
  int t = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j, ++t) A[t] = H[t] * d[i] * d[j];
    y[i] = d[i] * g[i];
  }
  bool ok = true;
  min_pivot = 1.7976931348623157e308;
#define ST_A(i, j) A[(i) * ((i) + 1) / 2 + (j)]
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    double piv = ST_A(j, j);
#pragma unroll
    for (int k = 0; k < j; ++k) piv -= ST_A(j, k) * ST_A(j, k);
    if (!(piv > 0.0) || !lm_finite(piv)) ok = false;
    min_pivot = fmin(min_pivot, piv);
    piv = sqrt(piv); ST_A(j, j) = piv;
    const double di = 1.0 / piv;
#pragma unroll
    for (int i = j + 1; i < 3; ++i) {
      double s = ST_A(i, j);
#pragma unroll
      for (int k = 0; k < j; ++k) s -= ST_A(i, k) * ST_A(j, k);
      ST_A(i, j) = s * di;
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double s = y[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= ST_A(i, k) * y[k];
    y[i] = s / ST_A(i, i);
  }
#pragma unroll
  for (int i = 2; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < 3; ++k) s -= ST_A(k, i) * y[k];
    y[i] = s / ST_A(i, i);
  }
#undef ST_A
#pragma unroll
  for (int i = 0; i < 3; ++i) { x[i] = d[i] * y[i]; if (!lm_finite(x[i])) ok = false; }
  return ok;
}

struct StartGroupArgs {
  const uint32_t *goff, *gfr, *gpt;   // [G + 1] CSR of the observations by group, [G] frame and point of the group
  const double *u, *v, *mcx, *mcy;    // [N] sorted (fr, pt)-major, inside a group in the caller's order
  const double* cu;                   // [2N] c_u for the folded parameters
  const CamConsts* camc;              // [2] folded | as stored
  lifcal_start_group* groups;         // [G]
  double gate_px;
  uint32_t n_groups;
};

// One lane per group.  A group has 3 - 8 observations, so a lane walks its run serially: the fixed order comes for free, at the
// price of neighbouring lanes reading about 40 bytes apart per array (accepted for this first form).
template <int NR, bool TAN, bool ADJ>
__global__ __launch_bounds__(ST_THREADS) void k_start_groups(StartGroupArgs a) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= a.n_groups) return;
  const CamConsts& c = a.camc[0];
  const uint32_t b = a.goff[g], e = a.goff[g + 1];
  double x[3] = {0.0, 0.0, 0.0}, rms = 0.0;
  int32_t status = LIFCAL_START_GROUP_SINGLE;
  if (e - b > 1u) {
    double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, gv[3] = {0.0, 0.0, 0.0}, mp;
    for (uint32_t i = b; i < e; ++i) {
      const double2 w = *reinterpret_cast<const double2*>(a.cu + 2 * (size_t)i);
      double ax, azx, bx, ay, azy, by;
      start_ray<NR, TAN, ADJ>(c, a.u[i], a.v[i], a.mcx[i], a.mcy[i], w.x, w.y, ax, azx, bx, ay, azy, by);
      H[0] += ax * ax; H[2] += ay * ay; H[3] += ax * azx; H[4] += ay * azy; H[5] += azx * azx + azy * azy;
      gv[0] += ax * bx; gv[1] += ay * by; gv[2] += azx * bx + azy * by;
    }
    if (!start_solve3(H, gv, x, mp)) {
      status = LIFCAL_START_GROUP_SINGULAR;
      x[0] = 0.0; x[1] = 0.0; x[2] = 0.0;
    } else {
      const double iZq = 1.0 / (x[2] + c.zC0);
      double ss = 0.0;
      for (uint32_t i = b; i < e; ++i) {
        const double2 w = *reinterpret_cast<const double2*>(a.cu + 2 * (size_t)i);
        double ax, azx, bx, ay, azy, by;
        start_ray<NR, TAN, ADJ>(c, a.u[i], a.v[i], a.mcx[i], a.mcy[i], w.x, w.y, ax, azx, bx, ay, azy, by);
        const double rx = (ax * x[0] + azx * x[2] - bx) * iZq, ry = (ay * x[1] + azy * x[2] - by) * iZq;
        ss += rx * rx + ry * ry;
      }
      rms = sqrt(ss / (double)(e - b));
      status = x[2] <= 0.0 ? LIFCAL_START_GROUP_BEHIND : (rms > a.gate_px ? LIFCAL_START_GROUP_GATED : LIFCAL_START_GROUP_USED);
    }
  }
  lifcal_start_group row;
  row.xyz[0] = x[0]; row.xyz[1] = x[1]; row.xyz[2] = x[2]; row.rms_px = rms;
  row.fr = a.gfr[g]; row.pt = a.gpt[g]; row.n_obs = e - b; row.status = status;
  a.groups[g] = row;
}

// one cyclic Jacobi rotation of the symmetric 4x4 matrix A in the (P, Q) plane, accumulated into the eigenvector matrix V
template <int P, int Q>
LIFCAL_DEV void start_rotate(double (&A)[4][4], double (&V)[4][4]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
  A[P][P] -= t * apq; A[Q][Q] += t * apq; A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    if (r != P && r != Q) {
      const double arp = A[r][P], arq = A[r][Q];
      A[r][P] = cs * arp - sn * arq; A[P][r] = A[r][P];
      A[r][Q] = sn * arp + cs * arq; A[Q][r] = A[r][Q];
    }
    const double vrp = V[r][P], vrq = V[r][Q];
    V[r][P] = cs * vrp - sn * vrq; V[r][Q] = sn * vrp + cs * vrq;
  }
}

// Pose of one frame from the moment M[a][b] = sum w (P - Pm)_a (p_c - cm)_b (row-major) and the two centroids: Horn's 4x4 matrix,
// its largest eigenvector by cyclic Jacobi in the fixed order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) until the off-diagonal norm is
// <= eps * the Frobenius norm or 30 sweeps, R from the unit quaternion, t = cm - R Pm, the XYZ angles of frame_eval's R.
// Returns the frame status (OK or DEGENERATE); eig: the two largest eigenvalues.
LIFCAL_DEV int start_pose(const double* M, const double* Pm, const double* cm, double* view, double* eig) {
  const double Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
  double A[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
  double V[4][4] = {{1.0, 0.0, 0.0, 0.0}, {0.0, 1.0, 0.0, 0.0}, {0.0, 0.0, 1.0, 0.0}, {0.0, 0.0, 0.0, 1.0}};
  for (int sweep = 0; sweep < 30; ++sweep) {
    double off = 0.0, dg = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      dg += A[i][i] * A[i][i];
#pragma unroll
      for (int j = i + 1; j < 4; ++j) off += 2.0 * A[i][j] * A[i][j];
    }
    if (sqrt(off) <= 2.220446049250313e-16 * sqrt(dg + off)) break;
    start_rotate<0, 1>(A, V); start_rotate<0, 2>(A, V); start_rotate<0, 3>(A, V);
    start_rotate<1, 2>(A, V); start_rotate<1, 3>(A, V); start_rotate<2, 3>(A, V);
  }
  double l1 = A[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
  int at = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > l1) { l1 = A[k][k]; q0 = V[0][k]; q1 = V[1][k]; q2 = V[2][k]; q3 = V[3][k]; at = k; }
  double l2 = -1.7976931348623157e308;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (k != at) l2 = fmax(l2, A[k][k]);
  eig[0] = l1; eig[1] = l2;
  if (!(l1 - l2 > 1e-9 * fabs(l1))) return LIFCAL_START_FRAME_DEGENERATE;   // (also: a sum that is not finite)
  const double qn = 1.0 / sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  q0 *= qn; q1 *= qn; q2 *= qn; q3 *= qn;
  const double R00 = q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, R01 = 2.0 * (q1 * q2 - q0 * q3), R02 = 2.0 * (q1 * q3 + q0 * q2);
  const double R10 = 2.0 * (q2 * q1 + q0 * q3), R11 = q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, R12 = 2.0 * (q2 * q3 - q0 * q1);
  const double R20 = 2.0 * (q3 * q1 - q0 * q2), R21 = 2.0 * (q3 * q2 + q0 * q1), R22 = q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3;
  view[1] = asin(fmin(fmax(R02, -1.0), 1.0));
  if (1.0 - fabs(R02) < 1e-12) { view[0] = atan2(R21, R11); view[2] = 0.0; }
  else { view[0] = atan2(-R12, R22); view[2] = atan2(-R01, R00); }
  view[3] = cm[0] - (R00 * Pm[0] + R01 * Pm[1] + R02 * Pm[2]);
  view[4] = cm[1] - (R10 * Pm[0] + R11 * Pm[1] + R12 * Pm[2]);
  view[5] = cm[2] - (R20 * Pm[0] + R21 * Pm[1] + R22 * Pm[2]);
  return LIFCAL_START_FRAME_OK;
}

// The two sums of the alignment over the groups [gb, ge), this thread's share in ascending position.  MASKED (k_reg_frontier,
// register.hpp): only the groups whose point has pmask[pt] != 0 take part.
//   centroids  acc[0] sum w, [1..3] sum w P, [4..6] sum w p_c, [7] the number of groups that take part; w = 1 / Z_c^2
//   moment     acc[3 i + j] = sum w (P - Pm)_i (p_c - cm)_j
template <bool MASKED>
LIFCAL_DEV void st_centroid_sums(const lifcal_start_group* groups, uint32_t gb, uint32_t ge, const double* pts, const uint32_t* pmask, double (&acc)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  for (uint32_t g = gb + threadIdx.x; g < ge; g += ST_THREADS) {
    const lifcal_start_group* r = groups + g;
    if (r->status == LIFCAL_START_GROUP_USED && (!MASKED || pmask[r->pt])) {
      const double* P = pts + 3 * (size_t)r->pt;
      const double w = 1.0 / (r->xyz[2] * r->xyz[2]);
      acc[0] += w; acc[7] += 1.0;
#pragma unroll
      for (int k = 0; k < 3; ++k) { acc[1 + k] += w * P[k]; acc[4 + k] += w * r->xyz[k]; }
    }
  }
}

template <bool MASKED>
LIFCAL_DEV void st_moment_sums(const lifcal_start_group* groups, uint32_t gb, uint32_t ge, const double* pts, const uint32_t* pmask,
                               const double (&Pm)[3], const double (&cm)[3], double (&acc)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = 0.0;
  for (uint32_t g = gb + threadIdx.x; g < ge; g += ST_THREADS) {
    const lifcal_start_group* r = groups + g;
    if (r->status == LIFCAL_START_GROUP_USED && (!MASKED || pmask[r->pt])) {
      const double* P = pts + 3 * (size_t)r->pt;
      const double w = 1.0 / (r->xyz[2] * r->xyz[2]);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const double wl = w * (P[i] - Pm[i]);
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[3 * i + j] += wl * (r->xyz[j] - cm[j]);
      }
    }
  }
}

struct StartAlignArgs {
  const uint32_t *off, *fgoff;        // [F + 1] CSR of the observations | of the groups by frame
  const uint32_t* pt;                 // [N] sorted like u .. mcy
  const double *u, *v, *mcx, *mcy;
  const double* cu_stats;             // [2N] c_u for the parameters as stored
  const CamConsts* camc;              // [2] folded | as stored
  const double* pts;                  // [3P]
  const lifcal_start_group* groups;   // [G], written by k_start_groups
  double* views;                      // [6F] out, status 0 only
  lifcal_start_frame* rows;           // [F], zeroed by the host
  double thr2;
};

template <int NR, bool TAN, bool ADJ>
__global__ __launch_bounds__(ST_THREADS) void k_start_align(StartAlignArgs a) {
  __shared__ double s_red[ST_WAVES * 9], s_out[9], s_ft[FRAME_STRIDE], s_eig[2];
  __shared__ int s_status;
  const uint32_t f = blockIdx.x, tid = threadIdx.x;
  const uint32_t b = a.off[f], e = a.off[f + 1], gb = a.fgoff[f], ge = a.fgoff[f + 1];
  lifcal_start_frame* row = a.rows + f;
  if (b == e) { if (tid == 0) row->status = LIFCAL_START_FRAME_EMPTY; return; }
  double acc[9];

  // pass 1: weights, weighted centroids of the world points and of the camera-frame points, the count of used groups
  st_centroid_sums<false>(a.groups, gb, ge, a.pts, nullptr, acc);
  rs_fold<8>(acc, s_red, s_out);
  const double sw = s_out[0];
  const uint32_t n_used = (uint32_t)s_out[7];
  if (n_used < 3u) {   // (the same in every thread)
    if (tid == 0) { row->sum_w = sw; row->n_obs = e - b; row->n_groups = ge - gb; row->n_used = n_used; row->status = LIFCAL_START_FRAME_FEW; }
    return;
  }
  double Pm[3], cm[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) { Pm[k] = s_out[1 + k] / sw; cm[k] = s_out[4 + k] / sw; }

  // pass 2: the centred moment M = sum w (P - Pm)(p_c - cm)^T
  st_moment_sums<false>(a.groups, gb, ge, a.pts, nullptr, Pm, cm, acc);
  rs_fold<9>(acc, s_red, s_out);
  if (tid == 0) {
    double view[6];
    const int st = start_pose(s_out, Pm, cm, view, s_eig);
    if (st == LIFCAL_START_FRAME_OK) {
      frame_eval(view, s_ft);
#pragma unroll
      for (int k = 0; k < 6; ++k) a.views[6 * (size_t)f + k] = view[k];
    }
    s_status = st;
  }
  __syncthreads();
  if (s_status != LIFCAL_START_FRAME_OK) {
    if (tid == 0) {
      row->sum_w = sw; row->eig[0] = s_eig[0]; row->eig[1] = s_eig[1];
      row->n_obs = e - b; row->n_groups = ge - gb; row->n_used = n_used; row->status = s_status;
    }
    return;
  }

  // pass 3: the alignment residual over the used groups, the reprojection errors over all observations of the frame at the new
  // pose (the table of frame_eval at the returned angles: what a resection that starts here evaluates), parameters as stored
#pragma unroll
  for (int k = 0; k < 4; ++k) acc[k] = 0.0;
  for (uint32_t g = gb + tid; g < ge; g += ST_THREADS) {
    const lifcal_start_group* r = a.groups + g;
    if (r->status == LIFCAL_START_GROUP_USED) {
      const double* P = a.pts + 3 * (size_t)r->pt;
      const double w = 1.0 / (r->xyz[2] * r->xyz[2]);
      const double d0 = s_ft[0] * P[0] + s_ft[1] * P[1] + s_ft[2] * P[2] + s_ft[9] - r->xyz[0];
      const double d1 = s_ft[3] * P[0] + s_ft[4] * P[1] + s_ft[5] * P[2] + s_ft[10] - r->xyz[1];
      const double d2 = s_ft[6] * P[0] + s_ft[7] * P[1] + s_ft[8] * P[2] + s_ft[11] - r->xyz[2];
      acc[0] += w * (d0 * d0 + d1 * d1 + d2 * d2);
    }
  }
  const CamConsts& cs = a.camc[1];
  for (uint32_t i = b + tid; i < e; i += ST_THREADS) {
    const double* P = a.pts + 3 * (size_t)a.pt[i];
    const double2 w = *reinterpret_cast<const double2*>(a.cu_stats + 2 * (size_t)i);
    GroupConsts gc;
    group_prepare(cs, s_ft[0] * P[0] + s_ft[1] * P[1] + s_ft[2] * P[2] + s_ft[9], s_ft[3] * P[0] + s_ft[4] * P[1] + s_ft[5] * P[2] + s_ft[10],
                  s_ft[6] * P[0] + s_ft[7] * P[1] + s_ft[8] * P[2] + s_ft[11], gc);
    double rx, ry;
    obs_value<NR, TAN, ADJ>(cs, gc, a.mcx[i], a.mcy[i], w.x, w.y, a.u[i], a.v[i], rx, ry);
    acc[1] += rx * rx; acc[2] += ry * ry;
    if (rx * rx + ry * ry <= a.thr2) acc[3] += 1.0;
  }
  rs_fold<4>(acc, s_red, s_out);
  if (tid == 0) {
    row->sum_w = sw; row->align_rms = sqrt(s_out[0] / sw); row->eig[0] = s_eig[0]; row->eig[1] = s_eig[1];
    row->sum_xx = s_out[1]; row->sum_yy = s_out[2];
    row->n_obs = e - b; row->n_inliers = (uint32_t)s_out[3]; row->n_groups = ge - gb; row->n_used = n_used; row->status = LIFCAL_START_FRAME_OK;
  }
}

struct StartPointArgs {
  const uint32_t* off;                // [P + 1] CSR of the observations by point
  const uint32_t* fr;                 // [N] point-sorted, like u .. mcy
  const double *u, *v, *mcx, *mcy;
  const double *cu, *cu_stats;        // [2N] c_u for the folded parameters | for the parameters as stored
  const CamConsts* camc;              // [2] likewise
  const double* ft;                   // [F][FRAME_STRIDE], k_intersect_frames
  double* pts;                        // [3P] out, status 0 only
  lifcal_start_point* rows;           // [P], zeroed by the host
  double thr2;
  uint32_t n_points;
};

template <int NR, bool TAN, bool ADJ>
__global__ __launch_bounds__(ST_THREADS) void k_start_points(StartPointArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * ST_WAVES + (threadIdx.x >> 6)));   // wave w of block b owns point 4 b + w
  if (p >= a.n_points) return;
  const uint32_t b = a.off[p], e = a.off[p + 1];
  lifcal_start_point* row = a.rows + p;
  if (e - b < 2u) {
    if (lane == 0) { row->n_obs = e - b; row->status = e == b ? LIFCAL_START_POINT_EMPTY : LIFCAL_START_POINT_SINGLE; }
    return;
  }
  const CamConsts& c = a.camc[0];
  // the rows of every observation in the world frame: p_c = R P + t, so A_w = A R and b_w = b - A t
  double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};
  for (uint32_t i = b + lane; i < e; i += 64u) {
    const double2 w = *reinterpret_cast<const double2*>(a.cu + 2 * (size_t)i);
    double ax, azx, bx, ay, azy, by;
    start_ray<NR, TAN, ADJ>(c, a.u[i], a.v[i], a.mcx[i], a.mcy[i], w.x, w.y, ax, azx, bx, ay, azy, by);
    const double* __restrict__ ft = a.ft + (size_t)a.fr[i] * FRAME_STRIDE;
    double J[2][3], r[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) { J[0][k] = ax * ft[k] + azx * ft[6 + k]; J[1][k] = ay * ft[3 + k] + azy * ft[6 + k]; }
    r[0] = bx - (ax * ft[9] + azx * ft[11]); r[1] = by - (ay * ft[10] + azy * ft[11]);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      int t = 0;
#pragma unroll
      for (int m = 0; m < 3; ++m) {
        g[m] += J[q][m] * r[q];
#pragma unroll
        for (int n = 0; n <= m; ++n) H[t++] += J[q][m] * J[q][n];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) H[k] = wave_sum(H[k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = wave_sum(g[k]);
  // (every lane holds the same bits from here on)
  double x[3], mp;
  if (!start_solve3(H, g, x, mp)) {
    if (lane == 0) { row->min_pivot = lm_finite(mp) ? mp : 0.0; row->n_obs = e - b; row->status = LIFCAL_START_POINT_SINGULAR; }
    return;
  }
  // the reprojection errors at the new point, parameters as stored; a frame that has the point behind its main lens
  const CamConsts& cs = a.camc[1];
  double sxx = 0.0, syy = 0.0, inl = 0.0, behind = 0.0;
  for (uint32_t i = b + lane; i < e; i += 64u) {
    const double2 w = *reinterpret_cast<const double2*>(a.cu_stats + 2 * (size_t)i);
    const double* __restrict__ ft = a.ft + (size_t)a.fr[i] * FRAME_STRIDE;
    const double X = ft[0] * x[0] + ft[1] * x[1] + ft[2] * x[2] + ft[9], Y = ft[3] * x[0] + ft[4] * x[1] + ft[5] * x[2] + ft[10],
                 Z = ft[6] * x[0] + ft[7] * x[1] + ft[8] * x[2] + ft[11];
    if (!(Z + c.zC0 > 0.0)) behind += 1.0;
    GroupConsts gc;
    group_prepare(cs, X, Y, Z, gc);
    double rx, ry;
    obs_value<NR, TAN, ADJ>(cs, gc, a.mcx[i], a.mcy[i], w.x, w.y, a.u[i], a.v[i], rx, ry);
    sxx += rx * rx; syy += ry * ry;
    if (rx * rx + ry * ry <= a.thr2) inl += 1.0;
  }
  sxx = wave_sum(sxx); syy = wave_sum(syy); inl = wave_sum(inl); behind = wave_sum(behind);
  if (lane == 0) {
    row->min_pivot = mp; row->n_obs = e - b;
    if (behind > 0.0) {
      row->status = LIFCAL_START_POINT_BEHIND;
    } else {
      double* out = a.pts + 3 * (size_t)p;
      out[0] = x[0]; out[1] = x[1]; out[2] = x[2];
      row->sum_xx = sxx; row->sum_yy = syy; row->n_inliers = (uint32_t)inl; row->status = LIFCAL_START_POINT_OK;
    }
  }
}

}  // namespace lifcal

namespace {

int start_poses_impl(const lifcal_resect_problem* p, const lifcal_ba_options* o, double gate_px, double inlier_threshold,
                     lifcal_start_frame* per_frame, lifcal_start_group* groups, uint32_t* n_groups, double* seconds) {
  if (int rc = batch_checks("lifcal_start_poses", p, o, per_frame, true)) return rc;
  if (!(gate_px > 0.0)) { g_last_error = "lifcal_start_poses: gate_px must be > 0 (+infinity: no gate)"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (seconds) *seconds = 0.0;
  if (n_groups) *n_groups = 0;
  const uint32_t N = p->n_obs, F = p->n_frames, P = p->n_points;
  if (!F) return 0;
  if (!N) {   // no frame has an observation
    std::memset(per_frame, 0, (size_t)F * sizeof(lifcal_start_frame));
    for (uint32_t f = 0; f < F; ++f) per_frame[f].status = LIFCAL_START_FRAME_EMPTY;
    return 0;
  }
  std::vector<uint32_t> off((size_t)F + 1), idx(N);
  {
    std::vector<uint32_t> offp((size_t)P + 1), pidx(N);
    if (int rc = lifcal_group_index(N, P, p->pt, offp.data(), pidx.data())) return rc;
    if (int rc = frame_point_order(N, F, p->fr, pidx, off.data(), idx)) return rc;
  }
  const Groups g = build_groups(N, F, p->fr, p->pt, idx);
  const uint32_t G = g.G;

  ByteLayout L;
  const size_t at_u = L.take((size_t)N * 8), at_v = L.take((size_t)N * 8), at_mx = L.take((size_t)N * 8), at_my = L.take((size_t)N * 8), at_pt = L.take((size_t)N * 4),
               at_off = L.take(((size_t)F + 1) * 4), at_fgoff = L.take(((size_t)F + 1) * 4), at_goff = L.take(((size_t)G + 1) * 4), at_gfr = L.take((size_t)G * 4),
               at_gpt = L.take((size_t)G * 4), at_cam = L.take(LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8), at_pts = L.take((size_t)P * 24);
  const size_t in_bytes = L.bytes;
  const size_t at_cu = L.take((size_t)N * 16), at_cus = L.take((size_t)N * 16), at_camc = L.take(2 * sizeof(CamConsts)), at_grp = L.take((size_t)G * sizeof(lifcal_start_group)),
               at_views = L.take((size_t)F * 48), at_rows = L.take((size_t)F * sizeof(lifcal_start_frame));
  std::vector<unsigned char> host(in_bytes);
  stage_observations(host, idx, N, p, at_u, at_v, at_mx, at_my, at_pt, p->pt);
  std::memcpy(host.data() + at_off, off.data(), off.size() * 4);
  std::memcpy(host.data() + at_fgoff, g.fgoff.data(), g.fgoff.size() * 4);
  std::memcpy(host.data() + at_goff, g.goff.data(), g.goff.size() * 4);
  std::memcpy(host.data() + at_gfr, g.gfr.data(), (size_t)G * 4);
  std::memcpy(host.data() + at_gpt, g.gpt.data(), (size_t)G * 4);
  std::memcpy(host.data() + at_cam, p->cam, LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8);
  std::memcpy(host.data() + at_pts, p->pts, (size_t)P * 24);
  std::vector<double> views_out((size_t)F * 6);   // (p->views is output only: nothing of it goes to the device)

  if (int rc = mla::select_device(o->device, "lifcal_start_poses")) return rc;
  BatchCall D(o->device, "lifcal_start_poses");
  D.open(L.bytes);
  D.upload(host.data(), in_bytes);
  D.zero(at_views, (size_t)F * 48);
  D.zero(at_rows, (size_t)F * sizeof(lifcal_start_frame));
  D.begin();
  if (D.ok()) {
    unsigned char* const dev = D.dev;
    hipStream_t const stream = D.stream;
    const double* d_cam = (const double*)(dev + at_cam);
    StartGroupArgs ga;
    ga.goff = (const uint32_t*)(dev + at_goff); ga.gfr = (const uint32_t*)(dev + at_gfr); ga.gpt = (const uint32_t*)(dev + at_gpt);
    ga.u = (const double*)(dev + at_u); ga.v = (const double*)(dev + at_v); ga.mcx = (const double*)(dev + at_mx); ga.mcy = (const double*)(dev + at_my);
    ga.cu = (const double*)(dev + at_cu); ga.camc = (const CamConsts*)(dev + at_camc); ga.groups = (lifcal_start_group*)(dev + at_grp);
    ga.gate_px = gate_px; ga.n_groups = G;
    StartAlignArgs aa;
    aa.off = (const uint32_t*)(dev + at_off); aa.fgoff = (const uint32_t*)(dev + at_fgoff); aa.pt = (const uint32_t*)(dev + at_pt);
    aa.u = ga.u; aa.v = ga.v; aa.mcx = ga.mcx; aa.mcy = ga.mcy; aa.cu_stats = (const double*)(dev + at_cus); aa.camc = ga.camc;
    aa.pts = (const double*)(dev + at_pts); aa.groups = ga.groups; aa.views = (double*)(dev + at_views); aa.rows = (lifcal_start_frame*)(dev + at_rows);
    aa.thr2 = inlier_threshold * inlier_threshold;
    const uint32_t lens_grid = (N + 255u) / 256u, group_grid = (G + (uint32_t)ST_THREADS - 1u) / (uint32_t)ST_THREADS;
    const ModelCfg cfg = model_cfg(p->config);
    // (a dispatch table that refuses the configuration returns from here: D waits for the stream)
    for (int fold = 1; fold >= 0; --fold)
      if (int rc = launch_lens_pass(cfg, stream, lens_grid, d_cam, p->spx, p->spy, p->scale, o->loss_scale, fold, N, ga.mcx, ga.mcy, (CamConsts*)(dev + at_camc), (double*)(dev + (fold ? at_cu : at_cus)))) return rc;
#define CALL_START_POSES(NR, TAN, ADJ) do { \
    hipLaunchKernelGGL((k_start_groups<NR, TAN, ADJ>), dim3(group_grid), dim3(ST_THREADS), 0, stream, ga); \
    hipLaunchKernelGGL((k_start_align<NR, TAN, ADJ>), dim3(F), dim3(ST_THREADS), 0, stream, aa); } while (0)
    DISPATCH_CFG(&cfg, CALL_START_POSES);
#undef CALL_START_POSES
  }
  D.end();
  D.download(views_out.data(), at_views, (size_t)F * 48);
  D.download(per_frame, at_rows, (size_t)F * sizeof(lifcal_start_frame));
  if (groups) D.download(groups, at_grp, (size_t)G * sizeof(lifcal_start_group));
  if (int rc = D.finish(seconds)) return rc;
  for (uint32_t f = 0; f < F; ++f)
    if (per_frame[f].status == LIFCAL_START_FRAME_OK) std::memcpy(p->views + 6 * (size_t)f, views_out.data() + 6 * (size_t)f, 48);
  if (n_groups) *n_groups = G;
  return 0;
}

int start_points_impl(const lifcal_intersect_problem* p, const lifcal_ba_options* o, double inlier_threshold, lifcal_start_point* per_point, double* seconds) {
  if (int rc = batch_checks("lifcal_start_points", p, o, per_point, true)) return rc;
  if (seconds) *seconds = 0.0;
  const uint32_t N = p->n_obs, F = p->n_frames, P = p->n_points;
  if (!P) return 0;
  if (!N) {   // no point has an observation
    std::memset(per_point, 0, (size_t)P * sizeof(lifcal_start_point));
    for (uint32_t k = 0; k < P; ++k) per_point[k].status = LIFCAL_START_POINT_EMPTY;
    return 0;
  }
  // the observations point-major, inside a point in the caller's order (stable counting sort)
  std::vector<uint32_t> off((size_t)P + 1), idx(N);
  if (int rc = lifcal_group_index(N, P, p->pt, off.data(), idx.data())) return rc;
  ByteLayout L;
  const size_t at_u = L.take((size_t)N * 8), at_v = L.take((size_t)N * 8), at_mx = L.take((size_t)N * 8), at_my = L.take((size_t)N * 8), at_fr = L.take((size_t)N * 4),
               at_off = L.take(((size_t)P + 1) * 4), at_cam = L.take(LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8), at_views = L.take((size_t)F * 48);
  const size_t in_bytes = L.bytes;
  const size_t at_cu = L.take((size_t)N * 16), at_cus = L.take((size_t)N * 16), at_camc = L.take(2 * sizeof(CamConsts)), at_ft = L.take((size_t)F * FRAME_STRIDE * 8),
               at_pts = L.take((size_t)P * 24), at_rows = L.take((size_t)P * sizeof(lifcal_start_point));
  std::vector<unsigned char> host(in_bytes);
  stage_observations(host, idx, N, p, at_u, at_v, at_mx, at_my, at_fr, p->fr);
  std::memcpy(host.data() + at_off, off.data(), off.size() * 4);
  std::memcpy(host.data() + at_cam, p->cam, LIFCAL_BA_MAX_CAMERA_PARAMETERS * 8);
  std::memcpy(host.data() + at_views, p->views, (size_t)F * 48);
  std::vector<double> pts_out((size_t)P * 3);   // (p->pts is output only: nothing of it goes to the device)

  if (int rc = mla::select_device(o->device, "lifcal_start_points")) return rc;
  BatchCall D(o->device, "lifcal_start_points");
  D.open(L.bytes);
  D.upload(host.data(), in_bytes);
  D.zero(at_pts, (size_t)P * 24);
  D.zero(at_rows, (size_t)P * sizeof(lifcal_start_point));
  D.begin();
  if (D.ok()) {
    unsigned char* const dev = D.dev;
    hipStream_t const stream = D.stream;
    const double* d_cam = (const double*)(dev + at_cam);
    StartPointArgs a;
    a.off = (const uint32_t*)(dev + at_off); a.fr = (const uint32_t*)(dev + at_fr);
    a.u = (const double*)(dev + at_u); a.v = (const double*)(dev + at_v); a.mcx = (const double*)(dev + at_mx); a.mcy = (const double*)(dev + at_my);
    a.cu = (const double*)(dev + at_cu); a.cu_stats = (const double*)(dev + at_cus); a.camc = (const CamConsts*)(dev + at_camc);
    a.ft = (const double*)(dev + at_ft); a.pts = (double*)(dev + at_pts); a.rows = (lifcal_start_point*)(dev + at_rows);
    a.thr2 = inlier_threshold * inlier_threshold; a.n_points = P;
    const uint32_t lens_grid = (N + 255u) / 256u, frame_grid = (F + 255u) / 256u, point_grid = (P + (uint32_t)ST_WAVES - 1u) / (uint32_t)ST_WAVES;
    const ModelCfg cfg = model_cfg(p->config);
    // (a dispatch table that refuses the configuration returns from here: D waits for the stream)
    hipLaunchKernelGGL(k_intersect_frames, dim3(frame_grid), dim3(256), 0, stream, (const double*)(dev + at_views), F, (double*)(dev + at_ft));
    for (int fold = 1; fold >= 0; --fold)
      if (int rc = launch_lens_pass(cfg, stream, lens_grid, d_cam, p->spx, p->spy, p->scale, o->loss_scale, fold, N, a.mcx, a.mcy, (CamConsts*)(dev + at_camc), (double*)(dev + (fold ? at_cu : at_cus)))) return rc;
#define CALL_START_POINTS(NR, TAN, ADJ) hipLaunchKernelGGL((k_start_points<NR, TAN, ADJ>), dim3(point_grid), dim3(ST_THREADS), 0, stream, a)
    DISPATCH_CFG(&cfg, CALL_START_POINTS);
#undef CALL_START_POINTS
  }
  D.end();
  D.download(pts_out.data(), at_pts, (size_t)P * 24);
  D.download(per_point, at_rows, (size_t)P * sizeof(lifcal_start_point));
  if (int rc = D.finish(seconds)) return rc;
  for (uint32_t k = 0; k < P; ++k)
    if (per_point[k].status == LIFCAL_START_POINT_OK) std::memcpy(p->pts + 3 * (size_t)k, pts_out.data() + 3 * (size_t)k, 24);
  return 0;
}

}  // namespace

extern "C" int lifcal_start_poses(const lifcal_resect_problem* p, const lifcal_ba_options* o, double gate_px, double inlier_threshold,
                                  lifcal_start_frame* per_frame, lifcal_start_group* groups, uint32_t* n_groups, double* seconds) {
  return guard_abi("lifcal_start_poses", [&] { return start_poses_impl(p, o, gate_px, inlier_threshold, per_frame, groups, n_groups, seconds); });
}

extern "C" int lifcal_start_points(const lifcal_intersect_problem* p, const lifcal_ba_options* o, double inlier_threshold, lifcal_start_point* per_point, double* seconds) {
  return guard_abi("lifcal_start_points", [&] { return start_points_impl(p, o, inlier_threshold, per_point, seconds); });
}
