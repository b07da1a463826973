// align.hpp — scene alignment (include/lifcal_align.h): the closed-form similarity between two point sets and
// its application to poses and points.  Host C++ only, included from lifcal_ba.hip behind colmap.hpp (euler_xyz, quat_to_matrix)
// and covariance.hpp (sym_eig_jacobi).
#pragma once

extern "C" {

int lifcal_align_fit(uint32_t n, const double* from, const double* to, const double* w, int32_t with_scale, lifcal_alignment* out) {
  if (!from || !to || !out) { g_last_error = "lifcal_align_fit: null argument"; return LIFCAL_BA_ERR_INVALID_ARG; }
  typedef long double real;
  uint32_t used = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (w && !std::isfinite(w[i])) { g_last_error = "lifcal_align_fit: a non-finite weight"; return LIFCAL_BA_ERR_INVALID_ARG; }
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(from[3 * (size_t)i + k]) || !std::isfinite(to[3 * (size_t)i + k])) { g_last_error = "lifcal_align_fit: a non-finite coordinate"; return LIFCAL_BA_ERR_INVALID_ARG; }
    if (!w || w[i] > 0.0) ++used;
  }
  if (used < 3) { g_last_error = "lifcal_align_fit: fewer than three points with a positive weight"; return LIFCAL_BA_ERR_INVALID_ARG; }
  auto wt = [&](uint32_t i) -> real { return w ? (w[i] > 0.0 ? (real)w[i] : (real)0) : (real)1; };
  // weighted centroids, then the centred sums (index order, extended precision)
  real W = 0, cf[3] = {0, 0, 0}, ct[3] = {0, 0, 0};
  for (uint32_t i = 0; i < n; ++i) {
    const real wi = wt(i);
    W += wi;
    for (int k = 0; k < 3; ++k) { cf[k] += wi * from[3 * (size_t)i + k]; ct[k] += wi * to[3 * (size_t)i + k]; }
  }
  for (int k = 0; k < 3; ++k) { cf[k] /= W; ct[k] /= W; }
  real M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, C[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, D[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};   // sum w f t^T, sum w f f^T, sum w t t^T
  for (uint32_t i = 0; i < n; ++i) {
    const real wi = wt(i);
    if (wi == 0) continue;
    real f[3], t[3];
    for (int k = 0; k < 3; ++k) { f[k] = from[3 * (size_t)i + k] - cf[k]; t[k] = to[3 * (size_t)i + k] - ct[k]; }
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) { M[a][b] += wi * f[a] * t[b]; C[a][b] += wi * f[a] * f[b]; D[a][b] += wi * t[a] * t[b]; }
  }
  std::vector<double> A, ev, V;
  // either side collinear leaves the rotation about that line undetermined (Horn's matrix then has a repeated largest eigenvalue)
  for (int side = 0; side < 2; ++side) {
    A.resize(9);
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) A[3 * a + b] = (double)(side ? D[a][b] : C[a][b]);
    sym_eig_jacobi(3, A, ev, V);
    std::sort(ev.begin(), ev.end());
    if (!(ev[2] > 0.0) || ev[1] < 1e-12 * ev[2]) { g_last_error = std::string("lifcal_align_fit: the points of `") + (side ? "to" : "from") + "` are collinear (or coincide)"; return LIFCAL_BA_ERR_INVALID_ARG; }
  }
  // Horn's 4 x 4 matrix: its eigenvector of the largest eigenvalue is the unit quaternion (w, x, y, z) of R
  const double Sxx = (double)M[0][0], Sxy = (double)M[0][1], Sxz = (double)M[0][2], Syx = (double)M[1][0], Syy = (double)M[1][1], Syz = (double)M[1][2],
               Szx = (double)M[2][0], Szy = (double)M[2][1], Szz = (double)M[2][2];
  A = {Sxx + Syy + Szz, Syz - Szy,       Szx - Sxz,        Sxy - Syx,
       Syz - Szy,       Sxx - Syy - Szz, Sxy + Syx,        Szx + Sxz,
       Szx - Sxz,       Sxy + Syx,       -Sxx + Syy - Szz, Syz + Szy,
       Sxy - Syx,       Szx + Sxz,       Syz + Szy,        -Sxx - Syy + Szz};
  sym_eig_jacobi(4, A, ev, V);
  uint32_t best = 0;
  for (uint32_t e = 1; e < 4; ++e) if (ev[e] > ev[best]) best = e;
  double q[4] = {V[0 * 4 + best], V[1 * 4 + best], V[2 * 4 + best], V[3 * 4 + best]};
  {
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (double& x : q) x /= nq;
  }
  double R[3][3];
  lifcal_colmap::quat_to_matrix(q, R);
  real s = 1;
  if (with_scale) {
    // min over s of sum w |t - s R f|^2: s = sum w t . (R f) / sum w |f|^2
    real num = 0;
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) num += (real)R[a][b] * M[b][a];
    s = num / (C[0][0] + C[1][1] + C[2][2]);
  }
  out->scale = (double)s;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) out->R[3 * a + b] = R[a][b];
    out->t[a] = (double)(ct[a] - s * ((real)R[a][0] * cf[0] + (real)R[a][1] * cf[1] + (real)R[a][2] * cf[2]));
  }
  real ss = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const real wi = wt(i);
    if (wi == 0) continue;
    for (int a = 0; a < 3; ++a) {
      const real r = (real)to[3 * (size_t)i + a] - (real)out->scale * ((real)R[a][0] * from[3 * (size_t)i] + (real)R[a][1] * from[3 * (size_t)i + 1] + (real)R[a][2] * from[3 * (size_t)i + 2]) - (real)out->t[a];
      ss += wi * r * r;
    }
  }
  out->rms = (double)std::sqrt(ss / W);
  out->n_used = used; out->reserved = 0;
  return 0;
}

int lifcal_align_apply(const lifcal_alignment* a, uint32_t n_frames, double* views, uint64_t n_points, double* pts) {
  if (!a || (n_frames && !views) || (n_points && !pts)) { g_last_error = "lifcal_align_apply: null argument"; return LIFCAL_BA_ERR_INVALID_ARG; }
  const double s = a->scale;
  const double* R = a->R;
  for (uint64_t i = 0; i < n_points; ++i) {
    double* P = pts + 3 * i;
    const double x = P[0], y = P[1], z = P[2];
    for (int r = 0; r < 3; ++r) P[r] = s * (R[3 * r] * x + R[3 * r + 1] * y + R[3 * r + 2] * z) + a->t[r];
  }
  for (uint32_t f = 0; f < n_frames; ++f) {
    double* v = views + 6 * (size_t)f;
    // R_f = Rx(a0) Ry(a1) Rz(a2), the rotation of the projection model (device_model.hpp: frame_eval)
    const double s0 = std::sin(v[0]), c0 = std::cos(v[0]), s1 = std::sin(v[1]), c1 = std::cos(v[1]), s2 = std::sin(v[2]), c2 = std::cos(v[2]);
    const double Rf[3][3] = {{c1 * c2, -c1 * s2, s1}, {c0 * s2 + s0 * s1 * c2, c0 * c2 - s0 * s1 * s2, -s0 * c1}, {s0 * s2 - c0 * s1 * c2, s0 * c2 + c0 * s1 * s2, c0 * c1}};
    double Rn[3][3];   // R_f R^T
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Rn[r][c] = Rf[r][0] * R[3 * c] + Rf[r][1] * R[3 * c + 1] + Rf[r][2] * R[3 * c + 2];
    lifcal_colmap::euler_xyz(Rn, v);
    for (int r = 0; r < 3; ++r) v[3 + r] = s * v[3 + r] - (Rn[r][0] * a->t[0] + Rn[r][1] * a->t[1] + Rn[r][2] * a->t[2]);
  }
  return 0;
}

}  // extern "C"
