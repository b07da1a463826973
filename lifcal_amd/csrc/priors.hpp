// priors.hpp — Gaussian priors on the camera block and on poses (include/lifcal_prior.h) and on 3D points
// (section 7r; k_point_priors itself lives in point_priors.hip): the kernels, their launchers and the C ABI.  Included from
// lifcal_ba.hip behind the handle and in front of the launch helpers (launch_blocks and launch_value_cost call launch_priors).
//
// The term 1/2 d^T Lambda d, d = x - mean, touches reduced parameters only: it is added to the reduced block where k_constraints
// adds the distance constraints, behind the sweep kernels on the stream, and to the value-only cost of a candidate.  The handle keeps
// the priors in HBM in the internal order of the reduced system (poses | promoted points | camera): the camera matrix compacted to
// the nc structural columns, rows and columns of slots that are not free set to zero on the host (apply_prior_mask).
#pragma once

namespace lifcal {

constexpr uint32_t PRIOR_THREADS = 256, PRIOR_PER_WG = PRIOR_THREADS / 64;

// row r of the priors, the camera's nc_rows rows first and then six per prior-ed frame in ascending order: (Lambda d)_i, the sum
// in ascending column order, and d_i through *di
LIFCAL_DEV double prior_row(const Dev& d, const double* cam, const double* views, uint32_t r, uint32_t nc_rows, double* di) {
  const double *A, *x, *mean; uint32_t n, i;
  if (r < nc_rows) { A = d.pr_cam_info; x = cam; mean = d.pr_cam_mean; n = d.nc; i = r; }
  else { const uint32_t k = (r - nc_rows) / 6; A = d.pr_pose_info + 36 * (size_t)k; x = views + 6 * (size_t)d.pr_frame[k]; mean = d.pr_pose_mean + 6 * (size_t)k; n = 6; i = (r - nc_rows) % 6; }
  double s = 0.0;
  for (uint32_t j = 0; j < n; ++j) s += A[i * n + j] * (x[j] - mean[j]);
  *di = x[i] - mean[i];
  return s;
}

// Workgroup 0: the cost of every prior and the camera prior's blocks; workgroup 1 + g: the blocks of the pose priors 4 g .. 4 g + 3,
// one wave each (cost_only launches workgroup 0 alone).  Single writer, fixed order: the kernel is stream-ordered behind every
// kernel that adds to the bound copy of the reduced block and in front of k_finalize / k_fold_hot, and every word gets ONE plain
// add from one thread here — the canonical words, never the hot rows (fold_hot_rows ADDS onto the canonical word).  So the result
// has the same bits on every run and there is no second launch shape for options.deterministic.
//   cost    1/2 sum_i d_i (Lambda d)_i over the rows, camera first and then the prior-ed frames in ascending order: a thread sums
//           its rows (t, t + 256, ...) in ascending order, the wave reduction and the sum over the four waves have a fixed shape;
//           thread 0 adds the result once to *cost_out
//   S       one lane per lower-triangle entry adds Lambda_ij onto the canonical word (s_addr)
//   gB      one lane per row forms (Lambda d)_i in ascending column order: gB += (Lambda d)_i, hdiag += Lambda_ii
//           (k_finalize turns gB into rhs = -gB + ...; the diagonal feeds the Jacobi scaling and the LM clamp)
__global__ __launch_bounds__(PRIOR_THREADS) void k_priors(Dev d, int cost_only, const double* cam, const double* views, double* cost_out) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, NC = d.nc, A0 = 6 * d.F + 3 * d.Q;
  if (blockIdx.x == 0) {
    __shared__ double part[PRIOR_PER_WG];
    const uint32_t nc_rows = d.pr_cam_info ? NC : 0u, rows = nc_rows + 6 * d.pr_n;
    double s = 0.0;
    for (uint32_t r = tid; r < rows; r += PRIOR_THREADS) { double di; const double ld = prior_row(d, cam, views, r, nc_rows, &di); s += di * ld; }
    s = wave_sum(s);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (tid == 0) *cost_out += 0.5 * (((part[0] + part[1]) + part[2]) + part[3]);
    if (cost_only || !d.pr_cam_info) return;
    if (tid < NC * (NC + 1) / 2) {
      uint32_t i = 0; while ((i + 1) * (i + 2) / 2 <= tid) ++i;
      const uint32_t j = tid - i * (i + 1) / 2;
      *s_addr(d, A0 + i, A0 + j) += d.pr_cam_info[i * NC + j];
    } else if (tid >= 64 && tid < 64 + NC) {
      const uint32_t i = tid - 64;
      double di;
      d.gB[A0 + i] += prior_row(d, cam, views, i, NC, &di);
      d.hdiag[A0 + i] += d.pr_cam_info[i * NC + i];
    }
    return;
  }
  const uint32_t k = (blockIdx.x - 1) * PRIOR_PER_WG + wave;
  if (cost_only || k >= d.pr_n) return;
  const uint32_t f = d.pr_frame[k];
  const double* A = d.pr_pose_info + 36 * (size_t)k;
  if (lane < 21) {
    uint32_t i = 0; while ((i + 1) * (i + 2) / 2 <= lane) ++i;
    const uint32_t j = lane - i * (i + 1) / 2;
    *s_addr(d, 6 * f + i, 6 * f + j) += A[i * 6 + j];
  } else if (lane >= 32 && lane < 38) {
    const uint32_t i = lane - 32;
    double di;
    d.gB[6 * f + i] += prior_row(d, cam, views, 6 * k + i, 0u, &di);
    d.hdiag[6 * f + i] += A[i * 6 + i];
  }
}

}  // namespace lifcal

static void sym_eig_jacobi(uint32_t n, std::vector<double>& A, std::vector<double>& w, std::vector<double>& V);   // covariance.hpp

namespace {

// layout of lifcal_ba_handle::pr_buf in doubles: cost words | camera mean | camera matrix | pose means | pose matrices
constexpr size_t PR_COST = 0, PR_CAM_MEAN = 2, PR_CAM_INFO = PR_CAM_MEAN + NCMAX, PR_POSE = PR_CAM_INFO + NCMAX * NCMAX;

// the device copy of the matrices with the live mask of this moment: camera slots by fixed_mask and the structural columns, poses by
// the refine-poses bit and the frame mask (lifcal_ba_set_fixed_frames marks the copy stale)
int apply_prior_mask(lifcal_ba_handle* h) {
  Dev& d = h->d;
  const uint32_t NC = d.nc, n = (uint32_t)h->pr_frame.size();
  std::vector<double>& st = h->pr_stage;
  st.assign(PR_POSE + 42 * (size_t)n, 0.0);
  if (!h->pr_cam_info.empty()) {
    auto live = [&](uint32_t j) { return !((d.fixed_mask >> j) & 1u); };
    for (uint32_t i = 0; i < NC; ++i) {
      st[PR_CAM_MEAN + i] = h->pr_cam_mean[i];
      for (uint32_t j = 0; j < NC; ++j) st[PR_CAM_INFO + i * NC + j] = live(i) && live(j) ? h->pr_cam_info[i * 17 + j] : 0.0;
    }
  }
  for (uint32_t k = 0; k < n; ++k) {
    const bool live = d.use_poses && h->frame_live_host[h->pr_frame[k]];
    for (uint32_t e = 0; e < 6; ++e) st[PR_POSE + 6 * (size_t)k + e] = h->pr_pose_mean[6 * (size_t)k + e];
    if (live) for (uint32_t e = 0; e < 36; ++e) st[PR_POSE + 6 * (size_t)n + 36 * (size_t)k + e] = h->pr_pose_info[36 * (size_t)k + e];
  }
  // (stream-ordered: sweeps still queued read the old copy to the end; the staging vector belongs to the handle)
  HIP_TRY(hipMemcpyAsync(h->pr_buf, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  h->prior_stale = false;
  return 0;
}

// the prior term at (cam, views): cost and blocks onto the bound copy of the reduced block, or (cost_only) the cost alone, added to *out
int launch_priors(lifcal_ba_handle* h, int cost_only, const double* cam, const double* views, double* out) {
  if (!h->has_priors) return 0;
  if (h->prior_stale) { if (int rc = apply_prior_mask(h)) return rc; }
  hipLaunchKernelGGL(k_priors, dim3(cost_only ? 1u : 1u + (h->d.pr_n + PRIOR_PER_WG - 1) / PRIOR_PER_WG), dim3(PRIOR_THREADS), 0, h->stream, h->d, cost_only, cam, views, out);
  HIP_TRY(hipGetLastError());
  return 0;
}

// the point priors at `pts`: cost and blocks into the point slabs (in front of k_promote_diag / k_jacobi / k_schur), or (cost_only)
// the cost alone, added to *out.  Nothing is launched without them
int launch_point_priors(lifcal_ba_handle* h, int cost_only, const double* pts, double* out) {
  if (!h->pp_active) return 0;
  HIP_TRY(launch_k_point_priors(h->pp, cost_only, pts, out, h->stream));   // (point_priors.hip: a code object of its own)
  return 0;
}

// rows the priors add to the residual vector as lifcal_ba_covariance counts it: one per live slot whose prior row is non-zero
uint64_t prior_rows(const lifcal_ba_handle* h, const std::vector<uint8_t>& frame_live) {
  uint64_t m = 0;
  if (h->pp_active)
    for (size_t k = 0; k < h->pp_point.size(); ++k)
      for (uint32_t i = 0; i < 3; ++i) { const double* r = h->pp_info.data() + 9 * k + 3 * i; if (r[0] != 0.0 || r[1] != 0.0 || r[2] != 0.0) ++m; }
  if (!h->has_priors) return m;
  const Dev& d = h->d;
  auto nonzero_row = [](const double* A, uint32_t ld, uint32_t i, uint32_t n, auto&& live) { for (uint32_t j = 0; j < n; ++j) if (live(j) && A[i * ld + j] != 0.0) return true; return false; };
  if (!h->pr_cam_info.empty()) {
    auto live = [&](uint32_t j) { return !((d.fixed_mask >> j) & 1u); };
    for (uint32_t i = 0; i < d.nc; ++i) if (live(i) && nonzero_row(h->pr_cam_info.data(), 17, i, d.nc, live)) ++m;
  }
  for (size_t k = 0; k < h->pr_frame.size(); ++k) {
    if (!d.use_poses || !frame_live[h->pr_frame[k]]) continue;
    for (uint32_t i = 0; i < 6; ++i) if (nonzero_row(h->pr_pose_info.data() + 36 * k, 6, i, 6, [](uint32_t) { return true; })) ++m;
  }
  return m;
}

// symmetric, finite, non-negative diagonal, no eigenvalue below -1e-12 lambda_max
const char* check_information(const double* A, uint32_t n) {
  for (uint32_t i = 0; i < n * n; ++i) if (!std::isfinite(A[i])) return "a non-finite entry";
  for (uint32_t i = 0; i < n; ++i) if (A[i * n + i] < 0.0) return "a negative diagonal entry";
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = 0; j < i; ++j)
      if (std::fabs(A[i * n + j] - A[j * n + i]) > 1e-12 * std::sqrt(A[i * n + i] * A[j * n + j])) return "a matrix that is not symmetric";
  std::vector<double> S((size_t)n * n), w, V;
  for (uint32_t i = 0; i < n; ++i) for (uint32_t j = 0; j < n; ++j) S[(size_t)i * n + j] = 0.5 * (A[i * n + j] + A[j * n + i]);
  sym_eig_jacobi(n, S, w, V);
  double wmax = 0.0, wmin = 0.0;
  for (double x : w) { wmax = std::max(wmax, x); wmin = std::min(wmin, x); }
  if (wmin < -1e-12 * wmax || (wmax == 0.0 && wmin < 0.0)) return "a matrix that is not positive semi-definite";
  return nullptr;
}

}  // namespace

extern "C" {

int lifcal_ba_check_priors(uint32_t n_frames, const lifcal_ba_priors* p) {
  if (!p) { g_last_error = "lifcal_ba_check_priors: null argument"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if ((p->cam_mean == nullptr) != (p->cam_info == nullptr)) { g_last_error = "lifcal_ba_check_priors: cam_mean and cam_info go together"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (p->n_pose_priors && (!p->pose_frame || !p->pose_mean || !p->pose_info)) { g_last_error = "lifcal_ba_check_priors: n_pose_priors > 0 with a null pose array"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (p->cam_mean) {
    for (int i = 0; i < 17; ++i) if (!std::isfinite(p->cam_mean[i])) { g_last_error = "lifcal_ba_check_priors: camera prior: a non-finite mean"; return LIFCAL_BA_ERR_INVALID_ARG; }
    if (const char* e = check_information(p->cam_info, 17)) { g_last_error = std::string("lifcal_ba_check_priors: camera prior: ") + e; return LIFCAL_BA_ERR_INVALID_ARG; }
  }
  for (uint32_t k = 0; k < p->n_pose_priors; ++k) {
    const std::string who = "lifcal_ba_check_priors: pose prior " + std::to_string(k) + ": ";
    if (k && p->pose_frame[k] <= p->pose_frame[k - 1]) { g_last_error = who + "frames are not strictly ascending"; return LIFCAL_BA_ERR_INVALID_ARG; }
    for (int i = 0; i < 6; ++i) if (!std::isfinite(p->pose_mean[6 * (size_t)k + i])) { g_last_error = who + "a non-finite mean"; return LIFCAL_BA_ERR_INVALID_ARG; }
    if (const char* e = check_information(p->pose_info + 36 * (size_t)k, 6)) { g_last_error = who + e; return LIFCAL_BA_ERR_INVALID_ARG; }
  }
  for (uint32_t k = 0; k < p->n_pose_priors; ++k)
    if (p->pose_frame[k] >= n_frames) { g_last_error = "lifcal_ba_check_priors: pose prior " + std::to_string(k) + ": frame " + std::to_string(p->pose_frame[k]) + " of " + std::to_string(n_frames); return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  return 0;
}

int lifcal_ba_set_priors(lifcal_ba_handle* h, const lifcal_ba_priors* p) {
  if (!h) return LIFCAL_BA_ERR_INVALID_ARG;
  if (h->opt.world_size > 1) { g_last_error = "lifcal_ba_set_priors: world_size > 1 is not supported (every rank would add the term: a follow-up)"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (p) { if (int rc = lifcal_ba_check_priors(h->d.F, p)) return rc; }
  Dev& d = h->d;
  HIP_TRY(hipSetDevice(h->opt.device));
  HIP_TRY(hipStreamSynchronize(h->stream));   // a solve boundary, as lifcal_ba_set_fixed_frames
  const uint32_t n = p ? p->n_pose_priors : 0;
  const bool any = p && (p->cam_mean || n);
  if (any) {
    const size_t need = PR_POSE + 42 * (size_t)n;
    if (need > h->pr_cap) {
      double* buf = nullptr; uint32_t* fr = nullptr;
      if (hipMalloc((void**)&buf, need * sizeof(double)) != hipSuccess || hipMalloc((void**)&fr, std::max<size_t>(1, n) * sizeof(uint32_t)) != hipSuccess) {
        if (buf) (void)hipFree(buf);
        g_last_error = "lifcal_ba_set_priors: hipMalloc failed"; return LIFCAL_BA_ERR_NOMEM;
      }
      if (h->pr_buf) (void)hipFree(h->pr_buf);
      if (h->pr_frame_dev) (void)hipFree(h->pr_frame_dev);
      h->pr_buf = buf; h->pr_frame_dev = fr; h->pr_cap = need;
    }
  }
  h->pr_cam_mean.clear(); h->pr_cam_info.clear(); h->pr_frame.clear(); h->pr_pose_mean.clear(); h->pr_pose_info.clear();
  d.pr_cam_mean = d.pr_cam_info = d.pr_pose_mean = d.pr_pose_info = nullptr; d.pr_frame = nullptr; d.pr_n = 0;
  h->has_priors = false; h->prior_stale = false;
  h->sigma_valid = false;   // the Hessian diagonal behind the Jacobi scaling changes: a new solve
  h->swept = false;
  if (!any) return 0;
  if (p->cam_mean) {
    h->pr_cam_mean.assign(p->cam_mean, p->cam_mean + 17);
    h->pr_cam_info.resize(17 * 17);
    for (int i = 0; i < 17; ++i) for (int j = 0; j < 17; ++j) h->pr_cam_info[i * 17 + j] = 0.5 * (p->cam_info[i * 17 + j] + p->cam_info[j * 17 + i]);
    d.pr_cam_mean = h->pr_buf + PR_CAM_MEAN; d.pr_cam_info = h->pr_buf + PR_CAM_INFO;
  }
  if (n) {
    h->pr_frame.assign(p->pose_frame, p->pose_frame + n);
    h->pr_pose_mean.assign(p->pose_mean, p->pose_mean + 6 * (size_t)n);
    h->pr_pose_info.resize(36 * (size_t)n);
    for (uint32_t k = 0; k < n; ++k)
      for (int i = 0; i < 6; ++i) for (int j = 0; j < 6; ++j) h->pr_pose_info[36 * (size_t)k + i * 6 + j] = 0.5 * (p->pose_info[36 * (size_t)k + i * 6 + j] + p->pose_info[36 * (size_t)k + j * 6 + i]);
    HIP_TRY(hipMemcpy(h->pr_frame_dev, h->pr_frame.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice));
    d.pr_frame = h->pr_frame_dev; d.pr_pose_mean = h->pr_buf + PR_POSE; d.pr_pose_info = h->pr_buf + PR_POSE + 6 * (size_t)n; d.pr_n = n;
  }
  h->has_priors = true;
  return apply_prior_mask(h);
}

int lifcal_ba_prior_cost(lifcal_ba_handle* h, double* cam_cost, double* pose_cost) {
  if (!h) return LIFCAL_BA_ERR_INVALID_ARG;
  double c[2] = {0.0, 0.0};
  if (h->has_priors) {
    HIP_TRY(hipSetDevice(h->opt.device));
    if (h->prior_stale) { if (int rc = apply_prior_mask(h)) return rc; }
    HIP_TRY(hipMemsetAsync(h->pr_buf + PR_COST, 0, 2 * sizeof(double), h->stream));
    // the kernel's cost pass, once with the camera prior alone and once with the pose priors alone
    Dev dc = h->d; dc.pr_n = 0;
    Dev dp = h->d; dp.pr_cam_info = nullptr;
    if (h->d.pr_cam_info) hipLaunchKernelGGL(k_priors, dim3(1), dim3(PRIOR_THREADS), 0, h->stream, dc, 1, (const double*)h->d.cam, (const double*)h->d.views, h->pr_buf + PR_COST);
    if (h->d.pr_n) hipLaunchKernelGGL(k_priors, dim3(1), dim3(PRIOR_THREADS), 0, h->stream, dp, 1, (const double*)h->d.cam, (const double*)h->d.views, h->pr_buf + PR_COST + 1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c, h->pr_buf + PR_COST, sizeof(c), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
  }
  if (cam_cost) *cam_cost = c[0];
  if (pose_cost) *pose_cost = c[1];
  return 0;
}

int lifcal_ba_check_point_priors(uint32_t n_points, const lifcal_ba_point_priors* p) {
  if (!p) { g_last_error = "lifcal_ba_check_point_priors: null argument"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (p->n && (!p->point || !p->mean || !p->info)) { g_last_error = "lifcal_ba_check_point_priors: n > 0 with a null array"; return LIFCAL_BA_ERR_INVALID_ARG; }
  for (uint32_t k = 0; k < p->n; ++k) {
    const std::string who = "lifcal_ba_check_point_priors: prior " + std::to_string(k) + ": ";
    if (k && p->point[k] <= p->point[k - 1]) { g_last_error = who + "point ids are not strictly ascending"; return LIFCAL_BA_ERR_INVALID_ARG; }
    for (int i = 0; i < 3; ++i) if (!std::isfinite(p->mean[3 * (size_t)k + i])) { g_last_error = who + "a non-finite mean"; return LIFCAL_BA_ERR_INVALID_ARG; }
    if (const char* e = check_information(p->info + 9 * (size_t)k, 3)) { g_last_error = who + e; return LIFCAL_BA_ERR_INVALID_ARG; }
  }
  for (uint32_t k = 0; k < p->n; ++k)
    if (p->point[k] >= n_points) { g_last_error = "lifcal_ba_check_point_priors: prior " + std::to_string(k) + ": point " + std::to_string(p->point[k]) + " of " + std::to_string(n_points); return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  return 0;
}

int lifcal_ba_set_point_priors(lifcal_ba_handle* h, const lifcal_ba_point_priors* p) {
  if (!h) return LIFCAL_BA_ERR_INVALID_ARG;
  if (!h->pp_entry) { g_last_error = "lifcal_ba_set_point_priors: the handle was not created by lifcal_ba_create_with_point_priors"; return LIFCAL_BA_ERR_INVALID_ARG; }
  const uint32_t n = (uint32_t)h->pp_point.size();
  if (p) {
    if (int rc = lifcal_ba_check_point_priors(h->d.P, p)) return rc;
    if (p->n != n || !std::equal(h->pp_point.begin(), h->pp_point.end(), p->point)) {
      g_last_error = "lifcal_ba_set_point_priors: the point set differs from the one given at create (the planner placed those points)"; return LIFCAL_BA_ERR_INVALID_ARG;
    }
  }
  if (!n) return 0;
  HIP_TRY(hipSetDevice(h->opt.device));
  HIP_TRY(hipStreamSynchronize(h->stream));   // a solve boundary, as lifcal_ba_set_priors
  std::vector<double>& st = h->pp_stage;
  st.assign(2 + 12 * (size_t)n, 0.0);
  h->pp_info.assign(9 * (size_t)n, 0.0);
  if (p) {
    std::copy(p->mean, p->mean + 3 * (size_t)n, st.begin() + 2);
    for (uint32_t k = 0; k < n; ++k)
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) h->pp_info[9 * (size_t)k + 3 * i + j] = 0.5 * (p->info[9 * (size_t)k + 3 * i + j] + p->info[9 * (size_t)k + 3 * j + i]);
    std::copy(h->pp_info.begin(), h->pp_info.end(), st.begin() + 2 + 3 * (size_t)n);
  }
  HIP_TRY(hipMemcpyAsync(h->pp_buf, st.data(), st.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  // a problem that does not refine its points drops the term: the points are no parameters
  h->pp_active = p != nullptr && h->d.use_points;
  h->sigma_valid = false;   // the Hessian diagonal behind the Jacobi scaling changes: a new solve
  h->swept = false;
  return 0;
}

int lifcal_ba_point_prior_cost(lifcal_ba_handle* h, double* cost) {
  if (!h || !cost) return LIFCAL_BA_ERR_INVALID_ARG;
  *cost = 0.0;
  if (!h->pp_active) return 0;
  HIP_TRY(hipSetDevice(h->opt.device));
  HIP_TRY(hipMemsetAsync(h->pp_buf, 0, sizeof(double), h->stream));
  if (int rc = launch_point_priors(h, 1, h->d.pts, h->pp_buf)) return rc;
  HIP_TRY(hipMemcpyAsync(cost, h->pp_buf, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  return 0;
}

int lifcal_prior_from_covariance(const double* cov, uint32_t n, uint64_t use_mask, double rcond, double* info, uint32_t* rank) {
  if (!cov || !info || n == 0 || n > 64 || !(rcond >= 0.0)) { g_last_error = "lifcal_prior_from_covariance: null argument, n outside 1..64 or rcond < 0"; return LIFCAL_BA_ERR_INVALID_ARG; }
  std::vector<uint32_t> sel;
  for (uint32_t i = 0; i < n; ++i) if ((use_mask >> i) & 1ull) sel.push_back(i);
  const uint32_t m = (uint32_t)sel.size();
  for (uint32_t i = 0; i < m; ++i)
    for (uint32_t j = 0; j < m; ++j) if (!std::isfinite(cov[(size_t)sel[i] * n + sel[j]])) { g_last_error = "lifcal_prior_from_covariance: a non-finite entry"; return LIFCAL_BA_ERR_INVALID_ARG; }
  std::fill(info, info + (size_t)n * n, 0.0);
  uint32_t kept = 0;
  if (m) {
    // the rank is decided on the Jacobi-scaled matrix (unit diagonal: the slots have different units), as lifcal_ba_covariance
    // decides it; the pseudo-inverse is the Moore-Penrose inverse of the matrix itself over its `kept` largest eigenvalues
    std::vector<double> sc(m), A((size_t)m * m), w, V;
    for (uint32_t i = 0; i < m; ++i) { const double c = cov[(size_t)sel[i] * n + sel[i]]; sc[i] = c > 0.0 ? 1.0 / std::sqrt(c) : 1.0; }
    for (uint32_t i = 0; i < m; ++i)
      for (uint32_t j = 0; j < m; ++j) A[(size_t)i * m + j] = 0.5 * (cov[(size_t)sel[i] * n + sel[j]] + cov[(size_t)sel[j] * n + sel[i]]) * sc[i] * sc[j];
    sym_eig_jacobi(m, A, w, V);
    double wmax = 0.0;
    for (double x : w) wmax = std::max(wmax, x);
    for (uint32_t e = 0; e < m; ++e) if (w[e] > 0.0 && w[e] >= rcond * wmax) ++kept;
    for (uint32_t i = 0; i < m; ++i)
      for (uint32_t j = 0; j < m; ++j) A[(size_t)i * m + j] = 0.5 * (cov[(size_t)sel[i] * n + sel[j]] + cov[(size_t)sel[j] * n + sel[i]]);
    sym_eig_jacobi(m, A, w, V);
    std::vector<uint32_t> order(m);
    for (uint32_t e = 0; e < m; ++e) order[e] = e;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return w[x] > w[y]; });
    for (uint32_t i = 0; i < m; ++i)
      for (uint32_t j = 0; j <= i; ++j) {
        double s = 0.0;
        for (uint32_t q = 0; q < kept; ++q) { const uint32_t e = order[q]; if (w[e] > 0.0) s += V[(size_t)i * m + e] * V[(size_t)j * m + e] / w[e]; }
        info[(size_t)sel[i] * n + sel[j]] = s; info[(size_t)sel[j] * n + sel[i]] = s;
      }
  }
  if (rank) *rank = kept;
  return 0;
}

}  // extern "C"
