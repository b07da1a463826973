// residuals.hpp — lifcal_ba_residual_report / lifcal_ba_residual_groups: their two kernels, the host-side group index, then the host
// driver (included at the end of lifcal_ba.hip, behind the handle and build_stats_tables).  DESIGN.md section 7j.
//
//   k_residuals    per-observation e = projected - observed, loss weight and lens id at the stored parameters, written in the CALLER's
//                  observation order (the tile walk of k_project_obs, the batched loads of k_cost)
//   k_group_stats  segmented sums of those arrays over a CSR index (off, idx): one wave per segment, lane l adds entries l, l + 64, ...
//                  in that order, the lanes are folded by the xor butterfly.  No atomics: every sum has ONE order, which depends
//                  neither on the grid nor on options.deterministic.
#pragma once

namespace lifcal {

static_assert(sizeof(lifcal_ba_group_stats) == 64, "lifcal_ba_group_stats is one 64-byte row");

// |e|^2 and the weight rho'(|e|^2) of the Cauchy loss, every operation rounded on its own (no fma): the host reproduces both from
// ex, ey to the bit
LIFCAL_DEV double residual_sq(double ex, double ey) {
#pragma clang fp contract(off)
  const double xx = ex * ex, yy = ey * ey;
  return xx + yy;
}
LIFCAL_DEV double residual_weight(double sq, double loss_b) {
#pragma clang fp contract(off)
  const double t = sq / loss_b;
  return 1.0 / (1.0 + t);
}

template <int NR, bool TAN, bool ADJ>
__global__ __launch_bounds__(256) void k_residuals(Dev d, TileSet ts, const uint32_t* __restrict__ src, const CamConsts* camc, const double* ft_tab,
                                                   const double* lt_tab, const double* pts, double loss_b, double* __restrict__ ex_out,
                                                   double* __restrict__ ey_out, double* __restrict__ w_out, uint32_t* __restrict__ lens_out) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
  const CamConsts c = *camc;
  for (uint32_t tile = wave; tile < ts.n_tiles; tile += n_waves) {
    const uint32_t slot = tile * 64 + lane;
    const uint32_t cnt = ts.slot_cnt[slot];
    const uint32_t row0 = ts.tile_row0[tile], kmax = ts.tile_row0[tile + 1] - row0;
    const double* ft = ft_tab + (size_t)ts.slot_fr[slot] * FRAME_STRIDE;
    const double* P = pts + 3 * (size_t)ts.slot_pt[slot];
    GroupConsts g;
    {
      const double P0 = P[0], P1 = P[1], P2 = P[2];
      group_prepare(c, ft[0] * P0 + ft[1] * P1 + ft[2] * P2 + ft[9], ft[3] * P0 + ft[4] * P1 + ft[5] * P2 + ft[10],
                    ft[6] * P0 + ft[7] * P1 + ft[8] * P2 + ft[11], g);
    }
    // eight steps at a time, every load of a stage in flight together (clamped rows: unconditional loads), as in k_cost: lens
    // indices, then lens values + u, v + the observation's input index, then the arithmetic and the scattered stores
    for (uint32_t k0 = 0; k0 < kmax; k0 += 8) {
      uint32_t li[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) li[q] = ts.ell_lens[((size_t)row0 + min(k0 + (uint32_t)q, kmax - 1)) * 64 + lane];
      double2 La[8], Lb[8]; double uu[8], vv[8]; uint32_t dst[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const size_t at = ((size_t)row0 + min(k0 + (uint32_t)q, kmax - 1)) * 64 + lane;
        const double* L = lt_tab + (size_t)li[q] * LENS_STRIDE;
        La[q] = *reinterpret_cast<const double2*>(L); Lb[q] = *reinterpret_cast<const double2*>(L + 2);
        uu[q] = ts.ell_u[at]; vv[q] = ts.ell_v[at]; dst[q] = src[at];
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (k0 + (uint32_t)q < cnt) {
          double ex, ey;
          obs_value<NR, TAN, ADJ>(c, g, La[q].x, La[q].y, Lb[q].x, Lb[q].y, uu[q], vv[q], ex, ey);
          const uint32_t i = dst[q];
          ex_out[i] = ex; ey_out[i] = ey; lens_out[i] = li[q];
          w_out[i] = d.robust ? residual_weight(residual_sq(ex, ey), loss_b) : 1.0;
        }
      }
    }
  }
}

// One row per segment of the CSR index: off[n_keys + 1], idx[off[n_keys]] (idx == nullptr: the identity, the one-segment index of
// the total).  The caller guarantees idx[j] < the length of ex / ey / w (the host builds idx; caller keys are checked there).
__global__ __launch_bounds__(256) void k_group_stats(const uint32_t* __restrict__ off, const uint32_t* __restrict__ idx, uint32_t n_keys,
                                                     const double* __restrict__ ex, const double* __restrict__ ey, const double* __restrict__ w,
                                                     double thr2, lifcal_ba_group_stats* __restrict__ out) {
#pragma clang fp contract(off)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const uint32_t n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t seg = wave; seg < n_keys; seg += n_waves) {
    const uint32_t b = off[seg], e = off[seg + 1];
    double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0, sw = 0.0, mx = 0.0, my = 0.0;
    uint32_t n = 0, inl = 0;
    // eight entries of the lane at a time: the gathers through idx are scattered 8-byte reads, so their latency is covered by
    // having all of a batch in flight (clamped positions: unconditional loads); the adds stay in entry order
    for (uint32_t j0 = b + lane; j0 < e; j0 += 64u * 8u) {
      uint32_t ii[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) { const uint32_t j = min(j0 + 64u * (uint32_t)q, e - 1); ii[q] = idx ? idx[j] : j; }
      double vx[8], vy[8], vw[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) { vx[q] = ex[ii[q]]; vy[q] = ey[ii[q]]; vw[q] = w[ii[q]]; }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        if (j0 + 64u * (uint32_t)q < e) {
          const double xx = vx[q] * vx[q], yy = vy[q] * vy[q];
          sx += vx[q]; sy += vy[q]; sxx += xx; syy += yy; sw += vw[q];
          mx = fmax(mx, fabs(vx[q])); my = fmax(my, fabs(vy[q]));
          n += 1u; if (xx + yy <= thr2) inl += 1u;
        }
      }
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sxx = wave_sum(sxx); syy = wave_sum(syy); sw = wave_sum(sw);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      mx = fmax(mx, __shfl_xor(mx, m, 64)); my = fmax(my, __shfl_xor(my, m, 64));
      n += (uint32_t)__shfl_xor((int)n, m, 64); inl += (uint32_t)__shfl_xor((int)inl, m, 64);
    }
    if (lane == 0) {
      lifcal_ba_group_stats r;
      r.sum_x = sx; r.sum_y = sy; r.sum_xx = sxx; r.sum_yy = syy; r.sum_w = sw; r.max_abs_x = mx; r.max_abs_y = my; r.n = n; r.n_inliers = inl;
      out[seg] = r;
    }
  }
}

}  // namespace lifcal

// stable counting sort of the positions by key
extern "C" int lifcal_group_index(uint32_t n, uint32_t n_keys, const uint32_t* key, uint32_t* off, uint32_t* idx) {
  if (!off || (n && (!key || !idx))) { g_last_error = "lifcal_group_index: null argument"; return LIFCAL_BA_ERR_INVALID_ARG; }
  for (uint32_t k = 0; k <= n_keys; ++k) off[k] = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (key[i] >= n_keys) { g_last_error = "lifcal_group_index: key[" + std::to_string(i) + "] = " + std::to_string(key[i]) + " is not below n_keys = " + std::to_string(n_keys); return LIFCAL_BA_ERR_INVALID_ARG; }
    ++off[key[i] + 1];
  }
  for (uint32_t k = 0; k < n_keys; ++k) off[k + 1] += off[k];
  if (n) {
    std::vector<uint32_t> at(off, off + n_keys);
    for (uint32_t i = 0; i < n; ++i) idx[at[key[i]]++] = i;
  }
  return 0;
}

namespace {

// frame, point and lens of every observation in the caller's order, read back from the plan's two tile sets (the lens ids never
// leave the planner otherwise), their CSR indices, and the device buffers of the report.  Everything is owned by the handle.
int residual_state(lifcal_ba_handle* h) {
  if (h->res_ready) return 0;
  const Plan& L = h->plan;
  const uint32_t n = h->prob.n_obs;
  std::vector<uint32_t> key[3];
  for (auto& k : key) k.assign(n, 0);
  uint32_t seen = 0;
  auto walk = [&](uint32_t n_tiles, const std::vector<uint32_t>& row0, const std::vector<uint32_t>& s_pt, const std::vector<uint32_t>& s_fr,
                  const std::vector<uint32_t>& s_cnt, const uint32_t* lens, const std::vector<uint32_t>& src) -> bool {
    for (uint32_t t = 0; t < n_tiles; ++t)
      for (uint32_t lane = 0; lane < 64; ++lane) {
        const size_t slot = (size_t)t * 64 + lane;
        for (uint32_t k = 0; k < s_cnt[slot]; ++k) {
          const size_t at = ((size_t)row0[t] + k) * 64 + lane;
          const uint32_t i = src[at];
          if (i >= n || s_fr[slot] >= L.F || s_pt[slot] >= L.P || lens[at] >= L.n_lenses) return false;
          key[0][i] = s_fr[slot]; key[1][i] = s_pt[slot]; key[2][i] = lens[at];
          ++seen;
        }
      }
    return true;
  };
  const bool ok = walk(L.n_tiles, L.tile_row0, L.slot_pt, L.slot_fr, L.slot_cnt, L.ell_lens.data(), L.ell_src) &&
                  walk(L.pass_tiles() * L.n_passes, L.v2_tile_row0, L.v2f_pt, L.v2f_fr, L.v2f_cnt, L.v2_lens.data(), L.v2_src);
  if (!ok || seen != n) { g_last_error = "lifcal_ba_residual_report: internal: the tile payload does not cover the observations once each"; return LIFCAL_BA_ERR_INVALID_ARG; }
  const uint32_t n_keys[3] = {L.F, L.P, L.n_lenses};
  std::vector<uint32_t> off, idx(n);
  for (int t = 0; t < 3; ++t) {
    off.assign((size_t)n_keys[t] + 1, 0);
    if (int rc = lifcal_group_index(n, n_keys[t], key[t].data(), off.data(), idx.data())) return rc;
    if (int rc = dev_upload(h, &h->res_off[t], off)) return rc;
    if (int rc = dev_upload(h, &h->res_idx[t], idx)) return rc;
  }
  { const std::vector<uint32_t> tot = {0u, n}; if (int rc = dev_upload(h, &h->res_tot_off, tot)) return rc; }
  if (int rc = dev_upload(h, &h->res_src1, L.ell_src)) return rc;
  if (int rc = dev_upload(h, &h->res_src2, L.v2_src)) return rc;
  if (int rc = dev_alloc(h, &h->res_ex, n)) return rc;
  if (int rc = dev_alloc(h, &h->res_ey, n)) return rc;
  if (int rc = dev_alloc(h, &h->res_w, n)) return rc;
  if (int rc = dev_upload(h, &h->res_lens, key[2])) return rc;
  if (int rc = dev_alloc(h, &h->res_rows, (size_t)L.F + L.P + L.n_lenses + 1)) return rc;
  h->res_ready = true;
  return 0;
}

// e, weight and lens id of every observation at the stored parameters into the handle's buffers
int launch_residuals(lifcal_ba_handle* h) {
  Dev& d = h->d;
  if (int rc = build_stats_tables(h)) return rc;
  const TileSet* sets[2] = {&h->ts1, &h->ts2};
  const uint32_t* srcs[2] = {h->res_src1, h->res_src2};
  const double loss_b = d.loss_scale * d.loss_scale;
  for (int k = 0; k < 2; ++k) {
    const TileSet* ts = sets[k];
    if (!ts->n_tiles) continue;
    const uint32_t grid = std::max(1u, std::min((ts->n_tiles + 3) / 4, 2048u));
#define CALL_RES(NR, TAN, ADJ) hipLaunchKernelGGL((k_residuals<NR, TAN, ADJ>), dim3(grid), dim3(256), 0, h->stream, d, *ts, srcs[k], (const CamConsts*)h->camc_stats, (const double*)d.ft_c, (const double*)d.lt_c, (const double*)d.pts, loss_b, h->res_ex, h->res_ey, h->res_w, h->res_lens)
    DISPATCH_CFG(h, CALL_RES);
#undef CALL_RES
  }
  HIP_TRY(hipGetLastError());
  return 0;
}

void launch_group_stats(lifcal_ba_handle* h, const uint32_t* off, const uint32_t* idx, uint32_t n_keys, double thr, lifcal_ba_group_stats* rows) {
  if (!n_keys) return;
  const uint32_t grid = std::max(1u, std::min((n_keys + 3) / 4, 2048u));
  hipLaunchKernelGGL(k_group_stats, dim3(grid), dim3(256), 0, h->stream, off, idx, n_keys, (const double*)h->res_ex, (const double*)h->res_ey, (const double*)h->res_w, thr * thr, rows);
}

int residual_entry_checks(lifcal_ba_handle* h, const char* who) {
  if (h->opt.world_size > 1) { g_last_error = std::string(who) + ": world_size > 1 is not supported (every rank holds its own points' observations only)"; return LIFCAL_BA_ERR_INVALID_ARG; }
  return 0;
}

}  // namespace

extern "C" int lifcal_ba_residual_report(lifcal_ba_handle* h, lifcal_ba_residual_report_io* io) {
  if (!h || !io) { g_last_error = "lifcal_ba_residual_report: null handle or report"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (int rc = residual_entry_checks(h, "lifcal_ba_residual_report")) return rc;
  const Plan& L = h->plan;
  const size_t n = h->prob.n_obs;
  HIP_TRY(hipSetDevice(h->opt.device));
  if (int rc = residual_state(h)) return rc;
  HIP_TRY(hipEventRecord(h->ev0, h->stream));
  if (int rc = launch_residuals(h)) return rc;
  // rows: [frames | points | lenses | total]
  lifcal_ba_group_stats* rows[3] = {h->res_rows, h->res_rows + L.F, h->res_rows + (size_t)L.F + L.P};
  lifcal_ba_group_stats* const total = h->res_rows + (size_t)L.F + L.P + L.n_lenses;
  lifcal_ba_group_stats* const want[3] = {io->per_frame, io->per_point, io->per_lens};
  const uint32_t n_keys[3] = {L.F, L.P, L.n_lenses};
  for (int t = 0; t < 3; ++t) if (want[t]) launch_group_stats(h, h->res_off[t], h->res_idx[t], n_keys[t], io->inlier_threshold, rows[t]);
  launch_group_stats(h, h->res_tot_off, nullptr, 1u, io->inlier_threshold, total);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipEventRecord(h->ev1, h->stream));
  for (int t = 0; t < 3; ++t) if (want[t] && n_keys[t]) HIP_TRY(hipMemcpyAsync(want[t], rows[t], (size_t)n_keys[t] * sizeof(lifcal_ba_group_stats), hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&io->total, total, sizeof(lifcal_ba_group_stats), hipMemcpyDeviceToHost, h->stream));
  if (n) {
    if (io->ex) HIP_TRY(hipMemcpyAsync(io->ex, h->res_ex, n * 8, hipMemcpyDeviceToHost, h->stream));
    if (io->ey) HIP_TRY(hipMemcpyAsync(io->ey, h->res_ey, n * 8, hipMemcpyDeviceToHost, h->stream));
    if (io->weight) HIP_TRY(hipMemcpyAsync(io->weight, h->res_w, n * 8, hipMemcpyDeviceToHost, h->stream));
    if (io->lens) HIP_TRY(hipMemcpyAsync(io->lens, h->res_lens, n * 4, hipMemcpyDeviceToHost, h->stream));
  }
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (io->lens_xy && !L.lens_xy.empty()) std::memcpy(io->lens_xy, L.lens_xy.data(), L.lens_xy.size() * sizeof(double));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  io->seconds = 1e-3 * (double)ms;
  return 0;
}

extern "C" int lifcal_ba_residual_groups(lifcal_ba_handle* h, double inlier_threshold, uint32_t n_keys, const uint32_t* key, lifcal_ba_group_stats* out) {
  if (!h || !out || !n_keys || (h->prob.n_obs && !key)) { g_last_error = "lifcal_ba_residual_groups: null handle, keys or output, or n_keys = 0"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (int rc = residual_entry_checks(h, "lifcal_ba_residual_groups")) return rc;
  const uint32_t n = h->prob.n_obs;
  // the index is built (and every key checked) on the host before anything is launched: the kernel never sees an unchecked key
  std::vector<uint32_t> off((size_t)n_keys + 1), idx(n);
  if (int rc = lifcal_group_index(n, n_keys, key, off.data(), idx.data())) { g_last_error = "lifcal_ba_residual_groups: " + g_last_error; return rc; }
  HIP_TRY(hipSetDevice(h->opt.device));
  if (int rc = residual_state(h)) return rc;
  uint32_t *d_off = nullptr, *d_idx = nullptr; lifcal_ba_group_stats* d_rows = nullptr;
  auto release = [&]() { for (void* q : {(void*)d_off, (void*)d_idx, (void*)d_rows}) if (q) (void)hipFree(q); };
  hipError_t e = hipMalloc((void**)&d_off, off.size() * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&d_idx, std::max<size_t>(1, idx.size()) * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&d_rows, (size_t)n_keys * sizeof(lifcal_ba_group_stats));
  if (e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, h->stream);
  if (e == hipSuccess && n) e = hipMemcpyAsync(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, h->stream);
  if (e != hipSuccess) { (void)hipStreamSynchronize(h->stream); release(); g_last_error = std::string("lifcal_ba_residual_groups: ") + hipGetErrorString(e); return LIFCAL_BA_ERR_HIP; }
  if (int rc = launch_residuals(h)) { (void)hipStreamSynchronize(h->stream); release(); return rc; }
  launch_group_stats(h, d_off, d_idx, n_keys, inlier_threshold, d_rows);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(out, d_rows, (size_t)n_keys * sizeof(lifcal_ba_group_stats), hipMemcpyDeviceToHost, h->stream);
  const hipError_t es = hipStreamSynchronize(h->stream);   // (always: off / idx are read by the queued copies and kernels)
  if (e == hipSuccess) e = es;
  release();
  if (e != hipSuccess) { g_last_error = std::string("lifcal_ba_residual_groups: ") + hipGetErrorString(e); return LIFCAL_BA_ERR_HIP; }
  return 0;
}
