// depth_views.hpp — depth maps of several frames against each other through the calibrated camera and the poses (parts (d)-(f) of
// include/lifcal_depth.h).  Included in lifcal_ba.hip after depth.hpp (uses its decode / back_project /
// to_world / k_depth_frames / Scratch / lifcal_depth_handle / DEPTH_TRY and frame_eval of device_model.hpp).
//
//   k_depth_project    the forward model (what projectPointBack inverts) per 3D point, one lane per point
//   k_view_pairs       RT_t * RT_s^-1 for every (source map, target slot) of a batch, 12 doubles each
//   k_depth_views      every valid source pixel against its 2 span targets: classes, support / conflict, the pair table's
//                      per-workgroup counts and sums, and (fusion) the emit decision with the count per workgroup
//   k_views_fold       the per-workgroup parts of every pair slot: sums added in ascending workgroup order, counts added up
//   k_views_scan       exclusive scan of the per-workgroup emit counts
//   k_views_compact    src / n_merged of every emitting pixel at its scanned position
//   k_depth_fuse       the fused point of every emitted point, one lane each
// Everything is fp64 with contraction off: bit-identical to the line-by-line restatement up to the sines and cosines of frame_eval.
#pragma once

namespace depth {

struct ViewCam {
  double fL, bL0, B, cx, cy, k0, k1, p0, p1, spx, spy;
  int32_t nr, tan;
};

inline ViewCam view_cam(const lifcal_depth_camera& c) {
  const DenseCam<double> d = dense_cam<double>(c, nullptr, 0.0);
  ViewCam v{};
  v.fL = d.fL; v.bL0 = d.bL0; v.B = d.B; v.cx = d.cx; v.cy = d.cy; v.k0 = d.k0; v.k1 = d.k1; v.p0 = d.p0; v.p1 = d.p1; v.spx = d.spx; v.spy = d.spy;
  v.nr = (int32_t)(c.config & 3u); v.tan = (c.config & 4u) ? 1 : 0;
  return v;
}

LIFCAL_DEV bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// The model projectPointBack inverts, with radialDistortion / tangentialDistortion (src/CameraModel.h:205-241) evaluated at the
// undistorted point.  false: invalid (a coordinate not finite, Z <= 0, Z == fL, v not > 0).  c.nr, c.tan: wave-uniform.
LIFCAL_DEV bool forward(const ViewCam& c, double X, double Y, double Z, double& x_v, double& y_v, double& v) {
#pragma clang fp contract(off)
  if (!finite3(X, Y, Z) || Z <= 0.0 || Z == c.fL) return false;
  const double xu = X / Z * c.bL0;
  const double yu = Y / Z * c.bL0;
  double dx = 0.0, dy = 0.0;
  if (c.nr > 0) {
    const double r0 = xu * xu + yu * yu;
    double dr = c.k0 * r0;
    if (c.nr > 1) { const double r1 = r0 * r0; dr = dr + c.k1 * r1; }
    dx = dx + xu * dr;
    dy = dy + yu * dr;
  }
  if (c.tan) {
    const double r2 = xu * xu + yu * yu;
    dx = dx + (c.p0 * (r2 + 2.0 * xu * xu) + 2.0 * c.p1 * xu * yu);
    dy = dy + (c.p1 * (r2 + 2.0 * yu * yu) + 2.0 * c.p0 * xu * yu);
  }
  const double b = c.fL * Z / (Z - c.fL);
  v = (b - c.bL0) / c.B;
  if (!(v > 0.0)) return false;
  const double s = c.bL0 + v * c.B;
  x_v = (xu + dx) * s / c.bL0 / c.spx + c.cx;
  y_v = (yu + dy) * s / c.bL0 / c.spy + c.cy;
  return true;
}

// q = R p + t with a frame-table entry, or M p + m with a pair-table entry (same layout)
template <class FT>
LIFCAL_DEV void transform(const FT& ft, const double p[3], double q[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int j = 0; j < 3; ++j) q[j] = ft[3 * j] * p[0] + ft[3 * j + 1] * p[1] + ft[3 * j + 2] * p[2] + ft[9 + j];
}

struct ForwardArgs {
  uint64_t n;
  const double* p; const uint32_t* fr; const double* views;
  double* x; double* y; double* v;
  unsigned long long* n_invalid;
  ViewCam cam;
};

__global__ __launch_bounds__(256) void k_depth_project(ForwardArgs a) {
#pragma clang fp contract(off)
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i < a.n) {
    const double P[3] = {a.p[3 * i], a.p[3 * i + 1], a.p[3 * i + 2]};
    double q[3] = {P[0], P[1], P[2]};
    if (a.fr) {
      double ft[16];
      lifcal::frame_eval(a.views + 6 * (size_t)a.fr[i], ft);
      transform(ft, P, q);
    }
    double x = 0.0, y = 0.0, v = 0.0;
    bad = !(finite3(P[0], P[1], P[2]) && forward(a.cam, q[0], q[1], q[2], x, y, v));
    if (bad) x = y = v = __builtin_nan("");
    a.x[i] = x; a.y[i] = y; a.v[i] = v;
  }
  const unsigned long long mask = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(a.n_invalid, (unsigned long long)__popcll(mask));
}

// slot j of source s is target s + j - span for j < span, s + j - span + 1 otherwise
LIFCAL_DEV int slot_target(int s, int j, int span) { return s + j - span + (j >= span ? 1 : 0); }

// per (source map, slot): M = R_t R_s^T at [0..8], t_t - M t_s at [9..11]; slots whose target is outside the batch stay untouched
__global__ void k_view_pairs(const double* ftab, int count, int span, double* ptab) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int nslots = 2 * span;
  if (i >= count * nslots) return;
  const int s = i / nslots, t = slot_target(s, i - s * nslots, span);
  if (t < 0 || t >= count) return;
  const double* fs = ftab + 16 * (size_t)s;
  const double* ft = ftab + 16 * (size_t)t;
  double* o = ptab + 12 * (size_t)i;
  for (int a = 0; a < 3; ++a) {
    for (int b = 0; b < 3; ++b) o[3 * a + b] = ft[3 * a] * fs[3 * b] + ft[3 * a + 1] * fs[3 * b + 1] + ft[3 * a + 2] * fs[3 * b + 2];
    o[9 + a] = ft[9 + a] - (o[3 * a] * fs[9] + o[3 * a + 1] * fs[10] + o[3 * a + 2] * fs[11]);
  }
}

// what one workgroup of k_depth_views leaves for one pair slot: the sums over its consistent pixels, and n_valid, n_consistent,
// n_occluded, n_violation
struct ViewPartial { double se, se2; uint32_t n[4]; };

enum ViewClass : int { kNotASource = -1, kNoData = 0, kConsistent = 1, kOccluded = 2, kViolation = 3 };

struct ViewsArgs {
  const uint16_t* maps;     // first pixel of the first map of the batch
  int32_t W, H, count, span;
  uint32_t HW, bpm;         // pixels per map, workgroups per map
  double tol;
  const double* ptab;       // [count][2 span][12]
  const double* ftab;       // [count][16]
  uint8_t* support; uint8_t* conflict;          // [count][HW] or NULL
  lifcal_depth_pair_stats* pair;                // [count][2 span] or NULL, zeroed before the launch
  ViewPartial* slab;                            // [count][2 span][bpm]: every workgroup's part of every pair slot
  uint8_t* flag;                                // fusion: [count][HW], 1 + support of an emitting pixel, else 0
  uint32_t* block_count;                        // fusion: [count][bpm] emitting pixels per workgroup, later their exclusive scan
  uint32_t min_support, max_conflict;
  uint64_t capacity;
  int32_t out_double;
  void* xyz; uint8_t* n_merged; uint32_t* src;
  ViewCam cam;
};

// decode + back_project of the source pixel `pix` of map s; false: invalid
LIFCAL_DEV bool source_pixel(const ViewsArgs& a, int s, uint32_t pix, double& v, double pc[3]) {
#pragma clang fp contract(off)
  double iv;
  if (!decode(a.maps[(size_t)s * a.HW + pix], iv)) return false;
  v = 1.0 / iv;
  const uint32_t row = pix / (uint32_t)a.W, col = pix - row * (uint32_t)a.W;
  const ViewCam& c = a.cam;
  back_project<double>((double)col, (double)row, v, c.spx, c.spy, c.fL, c.bL0, c.B, c.cx, c.cy, c.k0, c.k1, c.p0, c.p1, c.nr, c.tan != 0, pc);
  return true;
}

// One source point against one target map (M: the pair's 12 doubles, wave-uniform).  For a compared pixel: e = 1/v_obs - 1/v_pred,
// the sampled pixel (tx, ty) and its v_obs.
LIFCAL_DEV int classify(const ViewsArgs& a, const double* M, const uint16_t* tmap, const double pc[3], double& e, int& tx, int& ty, double& v_obs) {
#pragma clang fp contract(off)
  double q[3], xt, yt, v_pred;
  transform(M, pc, q);
  if (!forward(a.cam, q[0], q[1], q[2], xt, yt, v_pred)) return kNoData;
  const double fx = xt + 0.5, fy = yt + 0.5;
  if (!(fx > -1.0e9 && fx < 1.0e9 && fy > -1.0e9 && fy < 1.0e9)) return kNoData;
  tx = (int)fx; ty = (int)fy;
  if (tx < 0 || tx >= a.W || ty < 0 || ty >= a.H) return kNoData;
  double iv;
  if (!decode(tmap[(size_t)ty * a.W + tx], iv)) return kNoData;
  v_obs = 1.0 / iv;
  e = 1.0 / v_obs - 1.0 / v_pred;
  if (fabs(e) <= a.tol) return kConsistent;
  return e < -a.tol ? kOccluded : kViolation;
}

// grid (bpm, count): a workgroup holds 256 consecutive pixels (consecutive columns) of ONE source map, so the target slot loop and
// the pair transforms are uniform.  Dynamic LDS: [2 span][4 waves] of {sum_e, sum_e2} then [2 span][4 waves][4] counts.
__global__ __launch_bounds__(256) void k_depth_views(ViewsArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double s_sum[];
  __shared__ uint32_t s_emit[4];
  const int nslots = 2 * a.span;
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_sum + (size_t)nslots * 8);
  const int s = blockIdx.y;
  const uint32_t pix = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  bool valid = false;
  double v = 0.0, pc[3] = {0.0, 0.0, 0.0};
  if (pix < a.HW) valid = source_pixel(a, s, pix, v, pc);
  uint32_t sup = 0, con = 0;
  bool lower = false;
  for (int j = 0; j < nslots; ++j) {
    const int t = slot_target(s, j, a.span);
    if (t < 0 || t >= a.count) continue;
    int cls = kNotASource, tx = 0, ty = 0;
    double e = 0.0, v_obs = 0.0;
    if (valid) cls = classify(a, a.ptab + 12 * ((size_t)s * nslots + j), a.maps + (size_t)t * a.HW, pc, e, tx, ty, v_obs);
    if (cls == kConsistent) { ++sup; if (t < s) lower = true; }
    else if (cls == kViolation) ++con;
    if (a.pair) {
      double se = cls == kConsistent ? e : 0.0, se2 = cls == kConsistent ? e * e : 0.0;
      for (int off = 32; off > 0; off >>= 1) { se += __shfl_xor(se, off); se2 += __shfl_xor(se2, off); }   // a fixed tree
      const unsigned long long m_valid = __ballot(valid), m_con = __ballot(cls == kConsistent), m_occ = __ballot(cls == kOccluded),
                               m_vio = __ballot(cls == kViolation);
      if (lane == 0) {
        double* q = s_sum + ((size_t)j * 4 + wave) * 2;
        q[0] = se; q[1] = se2;
        uint32_t* c = s_cnt + ((size_t)j * 4 + wave) * 4;
        c[0] = (uint32_t)__popcll(m_valid); c[1] = (uint32_t)__popcll(m_con); c[2] = (uint32_t)__popcll(m_occ); c[3] = (uint32_t)__popcll(m_vio);
      }
    }
  }
  if (pix < a.HW) {
    const size_t o = (size_t)s * a.HW + pix;
    if (a.support) a.support[o] = (uint8_t)sup;
    if (a.conflict) a.conflict[o] = (uint8_t)con;
  }
  bool emit = false;
  if (a.flag) {
    emit = valid && sup >= a.min_support && con <= a.max_conflict && !lower;
    if (pix < a.HW) a.flag[(size_t)s * a.HW + pix] = emit ? (uint8_t)(1u + sup) : (uint8_t)0;
    const unsigned long long m_emit = __ballot(emit);
    if (lane == 0) s_emit[wave] = (uint32_t)__popcll(m_emit);
  }
  __syncthreads();
  if (a.flag && threadIdx.x == 0) a.block_count[(size_t)s * a.bpm + blockIdx.x] = s_emit[0] + s_emit[1] + s_emit[2] + s_emit[3];
  if (a.pair) {
    for (int j = (int)threadIdx.x; j < nslots; j += 256) {
      const int t = slot_target(s, j, a.span);
      if (t < 0 || t >= a.count) continue;
      const double* q = s_sum + (size_t)j * 8;
      const uint32_t* c = s_cnt + (size_t)j * 16;
      ViewPartial* out = a.slab + ((size_t)s * nslots + j) * a.bpm + blockIdx.x;
      out->se = ((q[0] + q[2]) + q[4]) + q[6];
      out->se2 = ((q[1] + q[3]) + q[5]) + q[7];
      for (int k = 0; k < 4; ++k) out->n[k] = c[k] + c[4 + k] + c[8 + k] + c[12 + k];
    }
  }
}

// One workgroup per pair slot.  The sums: 256 partials at a time are staged in LDS with coalesced loads and lane 0 adds them one
// after the other, in ascending workgroup order.  The counts are integers: every lane adds what it loaded.  No atomics on HBM:
// a few hundred words that every workgroup of k_depth_views adds to cost more than the kernel's arithmetic.
__global__ __launch_bounds__(256) void k_views_fold(const ViewPartial* slab, int count, int span, uint32_t bpm, lifcal_depth_pair_stats* pair) {
#pragma clang fp contract(off)
  typedef double d2 __attribute__((ext_vector_type(2)));
  __shared__ d2 s_buf[256];
  __shared__ unsigned long long s_n[4];
  const int i = blockIdx.x;
  const int nslots = 2 * span;
  const int s = i / nslots, t = slot_target(s, i - s * nslots, span);
  if (t < 0 || t >= count) return;
  if (threadIdx.x < 4) s_n[threadIdx.x] = 0ull;
  const ViewPartial* q = slab + (size_t)i * bpm;
  double se = 0.0, se2 = 0.0;
  unsigned long long n[4] = {0ull, 0ull, 0ull, 0ull};
  for (uint32_t base = 0; base < bpm; base += 256u) {
    const uint32_t b = base + threadIdx.x;
    if (b < bpm) {
      const ViewPartial p = q[b];
      d2 v; v.x = p.se; v.y = p.se2;
      s_buf[threadIdx.x] = v;
      for (int k = 0; k < 4; ++k) n[k] += p.n[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t m = bpm - base < 256u ? bpm - base : 256u;
#pragma unroll 8
      for (uint32_t k = 0; k < m; ++k) { const d2 v = s_buf[k]; se += v.x; se2 += v.y; }
    }
    __syncthreads();
  }
  for (int k = 0; k < 4; ++k) if (n[k]) atomicAdd(&s_n[k], n[k]);
  __syncthreads();
  if (threadIdx.x == 0) {
    lifcal_depth_pair_stats r;
    r.n_valid = s_n[0]; r.n_compared = s_n[1] + s_n[2] + s_n[3]; r.n_consistent = s_n[1]; r.n_occluded = s_n[2]; r.n_violation = s_n[3];
    r.sum_e = se; r.sum_e2 = se2;
    pair[i] = r;
  }
}

// Exclusive scan of n counts in place, one workgroup of 1024 walking tiles of 4096: four counts per lane (one 16-byte load, the
// next tile's issued before this one is scanned), a shuffle scan per wave, the sixteen wave totals through LDS.  total: the sum.
__global__ __launch_bounds__(1024) void k_views_scan(uint32_t* cnt, uint64_t n, unsigned long long* total) {
  __shared__ uint32_t s_wave[16];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  auto load = [&](uint64_t i0, uint32_t (&c)[4]) {
    c[0] = c[1] = c[2] = c[3] = 0;
    if (i0 + 4 <= n) { const uint4 q = *reinterpret_cast<const uint4*>(cnt + i0); c[0] = q.x; c[1] = q.y; c[2] = q.z; c[3] = q.w; }
    else for (int k = 0; k < 4; ++k) if (i0 + k < n) c[k] = cnt[i0 + k];
  };
  unsigned long long base = 0;   // the same in every lane
  uint32_t nxt[4];
  load(4ull * threadIdx.x, nxt);
  for (uint64_t tile = 0; tile < n; tile += 4096) {
    const uint64_t i0 = tile + 4ull * threadIdx.x;
    const uint32_t c[4] = {nxt[0], nxt[1], nxt[2], nxt[3]};
    load(i0 + 4096, nxt);
    const uint32_t mine = c[0] + c[1] + c[2] + c[3];
    uint32_t incl = mine;
    for (int off = 1; off < 64; off <<= 1) { const uint32_t u = __shfl_up(incl, off); if ((int)lane >= off) incl += u; }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w < 16; ++w) { const uint32_t x = s_wave[w]; if (w < wave) before += x; all += x; }
    __syncthreads();
    unsigned long long run = base + before + (incl - mine);
    for (int k = 0; k < 4; ++k) if (i0 + k < n) { cnt[i0 + k] = (uint32_t)run; run += c[k]; }
    base += all;
  }
  if (threadIdx.x == 0) *total = base;
}

// 1 / (g v^2)^2 with g = dz/dv = -B fL^2 / (b - fL)^2: the inverse variance of z for noise uniform in inverse virtual depth
LIFCAL_DEV double depth_weight(const ViewCam& c, double v) {
#pragma clang fp contract(off)
  const double b = c.bL0 + v * c.B;
  const double d = b - c.fL;
  const double g = -c.B * c.fL * c.fL / (d * d);
  const double gv = g * v * v;
  return 1.0 / (gv * gv);
}

// Same grid as k_depth_views, after the scan: an emitting pixel (flag != 0) writes its src and n_merged at block offset + rank
// within the workgroup.  Ascending src, no cursor.
__global__ __launch_bounds__(256) void k_views_compact(ViewsArgs a) {
  __shared__ uint32_t s_emit[4];
  const int s = blockIdx.y;
  const uint32_t pix = blockIdx.x * 256u + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint8_t flag = pix < a.HW ? a.flag[(size_t)s * a.HW + pix] : (uint8_t)0;
  const unsigned long long m_emit = __ballot(flag != 0);
  if (lane == 0) s_emit[wave] = (uint32_t)__popcll(m_emit);
  __syncthreads();
  if (!flag) return;
  uint64_t idx = a.block_count[(size_t)s * a.bpm + blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) idx += s_emit[w];
  idx += (uint64_t)__popcll(m_emit & ((1ull << lane) - 1ull));
  if (idx >= a.capacity) return;
  a.src[idx] = (uint32_t)((size_t)s * a.HW + pix);
  if (a.n_merged) a.n_merged[idx] = flag;
}

// One lane per emitted point (dense lanes whatever the pattern of the emitting pixels): the pixel is evaluated again against its
// higher targets (a lower one is never consistent with it) and writes sum w p / sum w.
__global__ __launch_bounds__(256) void k_depth_fuse(ViewsArgs a, const unsigned long long* total) {
#pragma clang fp contract(off)
  const int nslots = 2 * a.span;
  const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  const uint64_t n = *total < a.capacity ? *total : a.capacity;
  if (idx >= n) return;
  const uint32_t id = a.src[idx];
  const int s = (int)(id / a.HW);
  const uint32_t pix = id - (uint32_t)s * a.HW;
  double v = 0.0, pc[3], pw[3];
  (void)source_pixel(a, s, pix, v, pc);
  to_world(a.ftab + 16 * (size_t)s, pc, pw);
  const ViewCam& c = a.cam;
  double w = depth_weight(c, v);
  double acc[3] = {w * pw[0], w * pw[1], w * pw[2]}, wsum = w;
  for (int j = a.span; j < nslots; ++j) {
    const int t = slot_target(s, j, a.span);
    if (t >= a.count) break;
    int tx = 0, ty = 0;
    double e = 0.0, v_obs = 0.0;
    if (classify(a, a.ptab + 12 * ((size_t)s * nslots + j), a.maps + (size_t)t * a.HW, pc, e, tx, ty, v_obs) != kConsistent) continue;
    double qc[3], qw[3];
    back_project<double>((double)tx, (double)ty, v_obs, c.spx, c.spy, c.fL, c.bL0, c.B, c.cx, c.cy, c.k0, c.k1, c.p0, c.p1, c.nr, c.tan != 0, qc);
    to_world(a.ftab + 16 * (size_t)t, qc, qw);
    w = depth_weight(c, v_obs);
    acc[0] = acc[0] + w * qw[0]; acc[1] = acc[1] + w * qw[1]; acc[2] = acc[2] + w * qw[2];
    wsum = wsum + w;
  }
  for (int k = 0; k < 3; ++k) {
    const double r = acc[k] / wsum;
    if (a.out_double) ((double*)a.xyz)[3 * idx + k] = r; else ((float*)a.xyz)[3 * idx + k] = (float)r;
  }
}

// what lifcal_depth_check_maps and lifcal_depth_fuse_maps share
struct ViewsInput {
  int32_t first, count; uint32_t span; int32_t out_on_device; uint32_t n_frames;
  const uint32_t* frame; const double* views; double tol_iv;
};

inline int views_validate(const char* who, const lifcal_depth_handle* h, const lifcal_depth_camera* cam, const void* io, const ViewsInput& in) {
  if (!h || !camera_ok(cam) || !io || !in.views || !in.frame || in.span == 0 || in.span > 127u || !(in.tol_iv >= 0.0) || in.count <= 0) {
    g_last_error = std::string(who) + ": bad argument"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
  if (in.first < 0 || (int64_t)in.first + in.count > h->max_maps) { g_last_error = std::string(who) + ": map range exceeds max_maps"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  for (int32_t m = 0; m < in.count; ++m)
    if (in.frame[m] >= in.n_frames) { g_last_error = std::string(who) + ": frame index out of range"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  if ((uint64_t)h->width * h->height * (uint64_t)in.count > 0x7fffff00ull) { g_last_error = std::string(who) + ": more than 2^31 pixels in one call"; return LIFCAL_BA_ERR_INVALID_ARG; }
  return 0;
}

// uploads the poses and fills the frame and pair tables and the fields of `a` every kernel of the two calls reads
inline int views_prepare(const char* who, lifcal_depth_handle* h, const lifcal_depth_camera* cam, const ViewsInput& in, Scratch& s, ViewsArgs& a) {
  const size_t hw = (size_t)h->width * h->height;
  const int nslots = 2 * (int)in.span;
  const double* d_views = nullptr; const uint32_t* d_frame = nullptr; double* ftab = nullptr; double* ptab = nullptr;
  DEPTH_TRY(s.up(&d_views, in.views, 6 * (size_t)in.n_frames), who);
  DEPTH_TRY(s.up(&d_frame, in.frame, (size_t)in.count), who);
  DEPTH_TRY(s.alloc((void**)&ftab, (size_t)in.count * 16 * 8), who);
  DEPTH_TRY(s.alloc((void**)&ptab, (size_t)in.count * nslots * 12 * 8), who);
  hipLaunchKernelGGL(k_depth_frames, dim3((unsigned)((in.count + 63) / 64)), dim3(64), 0, 0, d_views, d_frame, (int)in.count, ftab);
  hipLaunchKernelGGL(k_view_pairs, dim3((unsigned)((in.count * nslots + 63) / 64)), dim3(64), 0, 0, (const double*)ftab, (int)in.count, (int)in.span, ptab);
  DEPTH_TRY(hipGetLastError(), who);
  a.maps = h->maps + hw * in.first;
  a.W = h->width; a.H = h->height; a.count = in.count; a.span = (int32_t)in.span;
  a.HW = (uint32_t)hw; a.bpm = (uint32_t)((hw + 255) / 256);
  a.tol = in.tol_iv;
  a.ptab = ptab; a.ftab = ftab;
  a.cam = view_cam(*cam);
  return 0;
}

inline size_t views_lds(uint32_t span) { return (size_t)2 * span * (4 * 2 * sizeof(double) + 4 * 4 * sizeof(uint32_t)); }

}  // namespace depth

extern "C" {

int lifcal_depth_project_points(int32_t device, const lifcal_depth_camera* cam, lifcal_depth_forward* io) {
  const char* who = "lifcal_depth_project_points";
  if (!depth::camera_ok(cam) || !io || (io->n && (!io->p || !io->x || !io->y || !io->vdepth)) || io->n > 0x7ffffff0ull ||
      ((io->fr != nullptr) != (io->views != nullptr))) {
    g_last_error = std::string(who) + ": bad argument"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
  const uint64_t n = io->n;
  if (io->fr) for (uint64_t i = 0; i < n; ++i) if (io->fr[i] >= io->n_frames) { g_last_error = std::string(who) + ": frame index out of range"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  io->n_invalid = 0;
  if (int rc = mla::select_device(device, who)) return rc;
  if (n == 0) return 0;
  depth::Scratch s;
  depth::ForwardArgs a{};
  a.n = n; a.cam = depth::view_cam(*cam);
  DEPTH_TRY(s.up(&a.p, io->p, 3 * n), who);
  if (io->fr) { DEPTH_TRY(s.up(&a.fr, io->fr, n), who); DEPTH_TRY(s.up(&a.views, io->views, 6 * (size_t)io->n_frames), who); }
  DEPTH_TRY(s.alloc((void**)&a.x, n * 8), who);
  DEPTH_TRY(s.alloc((void**)&a.y, n * 8), who);
  DEPTH_TRY(s.alloc((void**)&a.v, n * 8), who);
  DEPTH_TRY(s.alloc((void**)&a.n_invalid, 8), who);
  DEPTH_TRY(hipMemset(a.n_invalid, 0, 8), who);
  hipLaunchKernelGGL(depth::k_depth_project, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, a);
  DEPTH_TRY(hipGetLastError(), who);
  DEPTH_TRY(hipMemcpy(io->x, a.x, n * 8, hipMemcpyDeviceToHost), who);
  DEPTH_TRY(hipMemcpy(io->y, a.y, n * 8, hipMemcpyDeviceToHost), who);
  DEPTH_TRY(hipMemcpy(io->vdepth, a.v, n * 8, hipMemcpyDeviceToHost), who);
  unsigned long long bad = 0;
  DEPTH_TRY(hipMemcpy(&bad, a.n_invalid, 8, hipMemcpyDeviceToHost), who);
  io->n_invalid = bad;
  return 0;
}

int lifcal_depth_check_maps(lifcal_depth_handle* h, const lifcal_depth_camera* cam, lifcal_depth_views* io) {
  const char* who = "lifcal_depth_check_maps";
  depth::ViewsInput in{};
  if (io) in = depth::ViewsInput{io->first, io->count, io->span, io->out_on_device, io->n_frames, io->frame, io->views, io->tol_iv};
  if (int rc = depth::views_validate(who, h, cam, io, in)) return rc;
  io->seconds = 0.0;
  DEPTH_TRY(hipSetDevice(h->device), who);
  depth::Scratch s;
  depth::ViewsArgs a{};
  if (int rc = depth::views_prepare(who, h, cam, in, s, a)) return rc;
  const size_t npix = (size_t)a.HW * (size_t)in.count, nrows = (size_t)in.count * 2 * in.span;
  if (io->out_on_device) { a.support = io->support; a.conflict = io->conflict; a.pair = io->pair; }
  else {
    if (io->support) DEPTH_TRY(s.alloc((void**)&a.support, npix), who);
    if (io->conflict) DEPTH_TRY(s.alloc((void**)&a.conflict, npix), who);
    if (io->pair) DEPTH_TRY(s.alloc((void**)&a.pair, nrows * sizeof(lifcal_depth_pair_stats)), who);
  }
  if (a.pair) {
    DEPTH_TRY(s.alloc((void**)&a.slab, nrows * a.bpm * sizeof(depth::ViewPartial)), who);
    DEPTH_TRY(hipMemsetAsync(a.pair, 0, nrows * sizeof(lifcal_depth_pair_stats), 0), who);
  }
  DEPTH_TRY(hipEventRecord(h->ev0, 0), who);
  hipLaunchKernelGGL(depth::k_depth_views, dim3(a.bpm, (unsigned)in.count), dim3(256), depth::views_lds(in.span), 0, a);
  if (a.pair) hipLaunchKernelGGL(depth::k_views_fold, dim3((unsigned)nrows), dim3(256), 0, 0, (const depth::ViewPartial*)a.slab, (int)in.count, (int)in.span, a.bpm, a.pair);
  DEPTH_TRY(hipGetLastError(), who);
  DEPTH_TRY(hipEventRecord(h->ev1, 0), who);
  DEPTH_TRY(hipEventSynchronize(h->ev1), who);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
  io->seconds = ms * 1e-3;
  if (!io->out_on_device) {
    if (io->support) DEPTH_TRY(hipMemcpy(io->support, a.support, npix, hipMemcpyDeviceToHost), who);
    if (io->conflict) DEPTH_TRY(hipMemcpy(io->conflict, a.conflict, npix, hipMemcpyDeviceToHost), who);
    if (io->pair) DEPTH_TRY(hipMemcpy(io->pair, a.pair, nrows * sizeof(lifcal_depth_pair_stats), hipMemcpyDeviceToHost), who);
  }
  return 0;
}

int lifcal_depth_fuse_maps(lifcal_depth_handle* h, const lifcal_depth_camera* cam, lifcal_depth_fusion* io) {
  const char* who = "lifcal_depth_fuse_maps";
  depth::ViewsInput in{};
  if (io) in = depth::ViewsInput{io->first, io->count, io->span, io->out_on_device, io->n_frames, io->frame, io->views, io->tol_iv};
  if (int rc = depth::views_validate(who, h, cam, io, in)) return rc;
  if (io->capacity && !io->xyz) { g_last_error = std::string(who) + ": capacity without xyz"; return LIFCAL_BA_ERR_INVALID_ARG; }
  io->seconds = 0.0; io->n_points = 0;
  DEPTH_TRY(hipSetDevice(h->device), who);
  depth::Scratch s;
  depth::ViewsArgs a{};
  if (int rc = depth::views_prepare(who, h, cam, in, s, a)) return rc;
  const size_t npix = (size_t)a.HW * (size_t)in.count, nblocks = (size_t)a.bpm * (size_t)in.count;
  const size_t cap = (size_t)std::min<uint64_t>(io->capacity, npix), osz = io->out_double ? 8 : 4;
  a.min_support = io->min_support; a.max_conflict = io->max_conflict; a.capacity = cap; a.out_double = io->out_double;
  unsigned long long* d_total = nullptr;
  DEPTH_TRY(s.alloc((void**)&a.flag, npix), who);
  DEPTH_TRY(s.alloc((void**)&a.block_count, nblocks * sizeof(uint32_t)), who);
  DEPTH_TRY(s.alloc((void**)&d_total, 8), who);
  if (io->out_on_device) { a.xyz = io->xyz; a.n_merged = io->n_merged; a.src = io->src; }
  else if (cap) {
    DEPTH_TRY(s.alloc(&a.xyz, cap * 3 * osz), who);
    if (io->n_merged) DEPTH_TRY(s.alloc((void**)&a.n_merged, cap), who);
    if (io->src) DEPTH_TRY(s.alloc((void**)&a.src, cap * sizeof(uint32_t)), who);
  }
  if (cap && !a.src) DEPTH_TRY(s.alloc((void**)&a.src, cap * sizeof(uint32_t)), who);   // the fusion kernel reads it
  DEPTH_TRY(hipEventRecord(h->ev0, 0), who);
  hipLaunchKernelGGL(depth::k_depth_views, dim3(a.bpm, (unsigned)in.count), dim3(256), depth::views_lds(in.span), 0, a);
  hipLaunchKernelGGL(depth::k_views_scan, dim3(1), dim3(1024), 0, 0, a.block_count, (uint64_t)nblocks, d_total);
  if (cap) {
    hipLaunchKernelGGL(depth::k_views_compact, dim3(a.bpm, (unsigned)in.count), dim3(256), 0, 0, a);
    hipLaunchKernelGGL(depth::k_depth_fuse, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, 0, a, (const unsigned long long*)d_total);
  }
  DEPTH_TRY(hipGetLastError(), who);
  DEPTH_TRY(hipEventRecord(h->ev1, 0), who);
  DEPTH_TRY(hipEventSynchronize(h->ev1), who);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
  io->seconds = ms * 1e-3;
  unsigned long long total = 0;
  DEPTH_TRY(hipMemcpy(&total, d_total, 8, hipMemcpyDeviceToHost), who);
  io->n_points = total;
  const size_t nw = (size_t)std::min<uint64_t>(total, cap);
  if (!io->out_on_device && nw) {
    DEPTH_TRY(hipMemcpy(io->xyz, a.xyz, nw * 3 * osz, hipMemcpyDeviceToHost), who);
    if (io->n_merged) DEPTH_TRY(hipMemcpy(io->n_merged, a.n_merged, nw, hipMemcpyDeviceToHost), who);
    if (io->src) DEPTH_TRY(hipMemcpy(io->src, a.src, nw * sizeof(uint32_t), hipMemcpyDeviceToHost), who);
  }
  return 0;
}

}  // extern "C"
