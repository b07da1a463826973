// depth_map.hip — the virtual-image depth map from the raw-pixel depth (include/lifcal_depthmap.h), in a code
// object of its own like raw_depth.hip (raw_depth.hpp says why).
//
// What runs where: the host checks the arguments; the device does everything per sample and per cell.  k_depthmap_flag marks the
// samples and hipcub compacts their pixel indices in ascending order; k_depthmap_scatter<1> takes the minimum q per cell of every
// footprint (32-bit atomicMin), k_depthmap_scatter<2> adds the samples of the front cluster (one 64-bit integer atomicAdd per
// cell); k_depthmap_resolve, k_depthmap_fill (ping-pong) and k_depthmap_encode work per cell.  Nothing that is accumulated is a
// float, so the bytes do not depend on the order of the atomics.
#include "raw_depth.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/lifcal_ba.h"
#include "../../include/lifcal_depthmap.h"

namespace lifcal {
namespace depthmap {

constexpr int kThreads = 256;
constexpr int kGroup = 16;                    // lanes that stride one sample's footprint
constexpr double kQ = 1048576.0;              // 2^20
constexpr uint32_t kNoValue = 0xffffffffu;    // front without a sample, q of a cell without a value
constexpr uint32_t kNaN = 0x7fc00000u;
constexpr int kCountShift = 24;               // pass 2 packs (q - front) << 24 | 1
constexpr int kMaxFillRounds = 64;

// ------------------------------------------------------------------------------------------------ device side

struct Args {
  int32_t W, ow, oh;
  uint32_t tq;
  double scale, iv_min;
  const float* cx; const float* cy; const int32_t* map_ml;
  const float* inv_depth;
  const uint32_t* src;          // sample -> pixel index, ascending
  const uint32_t* n_samples;
  uint32_t* front;              // [oh][ow]
  unsigned long long* acc;      // [oh][ow]
};

__global__ __launch_bounds__(kThreads) void k_depthmap_flag(int64_t npix, const float* __restrict__ inv_depth, const int32_t* __restrict__ map_ml, double iv_min,
                                                            uint8_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= npix) return;
  const double iv = (double)inv_depth[i];
  flag[i] = (map_ml[i] >= 0 && iv >= iv_min && iv <= 1.0) ? 1 : 0;   // false for NaN
}

// Every lane derives the footprint of one sample; then the wave's four groups of 16 lanes take the wave's 64 samples four at a
// time, a group striding one footprint row-major, so that the atomics of a group fall on runs of adjacent cells.
template <int PASS>
__global__ __launch_bounds__(kThreads) void k_depthmap_scatter(Args a) {
#pragma clang fp contract(off)
  const uint32_t n = *a.n_samples;
  const uint32_t base = blockIdx.x * (uint32_t)kThreads;
  if (base >= n) return;                                  // the whole workgroup leaves
  const uint32_t i = base + threadIdx.x;
  int x0 = 0, y0 = 0, fw = 1, cells = 0;
  uint32_t q = 0;
  if (i < n) {
    const uint32_t p = a.src[i];
    const int32_t l = a.map_ml[p];
    const double iv = (double)a.inv_depth[p];
    const double v = 1.0 / iv;
    const double px = (double)(p % (uint32_t)a.W), py = (double)(p / (uint32_t)a.W);
    const double lcx = (double)a.cx[l], lcy = (double)a.cy[l];
    const double xu = lcx + v * (px - lcx), yu = lcy + v * (py - lcy);
    const double x = (xu + 0.5) / a.scale - 0.5, y = (yu + 0.5) / a.scale - 0.5;
    const double h = (0.5 * v) / a.scale;
    const double X0 = ceil(x - h), X1 = ceil(x + h) - 1.0, Y0 = ceil(y - h), Y1 = ceil(y + h) - 1.0;
    const double xm = (double)(a.ow - 1), ym = (double)(a.oh - 1);
    if (X0 <= X1 && Y0 <= Y1 && X0 <= xm && X1 >= 0.0 && Y0 <= ym && Y1 >= 0.0) {   // false for a NaN
      x0 = (int)fmax(X0, 0.0); y0 = (int)fmax(Y0, 0.0);
      const int x1 = (int)fmin(X1, xm), y1 = (int)fmin(Y1, ym);
      fw = x1 - x0 + 1;
      cells = fw * (y1 - y0 + 1);
    }
    q = (uint32_t)floor(iv * kQ + 0.5);
  }
  const int lane = threadIdx.x & 63;
  const int first = lane & ~(kGroup - 1), sub = lane & (kGroup - 1);
  for (int j = 0; j < kGroup; ++j) {
    const int from = first + j;
    const int sx0 = __shfl(x0, from), sy0 = __shfl(y0, from), sfw = __shfl(fw, from), scells = __shfl(cells, from);
    const uint32_t sq = (uint32_t)__shfl((int)q, from);
    for (int t = sub; t < scells; t += kGroup) {
      const int r = t / sfw, c = t - r * sfw;
      const size_t cell = (size_t)(sy0 + r) * (size_t)a.ow + (size_t)(sx0 + c);
      if (PASS == 1) {
        atomicMin(&a.front[cell], sq);
      } else {
        const uint32_t f = a.front[cell];
        if (sq <= f + a.tq) atomicAdd(&a.acc[cell], ((unsigned long long)(sq - f) << kCountShift) + 1ull);
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_depthmap_resolve(int64_t ncell, int min_support, const uint32_t* __restrict__ front, const unsigned long long* __restrict__ acc,
                                                               uint32_t* __restrict__ qmap, uint8_t* __restrict__ status, uint16_t* __restrict__ support) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= ncell) return;
  const uint32_t f = front[i];
  uint32_t q = kNoValue, sup = 0;
  int st = LIFCAL_DEPTHMAP_EMPTY;
  if (f != kNoValue) {
    const unsigned long long w = acc[i];
    const unsigned long long n = w & ((1ull << kCountShift) - 1ull);
    const unsigned long long sum = n * (unsigned long long)f + (w >> kCountShift);
    sup = n > 65535ull ? 65535u : (uint32_t)n;
    if (n < (unsigned long long)min_support) {
      st = LIFCAL_DEPTHMAP_REJECTED;
    } else {
      st = LIFCAL_DEPTHMAP_MEASURED;
      q = (uint32_t)((2ull * sum + n) / (2ull * n));
    }
  }
  qmap[i] = q;
  status[i] = (uint8_t)st;
  support[i] = (uint16_t)sup;
}

// one Jacobi round: reads (q_in, st_in), writes (q_out, st_out) for every cell
__global__ __launch_bounds__(kThreads) void k_depthmap_fill(int ow, int oh, uint32_t tq, int min_nb, const uint32_t* __restrict__ q_in, const uint8_t* __restrict__ st_in,
                                                            uint32_t* __restrict__ q_out, uint8_t* __restrict__ st_out, uint16_t* __restrict__ support) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (int64_t)ow * oh) return;
  uint32_t q = q_in[i];
  int st = st_in[i];
  if (st >= LIFCAL_DEPTHMAP_EMPTY) {
    const int y = (int)(i / ow), x = (int)(i - (int64_t)y * ow);
    uint32_t nb[8];
    uint32_t qmin = kNoValue;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int dy = (k < 3) ? -1 : (k < 5 ? 0 : 1);
      const int dx = (k < 3) ? k - 1 : (k == 3 ? -1 : (k == 4 ? 1 : k - 6));
      const int yy = y + dy, xx = x + dx;
      uint32_t v = kNoValue;
      if (yy >= 0 && yy < oh && xx >= 0 && xx < ow) v = q_in[(int64_t)yy * ow + xx];
      nb[k] = v;
      qmin = v < qmin ? v : qmin;
    }
    if (qmin != kNoValue) {
      const unsigned long long lim = (unsigned long long)qmin + tq;
      unsigned long long S = 0, c = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k)
        if (nb[k] != kNoValue && (unsigned long long)nb[k] <= lim) { S += nb[k]; ++c; }
      if (c >= (unsigned long long)min_nb) {
        q = (uint32_t)((2ull * S + c) / (2ull * c));
        st = LIFCAL_DEPTHMAP_FILLED;
        support[i] = 0;
      }
    }
  }
  q_out[i] = q;
  st_out[i] = (uint8_t)st;
}

__global__ __launch_bounds__(kThreads) void k_depthmap_encode(int64_t ncell, const uint32_t* __restrict__ qmap, const uint8_t* __restrict__ st_in, const uint16_t* __restrict__ sup_in,
                                                              float* __restrict__ inv_depth, uint16_t* __restrict__ depth16, uint8_t* __restrict__ status,
                                                              uint16_t* __restrict__ support, unsigned long long* __restrict__ count) {
#pragma clang fp contract(off)
  __shared__ unsigned s_count[4];
  if (threadIdx.x < 4) s_count[threadIdx.x] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < ncell) {
    const uint32_t q = qmap[i];
    const int st = st_in[i];
    float iv = __uint_as_float(kNaN);
    uint32_t d16 = 0;
    if (q != kNoValue) {
      const double r = (double)q / kQ;
      iv = (float)r;
      const double value = floor(65535.0 * (1.0 - r) + 0.5);
      const uint32_t val = (uint32_t)value;
      double back = (double)val / 65535.0;      // the direct rule of lifcal_depth_sample
      back = 1.0 - back;
      if (val > 0u && val <= 65535u && back <= 0.5 && back > 0.0) d16 = val;
    }
    if (inv_depth) inv_depth[i] = iv;
    if (depth16) depth16[i] = (uint16_t)d16;
    if (status) status[i] = (uint8_t)st;
    if (support) support[i] = sup_in[i];
    atomicAdd(&s_count[st & 3], 1u);
  }
  __syncthreads();
  if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(&count[threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

// ------------------------------------------------------------------------------------------------ host side

static int fail(int code, const std::string& text) { set_last_error(text.c_str()); return code; }
static int fail_hip(const char* who, hipError_t e) { return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }

struct Plan {
  lifcal_depthmap_options opt;   // defaults resolved
  int32_t tq = 0, max_side = 0;
  int64_t max_samples = 0;
};

// the options against the grid's parameters.  No device.
static int make_plan(const char* who, const lifcal_mla_params* p, int32_t width, int32_t height, const lifcal_depthmap_options* o, Plan* t) {
#pragma clang fp contract(off)
  const std::string w = std::string(who) + ": ";
  if (!p || p->width <= 0 || p->height <= 0 || !(p->lens_diameter > 2.0f) || !(p->lens_diameter < 1.0e4f))
    return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "bad grid parameters");
  if (width != p->width || height != p->height) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "raw depth size differs from the grid's");
  lifcal_depthmap_options q{};
  if (o) q = *o;
  if (q.scale == 0) q.scale = 1;
  if (q.min_support == 0) q.min_support = 2;
  if (q.fill_rounds == 0) q.fill_rounds = 2;
  if (q.fill_min_neighbours == 0) q.fill_min_neighbours = 3;
  if (q.tol_iv == 0.0) q.tol_iv = 0.02;
  if (q.iv_min == 0.0) q.iv_min = 0.04;
  if (q.scale < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "scale must be at least 1");
  if (q.out_width < 0 || q.out_height < 0) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "out_width and out_height must not be negative");
  if (q.out_width == 0) q.out_width = width / q.scale;
  if (q.out_height == 0) q.out_height = height / q.scale;
  if (q.out_width < 1 || q.out_height < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "the output has no cells (scale above the image size)");
  if (q.min_support < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_support must be at least 1");
  if (q.fill_rounds > kMaxFillRounds) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "fill_rounds above 64");
  if (q.fill_min_neighbours < 1 || q.fill_min_neighbours > 8) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "fill_min_neighbours outside 1 .. 8");
  if (!(q.tol_iv > 0.0) || !(q.tol_iv <= 0.5)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "need 0 < tol_iv <= 0.5");
  if (!(q.iv_min >= 1.0e-3) || !(q.iv_min <= 1.0)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "need 0.001 <= iv_min <= 1");
  t->opt = q;
  t->tq = (int32_t)std::floor(q.tol_iv * kQ + 0.5);
  t->max_side = (int32_t)std::floor(1.0 / (q.iv_min * (double)q.scale)) + 1;
  if ((int64_t)width * height >= (1ll << 31) || (int64_t)q.out_width * q.out_height >= (1ll << 31))
    return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "2^31 raw pixels or cells and more are not supported");
  // the samples that can reach one cell (include/lifcal_depthmap.h): pass 2 keeps their count in 24 bits and sum (q - front) in 40
  const double d = (double)p->lens_diameter;
  const double valid_r = (double)(p->lens_diameter * 0.5f - 1.0f);
  const double reach = std::ceil((valid_r + 0.5) / q.iv_min + (double)q.scale + 0.5 * d);
  const double side = 2.0 * reach + 1.0;
  t->max_samples = (int64_t)std::min((double)width * (double)height, side * side);
  if (t->max_samples >= (1ll << kCountShift) || (double)t->max_samples * (double)t->tq >= 1099511627776.0)
    return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "up to " + std::to_string(t->max_samples) + " samples can reach one cell: beyond the 24-bit count or the 40-bit sum of pass 2");
  return 0;
}

struct DeviceBuffers {
  std::vector<void*> q;
  hipEvent_t ev[2] = {nullptr, nullptr};
  ~DeviceBuffers() {
    for (void* p : q) (void)hipFree(p);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
  template <class T>
  hipError_t alloc(T** out, size_t bytes) {
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, std::max<size_t>(bytes, 8));
    if (e == hipSuccess) q.push_back(p);
    *out = (T*)p;
    return e;
  }
};

}  // namespace depthmap
}  // namespace lifcal

extern "C" {

using namespace lifcal::depthmap;

int lifcal_depthmap_check(const lifcal_mla_params* grid_params, int32_t width, int32_t height, const lifcal_depthmap_options* options,
                          lifcal_depthmap_plan* plan) {
  Plan t;
  if (int rc = make_plan("lifcal_depthmap_check", grid_params, width, height, options, &t)) return rc;
  if (plan) {
    plan->options = t.opt;
    plan->out_width = t.opt.out_width;
    plan->out_height = t.opt.out_height;
    plan->tq = t.tq;
    plan->max_side = t.max_side;
    plan->max_samples_per_cell = t.max_samples;
  }
  return 0;
}

int lifcal_depthmap_from_raw(lifcal_mla_handle* grid, const float* inv_depth, int32_t on_device, const lifcal_depthmap_options* options,
                             lifcal_depthmap_result* out) {
  const char* who = "lifcal_depthmap_from_raw";
  lifcal::MlaView g;
  if (!lifcal::mla_view(grid, &g) || !out) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no grid or no result");
  if (!inv_depth) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no raw depth");
  Plan t;
  if (int rc = make_plan(who, &g.prm, g.prm.width, g.prm.height, options, &t)) return rc;
  out->seconds = 0.0;
  out->n_samples = 0;
  for (uint64_t& c : out->count) c = 0;
  if (hipSetDevice(g.device) != hipSuccess) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");

  const int W = g.prm.width, H = g.prm.height, ow = t.opt.out_width, oh = t.opt.out_height;
  const size_t npix = (size_t)W * H, ncell = (size_t)ow * oh;
  DeviceBuffers buf;
  Args a{};
  a.W = W; a.ow = ow; a.oh = oh; a.tq = (uint32_t)t.tq;
  a.scale = (double)t.opt.scale; a.iv_min = t.opt.iv_min;
  a.cx = g.cx; a.cy = g.cy; a.map_ml = g.map_ml;
  hipError_t e = hipSuccess;
  a.inv_depth = inv_depth;
  if (!on_device) {
    float* q = nullptr;
    e = buf.alloc(&q, npix * 4);
    if (e == hipSuccess) e = hipMemcpy(q, inv_depth, npix * 4, hipMemcpyHostToDevice);
    a.inv_depth = q;
  }
  uint8_t* flag = nullptr; uint32_t* src = nullptr; uint32_t* d_n = nullptr; void* scratch = nullptr; size_t scratch_bytes = 0;
  uint32_t* qmap[2] = {nullptr, nullptr}; uint8_t* st[2] = {nullptr, nullptr}; uint16_t* sup = nullptr; unsigned long long* count = nullptr;
  float* o_iv = nullptr; uint16_t* o_d16 = nullptr; uint8_t* o_st = nullptr; uint16_t* o_sup = nullptr;
  if (e == hipSuccess) e = buf.alloc(&flag, npix);
  if (e == hipSuccess) e = buf.alloc(&src, npix * 4);
  if (e == hipSuccess) e = buf.alloc(&d_n, 4);
  if (e == hipSuccess) e = buf.alloc(&a.front, ncell * 4);
  if (e == hipSuccess) e = buf.alloc(&a.acc, ncell * 8);
  for (int k = 0; k < 2; ++k) {
    if (e == hipSuccess) e = buf.alloc(&qmap[k], ncell * 4);
    if (e == hipSuccess) e = buf.alloc(&st[k], ncell);
  }
  if (e == hipSuccess) e = buf.alloc(&sup, ncell * 2);
  if (e == hipSuccess) e = buf.alloc(&count, 4 * sizeof(unsigned long long));
  if (out->out_on_device) {
    o_iv = out->inv_depth; o_d16 = out->depth16; o_st = out->status; o_sup = out->support;
  } else {
    if (e == hipSuccess && out->inv_depth) e = buf.alloc(&o_iv, ncell * 4);
    if (e == hipSuccess && out->depth16) e = buf.alloc(&o_d16, ncell * 2);
    if (e == hipSuccess && out->status) e = buf.alloc(&o_st, ncell);
    if (e == hipSuccess && out->support) e = buf.alloc(&o_sup, ncell * 2);
  }
  hipcub::CountingInputIterator<uint32_t> ids(0u);
  if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged(nullptr, scratch_bytes, ids, flag, src, d_n, (int)npix);
  if (e == hipSuccess) e = buf.alloc(&scratch, scratch_bytes);
  if (e == hipSuccess) e = hipEventCreate(&buf.ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&buf.ev[1]);
  if (e != hipSuccess) return fail_hip(who, e);
  a.src = src; a.n_samples = d_n;

  const dim3 blk(kThreads), grd_pix((unsigned)((npix + kThreads - 1) / kThreads)), grd_cell((unsigned)((ncell + kThreads - 1) / kThreads));
  e = hipEventRecord(buf.ev[0], 0);
  if (e == hipSuccess) e = hipMemsetAsync(a.front, 0xff, ncell * 4, 0);
  if (e == hipSuccess) e = hipMemsetAsync(a.acc, 0, ncell * 8, 0);
  if (e == hipSuccess) e = hipMemsetAsync(count, 0, 4 * sizeof(unsigned long long), 0);
  if (e != hipSuccess) return fail_hip(who, e);
  hipLaunchKernelGGL(k_depthmap_flag, grd_pix, blk, 0, 0, (int64_t)npix, a.inv_depth, g.map_ml, a.iv_min, flag);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged(scratch, scratch_bytes, ids, flag, src, d_n, (int)npix);
  if (e != hipSuccess) return fail_hip(who, e);
  // one lane per sample slot; the workgroups past n_samples leave at once, so the count never travels to the host in between
  hipLaunchKernelGGL(k_depthmap_scatter<1>, grd_pix, blk, 0, 0, a);
  hipLaunchKernelGGL(k_depthmap_scatter<2>, grd_pix, blk, 0, 0, a);
  hipLaunchKernelGGL(k_depthmap_resolve, grd_cell, blk, 0, 0, (int64_t)ncell, t.opt.min_support, a.front, a.acc, qmap[0], st[0], sup);
  int cur = 0;
  for (int r = 0; r < t.opt.fill_rounds; ++r) {
    hipLaunchKernelGGL(k_depthmap_fill, grd_cell, blk, 0, 0, ow, oh, a.tq, t.opt.fill_min_neighbours, qmap[cur], st[cur], qmap[cur ^ 1], st[cur ^ 1], sup);
    cur ^= 1;
  }
  hipLaunchKernelGGL(k_depthmap_encode, grd_cell, blk, 0, 0, (int64_t)ncell, qmap[cur], st[cur], sup, o_iv, o_d16, o_st, o_sup, count);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(buf.ev[1], 0);
  if (e == hipSuccess) e = hipEventSynchronize(buf.ev[1]);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, buf.ev[0], buf.ev[1]);
  unsigned long long cnt[4] = {0, 0, 0, 0};
  uint32_t n = 0;
  if (e == hipSuccess) e = hipMemcpy(cnt, count, sizeof(cnt), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(&n, d_n, 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && !out->out_on_device) {
    if (out->inv_depth) e = hipMemcpy(out->inv_depth, o_iv, ncell * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out->depth16) e = hipMemcpy(out->depth16, o_d16, ncell * 2, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out->status) e = hipMemcpy(out->status, o_st, ncell, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out->support) e = hipMemcpy(out->support, o_sup, ncell * 2, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return fail_hip(who, e);
  for (int i = 0; i < 4; ++i) out->count[i] = cnt[i];
  out->n_samples = n;
  out->seconds = 1.0e-3 * (double)ms;
  return 0;
}

}  // extern "C"
