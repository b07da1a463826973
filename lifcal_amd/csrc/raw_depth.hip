// raw_depth.hip — virtual depth from the raw image (include/lifcal_rawdepth.h), in a code object of its own
// (raw_depth.hpp says why).
//
// What runs where: the host builds the tables (hypotheses, lattice vectors to the neighbours, shifts in 1/64 pixel; a few
// thousand numbers) and checks the arguments; the device does everything per pixel.  k_rawdepth_fill writes the "no lens"
// record to every pixel; k_rawdepth_lens, one workgroup per lens, copies the lens's neighbourhood to LDS once, lists the pixels
// of the lens that can have an estimate, and then each lane sweeps the hypotheses for its pixels with the selection state in
// registers: no cost volume exists anywhere.  All image arithmetic is integer and every floating-point step is an IEEE double
// operation without fused multiply-add, so the bytes are the same on every run and equal to the numpy restatement's.
#include "raw_depth.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lifcal_ba.h"
#include "../../include/lifcal_rawdepth.h"

namespace lifcal {
namespace rawdepth {

// ------------------------------------------------------------------------------------------------ device side

struct Args {
  int32_t W, H, n_sub0;
  int32_t K, N, min_neighbours, min_contrast;
  int32_t rb, half;            // a lens's pixels lie within rb of its centre pixel, everything read for them within half
  double r0sq, r1sq;           // (valid_r - w)^2 and (valid_r - w - 1)^2; r1sq < 0: no pair counts
  double step, ratio, cost_scale;
  const float* cx; const float* cy; const int32_t* map_ml;
  const void* img; int64_t pitch;
  const double* iv;            // [K]
  const double* delta;         // [2][N][2]
  const int32_t* shift;        // [2][K][N][2], 1/64 pixel
  float* inv_depth; float* cost; uint8_t* status; uint8_t* nn;
  unsigned long long* count;   // [5]; entry 1 is set by the host
};

constexpr uint32_t kNaN = 0x7fc00000u;

__global__ __launch_bounds__(kThreads) void k_rawdepth_fill(int64_t npix, float* inv_depth, float* cost, uint8_t* status, uint8_t* nn) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= npix) return;
  if (inv_depth) inv_depth[i] = __uint_as_float(kNaN);
  if (cost) cost[i] = __uint_as_float(kNaN);
  if (status) status[i] = LIFCAL_RAWDEPTH_NO_LENS;
  if (nn) nn[i] = 0;
}

// Sum over the (2 WR + 1)^2 patch of |own - bilinear sample| for one (neighbour, hypothesis) pair.  `r` points at the top-left
// raw value of the shifted patch in the LDS window; the weights are the same for the whole patch, so a row of horizontal
// interpolants is formed from 2 WR + 2 reads and shared by the two patch rows it touches: (2 WR + 2)^2 LDS reads per pair.
// Exact in 32 bits: a sample is at most 4096 * 65535 < 2^31 and a row of five differences stays below 2^32.
template <int WR>
__device__ __forceinline__ uint64_t patch_cost(const uint16_t* __restrict__ r, int side, const int32_t* own, uint32_t fx, uint32_t fy) {
  constexpr int P = 2 * WR + 1;
  const uint32_t wx1 = fx, wx0 = 64u - fx, wy1 = fy, wy0 = 64u - fy;
  uint32_t hp[P], hc[P];
  uint64_t total = 0;
#pragma unroll
  for (int row = 0; row <= P; ++row) {
    uint32_t v[P + 1];
#pragma unroll
    for (int j = 0; j <= P; ++j) v[j] = r[row * side + j];
#pragma unroll
    for (int j = 0; j < P; ++j) hc[j] = wx0 * v[j] + wx1 * v[j + 1];
    if (row > 0) {
      uint32_t acc = 0;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const int32_t b = (int32_t)(wy0 * hp[j] + wy1 * hc[j]);
        const int32_t df = own[(row - 1) * P + j] - b;
        acc += (uint32_t)(df < 0 ? -df : df);
      }
      total += acc;
    }
#pragma unroll
    for (int j = 0; j < P; ++j) hp[j] = hc[j];
  }
  return total;
}

template <class T, int WR>
__global__ __launch_bounds__(kThreads) void k_rawdepth_lens(Args a) {
#pragma clang fp contract(off)
  constexpr int P = 2 * WR + 1;
  extern __shared__ uint16_t s_mem[];
  using Scan = hipcub::BlockScan<int, kThreads>;
  __shared__ typename Scan::TempStorage s_scan;
  __shared__ unsigned s_count[5];
  const int tid = threadIdx.x;
  const int lens = blockIdx.x;
  const double lcx = (double)a.cx[lens], lcy = (double)a.cy[lens];
  const double fcx = floor(lcx + 0.5), fcy = floor(lcy + 0.5);
  if (!(fcx > -1.0e9 && fcx < 1.0e9 && fcy > -1.0e9 && fcy < 1.0e9)) return;   // the whole workgroup leaves
  const int pcx = (int)fcx, pcy = (int)fcy;
  if (pcx + a.rb < 0 || pcx - a.rb >= a.W || pcy + a.rb < 0 || pcy - a.rb >= a.H) return;
  const int side = 2 * a.half + 1, bs = 2 * a.rb + 1;
  uint16_t* s_win = s_mem;
  uint16_t* s_list = s_mem + ((side * side + 1) & ~1);
  const int wx0 = pcx - a.half, wy0 = pcy - a.half;
  const T* __restrict__ img = (const T*)a.img;
  if (tid < 5) s_count[tid] = 0;
  // the neighbourhood, zero outside the image (no pair that counts reads there)
  for (int i = tid; i < side * side; i += kThreads) {
    const int ly = i / side, lx = i - ly * side;
    const int gx = wx0 + lx, gy = wy0 + ly;
    uint16_t v = 0;
    if (gx >= 0 && gx < a.W && gy >= 0 && gy < a.H) v = (uint16_t)img[(int64_t)gy * a.pitch + gx];
    s_win[i] = v;
  }
  // the pixels of this lens that are not status 1, in ascending order of their index in the bounding box
  int n_list = 0;
  for (int base = 0; base < bs * bs; base += kThreads) {
    const int i = base + tid;
    int active = 0;
    if (i < bs * bs) {
      const int by = i / bs, bx = i - by * bs;
      const int px = pcx - a.rb + bx, py = pcy - a.rb + by;
      if (px >= WR && px <= a.W - 1 - WR && py >= WR && py <= a.H - 1 - WR && a.map_ml[(int64_t)py * a.W + px] == lens) {
        const double ox = (double)px - lcx, oy = (double)py - lcy;
        active = (ox * ox + oy * oy > a.r0sq) ? 0 : 1;
      }
    }
    int pos = 0, total = 0;
    Scan(s_scan).ExclusiveSum(active, pos, total);
    if (active) s_list[n_list + pos] = (uint16_t)i;
    n_list += total;
    __syncthreads();
  }
  __syncthreads();

  const int sub = lens < a.n_sub0 ? 0 : 1;
  const double* __restrict__ delta = a.delta + (size_t)sub * a.N * 2;
  const int32_t* __restrict__ shift = a.shift + (size_t)sub * a.K * a.N * 2;
  const double inf = __builtin_huge_val();
  for (int it = tid; it < n_list; it += kThreads) {
    const int i = s_list[it];
    const int by = i / bs, bx = i - by * bs;
    const int px = pcx - a.rb + bx, py = pcy - a.rb + by;
    const int lx = px - wx0, ly = py - wy0;
    const int64_t gidx = (int64_t)py * a.W + px;
    int32_t own[P * P];
    int32_t mn = 0x7fffffff, mx = -1;
#pragma unroll
    for (int r = 0; r < P; ++r)
#pragma unroll
      for (int c = 0; c < P; ++c) {
        const int32_t v = s_win[(ly - WR + r) * side + (lx - WR + c)];
        mn = v < mn ? v : mn; mx = v > mx ? v : mx;
        own[r * P + c] = 4096 * v;
      }
    int st = LIFCAL_RAWDEPTH_OK;
    float out_iv = __uint_as_float(kNaN), out_cost = __uint_as_float(kNaN);
    int out_nn = 0;
    if (mx - mn < a.min_contrast) {
      st = LIFCAL_RAWDEPTH_FLAT;
    } else {
      const double ox = (double)px - lcx, oy = (double)py - lcy;
      // the four smallest local minima so far, by (cost, k); for the smallest also its neighbours' costs and its pair count
      double t0c = inf, t1c = inf, t2c = inf, t3c = inf, bm = inf, bp = inf;
      int t0k = -1, t1k = -1, t2k = -1, t3k = -1, bn = 0;
      double prev2 = inf, prev = inf;
      int nprev = 0;
      for (int k = 0; k <= a.K; ++k) {
        double cur = inf;
        int ncur = 0;
        if (k < a.K) {
          const double ivk = a.iv[k];
          uint64_t sum = 0;
          for (int n = 0; n < a.N; ++n) {
            const double tx = ox - delta[2 * n] * ivk, ty = oy - delta[2 * n + 1] * ivk;
            if (!(tx * tx + ty * ty <= a.r1sq)) continue;
            const int32_t sx = shift[((size_t)k * a.N + n) * 2], sy = shift[((size_t)k * a.N + n) * 2 + 1];
            const int ix = sx >> 6, iy = sy >> 6;
            if (px - WR + ix < 0 || px + WR + ix + 1 > a.W - 1 || py - WR + iy < 0 || py + WR + iy + 1 > a.H - 1) continue;
            sum += patch_cost<WR>(s_win + (ly - WR + iy) * side + (lx - WR + ix), side, own, (uint32_t)(sx & 63), (uint32_t)(sy & 63));
            ++ncur;
          }
          if (ncur >= a.min_neighbours) cur = (double)sum / (double)ncur;
        }
        // is k - 1 a local minimum?
        if (prev < inf && prev < prev2 && prev <= cur) {
          const int km = k - 1;
          if (prev < t0c) { t3c = t2c; t3k = t2k; t2c = t1c; t2k = t1k; t1c = t0c; t1k = t0k; t0c = prev; t0k = km; bm = prev2; bp = cur; bn = nprev; }
          else if (prev < t1c) { t3c = t2c; t3k = t2k; t2c = t1c; t2k = t1k; t1c = prev; t1k = km; }
          else if (prev < t2c) { t3c = t2c; t3k = t2k; t2c = prev; t2k = km; }
          else if (prev < t3c) { t3c = prev; t3k = km; }
        }
        prev2 = prev; prev = cur; nprev = ncur;
      }
      const double den = (bm - 2.0 * t0c) + bp;
      if (t0k <= 0 || t0k == a.K - 1 || !(bm < inf) || !(bp < inf) || !(den > 0.0)) {
        st = LIFCAL_RAWDEPTH_NO_MINIMUM;
      } else {
        const double thr = a.ratio * t0c;
        const bool amb = (t1k >= 0 && abs(t1k - t0k) >= 3 && t1c < thr) || (t2k >= 0 && abs(t2k - t0k) >= 3 && t2c < thr) ||
                         (t3k >= 0 && abs(t3k - t0k) >= 3 && t3c < thr);
        st = amb ? LIFCAL_RAWDEPTH_AMBIGUOUS : LIFCAL_RAWDEPTH_OK;
        if (!amb) out_iv = (float)(a.iv[t0k] + ((0.5 * (bm - bp)) / den) * a.step);
        out_cost = (float)(t0c / a.cost_scale);
        out_nn = bn;
      }
    }
    if (a.inv_depth) a.inv_depth[gidx] = out_iv;
    if (a.cost) a.cost[gidx] = out_cost;
    if (a.status) a.status[gidx] = (uint8_t)st;
    if (a.nn) a.nn[gidx] = (uint8_t)out_nn;
    atomicAdd(&s_count[st], 1u);
  }
  __syncthreads();
  if (tid < 5 && s_count[tid]) atomicAdd(&a.count[tid], (unsigned long long)s_count[tid]);
}

// lifcal_rawdepth_points: flag, compaction in ascending pixel index, fill
__global__ __launch_bounds__(kThreads) void k_rawdepth_flag(int64_t npix, const float* __restrict__ inv_depth, const int32_t* __restrict__ map_ml, uint8_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= npix) return;
  const float v = inv_depth[i];
  flag[i] = (v == v && map_ml[i] >= 0) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_rawdepth_points(uint32_t n, const uint32_t* __restrict__ src, int W, double scale, const float* __restrict__ inv_depth,
                                                              const int32_t* __restrict__ map_ml, const float* __restrict__ cx, const float* __restrict__ cy,
                                                              double* __restrict__ x, double* __restrict__ y, double* __restrict__ vd, int32_t* __restrict__ lens) {
#pragma clang fp contract(off)
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = src[i];
  const int32_t l = map_ml[p];
  const double v = 1.0 / (double)inv_depth[p];
  const double px = (double)(p % (uint32_t)W), py = (double)(p / (uint32_t)W);
  const double lcx = (double)cx[l], lcy = (double)cy[l];
  const double xu = lcx + v * (px - lcx), yu = lcy + v * (py - lcy);
  x[i] = (xu + 0.5) / scale - 0.5;
  y[i] = (yu + 0.5) / scale - 0.5;
  vd[i] = v;
  lens[i] = l;
}

// ------------------------------------------------------------------------------------------------ host side

static int fail(int code, const std::string& text) { set_last_error(text.c_str()); return code; }
static int fail_hip(const char* who, hipError_t e) { return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }

struct Tables {
  lifcal_rawdepth_options opt;     // defaults resolved
  int N = 0;
  std::vector<double> iv;          // [K]
  std::vector<double> delta;       // [2][N][2]
  std::vector<int32_t> shift;      // [2][K][N][2]
  double step = 0, valid_r = 0, r0 = 0, r1 = 0;
  int rb = 0, half = 0;
  size_t lds_bytes = 0;
};

struct Cand { double len, ang, x, y; };

// arguments and options against the grid's parameters; fills the tables.  No device.
static int make_tables(const char* who, const lifcal_mla_params* p, const lifcal_rawdepth_image* im, const lifcal_rawdepth_options* o, Tables* t) {
#pragma clang fp contract(off)
  const std::string w = std::string(who) + ": ";
  if (!p || p->width <= 0 || p->height <= 0 || !(p->lens_diameter > 2.0f) || !(p->lens_diameter < 1.0e4f) || !(p->lens_base_y[1] > 0.0f) ||
      !std::isfinite(p->lens_base_y[0]) || !std::isfinite(p->rotation))
    return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "bad grid parameters");
  if (!im || !im->data) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no image");
  if (im->bits != 8 && im->bits != 16) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image bits must be 8 or 16");
  if (im->width != p->width || im->height != p->height) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image size differs from the grid's");
  if (im->pitch < im->width) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image pitch is smaller than its width");
  lifcal_rawdepth_options q{};
  if (o) q = *o;
  if (q.n_hyp == 0) q.n_hyp = 64;
  if (q.patch_radius == 0) q.patch_radius = 1;
  if (q.min_neighbours == 0) q.min_neighbours = 2;
  if (q.min_contrast == 0) q.min_contrast = im->bits == 8 ? 8 : 2048;
  if (q.iv_min == 0.0) q.iv_min = 0.04;
  if (q.iv_max == 0.0) q.iv_max = 0.5;
  if (q.max_baseline == 0.0) q.max_baseline = 1.05;
  if (q.ambiguity_ratio == 0.0) q.ambiguity_ratio = 1.5;
  if (q.n_hyp < 8 || q.n_hyp > kMaxHyp) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "n_hyp outside 8 .. 256");
  if (q.patch_radius != 1 && q.patch_radius != 2) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "patch_radius must be 1 or 2");
  if (!(q.iv_min > 0.0) || !(q.iv_min < q.iv_max) || !(q.iv_max <= 0.5)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "need 0 < iv_min < iv_max <= 0.5");
  if (!(q.max_baseline > 0.0) || !(q.max_baseline < 8.0)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_baseline must be positive");
  if (q.min_neighbours < 1 || q.min_neighbours > kMaxNeighbours) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_neighbours outside 1 .. 18");
  if (q.min_contrast < 0 || q.min_contrast > 65535) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_contrast outside 0 .. 65535");
  if (!(q.ambiguity_ratio >= 1.0) || !std::isfinite(q.ambiguity_ratio)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "ambiguity_ratio must be at least 1");
  t->opt = q;
  const int K = q.n_hyp;
  t->step = (q.iv_max - q.iv_min) / (double)(K - 1);
  t->iv.resize(K);
  for (int k = 0; k < K; ++k) t->iv[k] = q.iv_min + (double)k * t->step;

  const double d = (double)p->lens_diameter, bx = (double)p->lens_base_y[0], by = (double)p->lens_base_y[1];
  const double rot = p->rotation_on_grid ? (double)p->rotation : 0.0;
  const double c = std::cos(rot), s = std::sin(rot);
  const double e1[2] = {c, -s}, e2[2] = {-s, -c};
  double A[2], C[2], D[2];
  for (int i = 0; i < 2; ++i) {
    A[i] = d * e1[i];
    C[i] = 2.0 * by * d * e2[i];
    D[i] = (1.0 + bx) * d * e1[i] + by * d * e2[i];
  }
  const double limit = q.max_baseline * d;
  std::vector<Cand> cand[2];
  for (int sub = 0; sub < 2; ++sub) {
    for (int use_d = 0; use_d < 2; ++use_d)
      for (int x = -8; x <= 8; ++x)
        for (int y = -8; y <= 8; ++y) {
          double vx = (double)x * A[0] + (double)y * C[0];
          double vy = (double)x * A[1] + (double)y * C[1];
          if (use_d) {
            if (sub == 0) { vx = vx + D[0]; vy = vy + D[1]; } else { vx = vx - D[0]; vy = vy - D[1]; }
          } else if (x == 0 && y == 0) {
            continue;
          }
          const double len = std::sqrt(vx * vx + vy * vy);
          if (len <= limit) cand[sub].push_back(Cand{len, std::atan2(vy, vx), vx, vy});
        }
    std::sort(cand[sub].begin(), cand[sub].end(), [](const Cand& l, const Cand& r) {
      if (l.len != r.len) return l.len < r.len;
      if (l.ang != r.ang) return l.ang < r.ang;
      return l.x != r.x ? l.x < r.x : l.y < r.y;
    });
  }
  if (cand[0].size() != cand[1].size() || cand[0].empty()) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_baseline reaches no neighbour");
  if (cand[0].size() > (size_t)kMaxNeighbours) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_baseline selects more than 18 neighbours");
  const int N = t->N = (int)cand[0].size();
  t->delta.resize((size_t)2 * N * 2);
  t->shift.resize((size_t)2 * K * N * 2);
  int64_t smax = 0;
  for (int sub = 0; sub < 2; ++sub)
    for (int n = 0; n < N; ++n) {
      const double dl[2] = {cand[sub][n].x, cand[sub][n].y};
      for (int i = 0; i < 2; ++i) {
        t->delta[((size_t)sub * N + n) * 2 + i] = dl[i];
        for (int k = 0; k < K; ++k) {
          const double u = 1.0 - t->iv[k];
          const double sh = std::floor(64.0 * (dl[i] * u) + 0.5);
          t->shift[(((size_t)sub * K + k) * N + n) * 2 + i] = (int32_t)sh;
          smax = std::max<int64_t>(smax, (int64_t)std::fabs(sh));
        }
      }
    }
  const float valid_r = p->lens_diameter * 0.5f - 1.0f;   // mla::derive
  t->valid_r = (double)valid_r;
  t->r0 = t->valid_r - (double)q.patch_radius;
  t->r1 = t->r0 - 1.0;
  t->rb = t->r0 >= 0.0 ? (int)std::floor(t->r0 + 0.5) : 0;
  t->half = t->rb + q.patch_radius + (int)((smax + 63) >> 6) + 1;
  const size_t side = 2 * (size_t)t->half + 1, bs = 2 * (size_t)t->rb + 1;
  t->lds_bytes = (((side * side + 1) & ~(size_t)1) + bs * bs) * 2;
  if (t->lds_bytes > (size_t)kLdsLimit - 2048 || bs * bs > 65535)
    return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "the neighbourhood of one lens (" + std::to_string(side) + " pixels square) does not fit 64 KB of LDS");
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
  template <class T>
  hipError_t upload(const T** out, const std::vector<T>& v) {
    T* p = nullptr;
    hipError_t e = alloc(&p, v.size() * sizeof(T));
    if (e == hipSuccess && !v.empty()) e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
    *out = p;
    return e;
  }
};

}  // namespace rawdepth
}  // namespace lifcal

extern "C" {

using namespace lifcal::rawdepth;

int lifcal_rawdepth_check(const lifcal_mla_params* grid_params, const lifcal_rawdepth_image* image, const lifcal_rawdepth_options* options,
                          lifcal_rawdepth_plan* plan) {
  Tables t;
  if (int rc = make_tables("lifcal_rawdepth_check", grid_params, image, options, &t)) return rc;
  if (plan) {
    plan->options = t.opt;
    plan->n_neighbours = t.N;
    plan->window = 2 * t.half + 1;
    plan->lds_bytes = (int32_t)t.lds_bytes;
    plan->reserved = 0;
  }
  return 0;
}

int lifcal_rawdepth_estimate(lifcal_mla_handle* grid, const lifcal_rawdepth_image* image, const lifcal_rawdepth_options* options,
                             lifcal_rawdepth_result* out) {
  const char* who = "lifcal_rawdepth_estimate";
  lifcal::MlaView g;
  if (!lifcal::mla_view(grid, &g) || !out) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no grid or no result");
  Tables t;
  if (int rc = make_tables(who, &g.prm, image, options, &t)) return rc;
  out->n_neighbours_used = t.N;
  out->seconds = 0.0;
  for (uint64_t& c : out->count) c = 0;
  if (hipSetDevice(g.device) != hipSuccess) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");

  const int W = g.prm.width, H = g.prm.height;
  const size_t npix = (size_t)W * H, es = image->bits == 8 ? 1 : 2;
  DeviceBuffers buf;
  Args a{};
  a.W = W; a.H = H; a.n_sub0 = g.n_sub0;
  a.K = t.opt.n_hyp; a.N = t.N; a.min_neighbours = t.opt.min_neighbours; a.min_contrast = t.opt.min_contrast;
  a.rb = t.rb; a.half = t.half;
  a.r0sq = t.r0 * t.r0;
  a.r1sq = t.r1 >= 0.0 ? t.r1 * t.r1 : -1.0;
  a.step = t.step; a.ratio = t.opt.ambiguity_ratio;
  a.cost_scale = 4096.0 * (double)((2 * t.opt.patch_radius + 1) * (2 * t.opt.patch_radius + 1));
  a.cx = g.cx; a.cy = g.cy; a.map_ml = g.map_ml;
  hipError_t e = hipSuccess;
  if (image->on_device) {
    a.img = image->data; a.pitch = image->pitch;
  } else {
    void* d_img = nullptr;
    e = buf.alloc(&d_img, npix * es);
    if (e == hipSuccess) e = hipMemcpy2D(d_img, (size_t)W * es, image->data, (size_t)image->pitch * es, (size_t)W * es, (size_t)H, hipMemcpyHostToDevice);
    a.img = d_img; a.pitch = W;
  }
  if (e == hipSuccess) e = buf.upload(&a.iv, t.iv);
  if (e == hipSuccess) e = buf.upload(&a.delta, t.delta);
  if (e == hipSuccess) e = buf.upload(&a.shift, t.shift);
  if (e == hipSuccess) e = buf.alloc(&a.count, 5 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(a.count, 0, 5 * sizeof(unsigned long long));
  if (out->out_on_device) {
    a.inv_depth = out->inv_depth; a.cost = out->cost; a.status = out->status; a.nn = out->n_neighbours;
  } else {
    if (e == hipSuccess && out->inv_depth) e = buf.alloc(&a.inv_depth, npix * 4);
    if (e == hipSuccess && out->cost) e = buf.alloc(&a.cost, npix * 4);
    if (e == hipSuccess && out->status) e = buf.alloc(&a.status, npix);
    if (e == hipSuccess && out->n_neighbours) e = buf.alloc(&a.nn, npix);
  }
  if (e == hipSuccess) e = hipEventCreate(&buf.ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&buf.ev[1]);
  if (e != hipSuccess) return fail_hip(who, e);

  e = hipEventRecord(buf.ev[0], 0);
  hipLaunchKernelGGL(k_rawdepth_fill, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, (int64_t)npix, a.inv_depth, a.cost, a.status, a.nn);
  if (t.r0 >= 0.0) {
    const dim3 grd((unsigned)g.n_lenses), blk(kThreads);
    const size_t lds = t.lds_bytes;
    const bool w1 = t.opt.patch_radius == 1;
    if (image->bits == 8) {
      if (w1) hipLaunchKernelGGL((k_rawdepth_lens<uint8_t, 1>), grd, blk, lds, 0, a);
      else hipLaunchKernelGGL((k_rawdepth_lens<uint8_t, 2>), grd, blk, lds, 0, a);
    } else {
      if (w1) hipLaunchKernelGGL((k_rawdepth_lens<uint16_t, 1>), grd, blk, lds, 0, a);
      else hipLaunchKernelGGL((k_rawdepth_lens<uint16_t, 2>), grd, blk, lds, 0, a);
    }
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(buf.ev[1], 0);
  if (e == hipSuccess) e = hipEventSynchronize(buf.ev[1]);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, buf.ev[0], buf.ev[1]);
  unsigned long long count[5] = {0, 0, 0, 0, 0};
  if (e == hipSuccess) e = hipMemcpy(count, a.count, sizeof(count), hipMemcpyDeviceToHost);
  if (e == hipSuccess && !out->out_on_device) {
    if (out->inv_depth) e = hipMemcpy(out->inv_depth, a.inv_depth, npix * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out->cost) e = hipMemcpy(out->cost, a.cost, npix * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out->status) e = hipMemcpy(out->status, a.status, npix, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out->n_neighbours) e = hipMemcpy(out->n_neighbours, a.nn, npix, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return fail_hip(who, e);
  count[1] = (unsigned long long)npix - count[0] - count[2] - count[3] - count[4];
  for (int i = 0; i < 5; ++i) out->count[i] = count[i];
  out->seconds = 1.0e-3 * (double)ms;
  return 0;
}

int lifcal_rawdepth_points(lifcal_mla_handle* grid, lifcal_rawdepth_point_list* io) {
  const char* who = "lifcal_rawdepth_points";
  lifcal::MlaView g;
  if (!lifcal::mla_view(grid, &g) || !io || !io->inv_depth || io->depth_to_raw_im_scale < 1 || (io->capacity && (!io->x || !io->y || !io->vdepth)))
    return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": bad argument");
  io->n = 0;
  if (hipSetDevice(g.device) != hipSuccess) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");
  const int W = g.prm.width, H = g.prm.height;
  const size_t npix = (size_t)W * H;
  DeviceBuffers buf;
  const float* d_iv = io->inv_depth;
  hipError_t e = hipSuccess;
  if (!io->on_device) {
    float* q = nullptr;
    e = buf.alloc(&q, npix * 4);
    if (e == hipSuccess) e = hipMemcpy(q, io->inv_depth, npix * 4, hipMemcpyHostToDevice);
    d_iv = q;
  }
  uint8_t* flag = nullptr; uint32_t* src = nullptr; uint32_t* d_n = nullptr; void* scratch = nullptr; size_t scratch_bytes = 0;
  if (e == hipSuccess) e = buf.alloc(&flag, npix);
  if (e == hipSuccess) e = buf.alloc(&src, npix * 4);
  if (e == hipSuccess) e = buf.alloc(&d_n, 4);
  if (e != hipSuccess) return fail_hip(who, e);
  hipLaunchKernelGGL(k_rawdepth_flag, dim3((unsigned)((npix + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, (int64_t)npix, d_iv, g.map_ml, flag);
  e = hipGetLastError();
  hipcub::CountingInputIterator<uint32_t> ids(0u);
  if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged(nullptr, scratch_bytes, ids, flag, src, d_n, (int)npix);
  if (e == hipSuccess) e = buf.alloc(&scratch, scratch_bytes);
  if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged(scratch, scratch_bytes, ids, flag, src, d_n, (int)npix);
  uint32_t n = 0;
  if (e == hipSuccess) e = hipMemcpy(&n, d_n, 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail_hip(who, e);
  io->n = n;
  if (n > io->capacity) return LIFCAL_MLA_MORE;
  if (n == 0) return 0;
  double *x = nullptr, *y = nullptr, *vd = nullptr; int32_t* lens = nullptr;
  e = buf.alloc(&x, (size_t)n * 8);
  if (e == hipSuccess) e = buf.alloc(&y, (size_t)n * 8);
  if (e == hipSuccess) e = buf.alloc(&vd, (size_t)n * 8);
  if (e == hipSuccess) e = buf.alloc(&lens, (size_t)n * 4);
  if (e != hipSuccess) return fail_hip(who, e);
  hipLaunchKernelGGL(k_rawdepth_points, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, n, src, W, (double)io->depth_to_raw_im_scale, d_iv, g.map_ml, g.cx, g.cy,
                     x, y, vd, lens);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpy(io->x, x, (size_t)n * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(io->y, y, (size_t)n * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(io->vdepth, vd, (size_t)n * 8, hipMemcpyDeviceToHost);
  if (e == hipSuccess && io->src) e = hipMemcpy(io->src, src, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e == hipSuccess && io->lens) e = hipMemcpy(io->lens, lens, (size_t)n * 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail_hip(who, e);
  return 0;
}

}  // extern "C"
