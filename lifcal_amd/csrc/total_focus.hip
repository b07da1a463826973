// total_focus.hip — the total-focus image from the raw image and the virtual-image depth map (include/lifcal_totalfocus.h,
// DESIGN.md section 7v), in a code object of its own like raw_depth.hip and depth_map.hip (raw_depth.hpp says why).
//
// What runs where: the host checks the arguments and sorts the lens centres into square bins of side d (a few thousand numbers,
// uploaded per call); k_totalfocus_gather does everything per cell.  One workgroup takes a 16 x 16 tile of cells, one cell per
// lane; the smallest depth of the tile bounds the bins that can hold a lens any of its cells uses, and the loop over those
// lenses is the same for the whole workgroup, so a lens's centre is read once through the scalar path and the lanes that take
// it read one small patch of one micro image.  Everything summed is an integer and every floating-point step is an IEEE double
// operation without fused multiply-add, so the bytes are the same on every run and equal to the numpy restatement's.
#include "raw_depth.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/lifcal_ba.h"
#include "../../include/lifcal_totalfocus.h"

namespace lifcal {
namespace totalfocus {

constexpr int kTile = 16;                     // cells per tile side
constexpr int kThreads = kTile * kTile;       // one cell per lane
constexpr int64_t kMaxLensesPerCell = 1ll << 18;
constexpr int64_t kMaxBins = 1ll << 26;

// ------------------------------------------------------------------------------------------------ device side

struct Args {
  int32_t W, H, ow, oh;
  int32_t min_lenses, nbx, nby;
  uint32_t white_level, full;
  double scale, iv_min, default_iv, r_use, r_use2, reach, reach2;
  double bin_x0, bin_y0, d;
  const double* bcx; const double* bcy;   // lens centres in bin order (row-major bins)
  const int32_t* bin_start;               // [nby * nbx + 1]
  const void* img; int64_t pitch;
  const void* white; int64_t wpitch;
  const float* inv_depth;                 // [oh][ow]
  void* image; uint8_t* n_lenses; uint8_t* status;
  unsigned long long* count;              // [4]
};

// (64-fx)(64-fy) I(ix,iy) + fx (64-fy) I(ix+1,iy) + (64-fx) fy I(ix,iy+1) + fx fy I(ix+1,iy+1): at most 4096 * 65535 < 2^32
template <class T>
__device__ __forceinline__ uint32_t bilinear(const T* __restrict__ p, int64_t pitch, uint32_t fx, uint32_t fy) {
  const uint32_t a = p[0], b = p[1], c = p[pitch], e = p[pitch + 1];
  return (64u - fx) * (64u - fy) * a + fx * (64u - fy) * b + (64u - fx) * fy * c + fx * fy * e;
}

template <class T, bool HAS_WHITE>
__global__ __launch_bounds__(kThreads) void k_totalfocus_gather(Args a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_min_iv;   // bits of the smallest iv of the tile (positive doubles order like their bits)
  __shared__ unsigned s_count[4];
  const int tid = threadIdx.x;
  if (tid < 4) s_count[tid] = 0;
  if (tid == 0) s_min_iv = ~0ull;
  __syncthreads();
  const int X0 = blockIdx.x * kTile, Y0 = blockIdx.y * kTile;
  const int X = X0 + (tid & (kTile - 1)), Y = Y0 + (tid >> 4);
  const bool inside = X < a.ow && Y < a.oh;
  const int64_t cell = (int64_t)Y * a.ow + X;
  double iv = 0.0;
  bool has_depth = false, active = false;
  if (inside) {
    iv = (double)a.inv_depth[cell];
    has_depth = iv >= a.iv_min && iv <= 1.0;   // false for NaN
    active = has_depth;
    if (!has_depth && a.default_iv > 0.0) { iv = a.default_iv; active = true; }
  }
  // the smallest iv of the tile: a minimum over each wave, then one LDS atomic per wave
  unsigned long long bits = active ? (unsigned long long)__double_as_longlong(iv) : ~0ull;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)bits, m), hi = (unsigned)__shfl_xor((int)(unsigned)(bits >> 32), m);
    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
    bits = other < bits ? other : bits;
  }
  if ((tid & 63) == 0) atomicMin(&s_min_iv, bits);
  __syncthreads();
  const unsigned long long min_bits = s_min_iv;

  const double xu = ((double)X + 0.5) * a.scale - 0.5, yu = ((double)Y + 0.5) * a.scale - 0.5;
  unsigned long long num = 0, den = 0;
  uint32_t n = 0;
  if (min_bits != ~0ull) {   // the same for the whole workgroup
    // A lens counts for a cell only within min(max_reach d, r_use / iv) of it; one pixel more covers the rounding of the
    // tests.  The host puts a centre into bin floor((c - x0) / d); the same expression is monotonic in c, so the bins
    // from that of the low end to that of the high end hold every centre in between.
    const double min_iv = __longlong_as_double((long long)min_bits);
    const double R = fmin(a.reach, a.r_use / min_iv) + 1.0;
    const int Xl = min(X0 + kTile - 1, a.ow - 1), Yl = min(Y0 + kTile - 1, a.oh - 1);
    const double x_lo = (((double)X0 + 0.5) * a.scale - 0.5) - R, x_hi = (((double)Xl + 0.5) * a.scale - 0.5) + R;
    const double y_lo = (((double)Y0 + 0.5) * a.scale - 0.5) - R, y_hi = (((double)Yl + 0.5) * a.scale - 0.5) + R;
    const double fxa = floor((x_lo - a.bin_x0) / a.d), fxb = floor((x_hi - a.bin_x0) / a.d);
    const double fya = floor((y_lo - a.bin_y0) / a.d), fyb = floor((y_hi - a.bin_y0) / a.d);
    int bxa = 0, bxb = -1, bya = 0, byb = -1;
    if (fxb >= 0.0 && fxa <= (double)(a.nbx - 1) && fyb >= 0.0 && fya <= (double)(a.nby - 1)) {
      bxa = (int)fmax(fxa, 0.0); bxb = (int)fmin(fxb, (double)(a.nbx - 1));
      bya = (int)fmax(fya, 0.0); byb = (int)fmin(fyb, (double)(a.nby - 1));
    }
    bxa = __builtin_amdgcn_readfirstlane(bxa); bxb = __builtin_amdgcn_readfirstlane(bxb);
    bya = __builtin_amdgcn_readfirstlane(bya); byb = __builtin_amdgcn_readfirstlane(byb);
    const T* __restrict__ img = (const T*)a.img;
    const T* __restrict__ wht = (const T*)a.white;
    for (int by = bya; by <= byb; ++by) {
      // the bins bxa .. bxb of one row are adjacent in the sorted list
      const int j0 = a.bin_start[by * a.nbx + bxa], j1 = a.bin_start[by * a.nbx + bxb + 1];
      for (int j = j0; j < j1; ++j) {
        const double cx = a.bcx[j], cy = a.bcy[j];
        const double dx = xu - cx, dy = yu - cy;
        if (!active || !(dx * dx + dy * dy <= a.reach2)) continue;
        const double ox = dx * iv, oy = dy * iv;
        if (!(ox * ox + oy * oy <= a.r_use2)) continue;
        const long long Sx = (long long)floor(64.0 * (cx + ox) + 0.5), Sy = (long long)floor(64.0 * (cy + oy) + 0.5);
        const long long ix = Sx >> 6, iy = Sy >> 6;
        if (ix < 0 || ix + 1 > a.W - 1 || iy < 0 || iy + 1 > a.H - 1) continue;
        const uint32_t fx = (uint32_t)(Sx & 63), fy = (uint32_t)(Sy & 63);
        num += bilinear<T>(img + iy * a.pitch + ix, a.pitch, fx, fy);
        if (HAS_WHITE) den += bilinear<T>(wht + iy * a.wpitch + ix, a.wpitch, fx, fy);
        ++n;
      }
    }
  }

  if (inside) {
    int st = LIFCAL_TOTALFOCUS_NO_DEPTH;
    uint32_t pixel = 0;
    if (active) {
      st = LIFCAL_TOTALFOCUS_NO_LENS;
      if (n >= (uint32_t)a.min_lenses && (!HAS_WHITE || den > 0ull)) {
        st = has_depth ? LIFCAL_TOTALFOCUS_OK : LIFCAL_TOTALFOCUS_DEFAULT_DEPTH;
        if (HAS_WHITE) {
          const unsigned long long q = (2ull * num * (unsigned long long)a.white_level + den) / (2ull * den);
          pixel = q > (unsigned long long)a.full ? a.full : (uint32_t)q;
        } else {
          pixel = (uint32_t)((2ull * num + 4096ull * n) / (2ull * 4096ull * n));
        }
      }
    }
    if (a.image) ((T*)a.image)[cell] = (T)pixel;
    if (a.n_lenses) a.n_lenses[cell] = (uint8_t)(n > 255u ? 255u : n);
    if (a.status) a.status[cell] = (uint8_t)st;
    atomicAdd(&s_count[st], 1u);
  }
  __syncthreads();
  if (tid < 4 && s_count[tid]) atomicAdd(&a.count[tid], (unsigned long long)s_count[tid]);
}

// ------------------------------------------------------------------------------------------------ host side

static int fail(int code, const std::string& text) { set_last_error(text.c_str()); return code; }
static int fail_hip(const char* who, hipError_t e) { return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }

struct Plan {
  lifcal_totalfocus_options opt;   // defaults resolved
  double r_use = 0.0;
  int64_t max_lenses = 0;
  int32_t bits = 0;
};

// arguments and options against the grid's parameters.  No device.
static int make_plan(const char* who, const lifcal_mla_params* p, const lifcal_rawdepth_image* im, const lifcal_rawdepth_image* white, bool check_depth,
                     int32_t depth_width, int32_t depth_height, const lifcal_totalfocus_options* o, Plan* t) {
#pragma clang fp contract(off)
  const std::string w = std::string(who) + ": ";
  if (!p || p->width <= 0 || p->height <= 0 || !(p->lens_diameter > 2.0f) || !(p->lens_diameter < 1.0e4f) || !(p->lens_base_y[1] > 0.0f) ||
      !std::isfinite(p->lens_base_y[1]))
    return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "bad grid parameters");
  if (!im || !im->data) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no image");
  if (im->bits != 8 && im->bits != 16) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image bits must be 8 or 16");
  if (im->width != p->width || im->height != p->height) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image size differs from the grid's");
  if (im->pitch < im->width) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image pitch is smaller than its width");
  if (white) {
    if (!white->data) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "white image without data");
    if (white->bits != im->bits) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "white image bits differ from the image's");
    if (white->width != im->width || white->height != im->height) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "white image size differs from the image's");
    if (white->pitch < white->width) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "white image pitch is smaller than its width");
  }
  const int32_t full = im->bits == 8 ? 255 : 65535;
  lifcal_totalfocus_options q{};
  if (o) q = *o;
  if (q.scale == 0) q.scale = 1;
  if (q.min_lenses == 0) q.min_lenses = 1;
  if (q.white_level == 0) q.white_level = full;
  if (q.margin == 0.0) q.margin = 1.5;
  if (q.max_reach == 0.0) q.max_reach = 4.0;
  if (q.iv_min == 0.0) q.iv_min = 0.04;
  if (q.scale < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "scale must be at least 1");
  if (q.out_width < 0 || q.out_height < 0) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "out_width and out_height must not be negative");
  if (q.out_width == 0) q.out_width = p->width / q.scale;
  if (q.out_height == 0) q.out_height = p->height / q.scale;
  if (q.out_width < 1 || q.out_height < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "the output has no cells (scale above the image size)");
  if (q.min_lenses < 1 || q.min_lenses > 255) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_lenses outside 1 .. 255");
  if (q.white_level < 1 || q.white_level > full) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "white_level outside 1 .. full scale");
  if (!(q.margin >= 0.0) || !std::isfinite(q.margin)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "margin must not be negative");
  const double valid_r = (double)(p->lens_diameter * 0.5f - 1.0f);   // mla::derive
  t->r_use = valid_r - q.margin;
  if (!(t->r_use >= 0.5)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "r_use = valid_r - margin is below 0.5");
  if (!(q.max_reach > 0.0) || !(q.max_reach <= 8.0)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "need 0 < max_reach <= 8");
  if (!(q.iv_min >= 1.0e-3) || !(q.iv_min <= 1.0)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "need 0.001 <= iv_min <= 1");
  if (q.default_iv != 0.0 && (!(q.default_iv >= q.iv_min) || !(q.default_iv <= 1.0))) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "default_iv must be 0 or in [iv_min, 1]");
  if (check_depth && (depth_width != q.out_width || depth_height != q.out_height))
    return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "depth map size differs from the output's (" + std::to_string(q.out_width) + " x " + std::to_string(q.out_height) + ")");
  t->opt = q;
  t->bits = im->bits;
  if ((int64_t)p->width * p->height >= (1ll << 31) || (int64_t)q.out_width * q.out_height >= (1ll << 31))
    return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "2^31 raw pixels or cells and more are not supported");
  // the lenses that can count for one cell (include/lifcal_totalfocus.h): num white_level must stay below 2^63
  const double by = (double)p->lens_base_y[1];
  const double span = 2.0 * (q.max_reach + 1.0);
  const double bound = (std::floor(span / by) + 1.0) * (std::floor(span) + 1.0);
  if (!(bound < (double)kMaxLensesPerCell))
    return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "too many lenses can reach one cell for the 64-bit sums (lens_base_y too small)");
  t->max_lenses = (int64_t)bound;
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
  // a host image as a dense device copy, a device image as it is
  hipError_t image(const lifcal_rawdepth_image* im, const void** data, int64_t* pitch) {
    if (im->on_device) { *data = im->data; *pitch = im->pitch; return hipSuccess; }
    const size_t es = im->bits == 8 ? 1 : 2, W = (size_t)im->width, H = (size_t)im->height;
    void* d = nullptr;
    hipError_t e = alloc(&d, W * H * es);
    if (e == hipSuccess) e = hipMemcpy2D(d, W * es, im->data, (size_t)im->pitch * es, W * es, H, hipMemcpyHostToDevice);
    *data = d; *pitch = (int64_t)W;
    return e;
  }
};

// The lens centres in square bins of side d, row-major, as a sorted list with the start of every bin.  Centres that are not
// finite are left out (no cell can use them).
struct Bins {
  double x0 = 0.0, y0 = 0.0;
  int32_t nbx = 1, nby = 1;
  std::vector<double> cx, cy;
  std::vector<int32_t> start;
};

static bool make_bins(const std::vector<float>& lx, const std::vector<float>& ly, double d, Bins* b) {
#pragma clang fp contract(off)
  const size_t n = lx.size();
  double xmin = 0.0, xmax = 0.0, ymin = 0.0, ymax = 0.0;
  bool any = false;
  for (size_t i = 0; i < n; ++i) {
    const double x = (double)lx[i], y = (double)ly[i];
    if (!std::isfinite(x) || !std::isfinite(y)) continue;
    if (!any) { xmin = xmax = x; ymin = ymax = y; any = true; }
    xmin = std::min(xmin, x); xmax = std::max(xmax, x); ymin = std::min(ymin, y); ymax = std::max(ymax, y);
  }
  b->x0 = xmin; b->y0 = ymin;
  const double fx = std::floor((xmax - xmin) / d) + 1.0, fy = std::floor((ymax - ymin) / d) + 1.0;
  if (!(fx * fy < (double)kMaxBins)) return false;
  b->nbx = (int32_t)fx; b->nby = (int32_t)fy;
  const size_t nb = (size_t)b->nbx * (size_t)b->nby;
  std::vector<int32_t> bin(n, -1);
  b->start.assign(nb + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    const double x = (double)lx[i], y = (double)ly[i];
    if (!std::isfinite(x) || !std::isfinite(y)) continue;
    const int32_t bx = (int32_t)std::floor((x - b->x0) / d), by = (int32_t)std::floor((y - b->y0) / d);   // within 0 .. nbx-1, 0 .. nby-1
    bin[i] = by * b->nbx + bx;
    ++b->start[(size_t)bin[i] + 1];
  }
  for (size_t k = 0; k < nb; ++k) b->start[k + 1] += b->start[k];
  b->cx.assign((size_t)b->start[nb], 0.0); b->cy.assign((size_t)b->start[nb], 0.0);
  std::vector<int32_t> at(b->start.begin(), b->start.end() - 1);
  for (size_t i = 0; i < n; ++i) {
    if (bin[i] < 0) continue;
    const size_t k = (size_t)at[(size_t)bin[i]]++;
    b->cx[k] = (double)lx[i]; b->cy[k] = (double)ly[i];
  }
  return true;
}

}  // namespace totalfocus
}  // namespace lifcal

extern "C" {

using namespace lifcal::totalfocus;

int lifcal_totalfocus_check(const lifcal_mla_params* grid_params, const lifcal_rawdepth_image* image, const lifcal_rawdepth_image* white,
                            int32_t depth_width, int32_t depth_height, const lifcal_totalfocus_options* options, lifcal_totalfocus_plan* plan) {
  Plan t;
  if (int rc = make_plan("lifcal_totalfocus_check", grid_params, image, white, true, depth_width, depth_height, options, &t)) return rc;
  if (plan) {
    plan->options = t.opt;
    plan->out_width = t.opt.out_width;
    plan->out_height = t.opt.out_height;
    plan->r_use = t.r_use;
    plan->max_lenses_per_cell = (int32_t)t.max_lenses;
    plan->reserved = 0;
  }
  return 0;
}

int lifcal_totalfocus_render(lifcal_mla_handle* grid, const lifcal_rawdepth_image* image, const lifcal_rawdepth_image* white,
                             const float* inv_depth, int32_t depth_on_device, const lifcal_totalfocus_options* options,
                             lifcal_totalfocus_result* out) {
  const char* who = "lifcal_totalfocus_render";
  lifcal::MlaView g;
  if (!lifcal::mla_view(grid, &g) || !out) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no grid or no result");
  if (!inv_depth) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no depth map");
  Plan t;
  if (int rc = make_plan(who, &g.prm, image, white, false, 0, 0, options, &t)) return rc;
  out->seconds = 0.0;
  for (uint64_t& c : out->count) c = 0;
  // the lens list of the handle (host copies), binned
  int32_t n_list = 0;
  if (lifcal_mla_info(grid, &n_list, nullptr, nullptr) != 0 || n_list < 0) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": the grid has no lens list");
  std::vector<float> lx((size_t)n_list), ly((size_t)n_list);
  if (n_list > 0 && lifcal_mla_get_lenses(grid, lx.data(), ly.data(), nullptr) != 0) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": the grid has no lens list");
  const double d = (double)g.prm.lens_diameter;
  Bins bins;
  if (!make_bins(lx, ly, d, &bins)) return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, std::string(who) + ": the lens centres span too many bins");
  if (hipSetDevice(g.device) != hipSuccess) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");

  const int ow = t.opt.out_width, oh = t.opt.out_height;
  const size_t ncell = (size_t)ow * oh, es = t.bits == 8 ? 1 : 2;
  DeviceBuffers buf;
  Args a{};
  a.W = g.prm.width; a.H = g.prm.height; a.ow = ow; a.oh = oh;
  a.min_lenses = t.opt.min_lenses; a.nbx = bins.nbx; a.nby = bins.nby;
  a.white_level = (uint32_t)t.opt.white_level; a.full = t.bits == 8 ? 255u : 65535u;
  a.scale = (double)t.opt.scale; a.iv_min = t.opt.iv_min; a.default_iv = t.opt.default_iv;
  {
#pragma clang fp contract(off)
    const double valid_r = (double)g.valid_r;
    a.r_use = valid_r - t.opt.margin;
    a.r_use2 = a.r_use * a.r_use;
    a.reach = t.opt.max_reach * d;
    a.reach2 = a.reach * a.reach;
  }
  if (!(a.r_use >= 0.5)) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": r_use = valid_r - margin is below 0.5");
  a.bin_x0 = bins.x0; a.bin_y0 = bins.y0; a.d = d;
  hipError_t e = buf.image(image, &a.img, &a.pitch);
  if (e == hipSuccess && white) e = buf.image(white, &a.white, &a.wpitch);
  a.inv_depth = inv_depth;
  if (e == hipSuccess && !depth_on_device) {
    float* q = nullptr;
    e = buf.alloc(&q, ncell * 4);
    if (e == hipSuccess) e = hipMemcpy(q, inv_depth, ncell * 4, hipMemcpyHostToDevice);
    a.inv_depth = q;
  }
  if (e == hipSuccess) e = buf.upload(&a.bcx, bins.cx);
  if (e == hipSuccess) e = buf.upload(&a.bcy, bins.cy);
  if (e == hipSuccess) e = buf.upload(&a.bin_start, bins.start);
  if (e == hipSuccess) e = buf.alloc(&a.count, 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(a.count, 0, 4 * sizeof(unsigned long long));
  if (out->out_on_device) {
    a.image = out->image; a.n_lenses = out->n_lenses; a.status = out->status;
  } else {
    if (e == hipSuccess && out->image) e = buf.alloc(&a.image, ncell * es);
    if (e == hipSuccess && out->n_lenses) e = buf.alloc(&a.n_lenses, ncell);
    if (e == hipSuccess && out->status) e = buf.alloc(&a.status, ncell);
  }
  if (e == hipSuccess) e = hipEventCreate(&buf.ev[0]);
  if (e == hipSuccess) e = hipEventCreate(&buf.ev[1]);
  if (e != hipSuccess) return fail_hip(who, e);

  const dim3 grd((unsigned)((ow + kTile - 1) / kTile), (unsigned)((oh + kTile - 1) / kTile)), blk(kThreads);
  if (grd.y > 65535u) return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, std::string(who) + ": more than 65535 tile rows");
  e = hipEventRecord(buf.ev[0], 0);
  if (t.bits == 8) {
    if (white) hipLaunchKernelGGL((k_totalfocus_gather<uint8_t, true>), grd, blk, 0, 0, a);
    else hipLaunchKernelGGL((k_totalfocus_gather<uint8_t, false>), grd, blk, 0, 0, a);
  } else {
    if (white) hipLaunchKernelGGL((k_totalfocus_gather<uint16_t, true>), grd, blk, 0, 0, a);
    else hipLaunchKernelGGL((k_totalfocus_gather<uint16_t, false>), grd, blk, 0, 0, a);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(buf.ev[1], 0);
  if (e == hipSuccess) e = hipEventSynchronize(buf.ev[1]);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, buf.ev[0], buf.ev[1]);
  unsigned long long cnt[4] = {0, 0, 0, 0};
  if (e == hipSuccess) e = hipMemcpy(cnt, a.count, sizeof(cnt), hipMemcpyDeviceToHost);
  if (e == hipSuccess && !out->out_on_device) {
    if (out->image) e = hipMemcpy(out->image, a.image, ncell * es, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out->n_lenses) e = hipMemcpy(out->n_lenses, a.n_lenses, ncell, hipMemcpyDeviceToHost);
    if (e == hipSuccess && out->status) e = hipMemcpy(out->status, a.status, ncell, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return fail_hip(who, e);
  for (int i = 0; i < 4; ++i) out->count[i] = cnt[i];
  out->seconds = 1.0e-3 * (double)ms;
  return 0;
}

}  // extern "C"
