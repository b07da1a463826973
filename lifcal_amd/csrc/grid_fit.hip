// grid_fit.hip — the micro-lens grid from a white image (include/lifcal_grid.h), in a code object of its
// own (grid_fit.hpp says why).
//
// What runs where: the per-pixel stages run on the device — k_grid_box (box sum), k_grid_peaks (local maxima of the box sum with
// a contrast test), a stream compaction of the peak flags in ascending pixel order, k_grid_centroid (integer moments over a disc,
// one wave per peak).  Everything in them is integer arithmetic except the disc test (doubles, no fused multiply-add) and the
// one division per coordinate, so a result is the same bits on every run and equal to the numpy restatement's.  Everything after
// the centroids is at most 10^5 small records and runs on the host in double: labelling, the 4 x 4 normal matrix of [1, x, y, k],
// the six-parameter Gauss-Newton fit and the outlier gate (lifcal_grid_fit_centres, no device needed).
#include "grid_fit.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/lifcal_ba.h"
#include "../../include/lifcal_grid.h"

static_assert(sizeof(lifcal::grid::Centre) == sizeof(lifcal_grid_centre) && sizeof(lifcal_grid_centre) == 48, "lifcal_grid_centre layout");
static_assert(sizeof(lifcal_grid_lens) == 32, "lifcal_grid_lens layout");

namespace lifcal {
namespace grid {

// ------------------------------------------------------------------------------------------------ device side

// Box sum of radius r (r <= kBoxRMax), zero outside the image.  The tile with its halo goes to LDS once (every load checked
// against the image), rows are summed by a sliding window (four lanes per row, 16 outputs each), then columns likewise.
template <class T>
__global__ __launch_bounds__(kBoxThreads) void k_grid_box(const T* __restrict__ img, int W, int H, int r, uint32_t* __restrict__ box) {
  constexpr int TW = kBoxX + 2 * kBoxRMax, TH = kBoxY + 2 * kBoxRMax;   // 96 x 64
  __shared__ uint16_t s_in[TH][TW + 2];
  __shared__ uint32_t s_h[TH][kBoxX];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kBoxX, y0 = blockIdx.y * kBoxY;
  const int tw = kBoxX + 2 * r, th = kBoxY + 2 * r;
  for (int i = tid; i < tw * th; i += kBoxThreads) {
    const int ly = i / tw, lx = i - ly * tw;
    const int gx = x0 - r + lx, gy = y0 - r + ly;
    uint16_t v = 0;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = (uint16_t)img[(size_t)gy * W + gx];
    s_in[ly][lx] = v;
  }
  __syncthreads();
  {
    const int row = tid >> 2, xs = (tid & 3) * 16;
    if (row < th) {
      uint32_t sum = 0;
      for (int j = 0; j <= 2 * r; ++j) sum += s_in[row][xs + j];
      s_h[row][xs] = sum;
      for (int x = xs + 1; x < xs + 16; ++x) {
        sum += s_in[row][x + 2 * r];
        sum -= s_in[row][x - 1];
        s_h[row][x] = sum;
      }
    }
  }
  __syncthreads();
  {
    const int col = tid & 63, ys = (tid >> 6) * 8;
    const int gx = x0 + col;
    uint32_t sum = 0;
    for (int j = 0; j <= 2 * r; ++j) sum += s_h[ys + j][col];
    for (int y = ys; y < ys + 8; ++y) {
      if (y > ys) { sum += s_h[y + 2 * r][col]; sum -= s_h[y - 1][col]; }
      const int gy = y0 + y;
      if (gx < W && gy < H) box[(size_t)gy * W + gx] = sum;
    }
  }
}

// A pixel is a peak when its key (box sum, then the lower pixel index) is the maximum of the (2m+1)^2 window around it, its
// box sum stands out against the window's minimum by at least an eighth of itself (a test against its own neighbourhood, so
// vignetting loses no lens), and it is at least `border` pixels inside the image.  Keys are unique, so the maximum is taken
// separably: rows first, into LDS, then columns.  Pixels outside the image take no part (key 0, no minimum).
// flag[idx] = 1 / 0 for every pixel; the tile's peak count goes to *count with one integer atomic per workgroup.
__global__ __launch_bounds__(kPeakThreads) void k_grid_peaks(const uint32_t* __restrict__ box, int W, int H, int m, int border,
                                                             uint8_t* __restrict__ flag, uint32_t* __restrict__ count) {
  constexpr int TW = kPeakX + 2 * kPeakMMax;   // 82
  __shared__ uint32_t s_box[TW][TW + 1];
  __shared__ uint64_t s_hmax[TW][kPeakX];
  __shared__ uint32_t s_hmin[TW][kPeakX];
  __shared__ uint32_t s_count;
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kPeakX, y0 = blockIdx.y * kPeakY;
  const int tw = kPeakX + 2 * m, th = kPeakY + 2 * m;
  if (tid == 0) s_count = 0;
  for (int i = tid; i < tw * th; i += kPeakThreads) {
    const int ly = i / tw, lx = i - ly * tw;
    const int gx = x0 - m + lx, gy = y0 - m + ly;
    uint32_t v = 0;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) v = box[(size_t)gy * W + gx];
    s_box[ly][lx] = v;
  }
  __syncthreads();
  for (int i = tid; i < th * kPeakX; i += kPeakThreads) {
    const int ly = i / kPeakX, lx = i - ly * kPeakX;
    const int gy = y0 - m + ly, gx = x0 + lx;
    uint64_t kmax = 0;
    uint32_t vmin = 0xffffffffu;
    if (gy >= 0 && gy < H) {
      for (int j = 0; j <= 2 * m; ++j) {
        const int xx = gx - m + j;
        if (xx < 0 || xx >= W) continue;
        const uint32_t v = s_box[ly][lx + j];
        const uint32_t idx = (uint32_t)gy * (uint32_t)W + (uint32_t)xx;
        const uint64_t key = ((uint64_t)v << 32) | (uint64_t)(0xffffffffu - idx);
        kmax = key > kmax ? key : kmax;
        vmin = v < vmin ? v : vmin;
      }
    }
    s_hmax[ly][lx] = kmax;
    s_hmin[ly][lx] = vmin;
  }
  __syncthreads();
  uint32_t mine = 0;
  for (int i = tid; i < kPeakY * kPeakX; i += kPeakThreads) {
    const int ly = i / kPeakX, lx = i - ly * kPeakX;
    const int gy = y0 + ly, gx = x0 + lx;
    if (gx >= W || gy >= H) continue;
    uint64_t kmax = 0;
    uint32_t vmin = 0xffffffffu;
    for (int j = 0; j <= 2 * m; ++j) {
      const uint64_t k = s_hmax[ly + j][lx];
      const uint32_t v = s_hmin[ly + j][lx];
      kmax = k > kmax ? k : kmax;
      vmin = v < vmin ? v : vmin;
    }
    const uint32_t v = s_box[ly + m][lx + m];
    const uint32_t idx = (uint32_t)gy * (uint32_t)W + (uint32_t)gx;
    const uint64_t key = ((uint64_t)v << 32) | (uint64_t)(0xffffffffu - idx);
    const bool inside = gx >= border && gx <= W - 1 - border && gy >= border && gy <= H - 1 - border;
    const bool peak = inside && key == kmax && v > 0 && (uint64_t)(v - vmin) * 8u >= (uint64_t)v;
    flag[(size_t)gy * W + gx] = peak ? 1 : 0;
    mine += peak ? 1u : 0u;
  }
  if (mine) atomicAdd(&s_count, mine);
  __syncthreads();
  if (tid == 0 && s_count) atomicAdd(count, s_count);
}

// One wave per peak, two rounds.  A round takes the pixels of the image whose centre lies in the disc of radius R about the
// current estimate (the peak pixel first, then round one's centroid), and sums, in 64-bit integers, 1, x, y, v, v x, v y and
// the minimum of v; the moments of the weight v - min follow from those without a second pass.  Integer wave reductions have
// no order, so the moments are exact; the disc test is the only floating-point decision (doubles, no fused multiply-add) and
// the two divisions are the only floating-point results.
template <class T>
__global__ __launch_bounds__(kCentroidThreads) void k_grid_centroid(const T* __restrict__ img, int W, int H, const uint32_t* __restrict__ peaks,
                                                                    uint32_t n, double R, double R2, Centre* __restrict__ out) {
#pragma clang fp contract(off)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t p = blockIdx.x * (kCentroidThreads / 64) + (threadIdx.x >> 6);
  if (p >= n) return;   // whole waves leave: no workgroup barrier below
  const uint32_t peak = peaks[p];
  double ex = (double)(peak % (uint32_t)W), ey = (double)(peak / (uint32_t)W);
  long long sw = 0, swx = 0, swy = 0;
  for (int round = 0; round < 2; ++round) {
    const double xl = ceil(ex - R), xh = floor(ex + R), yl = ceil(ey - R), yh = floor(ey + R);
    const int x_lo = xl < 0.0 ? 0 : (int)xl, x_hi = xh > (double)(W - 1) ? W - 1 : (int)xh;
    const int y_lo = yl < 0.0 ? 0 : (int)yl, y_hi = yh > (double)(H - 1) ? H - 1 : (int)yh;
    const int nx = x_hi - x_lo + 1, ny = y_hi - y_lo + 1;
    long long c1 = 0, cx = 0, cy = 0, cv = 0, cvx = 0, cvy = 0, mn = 0x7fffffff;
    if (nx > 0 && ny > 0) {
      for (int i = (int)lane; i < nx * ny; i += 64) {
        const int yy = i / nx;
        const int x = x_lo + (i - yy * nx), y = y_lo + yy;
        const double dx = (double)x - ex, dy = (double)y - ey;
        if (dx * dx + dy * dy <= R2) {
          const long long v = (long long)img[(size_t)y * W + x];
          c1 += 1; cx += x; cy += y; cv += v; cvx += v * x; cvy += v * y;
          mn = v < mn ? v : mn;
        }
      }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      c1 += __shfl_xor(c1, s, 64); cx += __shfl_xor(cx, s, 64); cy += __shfl_xor(cy, s, 64);
      cv += __shfl_xor(cv, s, 64); cvx += __shfl_xor(cvx, s, 64); cvy += __shfl_xor(cvy, s, 64);
      const long long o = __shfl_xor(mn, s, 64);
      mn = o < mn ? o : mn;
    }
    sw = cv - mn * c1; swx = cvx - mn * cx; swy = cvy - mn * cy;
    if (c1 == 0) { sw = 0; swx = 0; swy = 0; }
    if (sw > 0) { ex = (double)swx / (double)sw; ey = (double)swy / (double)sw; }   // a flat disc keeps its estimate
  }
  if (lane == 0) {
    Centre c;
    c.cx = ex; c.cy = ey; c.sum_w = sw; c.sum_wx = swx; c.sum_wy = swy; c.peak = (int64_t)peak;
    out[p] = c;
  }
}

// ------------------------------------------------------------------------------------------------ host driver of the detection

static Sizes sizes_of(double guess) {
#pragma clang fp contract(off)
  Sizes s;
  s.r = (int)std::floor(0.25 * guess + 0.5);
  s.m = (int)std::floor(0.4 * guess);
  s.border = (int)std::ceil(0.5 * guess) + 1;
  s.R = 0.5 * guess;
  s.R2 = s.R * s.R;
  return s;
}

static int fail(int code, const std::string& text) { set_last_error(text.c_str()); return code; }
static int fail_hip(const char* who, hipError_t e) { return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }

static int select_device(int32_t device, const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev)
    return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");
  hipDeviceProp_t prop;
  if (hipSetDevice(device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": hipSetDevice failed");
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": device is " + prop.gcnArchName + ", this library carries gfx950 code objects only");
  return 0;
}

static bool image_ok(const lifcal_grid_image* im) {
  return im && im->data && (im->bits == 8 || im->bits == 16) && im->width > 0 && im->height > 0 && im->pitch >= im->width &&
         (int64_t)im->width * im->height <= (int64_t)1 << 30;
}
static bool guess_ok(double g) { return std::isfinite(g) && g >= kGuessMin && g <= kGuessMax; }

// the image on the device (dense rows) and the per-pixel buffers of the detection, sized once and used by both passes
struct DeviceImage {
  void* img = nullptr;
  uint32_t* box = nullptr;
  uint8_t* flag = nullptr;
  uint32_t* count = nullptr;   // [0] peaks counted by k_grid_peaks, [1] entries the compaction wrote
  int W = 0, H = 0, bits = 0;
  std::vector<void*> extra;    // sized from the count of a pass: peak list, centres, the compaction's scratch
  ~DeviceImage() {
    for (void* q : extra) (void)hipFree(q);
    for (void* q : {img, (void*)box, (void*)flag, (void*)count}) if (q) (void)hipFree(q);
  }
  void drop_extra() { for (void* q : extra) (void)hipFree(q); extra.clear(); }
};

static hipError_t upload_image(DeviceImage& d, const lifcal_grid_image* im) {
  d.W = im->width; d.H = im->height; d.bits = im->bits;
  const size_t es = im->bits == 8 ? 1 : 2, npix = (size_t)d.W * d.H;
  hipError_t e = hipMalloc(&d.img, npix * es);
  if (e == hipSuccess) e = hipMalloc((void**)&d.box, npix * 4);
  if (e == hipSuccess) e = hipMalloc((void**)&d.flag, npix);
  if (e == hipSuccess) e = hipMalloc((void**)&d.count, 8);
  if (e == hipSuccess) e = hipMemcpy2D(d.img, (size_t)d.W * es, im->data, (size_t)im->pitch * es, (size_t)d.W * es, (size_t)d.H, hipMemcpyHostToDevice);
  return e;
}

// box sum and peak flags of the uploaded image; *n is the number of peaks (the count pass of the count-then-fill protocol)
static hipError_t find_peaks(DeviceImage& d, const Sizes& s, uint64_t* n) {
  const int W = d.W, H = d.H;
  hipError_t e = hipMemset(d.count, 0, 8);
  if (e != hipSuccess) return e;
  const dim3 gb((W + kBoxX - 1) / kBoxX, (H + kBoxY - 1) / kBoxY), gp((W + kPeakX - 1) / kPeakX, (H + kPeakY - 1) / kPeakY);
  if (d.bits == 8) hipLaunchKernelGGL(k_grid_box<uint8_t>, gb, dim3(kBoxThreads), 0, 0, (const uint8_t*)d.img, W, H, s.r, d.box);
  else hipLaunchKernelGGL(k_grid_box<uint16_t>, gb, dim3(kBoxThreads), 0, 0, (const uint16_t*)d.img, W, H, s.r, d.box);
  hipLaunchKernelGGL(k_grid_peaks, gp, dim3(kPeakThreads), 0, 0, d.box, W, H, s.m, s.border, d.flag, d.count);
  e = hipGetLastError();
  uint32_t count = 0;
  if (e == hipSuccess) e = hipMemcpy(&count, d.count, 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return e;
  *n = count;
  return hipSuccess;
}

// the fill pass behind find_peaks: compaction of its flags in ascending pixel order (the flagged entries of 0, 1, 2, ...), then
// the centroids; buffers sized from its count
static hipError_t centroids(DeviceImage& d, const Sizes& s, uint32_t count, std::vector<lifcal_grid_centre>* centres) {
  centres->clear();
  if (count == 0) return hipSuccess;
  const int W = d.W, H = d.H;
  const size_t npix = (size_t)W * H;
  hipError_t e = hipSuccess;
  d.drop_extra();
  uint32_t* peaks = nullptr; Centre* out = nullptr; void* scratch = nullptr; size_t scratch_bytes = 0;
  e = hipMalloc((void**)&peaks, (size_t)count * 4);
  if (e == hipSuccess) d.extra.push_back(peaks);
  if (e == hipSuccess) { e = hipMalloc((void**)&out, (size_t)count * sizeof(Centre)); if (e == hipSuccess) d.extra.push_back(out); }
  hipcub::CountingInputIterator<uint32_t> ids(0u);
  if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged(nullptr, scratch_bytes, ids, d.flag, peaks, d.count + 1, (int)npix);
  if (e == hipSuccess) { e = hipMalloc(&scratch, std::max<size_t>(scratch_bytes, 8)); if (e == hipSuccess) d.extra.push_back(scratch); }
  if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged(scratch, scratch_bytes, ids, d.flag, peaks, d.count + 1, (int)npix);
  if (e == hipSuccess) {
    const unsigned blocks = (count + kCentroidThreads / 64 - 1) / (kCentroidThreads / 64);
    if (d.bits == 8) hipLaunchKernelGGL(k_grid_centroid<uint8_t>, dim3(blocks), dim3(kCentroidThreads), 0, 0, (const uint8_t*)d.img, W, H, peaks, count, s.R, s.R2, out);
    else hipLaunchKernelGGL(k_grid_centroid<uint16_t>, dim3(blocks), dim3(kCentroidThreads), 0, 0, (const uint16_t*)d.img, W, H, peaks, count, s.R, s.R2, out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    centres->resize(count);
    e = hipMemcpy(centres->data(), out, (size_t)count * sizeof(Centre), hipMemcpyDeviceToHost);
  }
  return e;
}

// ------------------------------------------------------------------------------------------------ host fit (double, no device)
//
// The model in image coordinates: centre(k, x, y) = o + x A + y C + k D with A = d e1, C = 2 by d e2, D = (1 + bx) d e1 + by d e2,
// e1 = (cos, -sin), e2 = (-sin, -cos) (grid y points up, image y down).  Unconstrained, (o, A, C, D) is a linear model in
// phi = [1, x, y, k]; the six-parameter model is fitted to the same quadratic (normal matrix N = sum phi phi^T, integer, and
// right-hand sides Rx, Ry = sum p phi) by Gauss-Newton steps.

struct Model { double o[2], A[2], C[2], D[2]; };
struct Label { int32_t k, x, y; double frac; };

// solves the n x n system a z = b for nrhs right-hand sides (columns of b, row-major n x nrhs) in place, partial pivoting
static bool solve_linear(int n, double* a, double* b, int nrhs) {
#pragma clang fp contract(off)
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r) if (std::fabs(a[r * n + c]) > std::fabs(a[piv * n + c])) piv = r;
    if (!(std::fabs(a[piv * n + c]) > 1e-300)) return false;
    if (piv != c) {
      for (int j = 0; j < n; ++j) std::swap(a[c * n + j], a[piv * n + j]);
      for (int j = 0; j < nrhs; ++j) std::swap(b[c * nrhs + j], b[piv * nrhs + j]);
    }
    for (int r = c + 1; r < n; ++r) {
      const double f = a[r * n + c] / a[c * n + c];
      for (int j = c; j < n; ++j) a[r * n + j] = a[r * n + j] - f * a[c * n + j];
      for (int j = 0; j < nrhs; ++j) b[r * nrhs + j] = b[r * nrhs + j] - f * b[c * nrhs + j];
    }
  }
  for (int c = n - 1; c >= 0; --c) {
    for (int j = 0; j < nrhs; ++j) {
      double s = b[c * nrhs + j];
      for (int k = c + 1; k < n; ++k) s = s - a[c * n + k] * b[k * nrhs + j];
      b[c * nrhs + j] = s / a[c * n + c];
    }
  }
  return true;
}

static Label label_of(const Model& m, double px, double py) {
#pragma clang fp contract(off)
  const double det = m.A[0] * m.C[1] - m.A[1] * m.C[0];
  Label best{0, 0, 0, 0.0};
  for (int k = 0; k < 2; ++k) {
    const double vx = px - m.o[0] - k * m.D[0], vy = py - m.o[1] - k * m.D[1];
    const double qx = (vx * m.C[1] - vy * m.C[0]) / det, qy = (m.A[0] * vy - m.A[1] * vx) / det;
    const double rx = std::floor(qx + 0.5), ry = std::floor(qy + 0.5);
    const double f = std::max(std::fabs(qx - rx), std::fabs(qy - ry));
    if (k == 0 || f < best.frac) {
      const double lim = 1.0e9;
      best = Label{k, (int32_t)std::max(-lim, std::min(lim, rx)), (int32_t)std::max(-lim, std::min(lim, ry)), f};
    }
  }
  return best;
}

// the normal equations over the centres with use[i] != 0, in the order given: indices centred by the integers xbar, ybar
// (rounded means), coordinates by the image centre
struct Normal {
  double N[16];       // integer sums of [1, x - xbar, y - ybar, k]
  double R[8];        // [4][2]: sum phi (p - image centre)
  int64_t xbar, ybar;
  uint64_t count;
};

static Normal accumulate(uint64_t n, const double* cx, const double* cy, const Label* lab, const uint8_t* use, const double* imc) {
#pragma clang fp contract(off)
  Normal nm{};
  int64_t sx = 0, sy = 0; uint64_t cnt = 0;
  for (uint64_t i = 0; i < n; ++i) if (use[i]) { sx += lab[i].x; sy += lab[i].y; ++cnt; }
  nm.count = cnt;
  if (!cnt) return nm;
  nm.xbar = (int64_t)std::floor((double)sx / (double)cnt + 0.5);
  nm.ybar = (int64_t)std::floor((double)sy / (double)cnt + 0.5);
  int64_t Ni[16] = {0};
  for (uint64_t i = 0; i < n; ++i) {
    if (!use[i]) continue;
    const int64_t phi[4] = {1, lab[i].x - nm.xbar, lab[i].y - nm.ybar, lab[i].k};
    const double px = cx[i] - imc[0], py = cy[i] - imc[1];
    for (int a = 0; a < 4; ++a) {
      for (int b = 0; b < 4; ++b) Ni[a * 4 + b] += phi[a] * phi[b];
      nm.R[a * 2 + 0] = nm.R[a * 2 + 0] + (double)phi[a] * px;
      nm.R[a * 2 + 1] = nm.R[a * 2 + 1] + (double)phi[a] * py;
    }
  }
  for (int a = 0; a < 16; ++a) nm.N[a] = (double)Ni[a];
  return nm;
}

// unconstrained least squares: rows of the solution are o (at the centred indices, relative to the image centre), A, C, D
static bool solve_free(const Normal& nm, double* M /* [4][2] */) {
  double a[16], b[8];
  std::memcpy(a, nm.N, sizeof(a)); std::memcpy(b, nm.R, sizeof(b));
  double scale = 0;
  for (int i = 0; i < 4; ++i) scale = std::max(scale, std::fabs(a[i * 4 + i]));
  if (!solve_linear(4, a, b, 2)) return false;
  for (int i = 0; i < 8; ++i) if (!std::isfinite(b[i])) return false;
  // a normal matrix of rank < 4 (one sub-grid only, one row, one column) leaves a pivot at rounding level
  for (int i = 0; i < 4; ++i) if (!(std::fabs(a[i * 4 + i]) > 1e-9 * std::max(scale, 1.0))) return false;
  std::memcpy(M, b, sizeof(b));
  return true;
}

static Model model_of_free(const double* M, const Normal& nm, const double* imc) {
#pragma clang fp contract(off)
  Model m;
  for (int c = 0; c < 2; ++c) {
    m.A[c] = M[2 + c]; m.C[c] = M[4 + c]; m.D[c] = M[6 + c];
    m.o[c] = ((M[c] - (double)nm.xbar * m.A[c]) - (double)nm.ybar * m.C[c]) + imc[c];
  }
  return m;
}

struct Six { double oc[2], d, rot, by, bx; };   // oc: the origin at the centred indices, relative to the image centre

static void six_matrix(const Six& t, double* M /* [4][2] */) {
#pragma clang fp contract(off)
  const double c = std::cos(t.rot), s = std::sin(t.rot);
  const double e1[2] = {c, -s}, e2[2] = {-s, -c};
  for (int q = 0; q < 2; ++q) {
    M[q] = t.oc[q];
    M[2 + q] = t.d * e1[q];
    M[4 + q] = 2.0 * t.by * t.d * e2[q];
    M[6 + q] = (1.0 + t.bx) * t.d * e1[q] + t.by * t.d * e2[q];
  }
}

// Gauss-Newton on f = tr(M N M^T) - 2 tr(M R^T) over the six parameters, started at the unconstrained solution
static bool fit_six(const Normal& nm, const double* Mfree, Six* out) {
#pragma clang fp contract(off)
  Six t;
  const double* A = Mfree + 2; const double* Cc = Mfree + 4; const double* D = Mfree + 6;
  t.oc[0] = Mfree[0]; t.oc[1] = Mfree[1];
  t.d = std::sqrt(A[0] * A[0] + A[1] * A[1]);
  t.rot = std::atan2(-A[1], A[0]);
  {
    const double c = std::cos(t.rot), s = std::sin(t.rot);
    t.by = (Cc[0] * -s + Cc[1] * -c) / (2.0 * t.d);
    t.bx = (D[0] * c + D[1] * -s) / t.d - 1.0;
  }
  for (int it = 0; it < 6; ++it) {
    const double c = std::cos(t.rot), s = std::sin(t.rot);
    const double e1[2] = {c, -s}, e2[2] = {-s, -c};
    double M[8];
    six_matrix(t, M);
    // dM[i][row of phi][coordinate]
    double dM[6][8] = {{0}};
    dM[0][0] = 1.0; dM[1][1] = 1.0;
    for (int q = 0; q < 2; ++q) {
      dM[2][2 + q] = e1[q]; dM[2][4 + q] = 2.0 * t.by * e2[q]; dM[2][6 + q] = (1.0 + t.bx) * e1[q] + t.by * e2[q];
      dM[3][2 + q] = t.d * e2[q]; dM[3][4 + q] = -2.0 * t.by * t.d * e1[q]; dM[3][6 + q] = (1.0 + t.bx) * t.d * e2[q] - t.by * t.d * e1[q];
      dM[4][4 + q] = 2.0 * t.d * e2[q]; dM[4][6 + q] = t.d * e2[q];
      dM[5][6 + q] = t.d * e1[q];
    }
    double E[8];   // N M - R
    for (int a = 0; a < 4; ++a) for (int q = 0; q < 2; ++q) {
      double sum = 0;
      for (int b = 0; b < 4; ++b) sum = sum + nm.N[a * 4 + b] * M[b * 2 + q];
      E[a * 2 + q] = sum - nm.R[a * 2 + q];
    }
    double H[36], g[6];
    for (int i = 0; i < 6; ++i) {
      double NdM[8];
      for (int a = 0; a < 4; ++a) for (int q = 0; q < 2; ++q) {
        double sum = 0;
        for (int b = 0; b < 4; ++b) sum = sum + nm.N[a * 4 + b] * dM[i][b * 2 + q];
        NdM[a * 2 + q] = sum;
      }
      double gi = 0;
      for (int a = 0; a < 8; ++a) gi = gi + E[a] * dM[i][a];
      g[i] = -gi;
      for (int j = 0; j < 6; ++j) {
        double h = 0;
        for (int a = 0; a < 8; ++a) h = h + NdM[a] * dM[j][a];
        H[i * 6 + j] = h;
      }
    }
    if (!solve_linear(6, H, g, 1)) return false;
    t.oc[0] = t.oc[0] + g[0]; t.oc[1] = t.oc[1] + g[1]; t.d = t.d + g[2]; t.rot = t.rot + g[3]; t.by = t.by + g[4]; t.bx = t.bx + g[5];
    if (!(std::isfinite(t.d) && std::isfinite(t.rot) && std::isfinite(t.by) && std::isfinite(t.bx) && t.d > 0)) return false;
  }
  *out = t;
  return true;
}

static Model model_of_six(const Six& t, const Normal& nm, const double* imc) {
  double M[8];
  six_matrix(t, M);
  return model_of_free(M, nm, imc);
}

static int fit_centres(uint64_t n, const double* cx, const double* cy, int32_t W, int32_t H, double guess, double gate_px,
                       lifcal_mla_params* params, lifcal_grid_report* report) {
#pragma clang fp contract(off)
  const char* who = "lifcal_grid_fit_centres: ";
  if (!params || (n && (!cx || !cy)) || W <= 0 || H <= 0 || !guess_ok(guess) || !(gate_px >= 0.0) || !std::isfinite(gate_px) || n > (uint64_t)1 << 26)
    return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "bad argument (6 <= guess <= 64, gate_px >= 0)");
  if (report && ((report->capacity && !report->lens) || (report->capacity && report->capacity < n)))
    return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "report->capacity is smaller than the number of centres");
  if (n < 12) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "fewer than 12 centres");
  for (uint64_t i = 0; i < n; ++i) if (!std::isfinite(cx[i]) || !std::isfinite(cy[i])) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "non-finite centre");
  const double imc[2] = {((double)W - 1.0) / 2.0, ((double)H - 1.0) / 2.0};

  // seeds: the centres nearest to the image centre, nearest first; the first with a row neighbour and a next-row neighbour starts
  std::vector<uint32_t> order(n);
  std::vector<double> dist2(n);
  for (uint64_t i = 0; i < n; ++i) { order[i] = (uint32_t)i; const double dx = cx[i] - imc[0], dy = cy[i] - imc[1]; dist2[i] = dx * dx + dy * dy; }
  const size_t n_seeds = (size_t)std::min<uint64_t>(n, 16);
  std::partial_sort(order.begin(), order.begin() + n_seeds, order.end(), [&](uint32_t a, uint32_t b) { return dist2[a] < dist2[b] || (dist2[a] == dist2[b] && a < b); });
  Model mod{};
  double seed[2] = {0, 0};
  bool started = false;
  const double slope_max = 0.55;   // tan(29 degrees): hexagonal neighbours sit 60 degrees apart
  for (size_t si = 0; si < n_seeds && !started; ++si) {
    const uint32_t s = order[si];
    double A0[2] = {0, 0}, best_slope = 0; bool haveA = false;
    for (uint64_t j = 0; j < n; ++j) {
      if (j == s) continue;
      double ux = cx[j] - cx[s], uy = cy[j] - cy[s];
      const double len = std::sqrt(ux * ux + uy * uy);
      if (!(len >= 0.8 * guess && len <= 1.25 * guess)) continue;
      if (ux < 0) { ux = -ux; uy = -uy; }
      if (!(ux > 0)) continue;
      const double slope = std::fabs(uy) / ux;
      if (slope <= slope_max && (!haveA || slope < best_slope)) { haveA = true; best_slope = slope; A0[0] = ux; A0[1] = uy; }
    }
    if (!haveA) continue;
    const double d0 = std::sqrt(A0[0] * A0[0] + A0[1] * A0[1]);
    const double e1[2] = {A0[0] / d0, A0[1] / d0}, e2[2] = {e1[1], -e1[0]};
    double D0[2] = {0, 0}, best_h = 0; bool haveD = false;
    for (uint64_t j = 0; j < n; ++j) {
      if (j == s) continue;
      for (int sgn = 0; sgn < 2; ++sgn) {
        const double ux = sgn ? cx[s] - cx[j] : cx[j] - cx[s], uy = sgn ? cy[s] - cy[j] : cy[j] - cy[s];
        const double len = std::sqrt(ux * ux + uy * uy);
        const double h = ux * e2[0] + uy * e2[1], t = (ux * e1[0] + uy * e1[1]) / d0;
        if (!(len <= 1.6 * guess && h > 0.3 * guess && t >= -0.05 && t < 0.95)) continue;
        if (!haveD || h < best_h) { haveD = true; best_h = h; D0[0] = ux; D0[1] = uy; }
      }
    }
    if (!haveD) continue;
    mod.o[0] = cx[s]; mod.o[1] = cy[s];
    mod.A[0] = A0[0]; mod.A[1] = A0[1];
    mod.D[0] = D0[0]; mod.D[1] = D0[1];
    mod.C[0] = 2.0 * best_h * e2[0]; mod.C[1] = 2.0 * best_h * e2[1];
    seed[0] = cx[s]; seed[1] = cy[s];
    started = true;
  }
  if (!started) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "no centre near the image centre has a row neighbour and a next-row neighbour at the guessed diameter");

  // grow the labelled region about the seed, refitting the unconstrained lattice each time
  std::vector<Label> lab(n);
  std::vector<uint8_t> use(n);
  const double diag = std::sqrt((double)W * (double)W + (double)H * (double)H);
  double M[8];
  for (double rho = 3.5 * guess;; rho = rho * 3.0) {
    for (uint64_t i = 0; i < n; ++i) {
      const double dx = cx[i] - seed[0], dy = cy[i] - seed[1];
      lab[i] = label_of(mod, cx[i], cy[i]);
      use[i] = (dx * dx + dy * dy <= rho * rho && lab[i].frac <= 0.25) ? 1 : 0;
    }
    const Normal nm = accumulate(n, cx, cy, lab.data(), use.data(), imc);
    if (nm.count < 6 || !solve_free(nm, M)) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "the centres about the image centre do not span a two-dimensional lattice");
    mod = model_of_free(M, nm, imc);
    if (rho >= diag) break;
  }

  // the origin: the node nearest to the image centre becomes lens (0, 0, 0); D keeps its A component in [0, 1)
  {
    const double det = mod.A[0] * mod.C[1] - mod.A[1] * mod.C[0];
    double best[2] = {0, 0}, best_d2 = 0; int best_k = 0;
    for (int k = 0; k < 2; ++k) {
      const double vx = imc[0] - mod.o[0] - k * mod.D[0], vy = imc[1] - mod.o[1] - k * mod.D[1];
      const double rx = std::floor((vx * mod.C[1] - vy * mod.C[0]) / det + 0.5), ry = std::floor((mod.A[0] * vy - mod.A[1] * vx) / det + 0.5);
      const double px = mod.o[0] + rx * mod.A[0] + ry * mod.C[0] + k * mod.D[0], py = mod.o[1] + rx * mod.A[1] + ry * mod.C[1] + k * mod.D[1];
      const double d2 = (px - imc[0]) * (px - imc[0]) + (py - imc[1]) * (py - imc[1]);
      if (k == 0 || d2 < best_d2) { best_d2 = d2; best_k = k; best[0] = px; best[1] = py; }
    }
    mod.o[0] = best[0]; mod.o[1] = best[1];
    if (best_k == 1) { mod.D[0] = mod.C[0] - mod.D[0]; mod.D[1] = mod.C[1] - mod.D[1]; }
    const double t = (mod.D[0] * mod.A[0] + mod.D[1] * mod.A[1]) / (mod.A[0] * mod.A[0] + mod.A[1] * mod.A[1]);
    const double sh = std::floor(t);
    mod.D[0] = mod.D[0] - sh * mod.A[0]; mod.D[1] = mod.D[1] - sh * mod.A[1];
  }
  uint64_t n_label = 0, n_resid = 0;
  for (uint64_t i = 0; i < n; ++i) {
    lab[i] = label_of(mod, cx[i], cy[i]);
    use[i] = lab[i].frac <= 0.25 ? 1 : 0;
    n_label += use[i] ? 0 : 1;
  }

  // fit, gate on the residuals, fit once more
  Six six{}; Normal nm{}; Model fitted{};
  std::vector<double> rx(n), ry(n);
  double rms = 0, rmax = 0;
  for (int pass = 0; pass < 2; ++pass) {
    nm = accumulate(n, cx, cy, lab.data(), use.data(), imc);
    if (nm.count < 12) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "fewer than 12 accepted centres");
    if (!solve_free(nm, M) || !fit_six(nm, M, &six)) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "the accepted centres do not span a two-dimensional lattice");
    fitted = model_of_six(six, nm, imc);
    double ss = 0; rmax = 0;
    for (uint64_t i = 0; i < n; ++i) {
      const double fx = fitted.o[0] + (double)lab[i].x * fitted.A[0] + (double)lab[i].y * fitted.C[0] + (double)lab[i].k * fitted.D[0];
      const double fy = fitted.o[1] + (double)lab[i].x * fitted.A[1] + (double)lab[i].y * fitted.C[1] + (double)lab[i].k * fitted.D[1];
      rx[i] = cx[i] - fx; ry[i] = cy[i] - fy;
      if (use[i]) { const double r2 = rx[i] * rx[i] + ry[i] * ry[i]; ss = ss + r2; rmax = std::max(rmax, std::sqrt(r2)); }
    }
    rms = std::sqrt(ss / (double)nm.count);
    if (pass == 1) break;
    const double thr = std::max(gate_px, 4.0 * rms);
    for (uint64_t i = 0; i < n; ++i)
      if (use[i] && std::sqrt(rx[i] * rx[i] + ry[i] * ry[i]) > thr) { use[i] = 0; ++n_resid; }
  }
  {
    std::vector<int64_t> rows, cols;
    for (uint64_t i = 0; i < n; ++i) if (use[i]) { rows.push_back(2 * (int64_t)lab[i].y + lab[i].k); cols.push_back(2 * (int64_t)lab[i].x + lab[i].k); }
    for (std::vector<int64_t>* v : {&rows, &cols}) { std::sort(v->begin(), v->end()); v->erase(std::unique(v->begin(), v->end()), v->end()); }
    if (rows.size() < 3 || cols.size() < 3) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "the accepted centres span fewer than three rows or columns");
  }
  const double ten_degrees = 0.17453292519943295;
  if (!(std::fabs(six.rot) < ten_degrees)) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "rotation of 10 degrees or more: the row vector would not be the lattice vector nearest to +x");
  if (!(six.by > 0)) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + "fitted lens_base_y[1] is not positive");

  std::memset(params, 0, sizeof(*params));
  params->width = W; params->height = H;
  params->lens_diameter = (float)six.d;
  params->lens_base_y[0] = (float)six.bx; params->lens_base_y[1] = (float)six.by;
  params->rotation = (float)six.rot;
  // lifcal_mla_create: offset_cv = (offset[0] + width / 2 - 0.5, -offset[1] + height / 2 - 0.5)
  params->offset[0] = (float)(fitted.o[0] - imc[0]);
  params->offset[1] = (float)(-(fitted.o[1] - imc[1]));
  params->rotation_on_grid = 1;
  if (report) {
    report->n_centres = n; report->n_accepted = nm.count; report->n_rejected_label = n_label; report->n_rejected_residual = n_resid;
    report->rms = rms; report->max_residual = rmax;
    for (int q = 0; q < 2; ++q) { report->lattice_a[q] = M[2 + q]; report->lattice_b[q] = M[6 + q]; report->lattice_c[q] = M[4 + q]; }
    report->lens_diameter = six.d; report->rotation = six.rot; report->lens_base_y[0] = six.bx; report->lens_base_y[1] = six.by;
    report->origin[0] = fitted.o[0]; report->origin[1] = fitted.o[1];
    if (report->capacity)
      for (uint64_t i = 0; i < n; ++i) report->lens[i] = lifcal_grid_lens{lab[i].k, lab[i].x, lab[i].y, use[i] ? 1 : 0, rx[i], ry[i]};
  }
  return 0;
}

}  // namespace grid
}  // namespace lifcal

extern "C" {

using namespace lifcal::grid;

int lifcal_grid_detect(const lifcal_grid_image* image, double guess, int32_t device, lifcal_grid_centres* out) {
  if (!image_ok(image) || !guess_ok(guess) || !out || (out->capacity && !out->c))
    return fail(LIFCAL_BA_ERR_INVALID_ARG, "lifcal_grid_detect: bad argument (8- or 16-bit image, pitch >= width, 6 <= guess <= 64)");
  out->n = 0;
  if (int rc = select_device(device, "lifcal_grid_detect")) return rc;
  DeviceImage d;
  hipError_t e = upload_image(d, image);
  const Sizes s = sizes_of(guess);
  uint64_t n = 0;
  if (e == hipSuccess) e = find_peaks(d, s, &n);
  if (e != hipSuccess) return fail_hip("lifcal_grid_detect", e);
  out->n = n;
  if (n > out->capacity) return LIFCAL_MLA_MORE;
  if (n == 0) return 0;
  std::vector<lifcal_grid_centre> c;
  e = centroids(d, s, (uint32_t)n, &c);
  if (e != hipSuccess) return fail_hip("lifcal_grid_detect", e);
  std::memcpy(out->c, c.data(), n * sizeof(lifcal_grid_centre));
  return 0;
}

int lifcal_grid_fit_centres(uint64_t n, const double* cx, const double* cy, int32_t width, int32_t height, double guess, double gate_px,
                            lifcal_mla_params* params, lifcal_grid_report* report) {
  return fit_centres(n, cx, cy, width, height, guess, gate_px, params, report);
}

int lifcal_grid_fit(const lifcal_grid_image* image, double guess, double gate_px, int32_t device, lifcal_mla_params* params,
                    lifcal_grid_centres* centres, lifcal_grid_report* report) {
  if (!image_ok(image) || !guess_ok(guess) || !params || (centres && centres->capacity && !centres->c) || (report && report->capacity && !report->lens) ||
      !(gate_px >= 0.0) || !std::isfinite(gate_px))
    return fail(LIFCAL_BA_ERR_INVALID_ARG, "lifcal_grid_fit: bad argument (8- or 16-bit image, pitch >= width, 6 <= guess <= 64, gate_px >= 0)");
  if (centres) centres->n = 0;
  if (report) report->n_centres = 0;
  if (int rc = select_device(device, "lifcal_grid_fit")) return rc;
  DeviceImage d;
  hipError_t e = upload_image(d, image);
  if (e != hipSuccess) return fail_hip("lifcal_grid_fit", e);
  std::vector<lifcal_grid_centre> c;
  std::vector<double> cx, cy;
  lifcal_mla_params first{};
  double g = guess;
  for (int pass = 0; pass < 2; ++pass) {
    const Sizes s = sizes_of(g);
    uint64_t n = 0;
    e = find_peaks(d, s, &n);
    if (e == hipSuccess) e = centroids(d, s, (uint32_t)n, &c);
    if (e != hipSuccess) return fail_hip("lifcal_grid_fit", e);
    cx.resize(n); cy.resize(n);
    for (uint64_t i = 0; i < n; ++i) { cx[i] = c[i].cx; cy[i] = c[i].cy; }
    if (pass == 0) {
      if (int rc = fit_centres(n, cx.data(), cy.data(), image->width, image->height, g, gate_px, &first, nullptr)) return rc;
      g = std::min(kGuessMax, std::max(kGuessMin, (double)first.lens_diameter));
      continue;
    }
    if (centres) centres->n = n;
    if (report) report->n_centres = n;
    if ((centres && centres->capacity < n) || (report && report->capacity && report->capacity < n)) return LIFCAL_MLA_MORE;
    if (int rc = fit_centres(n, cx.data(), cy.data(), image->width, image->height, g, gate_px, params, report)) return rc;
    if (centres && n) std::memcpy(centres->c, c.data(), n * sizeof(lifcal_grid_centre));
  }
  return 0;
}

}  // extern "C"
