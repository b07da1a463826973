// features.hip — feature tracks from total-focus images (include/lifcal_features.h), in a code object of its
// own like total_focus.hip (raw_depth.hpp says why).
//
// What runs where.  k_features_detect: one workgroup per bucket.  It walks the bucket in sub-tiles of 32 x 32 pixels; per sub-tile
// the pixels (and the validity) with their halo go to LDS, then the Sobel gradients, the window sums and the score, the
// non-maximum suppression and the sub-pixel offsets, all from LDS, halos recomputed per sub-tile so that no workgroup waits on
// another; the survivors are ranked against the bucket's best so far and the best per_cell stay in the bucket's slots (a fixed
// capacity: no global atomic on the feature list).  The host compacts the slots.  k_features_describe: one wave per feature, the
// 31 x 31 patch to LDS, the 27 x 27 box sums, four tests per lane, the words assembled by ballot.  k_features_match: a workgroup
// takes 256 query features of one direction of one pair and streams the other frame's descriptors through LDS; best, second-best
// and index stay in registers.  The mutual test and the linker run on the host (features_host.hpp).
// Everything summed is an integer and every floating-point step is an IEEE double operation without fused multiply-add.
#include "raw_depth.hpp"

#include "features_host.hpp"

namespace lifcal {
namespace features {

constexpr int kThreads = 256;
constexpr int kSub = 32;                                          // sub-tile side
constexpr int kPixSide = kSub + 2 * (kMaxNmsR + kMaxWinR + 1);    // 52
constexpr int kGradSide = kSub + 2 * (kMaxNmsR + kMaxWinR);       // 50
constexpr int kScoreSide = kSub + 2 * kMaxNmsR;                   // 44
constexpr int kValSide = kSub + 2 * kPatchR;                      // 62
constexpr int kMaxNew = (kSub / 2) * (kSub / 2);                  // maxima lie more than nms_r >= 1 apart: at most 16 x 16 per sub-tile
constexpr int kMaxCand = kMaxNew + kMaxPerCell;
constexpr int kBox = 2 * 13 + 1;                                  // box sums the pattern can address: 27 x 27
constexpr int kPatch = 2 * kPatchR + 1;                           // 31

// ------------------------------------------------------------------------------------------------ device side

struct Slot {        // one kept feature of a bucket, 32 bytes
  double score, x, y;
  int32_t ix, iy;
};

struct DetectArgs {
  int32_t W, H, win_r, nms_r, cell, per_cell, nbx, pad;
  int64_t pitch;
  double min_score, full2;
  const void* img;
  const uint8_t* status;   // or nullptr
  Slot* slots;             // [buckets][per_cell]
  int32_t* count;          // [buckets]
};

// a before b in (score descending, y ascending, x ascending)
__device__ __forceinline__ bool before(const Slot& a, const Slot& b) {
  return a.score > b.score || (a.score == b.score && (a.iy < b.iy || (a.iy == b.iy && a.ix < b.ix)));
}

template <class T>
__global__ __launch_bounds__(kThreads) void k_features_detect(DetectArgs a) {
#pragma clang fp contract(off)
  __shared__ uint16_t s_pix[kPixSide * kPixSide];
  __shared__ int2 s_g[kGradSide * kGradSide];
  __shared__ double s_score[kScoreSide * kScoreSide];
  __shared__ uint8_t s_val[kValSide * kValSide];
  __shared__ uint8_t s_hv[kValSide * kSub];       // s_hv[r][c] = all of s_val[r][c .. c + 30]
  __shared__ Slot s_cand[kMaxCand];               // [0, n_top): the bucket's best so far; behind them the survivors of this sub-tile
  __shared__ Slot s_top[kMaxPerCell];
  __shared__ int s_n;
  const int tid = threadIdx.x;
  const int nr = a.nms_r, wr = a.win_r, R = nr + wr + 1;
  const int P = kSub + 2 * R, G = P - 2, C = kSub + 2 * nr;
  const int bx0 = blockIdx.x * a.cell, by0 = blockIdx.y * a.cell;
  const int lo = kPatchR + 1, xhi = a.W - 1 - lo, yhi = a.H - 1 - lo;   // candidates lie in [lo, xhi] x [lo, yhi]
  const T* __restrict__ img = (const T*)a.img;
  int n_top = 0;
  if (tid == 0) s_n = 0;
  __syncthreads();
  for (int sy = 0; sy < a.cell; sy += kSub) {
    for (int sx = 0; sx < a.cell; sx += kSub) {
      const int x0 = bx0 + sx, y0 = by0 + sy;
      const int sw = min(kSub, a.cell - sx), sh = min(kSub, a.cell - sy);
      // the same for the whole workgroup: a sub-tile without a candidate position is skipped
      if (x0 > xhi || x0 + sw - 1 < lo || y0 > yhi || y0 + sh - 1 < lo) continue;
      for (int i = tid; i < P * P; i += kThreads) {
        const int px = x0 - R + i % P, py = y0 - R + i / P;
        s_pix[i] = (px >= 0 && px < a.W && py >= 0 && py < a.H) ? (uint16_t)img[(int64_t)py * a.pitch + px] : (uint16_t)0;
      }
      if (a.status) {
        for (int i = tid; i < kValSide * kValSide; i += kThreads) {
          const int px = x0 - kPatchR + i % kValSide, py = y0 - kPatchR + i / kValSide;
          uint8_t v = 0;
          if (px >= 0 && px < a.W && py >= 0 && py < a.H) {
            const uint8_t st = a.status[(int64_t)py * a.W + px];
            v = (st == 0 || st == 3) ? 1 : 0;
          }
          s_val[i] = v;
        }
      }
      __syncthreads();
      // gradients at G x G positions: position (i, j) is pixel (i + 1, j + 1) of s_pix
      for (int i = tid; i < G * G; i += kThreads) {
        const uint16_t* p = s_pix + (i / G) * P + (i % G);
        const int p00 = p[0], p01 = p[1], p02 = p[2], p10 = p[P], p12 = p[P + 2], p20 = p[2 * P], p21 = p[2 * P + 1], p22 = p[2 * P + 2];
        s_g[i] = make_int2((p02 + 2 * p12 + p22) - (p00 + 2 * p10 + p20), (p20 + 2 * p21 + p22) - (p00 + 2 * p01 + p02));
      }
      if (a.status) {
        for (int i = tid; i < kValSide * kSub; i += kThreads) {
          const uint8_t* v = s_val + (i / kSub) * kValSide + (i % kSub);
          uint8_t all = 1;
          for (int k = 0; k < kPatch; ++k) all &= v[k];
          s_hv[i] = all;
        }
      }
      __syncthreads();
      // scores at C x C positions: position (i, j) is gradient (i + wr, j + wr)
      for (int i = tid; i < C * C; i += kThreads) {
        const int2* g = s_g + (i / C) * G + (i % C);
        long long A = 0, B = 0, Cc = 0;
        for (int dy = 0; dy <= 2 * wr; ++dy)
          for (int dx = 0; dx <= 2 * wr; ++dx) {
            const int2 v = g[dy * G + dx];
            A += (long long)v.x * v.x; B += (long long)v.x * v.y; Cc += (long long)v.y * v.y;
          }
        const double dA = (double)A, dB = (double)B, dC = (double)Cc;
        s_score[i] = ((dA * dC - dB * dB) / (dA + dC + 1.0)) / a.full2;
      }
      __syncthreads();
      // the maxima of the sub-tile: position (i, j) is score (i + nr, j + nr)
      for (int i = tid; i < kSub * kSub; i += kThreads) {
        const int cx = i % kSub, cy = i / kSub, x = x0 + cx, y = y0 + cy;
        if (cx >= sw || cy >= sh || x < lo || x > xhi || y < lo || y > yhi) continue;
        const double* s = s_score + (cy + nr) * C + (cx + nr);
        const double s0 = s[0];
        if (!(s0 >= a.min_score)) continue;
        bool is_max = true;
        for (int dy = -nr; dy <= nr && is_max; ++dy)
          for (int dx = -nr; dx <= nr; ++dx) {
            const double q = s[dy * C + dx];
            if (q > s0 || (q == s0 && (dy < 0 || (dy == 0 && dx < 0)))) { is_max = false; break; }
          }
        if (!is_max) continue;
        if (a.status) {
          uint8_t all = 1;
          for (int k = 0; k < kPatch; ++k) all &= s_hv[(cy + k) * kSub + cx];
          if (!all) continue;
        }
        double o[2];
        for (int ax = 0; ax < 2; ++ax) {
          const int st = ax ? C : 1;
          const double sm = s[-st], sp = s[st];
          const double den = (sm - 2.0 * s0) + sp;
          double v = den < 0.0 ? (0.5 * (sm - sp)) / den : 0.0;
          v = v < -0.5 ? -0.5 : (v > 0.5 ? 0.5 : v);
          o[ax] = v;
        }
        const int k = atomicAdd(&s_n, 1);
        if (k < kMaxCand) {
          Slot e;
          e.score = s0; e.x = (double)x + o[0]; e.y = (double)y + o[1]; e.ix = x; e.iy = y;
          s_cand[k] = e;
        }
      }
      __syncthreads();
      // rank the survivors together with the best so far: the order is total, so the outcome does not depend on the order of arrival
      const int n = min(s_n, kMaxCand);
      for (int e = tid; e < n; e += kThreads) {
        const Slot me = s_cand[e];
        int rank = 0;
        for (int f = 0; f < n; ++f) rank += (f != e && before(s_cand[f], me)) ? 1 : 0;
        if (rank < a.per_cell) s_top[rank] = me;
      }
      __syncthreads();
      n_top = min(n, a.per_cell);
      if (tid < n_top) s_cand[tid] = s_top[tid];
      if (tid == 0) s_n = n_top;
      __syncthreads();
    }
  }
  const int64_t bucket = (int64_t)blockIdx.y * a.nbx + blockIdx.x;
  if (tid < n_top) a.slots[bucket * a.per_cell + tid] = s_cand[tid];
  if (tid == 0) a.count[bucket] = n_top;
}

struct DescribeArgs {
  int32_t n, pad;
  int64_t pitch;
  const void* img;
  const int32_t* ix; const int32_t* iy;   // [n]
  const int8_t* pattern;                  // [256][4]
  uint32_t* desc;                         // [n][8]
};

// one wave per feature, four features per workgroup; every feature lies patch_r + 1 inside the image, so the patch does too
template <class T>
__global__ __launch_bounds__(kThreads) void k_features_describe(DescribeArgs a) {
  __shared__ uint16_t s_pix[4][kPatch * kPatch + 1];
  __shared__ uint32_t s_box[4][kBox * kBox];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.x * 4 + wave;
  const bool live = f < a.n;
  if (live) {
    const T* __restrict__ img = (const T*)a.img + (int64_t)(a.iy[f] - kPatchR) * a.pitch + (a.ix[f] - kPatchR);
    for (int i = lane; i < kPatch * kPatch; i += 64) s_pix[wave][i] = (uint16_t)img[(int64_t)(i / kPatch) * a.pitch + i % kPatch];
  }
  __syncthreads();
  if (live) {
    for (int i = lane; i < kBox * kBox; i += 64) {
      const uint16_t* p = s_pix[wave] + (i / kBox) * kPatch + i % kBox;   // box (u, v) covers patch columns u .. u + 4, rows v .. v + 4
      uint32_t sum = 0;
      for (int dy = 0; dy < 5; ++dy)
        for (int dx = 0; dx < 5; ++dx) sum += p[dy * kPatch + dx];
      s_box[wave][i] = sum;
    }
  }
  __syncthreads();
  if (live) {
    uint32_t mine = 0;
    for (int k = 0; k < 4; ++k) {
      const int i = k * 64 + lane;
      const int ax = a.pattern[4 * i], ay = a.pattern[4 * i + 1], bx = a.pattern[4 * i + 2], by = a.pattern[4 * i + 3];
      const bool bit = s_box[wave][(ay + 13) * kBox + ax + 13] < s_box[wave][(by + 13) * kBox + bx + 13];
      const unsigned long long m = __ballot(bit);   // bit `lane` of m is bit 64 k + lane of the descriptor
      if (lane == 2 * k) mine = (uint32_t)m;
      if (lane == 2 * k + 1) mine = (uint32_t)(m >> 32);
    }
    if (lane < 8) a.desc[(int64_t)f * 8 + lane] = mine;
  }
}

struct Job {   // one direction of one pair
  uint32_t q0, qn, c0, cn, out0, pad;
};

struct MatchArgs {
  const unsigned long long* desc;   // [N][4]
  const int32_t* ix; const int32_t* iy;
  const Job* jobs;
  int32_t max_shift, pad;
  int32_t* best_j;                  // per query: index within the other frame, -1 without a candidate
  uint32_t* best_d;                 // best | second << 16
};

__global__ __launch_bounds__(kThreads) void k_features_match(MatchArgs a) {
  __shared__ unsigned long long s_d[kThreads * 4];
  __shared__ int s_x[kThreads], s_y[kThreads];
  const Job job = a.jobs[blockIdx.y];
  if (blockIdx.x * kThreads >= job.qn) return;   // the same for the whole workgroup
  const int tid = threadIdx.x;
  const uint32_t q = blockIdx.x * kThreads + tid;
  const bool live = q < job.qn;
  const bool gate = a.max_shift > 0;
  unsigned long long d0 = 0, d1 = 0, d2 = 0, d3 = 0;
  int qx = 0, qy = 0;
  if (live) {
    const unsigned long long* p = a.desc + (int64_t)(job.q0 + q) * 4;
    d0 = p[0]; d1 = p[1]; d2 = p[2]; d3 = p[3];
    if (gate) { qx = a.ix[job.q0 + q]; qy = a.iy[job.q0 + q]; }
  }
  int best = kNoBest, second = kNoBest, arg = -1;
  for (uint32_t c = 0; c < job.cn; c += kThreads) {
    const uint32_t m = min((uint32_t)kThreads, job.cn - c);
    if ((uint32_t)tid < m) {
      const unsigned long long* p = a.desc + (int64_t)(job.c0 + c + tid) * 4;
      s_d[4 * tid] = p[0]; s_d[4 * tid + 1] = p[1]; s_d[4 * tid + 2] = p[2]; s_d[4 * tid + 3] = p[3];
      if (gate) { s_x[tid] = a.ix[job.c0 + c + tid]; s_y[tid] = a.iy[job.c0 + c + tid]; }
    }
    __syncthreads();
    if (live) {
      for (uint32_t j = 0; j < m; ++j) {
        if (gate && (abs(s_x[j] - qx) > a.max_shift || abs(s_y[j] - qy) > a.max_shift)) continue;
        const int d = __popcll(d0 ^ s_d[4 * j]) + __popcll(d1 ^ s_d[4 * j + 1]) + __popcll(d2 ^ s_d[4 * j + 2]) + __popcll(d3 ^ s_d[4 * j + 3]);
        if (d < best) { second = best; best = d; arg = (int)(c + j); }
        else if (d < second) second = d;
      }
    }
    __syncthreads();
  }
  if (live) {
    a.best_j[job.out0 + q] = arg;
    a.best_d[job.out0 + q] = (uint32_t)best | ((uint32_t)second << 16);
  }
}

// ------------------------------------------------------------------------------------------------ host side

static int fail_hip(const char* who, hipError_t e) { return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }

struct DeviceBuffers {
  std::vector<void*> q;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
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
  hipError_t upload(const T** out, const T* v, size_t n) {
    T* p = nullptr;
    hipError_t e = alloc(&p, n * sizeof(T));
    if (e == hipSuccess && n) e = hipMemcpy(p, v, n * sizeof(T), hipMemcpyHostToDevice);
    *out = p;
    return e;
  }
  hipError_t events() {
    for (hipEvent_t& e : ev)
      if (hipError_t rc = hipEventCreate(&e)) return rc;
    return hipSuccess;
  }
};

static bool set_device(int32_t device) {
  int n = 0;
  return device >= 0 && hipGetDeviceCount(&n) == hipSuccess && device < n && hipSetDevice(device) == hipSuccess;
}

}  // namespace features
}  // namespace lifcal

extern "C" {

using namespace lifcal::features;

int lifcal_features_check(const lifcal_rawdepth_image* image, const lifcal_features_options* options, lifcal_features_plan* plan) {
  DetectPlan t;
  if (int rc = make_detect_plan("lifcal_features_check", image, options, &t)) return rc;
  if (plan) {
    plan->options = t.opt;
    plan->buckets_x = t.bx; plan->buckets_y = t.by;
    plan->max_features = (int64_t)t.bx * t.by * t.opt.per_cell;
  }
  return 0;
}

int lifcal_features_pattern(int8_t* out) {
  if (!out) return fail(LIFCAL_BA_ERR_INVALID_ARG, "lifcal_features_pattern: no output");
  make_pattern(out);
  return 0;
}

int lifcal_features_detect(const lifcal_rawdepth_image* image, const uint8_t* status, int32_t device, const lifcal_features_options* options,
                           lifcal_features_list* out) {
  const char* who = "lifcal_features_detect";
  if (!out) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no result");
  DetectPlan t;
  if (int rc = make_detect_plan(who, image, options, &t)) return rc;
  out->n = 0; out->seconds = 0.0;
  if (!set_device(device)) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");
  if (t.bx == 0) return 0;   // too small for one patch: nothing to launch
  const int W = image->width, H = image->height;
  const size_t es = t.bits == 8 ? 1 : 2, nb = (size_t)t.bx * t.by, pc = (size_t)t.opt.per_cell;
  DeviceBuffers buf;
  DetectArgs a{};
  a.W = W; a.H = H; a.win_r = t.opt.win_r; a.nms_r = t.opt.nms_r; a.cell = t.opt.cell; a.per_cell = t.opt.per_cell; a.nbx = t.bx;
  a.min_score = t.opt.min_score;
  {
#pragma clang fp contract(off)
    const double full = t.bits == 8 ? 255.0 : 65535.0;
    a.full2 = full * full;
  }
  hipError_t e = hipSuccess;
  if (image->on_device) {
    a.img = image->data; a.pitch = image->pitch; a.status = status;
  } else {
    void* d = nullptr;
    e = buf.alloc(&d, (size_t)W * H * es);
    if (e == hipSuccess) e = hipMemcpy2D(d, W * es, image->data, (size_t)image->pitch * es, W * es, (size_t)H, hipMemcpyHostToDevice);
    a.img = d; a.pitch = W;
    if (e == hipSuccess && status) e = buf.upload(&a.status, status, (size_t)W * H);
  }
  if (e == hipSuccess) e = buf.alloc(&a.slots, nb * pc * sizeof(Slot));
  if (e == hipSuccess) e = buf.alloc(&a.count, nb * sizeof(int32_t));
  if (e == hipSuccess) e = buf.events();
  if (e != hipSuccess) return fail_hip(who, e);

  e = hipEventRecord(buf.ev[0], 0);
  const dim3 grd((unsigned)t.bx, (unsigned)t.by), blk(kThreads);
  if (t.bits == 8) hipLaunchKernelGGL((k_features_detect<uint8_t>), grd, blk, 0, 0, a);
  else hipLaunchKernelGGL((k_features_detect<uint16_t>), grd, blk, 0, 0, a);
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(buf.ev[1], 0);
  std::vector<int32_t> count(nb);
  std::vector<Slot> slots(nb * pc);
  if (e == hipSuccess) e = hipMemcpy(count.data(), a.count, nb * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(slots.data(), a.slots, nb * pc * sizeof(Slot), hipMemcpyDeviceToHost);
  float ms0 = 0.0f, ms1 = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms0, buf.ev[0], buf.ev[1]);
  if (e != hipSuccess) return fail_hip(who, e);
  // compact: buckets row-major, each in its kept order
  uint64_t n = 0;
  for (size_t b = 0; b < nb; ++b) {
    if (count[b] < 0 || count[b] > t.opt.per_cell) return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": a bucket reports an impossible count");
    n += (uint64_t)count[b];
  }
  out->n = n;
  out->seconds = 1.0e-3 * (double)ms0;
  if (out->capacity < n) return LIFCAL_MLA_MORE;
  if (n == 0) return 0;
  if (!out->x || !out->y || !out->ix || !out->iy || !out->score || !out->desc) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no output arrays");
  std::vector<int32_t> ix(n), iy(n);
  uint64_t k = 0;
  for (size_t b = 0; b < nb; ++b)
    for (int32_t r = 0; r < count[b]; ++r, ++k) {
      const Slot& s = slots[b * pc + (size_t)r];
      if (s.ix < kPatchR + 1 || s.ix > W - 2 - kPatchR || s.iy < kPatchR + 1 || s.iy > H - 2 - kPatchR)
        return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": a feature lies outside the candidate range");
      out->x[k] = s.x; out->y[k] = s.y; out->ix[k] = ix[k] = s.ix; out->iy[k] = iy[k] = s.iy; out->score[k] = s.score;
    }
  int8_t pattern[1024];
  make_pattern(pattern);
  DescribeArgs d{};
  d.n = (int32_t)n; d.pitch = a.pitch; d.img = a.img;
  e = buf.upload(&d.ix, ix.data(), n);
  if (e == hipSuccess) e = buf.upload(&d.iy, iy.data(), n);
  if (e == hipSuccess) e = buf.upload(&d.pattern, pattern, sizeof(pattern));
  if (e == hipSuccess) e = buf.alloc(&d.desc, n * 8 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipEventRecord(buf.ev[2], 0);
  if (e != hipSuccess) return fail_hip(who, e);
  const dim3 grd2((unsigned)((n + 3) / 4));
  if (t.bits == 8) hipLaunchKernelGGL((k_features_describe<uint8_t>), grd2, blk, 0, 0, d);
  else hipLaunchKernelGGL((k_features_describe<uint16_t>), grd2, blk, 0, 0, d);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(buf.ev[3], 0);
  if (e == hipSuccess) e = hipMemcpy(out->desc, d.desc, n * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms1, buf.ev[2], buf.ev[3]);
  if (e != hipSuccess) return fail_hip(who, e);
  out->seconds = 1.0e-3 * ((double)ms0 + (double)ms1);
  return 0;
}

int lifcal_features_match_check(const lifcal_features_set* set, uint32_t n_pairs, const uint32_t* pairs, const lifcal_match_options* options,
                                lifcal_match_options* resolved) {
  lifcal_match_options q;
  if (int rc = make_match_options("lifcal_features_match_check", set, n_pairs, pairs, options, &q)) return rc;
  if (resolved) *resolved = q;
  return 0;
}

int lifcal_features_match(const lifcal_features_set* set, uint32_t n_pairs, const uint32_t* pairs, int32_t device, const lifcal_match_options* options,
                          lifcal_match_list* out) {
  const char* who = "lifcal_features_match";
  if (!out) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no result");
  lifcal_match_options o;
  if (int rc = make_match_options(who, set, n_pairs, pairs, options, &o)) return rc;
  if (n_pairs && !out->pair_start) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no pair_start");
  out->n = 0; out->seconds = 0.0;
  if (!set_device(device)) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");
  const uint32_t* off = set->offset;
  const size_t N = off[set->n_frames];
  // two jobs per pair: a towards b, b towards a
  std::vector<Job> jobs(2 * (size_t)n_pairs);
  uint64_t total = 0;
  uint32_t max_q = 0;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const uint32_t fa = pairs[2 * p], fb = pairs[2 * p + 1];
    const uint32_t na = off[fa + 1] - off[fa], nb = off[fb + 1] - off[fb];
    if (total + na + nb >= (1ull << 31)) return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, std::string(who) + ": 2^31 queries and more in one call");
    jobs[2 * p] = Job{off[fa], na, off[fb], nb, (uint32_t)total, 0u};
    jobs[2 * p + 1] = Job{off[fb], nb, off[fa], na, (uint32_t)(total + na), 0u};
    total += (uint64_t)na + nb;
    max_q = std::max(max_q, std::max(na, nb));
  }
  std::vector<int32_t> best_j(total);
  std::vector<uint32_t> best_d(total);
  if (total > 0) {
    DeviceBuffers buf;
    MatchArgs a{};
    a.max_shift = o.max_shift;
    const uint32_t* d_desc = nullptr;
    hipError_t e = buf.upload(&d_desc, set->desc, N * 8);
    a.desc = (const unsigned long long*)d_desc;
    if (e == hipSuccess && o.max_shift > 0) e = buf.upload(&a.ix, set->ix, N);
    if (e == hipSuccess && o.max_shift > 0) e = buf.upload(&a.iy, set->iy, N);
    const Job* d_jobs = nullptr;
    if (e == hipSuccess) e = buf.upload(&d_jobs, jobs.data(), jobs.size());
    if (e == hipSuccess) e = buf.alloc(&a.best_j, total * sizeof(int32_t));
    if (e == hipSuccess) e = buf.alloc(&a.best_d, total * sizeof(uint32_t));
    if (e == hipSuccess) e = buf.events();
    if (e == hipSuccess) e = hipEventRecord(buf.ev[0], 0);
    if (e != hipSuccess) return fail_hip(who, e);
    const unsigned gx = (max_q + kThreads - 1) / kThreads;
    for (size_t j0 = 0; j0 < jobs.size() && gx > 0; j0 += 65535) {   // at most 65535 rows of workgroups per launch
      a.jobs = d_jobs + j0;
      hipLaunchKernelGGL(k_features_match, dim3(gx, (unsigned)std::min<size_t>(65535, jobs.size() - j0)), dim3(kThreads), 0, 0, a);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(buf.ev[1], 0);
    if (e == hipSuccess) e = hipMemcpy(best_j.data(), a.best_j, total * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(best_d.data(), a.best_d, total * sizeof(uint32_t), hipMemcpyDeviceToHost);
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, buf.ev[0], buf.ev[1]);
    if (e != hipSuccess) return fail_hip(who, e);
    out->seconds = 1.0e-3 * (double)ms;
  }
  // the mutual test, twice: to count, then to fill
  for (int pass = 0; pass < 2; ++pass) {
    uint64_t n = 0;
    for (uint32_t p = 0; p < n_pairs; ++p) {
      const Job &ja = jobs[2 * p], &jb = jobs[2 * p + 1];
      if (pass == 0) out->pair_start[p] = n;
      for (uint32_t i = 0; i < ja.qn; ++i) {
        const int32_t j = best_j[ja.out0 + i];
        if (j < 0 || (uint32_t)j >= jb.qn || best_j[jb.out0 + (uint32_t)j] != (int32_t)i) continue;
        const int64_t best = best_d[ja.out0 + i] & 0xffffu, second_i = best_d[ja.out0 + i] >> 16, second_j = best_d[jb.out0 + (uint32_t)j] >> 16;
        if (best > o.max_dist || !(o.ratio_den * best < o.ratio_num * second_i) || !(o.ratio_den * best < o.ratio_num * second_j)) continue;
        if (pass == 1) { out->i[n] = i; out->j[n] = (uint32_t)j; out->dist[n] = (uint32_t)best; }
        ++n;
      }
    }
    if (pass == 0) {
      if (n_pairs) out->pair_start[n_pairs] = n;
      out->n = n;
      if (out->capacity < n) return LIFCAL_MLA_MORE;
      if (n && (!out->i || !out->j || !out->dist)) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no output arrays");
    }
  }
  return 0;
}

int lifcal_tracks_link(uint32_t n_frames, const uint32_t* offset, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start,
                       const uint32_t* mi, const uint32_t* mj, lifcal_tracks* io) {
  return link_tracks(n_frames, offset, n_pairs, pairs, pair_start, mi, mj, io);
}

}  // extern "C"
