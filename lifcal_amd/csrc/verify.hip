// verify.hip — geometric verification of feature matches (include/lifcal_verify.h), in a code object of its
// own like features.hip (raw_depth.hpp says why).
//
// What runs where.  k_verify_score: a workgroup takes 256 hypotheses of one pair.  Every thread samples its three usable matches,
// builds its rigid transform in closed form and keeps the 12 doubles in registers; the workgroup then streams the pair's usable
// matches through LDS in tiles (a tile entry: p_a, p_b, the two summed tolerances, and the unit ray of p_b, which is the same for
// every hypothesis and so is computed once per entry while the tile is staged); every lane reads the same LDS address (a
// broadcast) and counts in a register; one count per hypothesis goes out by a plain store.  No atomics.  k_verify_classify: one
// thread per usable match under its pair's current transform; it serves the hypothesis stage's result and every refit.
// Sampling, the triad and the inlier test are the functions of verify_host.hpp, shared with the host, which picks the best
// hypothesis, refits (lifcal_align_fit) and applies the acceptance rule.  Every floating-point step is an IEEE double operation
// without fused multiply-add; square roots and divisions are the correctly rounded ones.
#include <hip/hip_runtime.h>

#include "verify_host.hpp"

namespace lifcal {
namespace verify {

constexpr uint32_t kTile = 256;     // usable matches per LDS tile
constexpr uint32_t kTileDoubles = 11;   // a[3], b[3], td, tl, ray[3]

// ------------------------------------------------------------------------------------------------ device side

struct ScoreArgs {
  const Entry* entries;      // the usable matches of all pairs
  const uint32_t* ustart;    // [n_pairs + 1]
  const uint32_t* rows;      // the pairs with at least three usable matches: one row of workgroups each
  int32_t* counts;           // [n_pairs][H]
  uint32_t row0, H, seed, pad;
};

__global__ __launch_bounds__(kThreads) void k_verify_score(ScoreArgs a) {
  __shared__ double s_e[kTile * kTileDoubles];
  const uint32_t p = a.rows[a.row0 + blockIdx.y];
  const uint32_t u0 = a.ustart[p], m = a.ustart[p + 1] - u0;
  if (m < 3) return;   // the same for the whole workgroup; the host lists no such pair
  const uint32_t tid = threadIdx.x, h = blockIdx.x * kThreads + tid;
  const Entry* __restrict__ E = a.entries + u0;
  uint32_t k[3];
  sample(a.seed, p, h, m, k);   // every k < m
  Transform T;
  const bool valid = make_transform(E[k[0]], E[k[1]], E[k[2]], &T);
  int32_t count = 0;
  for (uint32_t c = 0; c < m; c += kTile) {
    const uint32_t n = min(kTile, m - c);   // the last tile is guarded by the count
    if (tid < n) {
      const Entry e = E[c + tid];
      double* s = s_e + tid * kTileDoubles;
      double r[3];
      ray(e.b, r);
      s[0] = e.a[0]; s[1] = e.a[1]; s[2] = e.a[2]; s[3] = e.b[0]; s[4] = e.b[1]; s[5] = e.b[2]; s[6] = e.td; s[7] = e.tl;
      s[8] = r[0]; s[9] = r[1]; s[10] = r[2];
    }
    __syncthreads();
    if (valid) {
      for (uint32_t j = 0; j < n; ++j) {
        const double* s = s_e + j * kTileDoubles;
        double e_par, e_perp;
        count += residual(T, s, s + 3, s + 8, s[6], s[7], &e_par, &e_perp) ? 1 : 0;
      }
    }
    __syncthreads();
  }
  a.counts[(size_t)p * a.H + h] = valid ? count : -1;
}

struct ClassifyArgs {
  const Entry* entries;
  const uint32_t* ustart;      // [n_pairs + 1]
  const Transform* T;          // [n_pairs]
  const uint32_t* rows;        // the pairs to classify: one row of workgroups each
  uint8_t* keep;               // per entry
  double* e_par;
  double* e_perp;
  uint32_t row0, pad;
};

__global__ __launch_bounds__(kThreads) void k_verify_classify(ClassifyArgs a) {
  const uint32_t p = a.rows[a.row0 + blockIdx.y];
  const uint32_t u0 = a.ustart[p], m = a.ustart[p + 1] - u0;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= m) return;
  const Transform T = a.T[p];
  const Entry e = a.entries[u0 + i];
  double r[3], e_par, e_perp;
  ray(e.b, r);
  const bool in = residual(T, e.a, e.b, r, e.td, e.tl, &e_par, &e_perp);
  a.keep[u0 + i] = in ? 1 : 0;
  a.e_par[u0 + i] = e_par;
  a.e_perp[u0 + i] = e_perp;
}

// ------------------------------------------------------------------------------------------------ host side

static int fail_hip(const char* who, hipError_t e) { return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }

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
  hipError_t upload(const T** out, const T* v, size_t n) {
    T* p = nullptr;
    hipError_t e = alloc(&p, n * sizeof(T));
    if (e == hipSuccess && n) e = hipMemcpy(p, v, n * sizeof(T), hipMemcpyHostToDevice);
    *out = p;
    return e;
  }
};

static bool set_device(int32_t device) {
  int n = 0;
  return device >= 0 && hipGetDeviceCount(&n) == hipSuccess && device < n && hipSetDevice(device) == hipSuccess;
}

constexpr uint32_t kMaxRows = 65535;   // rows of workgroups per launch

// the device's copy of the usable matches and the two stages over it
struct Device {
  const char* who;
  DeviceBuffers buf;
  const Entry* entries = nullptr;
  const uint32_t* ustart = nullptr;
  Transform* T = nullptr;
  uint32_t* rows = nullptr;
  uint8_t* keep = nullptr;
  double* e_par = nullptr;
  double* e_perp = nullptr;
  bool ready = false;
  double ms = 0.0;

  int prepare(const Work& w, uint32_t n_pairs) {
    if (ready) return 0;
    const size_t U = w.entries.size();
    hipError_t e = buf.upload(&entries, w.entries.data(), U);
    if (e == hipSuccess) e = buf.upload(&ustart, w.ustart.data(), w.ustart.size());
    if (e == hipSuccess) e = buf.alloc(&T, n_pairs * sizeof(Transform));
    if (e == hipSuccess) e = buf.alloc(&rows, n_pairs * sizeof(uint32_t));
    if (e == hipSuccess) e = buf.alloc(&keep, U);
    if (e == hipSuccess) e = buf.alloc(&e_par, U * sizeof(double));
    if (e == hipSuccess) e = buf.alloc(&e_perp, U * sizeof(double));
    for (hipEvent_t& v : buf.ev)
      if (e == hipSuccess) e = hipEventCreate(&v);
    if (e != hipSuccess) return fail_hip(who, e);
    ready = true;
    return 0;
  }

  int finish(hipError_t e) {
    float t = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&t, buf.ev[0], buf.ev[1]);
    if (e != hipSuccess) return fail_hip(who, e);
    ms += (double)t;
    return 0;
  }

  int score(const Work& w, uint32_t H, uint32_t seed, std::vector<int32_t>& counts) {
    const uint32_t n_pairs = (uint32_t)w.ustart.size() - 1;
    if (int rc = prepare(w, n_pairs)) return rc;
    std::vector<uint32_t> list;
    for (uint32_t p = 0; p < n_pairs; ++p)
      if (w.m(p) >= 3) list.push_back(p);
    if (list.empty()) return 0;
    const uint32_t n_rows = (uint32_t)list.size();
    ScoreArgs a{};
    a.entries = entries; a.ustart = ustart; a.rows = rows; a.H = H; a.seed = seed;
    hipError_t e = buf.alloc(&a.counts, counts.size() * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(rows, list.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a.counts, counts.data(), counts.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventRecord(buf.ev[0], 0);
    if (e != hipSuccess) return fail_hip(who, e);
    for (uint32_t r0 = 0; r0 < n_rows; r0 += kMaxRows) {
      a.row0 = r0;
      hipLaunchKernelGGL(k_verify_score, dim3(H / kThreads, std::min(kMaxRows, n_rows - r0)), dim3(kThreads), 0, 0, a);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(buf.ev[1], 0);
    if (e == hipSuccess) e = hipMemcpy(counts.data(), a.counts, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
    return finish(e);
  }

  int classify(const Work& w, const std::vector<Transform>& Th, const std::vector<uint8_t>& act, Classes& out) {
    const uint32_t n_pairs = (uint32_t)w.ustart.size() - 1;
    if (int rc = prepare(w, n_pairs)) return rc;
    const size_t U = w.entries.size();
    uint32_t max_m = 0;
    std::vector<uint32_t> list;
    for (uint32_t p = 0; p < n_pairs; ++p)
      if (act[p] && w.m(p) > 0) { max_m = std::max(max_m, w.m(p)); list.push_back(p); }
    if (list.empty()) return 0;
    const uint32_t n_rows = (uint32_t)list.size();
    ClassifyArgs a{};
    a.entries = entries; a.ustart = ustart; a.T = T; a.rows = rows; a.keep = keep; a.e_par = e_par; a.e_perp = e_perp;
    hipError_t e = hipMemcpy(T, Th.data(), n_pairs * sizeof(Transform), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(rows, list.data(), n_rows * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipEventRecord(buf.ev[0], 0);
    if (e != hipSuccess) return fail_hip(who, e);
    for (uint32_t r0 = 0; r0 < n_rows; r0 += kMaxRows) {
      a.row0 = r0;
      hipLaunchKernelGGL(k_verify_classify, dim3((max_m + kThreads - 1) / kThreads, std::min(kMaxRows, n_rows - r0)), dim3(kThreads), 0, 0, a);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(buf.ev[1], 0);
    // entries of pairs that are not active keep what an earlier round wrote; run() reads the active ones only
    if (e == hipSuccess) e = hipMemcpy(out.keep.data(), keep, U, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out.e_par.data(), e_par, U * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(out.e_perp.data(), e_perp, U * sizeof(double), hipMemcpyDeviceToHost);
    return finish(e);
  }
};

}  // namespace verify
}  // namespace lifcal

extern "C" {

using namespace lifcal::verify;

int lifcal_matches_verify_check(const lifcal_verify_points* pts, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start,
                                const uint32_t* mi, const uint32_t* mj, const lifcal_verify_options* options, lifcal_verify_options* resolved) {
  return make_options("lifcal_matches_verify_check", pts, n_pairs, pairs, pair_start, mi, mj, options, resolved);
}

int lifcal_matches_verify(const lifcal_verify_points* pts, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start,
                          const uint32_t* mi, const uint32_t* mj, int32_t device, const lifcal_verify_options* opt, lifcal_verify_result* out) {
  const char* who = "lifcal_matches_verify";
  if (!out) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no result");
  lifcal_verify_options o;
  if (int rc = make_options(who, pts, n_pairs, pairs, pair_start, mi, mj, opt, &o)) return rc;
  out->seconds = 0.0;
  if (!set_device(device)) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");
  Device dev{who};
  const int rc = run(
      who, pts, n_pairs, pairs, pair_start, mi, mj, o,
      [&dev](const Work& w, uint32_t H, uint32_t seed, std::vector<int32_t>& counts) { return dev.score(w, H, seed, counts); },
      [&dev](const Work& w, const std::vector<Transform>& T, const std::vector<uint8_t>& active, Classes& c) { return dev.classify(w, T, active, c); }, out);
  out->seconds = 1.0e-3 * dev.ms;
  return rc;
}

}  // extern "C"
