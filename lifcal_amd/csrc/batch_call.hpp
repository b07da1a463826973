// batch_call.hpp — the host side the one-call routes share: lifcal_resect_frames, lifcal_intersect_points, lifcal_start_poses,
// lifcal_start_points, lifcal_register_scene (included by lifcal_ba.hip in front of resection.hpp).  DESIGN.md section 7o.
// A route checks its arguments (batch_checks), answers what needs no device, sorts (lifcal_group_index, frame_point_order,
// build_groups), lays one device block out (ByteLayout), stages it in one host vector (stage_observations), and only then selects
// the device and runs its kernels inside one BatchCall.  No kernel lives here.
#pragma once
#include "../../include/lifcal_ba.h"

namespace lifcal {
template <int NR, bool TAN>
__global__ __launch_bounds__(256) void k_resect_lens(const double* cam, double spx, double spy, double scale, double loss_scale, int fold, uint32_t n,
                              const double* __restrict__ mcx, const double* __restrict__ mcy, CamConsts* camc_out, double* __restrict__ cu_out);   // resection.hpp
}  // namespace lifcal

namespace {

// a byte layout of consecutive 256-byte aligned sections
struct ByteLayout {
  size_t bytes = 0;
  size_t take(size_t n) { const size_t at = bytes; bytes += (n + 255) & ~(size_t)255; return at; }
};

// Stream, device block and events of one call, and the first HIP error of the call: after an error every operation is a no-op.
// Declared behind the host vectors the queued copies read or write, so that it goes first: the destructor waits for the stream
// if anything is still queued (an error, or a dispatch table that refused the configuration), then releases everything.
struct BatchCall {
  const int device;
  const char* const name;   // the entry point, for the message of a failed call
  hipStream_t stream = nullptr;
  unsigned char* dev = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipError_t err = hipSuccess;
  bool queued = false;      // kernels go to `stream` directly, so only finish() knows that nothing is left
  BatchCall(int d, const char* n) : device(d), name(n), stream(stream_pool_take(d)) {}
  BatchCall(const BatchCall&) = delete;
  BatchCall& operator=(const BatchCall&) = delete;
  ~BatchCall() {
    if (queued && stream) (void)hipStreamSynchronize(stream);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (dev) (void)hipFree(dev);
    if (stream && !stream_pool_give(device, stream)) (void)hipStreamDestroy(stream);
  }
  bool ok() const { return err == hipSuccess; }
  void open(size_t bytes) {
    if (!stream) err = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
    if (ok()) err = hipMalloc((void**)&dev, bytes);
    if (ok()) err = hipEventCreate(&ev0);
    if (ok()) err = hipEventCreate(&ev1);
  }
  void upload(const void* host, size_t n) { if (ok()) { queued = true; err = hipMemcpyAsync(dev, host, n, hipMemcpyHostToDevice, stream); } }
  void zero(size_t at, size_t n) { if (ok()) { queued = true; err = hipMemsetAsync(dev + at, 0, n, stream); } }
  void download(void* dst, size_t at, size_t n) { if (ok()) { queued = true; err = hipMemcpyAsync(dst, dev + at, n, hipMemcpyDeviceToHost, stream); } }
  void launched() { if (ok()) err = hipGetLastError(); }   // behind a group of kernel launches
  void begin() { if (ok()) err = hipEventRecord(ev0, stream); }
  void end() { launched(); if (ok()) err = hipEventRecord(ev1, stream); }
  int fail() { g_last_error = std::string(name) + ": " + hipGetErrorString(err); return LIFCAL_BA_ERR_HIP; }
  // the host reads what was downloaded so far and the call goes on
  int wait() {
    if (ok()) err = hipStreamSynchronize(stream);
    return ok() ? 0 : fail();
  }
  // always synchronises (queued copies read the host vectors), then the time between begin() and end()
  int finish(double* seconds) {
    const hipError_t es = stream ? hipStreamSynchronize(stream) : hipSuccess;
    queued = false;
    if (ok()) err = es;
    float ms = 0.f;
    if (ok()) err = hipEventElapsedTime(&ms, ev0, ev1);
    if (!ok()) return fail();
    if (seconds) *seconds = 1e-3 * (double)ms;
    return 0;
  }
};

// the argument checks of every route (the problem structs name their fields alike); limit_points: lifcal_resect_frames alone
// never had the n_points limit
template <class Problem>
int batch_checks(const char* fn, const Problem* p, const lifcal_ba_options* o, const void* rows, bool limit_points) {
  const std::string name(fn);
  if (!p || !o || !rows) { g_last_error = name + ": null problem, options or output rows"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (o->world_size > 1) { g_last_error = name + ": world_size > 1 is not supported"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (o->precision != 0) { g_last_error = name + ": options.precision must be 0"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (!p->cam || (p->n_frames && !p->views) || (p->n_points && !p->pts) ||
      (p->n_obs && (!p->u || !p->v || !p->mcx || !p->mcy || !p->pt || !p->fr))) {
    g_last_error = name + ": null array in the problem"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
  if (p->n_obs > 0xFFFF0000u) { g_last_error = name + ": too many observations for 32-bit positions"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (limit_points && p->n_points > 0xFFFF0000u) { g_last_error = name + ": too many points for 32-bit positions"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if ((p->config & LIFCAL_BA_CFG_NRADIAL_MASK) > 2u) { g_last_error = name + ": more than two radial coefficients"; return LIFCAL_BA_ERR_INVALID_ARG; }
  for (uint32_t i = 0; i < p->n_obs; ++i)
    if (p->pt[i] >= p->n_points || p->fr[i] >= p->n_frames) {
      g_last_error = name + ": observation " + std::to_string(i) + " names point " + std::to_string(p->pt[i]) + " / frame " + std::to_string(p->fr[i]) + " out of range";
      return LIFCAL_BA_ERR_OUT_OF_RANGE;
    }
  return 0;
}

// the model bits of a problem's config in the shape DISPATCH_CFG and DISPATCH_LENS read: the same dispatch tables as the handle's
// kernels, on the bits of the config instead of a plan
struct ModelCfg { struct { int n_radial; bool tangential, adj; } plan; };
ModelCfg model_cfg(uint32_t config) {
  return ModelCfg{{(int)(config & LIFCAL_BA_CFG_NRADIAL_MASK), (config & LIFCAL_BA_CFG_TANGENTIAL) != 0, (config & LIFCAL_BA_CFG_ML_CENTER_ADJ) != 0}};
}

// one k_resect_lens launch over N observations: c_u into cu_out, the camera constants into camc[0] for the folded parameters
// (fold 1, the solve) and into camc[1] for the parameters as stored (fold 0, the error sums)
int launch_lens_pass(const ModelCfg& cfg, hipStream_t stream, uint32_t grid, const double* cam, double spx, double spy, double scale, double loss_scale,
                     int fold, uint32_t N, const double* mx, const double* my, CamConsts* camc, double* cu_out) {
#define CALL_LENS_PASS(NR, TAN) hipLaunchKernelGGL((k_resect_lens<NR, TAN>), dim3(grid), dim3(256), 0, stream, cam, spx, spy, scale, loss_scale, fold, N, mx, my, camc + (fold ? 0 : 1), cu_out)
  DISPATCH_LENS(&cfg, CALL_LENS_PASS);
#undef CALL_LENS_PASS
  return 0;
}

// u, v, mcx, mcy of the observations in the order idx into the sections of the staging vector, and key[] (p->pt or p->fr; null:
// none) likewise into the section at_key
template <class Problem>
void stage_observations(std::vector<unsigned char>& host, const std::vector<uint32_t>& idx, uint32_t N, const Problem* p,
                        size_t at_u, size_t at_v, size_t at_mx, size_t at_my, size_t at_key, const uint32_t* key) {
  double *hu = (double*)(host.data() + at_u), *hv = (double*)(host.data() + at_v), *hmx = (double*)(host.data() + at_mx), *hmy = (double*)(host.data() + at_my);
  uint32_t* hk = key ? (uint32_t*)(host.data() + at_key) : nullptr;
  for (uint32_t k = 0; k < N; ++k) { const uint32_t i = idx[k]; hu[k] = p->u[i]; hv[k] = p->v[i]; hmx[k] = p->mcx[i]; hmy[k] = p->mcy[i]; if (hk) hk[k] = key[i]; }
}

// the observations (fr, pt)-major, inside a group in the caller's order: the point-major order pidx (a stable counting sort by pt)
// sorted again, stably, by fr.  off [F + 1]: the CSR of the observations by frame.
int frame_point_order(uint32_t N, uint32_t F, const uint32_t* fr, const std::vector<uint32_t>& pidx, uint32_t* off, std::vector<uint32_t>& idx) {
  std::vector<uint32_t> key2(N), idx2(N);
  for (uint32_t k = 0; k < N; ++k) key2[k] = fr[pidx[k]];
  if (int rc = lifcal_group_index(N, F, key2.data(), off, idx2.data())) return rc;
  for (uint32_t k = 0; k < N; ++k) idx[k] = pidx[idx2[k]];
  return 0;
}

// the groups of an (fr, pt)-major order: runs of equal (fr, pt), goff [G + 1] their positions, gfr, gpt [G] their keys; fgoff
// [F + 1] per frame its run of groups
struct Groups {
  std::vector<uint32_t> goff, gfr, gpt, fgoff;
  uint32_t G = 0;
};
Groups build_groups(uint32_t N, uint32_t F, const uint32_t* fr, const uint32_t* pt, const std::vector<uint32_t>& idx) {
  Groups g;
  g.fgoff.assign((size_t)F + 1, 0u);
  for (uint32_t k = 0; k < N; ++k) {
    const uint32_t f = fr[idx[k]], q = pt[idx[k]];
    if (k == 0 || f != g.gfr.back() || q != g.gpt.back()) { g.goff.push_back(k); g.gfr.push_back(f); g.gpt.push_back(q); ++g.fgoff[(size_t)f + 1]; }
  }
  g.goff.push_back(N);
  g.G = (uint32_t)g.gfr.size();
  for (uint32_t f = 0; f < F; ++f) g.fgoff[(size_t)f + 1] += g.fgoff[f];
  return g;
}

// no exception crosses the C ABI
template <class Fn>
int guard_abi(const char* name, Fn fn) {
  try {
    return fn();
  } catch (const std::bad_alloc&) {
    g_last_error = std::string(name) + ": out of host memory"; return LIFCAL_BA_ERR_NOMEM;
  } catch (...) {
    g_last_error = std::string(name) + ": unexpected exception"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
}

}  // namespace
