// verify_host.hpp — the part of include/lifcal_verify.h that needs no device: the argument checks, the
// usable lists, the sampler, the closed-form hypothesis and the inlier test as functions that the kernels of verify.hip and the
// host share, the choice of the best hypothesis, the refit loop over lifcal_align_fit (align.hpp) and the acceptance.  The two
// stages that run on the GPU come in as callables, so a stand-alone program with its own main (verify_host_check.cpp) can run
// everything else under the host sanitizers; it then defines lifcal::set_last_error itself.
#pragma once
#include <cfloat>

#include "features_host.hpp"

#include "../../include/lifcal_align.h"
#include "../../include/lifcal_verify.h"

#if defined(__HIPCC__)
#define LIFCAL_VERIFY_HD __host__ __device__ __forceinline__
#else
#define LIFCAL_VERIFY_HD inline
#endif

// every double operation below, and in what includes this header, stands alone: no fused multiply-add
#pragma clang fp contract(off)

namespace lifcal {
namespace verify {

using features::fail;

constexpr uint32_t kThreads = 256;          // hypotheses per workgroup
constexpr uint32_t kMaxHypotheses = 4096;
constexpr int kMaxRefine = 4;

struct Entry {       // one usable match, 64 bytes
  double a[3], b[3];   // its points in frame a and frame b
  double td, tl;       // the summed tolerances along and across the ray
};

struct Transform {
  double R[9], t[3];   // p_b ~ R p_a + t
};

// ------------------------------------------------------------------------------------------------ the rule (host and device)

LIFCAL_VERIFY_HD double rn_sqrt(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dsqrt_rn(x);
#else
  return std::sqrt(x);
#endif
}

LIFCAL_VERIFY_HD double rn_div(double x, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(x, y);
#else
  return x / y;
#endif
}

LIFCAL_VERIFY_HD bool is_finite(double x) { return fabs(x) <= DBL_MAX; }

LIFCAL_VERIFY_HD double dot3(const double* a, const double* b) {
#pragma clang fp contract(off)
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

LIFCAL_VERIFY_HD void cross3(const double* a, const double* b, double* o) {
#pragma clang fp contract(off)
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

LIFCAL_VERIFY_HD uint32_t draw(uint32_t& s, uint32_t m) {
  s = 1664525u * s + 1013904223u;
  return (uint32_t)(((uint64_t)s * m) >> 32);
}

// the three usable matches of hypothesis h of pair p; needs m >= 3
LIFCAL_VERIFY_HD void sample(uint32_t seed, uint32_t p, uint32_t h, uint32_t m, uint32_t k[3]) {
  uint32_t s = seed + 0x9E3779B9u * (p + 1u) + 0x85EBCA6Bu * (h + 1u);
  k[0] = draw(s, m);
  do k[1] = draw(s, m); while (k[1] == k[0]);
  do k[2] = draw(s, m); while (k[2] == k[0] || k[2] == k[1]);
}

// e[0..2] = e1, e[3..5] = e2, e[6..8] = e3, c = the centroid; false when the three points are (nearly) collinear
LIFCAL_VERIFY_HD bool triad(const double* q0, const double* q1, const double* q2, double* e, double* c) {
#pragma clang fp contract(off)
  double d1[3], d2[3], n[3];
  for (int k = 0; k < 3; ++k) { d1[k] = q1[k] - q0[k]; d2[k] = q2[k] - q0[k]; c[k] = rn_div((q0[k] + q1[k]) + q2[k], 3.0); }
  cross3(d1, d2, n);
  const double l1 = dot3(d1, d1), l2 = dot3(d2, d2), ln = dot3(n, n);
  if (!(ln > (1.0e-6 * l1) * l2)) return false;
  const double s1 = rn_sqrt(l1), sn = rn_sqrt(ln);
  for (int k = 0; k < 3; ++k) { e[k] = rn_div(d1[k], s1); e[6 + k] = rn_div(n[k], sn); }
  cross3(e + 6, e, e + 3);
  return true;
}

LIFCAL_VERIFY_HD bool make_transform(const Entry& x0, const Entry& x1, const Entry& x2, Transform* T) {
#pragma clang fp contract(off)
  double ea[9], eb[9], ca[3], cb[3];
  const bool oka = triad(x0.a, x1.a, x2.a, ea, ca);
  const bool okb = triad(x0.b, x1.b, x2.b, eb, cb);
  if (!oka || !okb) return false;
  bool ok = true;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      T->R[3 * r + c] = (eb[r] * ea[c] + eb[3 + r] * ea[3 + c]) + eb[6 + r] * ea[6 + c];
      ok = ok && is_finite(T->R[3 * r + c]);
    }
  for (int r = 0; r < 3; ++r) {
    T->t[r] = cb[r] - dot3(T->R + 3 * r, ca);
    ok = ok && is_finite(T->t[r]);
  }
  return ok;
}

LIFCAL_VERIFY_HD void ray(const double* pb, double* r) {
  const double l = rn_sqrt(dot3(pb, pb));
  for (int k = 0; k < 3; ++k) r[k] = rn_div(pb[k], l);
}

// the inlier test of one usable match; r = ray(pb)
LIFCAL_VERIFY_HD bool residual(const Transform& T, const double* pa, const double* pb, const double* r, double td, double tl, double* e_par,
                               double* e_perp) {
#pragma clang fp contract(off)
  double e[3];
  for (int k = 0; k < 3; ++k) e[k] = (dot3(T.R + 3 * k, pa) + T.t[k]) - pb[k];
  const double par = dot3(e, r);
  const double q = dot3(e, e) - par * par;
  const double perp = rn_sqrt(q > 0.0 ? q : 0.0);
  *e_par = par; *e_perp = perp;
  return fabs(par) <= td && perp <= tl;
}

// ------------------------------------------------------------------------------------------------ host only

static bool usable(const lifcal_verify_points* pts, uint32_t g) {
  const double* p = pts->xyz + 3 * (size_t)g;
  return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]) && std::isfinite(pts->tol_lat[g]) && std::isfinite(pts->tol_dep[g]) &&
         p[2] > 0.0 && pts->tol_lat[g] > 0.0 && pts->tol_dep[g] > 0.0;
}

// every check of lifcal_matches_verify; after it every index that the rest of the call forms lies inside its array
static int make_options(const char* who, const lifcal_verify_points* pts, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start,
                        const uint32_t* mi, const uint32_t* mj, const lifcal_verify_options* o, lifcal_verify_options* out) {
  const std::string w = std::string(who) + ": ";
  if (!pts) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no points");
  if (int rc = features::check_offsets(w, pts->n_frames, pts->offset)) return rc;
  if (pts->offset[pts->n_frames] > 0 && (!pts->xyz || !pts->tol_lat || !pts->tol_dep)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no coordinates or tolerances");
  if (int rc = features::check_pairs(w, pts->n_frames, n_pairs, pairs)) return rc;
  if (n_pairs && !pair_start) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no pair_start");
  for (uint32_t p = 0; p < n_pairs; ++p)
    if (pair_start[p + 1] < pair_start[p]) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "pair_start descends at pair " + std::to_string(p));
  if (n_pairs && pair_start[n_pairs] >= (1ull << 31)) return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "2^31 matches and more are not supported");
  if (n_pairs && pair_start[n_pairs] > pair_start[0] && (!mi || !mj)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no matches");
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const uint32_t a = pairs[2 * p], b = pairs[2 * p + 1];
    const uint32_t na = pts->offset[a + 1] - pts->offset[a], nb = pts->offset[b + 1] - pts->offset[b];
    for (uint64_t k = pair_start[p]; k < pair_start[p + 1]; ++k)
      if (mi[k] >= na || mj[k] >= nb) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "match " + std::to_string(k) + " names a feature out of range");
  }
  lifcal_verify_options q{};
  if (o) q = *o;
  if (q.hypotheses == 0) q.hypotheses = 256;
  if (q.min_inliers == 0) q.min_inliers = 8;
  if (q.refine == 0) q.refine = 2;
  if (q.refine < 0) q.refine = -1;
  if (q.min_ratio == 0.0) q.min_ratio = 0.25;
  if (q.hypotheses % kThreads != 0 || q.hypotheses > kMaxHypotheses) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "hypotheses must be a multiple of 256, up to 4096");
  if (q.min_inliers < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_inliers must be at least 1");
  if (q.refine > kMaxRefine) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "refine above 4");
  if (!(q.min_ratio >= 0.0 && q.min_ratio <= 1.0)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_ratio outside [0, 1]");
  if (out) *out = q;
  return 0;
}

// the usable matches of all pairs, pair after pair: pair p holds ustart[p] .. ustart[p + 1] - 1
struct Work {
  std::vector<Entry> entries;
  std::vector<uint64_t> match;     // per entry: its index in mi, mj
  std::vector<uint32_t> ustart;    // [n_pairs + 1]
  uint32_t max_m = 0;
  uint32_t m(uint32_t p) const { return ustart[p + 1] - ustart[p]; }
};

static void make_work(const lifcal_verify_points* pts, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start, const uint32_t* mi,
                      const uint32_t* mj, Work* w) {
  w->ustart.assign((size_t)n_pairs + 1, 0u);
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const uint32_t oa = pts->offset[pairs[2 * p]], ob = pts->offset[pairs[2 * p + 1]];
    for (uint64_t k = pair_start[p]; k < pair_start[p + 1]; ++k) {
      const uint32_t i = oa + mi[k], j = ob + mj[k];
      if (!usable(pts, i) || !usable(pts, j)) continue;
      Entry e;
      for (int c = 0; c < 3; ++c) { e.a[c] = pts->xyz[3 * (size_t)i + c]; e.b[c] = pts->xyz[3 * (size_t)j + c]; }
      e.td = pts->tol_dep[i] + pts->tol_dep[j];
      e.tl = pts->tol_lat[i] + pts->tol_lat[j];
      w->entries.push_back(e);
      w->match.push_back(k);
    }
    w->ustart[p + 1] = (uint32_t)w->entries.size();
    w->max_m = std::max(w->max_m, w->m(p));
  }
}

// what a classification writes, per entry
struct Classes {
  std::vector<uint8_t> keep;
  std::vector<double> e_par, e_perp;
  void resize(size_t n) { keep.assign(n, 0); e_par.assign(n, 0.0); e_perp.assign(n, 0.0); }
};

// score(work, H, seed, counts): counts[p * H + h] = the inliers of hypothesis h of pair p, -1 when it is invalid; only pairs with
// m >= 3 are written.  classify(work, T, active, out): the entries of every pair p with active[p] under T[p].  Both return a status.
template <class Score, class Classify>
static int run(const char* who, const lifcal_verify_points* pts, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start, const uint32_t* mi,
               const uint32_t* mj, const lifcal_verify_options& o, Score&& score, Classify&& classify, lifcal_verify_result* out) {
  const std::string w = std::string(who) + ": ";
  const uint64_t k_begin = n_pairs ? pair_start[0] : 0, k_end = n_pairs ? pair_start[n_pairs] : 0;
  if (k_end > k_begin && (!out->keep || !out->e_par || !out->e_perp)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no output arrays");
  if (n_pairs && !out->pair) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no pair rows");
  Work work;
  make_work(pts, n_pairs, pairs, pair_start, mi, mj, &work);
  const double nan = std::nan("");
  for (uint64_t k = k_begin; k < k_end; ++k) { out->keep[k] = 0; out->e_par[k] = nan; out->e_perp[k] = nan; }
  std::vector<uint8_t> active(n_pairs, 0);
  bool any = false;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    lifcal_verify_pair row{};
    row.status = LIFCAL_VERIFY_FEW;
    row.n_matches = (uint32_t)(pair_start[p + 1] - pair_start[p]);
    row.n_usable = work.m(p);
    row.best_hypothesis = LIFCAL_VERIFY_NO_HYPOTHESIS;
    out->pair[p] = row;
    if (work.m(p) >= 3) { active[p] = 1; any = true; }
  }
  if (!any) return 0;
  const uint32_t H = o.hypotheses;
  std::vector<int32_t> counts((size_t)n_pairs * H, -1);
  if (int rc = score(work, H, o.seed, counts)) return rc;
  std::vector<Transform> T(n_pairs), Tn(n_pairs);
  for (uint32_t p = 0; p < n_pairs; ++p) {
    if (!active[p]) continue;
    lifcal_verify_pair& row = out->pair[p];
    int32_t best = -1;
    for (uint32_t h = 0; h < H; ++h) {
      const int32_t c = counts[(size_t)p * H + h];
      if (c < -1 || (uint32_t)(c + 1) > work.m(p) + 1u) return fail(LIFCAL_BA_ERR_HIP, w + "a hypothesis reports an impossible count");
      if (c > best) { best = c; row.best_hypothesis = h; }
    }
    if (best < 0) { row.status = LIFCAL_VERIFY_DEGENERATE; active[p] = 0; continue; }
    row.n_inliers_hypothesis = (uint32_t)best;
    uint32_t k[3];
    sample(o.seed, p, row.best_hypothesis, work.m(p), k);
    const Entry* e = work.entries.data() + work.ustart[p];
    if (!make_transform(e[k[0]], e[k[1]], e[k[2]], &T[p])) return fail(LIFCAL_BA_ERR_HIP, w + "the best hypothesis is not valid on the host");
  }
  Classes cur, nxt;
  cur.resize(work.entries.size()); nxt.resize(work.entries.size());
  if (int rc = classify(work, T, active, cur)) return rc;
  std::vector<uint32_t> n_in(n_pairs, 0u);
  auto count = [&work](const Classes& c, uint32_t p) {
    uint32_t n = 0;
    for (uint32_t u = work.ustart[p]; u < work.ustart[p + 1]; ++u) n += c.keep[u] ? 1u : 0u;
    return n;
  };
  for (uint32_t p = 0; p < n_pairs; ++p) {
    if (!active[p]) continue;
    n_in[p] = count(cur, p);
    if (n_in[p] != out->pair[p].n_inliers_hypothesis) return fail(LIFCAL_BA_ERR_HIP, w + "scoring and classification disagree on pair " + std::to_string(p));
  }
  // the refit rounds: all pairs that still refine go through one classification per round
  std::vector<uint8_t> refining(active);
  std::vector<double> from, to, wt;
  for (int round = 0; round < o.refine; ++round) {
    bool some = false;
    for (uint32_t p = 0; p < n_pairs; ++p) {
      if (!refining[p]) continue;
      from.clear(); to.clear(); wt.clear();
      for (uint32_t u = work.ustart[p]; u < work.ustart[p + 1]; ++u) {
        if (!cur.keep[u]) continue;
        const Entry& e = work.entries[u];
        for (int c = 0; c < 3; ++c) { from.push_back(e.a[c]); to.push_back(e.b[c]); }
        wt.push_back(1.0 / (e.td * e.td));
      }
      lifcal_alignment al{};
      if (lifcal_align_fit((uint32_t)wt.size(), from.data(), to.data(), wt.data(), 0, &al) != 0) { refining[p] = 0; continue; }
      for (int c = 0; c < 9; ++c) Tn[p].R[c] = al.R[c];
      for (int c = 0; c < 3; ++c) Tn[p].t[c] = al.t[c];
      some = true;
    }
    if (!some) break;
    if (int rc = classify(work, Tn, refining, nxt)) return rc;
    for (uint32_t p = 0; p < n_pairs; ++p) {
      if (!refining[p]) continue;
      const uint32_t n = count(nxt, p);
      if (n < n_in[p]) { refining[p] = 0; continue; }
      n_in[p] = n; T[p] = Tn[p]; ++out->pair[p].rounds_used;
      for (uint32_t u = work.ustart[p]; u < work.ustart[p + 1]; ++u) { cur.keep[u] = nxt.keep[u]; cur.e_par[u] = nxt.e_par[u]; cur.e_perp[u] = nxt.e_perp[u]; }
    }
  }
  for (uint32_t p = 0; p < n_pairs; ++p) {
    if (!active[p]) continue;
    lifcal_verify_pair& row = out->pair[p];
    const uint32_t n = n_in[p], m = work.m(p);
    row.n_inliers = n;
    for (int c = 0; c < 9; ++c) row.R[c] = T[p].R[c];
    for (int c = 0; c < 3; ++c) row.t[c] = T[p].t[c];
    const bool ok = n >= (uint32_t)o.min_inliers && !((double)n < o.min_ratio * (double)m);
    row.status = ok ? LIFCAL_VERIFY_OK : LIFCAL_VERIFY_REJECTED;
    double S = 0.0;
    for (uint32_t u = work.ustart[p]; u < work.ustart[p + 1]; ++u) {
      const uint64_t k = work.match[u];
      out->e_par[k] = cur.e_par[u]; out->e_perp[k] = cur.e_perp[u];
      out->keep[k] = (ok && cur.keep[u]) ? 1 : 0;
      if (cur.keep[u]) S += cur.e_par[u] * cur.e_par[u] + cur.e_perp[u] * cur.e_perp[u];
    }
    row.rms = n ? std::sqrt(S / (double)n) : 0.0;
  }
  return 0;
}

}  // namespace verify
}  // namespace lifcal
