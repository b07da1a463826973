// verify_host_check.cpp — the host-only part of include/lifcal_verify.h (verify_host.hpp) as a stand-alone program, so that the
// argument checks, the sampler, the closed-form hypothesis, the choice, the refit loop over lifcal_align_fit (align.hpp itself, not
// a copy) and the acceptance can run under the host sanitizers:
//   make -C lifcal_amd/csrc verify_host_check && lifcal_amd/csrc/verify_host_check
// (the target compiles with -fsanitize=address,undefined).  No HIP, no device, no Python.  The two stages that the library runs
// on the GPU are stood in for by host loops over the same functions.  Every array is allocated at its exact size so that a read
// or write past an end is caught.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/lifcal_ba.h"
#include "../../include/lifcal_align.h"

static thread_local std::string g_last_error;   // what align.hpp and colmap.hpp report into (lifcal_ba.hip has its own)
#include "sym_eig.hpp"
#include "colmap.hpp"
#include "align.hpp"

#include "verify_host.hpp"

namespace lifcal {
void set_last_error(const char* text) { g_last_error = text; }
}  // namespace lifcal

using namespace lifcal::verify;
using U = std::vector<uint32_t>;
using D = std::vector<double>;

static int g_failed = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
  } while (0)

static uint32_t g_state = 2463534242u;
static uint32_t rnd(uint32_t n) { g_state = 1664525u * g_state + 1013904223u; return (uint32_t)(((uint64_t)g_state * n) >> 32); }
static double uni(double lo, double hi) { return lo + (hi - lo) * ((double)rnd(1u << 24) / (double)(1u << 24)); }

// the stand-ins of k_verify_score and k_verify_classify
static int host_score(const Work& w, uint32_t H, uint32_t seed, std::vector<int32_t>& counts) {
  const uint32_t n_pairs = (uint32_t)w.ustart.size() - 1;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const uint32_t m = w.m(p);
    if (m < 3) continue;
    const Entry* E = w.entries.data() + w.ustart[p];
    for (uint32_t h = 0; h < H; ++h) {
      uint32_t k[3];
      sample(seed, p, h, m, k);
      EXPECT(k[0] < m && k[1] < m && k[2] < m && k[0] != k[1] && k[0] != k[2] && k[1] != k[2]);
      Transform T;
      if (!make_transform(E[k[0]], E[k[1]], E[k[2]], &T)) { counts[(size_t)p * H + h] = -1; continue; }
      int32_t c = 0;
      for (uint32_t j = 0; j < m; ++j) {
        double r[3], a, b;
        ray(E[j].b, r);
        c += residual(T, E[j].a, E[j].b, r, E[j].td, E[j].tl, &a, &b) ? 1 : 0;
      }
      counts[(size_t)p * H + h] = c;
    }
  }
  return 0;
}

static int host_classify(const Work& w, const std::vector<Transform>& T, const std::vector<uint8_t>& active, Classes& out) {
  const uint32_t n_pairs = (uint32_t)w.ustart.size() - 1;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    if (!active[p]) continue;
    for (uint32_t u = w.ustart[p]; u < w.ustart[p + 1]; ++u) {
      const Entry& e = w.entries[u];
      double r[3];
      ray(e.b, r);
      out.keep[u] = residual(T[p], e.a, e.b, r, e.td, e.tl, &out.e_par[u], &out.e_perp[u]) ? 1 : 0;
    }
  }
  return 0;
}

struct Case {
  U offset{0}, pairs, mi, mj;
  std::vector<uint64_t> start{0};
  D xyz, tol_lat, tol_dep;
  uint32_t add_frame(const D& p) {   // p: [n][3]; the tolerances of the test scenes
    for (size_t i = 0; i < p.size() / 3; ++i) {
      const double z = p[3 * i + 2];
      tol_lat.push_back(1.0e-3 * z); tol_dep.push_back(2.0e-6 * z * z);
    }
    xyz.insert(xyz.end(), p.begin(), p.end());
    offset.push_back((uint32_t)(xyz.size() / 3));
    return (uint32_t)offset.size() - 2;
  }
};

struct Run {
  int rc = 0;
  std::vector<uint8_t> keep;
  D e_par, e_perp;
  std::vector<lifcal_verify_pair> rows;
};

static Run verify(const Case& c, const lifcal_verify_options* opt) {
  const uint32_t n_pairs = (uint32_t)(c.pairs.size() / 2);
  lifcal_verify_points pts{(uint32_t)c.offset.size() - 1, 0, c.offset.data(), c.xyz.data(), c.tol_lat.data(), c.tol_dep.data()};
  Run r;
  lifcal_verify_options o{};
  r.rc = make_options("check", &pts, n_pairs, c.pairs.data(), c.start.data(), c.mi.data(), c.mj.data(), opt, &o);
  if (r.rc) return r;
  const size_t n = (size_t)c.start.back();
  r.keep.resize(n); r.e_par.resize(n); r.e_perp.resize(n); r.rows.resize(n_pairs);
  lifcal_verify_result out{r.keep.data(), r.e_par.data(), r.e_perp.data(), r.rows.data(), 0.0};
  r.rc = run("check", &pts, n_pairs, c.pairs.data(), c.start.data(), c.mi.data(), c.mj.data(), o, host_score, host_classify, &out);
  return r;
}

static D cloud(uint32_t n) {
  D p;
  for (uint32_t i = 0; i < n; ++i) { const double z = uni(300.0, 1500.0); p.push_back(z * uni(-0.3, 0.3)); p.push_back(z * uni(-0.2, 0.2)); p.push_back(z); }
  return p;
}

// a rotation of 3 degrees about z, then one of 2 degrees about x, and a shift
static D moved(const D& p) {
  const double c1 = std::cos(0.05235987755982988), s1 = std::sin(0.05235987755982988), c2 = std::cos(0.03490658503988659), s2 = std::sin(0.03490658503988659);
  D q(p.size());
  for (size_t i = 0; i < p.size() / 3; ++i) {
    const double x = c1 * p[3 * i] - s1 * p[3 * i + 1], y = s1 * p[3 * i] + c1 * p[3 * i + 1], z = p[3 * i + 2];
    q[3 * i] = x + 20.0; q[3 * i + 1] = c2 * y - s2 * z - 10.0; q[3 * i + 2] = s2 * y + c2 * z + 15.0;
  }
  return q;
}

int main() {
  {  // the sampler's first draws, by hand: state 5 + 0x9E3779B9 + 0x85EBCA6B = 0x24234429 (mod 2^32)
    uint32_t s = 5u + 0x9E3779B9u + 0x85EBCA6Bu;
    EXPECT(s == 0x24234429u);
    uint32_t k[3];
    sample(5u, 0u, 0u, 1000u, k);
    const uint32_t s1 = 1664525u * s + 1013904223u;
    EXPECT(k[0] == (uint32_t)(((uint64_t)s1 * 1000u) >> 32));
    for (uint32_t m = 3; m < 40; ++m)
      for (uint32_t h = 0; h < 300; ++h) {
        sample(m, h & 3u, h, m, k);
        EXPECT(k[0] < m && k[1] < m && k[2] < m && k[0] != k[1] && k[0] != k[2] && k[1] != k[2]);
      }
  }
  {  // the triad on a right-angle triple
    const double q0[3] = {1.0, 2.0, 3.0}, q1[3] = {4.0, 2.0, 3.0}, q2[3] = {1.0, 6.0, 3.0};
    double e[9], c[3];
    EXPECT(triad(q0, q1, q2, e, c));
    const double want[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int i = 0; i < 9; ++i) EXPECT(e[i] == want[i]);
    EXPECT(c[0] == 2.0 && c[1] == 10.0 / 3.0 && c[2] == 3.0);
    const double q3[3] = {7.0, 2.0, 3.0};
    EXPECT(!triad(q0, q1, q3, e, c));   // collinear
    EXPECT(!triad(q0, q0, q2, e, c));   // a repeated point
  }
  Case edge;
  {  // the edge scene: 0 .. 257 usable matches with three that are not usable among them, a collinear pair, pure outliers
    const uint32_t usable_counts[8] = {0, 1, 2, 3, 4, 255, 256, 257};
    for (uint32_t m : usable_counts) {
      D a = cloud(m + 3), b = moved(a);
      const uint32_t fa = edge.add_frame(a), fb = edge.add_frame(b);
      const uint32_t g = edge.offset[fa], h = edge.offset[fb];
      edge.xyz[3 * (size_t)g + 1] = std::nan("");           // feature 0 of frame a
      edge.xyz[3 * (size_t)(h + 1) + 2] = -5.0;             // feature 1 of frame b
      edge.tol_lat[(size_t)g + 2] = 0.0;                    // feature 2 of frame a
      edge.pairs.push_back(fa); edge.pairs.push_back(fb);
      for (uint32_t i = 0; i < m + 3; ++i) { edge.mi.push_back(i); edge.mj.push_back(i); }
      edge.start.push_back(edge.mi.size());
    }
    D line;
    for (int i = 0; i < 50; ++i) { line.push_back(2.0 * i); line.push_back(1.0 * i); line.push_back(400.0 + 6.0 * i); }
    uint32_t fa = edge.add_frame(line), fb = edge.add_frame(moved(line));
    edge.pairs.push_back(fa); edge.pairs.push_back(fb);
    for (uint32_t i = 0; i < 50; ++i) { edge.mi.push_back(i); edge.mj.push_back(i); }
    edge.start.push_back(edge.mi.size());
    fa = edge.add_frame(cloud(100)); fb = edge.add_frame(cloud(100));
    edge.pairs.push_back(fa); edge.pairs.push_back(fb);
    for (uint32_t i = 0; i < 100; ++i) { edge.mi.push_back(i); edge.mj.push_back(i); }
    edge.start.push_back(edge.mi.size());

    for (int refine = -1; refine <= 4; ++refine) {
      if (refine == 0) continue;
      lifcal_verify_options o{};
      o.refine = refine; o.seed = 3u;
      const Run r = verify(edge, &o);
      EXPECT(r.rc == 0);
      if (r.rc) continue;
      const uint32_t want[10] = {LIFCAL_VERIFY_FEW, LIFCAL_VERIFY_FEW, LIFCAL_VERIFY_FEW, LIFCAL_VERIFY_REJECTED, LIFCAL_VERIFY_REJECTED, LIFCAL_VERIFY_OK,
                                 LIFCAL_VERIFY_OK, LIFCAL_VERIFY_OK, LIFCAL_VERIFY_DEGENERATE, LIFCAL_VERIFY_REJECTED};
      for (int p = 0; p < 10; ++p) {
        const lifcal_verify_pair& row = r.rows[p];
        EXPECT(row.status == want[p]);
        EXPECT(row.rounds_used <= (uint32_t)std::max(refine, 0));
        if (p < 8) EXPECT(row.n_usable == usable_counts[p] && row.n_matches == usable_counts[p] + 3);
        if (p >= 5 && p < 8) EXPECT(row.n_inliers == usable_counts[p] && row.rms < 1e-6);
        uint32_t kept = 0;
        for (uint64_t k = edge.start[p]; k < edge.start[p + 1]; ++k) kept += r.keep[k];
        EXPECT(kept == (row.status == LIFCAL_VERIFY_OK ? row.n_inliers : 0u));
      }
      for (uint64_t k = 0; k < 3; ++k) EXPECT(std::isnan(r.e_par[edge.start[5] + k]) && r.keep[edge.start[5] + k] == 0);
    }
  }
  {  // every argument check
    lifcal_verify_options o{};
    EXPECT(verify(edge, &o).rc == 0);
    o.hypotheses = 300; EXPECT(verify(edge, &o).rc == LIFCAL_BA_ERR_INVALID_ARG);
    o.hypotheses = 4352; EXPECT(verify(edge, &o).rc == LIFCAL_BA_ERR_INVALID_ARG);
    o = {}; o.min_ratio = 1.5; EXPECT(verify(edge, &o).rc == LIFCAL_BA_ERR_INVALID_ARG);
    o = {}; o.min_ratio = -0.1; EXPECT(verify(edge, &o).rc == LIFCAL_BA_ERR_INVALID_ARG);
    o = {}; o.refine = 5; EXPECT(verify(edge, &o).rc == LIFCAL_BA_ERR_INVALID_ARG);
    o = {}; o.min_inliers = -1; EXPECT(verify(edge, &o).rc == LIFCAL_BA_ERR_INVALID_ARG);
    Case c = edge;
    c.pairs[1] = c.pairs[0]; EXPECT(verify(c, nullptr).rc == LIFCAL_BA_ERR_INVALID_ARG);
    c = edge; c.pairs[0] = 1000; EXPECT(verify(c, nullptr).rc == LIFCAL_BA_ERR_INVALID_ARG);
    c = edge; c.mi[0] = 3; EXPECT(verify(c, nullptr).rc == LIFCAL_BA_ERR_INVALID_ARG);
    c = edge; c.mj[2] = 0xffffffffu; EXPECT(verify(c, nullptr).rc == LIFCAL_BA_ERR_INVALID_ARG);
    c = edge; c.start[2] = 1; EXPECT(verify(c, nullptr).rc == LIFCAL_BA_ERR_INVALID_ARG);
    lifcal_verify_points pts{1, 0, edge.offset.data(), edge.xyz.data(), edge.tol_lat.data(), edge.tol_dep.data()};
    EXPECT(make_options("check", nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(make_options("check", &pts, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);
    pts.xyz = nullptr;
    EXPECT(make_options("check", &pts, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
  }
  {  // 200 random match lists: random frames, pairs, indices, a share of features that are not usable
    for (int trial = 0; trial < 200; ++trial) {
      Case c;
      const uint32_t n_frames = 2 + rnd(4);
      std::vector<D> base;
      const D world = cloud(40);
      for (uint32_t f = 0; f < n_frames; ++f) {
        D p(world.begin(), world.begin() + 3 * rnd(41));
        if (f & 1u) p = moved(p);
        c.add_frame(p);
      }
      for (size_t g = 0; g < c.tol_lat.size(); ++g) {
        const uint32_t what = rnd(12);
        if (what == 0) c.xyz[3 * g + rnd(3)] = std::nan("");
        if (what == 1) c.tol_dep[g] = 0.0;
        if (what == 2) c.xyz[3 * g + 2] = 0.0;
      }
      for (uint32_t a = 0; a < n_frames; ++a)
        for (uint32_t b = 0; b < n_frames; ++b) {
          if (a == b || rnd(2)) continue;
          const uint32_t na = c.offset[a + 1] - c.offset[a], nb = c.offset[b + 1] - c.offset[b];
          c.pairs.push_back(a); c.pairs.push_back(b);
          for (uint32_t k = rnd(60); k > 0 && na && nb; --k) {
            const uint32_t i = rnd(na);
            c.mi.push_back(i); c.mj.push_back(rnd(4) && i < nb ? i : rnd(nb));
          }
          c.start.push_back(c.mi.size());
        }
      lifcal_verify_options o{};
      o.seed = (uint32_t)trial; o.refine = (trial % 5) - 1 == 0 ? 3 : (trial % 5) - 1; o.min_inliers = 3 + (trial & 3);
      const Run r = verify(c, &o);
      EXPECT(r.rc == 0);
      for (size_t p = 0; r.rc == 0 && p < r.rows.size(); ++p) {
        uint32_t kept = 0;
        for (uint64_t k = c.start[p]; k < c.start[p + 1]; ++k) kept += r.keep[k];
        EXPECT(kept == (r.rows[p].status == LIFCAL_VERIFY_OK ? r.rows[p].n_inliers : 0u));
        EXPECT(r.rows[p].n_usable <= r.rows[p].n_matches && r.rows[p].n_inliers <= r.rows[p].n_usable);
      }
    }
  }
  std::printf(g_failed ? "verify_host_check: %d FAILED\n" : "verify_host_check ok\n", g_failed);
  return g_failed ? 1 : 0;
}
