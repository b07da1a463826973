// features_host_check.cpp — the host-only part of include/lifcal_features.h (features_host.hpp) as a stand-alone program, so that
// the track linker and the argument checks can run under the host sanitizers:
//   make -C lifcal_amd/csrc features_host_check && lifcal_amd/csrc/features_host_check
// (the target compiles with -fsanitize=address,undefined).  No HIP, no device, no Python.  It runs the hand-made linker cases of
// tests/test_features_cpu.py, with every array allocated at its exact size so that a read or write past an end is caught.
#include <cstdio>
#include <cstring>

#include "features_host.hpp"

namespace lifcal {
static std::string g_error;
void set_last_error(const char* text) { g_error = text; }
}  // namespace lifcal

using namespace lifcal::features;
using U = std::vector<uint32_t>;

static int g_failed = 0;
#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++g_failed; } \
  } while (0)

struct Out {
  int rc = 0;
  lifcal_tracks t{};
  U fr, pt, ft;
};

// count, then fill, with exactly-sized heap arrays
static Out link(const U& counts, const U& pairs, const std::vector<uint64_t>& start, const U& mi, const U& mj, uint32_t min_length = 0) {
  U off(counts.size() + 1, 0u);
  for (size_t f = 0; f < counts.size(); ++f) off[f + 1] = off[f] + counts[f];
  const uint32_t n_pairs = (uint32_t)(pairs.size() / 2);
  Out o;
  o.t.min_length = min_length;
  o.rc = link_tracks((uint32_t)counts.size(), off.data(), n_pairs, pairs.empty() ? nullptr : pairs.data(), start.empty() ? nullptr : start.data(),
                     mi.empty() ? nullptr : mi.data(), mj.empty() ? nullptr : mj.data(), &o.t);
  if (o.rc != LIFCAL_MLA_MORE) return o;
  o.fr.resize(o.t.n); o.pt.resize(o.t.n); o.ft.resize(o.t.n);
  o.t.capacity = o.t.n; o.t.fr = o.fr.data(); o.t.pt = o.pt.data(); o.t.feature = o.ft.data();
  o.rc = link_tracks((uint32_t)counts.size(), off.data(), n_pairs, pairs.data(), start.data(), mi.data(), mj.data(), &o.t);
  return o;
}

int main() {
  const U counts{3, 3, 3}, pairs{0, 1, 1, 2, 0, 2};
  const std::vector<uint64_t> one_each{0, 1, 2, 3};
  {  // a chain a-b-c and a two-frame track; the ordering rules
    const Out o = link(counts, pairs, one_each, U{2, 0, 1}, U{0, 1, 2});
    EXPECT(o.rc == 0 && o.t.n_tracks == 2 && o.t.n_conflicts == 0 && o.t.n == 5);
    EXPECT((o.fr == U{0, 0, 1, 2, 2}) && (o.ft == U{1, 2, 3, 7, 8}) && (o.pt == U{0, 1, 1, 1, 0}));
  }
  {  // min_length
    const Out o = link(counts, pairs, one_each, U{2, 0, 1}, U{0, 1, 2}, 3);
    EXPECT(o.rc == 0 && o.t.n_tracks == 1 && (o.ft == U{2, 3, 7}));
    EXPECT(link(counts, pairs, one_each, U{2, 0, 1}, U{0, 1, 2}, 1).rc == LIFCAL_BA_ERR_INVALID_ARG);
  }
  {  // a conflict, dropped whole and counted; it leaves another track alone
    Out o = link(counts, pairs, one_each, U{0, 0, 1}, U{0, 0, 0});
    EXPECT(o.rc == 0 && o.t.n_tracks == 0 && o.t.n_conflicts == 1 && o.t.n == 0);
    o = link(counts, pairs, {0, 2, 3, 4}, U{0, 2, 0, 1}, U{0, 2, 0, 0});
    EXPECT(o.rc == 0 && o.t.n_tracks == 1 && o.t.n_conflicts == 1 && (o.ft == U{2, 5}));
  }
  {  // an empty pair, a frame without features, no pairs, no frames
    Out o = link(U{2, 0, 2}, U{0, 2, 0, 1, 2, 0}, {0, 1, 1, 2}, U{1, 0}, U{0, 1});
    EXPECT(o.rc == 0 && o.t.n_tracks == 1 && (o.ft == U{1, 2}) && (o.fr == U{0, 2}));
    o = link(U{2, 2}, U{}, {}, U{}, U{});
    EXPECT(o.rc == 0 && o.t.n_tracks == 0 && o.t.n == 0);
    o = link(U{}, U{}, {}, U{}, U{});
    EXPECT(o.rc == 0 && o.t.n == 0);
  }
  {  // indices out of range are refused, never read
    EXPECT(link(counts, pairs, one_each, U{3, 0, 1}, U{0, 1, 2}).rc == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(link(counts, pairs, one_each, U{2, 0, 0xffffffffu}, U{0, 1, 2}).rc == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(link(counts, pairs, one_each, U{2, 0, 1}, U{0, 1, 3}).rc == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(link(counts, U{0, 1, 1, 3, 0, 2}, one_each, U{2, 0, 1}, U{0, 1, 2}).rc == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(link(counts, U{0, 1, 1, 1, 0, 2}, one_each, U{2, 0, 1}, U{0, 1, 2}).rc == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(link(counts, pairs, {0, 2, 1, 3}, U{2, 0, 1}, U{0, 1, 2}).rc == LIFCAL_BA_ERR_INVALID_ARG);
    EXPECT(link_tracks(0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == LIFCAL_BA_ERR_INVALID_ARG);
  }
  {  // a longer random run: every array at its exact size
    uint32_t s = 12345u;
    auto rnd = [&s](uint32_t n) { s = 1664525u * s + 1013904223u; return (s >> 16) % n; };
    for (int trial = 0; trial < 200; ++trial) {
      U c(6);
      for (uint32_t& v : c) v = rnd(7);
      U pr, mi, mj;
      std::vector<uint64_t> st{0};
      for (uint32_t a = 0; a < 6; ++a)
        for (uint32_t b = 0; b < 6; ++b) {
          if (a == b || rnd(3)) continue;
          pr.push_back(a); pr.push_back(b);
          for (uint32_t k = rnd(4); k > 0 && c[a] && c[b]; --k) { mi.push_back(rnd(c[a])); mj.push_back(rnd(c[b])); }
          st.push_back(mi.size());
        }
      const Out o = link(c, pr, pr.empty() ? std::vector<uint64_t>{} : st, mi, mj, 2 + (uint32_t)(trial & 1));
      EXPECT(o.rc == 0 && o.t.n == o.fr.size());
      for (size_t k = 1; k < o.ft.size(); ++k) EXPECT(o.ft[k - 1] < o.ft[k] && o.fr[k - 1] <= o.fr[k]);
    }
  }
  {  // the argument checks of detection and matching, and the pattern
    uint16_t px[4] = {0, 0, 0, 0};
    lifcal_rawdepth_image im{px, 8, 200, 160, 0, 200};
    DetectPlan plan;
    EXPECT(make_detect_plan("check", &im, nullptr, &plan) == 0 && plan.bx == 7 && plan.by == 5 && plan.opt.per_cell == 4);
    lifcal_features_options fo{};
    fo.cell = 7;
    EXPECT(make_detect_plan("check", &im, &fo, &plan) == LIFCAL_BA_ERR_INVALID_ARG && lifcal::g_error.find("cell") != std::string::npos);
    im.width = 32;
    EXPECT(make_detect_plan("check", &im, nullptr, &plan) == 0 && plan.bx == 0);
    EXPECT(make_detect_plan("check", nullptr, nullptr, &plan) == LIFCAL_BA_ERR_INVALID_ARG);
    const U off{0, 2, 5}, desc(5 * 8, 0u), good{0, 1}, bad{0, 2};
    lifcal_features_set set{2, 0, off.data(), desc.data(), nullptr, nullptr};
    lifcal_match_options mo{}, res{};
    EXPECT(make_match_options("check", &set, 1, good.data(), &mo, &res) == 0 && res.max_dist == 64 && res.ratio_num == 3 && res.ratio_den == 4);
    EXPECT(make_match_options("check", &set, 1, bad.data(), &mo, &res) == LIFCAL_BA_ERR_INVALID_ARG);
    mo.max_shift = 5;
    EXPECT(make_match_options("check", &set, 1, good.data(), &mo, &res) == LIFCAL_BA_ERR_INVALID_ARG);
    std::vector<int8_t> pat(1024);
    make_pattern(pat.data());
    EXPECT(pat[0] == 12 && pat[1] == -5 && pat[2] == 12 && pat[3] == 12 && pat[1020] == 9 && pat[1023] == -9);
  }
  std::printf(g_failed ? "features_host_check: %d FAILED\n" : "features_host_check ok\n", g_failed);
  return g_failed ? 1 : 0;
}
