// markers_host.hpp — the host-only part of include/lifcal_markers.h: the argument checks, the dictionary's
// distance and generator, the candidate filter and the quad of steps 3 and 4, the constraints reader, the start values of the
// marker points and the scale factor.  No HIP in here: markers.hip includes it for the library (the small integer and double
// helpers marked LIFCAL_HD are then compiled for the device as well), and a stand-alone program with its own main can include
// it to run the same code under the host sanitizers (it then defines lifcal::set_last_error itself).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/lifcal_ba.h"
#include "../../include/lifcal_markers.h"

#ifdef __HIPCC__
#define LIFCAL_HD __host__ __device__
#else
#define LIFCAL_HD
#endif

// every double step of include/lifcal_markers.h is one IEEE operation: nothing in this translation unit is contracted
#pragma clang fp contract(off)

namespace lifcal {

void set_last_error(const char* text);   // lifcal_ba.hip: the thread's text behind lifcal_ba_last_error()

namespace markers {

constexpr int kTile = 32;          // tiles of the dark map and the labelling
constexpr int kMaxW = 31;
constexpr int kMinBits = 3, kMaxBits = 7;

static int fail(int code, const std::string& text) { set_last_error(text.c_str()); return code; }

// rot of include/lifcal_markers.h step 5: rot(B)[r][c] = B[m-1-c][r]
LIFCAL_HD inline uint64_t rot_word(uint64_t w, int m) {
  uint64_t out = 0;
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c)
      if ((w >> ((m - 1 - c) * m + r)) & 1ull) out |= 1ull << (r * m + c);
  return out;
}

LIFCAL_HD inline int popcount64(uint64_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}

// the least popcount(a xor rot_k(b)), k = k0 .. 3
inline int word_distance(uint64_t a, uint64_t b, int m, int k0) {
  int best = 65;
  uint64_t r = b;
  for (int k = 0; k < 4; ++k) {
    if (k >= k0) best = std::min(best, popcount64(a ^ r));
    r = rot_word(r, m);
  }
  return best;
}

static int check_dictionary(const std::string& w, const lifcal_marker_dictionary* d) {
  if (!d || !d->words) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no dictionary");
  if (d->marker_bits < kMinBits || d->marker_bits > kMaxBits) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "marker_bits outside 3 .. 7");
  if (d->n < 1 || d->n > LIFCAL_MARKERS_MAX_WORDS) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "dictionary size outside 1 .. 4096");
  const int nb = d->marker_bits * d->marker_bits;
  for (uint32_t i = 0; i < d->n; ++i)
    if (d->words[i] >> nb) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "word " + std::to_string(i) + " has bits above marker_bits^2");
  return 0;
}

static int dictionary_distance(const lifcal_marker_dictionary* d) {
  int best = 65;
  for (uint32_t i = 0; i < d->n; ++i) {
    best = std::min(best, word_distance(d->words[i], d->words[i], d->marker_bits, 1));
    for (uint32_t j = i + 1; j < d->n; ++j) best = std::min(best, word_distance(d->words[i], d->words[j], d->marker_bits, 0));
  }
  return best;
}

static int generate_dictionary(int32_t bits, uint32_t n, uint32_t seed, uint64_t* out, int32_t* min_distance) {
  const std::string w = "lifcal_marker_dictionary_generate: ";
  if (!out) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no output");
  if (bits < kMinBits || bits > kMaxBits) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "marker_bits outside 3 .. 7");
  if (n < 1 || n > LIFCAL_MARKERS_MAX_WORDS) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "dictionary size outside 1 .. 4096");
  const int nb = bits * bits, draws = (nb + 15) / 16;
  const uint64_t mask = (1ull << nb) - 1ull;
  uint32_t s = seed;
  int tau = nb / 2, refused = 0;
  uint32_t have = 0;
  while (have < n) {
    uint64_t word = 0;
    for (int i = 0; i < draws; ++i) {
      s = 1664525u * s + 1013904223u;
      word |= (uint64_t)((s >> 16) & 0xffffu) << (16 * i);
    }
    word &= mask;
    bool ok = word_distance(word, word, bits, 1) >= tau;
    for (uint32_t j = 0; ok && j < have; ++j) ok = word_distance(word, out[j], bits, 0) >= tau;
    if (ok) { out[have++] = word; refused = 0; continue; }
    if (++refused == 2000) {
      if (tau == 1) return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "the space of words is exhausted");
      --tau; refused = 0;
    }
  }
  if (min_distance) {
    const lifcal_marker_dictionary d{bits, n, out};
    *min_distance = dictionary_distance(&d);
  }
  return 0;
}

struct Plan {
  lifcal_markers_options opt;   // defaults resolved
  int32_t bits = 0, min_distance = 0, tx = 0, ty = 0;
  int64_t max_candidates = 0;
  int64_t C = 0, C_cell = 0;    // contrast and cell_contrast in grey levels
};

static int make_plan(const char* who, const lifcal_rawdepth_image* im, const lifcal_marker_dictionary* dict, const lifcal_markers_options* o, Plan* t) {
  const std::string w = std::string(who) + ": ";
  if (!im || !im->data) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no image");
  if (im->bits != 8 && im->bits != 16) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image bits must be 8 or 16");
  if (im->width < 1 || im->height < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image size must be at least 1 x 1");
  if (im->pitch < im->width) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image pitch is smaller than its width");
  if (dict)
    if (int rc = check_dictionary(w, dict)) return rc;
  lifcal_markers_options q{};
  if (o) q = *o;
  if (q.w == 0) q.w = 7;
  if (q.contrast == 0) q.contrast = 12;
  if (q.w < 1 || q.w > kMaxW) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "w outside 1 .. 31");
  if (q.contrast < 1 || q.contrast > 255) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "contrast outside 1 .. 255");
  if (q.cell_contrast == 0) q.cell_contrast = std::min(2 * q.contrast, 255);
  if (q.cell_contrast < 1 || q.cell_contrast > 255) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "cell_contrast outside 1 .. 255");
  if (q.min_area == 0) q.min_area = 32;
  if (q.min_area < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_area must be at least 1");
  if (q.min_side == 0) q.min_side = 12;
  if (q.min_side < 2 || q.min_side > 32768) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_side outside 2 .. 32768");
  if (q.max_side == 0) q.max_side = std::max(std::min(im->width, im->height), q.min_side);
  if (q.max_side < q.min_side) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_side is smaller than min_side");
  const int cells = (dict ? dict->marker_bits : kMaxBits) + 2;
  if (q.max_border_errors < 0 || q.max_border_errors > 4 * (cells - 1)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_border_errors outside 0 .. 4 (n - 1)");
  if (q.refine_max == 0.0) q.refine_max = 3.0;
  if (!(q.refine_max > 0.0) || !std::isfinite(q.refine_max)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "refine_max must be positive and finite");
  if ((int64_t)im->width * im->height >= (1ll << 31) || (int64_t)im->pitch * im->height >= (1ll << 31))
    return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "2^31 pixels and more are not supported");
  t->min_distance = 0;
  if (dict) {
    t->min_distance = dictionary_distance(dict);
    if (t->min_distance == 0) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "two words of the dictionary coincide, or one is its own rotation");
    const int bound = (t->min_distance - 1) / 2;
    if (q.max_correction == 0) q.max_correction = bound;
    else if (q.max_correction == -1) q.max_correction = 0;
    if (q.max_correction < 0 || q.max_correction > bound)
      return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_correction exceeds (min_distance - 1) / 2 = " + std::to_string(bound));
  } else {
    if (q.max_correction != 0 && q.max_correction != -1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_correction without a dictionary");
    q.max_correction = 0;
  }
  t->opt = q;
  t->bits = im->bits;
  t->tx = (im->width + kTile - 1) / kTile;
  t->ty = (im->height + kTile - 1) / kTile;
  t->max_candidates = (int64_t)im->width * im->height / q.min_area;
  const int64_t unit = im->bits == 8 ? 1 : 256;
  t->C = q.contrast * unit;
  t->C_cell = q.cell_contrast * unit;
  return 0;
}

static void fill_plan(const Plan& t, lifcal_markers_plan* plan) {
  plan->options = t.opt;
  plan->min_distance = t.min_distance;
  plan->tiles_x = t.tx; plan->tiles_y = t.ty; plan->reserved = 0;
  plan->max_candidates = t.max_candidates;
}

// step 3 of include/lifcal_markers.h on a component's area and extremes; fills the box
inline bool is_candidate(lifcal_marker_component* c, const lifcal_markers_options& o, int W, int H) {
  c->x0 = c->ext[0][0]; c->x1 = c->ext[1][0]; c->y0 = c->ext[2][1]; c->y1 = c->ext[3][1];
  const int sx = c->x1 - c->x0 + 1, sy = c->y1 - c->y0 + 1;
  return c->area >= o.min_area && sx >= o.min_side && sy >= o.min_side && sx <= o.max_side && sy <= o.max_side && c->x0 >= 1 && c->y0 >= 1 &&
         c->x1 <= W - 2 && c->y1 <= H - 2;
}

// step 4: false when the quad is rejected
LIFCAL_HD inline bool choose_quad(const int32_t* ext /* [8][2] */, int min_side, double* q /* [4][2] */) {
  const int diag[4] = {4, 7, 5, 6}, axis[4] = {2, 1, 3, 0};
  long long best = 0;
  const int* pick = diag;
  for (int set = 0; set < 2; ++set) {
    const int* idx = set ? axis : diag;
    long long a2 = 0;
    for (int i = 0; i < 4; ++i) {
      const int j = (i + 1) & 3;
      a2 += (long long)ext[2 * idx[i]] * ext[2 * idx[j] + 1] - (long long)ext[2 * idx[j]] * ext[2 * idx[i] + 1];
    }
    if (set == 0 || a2 > best) { best = a2; pick = idx; }
  }
  if (best < (long long)min_side * min_side) return false;
  long long sx = 0, sy = 0;
  for (int i = 0; i < 4; ++i) { sx += ext[2 * pick[i]]; sy += ext[2 * pick[i] + 1]; }
  for (int i = 0; i < 4; ++i) {
    const long long px = ext[2 * pick[i]], py = ext[2 * pick[i] + 1];
    const long long dx = 4 * px - sx, dy = 4 * py - sy;
    q[2 * i] = (double)px + 0.5 * (double)((dx > 0) - (dx < 0));
    q[2 * i + 1] = (double)py + 0.5 * (double)((dy > 0) - (dy < 0));
  }
  return true;
}

// ---------------------------------------------------------------------------------------------- constraints, seeds, scale

static int read_constraints(const char* path, lifcal_constraints* io) {
  const std::string w = "lifcal_constraints_read: ";
  if (!path || !io) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no path or no result");
  std::ifstream in(path);
  if (!in.is_open()) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "cannot open " + path);
  std::vector<uint32_t> a, b, ids;
  std::vector<double> dist, sig;
  std::string line;
  int64_t no = 0;
  while (std::getline(in, line)) {
    ++no;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty() || line[0] == '#') continue;
    const char* p = line.c_str();
    char* end = nullptr;
    long long id[2] = {0, 0};
    double v[2] = {0.0, 0.0};
    bool ok = true;
    for (int k = 0; k < 2 && ok; ++k) {
      id[k] = std::strtoll(p, &end, 10);
      ok = end != p && id[k] >= 0 && id[k] < (1ll << 31);
      p = end;
    }
    for (int k = 0; k < 2 && ok; ++k) {
      v[k] = std::strtod(p, &end);
      ok = end != p && std::isfinite(v[k]) && v[k] > 0.0;
      p = end;
    }
    if (ok) {
      while (*p == ' ' || *p == '\t') ++p;
      ok = *p == '\0';
    }
    if (!ok) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "line " + std::to_string(no) + " is not `id1 id2 distance sigma`");
    a.push_back((uint32_t)id[0]); b.push_back((uint32_t)id[1]); dist.push_back(v[0]); sig.push_back(v[1]);
    for (int k = 0; k < 2; ++k)
      if (std::find(ids.begin(), ids.end(), (uint32_t)id[k]) == ids.end()) ids.push_back((uint32_t)id[k]);
  }
  io->n = a.size();
  io->n_ids = ids.size();
  if (io->capacity < io->n || io->ids_capacity < io->n_ids) return LIFCAL_MLA_MORE;
  if (io->n && (!io->id1 || !io->id2 || !io->distance || !io->sigma || !io->ids)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no output arrays");
  for (size_t k = 0; k < a.size(); ++k) { io->id1[k] = a[k]; io->id2[k] = b[k]; io->distance[k] = dist[k]; io->sigma[k] = sig[k]; }
  for (size_t k = 0; k < ids.size(); ++k) io->ids[k] = ids[k];
  return 0;
}

static int seed_points(uint64_t n_markers, const double* mx, const double* my, const uint32_t* mfr, const uint32_t* mid, uint64_t n_tracked,
                       const double* tx, const double* ty, const uint32_t* tfr, const uint32_t* tpt, uint64_t n_points, const double* pts,
                       lifcal_marker_seeds* io) {
  const std::string w = "lifcal_markers_seed_points: ";
  if (!io) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no result");
  if (n_markers && (!mx || !my || !mfr || !mid)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no marker observations");
  if (n_tracked && (!tx || !ty || !tfr || !tpt)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no tracked image points");
  if (n_tracked && !pts) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no points");
  for (uint64_t k = 0; k < n_tracked; ++k)
    if (tpt[k] >= n_points) return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "tracked image point " + std::to_string(k) + " names a point out of range");
  std::vector<uint32_t> ids;
  std::vector<uint64_t> first;   // per id: its first observation with the lowest frame
  for (uint64_t k = 0; k < n_markers; ++k) {
    if (!std::isfinite(mx[k]) || !std::isfinite(my[k])) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "a marker centre is not finite");
    const auto it = std::find(ids.begin(), ids.end(), mid[k]);
    if (it == ids.end()) { ids.push_back(mid[k]); first.push_back(k); }
    else if (mfr[k] < mfr[first[(size_t)(it - ids.begin())]]) first[(size_t)(it - ids.begin())] = k;
  }
  io->n_ids = ids.size();
  io->n_unseeded = 0;
  const bool fill = io->capacity >= ids.size();
  if (fill && !ids.empty() && (!io->ids || !io->xyz || !io->seeded)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no output arrays");
  for (size_t i = 0; i < ids.size(); ++i) {
    const uint64_t m = first[i];
    bool have = false;
    double best = 0.0;
    uint64_t arg = 0;
    for (uint64_t k = 0; k < n_tracked; ++k) {
      if (tfr[k] != mfr[m]) continue;
      const double dx = tx[k] - mx[m], dy = ty[k] - my[m];
      const double d2 = dx * dx + dy * dy;
      if (!have || d2 < best) { have = true; best = d2; arg = k; }
    }
    if (!have) ++io->n_unseeded;
    if (!fill) continue;
    io->ids[i] = ids[i];
    io->seeded[i] = have ? 1 : 0;
    for (int c = 0; c < 3; ++c) io->xyz[3 * i + c] = have ? pts[3 * (uint64_t)tpt[arg] + c] : 0.0;
  }
  return fill ? 0 : LIFCAL_MLA_MORE;
}

static int scale_factor(const double* p1, const double* p2, double distance, double* factor) {
  const std::string w = "lifcal_scene_scale_factor: ";
  if (!p1 || !p2 || !factor) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no points or no result");
  if (!(distance > 0.0) || !std::isfinite(distance)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "the distance must be positive and finite");
  const double dx = p1[0] - p2[0], dy = p1[1] - p2[1], dz = p1[2] - p2[2];
  const double len = std::sqrt(dx * dx + dy * dy + dz * dz);
  if (!std::isfinite(len) || !(len > 0.0)) return fail(LIFCAL_BA_ERR_NUMERIC, w + "the two points coincide or are not finite");
  *factor = distance / len;
  return 0;
}

}  // namespace markers
}  // namespace lifcal
