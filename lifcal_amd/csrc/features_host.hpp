// features_host.hpp — the host-only part of include/lifcal_features.h: the argument checks of detection and
// matching, the descriptor's point pairs and the track linker.  No HIP in here: features.hip includes it for the library, and a
// stand-alone program with its own main can include it to run the same code under the host sanitizers (it then defines
// lifcal::set_last_error itself).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/lifcal_ba.h"
#include "../../include/lifcal_features.h"

namespace lifcal {

void set_last_error(const char* text);   // lifcal_ba.hip: the thread's text behind lifcal_ba_last_error()

namespace features {

constexpr int kPatchR = LIFCAL_FEATURES_PATCH_R;
constexpr int kMaxWinR = 3, kMaxNmsR = 6, kMinCell = 8, kMaxCell = 256, kMaxPerCell = 16;
constexpr int kNoBest = 257;   // second-best of a feature with one candidate; best of one with none

static int fail(int code, const std::string& text) { set_last_error(text.c_str()); return code; }

struct DetectPlan {
  lifcal_features_options opt;   // defaults resolved
  int32_t bx = 0, by = 0, bits = 0;
};

static int make_detect_plan(const char* who, const lifcal_rawdepth_image* im, const lifcal_features_options* o, DetectPlan* t) {
  const std::string w = std::string(who) + ": ";
  if (!im || !im->data) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no image");
  if (im->bits != 8 && im->bits != 16) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image bits must be 8 or 16");
  if (im->width < 1 || im->height < 1) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image size must be at least 1 x 1");
  if (im->pitch < im->width) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "image pitch is smaller than its width");
  lifcal_features_options q{};
  if (o) q = *o;
  if (q.win_r == 0) q.win_r = 3;
  if (q.nms_r == 0) q.nms_r = 4;
  if (q.cell == 0) q.cell = 32;
  if (q.per_cell == 0) q.per_cell = 4;
  if (q.min_score == 0.0) q.min_score = 1.0e-4;
  if (q.win_r < 1 || q.win_r > kMaxWinR) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "win_r outside 1 .. 3");
  if (q.nms_r < 1 || q.nms_r > kMaxNmsR) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "nms_r outside 1 .. 6");
  if (q.cell < kMinCell || q.cell > kMaxCell) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "cell outside 8 .. 256");
  if (q.per_cell < 1 || q.per_cell > kMaxPerCell) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "per_cell outside 1 .. 16");
  if (!(q.min_score > 0.0) || !std::isfinite(q.min_score)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_score must be positive and finite");
  if ((int64_t)im->width * im->height >= (1ll << 31) || (int64_t)im->pitch * im->height >= (1ll << 31))
    return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "2^31 pixels and more are not supported");
  t->opt = q;
  t->bits = im->bits;
  t->bx = t->by = 0;
  const int least = 2 * (kPatchR + 1) + 1;
  if (im->width >= least && im->height >= least) {
    t->bx = (im->width + q.cell - 1) / q.cell;
    t->by = (im->height + q.cell - 1) / q.cell;
    if (t->by > 65535) return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, w + "more than 65535 bucket rows");
  }
  return 0;
}

// ax, ay, bx, by of the 256 pairs (include/lifcal_features.h)
static void make_pattern(int8_t* out) {
  uint32_t s = 1u;
  auto draw = [&s]() { s = 1664525u * s + 1013904223u; return (int)((s >> 16) % 27u) - 13; };
  for (int i = 0; i < 256; ++i) {
    int v[4];
    do {
      for (int& c : v) c = draw();
    } while (v[0] == v[2] && v[1] == v[3]);
    for (int k = 0; k < 4; ++k) out[4 * i + k] = (int8_t)v[k];
  }
}

static int check_offsets(const std::string& w, uint32_t n_frames, const uint32_t* offset) {
  if (!offset) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no offsets");
  if (n_frames >= (1u << 30)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "too many frames");
  if (offset[0] != 0) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "offset[0] must be 0");
  for (uint32_t f = 0; f < n_frames; ++f)
    if (offset[f + 1] < offset[f]) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "the offsets descend at frame " + std::to_string(f));
  if (offset[n_frames] >= (1u << 31)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "2^31 features and more are not supported");
  return 0;
}

static int check_pairs(const std::string& w, uint32_t n_frames, uint32_t n_pairs, const uint32_t* pairs) {
  if (n_pairs && !pairs) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no pairs");
  if (n_pairs >= (1u << 30)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "too many pairs");
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const uint32_t a = pairs[2 * p], b = pairs[2 * p + 1];
    if (a >= n_frames || b >= n_frames) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "pair " + std::to_string(p) + " names a frame out of range");
    if (a == b) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "pair " + std::to_string(p) + " names one frame twice");
  }
  return 0;
}

static int make_match_options(const char* who, const lifcal_features_set* set, uint32_t n_pairs, const uint32_t* pairs, const lifcal_match_options* o,
                              lifcal_match_options* out) {
  const std::string w = std::string(who) + ": ";
  if (!set) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no features");
  if (int rc = check_offsets(w, set->n_frames, set->offset)) return rc;
  if (set->offset[set->n_frames] > 0 && !set->desc) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no descriptors");
  if (int rc = check_pairs(w, set->n_frames, n_pairs, pairs)) return rc;
  lifcal_match_options q{};
  if (o) q = *o;
  if (q.max_dist == 0) q.max_dist = 64;
  if (q.ratio_num == 0 && q.ratio_den == 0) { q.ratio_num = 3; q.ratio_den = 4; }
  if (q.max_dist < 1 || q.max_dist > 256) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_dist outside 1 .. 256");
  if (q.ratio_num < 1 || q.ratio_num > q.ratio_den || q.ratio_den > 32768) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "need 0 < ratio_num <= ratio_den <= 32768");
  if (q.max_shift < 0) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_shift must not be negative");
  if (q.max_shift > 0 && set->offset[set->n_frames] > 0 && (!set->ix || !set->iy)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "max_shift needs ix and iy");
  *out = q;
  return 0;
}

// include/lifcal_features.h (c)
static int link_tracks(uint32_t n_frames, const uint32_t* offset, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start, const uint32_t* mi,
                       const uint32_t* mj, lifcal_tracks* io) {
  const std::string w = "lifcal_tracks_link: ";
  if (!io) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no result");
  if (int rc = check_offsets(w, n_frames, offset)) return rc;
  if (int rc = check_pairs(w, n_frames, n_pairs, pairs)) return rc;
  if (n_pairs && !pair_start) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no pair_start");
  const uint32_t min_length = io->min_length ? io->min_length : 2u;
  if (min_length < 2) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "min_length must be at least 2");
  for (uint32_t p = 0; p < n_pairs; ++p)
    if (pair_start[p + 1] < pair_start[p]) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "pair_start descends at pair " + std::to_string(p));
  const uint64_t n_matches = n_pairs ? pair_start[n_pairs] - pair_start[0] : 0;
  if (n_matches && (!mi || !mj)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no matches");
  const uint32_t N = offset[n_frames];
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const uint32_t a = pairs[2 * p], b = pairs[2 * p + 1];
    const uint32_t na = offset[a + 1] - offset[a], nb = offset[b + 1] - offset[b];
    for (uint64_t k = pair_start[p]; k < pair_start[p + 1]; ++k)
      if (mi[k] >= na || mj[k] >= nb) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "match " + std::to_string(k) + " names a feature out of range");
  }
  std::vector<uint32_t> parent(N);
  std::iota(parent.begin(), parent.end(), 0u);
  auto find = [&parent](uint32_t v) {
    while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
    return v;
  };
  for (uint32_t p = 0; p < n_pairs; ++p) {
    const uint32_t oa = offset[pairs[2 * p]], ob = offset[pairs[2 * p + 1]];
    for (uint64_t k = pair_start[p]; k < pair_start[p + 1]; ++k) {
      const uint32_t ra = find(oa + mi[k]), rb = find(ob + mj[k]);
      if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);   // the root is the smallest feature of the component
    }
  }
  // per root: size, and whether some frame occurs twice (features come frame by frame, so a repeat is adjacent per root)
  std::vector<uint32_t> size(N, 0u), last_frame(N, 0xffffffffu), root(N);
  std::vector<uint8_t> conflict(N, 0);
  for (uint32_t f = 0; f < n_frames; ++f)
    for (uint32_t g = offset[f]; g < offset[f + 1]; ++g) {
      const uint32_t r = root[g] = find(g);
      ++size[r];
      if (last_frame[r] == f) conflict[r] = 1;
      last_frame[r] = f;
    }
  std::vector<uint32_t> track(N, 0xffffffffu);
  uint32_t n_tracks = 0;
  uint64_t n_obs = 0, n_conflicts = 0;
  for (uint32_t g = 0; g < N; ++g) {
    if (root[g] != g || size[g] < 2) continue;
    if (conflict[g]) { ++n_conflicts; continue; }
    if (size[g] < min_length) continue;
    track[g] = n_tracks++;   // roots ascend with their component's smallest feature
    n_obs += size[g];
  }
  io->n_tracks = n_tracks;
  io->n_conflicts = n_conflicts;
  io->n = n_obs;
  if (io->capacity < n_obs) return LIFCAL_MLA_MORE;
  if (n_obs && (!io->fr || !io->pt || !io->feature)) return fail(LIFCAL_BA_ERR_INVALID_ARG, w + "no output arrays");
  uint64_t k = 0;
  for (uint32_t f = 0; f < n_frames; ++f)
    for (uint32_t g = offset[f]; g < offset[f + 1]; ++g) {
      const uint32_t t = track[root[g]];
      if (t == 0xffffffffu) continue;
      io->fr[k] = f; io->pt[k] = t; io->feature[k] = g;
      ++k;
    }
  return 0;
}

}  // namespace features
}  // namespace lifcal
