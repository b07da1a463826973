/* lifcal_features.h — feature tracks from total-focus images: image points in every total-focus image
 * (include/lifcal_totalfocus.h), their correspondences between frames, and the tracks (x, y, fr, pt) that lifcal_depth_sample,
 * lifcal_mla_project, lifcal_register_scene and lifcal_ba_create take.  Same shared library as include/lifcal_ba.h
 * (liblifcal_ba.so), same error codes and lifcal_ba_last_error().  Argument checks come first and need no device; detection and
 * matching run on the GPU and have no CPU fallback (LIFCAL_BA_ERR_NO_DEVICE without a gfx950 device); the linker is host only.
 *
 * The algorithm, exactly.  Everything summed is an integer; doubles are IEEE without fused multiply-add, evaluated in the order
 * written.  Two calls give the same bytes, equal to those of the numpy restatement in tests/features_reference.py.
 *
 * (a) lifcal_features_detect.  I(x, y) is the image, x = column, y = row; full = 2^bits - 1; patch_r = 15.
 *   Gradient (Sobel, 64-bit integers), for 1 <= x <= width - 2, 1 <= y <= height - 2:
 *     gx = (I(x+1,y-1) + 2 I(x+1,y) + I(x+1,y+1)) - (I(x-1,y-1) + 2 I(x-1,y) + I(x-1,y+1)),
 *     gy = (I(x-1,y+1) + 2 I(x,y+1) + I(x+1,y+1)) - (I(x-1,y-1) + 2 I(x,y-1) + I(x+1,y-1));  |g| <= 4 full < 2^18.
 *   Structure tensor over the (2 win_r + 1)^2 window about (x, y):  A = sum gx gx,  B = sum gx gy,  C = sum gy gy, below 2^42
 *   for win_r <= 3, so exact in int64 and in double.
 *     score(x, y) = ((dA dC - dB dB) / (dA + dC + 1.0)) / (dfull dfull),   dA = (double)A etc.
 *   The score uses pixel values whatever their validity; it is defined win_r + 1 from every border, which is all a candidate reads.
 *   Valid pixel: status 0 or 3 (the statuses under which lifcal_totalfocus_render wrote a pixel); without a status map all are.
 *   (x, y) is a candidate when  patch_r + 1 <= x <= width - 1 - (patch_r + 1), the same in y;  every pixel of the
 *   (2 patch_r + 1)^2 patch about it is valid;  score >= min_score;  and for every other (x', y') with |x' - x| <= nms_r and
 *   |y' - y| <= nms_r:  score(x', y') < score, or score(x', y') == score and (y', x') comes after (y, x) in lexicographic order
 *   (of tied pixels the first in (y, x) order wins).  nms_r + win_r + 1 <= patch_r + 1, so all of that lies inside the image.
 *   Bucket of a candidate: (x / cell, y / cell) in integers.  Of the candidates of a bucket the best per_cell stay, in the order
 *   score descending, then y ascending, then x ascending.  The output lists the buckets row-major and each bucket in that order.
 *   Sub-pixel position, per axis, from s0 = score(x, y), sm = score(x-1, y), sp = score(x+1, y) (y likewise):
 *     den = (sm - 2.0 s0) + sp;  o = den < 0 ? (0.5 (sm - sp)) / den : 0;  o clamped to [-0.5, 0.5];  x_out = (double)x + o.
 *   Descriptor, 256 bits, upright.  S(u, v) = the sum of I over the 5 x 5 box about (u, v).  Bit i, i = 0 .. 255, is
 *     S(x + ax_i, y + ay_i) < S(x + bx_i, y + by_i)   and is stored as bit (i & 31) of word i >> 5.
 *   The pairs (lifcal_features_pattern):  a 32-bit state s starts at 1; a draw is  s = 1664525 s + 1013904223 (mod 2^32), then
 *   the value ((s >> 16) mod 27) - 13.  A pair is four draws in the order ax, ay, bx, by; when (ax, ay) == (bx, by) the four are
 *   drawn again.  All offsets lie in [-13, 13], the box adds 2: the descriptor reads exactly the (2 patch_r + 1)^2 patch.
 *   An image narrower or lower than 2 (patch_r + 1) + 1 has no candidate: n = 0 and nothing is launched.
 *
 * (b) lifcal_features_match.  D(p, q) = the number of bits in which descriptors p and q differ.  For a pair of frames (a, b),
 *   a != b, the candidates of feature i of a are all features j of b, and with max_shift > 0 only those with
 *   |ix_j - ix_i| <= max_shift and |iy_j - iy_i| <= max_shift.  best(i) = the least D over the candidates, arg(i) = the lowest j
 *   that attains it, second(i) = the least D over the candidates other than arg(i), or 257 when there is none.  A feature
 *   without candidates has no best.  The same from every feature of b towards a.  (i, j) is a match when
 *     arg(i) = j and arg(j) = i,   D(i, j) <= max_dist,   ratio_den D(i, j) < ratio_num second(i)  and  < ratio_num second(j)
 *   (strictly: two identical candidates never match).  Per pair the matches are listed by ascending i.
 *
 * (c) lifcal_tracks_link.  Features are numbered through the concatenated list, g = offset[frame] + index.  Union-find over the
 *   matches of all pairs.  A component that holds two features of one frame is dropped whole and counted in n_conflicts (COLMAP's
 *   rule); of the rest, those with fewer than min_length features (one per frame) are dropped.  The tracks that stay are numbered
 *   0, 1, ... by their smallest g; the observations are listed by ascending g (frame, then feature index).
 */
#ifndef LIFCAL_FEATURES_H
#define LIFCAL_FEATURES_H
#include <stdint.h>
#include "lifcal_mla.h"
#include "lifcal_rawdepth.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LIFCAL_FEATURES_PATCH_R 15
#define LIFCAL_FEATURES_DESC_WORDS 8

/* 0 (0.0) in a field selects its default */
typedef struct lifcal_features_options {
  int32_t win_r;      /* window of the structure tensor, 1 .. 3; default 3 */
  int32_t nms_r;      /* non-maximum suppression, 1 .. 6; default 4 */
  int32_t cell;       /* bucket side in pixels, 8 .. 256; default 32 */
  int32_t per_cell;   /* features kept per bucket, 1 .. 16; default 4 */
  double min_score;   /* > 0 and finite; default 1e-4 */
} lifcal_features_options;

/* what the argument checks of lifcal_features_detect derive before any device is touched */
typedef struct lifcal_features_plan {
  lifcal_features_options options;   /* with the defaults filled in */
  int32_t buckets_x, buckets_y;      /* ceil(width / cell), ceil(height / cell); both 0 when the image is too small for a patch */
  int64_t max_features;              /* buckets_x buckets_y per_cell: a capacity that always suffices */
} lifcal_features_plan;

/* count-then-fill as lifcal_mla_project: n is always set; capacity < n writes no array and returns LIFCAL_MLA_MORE */
typedef struct lifcal_features_list {
  uint64_t capacity;
  uint64_t n;          /* out */
  double* x;           /* capacity entries each (host), or NULL when capacity = 0 */
  double* y;
  int32_t* ix;         /* the integer position of the maximum */
  int32_t* iy;
  double* score;
  uint32_t* desc;      /* [capacity][8] */
  double seconds;      /* out: device time of the kernels (HIP events) */
} lifcal_features_list;

/* Host only: exactly the checks lifcal_features_detect makes of `image` and `options` (image->data is only tested against
 * NULL; width and height of at least 1, 8 or 16 bits, pitch >= width).  options and plan may be NULL.
 * LIFCAL_BA_ERR_OUT_OF_RANGE for 2^31 pixels and more or more than 65535 bucket rows. */
int lifcal_features_check(const lifcal_rawdepth_image* image, const lifcal_features_options* options, lifcal_features_plan* plan);

/* image: one channel, a host pointer or (on_device = 1) a device pointer on `device`.  status: NULL (all pixels valid) or
 * [height][width] uint8_t with row pitch = width, a pointer of the same kind as the image's. */
int lifcal_features_detect(const lifcal_rawdepth_image* image, const uint8_t* status, int32_t device, const lifcal_features_options* options,
                           lifcal_features_list* out);

/* the 256 point pairs: out[4 i .. 4 i + 3] = ax_i, ay_i, bx_i, by_i.  Host only. */
int lifcal_features_pattern(int8_t* out);

/* the features of n_frames frames, concatenated: frame f holds offset[f] .. offset[f+1] - 1 */
typedef struct lifcal_features_set {
  uint32_t n_frames, reserved;
  const uint32_t* offset;   /* [n_frames + 1], offset[0] = 0, not descending, offset[n_frames] < 2^31 */
  const uint32_t* desc;     /* [offset[n_frames]][8], host */
  const int32_t* ix;        /* [offset[n_frames]] host; may be NULL when max_shift = 0 */
  const int32_t* iy;
} lifcal_features_set;

typedef struct lifcal_match_options {
  int32_t max_dist;               /* 1 .. 256; default 64 */
  int32_t ratio_num, ratio_den;   /* 0 < num <= den <= 32768; default 3 / 4 (both 0) */
  int32_t max_shift;              /* >= 0; 0 (the default): no gate */
} lifcal_match_options;

/* count-then-fill as above for i, j, dist; pair_start is always written */
typedef struct lifcal_match_list {
  uint64_t capacity;
  uint64_t n;             /* out: matches of all pairs */
  uint64_t* pair_start;   /* [n_pairs + 1] out: the matches of pair p are pair_start[p] .. pair_start[p+1] - 1 */
  uint32_t* i;            /* index within frame a */
  uint32_t* j;            /* index within frame b */
  uint32_t* dist;
  double seconds;         /* out */
} lifcal_match_list;

/* Host only: the checks lifcal_features_match makes (pairs: [n_pairs][2] frame indices a, b < n_frames, a != b).  options and
 * resolved (the options with the defaults filled in) may be NULL. */
int lifcal_features_match_check(const lifcal_features_set* set, uint32_t n_pairs, const uint32_t* pairs, const lifcal_match_options* options,
                                lifcal_match_options* resolved);

int lifcal_features_match(const lifcal_features_set* set, uint32_t n_pairs, const uint32_t* pairs, int32_t device, const lifcal_match_options* options,
                          lifcal_match_list* out);

typedef struct lifcal_tracks {
  uint32_t min_length;    /* >= 2; 0 selects 2 */
  uint32_t n_tracks;      /* out */
  uint64_t n_conflicts;   /* out: components dropped because they hold two features of one frame */
  uint64_t capacity;
  uint64_t n;             /* out: observations */
  uint32_t* fr;           /* capacity entries each, or NULL when capacity = 0 */
  uint32_t* pt;
  uint32_t* feature;      /* index into the concatenated list */
} lifcal_tracks;

/* Host only, no device.  offset as in lifcal_features_set; pairs, pair_start, mi, mj as lifcal_features_match took and wrote
 * them.  LIFCAL_BA_ERR_INVALID_ARG for a frame or feature index out of range, a pair (a, a) or a pair_start that descends;
 * nothing outside the arrays is read.  Count-then-fill as above. */
int lifcal_tracks_link(uint32_t n_frames, const uint32_t* offset, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* pair_start,
                       const uint32_t* mi, const uint32_t* mj, lifcal_tracks* io);

#ifdef __cplusplus
}
#endif
#endif
