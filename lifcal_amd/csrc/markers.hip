// markers.hip — fiducial markers in total-focus images (include/lifcal_markers.h), in a code object of its own
// like features.hip (raw_depth.hpp says why).
//
// What runs where.  k_markers_dark: one workgroup per 32 x 32 tile, the pixels with their halo of w in LDS, the box sum separably
// (rows, then columns) in integers.  k_markers_label_tile: union-find of the tile's dark pixels in LDS (atomicMin on the parent
// links, so a root is the lowest index of its set), written out as parent links into the image-wide label array.
// k_markers_seam: the pixels along tile borders unite with their dark neighbours in other tiles, atomicMin on the global parent
// links.  k_markers_flatten: every pixel finds its root and adds one to the root's area.  Roots with area >= min_area are
// compacted in ascending order (hipcub) and get slots; k_markers_extremes: the pixels of slotted components fold their eight
// projections into 64-bit keys (projection, tie-break) with atomicMin / atomicMax, reduced in the wave first when all its
// pixels share one slot.  Every one of these is an integer minimum, maximum or sum, so the order of arrival cannot show.  The
// host filters the candidates (step 3) from the per-slot table and k_markers_decode takes one wave per candidate: lanes take
// cells, then dictionary entries x rotations, then the 48 edge stations; the short double tail (lines, corners, centre) is
// evaluated by every lane alike in the order of the header.
#include "raw_depth.hpp"

#include <hipcub/hipcub.hpp>

#include "markers_host.hpp"

// The kernels below must equal the numpy restatement in every byte, so none of their double steps may be contracted into a fused
// multiply-add.  markers_host.hpp switches contraction off for the code it shares with the device; the same is said here for the
// kernels themselves, so that it does not hang on an included file (the Makefile passes no -ffp-contract flag).
#pragma clang fp contract(off)

namespace lifcal {
namespace markers {

constexpr int kThreads = 256;
constexpr int kPixSide = kTile + 2 * kMaxW;   // 94
constexpr int kMaxCells = (kMaxBits + 2) * (kMaxBits + 2);   // 81
constexpr int kStations = 12, kSamples = 17;

// ------------------------------------------------------------------------------------------------ device side

struct DarkArgs {
  int32_t W, H, w, pad;
  int64_t pitch, C;
  const void* img;
  const uint8_t* status;   // or nullptr
  uint8_t* dark;           // [H][W]
};

template <class T>
__global__ __launch_bounds__(kThreads) void k_markers_dark(DarkArgs a) {
  __shared__ uint16_t s_pix[kPixSide * kPixSide];
  __shared__ uint32_t s_h[kPixSide * kTile];
  const int tid = threadIdx.x, w = a.w, P = kTile + 2 * w;
  const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  const T* __restrict__ img = (const T*)a.img;
  for (int i = tid; i < P * P; i += kThreads) {
    const int px = x0 - w + i % P, py = y0 - w + i / P;
    s_pix[i] = (px >= 0 && px < a.W && py >= 0 && py < a.H) ? (uint16_t)img[(int64_t)py * a.pitch + px] : (uint16_t)0;
  }
  __syncthreads();
  for (int i = tid; i < P * kTile; i += kThreads) {
    const uint16_t* p = s_pix + (i / kTile) * P + (i % kTile);
    uint32_t sum = 0;
    for (int k = 0; k <= 2 * w; ++k) sum += p[k];
    s_h[i] = sum;   // at most 63 * 65535
  }
  __syncthreads();
  for (int i = tid; i < kTile * kTile; i += kThreads) {
    const int cx = i % kTile, cy = i / kTile, x = x0 + cx, y = y0 + cy;
    if (x >= a.W || y >= a.H) continue;
    uint32_t sum = 0;   // at most 63 * 63 * 65535 < 2^28
    for (int k = 0; k <= 2 * w; ++k) sum += s_h[(cy + k) * kTile + cx];
    const long long nx = min(x + w, a.W - 1) - max(x - w, 0) + 1, ny = min(y + w, a.H - 1) - max(y - w, 0) + 1, n = nx * ny;
    const long long v = s_pix[(cy + w) * P + cx + w];
    bool valid = true;
    if (a.status) {
      const uint8_t st = a.status[(int64_t)y * a.W + x];
      valid = st == 0 || st == 3;
    }
    a.dark[(int64_t)y * a.W + x] = (valid && n * v + n * a.C < (long long)sum) ? 1 : 0;
  }
}

// parent links: L[v] <= v, a root has L[v] == v.  Other lanes change links while this one reads them, hence the atomic loads.
__device__ __forceinline__ int uf_find(int* L, int v) {
  int p;
  while ((p = __atomic_load_n(&L[v], __ATOMIC_RELAXED)) != v) v = p;
  return v;
}

// links only ever go to a lower index, so the root of a set is its lowest member whatever the order of the unions
__device__ __forceinline__ void uf_unite(int* L, int a, int b) {
  for (;;) {
    a = uf_find(L, a); b = uf_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(&L[a], b);
    if (old == a) return;
    a = old;   // a had been linked elsewhere meanwhile: its former parent and b still have to meet
  }
}

__global__ __launch_bounds__(kThreads) void k_markers_label_tile(int W, int H, const uint8_t* __restrict__ dark, int* __restrict__ labels) {
  __shared__ int s_lab[kTile * kTile];
  const int tid = threadIdx.x, x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
  for (int i = tid; i < kTile * kTile; i += kThreads) {
    const int x = x0 + i % kTile, y = y0 + i / kTile;
    s_lab[i] = (x < W && y < H && dark[(int64_t)y * W + x]) ? i : -1;
  }
  __syncthreads();
  for (int i = tid; i < kTile * kTile; i += kThreads) {
    if (__atomic_load_n(&s_lab[i], __ATOMIC_RELAXED) < 0) continue;
    const int cx = i % kTile, cy = i / kTile;
    // the four neighbours that come before i; the other four see i from their side
    if (cx > 0 && __atomic_load_n(&s_lab[i - 1], __ATOMIC_RELAXED) >= 0) uf_unite(s_lab, i, i - 1);
    if (cy > 0) {
      if (cx > 0 && __atomic_load_n(&s_lab[i - kTile - 1], __ATOMIC_RELAXED) >= 0) uf_unite(s_lab, i, i - kTile - 1);
      if (__atomic_load_n(&s_lab[i - kTile], __ATOMIC_RELAXED) >= 0) uf_unite(s_lab, i, i - kTile);
      if (cx < kTile - 1 && __atomic_load_n(&s_lab[i - kTile + 1], __ATOMIC_RELAXED) >= 0) uf_unite(s_lab, i, i - kTile + 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < kTile * kTile; i += kThreads) {
    const int x = x0 + i % kTile, y = y0 + i / kTile;
    if (x >= W || y >= H) continue;
    int out = -1;
    if (s_lab[i] >= 0) {
      const int r = uf_find(s_lab, i);   // the order of a tile's cells is that of their linear indices in the image
      out = (y0 + r / kTile) * W + x0 + r % kTile;
    }
    labels[(int64_t)y * W + x] = out;
  }
}

__global__ __launch_bounds__(kThreads) void k_markers_seam(int W, int H, int* labels) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= (int64_t)W * H) return;
  const int x = (int)(p % W), y = (int)(p / W), cx = x % kTile, cy = y % kTile;
  if (cx != 0 && cy != 0 && cx != kTile - 1) return;
  if (__atomic_load_n(&labels[p], __ATOMIC_RELAXED) < 0) return;
  const int dx[4] = {-1, -1, 0, 1}, dy[4] = {0, -1, -1, -1};
  for (int k = 0; k < 4; ++k) {
    const int qx = x + dx[k], qy = y + dy[k];
    if (qx < 0 || qx >= W || qy < 0) continue;
    if (qx / kTile == x / kTile && qy / kTile == y / kTile) continue;   // the tile's own unions are done
    const int64_t q = (int64_t)qy * W + qx;
    if (__atomic_load_n(&labels[q], __ATOMIC_RELAXED) >= 0) uf_unite(labels, (int)p, (int)q);
  }
}

__global__ __launch_bounds__(kThreads) void k_markers_flatten(int64_t N, int* labels, int* area) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p >= N) return;
  if (__atomic_load_n(&labels[p], __ATOMIC_RELAXED) < 0) return;
  const int r = uf_find(labels, (int)p);   // no union runs any more: every link met on the way leads to the final root
  __atomic_store_n(&labels[p], r, __ATOMIC_RELAXED);
  atomicAdd(&area[r], 1);
}

__global__ __launch_bounds__(kThreads) void k_markers_flag(int64_t N, const int* __restrict__ area, int min_area, uint8_t* __restrict__ flag) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (p < N) flag[p] = area[p] >= min_area ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void k_markers_slots(int n, const uint32_t* __restrict__ roots, const int* __restrict__ area, int* __restrict__ slot,
                                                            int* __restrict__ slot_area, unsigned long long* __restrict__ stat) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  const uint32_t r = roots[k];
  slot[r] = k;
  slot_area[k] = area[r];
  for (int j = 0; j < 8; ++j) stat[8 * (int64_t)k + j] = (j & 1) ? 0ull : ~0ull;   // even entries are minima, odd ones maxima
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(v, o); v = u < v ? u : v; }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) { const unsigned long long u = __shfl_xor(v, o); v = u > v ? u : v; }
  return v;
}

// keys: (projection + 2^31) << 32 | tie-break; the tie-break is the linear index for a minimum and its complement for a maximum,
// so that of equal projections the lowest index wins either way
__global__ __launch_bounds__(kThreads) void k_markers_extremes(int W, int H, const int* __restrict__ labels, const int* __restrict__ slot,
                                                               unsigned long long* stat) {
  const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  int s = -1;
  if (p < (int64_t)W * H) {
    const int l = labels[p];
    if (l >= 0) s = slot[l];
  }
  const unsigned long long live = __ballot(s >= 0);
  if (live == 0ull) return;   // the same for the whole wave
  unsigned long long key[8];
  if (s >= 0) {
    const long long x = p % W, y = p / W;
    const long long proj[4] = {x, y, x + y, x - y};
    for (int j = 0; j < 4; ++j) {
      const unsigned long long hi = (unsigned long long)(proj[j] + 2147483648ll) << 32;
      key[2 * j] = hi | (unsigned long long)p;
      key[2 * j + 1] = hi | (unsigned long long)(0xffffffffll - p);
    }
  } else {
    for (int j = 0; j < 8; ++j) key[j] = (j & 1) ? 0ull : ~0ull;
  }
  const int first = __ffsll((long long)live) - 1;
  const int s0 = __shfl(s, first);
  if (__ballot(s >= 0 && s != s0) == 0ull) {   // one slot in the whole wave: one lane speaks for it
    for (int j = 0; j < 8; ++j) key[j] = (j & 1) ? wave_max(key[j]) : wave_min(key[j]);
    if ((int)(threadIdx.x & 63) != first) return;
  } else if (s < 0) {
    return;
  }
  unsigned long long* t = stat + 8 * (int64_t)s;
  for (int j = 0; j < 8; ++j) {
    if (j & 1) atomicMax(&t[j], key[j]);
    else atomicMin(&t[j], key[j]);
  }
}

struct DecodeOut {   // 104 bytes
  int32_t ok, id, rotation, hamming, refined, pad;
  double corners[8], x, y;
};

struct DecodeArgs {
  int32_t W, H, m, n_words, n_cand, min_side, max_border_errors, max_correction;
  int64_t pitch, contrast9;          // 9 * 4096 * C_cell
  double refine_max2;
  const void* img;
  const int32_t* ext;                // [n_cand][8][2]
  const unsigned long long* words;   // [n_words][4]: rot_k of every word
  DecodeOut* out;                    // [n_cand]
};

// a sample of step 5: false where the header rejects (step 5) or skips (step 6)
template <class T>
__device__ __forceinline__ bool sample(const DecodeArgs& a, double X, double Y, long long* value) {
  if (!(fabs(X) < 1048576.0) || !(fabs(Y) < 1048576.0)) return false;
  const long long Sx = (long long)floor(64.0 * X + 0.5), Sy = (long long)floor(64.0 * Y + 0.5);
  const long long ix = Sx >> 6, iy = Sy >> 6, fx = Sx & 63, fy = Sy & 63;
  if (ix < 0 || ix + 1 > a.W - 1 || iy < 0 || iy + 1 > a.H - 1) return false;
  const T* __restrict__ p = (const T*)a.img + iy * a.pitch + ix;
  const long long i00 = p[0], i10 = p[1], i01 = p[a.pitch], i11 = p[a.pitch + 1];
  *value = (64 - fx) * (64 - fy) * i00 + fx * (64 - fy) * i10 + (64 - fx) * fy * i01 + fx * fy * i11;
  return true;
}

// P + q T where line (M, T) meets line (M2, T2); false for parallel lines
__device__ __forceinline__ bool meet(const double* M, const double* T, const double* M2, const double* T2, double* out) {
  const double det = T[0] * T2[1] - T[1] * T2[0];
  if (det == 0.0) return false;
  const double q = ((M2[0] - M[0]) * T2[1] - (M2[1] - M[1]) * T2[0]) / det;
  out[0] = M[0] + q * T[0];
  out[1] = M[1] + q * T[1];
  return true;
}

template <class T>
__global__ __launch_bounds__(kThreads) void k_markers_decode(DecodeArgs a) {
  __shared__ long long s_V[4][kMaxCells];
  __shared__ double s_cx[4][4 * kStations], s_cy[4][4 * kStations];
  __shared__ int s_has[4][4 * kStations];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ci = blockIdx.x * 4 + wv;
  const int m = a.m, n = m + 2;
  bool ok = ci < a.n_cand;   // the same in every lane of a wave, all the way down
  double q[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double ha = 0, hb = 0, hc = 0, hd = 0, he = 0, hf = 0, hg = 0, hh = 0;
  if (ok) ok = choose_quad(a.ext + 16 * (int64_t)ci, a.min_side, q);
  if (ok) {
    const double x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3], x2 = q[4], y2 = q[5], x3 = q[6], y3 = q[7];
    const double dx1 = x1 - x2, dx2 = x3 - x2, sx = ((x0 - x1) + x2) - x3;
    const double dy1 = y1 - y2, dy2 = y3 - y2, sy = ((y0 - y1) + y2) - y3;
    const double den = dx1 * dy2 - dy1 * dx2;
    if (den == 0.0) ok = false;
    else {
      hg = (sx * dy2 - sy * dx2) / den; hh = (dx1 * sy - dy1 * sx) / den;
      ha = (x1 - x0) + hg * x1; hb = (x3 - x0) + hh * x3; hc = x0;
      hd = (y1 - y0) + hg * y1; he = (y3 - y0) + hh * y3; hf = y0;
    }
  }
  // cells
  bool bad = false;
  if (ok) {
    for (int cell = lane; cell < n * n; cell += 64) {
      const int r = cell / n, c = cell % n;
      long long V = 0;
      for (int bv = 0; bv < 3; ++bv)
        for (int bu = 0; bu < 3; ++bu) {
          const double u = (((double)c + 0.25) + (0.5 * ((double)bu + 0.5)) / 3.0) / (double)n;
          const double v = (((double)r + 0.25) + (0.5 * ((double)bv + 0.5)) / 3.0) / (double)n;
          const double w = (hg * u + hh * v) + 1.0;
          long long val = 0;
          if (!(w > 0.0) || !sample<T>(a, ((ha * u + hb * v) + hc) / w, ((hd * u + he * v) + hf) / w, &val)) bad = true;
          V += val;
        }
      s_V[wv][cell] = V;
    }
  }
  if (__ballot(bad) != 0ull) ok = false;
  __syncthreads();
  long long lo = 0, hi = 0;
  unsigned long long word = 0;
  if (ok) {
    long long l = 0x7fffffffffffffffll, h = -1;
    for (int cell = lane; cell < n * n; cell += 64) { const long long V = s_V[wv][cell]; l = V < l ? V : l; h = V > h ? V : h; }
    lo = (long long)wave_min((unsigned long long)l);   // the sums are not negative
    hi = (long long)wave_max((unsigned long long)(h < 0 ? 0 : h));
    if (hi - lo < a.contrast9) ok = false;
  }
  if (ok) {
    int white_border = 0;
    for (int cell = 0; cell < n * n; ++cell) {
      const int r = cell / n, c = cell % n;
      const bool white = 2 * s_V[wv][cell] > lo + hi;
      if (r == 0 || c == 0 || r == n - 1 || c == n - 1) white_border += white ? 1 : 0;
      else if (white) word |= 1ull << ((r - 1) * m + (c - 1));
    }
    if (white_border > a.max_border_errors) ok = false;
  }
  int id = 0, rot = 0, ham = 0;
  if (ok) {
    unsigned long long best = ~0ull;
    for (int e = lane; e < 4 * a.n_words; e += 64) {
      const unsigned long long key = ((unsigned long long)__popcll(word ^ a.words[e]) << 32) | (unsigned long long)e;   // e = 4 j + k
      best = key < best ? key : best;
    }
    best = wave_min(best);
    ham = (int)(best >> 32); id = (int)((best & 0xffffffffull) >> 2); rot = (int)(best & 3ull);
    if (ham > a.max_correction) ok = false;
  }
  double p[8];
  for (int i = 0; i < 4; ++i) { p[2 * i] = q[2 * ((i + rot) & 3)]; p[2 * i + 1] = q[2 * ((i + rot) & 3) + 1]; }
  // stations
  if (ok && lane < 4 * kStations) {
    const int e = lane / kStations, k = lane % kStations;
    const double Ax = p[2 * e], Ay = p[2 * e + 1], Bx = p[2 * ((e + 1) & 3)], By = p[2 * ((e + 1) & 3) + 1];
    const double dx = Bx - Ax, dy = By - Ay, L = __dsqrt_rn(dx * dx + dy * dy);
    const double nx = dy / L, ny = -dx / L;
    const double s = 0.15 + (0.7 * ((double)k + 0.5)) / 12.0;
    const double Px = Ax + s * dx, Py = Ay + s * dy;
    const long long Tt = lo + hi;
    bool has = false, prev_ok = false;
    long long prev = 0;
    double best_o = 0.0;
    for (int i = 0; i < kSamples; ++i) {
      const double o = -4.0 + 0.5 * (double)i;
      long long v = 0;
      const bool here = sample<T>(a, Px + o * nx, Py + o * ny, &v);
      if (here && prev_ok && 18 * prev < Tt && Tt <= 18 * v) {
        const double oc = (-4.0 + 0.5 * (double)(i - 1)) + 0.5 * ((double)(Tt - 18 * prev) / (double)(18 * v - 18 * prev));
        if (!has || fabs(oc) < fabs(best_o)) { has = true; best_o = oc; }
      }
      prev = v; prev_ok = here;
    }
    s_has[wv][lane] = has ? 1 : 0;
    s_cx[wv][lane] = Px + best_o * nx;
    s_cy[wv][lane] = Py + best_o * ny;
  }
  __syncthreads();
  if (!ok) {
    if (ci < a.n_cand && lane == 0) a.out[ci].ok = 0;
    return;
  }
  // lines, corners, centre: every lane alike
  int refined = 1;
  double M[8], D[8], c[8];
  for (int e = 0; e < 4 && refined; ++e) {
    int N = 0;
    double sumx = 0.0, sumy = 0.0;
    for (int k = 0; k < kStations; ++k)
      if (s_has[wv][e * kStations + k]) { ++N; sumx += s_cx[wv][e * kStations + k]; sumy += s_cy[wv][e * kStations + k]; }
    if (N < 4) { refined = 0; break; }
    const double mx = sumx / (double)N, my = sumy / (double)N;
    double sxx = 0.0, sxy = 0.0, syy = 0.0;
    for (int k = 0; k < kStations; ++k)
      if (s_has[wv][e * kStations + k]) {
        const double ddx = s_cx[wv][e * kStations + k] - mx, ddy = s_cy[wv][e * kStations + k] - my;
        sxx += ddx * ddx; sxy += ddx * ddy; syy += ddy * ddy;
      }
    const double lambda = ((sxx + syy) + __dsqrt_rn((sxx - syy) * (sxx - syy) + 4.0 * (sxy * sxy))) / 2.0;
    M[2 * e] = mx; M[2 * e + 1] = my;
    if (sxx >= syy) { D[2 * e] = lambda - syy; D[2 * e + 1] = sxy; }
    else { D[2 * e] = sxy; D[2 * e + 1] = lambda - sxx; }
  }
  for (int e = 0; e < 4 && refined; ++e) {
    const int b = (e + 3) & 3;
    if (!meet(M + 2 * b, D + 2 * b, M + 2 * e, D + 2 * e, c + 2 * e)) { refined = 0; break; }
    const double ddx = c[2 * e] - p[2 * e], ddy = c[2 * e + 1] - p[2 * e + 1];
    if (!(fabs(c[2 * e]) < 1.0e300) || !(fabs(c[2 * e + 1]) < 1.0e300) || ddx * ddx + ddy * ddy > a.refine_max2) refined = 0;
  }
  if (refined)
    for (int i = 0; i < 8; ++i) p[i] = c[i];
  const double T1[2] = {p[4] - p[0], p[5] - p[1]}, T2[2] = {p[6] - p[2], p[7] - p[3]};
  double ctr[2] = {0.0, 0.0};
  const bool have = meet(p, T1, p + 2, T2, ctr);
  if (lane == 0) {
    DecodeOut o;
    o.ok = have ? 1 : 0; o.id = id; o.rotation = rot; o.hamming = ham; o.refined = refined; o.pad = 0;
    for (int i = 0; i < 8; ++i) o.corners[i] = p[i];
    o.x = ctr[0]; o.y = ctr[1];
    a.out[ci] = o;
  }
}

// ------------------------------------------------------------------------------------------------ host side

static int fail_hip(const char* who, hipError_t e) { return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e)); }

struct DeviceBuffers {
  std::vector<void*> q;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
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

// steps 1 to 3 on the device, then (with a dictionary) steps 4 to 7.  comps: the candidates; dark, labels: host maps or nullptr.
static int run(const char* who, const lifcal_rawdepth_image* image, const uint8_t* status, int32_t device, const Plan& t, const lifcal_marker_dictionary* dict,
               uint8_t* dark_out, int32_t* labels_out, std::vector<lifcal_marker_component>* comps, std::vector<DecodeOut>* decoded, double* seconds) {
  if (!set_device(device)) return fail(LIFCAL_BA_ERR_NO_DEVICE, std::string(who) + ": no HIP device (this path has no CPU fallback)");
  const int W = image->width, H = image->height;
  const int64_t N = (int64_t)W * H;
  const size_t es = t.bits == 8 ? 1 : 2;
  const unsigned pix_blocks = (unsigned)((N + kThreads - 1) / kThreads);
  const dim3 tiles((unsigned)t.tx, (unsigned)t.ty), blk(kThreads);
  if (t.ty > 65535) return fail(LIFCAL_BA_ERR_OUT_OF_RANGE, std::string(who) + ": more than 65535 tile rows");
  DeviceBuffers buf;
  DarkArgs a{};
  a.W = W; a.H = H; a.w = t.opt.w; a.C = t.C;
  hipError_t e = hipSuccess;
  if (image->on_device) {
    a.img = image->data; a.pitch = image->pitch; a.status = status;
  } else {
    void* d = nullptr;
    e = buf.alloc(&d, (size_t)N * es);
    if (e == hipSuccess) e = hipMemcpy2D(d, W * es, image->data, (size_t)image->pitch * es, W * es, (size_t)H, hipMemcpyHostToDevice);
    a.img = d; a.pitch = W;
    if (e == hipSuccess && status) e = buf.upload(&a.status, status, (size_t)N);
  }
  int *labels = nullptr, *area = nullptr, *slot = nullptr, *slot_area = nullptr, *d_n = nullptr;
  uint8_t* flag = nullptr;
  uint32_t* roots = nullptr;
  unsigned long long* stat = nullptr;
  void* scratch = nullptr;
  size_t scratch_bytes = 0;
  const size_t cap = (size_t)t.max_candidates + 1;
  hipcub::CountingInputIterator<uint32_t> ids(0u);
  if (e == hipSuccess) e = buf.alloc(&a.dark, (size_t)N);
  if (e == hipSuccess) e = buf.alloc(&labels, (size_t)N * sizeof(int));
  if (e == hipSuccess) e = buf.alloc(&area, (size_t)N * sizeof(int));
  if (e == hipSuccess) e = buf.alloc(&slot, (size_t)N * sizeof(int));
  if (e == hipSuccess) e = buf.alloc(&flag, (size_t)N);
  if (e == hipSuccess) e = buf.alloc(&roots, cap * sizeof(uint32_t));
  if (e == hipSuccess) e = buf.alloc(&slot_area, cap * sizeof(int));
  if (e == hipSuccess) e = buf.alloc(&stat, cap * 8 * sizeof(unsigned long long));
  if (e == hipSuccess) e = buf.alloc(&d_n, sizeof(int));
  if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged(nullptr, scratch_bytes, ids, flag, roots, d_n, (int)N);
  if (e == hipSuccess) e = buf.alloc(&scratch, scratch_bytes);
  if (e == hipSuccess) e = buf.events();
  if (e != hipSuccess) return fail_hip(who, e);

  e = hipEventRecord(buf.ev[0], 0);
  if (e == hipSuccess) e = hipMemsetAsync(area, 0, (size_t)N * sizeof(int), 0);
  if (e == hipSuccess) e = hipMemsetAsync(slot, 0xff, (size_t)N * sizeof(int), 0);
  if (e != hipSuccess) return fail_hip(who, e);
  if (t.bits == 8) hipLaunchKernelGGL((k_markers_dark<uint8_t>), tiles, blk, 0, 0, a);
  else hipLaunchKernelGGL((k_markers_dark<uint16_t>), tiles, blk, 0, 0, a);
  hipLaunchKernelGGL(k_markers_label_tile, tiles, blk, 0, 0, W, H, (const uint8_t*)a.dark, labels);
  hipLaunchKernelGGL(k_markers_seam, dim3(pix_blocks), blk, 0, 0, W, H, labels);
  hipLaunchKernelGGL(k_markers_flatten, dim3(pix_blocks), blk, 0, 0, N, labels, area);
  hipLaunchKernelGGL(k_markers_flag, dim3(pix_blocks), blk, 0, 0, N, (const int*)area, (int)t.opt.min_area, flag);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipcub::DeviceSelect::Flagged(scratch, scratch_bytes, ids, flag, roots, d_n, (int)N);
  if (e == hipSuccess) e = hipEventRecord(buf.ev[1], 0);
  int n_slots = 0;
  if (e == hipSuccess) e = hipMemcpy(&n_slots, d_n, sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail_hip(who, e);
  if (n_slots < 0 || (int64_t)n_slots > t.max_candidates) return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": an impossible number of components");
  float ms = 0.0f;
  e = hipEventElapsedTime(&ms, buf.ev[0], buf.ev[1]);
  if (e != hipSuccess) return fail_hip(who, e);
  *seconds = 1.0e-3 * (double)ms;
  if (dark_out) e = hipMemcpy(dark_out, a.dark, (size_t)N, hipMemcpyDeviceToHost);
  comps->clear();
  if (n_slots > 0) {
    if (e == hipSuccess) e = hipEventRecord(buf.ev[2], 0);
    if (e != hipSuccess) return fail_hip(who, e);
    hipLaunchKernelGGL(k_markers_slots, dim3((unsigned)((n_slots + kThreads - 1) / kThreads)), blk, 0, 0, n_slots, (const uint32_t*)roots, (const int*)area, slot,
                       slot_area, stat);
    hipLaunchKernelGGL(k_markers_extremes, dim3(pix_blocks), blk, 0, 0, W, H, (const int*)labels, (const int*)slot, stat);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(buf.ev[3], 0);
    std::vector<uint32_t> h_roots((size_t)n_slots);
    std::vector<int> h_area((size_t)n_slots);
    std::vector<unsigned long long> h_stat((size_t)n_slots * 8);
    if (e == hipSuccess) e = hipMemcpy(h_roots.data(), roots, h_roots.size() * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_area.data(), slot_area, h_area.size() * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_stat.data(), stat, h_stat.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, buf.ev[2], buf.ev[3]);
    if (e != hipSuccess) return fail_hip(who, e);
    *seconds += 1.0e-3 * (double)ms;
    for (int k = 0; k < n_slots; ++k) {
      lifcal_marker_component c{};
      c.label = (int32_t)h_roots[(size_t)k];
      c.area = h_area[(size_t)k];
      for (int j = 0; j < 8; ++j) {
        const uint64_t low = h_stat[8 * (size_t)k + j] & 0xffffffffull;
        const int64_t idx = (j & 1) ? (int64_t)(0xffffffffull - low) : (int64_t)low;
        if (idx < 0 || idx >= N) return fail(LIFCAL_BA_ERR_HIP, std::string(who) + ": an extreme pixel lies outside the image");
        c.ext[j][0] = (int32_t)(idx % W); c.ext[j][1] = (int32_t)(idx / W);
      }
      if (is_candidate(&c, t.opt, W, H)) comps->push_back(c);
    }
  }
  if (e == hipSuccess && labels_out) e = hipMemcpy(labels_out, labels, (size_t)N * sizeof(int), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail_hip(who, e);
  if (!dict || !decoded) return 0;
  decoded->assign(comps->size(), DecodeOut{});
  if (comps->empty()) return 0;

  const size_t nc = comps->size();
  std::vector<int32_t> ext(nc * 16);
  for (size_t k = 0; k < nc; ++k) std::memcpy(&ext[16 * k], (*comps)[k].ext, 16 * sizeof(int32_t));
  std::vector<unsigned long long> words((size_t)dict->n * 4);
  for (uint32_t j = 0; j < dict->n; ++j) {
    uint64_t r = dict->words[j];
    for (int k = 0; k < 4; ++k) { words[4 * (size_t)j + k] = r; r = rot_word(r, dict->marker_bits); }
  }
  DecodeArgs d{};
  d.W = W; d.H = H; d.m = dict->marker_bits; d.n_words = (int32_t)dict->n; d.n_cand = (int32_t)nc; d.min_side = t.opt.min_side;
  d.max_border_errors = t.opt.max_border_errors; d.max_correction = t.opt.max_correction;
  d.pitch = a.pitch; d.contrast9 = 9 * 4096 * t.C_cell; d.refine_max2 = t.opt.refine_max * t.opt.refine_max; d.img = a.img;
  e = buf.upload(&d.ext, ext.data(), ext.size());
  if (e == hipSuccess) e = buf.upload(&d.words, words.data(), words.size());
  if (e == hipSuccess) e = buf.alloc(&d.out, nc * sizeof(DecodeOut));
  if (e == hipSuccess) e = hipEventRecord(buf.ev[4], 0);
  if (e != hipSuccess) return fail_hip(who, e);
  const dim3 grd((unsigned)((nc + 3) / 4));
  if (t.bits == 8) hipLaunchKernelGGL((k_markers_decode<uint8_t>), grd, blk, 0, 0, d);
  else hipLaunchKernelGGL((k_markers_decode<uint16_t>), grd, blk, 0, 0, d);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipEventRecord(buf.ev[5], 0);
  if (e == hipSuccess) e = hipMemcpy(decoded->data(), d.out, nc * sizeof(DecodeOut), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, buf.ev[4], buf.ev[5]);
  if (e != hipSuccess) return fail_hip(who, e);
  *seconds += 1.0e-3 * (double)ms;
  return 0;
}

}  // namespace markers
}  // namespace lifcal

extern "C" {

using namespace lifcal::markers;

int lifcal_markers_check(const lifcal_rawdepth_image* image, const lifcal_marker_dictionary* dictionary, const lifcal_markers_options* options,
                         lifcal_markers_plan* plan) {
  Plan t;
  if (int rc = make_plan("lifcal_markers_check", image, dictionary, options, &t)) return rc;
  if (plan) fill_plan(t, plan);
  return 0;
}

int lifcal_markers_detect(const lifcal_rawdepth_image* image, const uint8_t* status, int32_t device, const lifcal_marker_dictionary* dictionary,
                          const lifcal_markers_options* options, lifcal_marker_list* out) {
  const char* who = "lifcal_markers_detect";
  if (!out) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no result");
  if (!dictionary) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no dictionary");
  Plan t;
  if (int rc = make_plan(who, image, dictionary, options, &t)) return rc;
  out->n = 0; out->n_candidates = 0; out->seconds = 0.0;
  std::vector<lifcal_marker_component> comps;
  std::vector<DecodeOut> dec;
  if (int rc = run(who, image, status, device, t, dictionary, nullptr, nullptr, &comps, &dec, &out->seconds)) return rc;
  out->n_candidates = comps.size();
  uint64_t n = 0;
  for (const DecodeOut& d : dec) n += d.ok ? 1 : 0;
  out->n = n;
  if (out->capacity < n) return LIFCAL_MLA_MORE;
  if (n && !out->markers) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no output array");
  uint64_t k = 0;
  for (size_t i = 0; i < dec.size(); ++i) {
    const DecodeOut& d = dec[i];
    if (!d.ok) continue;
    lifcal_marker& mk = out->markers[k++];
    mk.id = d.id; mk.rotation = d.rotation; mk.hamming = d.hamming; mk.refined = d.refined;
    mk.label = comps[i].label; mk.area = comps[i].area;
    for (int c = 0; c < 8; ++c) mk.corners[c / 2][c % 2] = d.corners[c];
    mk.x = d.x; mk.y = d.y;
  }
  return 0;
}

int lifcal_markers_components(const lifcal_rawdepth_image* image, const uint8_t* status, int32_t device, const lifcal_markers_options* options,
                              lifcal_marker_components* out) {
  const char* who = "lifcal_markers_components";
  if (!out) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no result");
  Plan t;
  if (int rc = make_plan(who, image, nullptr, options, &t)) return rc;
  out->n = 0; out->seconds = 0.0;
  std::vector<lifcal_marker_component> comps;
  if (int rc = run(who, image, status, device, t, nullptr, out->dark, out->labels, &comps, nullptr, &out->seconds)) return rc;
  out->n = comps.size();
  if (out->capacity < out->n) return LIFCAL_MLA_MORE;
  if (out->n && !out->comp) return fail(LIFCAL_BA_ERR_INVALID_ARG, std::string(who) + ": no output array");
  std::copy(comps.begin(), comps.end(), out->comp);
  return 0;
}

int lifcal_marker_dictionary_distance(const lifcal_marker_dictionary* dictionary, int32_t* min_distance) {
  if (int rc = check_dictionary("lifcal_marker_dictionary_distance: ", dictionary)) return rc;
  if (min_distance) *min_distance = dictionary_distance(dictionary);
  return 0;
}

int lifcal_marker_dictionary_generate(int32_t marker_bits, uint32_t n, uint32_t seed, uint64_t* out, int32_t* min_distance) {
  return generate_dictionary(marker_bits, n, seed, out, min_distance);
}

int lifcal_constraints_read(const char* path, lifcal_constraints* io) { return read_constraints(path, io); }

int lifcal_markers_seed_points(uint64_t n_markers, const double* mx, const double* my, const uint32_t* mfr, const uint32_t* mid, uint64_t n_tracked,
                               const double* tx, const double* ty, const uint32_t* tfr, const uint32_t* tpt, uint64_t n_points, const double* pts,
                               lifcal_marker_seeds* io) {
  return seed_points(n_markers, mx, my, mfr, mid, n_tracked, tx, ty, tfr, tpt, n_points, pts, io);
}

int lifcal_scene_scale_factor(const double* p1, const double* p2, double distance, double* factor) { return scale_factor(p1, p2, distance, factor); }

}  // extern "C"
