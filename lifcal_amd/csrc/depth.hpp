// depth.hpp — virtual depth in and metric depth out (include/lifcal_depth.h, lifcal_ba_object_space_stats of include/lifcal_ba.h).
// Included at the end of lifcal_ba.hip (uses its g_last_error / error codes / lifcal_ba_handle, mla::select_device and
// frame_eval / f32x2 of device_model.hpp).
//
//   k_depth_sample    readDepthData per image point (src/CameraCalibration.cpp:385-448), one lane per point
//   k_depth_points    projectPointBack (src/CameraModel.h:26-81) per image point, fp64, with the forward-mode Jacobian
//   k_depth_dense     the same for every pixel of a batch of depth maps: four consecutive pixels per lane, fp64 or packed fp32
//   k_object_space    reference and back-projected camera coordinates of image points at a solver handle's parameters
// The fp64 paths repeat the reference's operations in its order with contraction off (`#pragma clang fp contract(off)`, as
// mla.hpp), so they are bit-identical to a line-by-line restatement.
#pragma once
#include "../../include/lifcal_depth.h"

namespace depth {

using lifcal::f32x2;
using lifcal::pk;
using lifcal::pk1;

// the coding of the depth images (:391-396): iv = 1 - value / 65535 is the inverse virtual depth, valid in (0, 0.5]
LIFCAL_DEV bool decode(uint32_t value, double& iv) {
#pragma clang fp contract(off)
  iv = 0.0;
  if (value == 0) return false;
  iv = (double)value / 65535.0;
  iv = 1.0 - iv;
  return iv <= 0.5 && iv > 0.0;
}

struct SampleArgs {
  const uint16_t* maps;
  int32_t W, H;
  uint64_t n;
  const double* x; const double* y; const int32_t* map_index;
  double* out;
  unsigned long long* counts;   // direct, interpolated, failed
};

__global__ __launch_bounds__(256) void k_depth_sample(SampleArgs a) {
#pragma clang fp contract(off)
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int cls = -1;
  if (i < a.n) {
    double r = -1.0;
    cls = 2;
    const double tx = a.x[i] + 0.5, ty = a.y[i] + 0.5;
    if (tx > -1.0e9 && tx < 1.0e9 && ty > -1.0e9 && ty < 1.0e9) {   // (also false for NaN)
      const int cx = (int)tx, cy = (int)ty;
      if (cx >= 0 && cx < a.W && cy >= 0 && cy < a.H) {
        const uint16_t* m = a.maps + (size_t)a.map_index[i] * a.W * a.H;
        double iv;
        if (decode(m[cx + (size_t)cy * a.W], iv)) { r = 1.0 / iv; cls = 0; }
        else {
          for (int dist = 1; dist < 50; ++dist) {
            int num = 0;
            double sum = 0.0;
            const int x0 = cx - dist < 0 ? 0 : cx - dist, x1 = cx + dist >= a.W ? a.W - 1 : cx + dist;
            const int y0 = cy - dist < 0 ? 0 : cy - dist, y1 = cy + dist >= a.H ? a.H - 1 : cy + dist;
            for (int x = x0; x <= x1; ++x)
              for (int y = y0; y <= y1; ++y)
                if (decode(m[x + (size_t)y * a.W], iv)) { ++num; sum += iv; }
            if (num >= 10) { r = (double)num / sum; cls = 1; break; }
          }
        }
      }
    }
    a.out[i] = r;
  }
  for (int k = 0; k < 3; ++k) {
    const unsigned long long mask = __ballot(cls == k);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&a.counts[k], (unsigned long long)__popcll(mask));
  }
}

// ---- forward-mode number: value + N partials ----
template <int N>
struct Dual {
  double v;
  double d[N];
  LIFCAL_DEV Dual() {}
  LIFCAL_DEV Dual(double c) : v(c) {
#pragma unroll
    for (int i = 0; i < N; ++i) d[i] = 0.0;
  }
};
template <int N> LIFCAL_DEV Dual<N> operator+(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r; r.v = a.v + b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
template <int N> LIFCAL_DEV Dual<N> operator-(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r; r.v = a.v - b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
template <int N> LIFCAL_DEV Dual<N> operator*(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r; r.v = a.v * b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
template <int N> LIFCAL_DEV Dual<N> operator/(const Dual<N>& a, const Dual<N>& b) {
  Dual<N> r;
  const double ib = 1.0 / b.v;
  r.v = a.v / b.v;
#pragma unroll
  for (int i = 0; i < N; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * ib;
  return r;
}

// CameraModel::projectPointBack (src/CameraModel.h:26-81) with radialDistortion / tangentialDistortion (:205-241), operation by
// operation.  T = double (the value, bit-identical to the reference) or Dual<N> (the derivative of the iteration as executed; the
// reference templates on T for the same reason).  nr, tan: wave-uniform.
template <class T>
LIFCAL_DEV void back_project(const T& x_v, const T& y_v, const T& v_depth, const T& spx, const T& spy, const T& fL, const T& bL0, const T& B,
                             const T& c_x, const T& c_y, const T& k0, const T& k1, const T& p0, const T& p1, int nr, bool tan, T out[3]) {
#pragma clang fp contract(off)
  T px = (x_v - c_x) * spx;
  T py = (y_v - c_y) * spy;
  T pz = v_depth * B;
  px = (px / (bL0 + pz)) * bL0;
  py = (py / (bL0 + pz)) * bL0;
  if (nr > 0 || tan) {
    const T xd = px, yd = py;
    const T two(2.0);
    T drx(0.0), dry(0.0), dtx(0.0), dty(0.0);
    for (int i = 0; i < 10; ++i) {
      if (nr > 0) {
        const T r0 = px * px + py * py;
        T dr = k0 * r0;
        if (nr > 1) { const T r1 = r0 * r0; dr = dr + k1 * r1; }
        drx = px * dr; dry = py * dr;
      }
      if (tan) {
        const T r2 = px * px + py * py;
        dtx = p0 * (r2 + two * px * px) + two * p1 * px * py;
        dty = p1 * (r2 + two * py * py) + two * p0 * px * py;
      }
      px = xd - drx - dtx;
      py = yd - dry - dty;
    }
  }
  pz = pz + bL0;
  out[2] = fL * pz / (pz - fL);
  out[0] = px / bL0 * out[2];
  out[1] = py / bL0 * out[2];
}

// p_w = R^T (p_c - t) with the frame-table entry of frame_eval (R row-major at [0..8], t at [9..11])
template <class FT>
LIFCAL_DEV void to_world(const FT& ft, const double p[3], double w[3]) {
#pragma clang fp contract(off)
  const double d0 = p[0] - ft[9], d1 = p[1] - ft[10], d2 = p[2] - ft[11];
#pragma unroll
  for (int j = 0; j < 3; ++j) w[j] = ft[j] * d0 + ft[3 + j] * d1 + ft[6 + j] * d2;
}

struct PointsArgs {
  uint64_t n;
  const double* x; const double* y; const double* vd;
  const uint32_t* fr; const double* views;
  const double* G; double sigma_v;
  double* pc; double* pw; double* jac; double* dv; double* cov;
  unsigned long long* n_invalid;
  lifcal_depth_camera cam;
};

__global__ __launch_bounds__(256) void k_depth_points(PointsArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int nr = (int)(a.cam.config & 3u);
  const bool tan = (a.cam.config & 4u) != 0;
  const double* c = a.cam.cam;
  bool bad = false;
  if (i < a.n) {
    const double v = a.vd[i];
    bad = !(v > 0.0);
    const double nan = __builtin_nan("");
    if (bad) {
      for (int r = 0; r < 3; ++r) { a.pc[3 * i + r] = nan; if (a.pw) a.pw[3 * i + r] = nan; if (a.dv) a.dv[3 * i + r] = nan; }
      if (a.jac) for (int e = 0; e < 51; ++e) a.jac[51 * i + e] = nan;
      if (a.cov) for (int e = 0; e < 6; ++e) a.cov[6 * i + e] = nan;
    } else {
      const double k0 = nr > 0 ? c[5] : 0.0, k1 = nr > 1 ? c[6] : 0.0, p0 = tan ? c[5 + nr] : 0.0, p1 = tan ? c[6 + nr] : 0.0;
      double p[3];
      back_project<double>(a.x[i], a.y[i], v, a.cam.spx, a.cam.spy, c[0], c[1], c[2], c[3], c[4], k0, k1, p0, p1, nr, tan, p);
      for (int r = 0; r < 3; ++r) a.pc[3 * i + r] = p[r];
      if (a.pw) {
        double ft[16], w[3];
        lifcal::frame_eval(a.views + 6 * (size_t)a.fr[i], ft);
        to_world(ft, p, w);
        for (int r = 0; r < 3; ++r) a.pw[3 * i + r] = w[r];
      }
      if (a.jac) {
        // seeds in chunks of three: slots 0..16 of cam, slot 17 = the virtual depth
        typedef Dual<3> D;
        const int s_k0 = nr > 0 ? 5 : -1, s_k1 = nr > 1 ? 6 : -1, s_p0 = tan ? 5 + nr : -1, s_p1 = tan ? 6 + nr : -1;
        for (int ch = 0; ch < 6; ++ch) {
          auto mk = [&](double val, int slot) { D r(val); for (int e = 0; e < 3; ++e) r.d[e] = (slot == 3 * ch + e) ? 1.0 : 0.0; return r; };
          D o[3];
          back_project<D>(D(a.x[i]), D(a.y[i]), mk(v, 17), D(a.cam.spx), D(a.cam.spy), mk(c[0], 0), mk(c[1], 1), mk(c[2], 2), mk(c[3], 3), mk(c[4], 4),
                          mk(k0, s_k0), mk(k1, s_k1), mk(p0, s_p0), mk(p1, s_p1), nr, tan, o);
          for (int e = 0; e < 3; ++e) {
            const int s = 3 * ch + e;
            for (int r = 0; r < 3; ++r) {
              if (s < 17) a.jac[51 * i + 17 * r + s] = o[r].d[e];
              else if (a.dv) a.dv[3 * i + r] = o[r].d[e];
            }
          }
        }
        if (a.cov) {
          const double* J = a.jac + 51 * i;
          double q[6] = {0, 0, 0, 0, 0, 0};
          for (int j = 0; j < 17; ++j) {
            double t0 = 0, t1 = 0, t2 = 0;
            for (int k = 0; k < 17; ++k) { const double g = a.G[17 * j + k]; t0 += g * J[k]; t1 += g * J[17 + k]; t2 += g * J[34 + k]; }
            q[0] += J[j] * t0; q[1] += J[j] * t1; q[2] += J[j] * t2; q[3] += J[17 + j] * t1; q[4] += J[17 + j] * t2; q[5] += J[34 + j] * t2;
          }
          const double s2 = a.sigma_v * a.sigma_v, d0 = a.dv[3 * i], d1 = a.dv[3 * i + 1], d2 = a.dv[3 * i + 2];
          q[0] += s2 * d0 * d0; q[1] += s2 * d0 * d1; q[2] += s2 * d0 * d2; q[3] += s2 * d1 * d1; q[4] += s2 * d1 * d2; q[5] += s2 * d2 * d2;
          for (int e = 0; e < 6; ++e) a.cov[6 * i + e] = q[e];
        }
      }
    }
  }
  const unsigned long long mask = __ballot(bad);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(a.n_invalid, (unsigned long long)__popcll(mask));
}

// frame-table entries (frame_eval) of the frames of a batch of maps
__global__ void k_depth_frames(const double* views, const uint32_t* frame, int count, double* ftab) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < count) lifcal::frame_eval(views + 6 * (size_t)frame[m], ftab + 16 * (size_t)m);
}

// ---- the dense path ----
template <class T>
struct DenseCam {
  T fL, bL0, B, cx, cy, k0, k1, p0, p1, spx, spy;
  T G[6];   // {fL, bL0, B} block of the camera covariance: 00 01 02 11 12 22
  T sv2;    // sigma_v^2
};

struct DenseArgs {
  const uint16_t* maps;   // first pixel of the first map of the batch
  uint32_t npix, W, HW;
  int32_t vec_in;         // maps is 8-byte aligned: four values per load
  const double* ftab;     // [count][16] or NULL (camera coordinates)
  void* xyz; void* z; void* sz;
  unsigned long long* n_invalid;
  DenseCam<double> c64;
  DenseCam<float> c32;
};

constexpr int kPixPerLane = 4;

struct Pixel64 { double p[3], zc, sz; };

// one pixel in fp64: the reference's operations (decode + back_project + to_world), then the closed form of sigma_z
template <int NR, bool TAN>
LIFCAL_DEV bool dense_pixel_f64(const DenseCam<double>& c, uint32_t value, uint32_t col, uint32_t row, bool world, const double (&ft)[12], bool want_sz, Pixel64& o) {
#pragma clang fp contract(off)
  double iv;
  if (!decode(value, iv)) return false;
  const double v = 1.0 / iv;
  double p[3];
  back_project<double>((double)col, (double)row, v, c.spx, c.spy, c.fL, c.bL0, c.B, c.cx, c.cy, c.k0, c.k1, c.p0, c.p1, NR, TAN, p);
  o.zc = p[2];
  if (world) to_world(ft, p, o.p);
  else { o.p[0] = p[0]; o.p[1] = p[1]; o.p[2] = p[2]; }
  if (want_sz) {
    const double b = c.bL0 + v * c.B, d = b - c.fL, id2 = 1.0 / (d * d);
    const double q = c.fL * c.fL * id2;
    const double g0 = b * b * id2, g1 = -q, g2 = -v * q, gv = -c.B * q;
    const double s2 = g0 * (c.G[0] * g0 + 2.0 * (c.G[1] * g1 + c.G[2] * g2)) + g1 * (c.G[3] * g1 + 2.0 * c.G[4] * g2) + g2 * c.G[5] * g2 + gv * gv * c.sv2;
    o.sz = sqrt(s2 > 0.0 ? s2 : 0.0);
  }
  return true;
}

// one pixel in fp32: (x, y) are one packed pair through the undistortion (v_pk_mul_f32 / v_pk_fma_f32), two divisions per pixel.
// The valid set is that of decode(): 1 - value / 65535 in (0, 0.5] holds exactly for 32768 <= value <= 65534.
template <int NR, bool TAN>
LIFCAL_DEV bool dense_pixel_f32(const DenseCam<float>& c, uint32_t value, uint32_t col, uint32_t row, bool world, const float (&ft)[12], bool want_sz, float (&p)[3], float& zc, float& sz) {
  if (value < 32768u || value > 65534u) return false;
  const float v = 65535.0f / (float)(65535u - value);
  const float b = c.bL0 + v * c.B;
  f32x2 xy = (pk((float)col, (float)row) - pk(c.cx, c.cy)) * pk(c.spx, c.spy);
  xy = xy * (c.bL0 / b);
  if (NR > 0 || TAN) {
    const f32x2 xyd = xy;
    const f32x2 pT = pk(c.p0, c.p1), pS = pk(c.p1, c.p0);
#pragma unroll
    for (int i = 0; i < 10; ++i) {
      const f32x2 pp = xy * xy;
      const float r2 = pp.x + pp.y;
      f32x2 delta = pk1(0.f);
      if (NR > 0) { float dr = c.k0 * r2; if (NR > 1) dr += c.k1 * (r2 * r2); delta = xy * dr; }
      if (TAN) delta += pT * (pk1(r2) + pp * 2.f) + pS * (2.f * (xy.x * xy.y));
      xy = xyd - delta;
    }
  }
  const float d = b - c.fL;
  const float Z = c.fL * b / d;
  xy = xy * (Z * (1.0f / c.bL0));
  zc = Z;
  if (world) {
    const float d0 = xy.x - ft[9], d1 = xy.y - ft[10], d2 = Z - ft[11];
#pragma unroll
    for (int j = 0; j < 3; ++j) p[j] = ft[j] * d0 + ft[3 + j] * d1 + ft[6 + j] * d2;
  } else { p[0] = xy.x; p[1] = xy.y; p[2] = Z; }
  if (want_sz) {
    const float id2 = 1.0f / (d * d), q = c.fL * c.fL * id2;
    const float g0 = b * b * id2, g1 = -q, g2 = -v * q, gv = -c.B * q;
    const float s2 = g0 * (c.G[0] * g0 + 2.f * (c.G[1] * g1 + c.G[2] * g2)) + g1 * (c.G[3] * g1 + 2.f * c.G[4] * g2) + g2 * c.G[5] * g2 + gv * gv * c.sv2;
    sz = sqrtf(s2 > 0.f ? s2 : 0.f);
  }
  return true;
}

// Four consecutive pixels per lane (one 8-byte load of the raw values), 1024 per workgroup.  xyz goes through LDS so that every
// store instruction of a wave covers one contiguous kilobyte; z / sigma_z are 16 or 32 contiguous bytes per lane as they are.
template <int NR, bool TAN, bool F32, class OT>
__global__ __launch_bounds__(256) void k_depth_dense(DenseArgs a) {
  constexpr int WAVE_ELEMS = 64 * kPixPerLane * 3;
  constexpr int VEC = 16 / (int)sizeof(OT);
  typedef OT ovec __attribute__((ext_vector_type(VEC)));
  __shared__ __attribute__((aligned(16))) OT s_xyz[4][WAVE_ELEMS];
  __shared__ uint32_t s_cnt[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t wave_base = blockIdx.x * (256u * kPixPerLane) + wave * (64u * kPixPerLane);
  const uint32_t base = wave_base + lane * kPixPerLane;
  const bool want_sz = a.sz != nullptr;
  const OT nan = (OT)__builtin_nanf("");

  uint32_t raw[kPixPerLane] = {0, 0, 0, 0};
  if (a.vec_in && base + kPixPerLane <= a.npix) {
    const ushort4 q = *reinterpret_cast<const ushort4*>(a.maps + base);
    raw[0] = q.x; raw[1] = q.y; raw[2] = q.z; raw[3] = q.w;
  } else {
    for (int j = 0; j < kPixPerLane; ++j) if (base + j < a.npix) raw[j] = a.maps[base + j];
  }
  uint32_t m = 0, col = 0, row = 0;
  if (base < a.npix) { m = base / a.HW; const uint32_t rem = base - m * a.HW; row = rem / a.W; col = rem - row * a.W; }
  const uint32_t H = a.HW / a.W;
  const bool world = a.ftab != nullptr;
  double ft64[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  float ft32[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  auto load_frame = [&]() {
    if (!world) return;
#pragma unroll
    for (int e = 0; e < 12; ++e) { const double t = a.ftab[16 * (size_t)m + e]; if (F32) ft32[e] = (float)t; else ft64[e] = t; }
  };
  load_frame();

  OT zv[kPixPerLane], sv[kPixPerLane];
  uint32_t invalid = 0;
#pragma unroll
  for (int j = 0; j < kPixPerLane; ++j) {
    OT p[3] = {nan, nan, nan};
    zv[j] = nan; sv[j] = nan;
    if (base + j < a.npix) {
      bool ok;
      if (F32) {
        float pf[3], zc = 0.f, sz = 0.f;
        ok = dense_pixel_f32<NR, TAN>(a.c32, raw[j], col, row, world, ft32, want_sz, pf, zc, sz);
        if (ok) { p[0] = (OT)pf[0]; p[1] = (OT)pf[1]; p[2] = (OT)pf[2]; zv[j] = (OT)zc; sv[j] = (OT)sz; }
      } else {
        Pixel64 o; o.sz = 0.0;
        ok = dense_pixel_f64<NR, TAN>(a.c64, raw[j], col, row, world, ft64, want_sz, o);
        if (ok) { p[0] = (OT)o.p[0]; p[1] = (OT)o.p[1]; p[2] = (OT)o.p[2]; zv[j] = (OT)o.zc; sv[j] = (OT)o.sz; }
      }
      if (!ok) ++invalid;
      if (++col == a.W) { col = 0; if (++row == H) { row = 0; ++m; if (base + j + 1 < a.npix) load_frame(); } }
    }
    OT* s = &s_xyz[wave][(lane * kPixPerLane + j) * 3];
    s[0] = p[0]; s[1] = p[1]; s[2] = p[2];
  }
  // invalid pixels: one sum per wave, one atomic per workgroup
  for (int off = 32; off > 0; off >>= 1) invalid += __shfl_xor(invalid, off);
  if (lane == 0) s_cnt[wave] = invalid;
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (t) atomicAdd(a.n_invalid, (unsigned long long)t);
  }
  if (wave_base >= a.npix) return;
  if (a.xyz) {
    const uint32_t left = a.npix - wave_base;
    const uint32_t elems = left >= 64u * kPixPerLane ? (uint32_t)WAVE_ELEMS : left * 3u;
    OT* dst = (OT*)a.xyz + (size_t)wave_base * 3;
    for (uint32_t e = lane * VEC; e < elems; e += 64u * VEC) {
      if (e + VEC <= elems) *reinterpret_cast<ovec*>(dst + e) = *reinterpret_cast<const ovec*>(&s_xyz[wave][e]);
      else for (uint32_t t = e; t < elems; ++t) dst[t] = s_xyz[wave][t];
    }
  }
  if (base < a.npix) {
    typedef OT ovec4 __attribute__((ext_vector_type(4)));
    const bool full = base + kPixPerLane <= a.npix;
    for (int which = 0; which < 2; ++which) {
      OT* out = (OT*)(which ? a.sz : a.z);
      const OT* val = which ? sv : zv;
      if (!out) continue;
      if (full) { ovec4 q; q.x = val[0]; q.y = val[1]; q.z = val[2]; q.w = val[3]; *reinterpret_cast<ovec4*>(out + base) = q; }
      else for (int j = 0; j < kPixPerLane; ++j) if (base + j < a.npix) out[base + j] = val[j];
    }
  }
}

template <int NR, bool TAN>
void launch_dense(bool f32, bool out_double, unsigned grid, const DenseArgs& a) {
  if (f32) {
    if (out_double) hipLaunchKernelGGL((k_depth_dense<NR, TAN, true, double>), dim3(grid), dim3(256), 0, 0, a);
    else hipLaunchKernelGGL((k_depth_dense<NR, TAN, true, float>), dim3(grid), dim3(256), 0, 0, a);
  } else {
    if (out_double) hipLaunchKernelGGL((k_depth_dense<NR, TAN, false, double>), dim3(grid), dim3(256), 0, 0, a);
    else hipLaunchKernelGGL((k_depth_dense<NR, TAN, false, float>), dim3(grid), dim3(256), 0, 0, a);
  }
}

// ---- object-space comparison at a solver handle's parameters ----
struct ObjArgs {
  uint64_t n;
  const double* x; const double* y; const double* vd;
  const uint32_t* fr; const uint32_t* pt;
  const double* cam; const double* views; const double* pts;   // the handle's device-resident parameters
  double spx, spy;
  uint32_t config;
  double* ref; double* proj;
  double* slots;   // [gridDim.x][9]: sum dx^2, dy^2, dz^2, sum rel^2, max |dx|, |dy|, |dz|, used, skipped
};
constexpr int kObjSlots = 9;

__global__ __launch_bounds__(256) void k_object_space(ObjArgs a) {
  __shared__ double s_red[kObjSlots][256];
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double acc[kObjSlots] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (i < a.n) {
    const int nr = (int)(a.config & 3u);
    const bool tan = (a.config & 4u) != 0;
    const double* c = a.cam;
    const double k0 = nr > 0 ? c[5] : 0.0, k1 = nr > 1 ? c[6] : 0.0, p0 = tan ? c[5 + nr] : 0.0, p1 = tan ? c[6 + nr] : 0.0;
    const double v = a.vd[i];
    double ft[16], ref[3], p[3];
    lifcal::frame_eval(a.views + 6 * (size_t)a.fr[i], ft);
    const double* P = a.pts + 3 * (size_t)a.pt[i];
    for (int j = 0; j < 3; ++j) ref[j] = ft[3 * j] * P[0] + ft[3 * j + 1] * P[1] + ft[3 * j + 2] * P[2] + ft[9 + j];
    if (v > 0.0) back_project<double>(a.x[i], a.y[i], v, a.spx, a.spy, c[0], c[1], c[2], c[3], c[4], k0, k1, p0, p1, nr, tan, p);
    else p[0] = p[1] = p[2] = __builtin_nan("");
    for (int j = 0; j < 3; ++j) { a.ref[3 * i + j] = ref[j]; a.proj[3 * i + j] = p[j]; }
    if (v >= 2.0) {   // the reference leaves v < 2 out of the initial fit (:482); so does this comparison
      for (int j = 0; j < 3; ++j) { const double e = p[j] - ref[j]; acc[j] = e * e; acc[4 + j] = fabs(e); }
      const double rel = (p[2] - ref[2]) / ref[2];
      acc[3] = rel * rel; acc[7] = 1.0;
    } else acc[8] = 1.0;
  }
  // fixed-order tree per workgroup; the host adds the workgroups' slots in order
  for (int k = 0; k < kObjSlots; ++k) s_red[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
      for (int k = 0; k < kObjSlots; ++k) {
        const double o = s_red[k][threadIdx.x + w];
        if (k >= 4 && k < 7) s_red[k][threadIdx.x] = fmax(s_red[k][threadIdx.x], o);
        else s_red[k][threadIdx.x] += o;
      }
    __syncthreads();
  }
  if (threadIdx.x < kObjSlots) a.slots[(size_t)blockIdx.x * kObjSlots + threadIdx.x] = s_red[threadIdx.x][0];
}

// device buffers of one call, released when the call returns
struct Scratch {
  std::vector<void*> bufs;
  ~Scratch() { for (void* q : bufs) (void)hipFree(q); }
  hipError_t alloc(void** q, size_t bytes) {
    *q = nullptr;
    hipError_t e = hipMalloc(q, bytes ? bytes : 8);
    if (e == hipSuccess) bufs.push_back(*q);
    return e;
  }
  template <class T>
  hipError_t up(const T** q, const T* src, size_t n) {
    *q = nullptr;
    if (!src) return hipSuccess;
    void* w = nullptr;
    hipError_t e = alloc(&w, n * sizeof(T));
    if (e != hipSuccess) return e;
    *q = (const T*)w;
    return n ? hipMemcpy(w, src, n * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  }
};

inline bool camera_ok(const lifcal_depth_camera* c) { return c && (c->config & 3u) <= 2u; }

template <class T>
DenseCam<T> dense_cam(const lifcal_depth_camera& c, const double* G, double sigma_v) {
  const int nr = (int)(c.config & 3u);
  const bool tan = (c.config & 4u) != 0;
  DenseCam<T> d{};
  d.fL = (T)c.cam[0]; d.bL0 = (T)c.cam[1]; d.B = (T)c.cam[2]; d.cx = (T)c.cam[3]; d.cy = (T)c.cam[4];
  d.k0 = (T)(nr > 0 ? c.cam[5] : 0.0); d.k1 = (T)(nr > 1 ? c.cam[6] : 0.0);
  d.p0 = (T)(tan ? c.cam[5 + nr] : 0.0); d.p1 = (T)(tan ? c.cam[6 + nr] : 0.0);
  d.spx = (T)c.spx; d.spy = (T)c.spy;
  if (G) { d.G[0] = (T)G[0]; d.G[1] = (T)G[1]; d.G[2] = (T)G[2]; d.G[3] = (T)G[17 + 1]; d.G[4] = (T)G[17 + 2]; d.G[5] = (T)G[2 * 17 + 2]; }
  d.sv2 = (T)(sigma_v * sigma_v);
  return d;
}

}  // namespace depth

struct lifcal_depth_handle {
  int32_t width = 0, height = 0, max_maps = 0, device = 0;
  uint16_t* maps = nullptr;
  unsigned long long* counters = nullptr;   // 4 device counters
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  void* out_scratch = nullptr; size_t out_bytes = 0;   // outputs of the dense path when the caller's arrays are on the host
};

#define DEPTH_TRY(expr, who)                                                                            \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess) { g_last_error = std::string(who) + ": " + hipGetErrorString(e_); return LIFCAL_BA_ERR_HIP; } \
  } while (0)

extern "C" {

int lifcal_depth_create(int32_t width, int32_t height, int32_t max_maps, int32_t device, lifcal_depth_handle** out) {
  if (!out) return LIFCAL_BA_ERR_INVALID_ARG;
  *out = nullptr;
  if (width <= 0 || height <= 0 || max_maps <= 0 || (int64_t)width * height > ((int64_t)1 << 28) || (int64_t)width * height * max_maps > ((int64_t)1 << 33)) {
    g_last_error = "lifcal_depth_create: bad size"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
  if (int rc = mla::select_device(device, "lifcal_depth_create")) return rc;
  lifcal_depth_handle* h = new (std::nothrow) lifcal_depth_handle();
  if (!h) return LIFCAL_BA_ERR_NOMEM;
  h->width = width; h->height = height; h->max_maps = max_maps; h->device = device;
  const size_t bytes = (size_t)width * height * max_maps * 2;
  hipError_t e = hipMalloc((void**)&h->maps, bytes);
  if (e == hipSuccess) e = hipMemset(h->maps, 0, bytes);
  if (e == hipSuccess) e = hipMalloc((void**)&h->counters, 4 * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipEventCreate(&h->ev0);
  if (e == hipSuccess) e = hipEventCreate(&h->ev1);
  if (e != hipSuccess) { g_last_error = std::string("lifcal_depth_create: ") + hipGetErrorString(e); lifcal_depth_destroy(h); return e == hipErrorOutOfMemory ? LIFCAL_BA_ERR_NOMEM : LIFCAL_BA_ERR_HIP; }
  *out = h;
  return 0;
}

void lifcal_depth_destroy(lifcal_depth_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->maps) (void)hipFree(h->maps);
  if (h->counters) (void)hipFree(h->counters);
  if (h->out_scratch) (void)hipFree(h->out_scratch);
  if (h->ev0) (void)hipEventDestroy(h->ev0);
  if (h->ev1) (void)hipEventDestroy(h->ev1);
  delete h;
}

int lifcal_depth_set_maps(lifcal_depth_handle* h, int32_t first, int32_t count, const uint16_t* maps, int32_t on_device) {
  if (!h || !maps || count < 0) { g_last_error = "lifcal_depth_set_maps: bad argument"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (first < 0 || (int64_t)first + count > h->max_maps) { g_last_error = "lifcal_depth_set_maps: map range exceeds max_maps"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  if (count == 0) return 0;
  DEPTH_TRY(hipSetDevice(h->device), "lifcal_depth_set_maps");
  const size_t hw = (size_t)h->width * h->height;
  DEPTH_TRY(hipMemcpy(h->maps + hw * first, maps, hw * count * 2, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice), "lifcal_depth_set_maps");
  return 0;
}

int lifcal_depth_sample(lifcal_depth_handle* h, uint64_t n, const double* x, const double* y, const int32_t* map_index, double* vdepth,
                        lifcal_depth_sample_counts* counts) {
  if (!h || (n && (!x || !y || !map_index || !vdepth)) || n > 0x7ffffff0ull) { g_last_error = "lifcal_depth_sample: bad argument"; return LIFCAL_BA_ERR_INVALID_ARG; }
  for (uint64_t i = 0; i < n; ++i)
    if (map_index[i] < 0 || map_index[i] >= h->max_maps) { g_last_error = "lifcal_depth_sample: map index out of range"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  if (counts) *counts = lifcal_depth_sample_counts{0, 0, 0};
  if (n == 0) return 0;
  DEPTH_TRY(hipSetDevice(h->device), "lifcal_depth_sample");
  depth::Scratch s;
  depth::SampleArgs a{};
  a.maps = h->maps; a.W = h->width; a.H = h->height; a.n = n; a.counts = h->counters;
  DEPTH_TRY(s.up(&a.x, x, n), "lifcal_depth_sample");
  DEPTH_TRY(s.up(&a.y, y, n), "lifcal_depth_sample");
  DEPTH_TRY(s.up(&a.map_index, map_index, n), "lifcal_depth_sample");
  DEPTH_TRY(s.alloc((void**)&a.out, n * 8), "lifcal_depth_sample");
  DEPTH_TRY(hipMemset(h->counters, 0, 4 * sizeof(unsigned long long)), "lifcal_depth_sample");
  hipLaunchKernelGGL(depth::k_depth_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, a);
  DEPTH_TRY(hipGetLastError(), "lifcal_depth_sample");
  DEPTH_TRY(hipMemcpy(vdepth, a.out, n * 8, hipMemcpyDeviceToHost), "lifcal_depth_sample");
  unsigned long long c[4];
  DEPTH_TRY(hipMemcpy(c, h->counters, sizeof c, hipMemcpyDeviceToHost), "lifcal_depth_sample");
  if (counts) { counts->direct = c[0]; counts->interpolated = c[1]; counts->failed = c[2]; }
  return 0;
}

int lifcal_depth_back_project_points(int32_t device, const lifcal_depth_camera* cam, lifcal_depth_points* io) {
  const char* who = "lifcal_depth_back_project_points";
  if (!depth::camera_ok(cam) || !io || (io->n && (!io->x || !io->y || !io->vdepth || !io->p_c)) || io->n > 0x7ffffff0ull ||
      (io->p_w && (!io->fr || !io->views)) || (io->cov_pc && !io->cam_cov)) {
    g_last_error = std::string(who) + ": bad argument"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
  const uint64_t n = io->n;
  if (io->p_w) for (uint64_t i = 0; i < n; ++i) if (io->fr[i] >= io->n_frames) { g_last_error = std::string(who) + ": frame index out of range"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  io->n_invalid = 0;
  if (int rc = mla::select_device(device, who)) return rc;
  if (n == 0) return 0;
  depth::Scratch s;
  depth::PointsArgs a{};
  a.n = n; a.cam = *cam; a.sigma_v = io->sigma_v;
  const bool want_jac = io->jac || io->dpc_dv || io->cov_pc;
  DEPTH_TRY(s.up(&a.x, io->x, n), who);
  DEPTH_TRY(s.up(&a.y, io->y, n), who);
  DEPTH_TRY(s.up(&a.vd, io->vdepth, n), who);
  if (io->p_w) { DEPTH_TRY(s.up(&a.fr, io->fr, n), who); DEPTH_TRY(s.up(&a.views, io->views, 6 * (size_t)io->n_frames), who); }
  if (io->cov_pc) DEPTH_TRY(s.up(&a.G, io->cam_cov, (size_t)17 * 17), who);
  DEPTH_TRY(s.alloc((void**)&a.pc, n * 24), who);
  if (io->p_w) DEPTH_TRY(s.alloc((void**)&a.pw, n * 24), who);
  if (want_jac) { DEPTH_TRY(s.alloc((void**)&a.jac, n * 51 * 8), who); DEPTH_TRY(s.alloc((void**)&a.dv, n * 24), who); }
  if (io->cov_pc) DEPTH_TRY(s.alloc((void**)&a.cov, n * 48), who);
  DEPTH_TRY(s.alloc((void**)&a.n_invalid, 8), who);
  DEPTH_TRY(hipMemset(a.n_invalid, 0, 8), who);
  hipLaunchKernelGGL(depth::k_depth_points, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, a);
  DEPTH_TRY(hipGetLastError(), who);
  DEPTH_TRY(hipMemcpy(io->p_c, a.pc, n * 24, hipMemcpyDeviceToHost), who);
  if (io->p_w) DEPTH_TRY(hipMemcpy(io->p_w, a.pw, n * 24, hipMemcpyDeviceToHost), who);
  if (io->jac) DEPTH_TRY(hipMemcpy(io->jac, a.jac, n * 51 * 8, hipMemcpyDeviceToHost), who);
  if (io->dpc_dv) DEPTH_TRY(hipMemcpy(io->dpc_dv, a.dv, n * 24, hipMemcpyDeviceToHost), who);
  if (io->cov_pc) DEPTH_TRY(hipMemcpy(io->cov_pc, a.cov, n * 48, hipMemcpyDeviceToHost), who);
  unsigned long long bad = 0;
  DEPTH_TRY(hipMemcpy(&bad, a.n_invalid, 8, hipMemcpyDeviceToHost), who);
  io->n_invalid = bad;
  return 0;
}

int lifcal_depth_back_project_maps(lifcal_depth_handle* h, const lifcal_depth_camera* cam, lifcal_depth_maps* io) {
  const char* who = "lifcal_depth_back_project_maps";
  if (!h || !depth::camera_ok(cam) || !io || io->count < 0 || (io->eval != 0 && io->eval != 1) || (io->sigma_z && !io->cam_cov) ||
      ((io->frame != nullptr) != (io->views != nullptr))) {
    g_last_error = std::string(who) + ": bad argument"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
  if (io->first < 0 || (int64_t)io->first + io->count > h->max_maps) { g_last_error = std::string(who) + ": map range exceeds max_maps"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  if (io->frame) for (int32_t m = 0; m < io->count; ++m) if (io->frame[m] >= io->n_frames) { g_last_error = std::string(who) + ": frame index out of range"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  const size_t hw = (size_t)h->width * h->height;
  const uint64_t npix = (uint64_t)hw * (uint64_t)io->count;
  if (npix > 0x7fffff00ull) { g_last_error = std::string(who) + ": more than 2^31 pixels in one call"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (io->out_on_device)
    for (const void* q : {(const void*)io->xyz, (const void*)io->z, (const void*)io->sigma_z})
      if (((uintptr_t)q & 15u) != 0) { g_last_error = std::string(who) + ": device outputs must be 16-byte aligned"; return LIFCAL_BA_ERR_INVALID_ARG; }
  io->n_invalid = 0; io->seconds = 0.0;
  if (npix == 0) return 0;
  DEPTH_TRY(hipSetDevice(h->device), who);
  const size_t osz = io->out_double ? 8 : 4;
  const size_t b_xyz = io->xyz ? ((npix * 3 * osz + 255) & ~(size_t)255) : 0, b_z = io->z ? ((npix * osz + 255) & ~(size_t)255) : 0, b_s = io->sigma_z ? ((npix * osz + 255) & ~(size_t)255) : 0;
  depth::DenseArgs a{};
  if (io->out_on_device) { a.xyz = io->xyz; a.z = io->z; a.sz = io->sigma_z; }
  else {
    const size_t need = b_xyz + b_z + b_s;
    if (need > h->out_bytes) {
      if (h->out_scratch) (void)hipFree(h->out_scratch);
      h->out_scratch = nullptr; h->out_bytes = 0;
      DEPTH_TRY(hipMalloc(&h->out_scratch, need), who);
      h->out_bytes = need;
    }
    char* q = (char*)h->out_scratch;
    if (io->xyz) a.xyz = q;
    if (io->z) a.z = q + b_xyz;
    if (io->sigma_z) a.sz = q + b_xyz + b_z;
  }
  depth::Scratch s;
  if (io->frame) {
    const double* d_views = nullptr; const uint32_t* d_frame = nullptr; double* ftab = nullptr;
    DEPTH_TRY(s.up(&d_views, io->views, 6 * (size_t)io->n_frames), who);
    DEPTH_TRY(s.up(&d_frame, io->frame, (size_t)io->count), who);
    DEPTH_TRY(s.alloc((void**)&ftab, (size_t)io->count * 16 * 8), who);
    hipLaunchKernelGGL(depth::k_depth_frames, dim3((unsigned)((io->count + 63) / 64)), dim3(64), 0, 0, d_views, d_frame, (int)io->count, ftab);
    a.ftab = ftab;
  }
  a.maps = h->maps + hw * io->first;
  a.npix = (uint32_t)npix; a.W = (uint32_t)h->width; a.HW = (uint32_t)hw;
  a.vec_in = ((uintptr_t)a.maps & 7u) == 0 ? 1 : 0;
  a.n_invalid = h->counters + 3;
  a.c64 = depth::dense_cam<double>(*cam, io->cam_cov, io->sigma_v);
  a.c32 = depth::dense_cam<float>(*cam, io->cam_cov, io->sigma_v);
  DEPTH_TRY(hipMemsetAsync(h->counters + 3, 0, 8, 0), who);
  const unsigned grid = (unsigned)((npix + 256 * depth::kPixPerLane - 1) / (256 * depth::kPixPerLane));
  const bool f32 = io->eval == 1, dbl = io->out_double != 0;
  DEPTH_TRY(hipEventRecord(h->ev0, 0), who);
  switch ((int)(cam->config & 3u) + ((cam->config & 4u) ? 3 : 0)) {
    case 0: depth::launch_dense<0, false>(f32, dbl, grid, a); break;
    case 1: depth::launch_dense<1, false>(f32, dbl, grid, a); break;
    case 2: depth::launch_dense<2, false>(f32, dbl, grid, a); break;
    case 3: depth::launch_dense<0, true>(f32, dbl, grid, a); break;
    case 4: depth::launch_dense<1, true>(f32, dbl, grid, a); break;
    default: depth::launch_dense<2, true>(f32, dbl, grid, a); break;
  }
  DEPTH_TRY(hipGetLastError(), who);
  DEPTH_TRY(hipEventRecord(h->ev1, 0), who);
  DEPTH_TRY(hipEventSynchronize(h->ev1), who);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
  io->seconds = ms * 1e-3;
  if (!io->out_on_device) {
    if (io->xyz) DEPTH_TRY(hipMemcpy(io->xyz, a.xyz, npix * 3 * osz, hipMemcpyDeviceToHost), who);
    if (io->z) DEPTH_TRY(hipMemcpy(io->z, a.z, npix * osz, hipMemcpyDeviceToHost), who);
    if (io->sigma_z) DEPTH_TRY(hipMemcpy(io->sigma_z, a.sz, npix * osz, hipMemcpyDeviceToHost), who);
  }
  unsigned long long bad = 0;
  DEPTH_TRY(hipMemcpy(&bad, h->counters + 3, 8, hipMemcpyDeviceToHost), who);
  io->n_invalid = bad;
  return 0;
}

int lifcal_ba_object_space_stats(lifcal_ba_handle* h, uint64_t n, const double* x, const double* y, const double* vdepth, const uint32_t* fr, const uint32_t* pt,
                                 double* ref_c, double* proj_c, lifcal_ba_object_space* out) {
  const char* who = "lifcal_ba_object_space_stats";
  if (!h || !out || (n && (!x || !y || !vdepth || !fr || !pt)) || n > 0x7ffffff0ull || h->opt.world_size > 1 || (h->prob.config & 3u) > 2u) {
    g_last_error = std::string(who) + ": bad argument (one rank only)"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
  Dev& d = h->d;
  for (uint64_t i = 0; i < n; ++i) if (fr[i] >= d.F || pt[i] >= d.P) { g_last_error = std::string(who) + ": frame or point index out of range"; return LIFCAL_BA_ERR_OUT_OF_RANGE; }
  *out = lifcal_ba_object_space{};
  if (n == 0) return 0;
  DEPTH_TRY(hipSetDevice(h->opt.device), who);
  DEPTH_TRY(hipStreamSynchronize(h->stream), who);   // the parameters are produced on the handle's stream
  depth::Scratch s;
  depth::ObjArgs a{};
  a.n = n; a.cam = d.cam; a.views = d.views; a.pts = d.pts; a.spx = h->prob.spx; a.spy = h->prob.spy; a.config = h->prob.config;
  DEPTH_TRY(s.up(&a.x, x, n), who);
  DEPTH_TRY(s.up(&a.y, y, n), who);
  DEPTH_TRY(s.up(&a.vd, vdepth, n), who);
  DEPTH_TRY(s.up(&a.fr, fr, n), who);
  DEPTH_TRY(s.up(&a.pt, pt, n), who);
  const unsigned grid = (unsigned)((n + 255) / 256);
  DEPTH_TRY(s.alloc((void**)&a.ref, n * 24), who);
  DEPTH_TRY(s.alloc((void**)&a.proj, n * 24), who);
  DEPTH_TRY(s.alloc((void**)&a.slots, (size_t)grid * depth::kObjSlots * 8), who);
  hipLaunchKernelGGL(depth::k_object_space, dim3(grid), dim3(256), 0, 0, a);
  DEPTH_TRY(hipGetLastError(), who);
  std::vector<double> slots((size_t)grid * depth::kObjSlots);
  DEPTH_TRY(hipMemcpy(slots.data(), a.slots, slots.size() * 8, hipMemcpyDeviceToHost), who);
  if (ref_c) DEPTH_TRY(hipMemcpy(ref_c, a.ref, n * 24, hipMemcpyDeviceToHost), who);
  if (proj_c) DEPTH_TRY(hipMemcpy(proj_c, a.proj, n * 24, hipMemcpyDeviceToHost), who);
  double t[depth::kObjSlots] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (unsigned b = 0; b < grid; ++b)
    for (int k = 0; k < depth::kObjSlots; ++k) {
      const double v = slots[(size_t)b * depth::kObjSlots + k];
      if (k >= 4 && k < 7) t[k] = std::max(t[k], v); else t[k] += v;
    }
  out->n_used = (uint64_t)t[7]; out->n_skipped = (uint64_t)t[8];
  for (int j = 0; j < 3; ++j) { out->rms[j] = t[7] > 0 ? std::sqrt(t[j] / t[7]) : 0.0; out->max_abs[j] = t[4 + j]; }
  out->rms_rel_depth = t[7] > 0 ? std::sqrt(t[3] / t[7]) : 0.0;
  return 0;
}

}  // extern "C"
