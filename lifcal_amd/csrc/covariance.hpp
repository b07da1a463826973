// covariance.hpp — lifcal_ba_covariance: its kernels, then its host driver (included at the end of lifcal_ba.hip, behind the handle
// and the launch helpers the driver uses).  DESIGN.md section 7h.
//
// H = [S_ff S_fa; S_af S_aa] is the UNDAMPED reduced system of the sweep at radius = infinity (poses f | arrow a = promoted
// points + camera slots).  With S_ff = L_ff L_ff^T, C = S_aa - S_af S_ff^-1 S_fa and Y = S_ff^-1 S_fa = L_ff^-T L_af^T, a
// g-inverse of H is
//   G_aa = C+,   G_fa = -Y C+,   G_ff = S_ff^-1 + Y C+ Y^T
// (C+ is formed on the host: C is NA x NA).  Four single-purpose kernels, every sum in a fixed order (no atomics):
//   K1 k_cov_chol_w    the chain of k_band_chol_w over the pose blocks, arrow block left unfactored -> C, Lpanel, Linv
//   K2 k_cov_selinv    selected inversion of the band factor (Takahashi / Erisman-Tinney): Z = S_ff^-1 inside the band
//   K3 k_cov_backsolve Y = L_ff^-T L_af^T, all NA columns at once
//   K4 k_cov_combine   G_jj = Z_jj + Y_j C+ Y_j^T per frame
#pragma once

namespace lifcal {

// K1: the chain of k_band_chol_w (bandchol.hpp) over the pose blocks, restated so that the solve's kernel stays as it is: same
// window, panels (Lpanel) and L_jj^-1 (d.Linv); it stops before the arrow block.  fail_out[0] = 1 + the first frame whose pivot is
// not positive (0: none).  One workgroup of 256 threads, LDS as k_band_chol_w (BandLds).
__global__ __launch_bounds__(256) void k_cov_chol_w(Dev d, double* Lpanel, double* Cout, double* fail_out) {
  extern __shared__ __attribute__((aligned(16))) double bl[];
  const uint32_t F = d.F, bw = d.bw, NAx = d.NA + 1, ld = d.ld, R = bw + 1;
  const BandLds lay(bw, d.NA);
  const uint32_t nw = lay.nw, arow0 = 6 * R, NR = lay.nr4;
  double* Wd = bl; double* Pn = bl + lay.off_pn; double* Ld = bl + lay.off_d; double* Li = Ld + 36; double* failp = Ld + 72;
  const uint32_t lane = threadIdx.x;   // 256 threads
  uint32_t* wmap = (uint32_t*)(bl + lay.off_map);
  auto slot = [&](uint32_t f) { return 6 * (f % R); };
  if (lane == 0) *failp = 0.0;
  // ---- load the initial window: frames 0..min(bw, F-1), all arrow rows ----
  for (uint32_t i = lane; i < nw * nw; i += 256) Wd[i] = 0.0;
  __syncthreads();
  auto load_frame_row = [&](uint32_t f) {   // blocks (f, f-dd), dd = 0..min(bw, f), and the arrow entries of column f
    const uint32_t ndd = min(bw, f) + 1;
    for (uint32_t t = lane; t < ndd * 36; t += 256) {
      const uint32_t dd = t / 36, e = t % 36, a = e / 6, b = e % 6;
      if (dd == 0 && b > a) continue;
      Wd[(size_t)(slot(f) + a) * nw + slot(f - dd) + b] = d.Sband[((size_t)f * (bw + 1) + dd) * 36 + e];
    }
    for (uint32_t t = lane; t < NAx * 6; t += 256) {
      const uint32_t a = t / 6, b = t % 6;
      Wd[(size_t)(arow0 + a) * nw + slot(f) + b] = d.Sarrow[(size_t)a * ld + 6 * f + b];
    }
  };
  for (uint32_t f = 0; f < min(R, F); ++f) load_frame_row(f);
  for (uint32_t t = lane; t < NAx * NAx; t += 256) {
    const uint32_t a = t / NAx, b = t % NAx;
    if (b <= a) Wd[(size_t)(arow0 + a) * nw + arow0 + b] = d.Sarrow[(size_t)a * ld + 6 * F + b];
  }
  __syncthreads();
  // 6x6 Cholesky of pose block jf and the inverse of its factor: ONE lane, a pure dependency chain
  auto factor_block = [&](uint32_t jf, bool subtract_panel) {
    const uint32_t sf = slot(jf);
    // One lane, a pure dependency chain: reciprocal square roots only (v_rsq_f64 + Newton steps) — the sqrt + divide
    // pairs of the textbook form were most of the time of a chain step.  ir[c] = 1 / L[c][c].
    double L[6][6], ir[6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b <= a; ++b) L[a][b] = Wd[(size_t)(sf + a) * nw + sf + b];
    if (subtract_panel) {   // last contribution to this block: the first six rows of the current column's panel (all loads first)
      double P6[6][6];
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int a = 0; a < 6; ++a) P6[k][a] = Pn[(size_t)k * NR + a];
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b <= a; ++b) {
#pragma unroll
          for (int k = 0; k < 6; ++k) L[a][b] -= P6[k][a] * P6[k][b];
        }
    }
    bool ok = true;
#pragma unroll
    for (int cI = 0; cI < 6; ++cI) {
      double dg = L[cI][cI];
#pragma unroll
      for (int k = 0; k < cI; ++k) dg -= L[cI][k] * L[cI][k];
      if (!(dg > 0.0)) { ok = false; dg = 1.0; }
      const double idg = rsqrt(dg);
      ir[cI] = idg; L[cI][cI] = dg * idg;
#pragma unroll
      for (int r = cI + 1; r < 6; ++r) { double s = L[r][cI];
#pragma unroll
        for (int k = 0; k < cI; ++k) s -= L[r][k] * L[cI][k];
        L[r][cI] = s * idg; }
    }
    if (!ok && *failp == 0.0) *failp = 1.0 + (double)jf;   // the first frame the data do not pin down
    double I[6][6];
#pragma unroll
    for (int cI = 0; cI < 6; ++cI) {
#pragma unroll
      for (int r = 0; r < 6; ++r) I[r][cI] = 0.0;
      I[cI][cI] = ir[cI];
#pragma unroll
      for (int r = cI + 1; r < 6; ++r) { double s = 0.0;
#pragma unroll
        for (int k = cI; k < r; ++k) s -= L[r][k] * I[k][cI];
        I[r][cI] = s * ir[r]; }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = 0; b < 6; ++b) { Li[a * 6 + b] = (b <= a) ? I[a][b] : 0.0; }
  };
  auto tri_block = [](uint32_t t, uint32_t& bi, uint32_t& bj) {
    bi = (uint32_t)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (bi * (bi + 1) / 2 > t) --bi;
    while ((bi + 1) * (bi + 2) / 2 <= t) ++bi;
    bj = t - bi * (bi + 1) / 2;
  };
  uint32_t bi0, bj0;
  tri_block(lane, bi0, bj0);
  const bool pf_ok = (R * 36 <= 512) && (NAx * 6 <= 256);
  double pfn[3] = {0.0, 0.0, 0.0};
  auto fetch_frame = [&](uint32_t f) {
#pragma unroll
    for (int q = 0; q < 2; ++q) { const uint32_t t = lane + 256 * q; if (t < R * 36) pfn[q] = d.Sband[((size_t)f * (bw + 1) + t / 36) * 36 + t % 36]; }
    if (lane < NAx * 6) pfn[2] = d.Sarrow[(size_t)(lane / 6) * ld + 6 * f + lane % 6];
  };
  if (pf_ok && R < F) fetch_frame(R);
  // ---- the chain over the pose blocks ----
  // (barriers inside the chain order LDS only: __syncthreads() would also wait for the panel / L^-1 stores on their way to
  // HBM — a write round trip per barrier, four per pose block — and nothing in the chain reads them back)
  for (uint32_t j = 0; j < F; ++j) {
    const uint32_t sj = slot(j);
    if (j == 0 && lane == 192) factor_block(0, false);   // later blocks are factored by wave 3 inside the previous step's update
    lds_barrier();
    const uint32_t nbel = min(bw, F - 1 - j);
    const uint32_t nrows = 6 * nbel + NAx;
    double* Lp = Lpanel + (size_t)j * (6 * bw + NAx) * 6;
    if (lane >= 192 && lane < 228) d.Linv[(size_t)j * 36 + (lane - 192)] = Li[lane - 192];   // L_jj^-1 to HBM for the back-substitution: 36 lanes, off the factoring lane's path
    for (uint32_t r = lane; r < nrows; r += 256) {
      const uint32_t wrow = (r < 6 * nbel) ? slot(j + 1 + r / 6) + r % 6 : arow0 + (r - 6 * nbel);
      wmap[r] = wrow;
      const double* src = Wd + (size_t)wrow * nw + sj;
      double x[6], y[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) x[k] = src[k];
#pragma unroll
      for (int cI = 0; cI < 6; ++cI) { double s = 0.0;
#pragma unroll
        for (int k = 0; k <= cI; ++k) s += x[k] * Li[cI * 6 + k];
        y[cI] = s; }
#pragma unroll
      for (int k = 0; k < 6; ++k) { Pn[(size_t)k * NR + r] = y[k]; Lp[(size_t)r * 6 + k] = y[k]; }
    }
    lds_barrier();
    // the frame that enters the ring after this step was requested from HBM ONE STEP AGO (pfn); the request for the frame
    // of the next step goes out now — a step is shorter than the HBM round trip
    // (up to 2 band values + 1 arrow value per thread for bw <= 13; wider bands take the plain path below)
    const bool has_next = (j + R < F);
    const bool pf = has_next && pf_ok;
    double pfv[3] = {pfn[0], pfn[1], pfn[2]};
    if (pf_ok && j + 1 + R < F) fetch_frame(j + 1 + R);
    // rank-6 update of the window in 4x4 blocks of (panel row, panel row) pairs over the lower triangle, one block per
    // thread.  The phase is bound by LDS traffic: the panel is stored component-major (Pn[k][row]) so that the four rows of
    // a block are one 32-byte run per component (12 + 12 ds_read_b128 for 96 MACs, no bank-conflicting 48-byte strides),
    // 5.5 LDS operations per pair instead of 9 with a row per thread, and every thread has the same amount of work.
    // The diagonal block of frame j+1 receives its last contribution from this column: lane 192 (wave 3, idle in the
    // blocked update below for the usual band widths) applies it first and factors the block right away, so that the
    // single-lane factorisation of step j+1 runs UNDER this step's update instead of in front of the next one.
    const bool ahead = nbel > 0;
    if (ahead && lane == 192) factor_block(j + 1, true);   // (the block itself is not written back: nothing reads it after its factorisation)
    {
      const uint32_t nb4 = (nrows + 3u) >> 2, nblk = nb4 * (nb4 + 1) / 2;
      const uint32_t first = lane < 192 ? lane : lane - 192 + 192;   // (all four waves take blocks; lane 192 joins after its factorisation)
      for (uint32_t t = first; t < nblk; t += 256) {
        uint32_t bi = bi0, bj = bj0;   // block of t = lane, decoded once before the chain (a shorter panel uses a prefix of the blocks)
        if (t != lane) tri_block(t, bi, bj);
        double2 pr[6][2], pc[6][2];
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          pr[k][0] = *reinterpret_cast<const double2*>(Pn + (size_t)k * NR + 4 * bi); pr[k][1] = *reinterpret_cast<const double2*>(Pn + (size_t)k * NR + 4 * bi + 2);
          pc[k][0] = *reinterpret_cast<const double2*>(Pn + (size_t)k * NR + 4 * bj); pc[k][1] = *reinterpret_cast<const double2*>(Pn + (size_t)k * NR + 4 * bj + 2);
        }
        uint32_t wr[4], wc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { wr[i] = wmap[min(4 * bi + i, nrows - 1)] * nw; wc[i] = wmap[min(4 * bj + i, nrows - 1)]; }
        // branch-free: entries that are not this block's to update (upper triangle of a diagonal block, rows past the panel,
        // the six rows lane 192 takes) are pointed at the thread's scratch double; all reads come before all writes (written
        // one by one the compiler has to assume that the entries alias and pays an LDS round trip per entry)
        const uint32_t scratch = lay.off_dummy + lane;
        uint32_t wa[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jx = 0; jx < 4; ++jx) {
            const uint32_t r = 4 * bi + i, cI = 4 * bj + jx;
            wa[i][jx] = (r < nrows && cI <= r && !(ahead && r < 6)) ? wr[i] + wc[jx] : scratch;
          }
        double oldv[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jx = 0; jx < 4; ++jx) oldv[i][jx] = bl[wa[i][jx]];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jx = 0; jx < 4; ++jx) {
            double sacc = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) sacc += ((i & 1) ? pr[k][i >> 1].y : pr[k][i >> 1].x) * ((jx & 1) ? pc[k][jx >> 1].y : pc[k][jx >> 1].x);
            bl[wa[i][jx]] = oldv[i][jx] - sacc;
          }
      }
    }
    // slide: frame j leaves its slot, frame j + bw + 1 (if any) enters it — in the SAME phase as the update: the update
    // touches rows and columns of the frames j+1..j+bw and of the arrow only, the incoming frame's row and column live in
    // the slot frame j has just vacated (its column was last read by the panel phase, a barrier ago).  No zeroing is
    // needed: every entry of the slot's row that is read later is overwritten here (all bw+1 blocks of the incoming frame),
    // and stale entries of the slot's column are overwritten when the rows that use them enter.
    if (has_next) {
      const uint32_t f = j + R;
      if (pf) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const uint32_t t = lane + 256 * q;
          if (t < R * 36) { const uint32_t dd = t / 36, e = t % 36, a = e / 6, b2 = e % 6; if (!(dd == 0 && b2 > a)) Wd[(size_t)(slot(f) + a) * nw + slot(f - dd) + b2] = pfv[q]; }
        }
        if (lane < NAx * 6) Wd[(size_t)(arow0 + lane / 6) * nw + slot(f) + lane % 6] = pfv[2];
      } else {
        load_frame_row(f);
      }
    }
    lds_barrier();
  }
  // the window's arrow block is now C = S_aa - S_af S_ff^-1 S_fa: written out unfactored, both triangles
  const double* Aa = Wd + (size_t)arow0 * nw + arow0;
  for (uint32_t t = lane; t < d.NA * d.NA; t += 256) {
    const uint32_t a = t / d.NA, b = t % d.NA;
    Cout[t] = Aa[(size_t)max(a, b) * nw + min(a, b)];
  }
  if (lane == 0) fail_out[0] = *failp;
}

// LDS of K2 in doubles: the Z ring (6 (bw+1))^2 | M = L_{k,j} L_jj^-1 (6 bw x 6) | L_jj^-1 (36) | ring row of each panel row (6 bw words)
__host__ __device__ inline uint32_t cov_selinv_lds(uint32_t bw) { const uint32_t nz = 6 * (bw + 1); return nz * nz + 36 * bw + 36 + 3 * bw + 1; }
// LDS of K3 in doubles: the Y ring (6 (bw+1) x NA) | T (6 x NA) | the column's panel ((6 bw + NA) x 6) | L_jj^-1 (36) | row map (6 bw words)
__host__ __device__ inline uint32_t cov_backsolve_lds(uint32_t bw, uint32_t NA) { return (6 * (bw + 1) + 6) * NA + (6 * bw + NA) * 6 + 36 + 3 * bw + 1; }

// K2: Z = S_ff^-1 on the band, walking the frames from F-1 down to 0.  With M_kj = L_kj L_jj^-1 (L_kj: rows of frame k of
// column j's panel), for the frames i = j+1 .. j+nbel:
//   Z_ij = - sum_k Z_ik M_kj          Z_jj = L_jj^-T L_jj^-1 - sum_k Z_kj^T M_kj
// Every Z_ik needed lies among the frames j+1..j+bw: the ring holds those (bw+1)^2 blocks (slot = frame mod (bw+1), the mirror
// of the factor's window); frame j takes the slot frame j+bw+1 has just left.  Outputs: Zd[j] = Z_jj (F x 36) and, if Zb is not
// null, Zb[j][dd-1] = Z_{j,j+dd} (F x bw x 36, dd = 1..bw; blocks past the last frame are left untouched).
__global__ __launch_bounds__(256) void k_cov_selinv(Dev d, const double* Lpanel, double* Zd, double* Zb) {
  extern __shared__ __attribute__((aligned(16))) double zs[];
  const uint32_t F = d.F, bw = d.bw, R = bw + 1, NAx = d.NA + 1, nz = 6 * R, prow = 6 * bw + NAx, lane = threadIdx.x;
  double* Zr = zs;                      // Zr[(slot(i) + a) * nz + slot(k) + b] = Z_ik[a][b]
  double* M = Zr + (size_t)nz * nz;     // M[(6 (k-j-1) + a) * 6 + b] = M_kj[a][b]
  double* Li = M + 36 * bw;             // L_jj^-1, row-major (lower triangle)
  uint32_t* rmap = (uint32_t*)(Li + 36);   // ring row of panel row r: slot(j + 1 + r / 6) + r % 6
  auto slot = [&](uint32_t f) { return 6 * (f % R); };
  for (int jj = (int)F - 1; jj >= 0; --jj) {
    const uint32_t j = (uint32_t)jj, nbel = min(bw, F - 1 - j), nr = 6 * nbel, sj = slot(j);
    const double* Lp = Lpanel + (size_t)j * prow * 6;
    const double* Lij = d.Linv + (size_t)j * 36;
    // M = P L_jj^-1 (P: the nr frame rows of the panel; L_jj^-1 lower triangular)
    for (uint32_t t = lane; t < nr * 6; t += 256) {
      const uint32_t r = t / 6, b = t % 6;
      double s = 0.0;
      for (uint32_t c = b; c < 6; ++c) s += Lp[(size_t)r * 6 + c] * Lij[c * 6 + b];
      M[t] = s;
    }
    if (lane < 36) Li[lane] = Lij[lane];
    for (uint32_t r = lane; r < nr; r += 256) rmap[r] = slot(j + 1 + r / 6) + r % 6;
    __syncthreads();
    // Z_ij for the nr rows below the diagonal block: thread (r, half) forms three columns of row r
    for (uint32_t t = lane; t < nr * 2; t += 256) {
      const uint32_t r = t >> 1, b0 = 3 * (t & 1u);
      const double* zrow = Zr + (size_t)rmap[r] * nz;
      double x0 = 0.0, x1 = 0.0, x2 = 0.0;
      for (uint32_t s = 0; s < nr; ++s) {
        const double z = zrow[rmap[s]];
        x0 += z * M[s * 6 + b0]; x1 += z * M[s * 6 + b0 + 1]; x2 += z * M[s * 6 + b0 + 2];
      }
      const double x[3] = {-x0, -x1, -x2};
      const uint32_t rr = rmap[r];
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const uint32_t b = b0 + q;
        Zr[(size_t)rr * nz + sj + b] = x[q];     // Z_{i,j}[r%6][b]
        Zr[(size_t)(sj + b) * nz + rr] = x[q];   // Z_{j,i}[b][r%6]
        if (Zb) Zb[((size_t)j * bw + r / 6) * 36 + b * 6 + r % 6] = x[q];
      }
    }
    __syncthreads();
    // Z_jj (lower triangle, mirrored): L_jj^-T L_jj^-1 - sum_s Z_{s,j}[.][a] M[s][b]
    if (lane < 36) {
      const uint32_t a = lane / 6, b = lane % 6;
      if (b <= a) {
        double s = 0.0;
        for (uint32_t c = a; c < 6; ++c) s += Li[c * 6 + a] * Li[c * 6 + b];
        double m = 0.0;
        for (uint32_t r = 0; r < nr; ++r) m += Zr[(size_t)rmap[r] * nz + sj + a] * M[r * 6 + b];
        const double z = s - m;
        Zr[(size_t)(sj + a) * nz + sj + b] = z; Zr[(size_t)(sj + b) * nz + sj + a] = z;
        Zd[(size_t)j * 36 + a * 6 + b] = z; Zd[(size_t)j * 36 + b * 6 + a] = z;
      }
    }
    __syncthreads();
  }
}

// K3: L_ff^T Y = W, W = L_af^T (the arrow rows of the panels): Y_j = L_jj^-T (W_j - sum_{i=j+1}^{j+nbel} L_ij^T Y_i), frames
// F-1 down to 0, the 6 NA entries of a block row spread over the lanes.  Y is 6F x NA, row-major.
__global__ __launch_bounds__(256) void k_cov_backsolve(Dev d, const double* Lpanel, double* Y) {
  extern __shared__ __attribute__((aligned(16))) double ys[];
  const uint32_t F = d.F, bw = d.bw, R = bw + 1, NA = d.NA, NAx = NA + 1, prow = 6 * bw + NAx, lane = threadIdx.x;
  double* Yr = ys;                       // Yr[(slot(i) + k) * NA + a]
  double* T = Yr + (size_t)6 * R * NA;   // 6 x NA
  double* Ps = T + (size_t)6 * NA;        // the column's panel: (nr + NA) rows of 6
  double* Lij = Ps + (size_t)(6 * bw + NA) * 6;
  uint32_t* rmap = (uint32_t*)(Lij + 36);  // ring row of panel row r
  auto slot = [&](uint32_t f) { return 6 * (f % R); };
  for (int jj = (int)F - 1; jj >= 0; --jj) {
    const uint32_t j = (uint32_t)jj, nbel = min(bw, F - 1 - j), nr = 6 * nbel;
    const double* Lp = Lpanel + (size_t)j * prow * 6;
    for (uint32_t t = lane; t < (nr + NA) * 6; t += 256) Ps[t] = Lp[t];   // coalesced, once per column
    if (lane < 36) Lij[lane] = d.Linv[(size_t)j * 36 + lane];
    for (uint32_t r = lane; r < nr; r += 256) rmap[r] = slot(j + 1 + r / 6) + r % 6;
    __syncthreads();
    for (uint32_t t = lane; t < 6 * NA; t += 256) {
      const uint32_t k = t / NA, a = t % NA;
      double s = Ps[(nr + a) * 6 + k];
      for (uint32_t r = 0; r < nr; ++r) s -= Ps[r * 6 + k] * Yr[(size_t)rmap[r] * NA + a];
      T[t] = s;
    }
    __syncthreads();
    for (uint32_t t = lane; t < 6 * NA; t += 256) {
      const uint32_t k = t / NA, a = t % NA;
      double s = 0.0;
      for (uint32_t c = k; c < 6; ++c) s += Lij[c * 6 + k] * T[c * NA + a];
      Yr[(size_t)(slot(j) + k) * NA + a] = s;
      Y[((size_t)6 * j + k) * NA + a] = s;
    }
    __syncthreads();
  }
}

// K4: G_jj = mult (Z_jj + Y_j C+ Y_j^T), one workgroup of 64 threads per frame; frames whose pose is not a column (constant,
// unobserved, the gauge frame) get zero blocks
__global__ __launch_bounds__(64) void k_cov_combine(Dev d, const double* Zd, const double* Y, const double* Cp, double mult, double* G) {
  extern __shared__ __attribute__((aligned(16))) double cs[];   // T = Y_j C+ (6 x NA)
  const uint32_t j = blockIdx.x, NA = d.NA, lane = threadIdx.x;
  const bool live = d.use_poses && d.frame_live[j];
  const double* Yj = Y + (size_t)6 * j * NA;
  for (uint32_t t = lane; t < 6 * NA; t += 64) {
    const uint32_t r = t / NA, b = t % NA;
    double s = 0.0;
    for (uint32_t a = 0; a < NA; ++a) s += Yj[(size_t)r * NA + a] * Cp[(size_t)a * NA + b];
    cs[t] = s;
  }
  __syncthreads();
  if (lane < 36) {
    const uint32_t r = lane / 6, c = lane % 6;
    double s = 0.0;
    for (uint32_t b = 0; b < NA; ++b) s += cs[r * NA + b] * Yj[(size_t)c * NA + b];
    G[(size_t)j * 36 + lane] = live ? mult * (Zd[(size_t)j * 36 + lane] + s) : 0.0;
  }
}

}  // namespace lifcal

// ---- host side ----  sym_eig_jacobi, the symmetric eigen-decomposition of a small n x n matrix
#include "sym_eig.hpp"

extern "C" void lifcal_ba_default_covariance_options(lifcal_ba_covariance_options* o) {
  if (!o) return;
  o->gauge_frame = -1; o->want_pose_blocks = 1; o->scale_by_residual_variance = 0; o->reserved = 0;
  o->null_rcond = 1e-9; o->estimable_tol = 1e-3;
}

// sweep at radius = infinity (no damping anywhere: clamp(..) / (inf s^2) = 0, on the point blocks U_p too),
// K1 chain -> C, K2 / K3 on the factor, C+ on the host, K4.  The handle's state is put back before returning, on every path.
extern "C" int lifcal_ba_covariance(lifcal_ba_handle* h, const lifcal_ba_covariance_options* oin, lifcal_ba_covariance_out* out) {
  if (!h || !out || !out->camera) { g_last_error = "lifcal_ba_covariance: null handle, output or output->camera"; return LIFCAL_BA_ERR_INVALID_ARG; }
  lifcal_ba_covariance_options o; if (oin) o = *oin; else lifcal_ba_default_covariance_options(&o);
  Dev& d = h->d;
  const uint32_t F = d.F, NA = d.NA, Q3 = 3 * d.Q, nc = d.nc;
  if (h->opt.world_size > 1) { g_last_error = "lifcal_ba_covariance: world_size > 1 is not supported (every rank holds the reduced system: a follow-up)"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (h->opt.precision != 0) { g_last_error = "lifcal_ba_covariance: options.precision = 1 is not supported; create a second fp64 handle at the solved parameters"; return LIFCAL_BA_ERR_INVALID_ARG; }
  if (!h->use_sweep3) { g_last_error = "lifcal_ba_covariance needs k_sweep3 (unset LIFCAL_SWEEP_KERNEL)"; return LIFCAL_BA_ERR_INVALID_ARG; }
  const size_t lds2 = (size_t)cov_selinv_lds(d.bw) * 8, lds3 = (size_t)cov_backsolve_lds(d.bw, NA) * 8, lds4 = (size_t)6 * NA * 8;
  if (!h->bandw_ok || lds2 > 160 * 1024 || lds3 > 160 * 1024 || lds4 > 64 * 1024) {
    g_last_error = "lifcal_ba_covariance: the band window (" + std::to_string(d.bw + 1) + " frames, " + std::to_string(NA) + " arrow rows) does not fit LDS; only the LDS-window factorisation is supported";
    return LIFCAL_BA_ERR_INVALID_ARG;
  }
  if (!(o.null_rcond >= 0.0) || !(o.estimable_tol >= 0.0) || o.gauge_frame < -2 || (o.gauge_frame >= 0 && (uint32_t)o.gauge_frame >= F)) {
    g_last_error = "lifcal_ba_covariance: gauge_frame must be -2, -1 or a frame index; null_rcond and estimable_tol >= 0"; return LIFCAL_BA_ERR_INVALID_ARG;
  }
  // the gauge frame: held constant for this call only
  const std::vector<uint8_t> live_saved = h->frame_live_host;
  bool any_fixed = false;
  for (uint32_t f = 0; f < F; ++f) if (h->plan.frame_used[f] && !live_saved[f]) any_fixed = true;
  int32_t gauge = -1;
  if (o.gauge_frame >= 0) {
    if (!d.use_poses || !live_saved[o.gauge_frame]) { g_last_error = "lifcal_ba_covariance: the gauge frame must be an observed frame whose pose is refined"; return LIFCAL_BA_ERR_INVALID_ARG; }
    gauge = o.gauge_frame;
  } else if (o.gauge_frame == -1 && d.use_poses && d.use_points && !any_fixed) {
    for (uint32_t f = 0; f < F; ++f) if (live_saved[f]) { gauge = (int32_t)f; break; }
  }
  HIP_TRY(hipSetDevice(h->opt.device));
  HIP_TRY(hipStreamSynchronize(h->stream));
  HIP_TRY(hipFuncSetAttribute((const void*)k_cov_chol_w, hipFuncAttributeMaxDynamicSharedMemorySize, (int)h->bandw_lds));
  HIP_TRY(hipFuncSetAttribute((const void*)k_cov_selinv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2));
  HIP_TRY(hipFuncSetAttribute((const void*)k_cov_backsolve, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds3));
#define CA(ptr, n) do { if (!(ptr)) { if (int rc_ = dev_alloc(h, &(ptr), (n))) return rc_; } } while (0)
  CA(h->cov_C, (size_t)NA * NA); CA(h->cov_Cp, (size_t)NA * NA); CA(h->cov_Zd, (size_t)std::max(1u, F) * 36); CA(h->cov_Y, (size_t)std::max(1u, F) * 6 * NA);
  CA(h->cov_G, (size_t)std::max(1u, F) * 36); CA(h->cov_fail, 1);
  if (out->pose_band && d.bw) CA(h->cov_Zb, (size_t)std::max(1u, F) * d.bw * 36);
#undef CA
  // what the call changes and puts back: the frame mask, the Jacobi scaling state, the device LM state, the profile span
  const bool sigma_saved = h->sigma_valid, prof_saved = h->prof_on;
  double lm_saved[LM_N];
  HIP_TRY(hipMemcpy(lm_saved, d.lm, sizeof(lm_saved), hipMemcpyDeviceToHost));
  auto restore = [&]() -> int {
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (F) HIP_TRY(hipMemcpy(h->frame_live_dev, live_saved.data(), F, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d.lm, lm_saved, sizeof(lm_saved), hipMemcpyHostToDevice));
    h->sigma_valid = sigma_saved; h->prof_on = prof_saved;
    if (gauge >= 0) { h->frame_live_host = live_saved; h->prior_stale = h->has_priors; }   // (a pose prior on the gauge frame comes back)
    return 0;
  };
  auto bail = [&](int rc) { const std::string e = g_last_error; restore(); g_last_error = e; return rc; };
  h->prof_on = false;
  if (gauge >= 0) {
    std::vector<uint8_t> live(live_saved); live[gauge] = 0;
    if (hipMemcpy(h->frame_live_dev, live.data(), F, hipMemcpyHostToDevice) != hipSuccess) { g_last_error = "lifcal_ba_covariance: frame mask upload failed"; return bail(LIFCAL_BA_ERR_HIP); }
    h->frame_live_host = live; h->prior_stale = h->has_priors;   // a prior on the gauge frame's pose leaves the term with its columns
  }
  // ---- the undamped reduced system, K1 .. K3 ----
  if (hipEventRecord(h->ev0, h->stream) != hipSuccess) { g_last_error = "hipEventRecord failed"; return bail(LIFCAL_BA_ERR_HIP); }
  if (int rc = launch_sweep(h, std::numeric_limits<double>::infinity())) return bail(rc);
  hipLaunchKernelGGL(k_cov_chol_w, dim3(1), dim3(256), h->bandw_lds, h->stream, d, h->Lpanel, h->cov_C, h->cov_fail);
  hipLaunchKernelGGL(k_cov_backsolve, dim3(1), dim3(256), lds3, h->stream, d, (const double*)h->Lpanel, h->cov_Y);
  const bool want_pose = d.use_poses && (o.want_pose_blocks || out->pose_band);
  if (want_pose) hipLaunchKernelGGL(k_cov_selinv, dim3(1), dim3(256), lds2, h->stream, d, (const double*)h->Lpanel, h->cov_Zd, out->pose_band && d.bw ? h->cov_Zb : nullptr);
  if (hipGetLastError() != hipSuccess) { g_last_error = "lifcal_ba_covariance: kernel launch failed"; return bail(LIFCAL_BA_ERR_HIP); }
  double cost, gmax, bad;
  if (int rc = read_sweep_scalars(h, &cost, &gmax, &bad)) return bail(rc);
  std::vector<double> C((size_t)NA * NA);
  double failv = 0.0;
  if (hipMemcpy(C.data(), h->cov_C, C.size() * 8, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(&failv, h->cov_fail, 8, hipMemcpyDeviceToHost) != hipSuccess) {
    g_last_error = "lifcal_ba_covariance: read-back failed"; return bail(LIFCAL_BA_ERR_HIP);
  }
  if (!std::isfinite(cost)) { g_last_error = "lifcal_ba_covariance: non-finite cost at the stored parameters"; return bail(LIFCAL_BA_ERR_NUMERIC); }
  if (failv != 0.0) {
    g_last_error = "lifcal_ba_covariance: the pose block of frame " + std::to_string((long long)failv - 1) + " is not positive definite after elimination: the data do not pin that frame down";
    return bail(LIFCAL_BA_ERR_NUMERIC);
  }
  // ---- C+ on the live arrow slots (promoted points, free camera slots), Jacobi-scaled ----
  CamConsts cc;
  if (hipMemcpy(&cc, d.camc, sizeof(cc), hipMemcpyDeviceToHost) != hipSuccess) { g_last_error = "lifcal_ba_covariance: read-back failed"; return bail(LIFCAL_BA_ERR_HIP); }
  std::vector<uint32_t> la;   // live arrow rows
  for (uint32_t a = 0; a < NA; ++a) if (a < Q3 || cc.chm[a - Q3] != 0.0) la.push_back(a);
  const uint32_t n = (uint32_t)la.size();
  std::vector<double> sc(n), Cs((size_t)n * n), w, V;
  for (uint32_t i = 0; i < n; ++i) { const double c = C[(size_t)la[i] * NA + la[i]]; sc[i] = c > 0.0 ? 1.0 / std::sqrt(c) : 1.0; }
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < n; ++k) Cs[(size_t)i * n + k] = 0.5 * (C[(size_t)la[i] * NA + la[k]] + C[(size_t)la[k] * NA + la[i]]) * sc[i] * sc[k];
  sym_eig_jacobi(n, Cs, w, V);
  double wmax = 0.0;
  for (double x : w) wmax = std::max(wmax, x);
  std::vector<uint32_t> nulls;
  for (uint32_t i = 0; i < n; ++i) if (!(w[i] > o.null_rcond * wmax)) nulls.push_back(i);
  std::sort(nulls.begin(), nulls.end(), [&](uint32_t x, uint32_t y) { return w[x] < w[y]; });
  std::vector<double> Cp((size_t)NA * NA, 0.0);
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t k = 0; k < n; ++k) {
      double s = 0.0;
      for (uint32_t e = 0; e < n; ++e) if (w[e] > o.null_rcond * wmax) s += V[(size_t)i * n + e] * V[(size_t)k * n + e] / w[e];
      Cp[(size_t)la[i] * NA + la[k]] = s * sc[i] * sc[k];
    }
  // ---- units: residual variance over the rank of H ----
  uint64_t n_free = 0, n_pts = 0;
  for (uint32_t f = 0; f < F; ++f) if (d.use_poses && live_saved[f]) n_free += 6;
  if (d.use_points) for (uint32_t q = 0; q < d.P; ++q) if (h->plan.point_used[q]) ++n_pts;
  n_free += 3 * n_pts;
  uint32_t live_mask = 0;
  for (uint32_t j = 0; j < nc; ++j) if (cc.chm[j] != 0.0) { live_mask |= 1u << j; ++n_free; }
  const uint64_t m = 2 * (uint64_t)h->plan.n_obs_local + d.M_local + prior_rows(h, h->frame_live_host);   // (priors: one row per live slot with a non-zero prior row)
  const double r = (double)n_free - (gauge >= 0 ? 6.0 : 0.0) - (double)nulls.size();
  const double sigma2 = (double)m > r ? 2.0 * cost / ((double)m - r) : std::numeric_limits<double>::quiet_NaN();
  const double mult = o.scale_by_residual_variance ? sigma2 : 1.0;
  // ---- K4 ----
  if (want_pose && o.want_pose_blocks && out->pose) {
    if (hipMemcpyAsync(h->cov_Cp, Cp.data(), Cp.size() * 8, hipMemcpyHostToDevice, h->stream) != hipSuccess) { g_last_error = "lifcal_ba_covariance: upload failed"; return bail(LIFCAL_BA_ERR_HIP); }
    hipLaunchKernelGGL(k_cov_combine, dim3(F), dim3(64), lds4, h->stream, d, (const double*)h->cov_Zd, (const double*)h->cov_Y, (const double*)h->cov_Cp, mult, h->cov_G);
    if (hipGetLastError() != hipSuccess) { g_last_error = "lifcal_ba_covariance: kernel launch failed"; return bail(LIFCAL_BA_ERR_HIP); }
  }
  if (hipEventRecord(h->ev1, h->stream) != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) { g_last_error = "lifcal_ba_covariance: device failure"; return bail(LIFCAL_BA_ERR_HIP); }
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, h->ev0, h->ev1);
  // ---- outputs ----
  std::fill(out->camera, out->camera + 17 * 17, 0.0);
  for (uint32_t i = 0; i < nc; ++i)
    for (uint32_t k = 0; k < nc; ++k) out->camera[i * 17 + k] = mult * Cp[(size_t)(Q3 + i) * NA + Q3 + k];
  uint32_t est = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (la[i] < Q3) continue;
    bool e = true;
    for (uint32_t k : nulls) if (std::fabs(V[(size_t)i * n + k]) > o.estimable_tol) e = false;
    if (e) est |= 1u << (la[i] - Q3);
  }
  if (out->camera_null) {
    std::fill(out->camera_null, out->camera_null + 17 * 17, 0.0);
    for (size_t r2 = 0; r2 < nulls.size() && r2 < 17; ++r2) {
      double nrm = 0.0;   // the null direction in parameter units (unscaled), unit length over the live arrow slots
      for (uint32_t i = 0; i < n; ++i) { const double v = V[(size_t)i * n + nulls[r2]] * sc[i]; nrm += v * v; }
      nrm = nrm > 0.0 ? 1.0 / std::sqrt(nrm) : 0.0;
      for (uint32_t i = 0; i < n; ++i) if (la[i] >= Q3) out->camera_null[r2 * 17 + (la[i] - Q3)] = V[(size_t)i * n + nulls[r2]] * sc[i] * nrm;
    }
  }
  if (out->pose) {
    if (want_pose && o.want_pose_blocks && F) { if (hipMemcpy(out->pose, h->cov_G, (size_t)F * 36 * 8, hipMemcpyDeviceToHost) != hipSuccess) { g_last_error = "lifcal_ba_covariance: read-back failed"; return bail(LIFCAL_BA_ERR_HIP); } }
    else std::fill(out->pose, out->pose + (size_t)F * 36, 0.0);
  }
  if (out->pose_band && d.bw) {
    std::vector<double> zb((size_t)F * d.bw * 36, 0.0);
    if (want_pose && hipMemcpy(zb.data(), h->cov_Zb, zb.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { g_last_error = "lifcal_ba_covariance: read-back failed"; return bail(LIFCAL_BA_ERR_HIP); }
    for (uint32_t f = 0; f < F; ++f)   // blocks past the last frame and blocks of frames that are not columns: zero
      for (uint32_t dd = 1; dd <= d.bw; ++dd) {
        const bool ok = f + dd < F && d.use_poses && live_saved[f] && live_saved[f + dd] && (int32_t)f != gauge && (int32_t)(f + dd) != gauge;
        for (uint32_t e = 0; e < 36; ++e) out->pose_band[((size_t)f * d.bw + dd - 1) * 36 + e] = ok ? mult * zb[((size_t)f * d.bw + dd - 1) * 36 + e] : 0.0;
      }
  }
  out->estimable_mask = est; out->null_rank = (uint32_t)nulls.size(); out->gauge_frame_used = gauge; out->live_mask = live_mask;
  out->sigma2 = sigma2; out->cost = cost; out->seconds = ms * 1e-3;
  return restore();
}
