// sym_eig.hpp — symmetric eigen-decomposition of a small matrix on the host.  A header of its own so that host-only code
// (align.hpp behind verify_host_check.cpp) can share it without the kernels of covariance.hpp, which includes it.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

// symmetric eigen-decomposition of a small n x n matrix (cyclic Jacobi, fixed sweep order: deterministic): A row-major, destroyed;
// w[i] eigenvalues, V[r * n + i] the unit eigenvector of w[i] in column i
static void sym_eig_jacobi(uint32_t n, std::vector<double>& A, std::vector<double>& w, std::vector<double>& V) {
  V.assign((size_t)n * n, 0.0);
  for (uint32_t i = 0; i < n; ++i) V[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, tot = 0.0;
    for (uint32_t p = 0; p < n; ++p)
      for (uint32_t q = 0; q < n; ++q) { const double v = A[(size_t)p * n + q] * A[(size_t)p * n + q]; tot += v; if (p != q) off += v; }
    if (off <= 1e-34 * tot || off == 0.0) break;
    for (uint32_t p = 0; p + 1 < n; ++p)
      for (uint32_t q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double app = A[(size_t)p * n + p], aqq = A[(size_t)q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
        for (uint32_t k = 0; k < n; ++k) {   // A <- A J (columns p, q)
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * akp - sn * akq; A[(size_t)k * n + q] = sn * akp + c * akq;
        }
        for (uint32_t k = 0; k < n; ++k) {   // A <- J^T A (rows p, q)
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * apk - sn * aqk; A[(size_t)q * n + k] = sn * apk + c * aqk;
        }
        A[(size_t)p * n + q] = 0.0; A[(size_t)q * n + p] = 0.0;
        for (uint32_t k = 0; k < n; ++k) {
          const double vkp = V[(size_t)k * n + p], vkq = V[(size_t)k * n + q];
          V[(size_t)k * n + p] = c * vkp - sn * vkq; V[(size_t)k * n + q] = sn * vkp + c * vkq;
        }
      }
  }
  w.resize(n);
  for (uint32_t i = 0; i < n; ++i) w[i] = A[(size_t)i * n + i];
}
