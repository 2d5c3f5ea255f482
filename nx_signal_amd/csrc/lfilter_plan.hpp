// Filters.lfilter / lfilter_zi / filtfilt: the host side, free of HIP so that a stand-alone program can drive it under a sanitizer
// (tests/san_lfilter.cpp): the argument checks and the normalisation by a[0], the padded order, the reference step, the companion
// matrix and its powers (the helpers of iir_plan.hpp on a dense matrix), scipy's lfilter_zi, the padding of filtfilt, the chunk / tile
// geometry, the tables of the scan and the conditioning guard that decides whether a filter may use them.  A filter (b, a) of order n in
// transposed direct form II is the linear system
//     z[m + 1] = A z[m] + B x[m],   y[m] = b0 x[m] + z[m][0],      A[i][0] = -a[i + 1], A[i][i + 1] = 1      (n states)
// A is a dense companion matrix.  Everything is double.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "iir_plan.hpp"

namespace nxsig {

constexpr int32_t kLfMaxOrder = 16;

// the order a kernel is instantiated for: b and a are filled up with zeros, so a padded state stays an exact zero
inline int32_t lf_padded_order(int32_t n) { return n <= 1 ? 1 : n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : 16; }
// samples per lane and per workgroup tile: functions of the order only (0 outside 0 .. 16); the values sosfilt uses for as many states
inline int32_t lf_chunk(int32_t n) { return n < 0 || n > kLfMaxOrder ? 0 : (n <= 4 ? 32 : 64); }
inline int32_t lf_tile(int32_t n) { return lf_chunk(n) * kIirLanes; }
inline int64_t lf_tiles(int64_t length, int32_t n) { const int64_t T = lf_tile(n); return (length + T - 1) / T; }

// nullptr, or what is wrong with b = f64[nb], a = f64[na] (worded after scipy's lfilter); *unsupported: a valid filter that is not built
inline const char* lf_check_ba(const double* b, int32_t nb, const double* a, int32_t na, bool* unsupported) {
  *unsupported = false;
  if (nb < 1 || na < 1) return "b and a must have at least one coefficient each";
  if (nb > (1 << 20) || na > (1 << 20)) return "b and a are too long";
  for (int32_t k = 0; k < nb; ++k)
    if (!std::isfinite(b[k])) return "b and a must be finite";
  for (int32_t k = 0; k < na; ++k)
    if (!std::isfinite(a[k])) return "b and a must be finite";
  if (a[0] == 0.0) return "a[0] must not be zero";
  if ((nb > na ? nb : na) - 1 > kLfMaxOrder) {
    *unsupported = true;
    return na == 1 ? "order above 16 (an FIR filter: filters.fir runs any number of taps)"
                   : "order above 16 (a recursive filter of this order belongs in second-order sections: sosfilt)";
  }
  return nullptr;
}

// b and a divided by a[0] and filled up with zeros to kLfMaxOrder + 1 coefficients
struct LfCoefs {
  int32_t n;   // order: max(nb, na) - 1
  double b[kLfMaxOrder + 1], a[kLfMaxOrder + 1];
};
inline LfCoefs lf_normalise(const double* b, int32_t nb, const double* a, int32_t na) {
  LfCoefs cf;
  cf.n = (nb > na ? nb : na) - 1;
  for (int k = 0; k <= kLfMaxOrder; ++k) {
    cf.b[k] = k < nb ? b[k] / a[0] : 0.0;
    cf.a[k] = k < na ? a[k] / a[0] : 0.0;
  }
  return cf;
}

// ---- one sample, scipy's recurrence in scipy's order of operations; z holds cf.n states
inline double lf_step(const LfCoefs& cf, double* z, double x) {
  const int n = cf.n;
  if (n == 0) return cf.b[0] * x;
  const double y = z[0] + cf.b[0] * x;
  for (int i = 0; i < n - 1; ++i) z[i] = z[i + 1] + x * cf.b[i + 1] - y * cf.a[i + 1];
  z[n - 1] = x * cf.b[n] - y * cf.a[n];
  return y;
}

// A as a dense row-major n x n matrix: column c is one step from the unit state e_c with x = 0
inline std::vector<double> lf_state_matrix(const LfCoefs& cf) {
  const int n = cf.n;
  std::vector<double> A((size_t)n * n, 0.0), z((size_t)n);
  for (int c = 0; c < n; ++c) {
    for (int r = 0; r < n; ++r) z[r] = r == c ? 1.0 : 0.0;
    lf_step(cf, z.data(), 0.0);
    for (int r = 0; r < n; ++r) A[(size_t)r * n + c] = z[r];
  }
  return A;
}

// scipy.signal.lfilter_zi: (I - A) zi = B with B[i] = b[i + 1] - a[i + 1] b0 (A as above is scipy's companion(a).T), by elimination
// with partial pivoting as LAPACK does it for scipy.  false: the system is singular, a pole at z = 1 (scipy raises LinAlgError)
inline bool lf_zi(const LfCoefs& cf, double* zi) {
  const int n = cf.n;
  if (n == 0) return true;
  std::vector<double> M = lf_state_matrix(cf), r((size_t)n);
  for (int i = 0; i < n; ++i) {
    for (int c = 0; c < n; ++c) M[(size_t)i * n + c] = (i == c ? 1.0 : 0.0) - M[(size_t)i * n + c];
    r[i] = cf.b[i + 1] - cf.a[i + 1] * cf.b[0];
  }
  for (int k = 0; k < n; ++k) {
    int p = k;
    for (int i = k + 1; i < n; ++i)
      if (std::fabs(M[(size_t)i * n + k]) > std::fabs(M[(size_t)p * n + k])) p = i;
    if (M[(size_t)p * n + k] == 0.0) return false;
    if (p != k) {
      for (int c = 0; c < n; ++c) { const double t = M[(size_t)k * n + c]; M[(size_t)k * n + c] = M[(size_t)p * n + c]; M[(size_t)p * n + c] = t; }
      const double t = r[k]; r[k] = r[p]; r[p] = t;
    }
    for (int i = k + 1; i < n; ++i) {
      const double l = M[(size_t)i * n + k] / M[(size_t)k * n + k];
      if (l == 0.0) continue;
      for (int c = k; c < n; ++c) M[(size_t)i * n + c] -= l * M[(size_t)k * n + c];
      r[i] -= l * r[k];
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    double v = r[i];
    for (int c = i + 1; c < n; ++c) v -= M[(size_t)i * n + c] * zi[c];
    zi[i] = v / M[(size_t)i * n + i];
    if (!std::isfinite(zi[i])) return false;
  }
  return true;
}

// ---- filtfilt (method "pad"): padtype 0 none, 1 odd, 2 even, 3 constant; padlen < 0 asks for scipy's default 3 max(na, nb)
inline int32_t lf_default_padlen(int32_t nb, int32_t na) { return 3 * (nb > na ? nb : na); }
// the edge scipy pads with (>= 0), or -1: padtype unknown, -2: padlen >= length
inline int64_t lf_edge(int32_t nb, int32_t na, int32_t padtype, int64_t padlen, int64_t length) {
  if (padtype < 0 || padtype > 3) return -1;
  const int64_t edge = padtype == 0 ? 0 : (padlen < 0 ? lf_default_padlen(nb, na) : padlen);
  return length <= edge ? -2 : edge;
}

// ---- the tables of lfilter.scan and the conditioning guard.
// mc and mt are iir_scan_matrices of A padded to np x np: mc [0 .. 5] A^(C 2^k); mt [0 .. 5] A^(T R 2^k), [6] A^T.
// The guard: the scan adds zero-state responses that were carried through these powers, and a chunk that starts from a state that is
// off by d puts (A^k d)[0] into its k-th output.  A companion matrix with clustered poles is far from normal: its powers grow before
// they decay (entries of 1e5 at A^2 .. A^32 for fifteen poles near radius 0.7, gone again by A^64), the stored powers are then small
// numbers left over by cancellation, and the scan loses what the growth amplifies although no table entry is large.  So the quantity
// takes the growth inside a chunk as well as the tables:
//     G = max |entry| over A^1 .. A^C (C steps of the recurrence from every unit state) and over mc, mt
//     kappa = G x sum_k |a[k]|          (a state of the direct form is a sum of terms a[k] y: up to sum |a[k]| times the output)
// a function of the normalised (b, a) and R alone.  A filter runs on the scan when every entry is finite, kappa <= kLfGuardMax, and the
// table's A^C agrees with those C steps of the recurrence within kLfTableGapMax of G (a table that squaring has spoilt does not).
// The thresholds come from the host emulation of tests/san_lfilter.cpp (figures: profiles/lfilter/accuracy.txt)
constexpr double kLfGuardMax = 1.0e4;
constexpr double kLfTableGapMax = 1.0e-11;
struct LfTables {
  std::vector<double> mc, mt;
  double kappa, growth, table_gap;
  bool scan_ok;
};
inline LfTables lf_tables(const LfCoefs& cf, int64_t R) {
  const int n = cf.n, np = lf_padded_order(n), C = lf_chunk(n);
  const std::vector<double> A = lf_state_matrix(cf);
  LfTables t;
  t.mc = iir_scan_matrices(A, n, np, (uint64_t)C, 0);
  t.mt = iir_scan_matrices(A, n, np, (uint64_t)lf_tile(n) * (uint64_t)R, (uint64_t)lf_tile(n));
  double big = 0.0, a1 = 0.0, gap = 0.0;
  bool finite = true;
  const size_t used = (size_t)kIirLevels * np * np;   // slot 6 of mc is not read
  for (size_t i = 0; i < t.mt.size(); ++i) {
    const double m = t.mt[i], c = i < used ? t.mc[i] : 0.0;
    finite = finite && std::isfinite(m) && std::isfinite(c);
    big = std::fmax(big, std::fmax(std::fabs(m), std::fabs(c)));
  }
  // A^1 .. A^C column by column: C steps without input from every unit state; the last is the table's A^C formed another way
  std::vector<double> z((size_t)(n ? n : 1));
  for (int c = 0; c < n; ++c) {
    for (int r = 0; r < n; ++r) z[r] = r == c ? 1.0 : 0.0;
    for (int k = 0; k < C; ++k) {
      lf_step(cf, z.data(), 0.0);
      for (int r = 0; r < n; ++r) {
        finite = finite && std::isfinite(z[r]);
        big = std::fmax(big, std::fabs(z[r]));
      }
    }
    for (int r = 0; r < n; ++r) gap = std::fmax(gap, std::fabs(z[r] - t.mc[(size_t)r * np + c]));
  }
  for (int k = 0; k <= n; ++k) a1 += std::fabs(cf.a[k]);
  t.growth = finite ? big : INFINITY;
  t.kappa = finite ? big * a1 : INFINITY;
  t.table_gap = finite && big > 0.0 ? gap / big : (finite ? 0.0 : INFINITY);
  t.scan_ok = finite && t.kappa <= kLfGuardMax && t.table_gap <= kLfTableGapMax;
  return t;
}

// nullptr, or what is wrong with the shape arguments of nxsig_lfilter_f32 (after the null, mem and coefficient checks)
inline const char* lf_check_args(int64_t length, int32_t batch, int64_t batch_stride, int32_t zi_rows, bool has_zi, int32_t direction) {
  return iir_check_args(length, batch, batch_stride, zi_rows, has_zi, direction);
}

}  // namespace nxsig
