// Filters.savgol_filter / savgol_coeffs: everything of it that is plain C++ — the argument checks, the
// least-squares weights and the edge table of mode "interp", the index rule of the five extensions, and the tile arithmetic.  The kernels
// of kernels_savgol.hip call savgol_ext and the tile constants as they stand here, and the C entry points call the rest, so the
// stand-alone program tests/san_savgol.cpp runs the same code on the host under ASan / UBSan.  No HIP types.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NXSIG_SG_HD __host__ __device__ __forceinline__
#else
#define NXSIG_SG_HD inline
#endif

namespace nxsig {

constexpr int kSavgolMaxWindow = 1025;
constexpr int kSavgolMaxOrder = 15;
// savgol.tiles: one workgroup of kSavgolLanes lanes per tile of kSavgolTile consecutive outputs of a row, kSavgolPer outputs per lane
constexpr int kSavgolLanes = 256;
constexpr int kSavgolPer = 8;
constexpr int kSavgolTile = 2048;
static_assert(kSavgolTile == kSavgolLanes * kSavgolPer, "a lane owns kSavgolPer consecutive outputs");

enum SavgolMode : int32_t { kSgMirror = 0, kSgConstant = 1, kSgNearest = 2, kSgWrap = 3, kSgInterp = 4, kSgModes = 5 };
enum SavgolUse : int32_t { kSgConv = 0, kSgDot = 1 };

// samples in front of output i that its window covers: y[i] = sum_j k[j] ext(i - L + j)
NXSIG_SG_HD int savgol_left(int W) { return (W & 1) ? W / 2 : W / 2 - 1; }
inline int64_t savgol_tiles(int64_t n) { return (n + kSavgolTile - 1) / kSavgolTile; }
// samples a tile loads: its outputs and the W - 1 around them
inline int savgol_tile_span(int W) { return kSavgolTile + W - 1; }

// the sample of a row of n that stands at index i of the extended row: its index in [0, n), or -1 where the extension holds a constant
// (cval for "constant", zero for "interp", whose edge outputs are replaced afterwards)
NXSIG_SG_HD int64_t savgol_ext(int64_t i, int64_t n, int mode) {
  if (i >= 0 && i < n) return i;
  switch (mode) {
    case kSgMirror: {
      if (n == 1) return 0;
      const int64_t period = 2 * (n - 1);
      int64_t m = i % period;
      if (m < 0) m += period;
      return m < n ? m : period - m;
    }
    case kSgNearest: return i < 0 ? 0 : n - 1;
    case kSgWrap: {
      int64_t m = i % n;
      return m < 0 ? m + n : m;
    }
    default: return -1;
  }
}

// the argument errors that need neither the tensor nor a context; nullptr when all is well.  *unsupported: the argument is well formed
// but beyond what is built
inline const char* savgol_check_design(int64_t W, int64_t p, int64_t deriv, double delta, bool* unsupported) {
  *unsupported = false;
  if (W < 1) return "window_length must be a positive integer";
  if (p < 0) return "polyorder must be a nonnegative integer";
  if (p >= W) return "polyorder must be less than window_length.";
  if (deriv < 0) return "deriv must be a nonnegative integer";
  if (!std::isfinite(delta) || delta == 0.0) return "delta must be finite and non-zero";
  *unsupported = true;
  if (W > kSavgolMaxWindow) return "window_length must be at most 1025";
  if (p > kSavgolMaxOrder) return "polyorder must be at most 15";
  *unsupported = false;
  return nullptr;
}

inline const char* savgol_check_rows(int64_t W, int32_t mode, double cval, int64_t length, int64_t batch, int64_t batch_stride) {
  if (mode < 0 || mode >= kSgModes) return "mode must be 'mirror', 'constant', 'nearest' 'wrap' or 'interp'.";
  if (!std::isfinite(cval)) return "cval must be finite";
  if (length < 1) return "length must be >= 1";
  if (batch < 1) return "batch must be >= 1";
  if (batch_stride < length) return "batch_stride must be >= length";
  if (mode == kSgInterp && W > length) return "If mode is 'interp', window_length must be less than or equal to the size of x.";
  return nullptr;
}

// ---- the weights.  The degree-p least-squares polynomial through the W samples of a window is expanded in the monic polynomials
// orthogonal over the window's points x_j = (2 j - (W - 1)) / (W - 1) in [-1, 1]: P_k = x P_(k-1) - beta_(k-1) P_(k-2) — the points are
// symmetric, so the recurrence has no alpha term and P_k(-x) = (-1)^k P_k(x) holds to the last bit.  The weight of sample j for the
// deriv-th derivative at window position pos is  sum_k P_k^(deriv)(x0) P_k(x_j) / |P_k|^2  over k = deriv .. p, times (2 / (W - 1))^deriv
// / delta^deriv.  Everything in long double; the result is rounded to double once.
struct SavgolBasis {
  int W = 0, p = 0;
  std::vector<long double> x;      // [W]
  std::vector<long double> P;      // [p + 1][W]
  std::vector<long double> norm;   // [p + 1]
  std::vector<long double> beta;   // [p + 1]: beta[k] = norm[k] / norm[k - 1] (k >= 1)
};

inline SavgolBasis savgol_basis(int W, int p) {
  SavgolBasis b;
  b.W = W; b.p = p;
  b.x.resize(W);
  b.P.assign((size_t)(p + 1) * W, 0.0L);
  b.norm.assign(p + 1, 0.0L);
  b.beta.assign(p + 1, 0.0L);
  for (int j = 0; j < W; ++j) b.x[j] = W > 1 ? (long double)(2 * j - (W - 1)) / (long double)(W - 1) : 0.0L;
  for (int k = 0; k <= p; ++k) {
    long double* Pk = &b.P[(size_t)k * W];
    for (int j = 0; j < W; ++j) {
      if (k == 0) Pk[j] = 1.0L;
      else if (k == 1) Pk[j] = b.x[j];
      else Pk[j] = b.x[j] * Pk[j - W] - b.beta[k - 1] * Pk[j - 2 * W];
    }
    // squares from the outside in: both halves add the same numbers in the same order
    long double s = 0.0L;
    for (int j = 0; j < W / 2; ++j) s += 2.0L * Pk[j] * Pk[j];
    if (W & 1) s += Pk[W / 2] * Pk[W / 2];
    b.norm[k] = s;
    if (k >= 1) b.beta[k] = b.norm[k] / b.norm[k - 1];
  }
  return b;
}

// correlation weights ("dot" order) for the deriv-th derivative at window position pos (0 <= pos <= W - 1, fractional allowed)
inline void savgol_weights_at(const SavgolBasis& b, int deriv, double delta, double pos, double* out) {
  const int W = b.W, p = b.p;
  for (int j = 0; j < W; ++j) out[j] = 0.0;
  if (deriv > p) return;
  const long double x0 = W > 1 ? (2.0L * (long double)pos - (long double)(W - 1)) / (long double)(W - 1) : 0.0L;
  // D[k][m] = P_k^(m)(x0)
  std::vector<long double> D((size_t)(p + 1) * (deriv + 1), 0.0L);
  auto at = [&](int k, int m) -> long double& { return D[(size_t)k * (deriv + 1) + m]; };
  for (int k = 0; k <= p; ++k)
    for (int m = 0; m <= deriv; ++m) {
      if (k == 0) { at(k, m) = m == 0 ? 1.0L : 0.0L; continue; }
      long double v = x0 * at(k - 1, m);
      if (m > 0) v += (long double)m * at(k - 1, m - 1);
      if (k >= 2) v -= b.beta[k - 1] * at(k - 2, m);
      at(k, m) = v;
    }
  long double scale = 1.0L;
  for (int m = 0; m < deriv; ++m) scale *= (W > 1 ? 2.0L / (long double)(W - 1) : 1.0L) / (long double)delta;
  std::vector<long double> g(p + 1, 0.0L);
  for (int k = deriv; k <= p; ++k) g[k] = at(k, deriv) / b.norm[k];
  const bool centred = x0 == 0.0L;
  const int upto = centred ? (W + 1) / 2 : W;
  for (int j = 0; j < upto; ++j) {
    long double s = 0.0L;
    for (int k = p; k >= deriv; --k) s += g[k] * b.P[(size_t)k * W + j];   // highest degree (smallest term) first
    const double w = (double)(s * scale);
    out[j] = w == 0.0 ? 0.0 : w;
  }
  if (centred) {   // the fit at the centre is even (odd) in the samples for an even (odd) derivative: mirror the computed half
    if ((W & 1) && (deriv & 1)) out[W / 2] = 0.0;
    for (int j = 0; j < W / 2; ++j) out[W - 1 - j] = (deriv & 1) ? -out[j] : out[j];
  }
}

// scipy.signal.savgol_coeffs: pos < 0 stands for the default (the centre: W / 2 for an odd window, W / 2 - 0.5 for an even one)
inline double savgol_default_pos(int W) { return (W & 1) ? (double)(W / 2) : (double)(W / 2) - 0.5; }
inline void savgol_coeffs(int W, int p, int deriv, double delta, double pos, int use, double* out) {
  const SavgolBasis b = savgol_basis(W, p);
  savgol_weights_at(b, deriv, delta, pos < 0 ? savgol_default_pos(W) : pos, out);
  if (use == kSgConv)
    for (int j = 0; j < W / 2; ++j) { const double t = out[j]; out[j] = out[W - 1 - j]; out[W - 1 - j] = t; }
}

// the edge table of mode "interp", TRANSPOSED: Et[j * h + i] is the weight of sample j of the first W samples of a row in output i
// (0 <= i < h = W / 2): the deriv-th derivative at position i of the polynomial through those samples.  Output n - 1 - i takes the same
// row over the samples n - 1 - j, times (-1)^deriv
inline std::vector<double> savgol_edge_table(int W, int p, int deriv, double delta) {
  const int h = W / 2;
  std::vector<double> Et((size_t)h * W), row(W);
  if (h == 0) return Et;
  const SavgolBasis b = savgol_basis(W, p);
  for (int i = 0; i < h; ++i) {
    savgol_weights_at(b, deriv, delta, (double)i, row.data());
    for (int j = 0; j < W; ++j) Et[(size_t)j * h + i] = row[j];
  }
  return Et;
}

// ---- the definition on the host, in the summation order of include/nxsig.h (ascending j, one fused multiply-add per weight): what
// tests/san_savgol.cpp holds the index rule and the tables to
template <typename T>
inline void savgol_reference_row(const T* x, int64_t n, const double* k, int W, int mode, double cval, const double* Et, int deriv, T* y) {
  const int L = savgol_left(W), h = W / 2;
  for (int64_t i = 0; i < n; ++i) {
    double acc = 0.0;
    for (int j = 0; j < W; ++j) {
      const int64_t s = savgol_ext(i - L + j, n, mode);
      acc = std::fma(k[j], s < 0 ? (mode == kSgConstant ? cval : 0.0) : (double)x[s], acc);
    }
    y[i] = (T)acc;
  }
  if (mode != kSgInterp) return;
  for (int side = 0; side < 2; ++side)
    for (int i = 0; i < h; ++i) {
      double acc = 0.0;
      for (int j = 0; j < W; ++j) acc = std::fma(Et[(size_t)j * h + i], (double)x[side ? n - 1 - j : j], acc);
      y[side ? n - 1 - i : i] = (T)((side && (deriv & 1)) ? -acc : acc);
    }
}

}  // namespace nxsig
