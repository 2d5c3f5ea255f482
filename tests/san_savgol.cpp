// The host side of Filters.savgol_filter (csrc/savgol_plan.hpp) in a stand-alone program for ASan / UBSan: the argument checks, the
// weights against the moment conditions that define them and against a direct solve of the normal equations, the edge table E against
// the direct fit, savgol_ext against a brute-force extension for every mode and n = 1 .. 12, the tile arithmetic, and the definition
// run over small rows in every mode.  Built and run by tests/test_savgol_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "savgol_plan.hpp"

using namespace nxsig;

static int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__);     \
      std::printf(__VA_ARGS__);                            \
      std::printf("\n");                                   \
      ++failures;                                          \
    }                                                      \
  } while (0)

// the weights of the fit at window position pos by the textbook route: normal equations of the monomials over the centred points
// t_j = j - (W - 1) / 2, solved by Gaussian elimination with pivoting in long double, the derivative taken at t0 = pos - (W - 1) / 2
// (sound for the small windows and low orders it is used on)
static std::vector<double> direct_weights(int W, int p, int deriv, double delta, double pos) {
  const int m = p + 1;
  std::vector<double> out(W, 0.0);
  if (deriv > p) return out;
  std::vector<long double> G((size_t)m * m, 0.0L), rhs(m, 0.0L), t(W);
  const long double centre = (W - 1) / 2.0L, t0 = (long double)pos - centre;
  for (int j = 0; j < W; ++j) t[j] = (long double)j - centre;
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < m; ++c)
      for (int j = 0; j < W; ++j) G[(size_t)r * m + c] += std::pow(t[j], (long double)(r + c));
  for (int q = deriv; q < m; ++q) {   // d^deriv/dt^deriv of t^q at t0
    long double f = 1.0L;
    for (int a = 0; a < deriv; ++a) f *= (long double)(q - a);
    rhs[q] = f * std::pow(t0, (long double)(q - deriv)) / std::pow((long double)delta, (long double)deriv);
  }
  for (int col = 0; col < m; ++col) {
    int piv = col;
    for (int r = col + 1; r < m; ++r)
      if (std::fabs(G[(size_t)r * m + col]) > std::fabs(G[(size_t)piv * m + col])) piv = r;
    for (int c = 0; c < m; ++c) std::swap(G[(size_t)col * m + c], G[(size_t)piv * m + c]);
    std::swap(rhs[col], rhs[piv]);
    for (int r = 0; r < m; ++r) {
      if (r == col) continue;
      const long double f = G[(size_t)r * m + col] / G[(size_t)col * m + col];
      for (int c = 0; c < m; ++c) G[(size_t)r * m + c] -= f * G[(size_t)col * m + c];
      rhs[r] -= f * rhs[col];
    }
  }
  for (int j = 0; j < W; ++j) {
    long double s = 0.0L;
    for (int r = 0; r < m; ++r) s += rhs[r] / G[(size_t)r * m + r] * std::pow(t[j], (long double)r);
    out[j] = (double)s;
  }
  return out;
}

static double max_abs(const std::vector<double>& v) {
  double m = 0.0;
  for (double a : v) m = std::fmax(m, std::fabs(a));
  return m;
}

static void test_checks() {
  bool u = false;
  CHECK(savgol_check_design(5, 2, 0, 1.0, &u) == nullptr && !u, "valid design refused");
  CHECK(std::strcmp(savgol_check_design(5, 5, 0, 1.0, &u), "polyorder must be less than window_length.") == 0 && !u, "polyorder message");
  CHECK(savgol_check_design(0, 0, 0, 1.0, &u) && savgol_check_design(5, -1, 0, 1.0, &u) && savgol_check_design(5, 2, -1, 1.0, &u), "ranges");
  CHECK(savgol_check_design(5, 2, 0, 0.0, &u) && savgol_check_design(5, 2, 0, NAN, &u) && savgol_check_design(5, 2, 0, INFINITY, &u), "delta");
  CHECK(savgol_check_design(1027, 2, 0, 1.0, &u) && u, "window above 1025 is unsupported");
  CHECK(savgol_check_design(1025, 16, 0, 1.0, &u) && u, "order above 15 is unsupported");
  CHECK(savgol_check_design(1025, 15, 20, -0.5, &u) == nullptr, "the limits themselves are built");
  CHECK(savgol_check_rows(5, kSgInterp, 0.0, 5, 1, 5) == nullptr && savgol_check_rows(5, kSgInterp, 0.0, 4, 1, 4) != nullptr, "interp needs W <= n");
  CHECK(savgol_check_rows(5, kSgMirror, 0.0, 1, 1, 1) == nullptr, "the other modes take n = 1");
  CHECK(savgol_check_rows(5, 5, 0.0, 8, 1, 8) && savgol_check_rows(5, -1, 0.0, 8, 1, 8), "mode range");
  CHECK(savgol_check_rows(5, kSgConstant, NAN, 8, 1, 8) && savgol_check_rows(5, 0, 0.0, 0, 1, 0) && savgol_check_rows(5, 0, 0.0, 8, 0, 8) &&
            savgol_check_rows(5, 0, 0.0, 8, 2, 7), "rows");
}

static void test_weights() {
  const int cases[][3] = {{1, 0, 0}, {3, 1, 0}, {4, 1, 0}, {5, 2, 0}, {5, 4, 3}, {6, 3, 1}, {16, 15, 0}, {31, 3, 1}, {101, 4, 2},
                          {255, 5, 2}, {512, 7, 3}, {1025, 9, 4}, {1025, 15, 4}, {7, 2, 5}};
  for (const auto& c : cases) {
    const int W = c[0], p = c[1], d = c[2];
    const double delta = 0.5;
    std::vector<double> k(W), conv(W);
    savgol_coeffs(W, p, d, delta, -1.0, kSgDot, k.data());
    savgol_coeffs(W, p, d, delta, -1.0, kSgConv, conv.data());
    for (int j = 0; j < W; ++j) {
      CHECK(k[j] == ((d & 1) ? -k[W - 1 - j] : k[W - 1 - j]), "W=%d p=%d d=%d: weight %d is not the mirror of its partner", W, p, d, j);
      CHECK(conv[j] == k[W - 1 - j], "W=%d: conv is not dot reversed", W);
    }
    if ((W & 1) && (d & 1)) CHECK(k[W / 2] == 0.0 && !std::signbit(k[W / 2]), "W=%d d=%d: centre weight %g", W, d, k[W / 2]);
    if (d > p) {
      CHECK(max_abs(k) == 0.0, "deriv > polyorder must give zeros");
      continue;
    }
    // the moment conditions: sum_j k[j] t_j^m = d! / delta^d at m = d, zero at every other m <= p (t about the centre, scaled to [-1, 1])
    const long double half = W > 1 ? (W - 1) / 2.0L : 1.0L;
    long double fact = 1.0L;
    for (int q = 2; q <= d; ++q) fact *= q;
    for (int m = 0; m <= p; ++m) {
      long double s = 0.0L, mag = 0.0L;
      for (int j = 0; j < W; ++j) {
        const long double power = std::pow(((long double)j - half) / half, (long double)m);
        s += (long double)k[j] * power;
        mag += std::fabs(power);   // a weight is held to its error against max |k|, not against itself
      }
      const long double want = m == d ? fact / std::pow((long double)delta * half, (long double)d) : 0.0L;
      CHECK(std::fabs(s - want) <= 1e-13L * (mag * (long double)max_abs(k) + std::fabs(want)), "W=%d p=%d d=%d: moment %d is %Lg, want %Lg", W, p, d, m, s, want);
    }
    if (W <= 31 && p <= 5) {
      for (double pos : {-1.0, 0.0, 1.0, (double)(W - 1)}) {
        if (pos >= W) continue;
        std::vector<double> got(W);
        savgol_coeffs(W, p, d, delta, pos, kSgDot, got.data());
        const std::vector<double> want = direct_weights(W, p, d, delta, pos < 0 ? savgol_default_pos(W) : pos);
        const double scale = max_abs(want);
        for (int j = 0; j < W; ++j)
          CHECK(std::fabs(got[j] - want[j]) <= 1e-9 * scale, "W=%d p=%d d=%d pos=%g: weight %d is %g, the direct solve gives %g", W, p, d, pos, j, got[j], want[j]);
      }
    }
  }
}

static void test_edge_table() {
  const int cases[][3] = {{3, 1, 0}, {4, 1, 0}, {5, 2, 1}, {6, 3, 2}, {11, 3, 0}, {31, 3, 1}, {32, 5, 2}};
  for (const auto& c : cases) {
    const int W = c[0], p = c[1], d = c[2], h = W / 2;
    const std::vector<double> Et = savgol_edge_table(W, p, d, 0.5);
    CHECK((int)Et.size() == h * W, "edge table size");
    for (int i = 0; i < h; ++i) {
      const std::vector<double> want = direct_weights(W, p, d, 0.5, (double)i);
      const double scale = max_abs(want);
      for (int j = 0; j < W; ++j)
        CHECK(std::fabs(Et[(size_t)j * h + i] - want[j]) <= 1e-9 * scale, "W=%d p=%d d=%d: E[%d][%d] is %g, the direct fit gives %g", W, p, d, i, j,
              Et[(size_t)j * h + i], want[j]);
    }
  }
  CHECK(savgol_edge_table(1, 0, 0, 1.0).empty(), "a window of one sample has no edge");
  // a polynomial of degree <= p comes back exactly (to rounding) at both ends, derivative and sign included
  const int W = 9, p = 3, d = 1, n = 20;
  std::vector<double> x(n), y(n), k(W);
  for (int i = 0; i < n; ++i) x[i] = 1.0 + 0.5 * i - 0.25 * i * i + 0.01 * i * i * i;
  savgol_coeffs(W, p, d, 1.0, -1.0, kSgDot, k.data());
  const std::vector<double> Et = savgol_edge_table(W, p, d, 1.0);
  savgol_reference_row<double>(x.data(), n, k.data(), W, kSgInterp, 0.0, Et.data(), d, y.data());
  for (int i = 0; i < n; ++i) {
    const double want = 0.5 - 0.5 * i + 0.03 * i * i;
    CHECK(std::fabs(y[i] - want) <= 1e-10 * 12.0, "interp: derivative of a cubic at %d is %g, want %g", i, y[i], want);
  }
}

// the extended row built sample by sample the slow way: position i of ... | row | ... for i in [-reach, n + reach)
static std::vector<int64_t> brute_extension(int n, int mode, int reach) {
  std::vector<int64_t> idx(n + 2 * reach);
  for (int i = -reach; i < n + reach; ++i) {
    int64_t s;
    if (i >= 0 && i < n) s = i;
    else if (mode == kSgNearest) s = i < 0 ? 0 : n - 1;
    else if (mode == kSgWrap) { s = i; while (s < 0) s += n; while (s >= n) s -= n; }
    else if (mode == kSgMirror) {
      // a walk that bounces between 0 and n - 1 without repeating the edge sample; the mirror image is even about 0, so |i| steps
      // from sample 0 land on the sample of position i
      int64_t at = 0;
      int dir = 1;
      if (n == 1) s = 0;
      else {
        const int steps = i < 0 ? -i : i;
        for (int q = 0; q < steps; ++q) {
          if (at + dir > n - 1 || at + dir < 0) dir = -dir;
          at += dir;
        }
        s = at;
      }
    } else s = -1;
    idx[i + reach] = s;
  }
  return idx;
}

static void test_ext() {
  const int reach = 40;
  for (int mode = 0; mode < kSgModes; ++mode)
    for (int n = 1; n <= 12; ++n) {
      const std::vector<int64_t> want = brute_extension(n, mode, reach);
      for (int i = -reach; i < n + reach; ++i)
        CHECK(savgol_ext(i, n, mode) == want[i + reach], "mode %d n=%d: ext(%d) = %lld, want %lld", mode, n, i, (long long)savgol_ext(i, n, mode),
              (long long)want[i + reach]);
    }
  CHECK(savgol_ext(-1, INT64_C(1) << 40, kSgMirror) == 1 && savgol_ext((INT64_C(1) << 40), INT64_C(1) << 40, kSgWrap) == 0, "large rows");
}

static void test_tiles_and_rows() {
  CHECK(savgol_left(5) == 2 && savgol_left(4) == 1 && savgol_left(1) == 0 && savgol_left(2) == 0 && savgol_left(1025) == 512, "samples in front");
  CHECK(savgol_tiles(1) == 1 && savgol_tiles(kSavgolTile) == 1 && savgol_tiles(kSavgolTile + 1) == 2, "tiles of a row");
  CHECK(savgol_tile_span(1025) == kSavgolTile + 1024, "samples of a tile");
  CHECK(kSavgolTile % kSavgolPer == 0 && kSavgolPer % 2 == 0, "tile geometry");
  // the definition over every mode and a few lengths, shorter than half a window included: every read stays inside the row
  for (int mode = 0; mode < kSgModes; ++mode)
    for (int W : {1, 2, 3, 4, 7, 12})
      for (int n : {1, 2, 3, 5, 12, 13}) {
        if (mode == kSgInterp && W > n) continue;
        const int p = W > 2 ? 2 : W - 1, d = 1;
        std::vector<float> x(n), y(n);
        for (int i = 0; i < n; ++i) x[i] = 0.5f * i - 1.0f;
        std::vector<double> k(W);
        savgol_coeffs(W, p, d, 1.0, -1.0, kSgDot, k.data());
        const std::vector<double> Et = savgol_edge_table(W, p, d, 1.0);
        savgol_reference_row<float>(x.data(), n, k.data(), W, mode, 0.25, Et.data(), d, y.data());
        for (int i = 0; i < n; ++i) CHECK(std::isfinite(y[i]), "mode %d W=%d n=%d: output %d is not finite", mode, W, n, i);
        if (mode == kSgInterp && p >= 1)
          for (int i = 0; i < n; ++i) CHECK(std::fabs(y[i] - 0.5f) <= 1e-5f, "interp: slope of a line at %d is %g", i, y[i]);
      }
}

int main() {
  test_checks();
  test_weights();
  test_edge_table();
  test_ext();
  test_tiles_and_rows();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitized savgol host side ok\n");
  return 0;
}
