// The host side of Transforms.dct / idct (csrc/dct_plan.hpp) in a stand-alone program for ASan / UBSan: the argument checks over a sweep
// with the rejected ones, the reduced cosine against the plain one, the tables of both tiers (exact zeros, symmetry, the norm), the tier
// choice, and the direct kernel's tile, LDS and store arithmetic walked thread by thread over heap buffers of exactly the size the C
// entry point is promised — a load or a store outside them is the sanitizer's to report — with the result held to the definition in
// double.  The permutations of the fft tier are walked the same way.  Built and run by tests/test_dct_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "dct_plan.hpp"

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

static const int64_t kSizes[] = {1, 2, 3, 8, 13, 80, 128, 255, 256, 257, 400, 1000, 1024, 4099};

static void test_check() {
  bool u = false;
  CHECK(dct_check(24, 2, 24, 32, 2, 1, 13, &u) == nullptr && !u, "the valid call");
  CHECK(dct_check(24, 0, 24, 32, 3, 0, 32, &u) == nullptr, "batch = 0 is valid");
  CHECK(dct_check(0, 2, 24, 32, 2, 1, 13, &u) && !u, "length = 0");
  CHECK(dct_check(24, 2, 24, 0, 2, 1, 13, &u) && !u, "n = 0");
  CHECK(dct_check(24, -1, 24, 32, 2, 1, 13, &u) && !u, "batch = -1");
  CHECK(dct_check(24, 2, 23, 32, 2, 1, 13, &u) && !u, "batch_stride < length");
  CHECK(dct_check(24, 2, 24, 32, 1, 1, 13, &u) && u, "type 1 is unsupported");
  CHECK(dct_check(24, 2, 24, 32, 4, 1, 13, &u) && u, "type 4 is unsupported");
  for (int32_t t : {-1, 0, 5, 6, 1 << 30}) CHECK(dct_check(24, 2, 24, 32, t, 1, 13, &u) && !u, "type %d", t);
  for (int32_t m : {-1, 3, 99}) CHECK(dct_check(24, 2, 24, 32, 2, m, 13, &u) && !u, "norm %d", m);
  for (int64_t k : {(int64_t)-1, (int64_t)0, (int64_t)33}) CHECK(dct_check(24, 2, 24, 32, 2, 1, k, &u) && !u, "keep %lld", (long long)k);
  CHECK(dct_check(24, 2, 24, (int64_t)1 << 31, 2, 1, 13, &u) && u, "n = 2^31");
  CHECK(dct_check((int64_t)1 << 59, 16, (int64_t)1 << 59, 32, 2, 1, 13, &u) && u, "rows too large");
  CHECK(dct_check(24, (int64_t)1 << 30, 24, ((int64_t)1 << 31) - 1, 2, 1, 13, &u) && u, "result too large");
  for (int64_t n : kSizes) {
    CHECK(dct_tier(n, false) == (n <= 256 ? kDctDirect : kDctFft), "tier of %lld", (long long)n);
    CHECK(dct_tier(n, true) == kDctFft, "tier of %lld, direct off", (long long)n);
  }
}

static void test_cos() {
  for (int64_t n : kSizes) {
    const int64_t top = n <= 256 ? (2 * n - 1) * (n - 1) : 4 * n + 7;
    for (int64_t m = 0; m <= top; m += (n <= 256 ? 1 : 3)) {
      const double got = dct_cos(m, n), want = std::cos(M_PI * (double)(m % (4 * n)) / (2.0 * (double)n));
      // the plain argument is below 2 pi and carries three roundings of 1.1e-16 relative: 2.1e-15 absolute, plus the two cos results' own
      CHECK(std::fabs(got - want) <= 2.5e-15, "cos(pi %lld / (2 %lld)) = %.17g, plain %.17g", (long long)m, (long long)n, got, want);
      if (m % (2 * n) == n) CHECK(got == 0.0, "an odd multiple of pi / 2 is an exact zero (m %lld, n %lld)", (long long)m, (long long)n);
    }
  }
}

static double scale_out(int64_t n, int32_t norm, int64_t k) {
  if (norm == kDctOrtho) return k == 0 ? std::sqrt(1.0 / (4.0 * n)) : std::sqrt(1.0 / (2.0 * n));
  return norm == kDctForward ? 1.0 / (2.0 * n) : 1.0;
}

// the definition of include/nxsig.h in double, plain cos of the plain argument
static std::vector<double> define(const std::vector<double>& x, int32_t type, int32_t norm) {
  const int64_t n = (int64_t)x.size();
  std::vector<double> y(n);
  for (int64_t k = 0; k < n; ++k) {
    double acc = 0.0;
    if (type == 2) {
      for (int64_t j = 0; j < n; ++j) acc += x[j] * std::cos(M_PI * (double)k * (double)(2 * j + 1) / (2.0 * n));
      y[k] = 2.0 * acc * scale_out(n, norm, k);
    } else {
      for (int64_t j = 1; j < n; ++j) acc += x[j] * std::cos(M_PI * (double)(2 * k + 1) * (double)j / (2.0 * n));
      if (norm == kDctOrtho) y[k] = x[0] / std::sqrt((double)n) + std::sqrt(2.0 / n) * acc;
      else y[k] = (x[0] + 2.0 * acc) * (norm == kDctForward ? 1.0 / (2.0 * n) : 1.0);
    }
  }
  return y;
}

static void test_tables() {
  for (int64_t n : kSizes) {
    for (int32_t type : {2, 3})
      for (int32_t norm : {0, 1, 2}) {
        const std::vector<float> tw = dct_fft_table(n, type, norm);
        CHECK((int64_t)tw.size() == 2 * n, "fft table size");
        CHECK(tw[1] == 0.0f, "sin(0) is an exact zero");
        if (n > kDctDirectMax) continue;
        for (int64_t keep : {(int64_t)1, n / 2 > 0 ? n / 2 : 1, n}) {
          const std::vector<float> t = dct_direct_table(n, keep, type, norm);
          CHECK((int64_t)t.size() == n * keep, "direct table size");
          const std::vector<float> full = dct_direct_table(n, n, type, norm);
          for (int64_t j = 0; j < n; ++j)
            for (int64_t k = 0; k < keep; ++k) {
              CHECK(t[j * keep + k] == full[j * n + k], "a table of keep coefficients is the leading part of the full one");
              if (type == 2) {
                if ((k * (2 * j + 1)) % (2 * n) == n) CHECK(t[j * keep + k] == 0.0f, "exact zero at n %lld k %lld j %lld", (long long)n, (long long)k, (long long)j);
                const float mirror = t[(n - 1 - j) * keep + k];
                CHECK(mirror == ((k & 1) ? -t[j * keep + k] : t[j * keep + k]), "symmetry at n %lld k %lld j %lld", (long long)n, (long long)k, (long long)j);
              }
            }
        }
        // type 2: the k = 0 column sums to the gain the centred row's mean returns with; every other column to zero
        if (type == 2) {
          const std::vector<float> full = dct_direct_table(n, n, type, norm);
          for (int64_t k = 0; k < n; ++k) {
            double sum = 0.0;
            for (int64_t j = 0; j < n; ++j) sum += full[j * n + k];
            const double want = k == 0 ? (double)dct_dc_gain(n, norm) : 0.0;
            CHECK(std::fabs(sum - want) <= 1e-5 * (double)dct_dc_gain(n, norm) + 1e-12, "column %lld of n %lld sums to %.9g", (long long)k, (long long)n, sum);
          }
        }
      }
  }
}

// k_dct_direct thread by thread: the same index arithmetic over exactly sized buffers
static void direct_walk(int64_t length, int64_t stride, int64_t batch, int64_t n, int64_t keep, int32_t type, int32_t norm) {
  const int64_t n_used = dct_used(length, n);
  std::vector<float> x((size_t)((batch - 1) * stride + length));
  for (size_t i = 0; i < x.size(); ++i) x[i] = (float)((double)((i * 2654435761u) % 2048) / 1024.0 - 1.0);
  const std::vector<float> table = dct_direct_table(n, keep, type, norm);
  std::vector<float> out((size_t)(batch * keep), -77.0f);
  const DctGeom g = dct_geom(n, keep, batch);
  CHECK(g.pitch >= n + 1 && g.pitch % 4 == 0 && ((g.pitch / 4) & 1) == 1, "pitch %d of n %lld", g.pitch, (long long)n);
  CHECK(g.groups >= 1 && (int64_t)g.groups * keep <= kDctThreads, "groups %d at keep %lld", g.groups, (long long)keep);
  CHECK((int64_t)g.tile_rows * g.pitch <= kDctLdsFloats, "a tile of %d rows at pitch %d overflows the LDS image", g.tile_rows, g.pitch);
  const bool centre = type == 2;
  const float dc = dct_dc_gain(n, norm);
  for (int64_t tile = 0; tile < g.tiles; ++tile) {
    std::vector<float> s((size_t)g.tile_rows * g.pitch);   // exactly what the tile may touch (<= kDctLdsFloats)
    const int64_t row0 = tile * g.tile_rows, left = batch - row0;
    const int here = left < g.tile_rows ? (int)left : g.tile_rows;
    CHECK(here >= 1, "an empty tile");
    const float* base = x.data() + row0 * stride;
    const bool wide = stride == n && n_used == n && (n & 3) == 0;
    if (wide) {
      const int Q = (int)n >> 2, total = g.tile_rows * Q;
      for (int i = 0; i < total; ++i) {
        const int r = i / Q, c4 = i - r * Q;
        for (int e = 0; e < 4; ++e) s.at((size_t)r * g.pitch + 4 * c4 + e) = r < here ? base[(size_t)4 * i + e] : 0.0f;
      }
    } else {
      const int total = g.tile_rows * (int)n;
      for (int i = 0; i < total; ++i) {
        const int r = i / (int)n, j = i - r * (int)n;
        s.at((size_t)r * g.pitch + j) = (r < here && j < n_used) ? base[(size_t)r * stride + j] : 0.0f;
      }
    }
    if (centre)
      for (int r = 0; r < here; ++r) {
        // four lanes per row, each over its quarter (dct_quarter), the partial sums added as (p0 + p1) + (p2 + p3)
        const bool quads = (n & 3) == 0;
        const int units = quads ? (int)n >> 2 : (int)n, per = quads ? 4 : 1;
        float p[4];
        int covered = 0;
        for (int q = 0; q < 4; ++q) {
          p[q] = 0.0f;
          for (int u = dct_quarter(q, units); u < dct_quarter(q + 1, units); ++u, ++covered)
            for (int e = 0; e < per; ++e) p[q] += s.at((size_t)r * g.pitch + per * u + e);
        }
        CHECK(covered == units && dct_quarter(0, units) == 0 && dct_quarter(4, units) == units, "the quarters of %d units", units);
        const float c = ((p[0] + p[1]) + (p[2] + p[3])) / (float)n;
        for (int j = 0; j < n; ++j) s.at((size_t)r * g.pitch + j) -= c;
        s.at((size_t)r * g.pitch + n) = c;
      }
    for (int tid = 0; tid < g.groups * (int)keep; ++tid) {
      const int gq = tid / (int)keep, k = tid - gq * (int)keep;
      for (int rr = 0; rr < kDctRR; ++rr) {
        const int r = gq + g.groups * rr;
        CHECK(r < g.tile_rows, "row %d beyond the tile", r);
        float acc = 0.0f;
        for (int j = 0; j < n; ++j) acc = std::fmaf(s.at((size_t)r * g.pitch + j), table.at((size_t)j * keep + k), acc);
        if (r >= here) continue;
        if (centre && k == 0) acc = std::fmaf(s.at((size_t)r * g.pitch + n), dc, acc);
        float& o = out.at((size_t)(row0 + r) * keep + k);
        CHECK(o == -77.0f, "output written twice");
        o = acc;
      }
    }
  }
  for (int64_t r = 0; r < batch; ++r) {
    std::vector<double> xr(n, 0.0);
    for (int64_t j = 0; j < n_used; ++j) xr[j] = x[r * stride + j];
    const std::vector<double> ref = define(xr, type, norm);
    double top = 0.0;
    for (double v : ref) top = std::fmax(top, std::fabs(v));
    for (int64_t k = 0; k < keep; ++k) {
      const float got = out[r * keep + k];
      CHECK(got != -77.0f, "output never written: row %lld k %lld", (long long)r, (long long)k);
      CHECK(std::fabs((double)got - ref[k]) <= 1e-5 * top + 1e-30, "n %lld type %d norm %d row %lld k %lld: %.9g, definition %.9g", (long long)n, type, norm,
            (long long)r, (long long)k, (double)got, ref[k]);
    }
  }
}

static void test_direct() {
  for (int64_t n : kSizes) {
    if (n > kDctDirectMax) continue;
    for (int32_t type : {2, 3})
      for (int32_t norm : {0, 1, 2}) {
        direct_walk(n, n, 3, n, n, type, norm);
        direct_walk(n, n + 5, 3, n, n > 1 ? n - 1 : 1, type, norm);
      }
    direct_walk(n, n, 300, n, n < 13 ? n : 13, 2, 1);   // several tiles, the last one ragged
  }
  direct_walk(7, 7, 5, 16, 16, 2, 0);      // padding
  direct_walk(100, 100, 5, 256, 20, 3, 1);
  direct_walk(8, 9, 5, 5, 5, 2, 1);        // truncation
  direct_walk(300, 300, 5, 128, 13, 2, 2);
  direct_walk(1, 1, 70000, 1, 1, 2, 0);    // the widest tile: 2048 rows
}

// the fft tier's permutations: each a bijection of [0, n), inverse to each other; Makhoul's identity in double through a naive DFT
static void test_fft_form() {
  for (int64_t n : kSizes) {
    std::vector<int> seen(n, 0);
    for (int64_t i = 0; i < n; ++i) {
      const int64_t src = dct_perm(i, n);
      CHECK(src >= 0 && src < n, "perm(%lld, %lld) = %lld", (long long)i, (long long)n, (long long)src);
      if (src >= 0 && src < n) {
        ++seen[src];
        CHECK(dct_unperm(src, n) == i, "unperm(perm(%lld)) of n %lld", (long long)i, (long long)n);
      }
    }
    for (int64_t i = 0; i < n; ++i) CHECK(seen[i] == 1, "perm of n %lld is no bijection at %lld", (long long)n, (long long)i);
  }
  for (int64_t n : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)8, (int64_t)13, (int64_t)80}) {
    std::vector<double> x(n);
    for (int64_t j = 0; j < n; ++j) x[j] = 0.25 * (double)((j * 37) % 11) - 1.0;
    for (int32_t norm : {0, 1, 2}) {
      // type 2: y[k] = tw[k].x Re V[k] + tw[k].y Im V[k], V = DFT(v), v[i] = x[perm(i)]
      const std::vector<float> tw = dct_fft_table(n, 2, norm);
      const std::vector<double> ref = define(x, 2, norm), ref3 = define(x, 3, norm);
      double top = 0.0, top3 = 0.0;
      for (int64_t k = 0; k < n; ++k) { top = std::fmax(top, std::fabs(ref[k])); top3 = std::fmax(top3, std::fabs(ref3[k])); }
      for (int64_t k = 0; k < n; ++k) {
        double re = 0.0, im = 0.0;
        for (int64_t i = 0; i < n; ++i) {
          const double a = -2.0 * M_PI * (double)((k * i) % n) / (double)n;
          re += x[dct_perm(i, n)] * std::cos(a);
          im += x[dct_perm(i, n)] * std::sin(a);
        }
        CHECK(std::fabs(tw[2 * k] * re + tw[2 * k + 1] * im - ref[k]) <= 1e-6 * top, "Makhoul type 2 at n %lld k %lld norm %d", (long long)n, (long long)k, norm);
      }
      // type 3: W[0] = tw[0].x x[0], W[k] = tw[k] (x[k] - i x[n - k]); y[m] = Re IDFT(W)[unperm(m)] with its 1 / n
      const std::vector<float> t3 = dct_fft_table(n, 3, norm);
      std::vector<double> wr(n), wi(n);
      wr[0] = t3[0] * x[0]; wi[0] = 0.0;
      for (int64_t k = 1; k < n; ++k) {
        const double c = t3[2 * k], s = t3[2 * k + 1], p = x[k], q = x[n - k];
        wr[k] = c * p + s * q;
        wi[k] = s * p - c * q;
      }
      for (int64_t m = 0; m < n; ++m) {
        const int64_t i = dct_unperm(m, n);
        double re = 0.0;
        for (int64_t k = 0; k < n; ++k) {
          const double a = 2.0 * M_PI * (double)((k * i) % n) / (double)n;
          re += wr[k] * std::cos(a) - wi[k] * std::sin(a);
        }
        CHECK(std::fabs(re / (double)n - ref3[m]) <= 1e-6 * top3, "Makhoul type 3 at n %lld m %lld norm %d: %.9g, definition %.9g", (long long)n, (long long)m, norm,
              re / (double)n, ref3[m]);
      }
    }
  }
}

int main() {
  test_check();
  test_cos();
  test_tables();
  test_direct();
  test_fft_form();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("sanitized dct host side ok\n");
  return 0;
}
